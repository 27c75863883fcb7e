// The d = 128 backward tail, decided on the host before anything runs: tail_form_from_env (the switches),
// plan_tail (where every slab lies, which launch carries which job, every grid).  Host code only: nothing here
// launches or dereferences a device pointer.  bwd_defer.hip runs the plan.
#include "bwd_defer.hpp"

#include <algorithm>

namespace pca {

// unset = the measured defaults (PCA_WGRAD_RIDE: DESIGN 4.4.4; PCA_D128_MIDFUSE: each layer's winner, 4.4.2)
constexpr bool WGRAD_RIDE_DEFAULT = true, MIDFUSE_DEFAULT_WIDE = true, MIDFUSE_DEFAULT_SMALL = true;

TailForm tail_form_from_env() {
  TailForm f{};
  f.slabs = env_not_zero("PCA_WGRAD_SLABS");
  f.fold = env_not_zero("PCA_WGRAD_FOLD");
  f.post_fuse = env_not_zero("PCA_POST_FUSE");
  f.dz_mask = env_not_zero("PCA_D128_DZ_MASK");
  // 0 = k_mid_bwd as a launch in both layers, 1 = fused in both, "wide" / "small" = fused in that form only
  const char* m = getenv("PCA_D128_MIDFUSE");
  const bool m_unset = m == nullptr || m[0] == 0;
  f.midfuse_wide = m_unset ? MIDFUSE_DEFAULT_WIDE : m[0] == 'w' || (m[0] != 's' && m[0] != '0');
  f.midfuse_small = m_unset ? MIDFUSE_DEFAULT_SMALL : m[0] == 's' || (m[0] != 'w' && m[0] != '0');
  const char* r = getenv("PCA_WGRAD_RIDE");
  const bool ride = (r == nullptr || r[0] == 0) ? WGRAD_RIDE_DEFAULT : r[0] != '0';
  f.ride = ride && f.slabs && f.fold && f.midfuse_small;
  return f;
}

// ---- shapes of the weight-gradient launches (wgrad128.hip launches them) ------------------
// Widens grid.x to the widest rider row, and counts the rows of the layer-1 fc_v job (slab mode only: its partials
// are summed later; as wide as the grid, blocks_per_wg blocks of its rows_per_wg rows to a workgroup)
static int extra_rows(const SlabSumJobs& riders, const SmallWgradArgs* sw, int blocks_per_wg, unsigned& gx,
                      int* sw_rows) {
  for (int i = 0; i < riders.n; ++i) {
    PCA_REQUIRE(slab_sum_job_ok(riders.j[i]), "wgrad128: rider alignment");
    gx = std::max(gx, (unsigned)cdiv(riders.j[i].n, 256));
  }
  PCA_REQUIRE(sw == nullptr || (sw->slab != nullptr && sw->M > 0 && sw->rows_per_wg > 0 && sw->dq >= 1 &&
                                sw->dq <= 4), "wgrad128: the small job rides with a slab");
  *sw_rows = sw == nullptr ? 0 : (int)cdiv(cdiv(sw->M, (int64_t)blocks_per_wg * sw->rows_per_wg), gx);
  return PCA_OK;
}

int wgrad128_shape(const WgradJobs& jobs, int rows_per_wg, const SlabSumJobs& riders, const SmallWgradArgs* sw,
                   unsigned* gx, unsigned* gy, int* sw_rows) {
  *gx = (unsigned)cdiv(wgrad_max_rows(jobs), rows_per_wg);
  // (two row groups per workgroup when every workgroup has at least four tiles to share)
  PCA_TRY(extra_rows(riders, sw, rows_per_wg >= 128 ? 2 : 1, *gx, sw_rows));
  *gy = (unsigned)(jobs.n + *sw_rows + riders.n);
  return PCA_OK;
}

int wgrad128_step_shape(const WgradJobs& bf, int rpw_bf, const WgradJobs& f32, int rpw_f32,
                        const SlabSumJobs& riders, const SmallWgradArgs* sw, WgradStepShape* out) {
  // (an empty bf16 list: it ran beside layer 1's few-queries backward, mab0_small_ride_launch)
  PCA_REQUIRE((bf.n == 0 || wgrad_max_rows(bf) > 0) && f32.n > 0 && wgrad_max_rows(f32) > 0,
              "wgrad128: the step launch takes lists with rows");
  PCA_REQUIRE(rpw_bf >= 128 && rpw_f32 >= 128, "wgrad128: the step launch runs two row groups");
  unsigned gx = std::max((unsigned)cdiv(wgrad_max_rows(bf), rpw_bf), (unsigned)cdiv(wgrad_max_rows(f32), rpw_f32));
  SlabSumJobs& rd = out->riders;
  rd = riders;
  if (bf.n == 0) {
    // No long rows hide the workgroups that leave at once (each takes a compute unit's whole LDS and
    // register file while it does): a rider wider than the fp32 rows is cut into column ranges of their
    // width, rows of its own (element by element the same sums).
    rd.n = 0;
    const int width = (int)gx * 256;
    for (int i = 0; i < riders.n; ++i) {
      const SlabSumJob& j = riders.j[i];
      for (int c = 0; c < j.n; c += width) {
        PCA_REQUIRE(rd.n < 40, "wgrad128: slab-sum table full");
        rd.j[rd.n++] = SlabSumJob{j.slabs + c, j.out + c, j.S, j.n - c < width ? j.n - c : width,
                                  j.accumulate, j.stride > 0 ? j.stride : j.n};
      }
    }
  }
  PCA_TRY(extra_rows(rd, sw, 2, gx, &out->sw_rows));
  out->gx = gx;
  out->gy = (unsigned)(bf.n + f32.n + out->sw_rows + rd.n);
  return PCA_OK;
}

// ---- shapes of the post launches ------------------
// shapes the fused post rows cover (post_fused_body: d = 128 as m x POST_FC and d threads of 256, a thread's
// dWq outputs in one column of I, at most POST_MAXM queries held in registers)
static bool post_fused_ok(const Mab0PostJob& a) {
  return a.d == 128 && a.h > 0 && a.m >= 1 && a.m <= POST_MAXM && a.dq >= 1 && a.dq <= 256 && 256 % a.dq == 0;
}
// whether a rider of the same launch writes where the job's second stage accumulates
static bool post_outputs_overlap(const Mab0PostJob& a, const SlabSumJobs& riders) {
  for (int i = 0; i < riders.n; ++i) {
    const SlabSumJob& r = riders.j[i];
    auto meets = [&](const float* q, int64_t k) {
      return r.out != nullptr && q != nullptr && r.out < q + k && q < r.out + r.n;
    };
    if (meets(a.dWq, (int64_t)a.d * a.dq) || meets(a.dbq, a.d) || meets(a.dI, (int64_t)a.m * a.dq)) return true;
  }
  return false;
}

// ---- the planner ------------------
static void push(TailPlan* P, TailKernel k, int64_t gx, int64_t gy) {
  P->seq[P->nseq++] = TailLaunch{k, (unsigned)gx, (unsigned)gy};
}
// THE cursor: the next 256-byte-aligned range of the slab area, null when it would pass `limit`
static float* take_slabs(const BwdDefer& D, TailPlaced& c, size_t bytes, size_t limit) {
  if (c.used + bytes > limit) return nullptr;
  float* at = D.slab_ws + c.used / sizeof(float);
  c.used += align256(bytes);
  return at;
}
// one slab per workgroup and job, and their sum jobs; more rows per workgroup until the list fits below `limit`
static int place_list(const BwdDefer& D, TailPlaced& c, WgradJobs& jobs, int& rows_per_wg, size_t limit) {
  size_t need;
  for (;; rows_per_wg *= 2) {
    need = 0;
    for (int i = 0; i < jobs.n; ++i) {
      const WgradJob& j = jobs.j[i];
      need += (size_t)cdiv(j.M, rows_per_wg) * ((j.g_hi - j.g_lo) * 128 + (j.db ? 128 : 0)) * 4;
    }
    if (c.used + need <= limit) break;
    PCA_REQUIRE(rows_per_wg < wgrad_max_rows(jobs), "plan_tail: no room for one slab per job (%zu bytes)", limit);
  }
  float* at = take_slabs(D, c, need, limit);
  for (int i = 0; i < jobs.n; ++i) {
    WgradJob& j = jobs.j[i];
    if (j.M <= 0) continue;
    const int nwg = (int)cdiv(j.M, rows_per_wg), n1 = (j.g_hi - j.g_lo) * 128, stride = n1 + (j.db ? 128 : 0);
    j.slab = at;
    PCA_REQUIRE(c.late.n + 2 <= 40, "wgrad128: slab-sum table full");
    c.late.j[c.late.n++] = SlabSumJob{at, j.dW + (int64_t)j.g_lo * 128, nwg, n1, 1, stride};
    if (j.db) c.late.j[c.late.n++] = SlabSumJob{at + n1, j.db, nwg, 128, 1, stride};
    at += (size_t)nwg * stride;
  }
  return PCA_OK;
}
// the layer-1 fc_v job's slab ([workgroups][128 dq + 128] partials) and its two sums, appended to `sums`
static bool place_fcv(const BwdDefer& D, TailPlaced& c, SmallWgradArgs& sw, SlabSumJobs& sums) {
  const int nwg = (int)cdiv(sw.M, sw.rows_per_wg), n1 = 128 * sw.dq, stride = n1 + 128;
  if (n1 % 4 != 0) return false;
  sw.slab = take_slabs(D, c, (size_t)nwg * stride * 4, D.slab_cap);
  if (sw.slab == nullptr) return false;
  sums.j[sums.n++] = SlabSumJob{sw.slab, sw.dW, nwg, n1, 1, stride};
  if (sw.db != nullptr) sums.j[sums.n++] = SlabSumJob{sw.slab + n1, sw.db, nwg, 128, 1, stride};
  return true;
}
// Every workgroup costs a 64 KiB slab: aim at ~200 workgroups over all bf16 jobs (512 rows for one B*N-row job,
// 1024 for three; swept: 1024 beat 512 / 768 and 2048 at 3 x 65536 rows; the fp32 jobs' 128 beat 64 and 256)
static int bf16_rows_per_wg(double rows) {
  const int rpw = 512 * (int)((rows + 98303.0) / 98304.0);
  return rpw < 512 ? 512 : (rpw > 1024 ? 1024 : rpw);
}
static double list_rows(WgradJobs& jobs) {       // (a list without rows counts as empty)
  double rows = 0;
  for (int i = 0; i < jobs.n; ++i) rows += (double)jobs.j[i].M;
  if (rows <= 0) jobs.n = 0;
  return rows;
}
// k_terminal1 (+ k_mab0_post2), or the post stages alone
static int plan_posts(const BwdDefer& D, TailPlan* P) {
  const Mab0PostJobs& J = D.posts;
  const SlabSumJobs& late = P->placed.late;
  const int has_sw = P->fcv == FcvRuns::TerminalRows || P->fcv == FcvRuns::TerminalRowsPost2Sums;
  int n1 = 0, n2 = 0;      // threads the widest job needs in each post stage (one output element per thread)
  for (int i = 0; i < J.n; ++i) {
    const Mab0PostJob& a = J.j[i];
    n1 = std::max(n1, a.d * a.dk + a.m * a.d);
    n2 = std::max(n2, a.d * a.dq + a.d + (a.dI ? a.m * a.dq : 0));
  }
  if (!D.has_cls && !has_sw && late.n == 0) {      // nothing rides: the two post launches
    if (J.n > 0) push(P, TailKernel::Post1, cdiv(n1, 256), J.n);
    if (J.n > 0) push(P, TailKernel::Post2, cdiv(n2, 256), J.n);
    return PCA_OK;
  }
  // Both post stages in k_terminal1 when every job has a shape the fused rows cover, no rider writes what they
  // accumulate into (in the two-launch form the launch boundary orders them) and no partials are left to sum.
  bool fuse = D.form.post_fuse && J.n > 0 && P->fcv != FcvRuns::TerminalRowsPost2Sums;
  for (int i = 0; fuse && i < J.n; ++i) fuse = post_fused_ok(J.j[i]) && !post_outputs_overlap(J.j[i], late);
  int gx = (int)cdiv(n1, 256);
  if (fuse) {                    // rows of fused workgroups, and rows of dWk workgroups
    gx = 0;
    for (int i = 0; i < J.n; ++i) {
      const Mab0PostJob& a = J.j[i];
      const int wk = a.DG != nullptr ? (int)cdiv(a.d * a.dk, 256) : 0;
      const int fw = a.d / POST_FC + (a.dI != nullptr ? a.m : 0);
      gx = std::max(gx, std::max(wk, fw));
    }
  }
  if (D.has_cls) gx = std::max(gx, D.cls.C);
  if (has_sw) gx = std::max(gx, (int)cdiv(P->small.M, P->small.rows_per_wg));
  for (int i = 0; i < late.n; ++i) {
    PCA_REQUIRE(slab_sum_job_ok(late.j[i]), "terminal: rider alignment");
    gx = std::max(gx, (int)cdiv(late.j[i].n, 256));
  }
  P->post_fused = fuse;
  push(P, TailKernel::Terminal1, gx, (fuse ? J.n : 0) + J.n + (D.has_cls ? 1 : 0) + has_sw + late.n);
  for (int i = 0; i < P->late2.n; ++i) n2 = std::max(n2, P->late2.j[i].n);
  if (!fuse && J.n > 0) push(P, TailKernel::Post2, cdiv(n2, 256), J.n + P->late2.n);
  if (!fuse && J.n == 0 && P->late2.n > 0) push(P, TailKernel::SumsLate2, 0, 0);
  return PCA_OK;
}

int plan_tail(const BwdDefer& D, TailPlan* P, bool bf16_only) {
  *P = TailPlan{};
  const TailForm& f = D.form;
  // Slab mode (the default when the caller lent room): per-workgroup partials, summed in a fixed order by rider
  // rows of k_terminal1 (`late`), no atomics: 0.324 ms/step at configs[1] against 0.335, and bit-reproducible.
  const bool slab_mode = f.slabs && D.slab_ws != nullptr && D.slab_cap > 0;
  TailPlaced& c = P->placed;
  c = D.placed;                  // (the bf16 list ran already: its slabs lie first, its sums come first)
  PCA_REQUIRE(!c.bf16_ran || (slab_mode && D.wg_bf16.n == 0), "plan_tail: bf16 jobs queued after the list ran");
  P->bf16 = D.wg_bf16, P->f32 = D.wg_f32;
  P->rows_bf16 = list_rows(P->bf16);
  P->rpw_bf16 = bf16_rows_per_wg(P->rows_bf16), P->rpw_f32 = 128;
  if (slab_mode && P->bf16.n > 0) PCA_TRY(place_list(D, c, P->bf16, P->rpw_bf16, D.slab_cap * 3 / 4));
  if (bf16_only) return PCA_OK;
  P->rows_f32 = list_rows(P->f32);
  const int at_f32 = c.late.n;
  if (slab_mode && P->f32.n > 0) PCA_TRY(place_list(D, c, P->f32, P->rpw_f32, D.slab_cap));
  // ONE launch for both lists: same partition, slabs and order of sums as the two: the same bits
  const bool folded = f.fold && P->f32.n > 0 && (P->bf16.n > 0 || c.bf16_ran);
  P->small = D.sw;
  if (D.has_sw) {
    // post_fuse: the fc_v job (it reads what layer 1's few-queries backward wrote, as the fp32 list does) runs as
    // rows of that list's launch and its two sums ride in k_terminal1 - when the table has room for them
    const bool with_f32 = f.post_fuse && slab_mode && P->f32.n > 0 && c.late.n + D.late.n + 2 <= 40;
    P->fcv = !(slab_mode && place_fcv(D, c, P->small, with_f32 ? c.late : P->late2)) ? FcvRuns::TerminalRows
             : with_f32 ? FcvRuns::WgradRows : FcvRuns::TerminalRowsPost2Sums;
    // (a launch per list: the fc_v sums precede the fp32 list's, the order k_terminal1 has run them in)
    if (P->fcv == FcvRuns::WgradRows && !folded)
      std::rotate(c.late.j + at_f32, c.late.j + c.late.n - (P->small.db != nullptr ? 2 : 1), c.late.j + c.late.n);
  }
  for (int i = 0; i < D.late.n; ++i) {
    PCA_REQUIRE(c.late.n < 40, "plan_tail: slab-sum table full");
    c.late.j[c.late.n++] = D.late.j[i];
  }
  // The sums the post stages read (D.sums: dG of the few-queries blocks) ride in the first weight-gradient launch
  const SmallWgradArgs* sw = P->fcv == FcvRuns::WgradRows ? &P->small : nullptr;
  P->step.riders = D.sums;
  bool carried = folded;
  if (folded) {
    PCA_TRY(wgrad128_step_shape(P->bf16, P->rpw_bf16, P->f32, P->rpw_f32, D.sums, sw, &P->step));
    push(P, TailKernel::WgradStep, P->step.gx, P->step.gy);
  } else {
    unsigned gx, gy;
    int rows;
    if (P->bf16.n > 0) {
      PCA_TRY(wgrad128_shape(P->bf16, P->rpw_bf16, D.sums, nullptr, &gx, &gy, &rows));
      push(P, TailKernel::Wgrad128Bf16, gx, gy);
    }
    if (P->f32.n > 0) {
      PCA_TRY(wgrad128_shape(P->f32, P->rpw_f32, P->nseq > 0 ? SlabSumJobs{} : D.sums, sw, &gx, &gy, &rows));
      push(P, TailKernel::Wgrad128F32, gx, gy);
    }
    carried = P->nseq > 0;
  }
  if (D.wg256_n > 0) push(P, TailKernel::Wgrad256, 0, 0);
  if (!carried && D.sums.n > 0) push(P, TailKernel::SumsDue, 0, 0);      // (nobody carried them)
  return plan_posts(D, P);
}

}  // namespace pca

// ---- a host view of the plan (tests/test_tail_plan_host.py; not part of the documented ABI) ------------------
// in:  [0] TailForm as bits (slabs 1, fold 2, ride 4, post_fuse 8, midfuse_wide 16, midfuse_small 32, dz_mask 64;
//      -1: tail_form_from_env), [1] slab_cap in bytes, [2] the bf16 list rode (planned alone first, as
//      bwd_defer_ride does), [3] bf16 jobs, [4] fp32 jobs, [5] fc_v job present, [6] its M, [7] its dq, [8] post
//      jobs, [9] due sums, [10] pending late sums, [11] classes of the classifier's job (0: none), then per
//      weight-gradient job (M, db present, g_lo, g_hi), per post job (m, dq, dk, dI present), per sum its width.
// out: [0] form bits, [1] rows per workgroup bf16, [2] fp32, [3] FcvRuns, [4] post_fused, [5] launches, [6] slabs,
//      [7] late, [8] late2, [9] riders of the first weight-gradient launch, [10] bytes of the slab area used,
//      then per launch (TailKernel, grid x, grid y), per slab (list 0 bf16 / 1 fp32 / 2 fc_v, job, byte offset,
//      bytes), per late and late2 entry (slab byte offset or -1 - index of the pending sum, output buffer, width,
//      slabs), per rider its width.  Buffers are numbered: job i of list l writes dW 2 (16 l + i) and db
//      2 (16 l + i) + 1, the fc_v job 64 / 65, pending late sum i 100 + i.
// Every pointer is a made-up address that nothing reads.  Returns PCA_EINVAL when `out` is too short.
extern "C" int pca_debug_tail_plan(const int64_t* in, int n_in, int64_t* out, int n_out) {
  using namespace pca;
  PCA_REQUIRE(in != nullptr && out != nullptr && n_in >= 12, "pca_debug_tail_plan: null or short input");
  const int nb = (int)in[3], nf = (int)in[4], np = (int)in[8], ns = (int)in[9], nl = (int)in[10];
  PCA_REQUIRE(nb >= 0 && nb <= 16 && nf >= 0 && nf <= 16 && np >= 0 && np <= 3 && ns >= 0 && ns <= 40 && nl >= 0 &&
                  nl <= 40 && n_in >= 12 + 4 * (nb + nf + np) + ns + nl,
              "pca_debug_tail_plan: table sizes");
  auto buf = [](int64_t id) { return reinterpret_cast<float*>((uintptr_t)0x100000000ull + ((uintptr_t)id << 24)); };
  float* const slab_ws = reinterpret_cast<float*>((uintptr_t)0x700000000000ull);
  BwdDefer D{};
  if (in[0] < 0) {
    D.form = tail_form_from_env();
  } else {
    const int64_t b = in[0];
    D.form = TailForm{(b & 1) != 0, (b & 2) != 0, (b & 4) != 0, (b & 8) != 0, (b & 16) != 0, (b & 32) != 0, (b & 64) != 0};
  }
  D.slab_cap = (size_t)in[1];
  D.slab_ws = D.slab_cap > 0 ? slab_ws : nullptr;
  const int64_t* q = in + 12;
  for (int l = 0; l < 2; ++l) {
    WgradJobs& L = l == 0 ? D.wg_bf16 : D.wg_f32;
    for (int i = 0; i < (l == 0 ? nb : nf); ++i, q += 4)
      L.j[L.n++] = WgradJob{buf(200 + 32 * l + 2 * i), buf(201 + 32 * l + 2 * i), buf(2 * (16 * l + i)),
                            q[1] ? buf(2 * (16 * l + i) + 1) : nullptr, q[0], (int)q[2], (int)q[3]};
  }
  if (in[5]) {
    D.sw = SmallWgradArgs{buf(300), buf(301), in[6], (int)in[7], 64, in[6] * in[7], buf(64), buf(65), nullptr};
    D.has_sw = 1;
  }
  for (int i = 0; i < np; ++i, q += 4) {
    Mab0PostJob a{};
    a.DG = buf(310 + 8 * i); a.dWq = buf(311 + 8 * i); a.dbq = buf(312 + 8 * i);
    a.dI = q[3] ? buf(313 + 8 * i) : nullptr;
    a.m = (int)q[0]; a.d = 128; a.dq = (int)q[1]; a.dk = (int)q[2]; a.h = 4;
    D.posts.j[D.posts.n++] = a;
  }
  for (int i = 0; i < ns; ++i) D.sums.j[D.sums.n++] = SlabSumJob{buf(400 + i), buf(450 + i), 3, (int)*q++, 0, 0};
  for (int i = 0; i < nl; ++i) D.late.j[D.late.n++] = SlabSumJob{buf(500 + i), buf(100 + i), 3, (int)*q++, 1, 0};
  if (in[11] > 0) {
    D.has_cls = 1;
    D.cls.C = (int)in[11];
  }
  TailPlan P{};
  WgradJobs rode{};
  if (in[2]) {
    PCA_TRY(plan_tail(D, &P, true));
    rode = P.bf16;
    D.placed = P.placed;
    D.placed.bf16_ran = true;
    D.wg_bf16.n = 0;
  }
  const int rpw_rode = P.rpw_bf16;
  PCA_TRY(plan_tail(D, &P));
  if (in[2]) {
    P.bf16 = rode;
    P.rpw_bf16 = rpw_rode;
  }
  const TailForm& f = D.form;
  int64_t slabs[33][4];
  int nslab = 0;
  auto slab = [&](int list, int job, const float* at, int64_t floats) {
    if (at == nullptr) return;
    slabs[nslab][0] = list; slabs[nslab][1] = job;
    slabs[nslab][2] = (int64_t)(at - slab_ws) * 4; slabs[nslab++][3] = floats * 4;
  };
  for (int l = 0; l < 2; ++l) {
    const WgradJobs& L = l == 0 ? P.bf16 : P.f32;
    for (int i = 0; i < L.n; ++i) {
      const WgradJob& j = L.j[i];
      slab(l, i, j.slab, cdiv(j.M, l == 0 ? P.rpw_bf16 : P.rpw_f32) * ((j.g_hi - j.g_lo) * 128 + (j.db ? 128 : 0)));
    }
  }
  if (P.fcv != FcvRuns::Nowhere)
    slab(2, 0, P.small.slab, cdiv(P.small.M, P.small.rows_per_wg) * (128 * P.small.dq + 128));
  const SlabSumJobs& late = P.placed.late;
  const int need = 11 + 3 * P.nseq + 4 * nslab + 4 * (late.n + P.late2.n) + P.step.riders.n;
  PCA_REQUIRE(n_out >= need, "pca_debug_tail_plan: out holds %d words, the plan %d", n_out, need);
  int64_t* o = out;
  *o++ = f.slabs | f.fold << 1 | f.ride << 2 | f.post_fuse << 3 | f.midfuse_wide << 4 | f.midfuse_small << 5 | f.dz_mask << 6;
  *o++ = P.rpw_bf16; *o++ = P.rpw_f32; *o++ = (int64_t)P.fcv; *o++ = P.post_fused; *o++ = P.nseq; *o++ = nslab;
  *o++ = late.n; *o++ = P.late2.n; *o++ = P.step.riders.n; *o++ = (int64_t)P.placed.used;
  for (int i = 0; i < P.nseq; ++i) { *o++ = (int64_t)P.seq[i].kernel; *o++ = P.seq[i].gx; *o++ = P.seq[i].gy; }
  for (int i = 0; i < nslab; ++i) for (int k = 0; k < 4; ++k) *o++ = slabs[i][k];
  for (int t = 0; t < 2; ++t) {
    const SlabSumJobs& S = t == 0 ? late : P.late2;
    for (int i = 0; i < S.n; ++i) {
      const SlabSumJob& j = S.j[i];
      const bool mine = j.slabs >= slab_ws;
      *o++ = mine ? (int64_t)(j.slabs - slab_ws) * 4 : -1 - (int64_t)(((uintptr_t)j.slabs - 0x100000000ull) >> 24) + 500;
      *o++ = (int64_t)(((uintptr_t)j.out - 0x100000000ull) >> 24);
      *o++ = j.n; *o++ = j.S;
    }
  }
  for (int i = 0; i < P.step.riders.n; ++i) *o++ = P.step.riders.j[i].n;
  return PCA_OK;
}
