// The end of a backward pass: bwd_defer_flush runs everything the blocks of a step queued in their BwdDefer
// (bwd_defer.hpp) - the weight-gradient launch (wgrad128.hip: both d = 128 lists in one; wgrad256.hip) with
// the due slab sums as riders, then the post stages:
//
//   k_mab0_post1 / k_terminal1   dWk and dQp of the shared queries (k_terminal1: the same plus the classifier's
//                                weight gradient, the layer-1 fc_v gradient and late slab sums as extra rows;
//                                with PCA_POST_FUSE, the default, also what k_mab0_post2 computes, in rows of
//                                workgroups that keep their part of dQp in LDS - no second launch)
//   k_mab0_post2                 dWq, dbq, dI from dQp (+ the sums of the partials k_terminal1 itself wrote)
#include "bwd_defer.hpp"
#include "terminal_bodies.hpp"
#include "slab_sum_body.hpp"

#include <stdlib.h>

namespace pca {

namespace {

// ---------------------------------------------------------------------------------
// shared-query parameters.  dQs = sum_b dO[b] ([m][d]); DG = sum over sets of dS X in
// "ln2 units": dG_raw = sl2e * DG.
//   dWk[f][c]  += sum_q Qp[q][f] dG_raw[j m + q][c]            (j = head of f)
//   dQp[q][f]   = dQs[q][f] + sum_c dG_raw[j m + q][c] Wk[f][c]
//   dWq += dQp^T I ; dbq += colsum(dQp) ; dI += dQp Wq
// ---------------------------------------------------------------------------------
// dot of two strided sequences with NF independent load pairs in flight (the post kernels are a
// few dependent L2 round trips long and nothing else: a 128-term dot is 2 trips at NF = 64, 8 at 16)
template <int NF = 64>
__device__ __forceinline__ float dot_strided(const float* __restrict__ a, int64_t sa,
                                             const float* __restrict__ b, int64_t sb, int n) {
  float acc = 0.f;
  int i = 0;
  for (; i + NF <= n; i += NF) {
    float x[NF], y[NF];
#pragma unroll
    for (int u = 0; u < NF; ++u) { x[u] = a[(i + u) * sa]; y[u] = b[(i + u) * sb]; }
#pragma unroll
    for (int u = 0; u < NF; ++u) acc = fmaf(x[u], y[u], acc);
  }
  for (; i + 16 <= n; i += 16) {
    float x[16], y[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) { x[u] = a[(i + u) * sa]; y[u] = b[(i + u) * sb]; }
#pragma unroll
    for (int u = 0; u < 16; ++u) acc = fmaf(x[u], y[u], acc);
  }
  for (; i < n; ++i) acc = fmaf(a[i * sa], b[i * sb], acc);
  return acc;
}

// one element of dQp = dQs + (dG_raw Wk_h^T): the sum over the sets of dO in batches of 64 / 16 loads, then
// + sl2e * <DG row, Wk row>.  Shared by post1_body and the fused post rows (post_fused_body), which have to
// round alike.
__device__ __forceinline__ float post_dqp(const Mab0PostJob& a, int q, int f) {
  const int m = a.m, d = a.d, dk = a.dk;
  const int j = f / (d / a.h);
  const int oo = q * d + f;
  float qs;
  if (a.dQs != nullptr) {
    qs = a.dQs[oo];
  } else {                                  // sum over the sets, 16 loads in flight
    qs = 0.f;
    const int64_t sb = (int64_t)m * d;
    int bb = 0;
    for (; bb + 64 <= a.B; bb += 64) {
      float v[64];
#pragma unroll
      for (int u = 0; u < 64; ++u) v[u] = a.dO[(bb + u) * sb + oo];
#pragma unroll
      for (int u = 0; u < 64; ++u) qs += v[u];
    }
    for (; bb + 16 <= a.B; bb += 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = a.dO[(bb + u) * sb + oo];
#pragma unroll
      for (int u = 0; u < 16; ++u) qs += v[u];
    }
    for (; bb < a.B; ++bb) qs += a.dO[bb * sb + oo];
  }
  return a.DG == nullptr ? qs
                         : qs + a.sl2e * dot_strided(a.DG + (int64_t)(j * m + q) * dk, 1,
                                                     a.Wk + (int64_t)f * dk, 1, dk);
}

// stage 1 (grid-parallel): dWk and dQp = dQs + (dG_raw Wk_h^T); blockIdx.y = MAB.  wk_only: the dWk
// workgroups alone (dQp belongs to the fused post rows of the same launch)
__device__ __forceinline__ void post1_body(const Mab0PostJob& a, int blk, bool wk_only = false) {
  const int m = a.m, d = a.d, dk = a.dk;
  const int dh = d / a.h;
  const int o = blk * 256 + threadIdx.x;
  if (o < d * dk) {
    if (a.DG == nullptr) return;            // keys were projected: dWk comes from the GEMM path
    const int f = o / dk, c = o - f * dk, j = f / dh;
    a.dWk[o] += a.sl2e * dot_strided(a.Qp + f, d, a.DG + (int64_t)j * m * dk + c, dk, m);
  } else if (!wk_only && o < d * dk + m * d) {
    const int oo = o - d * dk;
    const int q = oo / d, f = oo - q * d;
    a.dQp[oo] = post_dqp(a, q, f);
  }
}

// Both post stages of one job in ONE launch (fused post rows of k_terminal1): what k_mab0_post2 reads from
// stage 1 is dQp alone, [m][d] floats, so a workgroup computes the part of dQp it needs itself, keeps it in
// LDS and goes on after a workgroup barrier - no second launch orders the two stages.
//   column workgroups [0, d / POST_FC): POST_FC features f each.  Phase 1: thread (q, f) computes dQp[q][f]
//     (post_dqp: the bits of stage 1), to LDS and to a.dQp.  Phase 2: dWq[f][c] += sum_q dQp[q][f] I[q][c]
//     (fmaf over q from 0, as dot_strided), dbq[f] += sum_q dQp[q][f] (sequential adds, as k_mab0_post2).
//   row workgroups [d / POST_FC, + m) (dI != null): phase 1 recomputes row q of dQp (the same bits), phase 2
//     is dI[q][c] += <dQp row, Wq column> (fmaf over f from 0, 64 loads in flight as dot_strided).
// I and the old dWq / dbq / dI do not depend on dQp: they are requested before phase 1.  Every thread of a
// live workgroup reaches the barrier.  Shapes: post_fused_ok.
constexpr int POST_FC = 4, POST_MAXM = 16;
__device__ __forceinline__ void post_fused_body(const Mab0PostJob& a, int x) {
  const int m = a.m, d = a.d, dq = a.dq;
  const int ncol = d / POST_FC, nrow = a.dI != nullptr ? m : 0;
  if (x >= ncol + nrow) return;             // (uniform per workgroup)
  __shared__ float sq[256];
  const int tid = threadIdx.x;
  if (x < ncol) {
    const int f0 = x * POST_FC;
    const int c = tid % dq;                 // 256 % dq == 0: the same column for every output of a thread
    float iv[POST_MAXM], old[4], oldb[4];
#pragma unroll
    for (int q = 0; q < POST_MAXM; ++q) iv[q] = q < m ? a.I[q * dq + c] : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int o = tid + 256 * k;
      const bool act = o < POST_FC * dq;
      const int f = f0 + o / dq;
      old[k] = act ? a.dWq[f * dq + c] : 0.f;
      oldb[k] = act && c == 0 ? a.dbq[f] : 0.f;
    }
    if (tid < m * POST_FC) {
      const int q = tid / POST_FC, f = f0 + tid % POST_FC;
      const float v = post_dqp(a, q, f);
      sq[tid] = v;
      a.dQp[q * d + f] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int o = tid + 256 * k;
      if (o < POST_FC * dq) {
        const int fl = o / dq;
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < POST_MAXM; ++q)
          if (q < m) acc = fmaf(sq[q * POST_FC + fl], iv[q], acc);
        a.dWq[(f0 + fl) * dq + c] = old[k] + acc;
        if (c == 0) {
          float s = 0.f;
          for (int q = 0; q < m; ++q) s += sq[q * POST_FC + fl];
          a.dbq[f0 + fl] = oldb[k] + s;
        }
      }
    }
  } else {
    const int q = x - ncol;
    const bool act = tid < dq;
    const float old = act ? a.dI[q * dq + tid] : 0.f;
    if (tid < d) sq[tid] = post_dqp(a, q, tid);
    __syncthreads();
    if (act) {
      const float* __restrict__ w = a.Wq + tid;
      float acc = 0.f;
      int i = 0;
      for (; i + 64 <= d; i += 64) {
        float y[64];
#pragma unroll
        for (int u = 0; u < 64; ++u) y[u] = w[(int64_t)(i + u) * dq];
#pragma unroll
        for (int u = 0; u < 64; ++u) acc = fmaf(sq[i + u], y[u], acc);
      }
      for (; i < d; ++i) acc = fmaf(sq[i], w[(int64_t)i * dq], acc);
      a.dI[q * dq + tid] = old + acc;
    }
  }
}
__global__ __launch_bounds__(256) void k_mab0_post1(const Mab0PostJobs jobs) {
  post1_body(jobs.j[blockIdx.y], blockIdx.x);
}
// stage 1 + riders: rows [0, J.n) of blockIdx.y are the post-1 jobs, then (when present) the
// classifier weight gradient (one workgroup per class) and the layer-1 fc_v gradient.
// nfuse = J.n (else 0): J.n rows of fused post workgroups (post_fused_body: dQp and everything k_mab0_post2
// would compute from it) come first - the longest chains of the launch - and the post-1 rows behind them hold
// the dWk workgroups alone.
__global__ __launch_bounds__(256) void k_terminal1(const Mab0PostJobs jobs, int nfuse, const ClsWgradArgs c,
                                                   int has_cls, const SmallWgradArgs w,
                                                   int has_sw, const SlabSumJobs late) {
  if ((int)blockIdx.y < nfuse) {
    post_fused_body(jobs.j[blockIdx.y], blockIdx.x);
    return;
  }
  const int y = (int)blockIdx.y - nfuse;
  if (y < jobs.n) {
    post1_body(jobs.j[y], blockIdx.x, nfuse != 0);
  } else if (has_cls && y == jobs.n) {
    if ((int)blockIdx.x < c.C)
      cls_wgrad_body(c.dlogits, c.P, c.lossv, c.corrv, c.B, c.d, c.C, c.dWc, c.dbc, c.loss_out,
                     c.stats, blockIdx.x);
  } else if (has_sw && y == jobs.n + has_cls) {
    if ((int64_t)blockIdx.x * w.rows_per_wg < w.M)
      wgrad_small_body<float>(w.G, w.X, w.M, w.dq, w.rows_per_wg, w.x_head_stride, w.dW, w.db,
                              blockIdx.x, w.slab);
  } else {
    // rider rows: the weight-gradient slabs of this step, added in a fixed order
    __shared__ float4 red[4 * 64];
    slab_sum_body(late.j[y - jobs.n - has_cls - has_sw], blockIdx.x, threadIdx.x, red);
  }
}
// stage 2: dWq += dQp^T I ; dbq += colsum(dQp) ; dI += dQp Wq
__global__ __launch_bounds__(256) void k_mab0_post2(const Mab0PostJobs jobs, const SlabSumJobs late) {
  if ((int)blockIdx.y >= jobs.n) {       // rider rows (partials written by k_terminal1 itself)
    __shared__ float4 red[4 * 64];
    slab_sum_body(late.j[blockIdx.y - jobs.n], blockIdx.x, threadIdx.x, red);
    return;
  }
  const Mab0PostJob a = jobs.j[blockIdx.y];
  const int m = a.m, d = a.d, dq = a.dq;
  const int o = blockIdx.x * 256 + threadIdx.x;
  const int n1 = d * dq, n2 = n1 + d, n3 = n2 + (a.dI != nullptr ? m * dq : 0);
  if (o < n1) {
    const int f = o / dq, c = o - f * dq;
    a.dWq[o] += dot_strided(a.dQp + f, d, a.I + c, dq, m);
  } else if (o < n2) {
    const int f = o - n1;
    float acc = 0.f;
    for (int q = 0; q < m; ++q) acc += a.dQp[q * d + f];
    a.dbq[f] += acc;
  } else if (o < n3) {
    const int oo = o - n2;
    const int q = oo / dq, c = oo - q * dq;
    a.dI[oo] += dot_strided(a.dQp + (int64_t)q * d, 1, a.Wq + c, dq, d);
  }
}

}  // namespace

// threads the widest job needs in each post stage (one output element per thread; grid.x = cdiv(., 256))
struct PostExtents { int n1, n2; };
static PostExtents post_extents(const Mab0PostJobs& J) {
  PostExtents x{0, 0};
  for (int i = 0; i < J.n; ++i) {
    const Mab0PostJob& a = J.j[i];
    const int e1 = a.d * a.dk + a.m * a.d, e2 = a.d * a.dq + a.d + (a.dI ? a.m * a.dq : 0);
    x.n1 = e1 > x.n1 ? e1 : x.n1;
    x.n2 = e2 > x.n2 ? e2 : x.n2;
  }
  return x;
}

// shapes the fused post rows cover (post_fused_body: d = 128 as m x POST_FC and d threads of 256, a thread's
// dWq outputs in one column of I, at most POST_MAXM queries held in registers)
static bool post_fused_ok(const Mab0PostJob& a) {
  return a.d == 128 && a.h > 0 && a.m >= 1 && a.m <= POST_MAXM && a.dq >= 1 && a.dq <= 256 && 256 % a.dq == 0;
}
static bool ranges_meet(const float* p, int64_t n, const float* q, int64_t k) {
  return p != nullptr && q != nullptr && p < q + k && q < p + n;
}
// whether a rider of the same launch writes where the job's second stage accumulates
static bool post_outputs_overlap(const Mab0PostJob& a, const SlabSumJobs& riders) {
  for (int i = 0; i < riders.n; ++i) {
    const SlabSumJob& r = riders.j[i];
    if (ranges_meet(r.out, r.n, a.dWq, (int64_t)a.d * a.dq) || ranges_meet(r.out, r.n, a.dbq, a.d) ||
        ranges_meet(r.out, r.n, a.dI, (int64_t)a.m * a.dq))
      return true;
  }
  return false;
}
bool post_fuse_on() {            // (read per call, like the switches below)
  return env_not_zero("PCA_POST_FUSE");
}

int terminal_launch(const BwdDefer& D, hipStream_t st, const SlabSumJobs* late_in) {
  SlabSumJobs late{};
  if (late_in != nullptr) late = *late_in;
  if (!D.has_cls && !D.has_sw && late.n == 0) return mab0_post_launch(D.posts, st);
  const Mab0PostJobs& J = D.posts;
  const PostExtents x = post_extents(J);
  // Both post stages in this launch (PCA_POST_FUSE) when every job has a shape the fused rows cover, no rider
  // writes what they accumulate into (in the two-launch form the launch boundary orders them) and this launch
  // leaves no partials to sum (the layer-1 fc_v job ran in k_wgrad128_step); else k_terminal1, then k_mab0_post2.
  bool fuse = post_fuse_on() && J.n > 0 && !(D.has_sw && D.sw.slab != nullptr);
  for (int i = 0; fuse && i < J.n; ++i) fuse = post_fused_ok(J.j[i]) && !post_outputs_overlap(J.j[i], late);
  int gx = (int)cdiv(x.n1, 256);
  if (fuse) {                    // rows of fused workgroups, and rows of dWk workgroups
    gx = 0;
    for (int i = 0; i < J.n; ++i) {
      const Mab0PostJob& a = J.j[i];
      const int wk = a.DG != nullptr ? (int)cdiv(a.d * a.dk, 256) : 0;
      const int fw = a.d / POST_FC + (a.dI != nullptr ? a.m : 0);
      gx = wk > gx ? wk : gx;
      gx = fw > gx ? fw : gx;
    }
  }
  if (D.has_cls && D.cls.C > gx) gx = D.cls.C;
  if (D.has_sw) {
    const int gs = (int)cdiv(D.sw.M, D.sw.rows_per_wg);
    gx = gs > gx ? gs : gx;
  }
  for (int i = 0; i < late.n; ++i) {
    PCA_REQUIRE(slab_sum_job_ok(late.j[i]), "terminal: rider alignment");
    const int need = (int)cdiv(late.j[i].n, 256);
    gx = need > gx ? need : gx;
  }
  const int nfuse = fuse ? J.n : 0;
  hipLaunchKernelGGL(k_terminal1,
                     dim3(gx, nfuse + J.n + (D.has_cls ? 1 : 0) + (D.has_sw ? 1 : 0) + late.n),
                     dim3(256), 0, st, J, nfuse, D.cls, D.has_cls ? 1 : 0, D.sw, D.has_sw ? 1 : 0, late);
  PCA_TRY(check_launch("k_terminal1"));
  if (fuse) return PCA_OK;
  // the layer-1 fc_v partials k_terminal1 wrote (slab mode) are summed by rider rows of post 2
  SlabSumJobs late2{};
  if (D.has_sw && D.sw.slab != nullptr) {
    const int nwg = (int)cdiv(D.sw.M, D.sw.rows_per_wg), n1 = 128 * D.sw.dq, stride = n1 + 128;
    late2.j[late2.n++] = SlabSumJob{D.sw.slab, D.sw.dW, nwg, n1, 1, stride};
    if (D.sw.db != nullptr) late2.j[late2.n++] = SlabSumJob{D.sw.slab + n1, D.sw.db, nwg, 128, 1, stride};
  }
  if (J.n == 0) return slab_sum_jobs(late2, st);
  int n2 = x.n2;
  for (int i = 0; i < late2.n; ++i) n2 = late2.j[i].n > n2 ? late2.j[i].n : n2;
  hipLaunchKernelGGL(k_mab0_post2, dim3((unsigned)cdiv(n2, 256), J.n + late2.n), dim3(256), 0, st, J,
                     late2);
  return check_launch("k_mab0_post2");
}

int mab0_post_launch(const Mab0PostJobs& J, hipStream_t st) {
  if (J.n == 0) return PCA_OK;
  const PostExtents x = post_extents(J);
  hipLaunchKernelGGL(k_mab0_post1, dim3((unsigned)cdiv(x.n1, 256), J.n), dim3(256), 0, st, J);
  PCA_TRY(check_launch("k_mab0_post1"));
  hipLaunchKernelGGL(k_mab0_post2, dim3((unsigned)cdiv(x.n2, 256), J.n), dim3(256), 0, st, J,
                     SlabSumJobs{});
  return check_launch("k_mab0_post2");
}

bool wgrad_slabs_on() {          // (read per call: a test switches it between two engines)
  return env_not_zero("PCA_WGRAD_SLABS");
}
bool wgrad_fold_on() {           // (read per call, like the switch above)
  return env_not_zero("PCA_WGRAD_FOLD");
}
// PCA_WGRAD_RIDE: the bf16 list in the launch of layer 1's few-queries backward (k_mab0_small_ride);
// unset = the measured default.  Read per call, like the switches above.
constexpr bool WGRAD_RIDE_DEFAULT = true;
bool wgrad_ride_on() {
  const char* e = getenv("PCA_WGRAD_RIDE");
  if (e == nullptr || e[0] == 0) return WGRAD_RIDE_DEFAULT;
  return e[0] != '0';
}
// Every workgroup costs a 64 KiB slab (16384 atomics without the slabs): aim at ~200 workgroups over all
// bf16 jobs (512 rows for one B*N-row job, 1024 for three, ...).  (Swept before k_wgrad128 kept several
// tiles in flight, and kept because the partition fixes the summation order: 1024 beat 512 / 768 and 2048
// at 3 x 65536 rows.)
static int bf16_rows_per_wg(double rows) {
  const int rpw = 512 * (int)((rows + 98303.0) / 98304.0);
  return rpw < 512 ? 512 : (rpw > 1024 ? 1024 : rpw);
}
static size_t bf16_slab_cap(const BwdDefer& D) { return D.slab_cap * 3 / 4; }

bool bwd_defer_ride(BwdDefer& D, WgradJobs* jobs, int* rows_per_wg, int* rc) {
  *rc = PCA_OK;
  if (!(wgrad_slabs_on() && D.slab_ws != nullptr && D.slab_cap > 0 && wgrad_fold_on() && wgrad_ride_on()))
    return false;
  if (D.wg_bf16.n == 0 || D.ride_done) return false;
  double rows = 0;
  for (int i = 0; i < D.wg_bf16.n; ++i) rows += (double)D.wg_bf16.j[i].M;
  if (rows <= 0) return false;
  *jobs = D.wg_bf16;
  *rows_per_wg = bf16_rows_per_wg(rows);
  D.ride_late.n = 0;
  WgradSlabs sl{D.slab_ws, bf16_slab_cap(D), &D.ride_late, nullptr, 0};
  *rc = wgrad128_place(*jobs, *rows_per_wg, &sl);
  if (*rc != PCA_OK) return false;
  D.ride_used = (sl.used + 255) & ~(size_t)255;
  D.ride_done = 1;
  D.wg_bf16.n = 0;
  return true;
}

int bwd_defer_flush(BwdDefer& D, hipStream_t st) {
  // The sums the post stages read (D.sums: dG of the few-queries blocks) ride in the first
  // weight-gradient launch as extra workgroup rows.  Slab mode (the default when the caller lent
  // room; PCA_WGRAD_SLABS=0 switches back to fp32 atomics): the weight gradients themselves use no
  // atomics either - per-workgroup partials, summed in a fixed order by rider rows of k_terminal1
  // (`late`: only the optimizer reads them).  With EVERY reduction of the step in this form
  // configs[1] measured 0.324 ms/step against 0.335 with the atomics (three same-box pairs), and the
  // step is bit-reproducible.  (With only k_wgrad128 converted it was 0.343 ... 0.361 against 0.348,
  // depending on where the partials happened to lie.)
  const bool slab_mode = wgrad_slabs_on() && D.slab_ws != nullptr && D.slab_cap > 0;
  SlabSumJobs late{};
  size_t used = 0;          // the two lists' slabs lie back to back
  if (D.ride_done) {        // the bf16 list ran already: its slabs lie first, its sums come first
    PCA_REQUIRE(slab_mode && D.wg_bf16.n == 0, "bwd_defer_flush: bf16 jobs queued after the list ran");
    late = D.ride_late;
    used = D.ride_used;
  }
  double rows = 0, rows_f32 = 0;
  for (int i = 0; i < D.wg_bf16.n; ++i) rows += (double)D.wg_bf16.j[i].M;
  for (int i = 0; i < D.wg_f32.n; ++i) rows_f32 += (double)D.wg_f32.j[i].M;
  // the fp32 jobs ([B*m] rows) take 128 rows per workgroup (128 beat 64 and 256, swept with the bf16
  // list's rows above)
  int rpw = bf16_rows_per_wg(rows);
  int rpw_f32 = 128;
  const size_t cap_bf16 = bf16_slab_cap(D);
  // PCA_POST_FUSE: the layer-1 fc_v job (it reads what layer 1's few-queries backward wrote, as the fp32 list
  // does) runs as rows of the folded launch instead of k_terminal1's, so that its two slab sums are riders of
  // k_terminal1 and nothing is left for a launch behind it.  Its slab lies behind the fp32 list's, where the
  // flush put it before; called once the lists are placed.
  SmallWgradArgs small{};
  auto take_small = [&](int reserve = 0) -> const SmallWgradArgs* {   // reserve: sum jobs still to be appended
    if (!(post_fuse_on() && slab_mode && D.has_sw) || (128 * D.sw.dq) % 4 != 0 ||
        late.n + D.late.n + reserve + 2 > 40)
      return nullptr;
    const int nwg = (int)cdiv(D.sw.M, D.sw.rows_per_wg), n1 = 128 * D.sw.dq, stride = n1 + 128;
    if (used + (size_t)nwg * stride * 4 > D.slab_cap) return nullptr;
    small = D.sw;
    small.slab = D.slab_ws + used / sizeof(float);
    used += ((size_t)nwg * stride * 4 + 255) & ~(size_t)255;
    late.j[late.n++] = SlabSumJob{small.slab, small.dW, nwg, n1, 1, stride};
    if (small.db != nullptr) late.j[late.n++] = SlabSumJob{small.slab + n1, small.db, nwg, 128, 1, stride};
    D.has_sw = 0;
    return &small;
  };
  if (D.ride_done && rows_f32 > 0 && wgrad_fold_on()) {
    // the same launch with an empty bf16 list: the fp32 jobs and the sums that are due now
    WgradJobs f32 = D.wg_f32;
    ProfScope ps(PCA_K_WGRAD, st, 2.0 * rows_f32 * 128 * 128, 8.0 * rows_f32 * 128);
    WgradSlabs sf{D.slab_ws + used / sizeof(float), D.slab_cap - used, &late, nullptr, 0};
    PCA_TRY(wgrad128_place(f32, rpw_f32, &sf));
    used += (sf.used + 255) & ~(size_t)255;
    PCA_TRY(wgrad128_launch_step(WgradJobs{}, rpw, f32, rpw_f32, D.sums, st, take_small()));
    ps.end();
    D.wg_f32.n = 0;
    D.sums.n = 0;
  }
  if (rows > 0 && rows_f32 > 0 && wgrad_fold_on()) {
    // ONE launch (k_wgrad128_step): the fp32 jobs run beside the bf16 rows (which leave a quarter of
    // the compute units idle) instead of paying a launch boundary and a ramp of their own: 32 us
    // against 25 + 9.5.  Same partition, same slabs, same order of the slab sums as the two launches
    // below: the same bits.
    WgradJobs bf = D.wg_bf16, f32 = D.wg_f32;
    ProfScope ps(PCA_K_WGRAD, st, 2.0 * (rows + rows_f32) * 128 * 128,
                 4.0 * rows * 128 + 8.0 * rows_f32 * 128);
    WgradSlabs sl{slab_mode ? D.slab_ws : nullptr, cap_bf16, &late, nullptr, 0};
    PCA_TRY(wgrad128_place(bf, rpw, &sl));
    used = (sl.used + 255) & ~(size_t)255;
    WgradSlabs sf{slab_mode ? D.slab_ws + used / sizeof(float) : nullptr, D.slab_cap - used, &late,
                  nullptr, 0};
    PCA_TRY(wgrad128_place(f32, rpw_f32, &sf));
    used += (sf.used + 255) & ~(size_t)255;
    PCA_TRY(wgrad128_launch_step(bf, rpw, f32, rpw_f32, D.sums, st, take_small()));
    ps.end();
    D.wg_bf16.n = D.wg_f32.n = 0;
    D.sums.n = 0;
  }
  if (D.wg_bf16.n > 0) {
    ProfScope ps(PCA_K_WGRAD, st, 2.0 * rows * 128 * 128, 4.0 * rows * 128);
    WgradSlabs sl{slab_mode ? D.slab_ws : nullptr, cap_bf16, &late, &D.sums, 0};
    PCA_TRY(wgrad128_launch(D.wg_bf16, true, true, rpw, st, &sl));
    used = (sl.used + 255) & ~(size_t)255;
    ps.end();
    D.wg_bf16.n = 0;
    D.sums.n = 0;
  }
  if (D.wg_f32.n > 0) {
    WgradSlabs sl{slab_mode ? D.slab_ws + used / sizeof(float) : nullptr, D.slab_cap - used, &late,
                  &D.sums, 0};
    // (the two lists as a launch each, PCA_WGRAD_FOLD=0: the fc_v job rides with the fp32 one, behind its
    //  slabs - placed here first to learn where they end; the launch places them again, the same way)
    const SmallWgradArgs* sw = nullptr;
    if (slab_mode && rows_f32 > 0 && D.has_sw && post_fuse_on()) {
      WgradJobs f32 = D.wg_f32;
      int rpw = rpw_f32;
      const int n_late = late.n;
      PCA_TRY(wgrad128_place(f32, rpw, &sl));
      const int n_f32 = late.n - n_late;
      late.n = n_late;
      const size_t used_jobs = used;
      used += (sl.used + 255) & ~(size_t)255;
      sw = take_small(n_f32);
      used = used_jobs;
    }
    PCA_TRY(wgrad128_launch(D.wg_f32, false, false, rpw_f32, st, &sl, sw));
    used += (sl.used + 255) & ~(size_t)255;
    if (sw != nullptr) used += ((size_t)cdiv(sw->M, sw->rows_per_wg) * (128 * sw->dq + 128) * 4 + 255) & ~(size_t)255;
    D.wg_f32.n = 0;
    D.sums.n = 0;
  }
  if (D.wg256_n > 0) PCA_TRY(wgrad256_flush_deferred(D, st));
  PCA_TRY(slab_sum_jobs(D.sums, st));        // (nobody carried them)
  D.sums.n = 0;
  for (int i = 0; i < D.late.n; ++i) {
    PCA_REQUIRE(late.n < 40, "bwd_defer_flush: slab-sum table full");
    late.j[late.n++] = D.late.j[i];
  }
  D.late.n = 0;
  if (slab_mode && D.has_sw) {     // layer-1 fc_v gradient (rider of k_terminal1): slabs as well
    const int nwg = (int)cdiv(D.sw.M, D.sw.rows_per_wg), stride = 128 * D.sw.dq + 128;
    if ((128 * D.sw.dq) % 4 == 0 && used + (size_t)nwg * stride * 4 <= D.slab_cap)
      D.sw.slab = D.slab_ws + used / sizeof(float);
  }
  PCA_TRY(terminal_launch(D, st, &late));
  D.posts.n = 0;
  D.has_cls = D.has_sw = 0;
  D.ride_done = 0;
  D.ride_used = 0;
  D.ride_late.n = 0;
  return PCA_OK;
}

}  // namespace pca
