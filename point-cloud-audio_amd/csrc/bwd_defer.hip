// The end of a backward pass: bwd_defer_flush runs the plan (plan_tail, tail_plan.hip) of everything the blocks
// of a step queued in their BwdDefer (bwd_defer.hpp) - the weight-gradient launch (wgrad128.hip: both d = 128
// lists in one; wgrad256.hip) with the due slab sums as riders, then the post stages:
//
//   k_mab0_post1 / k_terminal1   dWk and dQp of the shared queries (k_terminal1: the same plus the classifier's
//                                weight gradient, the layer-1 fc_v gradient and late slab sums as extra rows;
//                                with PCA_POST_FUSE, the default, also what k_mab0_post2 computes, in rows of
//                                workgroups that keep their part of dQp in LDS - no second launch)
//   k_mab0_post2                 dWq, dbq, dI from dQp (+ the sums of the partials k_terminal1 itself wrote)
#include "bwd_defer.hpp"
#include "terminal_bodies.hpp"
#include "slab_sum_body.hpp"

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
// live workgroup reaches the barrier.  Shapes: post_fused_ok (tail_plan.hip; POST_FC, POST_MAXM: bwd_defer.hpp).
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

int mab0_post_launch(const Mab0PostJobs& J, hipStream_t st) {     // (nothing rides: k_mab0_post1, k_mab0_post2)
  BwdDefer D{};
  D.posts = J;
  return bwd_defer_flush(D, st);
}

bool bwd_defer_ride(BwdDefer& D, WgradJobs* jobs, int* rows_per_wg, int* rc) {
  *rc = PCA_OK;
  if (!(D.form.ride && D.slab_ws != nullptr && D.slab_cap > 0) || D.wg_bf16.n == 0 || D.placed.bf16_ran)
    return false;
  TailPlan P;
  *rc = plan_tail(D, &P, true);
  if (*rc != PCA_OK || P.bf16.n == 0) return false;
  *jobs = P.bf16;
  *rows_per_wg = P.rpw_bf16;
  D.placed = P.placed;
  D.placed.bf16_ran = true;
  D.wg_bf16.n = 0;
  return true;
}

// walks the plan: one case per launch, charged to the profiler as before
int bwd_defer_flush(BwdDefer& D, hipStream_t st) {
  TailPlan P;
  PCA_TRY(plan_tail(D, &P));
  const Mab0PostJobs& J = D.posts;
  const SmallWgradArgs* sw = P.fcv == FcvRuns::WgradRows ? &P.small : nullptr;
  const int term_sw = P.fcv == FcvRuns::TerminalRows || P.fcv == FcvRuns::TerminalRowsPost2Sums;
  const double rows = P.rows_bf16, rows_f32 = P.rows_f32;
  const SlabSumJobs* due = &P.step.riders;       // riders of the first weight-gradient launch
  static const char* const name[] = {"k_wgrad128_step", "k_wgrad128", "k_wgrad128", "wgrad256", "k_slab_sum_jobs",
                                     "k_terminal1", "k_mab0_post1", "k_mab0_post2", "k_slab_sum_jobs"};
  for (int i = 0; i < P.nseq; ++i) {
    const TailLaunch& L = P.seq[i];
    const dim3 grid(L.gx, L.gy);
    switch (L.kernel) {
      case TailKernel::WgradStep: {
        ProfScope ps(PCA_K_WGRAD, st, 2.0 * (rows + rows_f32) * 128 * 128,
                     4.0 * rows * 128 + 8.0 * rows_f32 * 128);
        PCA_TRY(wgrad128_launch_step(P.bf16, P.rpw_bf16, P.f32, P.rpw_f32, P.step, st, sw));
        ps.end();
        break;
      }
      case TailKernel::Wgrad128Bf16: {
        ProfScope ps(PCA_K_WGRAD, st, 2.0 * rows * 128 * 128, 4.0 * rows * 128);
        PCA_TRY(wgrad128_launch(P.bf16, true, true, P.rpw_bf16, st, due));
        ps.end();
        due = nullptr;
        break;
      }
      case TailKernel::Wgrad128F32: PCA_TRY(wgrad128_launch(P.f32, false, false, P.rpw_f32, st, due, sw)); break;
      case TailKernel::Wgrad256: PCA_TRY(wgrad256_flush_deferred(D, st)); break;
      case TailKernel::SumsDue: PCA_TRY(slab_sum_jobs(P.step.riders, st)); break;
      case TailKernel::SumsLate2: PCA_TRY(slab_sum_jobs(P.late2, st)); break;
      case TailKernel::Terminal1:
        hipLaunchKernelGGL(k_terminal1, grid, dim3(256), 0, st, J, P.post_fused ? J.n : 0, D.cls,
                           D.has_cls ? 1 : 0, P.small, term_sw, P.placed.late);
        break;
      case TailKernel::Post1: hipLaunchKernelGGL(k_mab0_post1, grid, dim3(256), 0, st, J); break;
      case TailKernel::Post2: hipLaunchKernelGGL(k_mab0_post2, grid, dim3(256), 0, st, J, P.late2); break;
    }
    PCA_TRY(check_launch(name[(int)L.kernel]));
  }
  D.wg_bf16.n = D.wg_f32.n = D.sums.n = D.late.n = D.posts.n = D.has_cls = D.has_sw = 0;
  D.placed = TailPlaced{};
  return PCA_OK;
}

}  // namespace pca
