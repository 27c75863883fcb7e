// The d = 128 weight-gradient engine (the peer of wgrad64.hip / wgrad256.hip): job tables in bwd_defer.hpp.
//
//   k_wgrad128     dW[128 x 128] += G^T.A over a row range (G = dZ|dQp|dKp.., A = O|X|H..), several jobs per
//                  launch: both operands come from row-major [point][feature] LDS images through
//                  ds_read_tr16_b64 (hardware transpose); the result leaves as a per-workgroup slab summed in
//                  a fixed order afterwards, or as fp32 atomics; column sums of G (bias gradients) ride along,
//                  and so do slab sums that are due now (rider rows).
//   k_wgrad_small  layer 1: dW[128 x dq] += G^T.X with dq <= 4 (body: terminal_bodies.hpp).
#include "bwd_defer.hpp"
#include "mfma_common.hpp"
#include "terminal_bodies.hpp"
#include "slab_sum_body.hpp"

namespace pca {

namespace {

// ---------------------------------------------------------------------------------
// dW[DG x DA] += G[rows, DG]^T . A[rows, DA]  (+ db[DG] += column sums of G)
// ---------------------------------------------------------------------------------

__device__ __forceinline__ bf16x8 load8(const __bf16* p) {
  return *reinterpret_cast<const bf16x8*>(p);
}
__device__ __forceinline__ bf16x8 load8(const float* p) {
  const float4 lo = reinterpret_cast<const float4*>(p)[0], hi = reinterpret_cast<const float4*>(p)[1];
  bf16x8 v;
  v[0] = (__bf16)lo.x; v[1] = (__bf16)lo.y; v[2] = (__bf16)lo.z; v[3] = (__bf16)lo.w;
  v[4] = (__bf16)hi.x; v[5] = (__bf16)hi.y; v[6] = (__bf16)hi.z; v[7] = (__bf16)hi.w;
  return v;
}

// Software-pipelined: the next 32-row tile is fetched into registers while the current one is
// consumed from LDS; two LDS buffers -> one barrier per tile.  blockIdx.y selects the job.
// NG row groups of four waves each (NG = 2 for the long B*N-row jobs: twice the loads in flight
// per CU; the kernel runs on at most half the CUs because every workgroup costs 16384 atomics):
// group q takes the 32-row tiles q, q + NG, ...; the groups' [128][128] blocks are summed in LDS.
template <typename GT, typename AT, int NG>
__global__ __launch_bounds__(256 * NG) void k_wgrad128(const WgradJobs jobs, int rows_per_wg,
                                                       const SlabSumJobs riders) {
  constexpr int D = 128, NT = 256 * NG;
  // 64 KiB: 2 x 2 staging tiles per group during the loop, the fp32 [128][128] result afterwards
  __shared__ __attribute__((aligned(16))) char lds[4 * 32 * 256 * 2];
  if ((int)blockIdx.y >= jobs.n) {          // rider rows: partial sums that are due now
    slab_sum_body(riders.j[blockIdx.y - jobs.n], blockIdx.x, threadIdx.x,
                  reinterpret_cast<float4*>(lds));
    return;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3, grp = tid >> 8;
  const int gtid = tid & 255;
  char (*sG)[32 * 256] = reinterpret_cast<char (*)[32 * 256]>(lds + grp * (4 * 32 * 256));
  char (*sA)[32 * 256] = reinterpret_cast<char (*)[32 * 256]>(lds + grp * (4 * 32 * 256) + 2 * 32 * 256);
  const WgradJob job = jobs.j[blockIdx.y];
  const GT* __restrict__ G = reinterpret_cast<const GT*>(job.G);
  const AT* __restrict__ A = reinterpret_cast<const AT*>(job.A);
  const int64_t M = job.M;
  const int r = lane & 15, g = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  if (r0 >= M) return;
  const int64_t r1 = (r0 + rows_per_wg < M) ? r0 + rows_per_wg : M;
  // wave w owns the 64 x 64 output block (G features 64*(w>>1).., A features 64*(w&1)..):
  // 4 + 4 transposed fragments feed 16 MFMAs per 32-row tile
  const int gt0 = 4 * (wave >> 1), at0 = 4 * (wave & 1);
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // column sums of G, columns 8*(tid&15)..

  bf16x8 vg[2], va[2];
  uint32_t mk[2][2] = {{~0u, ~0u}, {~0u, ~0u}};       // ReLU mask words of the fetched chunks (job.mask)
  auto fetch = [&](int64_t base) {          // rows at and beyond r1 read as zeros
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int c = gtid + e * 256;
      const int row = c >> 4, ch = c & 15;
      if (base + row < r1) {          // (guarded on purpose: the unconditional form measured +18 %)
        vg[e] = load8(G + (base + row) * D + ch * 8);
        va[e] = load8(A + (base + row) * D + ch * 8);
        if (job.mask != nullptr) {
          // features 8 ch .. 8 ch + 7 of row R: two nibbles (bit 4 t + e of lane (r, g) <-> feature
          // 16 t + 4 g + e, t = ch / 2) of the words of lanes g0 = 2 (ch & 1) and g0 + 1.  Only
          // requested here; applied when the tile goes to LDS (the loads stay in flight meanwhile)
          const int64_t R = base + row;
          const uint32_t* mw = job.mask + (R >> 4) * 64 + (R & 15) + 32 * (ch & 1);
          mk[e][0] = mw[0];
          mk[e][1] = mw[16];
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) { vg[e][k] = (__bf16)0.f; va[e][k] = (__bf16)0.f; }
      }
    }
  };
  fetch(r0 + 32 * grp);
  int buf = 0;
  // uniform trip count for all groups (a group whose tile lies beyond r1 multiplies zeros)
  for (int64_t base0 = r0; base0 < r1; base0 += 32 * NG, buf ^= 1) {
    const int64_t base = base0 + 32 * grp;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int c = gtid + e * 256;
      const int row = c >> 4, ch = c & 15;
      if (job.mask != nullptr) {
        const uint32_t n0 = mk[e][0] >> (4 * (ch >> 1)), n1 = mk[e][1] >> (4 * (ch >> 1));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!((n0 >> k) & 1u)) vg[e][k] = (__bf16)0.f;
          if (!((n1 >> k) & 1u)) vg[e][4 + k] = (__bf16)0.f;
        }
      }
      *reinterpret_cast<bf16x8*>(sG[buf] + tr_off(row, ch)) = vg[e];
      *reinterpret_cast<bf16x8*>(sA[buf] + tr_off(row, ch)) = va[e];
      if (job.db != nullptr) {
#pragma unroll
        for (int k = 0; k < 8; ++k) bs[k] += (float)vg[e][k];
      }
    }
    __syncthreads();
    if (base0 + 32 * NG < r1) fetch(base + 32 * NG);
    bf16x8 ga[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ga[i] = tr_frag(sG[buf], gt0 + i, lane);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const bf16x8 ab = tr_frag(sA[buf], at0 + t, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][t] = mfma32(ga[i], ab, acc[i][t]);
    }
  }
  // The atomics cost per cache-line transaction, not per lane: stage the [128][128] block in
  // LDS and add it with fully coalesced instructions (64 consecutive floats per wave) instead
  // of 16-float row fragments straight from the accumulator layout.
  __syncthreads();
  float* res = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int q = NG - 1; q >= 0; --q) {       // last group stores, the others add on top
    if (grp == q) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int grow = 16 * (gt0 + i) + 4 * g + e;
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            float* dst = &res[grow * D + 16 * (at0 + t) + r];
            *dst = (q == NG - 1) ? acc[i][t][e] : *dst + acc[i][t][e];
          }
        }
    }
    __syncthreads();
  }
  // slab mode: this workgroup's [rows][128] block (+ its 128 bias sums) as plain stores
  const int n1 = (job.g_hi - job.g_lo) * D;
  float* slab = job.slab == nullptr
                    ? nullptr
                    : job.slab + (int64_t)blockIdx.x * (n1 + (job.db != nullptr ? D : 0));
  if (slab != nullptr)
    for (int i = tid; i < n1; i += NT) slab[i] = res[job.g_lo * D + i];
  else
    for (int i = job.g_lo * D + tid; i < job.g_hi * D; i += NT) atomicAdd(&job.dW[i], res[i]);
  if (job.db != nullptr) {
    // threads with equal (tid & 15) hold partial sums of the same 8 columns
    __syncthreads();
    float* red = reinterpret_cast<float*>(lds);         // [16 NG groups][128 columns]
#pragma unroll
    for (int k = 0; k < 8; ++k) red[(tid >> 4) * D + (tid & 15) * 8 + k] = bs[k];
    __syncthreads();
    if (tid < D) {
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < 16 * NG; ++q) t += red[q * D + tid];
      if (slab != nullptr) slab[n1 + tid] = t;
      else atomicAdd(&job.db[tid], t);
    }
  }
}

// layer 1: dW[D x dq] += dQp^T . X with dq <= 4 (fp32 X), db += colsum(dQp).
// 256 threads = 128 features x 2 row phases; 128 rows per workgroup, loads unrolled.
template <typename GT>
__global__ __launch_bounds__(256) void k_wgrad_small(const GT* __restrict__ G,
                                                     const float* __restrict__ X, int64_t M,
                                                     int dq, int rows_per_wg,
                                                     int64_t x_head_stride,   // A = X + (f/32)*stride
                                                     float* __restrict__ dW,
                                                     float* __restrict__ db) {
  wgrad_small_body<GT>(G, X, M, dq, rows_per_wg, x_head_stride, dW, db, blockIdx.x);
}

}  // namespace

int wgrad128_launch(const WgradJobs& jobs_in, bool g_bf16, bool a_bf16, int rows_per_wg,
                    hipStream_t st, WgradSlabs* sl) {
  WgradJobs jobs = jobs_in;
  int64_t maxM = 0;
  for (int i = 0; i < jobs.n; ++i) maxM = jobs.j[i].M > maxM ? jobs.j[i].M : maxM;
  SlabSumJobs riders{};
  if (sl != nullptr && sl->riders != nullptr) riders = *sl->riders;
  if (maxM == 0 || jobs.n == 0) return slab_sum_jobs(riders, st);
  if (sl != nullptr && sl->ws != nullptr) {
    // one slab per workgroup and job; more rows per workgroup until they fit
    for (;;) {
      size_t need = 0;
      for (int i = 0; i < jobs.n; ++i) {
        const WgradJob& j = jobs.j[i];
        need += (size_t)cdiv(j.M, rows_per_wg) * ((j.g_hi - j.g_lo) * 128 + (j.db ? 128 : 0)) * 4;
      }
      if (need <= sl->cap) break;
      rows_per_wg *= 2;
    }
    float* at = sl->ws;
    for (int i = 0; i < jobs.n; ++i) {
      WgradJob& j = jobs.j[i];
      if (j.M <= 0) continue;
      const int nwg = (int)cdiv(j.M, rows_per_wg), n1 = (j.g_hi - j.g_lo) * 128;
      const int stride = n1 + (j.db ? 128 : 0);
      j.slab = at;
      PCA_REQUIRE(sl->sums_out->n + 2 <= 40, "wgrad128: slab-sum table full");
      sl->sums_out->j[sl->sums_out->n++] = SlabSumJob{at, j.dW + (int64_t)j.g_lo * 128, nwg, n1, 1, stride};
      if (j.db) sl->sums_out->j[sl->sums_out->n++] = SlabSumJob{at + n1, j.db, nwg, 128, 1, stride};
      at += (size_t)nwg * stride;
    }
    sl->used = (size_t)(at - sl->ws) * sizeof(float);
  }
  unsigned gx = (unsigned)cdiv(maxM, rows_per_wg);
  for (int i = 0; i < riders.n; ++i) {
    PCA_REQUIRE(slab_sum_job_ok(riders.j[i]), "wgrad128: rider alignment");
    const unsigned need = (unsigned)cdiv(riders.j[i].n, 256);
    gx = need > gx ? need : gx;
  }
  const dim3 grid(gx, (unsigned)(jobs.n + riders.n));
  // two row groups per workgroup when every workgroup has at least four tiles to share
  const bool two = rows_per_wg >= 128;
  if (g_bf16 && a_bf16) {
    if (two) hipLaunchKernelGGL((k_wgrad128<__bf16, __bf16, 2>), grid, dim3(512), 0, st, jobs, rows_per_wg, riders);
    else hipLaunchKernelGGL((k_wgrad128<__bf16, __bf16, 1>), grid, dim3(256), 0, st, jobs, rows_per_wg, riders);
  } else if (g_bf16) {
    if (two) hipLaunchKernelGGL((k_wgrad128<__bf16, float, 2>), grid, dim3(512), 0, st, jobs, rows_per_wg, riders);
    else hipLaunchKernelGGL((k_wgrad128<__bf16, float, 1>), grid, dim3(256), 0, st, jobs, rows_per_wg, riders);
  } else if (!a_bf16) {
    if (two) hipLaunchKernelGGL((k_wgrad128<float, float, 2>), grid, dim3(512), 0, st, jobs, rows_per_wg, riders);
    else hipLaunchKernelGGL((k_wgrad128<float, float, 1>), grid, dim3(256), 0, st, jobs, rows_per_wg, riders);
  } else {
    set_error("wgrad128: fp32 G with bf16 A is not instantiated");
    return PCA_EUNSUPPORTED;
  }
  return check_launch("k_wgrad128");
}

int wgrad128_defer(BwdDefer* defer, const WgradJobs& jobs, bool bf16, int rows_per_wg,
                   hipStream_t st) {
  if (defer == nullptr) return wgrad128_launch(jobs, bf16, bf16, rows_per_wg, st);
  WgradJobs& L = bf16 ? defer->wg_bf16 : defer->wg_f32;
  if (L.n + jobs.n > 16) {                 // table full: run what has been collected
    PCA_TRY(wgrad128_launch(L, bf16, bf16, bf16 ? 512 : 64, st));
    L.n = 0;
  }
  for (int i = 0; i < jobs.n; ++i) L.j[L.n++] = jobs.j[i];
  return PCA_OK;
}

int wgrad_small_f32_launch(const float* G, const float* X, int64_t M, int dq,
                           int64_t x_head_stride, float* dW, float* db, hipStream_t st,
                           BwdDefer* defer) {
  if (defer != nullptr && !defer->has_sw) {
    defer->sw = SmallWgradArgs{G, X, M, dq, 64, x_head_stride, dW, db, nullptr};
    defer->has_sw = 1;
    return PCA_OK;
  }
  hipLaunchKernelGGL((k_wgrad_small<float>), dim3((unsigned)cdiv(M, 64)), dim3(256), 0, st, G, X, M,
                     dq, 64, x_head_stride, dW, db);
  return check_launch("k_wgrad_small<float>");
}

// the same with bf16 G over one input (no head stride), 128 rows per workgroup: never deferred
int wgrad_small_bf16_launch(const __bf16* G, const float* X, int64_t M, int dq, float* dW, float* db,
                            hipStream_t st) {
  hipLaunchKernelGGL((k_wgrad_small<__bf16>), dim3((unsigned)cdiv(M, 128)), dim3(256), 0, st,
                     G, X, M, dq, 128, (int64_t)0, dW, db);
  return check_launch("k_wgrad_small");
}

}  // namespace pca
