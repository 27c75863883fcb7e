// The small kernels of the d = 256 step (map: d256.hpp): fp32 <-> bf16 conversion, the layer-1
// weight gradient (inputs of dq <= 4 columns) and the per-set epilogues of the few-queries block.
#include "d256.hpp"
#include "mfma_common.hpp"

#include <math.h>

namespace pca {

namespace {

__global__ __launch_bounds__(256) void k_cvt_f32_bf16(const float* __restrict__ s,
                                                      __bf16* __restrict__ d, int64_t n4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 v = reinterpret_cast<const float4*>(s)[i];
  reinterpret_cast<bf16x4*>(d)[i] = bf16x4{(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
}
__global__ __launch_bounds__(256) void k_cvt_bf16_f32(const __bf16* __restrict__ s,
                                                      float* __restrict__ d, int64_t n4,
                                                      int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const bf16x4 v = reinterpret_cast<const bf16x4*>(s)[i];
  float4 o = float4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
  if (accumulate) {
    const float4 p = reinterpret_cast<const float4*>(d)[i];
    o.x += p.x; o.y += p.y; o.z += p.z; o.w += p.w;
  }
  reinterpret_cast<float4*>(d)[i] = o;
}

// dW[256 x dq] += G[M x 256]^T X[M x dq] (dq <= 4, fp32 X), db += colsum(G): layer-1 fc_q.
// HBM-bound read of G: a thread owns 8 features (one 16-byte load per row) of every 8th row of
// the workgroup's range, four rows in flight; the 8 row lanes meet in LDS, then one atomic per
// element per workgroup.
__global__ __launch_bounds__(256) void k_wgrad_small256(const __bf16* __restrict__ G,
                                                        const float* __restrict__ X, int64_t M,
                                                        int dq, int rows_per_wg,
                                                        float* __restrict__ slabs) {
  constexpr int D = 256;
  __shared__ __attribute__((aligned(16))) float red[8][D][5];
  const int fc = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t r1 = r0 + rows_per_wg < M ? r0 + rows_per_wg : M;
  float acc[8][4], bs[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    bs[k] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[k][c] = 0.f;
  }
  // the range's points, [row][4] (zero padded), staged once: fetched per row by every thread
  // they were 12 four-byte loads per 4 rows next to the 4 sixteen-byte loads of G - the kernel
  // was bound by load instructions, not bytes (2.2 TB/s)
  float* sXs = &red[0][0][0];
  for (int i = threadIdx.x; i < rows_per_wg * 4; i += 256) {
    const int64_t rr = r0 + (i >> 2);
    const int c = i & 3;
    const float v = X[(rr < r1 ? rr : r1 - 1) * dq + (c < dq ? c : 0)];
    sXs[i] = (rr < r1 && c < dq) ? v : 0.f;
  }
  __syncthreads();
  // (rows past the end are fetched from the last row and weighted by zero: a load under a
  //  divergent `if` gets its own basic block and its own s_waitcnt vmcnt(0) - four serialised
  //  round trips per iteration instead of four loads in flight)
  for (int64_t row = r0 + rl; row < r1; row += 32) {
    bf16x8 gv[4];
    float xv[4][4], wv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t rr = row + 8 * u;
      const int64_t rc = rr < r1 ? rr : r1 - 1;
      wv[u] = rr < r1 ? 1.f : 0.f;
      gv[u] = *reinterpret_cast<const bf16x8*>(G + rc * D + 8 * fc);
      const float4 x4 = *reinterpret_cast<const float4*>(sXs + (rc - r0) * 4);
      xv[u][0] = x4.x * wv[u]; xv[u][1] = x4.y * wv[u];
      xv[u][2] = x4.z * wv[u]; xv[u][3] = x4.w * wv[u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float g = (float)gv[u][k];
        bs[k] = fmaf(g, wv[u], bs[k]);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[k][c] = fmaf(g, xv[u][c], acc[k][c]);
      }
  }
  __syncthreads();                       // the staged points share their LDS with `red`
#pragma unroll
  for (int k = 0; k < 8; ++k) {
#pragma unroll
    for (int c = 0; c < 4; ++c) red[rl][8 * fc + k][c] = acc[k][c];
    red[rl][8 * fc + k][4] = bs[k];
  }
  __syncthreads();
  const int f = threadIdx.x;
  float t[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 8; ++q)
#pragma unroll
    for (int c = 0; c < 5; ++c) t[c] += red[q][f][c];
  // partial sums leave as a slab [workgroup][256][5]; k_wgrad_small256_sum adds the slabs in a
  // fixed order (1026 workgroups x 1024 fp32 atomics onto the same 1024 addresses measured
  // 30 us of this kernel's 117, and made the result depend on the arrival order)
  float* slab = slabs + (int64_t)blockIdx.x * D * 5;
#pragma unroll
  for (int c = 0; c < 5; ++c) slab[f * 5 + c] = t[c];
}

// out[o] += sum over slabs, o = 5 f + c: c < dq -> dW[f][c], c == 4 -> db[f].  One workgroup per 64
// outputs, 16 slab groups of 64 lanes, eight loads in flight each.
__global__ __launch_bounds__(1024) void k_wgrad_small256_sum(const float* __restrict__ slabs,
                                                            int nslabs, int dq,
                                                            float* __restrict__ dW,
                                                            float* __restrict__ db) {
  constexpr int NO = 256 * 5;
  __shared__ float red[16][64];
  const int sg = threadIdx.x >> 6, c = threadIdx.x & 63, o = blockIdx.x * 64 + c;
  const float* s = slabs + o;
  float t = 0.f;
  int w = sg;
  for (; w + 112 < nslabs; w += 128) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = s[(int64_t)(w + 16 * u) * NO];
#pragma unroll
    for (int u = 0; u < 8; ++u) t += v[u];
  }
  for (; w < nslabs; w += 16) t += s[(int64_t)w * NO];
  red[sg][c] = t;
  __syncthreads();
  if (sg == 0) {
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) v += red[q][c];
    const int f = o / 5, k = o - 5 * f;
    if (k < dq) dW[f * dq + k] += v;
    else if (k == 4 && db != nullptr) db[f] += v;
  }
}

// ---- per-set epilogue pieces of the few-queries block whose keys have dk <= 4 columns --------
// O[b][q][f] = Qp[q][f] + bv[f] + sum_c T[b][j m + q][c] Wv[f][c]      (j = head of f)
__global__ __launch_bounds__(256) void k_epi_small_fwd(const float* __restrict__ T,
                                                       const float* __restrict__ Qp,
                                                       const float* __restrict__ Wv,
                                                       const float* __restrict__ bv, int B, int m,
                                                       int D, int dk, float* __restrict__ O) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * m * D) return;
  const int f = (int)(i % D), q = (int)((i / D) % m);
  const int64_t b = i / ((int64_t)D * m);
  const int j = f / 32, R = (D / 32) * m;
  float acc = Qp[(int64_t)q * D + f] + bv[f];
  for (int c = 0; c < dk; ++c) acc = fmaf(T[(b * R + j * m + q) * dk + c], Wv[f * dk + c], acc);
  O[i] = acc;
}
// the same for dk = 256 (PMA): one wave per output, lanes over the contraction - a thread per
// output walks Wv[f][:] with a 1 KiB stride between neighbouring lanes (46 us for 32 K outputs)
__global__ __launch_bounds__(256) void k_epi_wide_fwd(const float* __restrict__ T,
                                                      const float* __restrict__ Qp,
                                                      const float* __restrict__ Wv,
                                                      const float* __restrict__ bv, int B, int m,
                                                      float* __restrict__ O) {
  constexpr int D = 256, DKW = 256, PER = 8;             // outputs per wave
  const int lane = threadIdx.x & 63;
  const int64_t w = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * PER;
  const int R = (D / 32) * m;
  float4 tv[PER], wv[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int64_t i = w + u < (int64_t)B * m * D ? w + u : (int64_t)B * m * D - 1;
    const int f = (int)(i % D), q = (int)((i / D) % m);
    const int64_t b = i / ((int64_t)D * m);
    tv[u] = *reinterpret_cast<const float4*>(T + (b * R + (f / 32) * m + q) * DKW + 4 * lane);
    wv[u] = *reinterpret_cast<const float4*>(Wv + (int64_t)f * DKW + 4 * lane);
  }
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    float acc = tv[u].x * wv[u].x + tv[u].y * wv[u].y + tv[u].z * wv[u].z + tv[u].w * wv[u].w;
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) acc += __shfl_xor(acc, sh);
    const int64_t i = w + u;
    if (lane == 0 && i < (int64_t)B * m * D) {
      const int f = (int)(i % D), q = (int)((i / D) % m);
      O[i] = acc + Qp[(int64_t)q * D + f] + bv[f];
    }
  }
}
// dT[b][r][c] = sum_{f in head j} dO[b][q][f] Wv[f][c] ; Delta[b][r] = sum_c dT T   (r = j m + q)
__global__ __launch_bounds__(256) void k_epi_small_bwd(const float* __restrict__ dO,
                                                       const float* __restrict__ T,
                                                       const float* __restrict__ Wv, int B, int m,
                                                       int D, int dk, float* __restrict__ dT,
                                                       float* __restrict__ Delta) {
  const int R = (D / 32) * m;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * R) return;
  const int rr = (int)(i % R), j = rr / m, q = rr - j * m;
  const int64_t b = i / R;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int f = 32 * j; f < 32 * j + 32; ++f) {
    const float g = dO[(b * m + q) * D + f];
    for (int c = 0; c < dk; ++c) acc[c] = fmaf(g, Wv[f * dk + c], acc[c]);
  }
  float del = 0.f;
  for (int c = 0; c < dk; ++c) {
    dT[i * dk + c] = acc[c];
    del = fmaf(acc[c], T[i * dk + c], del);
  }
  Delta[i] = del;
}
// dWv[f][c] += sum_{b,q} dO[b][q][f] T[b][j(f) m + q][c] ; dbv[f] += sum_{b,q} dO[b][q][f]
__global__ __launch_bounds__(256) void k_epi_small_wv(const float* __restrict__ dO,
                                                      const float* __restrict__ T, int B, int m,
                                                      int dk, int rows_per_wg,
                                                      float* __restrict__ slabs) {
  constexpr int D = 256;
  const int f = threadIdx.x, j = f / 32, R = (D / 32) * m;
  const int64_t M = (int64_t)B * m;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t r1 = r0 + rows_per_wg < M ? r0 + rows_per_wg : M;
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, bs = 0.f;
  for (int64_t row0 = r0; row0 < r1; row0 += 8) {           // 8 rows in flight
    float gv[8], tv[8][4];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t row = row0 + u < r1 ? row0 + u : r1 - 1;
      const int64_t b = row / m;
      const int q = (int)(row - b * m);
      gv[u] = row0 + u < r1 ? dO[row * D + f] : 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) tv[u][c] = c < dk ? T[(b * R + j * m + q) * dk + c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      bs += gv[u];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = fmaf(gv[u], tv[u][c], acc[c]);
    }
  }
  // (no atomics: a slab [workgroup][256][5] in the format of k_wgrad_small256, summed in order)
  float* slab = slabs + (int64_t)blockIdx.x * D * 5;
#pragma unroll
  for (int c = 0; c < 4; ++c) slab[f * 5 + c] = acc[c];
  slab[f * 5 + 4] = bs;
}

}  // namespace

// ---- launchers (declared in d256.hpp) ------------------------------------------------
int cvt_f32_bf16(const float* s, __bf16* d, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_cvt_f32_bf16, dim3((unsigned)cdiv(n / 4, 256)), dim3(256), 0, st, s, d,
                     n / 4);
  return check_launch("k_cvt_f32_bf16");
}
int cvt_bf16_f32(const __bf16* s, float* d, int64_t n, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(k_cvt_bf16_f32, dim3((unsigned)cdiv(n / 4, 256)), dim3(256), 0, st, s, d,
                     n / 4, accumulate);
  return check_launch("k_cvt_bf16_f32");
}

size_t wgrad_small256_ws_bytes(int64_t M) {
  return align256((size_t)cdiv(M, M >= 65536 ? 512 : 128) * 256 * 5 * sizeof(float));
}
int wgrad_small256(const __bf16* G, const float* X, int64_t M, int dq, float* dW, float* db,
                   void* ws, hipStream_t st) {
  const int rpw = M >= 65536 ? 512 : 128;
  const int nwg = (int)cdiv(M, rpw);
  float* slabs = reinterpret_cast<float*>(ws);
  hipLaunchKernelGGL(k_wgrad_small256, dim3((unsigned)nwg), dim3(256), 0, st, G, X, M, dq, rpw,
                     slabs);
  PCA_TRY(check_launch("k_wgrad_small256"));
  hipLaunchKernelGGL(k_wgrad_small256_sum, dim3(256 * 5 / 64), dim3(1024), 0, st, slabs, nwg, dq, dW,
                     db);
  return check_launch("k_wgrad_small256_sum");
}
int epi_small_fwd256(const float* T, const float* Qp, const float* Wv, const float* bv, int B, int m,
                     int dk, float* O, hipStream_t st) {
  if (dk == 256) {
    hipLaunchKernelGGL(k_epi_wide_fwd, dim3((unsigned)cdiv((int64_t)B * m * 256, 32)), dim3(256), 0,
                       st, T, Qp, Wv, bv, B, m, O);
    return check_launch("k_epi_wide_fwd");
  }
  hipLaunchKernelGGL(k_epi_small_fwd, dim3((unsigned)cdiv((int64_t)B * m * 256, 256)), dim3(256), 0,
                     st, T, Qp, Wv, bv, B, m, 256, dk, O);
  return check_launch("k_epi_small_fwd");
}
size_t epi_small_bwd256_ws_bytes(int B, int m) {
  return align256((size_t)cdiv((int64_t)B * m, 16) * 256 * 5 * sizeof(float));
}
int epi_small_bwd256(const float* dO, const float* T, const float* Wv, int B, int m, int dk,
                     float* dT, float* Delta, float* dWv, float* dbv, void* ws, hipStream_t st) {
  hipLaunchKernelGGL(k_epi_small_bwd, dim3((unsigned)cdiv((int64_t)B * 8 * m, 256)), dim3(256), 0,
                     st, dO, T, Wv, B, m, 256, dk, dT, Delta);
  PCA_TRY(check_launch("k_epi_small_bwd"));
  const int nwg = (int)cdiv((int64_t)B * m, 16);
  float* slabs = reinterpret_cast<float*>(ws);
  hipLaunchKernelGGL(k_epi_small_wv, dim3((unsigned)nwg), dim3(256), 0, st, dO, T, B, m, dk, 16, slabs);
  PCA_TRY(check_launch("k_epi_small_wv"));
  hipLaunchKernelGGL(k_wgrad_small256_sum, dim3(256 * 5 / 64), dim3(1024), 0, st, slabs, nwg, dk, dWv,
                     dbv);
  return check_launch("k_wgrad_small256_sum");
}

}  // namespace pca
