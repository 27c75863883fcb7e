// Weight and bias gradients of a Linear over a tall activation, deterministic (the self-attention blocks of
// BlockPath::ExactCore, api_mab.hip):
//
//     dW[dout][din] += dY[M][dout]^T X[M][din]      db[dout] += colsum(dY)          (nn.Linear's adjoint)
//
// The chain's k_gemm_bf16 serves this product with split-K over the M rows and float atomics: on average
// 253 us per call (191 - 349) over the two shapes of scripts/sab_bench.py (B N = 65 536 and 32 768 rows,
// d = 128 and 256), and results that vary from call to call.  Here:
//   k_wgrad_rows     a workgroup owns a slab of rows and a 128 x 128 tile of dW.  64-row chunks of dY and X
//                    are read once, coalesced (a thread: one feature, 32 consecutive rows), rounded to bf16 as
//                    k_gemm_bf16 rounds its operands, and written to LDS transposed ([feature][row], 16-byte
//                    pieces), which is the MFMA operand form of both sides (k = row).  Wave w owns dW rows
//                    32 w .. 32 w + 31 of the tile: 2 x 8 accumulator tiles of v_mfma_f32_16x16x32_bf16.  The
//                    column sums of dY are summed in fp32 by the thread that holds the feature.  The partial
//                    tile goes to its own slab: every element written once.
//   k_wgrad_reduce   dW += sum of the slabs, db += sum of the column-sum slabs, in a fixed order (8 threads per
//                    element over contiguous slab ranges, their sums added in range order).
// The result is bitwise reproducible, and does not depend on how the launch is captured or replayed.
#include "blocks.hpp"
#include "mfma_common.hpp"

namespace pca {

namespace {

constexpr int WT = 128;        // dW tile: WT x WT
constexpr int WCH = 64;        // rows per staged chunk
constexpr int WP = WCH + 8;    // pitch (bf16) of the transposed images: rows of 144 bytes, 16-byte aligned

struct WgPlan { int S, rows, to, ti; };
inline WgPlan wg_plan(int64_t M, int dout, int din) {
  WgPlan p;
  p.to = (int)cdiv(dout, WT);
  p.ti = (int)cdiv(din, WT);
  const int64_t want = 256 / (p.to * p.ti) > 0 ? 256 / (p.to * p.ti) : 1;     // one workgroup per CU
  const int64_t chunks = cdiv(M, WCH);
  const int64_t S = want < chunks ? want : chunks;
  p.rows = (int)(cdiv(chunks, S) * WCH);
  p.S = (int)cdiv(M, p.rows);
  return p;
}

struct WgArgs {
  const float *dY, *X;
  float *part, *cpart;         // [S][dout][din], [S][dout]
  int64_t M;
  int dout, din, rows;
};

// chunk rows r0 .. r0 + 63 (those below rend), features f0 .. f0 + 127 (those below w) of A[M][w], transposed
// into T[feature][row]; the thread owns feature f0 + (tid & 127) and rows 32 (tid >> 7) .. + 31.  csum (when
// given) accumulates the thread's fp32 values.
__device__ __forceinline__ void stage_tr(const float* __restrict__ A, int64_t rend, int w, int64_t r0, int f0,
                                         __bf16* __restrict__ T, float* csum) {
  const int tid = threadIdx.x, f = tid & (WT - 1), rg = tid >> 7;
  const bool fok = f0 + f < w;
  const float* p = A + (fok ? f0 + f : 0);
  float v[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    const int64_t row = r0 + 32 * rg + k;
    v[k] = *(p + (row < rend ? row : rend - 1) * w);
  }
#pragma unroll
  for (int k = 0; k < 32; ++k)
    if (!fok || r0 + 32 * rg + k >= rend) v[k] = 0.f;
  if (csum != nullptr) {
    float s = *csum;
#pragma unroll
    for (int k = 0; k < 32; ++k) s += v[k];
    *csum = s;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
    *reinterpret_cast<bf16x8*>(T + f * WP + 32 * rg + 8 * q) =
        pack8(f32x4{v[8 * q], v[8 * q + 1], v[8 * q + 2], v[8 * q + 3]},
              f32x4{v[8 * q + 4], v[8 * q + 5], v[8 * q + 6], v[8 * q + 7]});
}

__global__ __launch_bounds__(256) void k_wgrad_rows(const WgArgs a) {
  __shared__ __attribute__((aligned(16))) __bf16 TY[WT * WP];
  __shared__ __attribute__((aligned(16))) __bf16 TX[WT * WP];
  __shared__ float cs[WT];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 15, g = lane >> 4;
  const int s = blockIdx.x, o0 = blockIdx.y * WT, i0 = blockIdx.z * WT;
  const int64_t rb = (int64_t)s * a.rows;
  const int64_t re = rb + a.rows < a.M ? rb + a.rows : a.M;
  // live 16-wide tiles of this workgroup's dW tile (uniform)
  const int nb = (a.din - i0) >= WT ? 8 : (a.din - i0 + 15) / 16;
  const bool live = o0 + 32 * wv < a.dout;
  const bool want_cs = blockIdx.z == 0;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[2][8];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[u][b] = z4;
  float csum = 0.f;
  for (int64_t r0 = rb; r0 < re; r0 += WCH) {
    __syncthreads();                                   // the previous chunk is consumed
    stage_tr(a.dY, re, a.dout, r0, o0, TY, want_cs ? &csum : nullptr);
    stage_tr(a.X, re, a.din, r0, i0, TX, nullptr);
    __syncthreads();
    if (!live) continue;
#pragma unroll
    for (int ks = 0; ks < WCH / 32; ++ks) {
      bf16x8 ya[2];
#pragma unroll
      for (int u = 0; u < 2; ++u)                      // A [row = dW row o][k = row m]
        ya[u] = *reinterpret_cast<const bf16x8*>(TY + (32 * wv + 16 * u + r) * WP + 32 * ks + 8 * g);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        if (b >= nb) break;
        const bf16x8 xb =                              // B [k = row m][col = dW column i]
            *reinterpret_cast<const bf16x8*>(TX + (16 * b + r) * WP + 32 * ks + 8 * g);
#pragma unroll
        for (int u = 0; u < 2; ++u) acc[u][b] = mfma32(ya[u], xb, acc[u][b]);
      }
    }
  }
  if (live) {
    float* dst = a.part + (int64_t)s * a.dout * a.din;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const int i = i0 + 16 * b + r;
        if (b >= nb || i >= a.din) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int o = o0 + 32 * wv + 16 * u + 4 * g + e;
          if (o < a.dout) dst[(int64_t)o * a.din + i] = acc[u][b][e];
        }
      }
  }
  if (want_cs) {                                       // the two row groups of a feature, in a fixed order
    __syncthreads();
    if (tid >= WT) cs[tid - WT] = csum;
    __syncthreads();
    if (tid < WT && o0 + tid < a.dout) a.cpart[(int64_t)s * a.dout + o0 + tid] = csum + cs[tid];
  }
}

// 32 elements of dW (then of db) per workgroup, 8 threads per element: thread part q sums slabs
// q S / 8 .. (q + 1) S / 8 - 1 in order, then part 0 adds the 8 sums in order and adds them onto the gradient
constexpr int RED_OUT = 32, RED_PARTS = 8;
__global__ __launch_bounds__(256) void k_wgrad_reduce(float* __restrict__ dW, float* __restrict__ db,
                                                      const float* __restrict__ part,
                                                      const float* __restrict__ cpart, int S, int dout, int din) {
  __shared__ float acc[RED_PARTS][RED_OUT];
  const int64_t n = (int64_t)dout * din;
  const int t = threadIdx.x & (RED_OUT - 1), q = threadIdx.x / RED_OUT;
  const int64_t idx = (int64_t)blockIdx.x * RED_OUT + t;
  const int s0 = (int)((int64_t)S * q / RED_PARTS), s1 = (int)((int64_t)S * (q + 1) / RED_PARTS);
  float v = 0.f;
  if (idx < n) {
    for (int s = s0; s < s1; ++s) v += part[(int64_t)s * n + idx];
  } else if (idx < n + dout) {
    for (int s = s0; s < s1; ++s) v += cpart[(int64_t)s * dout + (idx - n)];
  }
  acc[q][t] = v;
  __syncthreads();
  if (q != 0 || idx >= n + dout) return;
  float sum = acc[0][t];
#pragma unroll
  for (int k = 1; k < RED_PARTS; ++k) sum += acc[k][t];
  if (idx < n) dW[idx] += sum;
  else db[idx - n] += sum;
}

}  // namespace

size_t wgrad_rows_ws_elems(int64_t M, int dout, int din) {
  const WgPlan p = wg_plan(M, dout, din);
  return align256((size_t)p.S * dout * din * sizeof(float)) / sizeof(float) +
         align256((size_t)p.S * dout * sizeof(float)) / sizeof(float);
}

int wgrad_rows(const float* dY, const float* X, float* dW, float* db, int64_t M, int din, int dout, float* ws,
               hipStream_t st) {
  PCA_REQUIRE(M > 0 && din > 0 && dout > 0, "wgrad_rows: bad extents");
  const WgPlan p = wg_plan(M, dout, din);
  PCA_REQUIRE(p.S <= 65535 && p.to <= 65535 && p.ti <= 65535, "wgrad_rows: grid too large");
  WgArgs a;
  a.dY = dY; a.X = X; a.M = M; a.dout = dout; a.din = din; a.rows = p.rows;
  a.part = ws;
  a.cpart = ws + align256((size_t)p.S * dout * din * sizeof(float)) / sizeof(float);
  hipLaunchKernelGGL(k_wgrad_rows, dim3(p.S, p.to, p.ti), dim3(256), 0, st, a);
  PCA_TRY(check_launch("k_wgrad_rows"));
  const int64_t n = (int64_t)dout * din + dout;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)cdiv(n, RED_OUT)), dim3(RED_OUT * RED_PARTS), 0, st, dW, db,
                     a.part, a.cpart, p.S, dout, din);
  return check_launch("k_wgrad_reduce");
}

}  // namespace pca
