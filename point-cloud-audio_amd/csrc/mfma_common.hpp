// Shared device helpers of the fused bf16 MFMA kernels (gfx950).
//
// Layout convention of the "transposed chain" (verified by scripts/probe/mfma_probe.hip):
// every intermediate lives in accumulator tiles T[t][nb] (f32x4) that hold a 16x16 block of
// X^T: row = feature 16t + 4g + e (e = register index), column = point 16nb + (lane & 15),
// g = lane >> 4.  With v_mfma_f32_16x16x32_bf16 (A[row = lane&15][k = 8g+j],
// B[k = 8g+j][col = lane&15], D[row = 4g+e][col = lane&15]) two such tiles (features
// 32s .. 32s+31) convert in registers into the B operand of the NEXT product that sums over
// features; the k-slot (g, j) then means feature 32s + perm32(8g + j), so the A operand
// (always a weight-like matrix) is stored with its K axis permuted the same way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pca {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef float f32x2 __attribute__((ext_vector_type(2)));   // packed-fp32 operand pair (v_pk_*_f32)

// position p = 8g + j inside a 32-wide K block -> index of the element that k-slot (g, j)
// carries when the B operand is built from two accumulator tiles
__host__ __device__ __forceinline__ int perm32(int p) {
  const int g = p >> 3, j = p & 7;
  return j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4);
}

__device__ __forceinline__ f32x4 mfma32(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(bf16x4 a, bf16x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a),
                                                   __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
}

__device__ __forceinline__ bf16x8 pack8(f32x4 lo, f32x4 hi) {
  bf16x8 r;
  r[0] = (__bf16)lo[0]; r[1] = (__bf16)lo[1]; r[2] = (__bf16)lo[2]; r[3] = (__bf16)lo[3];
  r[4] = (__bf16)hi[0]; r[5] = (__bf16)hi[1]; r[6] = (__bf16)hi[2]; r[7] = (__bf16)hi[3];
  return r;
}
__device__ __forceinline__ bf16x4 pack4(f32x4 v) {
  bf16x4 r;
  r[0] = (__bf16)v[0]; r[1] = (__bf16)v[1]; r[2] = (__bf16)v[2]; r[3] = (__bf16)v[3];
  return r;
}

__device__ __forceinline__ bf16x8 cat8(bf16x4 lo, bf16x4 hi) {
  bf16x8 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) { r[e] = lo[e]; r[4 + e] = hi[e]; }
  return r;
}
__device__ __forceinline__ f32x4 tof(bf16x4 v) {
  return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
// 8 consecutive bf16 of global memory (16-byte aligned) as one operand
__device__ __forceinline__ bf16x8 gload8(const __bf16* p) {
  return *reinterpret_cast<const bf16x8*>(p);
}
// the same from 8 consecutive fp32 (32-byte aligned), rounded to bf16 here
__device__ __forceinline__ bf16x8 gload8(const float* p) {
  const float4 lo = reinterpret_cast<const float4*>(p)[0], hi = reinterpret_cast<const float4*>(p)[1];
  bf16x8 v;
  v[0] = (__bf16)lo.x; v[1] = (__bf16)lo.y; v[2] = (__bf16)lo.z; v[3] = (__bf16)lo.w;
  v[4] = (__bf16)hi.x; v[5] = (__bf16)hi.y; v[6] = (__bf16)hi.z; v[7] = (__bf16)hi.w;
  return v;
}

// ---- LDS pointers (address space 3) and the transposing LDS read ------------------------------------
typedef __attribute__((address_space(3))) void lds_void_t;       // destination of an LDS-DMA
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;       // operand of ds_read_tr16_b64

// One 16-byte LDS-DMA: every lane's 16 bytes at `src` go to lds_dst + 16 * lane (lds_dst wave-uniform).
// m0 carries the LDS address and is restored: the compiler keeps values of its own there.  The s_nop
// covers the hazard between the write of m0 and the instruction that reads it.
__device__ __forceinline__ void lds_dma16(const void* src, char* lds_dst) {
  const unsigned ldst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_void_t*)lds_dst);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
               "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(ldst) : "memory");
}
// workgroup barrier that orders LDS traffic only: __syncthreads() would also wait for every outstanding
// global store and LDS-DMA (vmcnt(0)), i.e. expose a full memory round trip; the caller counts vmcnt itself
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// two transposing reads (ds_read_tr16_b64) joined into one MFMA operand: the k-slots of p0, then of p1
__device__ __forceinline__ bf16x8 tr_read2(const char* p0, const char* p1) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p1);
  const bf16x4 l4 = __builtin_bit_cast(bf16x4, lo), h4 = __builtin_bit_cast(bf16x4, hi);
  bf16x8 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) { r[e] = l4[e]; r[4 + e] = h4[e]; }
  return r;
}

// LDS image of a 32-row tile with 256-byte rows; 16-byte chunk ch of row `row` sits at
// (cdna_hip_programming.md T10, image (b)): serves the transposed reads conflict-free
__device__ __forceinline__ int tr_off(int row, int ch) {
  return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}
// A/B fragment with k = the 32 points of the tile (k-slot (g, j): j<4 -> point 4g+j,
// else 16+4g+j-4, i.e. perm32(8g + j)) for the 16 features of tile t of a tr_off image
__device__ __forceinline__ bf16x8 tr_frag(const char* img, int t, int lane) {
  const int g = lane >> 4, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
  const int a0 = tr_off(4 * g + q, 2 * t + (p >> 1)) + 8 * (p & 1);
  const int a1 = tr_off(16 + 4 * g + q, 2 * t + (p >> 1)) + 8 * (p & 1);
  // (the tail of tr_read2 written out: through the wrapper hipcc schedules k_mab0_attn_h4 differently)
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + a0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + a1));
  const bf16x4 l4 = __builtin_bit_cast(bf16x4, lo), h4 = __builtin_bit_cast(bf16x4, hi);
  bf16x8 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) { r[e] = l4[e]; r[4 + e] = h4[e]; }
  return r;
}
// the same fragment from a small row-major bf16 image with `rb` bytes per row (no swizzle), for the
// 16 columns from col0
__device__ __forceinline__ bf16x8 tr_frag_small(const char* img, int rb, int col0, int lane) {
  const int g = lane >> 4, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
  const int a0 = (4 * g + q) * rb + (col0 + 4 * p) * 2;
  const int a1 = (16 + 4 * g + q) * rb + (col0 + 4 * p) * 2;
  return tr_read2(img + a0, img + a1);
}

// [32 rows][256] bf16 tile as two [32][128] halves, each a tr_off image (conflict-free ds_read_tr16_b64)
__device__ __forceinline__ int tr_off256(int row, int ch) {
  return (ch >> 4) * (32 * 256) + 256 * row +
         16 * ((ch & 15) ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}
__device__ __forceinline__ bf16x8 tr_frag256(const char* img, int t, int lane) {
  const int g = lane >> 4, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
  const int a0 = tr_off256(4 * g + q, 2 * t + (p >> 1)) + 8 * (p & 1);
  const int a1 = tr_off256(16 + 4 * g + q, 2 * t + (p >> 1)) + 8 * (p & 1);
  return tr_read2(img + a0, img + a1);
}

// ---- fp8 (OCP e4m3) operands: same 16x16x32 shape and (g, j) k-slot structure as bf16, 8 values
// per lane in two VGPRs (element j = byte j) --------------------------------------------------
typedef long f8x8;
__device__ __forceinline__ f32x4 mfma32_f8(f8x8 a, f8x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float clamp_f8(float x) { return fminf(fmaxf(x, -448.f), 448.f); }
__device__ __forceinline__ uint32_t cvt4_f8(float a, float b, float c, float d) {
  int p = __builtin_amdgcn_cvt_pk_fp8_f32(clamp_f8(a), clamp_f8(b), 0, false);
  p = __builtin_amdgcn_cvt_pk_fp8_f32(clamp_f8(c), clamp_f8(d), p, true);
  return (uint32_t)p;
}
__device__ __forceinline__ f8x8 pack8_f8(f32x4 lo, f32x4 hi) {
  const uint64_t l = cvt4_f8(lo[0], lo[1], lo[2], lo[3]), h = cvt4_f8(hi[0], hi[1], hi[2], hi[3]);
  return (f8x8)(l | (h << 32));
}
__device__ __forceinline__ f8x8 bf_to_f8(bf16x8 v) {
  const uint64_t l = cvt4_f8((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
  const uint64_t h = cvt4_f8((float)v[4], (float)v[5], (float)v[6], (float)v[7]);
  return (f8x8)(l | (h << 32));
}
// byte offset of 8-byte slot `slot` (8 fp8) of row `row` in a [.][D] fp8 LDS image: the XOR makes
// the 32 (row, g) pairs of a half-wave's ds_read_b64 hit 32 different slots
template <int D>
__device__ __forceinline__ int f8off(int row, int slot) {
  return row * D + ((slot ^ (D == 256 ? ((2 * row) & 31) : (row & 15))) << 3);
}

// byte offset of 16-byte chunk c16 of row `row` in a row-major bf16 LDS image with
// `row_bytes` per row, XOR-swizzled so that 16 lanes reading the same chunk of 16 different
// rows hit 16 different bank groups (cdna_hip_programming.md T2)
__device__ __forceinline__ int swz(int row, int c16, int row_bytes) {
  return row * row_bytes + (((c16 & ~15) | ((c16 ^ row) & 15)) << 4);
}

// Reductions over the 4 lane groups g (lanes l, l^16, l^32, l^48), result in every lane.
// gfx950's v_permlane32_swap / v_permlane16_swap exchange half-waves / odd-even rows in the
// VALU (no trip through the LDS crossbar as ds_bpermute / __shfl_xor would take):
//   permlane32_swap(v, v) -> ([lo, lo], [hi, hi]);  permlane16_swap(v, v) -> ([r0,r0,r2,r2],
//   [r1,r1,r3,r3]); combining the two results of each is the xor-32 / xor-16 butterfly step.
// max as ONE instruction (v_med3_f32 with +inf); fmaxf costs a canonicalising v_max x, x in front of every
// operand the compiler cannot prove quiet.  For operands that are never NaN (scores of finite inputs).
__device__ __forceinline__ float max_nn(float x, float y) { return __builtin_amdgcn_fmed3f(x, y, INFINITY); }
__device__ __forceinline__ float wave16_max_nn(float v) {
  auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = max_nn(__uint_as_float(a[0]), __uint_as_float(a[1]));
  auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return max_nn(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float wave16_max(float v) {
  auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float wave16_sum(float v) {
  auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
// ---- bf16 tile operands in 16-byte pieces ----
// In the accumulator's shape lane (r, g) holds features 16t + 4g .. + 3 of point r: 8 bytes.  Tiles 2s and 2s + 1 of a
// point are 64 contiguous bytes, and lane group g moves the 16-byte chunk chunk_of(g) of them: v_permlane16_swap
// exchanges the odd 16-lane rows of its first operand with the even rows of its second, so with the first tile's dword
// in front and the second tile's behind, groups 0 and 2 receive their odd neighbour's part of the first tile (chunks
// 0, 1) and groups 1 and 3 their even neighbour's part of the second (chunks 2, 3).  The exchange is its own inverse:
// a chunk as loaded goes back into the two tiles' fragments by the same two swaps.  The lanes that exchange hold the
// same point, so a row's `live` guard holds for both.
__device__ __forceinline__ int chunk_of(int g) { return ((g & 1) << 1) | (g >> 1); }
__device__ __forceinline__ u32x4 frag_swap(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
  const auto x = __builtin_amdgcn_permlane16_swap(a0, b0, false, false);
  const auto y = __builtin_amdgcn_permlane16_swap(a1, b1, false, false);
  return u32x4{x[0], y[0], x[1], y[1]};
}
// this lane's four features of tiles 2s (a) and 2s + 1 (b) -> features 32s + 8 chunk_of(g) .. + 7
__device__ __forceinline__ u32x4 to_chunk(bf16x4 a, bf16x4 b) {
  const uint2 ua = __builtin_bit_cast(uint2, a), ub = __builtin_bit_cast(uint2, b);
  return frag_swap(ua.x, ua.y, ub.x, ub.y);
}
__device__ __forceinline__ void from_chunk(u32x4 w, bf16x4& a, bf16x4& b) {
  const u32x4 v = frag_swap(w[0], w[1], w[2], w[3]);
  a = __builtin_bit_cast(bf16x4, uint2{v[0], v[1]});
  b = __builtin_bit_cast(bf16x4, uint2{v[2], v[3]});
}

// 8 consecutive features of row `n` of a [rows][DK] activation tensor as bf16 (ABF: stored bf16,
// else fp32 rounded here); rows at or past `n_hi` read row n_hi - 1 and come back as zeros.
// UNCONDITIONAL loads on purpose: a load under a divergent `if` gets its own basic block and an
// s_waitcnt vmcnt(0) of its own, i.e. the 4-8 loads of a tile become as many serial round trips.
template <bool ABF>
__device__ __forceinline__ bf16x8 ld_x8_guard(const void* X, int64_t set_row0, int n, int n_hi,
                                              int DK, int ch) {
  const bool ok = n < n_hi;
  const int64_t row = set_row0 + (ok ? n : n_hi - 1);
  bf16x8 v;
  if (ABF) {
    v = gload8(reinterpret_cast<const __bf16*>(X) + row * DK + ch * 8);
  } else {
    v = gload8(reinterpret_cast<const float*>(X) + row * DK + ch * 8);
  }
  if (!ok) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (__bf16)0.f;
  }
  return v;
}

// The same load WITHOUT the zeroing (ABF only): for a register prefetch the zeroing has to wait until
// the registers are consumed - applied right behind the load it makes hipcc wait for the load there,
// and the tile that was meant to arrive during the current tile's arithmetic is waited for before it.
__device__ __forceinline__ bf16x8 ld_x8_clamped(const void* X, int64_t set_row0, int n, int n_hi,
                                                int DK, int ch) {
  // (an empty range - n_hi == 0, a zero-length set - reads row 0 of the set, never row -1)
  const int last = n_hi > 0 ? n_hi - 1 : 0;
  const int64_t row = set_row0 + (n < n_hi ? n : last);
  return *reinterpret_cast<const bf16x8*>(reinterpret_cast<const __bf16*>(X) + row * DK + ch * 8);
}
__device__ __forceinline__ bf16x8 zero_unless(bool ok, bf16x8 v) {
  if (!ok) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (__bf16)0.f;
  }
  return v;
}

// A chunk of cn <= 1024 points with dk (<= 4) fp32 components each, contiguous in memory, into LDS as
// [pair of points][component][2] (the operand pairs of the packed-fp32 loops of k_mab0_attn_small /
// k_mab0_bwd_small), unused components and the odd point zero - in two halves, so that the loads of
// the NEXT chunk are in flight while the current one is worked on:
//   fetch_points   the raw cn*dk floats into 16 registers per thread (coalesced dwords, all issued
//                  together: one float per loop trip, each waited for on its own, had made the
//                  staging - not the arithmetic - the cost of those kernels)
//   commit_points  registers -> LDS.  Every thread of the 256-thread workgroup must call it (two
//                  barriers inside: the first also ends the previous chunk's reads of sX)
// NT: threads of the workgroup (4096 / NT registers per thread; the same element goes to the same place)
constexpr int PCA_POINT_CHUNK = 1024;
template <int NT = 256>
__device__ __forceinline__ void fetch_points(const float* __restrict__ X, int cn, int dk,
                                             float (&v)[4096 / NT]) {
  const int n = cn * dk;
#pragma unroll
  for (int u = 0; u < 4096 / NT; ++u) {
    const int e = threadIdx.x + NT * u;
    v[u] = X[e < n ? e : n - 1];
  }
}
template <int NT = 256>
__device__ __forceinline__ void commit_points(const float (&v)[4096 / NT], int cn, int dk, float* sX) {
  const int tid = threadIdx.x;
  const int npairs = (cn + 1) >> 1, n = cn * dk;
  __syncthreads();
  if (dk < 4 || (cn & 1))
    for (int i = tid; i < npairs * 8; i += NT) sX[i] = 0.f;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4096 / NT; ++u) {
    const int e = tid + NT * u;
    if (e < n) {
      const int pt = e / dk, c = e - pt * dk;
      sX[(pt >> 1) * 8 + c * 2 + (pt & 1)] = v[u];
    }
  }
  __syncthreads();
}

// ---- the many-queries kernels' point tiling and the layout of their saved ReLU mask -------------------
constexpr int M1_TP = 128;     // points per workgroup tile (4 waves x 32)
constexpr int M1_NB = 2;       // 16-point blocks per wave

// one 32-bit word per lane covers 8 feature tiles (4 bits each)
template <int D>
__host__ __device__ __forceinline__ int64_t mab1_mask_index(int b, int tiles_per_set, int tile,
                                                            int wave, int nb, int w, int lane) {
  const int64_t pb = ((int64_t)b * tiles_per_set + tile) * (M1_TP / 16) + wave * M1_NB + nb;
  return (pb * (D / 128) + w) * 64 + lane;
}

// ---- per-set row GEMM on the VALU --------------------------------------------------------------------
// acc[q] += sum_c sX[q*ldx + c] * WT[c*ldw + f]   for q < MQ : thread-owned output column f,
// activations broadcast from LDS, weights read coalesced (consecutive threads = consecutive f)
template <int MQ>
__device__ __forceinline__ void col_gemm(const float* sX, int ldx, const float* __restrict__ WT,
                                         int ldw, int K, int f, float (&acc)[MQ]) {
  // 16 independent weight loads in flight per thread: these per-set kernels run at one
  // workgroup per set and are otherwise bound by L2 latency, not bandwidth
  int c = 0;
  for (; c + 16 <= K; c += 16) {
    float w[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) w[u] = WT[(int64_t)(c + u) * ldw + f];
#pragma unroll
    for (int u = 0; u < 16; ++u)
#pragma unroll
      for (int q = 0; q < MQ; ++q) acc[q] = fmaf(sX[q * ldx + c + u], w[u], acc[q]);
  }
  for (; c < K; ++c) {
    const float w = WT[(int64_t)c * ldw + f];
#pragma unroll
    for (int q = 0; q < MQ; ++q) acc[q] = fmaf(sX[q * ldx + c], w, acc[q]);
  }
}

}  // namespace pca
