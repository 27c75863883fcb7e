// The [256 x 256] weight gradients of the d = 256 blocks (map: d256.hpp): dW = G^T A over the B*N
// (or B*m) rows as per-workgroup fp32 slabs - k_wgrad256_dma (operand tiles by LDS-DMA) or k_wgrad256
// (register staged: fp32 operands, PCA_WGRAD256_DMA=0) - and k_wgrad256_sum, which adds the slabs of
// a job into dW / db in a fixed order.  Tile layout: tr_off256 / tr_frag256 (mfma_common.hpp).
#include "d256.hpp"
#include "bwd_defer.hpp"
#include "mfma_common.hpp"
#include "slab_sum_body.hpp"

#include <math.h>

namespace pca {

namespace {

// =====================================================================================
// k_wgrad256: dW[D x D] = G[M x D]^T A[M x D] (+ db = column sums of G), bf16 operands
// =====================================================================================
// One workgroup = one row range of one job; 8 waves, wave w owns the [64 x 128] output block
// (G features 64 (w >> 1) .., A features 128 (w & 1) ..): 4 + 8 transposed fragments feed 32 MFMAs
// per 32-row tile.  The fp32 block leaves as a slab ([nwg][D][D]); k_wgrad256_sum adds the slabs
// of a job into dW in a fixed order (no atomics: the result is reproducible run to run).

// T: element type of G and A in memory (bf16, or fp32 rounded to bf16 while staged: the [B*m]-row
// reductions of the per-set epilogues).  Two tiles are in flight per thread (registers) while a
// third is consumed from LDS: one 32-row tile (32 KiB) ahead per CU was latency-bound at 2.6 TB/s.
template <typename T>
__global__ __launch_bounds__(512, 2) void k_wgrad256(const Wgrad256Jobs jobs, int rows_per_wg,
                                                    float* __restrict__ slabs,
                                                    float* __restrict__ bslabs) {
  constexpr int D = 256, NT = 512, TB = 32 * D * 2;      // bytes of one 32-row tile
  __shared__ __attribute__((aligned(16))) char lds[4 * TB];     // 2 buffers x (G, A)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  // 1-D grid of nwg * jobs.n workgroups.  When the jobs share an operand (dKp^T X and dVp^T X), the
  // jobs of one row block sit eight linear ids apart, i.e. on the same XCD back to back, and read its
  // tiles from that XCD's L2 instead of twice from memory (measured 250 -> 198 us for the pair; for
  // jobs with nothing in common the same order costs 4 %, so they keep job-major ids).
  const int nwg = gridDim.x / jobs.n;
  int bx, by;
  if (nwg % 8 == 0 && rows_per_wg < 0) {         // (rows_per_wg < 0: the host's "jobs share an operand")
    const int g8 = blockIdx.x >> 3, l8 = blockIdx.x & 7;
    by = g8 % jobs.n;
    bx = (g8 / jobs.n) * 8 + l8;
  } else {
    by = blockIdx.x / nwg;
    bx = blockIdx.x - by * nwg;
  }
  const Wgrad256Job job = jobs.j[by];
  const T* __restrict__ G = reinterpret_cast<const T*>(job.G);
  const T* __restrict__ A = reinterpret_cast<const T*>(job.A);
  // 64-row blocks are dealt round-robin: the workgroups that run together read neighbouring
  // addresses (one contiguous range per workgroup puts all of them 512 KiB apart, on the same few
  // HBM channels at the same moment)
  (void)rows_per_wg;
  const int64_t r0 = (int64_t)bx * 64, r1 = job.M, stride = (int64_t)nwg * 64;
  const int gt0 = 4 * (wave >> 1), at0 = 8 * (wave & 1);
  f32x4 acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  bf16x8 vg[2][2], va[2][2];               // [ring slot][piece]
  auto fetch = [&](int64_t base, bf16x8 (&g2)[2], bf16x8 (&a2)[2]) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int c = tid + e * NT, row = c >> 5, ch = c & 31;
      // (unconditional loads, rows past the end zeroed afterwards: see k_wgrad_small256)
      const bool ok = base + row < r1;
      const int64_t rc = ok ? base + row : r1 - 1;
      g2[e] = gload8(G + rc * D + ch * 8);
      a2[e] = gload8(A + rc * D + ch * 8);
      if (!ok) {
#pragma unroll
        for (int k = 0; k < 8; ++k) { g2[e][k] = (__bf16)0.f; a2[e][k] = (__bf16)0.f; }
      }
    }
  };
  auto consume = [&](int buf, bf16x8 (&g2)[2], bf16x8 (&a2)[2], int64_t refill) {
    char* sG = lds + buf * 2 * TB;
    char* sA = sG + TB;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int c = tid + e * NT, row = c >> 5, ch = c & 31;
      *reinterpret_cast<bf16x8*>(sG + tr_off256(row, ch)) = g2[e];
      *reinterpret_cast<bf16x8*>(sA + tr_off256(row, ch)) = a2[e];
      if (job.db != nullptr) {
#pragma unroll
        for (int k = 0; k < 8; ++k) bs[k] += (float)g2[e][k];
      }
    }
    __syncthreads();
    if (refill < r1) fetch(refill, g2, a2);
    bf16x8 ga[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ga[i] = tr_frag256(sG, gt0 + i, lane);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const bf16x8 ab = tr_frag256(sA, at0 + t, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][t] = mfma32(ga[i], ab, acc[i][t]);
    }
  };
  if (r0 < r1) fetch(r0, vg[0], va[0]);
  if (r0 + 32 < r1) fetch(r0 + 32, vg[1], va[1]);
  for (int64_t base = r0; base < r1; base += stride) {
    consume(0, vg[0], va[0], base + stride);
    if (base + 32 < r1) consume(1, vg[1], va[1], base + stride + 32);
  }
  // slab layout [job][output row][workgroup][256]: the partial sums of one output row lie next to
  // each other, so the summing pass streams 1 KiB x nwg contiguous bytes per row (with one
  // [256][256] block per workgroup it read 1 KiB out of every 256 KiB: 1.2 TB/s)
  float* slab = slabs + (int64_t)by * D * nwg * D + (int64_t)bx * D;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int grow = 16 * (gt0 + i) + 4 * g + e;
#pragma unroll
      for (int t = 0; t < 8; ++t)
        slab[(int64_t)grow * nwg * D + 16 * (at0 + t) + r] = acc[i][t][e];
    }
  if (job.db != nullptr) {
    // threads with equal (tid & 31) hold partial sums of the same 8 columns
    __syncthreads();
    float* red = reinterpret_cast<float*>(lds);             // [16][256]
#pragma unroll
    for (int k = 0; k < 8; ++k) red[(tid >> 5) * D + (tid & 31) * 8 + k] = bs[k];
    __syncthreads();
    if (tid < D) {
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) t += red[q * D + tid];
      bslabs[((int64_t)by * nwg + bx) * D + tid] = t;
    }
  }
}

// Round 3: the bf16 jobs with the operand tiles streamed by LDS-DMA into a ring of four (G, A) tile
// pairs (128 KiB), three pairs ahead.  k_wgrad256 above keeps two 32-row tiles in registers per
// thread - 64 KiB in flight per CU, and 3.0 TB/s is what that bought by Little's law at the
// latency this streaming pattern sees; its MFMA work would sustain 16 TB/s.  Here 96 KiB are in
// flight, nothing is staged through registers, and the barrier per tile only publishes pieces
// that have already landed.  A 1 KiB piece of the transposed-read layout is 4 rows x 256 bytes
// of one [32][128] half: LDS is written linearly, so lane l fetches chunk (l & 15) ^ s(row) of row
// 4 p + (l >> 4) - the swizzle is an involution, the permutation moves to the source side.
__global__ __launch_bounds__(512, 2) void k_wgrad256_dma(const Wgrad256Jobs jobs, int rows_per_wg,
                                                        float* __restrict__ slabs,
                                                        float* __restrict__ bslabs) {
  constexpr int D = 256, TB = 32 * D * 2, NB = 4, PD = NB - 1;
  extern __shared__ __attribute__((aligned(16))) char lds[];    // [NB][G tile | A tile]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int nwg = gridDim.x / jobs.n;
  int bx, by;
  if (nwg % 8 == 0 && rows_per_wg < 0) {
    const int g8 = blockIdx.x >> 3, l8 = blockIdx.x & 7;
    by = g8 % jobs.n;
    bx = (g8 / jobs.n) * 8 + l8;
  } else {
    by = blockIdx.x / nwg;
    bx = blockIdx.x - by * nwg;
  }
  const Wgrad256Job job = jobs.j[by];
  const char* G = reinterpret_cast<const char*>(job.G);
  const char* A = reinterpret_cast<const char*>(job.A);
  const int64_t r0 = (int64_t)bx * 64, r1 = job.M, stride = (int64_t)nwg * 64;
  // tiles of this workgroup: 64-row blocks dealt round-robin, two 32-row tiles per block
  const int64_t nblk = r0 < r1 ? (r1 - r0 + stride - 1) / stride : 0;
  const int ntile = (int)(2 * nblk);
  auto tile_row = [&](int t) { return r0 + (int64_t)(t >> 1) * stride + 32 * (t & 1); };
  const int gt0 = 4 * (wave >> 1), at0 = 8 * (wave & 1);
  f32x4 acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // this wave's four pieces of a tile pair: pieces 2 wave, 2 wave + 1 of G and of A (piece p:
  // half p >> 3, rows 4 (p & 7) ..); per lane the row inside the tile and the source byte offset
  int prow[2], poff[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int p = 2 * wave + e, half = p >> 3, row = 4 * (p & 7) + (lane >> 4);
    const int sw = ((row & 3) << 2) | ((row >> 2) & 3);
    prow[e] = row;
    poff[e] = half * 256 + (((lane & 15) ^ sw) << 4);
  }
  // job.mask: the 256 ReLU-mask words of the tile's 32 rows (1 KiB, contiguous) ride along as a fifth
  // piece of wave 0 into the mask ring behind the tile ring
  const bool masked = job.mask != nullptr;
  const bool mask_wave = masked && wave == 0;
  char* sMaskRing = lds + NB * 2 * TB;
  auto dma = [&](int t) {
    const int64_t base = tile_row(t);
    char* dst = lds + (t % NB) * 2 * TB;
#pragma unroll
    for (int op = 0; op < 2; ++op)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        int64_t row = base + prow[e];
        row = row < r1 ? row : r1 - 1;                 // rows past the end: a valid line (zeroed below)
        const char* src = (op == 0 ? G : A) + row * (D * 2) + poff[e];
        lds_dma16(src, dst + op * TB + (2 * wave + e) * 1024);
      }
    if (mask_wave) {
      const char* src = reinterpret_cast<const char*>(job.mask) + base * 32 + lane * 16;
      lds_dma16(src, sMaskRing + (t % NB) * 1024);
    }
  };
#pragma unroll 1
  for (int t = 0; t < PD && t < ntile; ++t) dma(t);
#pragma unroll 1
  for (int t = 0; t < ntile; ++t) {
    // tile t has landed when at most the pieces of the (up to PD - 1) tiles behind it are pending
    {
      const int ahead = (ntile - 1 - t) < (PD - 1) ? (ntile - 1 - t) : (PD - 1);
      if (mask_wave) {                                 // (five pieces per tile in this wave)
        if (ahead >= 2) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        else if (ahead == 1) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      } else {
        if (ahead >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (ahead == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    lds_barrier();                      // every wave's pieces; tile t - 1 consumed
    if (t + PD < ntile) dma(t + PD);                   // into the buffer tile t - 1 just left
    char* sG = lds + (t % NB) * 2 * TB;
    char* sA = sG + TB;
    const int64_t base = tile_row(t);
    if (base + 32 > r1) {                              // (uniform; the last tile of the job only)
      // rows past the end contribute nothing
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int c = tid + e * 512, row = c >> 5, ch = c & 31;
        if (base + row >= r1) *reinterpret_cast<uint4*>(sG + tr_off256(row, ch)) = uint4{0u, 0u, 0u, 0u};
      }
      lds_barrier();
    }
    if (masked) {
      // G . [mask] in place: thread = (row, 8 features) as below; the features 8 ch .. 8 ch + 7 of a row
      // are two nibbles of the forward's layout (word = 16-row block x head half x lane (r, g), byte =
      // head, bit 4 t + e  <->  feature 32 j + 16 t + 4 g + e): lanes g0 = 2 (ch & 1) and g0 + 1
      const uint32_t* sM = reinterpret_cast<const uint32_t*>(sMaskRing + (t % NB) * 1024);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int c = tid + e * 512, row = c >> 5, ch = c & 31;
        const int wi = ((row >> 4) * 2 + (ch >> 4)) * 64 + (row & 15) + 32 * (ch & 1);
        const int sh = 8 * ((ch >> 2) & 3) + 4 * ((ch >> 1) & 1);
        const uint32_t n0 = sM[wi] >> sh, n1 = sM[wi + 16] >> sh;
        bf16x8 gv = *reinterpret_cast<const bf16x8*>(sG + tr_off256(row, ch));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!((n0 >> k) & 1u)) gv[k] = (__bf16)0.f;
          if (!((n1 >> k) & 1u)) gv[4 + k] = (__bf16)0.f;
        }
        *reinterpret_cast<bf16x8*>(sG + tr_off256(row, ch)) = gv;
        if (job.db != nullptr) {
#pragma unroll
          for (int k = 0; k < 8; ++k) bs[k] += (float)gv[k];
        }
      }
      lds_barrier();
    } else if (job.db != nullptr) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int c = tid + e * 512, row = c >> 5, ch = c & 31;
        const bf16x8 gv = *reinterpret_cast<const bf16x8*>(sG + tr_off256(row, ch));
#pragma unroll
        for (int k = 0; k < 8; ++k) bs[k] += (float)gv[k];
      }
    }
    bf16x8 ga[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ga[i] = tr_frag256(sG, gt0 + i, lane);
#pragma unroll
    for (int tt = 0; tt < 8; ++tt) {
      const bf16x8 ab = tr_frag256(sA, at0 + tt, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][tt] = mfma32(ga[i], ab, acc[i][tt]);
    }
  }
  float* slab = slabs + (int64_t)by * D * nwg * D + (int64_t)bx * D;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int grow = 16 * (gt0 + i) + 4 * g + e;
#pragma unroll
      for (int t = 0; t < 8; ++t)
        slab[(int64_t)grow * nwg * D + 16 * (at0 + t) + r] = acc[i][t][e];
    }
  if (job.db != nullptr) {
    __syncthreads();
    float* red = reinterpret_cast<float*>(lds);             // [16][256]
#pragma unroll
    for (int k = 0; k < 8; ++k) red[(tid >> 5) * D + (tid & 31) * 8 + k] = bs[k];
    __syncthreads();
    if (tid < D) {
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) t += red[q * D + tid];
      bslabs[((int64_t)by * nwg + bx) * D + tid] = t;
    }
  }
}

// dW (and db) += the slabs of a job, in a fixed order (slab_sum_body.hpp: four lane groups take every
// fourth slab, eight 16-byte loads in flight, fixed-order merge).  blockIdx.x < 256: output row of dW;
// == 256: the bias sums (same walk over [nwg][256] partials - as a plain loop of one load per slab in
// one workgroup it was 256 dependent round trips, 90 us); blockIdx.y = job
__global__ __launch_bounds__(256) void k_wgrad256_sum(const Wgrad256Jobs jobs, int nwg,
                                                     const float* __restrict__ slabs,
                                                     const float* __restrict__ bslabs) {
  constexpr int D = 256;
  __shared__ float4 red[4 * 64];
  const Wgrad256Job job = jobs.j[blockIdx.y];
  const int64_t blocks = (job.M + 63) / 64;
  const int used = (int)(blocks < nwg ? blocks : nwg);                  // slabs with rows
  const bool bias_row = blockIdx.x == D;
  if (bias_row && job.db == nullptr) return;
  SlabSumJob s;
  s.slabs = bias_row ? bslabs + (int64_t)blockIdx.y * nwg * D
                     : slabs + ((int64_t)blockIdx.y * D + blockIdx.x) * nwg * D;
  s.out = bias_row ? job.db : job.dW + blockIdx.x * D;
  s.S = used; s.n = D; s.accumulate = 1; s.stride = D;
  slab_sum_body(s, 0, threadIdx.x, red);
}

}  // namespace

// ---- launchers (declared in d256.hpp) ------------------------------------------------
// workgroups per job: enough to stream from every CU, few enough that the slab pass (256 KiB per
// workgroup written + read) stays small against the 1 KiB per row the job reads
int wgrad256_nwg(int64_t maxM) {
  // long jobs: one workgroup per CU; short ones ([B*m] rows): 64 rows each
  int nwg = (int)cdiv(maxM, maxM >= 65536 ? 1024 : 64);
  if (nwg > 256) nwg = 256;
  return nwg < 1 ? 1 : nwg;
}
// Room for `njobs` jobs of AT MOST maxM rows each.  wgrad256_nwg() is not monotonic in the row
// count (64 rows per workgroup below 65 536 rows, 1024 above), and one workspace serves the long
// [B N]-row jobs as well as the short [B m]-row ones of the same block: size for the largest
// workgroup count any job of up to maxM rows can get.
size_t wgrad256_ws_bytes(int njobs, int64_t maxM) {
  size_t nwg = (size_t)cdiv(maxM < 1 ? 1 : maxM, 64);
  if (nwg > 256) nwg = 256;
  return align256((size_t)njobs * nwg * 256 * 256 * sizeof(float)) +
         align256((size_t)njobs * nwg * 256 * sizeof(float));
}
int wgrad256_launch(const Wgrad256Jobs& jobs, void* ws, hipStream_t st) {
  return wgrad256_launch_t(jobs, ws, false, st);
}
static bool wgrad256_use_dma() {      // PCA_WGRAD256_DMA=0: the register-staged kernel (A/B measurements)
  static const bool on = env_not_zero("PCA_WGRAD256_DMA");
  return on;
}
// May a bf16 job hand over dY + the forward's ReLU mask instead of dZ?  (PCA_D256_DZ_MASK=0: no)
bool wgrad256_masked_ok(int64_t rows_per_set) {
  static const bool on = env_not_zero("PCA_D256_DZ_MASK");
  return on && wgrad256_use_dma() && rows_per_set % 128 == 0;
}
int wgrad256_launch_t(const Wgrad256Jobs& jobs, void* ws, bool f32_operands, hipStream_t st) {
  if (jobs.n == 0) return PCA_OK;
  int64_t maxM = 0;
  for (int i = 0; i < jobs.n; ++i) {
    maxM = jobs.j[i].M > maxM ? jobs.j[i].M : maxM;
    PCA_REQUIRE(((uintptr_t)jobs.j[i].dW & 15) == 0, "wgrad256: dW must be 16-byte aligned");
  }
  if (maxM == 0) return PCA_OK;
  const int nwg = wgrad256_nwg(maxM);
  int rpw = (int)cdiv(cdiv(maxM, nwg), 64) * 64;
  Carver c(ws);
  float* slabs = c.take<float>((size_t)jobs.n * nwg * 256 * 256);
  float* bslabs = c.take<float>((size_t)jobs.n * nwg * 256);
  double rows = 0;
  for (int i = 0; i < jobs.n; ++i) rows += (double)jobs.j[i].M;
  bool shared = jobs.n > 1;
  for (int i = 1; i < jobs.n; ++i) shared = shared && jobs.j[i].A == jobs.j[0].A;
  // algorithmic bytes: both operands of every job once (a shared A operand once for all jobs)
  const double eb = f32_operands ? 4.0 : 2.0;
  const double opbytes = shared ? eb * 256 * (rows + (double)jobs.j[0].M) : 2.0 * eb * 256 * rows;
  ProfScope ps(PCA_K_WGRAD, st, 2.0 * rows * 256 * 256, opbytes);
  if (shared) rpw = -rpw;
  const bool use_dma = wgrad256_use_dma();
  for (int i = 0; i < jobs.n; ++i)
    PCA_REQUIRE(jobs.j[i].mask == nullptr || (use_dma && !f32_operands),
                "wgrad256: a masked job needs the LDS-DMA kernel");
  if (f32_operands) {
    hipLaunchKernelGGL(k_wgrad256<float>, dim3(nwg * jobs.n), dim3(512), 0, st, jobs, rpw, slabs,
                       bslabs);
  } else if (use_dma) {
    allow_lds160<k_wgrad256_dma>();
    for (int i = 0; i < jobs.n; ++i)
      PCA_REQUIRE(jobs.j[i].mask == nullptr || jobs.j[i].M % 32 == 0, "wgrad256: masked job rows");
    hipLaunchKernelGGL(k_wgrad256_dma, dim3(nwg * jobs.n), dim3(512),
                       (size_t)4 * 2 * 32 * 256 * 2 + 4 * 1024, st, jobs, rpw, slabs, bslabs);
  } else {
    hipLaunchKernelGGL(k_wgrad256<__bf16>, dim3(nwg * jobs.n), dim3(512), 0, st, jobs, rpw, slabs,
                       bslabs);
  }
  ps.end();
  PCA_TRY(check_launch("k_wgrad256"));
  hipLaunchKernelGGL(k_wgrad256_sum, dim3((256 * 256 + 256 + 255) / 256, jobs.n), dim3(256), 0, st,
                     jobs, nwg, slabs, bslabs);
  return check_launch("k_wgrad256_sum");
}

}  // namespace pca
