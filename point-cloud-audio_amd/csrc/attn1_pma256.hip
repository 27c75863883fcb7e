// Two kernel families of the d = 256 / 8-head step in one translation unit (map: d256.hpp):
//  - the many-queries attention adjoint: k_attn1_bwd3 runs the fc_o adjoint and the attention adjoint in one
//    launch, WAVE = HEAD, and leaves per-range partials of the set's dKp / dVp; k_sum_parts256 adds them in
//    a fixed order;
//  - the PMA at dk = 256 in the reassociated form (k_pma_*256): the N keys are never projected and X is read
//    once; tile layout tr_off256 / tr_frag256 (mfma_common.hpp).
// They share the unit for the compiler's sake: hipcc emits another k_pma_bwd256 (5 instructions more, other
// registers) when the PMA is compiled without k_attn1_bwd3 or k_fq_attn_bwd2 beside it
// (profiles/r07_split_d256.txt, check A).
#include "d256.hpp"
#include "bwd_defer.hpp"
#include "mfma_common.hpp"

#include <math.h>

namespace pca {

namespace {

// =====================================================================================
// k_attn1_bwd3: fc_o adjoint + attention adjoint of the many-queries block, WAVE = HEAD
// =====================================================================================
struct Attn1BwdArgs {
  const __bf16* dO;         // [B*N][D]
  const __bf16* QpS;        // [B*N][D] projected queries saved by the forward
  const __bf16 *KpP, *VpP;  // [B][MI][D] (K-permuted features inside each head)
  const __bf16* Kt;         // [B][D][MI] (keys in perm32 order)
  __bf16* dQp;              // [B*N][D]
  float *dKpPart, *dVpPart; // [B][nparts][MI][D]
  int B, N, nparts, pts_per_part;
  float scale, scale_log2e;
};

// k_attn1_bwd3: fc_o adjoint + attention adjoint of the many-queries block in one launch, WAVE = HEAD,
// with full-line global traffic.  The workgroup moves whole [32 points][256] tiles: Qp and dY arrive by
// LDS-DMA (1 KiB per wave instruction, double buffered, swizzled like the single-launch forward's
// tiles), each wave reads / writes its head's slice of the tiles in LDS, and the dQp tile leaves in
// 16-byte pieces of full rows.  (With every wave fetching its head's 64-byte slice of each row straight
// from memory - 16 rows x 32 bytes per load instruction, 8-byte stores - the attention adjoint alone took
// 243 us at configs[3] for 0.8 GB, 3.3 TB/s.)
// dZ = dY . [Z > 0] ; dO = dY + dZ Wo: the head's 32 columns of dO are computed by the wave that consumes
// them - dO never goes to memory.  The wave keeps its [32 x 256] slice of Wo^T as MFMA A operands (64
// registers); the dZ tile is assembled in LDS from the waves' own slices (mask bytes in the forward's
// layout) and leaves for the weight-gradient pass in full rows.
struct Attn1Bwd3Args {
  Attn1BwdArgs base;
  const __bf16* dY;         // [B*N][D]
  const uint32_t* mask;     // ReLU mask words (mab1_mask_index<256>)
  const __bf16* WoT;        // [256][256] bf16: row = column c of Wo, col = feature f (Wo[f][c])
  __bf16* dZ;               // [B*N][D]
  int tiles128;             // 128-point tiles per set (mask pitch)
  // SMALLQ (layer 1, dq <= 4): Qp is recomputed from the points - nothing was saved
  const float* Xs;          // [B*N][dq] fp32
  const float* WqF;         // [256][dq] fp32
  const float* bq;
  int dq;
};
// SMALLQ: layer 1 (two or three input columns).  The projected queries are not read back (the
// forward does not save them: one [B*N, 256] tensor less written and one less read) but recomputed
// from the tile's points with the forward's own expression, so the bf16 values are the same.
// STORE_DZ = false: dZ does not leave the kernel - the fc_o weight-gradient job then reads dY and the
// mask itself (Wgrad256Job::mask): one [B*N, 256] tensor less written per block.
template <int D, bool SMALLQ, bool STORE_DZ = true>
__global__ __launch_bounds__(64 * (D / 32), 2) void k_attn1_bwd3(const Attn1Bwd3Args aa) {
  const Attn1BwdArgs& a = aa.base;
  constexpr int MI = 32, ROWB = D * 2, TILEB = 32 * ROWB, KS = D / 32;
  constexpr int PQ = 72, IMG = 32 * PQ;
  static_assert(D == 256, "8 waves, 2 DMA pieces per wave and tensor");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sY = smem;                        // dY tile (single: refilled once phase A has read it)
  char* sQb = smem + TILEB;               // [2][TILEB] Qp tiles
  char* sZ = smem + 3 * TILEB;            // dZ tile
  char* sOut = smem + 4 * TILEB;          // dQp tile
  uint32_t* sMaskb = reinterpret_cast<uint32_t*>(smem + 5 * TILEB);      // [2][256 words]
  // SMALLQ: the tile's points [32][dq] fp32 arrive by LDS-DMA too (in the unused Qp tile buffers):
  // ordinary global loads inside the loop make hipcc drain the DMA queue at their first use
  float* sPts = reinterpret_cast<float*>(sQb);                           // [2][128 floats]
  const int tid = threadIdx.x, lane = tid & 63;
  const int j = __builtin_amdgcn_readfirstlane(tid >> 6);      // head of this wave
  const int r = lane & 15, g = lane >> 4;
  const int b = blockIdx.x / a.nparts, part = blockIdx.x - b * a.nparts;
  char* myDS = smem + 5 * TILEB + 2048 + j * 4 * IMG;
  char* myP = myDS + IMG;
  char* myQ = myP + IMG;
  char* myO = myQ + IMG;

  bf16x8 woa[KS][2];
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int t = 0; t < 2; ++t)
      woa[s][t] = *reinterpret_cast<const bf16x8*>(aa.WoT + (int64_t)(32 * j + 16 * t + r) * D +
                                                   32 * s + 8 * g);
  bf16x8 kpa[2], vpa[2], kta[2];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int64_t o = ((int64_t)b * MI + 16 * kt + r) * D + 32 * j + 8 * g;
    kpa[kt] = *reinterpret_cast<const bf16x8*>(a.KpP + o);
    vpa[kt] = *reinterpret_cast<const bf16x8*>(a.VpP + o);
    kta[kt] = *reinterpret_cast<const bf16x8*>(a.Kt + ((int64_t)b * D + 32 * j + 16 * kt + r) * MI +
                                               8 * g);
  }
  float wqs[SMALLQ ? 2 : 1][4][4];
  f32x4 bqv[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  if (SMALLQ) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float4 b4 = *reinterpret_cast<const float4*>(aa.bq + 32 * j + 16 * t + 4 * g);
      bqv[t] = f32x4{b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          wqs[SMALLQ ? t : 0][e][c] =
              c < aa.dq ? aa.WqF[(32 * j + 16 * t + 4 * g + e) * aa.dq + c] : 0.f;
    }
  }
  f32x4 dkp[2][2], dvp[2][2];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      dkp[kt][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
      dvp[kt][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  const int n_lo = part * a.pts_per_part;
  const int n_hi = n_lo + a.pts_per_part < a.N ? n_lo + a.pts_per_part : a.N;
  const int T = n_lo < n_hi ? (n_hi - n_lo + 31) / 32 : 0;
  int oB[4], oD[2];
#pragma unroll
  for (int k = 0; k < 4; ++k) oB[k] = swz(r, 4 * k + g, ROWB);
#pragma unroll
  for (int t = 0; t < 2; ++t) oD[t] = swz(r, 4 * j + 2 * t + (g >> 1), ROWB) + 8 * (g & 1);
  const int oC = swz(tid >> 5, tid & 31, ROWB);
  // tile k of a [B*N][256] tensor into `dst` (2 pieces of 1 KiB per wave, swizzled at the source)
  auto dma_tile = [&](const __bf16* base, int k, char* dst) {
    const int n0 = n_lo + 32 * k;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int p = (2 * j + i) * 64 + lane;
      const int row = p >> 5, slot = p & 31;
      const int ch = (slot & ~15) | ((slot ^ row) & 15);
      const int n = n0 + row < a.N ? n0 + row : a.N - 1;
      lds_dma16(base + ((int64_t)b * a.N + n) * D + ch * 8, dst + (2 * j + i) * 1024);
    }
  };
  // Qp tile k and (wave 0) the tile's 256 mask words: 1 KiB contiguous in the forward's layout
  auto dma_q = [&](int k) {
    if (!SMALLQ) dma_tile(a.QpS, k, sQb + (k & 1) * TILEB);
    if (SMALLQ && (j == 1 || j == 2)) {
      // floats [64 (j - 1), 64 j) of the tile's 32 * dq (<= 128) values; past the end of the tensor:
      // its last element (such points are masked out below)
      const int64_t first = ((int64_t)b * a.N + n_lo + 32 * k) * aa.dq;
      const int64_t last = (int64_t)a.B * a.N * aa.dq - 1;
      int64_t i = first + 64 * (j - 1) + lane;
      i = i < last ? i : last;
      const unsigned ldst = __builtin_amdgcn_readfirstlane(
          (unsigned)(uintptr_t)(lds_void_t*)(sPts + (k & 1) * 128 + 64 * (j - 1)));
      unsigned keep;
      const float* src = aa.Xs + i;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                   "global_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(src), "s"(ldst) : "memory");
    }
    if (j == 0) {
      const int tile32 = (n_lo >> 5) + k;
      const uint32_t* m = aa.mask + (((int64_t)b * aa.tiles128 * 8 + 2 * tile32) * 2) * 64;
      lds_dma16(m + 4 * lane, reinterpret_cast<char*>(sMaskb + (k & 1) * 256));
    }
  };
  if (T > 0) {
    dma_q(0);
    dma_tile(aa.dY, 0, sY);
  }
  // DMA instructions of dma_q in this wave
  const int nq = (SMALLQ ? ((j == 1 || j == 2) ? 1 : 0) : 2) + (j == 0 ? 1 : 0);
  for (int k = 0; k < T; ++k) {
    const int par = k & 1, n0 = n_lo + 32 * k, nlive = n_hi - n0;
    const char* sQ = sQb + par * TILEB;
    const uint32_t* sMask = sMaskb + par * 256;
    float xv[2][4];
    // Qp / mask of tile k + 1 start now (their buffers were last read in iteration k - 1); what must
    // have landed is this tile's dY (issued after barrier B1 of iteration k - 1) and everything older:
    // younger are only the 4 stores of tile k - 1 (always a full tile) and the DMA just issued
    {
      int younger = k > 0 ? (STORE_DZ ? 4 : 2) : 0;
      if (k + 1 < T) {
        dma_q(k + 1);
        younger += nq;
      }
      switch (younger) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
      }
    }
    lds_barrier();                       // B0: dY, Qp, mask of tile k; tile k - 1 fully stored from LDS
    if (SMALLQ) {                        // this lane's points (row r of block nb)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          xv[nb][c] = c < aa.dq ? sPts[par * 128 + (16 * nb + r) * aa.dq + (c < aa.dq ? c : 0)] : 0.f;
    }
    // ---- phase A: own slice of dZ = dY . [Z > 0]; the dY slice stays as the residual ----
    bf16x4 res[2][2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const uint32_t bits = (sMask[(nb * 2 + (j >> 2)) * 64 + lane] >> (8 * (j & 3))) & 0xffu;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const bf16x4 y4 = *reinterpret_cast<const bf16x4*>(sY + oD[t] + 8192 * nb);
        res[t][nb] = y4;
        bf16x4 z4;
#pragma unroll
        for (int e = 0; e < 4; ++e) z4[e] = ((bits >> (4 * t + e)) & 1u) ? y4[e] : (__bf16)0.f;
        *reinterpret_cast<bf16x4*>(sZ + oD[t] + 8192 * nb) = z4;
      }
    }
    lds_barrier();                       // B1: dZ tile complete; dY tile consumed
    if (k + 1 < T) dma_tile(aa.dY, k + 1, sY);
    if (STORE_DZ) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c = tid + 512 * i, row = c >> 5, ch = c & 31;
        if (row < nlive)
          *reinterpret_cast<uint4*>(aa.dZ + ((int64_t)b * a.N + n0 + row) * D + ch * 8) =
              *reinterpret_cast<const uint4*>(sZ + oC + 8192 * i);
      }
    }
    // ---- phase B: dO_h = dY_h + (dZ Wo)_h, then the attention adjoint of this head ----
    f32x4 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) acc[t][nb] = tof(res[t][nb]);
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const bf16x8 zb =
            *reinterpret_cast<const bf16x8*>(sZ + oB[s & 3] + 256 * (s >> 2) + 8192 * nb);
        acc[0][nb] = mfma32(woa[s][0], zb, acc[0][nb]);
        acc[1][nb] = mfma32(woa[s][1], zb, acc[1][nb]);
      }
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const bool live = 16 * nb + r < nlive;
      bf16x4 qlo, qhi;
      if (SMALLQ) {                        // the forward's expression (k_isab1_fwd256<true>)
        f32x4 q[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            q[t][e] = bqv[t][e] + wqs[SMALLQ ? t : 0][e][0] * xv[nb][0] +
                      wqs[SMALLQ ? t : 0][e][1] * xv[nb][1] + wqs[SMALLQ ? t : 0][e][2] * xv[nb][2] +
                      wqs[SMALLQ ? t : 0][e][3] * xv[nb][3];
        qlo = pack4(q[0]);
        qhi = pack4(q[1]);
      } else {
        qlo = *reinterpret_cast<const bf16x4*>(sQ + oD[0] + 8192 * nb);
        qhi = *reinterpret_cast<const bf16x4*>(sQ + oD[1] + 8192 * nb);
      }
      const bf16x4 o0 = pack4(acc[0][nb]), o1 = pack4(acc[1][nb]);     // dO, bf16 as before
      const bf16x8 qb = cat8(qlo, qhi), dob = cat8(o0, o1);
      f32x4 dq0 = tof(o0), dq1 = tof(o1);                 // dQp starts as dO (residual Q_)
      f32x4 p0 = {0.f, 0.f, 0.f, 0.f}, p1 = p0, da0 = p0, da1 = p0;
      p0 = mfma32(kpa[0], qb, p0);
      p1 = mfma32(kpa[1], qb, p1);
      da0 = mfma32(vpa[0], dob, da0);
      da1 = mfma32(vpa[1], dob, da1);
      float mx = fmaxf(fmaxf(fmaxf(p0[0], p0[1]), fmaxf(p0[2], p0[3])),
                       fmaxf(fmaxf(p1[0], p1[1]), fmaxf(p1[2], p1[3])));
      mx = wave16_max(mx);
      float sum = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        p0[e] = __builtin_amdgcn_exp2f((p0[e] - mx) * a.scale_log2e);
        p1[e] = __builtin_amdgcn_exp2f((p1[e] - mx) * a.scale_log2e);
        sum += p0[e] + p1[e];
      }
      sum = wave16_sum(sum);
      const float inv = __builtin_amdgcn_rcpf(sum);
      float delta = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        p0[e] *= inv;
        p1[e] *= inv;
        delta += p0[e] * da0[e] + p1[e] * da1[e];
      }
      delta = wave16_sum(delta);
      f32x4 ds0, ds1;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ds0[e] = p0[e] * (da0[e] - delta) * a.scale;
        ds1[e] = p1[e] * (da1[e] - delta) * a.scale;
      }
      const int pt = 16 * nb + r;
      const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<bf16x4*>(myDS + pt * PQ + 8 * g) = pack4(live ? ds0 : zero4);
      *reinterpret_cast<bf16x4*>(myDS + pt * PQ + 32 + 8 * g) = pack4(live ? ds1 : zero4);
      *reinterpret_cast<bf16x4*>(myP + pt * PQ + 8 * g) = pack4(live ? p0 : zero4);
      *reinterpret_cast<bf16x4*>(myP + pt * PQ + 32 + 8 * g) = pack4(live ? p1 : zero4);
      *reinterpret_cast<bf16x4*>(myQ + pt * PQ + 8 * g) = qlo;
      *reinterpret_cast<bf16x4*>(myQ + pt * PQ + 32 + 8 * g) = qhi;
      *reinterpret_cast<bf16x4*>(myO + pt * PQ + 8 * g) = o0;
      *reinterpret_cast<bf16x4*>(myO + pt * PQ + 32 + 8 * g) = o1;
      const bf16x8 dsb = pack8(ds0, ds1);
      dq0 = mfma32(kta[0], dsb, dq0);
      dq1 = mfma32(kta[1], dsb, dq1);
      *reinterpret_cast<bf16x4*>(sOut + oD[0] + 8192 * nb) = pack4(dq0);
      *reinterpret_cast<bf16x4*>(sOut + oD[1] + 8192 * nb) = pack4(dq1);
    }
    bf16x8 qf[2], of[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      qf[tt] = tr_frag_small(myQ, PQ, 16 * tt, lane);
      of[tt] = tr_frag_small(myO, PQ, 16 * tt, lane);
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      const bf16x8 ads = tr_frag_small(myDS, PQ, 16 * kt, lane);
      const bf16x8 ap = tr_frag_small(myP, PQ, 16 * kt, lane);
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        dkp[kt][tt] = mfma32(ads, qf[tt], dkp[kt][tt]);
        dvp[kt][tt] = mfma32(ap, of[tt], dvp[kt][tt]);
      }
    }
    lds_barrier();                       // B2: the dQp tile is complete
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 512 * i, row = c >> 5, ch = c & 31;
      if (row < nlive)
        *reinterpret_cast<uint4*>(a.dQp + ((int64_t)b * a.N + n0 + row) * D + ch * 8) =
            *reinterpret_cast<const uint4*>(sOut + oC + 8192 * i);
    }
  }
  const int64_t pbase = ((int64_t)b * a.nparts + part) * MI * D;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t o = pbase + (int64_t)(16 * kt + 4 * g + e) * D + 32 * j + 16 * tt + r;
        a.dKpPart[o] = dkp[kt][tt][e];
        a.dVpPart[o] = dvp[kt][tt][e];
      }
}

// dk[b][i] = sum_p kp[b][p][i] (same for v): the per-range partials of k_attn1_bwd3
__global__ void k_sum_parts256(const float* __restrict__ kp, const float* __restrict__ vp,
                               float* __restrict__ dk, float* __restrict__ dv, int B, int nparts,
                               int n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * n) return;
  const int64_t b = i / n, o = i - b * n;
  float x = 0.f, y = 0.f;
  for (int p = 0; p < nparts; ++p) {
    x += kp[(b * nparts + p) * n + o];
    y += vp[(b * nparts + p) * n + o];
  }
  dk[i] = x;
  dv[i] = y;
}

// =====================================================================================
// PMA at dk = 256 (R = h*m <= 16 score rows): reassociated form of mab0_bf16.hip -
//   G' = sl2e Qp_h Wk_h (batch invariant), S = G' X^T, A = softmax_N(S), T = A X -
// so the N keys are never projected and X is read once.  One 16-row score tile; a wave streams
// its own 32-point tiles of X through a private LDS tile (row fragments + transposed fragments).
// =====================================================================================
struct PmaArgs {
  const __bf16* X;             // [B*N][256]
  const __bf16* Gb;            // [>= 16][256] rows r (sl2e folded in; rows >= R zero)
  float *Tp, *Mp, *Lp;         // forward partials [B][S][16][256], [B][S][16]
  const __bf16* dTb;           // [B][16][256]
  const __bf16* TG;            // [B][256][32]: k-slot 8 g + j = j < 4 ? dT[4g+j][c] : G'[4g+j-4][c]
  const float *LSEp, *Delta;   // [B][16]
  __bf16* dX;                  // [B*N][256] or null
  float* DG;                   // backward: slabs [B][S][16][256] of per-workgroup sums
  int B, N, R, S, accumulate_dx;
  const int32_t* lengths;
};

__global__ __launch_bounds__(256, 1) void k_pma_fwd256(const PmaArgs a) {
  constexpr int DK = 256, FT = DK / 16, KS = DK / 32, TB = 32 * DK * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sX = smem;                                             // 4 waves x 16 KiB, later slabs
  float* sAl = reinterpret_cast<float*>(smem + 4 * TB);        // 4 x 16
  float* sM = sAl + 64;
  float* sL = sM + 64;
  float* sT = reinterpret_cast<float*>(sX);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int b = blockIdx.x, sp = blockIdx.y;
  const int per = (int)(((int64_t)(a.N + 127) / 128 + a.S - 1) / a.S) * 128;
  int len = a.N;
  if (a.lengths != nullptr) len = a.lengths[b] < a.N ? a.lengths[b] : a.N;
  const int n_lo = sp * per, n_hi = (n_lo + per < len) ? n_lo + per : len;
  bf16x8 gB[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    gB[ks] = *reinterpret_cast<const bf16x8*>(a.Gb + (int64_t)r * DK + 32 * ks + 8 * g);
  char* myX = sX + wave * TB;
  float* myAl = sAl + wave * 16;
  float mrow = -INFINITY, lrow = 0.f;
  f32x4 T[FT];
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) T[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
  // The wave's next tile is fetched into registers (64 VGPRs - the kernel runs one wave per SIMD,
  // there are 512) while the current one is worked on: without it every tile starts with an
  // exposed round trip to memory.
  bf16x8 nx[16];
  auto fetch_tile = [&](int n0) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int c = lane + 64 * e, row = c >> 5, ch = c & 31;
      const int nr = n0 + row;
      // (rows past the end of the range read its last row and are zeroed when the tile goes to LDS,
      //  one iteration later: zeroed here, hipcc waits for every load right behind its issue -
      //  vmcnt(15) ... vmcnt(0) - and the tile that was meant to arrive during the current tile's
      //  arithmetic is waited for before that arithmetic starts)
      nx[e] = *reinterpret_cast<const bf16x8*>(
          a.X + ((int64_t)b * a.N + (nr < n_hi ? nr : n_hi - 1)) * DK + ch * 8);
    }
  };
  if (n_lo + wave * 32 < n_hi) fetch_tile(n_lo + wave * 32);
  for (int n0 = n_lo + wave * 32; n0 < n_hi; n0 += 128) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int c = lane + 64 * e, row = c >> 5, ch = c & 31;
      bf16x8 v = nx[e];
      if (n0 + row >= n_hi) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (__bf16)0.f;
      }
      *reinterpret_cast<bf16x8*>(myX + tr_off256(row, ch)) = v;
    }
    if (n0 + 128 < n_hi) fetch_tile(n0 + 128);
    f32x4 s[2];
    float mt = -INFINITY;
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
      s[pb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        s[pb] = mfma32(*reinterpret_cast<const bf16x8*>(myX + tr_off256(16 * pb + r, 4 * ks + g)),
                       gB[ks], s[pb]);
      // rows of s = points 16 pb + 4 g + e ; column = score row r
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (n0 + 16 * pb + 4 * g + e >= n_hi) s[pb][e] = -INFINITY;
        mt = fmaxf(mt, s[pb][e]);
      }
    }
    mt = wave16_max(mt);
    const float mnew = fmaxf(mrow, mt);            // finite: the tile has >= 1 live point
    const float alpha = __builtin_amdgcn_exp2f(mrow - mnew);
    float ls = 0.f;
#pragma unroll
    for (int pb = 0; pb < 2; ++pb)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s[pb][e] = __builtin_amdgcn_exp2f(s[pb][e] - mnew);
        ls += s[pb][e];
      }
    ls = wave16_sum(ls);
    lrow = lrow * alpha + ls;
    mrow = mnew;
    // the T tiles hold score rows 4g+e on their accumulator rows: fetch their alphas
    if (g == 0) myAl[r] = alpha;
    const float4 a4 = *reinterpret_cast<const float4*>(&myAl[4 * g]);
    const bf16x8 pa = pack8(s[0], s[1]);
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) {
      T[ft][0] *= a4.x; T[ft][1] *= a4.y; T[ft][2] *= a4.z; T[ft][3] *= a4.w;
      T[ft] = mfma32(pa, tr_frag256(myX, ft, lane), T[ft]);
    }
  }
  // ---- merge the four waves' partial (m, l, T): per-wave slabs over the dead X tiles ----
  __syncthreads();
  if (g == 0) {
    sM[wave * 16 + r] = mrow;
    sL[wave * 16 + r] = lrow;
  }
  __syncthreads();
  float* mySlab = sT + wave * 16 * DK;
  {
    float f4[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int rr = 4 * g + e;
      const float M = fmaxf(fmaxf(sM[rr], sM[16 + rr]), fmaxf(sM[32 + rr], sM[48 + rr]));
      const float mine = sM[wave * 16 + rr];
      f4[e] = (mine == -INFINITY) ? 0.f : exp2f(mine - M);
    }
#pragma unroll
    for (int ft = 0; ft < FT; ++ft)
#pragma unroll
      for (int e = 0; e < 4; ++e) mySlab[(4 * g + e) * DK + 16 * ft + r] = T[ft][e] * f4[e];
  }
  __syncthreads();
  const int64_t pbase = ((int64_t)b * a.S + sp) * 16;
  for (int i = tid; i < 16 * DK; i += 256) {
    const int rr = i / DK;
    a.Tp[pbase * DK + i] = sT[i] + sT[16 * DK + i] + sT[2 * 16 * DK + i] + sT[3 * 16 * DK + i];
    if (i == rr * DK) {
      float M = -INFINITY;
#pragma unroll
      for (int w = 0; w < 4; ++w) M = fmaxf(M, sM[w * 16 + rr]);
      float L = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float mw = sM[w * 16 + rr];
        if (mw != -INFINITY) L += sL[w * 16 + rr] * exp2f(mw - M);
      }
      a.Mp[pbase + rr] = M;
      a.Lp[pbase + rr] = L;
    }
  }
}

// T[b][r][c] = sum_s w_s Tp / sum_s w_s Lp ; LSE[b][r] = M + log2 L   (r < R)
__global__ __launch_bounds__(256) void k_pma_merge(const float* __restrict__ Tp,
                                                   const float* __restrict__ Mp,
                                                   const float* __restrict__ Lp, int B, int S,
                                                   int R, float* __restrict__ T,
                                                   float* __restrict__ LSE) {
  constexpr int DK = 256;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * R * DK) return;
  const int c = (int)(i % DK), rr = (int)((i / DK) % R);
  const int64_t b = i / ((int64_t)DK * R);
  float M = -INFINITY;
  for (int s = 0; s < S; ++s) M = fmaxf(M, Mp[(b * S + s) * 16 + rr]);
  float L = 0.f, t = 0.f;
  for (int s = 0; s < S; ++s) {
    const float ms = Mp[(b * S + s) * 16 + rr];
    if (ms == -INFINITY) continue;
    const float w = exp2f(ms - M);
    L += w * Lp[(b * S + s) * 16 + rr];
    t += w * Tp[((b * S + s) * 16 + rr) * DK + c];
  }
  T[i] = t / L;
  if (c == 0) LSE[b * R + rr] = M + log2f(L);
}

// per set: dT[r][c] = sum_{f in head j} dO[q][f] Wv[f][c], Delta[r] = <dT[r], T[r]>, and the
// operand images of k_pma_bwd256 (dTb natural rows, TG = [dT | G'] interleaved per column)
__global__ __launch_bounds__(256) void k_pma_epi_bwd(const float* __restrict__ dO,
                                                     const float* __restrict__ T,
                                                     const float* __restrict__ LSE,
                                                     const float* __restrict__ Wv,
                                                     const float* __restrict__ Gf, int m, int R,
                                                     __bf16* __restrict__ dTb,
                                                     __bf16* __restrict__ TG,
                                                     float* __restrict__ Delta,
                                                     float* __restrict__ LSEp) {
  constexpr int D = 256;
  __shared__ float sdO[2 * D];            // m <= 2 query rows
  __shared__ float sDel[16][4];
  const int b = blockIdx.x, c = threadIdx.x;
  for (int i = c; i < m * D; i += 256) sdO[i] = dO[(int64_t)b * m * D + i];
  __syncthreads();
  float dT[16];
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) dT[rr] = 0.f;
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    if (rr < R) {
      const int j = rr / m, q = rr - j * m;
      float acc = 0.f;
      for (int f = 0; f < 32; ++f) acc = fmaf(sdO[q * D + 32 * j + f], Wv[(32 * j + f) * D + c], acc);
      dT[rr] = acc;
    }
  }
  // Delta: block reduction per row (wave shuffle, then 4 partials)
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    float v = rr < R ? dT[rr] * T[((int64_t)b * R + rr) * D + c] : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((c & 63) == 0) sDel[rr][c >> 6] = v;
  }
  __syncthreads();
  if (c < 16) {
    Delta[(int64_t)b * 16 + c] = c < R ? sDel[c][0] + sDel[c][1] + sDel[c][2] + sDel[c][3] : 0.f;
    LSEp[(int64_t)b * 16 + c] = c < R ? LSE[(int64_t)b * R + c] : 1.0e30f;
  }
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) dTb[((int64_t)b * 16 + rr) * D + c] = (__bf16)dT[rr];
  bf16x8 row[4];
#pragma unroll
  for (int gq = 0; gq < 4; ++gq)
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int rr = 4 * gq + (jj & 3);
      row[gq][jj] = jj < 4 ? (__bf16)dT[rr] : (__bf16)(rr < R ? Gf[rr * D + c] : 0.f);
    }
#pragma unroll
  for (int gq = 0; gq < 4; ++gq)
    *reinterpret_cast<bf16x8*>(TG + ((int64_t)b * D + c) * 32 + 8 * gq) = row[gq];
}

// dWv[f][c] += sum_{b,q} dO[b][q][f] T[b][j(f) m + q][c]     (deterministic: one thread per (f, c))
__global__ __launch_bounds__(256) void k_pma_dwv(const float* __restrict__ dO,
                                                 const float* __restrict__ T, int B, int m, int R,
                                                 float* __restrict__ dWv) {
  constexpr int D = 256;
  const int f = blockIdx.x, c = threadIdx.x, j = f / 32;
  // (fixed summation order; 8 terms fetched at a time - one by one the B*m dependent round trips
  //  of this loop were 35 us at B = 128)
  float acc = 0.f;
  const int n = B * m;
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    float x[8], y[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int b = (i + u) / m, q = (i + u) - b * m;
      x[u] = dO[((int64_t)b * m + q) * D + f];
      y[u] = T[((int64_t)b * R + j * m + q) * D + c];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = fmaf(x[u], y[u], acc);
  }
  for (; i < n; ++i) {
    const int b = i / m, q = i - b * m;
    acc = fmaf(dO[((int64_t)b * m + q) * D + f], T[((int64_t)b * R + j * m + q) * D + c], acc);
  }
  dWv[f * D + c] += acc;
}

__global__ __launch_bounds__(256, 1) void k_pma_bwd256(const PmaArgs a) {
  constexpr int DK = 256, FT = DK / 16, KS = DK / 32, TB = 32 * DK * 2, PD = 40;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sX = smem;                                 // 4 x 16 KiB ; later the dG slabs (4 x 16 KiB)
  char* sTG = sX + 4 * TB;                         // [256][64 B]
  char* sDS = sTG + DK * 64;                       // 4 x 32 x PD
  float* sLSE = reinterpret_cast<float*>(sDS + 4 * 32 * PD);
  float* sDel = sLSE + 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int b = blockIdx.x, sp = blockIdx.y;
  const int per = (int)(((int64_t)(a.N + 127) / 128 + a.S - 1) / a.S) * 128;
  const int n_lo = sp * per, n_hi = (n_lo + per < a.N) ? n_lo + per : a.N;
  int len = a.N;
  if (a.lengths != nullptr) len = a.lengths[b] < a.N ? a.lengths[b] : a.N;
  for (int i = tid; i < DK * 4; i += 256)
    reinterpret_cast<uint4*>(sTG)[i] = reinterpret_cast<const uint4*>(a.TG + (int64_t)b * DK * 32)[i];
  if (tid < 16) {
    sLSE[tid] = a.LSEp[(int64_t)b * 16 + tid];
    sDel[tid] = a.Delta[(int64_t)b * 16 + tid];
  }
  bf16x8 gA[KS], tA[KS];                   // rows r of G' / dT as A operands [row = r][k = c]
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    gA[ks] = *reinterpret_cast<const bf16x8*>(a.Gb + (int64_t)r * DK + 32 * ks + 8 * g);
    tA[ks] = *reinterpret_cast<const bf16x8*>(a.dTb + ((int64_t)b * 16 + r) * DK + 32 * ks + 8 * g);
  }
  __syncthreads();
  const float4 l4 = *reinterpret_cast<const float4*>(&sLSE[4 * g]);
  const float4 d4 = *reinterpret_cast<const float4*>(&sDel[4 * g]);
  const float lse[4] = {l4.x, l4.y, l4.z, l4.w}, del[4] = {d4.x, d4.y, d4.z, d4.w};
  char* myX = sX + wave * TB;
  char* myDS = sDS + wave * 32 * PD;
  f32x4 dG[FT];
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) dG[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr float LN2 = 0.6931471805599453f;
  // The wave's next tile is fetched into registers (64 VGPRs - the kernel runs one wave per SIMD,
  // there are 512) while the current one is worked on: without it every tile starts with an
  // exposed round trip to memory.
  bf16x8 nx[16];
  auto fetch_tile = [&](int n0) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int c = lane + 64 * e, row = c >> 5, ch = c & 31;
      const int nr = n0 + row;
      // (rows past the end of the range read its last row and are zeroed when the tile goes to LDS,
      //  one iteration later: zeroed here, hipcc waits for every load right behind its issue -
      //  vmcnt(15) ... vmcnt(0) - and the tile that was meant to arrive during the current tile's
      //  arithmetic is waited for before that arithmetic starts)
      nx[e] = *reinterpret_cast<const bf16x8*>(
          a.X + ((int64_t)b * a.N + (nr < n_hi ? nr : n_hi - 1)) * DK + ch * 8);
    }
  };
  if (n_lo + wave * 32 < n_hi) fetch_tile(n_lo + wave * 32);
  for (int n0 = n_lo + wave * 32; n0 < n_hi; n0 += 128) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int c = lane + 64 * e, row = c >> 5, ch = c & 31;
      bf16x8 v = nx[e];
      if (n0 + row >= n_hi) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (__bf16)0.f;
      }
      *reinterpret_cast<bf16x8*>(myX + tr_off256(row, ch)) = v;
    }
    if (n0 + 128 < n_hi) fetch_tile(n0 + 128);
    bf16x8 pds[2];                          // B operand [k = (P rows | dS rows)][col = point]
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
      f32x4 sv = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 xr =
            *reinterpret_cast<const bf16x8*>(myX + tr_off256(16 * pb + r, 4 * ks + g));
        sv = mfma32(gA[ks], xr, sv);        // rows = score rows 4g+e, column = point 16 pb + r
        da = mfma32(tA[ks], xr, da);
      }
      const bool key = n0 + 16 * pb + r < len;
      f32x4 p, ds;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        p[e] = key ? __builtin_amdgcn_exp2f(sv[e] - lse[e]) : 0.f;
        ds[e] = LN2 * p[e] * (da[e] - del[e]);
      }
      pds[pb] = pack8(p, ds);
      *reinterpret_cast<bf16x4*>(myDS + (16 * pb + r) * PD + 8 * g) = pack4(ds);
    }
    // dG[r][c] += sum_points dS[r][pt] X[pt][c]   (before the X tile is re-used for dX)
    const bf16x8 dsa = tr_frag_small(myDS, PD, 0, lane);
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) dG[ft] = mfma32(dsa, tr_frag256(myX, ft, lane), dG[ft]);
    if (a.dX != nullptr) {
      // dX tile [32 points][256] assembled in the wave's own LDS tile (its X is no longer needed)
      // and stored / accumulated in 16-byte pieces of full rows - straight from the accumulator
      // layout it was 32 store instructions of 8 bytes per lane, 16 rows x 32 bytes each
#pragma unroll
      for (int ft = 0; ft < FT; ++ft) {
        const bf16x8 tg = *reinterpret_cast<const bf16x8*>(sTG + (16 * ft + r) * 64 + 16 * g);
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
          const f32x4 dx = mfma32(tg, pds[pb], f32x4{0.f, 0.f, 0.f, 0.f});
          *reinterpret_cast<bf16x4*>(myX + swz(16 * pb + r, 2 * ft + (g >> 1), 2 * DK) + 8 * (g & 1)) =
              pack4(dx);
        }
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int c = lane + 64 * e, row = c >> 5, ch = c & 31;
        const int n = n0 + row;
        bf16x8 v = *reinterpret_cast<const bf16x8*>(myX + swz(row, ch, 2 * DK));
        __bf16* pd = a.dX + ((int64_t)b * a.N + (n < n_hi ? n : n_hi - 1)) * DK + ch * 8;
        if (a.accumulate_dx) {              // (wave-uniform; the load itself is unconditional)
          const bf16x8 o = *reinterpret_cast<const bf16x8*>(pd);
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] = (__bf16)((float)v[k] + (float)o[k]);
        }
        if (n < n_hi) *reinterpret_cast<bf16x8*>(pd) = v;
      }
    }
  }
  __syncthreads();
  float* slab = reinterpret_cast<float*>(sX) + wave * 16 * DK;
#pragma unroll
  for (int ft = 0; ft < FT; ++ft)
#pragma unroll
    for (int e = 0; e < 4; ++e) slab[(4 * g + e) * DK + 16 * ft + r] = dG[ft][e];
  __syncthreads();
  const float* s0 = reinterpret_cast<const float*>(sX);
  // (no atomics: one [16][256] slab per workgroup, slab_sum adds them in a fixed order)
  float* out = a.DG + ((int64_t)b * a.S + sp) * 16 * DK;
  for (int i = tid; i < 16 * DK; i += 256)
    out[i] = s0[i] + s0[16 * DK + i] + s0[2 * 16 * DK + i] + s0[3 * 16 * DK + i];
}

}  // namespace

// ---- launchers (declared in d256.hpp) ------------------------------------------------
int attn1_bwd256_parts(int B, int N) {
  // point ranges per set so that B * parts workgroups (2 per CU) cover the chip
  int parts = 1;
  const int tiles = (int)cdiv(N, 32);
  while (parts * 2 <= tiles && B * parts < 512) parts *= 2;
  return parts;
}
// fc_o adjoint + attention adjoint in one launch (k_attn1_bwd3); WoT: transposed natural image
int attn1_bwd256_fused(const __bf16* dY, const uint32_t* mask, const __bf16* WoT, const __bf16* QpS,
                       const __bf16* KpP, const __bf16* VpP, const __bf16* Kt, __bf16* dZ,
                       __bf16* dQp, float* dKpPart, float* dVpPart, float* dKp, float* dVp, int B,
                       int N, hipStream_t st, const float* Xs, const float* WqF, const float* bq,
                       int dq) {
  constexpr int D = 256;
  int parts = attn1_bwd256_parts(B, N);
  if (B * parts > 256 && parts > 1) parts /= 2;            // 155 KiB of LDS: one workgroup per CU
  const int ppp = (int)cdiv(cdiv(N, 32), parts) * 32;
  Attn1Bwd3Args a{};
  a.base = Attn1BwdArgs{nullptr, QpS, KpP, VpP, Kt, dQp, dKpPart, dVpPart, B, N, parts, ppp,
                        1.0f / sqrtf((float)D), LOG2E / sqrtf((float)D)};
  a.dY = dY; a.mask = mask; a.WoT = WoT; a.dZ = dZ;
  a.tiles128 = (int)cdiv(N, 128);
  a.Xs = Xs; a.WqF = WqF; a.bq = bq; a.dq = dq;
  const bool smallq = QpS == nullptr;
  PCA_REQUIRE(!smallq || (Xs && WqF && bq && dq >= 1 && dq <= 4),
              "attn1_bwd256_fused: no saved Qp and no points to recompute it from");
  allow_lds160<k_attn1_bwd3<D, false, true>,
               k_attn1_bwd3<D, true, true>,
               k_attn1_bwd3<D, false, false>,
               k_attn1_bwd3<D, true, false>>();
  const size_t lds = (size_t)5 * 32 * D * 2 + 2048 + (size_t)8 * 4 * 32 * 72;
  const dim3 grid(B * parts), block(512);
  // dZ == nullptr: dZ stays inside the kernel (the weight-gradient job applies the mask to dY itself)
  if (dZ != nullptr) {
    if (smallq) hipLaunchKernelGGL((k_attn1_bwd3<D, true, true>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((k_attn1_bwd3<D, false, true>), grid, block, lds, st, a);
  } else {
    if (smallq) hipLaunchKernelGGL((k_attn1_bwd3<D, true, false>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((k_attn1_bwd3<D, false, false>), grid, block, lds, st, a);
  }
  PCA_TRY(check_launch("k_attn1_bwd3"));
  hipLaunchKernelGGL(k_sum_parts256, dim3((unsigned)cdiv((int64_t)B * 32 * D, 256)), dim3(256), 0,
                     st, dKpPart, dVpPart, dKp, dVp, B, parts, 32 * D);
  return check_launch("k_sum_parts256");
}

size_t pma_bwd256_slab_bytes(int B) {
  return align256((size_t)(B > 256 ? B : 256) * 16 * 256 * sizeof(float));
}
int pma_splits256(int B, int N) {
  int S = 1;
  const int tiles = (int)cdiv(N, 128);
  while (S * 2 <= tiles && B * S < 512 && S < 16) S *= 2;
  return S;
}
int pma_attn_fwd256(const __bf16* X, const __bf16* Gb, int B, int N, int R, const int32_t* lengths,
                    float* Tp, float* Mp, float* Lp, float* T, float* LSE, hipStream_t st) {
  PmaArgs a{};
  a.X = X; a.Gb = Gb; a.Tp = Tp; a.Mp = Mp; a.Lp = Lp;
  a.B = B; a.N = N; a.R = R; a.S = pma_splits256(B, N); a.lengths = lengths;
  allow_lds160<k_pma_fwd256>();
  hipLaunchKernelGGL(k_pma_fwd256, dim3(B, a.S), dim3(256), 4 * 32 * 256 * 2 + 3 * 64 * sizeof(float),
                     st, a);
  PCA_TRY(check_launch("k_pma_fwd256"));
  hipLaunchKernelGGL(k_pma_merge, dim3((unsigned)cdiv((int64_t)B * R * 256, 256)), dim3(256), 0, st,
                     Tp, Mp, Lp, B, a.S, R, T, LSE);
  return check_launch("k_pma_merge");
}
int pma_epi_bwd256(const float* dO, const float* T, const float* LSE, const float* Wv,
                   const float* Gf, int B, int m, int R, __bf16* dTb, __bf16* TG, float* Delta,
                   float* LSEp, float* dWv, hipStream_t st) {
  hipLaunchKernelGGL(k_pma_epi_bwd, dim3(B), dim3(256), 0, st, dO, T, LSE, Wv, Gf, m, R, dTb, TG,
                     Delta, LSEp);
  PCA_TRY(check_launch("k_pma_epi_bwd"));
  hipLaunchKernelGGL(k_pma_dwv, dim3(256), dim3(256), 0, st, dO, T, B, m, R, dWv);
  return check_launch("k_pma_dwv");
}
int pma_attn_bwd256(const __bf16* X, const __bf16* Gb, const __bf16* dTb, const __bf16* TG,
                    const float* LSEp, const float* Delta, int B, int N, int R,
                    const int32_t* lengths, __bf16* dX, int accumulate_dx, float* DG,
                    float* DGslabs, hipStream_t st) {
  PmaArgs a{};
  a.X = X; a.Gb = Gb; a.dTb = dTb; a.TG = TG; a.LSEp = LSEp; a.Delta = Delta;
  a.dX = dX; a.DG = DGslabs; a.accumulate_dx = accumulate_dx;
  a.B = B; a.N = N; a.R = R; a.lengths = lengths;
  int S = pma_splits256(B, N);
  while (S > 1 && B * S > 256) S /= 2;            // ~100 KiB of LDS: one workgroup per CU
  a.S = S;
  allow_lds160<k_pma_bwd256>();
  const size_t lds = 4 * 32 * 256 * 2 + 256 * 64 + 4 * 32 * 40 + 32 * sizeof(float);
  hipLaunchKernelGGL(k_pma_bwd256, dim3(B, S), dim3(256), lds, st, a);
  PCA_TRY(check_launch("k_pma_bwd256"));
  return slab_sum(DGslabs, B * S, 16 * 256, DG, 0, st);
}

}  // namespace pca
