// The few-queries attention (ISAB mab0 at dk = 256) over projected keys, wave = head, head dim 32
// (map: d256.hpp): the forward with the projection in the same pass (k_fq_proj_fwd, m = 32) or
// after k_rowstream PROJ2 (k_fq_attn_fwd, m <= 16), the backward (k_fq_attn_bwd2 / k_fq_attn_bwd) and
// the small kernels that join the per-range partials.
#include "d256.hpp"
#include "mfma_common.hpp"

#include <math.h>

namespace pca {

namespace {

// =====================================================================================
// few-queries attention (ISAB mab0 at dk = 256) over projected keys: wave = head, head dim 32
// =====================================================================================
struct FqArgs {
  const __bf16 *Kp, *Vp;     // [B*N][D]
  const float* Qp;           // [m][D] shared projected query (fp32)
  // forward
  float *Op, *Mp, *Lp;       // [B][S][m][D] unnormalised sum_n 2^(s-M) Vp ; [B][S][H][MQ] M, L
  // backward
  const float* dOa;          // [B][m][D] gradient w.r.t. A Vp (= dO)
  const float* LSE;          // [B][H][MQ] log2-domain
  const float* Delta;        // [B][H][MQ]
  __bf16 *dKp, *dVp;         // [B*N][D]
  float* dQpPart;            // [B][S][m][D]
  int B, N, m, S;
  float scale_log2e, scale;  // log2(e)/sqrt(d) ; 1/sqrt(d)
  const int32_t* lengths;
};

// shared query of head j as MFMA operands: element (q, f) = Qp[q][32 j + f] * mul
// as B operand [k = f][col = q] / as A operand [row = q][k = f]: the same registers
__device__ __forceinline__ bf16x8 q_frag(const float* Qp, int D, int m, int q, int j, int g,
                                         float mul) {
  bf16x8 v;
  if (q < m) {
    const float4 lo = *reinterpret_cast<const float4*>(Qp + (int64_t)q * D + 32 * j + 8 * g);
    const float4 hi = *reinterpret_cast<const float4*>(Qp + (int64_t)q * D + 32 * j + 8 * g + 4);
    v[0] = (__bf16)(lo.x * mul); v[1] = (__bf16)(lo.y * mul); v[2] = (__bf16)(lo.z * mul);
    v[3] = (__bf16)(lo.w * mul); v[4] = (__bf16)(hi.x * mul); v[5] = (__bf16)(hi.y * mul);
    v[6] = (__bf16)(hi.z * mul); v[7] = (__bf16)(hi.w * mul);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (__bf16)0.f;
  }
  return v;
}

// forward: S^T[pt][q] = Kp_h[pt][:] . (sl2e Qp_h[q][:]) on the MFMA with the points on the
// accumulator rows (a query's statistics: in-lane + 2 cross-lane steps), online softmax,
// O^T[f][q] += Vp_h^T[f][pt] P^T[pt][q] with the probability tile as B operand straight from the
// accumulators and Vp^T through a wave-private LDS tile + ds_read_tr16_b64.
template <int D, int QT>          // QT = query tiles of 16 (m <= 16 QT)
__global__ __launch_bounds__(64 * (D / 32)) void k_fq_attn_fwd(const FqArgs a) {
  constexpr int PV = 72, H = D / 32, MQ = 16 * QT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, j = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int b = blockIdx.x, sp = blockIdx.y;
  char* myV = smem + j * 32 * PV;
  const int per = (int)(((int64_t)(a.N + 31) / 32 + a.S - 1) / a.S) * 32;
  int len = a.N;
  if (a.lengths != nullptr) len = a.lengths[b] < a.N ? a.lengths[b] : a.N;
  const int n_lo = sp * per, n_hi = (n_lo + per < len) ? n_lo + per : len;
  bf16x8 qf[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) qf[qt] = q_frag(a.Qp, D, a.m, 16 * qt + r, j, g, a.scale_log2e);
  float mrow[QT], lrow[QT];
  f32x4 ot[2][QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    mrow[qt] = -INFINITY;
    lrow[qt] = 0.f;
    ot[0][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
    ot[1][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int n0 = n_lo; n0 < n_hi; n0 += 32) {
    bf16x8 kr[2];
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
      const int n = n0 + 16 * pb + r;
      bf16x8 vr;
      {   // unconditional loads (last row for points past the range), zeroed afterwards: a load
          // under a divergent `if` is waited for with vmcnt(0) before the next one is issued
        const int64_t o = ((int64_t)b * a.N + (n < n_hi ? n : n_hi - 1)) * D + 32 * j + 8 * g;
        kr[pb] = *reinterpret_cast<const bf16x8*>(a.Kp + o);
        vr = *reinterpret_cast<const bf16x8*>(a.Vp + o);
        if (n >= n_hi) {
#pragma unroll
          for (int e = 0; e < 8; ++e) { kr[pb][e] = (__bf16)0.f; vr[e] = (__bf16)0.f; }
        }
      }
      {   // (two 8-byte stores: the padded 72-byte pitch is not 16-byte aligned)
        bf16x4 lo4, hi4;
#pragma unroll
        for (int e = 0; e < 4; ++e) { lo4[e] = vr[e]; hi4[e] = vr[4 + e]; }
        *reinterpret_cast<bf16x4*>(myV + (16 * pb + r) * PV + 16 * g) = lo4;
        *reinterpret_cast<bf16x4*>(myV + (16 * pb + r) * PV + 16 * g + 8) = hi4;
      }
    }
    bf16x8 vt[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) vt[tt] = tr_frag_small(myV, PV, 16 * tt, lane);
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      f32x4 s[2];
      float mt = -INFINITY;
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) {
        s[pb] = mfma32(kr[pb], qf[qt], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (n0 + 16 * pb + 4 * g + e >= n_hi) s[pb][e] = -INFINITY;
          mt = fmaxf(mt, s[pb][e]);
        }
      }
      mt = wave16_max(mt);
      const float mnew = fmaxf(mrow[qt], mt);           // finite: the tile has >= 1 live point
      const float alpha = __builtin_amdgcn_exp2f(mrow[qt] - mnew);
      float ls = 0.f;
#pragma unroll
      for (int pb = 0; pb < 2; ++pb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s[pb][e] = __builtin_amdgcn_exp2f(s[pb][e] - mnew);
          ls += s[pb][e];
        }
      ls = wave16_sum(ls);
      lrow[qt] = lrow[qt] * alpha + ls;
      mrow[qt] = mnew;
      const bf16x8 pb8 = pack8(s[0], s[1]);
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
        for (int e = 0; e < 4; ++e) ot[tt][qt][e] *= alpha;     // column q = this lane's query
        ot[tt][qt] = mfma32(vt[tt], pb8, ot[tt][qt]);
      }
    }
  }
  // partial (O^T, M, L) of this range: rows f = 16 tt + 4 g + e, column q = 16 qt + r
  const int64_t pb0 = ((int64_t)b * a.S + sp);
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int q = 16 * qt + r;
    if (q < a.m) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
        *reinterpret_cast<float4*>(a.Op + (pb0 * a.m + q) * D + 32 * j + 16 * tt + 4 * g) =
            float4{ot[tt][qt][0], ot[tt][qt][1], ot[tt][qt][2], ot[tt][qt][3]};
      if (g == 0) {
        a.Mp[(pb0 * H + j) * MQ + q] = mrow[qt];
        a.Lp[(pb0 * H + j) * MQ + q] = lrow[qt];
      }
    }
  }
}

// k_fq_proj_fwd (m = 32, d = 256): fc_k / fc_v of the N keys AND the few-queries attention over
// them in one pass over X.  Per 32-point tile the workgroup computes the Kp / Vp tiles as
// k_rowstream<1,2> does (wave j: output features 32 j .. 32 j + 31 of both, the two [32 x 256]
// weight slices in 128 registers, X tiles by LDS-DMA three deep), every wave writes its slices to
// the Kp / Vp tiles in LDS - and head j's attention needs exactly the slices wave j just wrote, so
// it reads them back without a barrier and runs the online-softmax step of k_fq_attn_fwd on them (both
// query tiles, operands from LDS instead of global memory); after one barrier the two tiles leave for
// the backward in full rows.  Against PROJ2 + a separate attention launch the Kp / Vp tensors are
// written but never read back: two [B*N, 256] passes less.
struct FqProjArgs {
  FqArgs f;
  const __bf16* X;               // [B*N][256]
  const __bf16 *WkB, *WvB;       // natural bf16 images [256][256] (F8: fp8 e4m3 bytes of s * W)
  const float *bk, *bv;
  __bf16 *KpO, *VpO;             // [B*N][256] outputs (saved for the backward)
  const float* inv_scale;        // F8: 1 / s_k, 1 / s_v
};
// F8 (PCA_MODE_FP8, round 3): fc_k / fc_v on v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 operands, block
// scales 2^0: twice the bf16 rate, scripts/probe/mfma_f8_probe.hip).  The X tile is converted to
// fp8 ONCE per tile by the whole workgroup (16 elements per thread, into an 8 KiB fp8 tile with
// 16-byte chunks XOR-swizzled by row) instead of once per fragment and wave as k_rowstream<F8>
// does (28 VALU instructions per fragment, eight waves converting the same values); the weight
// slices are 32 + 32 registers instead of 64 + 64 and a tile's 64 MFMAs of 16 cycles become 16 of
// 32.  The attention on the bf16 Kp / Vp slices is unchanged.
typedef int fq_v8i __attribute__((ext_vector_type(8)));
template <bool F8>
__global__ __launch_bounds__(512, 2) void k_fq_proj_fwd(const FqProjArgs aa) {
  const FqArgs& a = aa.f;
  constexpr int D = 256, QT = 2, PV = 72, H = D / 32, MQ = 16 * QT, KS = D / 32;
  constexpr int ROWB = D * 2, TILEB = 32 * ROWB, NBUF = 3, PD = NBUF - 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sXb = smem;                        // [NBUF][TILEB]
  char* sK = smem + NBUF * TILEB;          // Kp tile
  char* sV = sK + TILEB;                   // Vp tile
  char* sX8 = sV + TILEB + H * 32 * PV;    // F8: the current X tile as fp8 [32][256 B]
  const int tid = threadIdx.x, lane = tid & 63;
  const int j = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int b = blockIdx.x, sp = blockIdx.y;
  char* myV = sV + TILEB + j * 32 * PV;
  const int per = (int)(((int64_t)(a.N + 31) / 32 + a.S - 1) / a.S) * 32;
  int len = a.N;
  if (a.lengths != nullptr) len = a.lengths[b] < a.N ? a.lengths[b] : a.N;
  // the projections cover every row of the range (the backward reads padded rows too); the
  // attention only the keys: rows below min(range end, len)
  const int n_lo = sp * per;
  const int n_end = (n_lo + per < a.N) ? n_lo + per : a.N;
  const int n_hi = n_end < len ? n_end : len;
  const int T = n_lo < n_end ? (n_end - n_lo + 31) / 32 : 0;
  bf16x8 wk[F8 ? 1 : KS][2], wv[F8 ? 1 : KS][2];
  fq_v8i wk8[F8 ? 2 : 1][2], wv8[F8 ? 2 : 1][2];
  float inv_k = 1.f, inv_v = 1.f;
  if (F8) {
    inv_k = aa.inv_scale[0];
    inv_v = aa.inv_scale[1];
#pragma unroll
    for (int S = 0; S < 2; ++S)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int o = (32 * j + 16 * t + r) * D + 128 * S + 32 * g;
        const uint4* pk = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(aa.WkB) + o);
        const uint4* pv = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(aa.WvB) + o);
        const uint4 k0 = pk[0], k1 = pk[1], v0 = pv[0], v1 = pv[1];
        wk8[F8 ? S : 0][t] = fq_v8i{(int)k0.x, (int)k0.y, (int)k0.z, (int)k0.w,
                                    (int)k1.x, (int)k1.y, (int)k1.z, (int)k1.w};
        wv8[F8 ? S : 0][t] = fq_v8i{(int)v0.x, (int)v0.y, (int)v0.z, (int)v0.w,
                                    (int)v1.x, (int)v1.y, (int)v1.z, (int)v1.w};
      }
  } else {
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int64_t o = (int64_t)(32 * j + 16 * t + r) * D + 32 * s + 8 * g;
        wk[F8 ? 0 : s][t] = *reinterpret_cast<const bf16x8*>(aa.WkB + o);
        wv[F8 ? 0 : s][t] = *reinterpret_cast<const bf16x8*>(aa.WvB + o);
      }
  }
  // F8: this thread's share of the tile conversion (row tid / 16, fp8 chunk tid % 16 = bf16 chunks
  // 2 c, 2 c + 1) and this lane's two 16-byte chunks of an fp8 row (k = 32 g .. 32 g + 31; + 128 S)
  const int cvr = tid >> 4, cvc = tid & 15;
  const int cv_src0 = swz(cvr, 2 * cvc, ROWB), cv_src1 = swz(cvr, 2 * cvc + 1, ROWB);
  const int cv_dst = cvr * D + ((cvc ^ (cvr & 15)) << 4);
  int x8r[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) x8r[c] = r * D + (((2 * g + c) ^ r) << 4);
  f32x4 bkz[2], bvz[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float4 k4 = *reinterpret_cast<const float4*>(aa.bk + 32 * j + 16 * t + 4 * g);
    const float4 v4 = *reinterpret_cast<const float4*>(aa.bv + 32 * j + 16 * t + 4 * g);
    bkz[t] = f32x4{k4.x, k4.y, k4.z, k4.w};
    bvz[t] = f32x4{v4.x, v4.y, v4.z, v4.w};
  }
  bf16x8 qf[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) qf[qt] = q_frag(a.Qp, D, a.m, 16 * qt + r, j, g, a.scale_log2e);
  float mrow[QT], lrow[QT];
  f32x4 ot[2][QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    mrow[qt] = -INFINITY;
    lrow[qt] = 0.f;
    ot[0][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
    ot[1][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  int oB[4], oD[2];
#pragma unroll
  for (int k = 0; k < 4; ++k) oB[k] = swz(r, 4 * k + g, ROWB);
#pragma unroll
  for (int t = 0; t < 2; ++t) oD[t] = swz(r, 4 * j + 2 * t + (g >> 1), ROWB) + 8 * (g & 1);
  const int oK = swz(r, 4 * j + g, ROWB);
  const int oC = swz(tid >> 5, tid & 31, ROWB);
  auto dma = [&](int k) {
    const int n0 = n_lo + 32 * k;
    char* dst = sXb + (k % NBUF) * TILEB;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int p = (2 * j + i) * 64 + lane;
      const int row = p >> 5, slot = p & 31;
      const int ch = (slot & ~15) | ((slot ^ row) & 15);
      const int n = n0 + row < a.N ? n0 + row : a.N - 1;
      const __bf16* src = aa.X + ((int64_t)b * a.N + n) * D + ch * 8;
      lds_dma16(src, dst + (2 * j + i) * 1024);
    }
  };
#pragma unroll 1
  for (int k = 0; k < PD && k < T; ++k) dma(k);
#pragma unroll 1
  for (int k = 0; k < T; ++k) {
    const int n0 = n_lo + 32 * k, nlive = a.N - n0;
    const char* sX = sXb + (k % NBUF) * TILEB;
    // tile k + PD streams in; tile k must have landed: younger are the DMAs of the tiles ahead (2
    // pieces each) and the 4 stores of each of the last PD tiles (all full: not the last of a range)
    if (k + PD < T) dma(k + PD);
    {
      const int ahead = (T - 1 - k) < PD ? (T - 1 - k) : PD;
      const int behind = k < PD ? k : PD;
      switch (2 * ahead + 4 * behind) {
        case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
        case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
      }
    }
    lds_barrier();                       // B0: X tile k; the previous Kp / Vp tiles are stored
    if (F8) {
      const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(sX + cv_src0);
      const bf16x8 x1 = *reinterpret_cast<const bf16x8*>(sX + cv_src1);
      uint4 q;
      q.x = cvt4_f8((float)x0[0], (float)x0[1], (float)x0[2], (float)x0[3]);
      q.y = cvt4_f8((float)x0[4], (float)x0[5], (float)x0[6], (float)x0[7]);
      q.z = cvt4_f8((float)x1[0], (float)x1[1], (float)x1[2], (float)x1[3]);
      q.w = cvt4_f8((float)x1[4], (float)x1[5], (float)x1[6], (float)x1[7]);
      *reinterpret_cast<uint4*>(sX8 + cv_dst) = q;
      lds_barrier();                     // B0b: the fp8 tile (the previous tile's readers passed B1)
    }
    // ---- Kp_h^T, Vp_h^T = W_h . X^T + b: own slices of the two tiles ----
    {
      f32x4 ak[2][2], av[2][2];
      if (F8) {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          fq_v8i fb8[2];
#pragma unroll
          for (int S = 0; S < 2; ++S) {
            const uint4 lo = *reinterpret_cast<const uint4*>(sX8 + 16 * D * nb + (x8r[0] ^ (S << 7)));
            const uint4 hi = *reinterpret_cast<const uint4*>(sX8 + 16 * D * nb + (x8r[1] ^ (S << 7)));
            fb8[S] = fq_v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w,
                            (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
          }
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            f32x4 k4 = {0.f, 0.f, 0.f, 0.f}, v4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int S = 0; S < 2; ++S) {
              k4 = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wk8[F8 ? S : 0][t], fb8[S], k4, 0, 0,
                                                                   0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
              v4 = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wv8[F8 ? S : 0][t], fb8[S], v4, 0, 0,
                                                                   0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              ak[t][nb][e] = __builtin_fmaf(k4[e], inv_k, bkz[t][e]);
              av[t][nb][e] = __builtin_fmaf(v4[e], inv_v, bvz[t][e]);
            }
          }
        }
      } else {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) { ak[t][nb] = bkz[t]; av[t][nb] = bvz[t]; }
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          const bf16x8 bx =
              *reinterpret_cast<const bf16x8*>(sX + oB[s & 3] + 256 * (s >> 2) + 8192 * nb);
          ak[0][nb] = mfma32(wk[F8 ? 0 : s][0], bx, ak[0][nb]);
          ak[1][nb] = mfma32(wk[F8 ? 0 : s][1], bx, ak[1][nb]);
          av[0][nb] = mfma32(wv[F8 ? 0 : s][0], bx, av[0][nb]);
          av[1][nb] = mfma32(wv[F8 ? 0 : s][1], bx, av[1][nb]);
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          *reinterpret_cast<bf16x4*>(sK + oD[t] + 8192 * nb) = pack4(ak[t][nb]);
          *reinterpret_cast<bf16x4*>(sV + oD[t] + 8192 * nb) = pack4(av[t][nb]);
        }
    }
    // ---- head j's attention on the slices this wave just wrote (k_fq_attn_fwd's tile step) ----
    if (n0 < n_hi) {
      bf16x8 kr[2];
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) {
        const int n = n0 + 16 * pb + r;
        kr[pb] = *reinterpret_cast<const bf16x8*>(sK + oK + 8192 * pb);
        bf16x8 vr = *reinterpret_cast<const bf16x8*>(sV + oK + 8192 * pb);
        if (n >= n_hi) {
#pragma unroll
          for (int e = 0; e < 8; ++e) { kr[pb][e] = (__bf16)0.f; vr[e] = (__bf16)0.f; }
        }
        bf16x4 lo4, hi4;
#pragma unroll
        for (int e = 0; e < 4; ++e) { lo4[e] = vr[e]; hi4[e] = vr[4 + e]; }
        *reinterpret_cast<bf16x4*>(myV + (16 * pb + r) * PV + 16 * g) = lo4;
        *reinterpret_cast<bf16x4*>(myV + (16 * pb + r) * PV + 16 * g + 8) = hi4;
      }
      bf16x8 vt[2];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) vt[tt] = tr_frag_small(myV, PV, 16 * tt, lane);
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        f32x4 s[2];
        float mt = -INFINITY;
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
          s[pb] = mfma32(kr[pb], qf[qt], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (n0 + 16 * pb + 4 * g + e >= n_hi) s[pb][e] = -INFINITY;
            mt = fmaxf(mt, s[pb][e]);
          }
        }
        mt = wave16_max(mt);
        const float mnew = fmaxf(mrow[qt], mt);
        const float alpha = __builtin_amdgcn_exp2f(mrow[qt] - mnew);
        float ls = 0.f;
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            s[pb][e] = __builtin_amdgcn_exp2f(s[pb][e] - mnew);
            ls += s[pb][e];
          }
        ls = wave16_sum(ls);
        lrow[qt] = lrow[qt] * alpha + ls;
        mrow[qt] = mnew;
        const bf16x8 pb8 = pack8(s[0], s[1]);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
          for (int e = 0; e < 4; ++e) ot[tt][qt][e] *= alpha;
          ot[tt][qt] = mfma32(vt[tt], pb8, ot[tt][qt]);
        }
      }
    }
    lds_barrier();                       // B1: Kp / Vp tiles complete (X tile k consumed)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 512 * i, row = c >> 5, ch = c & 31;
      if (row < nlive) {
        const int64_t o = ((int64_t)b * a.N + n0 + row) * D + ch * 8;
        *reinterpret_cast<uint4*>(aa.KpO + o) = *reinterpret_cast<const uint4*>(sK + oC + 8192 * i);
        *reinterpret_cast<uint4*>(aa.VpO + o) = *reinterpret_cast<const uint4*>(sV + oC + 8192 * i);
      }
    }
  }
  const int64_t pb0 = ((int64_t)b * a.S + sp);
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int q = 16 * qt + r;
    if (q < a.m) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
        *reinterpret_cast<float4*>(a.Op + (pb0 * a.m + q) * D + 32 * j + 16 * tt + 4 * g) =
            float4{ot[tt][qt][0], ot[tt][qt][1], ot[tt][qt][2], ot[tt][qt][3]};
      if (g == 0) {
        a.Mp[(pb0 * H + j) * MQ + q] = mrow[qt];
        a.Lp[(pb0 * H + j) * MQ + q] = lrow[qt];
      }
    }
  }
}

// backward.  Orientation A (points on accumulator rows, as the forward): P^T, dS^T -> the set's
// dQp_h^T[f][q] += Kp_h^T[f][pt] dS^T[pt][q] (Kp^T through the LDS tile).  Orientation B
// (queries on accumulator rows: S = Qp_h Kp_h^T recomputed with one more MFMA - the per-lane
// Kp row registers serve as A operand of one and B operand of the other) -> dVp^T[f][pt] =
// dO_h^T[f][q] P[q][pt], dKp^T[f][pt] = Qp_h^T[f][q] dS[q][pt] with P / dS as B operands straight
// from the accumulators; both leave as 8-byte bf16 stores.
template <int D, int QT>
__global__ __launch_bounds__(64 * (D / 32)) void k_fq_attn_bwd(const FqArgs a) {
  constexpr int PV = 72, H = D / 32, MQ = 16 * QT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, j = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int b = blockIdx.x, sp = blockIdx.y;
  char* myK = smem + j * 32 * PV;
  const int per = (int)(((int64_t)(a.N + 31) / 32 + a.S - 1) / a.S) * 32;
  int len = a.N;
  if (a.lengths != nullptr) len = a.lengths[b] < a.N ? a.lengths[b] : a.N;
  const int n_lo = sp * per;
  const int n_hi = (n_lo + per < a.N) ? n_lo + per : a.N;          // rows written (zeros past len)
  // operands of head j.  qs = sl2e Qp (scores in the log2 domain), qn = Qp (for dKp), do = dO
  bf16x8 qs[QT], dof[QT];
  // A operands [row = f][k = q] of the products that sum over the queries:
  //   m > 16: 16x16x32, k-slot 8 g + i <-> query perm32(8 g + i) (pack8 order of the B operand)
  //   m <= 16: 16x16x16, k-slot 4 g + e <-> query 4 g + e
  bf16x8 qnT[2], doT[2];
  bf16x4 qn4[2], do4[2];
  float lse_c[QT], del_c[QT];             // per column q = 16 qt + r        (orientation A)
  float lse_r[QT][4], del_r[QT][4];       // per row q = 16 qt + 4 g + e      (orientation B)
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int q = 16 * qt + r;
    qs[qt] = q_frag(a.Qp, D, a.m, q, j, g, a.scale_log2e);
    dof[qt] = q_frag(a.dOa + (int64_t)b * a.m * D, D, a.m, q, j, g, 1.0f);
    lse_c[qt] = q < a.m ? a.LSE[((int64_t)b * H + j) * MQ + q] : 1.0e30f;
    del_c[qt] = q < a.m ? a.Delta[((int64_t)b * H + j) * MQ + q] : 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int qq = 16 * qt + 4 * g + e;
      lse_r[qt][e] = qq < a.m ? a.LSE[((int64_t)b * H + j) * MQ + qq] : 1.0e30f;
      del_r[qt][e] = qq < a.m ? a.Delta[((int64_t)b * H + j) * MQ + qq] : 0.f;
    }
  }
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int f = 32 * j + 16 * tt + r;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int kq = perm32(8 * g + i);
      const bool ok = QT == 2 && kq < a.m;
      qnT[tt][i] = (__bf16)(ok ? a.Qp[(int64_t)kq * D + f] : 0.f);
      doT[tt][i] = (__bf16)(ok ? a.dOa[((int64_t)b * a.m + kq) * D + f] : 0.f);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int kq = 4 * g + e;
      const bool ok = QT == 1 && kq < a.m;
      qn4[tt][e] = (__bf16)(ok ? a.Qp[(int64_t)kq * D + f] : 0.f);
      do4[tt][e] = (__bf16)(ok ? a.dOa[((int64_t)b * a.m + kq) * D + f] : 0.f);
    }
  }
  f32x4 dq[2][QT];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) dq[tt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int n0 = n_lo; n0 < n_hi; n0 += 32) {
    bf16x8 kr[2], vr[2];
    bool key_c[2];                        // orientation B: column = point 16 pb + r
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
      const int n = n0 + 16 * pb + r;
      key_c[pb] = n < len;
      {
        const int64_t o = ((int64_t)b * a.N + (n < n_hi ? n : n_hi - 1)) * D + 32 * j + 8 * g;
        kr[pb] = *reinterpret_cast<const bf16x8*>(a.Kp + o);
        vr[pb] = *reinterpret_cast<const bf16x8*>(a.Vp + o);
        if (n >= n_hi) {
#pragma unroll
          for (int e = 0; e < 8; ++e) { kr[pb][e] = (__bf16)0.f; vr[pb][e] = (__bf16)0.f; }
        }
      }
      {
        bf16x4 lo4, hi4;
#pragma unroll
        for (int e = 0; e < 4; ++e) { lo4[e] = kr[pb][e]; hi4[e] = kr[pb][4 + e]; }
        *reinterpret_cast<bf16x4*>(myK + (16 * pb + r) * PV + 16 * g) = lo4;
        *reinterpret_cast<bf16x4*>(myK + (16 * pb + r) * PV + 16 * g + 8) = hi4;
      }
    }
    bf16x8 kt[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) kt[tt] = tr_frag_small(myK, PV, 16 * tt, lane);
    // ---- orientation A: dQp ----
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      f32x4 ds[2];
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 sv = mfma32(kr[pb], qs[qt], z);
        const f32x4 da = mfma32(vr[pb], dof[qt], z);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool key = n0 + 16 * pb + 4 * g + e < len;
          const float p = key ? __builtin_amdgcn_exp2f(sv[e] - lse_c[qt]) : 0.f;
          ds[pb][e] = p * (da[e] - del_c[qt]) * a.scale;
        }
      }
      const bf16x8 dsb = pack8(ds[0], ds[1]);
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) dq[tt][qt] = mfma32(kt[tt], dsb, dq[tt][qt]);
    }
    // ---- orientation B: dKp, dVp ----
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
      f32x4 pq[QT], dsq[QT];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 sv = mfma32(qs[qt], kr[pb], z);          // rows q, column pt
        const f32x4 da = mfma32(dof[qt], vr[pb], z);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = key_c[pb] ? __builtin_amdgcn_exp2f(sv[e] - lse_r[qt][e]) : 0.f;
          pq[qt][e] = p;
          dsq[qt][e] = p * (da[e] - del_r[qt][e]) * a.scale;
        }
      }
      const int n = n0 + 16 * pb + r;
      if (n < n_hi) {
        const int64_t o = ((int64_t)b * a.N + n) * D + 32 * j;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          f32x4 dv = {0.f, 0.f, 0.f, 0.f}, dk = {0.f, 0.f, 0.f, 0.f};
          if (QT == 2) {
            dv = mfma32(doT[tt], pack8(pq[0], pq[QT - 1]), dv);
            dk = mfma32(qnT[tt], pack8(dsq[0], dsq[QT - 1]), dk);
          } else {
            dv = mfma16(do4[tt], pack4(pq[0]), dv);
            dk = mfma16(qn4[tt], pack4(dsq[0]), dk);
          }
          *reinterpret_cast<bf16x4*>(a.dVp + o + 16 * tt + 4 * g) = pack4(dv);
          *reinterpret_cast<bf16x4*>(a.dKp + o + 16 * tt + 4 * g) = pack4(dk);
        }
      }
    }
  }
  const int64_t pb0 = ((int64_t)b * a.S + sp);
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int q = 16 * qt + r;
    if (q < a.m) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
        *reinterpret_cast<float4*>(a.dQpPart + (pb0 * a.m + q) * D + 32 * j + 16 * tt + 4 * g) =
            float4{dq[tt][qt][0], dq[tt][qt][1], dq[tt][qt][2], dq[tt][qt][3]};
    }
  }
}

// k_fq_attn_bwd2 (m = 32, d = 256): the same arithmetic as k_fq_attn_bwd with full-line global traffic.
// The workgroup streams whole [32 keys][256] tiles of Kp and Vp in
// by LDS-DMA (double buffered), each wave (= head) reads its 64-byte slices from LDS, writes its
// slices of the dKp / dVp tiles to LDS, and the two tiles leave in 16-byte pieces of full rows -
// the per-wave form reads 16 rows x 64 bytes per load instruction and writes 8-byte pieces.
__global__ __launch_bounds__(512, 2) void k_fq_attn_bwd2(const FqArgs a) {
  constexpr int D = 256, QT = 2, PV = 72, H = D / 32, MQ = 16 * QT;
  constexpr int ROWB = D * 2, TILEB = 32 * ROWB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sKb = smem;                        // [2][TILEB]
  char* sVb = smem + 2 * TILEB;            // [2][TILEB]
  char* sDK = smem + 4 * TILEB;            // dKp tile
  char* sDV = smem + 5 * TILEB;            // dVp tile
  const int tid = threadIdx.x, lane = tid & 63;
  const int j = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int b = blockIdx.x, sp = blockIdx.y;
  char* myK = smem + 6 * TILEB + j * 32 * PV;
  const int per = (int)(((int64_t)(a.N + 31) / 32 + a.S - 1) / a.S) * 32;
  int len = a.N;
  if (a.lengths != nullptr) len = a.lengths[b] < a.N ? a.lengths[b] : a.N;
  const int n_lo = sp * per;
  const int n_hi = (n_lo + per < a.N) ? n_lo + per : a.N;
  const int T = n_lo < n_hi ? (n_hi - n_lo + 31) / 32 : 0;
  bf16x8 qs[QT], dof[QT], qnT[2], doT[2];
  float lse_c[QT], del_c[QT], lse_r[QT][4], del_r[QT][4];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int q = 16 * qt + r;
    qs[qt] = q_frag(a.Qp, D, a.m, q, j, g, a.scale_log2e);
    dof[qt] = q_frag(a.dOa + (int64_t)b * a.m * D, D, a.m, q, j, g, 1.0f);
    lse_c[qt] = q < a.m ? a.LSE[((int64_t)b * H + j) * MQ + q] : 1.0e30f;
    del_c[qt] = q < a.m ? a.Delta[((int64_t)b * H + j) * MQ + q] : 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int qq = 16 * qt + 4 * g + e;
      lse_r[qt][e] = qq < a.m ? a.LSE[((int64_t)b * H + j) * MQ + qq] : 1.0e30f;
      del_r[qt][e] = qq < a.m ? a.Delta[((int64_t)b * H + j) * MQ + qq] : 0.f;
    }
  }
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int f = 32 * j + 16 * tt + r;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int kq = perm32(8 * g + i);
      const bool ok = kq < a.m;
      qnT[tt][i] = (__bf16)(ok ? a.Qp[(int64_t)kq * D + f] : 0.f);
      doT[tt][i] = (__bf16)(ok ? a.dOa[((int64_t)b * a.m + kq) * D + f] : 0.f);
    }
  }
  f32x4 dq[2][QT];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) dq[tt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // this lane's pieces of a tile: the head's 16 bytes of row r (natural chunk 4 j + g), its
  // accumulator-layout 8 bytes (features 32 j + 16 t + 4 g), the coalesced 16-byte piece
  int oK, oD[2];
  oK = swz(r, 4 * j + g, ROWB);
#pragma unroll
  for (int t = 0; t < 2; ++t) oD[t] = swz(r, 4 * j + 2 * t + (g >> 1), ROWB) + 8 * (g & 1);
  const int oC = swz(tid >> 5, tid & 31, ROWB);
  auto dma = [&](int k) {                 // tile k of Kp and Vp (issued from inline asm: k_isab1_fwd256)
    const int n0 = n_lo + 32 * k, par = k & 1;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const __bf16* base = w == 0 ? a.Kp : a.Vp;
      char* dst = (w == 0 ? sKb : sVb) + par * TILEB;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int p = (2 * j + i) * 64 + lane;
        const int row = p >> 5, slot = p & 31;
        const int ch = (slot & ~15) | ((slot ^ row) & 15);
        const int n = n0 + row < a.N ? n0 + row : a.N - 1;
        const __bf16* src = base + ((int64_t)b * a.N + n) * D + ch * 8;
        lds_dma16(src, dst + (2 * j + i) * 1024);
      }
    }
  };
  if (T > 0) dma(0);
  for (int k = 0; k < T; ++k) {
    const int par = k & 1, n0 = n_lo + 32 * k, nlive = n_hi - n0;
    const char* sK = sKb + par * TILEB;
    const char* sV = sVb + par * TILEB;
    // tile k + 1 starts to stream in; this tile's DMA (one iteration old) must have landed: younger
    // are the 4 pieces just issued and the 4 stores of tile k - 1 (always a full tile)
    if (k + 1 < T) {
      dma(k + 1);
      if (k == 0) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    lds_barrier();                       // B0: Kp / Vp tiles complete; previous output tiles stored
    bf16x8 kr[2], vr[2];
    bool key_c[2];
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
      const int n = n0 + 16 * pb + r;
      key_c[pb] = n < len;
      kr[pb] = *reinterpret_cast<const bf16x8*>(sK + oK + 8192 * pb);
      vr[pb] = *reinterpret_cast<const bf16x8*>(sV + oK + 8192 * pb);
      if (n >= n_hi) {                     // rows past the range: the DMA fetched a duplicate
#pragma unroll
        for (int e = 0; e < 8; ++e) { kr[pb][e] = (__bf16)0.f; vr[pb][e] = (__bf16)0.f; }
      }
      bf16x4 lo4, hi4;
#pragma unroll
      for (int e = 0; e < 4; ++e) { lo4[e] = kr[pb][e]; hi4[e] = kr[pb][4 + e]; }
      *reinterpret_cast<bf16x4*>(myK + (16 * pb + r) * PV + 16 * g) = lo4;
      *reinterpret_cast<bf16x4*>(myK + (16 * pb + r) * PV + 16 * g + 8) = hi4;
    }
    bf16x8 kt[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) kt[tt] = tr_frag_small(myK, PV, 16 * tt, lane);
    // ---- orientation A: dQp ----
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      f32x4 ds[2];
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 sv = mfma32(kr[pb], qs[qt], z);
        const f32x4 da = mfma32(vr[pb], dof[qt], z);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool key = n0 + 16 * pb + 4 * g + e < len;
          const float p = key ? __builtin_amdgcn_exp2f(sv[e] - lse_c[qt]) : 0.f;
          ds[pb][e] = p * (da[e] - del_c[qt]) * a.scale;
        }
      }
      const bf16x8 dsb = pack8(ds[0], ds[1]);
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) dq[tt][qt] = mfma32(kt[tt], dsb, dq[tt][qt]);
    }
    // ---- orientation B: dKp, dVp -> own slices of the output tiles ----
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
      f32x4 pq[QT], dsq[QT];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 sv = mfma32(qs[qt], kr[pb], z);          // rows q, column pt
        const f32x4 da = mfma32(dof[qt], vr[pb], z);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = key_c[pb] ? __builtin_amdgcn_exp2f(sv[e] - lse_r[qt][e]) : 0.f;
          pq[qt][e] = p;
          dsq[qt][e] = p * (da[e] - del_r[qt][e]) * a.scale;
        }
      }
      const bf16x8 pb8 = pack8(pq[0], pq[1]), ds8 = pack8(dsq[0], dsq[1]);
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 dv = mfma32(doT[tt], pb8, z);
        const f32x4 dk = mfma32(qnT[tt], ds8, z);
        *reinterpret_cast<bf16x4*>(sDV + oD[tt] + 8192 * pb) = pack4(dv);
        *reinterpret_cast<bf16x4*>(sDK + oD[tt] + 8192 * pb) = pack4(dk);
      }
    }
    lds_barrier();                       // B1: dKp / dVp tiles complete
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 512 * i, row = c >> 5, ch = c & 31;
      if (row < nlive) {
        const int64_t o = ((int64_t)b * a.N + n0 + row) * D + ch * 8;
        *reinterpret_cast<uint4*>(a.dKp + o) = *reinterpret_cast<const uint4*>(sDK + oC + 8192 * i);
        *reinterpret_cast<uint4*>(a.dVp + o) = *reinterpret_cast<const uint4*>(sDV + oC + 8192 * i);
      }
    }
  }
  const int64_t pb0 = ((int64_t)b * a.S + sp);
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int q = 16 * qt + r;
    if (q < a.m) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
        *reinterpret_cast<float4*>(a.dQpPart + (pb0 * a.m + q) * D + 32 * j + 16 * tt + 4 * g) =
            float4{dq[tt][qt][0], dq[tt][qt][1], dq[tt][qt][2], dq[tt][qt][3]};
    }
  }
}

// merge of the forward partials + residual: O[b][q][f] = Qp[q][f] + sum_s w_s Op_s / sum_s w_s L_s,
// LSE[b][h][q] = M + log2 L; Oa (= A Vp, for Delta) is O - Qp
__global__ __launch_bounds__(256) void k_fq_merge(const float* __restrict__ Op,
                                                  const float* __restrict__ Mp,
                                                  const float* __restrict__ Lp,
                                                  const float* __restrict__ Qp, int B, int S,
                                                  int m, int D, int MQ, float* __restrict__ O,
                                                  float* __restrict__ LSE) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * m * D) return;
  const int f = (int)(i % D);
  const int q = (int)((i / D) % m);
  const int64_t b = i / ((int64_t)D * m);
  const int H = D / 32, j = f / 32;
  float M = -INFINITY;
  for (int s = 0; s < S; ++s) M = fmaxf(M, Mp[((b * S + s) * H + j) * MQ + q]);
  float L = 0.f, t = 0.f;
  for (int s = 0; s < S; ++s) {
    const float ms = Mp[((b * S + s) * H + j) * MQ + q];
    if (ms == -INFINITY) continue;
    const float w = exp2f(ms - M);
    L += w * Lp[((b * S + s) * H + j) * MQ + q];
    t += w * Op[((b * S + s) * m + q) * D + f];
  }
  O[i] = Qp[(int64_t)q * D + f] + t / L;
  if ((f & 31) == 0) LSE[(b * H + j) * MQ + q] = M + log2f(L);
}

// Delta[b][h][q] = sum_{f in head} dO[b][q][f] (O[b][q][f] - Qp[q][f])
__global__ __launch_bounds__(256) void k_fq_delta(const float* __restrict__ dO,
                                                  const float* __restrict__ O,
                                                  const float* __restrict__ Qp, int B, int m,
                                                  int D, int MQ, float* __restrict__ Delta) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int H = D / 32;
  if (i >= (int64_t)B * H * m) return;
  const int q = (int)(i % m);
  const int j = (int)((i / m) % H);
  const int64_t b = i / ((int64_t)m * H);
  float t = 0.f;
  for (int f = 0; f < 32; ++f) {
    const int64_t o = (b * m + q) * D + 32 * j + f;
    t += dO[o] * (O[o] - Qp[(int64_t)q * D + 32 * j + f]);
  }
  Delta[(b * H + j) * MQ + q] = t;
}

// dOt[b][q][f] = dO[b][q][f] + sum_s dQpPart[b][s][q][f]   (gradient w.r.t. Qp of set b)
__global__ __launch_bounds__(256) void k_fq_dq_sum(const float* __restrict__ dO,
                                                   const float* __restrict__ part, int B, int S,
                                                   int md, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * md) return;
  const int64_t b = i / md, o = i - b * md;
  float t = dO[i];
  for (int s = 0; s < S; ++s) t += part[(b * S + s) * md + o];
  out[i] = t;
}

}  // namespace

// ---- launchers (declared in d256.hpp) ------------------------------------------------
int fq_splits256(int B, int N) {
  int S = 1;
  const int tiles = (int)cdiv(N, 32);
  while (S * 2 <= tiles && B * S < 1024 && S < 16) S *= 2;
  return S;
}
int fq_attn_fwd256(const __bf16* Kp, const __bf16* Vp, const float* Qp, int B, int N, int m,
                   const int32_t* lengths, float* Op, float* Mp, float* Lp, float* O, float* LSE,
                   hipStream_t st) {
  constexpr int D = 256;
  // (m > 16 has no attention-only forward: it goes through fq_proj_attn_fwd256, whose kernel projects the
  //  keys in the same pass)
  PCA_REQUIRE(m <= 16, "fq_attn_fwd256: m = %d (> 16: fq_proj_attn_fwd256)", m);
  const int S = fq_splits256(B, N), MQ = 16;
  FqArgs a{};
  a.Kp = Kp; a.Vp = Vp; a.Qp = Qp; a.Op = Op; a.Mp = Mp; a.Lp = Lp;
  a.B = B; a.N = N; a.m = m; a.S = S; a.lengths = lengths;
  a.scale = 1.0f / sqrtf((float)D);
  a.scale_log2e = LOG2E * a.scale;
  const size_t lds = (size_t)(D / 32) * 32 * 72;
  hipLaunchKernelGGL((k_fq_attn_fwd<D, 1>), dim3(B, S), dim3(512), lds, st, a);
  PCA_TRY(check_launch("k_fq_attn_fwd"));
  hipLaunchKernelGGL(k_fq_merge, dim3((unsigned)cdiv((int64_t)B * m * D, 256)), dim3(256), 0, st,
                     Op, Mp, Lp, Qp, B, S, m, D, MQ, O, LSE);
  return check_launch("k_fq_merge");
}
// fc_k / fc_v over the keys + the attention in one launch (k_fq_proj_fwd), then the merge; m = 32
int fq_proj_attn_fwd256(const __bf16* X, const __bf16* WkB, const __bf16* WvB, const float* bk,
                        const float* bv, const float* Qp, int B, int N, int m,
                        const int32_t* lengths, __bf16* Kp, __bf16* Vp, float* Op, float* Mp,
                        float* Lp, float* O, float* LSE, hipStream_t st, const float* inv_scale) {
  constexpr int D = 256;
  PCA_REQUIRE(m > 16 && m <= 32, "fq_proj_attn_fwd256: m = %d", m);
  int S2 = fq_splits256(B, N);
  while (S2 > 1 && B * S2 > 256) S2 /= 2;         // 98 KiB of LDS: one workgroup per CU
  FqProjArgs a{};
  a.f.Qp = Qp; a.f.Op = Op; a.f.Mp = Mp; a.f.Lp = Lp;
  a.f.B = B; a.f.N = N; a.f.m = m; a.f.S = S2; a.f.lengths = lengths;
  a.f.scale = 1.0f / sqrtf((float)D);
  a.f.scale_log2e = LOG2E * a.f.scale;
  a.X = X; a.WkB = WkB; a.WvB = WvB; a.bk = bk; a.bv = bv; a.KpO = Kp; a.VpO = Vp;
  a.inv_scale = inv_scale;
  allow_lds160<k_fq_proj_fwd<false>, k_fq_proj_fwd<true>>();
  const size_t lds = (size_t)5 * 32 * D * 2 + (size_t)(D / 32) * 32 * 72 +
                     (inv_scale != nullptr ? (size_t)32 * D : 0);
  if (inv_scale != nullptr) hipLaunchKernelGGL(k_fq_proj_fwd<true>, dim3(B, S2), dim3(512), lds, st, a);
  else hipLaunchKernelGGL(k_fq_proj_fwd<false>, dim3(B, S2), dim3(512), lds, st, a);
  PCA_TRY(check_launch("k_fq_proj_fwd"));
  hipLaunchKernelGGL(k_fq_merge, dim3((unsigned)cdiv((int64_t)B * m * D, 256)), dim3(256), 0, st,
                     Op, Mp, Lp, Qp, B, S2, m, D, 32, O, LSE);
  return check_launch("k_fq_merge");
}
int fq_attn_bwd256(const __bf16* Kp, const __bf16* Vp, const float* Qp, const float* dO,
                   const float* O, const float* LSE, float* Delta, int B, int N, int m,
                   const int32_t* lengths, __bf16* dKp, __bf16* dVp, float* dQpPart, float* dOt,
                   hipStream_t st) {
  constexpr int D = 256;
  const int S = fq_splits256(B, N), QT = m > 16 ? 2 : 1, MQ = 16 * QT;
  hipLaunchKernelGGL(k_fq_delta, dim3((unsigned)cdiv((int64_t)B * (D / 32) * m, 256)), dim3(256), 0,
                     st, dO, O, Qp, B, m, D, MQ, Delta);
  PCA_TRY(check_launch("k_fq_delta"));
  FqArgs a{};
  a.Kp = Kp; a.Vp = Vp; a.Qp = Qp; a.dOa = dO; a.LSE = LSE; a.Delta = Delta;
  a.dKp = dKp; a.dVp = dVp; a.dQpPart = dQpPart;
  a.B = B; a.N = N; a.m = m; a.S = S; a.lengths = lengths;
  a.scale = 1.0f / sqrtf((float)D);
  a.scale_log2e = LOG2E * a.scale;
  const size_t lds = (size_t)(D / 32) * 32 * 72;
  int S2 = S;
  if (QT == 2) {
    // full-line traffic through LDS tiles: 114 KiB per workgroup, one per CU - fewer point ranges
    // (the partial buffers are sized for S)
    while (S2 > 1 && B * S2 > 256) S2 /= 2;
    a.S = S2;
    allow_lds160<k_fq_attn_bwd2>();
    hipLaunchKernelGGL(k_fq_attn_bwd2, dim3(B, S2), dim3(512), (size_t)6 * 32 * D * 2 + lds, st, a);
  } else {          // m <= 16: the per-wave global-traffic form
    hipLaunchKernelGGL((k_fq_attn_bwd<D, 1>), dim3(B, S), dim3(512), lds, st, a);
  }
  PCA_TRY(check_launch("k_fq_attn_bwd"));
  hipLaunchKernelGGL(k_fq_dq_sum, dim3((unsigned)cdiv((int64_t)B * m * D, 256)), dim3(256), 0, st,
                     dO, dQpPart, B, S2, m * D, dOt);
  return check_launch("k_fq_dq_sum");
}

}  // namespace pca
