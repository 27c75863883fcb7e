// The per-set backward "mid" chain of an ISAB (see mid_bf16.hip) as a device function:
//   dKp / dVp = fixed-order sums of k_mab1_bwd's partials ; dH = dKp Wk + dVp Wv ; dZ = dH.[Z>0] ;
//   dO = dH + dZ Wo ; dT_h = dO_h Wv_h ; Delta = rowdot(dT, T)
// Shared by the stand-alone launch (k_mid_bwd) and by the few-queries backward kernels, which run it
// in their prologue - every workgroup of a set for itself, as the set-resident forward runs its mid
// stage - and take the dT / Delta / LSE images straight into their own LDS.  Same MFMAs
// on the same operands in the same summation order wherever it runs; only the sink of the images
// differs.  256 threads, wave w = head w; ONE workgroup barrier inside (every thread must call it).
// In a workgroup of NT > 256 threads (the set rows of k_mab0_small_ride, wgrad128.hip) waves 0-3 run the
// chain and the others only meet them at that barrier.
#pragma once
#include "blocks.hpp"
#include "mfma_common.hpp"

namespace pca {

struct MidBwdArgs {
  const float *dKpPart, *dVpPart;   // [B][nparts][16][128] fp32
  int nparts;
  float *dKp, *dVp;             // [B][16][128] fp32 sums (out)
  float* zero_ptr;
  int zero_n;
  const float *Z, *T, *LSE;     // saved by the forward
  const __bf16 *Wk1T, *Wv1T;    // [128][128] transposed natural:  W^T[c][f]
  const __bf16* Wo0TP;          // [128][128] transposed, K-permuted
  const __bf16* Wv0TP;          // [dk][128]  transposed, K-permuted (dk == 128)
  const __bf16* Wv0T;           // [dk][128]  transposed natural
  const float* Wv0f;            // fp32 [128][dk] for dk <= 4
  float *dZ, *dO;               // [B][16][128] fp32
  float* Th;                    // [4][B*16][dk] head-major copy of T
  float* dQs;                   // [16][128], atomically accumulated sum over sets of dO
  float* dTf;                   // [B][64][dk] fp32 (dk <= 4)
  __bf16 *dTb, *dTt;            // [B][64][128], [B][128][64]
  float *Delta, *LSEp;          // [B][64]
  int dk, B;
};

inline MidBwdArgs mid_bwd_args(const MidBwdLaunch& L) {
  MidBwdArgs a{};
  a.dKpPart = L.dKpPart; a.dVpPart = L.dVpPart; a.nparts = L.nparts; a.dKp = L.dKp;
  a.dVp = L.dVp; a.zero_ptr = L.zero_ptr; a.zero_n = L.zero_n; a.Z = L.Z; a.T = L.T; a.LSE = L.LSE; a.Wk1T = L.Wk1T;
  a.Wv1T = L.Wv1T; a.Wo0TP = L.Wo0TP; a.Wv0TP = L.Wv0TP; a.Wv0T = L.Wv0T; a.Wv0f = L.Wv0f;
  a.dZ = L.dZ; a.dO = L.dO; a.Th = L.Th; a.dQs = L.dQs; a.dTf = L.dTf; a.dTb = L.dTb;
  a.dTt = L.dTt; a.Delta = L.Delta; a.LSEp = L.LSEp; a.dk = L.dk; a.B = L.B;
  return a;
}

// LDS of the chain: dKp, dVp bf16 [q][f] (4 KiB each), per wave dO_j bf16 [q][32] (4 x 1 KiB), and
// the staged Wk1^T / Wv1^T (32 KiB each)
constexpr int MID_BWD_SMALL_LDS = 3 * 16 * 256;
constexpr int MID_BWD_W_LDS = 128 * 256;
struct MidBwdLds {
  char *sK, *sV, *sO, *sWk, *sWv;
};

// sink of the stand-alone kernel: the images in global memory, where the next launch reads them
struct MidSinkGlobal {
  const MidBwdArgs& a;
  int b;
  // columns 16ct + 4g .. +3 of row `row` (= 16w + r) of dT
  __device__ __forceinline__ void dTb(int row, int ct, int g, bf16x4 v) const {
    *reinterpret_cast<bf16x4*>(a.dTb + ((int64_t)b * 64 + row) * 128 + 16 * ct + 4 * g) = v;
  }
  // queries 4g .. 4g+3 of head w at column 16ct + r: the r-permuted transposed image
  __device__ __forceinline__ void dTt(int ct, int r, int w, int g, bf16x4 v) const {
    *reinterpret_cast<bf16x4*>(a.dTt + ((int64_t)b * 128 + 16 * ct + r) * 64 + 32 * (w >> 1) +
                               8 * g + 4 * (w & 1)) = v;
  }
  __device__ __forceinline__ void dTf(int row, int c, float v) const {
    a.dTf[((int64_t)b * 64 + row) * a.dk + c] = v;
  }
  __device__ __forceinline__ void stat(int row, float delta, float lse) const {
    a.Delta[(int64_t)b * 64 + row] = delta;
    a.LSEp[(int64_t)b * 64 + row] = lse;
  }
};

// wr: this workgroup also writes what later launches read from global memory (dKp, dVp, dZ, dO, Th)
template <bool SMALL, int NT = 256, class Sink>
__device__ __forceinline__ void mid_bwd_body(const MidBwdArgs& a, int b, const MidBwdLds& m,
                                             bool wr, const Sink& sink) {
  static_assert(NT >= 256 && NT % 64 == 0, "mid_bwd_body: four waves run the chain");
  constexpr int D = 128, MQ = 16, ROWB = 256;
  // wave-uniform: this wave takes part (always, in the 256-thread callers)
  const bool on = NT == 256 || threadIdx.x < 256;
  char* const sK = m.sK;
  char* const sV = m.sV;
  char* const sWk = m.sWk;
  char* const sWv = m.sWv;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int dk = a.dk;
  char* const sOw = m.sO + w * 16 * 64;

  // what the second half takes from the first in registers
  float4 zpre[8];
  bf16x8 wo_pre[2][4];
  bf16x8 wvp_pre[SMALL ? 1 : 8], wvt_pre[SMALL ? 1 : 8];
  float4 t_pre[SMALL ? 1 : 8];
  float wvf_pre[SMALL ? 4 : 1][8], ts_pre[SMALL ? 4 : 1];
  float lse_pre;
  if (on) {
    // every wave needs ALL of Wk1^T and Wv1^T: stage them once, cooperatively (coalesced,
    // 16 loads of 16 B in flight per thread) instead of 4 waves chasing fragments through L2
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = tid + 256 * e;                 // 2048 chunks of 16 B per matrix
      const int row = c >> 4, ch = c & 15;
      const uint4 kv = *reinterpret_cast<const uint4*>(a.Wk1T + (int64_t)row * D + ch * 8);
      const uint4 vv = *reinterpret_cast<const uint4*>(a.Wv1T + (int64_t)row * D + ch * 8);
      *reinterpret_cast<uint4*>(sWk + swz(row, ch, ROWB)) = kv;
      *reinterpret_cast<uint4*>(sWv + swz(row, ch, ROWB)) = vv;
    }
    // Every global operand of the chain below is fetched NOW, before the first barrier: the
    // chain is purely latency-bound, so the round trips must overlap instead of queueing behind
    // each other.
    const int64_t trow = (int64_t)b * 64 + 16 * w + r;           // this lane's query row of T
#pragma unroll
    for (int t = 0; t < 8; ++t)
      zpre[t] = *reinterpret_cast<const float4*>(a.Z + ((int64_t)b * MQ + r) * D + 16 * t + 4 * g);
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4)
        wo_pre[tt][s4] = gload8(a.Wo0TP + (int64_t)(16 * (2 * w + tt) + r) * D + 32 * s4 + 8 * g);
    if (SMALL) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        ts_pre[c] = c < dk ? a.T[trow * dk + c] : 0.f;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            wvf_pre[c][4 * tt + e] =
                c < dk ? a.Wv0f[(32 * w + 16 * tt + 4 * g + e) * dk + c] : 0.f;
      }
    } else {
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) {
        wvp_pre[ct] = gload8(a.Wv0TP + (int64_t)(16 * ct + r) * D + 32 * w + 8 * g);
        wvt_pre[ct] = gload8(a.Wv0T + (int64_t)(16 * ct + r) * D + 32 * w + 8 * g);
        t_pre[ct] = *reinterpret_cast<const float4*>(a.T + trow * D + 16 * ct + 4 * g);
      }
    }
    lse_pre = a.LSE[(int64_t)b * 64 + 16 * w + r];
    for (int i = tid; i < 16 * 16; i += 256) {
      const int row = i >> 4, ch = i & 15;
      float k[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      // four partials at a time, their loads issued together (one round trip per group, not per
      // partial); same summation order
      for (int p0 = 0; p0 < a.nparts; p0 += 4) {
        float4 k0[4], k1[4], v0[4], v1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int pp = p0 + u < a.nparts ? p0 + u : p0;
          const int64_t off = (((int64_t)b * a.nparts + pp) * MQ + row) * D + ch * 8;
          const float4* pk = reinterpret_cast<const float4*>(a.dKpPart + off);
          const float4* pv = reinterpret_cast<const float4*>(a.dVpPart + off);
          k0[u] = pk[0]; k1[u] = pk[1]; v0[u] = pv[0]; v1[u] = pv[1];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (p0 + u >= a.nparts) continue;
          k[0] += k0[u].x; k[1] += k0[u].y; k[2] += k0[u].z; k[3] += k0[u].w;
          k[4] += k1[u].x; k[5] += k1[u].y; k[6] += k1[u].z; k[7] += k1[u].w;
          v[0] += v0[u].x; v[1] += v0[u].y; v[2] += v0[u].z; v[3] += v0[u].w;
          v[4] += v1[u].x; v[5] += v1[u].y; v[6] += v1[u].z; v[7] += v1[u].w;
        }
      }
      if (wr) {
        const int64_t so = ((int64_t)b * MQ + row) * D + ch * 8;
        reinterpret_cast<float4*>(a.dKp + so)[0] = float4{k[0], k[1], k[2], k[3]};
        reinterpret_cast<float4*>(a.dKp + so)[1] = float4{k[4], k[5], k[6], k[7]};
        reinterpret_cast<float4*>(a.dVp + so)[0] = float4{v[0], v[1], v[2], v[3]};
        reinterpret_cast<float4*>(a.dVp + so)[1] = float4{v[4], v[5], v[6], v[7]};
      }
      bf16x8 kb, vb;
#pragma unroll
      for (int e = 0; e < 8; ++e) { kb[e] = (__bf16)k[e]; vb[e] = (__bf16)v[e]; }
      *reinterpret_cast<bf16x8*>(sK + swz(row, ch, ROWB)) = kb;
      *reinterpret_cast<bf16x8*>(sV + swz(row, ch, ROWB)) = vb;
    }
  }
  __syncthreads();
  if (!on) return;

  // ---- dH^T (all 8 feature tiles, every wave: avoids a cross-wave exchange) ----
  bf16x8 kb[4], vb[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    kb[ks] = *reinterpret_cast<const bf16x8*>(sK + swz(r, 4 * ks + g, ROWB));
    vb[ks] = *reinterpret_cast<const bf16x8*>(sV + swz(r, 4 * ks + g, ROWB));
  }
  f32x4 dh[8], dz[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    dh[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      dh[t] = mfma32(*reinterpret_cast<const bf16x8*>(sWk + swz(16 * t + r, 4 * ks + g, ROWB)),
                     kb[ks], dh[t]);
      dh[t] = mfma32(*reinterpret_cast<const bf16x8*>(sWv + swz(16 * t + r, 4 * ks + g, ROWB)),
                     vb[ks], dh[t]);
    }
    const int64_t off = ((int64_t)b * MQ + r) * D + 16 * t + 4 * g;
    const float4 z4 = zpre[t];
    dz[t][0] = z4.x > 0.f ? dh[t][0] : 0.f;
    dz[t][1] = z4.y > 0.f ? dh[t][1] : 0.f;
    dz[t][2] = z4.z > 0.f ? dh[t][2] : 0.f;
    dz[t][3] = z4.w > 0.f ? dh[t][3] : 0.f;
    if (wr && (t >> 1) == w)
      *reinterpret_cast<float4*>(a.dZ + off) = float4{dz[t][0], dz[t][1], dz[t][2], dz[t][3]};
  }

  // ---- dO^T tiles of head w ----
  f32x4 dO2[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  // select this wave's two tiles without dynamic register indexing
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    if (t == 2 * w) dO2[0] = dh[t];
    if (t == 2 * w + 1) dO2[1] = dh[t];
  }
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int t = 2 * w + tt;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      dO2[tt] = mfma32(wo_pre[tt][s], pack8(dz[2 * s], dz[2 * s + 1]), dO2[tt]);
    const int64_t off = ((int64_t)b * MQ + r) * D + 16 * t + 4 * g;
    if (wr)
      *reinterpret_cast<float4*>(a.dO + off) =
          float4{dO2[tt][0], dO2[tt][1], dO2[tt][2], dO2[tt][3]};
    // (the sum of dO over the sets is taken by k_mab0_post1: B workgroups adding atomically
    //  into the same 2048 addresses serialised for microseconds)
    // wave-private [q][32] image of dO_w (64-byte rows): feature 16tt+4g.. of query r
    *reinterpret_cast<bf16x4*>(sOw + r * 64 + (16 * tt + 4 * g) * 2) = pack4(dO2[tt]);
  }

  // ---- dT of head w (rows 16w .. 16w+15 of the [64][dk] tensor) and Delta ----
  float dl = 0.f;
  if (SMALL) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c >= dk) break;
      float part = 0.f;
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int e = 0; e < 4; ++e) part += dO2[tt][e] * wvf_pre[c][4 * tt + e];
      part = wave16_sum(part);
      const float tv = ts_pre[c];
      if (g == 0) {
        sink.dTf(16 * w + r, c, part);
        if (wr) a.Th[((int64_t)w * a.B * MQ + (int64_t)b * MQ + r) * dk + c] = tv;
      }
      // (every g-lane holds the full dT after the reduction: dl is complete in each of them)
      dl += part * tv;
    }
  } else {
    const bf16x8 dob = pack8(dO2[0], dO2[1]);
    // query-row operand for the second orientation: dO_w[q][f], f natural, from the image
    const bf16x8 doa = *reinterpret_cast<const bf16x8*>(sOw + r * 64 + 16 * g);
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) {
      // (1) rows = columns c of dT, col = query: natural-row image + Delta
      f32x4 t1 = {0.f, 0.f, 0.f, 0.f};
      t1 = mfma32(wvp_pre[ct], dob, t1);
      sink.dTb(16 * w + r, ct, g, pack4(t1));
      const float4 tv = t_pre[ct];
      dl += t1[0] * tv.x + t1[1] * tv.y + t1[2] * tv.z + t1[3] * tv.w;
      if (wr)
        *reinterpret_cast<float4*>(a.Th + ((int64_t)w * a.B * MQ + (int64_t)b * MQ + r) * D +
                                   16 * ct + 4 * g) = tv;
      // (2) rows = queries 4g+e, col = column c = 16ct + r: the r-permuted transposed image
      f32x4 t2 = {0.f, 0.f, 0.f, 0.f};
      t2 = mfma32(doa, wvt_pre[ct], t2);
      sink.dTt(ct, r, w, g, pack4(t2));
    }
    dl = wave16_sum(dl);
  }
  if (g == 0) sink.stat(16 * w + r, dl, lse_pre);
}

}  // namespace pca
