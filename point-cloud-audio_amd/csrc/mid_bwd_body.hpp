// The per-set backward "mid" chain of an ISAB (see mid_bf16.hip) as a device function:
//   dKp / dVp = fixed-order sums of k_mab1_bwd's partials ; dH = dKp Wk + dVp Wv ; dZ = dH.[Z>0] ;
//   dO = dH + dZ Wo ; dT_h = dO_h Wv_h ; Delta = rowdot(dT, T)
// Shared by the stand-alone launch (k_mid_bwd) and by the few-queries backward kernels, which run it
// in their prologue - every workgroup of a set for itself, as the set-resident forward runs its mid
// stage - and take the dT / Delta / LSE images straight into their own LDS.  Same MFMAs
// on the same operands in the same summation order wherever it runs; only the sink of the images
// differs.  256 threads, wave w = head w = feature tiles 2w, 2w + 1 of dH; TWO workgroup barriers inside
// (every thread must call both): one behind the partial sums, one behind the exchange of the masked dZ
// tiles.  In a workgroup of NT > 256 threads (the set rows of k_mab0_small_ride, wgrad128.hip) waves 0-3
// run the chain and the others only meet them at those barriers.
#pragma once
#include "blocks.hpp"
#include "mfma_common.hpp"
#ifdef PCA_DEBUG_CLOCKS
#include <stdlib.h>
#endif

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
#ifdef PCA_DEBUG_CLOCKS
  long long* dbg;               // phase stamps of set dbg_set (PCA_DBG_WG), written by the carrying kernel
  int dbg_set;
#endif
};

#ifdef PCA_DEBUG_CLOCKS
// diagnostic build: host-visible stamp buffers (0: the wide carrier, layer 2; 1: the small carrier, layer 1),
// the last launch's stamps printed at exit (mid_bf16.hip)
long long* mid_debug_clock_buffer(int which);
#endif

inline MidBwdArgs mid_bwd_args(const MidBwdLaunch& L) {
  MidBwdArgs a{};
  a.dKpPart = L.dKpPart; a.dVpPart = L.dVpPart; a.nparts = L.nparts; a.dKp = L.dKp;
  a.dVp = L.dVp; a.zero_ptr = L.zero_ptr; a.zero_n = L.zero_n; a.Z = L.Z; a.T = L.T; a.LSE = L.LSE; a.Wk1T = L.Wk1T;
  a.Wv1T = L.Wv1T; a.Wo0TP = L.Wo0TP; a.Wv0TP = L.Wv0TP; a.Wv0T = L.Wv0T; a.Wv0f = L.Wv0f;
  a.dZ = L.dZ; a.dO = L.dO; a.Th = L.Th; a.dQs = L.dQs; a.dTf = L.dTf; a.dTb = L.dTb;
  a.dTt = L.dTt; a.Delta = L.Delta; a.LSEp = L.LSEp; a.dk = L.dk; a.B = L.B;
#ifdef PCA_DEBUG_CLOCKS
  a.dbg = mid_debug_clock_buffer(L.dk <= 4 ? 1 : 0);
  a.dbg_set = getenv("PCA_DBG_WG") ? atoi(getenv("PCA_DBG_WG")) : 0;
#endif
  return a;
}

// LDS of the chain: dKp, dVp bf16 [q][f] (4 KiB each), per wave dO_j bf16 [q][32] (4 x 1 KiB), and the
// masked dZ tiles as the four B operands of the dO MFMAs ([s][lane] 16 B: wave s writes operand s, every
// wave reads all four)
constexpr int MID_BWD_SMALL_LDS = 4 * 16 * 256;
struct MidBwdLds {
  char *sK, *sV, *sO, *sDz;
};
inline __device__ MidBwdLds mid_bwd_lds(char* base) {
  return MidBwdLds{base, base + 16 * 256, base + 2 * 16 * 256, base + 3 * 16 * 256};
}

// Phase stamps of the chain (-DPCA_DEBUG_CLOCKS, a diagnostic build): kept in scalar registers by the
// caller, which passes its array and writes it once at the end.  0 entry (caller), 1 all requests issued,
// 2 partials summed, 3 barrier passed, 4 dH done, 5 images written, 6 first tile of the main loop (caller).
#ifdef PCA_DEBUG_CLOCKS
#define PCA_MID_STAMP(i)                                \
  do {                                                  \
    __builtin_amdgcn_sched_barrier(0);                  \
    if (stamps != nullptr) stamps[i] = wall_clock64();  \
    __builtin_amdgcn_sched_barrier(0);                  \
  } while (0)
// thread 0 of the workgroup that carries set a.dbg_set: the seven stamps, tagged with their index
#define PCA_MID_STAMPS_WRITE(a, b, first)                                                           \
  do {                                                                                              \
    if ((a).dbg != nullptr && (b) == (a).dbg_set && (first) && threadIdx.x == 0)                    \
      for (int i_ = 0; i_ < 7; ++i_) (a).dbg[i_] = ((long long)i_ << 48) | (stamps[i_] & 0xffffffffffffLL); \
  } while (0)
#else
#define PCA_MID_STAMP(i) do {} while (0)
#define PCA_MID_STAMPS_WRITE(a, b, first) do {} while (0)
#endif
// a carrying kernel: PCA_MID_STAMPS_DECL at its entry (stamp 0), PCA_MID_STAMPS_ARG behind the sink in the
// call of mid_bwd_body, PCA_MID_STAMP(6) where its main loop starts, PCA_MID_STAMPS_WRITE at its end
#ifdef PCA_DEBUG_CLOCKS
#define PCA_MID_STAMPS_DECL                        \
  long long stamp_[7] = {0, 0, 0, 0, 0, 0, 0};     \
  long long* const stamps = stamp_;                \
  PCA_MID_STAMP(0)
#define PCA_MID_STAMPS_ARG , stamps
#else
#define PCA_MID_STAMPS_DECL do {} while (0)
#define PCA_MID_STAMPS_ARG
#endif

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
                                             bool wr, const Sink& sink, long long* stamps = nullptr) {
  static_assert(NT >= 256 && NT % 64 == 0, "mid_bwd_body: four waves run the chain");
  constexpr int D = 128, MQ = 16, ROWB = 256;
  // wave-uniform: this wave takes part (always, in the 256-thread callers)
  const bool on = NT == 256 || threadIdx.x < 256;
  char* const sK = m.sK;
  char* const sV = m.sV;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int dk = a.dk;
  char* const sOw = m.sO + w * 16 * 64;
  char* const sDz = m.sDz;
  const int nparts = a.nparts;

  // what the later stages take from the first in registers
  float4 zpre[2];
  bf16x8 wk_pre[2][4], wv_pre[2][4];
  bf16x8 wo_pre[2][4];
  bf16x8 wvp_pre[SMALL ? 1 : 8], wvt_pre[SMALL ? 1 : 8];
  float4 t_pre[SMALL ? 1 : 8];
  float wvf_pre[SMALL ? 4 : 1][8], ts_pre[SMALL ? 4 : 1];
  float lse_pre;
  if (on) {
    // The chain is a dependent sequence of small steps, so EVERY global operand of it is requested here,
    // in one go, before anything waits for any of them: nothing is consumed, and no LDS store stands,
    // between two requests (a store of a loaded value orders every load behind it; a wave holds 63 loads
    // in flight, so the last requests leave as the first return - DESIGN 4.4.2).  The newest data first: the
    // partials were written by the previous launch on other XCDs, the weights and Z / T / LSE are older.
    // Thread = (row, 16-byte chunk) of the [16][128] sums; four partials per group, a clamped index in
    // place of a branch for the ones past nparts (their values are replaced by +0.f below).
    const int row = tid >> 4, ch = tid & 15;
    float4 k0[4], k1[4], v0[4], v1[4];
    auto request = [&](int p0) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int pp = p0 + u < nparts ? p0 + u : p0;
        const int64_t off = (((int64_t)b * nparts + pp) * MQ + row) * D + ch * 8;
        const float4* pk = reinterpret_cast<const float4*>(a.dKpPart + off);
        const float4* pv = reinterpret_cast<const float4*>(a.dVpPart + off);
        k0[u] = pk[0]; k1[u] = pk[1]; v0[u] = pv[0]; v1[u] = pv[1];
      }
    };
    request(0);
    // dH is split over the waves: wave w computes feature tiles 2w, 2w + 1 and takes its A fragments of
    // Wk1^T / Wv1^T straight from global memory (16 loads per lane, each byte of the two matrices read
    // once per workgroup; no staging through LDS)
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        wk_pre[tt][ks] = gload8(a.Wk1T + (int64_t)(16 * (2 * w + tt) + r) * D + 32 * ks + 8 * g);
        wv_pre[tt][ks] = gload8(a.Wv1T + (int64_t)(16 * (2 * w + tt) + r) * D + 32 * ks + 8 * g);
      }
    const int64_t trow = (int64_t)b * 64 + 16 * w + r;           // this lane's query row of T
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
      zpre[tt] = *reinterpret_cast<const float4*>(a.Z + ((int64_t)b * MQ + r) * D + 16 * (2 * w + tt) + 4 * g);
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4)
        wo_pre[tt][s4] = gload8(a.Wo0TP + (int64_t)(16 * (2 * w + tt) + r) * D + 32 * s4 + 8 * g);
    if (SMALL) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        // (columns at and past dk are never used: a clamped index, not a branch around the load)
        const int cc = c < dk ? c : dk - 1;
        ts_pre[c] = a.T[trow * dk + cc];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            wvf_pre[c][4 * tt + e] = a.Wv0f[(32 * w + 16 * tt + 4 * g + e) * dk + cc];
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
    // (the scheduler must not sink a request below the sums to save registers)
    __builtin_amdgcn_sched_barrier(0);
    PCA_MID_STAMP(1);
    {
      float k[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      // The fixed order of the sum: u = 0..3 inside a group, the groups in order of p0.  A partial past
      // nparts is added as +0.f: k and v start at +0.f and a sum that starts there is never -0.f, so the
      // addition leaves every bit alone - and the loads of a group stay one batch (a branch around an
      // addition took its loads with it: one round trip per partial).
      auto add = [&](int p0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bool in = p0 + u < nparts;
          const float4 a0 = in ? k0[u] : float4{0.f, 0.f, 0.f, 0.f}, a1 = in ? k1[u] : float4{0.f, 0.f, 0.f, 0.f};
          const float4 b0 = in ? v0[u] : float4{0.f, 0.f, 0.f, 0.f}, b1 = in ? v1[u] : float4{0.f, 0.f, 0.f, 0.f};
          k[0] += a0.x; k[1] += a0.y; k[2] += a0.z; k[3] += a0.w;
          k[4] += a1.x; k[5] += a1.y; k[6] += a1.z; k[7] += a1.w;
          v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w;
          v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
        }
      };
      add(0);
      // more than four partials (small batches): the further groups, one batch of 16 loads each
      for (int p0 = 4; p0 < nparts; p0 += 4) {
        request(p0);
        add(p0);
      }
      PCA_MID_STAMP(2);
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
  PCA_MID_STAMP(3);

  // ---- dH^T: feature tiles 2w, 2w + 1 in wave w; their masked dZ goes to the other waves ----
  f32x4 dO2[2];
  if (on) {
    bf16x8 kb[4], vb[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      kb[ks] = *reinterpret_cast<const bf16x8*>(sK + swz(r, 4 * ks + g, ROWB));
      vb[ks] = *reinterpret_cast<const bf16x8*>(sV + swz(r, 4 * ks + g, ROWB));
    }
    f32x4 dz[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      f32x4 dh = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        dh = mfma32(wk_pre[tt][ks], kb[ks], dh);
        dh = mfma32(wv_pre[tt][ks], vb[ks], dh);
      }
      const int64_t off = ((int64_t)b * MQ + r) * D + 16 * (2 * w + tt) + 4 * g;
      const float4 z4 = zpre[tt];
      dz[tt][0] = z4.x > 0.f ? dh[0] : 0.f;
      dz[tt][1] = z4.y > 0.f ? dh[1] : 0.f;
      dz[tt][2] = z4.z > 0.f ? dh[2] : 0.f;
      dz[tt][3] = z4.w > 0.f ? dh[3] : 0.f;
      if (wr) *reinterpret_cast<float4*>(a.dZ + off) = float4{dz[tt][0], dz[tt][1], dz[tt][2], dz[tt][3]};
      dO2[tt] = dh;
    }
    // B operand s = w of the dO MFMAs, lane-linear: the lane that reads it holds the same (r, g)
    *reinterpret_cast<bf16x8*>(sDz + (w * 64 + lane) * 16) = pack8(dz[0], dz[1]);
  }
  __syncthreads();
  if (!on) return;
  PCA_MID_STAMP(4);

  // ---- dO^T tiles of head w ----
  bf16x8 dzb[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) dzb[s] = *reinterpret_cast<const bf16x8*>(sDz + (s * 64 + lane) * 16);
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int t = 2 * w + tt;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      dO2[tt] = mfma32(wo_pre[tt][s], dzb[s], dO2[tt]);
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
  PCA_MID_STAMP(5);
}

}  // namespace pca
