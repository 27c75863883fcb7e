// Per-set "mid" kernels of an ISAB (set_transformer-master/modules.py:51-53) in the fused
// bf16 mode: everything that happens on the [m = 16, d = 128] inducing-point tensors between
// the two point-sized kernels, on the MFMA in the transposed-chain layout (mfma_common.hpp).
//
//   k_mid_fwd   merge the attention partials of mab0 -> T ; O = Qp + T_h Wv_h^T + bv ;
//               Z = O Wo^T + bo ; H = O + relu(Z)          (mab0 epilogue, modules.py:29-31)
//               Kp = H Wk^T + bk ; Vp = H Wv^T + bv        (mab1 projections, modules.py:21)
//               written in the four bf16 images k_mab1_fwd / k_mab1_bwd read.
//   k_mid_bwd   dH = dKp Wk + dVp Wv ; dZ = dH.[Z>0] ; dO = dH + dZ Wo ; dT_h = dO_h Wv_h ;
//               Delta = rowdot(dT, T)  -> the images k_mab0_bwd reads, plus dZ / dO / T_h
//               (fp32) for the weight-gradient reductions and sum_b dO for the shared query.
// One workgroup per set, wave w = head w.  Each wave needs every weight fragment exactly
// once, so fragments are read straight from L2 (no LDS staging); activations cross waves
// through small bf16 LDS images.
#include "blocks.hpp"
#include "mfma_common.hpp"
#include "mid_bwd_body.hpp"

#include <math.h>
#ifdef PCA_DEBUG_CLOCKS
#include <stdio.h>
#include <stdlib.h>
#endif

namespace pca {

namespace {

constexpr int D = 128, MQ = 16, ROWB = 256;

// write one accumulator tile (rows = features 16t+4g+e, col = query r) into a [query][feature]
// bf16 image
__device__ __forceinline__ void put_tile(char* img, int t, int r, int g, f32x4 v) {
  *reinterpret_cast<bf16x4*>(img + swz(r, 2 * t + (g >> 1), ROWB) + 8 * (g & 1)) = pack4(v);
}

struct MidFwdArgs {
  // attention partials of mab0 (S > 0) or merged T (S == 0, layer 1)
  const float *Tp, *Mp, *Lp;
  int S;
  float *T, *LSE;             // [B][64][dk], [B][64]  (saved)
  const float* Qp;            // [16][128]
  const __bf16* Wv0;          // [128][dk] natural (dk == 128) ...
  const float* Wv0f;          // ... or fp32 for dk <= 4
  const float *bv0, *bo0;
  const __bf16* Wo0;          // [128][128] natural
  const __bf16 *Wk1, *Wv1;    // [128][128] natural
  const float *bk1, *bv1;
  float *O, *Z, *H;           // [B][16][128] fp32
  __bf16 *KpP, *VpP, *Kt, *Vt;
  int dk;
};

template <bool SMALL>
__global__ __launch_bounds__(256) void k_mid_fwd(const MidFwdArgs a) {
  __shared__ __attribute__((aligned(16))) char sT[64 * ROWB];   // T  bf16 [r][c]
  __shared__ __attribute__((aligned(16))) char sA[16 * ROWB];   // O, then H  bf16 [q][f]
  __shared__ float sTf[SMALL ? 64 * 4 : 1];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int dk = a.dk;

  // every weight fragment / bias of phases A-C is fetched now (latency-bound kernel: one
  // workgroup per set; the round trips overlap the partial merge instead of following it)
  bf16x8 wv0_pre[2][SMALL ? 1 : 4], wo0_pre[2][4], wk1_pre[2][4], wv1_pre[2][4];
  float4 q_pre[2], bv0_pre[2], bo0_pre[2], bk1_pre[2], bv1_pre[2];
  float bk1c_pre[2], bv1c_pre[2];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int t = 2 * w + tt;
    q_pre[tt] = *reinterpret_cast<const float4*>(a.Qp + r * D + 16 * t + 4 * g);
    bv0_pre[tt] = *reinterpret_cast<const float4*>(a.bv0 + 16 * t + 4 * g);
    bo0_pre[tt] = *reinterpret_cast<const float4*>(a.bo0 + 16 * t + 4 * g);
    bk1_pre[tt] = *reinterpret_cast<const float4*>(a.bk1 + 16 * t + 4 * g);
    bv1_pre[tt] = *reinterpret_cast<const float4*>(a.bv1 + 16 * t + 4 * g);
    bk1c_pre[tt] = a.bk1[16 * t + r];
    bv1c_pre[tt] = a.bv1[16 * t + r];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if (!SMALL) wv0_pre[tt][ks] = gload8(a.Wv0 + (int64_t)(16 * t + r) * D + 32 * ks + 8 * g);
      wo0_pre[tt][ks] = gload8(a.Wo0 + (int64_t)(16 * t + r) * D + 32 * ks + 8 * g);
      wk1_pre[tt][ks] = gload8(a.Wk1 + (int64_t)(16 * t + r) * D + 32 * ks + 8 * g);
      wv1_pre[tt][ks] = gload8(a.Wv1 + (int64_t)(16 * t + r) * D + 32 * ks + 8 * g);
    }
  }
  // ---- merge partials -> T (global fp32, saved) and its bf16 image ----
  if (SMALL) {
    for (int i = tid; i < 64 * dk; i += 256) sTf[(i / dk) * 4 + (i % dk)] = a.T[(int64_t)b * 64 * dk + i];
  } else {
#pragma unroll
    for (int it = 0; it < 4; ++it) {                   // (row, 8-element chunk)
      const int i = tid + 256 * it;
      const int row = i >> 4, ch = i & 15;
      // the partials of up to four point ranges at a time, all loads issued together (clamped
      // slot, zero weight): one round trip per group instead of three dependent ones per range
      float M = -INFINITY;
      float L = 0.f, t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      float msv[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        msv[s] = a.Mp[((int64_t)b * a.S + (s < a.S ? s : 0)) * 64 + row];
        if (s < a.S) M = fmaxf(M, msv[s]);
      }
#pragma unroll
      for (int s0 = 0; s0 < 8; s0 += 4) {
        if (s0 >= a.S) break;
        float lpv[4];
        float4 lo[4], hi[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t o = ((int64_t)b * a.S + (s0 + u < a.S ? s0 + u : 0)) * 64 + row;
          lpv[u] = a.Lp[o];
          const float4* tp = reinterpret_cast<const float4*>(a.Tp + o * D + ch * 8);
          lo[u] = tp[0];
          hi[u] = tp[1];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float ms = msv[s0 + u];
          if (s0 + u >= a.S || ms == -INFINITY) continue;
          const float fs = exp2f(ms - M);
          L += fs * lpv[u];
          t[0] += fs * lo[u].x; t[1] += fs * lo[u].y; t[2] += fs * lo[u].z; t[3] += fs * lo[u].w;
          t[4] += fs * hi[u].x; t[5] += fs * hi[u].y; t[6] += fs * hi[u].z; t[7] += fs * hi[u].w;
        }
      }
      const float inv = 1.f / L;
      bf16x8 v;
      float4 o0, o1;
#pragma unroll
      for (int k = 0; k < 8; ++k) { t[k] *= inv; v[k] = (__bf16)t[k]; }
      o0 = float4{t[0], t[1], t[2], t[3]};
      o1 = float4{t[4], t[5], t[6], t[7]};
      float4* tg = reinterpret_cast<float4*>(a.T + ((int64_t)b * 64 + row) * D + ch * 8);
      tg[0] = o0; tg[1] = o1;
      *reinterpret_cast<bf16x8*>(sT + swz(row, ch, ROWB)) = v;
      if (ch == 0) a.LSE[(int64_t)b * 64 + row] = M + log2f(L);
    }
  }
  __syncthreads();

  // ---- phase A: O^T tiles of head w (features 32w .. 32w+31) ----
  f32x4 o[2];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int t = 2 * w + tt;
    const float4 q4 = q_pre[tt];
    const float4 b4 = bv0_pre[tt];
    o[tt] = f32x4{q4.x + b4.x, q4.y + b4.y, q4.z + b4.z, q4.w + b4.w};
    if (SMALL) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int f = 16 * t + 4 * g + e;
        for (int c = 0; c < dk; ++c) o[tt][e] += sTf[(16 * w + r) * 4 + c] * a.Wv0f[f * dk + c];
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        o[tt] = mfma32(wv0_pre[tt][ks],
                       *reinterpret_cast<const bf16x8*>(sT + swz(16 * w + r, 4 * ks + g, ROWB)),
                       o[tt]);
    }
    put_tile(sA, t, r, g, o[tt]);
    *reinterpret_cast<float4*>(a.O + ((int64_t)b * MQ + r) * D + 16 * t + 4 * g) =
        float4{o[tt][0], o[tt][1], o[tt][2], o[tt][3]};
  }
  __syncthreads();

  // ---- phase B: Z^T = Wo O^T + bo ; H = O + relu(Z) ----
  f32x4 hq[2];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int t = 2 * w + tt;
    const float4 b4 = bo0_pre[tt];
    f32x4 z = f32x4{b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      z = mfma32(wo0_pre[tt][ks],
                 *reinterpret_cast<const bf16x8*>(sA + swz(r, 4 * ks + g, ROWB)), z);
#pragma unroll
    for (int e = 0; e < 4; ++e) hq[tt][e] = o[tt][e] + fmaxf(z[e], 0.f);
    const int64_t off = ((int64_t)b * MQ + r) * D + 16 * t + 4 * g;
    *reinterpret_cast<float4*>(a.Z + off) = float4{z[0], z[1], z[2], z[3]};
    *reinterpret_cast<float4*>(a.H + off) = float4{hq[tt][0], hq[tt][1], hq[tt][2], hq[tt][3]};
  }
  __syncthreads();                     // every wave has read the O image
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) put_tile(sA, 2 * w + tt, r, g, hq[tt]);
  __syncthreads();

  // ---- phase C: Kp, Vp of mab1 in both orientations ----
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    __bf16* PP = which ? a.VpP : a.KpP;
    __bf16* TT = which ? a.Vt : a.Kt;
    f32x4 fr[2], kr[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const int t = 2 * w + tt;
      const float4 b4 = which ? bv1_pre[tt] : bk1_pre[tt];
      const float bc = which ? bv1c_pre[tt] : bk1c_pre[tt];
      fr[tt] = f32x4{b4.x, b4.y, b4.z, b4.w};      // rows = features, col = key
      kr[tt] = f32x4{bc, bc, bc, bc};              // rows = keys,     col = feature
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 wf = which ? wv1_pre[tt][ks] : wk1_pre[tt][ks];
        const bf16x8 hf = *reinterpret_cast<const bf16x8*>(sA + swz(r, 4 * ks + g, ROWB));
        fr[tt] = mfma32(wf, hf, fr[tt]);
        kr[tt] = mfma32(hf, wf, kr[tt]);
      }
      // keys 4g..4g+3 of feature 16t + r : 8 contiguous bytes of the [feature][key] image
      *reinterpret_cast<bf16x4*>(TT + ((int64_t)b * D + 16 * t + r) * MQ + 4 * g) = pack4(kr[tt]);
    }
    // features 32w + perm32(8g + .) of key r : 16 contiguous bytes of the permuted image
    *reinterpret_cast<bf16x8*>(PP + ((int64_t)b * MQ + r) * D + 32 * w + 8 * g) =
        pack8(fr[0], fr[1]);
  }
}

template <bool SMALL>
__global__ __launch_bounds__(256) void k_mid_bwd(const MidBwdArgs a) {
  __shared__ __attribute__((aligned(16))) char sKVO[MID_BWD_SMALL_LDS];   // dKp, dVp, per-wave dO_j, dZ
  const int b = blockIdx.x, tid = threadIdx.x;
  if (a.zero_ptr != nullptr)
    for (int i = blockIdx.x * 256 + tid; i < a.zero_n; i += gridDim.x * 256) a.zero_ptr[i] = 0.f;
  // one workgroup per set on half the CUs: the chain (mid_bwd_body.hpp) is purely latency-bound
  mid_bwd_body<SMALL>(a, b, mid_bwd_lds(sKVO), true, MidSinkGlobal{a, b});
}

}  // namespace

#ifdef PCA_DEBUG_CLOCKS
// diagnostic build: the phase stamps of the mid chain in the prologue of its carrying kernel (set PCA_DBG_WG
// of the last launch; mid_bwd_body.hpp names the phases) are printed at exit, in microseconds from the entry
long long* mid_debug_clock_buffer(int which) {
  static long long* buf[2] = {nullptr, nullptr};
  if (buf[which] == nullptr) {
    (void)hipHostMalloc(reinterpret_cast<void**>(&buf[which]), 8 * sizeof(long long), 0);
    for (int i = 0; i < 8; ++i) buf[which][i] = 0;
    struct P {
      static void dump(int w) {
        const long long* b = buf[w];
        const long long t0 = b[0] & 0xffffffffffffLL;
        fprintf(stderr, "mid chain stamps, %s (phase:us):", w == 0 ? "k_mab0_bwd<64, .>" : "small carrier");
        for (int i = 0; i < 7; ++i) fprintf(stderr, " %lld:%.2f", b[i] >> 48, ((b[i] & 0xffffffffffffLL) - t0) / 100.0);
        fprintf(stderr, "\n");
      }
    };
    if (which == 0) atexit([] { P::dump(0); });
    else atexit([] { P::dump(1); });
  }
  return buf[which];
}
#endif

int mid_fwd_launch(const MidFwdLaunch& L, hipStream_t st) {
  MidFwdArgs a{};
  a.Tp = L.Tp; a.Mp = L.Mp; a.Lp = L.Lp; a.S = L.S; a.T = L.T; a.LSE = L.LSE; a.Qp = L.Qp;
  a.Wv0 = L.Wv0; a.Wv0f = L.Wv0f; a.bv0 = L.bv0; a.bo0 = L.bo0; a.Wo0 = L.Wo0; a.Wk1 = L.Wk1;
  a.Wv1 = L.Wv1; a.bk1 = L.bk1; a.bv1 = L.bv1; a.O = L.O; a.Z = L.Z; a.H = L.H; a.KpP = L.KpP;
  a.VpP = L.VpP; a.Kt = L.Kt; a.Vt = L.Vt; a.dk = L.dk;
  if (L.dk <= 4) hipLaunchKernelGGL((k_mid_fwd<true>), dim3(L.B), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_mid_fwd<false>), dim3(L.B), dim3(256), 0, st, a);
  return check_launch("k_mid_fwd");
}

int mid_bwd_launch(const MidBwdLaunch& L, hipStream_t st) {
  const MidBwdArgs a = mid_bwd_args(L);
  if (L.dk <= 4) hipLaunchKernelGGL((k_mid_bwd<true>), dim3(L.B), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_mid_bwd<false>), dim3(L.B), dim3(256), 0, st, a);
  return check_launch("k_mid_bwd");
}

}  // namespace pca
