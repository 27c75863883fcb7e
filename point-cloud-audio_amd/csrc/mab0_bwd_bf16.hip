// Fused bf16-MFMA backward of the "few shared queries, many keys" MAB (ISAB mab0 / PMA) in
// the reassociated form of mab0_bf16.hip.  With G' = sl2e * Qp_h Wk_h (sl2e = log2(e)/sqrt d),
// P = exp2(G' X^T - lse), T = P X and the forward's epilogue O_h = Qp_h + T_h Wv_h^T + bv_h,
// H = O + relu(O Wo^T + bo):
//
//   k_mab0_epi_bwd (per set, fp32 VALU)   dZ = dH.[Z>0] ; dO = dH + dZ Wo ; dT_h = dO_h Wv_h ;
//                                         Delta = rowdot(dT, T)
//   k_mab0_bwd     (per set, MFMA)        per 32-point tile of a wave, transposed layout
//        S^T = G' X^T, dA^T = dT X^T  ->  P^T, dS^T = ln2 . P^T (dA^T - Delta)
//        dX^T += dT^T P^T + G'^T dS^T        (both sums run over accumulator ROWS: in registers)
//        dG   += dS X                         (sum over points: dS^T goes through a wave-private
//                                              LDS tile and comes back transposed, X^T through
//                                              ds_read_tr16_b64 of the X tile)
//   k_mab0_bwd_small                      layer 1 (dk <= 4): fp32 VALU, no dX needed
//   parameter gradients of the epilogue (dWo, dWv, dbo, dbv) are [B*m]-row reductions: jobs of
//   k_wgrad128 (wgrad128.hip); the post stages (k_mab0_post1 / 2, bwd_defer.hip) turn sum_b dO and dG
//   into dWk, dWq, dbq, dI.  d(bk) is identically zero (softmax shift invariance) and is left
//   untouched.  The PMA head launch that precedes this backward in the train step: pma_head.hip.
#include "blocks.hpp"
#include "bwd_defer.hpp"
#include "step_ctx.hpp"
#include "mfma_common.hpp"
#include "pma_head_bodies.hpp"
#include "mid_bwd_body.hpp"
#include "mab0_bwd_small_body.hpp"

#include <math.h>
#include <stdlib.h>

#include <mutex>

namespace pca {

namespace {

// [rows][RP] bf16 image (RP*2 bytes per row), 16-byte chunks XOR-swizzled by the row
template <int RP>
__device__ __forceinline__ int rp_off(int row, int ch) {
  constexpr int NCH = RP / 8;
  return row * RP * 2 + ((ch ^ (row & (NCH - 1))) << 4);
}

// ---------------------------------------------------------------------------------
// per-set epilogue adjoint (fp32)
// ---------------------------------------------------------------------------------
// thread = (output column, half of the queries); weights are read in their natural nn.Linear
// layout, which is already coalesced for these products (sum over the OUTPUT index).
template <int MQ>
__global__ __launch_bounds__(256) void k_mab0_epi_bwd(
    const float* __restrict__ dH, const float* __restrict__ Z, const float* __restrict__ T,
    const float* __restrict__ LSE, const float* __restrict__ Wo, const float* __restrict__ Wv,
    int m, int d, int dk, int h, int Rp, float* __restrict__ dZ, float* __restrict__ dO,
    float* __restrict__ Th,      // [h][B*m][dk] head-major copy of T (for dWv)
    float* __restrict__ dTf,     // [B][R][dk] fp32 (small-dk path)
    __bf16* __restrict__ dTb,    // [B][Rp][dk] natural rows
    __bf16* __restrict__ dTt,    // [B][dk][Rp] r-permuted
    float* __restrict__ Delta,   // [B][Rp]
    float* __restrict__ LSEp,    // [B][Rp] padded with +1e30
    int B, float* __restrict__ zero_ptr, int zero_n) {
  mab0_epi_bwd_body<MQ>(dH, Z, T, LSE, Wo, Wv, m, d, dk, h, Rp, dZ, dO, Th, dTf, dTb, dTt, Delta, LSEp, B, zero_ptr, zero_n, blockIdx.x);
}

// G'^T image shared by all sets: GtP[c][32 s + p] = G'[32 s + perm32(p)][c]  (zero padding)
__global__ void k_mab0_gt(const float* __restrict__ Gf, int R, int Rp, int dk,
                          __bf16* __restrict__ GtP) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= dk * Rp) return;
  const int c = idx / Rp, k = idx - c * Rp;
  const int r = (k & ~31) + perm32(k & 31);
  GtP[idx] = (__bf16)(r < R ? Gf[r * dk + c] : 0.f);
}

// ---------------------------------------------------------------------------------
// main backward over the points, dk == 128
// ---------------------------------------------------------------------------------
struct Mab0BwdArgs {
  const void* X;         // [B, N, 128] fp32, or bf16 when ABF
  const __bf16* Gb;      // [Rp][128] natural rows (sl2e folded in)
  const __bf16* GtP;     // [128][Rp]
  const __bf16* dTb;     // [B][Rp][128]
  const __bf16* dTt;     // [B][128][Rp]
  const float* LSEp;     // [B][Rp]
  const float* Delta;    // [B][Rp]
  void* dX;              // [B, N, 128] (fp32 / bf16 when ABF) or null
  float* DG;             // [Rp][128] fp32, accumulated over sets (ln2-scaled dS units)
  int B, N, accumulate_dx, S;
  const int32_t* lengths;   // [B] valid points per set, or null
  int R;                    // real score rows (<= RP): only these rows of dG are non-zero
  float* slabs;             // [B*S][R][128]: per-workgroup dG (summed in a fixed order afterwards)
  // fuse_mid (RP == 64, an ISAB's few-queries block): dTb / dTt / LSEp / Delta are not read; every
  // workgroup of a set runs the set's mid chain (mid_bwd_body.hpp) and keeps the images in LDS
  int fuse_mid;
  MidBwdArgs mid;
};

// sinks of the mid chain run in a prologue: the images in the layout the main loop reads them in
struct MidSinkWide {
  char *sdT, *sdTt;
  float *sLSE, *sDel;
  __device__ __forceinline__ void dTb(int row, int ct, int g, bf16x4 v) const {
    *reinterpret_cast<bf16x4*>(sdT + tr_off(row, 2 * ct + (g >> 1)) + 8 * (g & 1)) = v;
  }
  __device__ __forceinline__ void dTt(int ct, int r, int w, int g, bf16x4 v) const {
    *reinterpret_cast<bf16x4*>(sdTt + rp_off<64>(16 * ct + r, 4 * (w >> 1) + g) + 8 * (w & 1)) = v;
  }
  __device__ __forceinline__ void dTf(int, int, float) const {}
  __device__ __forceinline__ void stat(int row, float delta, float lse) const {
    sDel[row] = delta;
    sLSE[row] = lse;
  }
};

template <int RP, bool ABF>
__global__ __launch_bounds__(256, 1) void k_mab0_bwd(const Mab0BwdArgs a) {
  constexpr int DK = 128, FT = DK / 16, KS = DK / 32, RB = RP / 16, RS = RP / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sG = smem;                           // [RP][256]   tr_off rows
  char* sdT = sG + RP * 256;                 // [RP][256]
  char* sGt = sdT + RP * 256;                // [128][RP*2] rp_off
  char* sdTt = sGt + DK * RP * 2;            // [128][RP*2]
  char* sX = sdTt + DK * RP * 2;             // 4 x 32 x 256
  char* sDS = sX + 4 * 32 * 256;             // 4 x 32 x 256 (first RP*2 bytes of a row used)
  float* sLSE = reinterpret_cast<float*>(sDS + 4 * 32 * 256);
  float* sDel = sLSE + RP;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int b = blockIdx.x, sp = blockIdx.y;
  PCA_MID_STAMPS_DECL;       // (phase stamps of the fused mid chain: diagnostic builds only)
  const int per = (int)(((int64_t)(a.N + 127) / 128 + a.S - 1) / a.S) * 128;
  const int n_lo = sp * per, n_hi = (n_lo + per < a.N) ? n_lo + per : a.N;
  // variable-size sets: points at and beyond len have P = 0 (so dS = 0 and their dX rows are
  // written as exact zeros); the loops still cover all N rows
  int len = a.N;
  if (a.lengths != nullptr) len = a.lengths[b] < a.N ? a.lengths[b] : a.N;

  // the wave's next X tile is fetched into registers while the current one is worked on (the kernel
  // runs one wave per SIMD: registers are free, and every tile used to start with an exposed round trip)
  bf16x8 nx[8];
  auto fetch_tile = [&](int n0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = lane + 64 * e;
      // (bf16 activations: zeroed when the tile goes to LDS, see ld_x8_clamped)
      nx[e] = ABF ? ld_x8_clamped(a.X, (int64_t)b * a.N, n0 + (c >> 4), n_hi, DK, c & 15)
                  : ld_x8_guard<ABF>(a.X, (int64_t)b * a.N, n0 + (c >> 4), n_hi, DK, c & 15);
    }
  };
  bool fuse = false;
  if constexpr (RP == 64) fuse = a.fuse_mid != 0;
  if constexpr (RP == 64) if (fuse) {
    // the shared images and the first X tile are in flight while the set's mid chain runs: the chain's
    // small images live behind the statistics, and dT / dT^T / Delta / LSE land where the loop reads them
    constexpr int NA = RP * 16 / 256, NB2 = DK * (RP / 8) / 256;
    bf16x8 g1[NA], g2[NB2];
#pragma unroll
    for (int e = 0; e < NA; ++e) {
      const int c = tid + 256 * e, row = c >> 4, ch = c & 15;
      g1[e] = gload8(a.Gb + (int64_t)row * DK + ch * 8);
    }
#pragma unroll
    for (int e = 0; e < NB2; ++e) {
      const int c = tid + 256 * e, row = c / (RP / 8), ch = c % (RP / 8);
      g2[e] = gload8(a.GtP + (int64_t)row * RP + ch * 8);
    }
    if (n_lo + wave * 32 < n_hi) fetch_tile(n_lo + wave * 32);
    char* const tail = reinterpret_cast<char*>(sDel + RP);
    mid_bwd_body<false>(a.mid, b, mid_bwd_lds(tail), sp == 0, MidSinkWide{sdT, sdTt, sLSE, sDel} PCA_MID_STAMPS_ARG);
#pragma unroll
    for (int e = 0; e < NA; ++e) {
      const int c = tid + 256 * e, row = c >> 4, ch = c & 15;
      *reinterpret_cast<bf16x8*>(sG + tr_off(row, ch)) = g1[e];
    }
#pragma unroll
    for (int e = 0; e < NB2; ++e) {
      const int c = tid + 256 * e, row = c / (RP / 8), ch = c % (RP / 8);
      *reinterpret_cast<bf16x8*>(sGt + rp_off<RP>(row, ch)) = g2[e];
    }
  }
  if (!fuse) {
    // all image chunks of this thread are fetched before the first LDS store: one round trip
    // instead of one per loop iteration (the stores would order the loads behind them)
    constexpr int NA = RP * 16 / 256, NB2 = DK * (RP / 8) / 256;
    // (bf16x8, not uint4: copies of that struct type are memcpys, which kept these arrays in scratch
    //  memory once the mid chain was inlined above)
    bf16x8 g1[NA], t1[NA], g2[NB2], t2[NB2];
#pragma unroll
    for (int e = 0; e < NA; ++e) {
      const int c = tid + 256 * e, row = c >> 4, ch = c & 15;
      g1[e] = gload8(a.Gb + (int64_t)row * DK + ch * 8);
      t1[e] = gload8(a.dTb + ((int64_t)b * RP + row) * DK + ch * 8);
    }
#pragma unroll
    for (int e = 0; e < NB2; ++e) {
      const int c = tid + 256 * e, row = c / (RP / 8), ch = c % (RP / 8);
      g2[e] = gload8(a.GtP + (int64_t)row * RP + ch * 8);
      t2[e] = gload8(a.dTt + ((int64_t)b * DK + row) * RP + ch * 8);
    }
#pragma unroll
    for (int e = 0; e < NA; ++e) {
      const int c = tid + 256 * e, row = c >> 4, ch = c & 15;
      *reinterpret_cast<bf16x8*>(sG + tr_off(row, ch)) = g1[e];
      *reinterpret_cast<bf16x8*>(sdT + tr_off(row, ch)) = t1[e];
    }
#pragma unroll
    for (int e = 0; e < NB2; ++e) {
      const int c = tid + 256 * e, row = c / (RP / 8), ch = c % (RP / 8);
      *reinterpret_cast<bf16x8*>(sGt + rp_off<RP>(row, ch)) = g2[e];
      *reinterpret_cast<bf16x8*>(sdTt + rp_off<RP>(row, ch)) = t2[e];
    }
    for (int i = tid; i < RP; i += 256) {
      sLSE[i] = a.LSEp[(int64_t)b * RP + i];
      sDel[i] = a.Delta[(int64_t)b * RP + i];
    }
  }
  __syncthreads();

  char* myX = sX + wave * 32 * 256;
  char* myDS = sDS + wave * 32 * 256;
  f32x4 dG[RB][FT];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) dG[rb][ft] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr float LN2 = 0.6931471805599453f;

  if (!fuse && n_lo + wave * 32 < n_hi) fetch_tile(n_lo + wave * 32);
  PCA_MID_STAMP(6);
  for (int n0 = n_lo + wave * 32; n0 < n_hi; n0 += 128) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = lane + 64 * e;
      const int row = c >> 4, ch = c & 15;
      *reinterpret_cast<bf16x8*>(myX + tr_off(row, ch)) = zero_unless(n0 + row < n_hi, nx[e]);
    }
    if (n0 + 128 < n_hi) fetch_tile(n0 + 128);
    // the rows this tile's dX is added onto (mab1's dQ part) are fetched now, a whole tile of work
    // ahead of their use: read at the end they were an exposed round trip per tile (5 of 37 us)
    bf16x8 od[8];
    if (ABF && a.dX != nullptr && a.accumulate_dx) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = lane + 64 * e, n = n0 + (c >> 4);
        od[e] = *reinterpret_cast<const bf16x8*>(
            reinterpret_cast<const __bf16*>(a.dX) +
            ((int64_t)b * a.N + (n < n_hi ? n : n_hi - 1)) * DK + (c & 15) * 8);
      }
    }
    bf16x8 xrow[2][KS];
#pragma unroll
    for (int pb = 0; pb < 2; ++pb)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        xrow[pb][ks] = *reinterpret_cast<const bf16x8*>(myX + tr_off(16 * pb + r, 4 * ks + g));
    bool live[2], key[2];          // row exists / row is a key of the (possibly shorter) set
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
      live[pb] = n0 + 16 * pb + r < n_hi;
      key[pb] = n0 + 16 * pb + r < len;
    }

    f32x4 dx[FT][2];
#pragma unroll
    for (int ft = 0; ft < FT; ++ft)
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) dx[ft][pb] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int s = 0; s < RS; ++s) {
      f32x4 pt[2][2], dst[2][2];          // [row block within the 32][point block]
#pragma unroll
      for (int rbi = 0; rbi < 2; ++rbi) {
        const int rb = 2 * s + rbi;
        const float4 l4 = *reinterpret_cast<const float4*>(&sLSE[16 * rb + 4 * g]);
        const float4 d4 = *reinterpret_cast<const float4*>(&sDel[16 * rb + 4 * g]);
        const float lse[4] = {l4.x, l4.y, l4.z, l4.w}, del[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
          f32x4 sv = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            sv = mfma32(*reinterpret_cast<const bf16x8*>(sG + tr_off(16 * rb + r, 4 * ks + g)),
                        xrow[pb][ks], sv);
            da = mfma32(*reinterpret_cast<const bf16x8*>(sdT + tr_off(16 * rb + r, 4 * ks + g)),
                        xrow[pb][ks], da);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float p = key[pb] ? exp2f(sv[e] - lse[e]) : 0.f;
            pt[rbi][pb][e] = p;
            dst[rbi][pb][e] = LN2 * p * (da[e] - del[e]);
          }
          // dS^T tile -> wave-private [point][r] image (for the sum over points below)
          *reinterpret_cast<bf16x4*>(myDS + tr_off(16 * pb + r, 2 * rb + (g >> 1)) + 8 * (g & 1)) =
              pack4(dst[rbi][pb]);
        }
      }
      if (a.dX != nullptr) {
        bf16x8 pf[2], df[2];
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
          pf[pb] = pack8(pt[0][pb], pt[1][pb]);
          df[pb] = pack8(dst[0][pb], dst[1][pb]);
        }
#pragma unroll
        for (int ft = 0; ft < FT; ++ft) {
          const bf16x8 ta =
              *reinterpret_cast<const bf16x8*>(sdTt + rp_off<RP>(16 * ft + r, 4 * s + g));
          const bf16x8 ga =
              *reinterpret_cast<const bf16x8*>(sGt + rp_off<RP>(16 * ft + r, 4 * s + g));
#pragma unroll
          for (int pb = 0; pb < 2; ++pb) {
            dx[ft][pb] = mfma32(ta, pf[pb], dx[ft][pb]);
            dx[ft][pb] = mfma32(ga, df[pb], dx[ft][pb]);
          }
        }
      }
    }

    // dG[r][c] += sum_points dS[r][pt] X[pt][c]
    bf16x8 xtr[FT];
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) xtr[ft] = tr_frag(myX, ft, lane);
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const bf16x8 da = tr_frag(myDS, rb, lane);
#pragma unroll
      for (int ft = 0; ft < FT; ++ft) dG[rb][ft] = mfma32(da, xtr[ft], dG[rb][ft]);
    }

    if (a.dX != nullptr && ABF) {
      // bf16 dX: the [32 points][128] tile is assembled in the wave's own LDS tile (X is no longer
      // needed) and stored / accumulated in 16-byte pieces of full rows, the loads unconditional -
      // from the accumulator layout it was 16 guarded read-modify-writes of 8 bytes per lane, each
      // waited for on its own
#pragma unroll
      for (int pb = 0; pb < 2; ++pb)
#pragma unroll
        for (int ft = 0; ft < FT; ++ft)
          *reinterpret_cast<bf16x4*>(myX + swz(16 * pb + r, 2 * ft + (g >> 1), 2 * DK) + 8 * (g & 1)) =
              pack4(dx[ft][pb]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = lane + 64 * e, row = c >> 4, ch = c & 15;
        const int n = n0 + row;
        bf16x8 v = *reinterpret_cast<const bf16x8*>(myX + swz(row, ch, 2 * DK));
        __bf16* pd = reinterpret_cast<__bf16*>(a.dX) +
                     ((int64_t)b * a.N + (n < n_hi ? n : n_hi - 1)) * DK + ch * 8;
        if (a.accumulate_dx) {
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] = (__bf16)((float)v[k] + (float)od[e][k]);
        }
        if (n < n_hi) *reinterpret_cast<bf16x8*>(pd) = v;
      }
    } else if (a.dX != nullptr) {
#pragma unroll
      for (int pb = 0; pb < 2; ++pb)
        if (live[pb]) {
          const int64_t ro = ((int64_t)b * a.N + n0 + 16 * pb + r) * DK;
#pragma unroll
          for (int ft = 0; ft < FT; ++ft) {
            f32x4 v = dx[ft][pb];
            if (ABF) {
              bf16x4* pd = reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(a.dX) + ro +
                                                     16 * ft + 4 * g);
              if (a.accumulate_dx) {
                const bf16x4 o = *pd;
                v[0] += (float)o[0]; v[1] += (float)o[1]; v[2] += (float)o[2]; v[3] += (float)o[3];
              }
              *pd = pack4(v);
            } else {
              float4* pd = reinterpret_cast<float4*>(reinterpret_cast<float*>(a.dX) + ro +
                                                     16 * ft + 4 * g);
              float4 o4 = float4{v[0], v[1], v[2], v[3]};
              if (a.accumulate_dx) {
                const float4 o = *pd;
                o4.x += o.x; o4.y += o.y; o4.z += o.z; o4.w += o.w;
              }
              *pd = o4;
            }
          }
        }
    }
  }

  // ---- dG: per-wave slabs (plain LDS stores over the dead images), then one global atomic
  //      per element per workgroup ----
  __syncthreads();
  float* slab = reinterpret_cast<float*>(smem) + wave * RP * DK;      // 4 x RP x 128 fp32
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int ft = 0; ft < FT; ++ft)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        slab[(16 * rb + 4 * g + e) * DK + 16 * ft + r] = dG[rb][ft][e];
  __syncthreads();
  const float* s0 = reinterpret_cast<const float*>(smem);
  // (PMA: 4 of the 32 padded rows are real.)  One slab per workgroup, plain stores: 256 workgroups
  // adding into one [R][128] block cost 11 of this kernel's 37 us at B = 128 - the adds to one
  // address serialise at ~25 ns each - and made the result depend on their order
  float* out = a.slabs + ((int64_t)b * a.S + sp) * a.R * DK;
  for (int i = tid; i < a.R * DK; i += 256)
    out[i] = s0[i] + s0[RP * DK + i] + s0[2 * RP * DK + i] + s0[3 * RP * DK + i];
  PCA_MID_STAMPS_WRITE(a.mid, b, sp == 0);
}

// layer 1 (dk <= 4): mab0_bwd_small_body.hpp; gridDim.y workgroups share the rows of a set.
// MID (R == 64, an ISAB's first few-queries block): dTf / Delta are not read; every workgroup of a set
// runs the set's mid chain in the dynamic LDS block (MID_SMALL_FUSE_LDS bytes).  An instance of its own,
// so that the plain kernel does not carry the chain's registers.
template <bool MID>
__global__ __launch_bounds__(256) void k_mab0_bwd_small(
    const float* __restrict__ X, const float* __restrict__ Gf, const float* __restrict__ dTf,
    const float* __restrict__ LSE, const float* __restrict__ Delta, int N, int R, int Rp, int dk,
    float* __restrict__ DG, const int32_t* __restrict__ lengths, float* __restrict__ slabs,
    const MidBwdArgs mid) {
  __shared__ float sD[256][4];
  __shared__ __attribute__((aligned(16))) float sX[PCA_POINT_CHUNK * 4];
  extern __shared__ __attribute__((aligned(16))) char smid[];
  mab0_bwd_small_body<MID, 256>(Mab0SmallArgs{X, Gf, dTf, LSE, Delta, N, R, Rp, dk, DG, lengths, slabs, mid},
                                blockIdx.x, blockIdx.y, gridDim.y, sD, sX, smid);
}

}  // namespace

int mab0_bwd_small_launch(const float* X, const float* Gf, const float* dTf, const float* LSE,
                          const float* Delta, int B, int N, int R, int Rp, int dk, float* DG,
                          const int32_t* lengths, hipStream_t st, float* slabs) {
  PCA_REQUIRE(R == 64 || R == 128 || R == 256, "mab0_bwd_small: %d score rows", R);
  hipLaunchKernelGGL(k_mab0_bwd_small<false>, dim3(B, small_row_split(B, R)), dim3(256), 0, st, X, Gf,
                     dTf, LSE, Delta, N, R, Rp, dk, DG, lengths, slabs, MidBwdArgs{});
  return check_launch("k_mab0_bwd_small");
}

// point ranges per set of k_mab0_bwd (96+ KiB of LDS: one workgroup per CU)
int mab0_bwd_splits(const pca_mab_shape& s) {
  int S = mab0_splits(s);
  while (S > 1 && s.B * S > 256) S /= 2;
  return S;
}
size_t mab0_carve_bwd_ws(const pca_mab_shape& s, Mab0BwdWs* out, void* base) {
  Carver c(base);
  Mab0BwdWs w;
  const int R = s.h * s.nq, Rp = (int)cdiv(R, 32) * 32;
  const size_t Bm = (size_t)s.B * s.nq;
  w.dZ = c.take<float>(Bm * s.d);
  w.dO = c.take<float>(Bm * s.d);
  w.Th = c.take<float>((size_t)s.B * R * s.dk);
  w.dTf = c.take<float>((size_t)s.B * R * s.dk);
  w.Delta = c.take<float>((size_t)s.B * Rp);
  w.LSEp = c.take<float>((size_t)s.B * Rp);
  w.DG = c.take<float>((size_t)Rp * s.dk);
  w.dQs = c.take<float>((size_t)s.nq * s.d);
  w.dQp = c.take<float>((size_t)s.nq * s.d);
  w.dTb = c.take<__bf16>((size_t)s.B * Rp * s.dk);
  w.dTt = c.take<__bf16>((size_t)s.B * Rp * s.dk);
  w.GtP = c.take<__bf16>((size_t)Rp * s.dk);
  w.slabs = c.take<float>(s.dk <= 4 ? (size_t)s.B * R * s.dk
                                     : (size_t)s.B * mab0_bwd_splits(s) * R * s.dk);
  if (out) *out = w;
  return c.off;
}

size_t mab0_bf16_bwd_ws_bytes(const pca_mab_shape& s) {
  return mab0_carve_bwd_ws(s, nullptr, nullptr);
}

// a fixed-order slab sum: with the other sums of the step when the caller defers them, else right away
static int slab_sum_defer(BwdDefer* defer, const SlabSumJob& sj, hipStream_t st) {
  SlabSumJobs one{};
  SlabSumJobs& J = defer != nullptr ? defer->sums : one;
  PCA_REQUIRE(J.n < 40, "mab0_bf16_bwd: slab-sum table full");
  J.j[J.n++] = sj;
  return defer != nullptr ? PCA_OK : slab_sum_jobs(one, st);
}

// dQ -> dI [m, dq] (ACCUMULATED, may be null), dK -> dX [B, N, dk] (written or accumulated)
int mab0_bf16_bwd_ex(const pca_mab_shape& s, const float* I, const void* X,
                     const pca_mab_params& p, const void* saved, const float* dH, float* dI,
                     void* dX, int dk_accumulate, const pca_mab_grads& gr, void* ws, int flags,
                     hipStream_t st, StepCtx* ctx, const MidBwdLaunch* mid) {
  PCA_REQUIRE(mid == nullptr || (s.d == 128 && s.nq == 16 && s.h == 4 && (flags & PCA_F_SKIP_HEAD) &&
                                 !(flags & PCA_F_ATTN_DONE)),
              "mab0_bf16_bwd: the mid chain fuses into an ISAB's few-queries block only");
  PCA_REQUIRE(s.d == 128, "mab0_bf16_bwd: d = 128 only (d = 256: mab0_d256_bwd)");
  BwdDefer* const defer = defer_of(ctx);
  Mab0Saved v;
  mab0_carve_saved(s, &v, const_cast<void*>(saved));
  Mab0BwdWs w;
  mab0_carve_bwd_ws(s, &w, ws);
  const bool head_done = (flags & PCA_F_SKIP_HEAD) != 0;
  const int d = s.d, m = s.nq, h = s.h, dk = s.dk, R = h * m, Rp = (int)cdiv(R, 32) * 32;
  const int64_t Bm = (int64_t)s.B * m;
  const bool small = dk <= 4;
  const float sl2e = LOG2E / sqrtf((float)d);
  if (small && dX != nullptr) {
    set_error("mab0_bf16_bwd: dK for dk <= 4 is not built (the set is the model input)");
    return PCA_EUNSUPPORTED;
  }

  const size_t el = (2 * (size_t)m * d + (size_t)Rp + (size_t)d) * sizeof(float);   // + split scratch
  if (head_done) {
    // dZ, dO, Th, dT images, Delta, LSEp and dQs come from k_mid_bwd, or (mid != null) from the
    // mid chain in the prologue of the launch below
  } else if (m > 2)
    hipLaunchKernelGGL((k_mab0_epi_bwd<8>), dim3(s.B), dim3(256), el, st, dH, v.Z, v.T, v.LSE, p.wo,
                       p.wv, m, d, dk, h, Rp, w.dZ, w.dO, w.Th, small ? w.dTf : nullptr,
                       small ? nullptr : w.dTb, small ? nullptr : w.dTt, w.Delta, w.LSEp, s.B,
                       w.DG, Rp * dk);
  else
    hipLaunchKernelGGL((k_mab0_epi_bwd<1>), dim3(s.B), dim3(256), el, st, dH, v.Z, v.T, v.LSE, p.wo,
                       p.wv, m, d, dk, h, Rp, w.dZ, w.dO, w.Th, small ? w.dTf : nullptr,
                       small ? nullptr : w.dTb, small ? nullptr : w.dTt, w.Delta, w.LSEp, s.B,
                       w.DG, Rp * dk);
  PCA_TRY(check_launch("k_mab0_epi_bwd"));
  // (with head_done the caller's k_mid_bwd has cleared DG)

  if (small) {
    // slab mode: per-set partials [B][R][dk] instead of atomics, summed in a fixed order
    float* sl = (tail_form_of(defer).slabs && (R * dk) % 4 == 0) ? w.slabs : nullptr;
    const dim3 sgrid(s.B, (R % 64 == 0 && R <= 512) ? 2 : 1);
    if (mid != nullptr) {
      PCA_REQUIRE(R == 64, "mab0_bf16_bwd: fused mid chain with %d score rows", R);
      static std::once_flag once_small;
      std::call_once(once_small, [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_mab0_bwd_small<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, MID_SMALL_FUSE_LDS);
      });
      // the bf16 weight-gradient list collected so far needs nothing this kernel writes: when it may run
      // now (bwd_defer_ride), both go into one launch, this backward as one 512-thread workgroup per set
      WgradJobs ride{};
      int ride_rpw = 0, rc = PCA_OK;
      if (sl != nullptr && defer != nullptr && bwd_defer_ride(*defer, &ride, &ride_rpw, &rc)) {
        PCA_TRY(mab0_small_ride_launch(
            ride, ride_rpw,
            Mab0SmallArgs{reinterpret_cast<const float*>(X), v.Gf, w.dTf, v.LSE, w.Delta, s.nk, R, Rp, dk,
                          w.DG, s.k_lengths, sl, mid_bwd_args(*mid)},
            s.B, st));
      } else {
        PCA_TRY(rc);
        hipLaunchKernelGGL(k_mab0_bwd_small<true>, sgrid, dim3(256), MID_SMALL_FUSE_LDS, st,
                           reinterpret_cast<const float*>(X), v.Gf, w.dTf, v.LSE, w.Delta, s.nk, R, Rp, dk,
                           w.DG, s.k_lengths, sl, mid_bwd_args(*mid));
      }
    } else {
      hipLaunchKernelGGL(k_mab0_bwd_small<false>, sgrid, dim3(256), 0, st,
                         reinterpret_cast<const float*>(X), v.Gf, w.dTf, v.LSE, w.Delta, s.nk, R, Rp, dk,
                         w.DG, s.k_lengths, sl, MidBwdArgs{});
    }
    PCA_TRY(check_launch("k_mab0_bwd_small"));
    if (sl != nullptr) {
      // (only the first R * dk floats of the [Rp][dk] block are read by the post stage)
      PCA_TRY(slab_sum_defer(defer, SlabSumJob{sl, w.DG, s.B, R * dk, 0, 0}, st));
    }
  } else if (flags & PCA_F_ATTN_DONE) {
    // the set-resident forward ran the attention backward and left the slabs k_mab0_bwd would have
    // written: only their fixed-order sum is left
    PCA_REQUIRE(head_done && R * dk == 512, "mab0_bf16_bwd: set-resident PMA backward with R=%d dk=%d", R, dk);
    PCA_TRY(slab_sum_defer(defer, SlabSumJob{w.slabs, w.DG, s.B * mab0_bwd_splits(s), R * dk, 0, 0}, st));
  } else {
    const int S = mab0_bwd_splits(s);
    Mab0BwdArgs a{X, v.Gb, v.GtP, w.dTb, w.dTt, w.LSEp, w.Delta, dX, w.DG, s.B, s.nk,
                  dk_accumulate ? 1 : 0, S, s.k_lengths, R, w.slabs, 0, MidBwdArgs{}};
    size_t lds = 2 * (size_t)Rp * 256 + 2 * (size_t)128 * Rp * 2 + 2 * 4 * 32 * 256 +
                 2 * Rp * sizeof(float);
    if (mid != nullptr) {
      PCA_REQUIRE(Rp == 64, "mab0_bf16_bwd: fused mid chain with %d score rows", Rp);
      a.fuse_mid = 1;
      a.mid = mid_bwd_args(*mid);
      lds += MID_BWD_SMALL_LDS;       // dKp / dVp / dO_j / dZ images of the chain, behind the statistics
    }
    if (lds < (size_t)4 * Rp * 128 * 4) lds = (size_t)4 * Rp * 128 * 4;     // merge slabs
    allow_lds160<k_mab0_bwd<64, false>, k_mab0_bwd<64, true>, k_mab0_bwd<32, false>, k_mab0_bwd<32, true>>();
    const double pts = (double)s.B * s.nk;
    const bool abf = s.k_dtype == PCA_BF16;
    // algorithmic bytes: X in, dX out (read as well when it accumulates onto mab1's dQ)
    const double eb0 = abf ? 2.0 : 4.0;
    ProfScope ps(PCA_K_MAB0_BWD, st, 4.0 * pts * (2.0 * dk * d + 2.0 * m * d),
                 pts * eb0 * dk * (1.0 + (dX != nullptr ? (dk_accumulate ? 2.0 : 1.0) : 0.0)));
    const dim3 grid(s.B, S);
    if (Rp == 32 && abf) hipLaunchKernelGGL((k_mab0_bwd<32, true>), grid, dim3(256), lds, st, a);
    else if (Rp == 32) hipLaunchKernelGGL((k_mab0_bwd<32, false>), grid, dim3(256), lds, st, a);
    else if (abf) hipLaunchKernelGGL((k_mab0_bwd<64, true>), grid, dim3(256), lds, st, a);
    else hipLaunchKernelGGL((k_mab0_bwd<64, false>), grid, dim3(256), lds, st, a);
    ps.end();
    PCA_TRY(check_launch("k_mab0_bwd"));
    // dG = the workgroups' slabs added in a fixed order: with the other sums of the step when
    // the caller defers them, else right away
    PCA_TRY(slab_sum_defer(defer, SlabSumJob{w.slabs, w.DG, s.B * S, R * dk, 0, 0}, st));
  }

  // ---- parameter gradients of the epilogue: [B*m]-row reductions, ONE MFMA launch ----
  if (!(flags & PCA_F_SKIP_WGRAD)) {
    WgradJobs jobs{};
    jobs.j[0] = WgradJob{w.dZ, v.O, gr.wo, gr.bo, Bm, 0, 128};
    jobs.n = 1;
    if (!small) {
      const int dh = d / h;
      for (int j = 0; j < h; ++j)          // dWv rows of head j  <-  dO^T . T_j
        jobs.j[jobs.n++] = WgradJob{w.dO, w.Th + (int64_t)j * Bm * dk, gr.wv,
                                    j == 0 ? gr.bv : nullptr, Bm, j * dh, (j + 1) * dh};
    }
    PCA_TRY(wgrad128_defer(defer, jobs, false, 64, st));
    if (small)
      PCA_TRY(wgrad_small_f32_launch(w.dO, w.Th, Bm, dk, (int64_t)Bm * dk, gr.wv, gr.bv, st));
  }
  // (the sum of dO over the sets is taken inside k_mab0_post1)
  // k_mid_bwd / k_mab0_epi_bwd left dO per set, the post kernel sums it
  Mab0PostJob pj{nullptr, w.DG, v.Qp, p.wk, I, p.wq, gr.wk, w.dQp, gr.wq,
                 gr.bq, dI, m, d, dk, s.dq, h, sl2e, w.dO, s.B};
  Mab0PostJobs one{};
  Mab0PostJobs& J = defer != nullptr ? defer->posts : one;      // queued like the slab sums, or run now
  PCA_REQUIRE(J.n < 3, "mab0_bf16_bwd: post-job table full");
  J.j[J.n++] = pj;
  return defer != nullptr ? PCA_OK : mab0_post_launch(one, st);
}

}  // namespace pca
