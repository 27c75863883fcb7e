// Fused bf16-MFMA backward of ISAB's mab1(X, H) (adjoint of set_transformer-master/
// modules.py:19-33 in the "many queries, few keys" orientation; math in SURVEY.md 3c).
//
//   k_mab1_bwd   per 32 points of one wave, all in registers in the transposed layout:
//                dZ = dY.mask ; dO^T = dY^T + Wo^T.dZ^T ; per head: P^T recomputed from the
//                saved Qp, dA^T = Vp_h.dO_h^T, dS^T = P^T.(dA^T - rowsum) / sqrt(d),
//                dQp_h^T = dO_h^T + Kp_h^T.dS^T ; dX^T = Wq^T.dQp^T.
//                Writes dX and bf16 copies of dZ, dO, dQp, dS, P for the reductions over
//                points, which need the point index on the MFMA K axis:
//   (the weight gradients dWo / dWq = G^T.A over the points, G = dZ|dQp, A = O|X, are jobs of
//    k_wgrad128 / k_wgrad_small: wgrad128.hip)
//   k_kv_grad    per (set, head): dKp = dS^T.Qp, dVp = P^T.dO (m x 32 outputs, N-long sums).
// The tiny [B*m, d] projections of H (fc_k, fc_v) are differentiated with the fp32 GEMMs.
#include "blocks.hpp"
#include "weight_images.hpp"
#include "bwd_defer.hpp"
#include "step_ctx.hpp"
#include "mfma_common.hpp"

#include <math.h>
#include <stdlib.h>

#include <type_traits>

namespace pca {

namespace {

constexpr int TP = M1_TP;
constexpr int NB = M1_NB;

// (to_chunk / from_chunk, the 16-byte pieces of DESIGN.md 4.4.8: mfma_common.hpp)
// the two halves of a chunk that was loaded as two fragments (the instances that keep the 8-byte form)
__device__ __forceinline__ u32x4 two_frags(bf16x4 a, bf16x4 b) {
  const uint2 ua = __builtin_bit_cast(uint2, a), ub = __builtin_bit_cast(uint2, b);
  return u32x4{ua.x, ua.y, ub.x, ub.y};
}

struct Mab1BwdArgs {
  const void* dY;           // [B, N, D] fp32, or bf16 when ABF
  const __bf16* QpS;        // [B*N][D]
  const uint32_t* mask;
  const __bf16 *KpP, *VpP;  // [B][MI][D]  (K-permuted features)
  const __bf16* Kt;         // [B][D][MI]
  const __bf16 *WoTP, *WqTP;
  __bf16 *dZ, *dQp, *dOs;   // [B*N][D]
  __bf16 *dS, *P;           // [B*N][H*MI]
  void* dX;                 // [B, N, D] (fp32 / bf16 when ABF) or null
  float *dKpG, *dVpG;       // [B][nparts][MI][D] fp32 partial K/V gradients (fused mode)
  const float* Xs;          // layer 1 (dq <= 3): the fp32 points [B, N, dq] ...
  float *dWqS, *dbqS;       // ... and fc_q gradients accumulated here (fused reduction)
  float* wq_slab;           // ... or, when set, per-workgroup partials [wg][D*dq + D] (fixed-order sum later)
  const float *WqF, *bqF;   // ... and fc_q itself: Qp is recomputed (2..3 FMAs per element)
                            //     instead of being saved by the forward and read back
  int dq;
  float* zero_ptr;          // optional: zero_n floats cleared by this launch (consumer's
  int zero_n;               //           accumulator, e.g. the dQs of k_mid_bwd)
  long long* dbg;           // PCA_DEBUG_CLOCKS builds: phase time stamps of workgroup 0
  int B, N, tiles_per_set;
  int tpw;                  // consecutive tiles of ONE set per workgroup (fused mode)
  float scale, scale_log2e;
  int dbg_wg;               // PCA_DEBUG_CLOCKS builds: the workgroup whose phase stamps are kept
};


#ifdef PCA_DEBUG_CLOCKS
// (kept in scalar registers and written once at the end: a store per stamp would sit in vmcnt and be
//  waited for by the next phase's loads)
#define PCA_STAMP(i) do { stamp_[i] = wall_clock64(); } while (0)
#else
#define PCA_STAMP(i) do {} while (0)
#endif
// Waves per workgroup: 8 for the d -> d variant with dX (its 100+ KiB of LDS images allow one
// workgroup per CU; eight waves sharing them give every SIMD two wavefronts to interleave, and
// waves 4..7 take the next 128-point tile), otherwise 4 with two workgroups per CU.
template <bool WANT_DX, bool FUSE_KV>
struct BwdWaves {
  static constexpr int value = (WANT_DX && FUSE_KV) ? 8 : 4;
  static constexpr int per_cu = WANT_DX ? 1 : 2;        // workgroups per CU
};

template <int D, int MI, bool WANT_DX, bool FUSE_KV, bool FUSE_WQ, bool ABF>
__global__ __launch_bounds__((64 * BwdWaves<WANT_DX, FUSE_KV>::value),
                             (BwdWaves<WANT_DX, FUSE_KV>::per_cu))
void k_mab1_bwd(const Mab1BwdArgs a) {
  constexpr int NW = BwdWaves<WANT_DX, FUSE_KV>::value, NT = 64 * NW, SUBS = NW / 4;
  constexpr int DT = D / 16, KS = D / 32, ROWB = D * 2, HM = KS * MI;
  // bf16 tile operands move as 16-byte chunks; the fp32-activation instances keep their form (fp32 dY is 16 bytes
  // per lane as it is, and their bf16 Qp loads and dZ / dQp / dOs stores stay 8-byte fragments)
  constexpr bool WIDE = ABF;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sWoT = smem;
  char* sKp = sWoT + D * ROWB;
  char* sVp = sKp + MI * ROWB;
  char* sKt = sVp + MI * ROWB;
  char* sWqT = sKt + D * MI * 2;
  // fused K/V gradients: per wave [32][16] dS, [32][16] P, [32][32] Qp_j, [32][32] dO_j images
  char* sKV = sWqT + (WANT_DX ? D * ROWB : 0);

  const int tid = threadIdx.x, lane = tid & 63, wave8 = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
#ifdef PCA_DEBUG_CLOCKS
  long long stamp_[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
  PCA_STAMP(0);

  // One batch of requests per tile.  On the workgroup's first tile the Wo / Wq image chunks
  // lead it, on the first tile of a set the K / V images; then the tile's own operands - mask words, dY, the
  // saved Qp or layer 1's points - which depend on nothing in LDS.  The images are stored to LDS while the
  // tile is still in flight (vmcnt counts down to the tile's requests, not to zero: lds_barrier()), and
  // every convert, select and mask sits at the use, not behind its load.
  constexpr int NC = D * (D / 8) / NT;                       // Wo / Wq chunks per thread
  constexpr int KVC = (MI * (D / 8) + NT - 1) / NT;          // KpP / VpP / Kt chunks per thread
  const int total_tiles = a.B * a.tiles_per_set;
  int cur_b = -1;
  // row pitches padded by 8 bytes (40 / 72 instead of 32 / 64): with power-of-two pitches the
  // 16 point rows of a store or transposed read fall on 2 resp. 4 LDS banks repeatedly
  // (SQ_LDS_BANK_CONFLICT was 3x the LDS-active cycles of this kernel); 10 / 18 banks per row
  // spread them over all 64
  constexpr int PS = 40, PQ = 72, KVB = 2 * 32 * PS + 2 * 32 * PQ;
  // layer 1: fc_q rows as float4 (w0, w1, w2, bias) behind the per-wave images
  float4* sWq4 = reinterpret_cast<float4*>(sKV + NW * KVB);
  f32x4 dkp[FUSE_KV ? KS : 1][2], dvp[FUSE_KV ? KS : 1][2];
  if (FUSE_KV) {
#pragma unroll
    for (int j = 0; j < KS; ++j)
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        dkp[j][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
        dvp[j][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
  }
  // layer 1: fc_q gradients on the matrix core.  wqa[j][tt] = Xa . dQp_j with the augmented
  // point matrix Xa[16][32 points]: rows 0..2 = bf16 high parts of x, row 3 = ones (bias),
  // rows 4..6 = bf16 low parts (x = hi + lo to ~2^-17), so that
  // dWq[f][c] = row c + row 4+c and dbq[f] = row 3 of column f.
  f32x4 wqa[FUSE_WQ ? KS : 1][2];
  if (FUSE_WQ) {
#pragma unroll
    for (int j = 0; j < KS; ++j)
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) wqa[j][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // fused mode: a workgroup owns `tpw` consecutive tiles of one set; otherwise grid-stride
  const int t_first = FUSE_KV ? blockIdx.x * a.tpw : blockIdx.x;
  const int t_step = FUSE_KV ? 1 : gridDim.x;
  const int t_last = FUSE_KV ? t_first + a.tpw : total_tiles;
  // (fused mode with 8 waves: two consecutive tiles of the set per pass, one per wave quartet)
  // The pass over one tile, instantiated twice: for the workgroup's first tile, whose batch the weight images
  // lead (straight-line code in front of the loop), and for every later one (inside the loop, where only a new
  // set's K / V images join the tile's requests).  One body in the loop with a run-time `first` had every address
  // of the weight staging hoisted out of the loop and kept alive through it.
  auto pass = [&](auto first_c, const int tile0) __attribute__((always_inline)) {
    constexpr bool first = decltype(first_c)::value;
    // the thread index anew in each copy (rederive() of set128_fwd.hip): what is derived from it - lane, r, g,
    // the swizzled LDS offsets - is otherwise shared between the two copies and hoisted out of the loop, kept
    // alive across the first tile and spilled next to its requests
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    int lane = tid & 63, wave8 = tid >> 6, wave = wave8 & 3, sub = wave8 >> 2;
    int r = lane & 15, g = lane >> 4;
    char* myDS = sKV + wave8 * KVB;
    char* myP = myDS + 32 * PS;
    char* myQ = myP + 32 * PS;
    char* myO = myQ + 32 * PQ;
    const int b = tile0 / a.tiles_per_set;
    // odd count: waves 4..7 have no tile; they request the quartet's tile (in bounds, discarded) and
    // leave behind the barrier
    const bool work = tile0 + sub < t_last && tile0 + sub < total_tiles;
    const int tile_id = work ? tile0 + sub : tile0;
    const int tile = tile_id - b * a.tiles_per_set;
    const bool newset = first || b != cur_b;

    const int n_base = tile * TP + wave * 32;
    int nn[NB];
    bool live[NB];
    int64_t row[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      nn[nb] = n_base + 16 * nb + r;
      live[nb] = nn[nb] < a.N;
      row[nb] = (int64_t)b * a.N + (live[nb] ? nn[nb] : 0);
    }

    // ---- the requests ----
    u32x4 wo[NC], wq[WANT_DX ? NC : 1];
    if (first) {
#pragma unroll
      for (int e = 0; e < NC; ++e) {
        const int c = tid + NT * e, wrow = c / (D / 8), c16 = c % (D / 8);
        wo[e] = *reinterpret_cast<const u32x4*>(a.WoTP + (int64_t)wrow * D + c16 * 8);
        if (WANT_DX) wq[e] = *reinterpret_cast<const u32x4*>(a.WqTP + (int64_t)wrow * D + c16 * 8);
      }
    }
    u32x4 kp[KVC], vp[KVC], kt[KVC];
    if (newset) {
#pragma unroll
      for (int e = 0; e < KVC; ++e) {
        // (chunk index clamped, the LDS store guarded: the load stays unconditional)
        const int c = min(tid + NT * e, MI * (D / 8) - 1), krow = c / (D / 8), c16 = c % (D / 8);
        const int64_t src = ((int64_t)b * MI + krow) * D + c16 * 8;
        kp[e] = *reinterpret_cast<const u32x4*>(a.KpP + src);
        vp[e] = *reinterpret_cast<const u32x4*>(a.VpP + src);
        kt[e] = reinterpret_cast<const u32x4*>(a.Kt + (int64_t)b * D * MI)[c];
      }
    }
    float wq4[4];                    // layer 1: row min(tid, D - 1) of fc_q and its bias
    if (FUSE_WQ && first) {
      const int f = min(tid, D - 1);
#pragma unroll
      for (int c = 0; c < 3; ++c) wq4[c] = a.WqF[f * a.dq + min(c, a.dq - 1)];
      wq4[3] = a.bqF[f];
    }
    // (the images first: their LDS stores then wait for them alone, vmcnt counting in order)
    __builtin_amdgcn_sched_barrier(0);
    uint32_t bits[NB][D / 128];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int w = 0; w < D / 128; ++w)
        bits[nb][w] = a.mask[mab1_mask_index<D>(b, a.tiles_per_set, tile, wave, nb, w, lane)];
    // dY^T tiles as loaded (bf16: the 16-byte chunk chunk_of(g) of tiles 2s, 2s + 1; fp32 dY lands in dO itself).
    // Unconditional - row[] is clamped for padding points - and zeroed at the use
    f32x4 dO[DT][NB];
    u32x4 dyw[WIDE ? KS : 1][NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if (WIDE) {
#pragma unroll
        for (int s = 0; s < KS; ++s)
          dyw[WIDE ? s : 0][nb] = *reinterpret_cast<const u32x4*>(
              reinterpret_cast<const __bf16*>(a.dY) + row[nb] * D + 32 * s + 8 * chunk_of(g));
        continue;
      }
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        const float4 v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(a.dY) +
                                                          row[nb] * D + 16 * t + 4 * g);
        dO[t][nb] = f32x4{v.x, v.y, v.z, v.w};
      }
    }
    // layer 1: this lane's points for the Qp recomputation, and the points of the A operand below;
    // components at or past dq read component dq - 1 and are discarded
    float xq[NB][3], xa[8];
    if (FUSE_WQ) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int c = 0; c < 3; ++c) xq[nb][c] = a.Xs[row[nb] * a.dq + min(c, a.dq - 1)];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int pt = n_base + (k < 4 ? 4 * g + k : 16 + 4 * g + k - 4);
        xa[k] = a.Xs[((int64_t)b * a.N + (pt < a.N ? pt : 0)) * a.dq + min(r & 3, a.dq - 1)];
      }
    }
    // the saved Qp, features 32j + perm32(8g + .) of this lane's points: head 0's with the batch, head j + 1's
    // while head j is worked on (the whole tile's - 32 registers through the fc_o adjoint - spilled)
    // (with bf16 activations as one chunk, swapped into the two fragments at the use)
    u32x4 qs[FUSE_WQ ? 1 : KS][NB];
    auto request_qp = [&](const int j) __attribute__((always_inline)) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        if (WIDE)
          qs[j][nb] = *reinterpret_cast<const u32x4*>(a.QpS + row[nb] * D + 32 * j + 8 * chunk_of(g));
        else
          qs[j][nb] = two_frags(*reinterpret_cast<const bf16x4*>(a.QpS + row[nb] * D + 32 * j + 4 * g),
                                *reinterpret_cast<const bf16x4*>(a.QpS + row[nb] * D + 32 * j + 16 + 4 * g));
      }
    };
    if (!FUSE_WQ) request_qp(0);
    // (the scheduler must not sink a request below the LDS stores to save registers)
    __builtin_amdgcn_sched_barrier(0);
    PCA_STAMP(8);

    // ---- the images into LDS ---- (their offsets derived here, not kept from the requests)
    asm volatile("" : "+v"(tid));
    if (first) {
#pragma unroll
      for (int e = 0; e < NC; ++e) {
        const int c = tid + NT * e, wrow = c / (D / 8), c16 = c % (D / 8);
        *reinterpret_cast<u32x4*>(sWoT + swz(wrow, c16, ROWB)) = wo[e];
        if (WANT_DX) *reinterpret_cast<u32x4*>(sWqT + swz(wrow, c16, ROWB)) = wq[e];
      }
      if (FUSE_WQ && tid < D)
        sWq4[tid] = float4{wq4[0], a.dq > 1 ? wq4[1] : 0.f, a.dq > 2 ? wq4[2] : 0.f, wq4[3]};
    }
    if (newset) {
      if (!first) lds_barrier();         // the previous set's images have been read
#pragma unroll
      for (int e = 0; e < KVC; ++e) {
        const int c = tid + NT * e, krow = c / (D / 8), c16 = c % (D / 8);
        if (c < MI * (D / 8)) {
          *reinterpret_cast<u32x4*>(sKp + swz(krow, c16, ROWB)) = kp[e];
          *reinterpret_cast<u32x4*>(sVp + swz(krow, c16, ROWB)) = vp[e];
          reinterpret_cast<u32x4*>(sKt)[c] = kt[e];
        }
      }
      cur_b = b;
    }
    lds_barrier();                       // LDS only: the tile's requests stay in flight across it
    __builtin_amdgcn_sched_barrier(0);
    PCA_STAMP(1);
    if (!work) return;                   // (no barrier below)

    // ---- dY^T tiles and dZ = dY . [Z > 0] ----
    bf16x8 dzb[KS][NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      bf16x4 dzh[DT];
      bf16x4 dyf[WIDE ? DT : 1];          // the chunks back in the fragments' shape
      if (WIDE) {
#pragma unroll
        for (int s = 0; s < KS; ++s)
          from_chunk(dyw[WIDE ? s : 0][nb], dyf[WIDE ? 2 * s : 0], dyf[WIDE ? 2 * s + 1 : 0]);
      }
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        const uint32_t m4 = bits[nb][t / 8] >> ((t & 7) * 4);
        if (ABF) {
          // bf16 -> fp32 -> bf16 returns the bits it was given, so dZ is a select on the loaded words
          bf16x4 h4 = dyf[WIDE ? t : 0];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (!live[nb]) h4[e] = (__bf16)0.f;
            dO[t][nb][e] = (float)h4[e];
            dzh[t][e] = ((m4 >> e) & 1u) ? h4[e] : (__bf16)0.f;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (!live[nb]) dO[t][nb][e] = 0.f;
            dzh[t][e] = (__bf16)(((m4 >> e) & 1u) ? dO[t][nb][e] : 0.f);
          }
        }
      }
      if (nb == 0) PCA_STAMP(9);
#pragma unroll
      for (int s = 0; s < KS; ++s) dzb[s][nb] = cat8(dzh[2 * s], dzh[2 * s + 1]);
    }
    if (a.dZ != nullptr) {               // (null: the fc_o job masks dY itself, WgradJob::mask)
      // the materialised form: one block of stores per 16-row group, behind both groups' converts (a branch
      // between them split the tiles' registers)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        if (WIDE) {
          // (the swaps in front of the row's guard: every lane takes part in them)
          u32x4 zc[KS];
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            const bf16x8 z = dzb[s][nb];
            zc[s] = to_chunk(bf16x4{z[0], z[1], z[2], z[3]}, bf16x4{z[4], z[5], z[6], z[7]});
          }
          if (live[nb]) {
#pragma unroll
            for (int s = 0; s < KS; ++s)
              *reinterpret_cast<u32x4*>(a.dZ + row[nb] * D + 32 * s + 8 * chunk_of(g)) = zc[s];
          }
          continue;
        }
        if (live[nb]) {
#pragma unroll
          for (int t = 0; t < DT; ++t) {
            const bf16x8 z = dzb[t / 2][nb];
            *reinterpret_cast<bf16x4*>(a.dZ + row[nb] * D + 16 * t + 4 * g) =
                (t & 1) ? bf16x4{z[4], z[5], z[6], z[7]} : bf16x4{z[0], z[1], z[2], z[3]};
          }
        }
      }
    }
    bf16x8 xaug;
    if (FUSE_WQ) {
      // A operand: lane (row c' = r, k-slots 8g..8g+7 <-> points perm32(8g + .)) of this tile
      const int c = r & 3, part = r >> 2;          // part 0: hi / ones, 1: lo
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float x = xa[k], hi = (float)(__bf16)x;
        float v = part == 0 ? hi : x - hi;
        if (!(part <= 1 && r < 7 && r != 3 && c < a.dq)) v = r == 3 ? 1.f : 0.f;
        xaug[k] = (__bf16)v;
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int c2 = 0; c2 < 3; ++c2)
          if (c2 >= a.dq) xq[nb][c2] = 0.f;
    }

    __builtin_amdgcn_sched_barrier(0);
    PCA_STAMP(2);
    // ---- dO^T = dY^T + Wo^T . dZ^T ----
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        const bf16x8 wa =
            *reinterpret_cast<const bf16x8*>(sWoT + swz(16 * t + r, 4 * s + g, ROWB));
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) dO[t][nb] = mfma32(wa, dzb[s][nb], dO[t][nb]);
      }
    }
    if (!FUSE_KV) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        if (live[nb]) {
#pragma unroll
          for (int t = 0; t < DT; ++t)
            *reinterpret_cast<bf16x4*>(a.dOs + row[nb] * D + 16 * t + 4 * g) = pack4(dO[t][nb]);
        }
    }

    PCA_STAMP(3);
    // (a new phase: the LDS offsets of the heads are derived here, not kept alive from the tile's start)
    asm volatile("" : "+v"(tid));
    lane = tid & 63; r = lane & 15; g = lane >> 4;
    // ---- attention backward per head; dO tiles of the head become dQp in place ----
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      // (one scheduling region per head: across the four unrolled heads hipcc moved the next heads' LDS reads
      //  up until layer 1's accumulators no longer fitted)
      if (FUSE_KV) __builtin_amdgcn_sched_barrier(0);
      if (!FUSE_WQ && j + 1 < KS) {
        request_qp(j + 1);
        __builtin_amdgcn_sched_barrier(0);     // (leaves here, a head ahead of its use)
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        // saved Qp of this point, features 32j + perm32(8g + .)
        bf16x4 qlo, qhi;
        if (FUSE_WQ) {
          // Qp = x Wq^T + bq exactly as the forward computes it (fp32, then rounded to bf16)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float4 wl = sWq4[32 * j + 4 * g + e], wh = sWq4[32 * j + 16 + 4 * g + e];
            qlo[e] = (__bf16)(wl.w + wl.x * xq[nb][0] + wl.y * xq[nb][1] + wl.z * xq[nb][2] +
                              0.f * 0.f);
            qhi[e] = (__bf16)(wh.w + wh.x * xq[nb][0] + wh.y * xq[nb][1] + wh.z * xq[nb][2] +
                              0.f * 0.f);
          }
        } else if (WIDE) {
          from_chunk(qs[FUSE_WQ ? 0 : j][nb], qlo, qhi);
        } else {
          const u32x4 w = qs[FUSE_WQ ? 0 : j][nb];
          qlo = __builtin_bit_cast(bf16x4, uint2{w[0], w[1]});
          qhi = __builtin_bit_cast(bf16x4, uint2{w[2], w[3]});
        }
        bf16x8 qb;
#pragma unroll
        for (int e = 0; e < 4; ++e) { qb[e] = qlo[e]; qb[4 + e] = qhi[e]; }
        const bf16x8 dob = pack8(dO[2 * j][nb], dO[2 * j + 1][nb]);
        f32x4 p0 = {0.f, 0.f, 0.f, 0.f}, p1 = {0.f, 0.f, 0.f, 0.f};
        f32x4 da0 = {0.f, 0.f, 0.f, 0.f}, da1 = {0.f, 0.f, 0.f, 0.f};
        p0 = mfma32(*reinterpret_cast<const bf16x8*>(sKp + swz(r, 4 * j + g, ROWB)), qb, p0);
        da0 = mfma32(*reinterpret_cast<const bf16x8*>(sVp + swz(r, 4 * j + g, ROWB)), dob, da0);
        if (MI == 32) {
          p1 = mfma32(*reinterpret_cast<const bf16x8*>(sKp + swz(16 + r, 4 * j + g, ROWB)), qb,
                      p1);
          da1 = mfma32(*reinterpret_cast<const bf16x8*>(sVp + swz(16 + r, 4 * j + g, ROWB)), dob,
                       da1);
        }
        float mx = fmaxf(fmaxf(p0[0], p0[1]), fmaxf(p0[2], p0[3]));
        if (MI == 32) mx = fmaxf(mx, fmaxf(fmaxf(p1[0], p1[1]), fmaxf(p1[2], p1[3])));
        mx = wave16_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          p0[e] = exp2f((p0[e] - mx) * a.scale_log2e);
          sum += p0[e];
          if (MI == 32) {
            p1[e] = exp2f((p1[e] - mx) * a.scale_log2e);
            sum += p1[e];
          }
        }
        sum = wave16_sum(sum);
        const float inv = 1.0f / sum;
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
        if (FUSE_KV) {
          // wave-private images [point][.] of this head: dS, P (16 keys), Qp_j, dO_j (32 feats);
          // padding points contribute zeros
          const int pt = 16 * nb + r;
          f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
          *reinterpret_cast<bf16x4*>(myDS + pt * PS + 8 * g) = pack4(live[nb] ? ds0 : zero4);
          *reinterpret_cast<bf16x4*>(myP + pt * PS + 8 * g) = pack4(live[nb] ? p0 : zero4);
          *reinterpret_cast<bf16x4*>(myQ + pt * PQ + 8 * g) = qlo;
          *reinterpret_cast<bf16x4*>(myQ + pt * PQ + 32 + 8 * g) = qhi;
          *reinterpret_cast<bf16x4*>(myO + pt * PQ + 8 * g) = pack4(dO[2 * j][nb]);
          *reinterpret_cast<bf16x4*>(myO + pt * PQ + 32 + 8 * g) = pack4(dO[2 * j + 1][nb]);
        } else if (live[nb]) {
          *reinterpret_cast<bf16x4*>(a.P + row[nb] * HM + j * MI + 4 * g) = pack4(p0);
          *reinterpret_cast<bf16x4*>(a.dS + row[nb] * HM + j * MI + 4 * g) = pack4(ds0);
          if (MI == 32) {
            *reinterpret_cast<bf16x4*>(a.P + row[nb] * HM + j * MI + 16 + 4 * g) = pack4(p1);
            *reinterpret_cast<bf16x4*>(a.dS + row[nb] * HM + j * MI + 16 + 4 * g) = pack4(ds1);
          }
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          const int t = 2 * j + tt;
          const char* krow = sKt + (16 * t + r) * (MI * 2);
          if (MI == 16)
            dO[t][nb] = mfma16(*reinterpret_cast<const bf16x4*>(krow + 8 * g), pack4(ds0),
                               dO[t][nb]);
          else
            dO[t][nb] = mfma32(*reinterpret_cast<const bf16x8*>(krow + 16 * g), pack8(ds0, ds1),
                               dO[t][nb]);
        }
      }
      if (FUSE_KV) {
        // dKp_j[key][f] += sum_pt dS[key][pt] Qp[pt][f] ; dVp_j[key][f] += sum_pt P[key][pt] dO[pt][f]
        const bf16x8 ads = tr_frag_small(myDS, PS, 0, lane);
        const bf16x8 ap = tr_frag_small(myP, PS, 0, lane);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          dkp[j][tt] = mfma32(ads, tr_frag_small(myQ, PQ, 16 * tt, lane), dkp[j][tt]);
          dvp[j][tt] = mfma32(ap, tr_frag_small(myO, PQ, 16 * tt, lane), dvp[j][tt]);
        }
        if (FUSE_WQ) {
          // the dO_j image is consumed: overwrite it with dQp_j (padding points carry zeros)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
            const int pt = 16 * nb + r;
            *reinterpret_cast<bf16x4*>(myO + pt * PQ + 8 * g) = pack4(dO[2 * j][nb]);
            *reinterpret_cast<bf16x4*>(myO + pt * PQ + 32 + 8 * g) = pack4(dO[2 * j + 1][nb]);
          }
#pragma unroll
          for (int tt = 0; tt < 2; ++tt)
            wqa[j][tt] = mfma32(xaug, tr_frag_small(myO, PQ, 16 * tt, lane), wqa[j][tt]);
        }
      }
    }
    PCA_STAMP(4);
    // dO now holds dQp^T
    if (FUSE_WQ) {
      // reduced per head above
    } else {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        if (WIDE) {
          u32x4 qc[KS];
#pragma unroll
          for (int s = 0; s < KS; ++s) qc[s] = to_chunk(pack4(dO[2 * s][nb]), pack4(dO[2 * s + 1][nb]));
          if (live[nb]) {
#pragma unroll
            for (int s = 0; s < KS; ++s)
              *reinterpret_cast<u32x4*>(a.dQp + row[nb] * D + 32 * s + 8 * chunk_of(g)) = qc[s];
          }
          continue;
        }
        if (live[nb]) {
#pragma unroll
          for (int t = 0; t < DT; ++t)
            *reinterpret_cast<bf16x4*>(a.dQp + row[nb] * D + 16 * t + 4 * g) = pack4(dO[t][nb]);
        }
      }
    }

    if (WANT_DX) {
      f32x4 dx[DT][NB];
#pragma unroll
      for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) dx[t][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        bf16x8 qb2[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) qb2[nb] = pack8(dO[2 * s][nb], dO[2 * s + 1][nb]);
#pragma unroll
        for (int t = 0; t < DT; ++t) {
          const bf16x8 wa =
              *reinterpret_cast<const bf16x8*>(sWqT + swz(16 * t + r, 4 * s + g, ROWB));
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) dx[t][nb] = mfma32(wa, qb2[nb], dx[t][nb]);
        }
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        if (WIDE) {
          u32x4 xc[KS];
#pragma unroll
          for (int s = 0; s < KS; ++s) xc[s] = to_chunk(pack4(dx[2 * s][nb]), pack4(dx[2 * s + 1][nb]));
          if (live[nb]) {
#pragma unroll
            for (int s = 0; s < KS; ++s)
              *reinterpret_cast<u32x4*>(reinterpret_cast<__bf16*>(a.dX) + row[nb] * D + 32 * s +
                                        8 * chunk_of(g)) = xc[s];
          }
          continue;
        }
        if (live[nb]) {
#pragma unroll
          for (int t = 0; t < DT; ++t) {
            const int64_t xo = row[nb] * D + 16 * t + 4 * g;
            if (ABF) *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(a.dX) + xo) =
                         pack4(dx[t][nb]);
            else *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.dX) + xo) =
                     float4{dx[t][nb][0], dx[t][nb][1], dx[t][nb][2], dx[t][nb][3]};
          }
        }
      }
    }
  };
  if (t_first < t_last && t_first < total_tiles) {
    pass(std::true_type{}, t_first);
    for (int tile0 = t_first + t_step * SUBS; tile0 < t_last && tile0 < total_tiles; tile0 += t_step * SUBS)
      pass(std::false_type{}, tile0);
  }
  PCA_STAMP(5);
  // (behind the tiles: in front of them these stores would be the oldest entries of vmcnt, and the first
  //  LDS store of an image would wait for them)
  if (a.zero_ptr != nullptr)
    for (int i = blockIdx.x * NT + tid; i < a.zero_n; i += gridDim.x * NT) a.zero_ptr[i] = 0.f;
  if (FUSE_WQ) {
    // wqa rows (4g + e) = augmented-point rows, columns = features 32j + 16tt + r: combine
    // the hi (g = 0) and lo (g = 1) rows, sum the waves through LDS, one atomic per element
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);             // [4 waves][D][4]
#pragma unroll
    for (int j = 0; j < KS; ++j)
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float lo = __shfl(wqa[j][tt][e], 16 + r, 64);     // row 4 + e of column r
          v[e] = wqa[j][tt][e] + (e < 3 ? lo : 0.f);
        }
        if (g == 0) {
          float* dst = red + ((wave8 * D) + 32 * j + 16 * tt + r) * 4;
          dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
        }
      }
    __syncthreads();
    for (int i = tid; i < D * 4; i += NT) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) v += red[w * D * 4 + i];
      const int f = i >> 2, c = i & 3;
      if (a.wq_slab != nullptr) {
        float* slab = a.wq_slab + (int64_t)blockIdx.x * (D * a.dq + D);
        if (c < a.dq) slab[f * a.dq + c] = v;
        else if (c == 3) slab[D * a.dq + f] = v;
      } else if (c < a.dq) atomicAdd(&a.dWqS[f * a.dq + c], v);
      else if (c == 3) atomicAdd(&a.dbqS[f], v);
    }
    __syncthreads();
  }
  PCA_STAMP(6);
  if (FUSE_KV && cur_b >= 0) {
    // reduce the four waves' [MI][D] partials in LDS (the weight images are dead), then one
    // atomic per element per workgroup
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);            // [NW][2][MI*D] = 64 / 128 KiB
#pragma unroll
    for (int j = 0; j < KS; ++j)
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int o = (4 * g + e) * D + 32 * j + 16 * tt + r;
          red[(wave8 * 2 + 0) * MI * D + o] = dkp[j][tt][e];
          red[(wave8 * 2 + 1) * MI * D + o] = dvp[j][tt][e];
        }
    __syncthreads();
    const int nparts = a.tiles_per_set / a.tpw;
    const int part = (t_first - cur_b * a.tiles_per_set) / a.tpw;
    for (int i = tid; i < 2 * MI * D; i += NT) {
      const int which = i / (MI * D), o = i - which * MI * D;
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) v += red[(w * 2 + which) * MI * D + o];
      (which ? a.dVpG : a.dKpG)[((int64_t)cur_b * nparts + part) * MI * D + o] = v;
    }
  }
  PCA_STAMP(7);
#ifdef PCA_DEBUG_CLOCKS
  if (a.dbg && (int)blockIdx.x == a.dbg_wg && threadIdx.x == 0)
    for (int i = 0; i < 10; ++i) a.dbg[i] = ((long long)i << 48) | (stamp_[i] & 0xffffffffffffLL);
  if (a.dbg && threadIdx.x == 0 && blockIdx.x < 1024) {
    a.dbg[64 + 2 * blockIdx.x] = stamp_[0];
    a.dbg[65 + 2 * blockIdx.x] = stamp_[7];
  }
#endif
}

// dH[q][c] (+)= sum_f dKp[q][f] Wk[f][c] + dVp[q][f] Wv[f][c]; thread = (column c, query half)
__global__ __launch_bounds__(256) void k_kv_dh(const float* __restrict__ dKp,
                                               const float* __restrict__ dVp,
                                               const float* __restrict__ Wk,
                                               const float* __restrict__ Wv,
                                               float* __restrict__ dH, int m, int d,
                                               int accumulate) {
  extern __shared__ float sm[];
  float* sK = sm;
  float* sV = sm + m * d;
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < m * d; i += 256) {
    sK[i] = dKp[(int64_t)b * m * d + i];
    sV[i] = dVp[(int64_t)b * m * d + i];
  }
  __syncthreads();
  const int c = tid % d, q0 = (tid / d) * 8;
  if (q0 >= m) return;
  float acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q)
    acc[q] = (accumulate && q0 + q < m) ? dH[(int64_t)b * m * d + (q0 + q) * d + c] : 0.f;
  col_gemm<8>(sK + q0 * d, d, Wk, d, d, c, acc);
  col_gemm<8>(sV + q0 * d, d, Wv, d, d, c, acc);
#pragma unroll
  for (int q = 0; q < 8; ++q)
    if (q0 + q < m) dH[(int64_t)b * m * d + (q0 + q) * d + c] = acc[q];
}

// per (set, head): dKp[b][key][32j + c] = sum_n dS[n][j*MI + key] Qp[n][32j + c]
//                  dVp[b][key][32j + c] = sum_n  P[n][j*MI + key] dO[n][32j + c]
template <int MI>
__global__ __launch_bounds__(256) void k_kv_grad(const __bf16* __restrict__ dS,
                                                 const __bf16* __restrict__ P,
                                                 const __bf16* __restrict__ Qp,
                                                 const __bf16* __restrict__ dO, int N, int D,
                                                 int H, float* __restrict__ dKp,
                                                 float* __restrict__ dVp) {
  constexpr int CH = 64;                   // points per staged chunk
  __shared__ float sS[CH][MI + 1], sP[CH][MI + 1], sQ[CH][33], sO[CH][33];
  const int b = blockIdx.x / H, j = blockIdx.x % H;
  const int HM = H * MI;
  const int tid = threadIdx.x;
  const int c = tid & 31, k0 = tid >> 5;         // outputs (key = k0 + 8*i, c)
  constexpr int KPT = MI / 8;
  float ak[KPT], av[KPT];
#pragma unroll
  for (int i = 0; i < KPT; ++i) ak[i] = av[i] = 0.f;
  for (int n0 = 0; n0 < N; n0 += CH) {
    for (int i = tid; i < CH * MI; i += 256) {
      const int pnt = i / MI, key = i % MI;
      const int64_t row = (int64_t)b * N + n0 + pnt;
      const bool ok = n0 + pnt < N;
      sS[pnt][key] = ok ? (float)dS[row * HM + j * MI + key] : 0.f;
      sP[pnt][key] = ok ? (float)P[row * HM + j * MI + key] : 0.f;
    }
    for (int i = tid; i < CH * 32; i += 256) {
      const int pnt = i >> 5, cc = i & 31;
      const int64_t row = (int64_t)b * N + n0 + pnt;
      const bool ok = n0 + pnt < N;
      sQ[pnt][cc] = ok ? (float)Qp[row * D + 32 * j + cc] : 0.f;
      sO[pnt][cc] = ok ? (float)dO[row * D + 32 * j + cc] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int pnt = 0; pnt < CH; ++pnt) {
      const float q = sQ[pnt][c], o = sO[pnt][c];
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        ak[i] += sS[pnt][k0 + 8 * i] * q;
        av[i] += sP[pnt][k0 + 8 * i] * o;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < KPT; ++i) {
    const int64_t o = ((int64_t)b * MI + k0 + 8 * i) * D + 32 * j + c;
    dKp[o] = ak[i];
    dVp[o] = av[i];
  }
}

__global__ void k_sum_parts(const float* __restrict__ kp, const float* __restrict__ vp,
                            float* __restrict__ dk, float* __restrict__ dv, int B, int nparts,
                            int n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * n) return;
  const int64_t b = i / n, o = i - b * n;
  float a = 0.f, c = 0.f;
  for (int p = 0; p < nparts; ++p) {
    a += kp[(b * nparts + p) * n + o];
    c += vp[(b * nparts + p) * n + o];
  }
  dk[i] = a;
  dv[i] = c;
}

#ifdef PCA_DEBUG_CLOCKS
// diagnostic build: the last launch's phase stamps of workgroup 0 are printed at exit
long long* debug_clock_buffer(int which) {
  static long long* buf[2] = {nullptr, nullptr};
  if (buf[which] == nullptr) {
    (void)hipHostMalloc(reinterpret_cast<void**>(&buf[which]), (64 + 2048) * sizeof(long long), 0);
    for (int i = 0; i < 64 + 2048; ++i) buf[which][i] = 0;
    static int reg[2] = {0, 1};
    struct P { static void dump(int w) {
      long long* b = buf[w]; long long t0 = b[0] & 0xffffffffffffLL;
      fprintf(stderr, "k_mab1_bwd[%d] stamps (phase:us):", w);
      for (int i = 0; i < 64 && (i == 0 || b[i]); ++i)
        fprintf(stderr, " %lld:%.2f", b[i] >> 48, ((b[i] & 0xffffffffffffLL) - t0) / 100.0);
      fprintf(stderr, "\n");
      long long s0 = 0; int n = 0;
      for (int i = 0; i < 1024; ++i) if (b[64 + 2 * i]) { if (!n || b[64 + 2 * i] < s0) s0 = b[64 + 2 * i]; ++n; }
      fprintf(stderr, "k_mab1_bwd[%d] per-workgroup start/end us (%d wgs):", w, n);
      for (int i = 0; i < n; i += (n > 64 ? n / 32 : 1))
        fprintf(stderr, " %d:%.1f/%.1f", i, (b[64 + 2 * i] - s0) / 100.0, (b[65 + 2 * i] - s0) / 100.0);
      fprintf(stderr, "\n"); } };
    if (which == 0) atexit([] { P::dump(0); }); else atexit([] { P::dump(1); });
    (void)reg;
  }
  return buf[which];
}
#endif
template <int D, int MI, bool DX, bool FUSE, bool FWQ, bool ABF>
int launch_bwd(const Mab1BwdArgs& a, hipStream_t st, double flops, double bytes) {
  constexpr int NW = BwdWaves<DX, FUSE>::value;
  size_t lds = (size_t)D * D * 2 + 2 * (size_t)MI * D * 2 + (size_t)D * MI * 2 +
               (DX ? (size_t)D * D * 2 : 0) + (FUSE ? NW * (2 * 32 * 40 + 2 * 32 * 72) : 0) +
               (FWQ ? (size_t)D * sizeof(float4) : 0);
  if (FUSE && lds < (size_t)2 * NW * MI * D * 4) lds = (size_t)2 * NW * MI * D * 4;   // flush buffer
  allow_lds160<k_mab1_bwd<D, MI, DX, FUSE, FWQ, ABF>>();
  const int total = a.B * a.tiles_per_set;
  const int grid = FUSE ? (int)cdiv(total, a.tpw) : (total < 256 ? total : 256);
  ProfScope ps(PCA_K_MAB1_BWD, st, flops, bytes);
  hipLaunchKernelGGL((k_mab1_bwd<D, MI, DX, FUSE, FWQ, ABF>), dim3(grid), dim3(64 * NW), lds, st, a);
  ps.end();
  return check_launch("k_mab1_bwd");
}

}  // namespace
size_t mab1_carve_bwd_ws(const pca_mab_shape& s, Mab1BwdWs* out, void* base) {
  Carver c(base);
  Mab1BwdWs w;
  const size_t M = (size_t)s.B * s.nq, d = s.d;
  w.WoTP = c.take<__bf16>(d * d);
  w.WqTP = c.take<__bf16>(d * d);
  w.dZ = c.take<__bf16>(M * d);
  w.dQp = c.take<__bf16>(M * d);
  w.dOs = c.take<__bf16>(M * d);
  w.dS = c.take<__bf16>(M * s.h * s.nk);
  w.P = c.take<__bf16>(M * s.h * s.nk);
  w.dKp = c.take<float>((size_t)s.B * s.nk * d);
  w.dVp = c.take<float>((size_t)s.B * s.nk * d);
  const size_t tiles = (size_t)cdiv(s.nq, M1_TP);
  w.dKpPart = c.take<float>((size_t)s.B * tiles * s.nk * d);
  w.dVpPart = c.take<float>((size_t)s.B * tiles * s.nk * d);
  if (out) *out = w;
  return c.off;
}

size_t mab1_bf16_bwd_ws_bytes(const pca_mab_shape& s) {
  return mab1_carve_bwd_ws(s, nullptr, nullptr);
}

int kv_dh_launch(const float* dKp, const float* dVp, const float* Wk, const float* Wv, float* dH,
                 int B, int m, int d, int accumulate, hipStream_t st) {
  PCA_REQUIRE(d == 128 && m <= 16, "kv_dh: d=%d m=%d", d, m);
  hipLaunchKernelGGL(k_kv_dh, dim3(B), dim3(256), 2 * (size_t)m * d * sizeof(float), st, dKp, dVp,
                     Wk, Wv, dH, m, d, accumulate);
  return check_launch("k_kv_dh");
}

// Fused mode (m = 16): consecutive tiles per workgroup - the largest divisor of tiles_per_set that still
// leaves >= 256 workgroups (without the dX stage the kernel needs 72 KiB of LDS, two workgroups per CU:
// 512).  tiles_per_set / this is the number of dKp / dVp partials per set the mid chain sums.
static int fused_tiles_per_wg(int B, int tiles_per_set, bool want_dx) {
  const int min_wg = want_dx ? 256 : 512;
  int tpw = 1;
  for (int c = 1; c <= tiles_per_set; ++c)
    if (tiles_per_set % c == 0 && (int64_t)B * tiles_per_set / c >= min_wg) tpw = c;
  return tpw;
}

// dQ -> dX [B, nq, dq] (written; may be null), dK -> dH [B, nk, d] (written or accumulated)
int mab1_bf16_bwd_ex(const pca_mab_shape& s, const void* X, const float* H,
                     const pca_mab_params& p, const void* saved, const void* dY, void* dX,
                     float* dH, int dk_accumulate, const pca_mab_grads& gr, void* ws, int flags,
                     hipStream_t st, const IsabImg* img, float* zero_ptr, int zero_n,
                     int* nparts_out, StepCtx* ctx) {
  PCA_REQUIRE(s.d == 128, "mab1_bf16_bwd: d = 128 only (d = 256: mab1_d256_bwd)");
  BwdDefer* const defer = defer_of(ctx);
  Mab1Saved v;
  mab1_carve_saved(s, &v, const_cast<void*>(saved));
  Mab1BwdWs w;
  mab1_carve_bwd_ws(s, &w, ws);
  const int d = s.d, MI = s.nk;
  const int64_t M = (int64_t)s.B * s.nq;
  const bool small = s.dq <= 4;
  const bool want_dx = dX != nullptr && !small;
  const bool abf = s.y_dtype == PCA_BF16;
  if (dX != nullptr && small) {
    // the ST model never needs it (the set itself is the input of layer 1)
    set_error("mab1_bf16_bwd: dQ for dq <= 4 is not built");
    return PCA_EUNSUPPORTED;
  }

  if (img != nullptr) {
    w.WoTP = img->WoTP;
    w.WqTP = img->WqTP;
  } else {
    PCA_TRY(prep_weight(p.wo, w.WoTP, d, d, 2, st));
    if (want_dx) PCA_TRY(prep_weight(p.wq, w.WqTP, d, d, 2, st));
  }

  // dZ = dY . [Z > 0] is read by the fc_o weight-gradient job only: with bf16 gradients and whole
  // 128-point mask blocks per set that job takes dY and the mask words (WgradJob::mask) and dZ is
  // never written (PCA_D128_DZ_MASK=0: the materialised form)
  const TailForm form = tail_form_of(defer);
  const bool dz_masked = form.dz_mask && abf && MI == 16 && s.nq % 128 == 0;
  Mab1BwdArgs a{};
  a.dY = dY; a.QpS = v.QpS; a.mask = v.mask; a.KpP = v.KpP; a.VpP = v.VpP; a.Kt = v.Kt;
  a.WoTP = w.WoTP; a.WqTP = w.WqTP; a.dZ = dz_masked ? nullptr : w.dZ; a.dQp = w.dQp; a.dOs = w.dOs; a.dS = w.dS;
  a.P = w.P; a.dX = want_dx ? dX : nullptr;
  a.B = s.B; a.N = s.nq; a.tiles_per_set = (int)cdiv(s.nq, TP);
  a.scale = 1.0f / sqrtf((float)d);
  a.scale_log2e = LOG2E * a.scale;
#ifdef PCA_DEBUG_CLOCKS
  a.dbg_wg = getenv("PCA_DBG_WG") ? atoi(getenv("PCA_DBG_WG")) : 0;
#else
  a.dbg_wg = 0;
#endif
  // reference-formulation FLOPs of what THIS launch computes (round 3: not the whole block's
  // backward - dWo and, beyond layer 1, dWq run in k_wgrad128 and are charged there): fc_o adjoint
  // dO = dY + dZ Wo (2 M d^2), attention adjoint (recomputed scores, dP, dQp, dKp, dVp: 8 M m d),
  // dX = dQp Wq (2 M dq d) when asked for, layer 1's in-kernel dWq (2 M dq d)
  const double flops = (double)M * (2.0 * d * d + 8.0 * MI * d +
                                    (want_dx ? 2.0 * s.dq * d : 0.0) +
                                    ((small && s.dq <= 3 && MI == 16) ? 2.0 * s.dq * d : 0.0));
  // algorithmic HBM bytes (each operand once): dY in, X in, dX out
  const double eb = abf ? 2.0 : 4.0;
  const double bytes = (double)M * (eb * d + (small ? 4.0 * s.dq : eb * s.dq) +
                                    (want_dx ? eb * d : 0.0));
  int rc;
  const bool fuse = MI == 16;
  if (fuse) {
    const int tpw = fused_tiles_per_wg(a.B, a.tiles_per_set, want_dx);
    a.tpw = tpw;
    a.dKpG = w.dKpPart;
    a.dVpG = w.dVpPart;
    a.zero_ptr = zero_ptr;
    a.zero_n = zero_n;
#ifdef PCA_DEBUG_CLOCKS
    a.dbg = debug_clock_buffer(want_dx ? 1 : 0);
#endif
    const bool fwq = small && s.dq <= 3;
    a.Xs = reinterpret_cast<const float*>(X); a.dWqS = gr.wq; a.dbqS = gr.bq; a.dq = s.dq;
    a.WqF = p.wq; a.bqF = p.bq;
    // slab mode: the (unused in this mode) dS block of the workspace holds the fc_q partials
    if (fwq && form.slabs && (128 * s.dq) % 4 == 0 &&
        (size_t)a.B * a.tiles_per_set / tpw * (128 * s.dq + 128) * 4 <= (size_t)M * s.h * s.nk * 2)
      a.wq_slab = reinterpret_cast<float*>(w.dS);
    if (abf)
      rc = want_dx ? launch_bwd<128, 16, true, true, false, true>(a, st, flops, bytes)
           : fwq   ? launch_bwd<128, 16, false, true, true, true>(a, st, flops, bytes)
                   : launch_bwd<128, 16, false, true, false, true>(a, st, flops, bytes);
    else
      rc = want_dx ? launch_bwd<128, 16, true, true, false, false>(a, st, flops, bytes)
           : fwq   ? launch_bwd<128, 16, false, true, true, false>(a, st, flops, bytes)
                   : launch_bwd<128, 16, false, true, false, false>(a, st, flops, bytes);
  } else {
    PCA_REQUIRE(!abf, "mab1_bf16_bwd: bf16 activations need m = 16");
    rc = want_dx ? launch_bwd<128, 32, true, false, false, false>(a, st, flops, bytes)
                 : launch_bwd<128, 32, false, false, false, false>(a, st, flops, bytes);
  }
  PCA_TRY(rc);
  if (a.wq_slab != nullptr) {        // fc_q of layer 1: the workgroups' partials, summed in a fixed order
    const int nwg = a.B * a.tiles_per_set / a.tpw, n1 = 128 * s.dq, stride = n1 + 128;
    SlabSumJobs two{};
    two.j[two.n++] = SlabSumJob{a.wq_slab, gr.wq, nwg, n1, 1, stride};
    two.j[two.n++] = SlabSumJob{a.wq_slab + n1, gr.bq, nwg, 128, 1, stride};
    if (defer != nullptr) {
      PCA_REQUIRE(defer->late.n + 2 <= 40, "mab1_bf16_bwd: slab-sum table full");
      defer->late.j[defer->late.n++] = two.j[0];
      defer->late.j[defer->late.n++] = two.j[1];
    } else {
      PCA_TRY(slab_sum_jobs(two, st));
    }
  }
  if (nparts_out != nullptr) *nparts_out = fuse ? a.tiles_per_set / a.tpw : 0;
  // ---- reductions over points (one launch for dWo / dWq when both operands are bf16) ----
  // 512 rows per workgroup: the fp32 atomics of the [128 x 128] result cost ~1 lane-op per
  // clock per L2 channel, so fewer, longer workgroups win (256 rows: +50 %, 64 rows: 4x)
  const int rows_per_wg = 512;
  const bool wq_big = !small;
  {
    WgradJobs jobs{};
    if (dz_masked)
      jobs.j[jobs.n++] = WgradJob{dY, v.OS, gr.wo, gr.bo, M, 0, 128, nullptr, v.mask};
    else
      jobs.j[jobs.n++] = WgradJob{w.dZ, v.OS, gr.wo, gr.bo, M, 0, 128};
    if (wq_big && abf) jobs.j[jobs.n++] = WgradJob{w.dQp, X, gr.wq, gr.bq, M, 0, 128};
    if (defer != nullptr) {
      PCA_TRY(wgrad128_defer(defer, jobs, true, rows_per_wg, st));
    } else {
      ProfScope ps(PCA_K_WGRAD, st, 2.0 * jobs.n * M * d * d, 4.0 * jobs.n * M * d);
      PCA_TRY(wgrad128_launch(jobs, true, true, rows_per_wg, st));
      ps.end();
    }
  }
  if (small && fuse && s.dq <= 3) {
    // dWq / dbq were reduced inside the chain kernel
  } else if (small) {
    PCA_TRY(wgrad_small_bf16_launch(w.dQp, reinterpret_cast<const float*>(X), M, s.dq, gr.wq, gr.bq, st));
  } else if (!abf) {
    WgradJobs jobs{};
    jobs.j[0] = WgradJob{w.dQp, X, gr.wq, gr.bq, M, 0, 128};
    jobs.n = 1;
    ProfScope ps(PCA_K_WGRAD, st, 2.0 * M * d * d, 6.0 * M * d);
    PCA_TRY(wgrad128_launch(jobs, true, false, rows_per_wg, st));
    ps.end();
  }
  if (!fuse) {
    hipLaunchKernelGGL((k_kv_grad<32>), dim3(s.B * s.h), dim3(256), 0, st, w.dS, w.P, v.QpS,
                       w.dOs, s.nq, d, s.h, w.dKp, w.dVp);
    PCA_TRY(check_launch("k_kv_grad"));
  }

  if (flags & PCA_F_SKIP_KV_TAIL) return PCA_OK;
  if (fuse) {        // stand-alone MAB: sum the per-workgroup partials
    const int nparts = a.tiles_per_set / a.tpw;
    hipLaunchKernelGGL(k_sum_parts, dim3((unsigned)cdiv((int64_t)s.B * MI * d, 256)), dim3(256), 0,
                       st, w.dKpPart, w.dVpPart, w.dKp, w.dVp, s.B, nparts, MI * d);
    PCA_TRY(check_launch("k_sum_parts"));
  }
  // ---- fc_k / fc_v of the m inducing-point outputs: [B*m]-row reductions, one launch ----
  const int64_t Mk = (int64_t)s.B * MI;
  {
    WgradJobs jobs{};
    jobs.j[0] = WgradJob{w.dKp, H, gr.wk, gr.bk, Mk, 0, 128};
    jobs.j[1] = WgradJob{w.dVp, H, gr.wv, gr.bv, Mk, 0, 128};
    jobs.n = 2;
    PCA_TRY(wgrad128_launch(jobs, false, false, 64, st));
  }
  if (dH != nullptr) {
    if (MI <= 16) {
      PCA_TRY(kv_dh_launch(w.dKp, w.dVp, p.wk, p.wv, dH, s.B, MI, d, dk_accumulate ? 1 : 0, st));
    } else {
      PCA_TRY(linear_dx_acc_f32(w.dKp, p.wk, dH, Mk, d, d, dk_accumulate ? 1 : 0, st));
      PCA_TRY(linear_dx_acc_f32(w.dVp, p.wv, dH, Mk, d, d, 1, st));
    }
  }
  return PCA_OK;
}

}  // namespace pca

// For tests, outside the documented ABI: the number of dKp / dVp partials per set that the many-queries
// backward of an ISAB (m = 16) leaves for the mid chain, B sets of N points; want_dx: the layer also
// returns dX (every layer but the first).
extern "C" int pca_debug_mid_nparts(int B, int N, int want_dx) {
  if (B <= 0 || N <= 0) return -1;
  const int tiles = (int)pca::cdiv(N, pca::TP);
  return tiles / pca::fused_tiles_per_wg(B, tiles, want_dx != 0);
}
