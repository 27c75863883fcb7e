// Set-resident forward of the d = 128 / 4 heads / m = 16 inducing points / k = 1 Set Transformer
// (Code/models.py:34-44: ISAB, ISAB, PMA; set_transformer-master/modules.py:19-33, 51-53, 62-63),
// BASELINE configs[1] (N = 512, din = 2, B = 128).
//
// A PAIR of 1024-thread workgroups carries ONE set through
//     mab0(I1, X) -> mid -> mab1(X, H1) -> mab0(I2, Y1) -> mid -> mab1(Y1, H2) -> PMA attention partials
// each workgroup with ITS HALF of the set's [N, 128] bf16 activation tensor resident in LDS from the
// moment layer 1 produces it until the PMA has read it (B = 128 sets -> 256 workgroups = one per CU).
// The per-block kernels this replaces (k_mab0_attn_small, k_mid_fwd, k_mab1_fwd, k_mab0_attn_h4,
// k_mid_fwd, k_isab1_fwd_t, k_mab0_attn) each ran ONE 32-point unit per wave with all 2048 waves of
// the chip in the same phase at the same time: every launch paid its weight images, the input burst,
// the dependent MFMA chain and the store drain in lock-step, plus ~5 us of launch and drain - seven
// times per forward.  Here a phase boundary is a workgroup barrier, the activations between blocks
// never leave the CU (they go to HBM only as the tensors the backward reads), and the only
// cross-workgroup traffic of a set is the (m, l, T) partial of its two few-queries attentions, handed
// to the partner workgroup through write-through (sc1) stores, one flag and sc1 loads
// (cdna_hip_programming.md Guideline 16, R1); both halves then merge the same two partials in the same
// order and run the per-set "mid" stage redundantly, so nothing else has to cross.
//
// Wave w = (quad q = w >> 2, head j = w & 3): quad q owns a quarter of the workgroup's points, wave j of
// a quad the head j (features 32 j .. 32 j + 31) - the WAVE = HEAD, WEIGHTS IN REGISTERS form of
// k_isab1_fwd_t (d128_fused.hip) and k_mab0_attn_h4 (mab0_bf16.hip), whose arithmetic and saved layouts
// this kernel keeps (same MFMA operand orders, same K-permuted images), so that the existing backward
// kernels read what it saves.
//
// LDS: sY [N/2][256 B] (rows XOR-swizzled by y_off, so that the row-major operand reads, the transposing
// ds_read_tr16_b64 reads and the whole-row reads are conflict-free), sO [N/2][256 B] (the O tile of a many-queries
// block: fc_o contracts over all heads' features; between blocks: merge buffers), 32 KiB of images.
//
// Roofline unit: MACs_fwd / set = N (3 din d + 7 d^2 + 8 m d + 2 k d) + 6 m d^2 (the
// PMA epilogue and the classifier run in k_pma_head1); algorithmic bytes 4 N din + 4 (2 N d) per set.
#include "set128.hpp"
#include "mfma_common.hpp"
#include "softmax_merge.hpp"

#include <math.h>

#include <type_traits>

namespace pca {

namespace {

constexpr int D = 128, MQ = 16, ROWB = 256, NT = 1024;

// byte offset of 16-byte chunk ch of row `row` of a [rows][256 B] image.  The XOR term depends on row & 15
// only (any 16-aligned row block is an image); as a map of the row's four bits it is linear with the
// columns 2, 4, 8, 9, the one that keeps all three read shapes of the kernel conflict-free under the
// lane groups of MI355X_MICROARCH.md §LDS: ds_read_b128 of the operand rows (lane = (chunk 4 s + g, row r),
// 16-lane groups {0-3, 12-15, 20-27} ..), ds_read_b64_tr_b16 (two 32-lane groups: rows 4 g + q, chunks
// 2 t and 2 t + 1) and the ds_read_b128 of whole rows for the coalesced stores (4 rows per instruction).
// (k_mab0_attn_h4's term ((row & 3) << 2) | ((row >> 2) & 3), used here before, is 2-way on all three.)
// The ds_write_b64 of accumulator tiles (16 lanes = 16 rows, one 8-byte half of the same chunk) stay
// 2-way under any 16-byte swizzle.
__device__ __forceinline__ int y_off(int row, int ch) {
  return 256 * row + 16 * (ch ^ ((((row << 1) & 14) | ((row >> 3) & 1)) ^ (row & 8)));
}
// B operand [k = point (k-slot order of pack8 of two score tiles)][col = feature 16 t + (lane & 15)] of
// the 32-row image `img`, through the transposing LDS read
__device__ __forceinline__ bf16x8 y_tr_frag(const char* img, int t, int lane) {
  const int g = lane >> 4, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
  const int a0 = y_off(4 * g + q, 2 * t + (p >> 1)) + 8 * (p & 1);
  const int a1 = y_off(16 + 4 * g + q, 2 * t + (p >> 1)) + 8 * (p & 1);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + a0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + a1));
  const bf16x4 l4 = __builtin_bit_cast(bf16x4, lo), h4 = __builtin_bit_cast(bf16x4, hi);
  bf16x8 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) { r[e] = l4[e]; r[4 + e] = h4[e]; }
  return r;
}
// accumulator tile (rows = features 16 t + 4 g + e, col = query r) -> [query][feature] bf16 image
__device__ __forceinline__ void put_tile(char* img, int t, int r, int g, f32x4 v) {
  *reinterpret_cast<bf16x4*>(img + swz(r, 2 * t + (g >> 1), ROWB) + 8 * (g & 1)) = pack4(v);
}
// (lds_barrier() of mfma_common.hpp: global stores in flight - the saved tensors - are not waited for)
// max0 (as max_nn of mfma_common.hpp): ONE instruction (v_med3_f32 with +inf; fmaxf costs a canonicalising
// v_max x, x in front).  A builtin, NOT inline asm: hipcc's hazard recognizer does not look inside asm, and
// a VALU instruction reading an MFMA result needs wait states it would not insert (the first version of
// this kernel read the accumulators of the mid stage one instruction after the MFMA - and got the old value)
__device__ __forceinline__ float max0(float x) { return __builtin_amdgcn_fmed3f(x, 0.f, INFINITY); }
// bits = 2 bits + (z > 0)
__device__ __forceinline__ uint32_t push_gt0(uint32_t bits, float z) {
  return (bits << 1) | (z > 0.f ? 1u : 0u);
}

// ---- global accesses: workgroup-uniform base + UNSIGNED 32-bit byte offset of the lane (+ a constant) ----
// Every tensor this kernel touches has a base that is uniform over the workgroup (kernel argument, set index,
// half, wave): the base stays in a scalar register pair, the lane contributes one 32-bit VGPR, and hipcc emits
// `global_* v_off, .., s[base:base+1] offset:imm` - no 64-bit address pair, no v_lshl_add_u64 / v_ashrrev per
// access.  Offsets that differ by a compile-time constant share the VGPR (`cbytes`, the immediate where it
// fits).  set128_shape_ok() keeps every tensor below 2^31 bytes.
// The part of `cbytes` beyond the 12-bit immediate is added to the lane offset (one 32-bit v_add): left in the
// address, hipcc adds it to (base + lane offset) on the vector ALU as a 64-bit pair.  (NOT to the base behind an
// empty asm that pins the sum to scalar registers: hipcc's hazard recognizer counts an empty asm as one wait
// state, and one landed between an MFMA and the first VALU read of its result - the read then came one s_nop
// early and the <2, 2> instances returned different bits from pass to pass.)
template <class T>
__device__ __forceinline__ T* lane_ptr(T* base, uint32_t bytes, int cbytes = 0) {
  typedef typename std::conditional<std::is_const<T>::value, const char, char>::type byte_t;
  if (__builtin_constant_p(cbytes) && (cbytes < 0 || cbytes > 4095)) {
    bytes += (uint32_t)(cbytes & ~4095);
    cbytes &= 4095;
  }
  return reinterpret_cast<T*>(reinterpret_cast<byte_t*>(base) + bytes + cbytes);
}
template <class V, class T>
__device__ __forceinline__ V& lane_ref(T* base, uint32_t bytes, int cbytes = 0) {
  return *reinterpret_cast<V*>(lane_ptr(base, bytes, cbytes));
}
template <class V, class T>
__device__ __forceinline__ const V& lane_ref(const T* base, uint32_t bytes, int cbytes = 0) {
  return *reinterpret_cast<const V*>(lane_ptr(base, bytes, cbytes));
}

// a lane-dependent index at the top of a basic block, as a value the optimiser forms offsets from afresh.
// (An empty asm like rederive()'s: only right behind a barrier - hipcc's hazard recognizer counts it as a wait
// state, so it must never stand between an MFMA and the reader of its result.)
__device__ __forceinline__ int relane(int t) {
  asm volatile("" : "+v"(t));
  return t;
}

// ---- cross-workgroup hand-off (cdna_hip_programming.md Guideline 16, form R1): payload by sc1
// (write-through) stores, every storing wave drains, workgroup barrier, ONE lane stores the flag; the
// consumer polls the flag (bounded), then reads the payload with sc1 loads only -------------------
typedef __attribute__((address_space(1))) uint32_t gu32;
__device__ __forceinline__ void st16_sc1(float* p, float4 v4) {
  const f32x4 v = {v4.x, v4.y, v4.z, v4.w};
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
// the payload loads: buffer_load_dwordx4 .. sc1 through the builtin (cache-policy bit 4 = sc1 on gfx942 / gfx950),
// NOT an asm load: an asm hands the compiler the destination registers of a load that is still in flight as an
// ordinary value and needs a hand-counted wait; these hipcc counts in vmcnt like every other load, so it waits for
// them alone in front of their first use and leaves younger plain loads in flight.  `bytes`: the range of the
// descriptor (raw buffer, stride 0; word 3 = 32-bit data format, as for every gfx9 raw buffer)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t payload_rsrc(const float* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ f32x4 ld16_buf_sc1(__amdgpu_buffer_rsrc_t rs, uint32_t lane_bytes, int wave_bytes) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_bytes, wave_bytes, 16);
  return __builtin_bit_cast(f32x4, v);
}
__device__ __forceinline__ void drain_vm() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void flag_store(uint32_t* f, uint32_t v) {
  __hip_atomic_store((gu32*)(f), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one wave polls; a partner that never arrives (it would mean the pair is not co-resident) ends the
// spin after ~1 s, counts it in tmo[0] and lets the kernel finish with whatever the slot holds
__device__ __forceinline__ void flag_wait(uint32_t* f, uint32_t want, uint32_t* tmo) {
  for (unsigned spins = 0; spins < (1u << 20); ++spins) {
    if (__hip_atomic_load((gu32*)(f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == want) return;
    __builtin_amdgcn_s_sleep(4);
  }
  if ((threadIdx.x & 63) == 0) atomicAdd(tmo, 1u);
}

// -DPCA_SET_STAMPS (scripts/experiments/set_stamps.sh): wall-clock stamps (10 ns units) of workgroup 0,
// lane 0 of every wave, at the phase boundaries
#ifdef PCA_SET_STAMPS
__device__ unsigned long long g_set_stamps[16 * 32];
#define STAMP(i)                                                                         \
  do {                                                                                   \
    if (blockIdx.x == 0 && (threadIdx.x & 63) == 0)                                      \
      g_set_stamps[(threadIdx.x >> 6) * 32 + (i)] = wall_clock64();                      \
  } while (0)
#else
#define STAMP(i) do { } while (0)
#endif

// ---- variable-length sets (template parameter LEN of the kernel; Set128FwdArgs::lengths) ---------
// The points at and beyond len = min(lengths[b], N) are no keys: their scores are -inf before the running
// max, a 32-point unit (a wave's range of pairs in layer 1) that lies wholly beyond len skips its arithmetic
// and leaves the EMPTY partial (m, l, t) = (-inf, 0, 0), and every merge of two partials takes its factors
// from fac<LEN> (softmax_merge.hpp), for which the empty partial is the identity.  len is uniform over the
// workgroup, so is every skip; masking and skipping remove ARITHMETIC ONLY: whatever len is, every
// workgroup of a pair reaches every barrier, stores every flag, waits for every flag and writes complete
// hand-off payloads (an empty partial travels as zeros with m = -inf).  len >= 1: point 0 is a key, so half 0
// of a set, and with it every merge across the halves, has a finite max.  LEN = false: the dense kernel,
// the expressions it always had.
template <bool LEN>
__device__ __forceinline__ float fac(float m, float M) {
  if constexpr (LEN) return merge_factor(m, M);
  else return __builtin_amdgcn_exp2f(m - M);
}

// round B of layer 2's quad merge: take_partial's line T a1 + o a2 for one tile, written out as the instructions
// hipcc made of it in every instance while quad 0 ran it over its eight tiles (the saved tensors and the hashes
// of the tests are those bits): elements 0 and 1 round T a1 and fuse o a2 onto it (v_pk_mul, v_pk_fma), elements
// 2 and 3 round both products and add them (v_mul, v_mul, v_pk_add).  Contraction is off in here, so that the
// products that were rounded stay rounded whatever the surrounding code makes the vectoriser do.
__device__ __forceinline__ f32x4 round_b_tile(float4 t, float4 a1, float4 o, float4 a2) {
#pragma clang fp contract(off)
  f32x4 v;
  v[0] = __builtin_fmaf(o.x, a2.x, t.x * a1.x);
  v[1] = __builtin_fmaf(o.y, a2.y, t.y * a1.y);
  v[2] = t.z * a1.z + o.z * a2.z;
  v[3] = t.w * a1.w + o.w * a2.w;
  return v;
}

struct Ctx {
  int b, half, N, NH, tid, lane, wave, q, j, r, g;
  int UPQ;          // 32-point units per quad (N / 256)
  int qn0;          // first LOCAL row (of sY / sO) of this wave's quad
  int64_t row0;     // global row (b N + half N/2) of local row 0
};

// ---------------------------------------------------------------------------------------------
// per-set stage between the two blocks of an ISAB (k_mid_fwd, mid_bf16.hip, on 16 waves), run by BOTH
// workgroups of the pair on identical inputs (half 0 writes the saved copies):
//   A  O = Qp + T_h Wv_h^T + bv        (modules.py:29, reassociated: SURVEY 8d)     waves 0-7, tile t = wave
//   B  H = O + relu(O Wo^T + bo)       (modules.py:31)                              waves 0-7
//   C  Kp = H Wk^T + bk, Vp = H Wv^T + bv of the many-queries block (modules.py:21) all waves:
//      wave = (tile tc = wave >> 1, which = wave & 1); the two images the forward reads stay in LDS
//      (sKp: K-permuted [key][feature], sVt: [feature][key]), all four go to memory for the backward
// Every weight fragment a wave needs is requested by mid_prefetch() a phase ahead.
// ---------------------------------------------------------------------------------------------
struct MidPre {
  bf16x8 wa[4], wb[4], wc[4];
  float wvf[4][4];                 // SMALL: Wv0f[feature 16 t + 4 g + e][c]
  float4 qp, bv0, bo0, bkv;
  float bkvc;
};

// PART: 1 = what stages A and B read (qp, bv0, bo0, wa, wb), 2 = stage C's (wc, bkv, bkvc), 3 = both
template <bool SMALL, int PART = 3>
__device__ __forceinline__ void mid_prefetch(const Set128Layer& L, const Ctx& c, int dk, MidPre& P) {
  const int r = c.r, g = c.g;
  if (PART & 1) {
    // (waves 8-15 load the fragments of tile wave - 8 and never use them: under `if (wave < 8)` hipcc
    //  spilled every value of this block right behind its load, each with an s_waitcnt vmcnt(0))
    // (the tile is the wave's: it goes into the scalar bases; oW: the lane's 16 bytes of row r of a bf16 image)
    // waves 8-15 never use what they load here: all their lanes ask for the tile's first 16 bytes (one line per
    // request instead of sixteen)
    const int t = c.wave & 7;
    const uint32_t used = c.wave < 8 ? ~0u : 0u;
    const uint32_t oW = (256u * r + 16u * g) & used, o16 = (16u * g) & used;
    P.qp = lane_ref<float4>(L.Qp0 + 16 * t, (512u * r + 16u * g) & used);
    P.bv0 = lane_ref<float4>(L.bv0 + 16 * t, o16);
    P.bo0 = lane_ref<float4>(L.bo0 + 16 * t, o16);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if (!SMALL) P.wa[ks] = lane_ref<bf16x8>(L.Wv0 + 16 * t * D, oW, 64 * ks);
      P.wb[ks] = lane_ref<bf16x8>(L.Wo0 + 16 * t * D, oW, 64 * ks);
    }
    if (SMALL) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
          P.wvf[e][cc] = cc < dk ? lane_ref<float>(L.Wv0f + 16 * t * dk, (16u * g * dk) & used, 4 * (e * dk + cc)) : 0.f;
    }
  }
  if (PART & 2) {
    const int tc = c.wave >> 1, which = c.wave & 1;
    const __bf16* W = which ? L.Wv1 : L.Wk1;
    const float* bias = which ? L.bv1 : L.bk1;
    const uint32_t oW = 256u * r + 16u * g;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) P.wc[ks] = lane_ref<bf16x8>(W + 16 * tc * D, oW, 64 * ks);
    P.bkv = lane_ref<float4>(bias + 16 * tc, 16u * g);
    P.bkvc = lane_ref<float>(bias + 16 * tc, 4u * r);
  }
}

// sT: bf16 image [64][256 B] of the merged T (swz rows; !SMALL) / sTf: fp32 [64][4] (SMALL);
// sA, sH: [16][256 B] bf16 images of O and H.  Ends with a barrier.
// after_a(): requests of the NEXT phase, issued behind the barrier that ends stage A (a wave issues its loads in
// order: in front of stage A they would hold waves 0-7 back while the memory pipeline takes them in)
template <bool SMALL, class AfterA>
__device__ __forceinline__ void mid_stage(const Set128Layer& L, const Ctx& c, const MidPre& P,
                                          const char* sT, const float* sTf, char* sA, char* sH,
                                          char* sKp, char* sVt, AfterA after_a) {
  const int r = c.r, g = c.g, b = c.b;
  const bool save = c.half == 0;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  if (c.wave < 8) {                                   // ---- A
    const int t = c.wave, hh = t >> 1;
    o = f32x4{P.qp.x + P.bv0.x, P.qp.y + P.bv0.y, P.qp.z + P.bv0.z, P.qp.w + P.bv0.w};
    if (SMALL) {
      const float4 t4 = *reinterpret_cast<const float4*>(sTf + (16 * hh + r) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        o[e] += t4.x * P.wvf[e][0] + t4.y * P.wvf[e][1] + t4.z * P.wvf[e][2] + t4.w * P.wvf[e][3];
    } else {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        o = mfma32(P.wa[ks], *reinterpret_cast<const bf16x8*>(sT + swz(16 * hh + r, 4 * ks + g, ROWB)), o);
    }
    put_tile(sA, t, r, g, o);
    if (save)
      lane_ref<float4>(L.O0 + (int64_t)b * MQ * D + 16 * t, 512u * r + 16u * g) = float4{o[0], o[1], o[2], o[3]};
  }
  lds_barrier();
  STAMP(SMALL ? 28 : 30);                           // stage A done (the stamps of B: 29 / 31)
  after_a();
  if (c.wave < 8) {                                   // ---- B
    const int t = c.wave;
    f32x4 z = f32x4{P.bo0.x, P.bo0.y, P.bo0.z, P.bo0.w};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      z = mfma32(P.wb[ks], *reinterpret_cast<const bf16x8*>(sA + swz(r, 4 * ks + g, ROWB)), z);
    f32x4 hq;
#pragma unroll
    for (int e = 0; e < 4; ++e) hq[e] = o[e] + max0(z[e]);
    if (save) {
      const int64_t base = (int64_t)b * MQ * D + 16 * t;
      const uint32_t off = 512u * r + 16u * g;
      lane_ref<float4>(L.Z0 + base, off) = float4{z[0], z[1], z[2], z[3]};
      lane_ref<float4>(L.H + base, off) = float4{hq[0], hq[1], hq[2], hq[3]};
    }
    put_tile(sH, t, r, g, hq);
  }
  lds_barrier();
  STAMP(SMALL ? 29 : 31);
  {                                                   // ---- C
    const int tc = c.wave >> 1, which = c.wave & 1;
    f32x4 fr = f32x4{P.bkv.x, P.bkv.y, P.bkv.z, P.bkv.w};     // rows = features, col = key
    f32x4 kr = f32x4{P.bkvc, P.bkvc, P.bkvc, P.bkvc};         // rows = keys,     col = feature
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf16x8 hf = *reinterpret_cast<const bf16x8*>(sH + swz(r, 4 * ks + g, ROWB));
      fr = mfma32(P.wc[ks], hf, fr);
      kr = mfma32(hf, P.wc[ks], kr);
    }
    const bf16x4 krp = pack4(kr), frp = pack4(fr);
    // [feature][key] image: keys 4g .. 4g+3 of feature 16 tc + r (8 contiguous bytes);
    // K-permuted [key][feature] image: features 32 (tc >> 1) + perm32(8 g + 4 (tc & 1) + e) of key r -
    // half of the lane's 16 bytes (k_mid_fwd writes pack8 of the head's two tiles)
    const int o_t = (16 * tc + r) * MQ + 4 * g;
    const int o_p = r * D + 32 * (tc >> 1) + 8 * g + 4 * (tc & 1);
    if (which) *reinterpret_cast<bf16x4*>(sVt + o_t * 2) = krp;
    else *reinterpret_cast<bf16x4*>(sKp + o_p * 2) = frp;
    if (save) {
      __bf16* PP = which ? L.VpP : L.KpP;
      __bf16* TT = which ? L.Vt : L.Kt;
      lane_ref<bf16x4>(TT + (int64_t)b * D * MQ, 2u * o_t) = krp;
      lane_ref<bf16x4>(PP + (int64_t)b * MQ * D, 2u * o_p) = frp;
    }
  }
  lds_barrier();
}

// ---------------------------------------------------------------------------------------------
// many-queries block mab1(X, H) (modules.py:19-33) on the workgroup's rows; wave = (quad, head):
//   Qp_h = fc_q(x) ; A = softmax(Qp_h Kp_h^T / sqrt d) ; O_h = Qp_h + A Vp_h -> own slice of sO
//   barrier ; Z_h = fc_o(O) ; Y_h = O_h + relu(Z_h) -> own slice of sY ; barrier
//   coalesced stores of the saved O (from sO) and of Y (from sY)
// SMALL: layer 1 (dq = din <= 4: fc_q on the vector ALU from the points in sX, nothing in sY yet)
// ---------------------------------------------------------------------------------------------
template <bool SMALL, int DQ, int UPQ>
__device__ __forceinline__ void mab1_phase(const Set128Layer& L, const Ctx& c, char* sY, char* sO,
                                           const float* sX, const char* sKp, const char* sVt,
                                           float scale_log2e, int stamp0, bf16x8 (&wa)[4][2]) {
  (void)stamp0;
  const int r = c.r, g = c.g, j = c.j;
  constexpr int KS = 4;
  // this head's weight slices as A operands [row = feature 32 j + 16 t + r][k-slots 32 s + 8 g ..]:
  // wa arrives holding fc_q's (requested by the caller one stage ahead: mab1_load_wq)
  float wqs[2][4][SMALL ? DQ : 1];
  if (SMALL) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int cc = 0; cc < DQ; ++cc)
          wqs[t][e][SMALL ? cc : 0] = lane_ref<float>(L.WqF + 32 * j * DQ, 16u * g * DQ, 4 * ((16 * t + e) * DQ + cc));
  }
  f32x4 bqv[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float4 q4 = lane_ref<float4>(L.bq1 + 32 * j, 16u * g, 64 * t);
    bqv[t] = f32x4{q4.x, q4.y, q4.z, q4.w};
  }
  // the head's 16 keys: A operand [key r][k-slots 8 g .. of the head's 32 features] and
  // V^T: A operand [feature 16 t + r][keys 4 g ..]
  const bf16x8 kpa = *reinterpret_cast<const bf16x8*>(sKp + (r * D + 32 * j + 8 * g) * 2);
  bf16x4 vta[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
    vta[t] = *reinterpret_cast<const bf16x4*>(sVt + ((32 * j + 16 * t + r) * MQ + 4 * g) * 2);

  // per-lane byte offsets inside a 16-row block of sY / sO (y_off depends on row & 15 only); each
  // set is computed where its phase starts - held from the top they cost 14 registers the kernel does
  // not have (a spilled index reloaded next to a prefetch makes the reload's vmcnt(0) wait for it)
  int oB[KS], oD[2];
  // saved Qp: the head's 64 bytes of the quad's rows; the lane's chunk of row r
  __bf16* const qps = (SMALL && DQ != 4) ? nullptr : L.QpS + (c.row0 + c.qn0) * D + 32 * j;
  const uint32_t oQ = 256u * r + 16u * chunk_of(g);
#pragma unroll
  for (int s = 0; s < KS; ++s) oB[s] = y_off(r, 4 * s + g);
#pragma unroll
  for (int t = 0; t < 2; ++t) oD[t] = y_off(r, 4 * j + 2 * t + (g >> 1)) + 8 * (g & 1);

#pragma unroll
  for (int u = 0; u < UPQ; ++u) {     // (a compile-time bound: both units of a wave in ONE basic block, so
                                      //  that hipcc interleaves their dependent MFMA -> softmax -> MFMA chains)
    const int n0 = c.qn0 + 32 * u;
    f32x4 acc[2][2];
    if (SMALL) {
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const float4 x4 = *reinterpret_cast<const float4*>(sX + (n0 + 16 * nb + r) * 4);
        const float xc[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float v = bqv[t][e];
#pragma unroll
            for (int cc = 0; cc < DQ; ++cc) v += wqs[t][e][SMALL ? cc : 0] * xc[cc];
            acc[t][nb][e] = v;
          }
      }
      if (DQ == 4) {
        // the backward reads them at dq = 4 (mab1_saves_qp: k_mab1_bwd recomputes them from the
        // points only for up to three columns); the same stores as the hidden layer's below
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
          lane_ref<u32x4>(qps, oQ, (32 * u + 16 * nb) * ROWB) = to_chunk(pack4(acc[0][nb]), pack4(acc[1][nb]));
      }
    } else {
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        acc[0][nb] = bqv[0];
        acc[1][nb] = bqv[1];
      }
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          const bf16x8 bx = *reinterpret_cast<const bf16x8*>(sY + (n0 + 16 * nb) * ROWB + oB[s]);
          acc[0][nb] = mfma32(wa[s][0], bx, acc[0][nb]);
          acc[1][nb] = mfma32(wa[s][1], bx, acc[1][nb]);
        }
      // saved for the backward: straight from the accumulators, as the 16-byte chunk chunk_of(g) of the
      // head's 64 bytes of a row (to_chunk)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
        lane_ref<u32x4>(qps, oQ, (32 * u + 16 * nb) * ROWB) = to_chunk(pack4(acc[0][nb]), pack4(acc[1][nb]));
    }
    // attention over the 16 inducing keys, all inside the wave
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const bf16x8 qb = pack8(acc[0][nb], acc[1][nb]);
      const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
      f32x4 s0 = mfma32(kpa, qb, z4);            // [key 4 g + e][point r]
      float mx = max_nn(max_nn(s0[0], s0[1]), max_nn(s0[2], s0[3]));
      mx = wave16_max(mx);
      float sum = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s0[e] = __builtin_amdgcn_exp2f((s0[e] - mx) * scale_log2e);
        sum += s0[e];
      }
      sum = wave16_sum(sum);
      const float inv = __builtin_amdgcn_rcpf(sum);
#pragma unroll
      for (int e = 0; e < 4; ++e) s0[e] *= inv;
      const bf16x4 pb = pack4(s0);               // B operand [k = key 4 g + e][point r]
      acc[0][nb] = mfma16(vta[0], pb, acc[0][nb]);
      acc[1][nb] = mfma16(vta[1], pb, acc[1][nb]);
    }
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int t = 0; t < 2; ++t)
        *reinterpret_cast<bf16x4*>(sO + (n0 + 16 * nb) * ROWB + oD[t]) = pack4(acc[t][nb]);
  }
  // fc_o's weight slice replaces fc_q's (K-permuted image: the O tiles come back from sO in
  // accumulator order); requested before the barrier
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int t = 0; t < 2; ++t)
      wa[s][t] = lane_ref<bf16x8>(L.WoP + 32 * j * D, 256u * r + 16u * g, 2 * (16 * t * D + 32 * s));
  f32x4 bov[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float4 o4 = lane_ref<float4>(L.bo1 + 32 * j, 16u * g, 64 * t);
    bov[t] = f32x4{o4.x, o4.y, o4.z, o4.w};
  }
  uint8_t* const msk = reinterpret_cast<uint8_t*>(L.mask) + (c.row0 + c.qn0) * 16 + j;
  int oP[KS][2];
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) oP[s][hh] = y_off(r, 4 * s + 2 * hh + (g >> 1)) + 8 * (g & 1);
  STAMP(stamp0);
  lds_barrier();                        // O rows complete; every head has read the unit's input rows
  STAMP(stamp0 + 1);
#pragma unroll
  for (int u = 0; u < UPQ; ++u) {     // (a compile-time bound: both units of a wave in ONE basic block, so
                                      //  that hipcc interleaves their dependent MFMA -> softmax -> MFMA chains)
    const int n0 = c.qn0 + 32 * u;
    f32x4 acc[2][2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      acc[0][nb] = bov[0];
      acc[1][nb] = bov[1];
    }
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const char* rowp = sO + (n0 + 16 * nb) * ROWB;
        const bf16x4 lo = *reinterpret_cast<const bf16x4*>(rowp + oP[s][0]);
        const bf16x4 hi = *reinterpret_cast<const bf16x4*>(rowp + oP[s][1]);
        bf16x8 ob;
#pragma unroll
        for (int e = 0; e < 4; ++e) { ob[e] = lo[e]; ob[4 + e] = hi[e]; }
        acc[0][nb] = mfma32(wa[s][0], ob, acc[0][nb]);
        acc[1][nb] = mfma32(wa[s][1], ob, acc[1][nb]);
      }
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      // Y = O + relu(Z) = max(O + Z, O); byte j of the lane's mask word: bit 4 t + e <-> Z > 0
      uint32_t bits = 0u;
      f32x4 y[2];
#pragma unroll
      for (int t = 1; t >= 0; --t) {
        const bf16x4 o4 = *reinterpret_cast<const bf16x4*>(sO + (n0 + 16 * nb) * ROWB + oD[t]);   // the residual
#pragma unroll
        for (int e = 3; e >= 0; --e) {
          const float zz = acc[t][nb][e], of = (float)o4[e];
          bits = push_gt0(bits, zz);
          y[t][e] = max_nn(of + zz, of);
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
        *reinterpret_cast<bf16x4*>(sY + (n0 + 16 * nb) * ROWB + oD[t]) = pack4(y[t]);
      // byte j of word `lane` of the block's 64 mask words (mab1_mask_index<128>: 64 words per 16-row block,
      // block after block from word 4 row0 on).  (Whole words through an LDS image behind the barrier below
      // were no faster: DESIGN.md 4.4.1.)
      lane_ref<uint8_t>(msk, 4u * c.lane, (32 * u + 16 * nb) * 16) = (uint8_t)bits;
    }
  }
  STAMP(stamp0 + 2);
  lds_barrier();                        // Y rows complete (and every head has read the O rows)
  STAMP(stamp0 + 3);
  // saved O and the block's output: coalesced 16-byte pieces of full rows (no output when nothing
  // after this launch reads it).  Chunk p = tid + 1024 k is the 16 bytes ch = tid & 15 of row (tid >> 4) + 64 k:
  // 16 tid + 16384 k bytes from the workgroup's first row, in LDS y_off of k = 0 plus 16384 k.
  // The branch below opens a basic block: the lane offset is formed again INSIDE it (relane), since hipcc
  // matches `scalar base + 32-bit offset` only where it sees the 32-bit value in the block of the access.
  {
    const int t = c.tid;
    const uint32_t oT = 16u * t;
    const int oL = y_off(t >> 4, t & 15);
    __bf16* const os = L.OS + c.row0 * D;
#pragma unroll
    for (int k = 0; k < 2 * UPQ; ++k)                 // NH * 16 = 2048 UPQ chunks
      lane_ref<uint4>(os, oT, 16384 * k) = *reinterpret_cast<const uint4*>(sO + oL + 16384 * k);
  }
  if (L.Y != nullptr) {
    const int t = relane(c.tid);
    const uint32_t oT = 16u * t;
    const int oL = y_off(t >> 4, t & 15);
    __bf16* const ys = L.Y + c.row0 * D;
#pragma unroll
    for (int k = 0; k < 2 * UPQ; ++k)
      lane_ref<uint4>(ys, oT, 16384 * k) = *reinterpret_cast<const uint4*>(sY + oL + 16384 * k);
  }
  STAMP(stamp0 + 4);
}

// ---------------------------------------------------------------------------------------------
// The per-set stages between the PMA's attention forward and its attention backward (k_pma_head1,
// pma_head.hip, on 1024 threads): PMA epilogue O = Qp + T_h Wv_h^T + bv, P = O + relu(O Wo^T + bo)
// (modules.py:29-31), classifier + mean cross-entropy forward and backward (Code/models.py:40,
// Code/settransformer.py:104), and the adjoint of the epilogue: dZ, dO = dP + dZ Wo, dT_h = dO_h Wv_h,
// Delta = rowdot(dT, T).  Products over the INPUT index take 8 (16) adjacent lanes per output and a
// shuffle reduction; products over the OUTPUT index take thread = (column, eighth of the rows), coalesced
// weight rows, and an LDS reduction.  sPm: this workgroup's PMA partial, theirs: the partner's (sc1).
// The two partials are merged in the order of the halves, so that both workgroups of a pair compute
// bit-identical results when both run these stages (pma_bwd); wr: this one writes the global outputs.
// bw != nullptr: the operands of the tail's attention backward also go to LDS (PmaBwdLds).
// ---------------------------------------------------------------------------------------------
// LDS of the PMA attention backward in the tail (in sO, dead by then): G and dT as [16][256 B] images
// (y_off rows; rows >= 4 zero), their transposes [128][4] bf16, LSE / Delta, the P^T and dS^T tiles of the
// 32-point tiles ([32 points][16 rows] bf16 each), the dG partials of the summation chains
struct PmaBwdLds {
  static constexpr int G = 0, DT = 4096, GT = 8192, DTT = 9216, LD = 10240, PT = 12288, DS = 20480,
                       RED = 32768;
};

// The weights and biases of the first three stages: requested by head_prefetch() in front of hand-off 3's
// flag wait (behind the publishing waves' drain_vm() and its barrier, so no publish waits for them) and in
// flight while the partner's flag is polled.  The partner's partial is read behind the flag, and so is the
// set's label row: soft_row() selects between two loaded values, which is a wait where it stands - in front of
// the poll it would put a round trip of its own there.  (qp, bv: added where they are used, for the same reason.)
struct HeadPre {
  float4 wv4[4], wo4[4], wc4[2];
  float qp, bv, bo_f, bc3;
};

__device__ __forceinline__ void head_prefetch(const PmaHeadArgs& a, const Ctx& c, HeadPre& P) {
  const int tid = c.tid, C = a.C;
  const int fA = tid >> 3;                          // mapping A of head_stages
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    P.wv4[u] = lane_ref<float4>(a.Wv, 64u * tid, 16 * u);      // (fA D + 16 pA = 16 tid floats)
    P.wo4[u] = lane_ref<float4>(a.Wo, 64u * tid, 16 * u);
  }
  const int c3 = tid >> 4, p3 = tid & 15;
#pragma unroll
  for (int u = 0; u < 2; ++u)
    P.wc4[u] = lane_ref<float4>(a.Wc, 512u * (c3 < C ? c3 : 0) + 32u * p3, 16 * u);
  P.qp = lane_ref<float>(a.Qp, 4u * fA);
  P.bv = lane_ref<float>(a.bv, 4u * fA);
  P.bo_f = lane_ref<float>(a.bo, 4u * fA);
  P.bc3 = lane_ref<float>(a.bc, 4u * (c3 < C ? c3 : 0));
}

template <bool LEN>
__device__ __forceinline__ void head_stages(const PmaHeadArgs& a, const Ctx& c, const HeadPre& P,
                                            const float* sPm, const float* theirs, float* sh, bool wr,
                                            char* bw) {
  constexpr int DH = 32, R = 4;
  float* sT = sh;                 // [4][128] merged, normalised T
  float* sOv = sT + 512;          // O, P, Z, dP, dZ, dO: [128] each
  float* sP = sOv + 128;
  float* sZ = sP + 128;
  float* sdP = sZ + 128;
  float* sdZ = sdP + 128;
  float* sdO = sdZ + 128;
  float* sL = sdO + 128;          // logits / dlogits [64]
  float* part = sL + 64;          // [8][128] partial sums of the output-index products
  float* sDl = part + 1024;       // [4][2]
  float* red = sDl + 8;           // m, sum, (argmax), sum of the logits
  int* ramax = reinterpret_cast<int*>(red + 2);
  float* sLSE = red + 4;          // [4]
  const int tid = c.tid, b = c.b, C = a.C, B = a.B;
  const int fA = tid >> 3, pA = tid & 7;            // mapping A: 8 adjacent lanes per output f
  const int fB = tid & 127, pB = tid >> 7;          // mapping B: column f, eighth pB of the rows

  // the partner's partial; everything else the first three stages read from memory is on its way (HeadPre)
  float pth = 0.f;
  if (tid < 520)
    pth = __hip_atomic_load((__attribute__((address_space(1))) const float*)lane_ptr(theirs, 4u * tid),
                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const float4 (&wv4)[4] = P.wv4, (&wo4)[4] = P.wo4, (&wc4)[2] = P.wc4;
  const int c3 = tid >> 4, p3 = tid & 15;
  const float qb = P.qp + P.bv, bo_f = P.bo_f, bc3 = P.bc3;
  const SoftRow y = soft_row(a.soft, a.labels, b);
  if (wr && a.zero_ptr != nullptr)
    for (int i = b * NT + tid; i < a.zero_n; i += B * NT) a.zero_ptr[i] = 0.f;

  // ---- merge the two halves' partials (ordered by half) ----
  float* sEx = part;                                  // the partner's 520 values
  if (tid < 520) sEx[tid] = pth;
  lds_barrier();
  if (tid < 512) {
    const float* P0 = c.half ? sEx : sPm;
    const float* P1 = c.half ? sPm : sEx;
    const int rr = tid >> 7;
    const float m0 = P0[512 + rr], m1 = P1[512 + rr];
    const float M = fmaxf(m0, m1);
    const float f0 = fac<LEN>(m0, M), f1 = fac<LEN>(m1, M);     // (half 1 of a short set: the empty partial)
    const float Lt = f0 * P0[516 + rr] + f1 * P1[516 + rr];
    const float v = (f0 * P0[tid] + f1 * P1[tid]) / Lt;
    sT[tid] = v;
    if (wr) lane_ref<float>(a.T + (int64_t)b * R * D, 4u * tid) = v;
    if ((tid & 127) == 0) {
      const float lse = M + log2f(Lt);
      if (wr) lane_ref<float>(a.LSE + (int64_t)b * R, 4u * rr) = lse;
      sLSE[rr] = lse;
    }
  }
  lds_barrier();
  auto dot16 = [&](const float4 (&w)[4], const float* v) {
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float4 x = *reinterpret_cast<const float4*>(v + 4 * u);
      acc += w[u].x * x.x + w[u].y * x.y + w[u].z * x.z + w[u].w * x.w;
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    return acc;
  };
  // O = Qp + T_h Wv_h^T + bv
  {
    const float o1 = qb + dot16(wv4, sT + (fA / DH) * D + 16 * pA);
    if (pA == 0) sOv[fA] = o1;
  }
  lds_barrier();
  // Z = O Wo^T + bo ; P = O + relu(Z)
  {
    const float z1 = bo_f + dot16(wo4, sOv + 16 * pA);
    if (pA == 0) {
      const float o1 = sOv[fA], hv = o1 + fmaxf(z1, 0.f);
      const int64_t o = (int64_t)b * D;
      if (wr) {
        lane_ref<float>(a.H + o, 4u * fA) = hv;
        lane_ref<float>(a.Osave + o, 4u * fA) = o1;
        lane_ref<float>(a.Zsave + o, 4u * fA) = z1;
      }
      sP[fA] = hv;
      sZ[fA] = z1;
    }
  }
  lds_barrier();
  // the weights of the adjoint stages, requested under the classifier
  float wcB[8], woB[16];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int cc = pB + 8 * u;
    wcB[u] = lane_ref<float>(a.Wc, 512u * (cc < C ? cc : 0) + 4u * fB);
  }
#pragma unroll
  for (int u = 0; u < 16; ++u) woB[u] = lane_ref<float>(a.Wo, 512u * pB + 4u * fB, 4096 * u);
  // logits
  {
    float acc = 0.f;
    const float* x = sP + 8 * p3;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const float4 x4 = *reinterpret_cast<const float4*>(x + 4 * u);
      acc += wc4[u].x * x4.x + wc4[u].y * x4.y + wc4[u].z * x4.z + wc4[u].w * x4.w;
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    acc += __shfl_xor(acc, 8, 64);
    if (c3 < C && p3 == 0) {
      acc += bc3;
      sL[c3] = acc;
      if (wr) lane_ref<float>(a.logits + (int64_t)b * C, 4u * c3) = acc;
    }
  }
  lds_barrier();
  if (tid < 64) {
    float m = -INFINITY;
    int am = 0x7fffffff;
    for (int j = tid; j < C; j += 64)
      if (sL[j] > m) { m = sL[j]; am = j; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(m, o, 64);
      const int oa = __shfl_xor(am, o, 64);
      if (om > m || (om == m && oa < am)) { m = om; am = oa; }
    }
    float sm = 0.f;
    for (int j = tid; j < C; j += 64) sm += expf(sL[j] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o, 64);
    float sx = 0.f;
    if (y.eps > 0.f) {           // (uniform) sum of the logits, for the smoothing term (C <= 64)
      sx = tid < C ? sL[tid] : 0.f;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sx += __shfl_xor(sx, o, 64);
    }
    if (tid == 0) { red[0] = m; red[1] = sm; red[3] = sx; *ramax = am; }
  }
  lds_barrier();
  {
    const float m = red[0], sm = red[1];
    const float gs = a.grad_scale / (float)B;
    float g = 0.f;
    if (tid < C) g = (expf(sL[tid] - m) / sm - soft_target(y, tid, C)) * gs;
    if (wr && tid == 0) {
      a.lossv[b] = m + logf(sm) - soft_picked(y, sL[y.y1], sL[y.y2], red[3], C);
      a.corrv[b] = *ramax == (int)soft_dominant(y) ? 1.f : 0.f;
    }
    lds_barrier();
    if (tid < C) {
      sL[tid] = g;
      if (wr) lane_ref<float>(a.dlogits + (int64_t)b * C, 4u * tid) = g;
    }
    lds_barrier();
  }
  // dP = dlogits Wc
  {
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int cc = pB + 8 * u;
      if (cc < C) acc = fmaf(sL[cc], wcB[u], acc);
    }
    part[pB * D + fB] = acc;
  }
  lds_barrier();
  if (tid < D) {
    float dp = 0.f;
#pragma unroll
    for (int p = 0; p < 8; ++p) dp += part[p * D + tid];
    if (wr) lane_ref<float>(a.dP + (int64_t)b * D, 4u * tid) = dp;
    sdP[tid] = dp;
    const float v = sZ[tid] > 0.f ? dp : 0.f;          // dZ = dP . [Z > 0]
    sdZ[tid] = v;
    if (wr) lane_ref<float>(a.dZ + (int64_t)b * D, 4u * tid) = v;
  }
  lds_barrier();
  // dO = dP + dZ Wo
  float wvB[16];
  {
    const int j = (tid >> 7) & 3, hlf = tid >> 9;      // stage after this one: (column, head, half of the head)
#pragma unroll
    for (int u = 0; u < 16; ++u) wvB[u] = lane_ref<float>(a.Wv, 512u * (j * DH + 16 * hlf) + 4u * fB, 512 * u);
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < 16; ++u) acc = fmaf(sdZ[pB + 8 * u], woB[u], acc);
    part[pB * D + fB] = acc;
  }
  lds_barrier();
  if (tid < D) {
    float v = sdP[tid];
#pragma unroll
    for (int p = 0; p < 8; ++p) v += part[p * D + tid];
    sdO[tid] = v;
    if (wr) lane_ref<float>(a.dO + (int64_t)b * D, 4u * tid) = v;
  }
  lds_barrier();
  // dT_h = dO_h Wv_h ; Delta = rowdot(dT, T) ; the images k_mab0_bwd reads (bw: the tail's, in LDS)
  {
    const int j = (tid >> 7) & 3, hlf = tid >> 9;
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < 16; ++u) acc = fmaf(sdO[j * DH + 16 * hlf + u], wvB[u], acc);
    part[(hlf * 4 + j) * D + fB] = acc;
  }
  lds_barrier();
  if (tid < 512) {
    const int j = tid >> 7, f = tid & 127;
    const float acc = part[j * D + f] + part[(4 + j) * D + f];
    const float tv = sT[j * D + f];
    if (wr) lane_ref<float>(a.Th + (int64_t)b * D, 512u * j * B + 4u * f) = tv;
    if (bw != nullptr) {
      const __bf16 v = (__bf16)acc;
      *reinterpret_cast<__bf16*>(bw + PmaBwdLds::DT + y_off(j, f >> 3) + 2 * (f & 7)) = v;
      *reinterpret_cast<__bf16*>(bw + PmaBwdLds::DTT + 8 * f + 2 * j) = v;
    } else {
      a.dTb[((int64_t)b * a.Rp + j) * D + f] = (__bf16)acc;
      int pos = 0;
#pragma unroll
      for (int p = 0; p < 32; ++p)
        if (perm32(p) == j) pos = p;
      a.dTt[((int64_t)b * D + f) * a.Rp + pos] = (__bf16)acc;
    }
    float dl = acc * tv;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dl += __shfl_xor(dl, o, 64);
    if ((tid & 63) == 0) sDl[2 * j + ((tid >> 6) & 1)] = dl;
  }
  lds_barrier();
  if (bw != nullptr) {                // LSE, Delta of the four score rows; the images are the tail's
    if (tid < R) {
      float* ld = reinterpret_cast<float*>(bw + PmaBwdLds::LD);
      ld[tid] = sLSE[tid];
      ld[4 + tid] = sDl[2 * tid] + sDl[2 * tid + 1];
    }
    return;
  }
  for (int r = tid; r < a.Rp; r += NT) {
    a.Delta[(int64_t)b * a.Rp + r] = r < R ? sDl[2 * r] + sDl[2 * r + 1] : 0.f;
    a.LSEp[(int64_t)b * a.Rp + r] = r < R ? sLSE[r] : 1.0e30f;
  }
  for (int o = tid; o < (a.Rp - R) * D; o += NT) {          // padding rows / columns of the images
    const int r = R + o / D, cc = o % D;
    a.dTb[((int64_t)b * a.Rp + r) * D + cc] = (__bf16)0.f;
    const int rb32 = r & ~31, ro = r & 31;
    int pos = 0;
#pragma unroll
    for (int p = 0; p < 32; ++p)
      if (perm32(p) == ro) pos = p;
    a.dTt[((int64_t)b * D + cc) * a.Rp + rb32 + pos] = (__bf16)0.f;
  }
}

// ---------------------------------------------------------------------------------------------
// The PMA's attention backward (k_mab0_bwd<32, true>, mab0_bwd_bf16.hip) over the workgroup's resident
// rows of Y2, after the head stages have left dT, LSE and Delta of the set's 4 score rows in LDS (bw).
// It computes what k_mab0_bwd computed, bit for bit: the same MFMAs on the same operands (4 real score
// rows padded to 32, the K-permuted dT^T / G'^T operands, 32-point tiles), and dG summed in the same
// order - k_mab0_bwd's workgroup (b, split sp) covered the points [sp per, (sp + 1) per), its wave w the
// tiles w, w + 4 .. of them, one accumulator chain per wave, the four waves' chains then added in wave
// order into the slab b S + sp; a half of the set is S / 2 whole splits.
//   1  wave u < NH / 32, tile u: S^T = G' Y^T, dA^T = dT Y^T -> P^T, dS^T = ln2 P^T (dA^T - Delta): bf16
//      tiles in LDS ([point][row] image, the one k_mab0_bwd's tr_frag read)
//   2  wave 4 s + w < 2 S: chain (split s, wave w): dG += dS Y over its tiles (A: dS tile, B: Y, both
//      through the transposing read) -> LDS
//   3  wave u: dY^T = dT^T P^T + G'^T dS^T over the tile's own rows of sY -> full 256-byte rows of dY2;
//      waves 8 .. 15: the chains' sums into the slabs
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bf16x8 tr_frag_img(const char* img, int rowb, int t, int lane, bool compact) {
  // B / A operand [k = point (tr_frag's k order) of the 32-row image][col = element 16 t + (lane & 15)]:
  // rows of 256 B in y_off order, or (compact) of 32 B: the [point][16 rows] P^T / dS^T tiles
  const int g = lane >> 4, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
  const int a0 = compact ? 32 * (4 * g + q) + 8 * p : y_off(4 * g + q, 2 * t + (p >> 1)) + 8 * (p & 1);
  const int a1 = compact ? 32 * (16 + 4 * g + q) + 8 * p : y_off(16 + 4 * g + q, 2 * t + (p >> 1)) + 8 * (p & 1);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + rowb + a0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + rowb + a1));
  const bf16x4 l4 = __builtin_bit_cast(bf16x4, lo), h4 = __builtin_bit_cast(bf16x4, hi);
  bf16x8 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) { r[e] = l4[e]; r[4 + e] = h4[e]; }
  return r;
}

// LEN: a point at or beyond `len` (an index within the set) has P = 0 exactly, as in k_mab0_bwd with lengths: its
// dS is 0, its dY2 row is written as exact zeros, and the dG slab of a split without a valid point is exact
// zeros (0 times the finite rows of sY).  Every stage still runs over all the rows.
template <bool LEN>
__device__ __forceinline__ void pma_bwd_tail(const __bf16* Gpma, __bf16* dY2, float* slabs, int S,
                                             const Ctx& c, char* sY, char* bw, int len) {
  constexpr float LN2 = 0.6931471805599453f;
  const int tid = c.tid, lane = c.lane, r = c.r, g = c.g;
  const int ntile = c.NH >> 5, sph = S >> 1, tps = ntile / sph;      // tiles, splits of this half, tiles per split
  // G' image (rows 4 .. 15 of Gpma are zero), its transpose, the zero rows of the dT image
  if (tid < 256) {
    const int row = tid >> 4, ch = tid & 15;
    const bf16x8 v = lane_ref<bf16x8>(Gpma, 16u * tid);          // (row D + 8 ch = 8 tid elements)
    *reinterpret_cast<bf16x8*>(bw + PmaBwdLds::G + y_off(row, ch)) = v;
    if (row < 4) {
#pragma unroll
      for (int k = 0; k < 8; ++k) *reinterpret_cast<__bf16*>(bw + PmaBwdLds::GT + 8 * (8 * ch + k) + 2 * row) = v[k];
    }
  } else if (tid < 256 + 192) {
    const int row = 4 + ((tid - 256) >> 4), ch = tid & 15;
    *reinterpret_cast<uint4*>(bw + PmaBwdLds::DT + y_off(row, ch)) = uint4{0u, 0u, 0u, 0u};
  }
  lds_barrier();
  const bf16x4 z4 = {(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
  // ---- 1: P^T and dS^T of tile u (rows 4 g + e; only g = 0 are real: LSEp = +1e30 made the rest 0)
  if (c.wave < ntile) {
    const char* img = sY + 32 * c.wave * ROWB;
    const float* ld = reinterpret_cast<const float*>(bw + PmaBwdLds::LD);
    const float4 l4 = *reinterpret_cast<const float4*>(ld), d4 = *reinterpret_cast<const float4*>(ld + 4);
    const float lse[4] = {l4.x, l4.y, l4.z, l4.w}, del[4] = {d4.x, d4.y, d4.z, d4.w};
    char* tPT = bw + PmaBwdLds::PT + c.wave * 1024;
    char* tDS = bw + PmaBwdLds::DS + c.wave * 1024;
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
      f32x4 sv = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 xr = *reinterpret_cast<const bf16x8*>(img + y_off(16 * pb + r, 4 * ks + g));
        sv = mfma32(*reinterpret_cast<const bf16x8*>(bw + PmaBwdLds::G + y_off(r, 4 * ks + g)), xr, sv);
        da = mfma32(*reinterpret_cast<const bf16x8*>(bw + PmaBwdLds::DT + y_off(r, 4 * ks + g)), xr, da);
      }
      f32x4 pt, dst;
      const bool key = !LEN || c.half * c.NH + 32 * c.wave + 16 * pb + r < len;     // column r = the point
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = g == 0 && key ? exp2f(sv[e] - lse[e]) : 0.f;
        pt[e] = p;
        dst[e] = g == 0 ? LN2 * p * (da[e] - del[e]) : 0.f;     // (+0, as the padded rows were)
      }
      *reinterpret_cast<bf16x4*>(tPT + 32 * (16 * pb + r) + 8 * g) = pack4(pt);
      *reinterpret_cast<bf16x4*>(tDS + 32 * (16 * pb + r) + 8 * g) = pack4(dst);
    }
  }
  lds_barrier();
  // ---- 2: the dG chains (rows 16 .. 31 of k_mab0_bwd's dG are identically zero and not kept)
  float* red = reinterpret_cast<float*>(bw + PmaBwdLds::RED);
  if (c.wave < 4 * sph) {
    const int sp = c.wave >> 2, w = c.wave & 3;
    f32x4 dG[8];
#pragma unroll
    for (int ft = 0; ft < 8; ++ft) dG[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int u = sp * tps + w; u < (sp + 1) * tps; u += 4) {
      bf16x8 xtr[8];
#pragma unroll
      for (int ft = 0; ft < 8; ++ft) xtr[ft] = tr_frag_img(sY, 32 * u * ROWB, ft, lane, false);
      const bf16x8 da = tr_frag_img(bw + PmaBwdLds::DS, u * 1024, 0, lane, true);
#pragma unroll
      for (int ft = 0; ft < 8; ++ft) dG[ft] = mfma32(da, xtr[ft], dG[ft]);
    }
    if (g == 0) {
#pragma unroll
      for (int ft = 0; ft < 8; ++ft)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[c.wave * 512 + e * D + 16 * ft + r] = dG[ft][e];
    }
  }
  lds_barrier();
  // ---- 3: dY of tile u; the slabs
  if (c.wave < ntile) {
    char* img = sY + 32 * c.wave * ROWB;
    const char* tPT = bw + PmaBwdLds::PT + c.wave * 1024;
    const char* tDS = bw + PmaBwdLds::DS + c.wave * 1024;
    bf16x8 pf[2], df[2];
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
      const bf16x4 p4 = *reinterpret_cast<const bf16x4*>(tPT + 32 * (16 * pb + r) + 8 * g);
      const bf16x4 d4 = *reinterpret_cast<const bf16x4*>(tDS + 32 * (16 * pb + r) + 8 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pf[pb][e] = p4[e]; pf[pb][4 + e] = z4[e];
        df[pb][e] = d4[e]; df[pb][4 + e] = z4[e];
      }
    }
#pragma unroll
    for (int ft = 0; ft < 8; ++ft) {
      // A operands [feature 16 ft + i][k-slot 8 g + j = score row perm32(8 g + j)]: rows 0 .. 3 sit in
      // the slots j < 4 of g = 0, every other slot is padding
      bf16x4 t4 = *reinterpret_cast<const bf16x4*>(bw + PmaBwdLds::DTT + 8 * (16 * ft + r));
      bf16x4 g4 = *reinterpret_cast<const bf16x4*>(bw + PmaBwdLds::GT + 8 * (16 * ft + r));
      bf16x8 ta, ga;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ta[e] = g == 0 ? t4[e] : z4[e]; ta[4 + e] = z4[e];
        ga[e] = g == 0 ? g4[e] : z4[e]; ga[4 + e] = z4[e];
      }
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) {
        f32x4 dx = {0.f, 0.f, 0.f, 0.f};
        dx = mfma32(ta, pf[pb], dx);
        dx = mfma32(ga, df[pb], dx);
        *reinterpret_cast<bf16x4*>(img + y_off(16 * pb + r, 2 * ft + (g >> 1)) + 8 * (g & 1)) = pack4(dx);
      }
    }
    // (the tile's rows were last read in stage 2, before the barrier)
    __bf16* const dy = dY2 + (c.row0 + 32 * c.wave) * D;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int cidx = lane + 64 * k, row = cidx >> 4, ch = cidx & 15;
      lane_ref<uint4>(dy, 16u * lane, 1024 * k) = *reinterpret_cast<const uint4*>(img + y_off(row, ch));
    }
  } else if (tid >= 512) {
    const int i = tid - 512;
    for (int sp = 0; sp < sph; ++sp) {
      const float* rs = red + sp * 4 * 512;
      lane_ref<float>(slabs + ((int64_t)c.b * S + c.half * sph + sp) * 512, 4u * i) =
          rs[i] + rs[512 + i] + rs[1024 + i] + rs[1536 + i];
    }
  }
}

__device__ __forceinline__ void mab1_load_wq(const Set128Layer& L, const Ctx& c, bf16x8 (&wa)[4][2]) {
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int t = 0; t < 2; ++t)
      wa[s][t] = lane_ref<bf16x8>(L.WqB + 32 * c.j * D, 256u * c.r + 16u * c.g, 2 * (16 * t * D + 32 * s));
}

typedef __attribute__((address_space(4))) const Set128FwdArgs karg_t;
// The kernel's arguments are ~75 pointers: left to itself hipcc loads them all at entry and then spills
// SGPRs to VGPR lanes (930 v_readlane in the first version).  Reading them through a pointer the
// optimiser cannot see through keeps every s_load at its phase.
__device__ __forceinline__ karg_t* launder(karg_t* p) {
  asm volatile("" : "+s"(p));
  return p;
}
// The same for the thread index at a phase boundary: everything derived from it (lane, r, g, the swizzled
// LDS offsets ...) is recomputed in the next phase - a handful of VALU instructions - instead of being kept
// alive across phases by common-subexpression elimination, which cost ~20 spilled registers whose scratch
// reloads (vmcnt!) then sat next to the prefetches
__device__ __forceinline__ void rederive(Ctx& c) {
  int t = c.tid;
  asm volatile("" : "+v"(t));
  c.tid = t; c.lane = t & 63; c.r = t & 15; c.g = (t >> 4) & 3;
}

// (explicit address-space cast: the host pass of hipcc rejects the implicit one; the optimiser infers the
//  constant address space back, the loads stay scalar)
#define LAYER(i) (*(const Set128Layer*)(&ap->L[i]))

// the set's number of valid points: min(lengths[b], N) - a scalar load at the phase that asks, like every
// other argument - or N itself in the dense kernel
template <bool LEN>
__device__ __forceinline__ int set_len(karg_t* ap, int b, int N) {
  if constexpr (LEN) {
    const int l = ap->lengths[b];
    return l < N ? l : N;
  } else {
    return N;
  }
}

template <int DIN, int UPQ, bool LEN>
__global__ __launch_bounds__(NT) void k_set128_fwd(const Set128FwdArgs a_by_value) {
  (void)a_by_value;
  karg_t* ap = launder((karg_t*)__builtin_amdgcn_kernarg_segment_ptr());
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sY = smem;                               // [256][256 B]
  char* sO = smem + 256 * ROWB;                  // [256][256 B]; between blocks: merge buffers
  char* sS = smem + 512 * ROWB;                  // 32 KiB of images
  float* sX = reinterpret_cast<float*>(sS);      // [N][4] the set's points (layer 1)           0 ..  8 K
  char* sA = sS + 8192;                          // O image of the mid stage                    8 .. 12 K
  char* sH = sS + 12288;                         // H image                                    12 .. 16 K
  char* sKp = sS + 16384;                        // K image of the many-queries block          16 .. 20 K
  char* sVt = sS + 20480;                        // V^T image                                  20 .. 24 K
  float* sTf = reinterpret_cast<float*>(sS + 24576);   // layer 1: merged T fp32 [64][4]       24 .. 25 K
  float* sAl = reinterpret_cast<float*>(sS + 25600);   // 32 floats per wave                   25 .. 27 K
  float* sML = reinterpret_cast<float*>(sS + 27648);   // [16 waves][16 columns] float2        27 .. 29 K
  char* sT = sO;                                 // bf16 image of the merged T (layer 2)

  Ctx c;
  c.tid = threadIdx.x; c.lane = c.tid & 63;
  c.wave = __builtin_amdgcn_readfirstlane(c.tid >> 6);
  c.q = c.wave >> 2; c.j = c.wave & 3; c.r = c.lane & 15; c.g = c.lane >> 4;
  {
    // pair = workgroups w and w + 8: the same XCD when ids are dealt round-robin over the 8 XCDs (a
    // placement bonus - same L2 - never a correctness condition)
    const int w = blockIdx.x, xcd = w & 7, k = w >> 3;
    c.half = k & 1;
    c.b = (k >> 1) * 8 + xcd;
  }
  if (c.b >= ap->B) return;
  c.N = ap->N; c.NH = c.N >> 1;
  c.UPQ = c.N >> 8; c.qn0 = c.q * (c.NH >> 2);
  c.row0 = (int64_t)c.b * c.N + c.half * c.NH;
  constexpr int dk = DIN;
  const int b = c.b, NH = c.NH;
  uint32_t* const flags = ap->flags;
  STAMP(0);

  // ================= layer 1, few-queries block: scores G x, softmax over the points, T = A x ====
  // (k_mab0_attn_small's arithmetic: exact fp32 on the vector ALU.)  Its cost is 2 din + 6 operations
  // per (score row, point): BOTH workgroups of the pair run it over the WHOLE set instead of handing
  // partials to each other.  lane = score row (head * 16 + query), wave w walks the points
  // [w N/16, (w+1) N/16) - their coordinates are wave-uniform LDS broadcasts; wave 0 merges.
  MidPre pre;
  {
    const Set128Layer& L = LAYER(0);
    const int N = c.N, tid = c.tid, lane = c.lane;
    float xs[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {                 // N * 4 <= 2048 staged words
      const int i = tid + NT * it;
      const int pt = i >> 2, cc = i & 3;
      const int ptc = pt < N ? pt : N - 1, ccc = cc < dk ? cc : 0;      // unconditional, clamped
      const float v = lane_ref<float>(ap->X + (int64_t)b * N * dk, 4u * (ptc * dk + ccc));
      xs[it] = cc < dk ? v : 0.f;
    }
    float gk[DIN];
#pragma unroll
    for (int cc = 0; cc < DIN; ++cc) gk[cc] = lane_ref<float>(L.Gf, 4u * dk * lane, 4 * cc);
    // two images of the points: [point][4] for the layer-1 projection of the many-queries block, and
    // [pair of points][component][2] - the operand pairs of the packed-fp32 loop below (v_pk_fma_f32 /
    // v_pk_mul_f32 work on two points per issue slot, as in k_mab0_attn_small)
    float* sXp = reinterpret_cast<float*>(sO) + 8192;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = tid + NT * it;
      if (i < N * 4) {
        const int pt = i >> 2, cc = i & 3;
        sX[i] = xs[it];
        sXp[(pt >> 1) * 8 + cc * 2 + (pt & 1)] = xs[it];
      }
    }
    lds_barrier();
    const int npw = N >> 5, q0 = c.wave * npw;       // 8 or 16 pairs of points per wave
    // LEN: the wave walks the pairs that hold a valid point (none: both loops are empty and the wave keeps
    // (m, l, t) = (-inf, 0, 0) without an exp2 of -inf - -inf); the second point of the set's last pair is
    // masked when len is odd - the pair's first point is valid, so m is finite and its p is exp2(-inf) = 0
    const int len = set_len<LEN>(ap, b, N);
    int np = npw;
    if (LEN) {
      const int left = len - 2 * q0;                 // valid points from the wave's first one on
      np = left <= 0 ? 0 : (left + 1) >> 1 < npw ? (left + 1) >> 1 : npw;
    }
    float m = -INFINITY;
#pragma unroll 8
    for (int i = 0; i < np; ++i) {
      const float* px = sXp + (q0 + i) * 8;
      f32x2 sv = gk[0] * *reinterpret_cast<const f32x2*>(px);
#pragma unroll
      for (int cc = 1; cc < DIN; ++cc) sv += gk[cc] * *reinterpret_cast<const f32x2*>(px + 2 * cc);
      if (LEN && 2 * (q0 + i) + 1 >= len) sv[1] = -INFINITY;
      m = max_nn(m, max_nn(sv[0], sv[1]));
    }
    f32x2 l2 = {0.f, 0.f}, t2[DIN];
#pragma unroll
    for (int cc = 0; cc < DIN; ++cc) t2[cc] = f32x2{0.f, 0.f};
#pragma unroll 8
    for (int i = 0; i < np; ++i) {
      const float* px = sXp + (q0 + i) * 8;
      f32x2 xv[DIN];
#pragma unroll
      for (int cc = 0; cc < DIN; ++cc) xv[cc] = *reinterpret_cast<const f32x2*>(px + 2 * cc);
      f32x2 sv = gk[0] * xv[0];
#pragma unroll
      for (int cc = 1; cc < DIN; ++cc) sv += gk[cc] * xv[cc];
      if (LEN && 2 * (q0 + i) + 1 >= len) sv[1] = -INFINITY;
      const f32x2 p = {__builtin_amdgcn_exp2f(sv[0] - m), __builtin_amdgcn_exp2f(sv[1] - m)};
      l2 += p;
#pragma unroll
      for (int cc = 0; cc < DIN; ++cc) t2[cc] += p * xv[cc];
    }
    const float l = l2[0] + l2[1];
    float t4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cc = 0; cc < DIN; ++cc) t4[cc] = t2[cc][0] + t2[cc][1];
    float* sM = reinterpret_cast<float*>(sO);              // [16][64]
    float* sL = sM + 16 * 64;                              // [16][64]
    float* sTp = sL + 16 * 64;                             // [16][64][4]
    sM[c.wave * 64 + lane] = m;
    sL[c.wave * 64 + lane] = l;
    *reinterpret_cast<float4*>(sTp + (c.wave * 64 + lane) * 4) = float4{t4[0], t4[1], t4[2], t4[3]};
    // the mid stage's weight fragments, one barrier ahead.  (Requested at kernel entry they were live
    // across the whole attention loop and hipcc spilled every one of them right behind its load: seven
    // serialised round trips at the start of the kernel.)
    mid_prefetch<true>(L, c, dk, pre);
    STAMP(1);
    lds_barrier();
    if (c.wave == 0) {
      // the sixteen m are read once and kept, and the partials are requested eight at a time (unrolled whole, the
      // loop spills beside the mid stage's fragments in flight); p = 0 .. 15 and the expressions as they were,
      // the fused multiply-adds that hipcc made of them written out
      float mv[16];
#pragma unroll
      for (int p = 0; p < 16; ++p) mv[p] = sM[p * 64 + lane];
      float M = -INFINITY;
#pragma unroll
      for (int p = 0; p < 16; ++p) M = max_nn(M, mv[p]);
      float Ls = 0.f, tt[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
      for (int p = 0; p < 16; ++p) {
        const float f = __builtin_amdgcn_exp2f(mv[p] - M);
        const float4 tp = *reinterpret_cast<const float4*>(sTp + (p * 64 + lane) * 4);
        Ls = __builtin_fmaf(sL[p * 64 + lane], f, Ls);
        tt[0] = __builtin_fmaf(tp.x, f, tt[0]); tt[1] = __builtin_fmaf(tp.y, f, tt[1]);
        tt[2] = __builtin_fmaf(tp.z, f, tt[2]); tt[3] = __builtin_fmaf(tp.w, f, tt[3]);
      }
      const float inv = 1.f / Ls;
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) tt[cc] *= inv;
      *reinterpret_cast<float4*>(sTf + lane * 4) = float4{tt[0], tt[1], tt[2], tt[3]};
      if (c.half == 0) {
        for (int cc = 0; cc < dk; ++cc) lane_ref<float>(L.T + (int64_t)b * 64 * dk, 4u * dk * lane, 4 * cc) = tt[cc];
        lane_ref<float>(L.LSE + (int64_t)b * 64, 4u * lane) = M + log2f(Ls);
      }
    }
    lds_barrier();
  }
  STAMP(2);
  ap = launder(ap);
  rederive(c);
  mid_stage<true>(LAYER(0), c, pre, sT, sTf, sA, sH, sKp, sVt, [] {});
  STAMP(3);

  // ================= layer 1, many-queries block ================================================
  ap = launder(ap);
  rederive(c);
  bf16x8 wa[4][2];
  mab1_phase<true, DIN, UPQ>(LAYER(0), c, sY, sO, sX + c.half * NH * 4, sKp, sVt, ap->scale_log2e, 4, wa);

  // ================= layer 2, few-queries block over the rows in sY (k_mab0_attn_h4) ==============
  ap = launder(ap);
  rederive(c);
  {
    const Set128Layer& L = LAYER(1);
    const int tid = c.tid, lane = c.lane, r = c.r, g = c.g;
    bf16x8 gf[4];                     // this head's G rows: B operand of the score MFMAs
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) gf[ks] = lane_ref<bf16x8>(L.Gb + 16 * c.j * D, 256u * r + 16u * g, 64 * ks);
    float* myAl = sAl + c.wave * 32;
    float mrow = -INFINITY, lrow = 0.f;
    f32x4 T[8];
#pragma unroll
    for (int ft = 0; ft < 8; ++ft) T[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int len = set_len<LEN>(ap, b, c.N);
#pragma unroll
    for (int u = 0; u < UPQ; ++u) {
      const char* img = sY + (c.qn0 + 32 * u) * ROWB;
      // LEN: the unit's first point within the set; a unit wholly beyond len adds nothing to (m, l, T)
      // (wave-uniform: c.qn0 comes from the wave's index).  A unit that runs holds a valid point, so its
      // running max is finite
      const int p0 = c.half * NH + c.qn0 + 32 * u;
      if (LEN && p0 >= len) continue;
      f32x4 s[2];
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) {
        s[pb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          s[pb] = mfma32(*reinterpret_cast<const bf16x8*>(img + y_off(16 * pb + r, 4 * ks + g)), gf[ks],
                         s[pb]);
      }
      // rows of s = points 16 pb + 4 g + e ; column = query row r of this head
      if (LEN) {
        const int left = len - p0 - 4 * g;
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (16 * pb + e >= left) s[pb][e] = -INFINITY;
      }
      float mt = -INFINITY;
#pragma unroll
      for (int pb = 0; pb < 2; ++pb)
#pragma unroll
        for (int e = 0; e < 4; ++e) mt = max_nn(mt, s[pb][e]);
      mt = wave16_max(mt);
      const float mnew = max_nn(mrow, mt);
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
      if (g == 0) myAl[r] = alpha;                    // T rows are query rows 4g+e
      const float4 a4 = *reinterpret_cast<const float4*>(&myAl[4 * g]);
      const bf16x8 pa = pack8(s[0], s[1]);
#pragma unroll
      for (int ft = 0; ft < 8; ++ft) {
        T[ft][0] *= a4.x; T[ft][1] *= a4.y; T[ft][2] *= a4.z; T[ft][3] *= a4.w;
        T[ft] = mfma32(pa, y_tr_frag(img, ft, lane), T[ft]);
      }
    }
    STAMP(9);
    // ---- the four quads' partials of a head -> quad 0, in two rounds through sO (8 KiB per wave) ----
    // (m, l) of query row r live in every lane of column r; the T accumulators hold query rows
    // 4 g + e: their factors come back from LDS as a float4
    auto put_partial = [&](int slot) {
      float4* dst = reinterpret_cast<float4*>(sO) + slot * 512;
#pragma unroll
      for (int ft = 0; ft < 8; ++ft) dst[ft * 64 + lane] = float4{T[ft][0], T[ft][1], T[ft][2], T[ft][3]};
      if (g == 0) *reinterpret_cast<float2*>(sML + (c.wave * 16 + r) * 2) = float2{mrow, lrow};
    };
    auto take_partial = [&](int slot, int from_wave) {
      const float2 ml = *reinterpret_cast<const float2*>(sML + (from_wave * 16 + r) * 2);
      const float mn = max_nn(mrow, ml.x);
      const float f1 = fac<LEN>(mrow, mn), f2 = fac<LEN>(ml.x, mn);
      lrow = lrow * f1 + ml.y * f2;
      mrow = mn;
      if (g == 0) {
        myAl[r] = f1;
        myAl[16 + r] = f2;
      }
      const float4 a1 = *reinterpret_cast<const float4*>(&myAl[4 * g]);
      const float4 a2 = *reinterpret_cast<const float4*>(&myAl[16 + 4 * g]);
      const float4* src = reinterpret_cast<const float4*>(sO) + slot * 512;
#pragma unroll
      for (int ft = 0; ft < 8; ++ft) {
        const float4 o = src[ft * 64 + lane];
        T[ft][0] = T[ft][0] * a1.x + o.x * a2.x;
        T[ft][1] = T[ft][1] * a1.y + o.y * a2.y;
        T[ft][2] = T[ft][2] * a1.z + o.z * a2.z;
        T[ft][3] = T[ft][3] * a1.w + o.w * a2.w;
      }
    };
    lds_barrier();                       // all score reads of sY done; sO (saved O rows) is stored
    STAMP(20);
    if (c.q & 1) put_partial((c.q >> 1) * 4 + c.j);
    lds_barrier();
    if (!(c.q & 1)) take_partial((c.q >> 1) * 4 + c.j, c.wave + 4);
    lds_barrier();
    STAMP(21);
    // ---- round B, the publish, the fetch and the cross-half merge on ALL sixteen waves: quads 0 and 2 both put
    // their round-A result into LDS (quad 0 into the slots 4 - 7 that round A has emptied), then wave (q, j)
    // owns the feature tiles 2 q and 2 q + 1 of head j - two float4 per lane of the lane-linear image instead
    // of the eight (plus the partner's eight) that a quad-0 lane carried while twelve waves waited
    if (c.q == 2) put_partial(c.j);
    if (c.q == 0) put_partial(4 + c.j);
    lds_barrier();
    STAMP(22);
    float* mine = ap->ex2 + (int64_t)(b * 2 + c.half) * 9216;
    float* theirs = ap->ex2 + (int64_t)(b * 2 + (c.half ^ 1)) * 9216;
    const int ft0 = 2 * c.q;
    f32x4 Tm[2];
    {
      // take_partial's expressions on quad 0's (m, l, T) (slot 4 + j) and quad 2's (slot j): every wave of head
      // j forms the same (m, l) and the same factors from the same two sML entries
      const float2 mlA = *reinterpret_cast<const float2*>(sML + (c.j * 16 + r) * 2);
      const float2 mlB = *reinterpret_cast<const float2*>(sML + ((8 + c.j) * 16 + r) * 2);
      const float mn = max_nn(mlA.x, mlB.x);
      const float f1 = fac<LEN>(mlA.x, mn), f2 = fac<LEN>(mlB.x, mn);
      lrow = mlA.y * f1 + mlB.y * f2;
      mrow = mn;
      if (g == 0) {
        myAl[r] = f1;
        myAl[16 + r] = f2;
      }
      const float4 a1 = *reinterpret_cast<const float4*>(&myAl[4 * g]);
      const float4 a2 = *reinterpret_cast<const float4*>(&myAl[16 + 4 * g]);
      const float4* srcA = reinterpret_cast<const float4*>(sO) + (4 + c.j) * 512;
      const float4* srcB = reinterpret_cast<const float4*>(sO) + c.j * 512;
#pragma unroll
      for (int k = 0; k < 2; ++k)
        Tm[k] = round_b_tile(srcA[(ft0 + k) * 64 + lane], a1, srcB[(ft0 + k) * 64 + lane], a2);
    }
    // hand-off 2: the workgroup's partial (unnormalised T, m, l) at the addresses it always had; (m, l) of head
    // j once, by quad 0's wave.  Every wave stores, every wave drains, the barrier, one lane signals
#pragma unroll
    for (int k = 0; k < 2; ++k)
      st16_sc1(mine + (((ft0 + k) * 4 + c.j) * 64 + lane) * 4, float4{Tm[k][0], Tm[k][1], Tm[k][2], Tm[k][3]});
    if (c.q == 0) st16_sc1(mine + 8192 + (c.j * 64 + lane) * 4, float4{mrow, lrow, 0.f, 0.f});
    drain_vm();
    STAMP(23);
    lds_barrier();                       // every storing wave has drained
    if (tid == 0) flag_store(flags + 4 + (b * 2 + 1) * 2 + c.half, 2u);
    if (c.wave == 0) flag_wait(flags + 4 + (b * 2 + 1) * 2 + (c.half ^ 1), 2u, flags);   // nothing in front of the poll
    lds_barrier();
    STAMP(24);
    float* sTs = reinterpret_cast<float*>(sO) + 8192;       // staging [64][128] fp32 (the slots 4 - 7 are dead)
    {
      // the partner's two tiles and its (m, l) of the lane's row: the oldest requests of every wave, as sc1 BUFFER
      // loads - instructions that hipcc counts, so that it places the wait for them itself, in front of the first
      // use and behind the mid stage's fragments requested below, which stay in flight
      const __amdgpu_buffer_rsrc_t rs = payload_rsrc(theirs, 9216 * 4);
      f32x4 pt[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) pt[k] = ld16_buf_sc1(rs, 16u * lane, (((ft0 + k) * 4 + c.j) * 64) * 16);
      const f32x4 pml = ld16_buf_sc1(rs, 16u * lane, (8192 + c.j * 64 * 4) * 4);
      // the mid stage's fragments, all three stages': in flight from here on, through the merge and the image
      // block (two tiles per lane in the merge leave the registers for stage C's too)
      mid_prefetch<false, 3>(L, c, D, pre);
#ifdef PCA_SET_STAMPS
      asm volatile("" ::"v"(pt[0]), "v"(pt[1]), "v"(pml) : "memory");
#endif
      STAMP(26);
      // the SAME expression in both halves - f_1 x_1 + (f_0 x_0), the half-0 product rounded first, whoever
      // "own" is - so that the two workgroups of a set merge to bit-identical T (hipcc contracts
      // __fadd_rn(__fmul_rn(..), __fmul_rn(..)) into v_fmac: "own product first" differed between them)
      const bool h0 = c.half == 0;
      auto comb = [&](float fo_, float xo_, float fp_, float xp_) {
        return h0 ? __builtin_fmaf(fp_, xp_, fo_ * xo_) : __builtin_fmaf(fo_, xo_, fp_ * xp_);
      };
      const float Mx = fmaxf(mrow, pml.x);
      // (LEN: half 1 of a set with len <= N / 2 published the empty partial; half 0 holds point 0: Mx is finite)
      const float fo = fac<LEN>(mrow, Mx), fp = fac<LEN>(pml.x, Mx);
      const float Lt = comb(fo, lrow, fp, pml.y);
      const float inv = 1.f / Lt;
      if (g == 0) {
        myAl[r] = fo;
        myAl[16 + r] = fp;
      }
      // (inv, lse) of head j's rows where the image block reads them: once, by quad 0's wave
      if (c.q == 0 && g == 0) *reinterpret_cast<float2*>(sML + (c.wave * 16 + r) * 2) = float2{inv, Mx + log2f(Lt)};
      const float4 a1 = *reinterpret_cast<const float4*>(&myAl[4 * g]);
      const float4 a2 = *reinterpret_cast<const float4*>(&myAl[16 + 4 * g]);
      const float a1v[4] = {a1.x, a1.y, a1.z, a1.w}, a2v[4] = {a2.x, a2.y, a2.z, a2.w};
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const float pv[4] = {pt[k].x, pt[k].y, pt[k].z, pt[k].w};
#pragma unroll
        for (int e = 0; e < 4; ++e)       // unnormalised; row 16 j + 4 g + e, feature 16 ft + r
          sTs[(16 * c.j + 4 * g + e) * D + 16 * (ft0 + k) + r] = comb(a1v[e], Tm[k][e], a2v[e], pv[e]);
      }
    }
    STAMP(25);
    lds_barrier();
    {                                  // T (global fp32, saved) and its bf16 image; (inv, lse) of row: lane `row & 15` of wave j
      const int row = tid >> 4, ch = tid & 15;
      const float2 il = *reinterpret_cast<const float2*>(sML + ((row >> 4) * 16 + (row & 15)) * 2);
      const float4 lo = *reinterpret_cast<const float4*>(sTs + row * D + ch * 8);
      const float4 hi = *reinterpret_cast<const float4*>(sTs + row * D + ch * 8 + 4);
      float t[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      bf16x8 v;
#pragma unroll
      for (int k = 0; k < 8; ++k) { t[k] *= il.x; v[k] = (__bf16)t[k]; }
      if (c.half == 0) {
        float* const tg = L.T + (int64_t)b * 64 * D;             // (row D + 8 ch = 8 tid floats)
        lane_ref<float4>(tg, 32u * tid) = float4{t[0], t[1], t[2], t[3]};
        lane_ref<float4>(tg, 32u * tid, 16) = float4{t[4], t[5], t[6], t[7]};
        if (ch == 0) lane_ref<float>(L.LSE + (int64_t)b * 64, 4u * row) = il.y;
      }
      *reinterpret_cast<bf16x8*>(sT + swz(row, ch, ROWB)) = v;
    }
    lds_barrier();
    STAMP(10);
    // fc_q's slice of the many-queries block: two stages ahead, behind stage A
    mid_stage<false>(L, c, pre, sT, sTf, sA, sH, sKp, sVt, [&] { mab1_load_wq(L, c, wa); });
    STAMP(11);
  }

  // ================= layer 2, many-queries block ================================================
  ap = launder(ap);
  rederive(c);
  mab1_phase<false, D, UPQ>(LAYER(1), c, sY, sO, sX, sKp, sVt, ap->scale_log2e, 12, wa);

  // ================= PMA attention partials over Y2 (k_mab0_attn<1>): wave w < NH / 32 = unit w ====
  ap = launder(ap);
  rederive(c);
  {
    const int tid = c.tid, lane = c.lane, r = c.r, g = c.g;
    float mrow = -INFINITY, lrow = 0.f;
    f32x4 T[8];
#pragma unroll
    for (int ft = 0; ft < 8; ++ft) T[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nun = NH >> 5;                    // 4 or 8 units
    // LEN: a unit wholly beyond len keeps the empty partial (-inf, 0, 0) - its slab is written all the same -
    // and the merges below pass over it (fac)
    const int len = set_len<LEN>(ap, b, c.N);
    const int p0 = c.half * NH + 32 * c.wave;   // the unit's first point within the set
    if (c.wave < nun && (!LEN || p0 < len)) {
      const char* img = sY + (32 * c.wave) * ROWB;
      f32x4 s[2];
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) {
        s[pb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          s[pb] = mfma32(*reinterpret_cast<const bf16x8*>(img + y_off(16 * pb + r, 4 * ks + g)),
                         lane_ref<bf16x8>(ap->Gpma, 256u * r + 16u * g, 64 * ks), s[pb]);
      }
      if (LEN) {
        const int left = len - p0 - 4 * g;      // rows of s = points 16 pb + 4 g + e
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (16 * pb + e >= left) s[pb][e] = -INFINITY;
      }
      float mt = -INFINITY;
#pragma unroll
      for (int pb = 0; pb < 2; ++pb)
#pragma unroll
        for (int e = 0; e < 4; ++e) mt = max_nn(mt, s[pb][e]);
      mrow = wave16_max(mt);
      float ls = 0.f;
#pragma unroll
      for (int pb = 0; pb < 2; ++pb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s[pb][e] = __builtin_amdgcn_exp2f(s[pb][e] - mrow);
          ls += s[pb][e];
        }
      lrow = wave16_sum(ls);
      const bf16x8 pa = pack8(s[0], s[1]);
#pragma unroll
      for (int ft = 0; ft < 8; ++ft) T[ft] = mfma32(pa, y_tr_frag(img, ft, lane), T[ft]);
    }
    STAMP(17);
    lds_barrier();                     // sO is dead (its rows are on their way to memory): the slabs alias it
    STAMP(18);
    float* slab = reinterpret_cast<float*>(sO) + c.wave * 520;     // [4 rows][128] + m[4] + l[4]
    if (g == 0 && c.wave < nun) {
#pragma unroll
      for (int ft = 0; ft < 8; ++ft)
#pragma unroll
        for (int e = 0; e < 4; ++e) slab[e * D + 16 * ft + r] = T[ft][e];
      if (r < 4) {
        slab[512 + r] = mrow;
        slab[516 + r] = lrow;
      }
    }
    lds_barrier();
    if (!ap->fuse_head) {
      const int Spw = ap->Sp >> 1, upp = nun / Spw;         // partials of this workgroup, units per partial
      if (tid < Spw * 512) {
        const int p = tid >> 9, rr = (tid >> 7) & 3, f = tid & 127;
        const float* s0 = reinterpret_cast<const float*>(sO);
        float M = -INFINITY;
        for (int w = p * upp; w < (p + 1) * upp; ++w) M = fmaxf(M, s0[w * 520 + 512 + rr]);
        float Ls = 0.f, t = 0.f;
        for (int w = p * upp; w < (p + 1) * upp; ++w) {
          const float fs = fac<LEN>(s0[w * 520 + 512 + rr], M);
          Ls += fs * s0[w * 520 + 516 + rr];
          t += fs * s0[w * 520 + rr * D + f];
        }
        const int64_t o = ((int64_t)b * ap->Sp + c.half * Spw + p) * 4 + rr;
        ap->TpP[o * D + f] = t;
        if (f == 0) {
          ap->MpP[o] = M;
          ap->LpP[o] = Ls;
        }
      }
      STAMP(19);
      return;
    }
    // ---- the workgroup's ONE partial over all its units: (t [4][128], m [4], l [4]) -> sPm --------
    float* sPm = reinterpret_cast<float*>(sS);              // 528 floats (the images in sS are dead)
    if (tid < 512) {
      const int rr = tid >> 7, f = tid & 127;
      const float* s0 = reinterpret_cast<const float*>(sO);
      float M = -INFINITY;
      for (int w = 0; w < nun; ++w) M = fmaxf(M, s0[w * 520 + 512 + rr]);
      float Ls = 0.f, t = 0.f;
      for (int w = 0; w < nun; ++w) {
        const float fs = fac<LEN>(s0[w * 520 + 512 + rr], M);
        Ls += fs * s0[w * 520 + 516 + rr];
        t += fs * s0[w * 520 + rr * D + f];
      }
      sPm[tid] = t;
      if (f == 0) {
        sPm[512 + rr] = M;
        sPm[516 + rr] = Ls;
      }
    }
    lds_barrier();
    float* exMine = ap->exP + (int64_t)(b * 2 + c.half) * 528;
    float* exTheirs = ap->exP + (int64_t)(b * 2 + (c.half ^ 1)) * 528;
    const bool pbwd = ap->pma_bwd != 0;
    if (c.half == 1 || pbwd) {
      // hand-off 3 (R1 again: 4-byte write-through stores, drained, barrier, one flag): half 1 is done,
      // or (pma_bwd) both halves publish and both go on
      if (tid < 520)
        __hip_atomic_store((__attribute__((address_space(1))) float*)lane_ptr(exMine, 4u * tid), sPm[tid],
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      drain_vm();
      lds_barrier();
      if (tid == 0) flag_store(flags + 4 + (b * 2 + 0) * 2 + c.half, 3u);
      if (!pbwd) return;
    }
    HeadPre hp;
    head_prefetch(*(const PmaHeadArgs*)(&ap->head), c, hp);      // in flight under the flag wait
    if (c.wave == 0) flag_wait(flags + 4 + (b * 2 + 0) * 2 + (c.half ^ 1), 3u, flags);
    lds_barrier();
    head_stages<LEN>(*(const PmaHeadArgs*)(&ap->head), c, hp, sPm, exTheirs,
                     reinterpret_cast<float*>(sS) + 1024, c.half == 0, pbwd ? sO : nullptr);
    STAMP(19);
    if (pbwd) {
      ap = launder(ap);
      rederive(c);
      pma_bwd_tail<LEN>(ap->Gpma, ap->dY2, ap->pma_slabs, ap->pma_S, c, sY, sO, set_len<LEN>(ap, c.b, c.N));
      STAMP(27);
    }
  }
}

}  // namespace

#ifdef PCA_SET_STAMPS
extern "C" int pca_debug_set_stamps(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_set_stamps), sizeof(g_set_stamps));
}
#endif

// softmax_merge.hpp on the host, for the tests: the factor of a partial with max m against the merged max M as
// the kernel's merges form it (guarded != 0), or the bare 2^(m - M) they formed before sets had lengths
extern "C" float pca_debug_merge_factor(float m, float M, int guarded) {
  return guarded ? merge_factor(m, M) : merge_exp2(m - M);
}

size_t set128_flag_bytes(int B) { return align256((size_t)(4 + B * 4) * sizeof(uint32_t)); }

size_t set128_fwd_ws_bytes(int B) {
  return set128_flag_bytes(B) + align256((size_t)B * 2 * 9216 * sizeof(float)) +
         align256((size_t)B * 2 * 528 * sizeof(float));
}

// the shape rule on `cus` compute units (pca_debug_set128_shape_ok: the host tests)
static bool shape_ok_on(int B, int N, int din, int d, int h, int m, int k, int cus) {
  if (!(d == 128 && h == 4 && m == 16 && k == 1 && din >= 1 && din <= 4 && (N == 256 || N == 512)))
    return false;
  // the kernel addresses every tensor as a scalar base plus an UNSIGNED 32-bit byte offset of the lane
  // (lane_ptr): the largest tensor of a launch, a [B N, 128] bf16 activation, stays below 2^31 bytes
  if ((int64_t)B * N * 128 * 2 >= (int64_t)1 << 31) return false;
  // the two workgroups of a set wait for each other: every pair must be resident at once - one
  // workgroup per CU (160 KiB of LDS), workgroup ids dealt in order
  return 16 * cdiv((int64_t)B, 8) <= cus;
}

extern "C" int pca_debug_set128_shape_ok(int B, int N, int din, int d, int h, int m, int k, int cus) {
  return shape_ok_on(B, N, din, d, h, m, k, cus) ? 1 : 0;
}

bool set128_shape_ok(int B, int N, int din, int d, int h, int m, int k) {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return n;
  }();
  return shape_ok_on(B, N, din, d, h, m, k, cus);
}

// the eight (din, N / 256) instantiations of one LEN: 160 KiB of LDS allowed once, the one of `key` launched
template <bool LEN>
static void launch_instance(int key, dim3 grid, size_t lds, hipStream_t st, const Set128FwdArgs& a) {
  allow_lds160<k_set128_fwd<1, 1, LEN>, k_set128_fwd<2, 1, LEN>, k_set128_fwd<3, 1, LEN>, k_set128_fwd<4, 1, LEN>,
               k_set128_fwd<1, 2, LEN>, k_set128_fwd<2, 2, LEN>, k_set128_fwd<3, 2, LEN>, k_set128_fwd<4, 2, LEN>>();
  switch (key) {
    case 2: hipLaunchKernelGGL((k_set128_fwd<1, 1, LEN>), grid, dim3(NT), lds, st, a); break;
    case 3: hipLaunchKernelGGL((k_set128_fwd<1, 2, LEN>), grid, dim3(NT), lds, st, a); break;
    case 4: hipLaunchKernelGGL((k_set128_fwd<2, 1, LEN>), grid, dim3(NT), lds, st, a); break;
    case 5: hipLaunchKernelGGL((k_set128_fwd<2, 2, LEN>), grid, dim3(NT), lds, st, a); break;
    case 6: hipLaunchKernelGGL((k_set128_fwd<3, 1, LEN>), grid, dim3(NT), lds, st, a); break;
    case 7: hipLaunchKernelGGL((k_set128_fwd<3, 2, LEN>), grid, dim3(NT), lds, st, a); break;
    case 8: hipLaunchKernelGGL((k_set128_fwd<4, 1, LEN>), grid, dim3(NT), lds, st, a); break;
    default: hipLaunchKernelGGL((k_set128_fwd<4, 2, LEN>), grid, dim3(NT), lds, st, a); break;
  }
}

int set128_fwd_launch(const Set128FwdArgs& a, hipStream_t st) {
  PCA_REQUIRE(set128_shape_ok(a.B, a.N, a.din, 128, 4, 16, 1), "set128_fwd: B=%d N=%d din=%d not built",
              a.B, a.N, a.din);
  PCA_REQUIRE(a.Sp == 2 || a.Sp == 4, "set128_fwd: %d PMA partials", a.Sp);
  PCA_REQUIRE(a.Sp <= a.N / 128, "set128_fwd: %d PMA partials of %d points", a.Sp, a.N);
  const size_t lds = (size_t)512 * ROWB + 32768;
  // reference-formulation FLOPs of the three blocks this launch covers (the PMA's
  // epilogue and the classifier run in k_pma_head1), algorithmic bytes: X in, two [N, d] bf16 tensors
  // written and read once each
  // pma_bwd: plus the PMA attention backward in k_mab0_bwd's units (2 N (2 d^2 + 2 k d) MACs per set), and
  // the bytes move - dY2 is written instead of Y2
  PCA_REQUIRE(!a.pma_bwd || (a.fuse_head && a.dY2 != nullptr && a.pma_slabs != nullptr),
              "set128_fwd: the PMA backward needs the fused head and its outputs");
  PCA_REQUIRE(!a.pma_bwd || a.pma_S == 2 || (a.pma_S == 4 && a.N == 512),
              "set128_fwd: PMA backward in %d splits of %d points", a.pma_S, a.N);
  const double Nn = a.N, dd = 128, mm = 16;
  double macs = Nn * (3.0 * a.din * dd + 7.0 * dd * dd + 8.0 * mm * dd + 2.0 * dd) + 6.0 * mm * dd * dd;
  if (a.pma_bwd) macs += 2.0 * Nn * (2.0 * dd * dd + 2.0 * dd);
  // [N, d] bf16 tensors written here and read once later: Y1, Y2 (unless not stored), dY2
  const double nout = (a.L[1].Y != nullptr ? 2.0 : 1.0) + (a.pma_bwd ? 1.0 : 0.0);
  ProfScope ps(PCA_K_SET_FWD, st, 2.0 * macs * a.B, (double)a.B * (4.0 * Nn * a.din + 4.0 * Nn * dd * nout));
  const dim3 grid(16 * (unsigned)cdiv(a.B, 8));
  const int key = a.din * 2 + (a.N == 512 ? 1 : 0);       // units per quad of waves: N / 256
  if (a.lengths == nullptr) launch_instance<false>(key, grid, lds, st, a);
  else launch_instance<true>(key, grid, lds, st, a);      // variable-length sets: the masking instantiations
  ps.end();
  return check_launch("k_set128_fwd");
}

}  // namespace pca
