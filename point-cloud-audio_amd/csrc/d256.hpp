// Launchers of the d = 256 training kernels; all activations bf16 [rows][256].  The one declaration point of
// attn1_pma256.hip, wgrad256.hip, fq256.hip, small256.hip, d256_stream.hip, d256_fused.hip and mid256.hip
// (the blocks built from them: d256_host.hip, declared in blocks.hpp).
//
// Map of the d = 256 / 8-head / m = 32 Set Transformer's training step (BASELINE configs[3], the
// north-star shape): the pieces of the MAB adjoint (set_transformer-master/
// modules.py:19-33 backwards) that the d = 128 kernels hold in ONE launch do not fit a CU at
// d = 256 (two 128 KiB weight images), so the backward of the many-queries block runs as
//
//   k_attn1_bwd3         dZ = dY.[Z>0] ; dO = dY + dZ Wo (the wave's slice of Wo^T in registers), then
//   (attn1_pma256.hip)   per head: P recomputed, dA, dS, dQp = dO + dS Kp ; dKp, dVp of the set
//                        (WAVE = HEAD: a wave owns the 32 features of one head of its 32-point
//                        tiles), k_sum_parts256 sums the per-range dKp / dVp partials
//   k_rowstream DX1/DX3  dX = dQp Wq (+ dKp Wk + dVp Wv)            (d256_stream.hip)
//   k_wgrad256(_dma)     dW[256 x 256] = G^T A over the B*N rows, deterministic two-stage sum
//   (wgrad256.hip)
//
// and the few-queries block (ISAB mab0 at dk = 256) in the reference's own formulation
// (modules.py:21: the N keys ARE projected) because the four 128 KiB operand images of the
// reassociated backward exceed the register file + LDS of a CU (fq256.hip):
//
//   k_fq_proj_fwd        m = 32: Kp / Vp = X Wk^T + bk (bf16, [B*N, 256]) and the flash attention of
//                        the m shared queries over the set's keys in one pass over X (wave = head,
//                        head dim 32): online softmax, O partials per range, k_fq_merge joins them
//   k_rowstream PROJ2 +  m <= 16: the projection (d256_stream.hip) and the attention as two launches
//   k_fq_attn_fwd<256,1>
//   k_fq_attn_bwd2       dKp, dVp (bf16) and the set's dQp; both score orientations are
//   (m <= 16: _bwd<256,1>) recomputed on the MFMA (one extra 16x16x32 each) instead of transposed
//   k_rowstream DX2/DX3  dX (+)= dKp Wk + dVp Wv                    (d256_stream.hip)
//
// plus the PMA at dk = 256 in the reassociated form (k_pma_*256, attn1_pma256.hip), the small per-set / layer-1
// kernels (small256.hip) and the stand-alone fixed-order slab sum (slab_sum.hip).
//
// All activations cross these kernels in bf16 ([rows][256], row-major); accumulation, softmax
// statistics, biases and residuals are fp32.  Layout conventions: mfma_common.hpp.
#pragma once
#include "pca_common.h"
#include "weight_images.hpp"
#include "bwd_defer.hpp"

namespace pca {

// attention adjoint of the many-queries block (m = 32 keys): dQp, and the set's dKp / dVp (fp32,
// [B][32][256]; the per-range partials are summed into dKp / dVp)
int attn1_bwd256_parts(int B, int N);

// the whole many-queries block in ONE launch (d256_fused.hip): wave = head, both weight slices in
// registers.  WqB / WoB: natural bf16 images (prep mode 0); X bf16 [B*N][256] (or fp32 [B*N][dq],
// dq <= 4, with WqF); QpS / OS / mask nullable (saved for the backward)
int isab1_fwd256_fused(const void* X, int dq, const __bf16* WqB, const float* WqF, const float* bq,
                       const __bf16* KpP, const __bf16* Vt, const __bf16* WoB, const float* bo,
                       __bf16* Y, __bf16* QpS, __bf16* OS, uint32_t* mask, int B, int N,
                       hipStream_t st, const float* inv_o = nullptr);

bool wgrad256_masked_ok(int64_t rows_per_set);
// mid256.hip: the per-set stage between the two blocks of a d = 256 ISAB in one launch
int mid256_fwd(const float* O, const float* Wo, const float* bo, const float* Wk, const float* bk,
               const float* Wv, const float* bv, float* Z, float* H, __bf16* KpP, __bf16* VpP,
               __bf16* Kt, __bf16* Vt, int B, hipStream_t st);
// The query side (Qp, G: parameters only) of several few-queries blocks collected into `out`, for ONE
// launch the caller makes together with its other preparation jobs; the blocks' forward calls then take
// PCA_F_PREP_DONE (training only: the saved blocks must exist)
void mab0_d256_prep_collect(int n, const pca_mab_shape* const* shapes, const float* const* I,
                            const pca_mab_params* params, void* const* saved, Mab0PrepJobs* out);
// image mode (prep_weight) of every weight the d = 256 backward takes - fc_o / fc_q of the many-queries
// block, fc_k / fc_v of the few-queries block: the transposed natural image the register-resident
// kernels (k_attn1_bwd3, k_rowstream) read
constexpr int D256_BWD_WMODE = 3;
size_t wgrad256_ws_bytes(int njobs, int64_t maxM);
int wgrad256_launch(const Wgrad256Jobs& jobs, void* ws, hipStream_t st);
int wgrad256_launch_t(const Wgrad256Jobs& jobs, void* ws, bool f32_operands, hipStream_t st);

int cvt_f32_bf16(const float* s, __bf16* d, int64_t n, hipStream_t st);            // n % 4 == 0
int cvt_bf16_f32(const __bf16* s, float* d, int64_t n, int accumulate, hipStream_t st);

// layer 1 (inputs of dq <= 4 columns)
// d256_stream.hip: streaming row-GEMMs with the weights in registers
int rowstream256_proj2(const __bf16* X, const __bf16* WkB, const __bf16* WvB, const float* bk,
                       const float* bv, __bf16* Kp, __bf16* Vp, int B, int N, hipStream_t st);
int rowstream256_proj2_f8(const __bf16* X, const void* Wk8, const void* Wv8, const float* inv_scale,
                          const float* bk, const float* bv, __bf16* Kp, __bf16* Vp, int B, int N,
                          hipStream_t st);
int rowstream256_dx2(const __bf16* dKp, const __bf16* dVp, const __bf16* WkT, const __bf16* WvT,
                     __bf16* dX, int B, int N, int accumulate, hipStream_t st);
int fq_proj_attn_fwd256(const __bf16* X, const __bf16* WkB, const __bf16* WvB, const float* bk,
                        const float* bv, const float* Qp, int B, int N, int m,
                        const int32_t* lengths, __bf16* Kp, __bf16* Vp, float* Op, float* Mp,
                        float* Lp, float* O, float* LSE, hipStream_t st,
                        const float* inv_scale = nullptr);   // non-null: WkB / WvB are fp8 images
int rowstream256_dx3(const __bf16* dQp, const __bf16* dKp, const __bf16* dVp, const __bf16* WqT,
                     const __bf16* WkT, const __bf16* WvT, __bf16* dX, int B, int N, hipStream_t st);
int rowstream256_dx1(const __bf16* dQp, const __bf16* WqT, __bf16* dX, int B, int N,
                     hipStream_t st);
int attn1_bwd256_fused(const __bf16* dY, const uint32_t* mask, const __bf16* WoT, const __bf16* QpS,
                       const __bf16* KpP, const __bf16* VpP, const __bf16* Kt, __bf16* dZ,
                       __bf16* dQp, float* dKpPart, float* dVpPart, float* dKp, float* dVp, int B,
                       int N, hipStream_t st, const float* Xs = nullptr,
                       const float* WqF = nullptr, const float* bq = nullptr, int dq = 0);
size_t wgrad_small256_ws_bytes(int64_t M);
int wgrad_small256(const __bf16* G, const float* X, int64_t M, int dq, float* dW, float* db,
                   void* ws, hipStream_t st);
int epi_small_fwd256(const float* T, const float* Qp, const float* Wv, const float* bv, int B, int m,
                     int dk, float* O, hipStream_t st);
size_t epi_small_bwd256_ws_bytes(int B, int m);
int epi_small_bwd256(const float* dO, const float* T, const float* Wv, int B, int m, int dk,
                     float* dT, float* Delta, float* dWv, float* dbv, void* ws, hipStream_t st);

// PMA (R = h*m <= 16 score rows) at dk = 256, reassociated: X read once, keys never projected
int pma_splits256(int B, int N);
// Gb [>=16][256] bf16 (sl2e folded, rows >= R zero); Tp [B][S][16][256], Mp / Lp [B][S][16] scratch;
// T [B][R][256] = A X, LSE [B][R] (log2 domain)
int pma_attn_fwd256(const __bf16* X, const __bf16* Gb, int B, int N, int R, const int32_t* lengths,
                    float* Tp, float* Mp, float* Lp, float* T, float* LSE, hipStream_t st);
// per set: dT = dO_h Wv_h and its images (dTb [B][16][256], TG [B][256][32]), Delta, LSEp [B][16];
// dWv += sum over sets of dO^T T
int pma_epi_bwd256(const float* dO, const float* T, const float* LSE, const float* Wv,
                   const float* Gf, int B, int m, int R, __bf16* dTb, __bf16* TG, float* Delta,
                   float* LSEp, float* dWv, hipStream_t st);
// dX (+)= P^T dT + dS^T G' ; DG [16][256] += dS X (ln2 units, as k_mab0_bwd; caller zeroes it)
int pma_attn_bwd256(const __bf16* X, const __bf16* Gb, const __bf16* dTb, const __bf16* TG,
                    const float* LSEp, const float* Delta, int B, int N, int R,
                    const int32_t* lengths, __bf16* dX, int accumulate_dx, float* DG, float* DGslabs,
                    hipStream_t st);
size_t pma_bwd256_slab_bytes(int B);

// few shared queries over projected keys, head dim 32 (fq_attn_fwd256: m <= 16; m = 32 projects the keys in
// the same pass: fq_proj_attn_fwd256)
int fq_splits256(int B, int N);
// Op [B][S][m][256], Mp / Lp [B][S][8][MQ] scratch; O = Qp + A Vp [B][m][256]; LSE [B][8][MQ]
int fq_attn_fwd256(const __bf16* Kp, const __bf16* Vp, const float* Qp, int B, int N, int m,
                   const int32_t* lengths, float* Op, float* Mp, float* Lp, float* O, float* LSE,
                   hipStream_t st);
// dO [B][m][256] = gradient w.r.t. O; writes dKp, dVp (bf16 [B*N][256]) and
// dOt = dO + (attention gradient w.r.t. Qp) per set [B][m][256]
int fq_attn_bwd256(const __bf16* Kp, const __bf16* Vp, const float* Qp, const float* dO,
                   const float* O, const float* LSE, float* Delta, int B, int N, int m,
                   const int32_t* lengths, __bf16* dKp, __bf16* dVp, float* dQpPart, float* dOt,
                   hipStream_t st);

}  // namespace pca
