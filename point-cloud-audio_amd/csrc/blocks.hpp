// Host-side declarations of the attention blocks: every host entry point of the exact, d = 64 and d = 128
// paths, the d = 256 blocks' entries, the per-block dispatch (BlockPath), the saved / workspace layouts and
// the launch records of the per-set mid stages.  What the blocks take from their caller is declared in
// weight_images.hpp, bwd_defer.hpp and step_ctx.hpp.
#pragma once
#include "pca_common.h"
#include "soft_targets.hpp"
#include "weight_images.hpp"

namespace pca {

struct BwdDefer;     // bwd_defer.hpp
struct StepCtx;      // step_ctx.hpp

struct Mab1Saved {
  __bf16 *KpP, *VpP, *Kt, *Vt, *QpS, *OS;
  uint32_t* mask;
};
size_t mab1_carve_saved(const pca_mab_shape& s, Mab1Saved* out, void* base);

// saved-for-backward block of the fused mab0 (few queries, many keys)
struct Mab0Saved {
  float* Qp;      // [m][d]     fc_q(I)
  float* Gf;      // [Rpad][dk] scale*log2e * Qp_h Wk_h   (fp32)
  __bf16* Gb;     // same, bf16 (MFMA operand)
  __bf16* GtP;    // [dk][Rp] K-permuted transpose of G (backward)
  float* T;       // [B][R][dk] A X
  float* LSE;     // [B][R]     log2-domain
  float *O, *Z;   // [B][m][d]
  float *WvT, *WoT;   // transposed fp32 weights ([in][out]) for the per-set epilogue
  float *Tp, *Mp, *Lp;   // per point-range partials of the attention (merged by the epilogue)
};
int mab0_splits(const pca_mab_shape& s);
void mab0_collect_prep(const pca_mab_shape& s, const float* I, const pca_mab_params& p,
                       const Mab0Saved& v, bool training, bool epilogue_images,
                       Mab0PrepJobs* J);
size_t mab0_carve_saved(const pca_mab_shape& s, Mab0Saved* out, void* base);

// dH[q][c] (+)= dKp[q][:] . Wk[:][c] + dVp[q][:] . Wv[:][c]   per set (m = 16 rows, d = 128)
int kv_dh_launch(const float* dKp, const float* dVp, const float* Wk, const float* Wv, float* dH,
                 int B, int m, int d, int accumulate, hipStream_t st);

// scratch layouts of the two backward passes (shared with the ISAB-level orchestration)
struct Mab1BwdWs {
  __bf16 *WoTP, *WqTP, *dZ, *dQp, *dOs, *dS, *P;
  float *dKp, *dVp;            // [B][MI][D]
  float *dKpPart, *dVpPart;    // [B][nparts][MI][D] per-workgroup partials (fused mode)
};
size_t mab1_carve_bwd_ws(const pca_mab_shape& s, Mab1BwdWs* out, void* base);
struct Mab0BwdWs {
  float *dZ, *dO, *Th, *dTf, *Delta, *LSEp, *DG, *dQs, *dQp;
  __bf16 *dTb, *dTt, *GtP;
  float* slabs;           // [workgroups][R][dk] partial dG of k_mab0_bwd
};
int mab0_bwd_splits(const pca_mab_shape& s);
size_t mab0_carve_bwd_ws(const pca_mab_shape& s, Mab0BwdWs* out, void* base);

// flags of the *_ex host entry points used by the fused ISAB path
enum {
  PCA_F_SKIP_EPILOGUE = 1,   // mab0 fwd: stop after the attention partials (mid_fwd follows)
  PCA_F_KV_READY = 2,        // mab1 fwd: Kp/Vp images already written (by mid_fwd / mid256_fwd)
  PCA_F_SKIP_KV_TAIL = 4,    // mab1 bwd: stop after dKp/dVp (mid_bwd + batched wgrad follow)
  PCA_F_SKIP_HEAD = 8,       // mab0 bwd: dT/Delta images, dZ, dO, dQs already produced
  PCA_F_PREP_DONE = 32,      // mab0 fwd: Qp / G images were prepared by the caller
  PCA_F_SKIP_WGRAD = 64,     // mab0 bwd: dWo / dWv reductions are done by the caller; DG is clear
  PCA_F_ATTN_DONE = 128      // mab0 bwd (PMA, d = 128): the caller's launch ran k_mab0_bwd's part and left
                             // dX and its dG slabs [B][S][R][128] in the workspace (set128_fwd.hip)
};

// ---- per-set mid kernels of a fused ISAB (mid_bf16.hip); m = 16, d = 128, h = 4 ----------
struct MidFwdLaunch {
  int B, dk, S;
  const float *Tp, *Mp, *Lp;
  float *T, *LSE;
  const float* Qp;
  const __bf16* Wv0;
  const float* Wv0f;
  const float *bv0, *bo0;
  const __bf16 *Wo0, *Wk1, *Wv1;
  const float *bk1, *bv1;
  float *O, *Z, *H;
  __bf16 *KpP, *VpP, *Kt, *Vt;
};
int mid_fwd_launch(const MidFwdLaunch& L, hipStream_t st);
struct MidBwdLaunch {
  int B, dk;
  const float *dKpPart, *dVpPart;   // [B][nparts][16][128] partials from k_mab1_bwd
  int nparts;
  float *dKp, *dVp;                 // [B][16][128] sums (written; read by the wgrad jobs)
  float* zero_ptr;                  // optional accumulator cleared by this launch (DG)
  int zero_n;
  const float *Z, *T, *LSE;
  const __bf16 *Wk1T, *Wv1T, *Wo0TP, *Wv0TP, *Wv0T;
  const float* Wv0f;
  float *dZ, *dO, *Th, *dQs, *dTf;
  __bf16 *dTb, *dTt;
  float *Delta, *LSEp;
};
int mid_bwd_launch(const MidBwdLaunch& L, hipStream_t st);

bool mab1_saves_qp(const pca_mab_shape& s);
// ---- host entry points of the fused blocks (single source of truth for every TU) --------
// fused attention core of the bf16-operand GEMM chain for head dims <= 16 (attn_core.hip): O = Q_ + A V_
// and its adjoint without the [B h, nq, nk] matrix A (LSE [B][h][nq] is what is saved instead)
bool attn_core_ok(const pca_mab_shape& s);
// self-attention-shaped blocks (SAB) reached through the C ABI only (BlockPath::ExactCore): the same core
// for head dims 8 / 16 at d <= 128, and its head-dim-32 kernels for d <= 256.  Never consulted by the
// ST engine, whose blocks keep attn_core_ok.
bool attn_core_sab_ok(const pca_mab_shape& s);
// floats of the forward's saved statistics area / of the backward's Delta scratch
size_t attn_core_fwd_elems(const pca_mab_shape& s);
size_t attn_core_bwd_elems(const pca_mab_shape& s);
int attn_core_fwd(const pca_mab_shape& s, const float* Qp, const float* Kp, const float* Vp, float* O,
                  float* LSE, hipStream_t st);
int attn_core_bwd(const pca_mab_shape& s, const float* Qp, const float* Kp, const float* Vp,
                  const float* O, const float* LSE, const float* dO, float* dQp, float* dKp, float* dVp,
                  float* Delta, hipStream_t st);
// weight + bias gradient of a 64 -> 64 (or <= 4 -> 64) Linear over a tall activation in one launch
// (wgrad64.hip) that writes per-workgroup slabs into `part` (wgrad64_slab_elems floats: a function of the
// shape alone, 0 for a shape the kernels do not take) and appends the two fixed-order sums that finish
// dW += .. / db += .. to `jobs`: the caller runs them (slab_sum_jobs), several calls' jobs in one launch
struct SlabSumJobs;  // bwd_defer.hpp
size_t wgrad64_slab_elems(int64_t M, int din, int dout);
bool wgrad64_ok(const float* dY, const float* X, const float* dW, const float* db, int64_t M, int din,
                int dout);
int wgrad64(const float* dY, const float* X, float* dW, float* db, int64_t M, int din, float* part,
            SlabSumJobs* jobs, hipStream_t st);
// the 64 -> 64 / <= 4 -> 64 Linear layers over a tall activation with the weights in registers
// (linear64.hip): forward, input gradient, fc_o with the block's epilogue Y = O + relu(Z)
bool lin64_ok(const float* X, const float* Y, int64_t M, int din, int dout);
int lin64_fwd(const float* X, const float* W, const float* b, float* Y, int64_t M, int din,
              hipStream_t st);
int lin64_dx(const float* dY, const float* W, float* dX, int64_t M, int accumulate, hipStream_t st);
int lin64_fc_o(const float* O, const float* W, const float* b, float* Z, float* Y, int64_t M,
               hipStream_t st);
int lin64_fc_o_bwd(const float* dY, const float* Z, const float* W, float* dZ, float* dO, int64_t M,
                   hipStream_t st);
// exact fp32 path (mab_f32.hip)
int validate_shape(const pca_mab_shape* s);
// core / sab = true (BlockPath::ExactCore): the attention runs on the fused core and the
// backward's weight gradients on wgrad_rows; false: the core where attn_core_ok holds, else through the
// materialised A, and linear_dw_db
size_t mab_f32_saved_bytes(const pca_mab_shape& s, bool core = false);
size_t mab_f32_bwd_ws_bytes(const pca_mab_shape& s, bool sab = false);
int mab_f32_fwd(const pca_mab_shape& s, const float* Q, const float* K,
                const pca_mab_params& p, float* Y, void* saved, hipStream_t st, bool core = false);
int mab_f32_bwd(const pca_mab_shape& s, const float* Q, const float* K,
                const pca_mab_params& p, const void* saved, const float* dY, float* dQ,
                float* dK, int dk_accumulate, const pca_mab_grads& g, void* ws,
                hipStream_t st, bool sab = false, StepCtx* ctx = nullptr);
// dW[dout][din] += dY[M][dout]^T X[M][din], db += colsum(dY) with bf16 MFMA operands, bitwise reproducible
// (wgrad_rows.hip); ws: wgrad_rows_ws_elems floats
size_t wgrad_rows_ws_elems(int64_t M, int dout, int din);
int wgrad_rows(const float* dY, const float* X, float* dW, float* db, int64_t M, int din, int dout, float* ws,
               hipStream_t st);
// while alive: linear_fwd_f32 / linear_bwd_f32 / linear_dx_acc_f32 use k_gemm_bf16 instead of the
// exact fp32 GEMM: mode 1 = bf16 MFMA operands, mode 2 = hi + lo bf16 pairs (fp32-level results
// at the same launch cost); fp32 accumulation and I/O
struct Bf16OperandScope {
  int prev;
  explicit Bf16OperandScope(int mode);
  ~Bf16OperandScope();
};
int linear_fwd_f32(const float* X, const float* W, const float* b, float* Y, int64_t M,
                   int din, int dout, hipStream_t st);
int linear_bwd_f32(const float* X, const float* W, const float* dY, float* dX, float* dW,
                   float* db, int64_t M, int din, int dout, hipStream_t st);
int linear_dx_acc_f32(const float* dY, const float* W, float* dX, int64_t M, int din, int dout,
                      int accumulate, hipStream_t st);
// fused mab1 (many queries X, few keys H).  X / Y / dY / dX are fp32 or bf16 per the shape's
// q_dtype / y_dtype; H and dH are fp32
// the shipped d = 64 / 8 heads / <= 64 inducing points shape: fused fp32 forward (sd64_fwd.hip);
// 1 = many queries, 2 = few shared queries, 0 = another shape
int sd64_kind(const pca_mab_shape& s);
size_t sd64_fwd_ws_bytes(const pca_mab_shape& s);
int sd64_fwd(const pca_mab_shape& s, const float* Q, const float* K, const pca_mab_params& p,
             float* Y, void* ws, hipStream_t st);
bool mab1_bf16_supported(const pca_mab_shape& s, bool inference = false);
size_t mab1_bf16_saved_bytes(const pca_mab_shape& s);
size_t mab1_bf16_fwd_ws_bytes(const pca_mab_shape& s);
size_t mab1_bf16_bwd_ws_bytes(const pca_mab_shape& s);
// (ctx: what the engine call this block belongs to hands from stage to stage - StepCtx, step_ctx.hpp;
//  null in a stand-alone call)
int mab1_bf16_fwd_ex(const pca_mab_shape& s, const void* X, const float* H,
                     const pca_mab_params& p, void* Y, void* saved, void* ws, int flags,
                     hipStream_t st, const IsabImg* img = nullptr, const StepCtx* ctx = nullptr);
int mab1_bf16_bwd_ex(const pca_mab_shape& s, const void* X, const float* H,
                     const pca_mab_params& p, const void* saved, const void* dY, void* dX,
                     float* dH, int dk_accumulate, const pca_mab_grads& gr, void* ws, int flags,
                     hipStream_t st, const IsabImg* img = nullptr, float* zero_ptr = nullptr,
                     int zero_n = 0, int* nparts_out = nullptr, StepCtx* ctx = nullptr);
// fused mab0 / PMA (few shared queries I, many keys X).  X / dX fp32 or bf16 per k_dtype
bool mab0_bf16_supported(const pca_mab_shape& s);
size_t mab0_bf16_saved_bytes(const pca_mab_shape& s);
size_t mab0_bf16_fwd_ws_bytes(const pca_mab_shape& s);
size_t mab0_bf16_bwd_ws_bytes(const pca_mab_shape& s);
int mab0_bf16_fwd_ex(const pca_mab_shape& s, const float* I, const void* X,
                     const pca_mab_params& p, float* H, void* saved, void* ws, int flags,
                     hipStream_t st, StepCtx* ctx = nullptr);
// ctx->defer non-null: the post job is appended there instead of being launched
// mid non-null (an ISAB's few-queries block, with PCA_F_SKIP_HEAD): the per-set mid chain of
// mid_bwd_launch runs in the prologue of the attention backward instead of as a launch before it;
// its zero_ptr is ignored (the caller has the accumulator cleared by an earlier launch)
int mab0_bf16_bwd_ex(const pca_mab_shape& s, const float* I, const void* X,
                     const pca_mab_params& p, const void* saved, const float* dH, float* dI,
                     void* dX, int dk_accumulate, const pca_mab_grads& gr, void* ws, int flags,
                     hipStream_t st, StepCtx* ctx = nullptr, const MidBwdLaunch* mid = nullptr);
// d = 256 / 8 heads (d256_host.hip): the many-queries backward and the few-queries block
size_t mab1_d256_bwd_ws_bytes(const pca_mab_shape& s);
int mab1_d256_bwd(const pca_mab_shape& s, const void* X, const float* H, const pca_mab_params& p,
                  const void* saved, const void* dY, void* dX, float* dH, int dk_accumulate,
                  const pca_mab_grads& gr, void* ws, hipStream_t st, StepCtx* ctx);
bool mab0_d256_supported(const pca_mab_shape& s);
size_t mab0_d256_saved_bytes(const pca_mab_shape& s);
size_t mab0_d256_fwd_ws_bytes(const pca_mab_shape& s);
size_t mab0_d256_bwd_ws_bytes(const pca_mab_shape& s);
int mab0_d256_fwd(const pca_mab_shape& s, const float* I, const void* X, const pca_mab_params& p,
                  float* H, void* saved, void* ws, int flags, hipStream_t st, StepCtx* ctx);
int mab0_d256_bwd(const pca_mab_shape& s, const float* I, const void* X, const pca_mab_params& p,
                  const void* saved, const float* dH, float* dI, void* dX, int dk_accumulate,
                  const pca_mab_grads& gr, void* ws, hipStream_t st, StepCtx* ctx);
int small_row_split(int B, int R);
int mab0_attn_small_launch(const float* X, const float* Gf, int B, int N, int R, int dk, float* T,
                           float* LSE, const int32_t* lengths, hipStream_t st);
int mab0_bwd_small_launch(const float* X, const float* Gf, const float* dTf, const float* LSE,
                          const float* Delta, int B, int N, int R, int Rp, int dk, float* DG,
                          const int32_t* lengths, hipStream_t st, float* slabs = nullptr);
// Per-block dispatch (api_mab.hip).  The path of a block is decided once per call, by block_path, and handed
// to the functions below; flags / ctx go to the fused paths' entry points.
//   Exact      fp32 chain of GEMMs (mab_f32.hip), bf16 operands in the fused modes
//   ExactCore  the same chain with a self-attention block's attention on the fused core: pca_mab_* only (abi)
//   Mab1_*     fused many queries / few keys, d = 128 or 256 (one forward; the d = 256 backward in d256_host.hip)
//   Mab0_*     fused few shared queries / many keys, d = 128 (mab0_*.hip) or 256 (d256_host.hip)
//   Sd64       the d = 64 / 8-head fused fp32 forward, inference only (sd64_fwd.hip picks many / few queries
//              from q_shared, which it needs for its argument roles anyway)
enum class BlockPath { Exact, ExactCore, Mab1_128, Mab1_256, Mab0_128, Mab0_256, Sd64 };
BlockPath block_path(const pca_mab_shape& s, bool inference = false, bool abi = false);
inline bool is_mab1(BlockPath p) { return p == BlockPath::Mab1_128 || p == BlockPath::Mab1_256; }
inline bool is_mab0(BlockPath p) { return p == BlockPath::Mab0_128 || p == BlockPath::Mab0_256; }
size_t mab_saved_bytes(BlockPath path, const pca_mab_shape& s);
size_t mab_fwd_ws_bytes(BlockPath inference, BlockPath training, const pca_mab_shape& s);
size_t mab_bwd_ws_bytes(BlockPath path, const pca_mab_shape& s);
int mab_fwd(BlockPath path, const pca_mab_shape& s, const void* Q, const void* K, const pca_mab_params& p,
            void* Y, void* saved, void* ws, hipStream_t st, int flags = 0, StepCtx* ctx = nullptr);
int mab_bwd(BlockPath path, const pca_mab_shape& s, const void* Q, const void* K, const pca_mab_params& p,
            const void* saved, const void* dY, void* dQ, void* dK, int dk_accumulate,
            const pca_mab_grads& g, void* ws, hipStream_t st, StepCtx* ctx = nullptr);
// fused ISAB (isab_bf16.hip)
bool isab_bf16_supported(const pca_mab_shape& s0, const pca_mab_shape& s1);
size_t isab_bf16_fwd_ws_bytes(const pca_mab_shape& s0, const pca_mab_shape& s1);
size_t isab_bf16_bwd_ws_bytes(const pca_mab_shape& s0, const pca_mab_shape& s1);
size_t isab_img_bytes();
void isab_img_carve(void* base, IsabImg* im);
void isab_collect_prep(const pca_mab_shape& s0, const pca_mab_params& p0,
                       const pca_mab_params& p1, const IsabImg& im, bool training,
                       bool need_dx, PrepJobs* J);
int isab_bf16_fwd(const pca_mab_shape& s0, const pca_mab_shape& s1, const float* I,
                  const void* X, const pca_mab_params& p0, const pca_mab_params& p1, float* H,
                  void* Y, void* saved0, void* saved1, void* ws, const IsabImg& im,
                  hipStream_t st);
int isab_bf16_bwd(const pca_mab_shape& s0, const pca_mab_shape& s1, const float* I,
                  const void* X, const float* H, const pca_mab_params& p0,
                  const pca_mab_params& p1, const void* saved0, const void* saved1,
                  const void* dY, float* dI, void* dX, const pca_mab_grads& g0,
                  const pca_mab_grads& g1, void* ws, const IsabImg& im, hipStream_t st,
                  BwdDefer* defer = nullptr);
// classifier head (train_ops.hip); soft: soft_targets.hpp (all null / 0: the hard label)
int soft_targets_from(const PcaSoftTargets* soft, const char* who, SoftTargets* out);
int cls_train_head(const float* P, const float* Wc, const float* bc, const int64_t* labels,
                   const SoftTargets& soft, int B, int d, int C, float grad_scale, float* logits, float* dlogits,
                   float* dP, float* dWc, float* dbc, float* loss_out, float* stats, float* ws,
                   hipStream_t st, BwdDefer* defer = nullptr);
// d128_fused.hip: the same single-launch forward at d = 128 / 4 heads / m = 16
int isab1_fwd128_fused(const void* X, int dq, const __bf16* WqB, const float* WqF, const float* bq,
                       const __bf16* KpP, const __bf16* Vt, const __bf16* WoP, const float* bo,
                       __bf16* Y, __bf16* QpS, __bf16* OS, uint32_t* mask, int B, int N,
                       hipStream_t st);

}  // namespace pca
