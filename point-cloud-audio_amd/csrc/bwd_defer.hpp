// The end of a backward pass: the job tables of the reductions only the optimiser reads (weight gradients,
// fixed-order slab sums, the shared-query post stages, the classifier's gradient), BwdDefer, which collects
// them over the blocks of a step, and the launches that run them - wgrad128.hip (k_wgrad128, k_wgrad_small),
// bwd_defer.hip (bwd_defer_flush, k_terminal1, k_mab0_post1 / 2), slab_sum.hip, wgrad256.hip (the d = 256
// job) - plus the PMA head launch that queues the classifier's job (pma_head.hip).
#pragma once
#include "pca_common.h"
#include "soft_targets.hpp"

namespace pca {

// fixed-order sums of per-workgroup partial tensors ([S][n] fp32 -> out[n]), several per launch
struct SlabSumJob {
  const float* slabs;
  float* out;
  int S, n, accumulate;
  int stride;             // floats between consecutive slabs (0: n)
};
struct SlabSumJobs {
  SlabSumJob j[40];
  int n;
};
inline bool slab_sum_job_ok(const SlabSumJob& j) {      // 16-byte accesses throughout
  return j.n % 4 == 0 && j.stride % 4 == 0 && ((uintptr_t)j.out & 15) == 0 &&
         ((uintptr_t)j.slabs & 15) == 0;
}
int slab_sum_jobs(const SlabSumJobs& J, hipStream_t st);
int slab_sum(const float* slabs, int S, int n, float* out, int accumulate, hipStream_t st);

// ---- batched weight-gradient reduction on the MFMA (wgrad128.hip) ------------------
// job: dW[128 x 128] += G[M x 128]^T . A[M x 128]  (only output rows [g_lo, g_hi) are written:
// block-diagonal per-head products), db[128] += column sums of G (nullable).
struct WgradJob {
  const void* G;
  const void* A;
  float* dW;
  float* db;
  int64_t M;
  int g_lo, g_hi;
  float* slab;            // set by the launcher: [workgroups][(g_hi - g_lo) * 128 (+ 128 with db)]
                          // partials, summed in a fixed order afterwards (null: fp32 atomics)
  // optional (bf16 G): ReLU mask words of the many-queries forward over the same rows
  // (mab1_mask_index<128> with N % 128 == 0: 64 words per 16 rows); G is then used as G . [mask] -
  // the fc_o job reads dY and the mask instead of a materialised dZ
  const uint32_t* mask;
};
struct WgradJobs {
  WgradJob j[16];
  int n;
};
struct WgradSlabs {          // optional slab mode of wgrad128_launch
  float* ws;                 // partials go here (cap bytes) ...
  size_t cap;
  SlabSumJobs* sums_out;     // ... and their sum jobs are appended here (run them afterwards)
  const SlabSumJobs* riders; // sums that are due now: extra workgroup rows of this launch
  size_t used;               // out: bytes of ws taken
};
// g_bf16 / a_bf16: element type of every job's G / A (bf16 or fp32)
// `small`: the layer-1 fc_v job (wgrad_small_f32_launch's, with a slab) as further rows of the same launch
struct SmallWgradArgs;
int wgrad128_launch(const WgradJobs& jobs, bool g_bf16, bool a_bf16, int rows_per_wg,
                    hipStream_t st, WgradSlabs* slabs = nullptr, const SmallWgradArgs* small = nullptr);
// The two halves of wgrad128_launch for a caller that puts two lists into one launch: wgrad128_place
// gives every job of a list its slabs (slab mode; rows_per_wg doubles until they fit `slabs->cap`) and
// appends their sum jobs; wgrad128_launch_step runs a placed bf16 list (G, A bf16; empty when it ran
// beside layer 1's few-queries backward: bwd_defer_ride) and a placed fp32 list, each with its own rows
// per workgroup (>= 128), and the riders as ONE launch (k_wgrad128_step).
int wgrad128_place(WgradJobs& jobs, int& rows_per_wg, WgradSlabs* slabs);
int wgrad128_launch_step(const WgradJobs& bf16_jobs, int rows_per_wg_bf16, const WgradJobs& f32_jobs,
                         int rows_per_wg_f32, const SlabSumJobs& riders, hipStream_t st,
                         const SmallWgradArgs* small = nullptr);

// ---- the d = 256 job (wgrad256.hip; launchers in d256.hpp) ------------------
// dW[256 x 256] += G^T A, db[256] += colsum(G) (nullable); G, A bf16 [M][256]
struct Wgrad256Job {
  const void* G;      // bf16, or fp32 with wgrad256_launch_t(..., f32_operands = true)
  const void* A;
  float* dW;
  float* db;
  int64_t M;
  // optional (bf16 LDS-DMA kernel only, M % 32 == 0): ReLU mask words of the many-queries forward
  // over the same rows (mab1_mask_index<256> with N % 128 == 0, i.e. 128 words per 16 rows); G is
  // then used as G . [mask] - the job reads dY and the mask instead of a materialised dZ
  const uint32_t* mask;
};
struct Wgrad256Jobs {
  Wgrad256Job j[8];
  int n;
};

// ---- the small reductions that ride in the post launches (bwd_defer.hip) ------------------
struct ClsWgradArgs {
  const float *dlogits, *P, *lossv, *corrv;
  int B, d, C;
  float *dWc, *dbc, *loss_out, *stats;
};
struct SmallWgradArgs {
  const float *G, *X;
  int64_t M;
  int dq, rows_per_wg;
  int64_t x_head_stride;
  float *dW, *db;
  float* slab;            // per-workgroup partials [wg][128*dq + 128] instead of atomics (null: atomics)
};
// shared-query parameter gradients (dWk, dWq, dbq, dI) of up to 3 MABs: tiny, latency-bound
// kernels, so callers may collect them and run ONE pair of launches at the end of a phase
struct Mab0PostJob {
  const float *dQs, *DG, *Qp, *Wk, *I, *Wq;
  float *dWk, *dQp, *dWq, *dbq, *dI;
  int m, d, dk, dq, h;
  float sl2e;
  // dQs == null: the sum over sets of dO [B][m][d] is taken inside the post kernel (cheaper
  // than B workgroups adding atomically into the same m*d addresses)
  const float* dO;
  int B;
};
struct Mab0PostJobs {
  Mab0PostJob j[3];
  int n;
};
int mab0_post_launch(const Mab0PostJobs& J, hipStream_t st);

// ---- what a step collects, and its flush (bwd_defer.hip) ------------------
// Terminal reductions of a backward pass (only the optimiser / the all-reduce reads their
// results): a caller that runs several blocks collects them and flushes ONCE at the end of the
// phase - one weight-gradient launch over the bf16 and the fp32 job table (PCA_WGRAD_FOLD=0: one
// launch each) and one pair of post launches instead of one set per block.  Their operands live in per-block workspaces that
// stay untouched until then.
struct BwdDefer {
  SlabSumJobs sums;       // partial sums the post stages read: run before them
  SlabSumJobs late;       // partial sums only the optimizer reads (ride in the last launches)
  // d = 256: the [B*m]-row weight-gradient jobs of all blocks (fp32 operands, k_wgrad256<float>):
  // one launch + one sum at the end instead of one pair per block.  Collected only when wg256_ws is
  // set (room for wgrad256_ws_bytes(8, rows)); the operands stay in the blocks' workspaces
  struct Wg256 { const void *G, *A; float *dW, *db; int64_t M; } wg256[8];
  int wg256_n;
  void* wg256_ws;
  float* slab_ws;         // room for the weight-gradient partials of the two deferred lists
  size_t slab_cap;        // (bytes; null / 0: those reductions use fp32 atomics)
  Mab0PostJobs posts;
  WgradJobs wg_bf16;      // G, A bf16, M = B*N rows   (512 ... 1024 rows per workgroup: bwd_defer_flush)
  WgradJobs wg_f32;       // G, A fp32, M = B*m rows   (128 rows per workgroup)
  // classifier weight gradient + loss counters, layer-1 fc_v gradient: they ride in the first
  // post launch (k_terminal1) as extra job rows
  ClsWgradArgs cls;
  SmallWgradArgs sw;
  int has_cls, has_sw;
  // the bf16 list already ran, beside layer 1's few-queries backward (bwd_defer_ride): its sum jobs, and
  // the bytes of slab_ws its partials take (the flush places the fp32 list behind them)
  int ride_done;
  size_t ride_used;
  SlabSumJobs ride_late;
};
int bwd_defer_flush(BwdDefer& D, hipStream_t st);
// Whether the bf16 list collected so far may run now, in the launch of layer 1's few-queries backward
// (slab mode with room lent, the two lists folded, PCA_WGRAD_RIDE not 0); if so `jobs` receives the list
// placed exactly as the flush would place it (same rows per workgroup, same slabs at the start of slab_ws)
// and D records it as done.  The caller launches it (mab0_small_ride_launch).
bool bwd_defer_ride(BwdDefer& D, WgradJobs* jobs, int* rows_per_wg, int* rc);
// post stages + riders (`late`: sums nobody reads before the optimizer, e.g. weight gradients)
int terminal_launch(const BwdDefer& D, hipStream_t st, const SlabSumJobs* late = nullptr);
int wgrad256_flush_deferred(BwdDefer& D, hipStream_t st);       // d256_host.hip
bool wgrad_slabs_on();       // reductions of the fused d = 128 path as slabs + fixed-order sums
                             // (PCA_WGRAD_SLABS=0: fp32 atomics)
bool wgrad_fold_on();        // the two deferred d = 128 lists in one launch (PCA_WGRAD_FOLD=0: two)
bool wgrad_ride_on();        // the bf16 list beside layer 1's few-queries backward (PCA_WGRAD_RIDE)
bool post_fuse_on();         // both shared-query post stages inside k_terminal1, the layer-1 fc_v job in
                             // k_wgrad128_step (PCA_POST_FUSE=0: k_terminal1, then k_mab0_post2)
// launch `jobs` now, or append them to the matching list of `defer`
int wgrad128_defer(BwdDefer* defer, const WgradJobs& jobs, bool bf16, int rows_per_wg,
                   hipStream_t st);
// dW[128 x dq] += G[M x 128]^T . X_h[M x dq] (dq <= 4; X_h = X + head(f)*x_head_stride), db += colsum
int wgrad_small_f32_launch(const float* G, const float* X, int64_t M, int dq,
                           int64_t x_head_stride, float* dW, float* db, hipStream_t st,
                           BwdDefer* defer = nullptr);
// the same with bf16 G over one input (no head stride), 128 rows per workgroup: never deferred
int wgrad_small_bf16_launch(const __bf16* G, const float* X, int64_t M, int dq, float* dW, float* db,
                            hipStream_t st);

// ---- the PMA head launch (pma_head.hip) ------------------
// PMA epilogue + classifier + cross-entropy (forward and backward) + PMA backward epilogue of the
// train step in ONE launch per set (k_pma_head / k_pma_head1, after mab0_bf16_fwd_ex(...,
// PCA_F_SKIP_EPILOGUE); followed by mab0_bf16_bwd_ex(..., PCA_F_SKIP_HEAD)); the set-resident forward runs
// the same stages in its own tail (set128_fwd.hip).  Both take the arguments pma_head_args builds.
struct PmaHeadArgs {
  // forward epilogue
  const float *Tp, *Mp, *Lp;
  int S;
  float *T, *LSE;
  const float *Qp, *WvT, *bv, *WoT, *bo;
  int m, d, dk, h;
  float *H, *Osave, *Zsave;
  // classifier + loss
  const float *Wc, *bc;
  const int64_t* labels;
  SoftTargets soft;
  int B, C;
  float grad_scale;
  float *logits, *dlogits, *dP, *lossv, *corrv;
  // backward epilogue
  const float *Wo, *Wv;
  int Rp;
  float *dZ, *dO, *Th, *dTf;
  __bf16 *dTb, *dTt;
  float *Delta, *LSEp, *zero_ptr;
  int zero_n;
};
// P [B, d] receives the pooled features; the classifier's weight gradient is queued in `defer`.  ws_bwd is
// the PMA's backward workspace.
int pma_head_args(const pca_mab_shape& s, const pca_mab_params& p, void* saved, void* ws_bwd,
                  float* P, const float* Wc, const float* bc, const int64_t* labels,
                  const SoftTargets& soft, int C,
                  float grad_scale, float* logits, float* dlogits, float* dP, float* dWc,
                  float* dbc, float* loss_out, float* stats, float* cls_ws, BwdDefer* defer,
                  PmaHeadArgs* out);
int pma_head_launch(const PmaHeadArgs& a, hipStream_t st);

}  // namespace pca
