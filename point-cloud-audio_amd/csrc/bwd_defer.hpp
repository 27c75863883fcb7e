// The end of a backward pass: the job tables of the reductions only the optimiser reads (weight gradients,
// fixed-order slab sums, the shared-query post stages, the classifier's gradient), BwdDefer, which collects them
// over the blocks of a step, TailForm (the tail's switches) and TailPlan (every slab, rider and launch of the flush:
// tail_plan.hip, host code only), and the launches that run a plan - bwd_defer.hip (bwd_defer_flush, k_terminal1,
// k_mab0_post1 / 2), wgrad128.hip, slab_sum.hip, wgrad256.hip - plus the PMA head launch (pma_head.hip).
#pragma once
#include "pca_common.h"
#include "soft_targets.hpp"

namespace pca {

// fixed-order sums of per-workgroup partial tensors ([S][n] fp32 -> out[n]), several per launch
struct SlabSumJob {
  const float* slabs;
  float* out;
  int S, n;
  int accumulate;         // 0: out = sum; 1: out + sum, out first in the chain of additions; 2: out + sum, the
                          // sum formed as with 0 and added ONCE (|acc - (P + fresh)| is one fp32 rounding)
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
inline int64_t wgrad_max_rows(const WgradJobs& jobs) {
  int64_t m = 0;
  for (int i = 0; i < jobs.n; ++i) m = jobs.j[i].M > m ? jobs.j[i].M : m;
  return m;
}
// g_bf16 / a_bf16: element type of every job's G / A.  The jobs come placed (plan_tail; slab null: fp32
// atomics); `riders`: sums that are due now, `small`: the layer-1 fc_v job (with a slab), both as further rows
struct SmallWgradArgs;
int wgrad128_launch(const WgradJobs& jobs, bool g_bf16, bool a_bf16, int rows_per_wg, hipStream_t st,
                    const SlabSumJobs* riders = nullptr, const SmallWgradArgs* small = nullptr);
// its grid (k_wgrad128): x = the widest of the job rows and the rider rows
int wgrad128_shape(const WgradJobs& jobs, int rows_per_wg, const SlabSumJobs& riders,
                   const SmallWgradArgs* small, unsigned* gx, unsigned* gy, int* sw_rows);
// A placed bf16 list (empty when it ran beside layer 1's few-queries backward: bwd_defer_ride) and a placed fp32
// list, each with its own rows per workgroup (>= 128), and the riders as ONE launch (k_wgrad128_step)
struct WgradStepShape {
  unsigned gx, gy;
  int sw_rows;               // rows of the fc_v job
  SlabSumJobs riders;        // (bf16 list empty: cut into column ranges as wide as the fp32 rows)
};
int wgrad128_step_shape(const WgradJobs& bf16_jobs, int rows_per_wg_bf16, const WgradJobs& f32_jobs,
                        int rows_per_wg_f32, const SlabSumJobs& riders, const SmallWgradArgs* small,
                        WgradStepShape* out);
int wgrad128_launch_step(const WgradJobs& bf16_jobs, int rows_per_wg_bf16, const WgradJobs& f32_jobs,
                         int rows_per_wg_f32, const WgradStepShape& shape, hipStream_t st,
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
constexpr int POST_FC = 4, POST_MAXM = 16;      // shapes the fused post rows of k_terminal1 cover

// ---- the switches of the d = 128 backward tail, read in one place ------------------
// tail_form_from_env (tail_plan.hip) holds the defaults and resolves what depends on what in the environment (no
// caller sees `ride` without `slabs`); what depends on shapes stays with the code that knows them.  plan() reads it
// once per engine call, the step's BwdDefer carries it, a stand-alone block call reads it at its entry.
struct TailForm {
  bool slabs;          // reductions as per-workgroup slabs + fixed-order sums (PCA_WGRAD_SLABS=0: fp32 atomics)
  bool fold;           // the two deferred lists in one k_wgrad128_step (PCA_WGRAD_FOLD=0: a k_wgrad128 each)
  bool ride;           // the bf16 list beside layer 1's few-queries backward (PCA_WGRAD_RIDE; with slabs, fold and
                       // midfuse_small only)
  bool post_fuse;      // both post stages in k_terminal1, the layer-1 fc_v job in the fp32 list's launch (PCA_POST_FUSE)
  bool midfuse_wide, midfuse_small;   // the mid chain inside layer 2's / layer 1's few-queries backward
  bool dz_mask;        // the fc_o job masks dY itself (PCA_D128_DZ_MASK=0: the backward writes dZ)
};
TailForm tail_form_from_env();

// ---- what a step collects, its plan and its flush (tail_plan.hip, bwd_defer.hip) ------------------
// What the planner has handed out so far in a step (bwd_defer_ride leaves it for the flush to go on from)
struct TailPlaced {
  size_t used;            // bytes of slab_ws taken: 256-byte aligned ranges, bf16 list, fp32 list, fc_v job
  SlabSumJobs late;       // the sums of what has been placed, in the order k_terminal1 runs them
  bool bf16_ran;          // the bf16 list ran already, beside layer 1's few-queries backward
};
// Terminal reductions of a backward pass (only the optimiser / the all-reduce reads their results): a caller that runs
// several blocks collects them and flushes ONCE at the end of the phase; their operands stay in place until then.
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
  TailForm form;          // the call's switches (StepPlan::tail)
  Mab0PostJobs posts;
  WgradJobs wg_bf16;      // G, A bf16, M = B*N rows   (512 ... 1024 rows per workgroup: plan_tail)
  WgradJobs wg_f32;       // G, A fp32, M = B*m rows   (128 rows per workgroup)
  ClsWgradArgs cls;       // classifier weight gradient + loss counters: a row of k_terminal1
  SmallWgradArgs sw;      // layer-1 fc_v gradient: where TailPlan::fcv says
  int has_cls, has_sw;
  TailPlaced placed;
};
inline TailForm tail_form_of(const BwdDefer* d) { return d != nullptr ? d->form : tail_form_from_env(); }

enum class FcvRuns {      // where the layer-1 fc_v job runs, and who sums its partials
  Nowhere,                // (no such job)
  WgradRows,              // rows of the fp32 list's weight-gradient launch; its two sums are `late` riders
  TerminalRows,           // rows of k_terminal1, adding atomically
  TerminalRowsPost2Sums   // rows of k_terminal1 writing partials that rider rows of k_mab0_post2 sum
};
// (Wgrad256: wgrad256_flush_deferred; SumsDue / SumsLate2: k_slab_sum_jobs over the due sums no weight-gradient
//  launch carried / over late2 when there is no post job - launchers with grids of their own: 0 here)
enum class TailKernel { WgradStep, Wgrad128Bf16, Wgrad128F32, Wgrad256, SumsDue, Terminal1, Post1, Post2, SumsLate2 };
struct TailLaunch { TailKernel kernel; unsigned gx, gy; };
// Everything bwd_defer_flush runs, decided before the first launch: plan_tail launches nothing and dereferences no
// device pointer.  Slabs come from ONE cursor (placed.used) in the order bf16 list (inside 3/4 of the room), fp32
// list, fc_v job; rows per workgroup (bf16: 512, from 98304 rows on up to 1024; fp32: 128) double until a list fits.
struct TailPlan {
  int rpw_bf16, rpw_f32;
  double rows_bf16, rows_f32;  // (all jobs of a list together)
  WgradJobs bf16, f32;         // the lists with their slabs (a list without rows: empty)
  FcvRuns fcv;
  SmallWgradArgs small;        // the fc_v job with its slab
  WgradStepShape step;         // step.riders: the due sums, as the first weight-gradient launch carries them
  TailPlaced placed;           // placed.late: k_terminal1's riders
  SlabSumJobs late2;           // k_mab0_post2's riders
  bool post_fused;             // both post stages in k_terminal1
  TailLaunch seq[6];           // the launches in order
  int nseq;
};
// bf16_only: stop once the bf16 list is placed (bwd_defer_ride)
int plan_tail(const BwdDefer& D, TailPlan* P, bool bf16_only = false);
int bwd_defer_flush(BwdDefer& D, hipStream_t st);
// Whether the bf16 list collected so far may run now, in the launch of layer 1's few-queries backward (TailForm::ride,
// room lent); if so `jobs` receives it as plan_tail places it and D.placed records that.  The caller launches it.
bool bwd_defer_ride(BwdDefer& D, WgradJobs* jobs, int* rows_per_wg, int* rc);
int wgrad256_flush_deferred(BwdDefer& D, hipStream_t st);       // d256_host.hip
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
