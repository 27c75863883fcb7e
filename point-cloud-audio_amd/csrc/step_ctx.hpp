// StepCtx: what one engine call hands from one internal stage to the next, at every width.  The blocks'
// entry points (blocks.hpp) take it as a nullable pointer.
#pragma once
#include "pca_common.h"
#include "weight_images.hpp"
#include "bwd_defer.hpp"

namespace pca {

struct DxHandoff {            // mab1's dX = dQp Wq, deferred into the few-queries block's DX launch
  const __bf16 *dQp, *WqT;
  __bf16* dX;
  int B, N;
};
// What one engine call (pca_st_train_fwd_bwd, pca_st_forward) hands from one internal stage to the next.
// It lives on that call's stack and goes down as a nullable pointer: null is a stand-alone block call
// (pca_mab_fwd / pca_mab_bwd), which converts every image itself, defers nothing and hands nothing over.
struct StepCtx {
  const WeightImages* images;   // the step's ready-made weight images (null: converted on the spot)
  BwdDefer* defer;              // where the block queues its terminal reductions (null: it launches them)
  // d = 256 training forward, set around an ISAB's few-queries block (saved1 null: not set): that block
  // then ends in mid256_fwd, which also writes the K / V images of the many-queries block (s1, p1,
  // saved1), and says so in mid_done; the caller passes PCA_F_KV_READY to that block's forward
  pca_mab_shape s1;
  pca_mab_params p1;
  void* saved1;
  bool mid_done;
  // d = 256 backward, armed around an ISAB's pair of calls with separate workspaces for the two blocks
  // (dQp must outlive mab1's call): mab1's fc_q weight-gradient job {dQp, X} goes to the few-queries
  // block, whose two jobs {dKp, X}, {dVp, X} read the same X - launched together, the three share each
  // X tile through the XCD's L2 (k_wgrad256's shared-operand order) - and its dX = dQp Wq likewise
  bool armed, has, has_dx;
  Wgrad256Job job;
  DxHandoff dx;
  // d = 64 chain backward (mab_f32_bwd): where a block may leave the slabs of its wgrad64 calls until the flush
  // (room the step no longer uses; the block advances the cursor) and the list their sums join - rider rows of
  // the step's terminal launch instead of a launch per block.  Null: the block sums before it returns.
  SlabSumJobs* wg64_late;
  float* wg64_room;
  size_t wg64_room_elems;
};
inline BwdDefer* defer_of(const StepCtx* c) { return c != nullptr ? c->defer : nullptr; }
inline const WeightImages* images_of(const StepCtx* c) { return c != nullptr ? c->images : nullptr; }
// a handed-over job / dX nobody took (the following block was not the projected-keys few-queries one)
int wgrad256_handoff_flush(StepCtx* ctx, void* ws, hipStream_t st);

}  // namespace pca
