// extern "C" entry points for the multihead attention block: argument validation and
// dispatch on the arithmetic mode.  (set_transformer-master/modules.py:19-33)
#include "blocks.hpp"

namespace pca {

// ---- the path of one block (BlockPath, blocks.hpp), decided once per call and read by everything below ----
BlockPath block_path(const pca_mab_shape& s, bool inference, bool abi) {
  // LayerNorm variants: the exact chain only
  if (!s.ln && (s.mode == PCA_MODE_BF16 || s.mode == PCA_MODE_FP8)) {
    const bool d256 = s.d == 256;
    // (a fused mab1 has the m inducing-point outputs as keys: always all of them; a caller that
    // masks keys of such a shape gets the exact path, whose softmax honours k_lengths)
    if (s.k_lengths == nullptr && mab1_bf16_supported(s, inference))
      return d256 ? BlockPath::Mab1_256 : BlockPath::Mab1_128;
    if (d256 ? mab0_d256_supported(s) : mab0_bf16_supported(s))
      return d256 ? BlockPath::Mab0_256 : BlockPath::Mab0_128;
    if (inference && sd64_kind(s) != 0) return BlockPath::Sd64;
  }
  // a self-attention-shaped block (SAB, set_transformer-master/modules.py:35-41: per-set queries, nq = nk,
  // dq = dk) that no fused kernel takes, in PCA_MODE_BF16 or PCA_MODE_FP8 (run alike: no fp8 operands): the
  // bf16-operand chain of mab_f32.hip with its attention on the fused core (attn_core.hip, head dims 8 / 16 /
  // 32), so nothing of size nq x nk is ever stored.  Only the pca_mab_* entry points ask for it (abi); the ST
  // engine keeps its blocks as they are.
  return abi && attn_core_sab_ok(s) ? BlockPath::ExactCore : BlockPath::Exact;
}

size_t mab_saved_bytes(BlockPath path, const pca_mab_shape& s) {
  switch (path) {
    case BlockPath::Mab1_128: case BlockPath::Mab1_256: return mab1_bf16_saved_bytes(s);
    case BlockPath::Mab0_128: return mab0_bf16_saved_bytes(s);
    case BlockPath::Mab0_256: return mab0_d256_saved_bytes(s);
    case BlockPath::ExactCore: return mab_f32_saved_bytes(s, true);
    case BlockPath::Exact: case BlockPath::Sd64: break;      // (Sd64: inference only, nothing is saved)
  }
  return mab_f32_saved_bytes(s);
}
// The forward's scratch block serves both kinds of call: the inference path's scratch (inference, saved ==
// NULL, keeps the intermediates there), or the exact chain's saved block (its scratch) when training and
// inference paths differ, whichever is larger.
size_t mab_fwd_ws_bytes(BlockPath inference, BlockPath training, const pca_mab_shape& s) {
  size_t a = 0;
  switch (inference) {
    case BlockPath::Mab1_128: case BlockPath::Mab1_256: a = mab1_bf16_fwd_ws_bytes(s); break;
    case BlockPath::Mab0_128: a = mab0_bf16_fwd_ws_bytes(s); break;
    case BlockPath::Mab0_256: a = mab0_d256_fwd_ws_bytes(s); break;
    case BlockPath::Sd64: a = sd64_fwd_ws_bytes(s); break;
    case BlockPath::Exact: case BlockPath::ExactCore: a = mab_saved_bytes(inference, s); break;
  }
  const size_t b = training != inference ? mab_saved_bytes(training, s) : 0;
  return a > b ? a : b;
}
size_t mab_bwd_ws_bytes(BlockPath path, const pca_mab_shape& s) {
  switch (path) {
    case BlockPath::Mab1_128: return mab1_bf16_bwd_ws_bytes(s);
    case BlockPath::Mab1_256: return mab1_d256_bwd_ws_bytes(s);
    case BlockPath::Mab0_128: return mab0_bf16_bwd_ws_bytes(s);
    case BlockPath::Mab0_256: return mab0_d256_bwd_ws_bytes(s);
    case BlockPath::ExactCore: return mab_f32_bwd_ws_bytes(s, true);
    case BlockPath::Exact: case BlockPath::Sd64: break;
  }
  return mab_f32_bwd_ws_bytes(s);
}
int mab_fwd(BlockPath path, const pca_mab_shape& s, const void* Q, const void* K, const pca_mab_params& p,
            void* Y, void* saved, void* ws, hipStream_t st, int flags, StepCtx* ctx) {
  switch (path) {
    case BlockPath::Mab1_128: case BlockPath::Mab1_256:      // (the many-queries forward serves both widths)
      return mab1_bf16_fwd_ex(s, Q, (const float*)K, p, Y, saved, ws, flags, st, nullptr, ctx);
    case BlockPath::Mab0_128:
      return mab0_bf16_fwd_ex(s, (const float*)Q, K, p, (float*)Y, saved, ws, flags, st, ctx);
    case BlockPath::Mab0_256:
      return mab0_d256_fwd(s, (const float*)Q, K, p, (float*)Y, saved, ws, flags, st, ctx);
    case BlockPath::Sd64:
      return sd64_fwd(s, (const float*)Q, (const float*)K, p, (float*)Y, ws, st);
    case BlockPath::Exact: case BlockPath::ExactCore: break;
  }
  return mab_f32_fwd(s, (const float*)Q, (const float*)K, p, (float*)Y, saved ? saved : ws, st,
                     path == BlockPath::ExactCore);
}
int mab_bwd(BlockPath path, const pca_mab_shape& s, const void* Q, const void* K, const pca_mab_params& p,
            const void* saved, const void* dY, void* dQ, void* dK, int dk_accumulate,
            const pca_mab_grads& g, void* ws, hipStream_t st, StepCtx* ctx) {
  switch (path) {
    case BlockPath::Mab1_128:
      return mab1_bf16_bwd_ex(s, Q, (const float*)K, p, saved, dY, dQ, (float*)dK, dk_accumulate, g,
                              ws, 0, st, nullptr, nullptr, 0, nullptr, ctx);
    case BlockPath::Mab1_256:      // three launches + the 256-wide weight-gradient reduction (d256_host.hip)
      return mab1_d256_bwd(s, Q, (const float*)K, p, saved, dY, dQ, (float*)dK, dk_accumulate, g, ws, st, ctx);
    case BlockPath::Mab0_128:
      return mab0_bf16_bwd_ex(s, (const float*)Q, K, p, saved, (const float*)dY, (float*)dQ, dK,
                              dk_accumulate, g, ws, 0, st, ctx);
    case BlockPath::Mab0_256:
      return mab0_d256_bwd(s, (const float*)Q, K, p, saved, (const float*)dY, (float*)dQ, dK,
                           dk_accumulate, g, ws, st, ctx);
    case BlockPath::Exact: case BlockPath::ExactCore: case BlockPath::Sd64: break;
  }
  return mab_f32_bwd(s, (const float*)Q, (const float*)K, p, saved, (const float*)dY, (float*)dQ,
                     (float*)dK, dk_accumulate, g, ws, st, path == BlockPath::ExactCore, ctx);
}

int no_stale_pack(const char* where, bool pack_allowed) {
  PCA_REQUIRE(pack_allowed || !pack_pending(),
              "%s: a deferred pack is pending on this thread (only pca_st_forward / pca_st_train_fwd_bwd "
              "consume it)", where);
  return PCA_OK;
}
}  // namespace pca

extern "C" {

// the path of a pca_mab_* call: what block_path answers with the SAB chain on the fused core included
static pca::BlockPath abi_path(const pca_mab_shape* s, bool inference = false) {
  return pca::block_path(*s, inference, true);
}
static bool on_chain(pca::BlockPath path) {
  return path == pca::BlockPath::Exact || path == pca::BlockPath::ExactCore;
}

// An explicit PCA_MODE_BF16 request must be served by a fused kernel (no silent change of
// arithmetic at this level); callers that want "bf16 where available" query
// pca_mab_saved_bytes() first, which returns 0 for unsupported bf16 shapes.
static int bf16_demand(const pca_mab_shape* s, pca::BlockPath path) {
  if ((s->mode == PCA_MODE_BF16 || s->mode == PCA_MODE_FP8) && path == pca::BlockPath::Exact) {
    pca::set_error("mab: no bf16 / fp8 kernel for B=%d nq=%d nk=%d dq=%d dk=%d d=%d h=%d q_shared=%d",
                   s->B, s->nq, s->nk, s->dq, s->dk, s->d, s->h, s->q_shared);
    return PCA_EUNSUPPORTED;
  }
  if (s->mode != PCA_MODE_BF16 && s->mode != PCA_MODE_F32 && s->mode != PCA_MODE_FP8) {
    pca::set_error("mab: unknown mode %d", s->mode);
    return PCA_EINVAL;
  }
  return PCA_OK;
}
static int check_f32(const pca_mab_shape* s, pca::BlockPath path) {
  // the GEMM chains exchange fp32 only; the fused kernels validate their own dtypes
  PCA_REQUIRE(!on_chain(path) || (s->q_dtype == PCA_F32 && s->k_dtype == PCA_F32 && s->y_dtype == PCA_F32),
              "mab: the exact fp32 path needs fp32 Q, K and Y");
  return PCA_OK;
}

size_t pca_mab_saved_bytes(const pca_mab_shape* s) {
  if (pca::validate_shape(s) != PCA_OK) return 0;
  const pca::BlockPath path = abi_path(s);
  return bf16_demand(s, path) != PCA_OK ? 0 : pca::mab_saved_bytes(path, *s);
}
size_t pca_mab_fwd_ws_bytes(const pca_mab_shape* s) {
  if (pca::validate_shape(s) != PCA_OK) return 0;
  const pca::BlockPath inference = abi_path(s, true);
  return bf16_demand(s, inference) != PCA_OK ? 0 : pca::mab_fwd_ws_bytes(inference, abi_path(s), *s);
}
size_t pca_mab_bwd_ws_bytes(const pca_mab_shape* s) {
  if (pca::validate_shape(s) != PCA_OK) return 0;
  const pca::BlockPath path = abi_path(s);
  return bf16_demand(s, path) != PCA_OK ? 0 : pca::mab_bwd_ws_bytes(path, *s);
}

// runs the body between two checks that no deferred pack is pending: these calls do not consume one
#define PCA_WITH_PACK_CHECK(where, call)                             \
  do {                                                               \
    PCA_TRY(pca::no_stale_pack(where, false));                       \
    const int rc_ = (call);                                          \
    if (rc_ != PCA_OK) return rc_;                                   \
    return pca::no_stale_pack(where " (exit)", false);               \
  } while (0)

int pca_mab_fwd(const pca_mab_shape* s, const void* Q, const void* K,
                const pca_mab_params* p, void* Y, void* saved, void* ws, void* stream) {
  PCA_TRY(pca::validate_shape(s));
  PCA_REQUIRE(Q && K && p && Y, "mab_fwd: null pointer");
  PCA_REQUIRE(p->wq && p->bq && p->wk && p->bk && p->wv && p->bv && p->wo && p->bo,
              "mab_fwd: null parameter");
  const pca::BlockPath path = abi_path(s, saved == nullptr);
  PCA_TRY(bf16_demand(s, path));
  PCA_TRY(check_f32(s, path));
  PCA_REQUIRE(ws != nullptr || (saved != nullptr && on_chain(path)), "mab_fwd: scratch block required");
  PCA_WITH_PACK_CHECK("pca_mab_fwd",
                      pca::mab_fwd(path, *s, Q, K, *p, Y, saved, ws, pca::as_stream(stream)));
}

int pca_mab_bwd(const pca_mab_shape* s, const void* Q, const void* K,
                const pca_mab_params* p, const void* saved, const void* dY, void* dQ,
                void* dK, int dk_accumulate, const pca_mab_grads* g, void* ws, void* stream) {
  PCA_TRY(pca::validate_shape(s));
  PCA_REQUIRE(Q && K && p && saved && dY && g && ws, "mab_bwd: null pointer");
  PCA_REQUIRE(g->wq && g->bq && g->wk && g->bk && g->wv && g->bv && g->wo && g->bo,
              "mab_bwd: null gradient buffer");
  const pca::BlockPath path = abi_path(s);
  PCA_TRY(bf16_demand(s, path));
  PCA_TRY(check_f32(s, path));
  PCA_WITH_PACK_CHECK("pca_mab_bwd",
                      pca::mab_bwd(path, *s, Q, K, *p, saved, dY, dQ, dK, dk_accumulate, *g, ws,
                                   pca::as_stream(stream)));
}

int pca_linear_fwd(const float* X, const float* W, const float* b, float* Y, int64_t M,
                   int din, int dout, void* stream) {
  PCA_REQUIRE(X && W && b && Y && M > 0 && din > 0 && dout > 0, "linear_fwd: bad arguments");
  return pca::linear_fwd_f32(X, W, b, Y, M, din, dout, pca::as_stream(stream));
}
size_t pca_linear_bwd_ws_bytes(int64_t, int, int) { return 256; }
int pca_linear_bwd(const float* X, const float* W, const float* dY, float* dX, float* dW,
                   float* db, int64_t M, int din, int dout, void* ws, void* stream) {
  (void)ws;
  PCA_REQUIRE(X && W && dY && M > 0 && din > 0 && dout > 0, "linear_bwd: bad arguments");
  return pca::linear_bwd_f32(X, W, dY, dX, dW, db, M, din, dout, pca::as_stream(stream));
}
}
