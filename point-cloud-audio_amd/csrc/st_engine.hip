// Whole-model engine for the ST classifier (Code/models.py:13-44) and its train step
// (Code/settransformer.py:100-108): one host call enqueues every kernel of
// forward -> cross-entropy -> backward against flat parameter / gradient vectors laid out
// in state_dict order.  No Python, autograd or allocator sits between the kernels, so the
// caller can capture the call in a hipGraph.
#include <stdlib.h>
#include "blocks.hpp"
#include "weight_images.hpp"
#include "bwd_defer.hpp"
#include "step_ctx.hpp"
#include "d256.hpp"
#include "pack_body.hpp"
#include "set128.hpp"

namespace pca {

namespace {

struct MabOff {   // element offsets of one MAB's 8 tensors in the flat vector
  int64_t wq, bq, wk, bk, wv, bv, wo, bo;
};

struct Layout {
  int64_t I[2];
  MabOff mab0[2], mab1[2];
  int64_t S;
  MabOff pma;
  int64_t wc, bc;
  int64_t total;
  int64_t enc1_begin;
};

inline MabOff lay_mab(int64_t& o, int dq, int dk, int d) {
  MabOff m;
  m.wq = o; o += (int64_t)d * dq;
  m.bq = o; o += d;
  m.wk = o; o += (int64_t)d * dk;
  m.bk = o; o += d;
  m.wv = o; o += (int64_t)d * dk;
  m.bv = o; o += d;
  m.wo = o; o += (int64_t)d * d;
  m.bo = o; o += d;
  return m;
}

// state_dict order of Code/models.py:34-41 (ISAB: I, mab0, mab1 -- modules.py:45-49)
inline Layout layout(const pca_st_config& c) {
  Layout L;
  int64_t o = 0;
  for (int li = 0; li < 2; ++li) {
    const int din = li == 0 ? c.din : c.d;
    if (li == 1) L.enc1_begin = o;
    L.I[li] = o; o += (int64_t)c.m * c.d;
    L.mab0[li] = lay_mab(o, c.d, din, c.d);   // MAB(dim_out, dim_in, dim_out)
    L.mab1[li] = lay_mab(o, din, c.d, c.d);   // MAB(dim_in, dim_out, dim_out)
  }
  L.S = o; o += (int64_t)c.k * c.d;
  L.pma = lay_mab(o, c.d, c.d, c.d);
  L.wc = o; o += (int64_t)c.C * c.d;
  L.bc = o; o += c.C;
  L.total = o;
  return L;
}

inline pca_mab_params params_at(const float* base, const MabOff& m) {
  return pca_mab_params{base + m.wq, base + m.bq, base + m.wk, base + m.bk,
                        base + m.wv, base + m.bv, base + m.wo, base + m.bo,
                        nullptr, nullptr, nullptr, nullptr};
}
inline pca_mab_grads grads_at(float* base, const MabOff& m) {
  return pca_mab_grads{base + m.wq, base + m.bq, base + m.wk, base + m.bk,
                       base + m.wv, base + m.bv, base + m.wo, base + m.bo,
                       nullptr, nullptr, nullptr, nullptr};
}

inline pca_mab_shape shape(const pca_st_config& c, int nq, int nk, int dq, int dk,
                           int q_shared) {
  pca_mab_shape s{};
  s.B = c.B; s.nq = nq; s.nk = nk; s.dq = dq; s.dk = dk; s.d = c.d; s.h = c.h;
  s.q_shared = q_shared; s.mode = c.mode;
  s.q_dtype = s.k_dtype = s.y_dtype = PCA_F32;
  return s;
}

// The engine-level path of one call: which fused forms run, what is deferred, what gets room.  Filled once
// per call by plan() and read by carve(), the preparation, the forward and the backward, the blocks' own
// dispatch in api_mab.hip included: mab_fwd, mab_bwd and the *_bytes functions take the plan's path.  DESIGN.md 5
struct StepPlan {
  bool training;
  pca_mab_shape m0[2], m1[2], pma;   // per ISAB: mab0 = MAB(I, X), mab1 = MAB(X, H); the PMA
  BlockPath path_m0[2], path_m1[2], path_pma;   // which kernel family serves each (block_path; an inference
                                                // call: the inference paths)
  bool act_bf16;       // hidden activations Y1, Y2 (and their gradients) travel in bf16
  // everything below is false in an inference call
  bool isab128[2];     // the layer runs as ONE fused d = 128 ISAB (isab_bf16_fwd / _bwd)
  bool isab256[2];     // d = 256, both blocks on fused kernels: the few-queries forward ends in the per-set mid
                       // kernel (mid256.hip); [1] is also the hand-over form of enc.1's backward
  bool img_m1[2], img_m0[2];   // d = 256: the block asks for weight images of the step's table
  bool img256, img256_f8;      // d = 256: the table exists (bf16 images / the e4m3 ones of the fp8 mode)
  bool prep256;        // d = 256: the query side of all three few-queries blocks in the preparation launch
  bool pma_head;       // the PMA epilogue + classifier + loss launch (k_pma_head) exists: d = 128
  bool pma256;         // d = 256: the PMA's post stages wait for the flush, in a workspace of its own
  bool fq_defer[2];    // so does the post stage of the layer's few-queries block
  bool armed[2];       // d = 256 backward: mab1's fc_q weight-gradient job and dX are handed to the few-queries
                       // block, whose jobs read the same X (StepCtx::armed); the two blocks then need
                       // separate workspaces
  bool defer_wg;       // d = 256: the [B*m]-row weight-gradient jobs of all five blocks in one launch at the
                       // flush - needs every block's operands in place until then
  bool set128_room;    // the shape fits the set-resident launch: carve() reserves its exchange area on this alone
  // per-call switches (environment read on every call: tests compare the two forms in-process)
  bool set128;         // the set-resident forward (set128_fwd.hip) runs, with or without `lengths`
                       //                                                            (PCA_SET128=0: per-block launches)
  bool fuse_head;      // ... with the head stages in its own tail                   (PCA_SET128_HEAD=0: as a launch)
  bool pma_bwd;        // ... and then the PMA's attention backward too              (PCA_SET128_PMABWD=0: k_mab0_bwd)
  TailForm tail;       // the d = 128 backward tail's switches, resolved (tail_form_from_env)
};

inline StepPlan plan(const pca_st_config& c, bool training, const int32_t* lengths) {
  // `lengths` changes no answer here and no workspace size: only the q_shared blocks carry it, which
  // mab1_bf16_supported never takes, and neither mab0_bf16_supported, mab0_d256_supported, sd64_kind's
  // q_shared branch nor any *_bytes function reads k_lengths.  The set-resident d = 128 launch takes dense
  // and variable-length steps alike (Set128FwdArgs::lengths) in the exchange area reserved on the shape.  So
  // pca_st_ws_bytes, which has no lengths, and the calls carve alike.
  StepPlan pl{};
  pl.training = training;
  for (int li = 0; li < 2; ++li) {
    const int din = li == 0 ? c.din : c.d;
    pl.m0[li] = shape(c, c.m, c.N, c.d, din, 1);
    pl.m1[li] = shape(c, c.N, c.m, din, c.d, 0);
  }
  pl.pma = shape(c, c.k, c.N, c.d, c.d, 1);
  if (training && c.mode != PCA_MODE_F32) {
    // bf16 activations only when EVERY block runs on a fused kernel that understands them
    StepPlan t = pl;
    t.m1[0].y_dtype = PCA_BF16;
    t.m0[1].k_dtype = PCA_BF16;
    t.m1[1].q_dtype = PCA_BF16;
    t.m1[1].y_dtype = PCA_BF16;
    t.pma.k_dtype = PCA_BF16;
    const bool isab128 = isab_bf16_supported(t.m0[0], t.m1[0]) &&
                         isab_bf16_supported(t.m0[1], t.m1[1]);
    // d = 256: every block has a fused kernel of its own (no ISAB-level fusion)
    const bool blocks256 = block_path(t.m0[0]) == BlockPath::Mab0_256 && block_path(t.m1[0]) == BlockPath::Mab1_256 &&
                           block_path(t.m0[1]) == BlockPath::Mab0_256 && block_path(t.m1[1]) == BlockPath::Mab1_256;
    if ((isab128 || blocks256) && is_mab0(block_path(t.pma))) {
      pl = t;
      pl.act_bf16 = true;
    }
  }
  // variable-size sets: the points are the KEYS of the three blocks that attend over them
  pl.m0[0].k_lengths = pl.m0[1].k_lengths = pl.pma.k_lengths = lengths;
  for (int li = 0; li < 2; ++li) {
    pl.path_m0[li] = block_path(pl.m0[li], !training);
    pl.path_m1[li] = block_path(pl.m1[li], !training);
  }
  pl.path_pma = block_path(pl.pma, !training);
  if (!training) return pl;
  const bool d256 = c.d == 256;
  for (int li = 0; li < 2; ++li) {
    pl.isab128[li] = isab_bf16_supported(pl.m0[li], pl.m1[li]);
    pl.isab256[li] = pl.path_m0[li] == BlockPath::Mab0_256 && pl.path_m1[li] == BlockPath::Mab1_256;
    pl.img_m1[li] = pl.path_m1[li] == BlockPath::Mab1_256;      // (nk = 32: the only many-queries shape at d = 256)
    pl.img_m0[li] = pl.path_m0[li] == BlockPath::Mab0_256 && pl.m0[li].dk == 256;
  }
  pl.img256 = d256 && (c.mode == PCA_MODE_BF16 || c.mode == PCA_MODE_FP8);
  pl.img256_f8 = d256 && c.mode == PCA_MODE_FP8;
  pl.prep256 = pl.path_m0[0] == BlockPath::Mab0_256 && pl.path_m0[1] == BlockPath::Mab0_256 &&
               pl.path_pma == BlockPath::Mab0_256;
  pl.pma_head = pl.path_pma == BlockPath::Mab0_128;
  pl.pma256 = pl.path_pma == BlockPath::Mab0_256;
  pl.fq_defer[0] = pl.path_m0[0] == BlockPath::Mab0_256;
  pl.fq_defer[1] = pl.armed[1] = pl.isab256[1];      // (enc.0's mab1 reads the fp32 set: nothing to hand over)
  pl.defer_wg = pl.isab256[0] && pl.isab256[1] && pl.pma256;
  pl.set128_room = set128_shape_ok(c.B, c.N, c.din, c.d, c.h, c.m, c.k);
  // the set-resident forward takes a step whose blocks are all on the fused d = 128 kernels and whose sets fit
  // one workgroup's LDS - dense sets or padded ones with `lengths` (it masks the padding itself)
  pl.set128 = env_not_zero("PCA_SET128") && c.mode == PCA_MODE_BF16 && pl.act_bf16 && pl.set128_room &&
              pl.isab128[0] && pl.isab128[1] && pl.pma_head;
  pl.fuse_head = pl.set128 && c.C <= 64 && env_not_zero("PCA_SET128_HEAD");
  pl.pma_bwd = pl.fuse_head && env_not_zero("PCA_SET128_PMABWD");
  pl.tail = tail_form_from_env();
  return pl;
}

// Whether two identical training calls of this configuration give identical bits - logits, loss, statistics and
// every gradient, launched eagerly or replayed from a graph.  Conservative: true only in PCA_MODE_BF16 and only
// for the plans whose every reduction runs in a fixed order,
//   d = 128, all blocks on the fused kernels, the tail's reductions as slabs (TailForm::slabs), dense sets,
//          din <= 3: at din 4 layer 1's fc_q gradient leaves the chain kernel for k_wgrad_small's fp32 atomics
//          (mab1_bwd_bf16.hip; measured on delta sets: a captured and an eager run part ways);
//   d = 256, all blocks on the fused kernels, dense sets;
//   d = 64: the bf16-operand chain with every block's attention on the fused core and every
//          weight gradient on wgrad64 (slabs + fixed-order sums); the sum over sets of a shared query's
//          gradient is colsum()'s one-thread-per-column form up to 256 sets only, so B <= 256.
// The exact fp32 mode (split-K GEMMs add with atomics) and every other chain width: false.  Buffers are taken to
// be 16-byte aligned, as the engine's own are: the chain leaves a misaligned tensor to the split-K GEMM.
inline bool step_reproducible(const pca_st_config& c, bool has_lengths) {
  static const int32_t some_lengths = 1;      // (plan() and block_path() look at the pointer only)
  if (c.mode != PCA_MODE_BF16 || c.k != 1) return false;      // (the fp8 mode: nobody has asserted it yet)
  const StepPlan pl = plan(c, true, has_lengths ? &some_lengths : nullptr);
  if (pl.isab128[0] && pl.isab128[1] && pl.pma_head) return pl.tail.slabs && !has_lengths && c.din <= 3;
  if (pl.isab256[0] && pl.isab256[1] && pl.pma256) return !has_lengths;
  if (c.d != 64 || c.B > 256 || !(c.din == 64 || (c.din >= 1 && c.din <= 4)))
    return false;
  const pca_mab_shape* blocks[5] = {&pl.m0[0], &pl.m1[0], &pl.m0[1], &pl.m1[1], &pl.pma};
  const BlockPath path[5] = {pl.path_m0[0], pl.path_m1[0], pl.path_m0[1], pl.path_m1[1], pl.path_pma};
  for (int i = 0; i < 5; ++i)
    if (path[i] != BlockPath::Exact || !attn_core_ok(*blocks[i])) return false;
  return true;
}

struct Ws {
  void* saved[5];            // mab0[0], mab1[0], mab0[1], mab1[1], pma
  float *H[2], *Y[2], *P, *logits, *dlogits;
  float *dP, *dY2, *dY1, *dH, *clsws;
  void* scratch;             // forward + PMA backward
  size_t scratch_bytes;
  void* scratch_bw[2];       // backward of enc.0 / enc.1: separate, because the deferred reductions and
                             // post stages read each block's operands at the end of the step
                             // (bwd_defer_flush), after the other layer's backward has run
  void* scratch_pma;         // d = 256: the PMA's backward workspace, kept until the deferred post
                             // stages of all three few-queries blocks have run (else = scratch)
  void* scratch_fq[2];       // backward of the layer's few-queries block (else = scratch_bw[li]).  d = 256, enc.0:
                             // room of its own when its ISAB partner's [B*m]-row operands in scratch_bw[0] stay
                             // in place until the deferred launch; enc.1, hand-over form: the forward / PMA
                             // scratch, which is free by then
  IsabImg img[2];            // weight images of the two ISABs (fused bf16 path)
  float* wg_slabs;           // weight-gradient partials of the deferred reductions (fused d = 128)
  size_t wg_slab_bytes;
  __bf16* img256;            // d = 256: 24 weight images [256][256] prepared in one launch per step
  uint8_t* img256f8;         // d = 256, fp8 mode: e4m3 weight images of the step (one launch) ...
  float* inv256f8;           // ... and their inverse scales
  void* wg256_def;           // d = 256: slabs of the deferred [B*m]-row weight-gradient launch
  void* set128_ws;           // set-resident forward: pair flags + hand-off slots (its fused head writes the
                             // PMA's backward operands into `scratch` while other pairs still exchange)
};

inline size_t carve(const pca_st_config& c, const StepPlan& pl, Ws* out, void* base) {
  Carver cv(base);
  Ws w{};
  const pca_mab_shape* order[5] = {&pl.m0[0], &pl.m1[0], &pl.m0[1], &pl.m1[1], &pl.pma};
  const BlockPath path[5] = {pl.path_m0[0], pl.path_m1[0], pl.path_m0[1], pl.path_m1[1], pl.path_pma};
  size_t max_scratch = 0;
  for (int i = 0; i < 5; ++i) {
    // (one scratch size for both kinds of call: the inference path's block and the training one's)
    const size_t fb = mab_fwd_ws_bytes(block_path(*order[i], true), block_path(*order[i], false), *order[i]);
    max_scratch = fb > max_scratch ? fb : max_scratch;
    if (pl.training) {
      const size_t bb = mab_bwd_ws_bytes(path[i], *order[i]);
      max_scratch = bb > max_scratch ? bb : max_scratch;
      w.saved[i] = cv.take<char>(mab_saved_bytes(path[i], *order[i]));
    }
  }
  for (int li = 0; li < 2; ++li) {
    if (pl.isab128[li]) {
      const size_t fb = isab_bf16_fwd_ws_bytes(pl.m0[li], pl.m1[li]);
      const size_t bb = isab_bf16_bwd_ws_bytes(pl.m0[li], pl.m1[li]);
      max_scratch = fb > max_scratch ? fb : max_scratch;
      max_scratch = bb > max_scratch ? bb : max_scratch;
      char* ib = cv.take<char>(isab_img_bytes());
      if (base != nullptr) isab_img_carve(ib, &w.img[li]);
    }
  }
  if (pl.set128_room) w.set128_ws = cv.take<char>(set128_fwd_ws_bytes(c.B));   // (on the shape, not the switch)
  const size_t BN = (size_t)c.B * c.N, Bm = (size_t)c.B * c.m;
  w.H[0] = cv.take<float>(Bm * c.d);
  w.H[1] = cv.take<float>(Bm * c.d);
  w.Y[0] = cv.take<float>(BN * c.d);
  w.Y[1] = cv.take<float>(BN * c.d);
  w.P = cv.take<float>((size_t)c.B * c.k * c.d);
  w.logits = cv.take<float>((size_t)c.B * c.k * c.C);
  if (pl.training) {
    w.dlogits = cv.take<float>((size_t)c.B * c.k * c.C);
    w.dP = cv.take<float>((size_t)c.B * c.k * c.d);
    w.dY2 = cv.take<float>(BN * c.d);
    w.dY1 = cv.take<float>(BN * c.d);
    w.dH = cv.take<float>(Bm * c.d);
    w.clsws = cv.take<float>(2 * (size_t)c.B);
  }
  w.scratch = cv.take<char>(max_scratch);
  w.scratch_bytes = max_scratch;
  for (int li = 0; li < 2; ++li)
    w.scratch_bw[li] = pl.training ? (void*)cv.take<char>(max_scratch) : w.scratch;
  w.scratch_pma = pl.pma256 ? (void*)cv.take<char>(mab_bwd_ws_bytes(pl.path_pma, pl.pma)) : w.scratch;
  if ((pl.isab128[0] || pl.isab128[1]) && pl.tail.slabs) {
    // two lists (B*N-row and B*m-row jobs) of up to ~600 [128 x 128 (+128)] fp32 slabs each;
    // plan_tail gives a workgroup more rows when a list would not fit
    constexpr int slab_mb = 40;
    w.wg_slab_bytes = 2 * (size_t)slab_mb * 1024 * 1024;
    w.wg_slabs = cv.take<float>(w.wg_slab_bytes / sizeof(float));
  }
  if (pl.img256) w.img256 = cv.take<__bf16>((size_t)24 * 256 * 256);
  if (pl.img256_f8) {
    w.img256f8 = cv.take<uint8_t>((size_t)8 * 256 * 256);
    w.inv256f8 = cv.take<float>(16);
  }
  w.scratch_fq[0] = w.scratch_bw[0];
  w.scratch_fq[1] = pl.isab256[1] ? w.scratch : w.scratch_bw[1];
  if (pl.isab256[0]) {
    w.wg256_def = cv.take<char>(wgrad256_ws_bytes(8, (int64_t)c.B * c.m));
    void* own = cv.take<char>(mab_bwd_ws_bytes(pl.path_m0[0], pl.m0[0]));
    if (pl.defer_wg) w.scratch_fq[0] = own;
  }
  if (out) *out = w;
  return cv.off;
}

// Every bf16 weight image the d = 256 blocks of a training step ask for (weight_image1 / 2 in
// mab1_bf16.hip, d256_host.hip), registered in `tab`; launch != 0 also converts them: the bf16 image jobs
// go to `jobs`, which the caller launches together with the step's other preparation work (prepare_step),
// the fp8 ones run here.  A request this list does not foresee is converted on the spot by the block itself.
inline int images256_prepare(const Layout& L, const StepPlan& pl, const float* p, const Ws& w,
                             WeightImages* tab, bool launch, hipStream_t st, PrepJobs* jobs) {
  tab->n = 0;
  if (!pl.img256) return PCA_OK;
  PrepJobs J{};
  auto add = [&](const float* src, int mode) {
    if (tab->n >= 24) return;
    __bf16* img = w.img256 + (size_t)tab->n * 256 * 256;
    tab->e[tab->n++] = WeightImages::E{src, mode, 256, 256, img};
    J.j[J.n++] = PrepJob{src, img, 256, 256, mode};
  };
  for (int li = 0; li < 2; ++li) {
    if (pl.img_m1[li]) {
      const pca_mab_params pm = params_at(p, L.mab1[li]);
      const bool small = pl.m1[li].dq <= 4;
      add(pm.wo, mab1_fwd_wo_mode(pl.m1[li]));                // forward: fc_o (and fc_q of a d -> d block)
      if (!small) add(pm.wq, 0);
      add(pm.wo, D256_BWD_WMODE);                             // backward
      if (!small) add(pm.wq, D256_BWD_WMODE);
    }
    if (pl.img_m0[li]) {
      const pca_mab_params pk = params_at(p, L.mab0[li]);
      add(pk.wk, 0); add(pk.wv, 0);                          // forward: fc_k / fc_v over the keys
      add(pk.wk, D256_BWD_WMODE); add(pk.wv, D256_BWD_WMODE);
    }
  }
  // fp8 mode: the e4m3 images of the forward projections (fc_o of the many-queries blocks, fc_k / fc_v of
  // the d -> d few-queries block; natural layout: a block that wants another one converts its own)
  PrepF8Jobs F{};
  tab->nf8 = 0;
  if (pl.img256_f8) {
    auto add8 = [&](const float* src, int slot) {       // slot: index of the inverse scale
      if (tab->nf8 >= 8) return;
      const WeightImages::F8 e{src, 0, 256, 256, w.img256f8 + (size_t)tab->nf8 * 256 * 256,
                               w.inv256f8 + slot};
      tab->f8[tab->nf8++] = e;
      F.j[F.n++] = e;
    };
    for (int li = 0; li < 2; ++li) {
      if (pl.img_m1[li]) add8(params_at(p, L.mab1[li]).wo, 4 * li + 1);   // [., o]
      if (pl.img_m0[li]) {
        add8(params_at(p, L.mab0[li]).wk, 4 * li + 2);                   // [k, v]: adjacent
        add8(params_at(p, L.mab0[li]).wv, 4 * li + 3);
      }
    }
  }
  if (!launch) return PCA_OK;
  *jobs = J;
  return prep_f8_jobs_launch(F, st);
}

int validate(const pca_st_config* c) {
  PCA_REQUIRE(c != nullptr, "st: null config");
  PCA_REQUIRE(c->B > 0 && c->N > 0 && c->din > 0 && c->d > 0 && c->h > 0 && c->m > 0 &&
                  c->k > 0 && c->C > 0,
              "st: non-positive extent");
  PCA_REQUIRE(c->d % c->h == 0, "st: d=%d not divisible by h=%d", c->d, c->h);
  PCA_REQUIRE(c->mode == PCA_MODE_F32 || c->mode == PCA_MODE_BF16 || c->mode == PCA_MODE_FP8,
              "st: unknown mode %d",
              c->mode);
  return PCA_OK;
}

// The preparation of a training step in ONE launch: all weight images (`J` arrives with the d = 256 image
// table's jobs, images256_prepare), the flag clear of the set-resident forward and the query side (Qp, G
// images) of every fused mab0 / PMA.  (takes a deferred pack along: pca_pack_defer)
int prepare_step(const pca_st_config& c, const Layout& L, const StepPlan& pl, const float* p, const Ws& w,
                 PrepJobs J, hipStream_t st) {
  Mab0PrepJobs MJ{};
  for (int li = 0; li < 2; ++li)
    if (pl.isab128[li]) {
      isab_collect_prep(pl.m0[li], params_at(p, L.mab0[li]), params_at(p, L.mab1[li]), w.img[li], true,
                        li == 1, &J);
      Mab0Saved v;
      mab0_carve_saved(pl.m0[li], &v, w.saved[2 * li]);
      mab0_collect_prep(pl.m0[li], p + L.I[li], params_at(p, L.mab0[li]), v, true, false, &MJ);
    }
  if (pl.set128)                 // the pair flags of the set-resident forward start every step at zero
    // (not the 16-byte header in front of them: word 0 counts expired spin-waits and is the CALLER's to
    // clear and read - pca_st_handoff_counter)
    J.j[J.n++] = PrepJob{nullptr, reinterpret_cast<__bf16*>(static_cast<char*>(w.set128_ws) + 16), 1,
                         (int)((set128_flag_bytes(c.B) - 16) / 2), 4};
  if (pl.pma_head) {
    Mab0Saved v;
    mab0_carve_saved(pl.pma, &v, w.saved[4]);
    mab0_collect_prep(pl.pma, p + L.S, params_at(p, L.pma), v, true, true, &MJ);
  }
  if (pl.prep256) {              // (mab0_d256_prep_collect; the blocks' forward calls take PCA_F_PREP_DONE)
    const pca_mab_shape* sh[3] = {&pl.m0[0], &pl.m0[1], &pl.pma};
    const float* Iq[3] = {p + L.I[0], p + L.I[1], p + L.S};
    const pca_mab_params pr[3] = {params_at(p, L.mab0[0]), params_at(p, L.mab0[1]),
                                  params_at(p, L.pma)};
    void* sv[3] = {w.saved[0], w.saved[2], w.saved[4]};
    mab0_d256_prep_collect(3, sh, Iq, pr, sv, &MJ);
  }
  return prep_all_launch(J, MJ, st);
}

// arguments of the set-resident forward: both ISABs and the PMA's attention partials, the set resident in
// one workgroup's LDS; `head`: the stages it runs in its tail when the plan says so
Set128FwdArgs set128_args(const pca_st_config& c, const Layout& L, const StepPlan& pl, const float* p,
                          const float* X, const Ws& w, const PmaHeadArgs& head) {
  Set128FwdArgs a{};
  a.X = X; a.B = c.B; a.N = c.N; a.din = c.din;
  a.lengths = pl.pma.k_lengths;          // (plan(): the call's `lengths`, the keys of all three attentions)
  a.scale_log2e = LOG2E / sqrtf((float)c.d);
  for (int li = 0; li < 2; ++li) {
    Mab0Saved v0;
    mab0_carve_saved(pl.m0[li], &v0, w.saved[2 * li]);
    Mab1Saved v1;
    mab1_carve_saved(pl.m1[li], &v1, w.saved[2 * li + 1]);
    const pca_mab_params p0 = params_at(p, L.mab0[li]), p1 = params_at(p, L.mab1[li]);
    const IsabImg& im = w.img[li];
    Set128Layer& S = a.L[li];
    S.Gf = v0.Gf; S.Gb = v0.Gb; S.Qp0 = v0.Qp; S.Wv0 = im.Wv0; S.Wv0f = p0.wv; S.bv0 = p0.bv;
    S.bo0 = p0.bo; S.Wo0 = im.Wo0; S.T = v0.T; S.LSE = v0.LSE; S.O0 = v0.O; S.Z0 = v0.Z; S.H = w.H[li];
    S.Wk1 = im.Wk1; S.Wv1 = im.Wv1; S.bk1 = p1.bk; S.bv1 = p1.bv;
    S.KpP = v1.KpP; S.VpP = v1.VpP; S.Kt = v1.Kt; S.Vt = v1.Vt;
    S.WqB = im.WqB; S.WqF = p1.wq; S.bq1 = p1.bq; S.WoP = im.WoP; S.bo1 = p1.bo;
    S.QpS = v1.QpS; S.OS = v1.OS; S.Y = reinterpret_cast<__bf16*>(w.Y[li]); S.mask = v1.mask;
  }
  if (pl.pma_bwd) {              // the PMA's attention backward in the tail: Y2 has no reader left
    a.pma_bwd = 1;
    a.dY2 = reinterpret_cast<__bf16*>(w.dY2);
    Mab0BwdWs wb;
    mab0_carve_bwd_ws(pl.pma, &wb, w.scratch);
    a.pma_slabs = wb.slabs;
    a.pma_S = mab0_bwd_splits(pl.pma);
    a.L[1].Y = nullptr;
  }
  Carver cs(w.set128_ws);
  a.flags = reinterpret_cast<uint32_t*>(cs.take<char>(set128_flag_bytes(c.B)));   // (cleared by k_prep_all)
  a.ex2 = cs.take<float>((size_t)c.B * 2 * 9216);
  a.exP = cs.take<float>((size_t)c.B * 2 * 528);
  if (pl.fuse_head) {            // the PMA epilogue, the classifier and the loss in the same launch
    a.fuse_head = 1;
    a.head = head;
  }
  Mab0Saved vp;
  mab0_carve_saved(pl.pma, &vp, w.saved[4]);
  a.Gpma = vp.Gb; a.TpP = vp.Tp; a.MpP = vp.Mp; a.LpP = vp.Lp; a.Sp = mab0_splits(pl.pma);
  return a;
}

// `head`: the train step's head arguments (pma_head_args; read only by the set-resident launch), null in inference
int forward(const pca_st_config& c, const Layout& L, const StepPlan& pl, const float* p, const float* X,
            const Ws& w, hipStream_t st, StepCtx* ctx, const PmaHeadArgs* head = nullptr) {
  PCA_TRY(pack_flush(st));                  // a deferred pack nobody took runs now, before X is read
  if (pl.set128) {
    PCA_REQUIRE(head != nullptr, "st: the set-resident forward needs the head arguments");
    return set128_fwd_launch(set128_args(c, L, pl, p, X, w, *head), st);
  }
  const void* in = X;
  const int prep_flag = pl.prep256 ? PCA_F_PREP_DONE : 0;
  for (int li = 0; li < 2; ++li) {
    void* sv0 = pl.training ? w.saved[2 * li] : nullptr;
    void* sv1 = pl.training ? w.saved[2 * li + 1] : nullptr;
    if (pl.isab128[li]) {
      PCA_TRY(isab_bf16_fwd(pl.m0[li], pl.m1[li], p + L.I[li], in, params_at(p, L.mab0[li]),
                            params_at(p, L.mab1[li]), w.H[li], w.Y[li], sv0, sv1, w.scratch,
                            w.img[li], st));
      in = w.Y[li];
      continue;
    }
    // d = 256 training: the few-queries block ends in the per-set mid kernel, which also prepares
    // the K / V images of the many-queries block (mid256.hip; the blocks' saved areas are disjoint)
    const pca_mab_params p1 = params_at(p, L.mab1[li]);
    ctx->mid_done = false;
    if (pl.isab256[li]) { ctx->s1 = pl.m1[li]; ctx->p1 = p1; ctx->saved1 = sv1; }
    PCA_TRY(mab_fwd(pl.path_m0[li], pl.m0[li], p + L.I[li], in, params_at(p, L.mab0[li]), w.H[li], sv0, w.scratch,
                        st, prep_flag, ctx));                       // modules.py:52
    ctx->saved1 = nullptr;
    PCA_TRY(mab_fwd(pl.path_m1[li], pl.m1[li], in, w.H[li], p1, w.Y[li], sv1, w.scratch, st,
                        ctx->mid_done ? PCA_F_KV_READY : 0, ctx));  // modules.py:53
    in = w.Y[li];
  }
  if (pl.pma_head)                                                        // modules.py:63
    // (its epilogue runs inside k_pma_head together with the classifier and the loss)
    PCA_TRY(mab0_bf16_fwd_ex(pl.pma, p + L.S, w.Y[1], params_at(p, L.pma), w.P, w.saved[4],
                             w.scratch, PCA_F_PREP_DONE | (c.k == 1 ? PCA_F_SKIP_EPILOGUE : 0),
                             st));
  else
    PCA_TRY(mab_fwd(pl.path_pma, pl.pma, p + L.S, w.Y[1], params_at(p, L.pma), w.P,
                        pl.training ? w.saved[4] : nullptr, w.scratch, st, prep_flag, ctx));
  if (!pl.training)
    PCA_TRY(linear_fwd_f32(w.P, p + L.wc, p + L.bc, w.logits, (int64_t)c.B * c.k, c.d, c.C,
                           st));                                    // models.py:40
  return PCA_OK;
}

// a block queues its terminal reductions in `posts` when its call is given deferring(.., true), and launches
// them itself otherwise
inline StepCtx* deferring(StepCtx* ctx, BwdDefer* posts, bool on) {
  ctx->defer = on ? posts : nullptr;
  return ctx;
}

// Backward of enc.<li>: mab1(X, H) then mab0(I, X).  X feeds both blocks, so its gradient dX is written by
// the first and accumulated by the second (null: X is the input set, which needs no gradient).
int isab_bwd(int li, const Layout& L, const StepPlan& pl, const float* p, float* g, const void* X,
             const void* dY, void* dX, const Ws& w, BwdDefer* posts, StepCtx* ctx, hipStream_t st) {
  const pca_mab_params p0 = params_at(p, L.mab0[li]), p1 = params_at(p, L.mab1[li]);
  const pca_mab_grads g0 = grads_at(g, L.mab0[li]), g1 = grads_at(g, L.mab1[li]);
  if (pl.isab128[li])
    return isab_bf16_bwd(pl.m0[li], pl.m1[li], p + L.I[li], X, w.H[li], p0, p1, w.saved[2 * li],
                         w.saved[2 * li + 1], dY, g + L.I[li], dX, g0, g1, w.scratch_bw[li], w.img[li], st,
                         posts);
  ctx->armed = pl.armed[li];
  PCA_TRY(mab_bwd(pl.path_m1[li], pl.m1[li], X, w.H[li], p1, w.saved[2 * li + 1], dY, dX, w.dH, 0, g1, w.scratch_bw[li],
                      st, deferring(ctx, posts, pl.defer_wg)));
  PCA_TRY(mab_bwd(pl.path_m0[li], pl.m0[li], p + L.I[li], X, p0, w.saved[2 * li], w.dH, g + L.I[li], dX, dX != nullptr,
                      g0, w.scratch_fq[li], st, deferring(ctx, posts, pl.fq_defer[li])));
  ctx->armed = false;
  return wgrad256_handoff_flush(ctx, w.scratch, st);   // (what nobody took runs on its own; not armed: nothing)
}

int st_forward(const pca_st_config* c, const float* params, const float* X, const int32_t* lengths,
               float* logits, void* ws, void* stream) {
  PCA_TRY(validate(c));
  PCA_REQUIRE(params && X && logits && ws, "st_forward: null pointer");
  const StepPlan pl = plan(*c, false, lengths);
  Ws w;
  carve(*c, pl, &w, ws);
  w.logits = logits;
  StepCtx ctx{};
  return forward(*c, layout(*c), pl, params, X, w, as_stream(stream), &ctx);
}

// The attention scratch behind the inference workspace: pma_attention's own block and a home for the scores
// when the caller wants the key alone.
struct AttnWs {
  void* pa;
  float* attn;
};
inline size_t carve_attn(const pca_st_config& c, const StepPlan& pl, AttnWs* out, void* base) {
  Carver cv(base);
  AttnWs a{};
  a.pa = cv.take<char>(pma_attention_ws_bytes(pl.pma));
  a.attn = cv.take<float>((size_t)c.B * c.k * c.h * c.N);
  if (out) *out = a;
  return cv.off;
}
int attn_config_ok(const pca_st_config* c) {
  PCA_REQUIRE(c->d <= 256, "st_pool_attention: d=%d (max 256)", c->d);
  return PCA_OK;
}

int st_pool_attention(const pca_st_config* c, const float* params, const float* X, const int32_t* lengths,
                      float* logits, float* attn, float* key, void* ws, void* stream) {
  PCA_TRY(validate(c));
  PCA_TRY(attn_config_ok(c));
  PCA_REQUIRE(params && X && logits && ws, "st_pool_attention: null pointer");
  const StepPlan pl = plan(*c, false, lengths);
  // Y2 = w.Y[1] must be the complete fp32 [B, N, d] output of enc.1: an inference plan keeps every
  // activation in fp32 (act_bf16 and the set-resident launch belong to training plans) and each path of the
  // many-queries block (Mab1_128 / Mab1_256 / Sd64 / Exact) writes all B N rows of its Y.
  if (pl.act_bf16 || pl.set128 || pl.m1[1].y_dtype != PCA_F32 || pl.pma.k_dtype != PCA_F32) {
    set_error("st_pool_attention: this configuration's forward does not leave enc.1's output in fp32");
    return PCA_EUNSUPPORTED;
  }
  Ws w;
  const size_t fwd_bytes = carve(*c, pl, &w, ws);
  w.logits = logits;
  StepCtx ctx{};
  const Layout L = layout(*c);
  PCA_TRY(forward(*c, L, pl, params, X, w, as_stream(stream), &ctx));
  if (attn == nullptr && key == nullptr) return PCA_OK;
  AttnWs a;
  carve_attn(*c, pl, &a, static_cast<char*>(ws) + fwd_bytes);
  return pma_attention(pl.pma, params + L.S, w.Y[1], params_at(params, L.pma), attn != nullptr ? attn : a.attn,
                       key, a.pa, as_stream(stream));
}

int st_train_fwd_bwd(const pca_st_config* c, const float* p, const float* X, const int32_t* lengths,
                     const int64_t* labels, const PcaSoftTargets* soft_in, float* g, float* loss_out,
                     float* stats, float* logits, float grad_scale, int phase, void* ws, void* stream) {
  PCA_TRY(validate(c));
  SoftTargets soft;
  PCA_TRY(soft_targets_from(soft_in, "st_train_fwd_bwd", &soft));
  PCA_REQUIRE(p && X && labels && g && loss_out && ws, "st_train_fwd_bwd: null pointer");
  PCA_REQUIRE(c->k == 1, "st_train_fwd_bwd: the train step needs k == 1 (got %d)", c->k);
  PCA_REQUIRE(phase >= -1 && phase <= 1, "st_train_fwd_bwd: phase=%d", phase);
  // the classifier head (cls_fwd_bwd_body) keeps a set's pooled features and its logits in LDS
  PCA_REQUIRE((int64_t)c->d + c->C <= 16368,
              "st_train_fwd_bwd: d + C = %lld floats do not fit the classifier head's LDS (max 16368)",
              (long long)((int64_t)c->d + c->C));
  hipStream_t st = as_stream(stream);
  const StepPlan pl = plan(*c, true, lengths);
  Ws w;
  carve(*c, pl, &w, ws);
  const Layout L = layout(*c);
  if (logits != nullptr) w.logits = logits;
  // shared-query gradients of the fused blocks of this call: one pair of launches at the end
  // (their inputs live in per-block workspaces, which stay untouched until then)
  BwdDefer posts{};
  posts.slab_ws = w.wg_slabs;
  posts.slab_cap = w.wg_slab_bytes;
  posts.form = pl.tail;
  if (pl.defer_wg) posts.wg256_ws = w.wg256_def;
  // d = 256: all weight images of the step in one launch (phase 1 of a split step finds the images
  // of phase 0 still in place: the parameters do not change in between)
  WeightImages images{};
  PrepJobs image_jobs{};
  PCA_TRY(images256_prepare(L, pl, p, w, &images, phase != 1, st, &image_jobs));
  // what this call hands from block to block (StepCtx)
  StepCtx ctx{};
  ctx.images = images.n > 0 ? &images : nullptr;
  if (c->mode != PCA_MODE_F32 && c->d == 64 && pl.path_pma == BlockPath::Exact) {
    // the d = 64 chain: after the PMA's backward nothing of this call uses `scratch`, so the ISAB blocks leave
    // their weight-gradient slabs behind the PMA's area and the sums ride in the terminal launch (D.late)
    const size_t used = align256(mab_bwd_ws_bytes(pl.path_pma, pl.pma));
    if (used < w.scratch_bytes) {
      ctx.wg64_late = &posts.late;
      ctx.wg64_room = reinterpret_cast<float*>(static_cast<char*>(w.scratch) + used);
      ctx.wg64_room_elems = (w.scratch_bytes - used) / sizeof(float);
    }
  }
  if (phase != 1) {
    PmaHeadArgs head{};
    if (pl.pma_head)
      PCA_TRY(pma_head_args(pl.pma, params_at(p, L.pma), w.saved[4], w.scratch, w.P, p + L.wc, p + L.bc,
                            labels, soft, c->C, grad_scale, w.logits, w.dlogits, w.dP, g + L.wc, g + L.bc,
                            loss_out, stats, w.clsws, &posts, &head));
    PCA_TRY(prepare_step(*c, L, pl, p, w, image_jobs, st));
    PCA_TRY(forward(*c, L, pl, p, X, w, st, &ctx, &head));
    if (pl.pma_head) {
      // dec.0 epilogue + dec.1 (Linear) + mean cross-entropy forward and backward + dec.0
      // backward epilogue: one launch, one workgroup per set - or the tail of the set-resident forward
      if (!pl.fuse_head) PCA_TRY(pma_head_launch(head, st));
      PCA_TRY(mab0_bf16_bwd_ex(pl.pma, p + L.S, w.Y[1], params_at(p, L.pma), w.saved[4], w.dP, g + L.S,
                               w.dY2, 0, grads_at(g, L.pma), w.scratch,
                               PCA_F_SKIP_HEAD | (pl.pma_bwd ? PCA_F_ATTN_DONE : 0), st,
                               deferring(&ctx, &posts, true)));
    } else {
      // dec.1 (Linear) + mean cross-entropy, forward and backward
      PCA_TRY(cls_train_head(w.P, p + L.wc, p + L.bc, labels, soft, c->B, c->d, c->C, grad_scale, w.logits,
                             w.dlogits, w.dP, g + L.wc, g + L.bc, loss_out, stats, w.clsws, st, &posts));
      PCA_TRY(mab_bwd(pl.path_pma, pl.pma, p + L.S, w.Y[1], params_at(p, L.pma), w.saved[4], w.dP, g + L.S, w.dY2,
                          0, grads_at(g, L.pma), w.scratch_pma, st, deferring(&ctx, &posts, pl.pma256)));
    }
    PCA_TRY(isab_bwd(1, L, pl, p, g, w.Y[0], w.dY2, w.dY1, w, &posts, &ctx, st));
  }
  if (phase != 0) PCA_TRY(isab_bwd(0, L, pl, p, g, X, w.dY1, nullptr, w, &posts, &ctx, st));
  return bwd_defer_flush(posts, st);
}

}  // namespace
}  // namespace pca

extern "C" {

int64_t pca_st_param_count(const pca_st_config* c) {
  if (pca::validate(c) != PCA_OK) return -1;
  return pca::layout(*c).total;
}

int64_t pca_st_bucket_split(const pca_st_config* c) {
  if (pca::validate(c) != PCA_OK) return -1;
  return pca::layout(*c).enc1_begin;
}

int pca_st_step_reproducible(const pca_st_config* c, int has_lengths) {
  if (pca::validate(c) != PCA_OK) return 0;
  return pca::step_reproducible(*c, has_lengths != 0) ? 1 : 0;
}

size_t pca_st_ws_bytes(const pca_st_config* c, int training) {
  if (pca::validate(c) != PCA_OK) return 0;
  return pca::carve(*c, pca::plan(*c, training != 0, nullptr), nullptr, nullptr);
}

int pca_st_handoff_counter(const pca_st_config* c, void* ws, uint32_t** counter) {
  PCA_TRY(pca::validate(c));
  PCA_REQUIRE(ws != nullptr && counter != nullptr, "st_handoff_counter: null pointer");
  pca::Ws w;
  pca::carve(*c, pca::plan(*c, true, nullptr), &w, ws);
  *counter = static_cast<uint32_t*>(w.set128_ws);      // nullptr: no set-resident launch for this shape
  return PCA_OK;
}

int pca_st_ws_layout(const pca_st_config* c, int64_t* out) {
  PCA_TRY(pca::validate(c));
  PCA_REQUIRE(out != nullptr, "st_ws_layout: null pointer");
  pca::Ws w;
  char* const base = reinterpret_cast<char*>(256);      // (never dereferenced: offsets only)
  const size_t total = pca::carve(*c, pca::plan(*c, true, nullptr), &w, base);
  for (int i = 0; i < 5; ++i) out[i] = reinterpret_cast<char*>(w.saved[i]) - base;
  for (int i = 0; i < 2; ++i) {
    out[5 + i] = reinterpret_cast<char*>(w.H[i]) - base;
    out[7 + i] = reinterpret_cast<char*>(w.Y[i]) - base;
  }
  out[9] = reinterpret_cast<char*>(w.scratch) - base;
  out[10] = (int64_t)total;
  return PCA_OK;
}

int pca_st_forward(const pca_st_config* c, const float* params, const float* X,
                   const int32_t* lengths, float* logits, void* ws, void* stream) {
  PCA_TRY(pca::no_stale_pack("pca_st_forward", true));
  const int rc = pca::st_forward(c, params, X, lengths, logits, ws, stream);
  return rc != PCA_OK ? rc : pca::no_stale_pack("pca_st_forward (exit)", false);
}

size_t pca_st_pool_attention_ws_bytes(const pca_st_config* c) {
  if (pca::validate(c) != PCA_OK || pca::attn_config_ok(c) != PCA_OK) return 0;
  const pca::StepPlan pl = pca::plan(*c, false, nullptr);
  return pca::carve(*c, pl, nullptr, nullptr) + pca::carve_attn(*c, pl, nullptr, nullptr);
}

int pca_st_pool_attention(const pca_st_config* c, const float* params, const float* X,
                          const int32_t* lengths, float* logits, float* attn, float* key,
                          void* ws, void* stream) {
  PCA_TRY(pca::no_stale_pack("pca_st_pool_attention", true));
  const int rc = pca::st_pool_attention(c, params, X, lengths, logits, attn, key, ws, stream);
  return rc != PCA_OK ? rc : pca::no_stale_pack("pca_st_pool_attention (exit)", false);
}

int pca_st_train_fwd_bwd_soft(const pca_st_config* c, const float* params, const float* X,
                              const int32_t* lengths, const int64_t* labels,
                              const PcaSoftTargets* soft, float* grads, float* loss_out, float* stats,
                              float* logits, float grad_scale, int phase, void* ws, void* stream) {
  // phase 1 of a split step reads X again: the pack was consumed by phase 0
  PCA_TRY(pca::no_stale_pack("pca_st_train_fwd_bwd", phase != 1));
  const int rc = pca::st_train_fwd_bwd(c, params, X, lengths, labels, soft, grads, loss_out, stats,
                                       logits, grad_scale, phase, ws, stream);
  return rc != PCA_OK ? rc : pca::no_stale_pack("pca_st_train_fwd_bwd (exit)", false);
}

int pca_st_train_fwd_bwd(const pca_st_config* c, const float* params, const float* X,
                         const int32_t* lengths, const int64_t* labels, float* grads,
                         float* loss_out, float* stats,
                         float* logits, float grad_scale, int phase, void* ws,
                         void* stream) {
  return pca_st_train_fwd_bwd_soft(c, params, X, lengths, labels, nullptr, grads, loss_out, stats,
                                   logits, grad_scale, phase, ws, stream);
}
}
