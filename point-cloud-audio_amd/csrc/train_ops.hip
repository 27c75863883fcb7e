// Loss of the train step (Code/settransformer.py:88,104-105): nn.CrossEntropyLoss (mean)
// forward+gradient in one launch, and the fused classifier head (the optimiser: optim.hip).  Also the
// correct-count tally of the evaluation sweeps (Code/pceval.py:95, (preds.argmax(dim=1) == lbls).sum()).
#include "blocks.hpp"
#include "bwd_defer.hpp"
#include "terminal_bodies.hpp"
#include "pma_head_bodies.hpp"
#include "soft_targets.hpp"

#include <cmath>

namespace pca {
namespace {

// One sample of the cross-entropy on one wave: writes the sample's row of dlogits, counts a correct
// argmax in stats[1] and returns the sample's loss (the value of lane 0 is the one to use).
__device__ __forceinline__ float ce_sample(const float* __restrict__ logits,
                                           const int64_t* __restrict__ labels, int b, int B, int C,
                                           float grad_scale, float* __restrict__ dlogits,
                                           float* __restrict__ stats, const SoftTargets& soft,
                                           int lane) {
  const float* x = logits + (int64_t)b * C;
  float m = -INFINITY;
  int am = 0x7fffffff;
  for (int j = lane; j < C; j += 64) {
    const float v = x[j];
    if (v > m) { m = v; am = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    if (om > m || (om == m && oa < am)) { m = om; am = oa; }
  }
  float s = 0.f;
  for (int j = lane; j < C; j += 64) s += expf(x[j] - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const SoftRow t = soft_row(soft, labels, b);
  float sx = 0.f;
  if (t.eps > 0.f) {             // (uniform) sum of the logits: only the smoothing term reads it
    for (int j = lane; j < C; j += 64) sx += x[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sx += __shfl_xor(sx, o, 64);
  }
  const float lse = m + logf(s);
  const float inv_s = 1.f / s;
  const float gs = grad_scale / (float)B;
  if (dlogits != nullptr)
    for (int j = lane; j < C; j += 64) {
      const float pj = expf(x[j] - m) * inv_s;
      dlogits[(int64_t)b * C + j] = (pj - soft_target(t, j, C)) * gs;
    }
  if (lane == 0 && stats != nullptr && am == (int)soft_dominant(t)) atomicAdd(&stats[1], 1.f);
  return lse - soft_picked(t, x[t.y1], x[t.y2], sx, C);
}

// one wave per sample, four samples per workgroup.  The workgroup adds its samples' losses before the
// division by B and before its ONE atomic per sum: the mean over B samples then carries B / 4 atomic
// roundings at the magnitude of the running sum instead of B (129 samples with losses near 100:
// ~2e-5 of drift, as much as the rounding of the log-sum-exp itself).
__global__ __launch_bounds__(256) void k_cross_entropy(const float* __restrict__ logits,
                                                        const int64_t* __restrict__ labels,
                                                        int B, int C, float grad_scale,
                                                        float* __restrict__ loss_out,
                                                        float* __restrict__ dlogits,
                                                        float* __restrict__ stats,
                                                        const SoftTargets soft) {
  __shared__ float wl[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wv;
  float li = 0.f;                // (a wave without a sample adds an exact zero)
  if (b < B) li = ce_sample(logits, labels, b, B, C, grad_scale, dlogits, stats, soft, lane);
  if (lane == 0) wl[wv] = li;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = (wl[0] + wl[1]) + (wl[2] + wl[3]);
    atomicAdd(loss_out, t / (float)B);
    if (stats != nullptr) atomicAdd(&stats[0], t);
  }
}

// torch.argmax order of two (value, index) candidates: NaN is the maximum, equal values (and two
// NaNs) go to the lower index
__device__ inline bool argmax_before(float a, int ia, float b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na != nb) return na;
  if (!na && a != b) return a > b;
  return ia < ib;
}

// one wave per sample: counts[slot] += #(argmax_c logits[b, c] == labels[b]); integer atomics, so the
// count does not depend on the order the waves finish in
__global__ __launch_bounds__(256) void k_eval_tally(const float* __restrict__ logits,
                                                     const int64_t* __restrict__ labels, int B,
                                                     int C, unsigned long long* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* x = logits + (int64_t)b * C;
  float m = -INFINITY;
  int am = 0x7fffffff;
  for (int j = lane; j < C; j += 64) {
    const float v = x[j];
    if (argmax_before(v, j, m, am)) { m = v; am = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    if (argmax_before(om, oa, m, am)) { m = om; am = oa; }
  }
  if (lane == 0 && (int64_t)am == labels[b]) atomicAdd(count, 1ull);
}

// ---------------------------------------------------------------------------------
// Fused classifier head of the train step (Code/models.py:40 + Code/settransformer.py:104):
//   k_cls_fwd_bwd  one 128-thread workgroup per sample: logits = P Wc^T + bc, softmax,
//                  per-sample loss / correctness, dlogits = (softmax - onehot) gs / B,
//                  dP = dlogits Wc
//   k_cls_wgrad    dWc += dlogits^T P, dbc += colsum(dlogits); block 0 also reduces the
//                  per-sample losses (deterministic sum) into loss_out and the counters
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void k_cls_fwd_bwd(
    const float* __restrict__ P, const float* __restrict__ Wc, const float* __restrict__ bc,
    const int64_t* __restrict__ labels, int B, int d, int C, float grad_scale,
    float* __restrict__ logits, float* __restrict__ dlogits, float* __restrict__ dP,
    float* __restrict__ lossv, float* __restrict__ corrv, const SoftTargets soft) {
  cls_fwd_bwd_body(P, Wc, bc, labels, soft, B, d, C, grad_scale, logits, dlogits, dP, lossv, corrv,
                   blockIdx.x);
}

__global__ __launch_bounds__(128) void k_cls_wgrad(
    const float* __restrict__ dlogits, const float* __restrict__ P,
    const float* __restrict__ lossv, const float* __restrict__ corrv, int B, int d, int C,
    float* __restrict__ dWc, float* __restrict__ dbc, float* __restrict__ loss_out,
    float* __restrict__ stats) {
  cls_wgrad_body(dlogits, P, lossv, corrv, B, d, C, dWc, dbc, loss_out, stats, blockIdx.x);
}

}  // namespace

// PcaSoftTargets of the C ABI -> the kernels' argument; NULL is the hard target.  The smoothing is the
// one host value among the targets: refused here, before anything is enqueued.
int soft_targets_from(const PcaSoftTargets* soft, const char* who, SoftTargets* out) {
  *out = SoftTargets{nullptr, nullptr, 0.f};
  if (soft == nullptr) return PCA_OK;
  PCA_REQUIRE(std::isfinite(soft->smoothing) && soft->smoothing >= 0.f && soft->smoothing < 1.f,
              "%s: smoothing=%g must be finite and in [0, 1)", who, (double)soft->smoothing);
  *out = SoftTargets{soft->labels2, soft->weight, soft->smoothing};
  return PCA_OK;
}

// classifier head of the train step; ws needs 2*B floats
int cls_train_head(const float* P, const float* Wc, const float* bc, const int64_t* labels,
                   const SoftTargets& soft, int B, int d, int C, float grad_scale, float* logits, float* dlogits,
                   float* dP, float* dWc, float* dbc, float* loss_out, float* stats, float* ws,
                   hipStream_t st, BwdDefer* defer) {
  float* lossv = ws;
  float* corrv = ws + B;
  hipLaunchKernelGGL(k_cls_fwd_bwd, dim3(B), dim3(128), (size_t)(d + C) * sizeof(float), st, P, Wc,
                     bc, labels, B, d, C, grad_scale, logits, dlogits, dP, lossv, corrv, soft);
  PCA_TRY(check_launch("k_cls_fwd_bwd"));
  if (defer != nullptr) {          // rides in the phase's terminal launch
    defer->cls = ClsWgradArgs{dlogits, P, lossv, corrv, B, d, C, dWc, dbc, loss_out, stats};
    defer->has_cls = 1;
    return PCA_OK;
  }
  hipLaunchKernelGGL(k_cls_wgrad, dim3(C), dim3(128), 0, st, dlogits, P, lossv, corrv, B, d, C,
                     dWc, dbc, loss_out, stats);
  return check_launch("k_cls_wgrad");
}

}  // namespace pca

extern "C" {

int pca_cross_entropy_soft(const float* logits, const int64_t* labels, const PcaSoftTargets* soft,
                           int B, int C, float grad_scale, float* loss_out, float* dlogits,
                           float* stats_out, void* stream) {
  PCA_REQUIRE(logits && labels && loss_out, "cross_entropy: null pointer");
  PCA_REQUIRE(B > 0 && C > 0, "cross_entropy: B=%d C=%d", B, C);
  pca::SoftTargets t{nullptr, nullptr, 0.f};
  PCA_TRY(pca::soft_targets_from(soft, "cross_entropy", &t));
  hipStream_t st = pca::as_stream(stream);
  PCA_TRY(pca::fill_zero(loss_out, 1, st));
  hipLaunchKernelGGL(pca::k_cross_entropy, dim3((unsigned)pca::cdiv(B, 4)), dim3(256), 0, st,
                     logits, labels, B, C, grad_scale, loss_out, dlogits, stats_out, t);
  return pca::check_launch("k_cross_entropy");
}

int pca_cross_entropy(const float* logits, const int64_t* labels, int B, int C,
                      float grad_scale, float* loss_out, float* dlogits, float* stats_out,
                      void* stream) {
  return pca_cross_entropy_soft(logits, labels, nullptr, B, C, grad_scale, loss_out, dlogits,
                                stats_out, stream);
}

int pca_eval_tally(const float* logits, const int64_t* labels, int B, int C, int64_t* counts,
                   int slot, void* stream) {
  PCA_REQUIRE(logits && labels && counts, "eval_tally: null pointer");
  PCA_REQUIRE(B > 0 && C > 0 && slot >= 0, "eval_tally: B=%d C=%d slot=%d", B, C, slot);
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counter width");
  hipLaunchKernelGGL(pca::k_eval_tally, dim3((unsigned)pca::cdiv(B, 4)), dim3(256), 0,
                     pca::as_stream(stream), logits, labels, B, C,
                     reinterpret_cast<unsigned long long*>(counts + slot));
  return pca::check_launch("k_eval_tally");
}
}
