// Soft targets of the cross-entropy: a set carries two classes y1 / y2, the weight w of the first and a
// label smoothing eps shared by the batch (between-class learning / mixup on two labelled clips):
//   t_c  = (1 - eps) (w [c == y1] + (1 - w) [c == y2]) + eps / C
//   loss = logsumexp(x) - sum_c t_c x_c = lse - (1 - eps) (w x[y1] + (1 - w) x[y2]) - (eps / C) sum_c x_c
//   dx_c = (softmax(x)_c - t_c) grad_scale / B
// One statement of that arithmetic for the four loss sites (k_cross_entropy, cls_fwd_bwd_body,
// k_pma_head1, the head stages of k_set128_fwd).  A hard label is the value w = 1, eps = 0 of the same
// expressions: 1 * a + 0 * b + 0 is a for finite a, b, so t_c is exactly [c == y1], the picked term is
// exactly x[y1] and the sites compute the hard loss's bits without a second code path.  sum_c x_c is
// only reduced (and only read here) when eps > 0: a uniform branch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pca {

// labels2 == nullptr: y2 = y1; weight == nullptr: w = 1.  Device values, not validated (as labels).
struct SoftTargets {
  const int64_t* labels2;
  const float* weight;
  float smoothing;
};

// the targets of one set
struct SoftRow {
  int64_t y1, y2;
  float w, eps;
};

__device__ __forceinline__ SoftRow soft_row(const SoftTargets& s, const int64_t* __restrict__ labels,
                                            int b) {
  SoftRow r;
  r.y1 = labels[b];
  r.y2 = s.labels2 != nullptr ? s.labels2[b] : r.y1;
  r.w = s.weight != nullptr ? s.weight[b] : 1.f;
  r.eps = s.smoothing;
  return r;
}

// t_c
__device__ __forceinline__ float soft_target(const SoftRow& r, int c, int C) {
  const float t = (1.f - r.eps) * (r.w * (c == r.y1 ? 1.f : 0.f) + (1.f - r.w) * (c == r.y2 ? 1.f : 0.f));
  return r.eps > 0.f ? t + r.eps / (float)C : t;
}

// sum_c t_c x_c from the two picked logits and (eps > 0 only) the sum of all of them
__device__ __forceinline__ float soft_picked(const SoftRow& r, float x1, float x2, float sum_x, int C) {
  const float p = (1.f - r.eps) * (r.w * x1 + (1.f - r.w) * x2);
  return r.eps > 0.f ? p + (r.eps / (float)C) * sum_x : p;
}

// the label accuracy is counted against: the dominant one, a tie goes to y1
__device__ __forceinline__ int64_t soft_dominant(const SoftRow& r) { return r.w >= 0.5f ? r.y1 : r.y2; }

}  // namespace pca
