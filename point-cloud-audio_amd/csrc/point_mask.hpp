// Random interval masks over one axis of a point set (k_frame_points_ex: frequency bands over the bins,
// time stripes over the frames of a chunk): up to PCA_POINT_MASK_MAX intervals per axis, drawn per batch
// slot, their union removed.  Everything here depends on the slot alone, so it is uniform over a
// workgroup and lives in scalar registers.
//
// The rank of a kept index x among the kept ones is x minus the number of masked indices below x.  With
// at most four intervals that number is a closed form: sort the intervals by their start, cut from each
// what an earlier one already covers - they are then disjoint - and add up how much of each lies below
// x.  No scan over the axis, no LDS, no dependence between the workgroups of a slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pca_hip.h"

namespace pca {

struct MaskAxis {
  int lo[PCA_POINT_MASK_MAX], hi[PCA_POINT_MASK_MAX];   // disjoint [lo, hi), ascending; empty: lo == hi
  int start[PCA_POINT_MASK_MAX], width[PCA_POINT_MASK_MAX];   // as drawn (what the mask meta reports)
};

// masked indices below x (0 <= x <= extent)
__device__ __forceinline__ int mask_below(const MaskAxis& m, int x) {
  int n = 0;
#pragma unroll
  for (int k = 0; k < PCA_POINT_MASK_MAX; ++k) {
    const int d = (m.hi[k] < x ? m.hi[k] : x) - m.lo[k];
    n += d > 0 ? d : 0;
  }
  return n;
}

__device__ __forceinline__ bool mask_covers(const MaskAxis& m, int x) {
  bool in = false;
#pragma unroll
  for (int k = 0; k < PCA_POINT_MASK_MAX; ++k) in = in || (x >= m.lo[k] && x < m.hi[k]);
  return in;
}

// Interval k < n of an axis of `extent` indices from draws base + 2k (width, uniform over 0 .. max_width)
// and base + 2k + 1 (start, uniform over 0 .. extent - width); `draw(i)` is draw number i of the slot's
// stream.  n == 0 or max_width == 0: nothing is drawn, nothing is masked.
template <typename Draw>
__device__ __forceinline__ void mask_draw(MaskAxis& m, Draw draw, int base, int n, int max_width,
                                          int extent) {
#pragma unroll
  for (int k = 0; k < PCA_POINT_MASK_MAX; ++k) {
    int w = 0, s = 0;
    if (k < n && max_width > 0) {
      w = (int)(((draw(base + 2 * k) >> 32) * (uint64_t)(max_width + 1)) >> 32);
      s = (int)(((draw(base + 2 * k + 1) >> 32) * (uint64_t)(extent - w + 1)) >> 32);
    }
    m.start[k] = s;
    m.width[k] = w;
    // an empty interval sorts last and covers nothing
    m.lo[k] = w > 0 ? s : extent;
    m.hi[k] = w > 0 ? s + w : extent;
  }
  // sort by start: the five exchanges of the four-input network
#define PCA_MASK_CSWAP(i, j)                                    \
  if (m.lo[j] < m.lo[i]) {                                      \
    const int tl = m.lo[i], th = m.hi[i];                       \
    m.lo[i] = m.lo[j]; m.hi[i] = m.hi[j];                       \
    m.lo[j] = tl; m.hi[j] = th;                                 \
  }
  PCA_MASK_CSWAP(0, 1) PCA_MASK_CSWAP(2, 3) PCA_MASK_CSWAP(0, 2) PCA_MASK_CSWAP(1, 3) PCA_MASK_CSWAP(1, 2)
#undef PCA_MASK_CSWAP
  static_assert(PCA_POINT_MASK_MAX == 4, "the sorting network above is the four-input one");
  // cut from each interval what the ones before it reach
  int reach = 0;
#pragma unroll
  for (int k = 0; k < PCA_POINT_MASK_MAX; ++k) {
    m.lo[k] = m.lo[k] > reach ? m.lo[k] : reach;
    m.hi[k] = m.hi[k] > m.lo[k] ? m.hi[k] : m.lo[k];
    reach = m.hi[k];
  }
}

}  // namespace pca
