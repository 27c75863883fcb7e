// Merging two partials (m, l, t) of one softmax row - running max m in the log2 domain, sum l and
// weighted sum t, both relative to m: the merged max is M = max(m_0, m_1), and partial i enters with the
// factor 2^(m_i - M).  A partial over no keys at all is (-inf, 0, 0) - what a wave, a unit or a half of a
// variable-length set holds when every one of its points lies beyond the set's length - and must be the
// identity of the merge: its factor is 0 by definition, never the 2^(-inf - (-inf)) = NaN the bare
// expression gives when both partials are empty.  One expression for the set-resident forward
// (set128_fwd.hip) and for the host (pca_debug_merge_factor, tests/test_set128_merge_host.py).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace pca {

// the kernels' exp2 (v_exp_f32) on the device, the C library's on the host
__host__ __device__ inline float merge_exp2(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_exp2f(x);
#else
  return exp2f(x);
#endif
}

// factor of a partial with max m against the merged max M (M >= m); 0 when the partial is empty
__host__ __device__ inline float merge_factor(float m, float M) {
  return m == -INFINITY ? 0.f : merge_exp2(m - M);
}

}  // namespace pca
