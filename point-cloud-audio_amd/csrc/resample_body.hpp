// One output sample of the band-limited resampler, shared by k_resample (features.hip: a whole clip)
// and k_frame_points_ex (frame_points_ex.hip: the samples a frame needs, computed while it is
// loaded), so that both give the same fp32 sample.
//
// Smith's band-limited interpolation (resampy's resample_f restated): both wings of the filter, table
// entries linearly interpolated, fp64 accumulation.  Per output sample 2 * num_zeros / min(1, ratio)
// input samples are read (L2-resident: neighbouring threads share them).  The tap loops are unrolled by 4
// so that the loads of four taps are in flight together; the sum keeps its order, tap by tap.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pca {

// Output sample t (t / ratio must lie in [0, n_in)) of x[n_in] resampled by `ratio`, times `gain`.
// win / delta [nwin]: the right wing of the filter and its first difference, num_table entries per
// zero crossing, win pre-scaled by min(1, ratio); (int)(min(1, ratio) * num_table) >= 1.
__device__ __forceinline__ float resample_sample(const float* __restrict__ x, int64_t n_in, double ratio,
                                                 const double* __restrict__ win,
                                                 const double* __restrict__ delta, int nwin,
                                                 int num_table, float gain, int64_t t) {
  const double scale = ratio < 1.0 ? ratio : 1.0;
  const int index_step = (int)(scale * num_table);
  const double time_register = (double)t / ratio;
  const int64_t n = (int64_t)time_register;
  double acc = 0.0;
  {   // left wing: x[n], x[n - 1], ...
    const double frac = scale * (time_register - (double)n);
    const double index_frac = frac * num_table;
    const int offset = (int)index_frac;
    const double eta = index_frac - offset;
    int64_t i_max = (nwin - offset) / index_step;
    if (n + 1 < i_max) i_max = n + 1;
#pragma unroll 4
    for (int64_t i = 0; i < i_max; ++i) {
      const int k = offset + (int)i * index_step;
      acc += (win[k] + eta * delta[k]) * (double)x[n - i];
    }
  }
  {   // right wing: x[n + 1], x[n + 2], ...
    const double frac = scale - scale * (time_register - (double)n);
    const double index_frac = frac * num_table;
    const int offset = (int)index_frac;
    const double eta = index_frac - offset;
    int64_t k_max = (nwin - offset) / index_step;
    if (n_in - n - 1 < k_max) k_max = n_in - n - 1;
#pragma unroll 4
    for (int64_t k2 = 0; k2 < k_max; ++k2) {
      const int k = offset + (int)k2 * index_step;
      acc += (win[k] + eta * delta[k]) * (double)x[n + k2 + 1];
    }
  }
  return (float)(acc * (double)gain);
}

}  // namespace pca
