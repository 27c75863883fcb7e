// The LDS sort of the per-set point selections: a bitonic network over Np (a power of two) 64-bit keys,
// ascending, run by the 1024 threads of one workgroup.  Shared by the sub-sampler, the importance sampler
// (subsample.hip: k_subsample, k_importance) and the selection by an external key (k_select), so that all of
// them order (key, point index) pairs alike.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pca {

// keys[0 .. Np) in LDS, written by the caller and visible (a barrier has passed); sorted and visible on return.
// Every pair (i, i | j) is touched by exactly one thread.  Called by all 1024 threads of the workgroup.
__device__ __forceinline__ void lds_sort_asc_1024(uint64_t* keys, int Np, int tid) {
  for (int k = 2; k <= Np; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (Np >> 1); t += 1024) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int l = i | j;
        const uint64_t a = keys[i], c = keys[l];
        const bool up = (i & k) == 0;
        if ((a > c) == up) {
          keys[i] = c;
          keys[l] = a;
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace pca
