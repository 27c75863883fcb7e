// Stand-alone launch of the fixed-order slab sum (slab_sum_body.hpp): out[i] (+)= sum_s slabs[s][i], the
// replacement of fp32 atomics wherever workgroups reduce into one small tensor.
#include "bwd_defer.hpp"
#include "slab_sum_body.hpp"

namespace pca {

namespace {
// several slab sums in one launch (blockIdx.y = job)
__global__ __launch_bounds__(256) void k_slab_sum_jobs(const SlabSumJobs jobs) {
  __shared__ float4 red[4 * 64];
  slab_sum_body(jobs.j[blockIdx.y], blockIdx.x, threadIdx.x, red);
}
}  // namespace
int slab_sum_jobs(const SlabSumJobs& J, hipStream_t st) {
  if (J.n == 0) return PCA_OK;
  int nmax = 0;
  for (int i = 0; i < J.n; ++i) {
    PCA_REQUIRE(slab_sum_job_ok(J.j[i]), "slab_sum_jobs: alignment");
    nmax = J.j[i].n > nmax ? J.j[i].n : nmax;
  }
  hipLaunchKernelGGL(k_slab_sum_jobs, dim3((unsigned)cdiv(nmax, 256), (unsigned)J.n), dim3(256), 0,
                     st, J);
  return check_launch("k_slab_sum_jobs");
}
int slab_sum(const float* slabs, int S, int n, float* out, int accumulate, hipStream_t st) {
  SlabSumJobs J{};
  J.j[0] = SlabSumJob{slabs, out, S, n, accumulate, 0};
  J.n = 1;
  return slab_sum_jobs(J, st);
}

}  // namespace pca
