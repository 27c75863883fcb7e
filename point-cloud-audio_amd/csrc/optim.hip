// The guarded optimiser step: global gradient norm, clipping, non-finite skip and a per-step
// learning-rate table, all on the device so that a captured train step needs no host sync for them.
//   k_grad_sumsq  per-workgroup partial sums of squares of the flat gradient (fp64, fixed order)
//   k_adam_ex     the clip factor, the table lookup, the skip and the applied-step bias correction in
//                 front of k_adam's (train_ops.hip) element pass
// The partials cross from one launch to the next: the kernel boundary is the ordering.
#include "pca_common.h"

#include <math.h>

namespace pca {
namespace {

constexpr int SUMSQ_THREADS = 256;
// float4 quadruples per thread at which the grid stops growing with n: 16 fp32 terms a thread (the
// error bound of the norm is that many half-ulps), and at most 256 partials for the consumer to add
constexpr int SUMSQ_QUADS = 4;
constexpr int SUMSQ_MAX_PARTIALS = 256;

int64_t sumsq_partials(int64_t n) {
  int64_t g = cdiv(n, (int64_t)SUMSQ_THREADS * 4 * SUMSQ_QUADS);
  if (g > SUMSQ_MAX_PARTIALS) g = SUMSQ_MAX_PARTIALS;
  return g < 1 ? 1 : g;
}

// partials[blockIdx.x] = sum of g[i]^2 over this workgroup's grid-stride slice.  A thread adds its own
// terms in fp32 in index order; lanes (xor butterfly), waves (index order) in fp64.
__global__ __launch_bounds__(SUMSQ_THREADS) void k_grad_sumsq(const float* __restrict__ g, int64_t n,
                                                              double* __restrict__ partials) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const bool vec = ((uintptr_t)g & 15) == 0;
  float acc = 0.f;
  auto sq4 = [&](const float4& x) {
    acc += x.x * x.x; acc += x.y * x.y; acc += x.z * x.z; acc += x.w * x.w;
  };
  if (vec) {
    // two quadruples in flight, as k_adam
    float4 x0, x1;
    const bool h0 = i < n4, h1 = i + stride < n4;
    if (h0) x0 = g4[i];
    if (h1) x1 = g4[i + stride];
    if (h0) sq4(x0);
    if (h1) sq4(x1);
    for (int64_t k = i + 2 * stride; k < n4; k += stride) sq4(g4[k]);
  }
  // the tail (n % 4 elements), or everything when the pointer is not 16-byte aligned
  for (int64_t k = (vec ? (n4 << 2) : 0) + i; k < n; k += stride) {
    const float x = g[k];
    acc += x * x;
  }
  double s = (double)acc;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  __shared__ double wsum[SUMSQ_THREADS / 64];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = wsum[0];
#pragma unroll
    for (int w = 1; w < SUMSQ_THREADS / 64; ++w) t += wsum[w];
    partials[blockIdx.x] = t;
  }
}

// The element pass of k_adam (train_ops.hip), statement for statement, with the step number handed in.
// Kept out of line and behind by-value scalars on purpose: which of the two products of
// `a * b + c * d` the compiler fuses depends on how the operands reach the expression, and with clip == 1
// the guarded step has to round exactly as k_adam does (tests/test_gpu_optim.py compares the two bit for
// bit).  Each thread two float4 quadruples in flight in the first pass.
__device__ __noinline__ void adam_pass(float* __restrict__ p, float* __restrict__ g,
                                       float* __restrict__ m, float* __restrict__ v, int64_t n,
                                       float lr, float b1, float b2, float eps, float wd, float gscale,
                                       int ti, int zero_grad) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* g4 = reinterpret_cast<float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  float4 w0, g0, m0, v0, w1, g1, m1, v1;
  const bool h0 = vec && i < n4, h1 = vec && i + stride < n4;
  if (h0) { w0 = p4[i]; g0 = g4[i]; m0 = m4[i]; v0 = v4[i]; }
  if (h1) { w1 = p4[i + stride]; g1 = g4[i + stride]; m1 = m4[i + stride]; v1 = v4[i + stride]; }
  const float t = (float)ti;
  const float bc1 = 1.f - powf(b1, t);
  const float bc2 = 1.f - powf(b2, t);
  const float step_size = lr / bc1;
  const float inv_sqrt_bc2 = 1.f / sqrtf(bc2);
  auto upd = [&](float& w, float& gg, float& mm, float& vv) {
    const float gi = gg * gscale + wd * w;            // coupled L2 (torch.optim.Adam)
    mm = b1 * mm + (1.f - b1) * gi;
    vv = b2 * vv + (1.f - b2) * gi * gi;
    const float denom = sqrtf(vv) * inv_sqrt_bc2 + eps;
    w = w - step_size * (mm / denom);
    if (zero_grad) gg = 0.f;
  };
  auto upd4 = [&](float4& w, float4& gg, float4& mm, float4& vv) {
    upd(w.x, gg.x, mm.x, vv.x); upd(w.y, gg.y, mm.y, vv.y);
    upd(w.z, gg.z, mm.z, vv.z); upd(w.w, gg.w, mm.w, vv.w);
  };
  if (h0) {
    upd4(w0, g0, m0, v0);
    p4[i] = w0; m4[i] = m0; v4[i] = v0;
    if (zero_grad) g4[i] = g0;
  }
  if (h1) {
    upd4(w1, g1, m1, v1);
    p4[i + stride] = w1; m4[i + stride] = m1; v4[i + stride] = v1;
    if (zero_grad) g4[i + stride] = g1;
  }
  if (vec) {
    for (int64_t k = i + 2 * stride; k < n4; k += stride) {
      float4 w = p4[k], gg = g4[k], mm = m4[k], vv = v4[k];
      upd4(w, gg, mm, vv);
      p4[k] = w; m4[k] = mm; v4[k] = vv;
      if (zero_grad) g4[k] = gg;
    }
  }
  // the tail (n % 4 elements), or everything when a pointer is not 16-byte aligned
  for (int64_t k = (vec ? (n4 << 2) : 0) + i; k < n; k += stride) {
    float w = p[k], gg = g[k], mm = m[k], vv = v[k];
    upd(w, gg, mm, vv);
    p[k] = w; m[k] = mm; v[k] = vv;
    if (zero_grad) g[k] = gg;
  }
}

// step / ticket protocol: k_adam's (train_ops.hip).  Every workgroup reads step[0] and the state struct
// before it draws its ticket; the workgroup drawing the last ticket writes the struct and publishes the
// count.
__global__ __launch_bounds__(256) void k_adam_ex(float* __restrict__ p, float* __restrict__ g,
                                                 float* __restrict__ m, float* __restrict__ v,
                                                 int64_t n, float lr0, float b1, float b2,
                                                 float eps, float wd, float gscale0, float max_norm,
                                                 int skip_nonfinite,
                                                 const double* __restrict__ partials, int n_partials,
                                                 const float* __restrict__ lr_table,
                                                 int64_t lr_table_len, int32_t* __restrict__ step,
                                                 pca_optim_state* __restrict__ state,
                                                 int zero_grad) {
  // The step count, the state and this thread's partial are requested together; the table entry depends
  // on the step count, the element pass on the norm: two more L2 round trips than k_adam.
  __shared__ double part[SUMSQ_MAX_PARTIALS];
  const int ti = step[0] + 1;
  const pca_optim_state st = *state;
  const bool have_norm = partials != nullptr;
  const bool has_part = have_norm && (int)threadIdx.x < n_partials;
  double my_part = 0.0;
  if (has_part) my_part = partials[threadIdx.x];
  const int64_t tl = (int64_t)ti < lr_table_len ? (int64_t)ti : lr_table_len;
  const float lr = lr_table != nullptr ? lr_table[tl - 1] : lr0;

  // the global norm: every workgroup adds the partials itself, index order, fp64 (redundant, identical)
  float norm = 0.f;
  if (have_norm) {
    if (has_part) part[threadIdx.x] = my_part;
    __syncthreads();
    double s = 0.0;
    for (int k = 0; k < n_partials; ++k) s += part[k];
    norm = (float)((double)gscale0 * sqrt(s));
  }
  float clip = 1.f;
  if (max_norm > 0.f) {
    const float c = max_norm / (norm + 1e-6f);
    clip = c >= 1.f ? 1.f : c;           // a NaN norm stays a NaN factor (torch.clamp)
  }
  const bool finite = !have_norm || (norm - norm == 0.f);
  const bool skip = skip_nonfinite != 0 && !finite;
  if (!skip) {
    // gscale0 * 1.0f is gscale0; the bias correction counts the applied steps, this one included
    adam_pass(p, g, m, v, n, lr, b1, b2, eps, wd, gscale0 * clip, ti - st.skipped, zero_grad);
  } else if (zero_grad) {
    // parameters and moments stay bit for bit; the gradient is still handed back cleared
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool vec = ((uintptr_t)g & 15) == 0;
    if (vec) {
      float4* g4 = reinterpret_cast<float4*>(g);
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int64_t k = i; k < n4; k += stride) g4[k] = z;
    }
    for (int64_t k = (vec ? (n4 << 2) : 0) + i; k < n; k += stride) g[k] = 0.f;
  }
  // every wave has what it read of step[0] and the state (a skipped step consumes none of it in the
  // updates, so wait for the loads themselves) before thread 0 draws the ticket that may overwrite them
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const int ticket = atomicAdd(&step[1], 1);
    if (ticket == (int)gridDim.x - 1) {
      pca_optim_state ns = st;
      ns.skipped += skip ? 1 : 0;
      ns.clipped += (!skip && clip < 1.f) ? 1 : 0;
      ns.last_norm = norm;
      ns.last_lr = lr;
      if (have_norm && finite) {
        ns.norm_sum += (double)norm;
        ns.norm_count += 1;
      }
      *state = ns;
      step[1] = 0;
      step[0] = ti;
    }
  }
}

}  // namespace
}  // namespace pca

extern "C" {

int64_t pca_grad_sumsq_partials(int64_t n) { return n < 0 ? 0 : pca::sumsq_partials(n); }

int pca_grad_sumsq(const float* grad, int64_t n, double* partials, int n_partials, void* stream) {
  PCA_REQUIRE(grad && partials, "grad_sumsq: null pointer");
  PCA_REQUIRE(n >= 0, "grad_sumsq: n=%lld", (long long)n);
  PCA_REQUIRE((int64_t)n_partials == pca::sumsq_partials(n),
              "grad_sumsq: n_partials=%d, pca_grad_sumsq_partials(%lld) is %lld", n_partials,
              (long long)n, (long long)pca::sumsq_partials(n));
  hipLaunchKernelGGL(pca::k_grad_sumsq, dim3((unsigned)n_partials), dim3(pca::SUMSQ_THREADS), 0,
                     pca::as_stream(stream), grad, n, partials);
  return pca::check_launch("k_grad_sumsq");
}

int pca_adam_step_ex(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                     const pca_optim_cfg* o, const double* partials, int n_partials,
                     const float* lr_table, int64_t lr_table_len, int32_t* step_count_dev,
                     pca_optim_state* state_dev, int zero_grad, void* stream) {
  PCA_REQUIRE(param && grad && exp_avg && exp_avg_sq && o && step_count_dev && state_dev,
              "adam_step_ex: null pointer");
  PCA_REQUIRE(n >= 0, "adam_step_ex: n=%lld", (long long)n);
  PCA_REQUIRE(lr_table == nullptr || lr_table_len > 0, "adam_step_ex: lr_table with lr_table_len=%lld",
              (long long)lr_table_len);
  PCA_REQUIRE(o->max_norm == o->max_norm, "adam_step_ex: max_norm is NaN");
  if (partials != nullptr)
    PCA_REQUIRE((int64_t)n_partials == pca::sumsq_partials(n),
                "adam_step_ex: n_partials=%d, pca_grad_sumsq_partials(%lld) is %lld", n_partials,
                (long long)n, (long long)pca::sumsq_partials(n));
  else
    PCA_REQUIRE(!(o->max_norm > 0.f) && o->skip_nonfinite == 0,
                "adam_step_ex: partials is NULL with max_norm=%g skip_nonfinite=%d (both need the norm)",
                (double)o->max_norm, (int)o->skip_nonfinite);
  // the grid of pca_adam_step: few, longer workgroups (the arrival tickets are serialised atomics)
  int64_t blocks = pca::cdiv(n, 256 * 8);
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;                      // n == 0 still advances the step count
  hipLaunchKernelGGL(pca::k_adam_ex, dim3((unsigned)blocks), dim3(256), 0, pca::as_stream(stream),
                     param, grad, exp_avg, exp_avg_sq, n, o->lr, o->beta1, o->beta2, o->eps,
                     o->weight_decay, o->grad_scale, o->max_norm, (int)o->skip_nonfinite, partials,
                     partials ? n_partials : 0,
                     lr_table, lr_table ? lr_table_len : (int64_t)1, step_count_dev, state_dev,
                     zero_grad);
  return pca::check_launch("k_adam_ex");
}
}
