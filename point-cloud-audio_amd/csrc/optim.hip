// The optimiser of the train step, one translation unit:
//   k_adam         torch.optim.Adam with coupled weight decay as one fused pass over a flat parameter vector
//                  (Code/settransformer.py:89-91,106,108)
//   k_grad_sumsq   per-workgroup partial sums of squares of the flat gradient (fp64, fixed order)
//   k_adam_ex      the guarded step: global gradient norm, clipping, non-finite skip and a per-step
//                  learning-rate table, all on the device so that a captured train step needs no host sync
//                  for them, in front of adam_pass
//   k_adam_groups  the guarded step with three options, still one launch: decoupled weight decay (AdamW), a
//                  rate and a decay multiplier per segment of the flat vector, and an averaged copy of the
//                  weights (EMA) updated behind the element pass
// The partials cross from k_grad_sumsq's launch to the next: the kernel boundary is the ordering.
// Rounding contracts (tests/test_gpu_optim.py, tests/test_gpu_optim_groups.py, bit for bit): k_adam_ex with a
// clip factor of 1 is k_adam; k_adam_groups with no option, or with the averaged copy alone, is k_adam_ex.
// The second holds by construction (both kernels call the one adam_pass), the first by the text of adam_pass.
#include "pca_common.h"

#include <math.h>

namespace pca {
namespace {

constexpr int SUMSQ_THREADS = 256;
// float4 quadruples per thread at which the grid stops growing with n: 16 fp32 terms a thread (the
// error bound of the norm is that many half-ulps), and at most 256 partials for the consumer to add
constexpr int SUMSQ_QUADS = 4;
constexpr int MAX_PARTIALS = 256;           // one partial per thread of a consuming workgroup
constexpr int GROUPS_MAX_SEG = 256;         // one table entry per thread of a workgroup

int64_t sumsq_partials(int64_t n) {
  int64_t g = cdiv(n, (int64_t)SUMSQ_THREADS * 4 * SUMSQ_QUADS);
  if (g > MAX_PARTIALS) g = MAX_PARTIALS;
  return g < 1 ? 1 : g;
}

// The grid of all three Adam launches: few, longer workgroups of 256 threads (the arrival tickets are
// serialised atomics on one address; two float4 quadruples per thread in the first pass).
int64_t adam_blocks(int64_t n) {
  int64_t blocks = cdiv(n, 256 * 8);
  if (blocks > 1024) blocks = 1024;
  return blocks < 1 ? 1 : blocks;                  // n == 0 still advances the step count
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

// The element pass of the two guarded kernels: k_adam's statements with the step number handed in.  Out of
// line and behind by-value scalars on purpose: which of the two products of `a * b + c * d` the compiler
// fuses depends on how the operands reach the expression, and with clip == 1 the guarded step has to round
// exactly as k_adam does.  A templated variant and one inlined behind the norm each came out an ulp off in a
// few elements, so options go into groups_pass and average_pass, never into this signature or these
// statements.  Each thread two float4 quadruples in flight in the first pass.
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

// The single deliberate second copy of adam_pass's statements: k_adam requests step[0] together with its
// first operands, and a call to the out-of-line pass would put that L2 round trip in front of them on the
// path of the default Trainer.  An edit to either copy goes into both.
// step[0] = optimiser step count, step[1] = arrival ticket (zero between launches).  Every
// workgroup reads step[0] before it draws its ticket; the workgroup drawing the last ticket
// publishes step[0] + 1 and clears the ticket, so the count advances inside this launch
// (graph replays stay correct) without a second kernel.
__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, float* __restrict__ g,
                                              float* __restrict__ m, float* __restrict__ v,
                                              int64_t n, float lr, float b1, float b2,
                                              float eps, float wd, float gscale,
                                              int32_t* __restrict__ step, int zero_grad) {
  // The kernel is one dependent chain of L2 round trips long (1.2 MB of parameters at configs[1]):
  // the step count and the first batch of operands are requested together, 16-byte accesses, each
  // thread two float4 quadruples in flight.
  const int ti = step[0] + 1;
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
  // every wave of the workgroup has its step[0] (loaded at the top, consumed by the updates above)
  // before thread 0 draws the ticket that may publish the next count
  __syncthreads();
  if (threadIdx.x == 0) {
    const int ticket = atomicAdd(&step[1], 1);
    if (ticket == (int)gridDim.x - 1) {
      step[1] = 0;
      step[0] = ti;
    }
  }
}

// The element passes' index ownership without their two quadruples in flight: with `vec`, this thread's
// float4 quadruples k (grid stride) and then the n % 4 tail elements; without it, every element it owns.
template <class Quad, class One>
__device__ __forceinline__ void owned_elements(int64_t n, bool vec, Quad quad, One one) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec)
    for (int64_t k = i; k < n4; k += stride) quad(k);
  for (int64_t k = (vec ? (n4 << 2) : 0) + i; k < n; k += stride) one(k);
}

// what a skipped step with zero_grad still does: the gradient is handed back cleared
__device__ __forceinline__ void clear_grad(float* __restrict__ g, int64_t n) {
  float4* g4 = reinterpret_cast<float4*>(g);
  owned_elements(n, ((uintptr_t)g & 15) == 0,
                 [&](int64_t k) { g4[k] = make_float4(0.f, 0.f, 0.f, 0.f); },
                 [&](int64_t k) { g[k] = 0.f; });
}

// the segment table of one launch, in LDS (file scope: groups_pass is out of line and reads it there)
struct SegTable {
  int64_t end[GROUPS_MAX_SEG];     // ascending, end[n_seg - 1] == n
  float lr[GROUPS_MAX_SEG];
  float wd[GROUPS_MAX_SEG];
};
__shared__ SegTable T;

// The segment of element idx: the first s with end[s] > idx.  Bounded by the table whatever it holds.
__device__ __forceinline__ int seg_of(int n_seg, int64_t idx) {
  int lo = 0, hi = n_seg - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (T.end[mid] > idx) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// The element pass with a segment table and / or decoupled decay: adam_pass's loop structure and index
// ownership around an update that takes its scalars per segment.
//   GROUPED    lr and wd are scaled per segment; a quadruple inside one segment uses uniform scalars,
//              one that straddles a boundary goes element by element
//   DECOUPLED  w *= 1 - lr_e * wd_e first and the gradient carries no decay term (torch.optim.AdamW)
template <bool GROUPED, bool DECOUPLED>
__device__ __noinline__ void groups_pass(float* __restrict__ p, float* __restrict__ g,
                                         float* __restrict__ m, float* __restrict__ v, int64_t n,
                                         float lr, float b1, float b2, float eps, float wd, float gscale,
                                         int ti, int zero_grad, int n_seg) {
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
  const float inv_sqrt_bc2 = 1.f / sqrtf(bc2);
  // what one segment contributes to the update: its step size, its decay, its decoupled shrink factor
  struct Seg { float step_size, wd, shrink; bool frozen; };
  auto seg_scalars = [&](int s) {
    const float lr_e = lr * T.lr[s], wd_e = wd * T.wd[s];
    return Seg{lr_e / bc1, wd_e, 1.f - lr_e * wd_e, T.lr[s] == 0.f};
  };
  const Seg one{lr / bc1, wd, 1.f - lr * wd, false};  // without a table: one group, both scales 1
  // adam_pass's statements on one segment's scalars; a frozen segment (lr_scale == 0) keeps its weight
  // bit for bit while its moments move (a torch group with lr = 0)
  auto upd = [&](float& w, float& gg, float& mm, float& vv, const Seg& S) {
    const float w_in = w;
    float gi;
    if constexpr (DECOUPLED) {
      w = w * S.shrink;
      gi = gg * gscale;
    } else {
      gi = gg * gscale + S.wd * w;
    }
    mm = b1 * mm + (1.f - b1) * gi;
    vv = b2 * vv + (1.f - b2) * gi * gi;
    const float denom = sqrtf(vv) * inv_sqrt_bc2 + eps;
    w = w - S.step_size * (mm / denom);
    if (S.frozen) w = w_in;
    if (zero_grad) gg = 0.f;
  };
  auto upd4 = [&](float4& w, float4& gg, float4& mm, float4& vv, int64_t k) {
    if constexpr (GROUPED) {
      const int64_t e = k << 2;
      int s = seg_of(n_seg, e);
      if (T.end[s] >= e + 4) {                        // the quadruple lies inside segment s
        const Seg S = seg_scalars(s);
        upd(w.x, gg.x, mm.x, vv.x, S); upd(w.y, gg.y, mm.y, vv.y, S);
        upd(w.z, gg.z, mm.z, vv.z, S); upd(w.w, gg.w, mm.w, vv.w, S);
      } else {                                        // a boundary inside it: per element
        upd(w.x, gg.x, mm.x, vv.x, seg_scalars(s));
        while (s < n_seg - 1 && T.end[s] <= e + 1) ++s;
        upd(w.y, gg.y, mm.y, vv.y, seg_scalars(s));
        while (s < n_seg - 1 && T.end[s] <= e + 2) ++s;
        upd(w.z, gg.z, mm.z, vv.z, seg_scalars(s));
        while (s < n_seg - 1 && T.end[s] <= e + 3) ++s;
        upd(w.w, gg.w, mm.w, vv.w, seg_scalars(s));
      }
    } else {
      upd(w.x, gg.x, mm.x, vv.x, one); upd(w.y, gg.y, mm.y, vv.y, one);
      upd(w.z, gg.z, mm.z, vv.z, one); upd(w.w, gg.w, mm.w, vv.w, one);
    }
  };
  if (h0) {
    upd4(w0, g0, m0, v0, i);
    p4[i] = w0; m4[i] = m0; v4[i] = v0;
    if (zero_grad) g4[i] = g0;
  }
  if (h1) {
    upd4(w1, g1, m1, v1, i + stride);
    p4[i + stride] = w1; m4[i + stride] = m1; v4[i + stride] = v1;
    if (zero_grad) g4[i + stride] = g1;
  }
  if (vec) {
    for (int64_t k = i + 2 * stride; k < n4; k += stride) {
      float4 w = p4[k], gg = g4[k], mm = m4[k], vv = v4[k];
      upd4(w, gg, mm, vv, k);
      p4[k] = w; m4[k] = mm; v4[k] = vv;
      if (zero_grad) g4[k] = gg;
    }
  }
  // the tail (n % 4 elements), or everything when a pointer is not 16-byte aligned
  for (int64_t k = (vec ? (n4 << 2) : 0) + i; k < n; k += stride) {
    float w = p[k], gg = g[k], mm = m[k], vv = v[k];
    if constexpr (GROUPED) upd(w, gg, mm, vv, seg_scalars(seg_of(n_seg, k)));
    else upd(w, gg, mm, vv, one);
    p[k] = w; m[k] = mm; v[k] = vv;
    if (zero_grad) g[k] = gg;
  }
}

// The averaged copy, behind the element pass and apart from it so that it cannot touch the rounding of the
// weights: every thread reads back the weights it has just written itself (the element passes' index
// ownership: `vec` is their decision, from the alignment of p, g, m and v), so no other thread's store is
// waited for.  copy: avg = w (up to the applied step that starts the average); else avg += aw * (w - avg).
__device__ __noinline__ void average_pass(const float* p, const float* g, const float* m, const float* v,
                                          float* __restrict__ avg, int64_t n, float aw, int copy) {
  const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  const bool avec = ((uintptr_t)avg & 15) == 0;
  const float4* p4 = reinterpret_cast<const float4*>(p);
  float4* a4 = reinterpret_cast<float4*>(avg);
  auto mix = [&](float a, float w) { return copy ? w : a + aw * (w - a); };
  owned_elements(
      n, vec,
      [&](int64_t k) {
        const float4 w = p4[k];
        if (avec) {
          float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
          if (!copy) a = a4[k];
          a4[k] = make_float4(mix(a.x, w.x), mix(a.y, w.y), mix(a.z, w.z), mix(a.w, w.w));
        } else {
          float* a = avg + (k << 2);
          a[0] = mix(copy ? 0.f : a[0], w.x); a[1] = mix(copy ? 0.f : a[1], w.y);
          a[2] = mix(copy ? 0.f : a[2], w.z); a[3] = mix(copy ? 0.f : a[3], w.w);
        }
      },
      [&](int64_t k) { avg[k] = mix(copy ? 0.f : avg[k], p[k]); });
}

// what k_adam_groups takes beyond k_adam_ex (pca_optim_groups, by value)
struct GroupOpts {
  int decoupled, n_seg;
  const int64_t* seg_end;
  const float* seg_lr;
  const float* seg_wd;
  float* avg;
  float avg_weight;
  int avg_start;
};

// The guarded step, the body of both kernels.  OPTS false compiles the options out: no segment table in LDS,
// no averaged copy, adam_pass the only element pass.
// step / ticket protocol: k_adam's.  Every workgroup reads step[0] and the state struct before it draws
// its ticket; the workgroup drawing the last ticket writes the struct and publishes the count.  The
// applied-step number a = t - skipped (this launch included) is the bias correction's step and decides
// between the copy and the average, so the options keep no device state of their own.
template <bool OPTS>
__device__ __forceinline__ void guarded_step(float* __restrict__ p, float* __restrict__ g,
                                             float* __restrict__ m, float* __restrict__ v, int64_t n,
                                             float lr0, float b1, float b2, float eps, float wd,
                                             float gscale0, float max_norm, int skip_nonfinite,
                                             const double* __restrict__ partials, int n_partials,
                                             const float* __restrict__ lr_table, int64_t lr_table_len,
                                             int32_t* __restrict__ step,
                                             pca_optim_state* __restrict__ state, int zero_grad,
                                             const GroupOpts& G) {
  // The step count, the state and this thread's partial are requested together; the table entry depends
  // on the step count, the element pass on the norm: two more L2 round trips than k_adam.
  __shared__ double part[MAX_PARTIALS];
  const int n_seg = OPTS ? G.n_seg : 0;
  const int ti = step[0] + 1;
  const pca_optim_state st = *state;
  const bool have_norm = partials != nullptr;
  const bool has_part = have_norm && (int)threadIdx.x < n_partials;
  double my_part = 0.0;
  if (has_part) my_part = partials[threadIdx.x];
  if (OPTS && (int)threadIdx.x < n_seg) {
    T.end[threadIdx.x] = G.seg_end[threadIdx.x];
    T.lr[threadIdx.x] = G.seg_lr != nullptr ? G.seg_lr[threadIdx.x] : 1.f;
    T.wd[threadIdx.x] = G.seg_wd != nullptr ? G.seg_wd[threadIdx.x] : 1.f;
  }
  const int64_t tl = (int64_t)ti < lr_table_len ? (int64_t)ti : lr_table_len;
  const float lr = lr_table != nullptr ? lr_table[tl - 1] : lr0;

  // the global norm: every workgroup adds the partials itself, index order, fp64 (redundant, identical)
  float norm = 0.f;
  if (have_norm) {
    if (has_part) part[threadIdx.x] = my_part;
    __syncthreads();                                  // the segment table's barrier as well
    double s = 0.0;
    for (int k = 0; k < n_partials; ++k) s += part[k];
    norm = (float)((double)gscale0 * sqrt(s));
  } else if (OPTS && n_seg > 0) {
    __syncthreads();                                  // uniform: both are launch arguments
  }
  float clip = 1.f;
  if (max_norm > 0.f) {
    const float c = max_norm / (norm + 1e-6f);
    clip = c >= 1.f ? 1.f : c;           // a NaN norm stays a NaN factor (torch.clamp)
  }
  const bool finite = !have_norm || (norm - norm == 0.f);
  const bool skip = skip_nonfinite != 0 && !finite;
  if (!skip) {
    const int applied = ti - st.skipped;              // counts this launch
    const float gs = gscale0 * clip;                  // gscale0 * 1.0f is gscale0
    if (OPTS && n_seg > 0) {
      if (G.decoupled) groups_pass<true, true>(p, g, m, v, n, lr, b1, b2, eps, wd, gs, applied, zero_grad, n_seg);
      else groups_pass<true, false>(p, g, m, v, n, lr, b1, b2, eps, wd, gs, applied, zero_grad, n_seg);
    } else if (OPTS && G.decoupled) {
      groups_pass<false, true>(p, g, m, v, n, lr, b1, b2, eps, wd, gs, applied, zero_grad, 0);
    } else {
      adam_pass(p, g, m, v, n, lr, b1, b2, eps, wd, gs, applied, zero_grad);
    }
    if (OPTS && G.avg != nullptr) average_pass(p, g, m, v, G.avg, n, G.avg_weight, applied <= G.avg_start);
  } else if (zero_grad) {
    // parameters, moments and the averaged copy stay bit for bit
    clear_grad(g, n);
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
  guarded_step<false>(p, g, m, v, n, lr0, b1, b2, eps, wd, gscale0, max_norm, skip_nonfinite, partials,
                      n_partials, lr_table, lr_table_len, step, state, zero_grad, GroupOpts{});
}

__global__ __launch_bounds__(256) void k_adam_groups(
    float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
    int64_t n, float lr0, float b1, float b2, float eps, float wd, float gscale0, float max_norm,
    int skip_nonfinite, const double* __restrict__ partials, int n_partials,
    const float* __restrict__ lr_table, int64_t lr_table_len, int32_t* __restrict__ step,
    pca_optim_state* __restrict__ state, int zero_grad, int decoupled, int n_seg,
    const int64_t* __restrict__ seg_end, const float* __restrict__ seg_lr,
    const float* __restrict__ seg_wd, float* __restrict__ avg, float avg_weight, int avg_start) {
  guarded_step<true>(p, g, m, v, n, lr0, b1, b2, eps, wd, gscale0, max_norm, skip_nonfinite, partials,
                     n_partials, lr_table, lr_table_len, step, state, zero_grad,
                     GroupOpts{decoupled, n_seg, seg_end, seg_lr, seg_wd, avg, avg_weight, avg_start});
}

// What pca_adam_step_ex and pca_adam_step_groups refuse alike, under the entry's own name.
int check_guarded_args(const char* who, const float* param, const float* grad, const float* exp_avg,
                       const float* exp_avg_sq, int64_t n, const pca_optim_cfg* o,
                       const double* partials, int n_partials, const float* lr_table,
                       int64_t lr_table_len, const int32_t* step_count_dev,
                       const pca_optim_state* state_dev) {
  PCA_REQUIRE(param && grad && exp_avg && exp_avg_sq && o && step_count_dev && state_dev,
              "%s: null pointer", who);
  PCA_REQUIRE(n >= 0, "%s: n=%lld", who, (long long)n);
  PCA_REQUIRE(lr_table == nullptr || lr_table_len > 0, "%s: lr_table with lr_table_len=%lld", who,
              (long long)lr_table_len);
  PCA_REQUIRE(o->max_norm == o->max_norm, "%s: max_norm is NaN", who);
  if (partials != nullptr)
    PCA_REQUIRE((int64_t)n_partials == sumsq_partials(n),
                "%s: n_partials=%d, pca_grad_sumsq_partials(%lld) is %lld", who, n_partials,
                (long long)n, (long long)sumsq_partials(n));
  else
    PCA_REQUIRE(!(o->max_norm > 0.f) && o->skip_nonfinite == 0,
                "%s: partials is NULL with max_norm=%g skip_nonfinite=%d (both need the norm)", who,
                (double)o->max_norm, (int)o->skip_nonfinite);
  return PCA_OK;
}

}  // namespace
}  // namespace pca

extern "C" {

int pca_adam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float lr, float beta1, float beta2, float eps, float weight_decay,
                  float grad_scale, int32_t* step_count_dev, int zero_grad, void* stream) {
  PCA_REQUIRE(param && grad && exp_avg && exp_avg_sq && step_count_dev,
              "adam_step: null pointer");
  PCA_REQUIRE(n >= 0, "adam_step: n=%lld", (long long)n);
  hipStream_t st = pca::as_stream(stream);
  hipLaunchKernelGGL(pca::k_adam, dim3((unsigned)pca::adam_blocks(n)), dim3(256), 0, st, param, grad,
                     exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, grad_scale,
                     step_count_dev, zero_grad);
  return pca::check_launch("k_adam");
}

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
  PCA_TRY(pca::check_guarded_args("adam_step_ex", param, grad, exp_avg, exp_avg_sq, n, o, partials,
                                  n_partials, lr_table, lr_table_len, step_count_dev, state_dev));
  hipLaunchKernelGGL(pca::k_adam_ex, dim3((unsigned)pca::adam_blocks(n)), dim3(256), 0,
                     pca::as_stream(stream), param, grad, exp_avg, exp_avg_sq, n, o->lr, o->beta1,
                     o->beta2, o->eps, o->weight_decay, o->grad_scale, o->max_norm,
                     (int)o->skip_nonfinite, partials, partials ? n_partials : 0, lr_table,
                     lr_table ? lr_table_len : (int64_t)1, step_count_dev, state_dev, zero_grad);
  return pca::check_launch("k_adam_ex");
}

int pca_adam_step_groups(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                         const pca_optim_cfg* o, const double* partials, int n_partials,
                         const float* lr_table, int64_t lr_table_len, int32_t* step_count_dev,
                         pca_optim_state* state_dev, int zero_grad, const pca_optim_groups* gr,
                         const int64_t* seg_end_host, void* stream) {
  PCA_TRY(pca::check_guarded_args("adam_step_groups", param, grad, exp_avg, exp_avg_sq, n, o, partials,
                                  n_partials, lr_table, lr_table_len, step_count_dev, state_dev));
  PCA_REQUIRE(gr != nullptr, "adam_step_groups: gr is NULL");
  PCA_REQUIRE(gr->n_seg >= 0 && gr->n_seg <= pca::GROUPS_MAX_SEG,
              "adam_step_groups: n_seg=%d outside 0..%d", (int)gr->n_seg, pca::GROUPS_MAX_SEG);
  if (gr->n_seg > 0) {
    PCA_REQUIRE(gr->seg_end != nullptr && seg_end_host != nullptr,
                "adam_step_groups: n_seg=%d needs seg_end and its host mirror seg_end_host",
                (int)gr->n_seg);
    int64_t prev = 0;
    for (int s = 0; s < gr->n_seg; ++s) {
      PCA_REQUIRE(seg_end_host[s] > prev,
                  "adam_step_groups: seg_end is not strictly ascending from above 0 (seg_end[%d]=%lld "
                  "after %lld)", s, (long long)seg_end_host[s], (long long)prev);
      prev = seg_end_host[s];
    }
    PCA_REQUIRE(prev == n, "adam_step_groups: seg_end ends at %lld, n=%lld", (long long)prev,
                (long long)n);
  }
  PCA_REQUIRE(gr->avg_weight > 0.f && gr->avg_weight <= 1.f,
              "adam_step_groups: avg_weight=%g outside (0, 1]", (double)gr->avg_weight);
  PCA_REQUIRE(gr->avg_start >= 1, "adam_step_groups: avg_start=%d, must be >= 1",
              (int)gr->avg_start);
  hipLaunchKernelGGL(pca::k_adam_groups, dim3((unsigned)pca::adam_blocks(n)), dim3(256), 0,
                     pca::as_stream(stream), param, grad, exp_avg, exp_avg_sq, n, o->lr, o->beta1,
                     o->beta2, o->eps, o->weight_decay, o->grad_scale, o->max_norm,
                     (int)o->skip_nonfinite, partials, partials ? n_partials : 0, lr_table,
                     lr_table ? lr_table_len : (int64_t)1, step_count_dev, state_dev, zero_grad,
                     (int)gr->decoupled, (int)gr->n_seg, gr->seg_end, gr->seg_lr_scale,
                     gr->seg_wd_scale, gr->avg, gr->avg_weight, (int)gr->avg_start);
  return pca::check_launch("k_adam_groups");
}
}
