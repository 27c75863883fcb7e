// The guarded optimiser step of optim.hip with three options on top, still one launch:
//   decoupled weight decay (AdamW), a rate and a decay multiplier per segment of the flat vector, and an
//   averaged copy of the weights (EMA) updated in the same pass.
//   k_adam_groups  k_adam_ex's prologue and step / ticket protocol around one element pass (adam_pass
//                  as it stands in optim.hip, or groups_pass) and, with an averaged copy, average_pass
// Two rounding contracts (tests/test_gpu_optim_groups.py compares bit for bit): with no option, and with
// the averaged copy alone, p, m, v, the step words and the state words are k_adam_ex's.
#include "pca_common.h"

#include <math.h>

namespace pca {
namespace {

constexpr int GROUPS_MAX_SEG = 256;         // one table entry per thread of a workgroup
constexpr int GROUPS_MAX_PARTIALS = 256;    // pca_grad_sumsq_partials' bound for any n

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

// adam_pass of optim.hip, verbatim: the same signature and the same statements, so that this translation
// unit compiles it to the same instructions (it is out of line and behind by-value scalars; which product of
// `a * b + c * d` the compiler fuses depends on how the operands reach the expression, and differs from one
// element of a quadruple to the next).  The launch without groups and without decoupling runs it, with or
// without the averaged copy: that is the rounding contract tests/test_gpu_optim_groups.py checks bit for bit.
// Do not add a parameter or a statement here; options go into groups_pass and average_pass.
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
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  const bool avec = ((uintptr_t)avg & 15) == 0;
  auto mix = [&](float a, float w) { return copy ? w : a + aw * (w - a); };
  if (vec) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
    float4* a4 = reinterpret_cast<float4*>(avg);
    for (int64_t k = i; k < n4; k += stride) {
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
    }
  }
  for (int64_t k = (vec ? (n4 << 2) : 0) + i; k < n; k += stride)
    avg[k] = mix(copy ? 0.f : avg[k], p[k]);
}

// step / ticket protocol, clip, skip, table and state words: k_adam_ex's (optim.hip), statement for
// statement.  New: the segment table goes to LDS once per workgroup, and the applied-step number
// a = t - skipped (this launch included) decides between the copy and the average; no new device state.
__global__ __launch_bounds__(256) void k_adam_groups(
    float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
    int64_t n, float lr0, float b1, float b2, float eps, float wd, float gscale0, float max_norm,
    int skip_nonfinite, const double* __restrict__ partials, int n_partials,
    const float* __restrict__ lr_table, int64_t lr_table_len, int32_t* __restrict__ step,
    pca_optim_state* __restrict__ state, int zero_grad, int decoupled, int n_seg,
    const int64_t* __restrict__ seg_end, const float* __restrict__ seg_lr,
    const float* __restrict__ seg_wd, float* __restrict__ avg, float avg_weight, int avg_start) {
  __shared__ double part[GROUPS_MAX_PARTIALS];
  const int ti = step[0] + 1;
  const pca_optim_state st = *state;
  const bool have_norm = partials != nullptr;
  const bool has_part = have_norm && (int)threadIdx.x < n_partials;
  double my_part = 0.0;
  if (has_part) my_part = partials[threadIdx.x];
  if ((int)threadIdx.x < n_seg) {
    T.end[threadIdx.x] = seg_end[threadIdx.x];
    T.lr[threadIdx.x] = seg_lr != nullptr ? seg_lr[threadIdx.x] : 1.f;
    T.wd[threadIdx.x] = seg_wd != nullptr ? seg_wd[threadIdx.x] : 1.f;
  }
  const int64_t tl = (int64_t)ti < lr_table_len ? (int64_t)ti : lr_table_len;
  const float lr = lr_table != nullptr ? lr_table[tl - 1] : lr0;

  float norm = 0.f;
  if (has_part) part[threadIdx.x] = my_part;
  if (have_norm || n_seg > 0) __syncthreads();        // uniform: both are launch arguments
  if (have_norm) {
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
    const int applied = ti - st.skipped;              // counts this launch
    const float gs = gscale0 * clip;
    if (n_seg > 0) {
      if (decoupled) groups_pass<true, true>(p, g, m, v, n, lr, b1, b2, eps, wd, gs, applied, zero_grad, n_seg);
      else groups_pass<true, false>(p, g, m, v, n, lr, b1, b2, eps, wd, gs, applied, zero_grad, n_seg);
    } else if (decoupled) {
      groups_pass<false, true>(p, g, m, v, n, lr, b1, b2, eps, wd, gs, applied, zero_grad, 0);
    } else {
      adam_pass(p, g, m, v, n, lr, b1, b2, eps, wd, gs, applied, zero_grad);
    }
    if (avg != nullptr) average_pass(p, g, m, v, avg, n, avg_weight, applied <= avg_start);
  } else if (zero_grad) {
    // parameters, moments and the averaged copy stay bit for bit; the gradient is handed back cleared
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
  // as k_adam_ex: every wave holds what it read of step[0] and the state before the ticket is drawn
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

int pca_adam_step_groups(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                         const pca_optim_cfg* o, const double* partials, int n_partials,
                         const float* lr_table, int64_t lr_table_len, int32_t* step_count_dev,
                         pca_optim_state* state_dev, int zero_grad, const pca_optim_groups* gr,
                         const int64_t* seg_end_host, void* stream) {
  PCA_REQUIRE(param && grad && exp_avg && exp_avg_sq && o && step_count_dev && state_dev,
              "adam_step_groups: null pointer");
  PCA_REQUIRE(gr != nullptr, "adam_step_groups: gr is NULL");
  PCA_REQUIRE(n >= 0, "adam_step_groups: n=%lld", (long long)n);
  PCA_REQUIRE(lr_table == nullptr || lr_table_len > 0,
              "adam_step_groups: lr_table with lr_table_len=%lld", (long long)lr_table_len);
  PCA_REQUIRE(o->max_norm == o->max_norm, "adam_step_groups: max_norm is NaN");
  const int64_t want_partials = pca_grad_sumsq_partials(n);
  if (partials != nullptr)
    PCA_REQUIRE((int64_t)n_partials == want_partials && want_partials <= pca::GROUPS_MAX_PARTIALS,
                "adam_step_groups: n_partials=%d, pca_grad_sumsq_partials(%lld) is %lld", n_partials,
                (long long)n, (long long)want_partials);
  else
    PCA_REQUIRE(!(o->max_norm > 0.f) && o->skip_nonfinite == 0,
                "adam_step_groups: partials is NULL with max_norm=%g skip_nonfinite=%d (both need the norm)",
                (double)o->max_norm, (int)o->skip_nonfinite);
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
  // pca_adam_step_ex's grid
  int64_t blocks = pca::cdiv(n, 256 * 8);
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;                      // n == 0 still advances the step count
  hipLaunchKernelGGL(pca::k_adam_groups, dim3((unsigned)blocks), dim3(256), 0,
                     pca::as_stream(stream), param, grad, exp_avg, exp_avg_sq, n, o->lr, o->beta1,
                     o->beta2, o->eps, o->weight_decay, o->grad_scale, o->max_norm,
                     (int)o->skip_nonfinite, partials, partials ? n_partials : 0, lr_table,
                     lr_table ? lr_table_len : (int64_t)1, step_count_dev, state_dev, zero_grad,
                     (int)gr->decoupled, (int)gr->n_seg, gr->seg_end, gr->seg_lr_scale,
                     gr->seg_wd_scale, gr->avg, gr->avg_weight, (int)gr->avg_start);
  return pca::check_launch("k_adam_groups");
}
}
