// Clip-level aggregation of frame logits: mean log-probability, votes and the two clip predictions.
//
//   k_clip_aggregate : one workgroup per clip; wave w walks rows off[c] + w, + 4, ...; per row the
//                      log_softmax goes into the wave's fp32 partial and the argmax into a histogram;
//                      the four partials are merged in wave order
//
// replaces: nothing.  Code/pceval.py:95 counts correct FRAMES; the reference has no clip-level score.
//
// No floating-point atomics: a class's sum is the wave's rows in row order, then the four waves in wave
// order, so the same call gives the same bits whatever order the workgroups run in.  The histogram and the
// tally are integer adds.  A row of C <= 64 classes lives in one register per lane and is read once; a
// wider row is read once from HBM and twice more from cache.
//
// Rows of more than kClipChunk classes are aggregated kClipChunk classes at a time (the LDS holds the
// partials of one chunk); each pass re-reads the rows, which only a classifier of thousands of classes pays.
#include "pca_common.h"

#include <cmath>

namespace pca {
namespace {

constexpr int kClipWaves = 4;
constexpr int kClipChunk = 2048;       // classes per pass: 5 * 4 * 2048 = 40 KB of LDS at most
constexpr int kClipUnroll = 4;         // rows of one wave in flight on the C <= 64 path

// torch.argmax order of two (value, index) candidates, as k_eval_tally (train_ops.hip): NaN is the
// maximum, equal values (and two NaNs) go to the lower index
__device__ inline bool argmax_before(float a, int ia, float b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na != nb) return na;
  if (!na && a != b) return a > b;
  return ia < ib;
}

// vote rule: more votes, then the mean log-prob in argmax order, then the lower class
__device__ inline bool vote_before(int va, float ma, int ia, int vb, float mb, int ib) {
  if (va != vb) return va > vb;
  return argmax_before(ma, ia, mb, ib);
}

__device__ inline void wave_argmax(float& m, int& am) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    if (argmax_before(om, oa, m, am)) { m = om; am = oa; }
  }
}

__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// U rows of C <= 64 classes, one class per lane: acc += log_softmax(row)[lane] in row order, and the
// rows' argmax into hist.  The U reductions are independent, so their shuffles overlap.
template <int U>
__device__ inline void rows_small(const float* __restrict__ x, int64_t stride, int C, int lane,
                                  float& acc, int* hist) {
  const bool on = lane < C;
  float v[U], m[U], s[U];
  int am[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    v[u] = on ? x[u * stride + lane] : -INFINITY;
    m[u] = v[u];
    am[u] = on ? lane : 0x7fffffff;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) wave_argmax(m[u], am[u]);
#pragma unroll
  for (int u = 0; u < U; ++u) s[u] = wave_sum(on ? expf(v[u] - m[u]) : 0.f);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    acc += (v[u] - m[u]) - logf(s[u]);
    if (lane == 0) atomicAdd(&hist[am[u]], 1);
  }
}

__global__ __launch_bounds__(256) void k_clip_aggregate(
    const float* __restrict__ logits, int64_t n_sets, int C, const int64_t* __restrict__ off,
    const int64_t* __restrict__ labels, float* __restrict__ mean, int32_t* __restrict__ votes,
    int64_t* __restrict__ pred, unsigned long long* __restrict__ counts) {
  extern __shared__ float smem[];
  __shared__ int red_v[kClipWaves], red_vi[kClipWaves], red_mi[kClipWaves];
  __shared__ float red_vm[kClipWaves], red_m[kClipWaves];
  const int CH = C < kClipChunk ? C : kClipChunk;
  float* part = smem;                                        // [kClipWaves][CH]
  int* hist = reinterpret_cast<int*>(smem + kClipWaves * CH);  // [CH]
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;

  int64_t r0 = off[c], r1 = off[c + 1];
  r0 = r0 < 0 ? 0 : (r0 > n_sets ? n_sets : r0);
  r1 = r1 < r0 ? r0 : (r1 > n_sets ? n_sets : r1);
  const int64_t n = r1 - r0;
  if (n == 0) {
    for (int j = tid; j < C; j += 256) {
      if (mean) mean[c * C + j] = 0.f;
      if (votes) votes[c * C + j] = 0;
    }
    if (tid == 0 && pred) { pred[2 * c] = -1; pred[2 * c + 1] = -1; }
    return;
  }
  const float nf = (float)n;

  int bv = -1, bvi = 0x7fffffff, bmi = 0x7fffffff;   // this thread's best by votes / by mean
  float bvm = -INFINITY, bm = -INFINITY;
  for (int c0 = 0; c0 < C; c0 += CH) {
    const int cw = C - c0 < CH ? C - c0 : CH;
    float* p = part + w * CH;
    for (int j = lane; j < cw; j += 64) p[j] = 0.f;
    for (int j = tid; j < cw; j += 256) hist[j] = 0;
    __syncthreads();

    if (C <= 64) {
      float acc = 0.f;
      int64_t r = r0 + w;
      for (; r + kClipWaves * (kClipUnroll - 1) < r1; r += kClipWaves * kClipUnroll)
        rows_small<kClipUnroll>(logits + r * C, (int64_t)kClipWaves * C, C, lane, acc, hist);
      for (; r < r1; r += kClipWaves) rows_small<1>(logits + r * C, 0, C, lane, acc, hist);
      if (lane < C) p[lane] = acc;
    } else {
      for (int64_t r = r0 + w; r < r1; r += kClipWaves) {
        const float* __restrict__ x = logits + r * C;
        float m = -INFINITY;
        int am = 0x7fffffff;
        for (int j = lane; j < C; j += 64) {
          const float v = x[j];
          if (argmax_before(v, j, m, am)) { m = v; am = j; }
        }
        wave_argmax(m, am);
        float s = 0.f;
        for (int j = lane; j < C; j += 64) s += expf(x[j] - m);
        const float lse = logf(wave_sum(s));
        for (int j = lane; j < cw; j += 64) p[j] += (x[c0 + j] - m) - lse;
        if (lane == 0 && am >= c0 && am < c0 + cw) atomicAdd(&hist[am - c0], 1);
      }
    }
    __syncthreads();

    for (int j = tid; j < cw; j += 256) {
      const float sum = ((part[j] + part[CH + j]) + part[2 * CH + j]) + part[3 * CH + j];
      const float mu = sum / nf;
      const int v = hist[j];
      if (mean) mean[c * C + c0 + j] = mu;
      if (votes) votes[c * C + c0 + j] = v;
      if (vote_before(v, mu, c0 + j, bv, bvm, bvi)) { bv = v; bvm = mu; bvi = c0 + j; }
      if (argmax_before(mu, c0 + j, bm, bmi)) { bm = mu; bmi = c0 + j; }
    }
    __syncthreads();   // the next chunk clears part / hist
  }

#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int ov = __shfl_xor(bv, o, 64), ovi = __shfl_xor(bvi, o, 64);
    const float ovm = __shfl_xor(bvm, o, 64);
    if (vote_before(ov, ovm, ovi, bv, bvm, bvi)) { bv = ov; bvm = ovm; bvi = ovi; }
    const float om = __shfl_xor(bm, o, 64);
    const int omi = __shfl_xor(bmi, o, 64);
    if (argmax_before(om, omi, bm, bmi)) { bm = om; bmi = omi; }
  }
  if (lane == 0) {
    red_v[w] = bv; red_vm[w] = bvm; red_vi[w] = bvi;
    red_m[w] = bm; red_mi[w] = bmi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < kClipWaves; ++k) {
      if (vote_before(red_v[k], red_vm[k], red_vi[k], bv, bvm, bvi)) {
        bv = red_v[k]; bvm = red_vm[k]; bvi = red_vi[k];
      }
      if (argmax_before(red_m[k], red_mi[k], bm, bmi)) { bm = red_m[k]; bmi = red_mi[k]; }
    }
    if (pred) { pred[2 * c] = bvi; pred[2 * c + 1] = bmi; }
    if (labels) {
      const int64_t lab = labels[c];
      if ((int64_t)bvi == lab) atomicAdd(counts, 1ull);
      if ((int64_t)bmi == lab) atomicAdd(counts + 1, 1ull);
    }
  }
}

}  // namespace
}  // namespace pca

extern "C" {

int pca_clip_aggregate(const float* logits, int64_t n_sets, int C, const int64_t* clip_offsets,
                       int n_clips, const int64_t* labels, float* mean_logprob, int32_t* votes,
                       int64_t* pred, int64_t* counts, int slot, void* stream) {
  PCA_REQUIRE(n_sets >= 0 && n_clips >= 0 && C >= 1, "clip_aggregate: n_sets=%lld n_clips=%d C=%d",
              (long long)n_sets, n_clips, C);
  PCA_REQUIRE(clip_offsets && (logits || n_sets == 0), "clip_aggregate: null pointer");
  PCA_REQUIRE((labels == nullptr) == (counts == nullptr),
              "clip_aggregate: labels and counts go together (labels %s, counts %s)",
              labels ? "given" : "null", counts ? "given" : "null");
  PCA_REQUIRE(slot >= 0, "clip_aggregate: slot=%d", slot);
  if (n_clips == 0) return PCA_OK;
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counter width");
  const int CH = C < pca::kClipChunk ? C : pca::kClipChunk;
  const size_t lds = (size_t)(pca::kClipWaves + 1) * CH * sizeof(float);
  hipLaunchKernelGGL(pca::k_clip_aggregate, dim3((unsigned)n_clips), dim3(64 * pca::kClipWaves), lds,
                     pca::as_stream(stream), logits, n_sets, C, clip_offsets, labels, mean_logprob,
                     votes, pred,
                     counts ? reinterpret_cast<unsigned long long*>(counts + 2 * (int64_t)slot)
                            : nullptr);
  return pca::check_launch("k_clip_aggregate");
}
}
