// Leading / trailing silence trimming: the bounds librosa.effects.trim(x, top_db) returns.
//
//   k_trim_segsum : sums of squares over segments of the reflect-padded clips (reads the samples)
//   k_trim_bounds : per clip, frame powers from the segment sums -> dB against the loudest frame ->
//                   first / last non-silent frame -> (start, end)
//
// replaces: Code/settransformer.py:48, Code/pceval.py:74,127 and the same line of every other train /
// eval script (librosa 0.8 semantics restated; librosa is third-party and not vendored: "parity
// unpinned", as the resampler).
//
// Frame t of a clip covers samples [t*hop, t*hop + frame_length) of the signal reflect-padded by
// frame_length/2 on both sides.  When hop divides frame_length/2 (the reference's 2048 / 512) the padded
// signal is cut into hop-sized segments and a frame is the sum of R = frame_length/hop adjacent ones, so
// every sample is read once (the 2 * frame_length/2 padding samples of a clip a second time, by reflected
// index).  Otherwise ("direct form") a segment is a whole frame, R = 1.  Squares of fp32 samples are
// exact in fp64 and the sums are taken in fp64 in a fixed order (no atomics), so a sum depends on the
// order of its terms only in its last bits.
//
// Two launches, not one workgroup per clip: a corpus of a few long clips would leave most CUs idle with
// a workgroup per clip, and the segment sums that cross the launch boundary are 8 bytes per hop samples.
// Clip c's segment sums live at seg[wave_off[c] / hop + c * R ...]: a layout both kernels derive from
// wave_off alone (floor(a) + floor(b) <= floor(a + b), so consecutive clips never overlap).
#include "pca_common.h"

#include <cmath>

namespace pca {
namespace {

constexpr int kTrimWaves = 4;          // waves per workgroup of k_trim_segsum
constexpr int kTrimSegPerWave = 4;     // consecutive segments one wave sums

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One wave per segment; blockIdx.y = clip, blockIdx.x covers the segments of the longest clip.
// Segment j of a clip of L samples covers padded positions [j*hop, j*hop + seg_len), i.e. samples
// j*hop - pad + k, reflected about 0 and L - 1 (edge sample not repeated).
__global__ __launch_bounds__(256) void k_trim_segsum(const float* __restrict__ waves,
                                                      const int64_t* __restrict__ wave_off, int hop,
                                                      int seg_len, int pad, int R,
                                                      double* __restrict__ seg) {
  const int c = blockIdx.y;
  const int64_t w0 = wave_off[c];
  const int64_t L = wave_off[c + 1] - w0;
  const int64_t nseg = L / hop + R;
  const int lane = threadIdx.x & 63;
  const int64_t j0 = ((int64_t)blockIdx.x * kTrimWaves + (threadIdx.x >> 6)) * kTrimSegPerWave;
  if (j0 >= nseg || L <= pad) return;   // (uniform over the wave; L <= pad is rejected on the host)
  const float* __restrict__ y = waves + w0;
  double* __restrict__ out = seg + (w0 / hop + (int64_t)c * R);
  for (int s = 0; s < kTrimSegPerWave; ++s) {
    const int64_t j = j0 + s;
    if (j >= nseg) break;
    const int64_t a = j * hop - pad;    // first sample of the segment, before reflection
    double acc = 0.0;
    if (a >= 0 && a + seg_len <= L && (seg_len & 3) == 0 &&
        (reinterpret_cast<uintptr_t>(y + a) & 15) == 0) {
      const float4* __restrict__ v = reinterpret_cast<const float4*>(y + a);
      for (int k = lane; k < (seg_len >> 2); k += 64) {
        const float4 q = v[k];
        acc = fma((double)q.x, (double)q.x, acc);
        acc = fma((double)q.y, (double)q.y, acc);
        acc = fma((double)q.z, (double)q.z, acc);
        acc = fma((double)q.w, (double)q.w, acc);
      }
    } else {
      for (int k = lane; k < seg_len; k += 64) {
        int64_t i = a + k;
        if (i < 0) i = -i;
        if (i >= L) i = 2 * (L - 1) - i;
        i = i < 0 ? 0 : (i >= L ? L - 1 : i);   // in range already when L > pad
        const double q = (double)y[i];
        acc = fma(q, q, acc);
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) out[j] = acc;
  }
}

// One workgroup per clip.  mse[t] = (sum of R segment sums from t on) / frame_length;
// db[t] = 10 log10(max(1e-10, mse[t])) - 10 log10(max(1e-10, max_t mse[t])); frame t is non-silent iff
// db[t] > -top_db.  bounds[c] = (first * hop, min(L, (last + 1) * hop)), or (0, 0) without such a frame.
__global__ __launch_bounds__(256) void k_trim_bounds(const int64_t* __restrict__ wave_off, int hop,
                                                      int frame_length, int R, double top_db,
                                                      const double* __restrict__ seg,
                                                      int64_t* __restrict__ bounds) {
  __shared__ double red_m[256];
  __shared__ int64_t red_lo[256];
  __shared__ int64_t red_hi[256];
  const int c = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t w0 = wave_off[c];
  const int64_t L = wave_off[c + 1] - w0;
  const int64_t T = 1 + L / hop;
  const double* __restrict__ s = seg + (w0 / hop + (int64_t)c * R);
  const double amin = 1.0e-10;
  const double n = (double)frame_length;

  double m = 0.0;
  for (int64_t t = tid; t < T; t += 256) {
    double f = 0.0;
    for (int r = 0; r < R; ++r) f += s[t + r];
    m = fmax(m, f / n);
  }
  red_m[tid] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red_m[tid] = fmax(red_m[tid], red_m[tid + o]);
    __syncthreads();
  }
  const double ref_db = 10.0 * log10(fmax(amin, red_m[0]));

  int64_t lo = T, hi = -1;
  for (int64_t t = tid; t < T; t += 256) {
    double f = 0.0;
    for (int r = 0; r < R; ++r) f += s[t + r];
    const double db = 10.0 * log10(fmax(amin, f / n)) - ref_db;
    if (db > -top_db) {
      lo = t < lo ? t : lo;
      hi = t > hi ? t : hi;
    }
  }
  red_lo[tid] = lo;
  red_hi[tid] = hi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      red_lo[tid] = red_lo[tid + o] < red_lo[tid] ? red_lo[tid + o] : red_lo[tid];
      red_hi[tid] = red_hi[tid + o] > red_hi[tid] ? red_hi[tid + o] : red_hi[tid];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int64_t first = red_lo[0], last = red_hi[0];
    int64_t start = 0, end = 0;
    if (last >= 0) {
      start = first * hop;
      end = (last + 1) * hop;
      end = end < L ? end : L;
    }
    bounds[2 * c] = start;
    bounds[2 * c + 1] = end;
  }
}

// segments per frame: frame_length / hop when hop divides frame_length / 2, else 1 (direct form)
inline int trim_R(int frame_length, int hop) {
  return (frame_length / 2) % hop == 0 ? frame_length / hop : 1;
}

inline bool trim_geom_ok(int frame_length, int hop) {
  return frame_length >= 2 && frame_length <= 8192 && (frame_length & 1) == 0 && hop >= 1;
}

}  // namespace
}  // namespace pca

extern "C" {

size_t pca_trim_ws_bytes(int64_t total_len, int n_clips, int frame_length, int hop_length) {
  if (total_len <= 0 || n_clips <= 0 || n_clips > 65535 ||
      !pca::trim_geom_ok(frame_length, hop_length))
    return 0;
  const int64_t nseg = total_len / hop_length + (int64_t)n_clips * pca::trim_R(frame_length, hop_length);
  return pca::align256((size_t)nseg * sizeof(double));
}

int pca_trim_bounds(const float* waves, const int64_t* wave_off, int n_clips, int64_t max_len,
                    int64_t min_len, int frame_length, int hop_length, double top_db,
                    int64_t* bounds, void* ws, void* stream) {
  PCA_REQUIRE(waves && wave_off && bounds && ws, "trim_bounds: null pointer");
  PCA_REQUIRE(n_clips > 0 && n_clips <= 65535, "trim_bounds: n_clips=%d", n_clips);
  PCA_REQUIRE(frame_length >= 2 && frame_length <= 8192 && (frame_length & 1) == 0,
              "trim_bounds: frame_length=%d must be even and in [2, 8192]", frame_length);
  PCA_REQUIRE(hop_length >= 1, "trim_bounds: hop_length=%d", hop_length);
  PCA_REQUIRE(std::isfinite(top_db), "trim_bounds: top_db=%g must be finite", top_db);
  PCA_REQUIRE(min_len > frame_length / 2 && max_len >= min_len,
              "trim_bounds: reflect padding needs every clip longer than frame_length/2 "
              "(shortest %lld, longest %lld)", (long long)min_len, (long long)max_len);
  const int R = pca::trim_R(frame_length, hop_length);
  const int seg_len = R == 1 ? frame_length : hop_length;
  const int64_t max_nseg = max_len / hop_length + R;
  const int64_t gx = pca::cdiv(max_nseg, pca::kTrimWaves * pca::kTrimSegPerWave);
  PCA_REQUIRE(gx <= 0x7fffffffLL, "trim_bounds: %lld segments in the longest clip",
              (long long)max_nseg);
  hipStream_t st = pca::as_stream(stream);
  double* seg = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(pca::k_trim_segsum, dim3((unsigned)gx, (unsigned)n_clips), dim3(256), 0, st,
                     waves, wave_off, hop_length, seg_len, frame_length / 2, R, seg);
  PCA_TRY(pca::check_launch("k_trim_segsum"));
  hipLaunchKernelGGL(pca::k_trim_bounds, dim3((unsigned)n_clips), dim3(256), 0, st, wave_off,
                     hop_length, frame_length, R, top_db, (const double*)seg, bounds);
  return pca::check_launch("k_trim_bounds");
}
}
