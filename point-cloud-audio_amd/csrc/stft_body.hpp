// One STFT frame in LDS, shared by k_stft_logmag (features.hip: the whole-corpus pre-pass),
// k_frame_points (frame_points.hip: frames cut from the resident waveform per batch),
// k_frame_points_ex (frame_points_ex.hip: the same with speed change and background mix) and
// k_frame_points_reassigned (frame_points_reassigned.hip: the same frame, its points moved to their
// reassigned coordinates by one more transform in the same LDS), so that all give the same bits for the
// same frame.
//
// In-place radix-2 decimation-in-time FFT in float64: librosa computes the transform in double
// (numpy.fft) and only then rounds to complex64, so matching it to ~1e-7 in log-magnitude --
// including the near-silent bins that the log(1e-8 + .) floor amplifies -- needs double butterflies.
// LDS: n_fft complex doubles (data) + n_fft/2 (twiddles) = 24 B * n_fft (96 KiB at n_fft = 4096).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pca {

inline size_t stft_lds_bytes(int n_fft) { return ((size_t)n_fft + n_fft / 2) * sizeof(double2); }

// The frame comes in two stages so that a kernel can supply its own samples (frame_points_ex.hip
// resamples and mixes them on the way in): a load stage that fills tw and the bit-reversed, windowed
// x, and the butterfly stage.  stft_frame_fft is the two back to back with the plain load.

// tw[k] = exp(-2 pi i k / n_fft), k < n_fft/2
__device__ __forceinline__ void stft_twiddles(double2* tw, int n_fft, int tid) {
  const int half = n_fft >> 1;
  for (int k = tid; k < half; k += 256) {
    double sn, cs;
    sincospi(-2.0 * (double)k / (double)n_fft, &sn, &cs);
    tw[k] = make_double2(cs, sn);
  }
}

// sample n of the frame -> its bit-reversed slot of x, times the periodic Hann of win_length samples
// centred and zero-padded to n_fft, times `gain`
__device__ __forceinline__ void stft_store_sample(double2* x, int n, float sample, int n_fft, int log2n,
                                                  int win_length, double gain) {
  const int lpad = (n_fft - win_length) / 2;
  const int nw = n - lpad;
  double w = 0.0;
  if (nw >= 0 && nw < win_length)
    w = 0.5 - 0.5 * cospi(2.0 * (double)nw / (double)win_length);   // periodic Hann
  const int r = (int)(__brev((unsigned)n) >> (32 - log2n));          // bit-reversed slot
  x[r] = make_double2((double)sample * w * gain, 0.0);
}

// index i of a signal of L samples under reflect padding (numpy's "reflect": the edge sample is not
// repeated)
__device__ __forceinline__ int64_t stft_reflect(int64_t src, int64_t L) {
  if (src < 0) src = -src;
  if (src >= L) src = 2 * (L - 1) - src;
  if (src < 0) src = 0;  // only reachable when L <= n_fft/2 (rejected on the host)
  return src;
}

// Load stage: the n_fft samples of the reflect-padded signal that begin at `start` (a frame of
// centre c begins at c - n_fft/2).  No barrier: the butterfly stage begins with one.
__device__ __forceinline__ void stft_frame_load(double2* x, double2* tw,
                                                const float* __restrict__ wave, int64_t L,
                                                int64_t start, int n_fft, int log2n, int win_length,
                                                double gain, int tid) {
  stft_twiddles(tw, n_fft, tid);
  for (int n = tid; n < n_fft; n += 256)
    stft_store_sample(x, n, wave[stft_reflect(start + n, L)], n_fft, log2n, win_length, gain);
}

// Butterfly stage: in-place transform of the loaded frame.  256 threads; on return x[f] holds bin f
// and the workgroup is past a barrier.
__device__ __forceinline__ void stft_frame_butterflies(double2* x, const double2* tw, int n_fft,
                                                       int log2n, int tid) {
  const int half = n_fft >> 1;
  __syncthreads();

  for (int s = 1; s <= log2n; ++s) {
    const int hm = 1 << (s - 1);               // half butterfly span
    const int tstride = n_fft >> s;            // twiddle index stride
    for (int j = tid; j < half; j += 256) {
      const int k = j & (hm - 1);
      const int i0 = ((j - k) << 1) + k;
      const int i1 = i0 + hm;
      const double2 w = tw[k * tstride];
      const double2 a = x[i0];
      const double2 b = x[i1];
      const double2 bw = make_double2(b.x * w.x - b.y * w.y, b.x * w.y + b.y * w.x);
      x[i0] = make_double2(a.x + bw.x, a.y + bw.y);
      x[i1] = make_double2(a.x - bw.x, a.y - bw.y);
    }
    __syncthreads();
  }
}

// Transform of the n_fft samples of the reflect-padded signal that begin at `start`, times the
// periodic Hann of win_length samples centred and zero-padded to n_fft, times `gain` (1.0: an exact
// no-op).  256 threads; x[n_fft] and tw[n_fft/2] are LDS; on return x[f] holds bin f and the
// workgroup is past a barrier.
__device__ __forceinline__ void stft_frame_fft(double2* x, double2* tw,
                                               const float* __restrict__ wave, int64_t L,
                                               int64_t start, int n_fft, int log2n, int win_length,
                                               double gain, int tid) {
  stft_frame_load(x, tw, wave, L, start, n_fft, log2n, win_length, gain, tid);
  stft_frame_butterflies(x, tw, n_fft, log2n, tid);
}

// Load stage of the transform that time-frequency reassignment adds (frame_points_reassigned.hip): the
// same samples, window position and gain as stft_frame_load, packed as one complex sequence
//   z[n] = x th / n_fft + i x dh,   x = sample * gain,  h = the periodic Hann of stft_store_sample,
//   th[n] = (n - n_fft/2) h[n],     dh[n] = (pi / w) sin(2 pi nw / w) inside the window, 0 outside.
// th is scaled by the exact power of two 1/n_fft so that the two halves have comparable magnitude and
// neither loses bits to the other in the butterflies.  tw is left as stft_frame_load filled it.  No barrier.
__device__ __forceinline__ void stft_reassign_load(double2* x, const float* __restrict__ wave, int64_t L,
                                                   int64_t start, int n_fft, int log2n, int win_length,
                                                   double gain, int tid) {
  const int lpad = (n_fft - win_length) / 2;
  const double inv_n = 1.0 / (double)n_fft;
  for (int n = tid; n < n_fft; n += 256) {
    const int nw = n - lpad;
    double h = 0.0, dh = 0.0;
    if (nw >= 0 && nw < win_length) {
      double sn, cs;
      sincospi(2.0 * (double)nw / (double)win_length, &sn, &cs);
      h = 0.5 - 0.5 * cs;
      dh = (3.14159265358979323846 / (double)win_length) * sn;
    }
    const double s = (double)wave[stft_reflect(start + n, L)] * gain;
    const int r = (int)(__brev((unsigned)n) >> (32 - log2n));
    x[r] = make_double2(s * ((double)(n - n_fft / 2) * inv_n * h), s * dh);
  }
}

// The spectra of the two real sequences packed by stft_reassign_load, for bin k <= n_fft/2 of the
// transformed z: th = X_th[k] / n_fft, dh = X_dh[k].
__device__ __forceinline__ void stft_reassign_split(const double2* z, int k, int n_fft, double2* th,
                                                    double2* dh) {
  const double2 a = z[k], b = z[(n_fft - k) & (n_fft - 1)];
  *th = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
  *dh = make_double2(0.5 * (a.y + b.y), -0.5 * (a.x - b.x));
}

// log(1e-8 + |v| * inv) of one bin, inv = 1 / norm
__device__ __forceinline__ float stft_logmag_bin(double2 v, double inv) {
  // the reference rounds the spectrum to complex64 before |.| (librosa dtype=complex64)
  const float re = (float)(v.x * inv), im = (float)(v.y * inv);
  const float mag = sqrtf(re * re + im * im);
  return logf(1.0e-8f + mag);
}

}  // namespace pca
