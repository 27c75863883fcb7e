// Point sets framed from the resident waveforms with every point moved to where its energy lies:
// time-frequency reassignment (Auger-Flandrin; the form of librosa.reassigned_spectrogram).
//
// Replaces: nothing - no reference counterpart (the reference keeps grid points only).
// k_frame_points writes (farr[f], [tarr[j],] value) rows; here a bin that carries energy is written at its
// instantaneous frequency and group delay instead, with the same value.  A stationary partial collapses
// onto its true frequency, a click onto its true time.  The slot's clip, shift, level and window are
// derived exactly as k_frame_points derives them, and X_h is stft_frame_fft's transform, so the value
// column, the labels and meta are that launch's bits.
// Per frame: the transform of x h as before, whose bins each thread keeps in registers (bins tid + 256 i,
// at most 9), then ONE more complex transform of z = x th + i x dh in the same LDS with the same
// twiddles; X_th and X_dh separate by conjugate symmetry (stft_reassign_split).  LDS stays 24 B * n_fft;
// the samples are read twice (the second time from L2), n_bins rows are written.
#include "pca_common.h"
#include "select_keys.hpp"
#include "stft_body.hpp"

#include <math.h>

#include <mutex>

namespace pca {
namespace {

struct ReassignJob {
  const float* waves;
  const int64_t *wave_off, *set_off, *clip_labels, *idx;
  const float *farr, *tarr;
  const int32_t *win_lengths, *draw_dev;
  float* out;
  int64_t* labels_out;
  int32_t* meta_out;
  uint64_t seed, draw;
  int n_clips, n_fft, log2n, hop, n_bins, Nt, jitter, n_win, norm_mode;
  float gain_db;
  int axes;
  float rel_floor, abs_floor, max_df, max_dt, strength;
};

// Bins per thread, bins tid + 256 q: the kernel is built for 2, 3, 5 and 9 = ceil((4096/2 + 1) / 256), so
// that a launch keeps only as many X_h in registers as its n_bins needs (n_fft 1024: 2 or 3).

// draw number k of a slot's stream, as k_frame_points: 0 time shift, 1 level, 2 window length
__device__ __forceinline__ uint64_t frame_draw(uint64_t stream, int k) {
  return mix64(stream + (uint64_t)k * 0xd1342543de82ef95ull);
}

// Workgroup (j, b): frame j of the set in batch slot b.
template <int kBinsPerThread>
__global__ __launch_bounds__(256) void k_frame_points_reassigned(const ReassignJob a) {
  extern __shared__ __attribute__((aligned(16))) double2 lds_c[];
  double2* x = lds_c;                   // [n_fft]
  double2* tw = lds_c + a.n_fft;        // [n_fft/2]
  const int tid = threadIdx.x, j = blockIdx.x, b = blockIdx.y;

  // the slot, exactly as k_frame_points derives it
  const int64_t total = a.set_off[a.n_clips];
  if (total <= 0) return;               // (uniform) a corpus that yields no set
  int64_t i = a.idx[b];
  i = i < 0 ? 0 : (i >= total ? total - 1 : i);
  int lo = 0, hi = a.n_clips;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (a.set_off[m] > i) hi = m; else lo = m + 1;
  }
  const int c = lo > 0 ? lo - 1 : 0;
  const int64_t s = i - a.set_off[c];
  const int64_t w0 = a.wave_off[c];
  const int64_t L = a.wave_off[c + 1] - w0;

  uint64_t draw = a.draw;
  if (a.draw_dev != nullptr) draw += (uint64_t)(uint32_t)a.draw_dev[0];
  const uint64_t stream = select_stream(a.seed, draw, i, b);
  int64_t delta = 0;
  if (a.jitter > 0) {
    const uint64_t r = frame_draw(stream, 0) >> 32;
    delta = (int64_t)((r * (uint64_t)(2 * (int64_t)a.jitter + 1)) >> 32) - a.jitter;
  }
  float g = 1.0f;
  if (a.gain_db > 0.f) {
    const double u = (double)(frame_draw(stream, 1) >> 11) * (2.0 / 9007199254740992.0) - 1.0;  // [-1, 1)
    g = (float)exp2(u * (double)a.gain_db * 0.16609640474436813);          // 10^(u dB / 20)
  }
  int wi = 0;
  if (a.n_win > 1) wi = (int)(((frame_draw(stream, 2) >> 32) * (uint64_t)a.n_win) >> 32);
  int win = a.win_lengths[wi];
  win = win < 1 ? 1 : (win > a.n_fft ? a.n_fft : win);

  const int64_t first = s * a.Nt * a.hop + delta;
  int64_t centre = first + (int64_t)j * a.hop;
  centre = centre < 0 ? 0 : (centre > L ? L : centre);
  if (j == 0 && tid == 0) {
    if (a.clip_labels != nullptr && a.labels_out != nullptr) a.labels_out[b] = a.clip_labels[c];
    if (a.meta_out != nullptr) {
      int32_t* m = a.meta_out + (int64_t)b * 4;
      m[0] = c;
      m[1] = (int32_t)centre;
      m[2] = win;
      m[3] = (int32_t)__float_as_uint(g);
    }
  }

  const float* wave = a.waves + w0;
  const int64_t start = centre - a.n_fft / 2;
  stft_frame_fft(x, tw, wave, L, start, a.n_fft, a.log2n, win, (double)g, tid);

  // X_h of this thread's bins and their values, into registers; the frame's maximum value
  const double inv = 1.0 / (double)(a.norm_mode == 0 ? a.n_fft : win);
  double2 xh[kBinsPerThread];
  float v[kBinsPerThread];
  float vmax = -INFINITY;
#pragma unroll
  for (int q = 0; q < kBinsPerThread; ++q) {
    const int f = tid + 256 * q;
    xh[q] = make_double2(0.0, 0.0);
    v[q] = 0.f;
    if (f < a.n_bins) {
      xh[q] = x[f];
      v[q] = stft_logmag_bin(xh[q], inv);
      vmax = fmaxf(vmax, v[q]);          // fmaxf drops a NaN: NaN loses
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64));
  __syncthreads();                       // every bin of x is in registers: x is free
  float* red = reinterpret_cast<float*>(x);
  if ((tid & 63) == 0) red[tid >> 6] = vmax;
  __syncthreads();
  vmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();                       // red is read: x may be loaded again

  // the second transform: z = x th / n_fft + i x dh, twiddles reused
  stft_reassign_load(x, wave, L, start, a.n_fft, a.log2n, win, (double)g, tid);
  stft_frame_butterflies(x, tw, a.n_fft, a.log2n, tid);

  const float thr = vmax - a.rel_floor;  // one fp32 subtraction
  const bool do_f = (a.axes & 1) != 0, do_t = (a.axes & 2) != 0;
  const double max_df = (double)a.max_df, max_dt = (double)a.max_dt, strength = (double)a.strength;
  const double kf = (double)a.n_fft * 0.15915494309189533577;   // n_fft / (2 pi)
  const double kt = (double)a.n_fft / (double)a.hop;            // undoes the load's 1/n_fft, per hop
  const int64_t p0 = ((int64_t)b * a.Nt + j) * a.n_bins;        // point p = j*n_bins + f
  const float tgrid = a.tarr != nullptr ? a.tarr[j] : 0.f;
#pragma unroll
  for (int q = 0; q < kBinsPerThread; ++q) {
    const int f = tid + 256 * q;
    if (f < a.n_bins) {
      float fo = a.farr[f], to = tgrid;
      const double2 H = xh[q];
      const double p = H.x * H.x + H.y * H.y;
      if (v[q] >= thr && v[q] >= a.abs_floor && p > 0.0) {
        double2 th, dh;
        stft_reassign_split(x, f, a.n_fft, &th, &dh);
        const double db = -(dh.y * H.x - dh.x * H.y) / p * kf;
        const double dt = (th.x * H.x + th.y * H.y) / p * kt;
        if (isfinite(db) && isfinite(dt)) {
          if (do_f) {
            const double sh = strength * fmin(fmax(db, -max_df), max_df);
            if (sh != 0.0) {
              const double pos = fmin(fmax((double)f + sh, 0.0), (double)(a.n_bins - 1));
              int k = (int)floor(pos);
              k = k > a.n_bins - 2 ? a.n_bins - 2 : k;
              const double f0 = (double)a.farr[k], f1 = (double)a.farr[k + 1];
              fo = (float)(f0 + (pos - (double)k) * (f1 - f0));
            }
          }
          if (do_t) {
            const double sh = strength * fmin(fmax(dt, -max_dt), max_dt);
            if (sh != 0.0) {
              const double pos = (double)j + sh;
              int k = (int)floor(pos);
              k = k < 0 ? 0 : (k > a.Nt - 2 ? a.Nt - 2 : k);
              const double t0 = (double)a.tarr[k], t1 = (double)a.tarr[k + 1];
              to = (float)(t0 + (pos - (double)k) * (t1 - t0));
            }
          }
        }
      }
      if (a.tarr == nullptr) {
        reinterpret_cast<float2*>(a.out)[p0 + f] = make_float2(fo, v[q]);
      } else {
        float* o = a.out + (p0 + f) * 3;
        o[0] = fo;
        o[1] = to;
        o[2] = v[q];
      }
    }
  }
}

template <int kBinsPerThread>
void launch_reassigned(const ReassignJob& j, int B, void* stream) {
  static std::once_flag lds_once;   // allow > 64 KiB of dynamic LDS (96 KiB at n_fft 4096)
  std::call_once(lds_once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_frame_points_reassigned<kBinsPerThread>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
  });
  hipLaunchKernelGGL(k_frame_points_reassigned<kBinsPerThread>, dim3((unsigned)j.Nt, (unsigned)B),
                     dim3(256), stft_lds_bytes(j.n_fft), as_stream(stream), j);
}

}  // namespace
}  // namespace pca

extern "C" {

int pca_frame_points_reassigned(const float* waves, const int64_t* wave_off, const int64_t* set_off,
                                int n_clips, int64_t max_len, int64_t min_len,
                                const int64_t* clip_labels, const int64_t* idx, int B, int n_fft, int hop,
                                int n_bins, int Nt, const float* farr, const float* tarr,
                                const PcaFrameAug* aug, const PcaReassignSpec* spec, float* out,
                                int64_t* labels_out, int32_t* meta_out, void* stream) {
  PCA_REQUIRE(waves && wave_off && set_off && idx && farr && aug && out,
              "frame_points_reassigned: null pointer");
  PCA_REQUIRE(spec != nullptr, "frame_points_reassigned: null spec");
  PCA_REQUIRE(aug->win_lengths != nullptr, "frame_points_reassigned: null win_lengths");
  PCA_REQUIRE((clip_labels == nullptr) == (labels_out == nullptr),
              "frame_points_reassigned: clip_labels and labels_out go together");
  PCA_REQUIRE(n_clips > 0, "frame_points_reassigned: n_clips=%d", n_clips);
  PCA_REQUIRE(n_fft >= 64 && n_fft <= 4096 && (n_fft & (n_fft - 1)) == 0,
              "frame_points_reassigned: n_fft=%d must be a power of two in [64, 4096]", n_fft);
  PCA_REQUIRE(hop > 0, "frame_points_reassigned: hop=%d", hop);
  PCA_REQUIRE(n_bins >= 2 && n_bins <= n_fft / 2 + 1,
              "frame_points_reassigned: n_bins=%d (the frequency axis is interpolated: at least 2)", n_bins);
  PCA_REQUIRE(B > 0 && B <= 65535 && Nt > 0, "frame_points_reassigned: B=%d Nt=%d", B, Nt);
  PCA_REQUIRE((int64_t)Nt * n_bins <= 16384,
              "frame_points_reassigned: %lld points per set (max 16384)", (long long)Nt * n_bins);
  PCA_REQUIRE(min_len > n_fft / 2 && max_len >= min_len,
              "frame_points_reassigned: reflect padding needs every clip longer than n_fft/2 "
              "(shortest %lld, longest %lld)", (long long)min_len, (long long)max_len);
  PCA_REQUIRE(max_len <= INT32_MAX,
              "frame_points_reassigned: a clip of %lld samples (meta holds int32 centres)",
              (long long)max_len);
  PCA_REQUIRE(aug->jitter >= 0 && aug->jitter <= (1 << 30), "frame_points_reassigned: jitter=%d",
              aug->jitter);
  PCA_REQUIRE(aug->gain_db >= 0.f && aug->gain_db <= 200.f,
              "frame_points_reassigned: gain_db=%g must be finite and in [0, 200]", (double)aug->gain_db);
  PCA_REQUIRE(aug->n_win >= 1, "frame_points_reassigned: n_win=%d", aug->n_win);
  PCA_REQUIRE(aug->norm_mode == 0 || aug->norm_mode == 1, "frame_points_reassigned: norm_mode=%d",
              aug->norm_mode);
  PCA_REQUIRE(spec->axes >= 1 && spec->axes <= 3, "frame_points_reassigned: axes=%d must be 1..3",
              spec->axes);
  PCA_REQUIRE(!(spec->axes & 2) || (tarr != nullptr && Nt >= 2),
              "frame_points_reassigned: the time axis needs tarr and Nt >= 2 (Nt=%d)", Nt);
  PCA_REQUIRE(spec->rel_floor >= 0.f, "frame_points_reassigned: rel_floor=%g must be >= 0 (+inf = off)",
              (double)spec->rel_floor);
  PCA_REQUIRE(!isnan(spec->abs_floor), "frame_points_reassigned: abs_floor is NaN");
  PCA_REQUIRE(spec->max_df > 0.f && spec->max_df <= 64.f,
              "frame_points_reassigned: max_df=%g must be in (0, 64]", (double)spec->max_df);
  PCA_REQUIRE(spec->max_dt > 0.f && spec->max_dt <= 4.f,
              "frame_points_reassigned: max_dt=%g must be in (0, 4]", (double)spec->max_dt);
  PCA_REQUIRE(spec->strength >= 0.f && spec->strength <= 1.f,
              "frame_points_reassigned: strength=%g must be in [0, 1]", (double)spec->strength);
  pca::ReassignJob j{};
  j.waves = waves; j.wave_off = wave_off; j.set_off = set_off; j.clip_labels = clip_labels;
  j.idx = idx; j.farr = farr; j.tarr = tarr; j.win_lengths = aug->win_lengths;
  j.draw_dev = aug->draw_dev; j.out = out; j.labels_out = labels_out; j.meta_out = meta_out;
  j.seed = aug->seed; j.draw = aug->draw; j.n_clips = n_clips; j.n_fft = n_fft; j.hop = hop;
  j.n_bins = n_bins; j.Nt = Nt; j.jitter = aug->jitter; j.n_win = aug->n_win;
  j.norm_mode = aug->norm_mode; j.gain_db = aug->gain_db;
  j.axes = spec->axes; j.rel_floor = spec->rel_floor; j.abs_floor = spec->abs_floor;
  j.max_df = spec->max_df; j.max_dt = spec->max_dt; j.strength = spec->strength;
  while ((1 << j.log2n) < n_fft) ++j.log2n;
  if (n_bins <= 512) pca::launch_reassigned<2>(j, B, stream);
  else if (n_bins <= 768) pca::launch_reassigned<3>(j, B, stream);
  else if (n_bins <= 1280) pca::launch_reassigned<5>(j, B, stream);
  else pca::launch_reassigned<9>(j, B, stream);
  return pca::check_launch("k_frame_points_reassigned");
}
}
