// k_frame_points (frame_points.hip) with two more augmentations applied to the samples while the frame
// is loaded into LDS: a speed change (the clip resampled by one of a few ratios, which moves its content
// along the frequency axis the point sets carry) and a background mix (another clip added at a drawn
// signal-to-noise ratio).  The reference has neither; a user would resample or mix whole clips on the
// host per epoch and rebuild the dataset.  Here a slot's samples are computed where they are consumed:
//   y[t]    the resampled clip, resample_body.hpp's sum for the samples the frame needs, never stored
//   sample  (float)(y + alpha * background), the background read circularly
// and from there the frame is k_frame_points': window, gain, fp64 FFT (stft_body.hpp), rows.
// The filter taps are read through L2 as k_resample reads them, not staged in LDS: of the three loads per
// tap two are table entries (scattered over a 128 KiB table by the fractional phase) and only one is a
// clip sample, which neighbouring lanes already share; the transform keeps its 24 B * n_fft of LDS.
// The set lookup and draws 0 - 2 restate k_frame_points' lines: that kernel stays as it is, its bits are
// pinned against the spectrogram pipeline, and the tests here pin the two kernels against each other.
// Also k_clip_rms: the per-clip RMS that scales the background.
// Last, the launch decides which points a set keeps: random frequency bands and time stripes (draws 8 -
// 23, point_mask.hpp) are left out of the rows (drop: the kept points compacted to the front, zeros behind
// them, the count in lengths_out) or written at a silent bin's value (floor).  With the masks off the code
// below takes the branches it always took.
#include "pca_common.h"
#include "point_mask.hpp"
#include "resample_body.hpp"
#include "select_keys.hpp"
#include "stft_body.hpp"

#include <math.h>

#include <cmath>
#include <mutex>

namespace pca {
namespace {

struct FrameJobEx {
  const float* waves;
  const int64_t *wave_off, *set_off, *clip_labels, *idx;
  const float *farr, *tarr;
  const int32_t *win_lengths, *draw_dev;
  float* out;
  int64_t* labels_out;
  int32_t* meta_out;
  float* samples_out;
  uint64_t seed, draw;
  int n_clips, n_fft, log2n, hop, n_bins, Nt, jitter, n_win, norm_mode;
  float gain_db;
  // speed
  int n_speed, nwin, num_table, speed_on;
  double ratios[PCA_FRAME_MAX_SPEEDS];
  const double* tables;
  // mix
  const float* bg_waves;             // nullptr: mixing off
  const int64_t* bg_off;
  const double *bg_rms, *clip_rms;
  int n_bg;
  // soft targets (all three or none): the background clip's label and the primary label's weight
  const int64_t* bg_labels;
  int64_t* labels2_out;
  float* weight_out;
  double mix_prob, snr_lo_db, snr_hi_db;
  // point masks: bands over the bins, stripes over the frames (a count of 0: that kind is off)
  int n_freq, freq_width, n_time, time_width, mask_floor;
  int32_t *lengths_out, *mask_meta_out;
};

// draw number k of a slot's stream, as k_frame_points: 0 time shift, 1 level, 2 window length; here also
// 3 speed index, 4 mix decision, 5 background clip, 6 its start, 7 the SNR, 8 - 15 the frequency bands,
// 16 - 23 the time stripes (point_mask.hpp)
__device__ __forceinline__ uint64_t frame_draw(uint64_t stream, int k) {
  return mix64(stream + (uint64_t)k * 0xd1342543de82ef95ull);
}
// uniform in [0, 1)
__device__ __forceinline__ double frame_unit(uint64_t r) {
  return (double)(r >> 11) * (1.0 / 9007199254740992.0);
}

// Workgroup (j, b): frame j of the set in batch slot b.  The Nt workgroups of a slot derive the same
// draws from the slot's stream, so a chunk's frames stay `hop` apart in the resampled clip's timeline.
__global__ __launch_bounds__(256) void k_frame_points_ex(const FrameJobEx a) {
  extern __shared__ __attribute__((aligned(16))) double2 lds_c[];
  double2* x = lds_c;                   // [n_fft]
  double2* tw = lds_c + a.n_fft;        // [n_fft/2]
  const int tid = threadIdx.x, j = blockIdx.x, b = blockIdx.y;

  const int64_t total = a.set_off[a.n_clips];
  if (total <= 0) return;               // (uniform) a corpus that yields no set
  int64_t i = a.idx[b];
  i = i < 0 ? 0 : (i >= total ? total - 1 : i);
  int lo = 0, hi = a.n_clips;           // first clip whose set_off exceeds i (set_off[n_clips] does)
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (a.set_off[m] > i) hi = m; else lo = m + 1;
  }
  const int c = lo > 0 ? lo - 1 : 0;    // set_off[c] <= i < set_off[c + 1]  (set_off[0] is 0)
  const int64_t s = i - a.set_off[c];
  const int64_t w0 = a.wave_off[c];
  const int64_t L = a.wave_off[c + 1] - w0;

  uint64_t draw = a.draw;
  if (a.draw_dev != nullptr) draw += (uint64_t)(uint32_t)a.draw_dev[0];   // device-side counter
  const uint64_t stream = select_stream(a.seed, draw, i, b);
  int64_t delta = 0;                    // draws 0 - 2: k_frame_points' arithmetic, bit for bit
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
  int win = a.win_lengths[wi];          // device values: clamped here, not checked on the host
  win = win < 1 ? 1 : (win > a.n_fft ? a.n_fft : win);

  int si = 0;
  if (a.speed_on) si = (int)(((frame_draw(stream, 3) >> 32) * (uint64_t)a.n_speed) >> 32);
  const double ratio = a.ratios[si];
  const bool resampled = ratio != 1.0;

  int c2 = -1;
  int64_t p = 0, b0 = 0, Lb = 0;
  float alpha = 0.f, wgt = 1.f;         // wgt: the primary clip's share of the amplitude
  if (a.bg_waves != nullptr && frame_unit(frame_draw(stream, 4)) < a.mix_prob) {
    const int k = (int)(((frame_draw(stream, 5) >> 32) * (uint64_t)a.n_bg) >> 32);
    b0 = a.bg_off[k];
    Lb = a.bg_off[k + 1] - b0;
    if (Lb > 0) {                       // (an empty background clip: the slot does not mix)
      c2 = k;
      p = (int64_t)__umul64hi(frame_draw(stream, 6), (uint64_t)Lb);
      const double snr = a.snr_lo_db + frame_unit(frame_draw(stream, 7)) * (a.snr_hi_db - a.snr_lo_db);
      const double rc = a.clip_rms[c], rb = a.bg_rms[k];
      if (rc > 0.0 && rb > 0.0) {
        const double u = exp2(-snr * 0.16609640474436813);            // 10^(-snr/20)
        alpha = (float)(rc / rb * u);
        if (alpha != 0.f) wgt = (float)(1.0 / (1.0 + u));
      }
    }
  }

  // which points the slot keeps: one set of bands for all Nt frames, one set of stripes
  const bool masked = a.n_freq > 0 || a.n_time > 0;
  MaskAxis mf, mt;
  int kept_bins = a.n_bins, kept_frames = a.Nt;
  bool frame_off = false;
  if (masked) {
    const auto draw_k = [stream](int k) { return frame_draw(stream, k); };
    mask_draw(mf, draw_k, 8, a.n_freq, a.freq_width, a.n_bins);
    mask_draw(mt, draw_k, 16, a.n_time, a.time_width, a.Nt);
    kept_bins -= mask_below(mf, a.n_bins);
    kept_frames -= mask_below(mt, a.Nt);
    frame_off = mask_covers(mt, j);
  }

  // centres in the timeline of the (resampled) clip y of Ly samples
  const int64_t nominal = s * a.Nt * a.hop + delta;
  const int64_t Ly = resampled ? (int64_t)((double)L * ratio) : L;
  const int64_t first = resampled ? (int64_t)floor((double)nominal * ratio + 0.5) : nominal;
  int64_t centre = first + (int64_t)j * a.hop;
  centre = centre < 0 ? 0 : (centre > Ly ? Ly : centre);
  if (j == 0 && tid == 0) {
    if (a.clip_labels != nullptr && a.labels_out != nullptr) a.labels_out[b] = a.clip_labels[c];
    if (a.labels2_out != nullptr) {     // (the host passes them with clip_labels only)
      a.labels2_out[b] = alpha != 0.f ? a.bg_labels[c2] : a.clip_labels[c];
      a.weight_out[b] = wgt;
    }
    if (a.meta_out != nullptr) {
      int32_t* m = a.meta_out + (int64_t)b * 8;
      m[0] = c;
      m[1] = (int32_t)centre;
      m[2] = win;
      m[3] = (int32_t)__float_as_uint(g);
      m[4] = si;
      m[5] = c2;
      m[6] = (int32_t)p;
      m[7] = (int32_t)__float_as_uint(alpha);
    }
    if (a.lengths_out != nullptr) a.lengths_out[b] = kept_frames * kept_bins;
    if (a.mask_meta_out != nullptr) {
      int32_t* m = a.mask_meta_out + (int64_t)b * (4 * PCA_POINT_MASK_MAX);
      for (int k = 0; k < PCA_POINT_MASK_MAX; ++k) {
        m[2 * k] = masked ? mf.start[k] : 0;
        m[2 * k + 1] = masked ? mf.width[k] : 0;
        m[2 * PCA_POINT_MASK_MAX + 2 * k] = masked ? mt.start[k] : 0;
        m[2 * PCA_POINT_MASK_MAX + 2 * k + 1] = masked ? mt.width[k] : 0;
      }
    }
  }

  const int din = a.tarr == nullptr ? 2 : 3;
  if (frame_off) {                      // (uniform) a frame a stripe masks: no load, no transform
    if (a.samples_out != nullptr) {
      float* so = a.samples_out + ((int64_t)b * a.Nt + j) * a.n_fft;
      for (int n = tid; n < a.n_fft; n += 256) so[n] = 0.f;
    }
    if (a.mask_floor) {                 // its rows in place, at a silent bin's value
      const float quiet = stft_logmag_bin(make_double2(0.0, 0.0), 1.0);
      float* o = a.out + ((int64_t)b * a.Nt + j) * a.n_bins * din;
      for (int f = tid; f < a.n_bins; f += 256) {
        o[f * din] = a.farr[f];
        if (din == 3) o[f * 3 + 1] = a.tarr[j];
        o[f * din + din - 1] = quiet;
      }
    } else {                            // its n_bins rows of the zero tail, behind the kept frames' shares
      const int64_t row0 = (int64_t)b * a.Nt * a.n_bins + (int64_t)kept_frames * a.n_bins +
                           (int64_t)mask_below(mt, j) * a.n_bins;
      float* o = a.out + row0 * din;
      for (int q = tid; q < a.n_bins * din; q += 256) o[q] = 0.f;
    }
    return;
  }

  const float* wave = a.waves + w0;
  const int64_t start = centre - a.n_fft / 2;
  if (!resampled && alpha == 0.f && a.samples_out == nullptr) {
    stft_frame_load(x, tw, wave, L, start, a.n_fft, a.log2n, win, (double)g, tid);   // k_frame_points' load
  } else {
    stft_twiddles(tw, a.n_fft, tid);
    const double* twin = resampled ? a.tables + (int64_t)si * 2 * a.nwin : nullptr;
    const float* bg = a.bg_waves + b0;
    const int64_t q = (p + (int64_t)j * a.hop) % (Lb > 0 ? Lb : 1);   // background index of sample 0
    float* so = a.samples_out == nullptr
                    ? nullptr : a.samples_out + ((int64_t)b * a.Nt + j) * a.n_fft;
    for (int n = tid; n < a.n_fft; n += 256) {
      const int64_t src = stft_reflect(start + n, Ly);
      float v = resampled ? resample_sample(wave, L, ratio, twin, twin + a.nwin, a.nwin, a.num_table,
                                            1.0f, src)
                          : wave[src];
      if (alpha != 0.f) v = (float)((double)v + (double)alpha * (double)bg[(q + n) % Lb]);
      if (so != nullptr) so[n] = v;
      stft_store_sample(x, n, v, a.n_fft, a.log2n, win, (double)g);
    }
  }
  stft_frame_butterflies(x, tw, a.n_fft, a.log2n, tid);

  const double inv = 1.0 / (double)(a.norm_mode == 0 ? a.n_fft : win);
  const int64_t p0 = ((int64_t)b * a.Nt + j) * a.n_bins;            // point p = j*n_bins + f
  if (masked) {
    const float t = din == 3 ? a.tarr[j] : 0.f;
    if (a.mask_floor) {
      const float quiet = stft_logmag_bin(make_double2(0.0, 0.0), inv);
      float* o = a.out + p0 * din;
      for (int f = tid; f < a.n_bins; f += 256) {
        o[f * din] = a.farr[f];
        if (din == 3) o[f * 3 + 1] = t;
        o[f * din + din - 1] = mask_covers(mf, f) ? quiet : stft_logmag_bin(x[f], inv);
      }
    } else {
      // kept frame of rank r: rows [r * kept_bins, (r + 1) * kept_bins) of the slot, bin f at its rank
      // among the kept bins; then the n_bins - kept_bins rows of the zero tail that are this frame's share
      const int r = j - mask_below(mt, j);
      const int64_t slot = (int64_t)b * a.Nt * a.n_bins;
      float* o = a.out + (slot + (int64_t)r * kept_bins) * din;
      for (int f = tid; f < a.n_bins; f += 256) {
        if (mask_covers(mf, f)) continue;
        const int q = f - mask_below(mf, f);
        o[q * din] = a.farr[f];
        if (din == 3) o[q * 3 + 1] = t;
        o[q * din + din - 1] = stft_logmag_bin(x[f], inv);
      }
      const int spare = a.n_bins - kept_bins;
      float* z = a.out + (slot + (int64_t)kept_frames * kept_bins + (int64_t)r * spare) * din;
      for (int q = tid; q < spare * din; q += 256) z[q] = 0.f;
    }
  } else if (a.tarr == nullptr) {
    float2* o = reinterpret_cast<float2*>(a.out) + p0;
    for (int f = tid; f < a.n_bins; f += 256) o[f] = make_float2(a.farr[f], stft_logmag_bin(x[f], inv));
  } else {
    const float t = a.tarr[j];
    float* o = a.out + p0 * 3;
    for (int f = tid; f < a.n_bins; f += 256) {
      o[f * 3 + 0] = a.farr[f];
      o[f * 3 + 1] = t;
      o[f * 3 + 2] = stft_logmag_bin(x[f], inv);
    }
  }
}

// One workgroup per clip: thread t sums the squares of samples t, t + 256, ... in fp64 (a square of an
// fp32 sample is exact there), then the 256 partial sums are added pairwise in LDS - a fixed order.
__global__ __launch_bounds__(256) void k_clip_rms(const float* __restrict__ waves,
                                                  const int64_t* __restrict__ wave_off,
                                                  double* __restrict__ rms_out) {
  __shared__ double part[256];
  const int tid = threadIdx.x, c = blockIdx.x;
  const int64_t w0 = wave_off[c];
  const int64_t L = wave_off[c + 1] - w0;
  double acc = 0.0;
  for (int64_t n = tid; n < L; n += 256) {
    const double v = (double)waves[w0 + n];
    acc += v * v;
  }
  part[tid] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) part[tid] += part[tid + h];
    __syncthreads();
  }
  if (tid == 0) rms_out[c] = L > 0 ? sqrt(part[0] / (double)L) : 0.0;
}

}  // namespace
}  // namespace pca

extern "C" {

int pca_clip_rms(const float* waves, const int64_t* wave_off, int n_clips, int64_t max_len,
                 double* rms_out, void* stream) {
  PCA_REQUIRE(waves && wave_off && rms_out, "clip_rms: null pointer");
  PCA_REQUIRE(n_clips > 0, "clip_rms: n_clips=%d", n_clips);
  PCA_REQUIRE(max_len >= 0, "clip_rms: max_len=%lld", (long long)max_len);
  hipLaunchKernelGGL(pca::k_clip_rms, dim3((unsigned)n_clips), dim3(256), 0, pca::as_stream(stream),
                     waves, wave_off, rms_out);
  return pca::check_launch("k_clip_rms");
}

int pca_frame_points_masked(const float* waves, const int64_t* wave_off, const int64_t* set_off,
                            int n_clips, int64_t max_len, int64_t min_len, const int64_t* clip_labels,
                            const int64_t* idx, int B, int n_fft, int hop, int n_bins, int Nt,
                            const float* farr, const float* tarr, const PcaFrameAugEx* aug, float* out,
                            int64_t* labels_out, int32_t* meta_out, float* samples_out,
                            const int64_t* bg_labels, int64_t* labels2_out, float* weight_out,
                            const PcaPointMask* mask, int32_t* lengths_out, int32_t* mask_meta_out,
                            void* stream) {
  // everything pca_frame_points refuses
  PCA_REQUIRE(waves && wave_off && set_off && idx && farr && aug && out,
              "frame_points_ex: null pointer");
  PCA_REQUIRE(aug->win_lengths != nullptr, "frame_points_ex: null win_lengths");
  PCA_REQUIRE((clip_labels == nullptr) == (labels_out == nullptr),
              "frame_points_ex: clip_labels and labels_out go together");
  PCA_REQUIRE((bg_labels == nullptr) == (labels2_out == nullptr) &&
                  (bg_labels == nullptr) == (weight_out == nullptr),
              "frame_points_ex: bg_labels, labels2_out and weight_out go together");
  PCA_REQUIRE(bg_labels == nullptr || clip_labels != nullptr,
              "frame_points_ex: the soft targets need clip_labels and labels_out");
  PCA_REQUIRE(n_clips > 0, "frame_points_ex: n_clips=%d", n_clips);
  PCA_REQUIRE(n_fft >= 64 && n_fft <= 4096 && (n_fft & (n_fft - 1)) == 0,
              "frame_points_ex: n_fft=%d must be a power of two in [64, 4096]", n_fft);
  PCA_REQUIRE(hop > 0, "frame_points_ex: hop=%d", hop);
  PCA_REQUIRE(n_bins > 0 && n_bins <= n_fft / 2 + 1, "frame_points_ex: n_bins=%d", n_bins);
  PCA_REQUIRE(B > 0 && B <= 65535 && Nt > 0, "frame_points_ex: B=%d Nt=%d", B, Nt);
  PCA_REQUIRE((int64_t)Nt * n_bins <= 16384, "frame_points_ex: %lld points per set (max 16384)",
              (long long)Nt * n_bins);
  PCA_REQUIRE(min_len > n_fft / 2 && max_len >= min_len,
              "frame_points_ex: reflect padding needs every clip longer than n_fft/2 "
              "(shortest %lld, longest %lld)", (long long)min_len, (long long)max_len);
  PCA_REQUIRE(max_len <= INT32_MAX,
              "frame_points_ex: a clip of %lld samples (meta holds int32 centres)", (long long)max_len);
  PCA_REQUIRE(aug->jitter >= 0 && aug->jitter <= (1 << 30), "frame_points_ex: jitter=%d", aug->jitter);
  PCA_REQUIRE(aug->gain_db >= 0.f && aug->gain_db <= 200.f,
              "frame_points_ex: gain_db=%g must be finite and in [0, 200]", (double)aug->gain_db);
  PCA_REQUIRE(aug->n_win >= 1, "frame_points_ex: n_win=%d", aug->n_win);
  PCA_REQUIRE(aug->norm_mode == 0 || aug->norm_mode == 1, "frame_points_ex: norm_mode=%d",
              aug->norm_mode);
  // speed
  PCA_REQUIRE(aug->n_speed >= 1 && aug->n_speed <= PCA_FRAME_MAX_SPEEDS,
              "frame_points_ex: n_speed=%d must be in [1, %d]", aug->n_speed, PCA_FRAME_MAX_SPEEDS);
  double rmin = 2.0, rmax = 0.5;
  bool any_table = false;
  for (int k = 0; k < aug->n_speed; ++k) {
    const double r = aug->ratios[k];
    PCA_REQUIRE(r >= 0.5 && r <= 2.0, "frame_points_ex: ratios[%d]=%g must be finite and in [0.5, 2]",
                k, r);
    rmin = r < rmin ? r : rmin;
    rmax = r > rmax ? r : rmax;
    any_table = any_table || r != 1.0;
  }
  if (any_table) {
    PCA_REQUIRE(aug->tables != nullptr, "frame_points_ex: null tables with a ratio other than 1");
    PCA_REQUIRE(aug->nwin > 1, "frame_points_ex: nwin=%d", aug->nwin);
    PCA_REQUIRE(aug->num_table > 0 && (int)(rmin * aug->num_table) >= 1,
                "frame_points_ex: num_table=%d (entries per zero crossing) at ratio %g", aug->num_table,
                rmin);
    PCA_REQUIRE((int64_t)((double)min_len * rmin) > n_fft / 2,
                "frame_points_ex: reflect padding needs (int64)(min_len * ratio) > n_fft/2 "
                "(shortest %lld, ratio %g)", (long long)min_len, rmin);
    PCA_REQUIRE((double)max_len * rmax <= (double)INT32_MAX,
                "frame_points_ex: a clip of %lld samples at ratio %g (meta holds int32 centres)",
                (long long)max_len, rmax);
  }
  // mix
  PCA_REQUIRE(aug->mix_prob >= 0.0 && aug->mix_prob <= 1.0, "frame_points_ex: mix_prob=%g",
              aug->mix_prob);
  PCA_REQUIRE(std::isfinite(aug->snr_lo_db) && std::isfinite(aug->snr_hi_db) &&
                  aug->snr_lo_db <= aug->snr_hi_db,
              "frame_points_ex: snr_lo_db=%g snr_hi_db=%g must be finite and in order",
              aug->snr_lo_db, aug->snr_hi_db);
  const bool mix_on = aug->mix_prob > 0.0 && aug->bg_waves != nullptr;
  if (mix_on) {
    PCA_REQUIRE(aug->clip_rms != nullptr, "frame_points_ex: mixing without clip_rms");
    PCA_REQUIRE(aug->bg_rms != nullptr, "frame_points_ex: mixing without bg_rms");
    PCA_REQUIRE(aug->bg_off != nullptr, "frame_points_ex: mixing without bg_off");
    PCA_REQUIRE(aug->n_bg > 0, "frame_points_ex: mixing with n_bg=%d", aug->n_bg);
    PCA_REQUIRE(aug->bg_max_len > 0 && aug->bg_max_len <= INT32_MAX,
                "frame_points_ex: bg_max_len=%lld (meta holds int32 starts)",
                (long long)aug->bg_max_len);
  }
  // point masks
  bool freq_on = false, time_on = false;
  if (mask != nullptr) {
    PCA_REQUIRE(mask->n_freq >= 0 && mask->n_freq <= PCA_POINT_MASK_MAX,
                "frame_points_masked: n_freq=%d must be in [0, %d]", mask->n_freq, PCA_POINT_MASK_MAX);
    PCA_REQUIRE(mask->n_time >= 0 && mask->n_time <= PCA_POINT_MASK_MAX,
                "frame_points_masked: n_time=%d must be in [0, %d]", mask->n_time, PCA_POINT_MASK_MAX);
    PCA_REQUIRE(mask->freq_width >= 0, "frame_points_masked: freq_width=%d", mask->freq_width);
    PCA_REQUIRE(mask->time_width >= 0, "frame_points_masked: time_width=%d", mask->time_width);
    freq_on = mask->n_freq > 0 && mask->freq_width > 0;
    time_on = mask->n_time > 0 && mask->time_width > 0;
    PCA_REQUIRE(!freq_on || (int64_t)mask->n_freq * mask->freq_width < n_bins,
                "frame_points_masked: n_freq=%d bands of up to freq_width=%d bins could mask all "
                "n_bins=%d (one bin must survive)", mask->n_freq, mask->freq_width, n_bins);
    PCA_REQUIRE(!time_on || (int64_t)mask->n_time * mask->time_width < Nt,
                "frame_points_masked: n_time=%d stripes of up to time_width=%d frames could mask all "
                "Nt=%d (one frame must survive)", mask->n_time, mask->time_width, Nt);
    PCA_REQUIRE(mask->mode == 0 || mask->mode == 1, "frame_points_masked: mode=%d (0 drop, 1 floor)",
                mask->mode);
    PCA_REQUIRE(mask->mode != 0 || !(freq_on || time_on) || lengths_out != nullptr,
                "frame_points_masked: drop mode needs lengths_out");
    PCA_REQUIRE(mask->mode != 1 || lengths_out == nullptr,
                "frame_points_masked: floor mode keeps every row, lengths_out must be NULL");
  }
  pca::FrameJobEx j{};
  if (freq_on) { j.n_freq = mask->n_freq; j.freq_width = mask->freq_width; }
  if (time_on) { j.n_time = mask->n_time; j.time_width = mask->time_width; }
  j.mask_floor = mask != nullptr && mask->mode == 1;
  j.lengths_out = lengths_out; j.mask_meta_out = mask_meta_out;
  j.waves = waves; j.wave_off = wave_off; j.set_off = set_off; j.clip_labels = clip_labels;
  j.idx = idx; j.farr = farr; j.tarr = tarr; j.win_lengths = aug->win_lengths;
  j.draw_dev = aug->draw_dev; j.out = out; j.labels_out = labels_out; j.meta_out = meta_out;
  j.samples_out = samples_out;
  j.seed = aug->seed; j.draw = aug->draw; j.n_clips = n_clips; j.n_fft = n_fft; j.hop = hop;
  j.n_bins = n_bins; j.Nt = Nt; j.jitter = aug->jitter; j.n_win = aug->n_win;
  j.norm_mode = aug->norm_mode; j.gain_db = aug->gain_db;
  while ((1 << j.log2n) < n_fft) ++j.log2n;
  j.n_speed = aug->n_speed; j.nwin = aug->nwin; j.num_table = aug->num_table;
  j.speed_on = (aug->n_speed > 1 || any_table) ? 1 : 0;
  for (int k = 0; k < PCA_FRAME_MAX_SPEEDS; ++k) j.ratios[k] = k < aug->n_speed ? aug->ratios[k] : 1.0;
  j.tables = aug->tables;
  if (mix_on) {
    j.bg_waves = aug->bg_waves; j.bg_off = aug->bg_off; j.bg_rms = aug->bg_rms;
    j.clip_rms = aug->clip_rms; j.n_bg = aug->n_bg;
  }
  j.bg_labels = bg_labels; j.labels2_out = labels2_out; j.weight_out = weight_out;
  j.mix_prob = aug->mix_prob; j.snr_lo_db = aug->snr_lo_db; j.snr_hi_db = aug->snr_hi_db;
  static std::once_flag lds_once;   // allow > 64 KiB of dynamic LDS (96 KiB at n_fft 4096)
  std::call_once(lds_once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pca::k_frame_points_ex),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
  });
  hipLaunchKernelGGL(pca::k_frame_points_ex, dim3((unsigned)Nt, (unsigned)B), dim3(256),
                     pca::stft_lds_bytes(n_fft), pca::as_stream(stream), j);
  return pca::check_launch("k_frame_points_ex");
}

int pca_frame_points_ex_targets(const float* waves, const int64_t* wave_off, const int64_t* set_off,
                                int n_clips, int64_t max_len, int64_t min_len,
                                const int64_t* clip_labels, const int64_t* idx, int B, int n_fft,
                                int hop, int n_bins, int Nt, const float* farr, const float* tarr,
                                const PcaFrameAugEx* aug, float* out, int64_t* labels_out,
                                int32_t* meta_out, float* samples_out, const int64_t* bg_labels,
                                int64_t* labels2_out, float* weight_out, void* stream) {
  return pca_frame_points_masked(waves, wave_off, set_off, n_clips, max_len, min_len, clip_labels, idx, B,
                                 n_fft, hop, n_bins, Nt, farr, tarr, aug, out, labels_out, meta_out,
                                 samples_out, bg_labels, labels2_out, weight_out, nullptr, nullptr,
                                 nullptr, stream);
}

int pca_frame_points_ex(const float* waves, const int64_t* wave_off, const int64_t* set_off,
                        int n_clips, int64_t max_len, int64_t min_len, const int64_t* clip_labels,
                        const int64_t* idx, int B, int n_fft, int hop, int n_bins, int Nt,
                        const float* farr, const float* tarr, const PcaFrameAugEx* aug, float* out,
                        int64_t* labels_out, int32_t* meta_out, float* samples_out, void* stream) {
  return pca_frame_points_ex_targets(waves, wave_off, set_off, n_clips, max_len, min_len, clip_labels,
                                     idx, B, n_fft, hop, n_bins, Nt, farr, tarr, aug, out, labels_out,
                                     meta_out, samples_out, nullptr, nullptr, nullptr, stream);
}
}
