// Point sets framed straight from the resident waveforms, with the augmentation drawn on the device.
//
// Replaces, for a training batch, the spectrogram pre-pass plus the per-item pack of the reference:
//   Code/settransformer.py:43-53, Code/settransformertemp.py:45-61   librosa.stft per clip, once
//   Code/dataset.py:50-54, 160-166                                   __getitem__ per item
// A pre-computed spectrogram shows the model the same frames in every epoch.  Here a batch slot cuts
// its frame(s) out of the waveform where the slot's random time shift puts them, scales them by the
// slot's random level, windows them with the slot's random window length, transforms them with the
// frame body of k_stft_logmag (stft_body.hpp) and writes (f, [t,] value) rows into the batch: the
// launch stands where k_pack stood, and no spectrogram exists.  With every augmentation off the rows are
// bit for bit those of pca_stft_logmag_batch + pca_pack_points_2d / _3d.
// HBM traffic per frame: n_fft samples read (L2-resident between neighbouring frames), n_bins rows
// written; the transform never leaves LDS.
#include "pca_common.h"
#include "select_keys.hpp"
#include "stft_body.hpp"

#include <math.h>

#include <mutex>

namespace pca {
namespace {

struct FrameJob {
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
};

// draw number k of a slot's stream: 0 time shift, 1 level, 2 window length
__device__ __forceinline__ uint64_t frame_draw(uint64_t stream, int k) {
  return mix64(stream + (uint64_t)k * 0xd1342543de82ef95ull);
}

// Workgroup (j, b): frame j of the set in batch slot b.  The Nt workgroups of a slot derive the same
// clip, shift, level and window from the slot's stream, so a chunk's frames stay `hop` apart.
__global__ __launch_bounds__(256) void k_frame_points(const FrameJob a) {
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

  // one stream per (seed, draw, batch slot, set), as the sub-sampler: a set that appears twice in a
  // batch is augmented twice, independently.  A field that is off draws nothing and is exact.
  uint64_t draw = a.draw;
  if (a.draw_dev != nullptr) draw += (uint64_t)(uint32_t)a.draw_dev[0];   // device-side counter
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
  int win = a.win_lengths[wi];          // device values: clamped here, not checked on the host
  win = win < 1 ? 1 : (win > a.n_fft ? a.n_fft : win);

  const int64_t first = s * a.Nt * a.hop + delta;       // centre of frame 0 before the clamp
  int64_t centre = first + (int64_t)j * a.hop;
  centre = centre < 0 ? 0 : (centre > L ? L : centre);  // the range the regular grid can reach
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

  stft_frame_fft(x, tw, a.waves + w0, L, centre - a.n_fft / 2, a.n_fft, a.log2n, win, (double)g, tid);

  const double inv = 1.0 / (double)(a.norm_mode == 0 ? a.n_fft : win);
  const int64_t p0 = ((int64_t)b * a.Nt + j) * a.n_bins;            // point p = j*n_bins + f
  if (a.tarr == nullptr) {
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

}  // namespace
}  // namespace pca

extern "C" {

int pca_frame_points(const float* waves, const int64_t* wave_off, const int64_t* set_off,
                     int n_clips, int64_t max_len, int64_t min_len, const int64_t* clip_labels,
                     const int64_t* idx, int B, int n_fft, int hop, int n_bins, int Nt,
                     const float* farr, const float* tarr, const PcaFrameAug* aug, float* out,
                     int64_t* labels_out, int32_t* meta_out, void* stream) {
  PCA_REQUIRE(waves && wave_off && set_off && idx && farr && aug && out, "frame_points: null pointer");
  PCA_REQUIRE(aug->win_lengths != nullptr, "frame_points: null win_lengths");
  PCA_REQUIRE((clip_labels == nullptr) == (labels_out == nullptr),
              "frame_points: clip_labels and labels_out go together");
  PCA_REQUIRE(n_clips > 0, "frame_points: n_clips=%d", n_clips);
  PCA_REQUIRE(n_fft >= 64 && n_fft <= 4096 && (n_fft & (n_fft - 1)) == 0,
              "frame_points: n_fft=%d must be a power of two in [64, 4096]", n_fft);
  PCA_REQUIRE(hop > 0, "frame_points: hop=%d", hop);
  PCA_REQUIRE(n_bins > 0 && n_bins <= n_fft / 2 + 1, "frame_points: n_bins=%d", n_bins);
  PCA_REQUIRE(B > 0 && B <= 65535 && Nt > 0, "frame_points: B=%d Nt=%d", B, Nt);
  PCA_REQUIRE((int64_t)Nt * n_bins <= 16384, "frame_points: %lld points per set (max 16384)",
              (long long)Nt * n_bins);
  PCA_REQUIRE(min_len > n_fft / 2 && max_len >= min_len,
              "frame_points: reflect padding needs every clip longer than n_fft/2 "
              "(shortest %lld, longest %lld)", (long long)min_len, (long long)max_len);
  PCA_REQUIRE(max_len <= INT32_MAX, "frame_points: a clip of %lld samples (meta holds int32 centres)",
              (long long)max_len);
  PCA_REQUIRE(aug->jitter >= 0 && aug->jitter <= (1 << 30), "frame_points: jitter=%d", aug->jitter);
  PCA_REQUIRE(aug->gain_db >= 0.f && aug->gain_db <= 200.f,
              "frame_points: gain_db=%g must be finite and in [0, 200]", (double)aug->gain_db);
  PCA_REQUIRE(aug->n_win >= 1, "frame_points: n_win=%d", aug->n_win);
  PCA_REQUIRE(aug->norm_mode == 0 || aug->norm_mode == 1, "frame_points: norm_mode=%d",
              aug->norm_mode);
  pca::FrameJob j{};
  j.waves = waves; j.wave_off = wave_off; j.set_off = set_off; j.clip_labels = clip_labels;
  j.idx = idx; j.farr = farr; j.tarr = tarr; j.win_lengths = aug->win_lengths;
  j.draw_dev = aug->draw_dev; j.out = out; j.labels_out = labels_out; j.meta_out = meta_out;
  j.seed = aug->seed; j.draw = aug->draw; j.n_clips = n_clips; j.n_fft = n_fft; j.hop = hop;
  j.n_bins = n_bins; j.Nt = Nt; j.jitter = aug->jitter; j.n_win = aug->n_win;
  j.norm_mode = aug->norm_mode; j.gain_db = aug->gain_db;
  while ((1 << j.log2n) < n_fft) ++j.log2n;
  static std::once_flag lds_once;   // allow > 64 KiB of dynamic LDS (96 KiB at n_fft 4096)
  std::call_once(lds_once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pca::k_frame_points),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
  });
  hipLaunchKernelGGL(pca::k_frame_points, dim3((unsigned)Nt, (unsigned)B), dim3(256),
                     pca::stft_lds_bytes(n_fft), pca::as_stream(stream), j);
  return pca::check_launch("k_frame_points");
}
}
