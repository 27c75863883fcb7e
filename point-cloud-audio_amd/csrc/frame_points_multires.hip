// Multi-resolution point sets: one frame launch whose workgroups belong to several STFT resolutions.
//
// A set does not need a grid, so it can hold points from several analysis lengths at once: the long
// window's points are sharp in frequency, the short window's sharp in time, and one (f, t, value) set
// carries both.  No reference counterpart: Code/pceval.py:55-105 varies the analysis length one at a time.
// Every level of a batch slot shares the slot's clip, time shift, gain and window INDEX (k_frame_points'
// stream and draw numbers); each level has its own n_fft, hop, frame count, axes, window table and offset
// from the set's anchor.  The frame body is stft_body.hpp's, so a frame that k_frame_points also cuts has
// the same bits here.  The levels' rows land back to back in out[B, N, din]: what a caller otherwise gets
// from one pca_frame_points per level plus a concatenation, without the second trip through HBM.
#include "pca_common.h"
#include "select_keys.hpp"
#include "stft_body.hpp"

#include <math.h>

#include <mutex>

namespace pca {
namespace {

struct MultiresLevel {
  const float *farr, *tarr;
  const int32_t* win_lengths;
  int n_fft, log2n, hop, n_bins, Nt, offset;
  int point_off;                        // P_r: first point of the level inside a set
};

struct MultiresJob {
  const float* waves;
  const int64_t *wave_off, *set_off, *clip_labels, *idx;
  const int32_t* draw_dev;
  float* out;
  int64_t* labels_out;
  int32_t* meta_out;
  uint64_t seed, draw;
  int64_t span;
  int n_clips, n_levels, N, din, jitter, n_win, norm_mode;
  float gain_db;
  MultiresLevel lv[PCA_FRAME_MAX_LEVELS];   // the caller's order: the output layout
  // block order: entry k covers blockIdx.x in [blk_end[k-1], blk_end[k]) and belongs to level blk_level[k];
  // entries by descending n_fft, so the longest chains are dispatched first
  int blk_end[PCA_FRAME_MAX_LEVELS], blk_level[PCA_FRAME_MAX_LEVELS];
};

// draw number k of a slot's stream, as k_frame_points: 0 time shift, 1 level, 2 window index
__device__ __forceinline__ uint64_t multires_draw(uint64_t stream, int k) {
  return mix64(stream + (uint64_t)k * 0xd1342543de82ef95ull);
}

// Workgroup (x, b): frame j of level r of the set in batch slot b, (r, j) from the prefix table.  All
// workgroups of a slot derive the same clip, shift, gain and window index from the slot's stream.
__global__ __launch_bounds__(256) void k_frame_points_multires(const MultiresJob a) {
  extern __shared__ __attribute__((aligned(16))) double2 lds_c[];
  const int tid = threadIdx.x, b = blockIdx.y;

  int k = 0;                            // (uniform) the table entry of this workgroup
  while (k + 1 < a.n_levels && (int)blockIdx.x >= a.blk_end[k]) ++k;
  const int r = a.blk_level[k];
  const int j = (int)blockIdx.x - (k > 0 ? a.blk_end[k - 1] : 0);
  MultiresLevel l = a.lv[0];            // selected field by field: the table stays in scalar registers
#pragma unroll
  for (int q = 1; q < PCA_FRAME_MAX_LEVELS; ++q)
    if (q == r) l = a.lv[q];
  double2* x = lds_c;                   // [n_fft]
  double2* tw = lds_c + l.n_fft;        // [n_fft/2]

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

  // k_frame_points' stream and draws: a field that is off draws nothing and is exact
  uint64_t draw = a.draw;
  if (a.draw_dev != nullptr) draw += (uint64_t)(uint32_t)a.draw_dev[0];   // device-side counter
  const uint64_t stream = select_stream(a.seed, draw, i, b);
  int64_t delta = 0;
  if (a.jitter > 0) {
    const uint64_t u = multires_draw(stream, 0) >> 32;
    delta = (int64_t)((u * (uint64_t)(2 * (int64_t)a.jitter + 1)) >> 32) - a.jitter;
  }
  float g = 1.0f;
  if (a.gain_db > 0.f) {
    const double u = (double)(multires_draw(stream, 1) >> 11) * (2.0 / 9007199254740992.0) - 1.0;  // [-1, 1)
    g = (float)exp2(u * (double)a.gain_db * 0.16609640474436813);          // 10^(u dB / 20)
  }
  int wi = 0;
  if (a.n_win > 1) wi = (int)(((multires_draw(stream, 2) >> 32) * (uint64_t)a.n_win) >> 32);
  int win = l.win_lengths[wi];          // device values: clamped here, not checked on the host
  win = win < 1 ? 1 : (win > l.n_fft ? l.n_fft : win);

  const int64_t first = s * a.span + delta;             // the set's anchor
  int64_t centre = first + l.offset + (int64_t)j * l.hop;
  centre = centre < 0 ? 0 : (centre > L ? L : centre);  // the range the regular grid can reach
  if (r == 0 && j == 0 && tid == 0) {
    if (a.clip_labels != nullptr && a.labels_out != nullptr) a.labels_out[b] = a.clip_labels[c];
    if (a.meta_out != nullptr) {
      int32_t* m = a.meta_out + (int64_t)b * 8;
      m[0] = c;
      m[1] = (int32_t)centre;
      m[2] = win;
      m[3] = (int32_t)__float_as_uint(g);
      m[4] = (int32_t)delta;
      m[5] = wi;
      m[6] = 0;
      m[7] = 0;
    }
  }

  stft_frame_fft(x, tw, a.waves + w0, L, centre - l.n_fft / 2, l.n_fft, l.log2n, win, (double)g, tid);

  const double inv = 1.0 / (double)(a.norm_mode == 0 ? l.n_fft : win);
  const int64_t p0 = (int64_t)b * a.N + l.point_off + (int64_t)j * l.n_bins;   // point j*n_bins + f of the level
  if (a.din == 2) {
    float2* o = reinterpret_cast<float2*>(a.out) + p0;
    for (int f = tid; f < l.n_bins; f += 256) o[f] = make_float2(l.farr[f], stft_logmag_bin(x[f], inv));
  } else {
    const float t = l.tarr[j];
    float* o = a.out + p0 * 3;
    for (int f = tid; f < l.n_bins; f += 256) {
      o[f * 3 + 0] = l.farr[f];
      o[f * 3 + 1] = t;
      o[f * 3 + 2] = stft_logmag_bin(x[f], inv);
    }
  }
}

}  // namespace
}  // namespace pca

extern "C" {

int pca_frame_points_multires(const float* waves, const int64_t* wave_off, const int64_t* set_off,
                              int n_clips, int64_t max_len, int64_t min_len, const int64_t* clip_labels,
                              const int64_t* idx, int B, const PcaFrameLevel* levels, int n_levels,
                              int64_t span, const PcaFrameAug* aug, float* out, int64_t* labels_out,
                              int32_t* meta_out, void* stream) {
  PCA_REQUIRE(waves && wave_off && set_off && idx && levels && aug && out,
              "frame_points_multires: null pointer");
  PCA_REQUIRE((clip_labels == nullptr) == (labels_out == nullptr),
              "frame_points_multires: clip_labels and labels_out go together");
  PCA_REQUIRE(n_clips > 0, "frame_points_multires: n_clips=%d", n_clips);
  PCA_REQUIRE(n_levels >= 1 && n_levels <= PCA_FRAME_MAX_LEVELS,
              "frame_points_multires: n_levels=%d (1 .. %d)", n_levels, PCA_FRAME_MAX_LEVELS);
  PCA_REQUIRE(B > 0 && B <= 65535, "frame_points_multires: B=%d", B);
  PCA_REQUIRE(span > 0 && span <= ((int64_t)1 << 30), "frame_points_multires: span=%lld outside (0, 2^30]",
              (long long)span);
  int64_t N = 0, frames = 0;
  int max_fft = 0;
  for (int r = 0; r < n_levels; ++r) {
    const PcaFrameLevel& l = levels[r];
    PCA_REQUIRE(l.n_fft >= 64 && l.n_fft <= 4096 && (l.n_fft & (l.n_fft - 1)) == 0,
                "frame_points_multires: level %d n_fft=%d must be a power of two in [64, 4096]", r, l.n_fft);
    PCA_REQUIRE(l.hop > 0, "frame_points_multires: level %d hop=%d", r, l.hop);
    PCA_REQUIRE(l.n_bins > 0 && l.n_bins <= l.n_fft / 2 + 1, "frame_points_multires: level %d n_bins=%d",
                r, l.n_bins);
    PCA_REQUIRE(l.Nt > 0, "frame_points_multires: level %d Nt=%d", r, l.Nt);
    PCA_REQUIRE(l.offset >= -(1 << 30) && l.offset <= (1 << 30),
                "frame_points_multires: level %d offset=%d outside [-2^30, 2^30]", r, l.offset);
    PCA_REQUIRE(l.farr != nullptr, "frame_points_multires: level %d null farr", r);
    PCA_REQUIRE(l.win_lengths != nullptr, "frame_points_multires: level %d null win_lengths", r);
    PCA_REQUIRE((l.tarr == nullptr) == (levels[0].tarr == nullptr),
                "frame_points_multires: tarr is set in every level or in none (level %d differs)", r);
    N += (int64_t)l.Nt * l.n_bins;
    frames += l.Nt;
    PCA_REQUIRE(N <= 16384, "frame_points_multires: %lld points per set (max 16384)", (long long)N);
    max_fft = l.n_fft > max_fft ? l.n_fft : max_fft;
  }
  PCA_REQUIRE(min_len > max_fft / 2 && max_len >= min_len,
              "frame_points_multires: reflect padding needs every clip longer than n_fft/2 of the largest "
              "level (%d; shortest %lld, longest %lld)", max_fft / 2, (long long)min_len, (long long)max_len);
  PCA_REQUIRE(max_len <= INT32_MAX,
              "frame_points_multires: a clip of %lld samples (meta holds int32 centres)", (long long)max_len);
  PCA_REQUIRE(aug->jitter >= 0 && aug->jitter <= (1 << 30), "frame_points_multires: jitter=%d", aug->jitter);
  PCA_REQUIRE(aug->gain_db >= 0.f && aug->gain_db <= 200.f,
              "frame_points_multires: gain_db=%g must be finite and in [0, 200]", (double)aug->gain_db);
  PCA_REQUIRE(aug->n_win >= 1, "frame_points_multires: n_win=%d", aug->n_win);
  PCA_REQUIRE(aug->norm_mode == 0 || aug->norm_mode == 1, "frame_points_multires: norm_mode=%d",
              aug->norm_mode);

  pca::MultiresJob j{};
  j.waves = waves; j.wave_off = wave_off; j.set_off = set_off; j.clip_labels = clip_labels; j.idx = idx;
  j.draw_dev = aug->draw_dev; j.out = out; j.labels_out = labels_out; j.meta_out = meta_out;
  j.seed = aug->seed; j.draw = aug->draw; j.span = span; j.n_clips = n_clips; j.n_levels = n_levels;
  j.N = (int)N; j.din = levels[0].tarr == nullptr ? 2 : 3; j.jitter = aug->jitter; j.n_win = aug->n_win;
  j.norm_mode = aug->norm_mode; j.gain_db = aug->gain_db;
  int order[PCA_FRAME_MAX_LEVELS];
  for (int r = 0, p = 0; r < PCA_FRAME_MAX_LEVELS; ++r) {
    const PcaFrameLevel& l = levels[r < n_levels ? r : 0];   // unused entries repeat level 0: valid to select
    pca::MultiresLevel& d = j.lv[r];
    d.farr = l.farr; d.tarr = l.tarr; d.win_lengths = l.win_lengths; d.n_fft = l.n_fft; d.hop = l.hop;
    d.n_bins = l.n_bins; d.Nt = l.Nt; d.offset = l.offset; d.point_off = r < n_levels ? p : 0;
    while ((1 << d.log2n) < l.n_fft) ++d.log2n;
    if (r < n_levels) p += l.Nt * l.n_bins;
    order[r] = r;
  }
  for (int u = 1; u < n_levels; ++u)      // stable insertion sort by descending n_fft
    for (int v = u; v > 0 && levels[order[v]].n_fft > levels[order[v - 1]].n_fft; --v) {
      const int t = order[v]; order[v] = order[v - 1]; order[v - 1] = t;
    }
  for (int k = 0, e = 0; k < PCA_FRAME_MAX_LEVELS; ++k) {
    if (k < n_levels) e += levels[order[k]].Nt;
    j.blk_end[k] = e;
    j.blk_level[k] = k < n_levels ? order[k] : order[n_levels - 1];
  }
  static std::once_flag lds_once;   // allow > 64 KiB of dynamic LDS (96 KiB at n_fft 4096)
  std::call_once(lds_once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pca::k_frame_points_multires),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
  });
  hipLaunchKernelGGL(pca::k_frame_points_multires, dim3((unsigned)frames, (unsigned)B), dim3(256),
                     pca::stft_lds_bytes(max_fft), pca::as_stream(stream), j);
  return pca::check_launch("k_frame_points_multires");
}
}
