// The band launches' shared body (k_frame_points_bands, k_frame_points_pcen): which clip, shift, gain and
// window a batch slot draws, and the band stages 1 and 2 that follow stft_frame_fft - the energy term of every
// source bin written over the dead twiddles, then the fp64 sum of a band by four neighbouring lanes.  What a
// kernel does with the sum (logf and a row store, or a store to a workspace) is its own.
#pragma once
#include "pca_common.h"
#include "select_keys.hpp"

namespace pca {

struct BandsJob {
  const float* waves;
  const int64_t *wave_off, *set_off, *clip_labels, *idx;
  const float *farr, *tarr;
  const int32_t *win_lengths, *draw_dev;
  const int32_t *band_lo, *band_off;
  const float* weights;
  float* out;
  int64_t* labels_out;
  int32_t* meta_out;
  uint64_t seed, draw;
  int n_clips, n_fft, log2n, hop, n_bands, nnz, power, Nt, jitter, n_win, norm_mode;
  float gain_db, amin;
};

// draw number k of a slot's stream, as k_frame_points: 0 time shift, 1 level, 2 window length
__device__ __forceinline__ uint64_t bands_draw(uint64_t stream, int k) {
  return mix64(stream + (uint64_t)k * 0xd1342543de82ef95ull);
}

// What batch slot b cuts: clip c = waves[w0 .. w0 + L), the centre of frame 0 before the clamp, window, gain.
struct BandsSlot {
  int c, win;
  int64_t w0, L, first;
  float g;
};

// false (uniform over the grid): a corpus that yields no set
__device__ __forceinline__ bool bands_slot(const BandsJob& a, int b, BandsSlot& o) {
  const int64_t total = a.set_off[a.n_clips];
  if (total <= 0) return false;
  int64_t i = a.idx[b];
  i = i < 0 ? 0 : (i >= total ? total - 1 : i);
  int lo = 0, hi = a.n_clips;           // first clip whose set_off exceeds i (set_off[n_clips] does)
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (a.set_off[m] > i) hi = m; else lo = m + 1;
  }
  const int c = lo > 0 ? lo - 1 : 0;    // set_off[c] <= i < set_off[c + 1]  (set_off[0] is 0)
  const int64_t s = i - a.set_off[c];
  o.c = c;
  o.w0 = a.wave_off[c];
  o.L = a.wave_off[c + 1] - o.w0;

  // k_frame_points' stream and draws: a field that is off draws nothing and is exact
  uint64_t draw = a.draw;
  if (a.draw_dev != nullptr) draw += (uint64_t)(uint32_t)a.draw_dev[0];   // device-side counter
  const uint64_t stream = select_stream(a.seed, draw, i, b);
  int64_t delta = 0;
  if (a.jitter > 0) {
    const uint64_t r = bands_draw(stream, 0) >> 32;
    delta = (int64_t)((r * (uint64_t)(2 * (int64_t)a.jitter + 1)) >> 32) - a.jitter;
  }
  o.g = 1.0f;
  if (a.gain_db > 0.f) {
    const double u = (double)(bands_draw(stream, 1) >> 11) * (2.0 / 9007199254740992.0) - 1.0;  // [-1, 1)
    o.g = (float)exp2(u * (double)a.gain_db * 0.16609640474436813);        // 10^(u dB / 20)
  }
  int wi = 0;
  if (a.n_win > 1) wi = (int)(((bands_draw(stream, 2) >> 32) * (uint64_t)a.n_win) >> 32);
  int win = a.win_lengths[wi];          // device values: clamped here, not checked on the host
  o.win = win < 1 ? 1 : (win > a.n_fft ? a.n_fft : win);
  o.first = s * a.Nt * a.hop + delta;   // centre of frame 0 before the clamp
  return true;
}

// labels_out[b] and meta_out[b]: one thread of the workgroup that holds the set's frame 0 (centre: its own)
__device__ __forceinline__ void bands_write_meta(const BandsJob& a, int b, const BandsSlot& s, int64_t centre) {
  if (a.clip_labels != nullptr && a.labels_out != nullptr) a.labels_out[b] = a.clip_labels[s.c];
  if (a.meta_out != nullptr) {
    int32_t* m = a.meta_out + (int64_t)b * 4;
    m[0] = s.c;
    m[1] = (int32_t)centre;
    m[2] = s.win;
    m[3] = (int32_t)__float_as_uint(s.g);
  }
}

// Stage 1, after the butterflies' closing barrier: p[k], k <= n_fft/2, the fp32 magnitude (power 1) or its
// fp64 square (power 2) as a double, written over the twiddles; ends with a barrier.  Returns p.
__device__ __forceinline__ double* bands_energy_terms(const BandsJob& a, const double2* x, double2* tw, int win,
                                                      int tid) {
  const double inv = 1.0 / (double)(a.norm_mode == 0 ? a.n_fft : win);
  const int nb = a.n_fft / 2 + 1;
  double* p = reinterpret_cast<double*>(tw);            // [n_fft] doubles of room, nb used
  for (int k = tid; k < nb; k += 256) {
    const double2 v = x[k];
    const float re = (float)(v.x * inv), im = (float)(v.y * inv);   // stft_logmag_bin's magnitude
    const double mag = (double)sqrtf(re * re + im * im);
    p[k] = a.power == 1 ? mag : mag * mag;
  }
  __syncthreads();
  return p;
}

// Stage 2: band m = m0 + tid / 4 of the pass that starts at m0, summed by four neighbouring lanes.  Lane q adds
// the terms i0 + q, i0 + q + 4, ... of the band's clipped range in ascending i (fp64 fma); the partials are
// combined as (s0 + s1) + (s2 + s3), the same bits in all four lanes.  Every lane of the workgroup calls it
// (the shuffles): a lane whose m is past n_bands adds nothing.
__device__ __forceinline__ double bands_sum(const BandsJob& a, const double* p, int m, int q) {
  const int nb = a.n_fft / 2 + 1;
  double e = 0.0;
  if (m < a.n_bands) {
    int64_t o0 = a.band_off[m], o1 = a.band_off[m + 1];
    o0 = o0 < 0 ? 0 : (o0 > a.nnz ? a.nnz : o0);
    o1 = o1 < o0 ? o0 : (o1 > a.nnz ? a.nnz : o1);
    const int64_t blo = a.band_lo[m];
    const int64_t i0 = blo < 0 ? -blo : 0;                          // first term whose bin is >= 0
    const int64_t i1 = (o1 - o0) < (nb - blo) ? (o1 - o0) : (nb - blo);   // one past the last, bin < nb
    const float* w = a.weights + o0;
    for (int64_t ii = i0 + q; ii < i1; ii += 4) e = fma((double)w[ii], p[blo + ii], e);
  }
  e += __shfl_xor(e, 1);                // s0 + s1 | s2 + s3: the same bits in both lanes of a pair
  e += __shfl_xor(e, 2);                // (s0 + s1) + (s2 + s3)
  return e;
}

}  // namespace pca
