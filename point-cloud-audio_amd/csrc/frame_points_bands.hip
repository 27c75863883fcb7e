// Band point sets (log-mel and any other non-negative filter bank): k_frame_points' frame, its bins
// summed into bands while the spectrum still lies in LDS.
//
// No reference counterpart: the reference's sets have one point per FFT bin (Code/settransformer.py:43-53).
// What a caller otherwise builds from pca_frame_points plus exp -> matmul -> log in torch: the full set
// written to HBM and read back only to throw most of it away.  Clip, centre, shift, gain and window of a
// batch slot are k_frame_points' (the same stream and draw numbers), the transform is stft_body.hpp's, and
// the magnitude of a bin is the fp32 one stft_logmag_bin forms, so the identity bank with power 1 and
// amin 1e-8f gives pca_frame_points' bits.
//
// Band stage, after the butterflies' closing barrier:
//   1. p[k], k <= n_fft/2: the fp32 magnitude (power 1) or its fp64 square (power 2), as a double, written
//      over the twiddles (n_fft/2 double2 = n_fft doubles; dead once the butterflies are done).  One barrier.
//   2. four neighbouring lanes own band m = 64 * pass + tid / 4.  Lane q adds the terms i0 + q, i0 + q + 4, ...
//      of the band's clipped range [i0, i1) in ascending i (fp64 fma), then the four partials are combined as
//      (s0 + s1) + (s2 + s3) by two xor shuffles.  The order depends on the bank alone - not on the grid,
//      the batch or timing - and there are no atomics: the same arguments give the same bits.  Four lanes
//      read four consecutive weights and four consecutive doubles of LDS per step; a mel band of up to 65
//      bins takes at most 17 steps, 128 bands two passes.
//   3. lane 0 of the four stores the row, the sibling kernels' float2 / 3-float rows: a wave writes 16
//      consecutive rows per store.
// The bank is device memory: a band's range is clipped into [0, n_fft/2] and its weight offsets into
// [0, nnz] here, so nothing outside band_lo[n_bands], band_off[n_bands + 1] and weights[nnz] is read.
#include "pca_common.h"
#include "select_keys.hpp"
#include "stft_body.hpp"

#include <float.h>
#include <math.h>

#include <mutex>

namespace pca {
namespace {

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

// Workgroup (j, b): frame j of the set in batch slot b, as k_frame_points.
__global__ __launch_bounds__(256) void k_frame_points_bands(const BandsJob a) {
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

  // k_frame_points' stream and draws: a field that is off draws nothing and is exact
  uint64_t draw = a.draw;
  if (a.draw_dev != nullptr) draw += (uint64_t)(uint32_t)a.draw_dev[0];   // device-side counter
  const uint64_t stream = select_stream(a.seed, draw, i, b);
  int64_t delta = 0;
  if (a.jitter > 0) {
    const uint64_t r = bands_draw(stream, 0) >> 32;
    delta = (int64_t)((r * (uint64_t)(2 * (int64_t)a.jitter + 1)) >> 32) - a.jitter;
  }
  float g = 1.0f;
  if (a.gain_db > 0.f) {
    const double u = (double)(bands_draw(stream, 1) >> 11) * (2.0 / 9007199254740992.0) - 1.0;  // [-1, 1)
    g = (float)exp2(u * (double)a.gain_db * 0.16609640474436813);          // 10^(u dB / 20)
  }
  int wi = 0;
  if (a.n_win > 1) wi = (int)(((bands_draw(stream, 2) >> 32) * (uint64_t)a.n_win) >> 32);
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

  // 1. the energy term of every source bin, over the dead twiddles
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

  // 2. + 3. four lanes a band; the trip count is uniform, so every lane reaches the shuffles
  const int q = tid & 3;
  const int64_t p0 = ((int64_t)b * a.Nt + j) * a.n_bands;           // point p = j*n_bands + m
  const float t = a.tarr != nullptr ? a.tarr[j] : 0.f;
  for (int m0 = 0; m0 < a.n_bands; m0 += 64) {
    const int m = m0 + (tid >> 2);
    double e = 0.0;
    if (m < a.n_bands) {
      int64_t o0 = a.band_off[m], o1 = a.band_off[m + 1];
      o0 = o0 < 0 ? 0 : (o0 > a.nnz ? a.nnz : o0);
      o1 = o1 < o0 ? o0 : (o1 > a.nnz ? a.nnz : o1);
      const int64_t blo = a.band_lo[m];
      const int64_t i0 = blo < 0 ? -blo : 0;                        // first term whose bin is >= 0
      const int64_t i1 = (o1 - o0) < (nb - blo) ? (o1 - o0) : (nb - blo);   // one past the last, bin < nb
      const float* w = a.weights + o0;
      for (int64_t ii = i0 + q; ii < i1; ii += 4) e = fma((double)w[ii], p[blo + ii], e);
    }
    e += __shfl_xor(e, 1);              // s0 + s1 | s2 + s3: the same bits in both lanes of a pair
    e += __shfl_xor(e, 2);              // (s0 + s1) + (s2 + s3)
    if (q == 0 && m < a.n_bands) {
      const float v = logf(a.amin + (float)e);
      if (a.tarr == nullptr) {
        reinterpret_cast<float2*>(a.out)[p0 + m] = make_float2(a.farr[m], v);
      } else {
        float* o = a.out + (p0 + m) * 3;
        o[0] = a.farr[m];
        o[1] = t;
        o[2] = v;
      }
    }
  }
}

}  // namespace
}  // namespace pca

extern "C" {

int pca_frame_points_bands(const float* waves, const int64_t* wave_off, const int64_t* set_off,
                           int n_clips, int64_t max_len, int64_t min_len, const int64_t* clip_labels,
                           const int64_t* idx, int B, int n_fft, int hop, int Nt, const float* farr,
                           const float* tarr, const PcaFrameAug* aug, const PcaFrameBands* bands,
                           float* out, int64_t* labels_out, int32_t* meta_out, void* stream) {
  PCA_REQUIRE(waves && wave_off && set_off && idx && farr && aug && bands && out,
              "frame_points_bands: null pointer");
  PCA_REQUIRE(aug->win_lengths != nullptr, "frame_points_bands: null win_lengths");
  PCA_REQUIRE(bands->band_lo && bands->band_off && bands->weights, "frame_points_bands: null pointer in the bank");
  PCA_REQUIRE((clip_labels == nullptr) == (labels_out == nullptr),
              "frame_points_bands: clip_labels and labels_out go together");
  PCA_REQUIRE(n_clips > 0, "frame_points_bands: n_clips=%d", n_clips);
  PCA_REQUIRE(n_fft >= 64 && n_fft <= 4096 && (n_fft & (n_fft - 1)) == 0,
              "frame_points_bands: n_fft=%d must be a power of two in [64, 4096]", n_fft);
  PCA_REQUIRE(hop > 0, "frame_points_bands: hop=%d", hop);
  PCA_REQUIRE(bands->n_bands >= 1, "frame_points_bands: n_bands=%d", bands->n_bands);
  PCA_REQUIRE(bands->nnz >= bands->n_bands, "frame_points_bands: nnz=%d below n_bands=%d", bands->nnz,
              bands->n_bands);
  PCA_REQUIRE(bands->power == 1 || bands->power == 2, "frame_points_bands: power=%d (1: magnitude, 2: power)",
              bands->power);
  PCA_REQUIRE(bands->amin > 0.f && bands->amin <= FLT_MAX,
              "frame_points_bands: amin=%g must be finite and > 0", (double)bands->amin);
  PCA_REQUIRE(B > 0 && B <= 65535 && Nt > 0, "frame_points_bands: B=%d Nt=%d", B, Nt);
  PCA_REQUIRE((int64_t)Nt * bands->n_bands <= 16384, "frame_points_bands: %lld points per set (max 16384)",
              (long long)Nt * bands->n_bands);
  PCA_REQUIRE(min_len > n_fft / 2 && max_len >= min_len,
              "frame_points_bands: reflect padding needs every clip longer than n_fft/2 "
              "(shortest %lld, longest %lld)", (long long)min_len, (long long)max_len);
  PCA_REQUIRE(max_len <= INT32_MAX,
              "frame_points_bands: a clip of %lld samples (meta holds int32 centres)", (long long)max_len);
  PCA_REQUIRE(aug->jitter >= 0 && aug->jitter <= (1 << 30), "frame_points_bands: jitter=%d", aug->jitter);
  PCA_REQUIRE(aug->gain_db >= 0.f && aug->gain_db <= 200.f,
              "frame_points_bands: gain_db=%g must be finite and in [0, 200]", (double)aug->gain_db);
  PCA_REQUIRE(aug->n_win >= 1, "frame_points_bands: n_win=%d", aug->n_win);
  PCA_REQUIRE(aug->norm_mode == 0 || aug->norm_mode == 1, "frame_points_bands: norm_mode=%d",
              aug->norm_mode);
  pca::BandsJob j{};
  j.waves = waves; j.wave_off = wave_off; j.set_off = set_off; j.clip_labels = clip_labels;
  j.idx = idx; j.farr = farr; j.tarr = tarr; j.win_lengths = aug->win_lengths;
  j.draw_dev = aug->draw_dev; j.band_lo = bands->band_lo; j.band_off = bands->band_off;
  j.weights = bands->weights; j.out = out; j.labels_out = labels_out; j.meta_out = meta_out;
  j.seed = aug->seed; j.draw = aug->draw; j.n_clips = n_clips; j.n_fft = n_fft; j.hop = hop;
  j.n_bands = bands->n_bands; j.nnz = bands->nnz; j.power = bands->power; j.Nt = Nt;
  j.jitter = aug->jitter; j.n_win = aug->n_win; j.norm_mode = aug->norm_mode; j.gain_db = aug->gain_db;
  j.amin = bands->amin;
  while ((1 << j.log2n) < n_fft) ++j.log2n;
  static std::once_flag lds_once;   // allow > 64 KiB of dynamic LDS (96 KiB at n_fft 4096)
  std::call_once(lds_once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pca::k_frame_points_bands),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
  });
  hipLaunchKernelGGL(pca::k_frame_points_bands, dim3((unsigned)Nt, (unsigned)B), dim3(256),
                     pca::stft_lds_bytes(n_fft), pca::as_stream(stream), j);
  return pca::check_launch("k_frame_points_bands");
}
}
