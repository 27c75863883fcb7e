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
// The slot's draws and stages 1 - 2 live in band_sums.hpp, which k_frame_points_pcen shares.
#include "band_sums.hpp"
#include "pca_common.h"
#include "stft_body.hpp"

#include <float.h>
#include <math.h>

#include <mutex>

namespace pca {
namespace {

// Workgroup (j, b): frame j of the set in batch slot b, as k_frame_points.
__global__ __launch_bounds__(256) void k_frame_points_bands(const BandsJob a) {
  extern __shared__ __attribute__((aligned(16))) double2 lds_c[];
  double2* x = lds_c;                   // [n_fft]
  double2* tw = lds_c + a.n_fft;        // [n_fft/2]
  const int tid = threadIdx.x, j = blockIdx.x, b = blockIdx.y;

  BandsSlot s;
  if (!bands_slot(a, b, s)) return;     // (uniform) a corpus that yields no set
  int64_t centre = s.first + (int64_t)j * a.hop;
  centre = centre < 0 ? 0 : (centre > s.L ? s.L : centre);   // the range the regular grid can reach
  if (j == 0 && tid == 0) bands_write_meta(a, b, s, centre);

  stft_frame_fft(x, tw, a.waves + s.w0, s.L, centre - a.n_fft / 2, a.n_fft, a.log2n, s.win, (double)s.g, tid);

  // 1. the energy term of every source bin, over the dead twiddles
  const double* p = bands_energy_terms(a, x, tw, s.win, tid);

  // 2. + 3. four lanes a band; the trip count is uniform, so every lane reaches the shuffles
  const int q = tid & 3;
  const int64_t p0 = ((int64_t)b * a.Nt + j) * a.n_bands;           // point p = j*n_bands + m
  const float t = a.tarr != nullptr ? a.tarr[j] : 0.f;
  for (int m0 = 0; m0 < a.n_bands; m0 += 64) {
    const int m = m0 + (tid >> 2);
    const double e = bands_sum(a, p, m, q);
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
