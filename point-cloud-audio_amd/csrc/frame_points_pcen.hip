// PCEN point sets (per-channel energy normalisation, Wang et al. 2017; Lostanlen et al. 2019): the band
// launch's band energies, each divided by a smoothed version of itself over the frames before it, a root
// where the log was.  The definition stands in include/pca_hip.h at pca_frame_points_pcen.
//
// No reference counterpart: the reference's sets have one point per FFT bin and a log value
// (Code/settransformer.py:43-53).  What a caller otherwise builds from a band launch over context + Nt frames,
// exp, a Python loop over the frames (the smoother is a recursion), pow and a re-pack.
//
// One launch, grid (context + Nt, B).  Workgroup (u, b) is k_frame_points_bands' workgroup for the frame
// u - context of the set (band_sums.hpp: the slot's draws, stages 1 - 2) and stores its n_bands fp64 sums to
// energy[b][u][.].  The smoother needs all frames of a slot in order, so the slot's workgroups hand over by
// ticket:
//   producer   its energy stores are agent-scope write-through stores (8-byte relaxed atomic stores: they reach
//              the memory every workgroup of the device reads, which is the release, without writing a whole
//              cache back per workgroup as a release fence would); every wave drains them (s_waitcnt
//              vmcnt(0)); workgroup barrier; thread 0: a relaxed agent-scope fetch_add on ticket[b].
//   consumer   the workgroup that draws context + Nt - 1 is the slot's last: every other workgroup of the slot
//              has published.  Thread 0: an agent-scope acquire fence and a drain; the ticket goes through LDS
//              and a barrier to the other waves, which then read energy[b] with plain vector loads.
// Nobody waits: a workgroup that is not last exits, so the launch ends whatever the grid size, the number of
// resident workgroups or the other work on the device.  Which workgroup is last has no effect on the result:
// the tail reads finished doubles in a fixed order, the integer ticket is the only read-modify-write.  The
// last workgroup stores 0 back to ticket[b], so a graph replay finds the tickets as the first launch did.
// The tail: one lane per output point (frame u >= W, band m), 256 at a time, each running the smoother from
// u = 0 up to its own frame in ascending order and then the root once.  The smoother is a few multiplies a
// step and is repeated by the Nt lanes of a band; the fp64 exp, log and pow are what costs, and this way a
// set of 64 bands x 8 frames spends two of them per lane, not eight on one wave (measured: DESIGN section 4.2).
#include "band_sums.hpp"
#include "pca_common.h"
#include "stft_body.hpp"

#include <float.h>
#include <math.h>

#include <mutex>

namespace pca {
namespace {

struct PcenJob {
  BandsJob b;
  double* energy;      // [B][W + Nt][n_bands]
  int32_t* tickets;    // [B], zero on entry and on exit
  int W;
  float s, gain, bias, r, eps, scale;
};

// Workgroup (u, b): frame u - W of the set in batch slot b; frames u < W are the smoother's history.
__global__ __launch_bounds__(256) void k_frame_points_pcen(const PcenJob a) {
  extern __shared__ __attribute__((aligned(16))) double2 lds_c[];
  double2* x = lds_c;                   // [n_fft]
  double2* tw = lds_c + a.b.n_fft;      // [n_fft/2]
  const int tid = threadIdx.x, u = blockIdx.x, b = blockIdx.y;
  const int T = a.W + a.b.Nt, n_bands = a.b.n_bands;

  BandsSlot s;
  if (!bands_slot(a.b, b, s)) return;   // (uniform over the grid) no set: no ticket is drawn, no row written
  int64_t centre = s.first + (int64_t)(u - a.W) * a.b.hop;
  centre = centre < 0 ? 0 : (centre > s.L ? s.L : centre);   // context before the clip repeats the frame at 0
  if (u == a.W && tid == 0) bands_write_meta(a.b, b, s, centre);

  stft_frame_fft(x, tw, a.b.waves + s.w0, s.L, centre - a.b.n_fft / 2, a.b.n_fft, a.b.log2n, s.win, (double)s.g,
                 tid);
  const double* p = bands_energy_terms(a.b, x, tw, s.win, tid);

  double* slot = a.energy + (int64_t)b * T * n_bands;
  const int q = tid & 3;
  for (int m0 = 0; m0 < n_bands; m0 += 64) {
    const int m = m0 + (tid >> 2);
    const double e = bands_sum(a.b, p, m, q);
    if (q == 0 && m < n_bands)
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(slot + (int64_t)u * n_bands + m),
                         (unsigned long long)__double_as_longlong(e), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }

  // publish, then draw the ticket.  x is dead since stage 1's barrier: its first word carries the ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int* drawn = reinterpret_cast<int*>(x);
  if (tid == 0) {
    const int t = __hip_atomic_fetch_add(a.tickets + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == T - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    drawn[0] = t;
  }
  __syncthreads();
  if (drawn[0] != T - 1) return;        // (uniform) not the slot's last

  // the slot's last workgroup: smoother and root, one lane per output point, u ascending
  {
#pragma clang fp contract(off)          // the header's operations one by one, no fused multiply-add
    const double sm = (double)a.s, keep = 1.0 - sm, gain = (double)a.gain, bias = (double)a.bias;
    const double r = (double)a.r, eps = (double)a.eps, scale = (double)a.scale;
    const double floor_r = pow(bias, r);
    const int n_out = a.b.Nt * n_bands;
    for (int pt = tid; pt < n_out; pt += 256) {
      const int j = pt / n_bands, m = pt - j * n_bands;
      double xv = scale * slot[m], M = xv;
      for (int v = 1; v <= a.W + j; ++v) {
        xv = scale * slot[(int64_t)v * n_bands + m];
        M = keep * M + sm * xv;
      }
      const float y = (float)(pow(bias + xv * exp(-gain * log(eps + M)), r) - floor_r);
      const int64_t row = (int64_t)b * n_out + pt;
      if (a.b.tarr == nullptr) {
        reinterpret_cast<float2*>(a.b.out)[row] = make_float2(a.b.farr[m], y);
      } else {
        float* o = a.b.out + row * 3;
        o[0] = a.b.farr[m];
        o[1] = a.b.tarr[j];
        o[2] = y;
      }
    }
  }
  if (tid == 0) __hip_atomic_store(a.tickets + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace
}  // namespace pca

extern "C" {

int pca_frame_points_pcen(const float* waves, const int64_t* wave_off, const int64_t* set_off, int n_clips,
                          int64_t max_len, int64_t min_len, const int64_t* clip_labels, const int64_t* idx,
                          int B, int n_fft, int hop, int Nt, const float* farr, const float* tarr,
                          const PcaFrameAug* aug, const PcaFrameBands* bands, const PcaPcen* pcen,
                          double* energy_ws, int64_t energy_ws_elems, int32_t* tickets, float* out,
                          int64_t* labels_out, int32_t* meta_out, void* stream) {
  PCA_REQUIRE(waves && wave_off && set_off && idx && farr && aug && bands && pcen && energy_ws && tickets && out,
              "frame_points_pcen: null pointer");
  PCA_REQUIRE(aug->win_lengths != nullptr, "frame_points_pcen: null win_lengths");
  PCA_REQUIRE(bands->band_lo && bands->band_off && bands->weights, "frame_points_pcen: null pointer in the bank");
  PCA_REQUIRE((clip_labels == nullptr) == (labels_out == nullptr),
              "frame_points_pcen: clip_labels and labels_out go together");
  PCA_REQUIRE(n_clips > 0, "frame_points_pcen: n_clips=%d", n_clips);
  PCA_REQUIRE(n_fft >= 64 && n_fft <= 4096 && (n_fft & (n_fft - 1)) == 0,
              "frame_points_pcen: n_fft=%d must be a power of two in [64, 4096]", n_fft);
  PCA_REQUIRE(hop > 0, "frame_points_pcen: hop=%d", hop);
  PCA_REQUIRE(bands->n_bands >= 1, "frame_points_pcen: n_bands=%d", bands->n_bands);
  PCA_REQUIRE(bands->nnz >= bands->n_bands, "frame_points_pcen: nnz=%d below n_bands=%d", bands->nnz,
              bands->n_bands);
  PCA_REQUIRE(bands->power == 1 || bands->power == 2, "frame_points_pcen: power=%d (1: magnitude, 2: power)",
              bands->power);
  PCA_REQUIRE(bands->amin > 0.f && bands->amin <= FLT_MAX,
              "frame_points_pcen: amin=%g must be finite and > 0", (double)bands->amin);
  PCA_REQUIRE(B > 0 && B <= 65535 && Nt > 0, "frame_points_pcen: B=%d Nt=%d", B, Nt);
  PCA_REQUIRE((int64_t)Nt * bands->n_bands <= 16384, "frame_points_pcen: %lld points per set (max 16384)",
              (long long)Nt * bands->n_bands);
  PCA_REQUIRE(min_len > n_fft / 2 && max_len >= min_len,
              "frame_points_pcen: reflect padding needs every clip longer than n_fft/2 "
              "(shortest %lld, longest %lld)", (long long)min_len, (long long)max_len);
  PCA_REQUIRE(max_len <= INT32_MAX,
              "frame_points_pcen: a clip of %lld samples (meta holds int32 centres)", (long long)max_len);
  PCA_REQUIRE(aug->jitter >= 0 && aug->jitter <= (1 << 30), "frame_points_pcen: jitter=%d", aug->jitter);
  PCA_REQUIRE(aug->gain_db >= 0.f && aug->gain_db <= 200.f,
              "frame_points_pcen: gain_db=%g must be finite and in [0, 200]", (double)aug->gain_db);
  PCA_REQUIRE(aug->n_win >= 1, "frame_points_pcen: n_win=%d", aug->n_win);
  PCA_REQUIRE(aug->norm_mode == 0 || aug->norm_mode == 1, "frame_points_pcen: norm_mode=%d", aug->norm_mode);
  // the comparisons are written so that a NaN fails them
  PCA_REQUIRE(pcen->context >= 0 && pcen->context <= 255, "frame_points_pcen: context=%d outside [0, 255]",
              pcen->context);
  PCA_REQUIRE(pcen->s > 0.f && pcen->s <= 1.f, "frame_points_pcen: s=%g outside (0, 1]", (double)pcen->s);
  PCA_REQUIRE(pcen->gain >= 0.f && pcen->gain <= 4.f, "frame_points_pcen: gain=%g outside [0, 4]",
              (double)pcen->gain);
  PCA_REQUIRE(pcen->bias >= 0.f && pcen->bias <= 1e6f, "frame_points_pcen: bias=%g outside [0, 1e6]",
              (double)pcen->bias);
  PCA_REQUIRE(pcen->r > 0.f && pcen->r <= 1.f, "frame_points_pcen: r=%g outside (0, 1]", (double)pcen->r);
  PCA_REQUIRE(pcen->eps > 0.f && pcen->eps <= FLT_MAX, "frame_points_pcen: eps=%g must be finite and > 0",
              (double)pcen->eps);
  PCA_REQUIRE(pcen->scale > 0.f && pcen->scale <= FLT_MAX, "frame_points_pcen: scale=%g must be finite and > 0",
              (double)pcen->scale);
  const int64_t T = (int64_t)pcen->context + Nt;
  PCA_REQUIRE(energy_ws_elems >= 0 && (int64_t)B * T * bands->n_bands <= energy_ws_elems,
              "frame_points_pcen: the workspace holds %lld doubles, B=%d slots of (context + Nt) * n_bands = "
              "%lld need %lld", (long long)energy_ws_elems, B, (long long)(T * bands->n_bands),
              (long long)((int64_t)B * T * bands->n_bands));
  pca::PcenJob p{};
  pca::BandsJob& j = p.b;
  j.waves = waves; j.wave_off = wave_off; j.set_off = set_off; j.clip_labels = clip_labels;
  j.idx = idx; j.farr = farr; j.tarr = tarr; j.win_lengths = aug->win_lengths;
  j.draw_dev = aug->draw_dev; j.band_lo = bands->band_lo; j.band_off = bands->band_off;
  j.weights = bands->weights; j.out = out; j.labels_out = labels_out; j.meta_out = meta_out;
  j.seed = aug->seed; j.draw = aug->draw; j.n_clips = n_clips; j.n_fft = n_fft; j.hop = hop;
  j.n_bands = bands->n_bands; j.nnz = bands->nnz; j.power = bands->power; j.Nt = Nt;
  j.jitter = aug->jitter; j.n_win = aug->n_win; j.norm_mode = aug->norm_mode; j.gain_db = aug->gain_db;
  j.amin = bands->amin;
  while ((1 << j.log2n) < n_fft) ++j.log2n;
  p.energy = energy_ws; p.tickets = tickets; p.W = pcen->context;
  p.s = pcen->s; p.gain = pcen->gain; p.bias = pcen->bias; p.r = pcen->r; p.eps = pcen->eps;
  p.scale = pcen->scale;
  static std::once_flag lds_once;   // allow > 64 KiB of dynamic LDS (96 KiB at n_fft 4096)
  std::call_once(lds_once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pca::k_frame_points_pcen),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
  });
  hipLaunchKernelGGL(pca::k_frame_points_pcen, dim3((unsigned)T, (unsigned)B), dim3(256),
                     pca::stft_lds_bytes(n_fft), pca::as_stream(stream), p);
  return pca::check_launch("k_frame_points_pcen");
}
}
