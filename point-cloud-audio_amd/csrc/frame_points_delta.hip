// Delta point sets: the grid launch's or the band launch's rows with regression deltas of the value column as
// further columns - how a point's value compares with the frames before and after it (dt) and with the rows
// below and above it (df).  A grid model gets this from its first convolution; a set model has no
// neighbourhood, so the difference travels with the point.  The definition stands in include/pca_hip.h at
// pca_frame_points_delta.
//
// No reference counterpart: the reference's sets carry (f, [t,] value) only (Code/settransformer.py:43-53).
// What a caller otherwise builds from a frame launch over Nt + 2 W frames, slicing, padding and a re-pack.
//
// One launch, grid (T, B), T = Nt + 2 Wt (Wt = W with a time delta, else 0).  Workgroup (u, b) is
// k_frame_points' / k_frame_points_bands' workgroup for the frame u - Wt of the set (band_sums.hpp: the slot's
// draws; stft_body.hpp: the frame and its value; band stages 1 - 2 with a bank) and stores the F fp32 values of
// its frame to values[b][u][.].  A delta needs the frames around it, so the slot's workgroups hand over by
// ticket, as k_frame_points_pcen's do:
//   producer   its value stores are agent-scope write-through stores (4-byte relaxed atomic stores: they reach
//              the memory every workgroup of the device reads, which is the release); every wave drains them
//              (s_waitcnt vmcnt(0)); workgroup barrier; thread 0: a relaxed agent-scope fetch_add on ticket[b].
//   consumer   the workgroup that draws T - 1 is the slot's last: every other workgroup of the slot has
//              published.  Thread 0: an agent-scope acquire fence and a drain; the ticket goes through LDS and
//              a barrier to the other waves, which then read values[b] with plain vector loads.
// The launch's properties:
//   - no workgroup waits for another: one that is not last exits, so the launch ends whatever the grid size,
//     the number of resident workgroups or the other work on the device;
//   - which workgroup is last has no effect on a bit: the tail reads finished floats in a fixed order;
//   - the only read-modify-write is the integer ticket; there are no float atomics;
//   - the last workgroup stores 0 back to ticket[b], so the tickets are zero on exit and a captured launch
//     replays without a memset;
//   - values is written with vector stores from plain C++; the only inline assembly is the s_waitcnt that
//     k_frame_points_pcen uses.
// The tail: one lane per output point (frame j, row m), 256 at a time and up to four of them a lane in flight; it
// reads its 2 W neighbours along each axis, forms the deltas in fp64 one IEEE operation at a time and stores the
// whole row.
#include "band_sums.hpp"
#include "pca_common.h"
#include "stft_body.hpp"

#include <float.h>
#include <math.h>

#include <mutex>

namespace pca {
namespace {

struct DeltaJob {
  BandsJob b;          // n_bands holds F, the rows of a frame; the bank's pointers are null on grid sets
  float* values;       // [B][T][F]
  int32_t* tickets;    // [B], zero on entry and on exit
  int banded, axes, W, Wt;
};

// The tail of a slot's last workgroup: the rows of the slot from its finished values.  One lane per output
// point (j, m), U points a lane in flight: all loads of the U are requested before the first is used - a trip
// of the loop is one round of loads from beyond this chip's L2, and the trips are what the tail costs
// (measured).  U comes from a budget of 32 registers, which keeps the kernel at the frame
// stage's 8 waves a SIMD; with four everywhere it fell to 4 and the launch got slower.  The arithmetic of a
// point is the header's, one IEEE operation at a time, whatever the batching.  Templated on the width and the
// axes so that the loads of a point are a fixed list.
template <int W, int AXES>
__device__ __forceinline__ void delta_tail(const DeltaJob& a, const float* __restrict__ slot, int b, int tid) {
#pragma clang fp contract(off)          // the header's operations one by one, no fused multiply-add
  constexpr bool DT = (AXES & 1) != 0, DF = (AXES & 2) != 0;
  constexpr int PER = 3 + 2 * W * (AXES == 3 ? 2 : 1);              // registers a point holds between load and use
  constexpr int U = 32 / PER > 4 ? 4 : (32 / PER < 1 ? 1 : 32 / PER);   // points a lane has in flight: 4 .. 1
  const int F = a.b.n_bands, n_out = a.b.Nt * F;
  const double D = (double)(W * (W + 1) * (2 * W + 1) / 3);          // 2 (1 + 4 + .. + W^2)
  const float* __restrict__ farr = a.b.farr;
  const float* __restrict__ tarr = a.b.tarr;
  float* __restrict__ out = a.b.out;
  for (int p0 = tid; p0 < n_out; p0 += 256 * U) {
    float c0[U], tj[U], v[U], tp[DT ? U : 1][W], tm[DT ? U : 1][W], fp[DF ? U : 1][W], fm[DF ? U : 1][W];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int pt = p0 + i * 256 < n_out ? p0 + i * 256 : n_out - 1;   // a lane past the end re-reads the last
      const int j = pt / F, m = pt - j * F;
      const float* row = slot + (int64_t)(a.Wt + j) * F;
      c0[i] = farr[m];
      tj[i] = tarr != nullptr ? tarr[j] : 0.f;
      v[i] = row[m];
      if (DT) {
#pragma unroll
        for (int n = 1; n <= W; ++n) {
          tp[i][n - 1] = row[m + (int64_t)n * F];
          tm[i][n - 1] = row[m - (int64_t)n * F];
        }
      }
      if (DF) {
#pragma unroll
        for (int n = 1; n <= W; ++n) {
          fp[i][n - 1] = row[m + n < F ? m + n : F - 1];
          fm[i][n - 1] = row[m - n > 0 ? m - n : 0];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int pt = p0 + i * 256;
      if (pt >= n_out) break;
      float dt = 0.f, df = 0.f;
      if (DT) {
        double acc = 0.0;
#pragma unroll
        for (int n = 1; n <= W; ++n) acc = acc + (double)n * ((double)tp[i][n - 1] - (double)tm[i][n - 1]);
        dt = (float)(acc / D);
      }
      if (DF) {
        double acc = 0.0;
#pragma unroll
        for (int n = 1; n <= W; ++n) acc = acc + (double)n * ((double)fp[i][n - 1] - (double)fm[i][n - 1]);
        df = (float)(acc / D);
      }
      const float d0 = DT ? dt : df;                                // the first delta column
      const int64_t at = (int64_t)b * n_out + pt;
      if (tarr != nullptr) {                                        // (f, t, v, d0)
        reinterpret_cast<float4*>(out)[at] = make_float4(c0[i], tj[i], v[i], d0);
      } else if (AXES == 3) {                                       // (f, v, dt, df)
        reinterpret_cast<float4*>(out)[at] = make_float4(c0[i], v[i], dt, df);
      } else {                                                      // (f, v, d0)
        float* o = out + at * 3;
        o[0] = c0[i];
        o[1] = v[i];
        o[2] = d0;
      }
    }
  }
}

template <int W>
__device__ __forceinline__ void delta_tail_axes(const DeltaJob& a, const float* slot, int b, int tid) {
  if (a.axes == 1) delta_tail<W, 1>(a, slot, b, tid);               // (uniform)
  else if (a.axes == 2) delta_tail<W, 2>(a, slot, b, tid);
  else delta_tail<W, 3>(a, slot, b, tid);
}

// Workgroup (u, b): frame u - Wt of the set in batch slot b; frames outside [Wt, Wt + Nt) are context.
__global__ __launch_bounds__(256) void k_frame_points_delta(const DeltaJob a) {
  extern __shared__ __attribute__((aligned(16))) double2 lds_c[];
  double2* x = lds_c;                   // [n_fft]
  double2* tw = lds_c + a.b.n_fft;      // [n_fft/2]
  const int tid = threadIdx.x, u = blockIdx.x, b = blockIdx.y;
  const int F = a.b.n_bands, T = a.b.Nt + 2 * a.Wt;

  BandsSlot s;
  if (!bands_slot(a.b, b, s)) return;   // (uniform over the grid) no set: no ticket is drawn, no row written
  int64_t centre = s.first + (int64_t)(u - a.Wt) * a.b.hop;
  centre = centre < 0 ? 0 : (centre > s.L ? s.L : centre);   // context outside the clip repeats its end frames
  if (u == a.Wt && tid == 0) bands_write_meta(a.b, b, s, centre);

  stft_frame_fft(x, tw, a.b.waves + s.w0, s.L, centre - a.b.n_fft / 2, a.b.n_fft, a.b.log2n, s.win, (double)s.g,
                 tid);

  float* slot = a.values + (int64_t)b * T * F;
  float* mine = slot + (int64_t)u * F;
  if (!a.banded) {                      // (uniform) k_frame_points' value of every bin
    const double inv = 1.0 / (double)(a.b.norm_mode == 0 ? a.b.n_fft : s.win);
    for (int f = tid; f < F; f += 256)
      __hip_atomic_store(reinterpret_cast<unsigned*>(mine + f), __float_as_uint(stft_logmag_bin(x[f], inv)),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {                              // k_frame_points_bands' value of every band
    const double* p = bands_energy_terms(a.b, x, tw, s.win, tid);
    const int q = tid & 3;
    for (int m0 = 0; m0 < F; m0 += 64) {
      const int m = m0 + (tid >> 2);
      const double e = bands_sum(a.b, p, m, q);
      if (q == 0 && m < F)
        __hip_atomic_store(reinterpret_cast<unsigned*>(mine + m), __float_as_uint(logf(a.b.amin + (float)e)),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }

  // publish, then draw the ticket.  The LDS is dead once every wave is past the barrier: its first word
  // carries the ticket
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

  // the slot's last workgroup: the deltas, one lane per output point
  switch (a.W) {                        // (uniform)
    case 1: delta_tail_axes<1>(a, slot, b, tid); break;
    case 2: delta_tail_axes<2>(a, slot, b, tid); break;
    case 3: delta_tail_axes<3>(a, slot, b, tid); break;
    default: delta_tail_axes<4>(a, slot, b, tid); break;
  }
  if (tid == 0) __hip_atomic_store(a.tickets + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace
}  // namespace pca

extern "C" {

int pca_frame_points_delta(const float* waves, const int64_t* wave_off, const int64_t* set_off, int n_clips,
                           int64_t max_len, int64_t min_len, const int64_t* clip_labels, const int64_t* idx,
                           int B, int n_fft, int hop, int n_bins, int Nt, const float* farr, const float* tarr,
                           const PcaFrameAug* aug, const PcaFrameBands* bands, const PcaDelta* delta,
                           float* value_ws, int64_t value_ws_elems, int32_t* tickets, float* out,
                           int64_t* labels_out, int32_t* meta_out, void* stream) {
  PCA_REQUIRE(waves && wave_off && set_off && idx && farr && aug && delta && value_ws && tickets && out,
              "frame_points_delta: null pointer");
  PCA_REQUIRE(aug->win_lengths != nullptr, "frame_points_delta: null win_lengths");
  PCA_REQUIRE((clip_labels == nullptr) == (labels_out == nullptr),
              "frame_points_delta: clip_labels and labels_out go together");
  PCA_REQUIRE(n_clips > 0, "frame_points_delta: n_clips=%d", n_clips);
  PCA_REQUIRE(n_fft >= 64 && n_fft <= 4096 && (n_fft & (n_fft - 1)) == 0,
              "frame_points_delta: n_fft=%d must be a power of two in [64, 4096]", n_fft);
  PCA_REQUIRE(hop > 0, "frame_points_delta: hop=%d", hop);
  PCA_REQUIRE(n_bins > 0 && n_bins <= n_fft / 2 + 1, "frame_points_delta: n_bins=%d", n_bins);
  if (bands != nullptr) {
    PCA_REQUIRE(bands->band_lo && bands->band_off && bands->weights,
                "frame_points_delta: null pointer in the bank");
    PCA_REQUIRE(bands->n_bands >= 1, "frame_points_delta: n_bands=%d", bands->n_bands);
    PCA_REQUIRE(bands->nnz >= bands->n_bands, "frame_points_delta: nnz=%d below n_bands=%d", bands->nnz,
                bands->n_bands);
    PCA_REQUIRE(bands->power == 1 || bands->power == 2, "frame_points_delta: power=%d (1: magnitude, 2: power)",
                bands->power);
    PCA_REQUIRE(bands->amin > 0.f && bands->amin <= FLT_MAX,
                "frame_points_delta: amin=%g must be finite and > 0", (double)bands->amin);
  }
  const int F = bands != nullptr ? bands->n_bands : n_bins;
  PCA_REQUIRE(B > 0 && B <= 65535 && Nt > 0, "frame_points_delta: B=%d Nt=%d", B, Nt);
  PCA_REQUIRE((int64_t)Nt * F <= 16384, "frame_points_delta: %lld points per set (max 16384)",
              (long long)Nt * F);
  PCA_REQUIRE(min_len > n_fft / 2 && max_len >= min_len,
              "frame_points_delta: reflect padding needs every clip longer than n_fft/2 "
              "(shortest %lld, longest %lld)", (long long)min_len, (long long)max_len);
  PCA_REQUIRE(max_len <= INT32_MAX,
              "frame_points_delta: a clip of %lld samples (meta holds int32 centres)", (long long)max_len);
  PCA_REQUIRE(aug->jitter >= 0 && aug->jitter <= (1 << 30), "frame_points_delta: jitter=%d", aug->jitter);
  PCA_REQUIRE(aug->gain_db >= 0.f && aug->gain_db <= 200.f,
              "frame_points_delta: gain_db=%g must be finite and in [0, 200]", (double)aug->gain_db);
  PCA_REQUIRE(aug->n_win >= 1, "frame_points_delta: n_win=%d", aug->n_win);
  PCA_REQUIRE(aug->norm_mode == 0 || aug->norm_mode == 1, "frame_points_delta: norm_mode=%d", aug->norm_mode);
  PCA_REQUIRE(delta->axes >= 1 && delta->axes <= 3, "frame_points_delta: axes=%d outside [1, 3]", delta->axes);
  PCA_REQUIRE(delta->width >= 1 && delta->width <= 4, "frame_points_delta: width=%d outside [1, 4]",
              delta->width);
  const int din = (tarr != nullptr ? 3 : 2) + (delta->axes == 3 ? 2 : 1);
  PCA_REQUIRE(din <= 4, "frame_points_delta: din=%d (a set with a time column takes one axis; max 4)", din);
  const int Wt = (delta->axes & 1) ? delta->width : 0;
  const int64_t T = (int64_t)Nt + 2 * Wt;
  PCA_REQUIRE(value_ws_elems >= 0 && (int64_t)B * T * F <= value_ws_elems,
              "frame_points_delta: the workspace holds %lld floats, B=%d slots of (Nt + 2 Wt) * F = %lld need "
              "%lld", (long long)value_ws_elems, B, (long long)(T * F), (long long)((int64_t)B * T * F));
  pca::DeltaJob p{};
  pca::BandsJob& j = p.b;
  j.waves = waves; j.wave_off = wave_off; j.set_off = set_off; j.clip_labels = clip_labels;
  j.idx = idx; j.farr = farr; j.tarr = tarr; j.win_lengths = aug->win_lengths;
  j.draw_dev = aug->draw_dev; j.out = out; j.labels_out = labels_out; j.meta_out = meta_out;
  j.seed = aug->seed; j.draw = aug->draw; j.n_clips = n_clips; j.n_fft = n_fft; j.hop = hop;
  j.n_bands = F; j.Nt = Nt;
  j.jitter = aug->jitter; j.n_win = aug->n_win; j.norm_mode = aug->norm_mode; j.gain_db = aug->gain_db;
  if (bands != nullptr) {
    j.band_lo = bands->band_lo; j.band_off = bands->band_off; j.weights = bands->weights;
    j.nnz = bands->nnz; j.power = bands->power; j.amin = bands->amin;
    p.banded = 1;
  }
  while ((1 << j.log2n) < n_fft) ++j.log2n;
  p.values = value_ws; p.tickets = tickets; p.axes = delta->axes; p.W = delta->width; p.Wt = Wt;
  static std::once_flag lds_once;   // allow > 64 KiB of dynamic LDS (96 KiB at n_fft 4096)
  std::call_once(lds_once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pca::k_frame_points_delta),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
  });
  hipLaunchKernelGGL(pca::k_frame_points_delta, dim3((unsigned)T, (unsigned)B), dim3(256),
                     pca::stft_lds_bytes(n_fft), pca::as_stream(stream), p);
  return pca::check_launch("k_frame_points_delta");
}
}
