// Spectral-peak point sets: pick, refine, rank and pack the peaks of packed point sets on the device.
//
// No reference counterpart: the reference keeps grid points only (all bins, max-K, random-K, its heat
// map).  A peak is a local maximum of the value column over a (2 radius_f + 1) x (2 radius_t + 1) window of
// the set's own grid; with `refine` its frequency and level come from the parabola through the
// log-magnitudes of the bin and its two frequency neighbours - the first off-grid points of this code
// base.  Contracts: pca_peak_points in include/pca_hip.h.
//
// One workgroup of 1024 threads per set:
//   1. the value column is staged in LDS once (N floats); a workgroup min of (desc_key, p) gives both
//      vmax and the row a set without peaks falls back to
//   2. every thread tests its points p = 1024 u + tid against the LDS copy (early exit on the first
//      neighbour that beats it)
//   3. the surviving (desc_key, p) pairs are compacted in point order into a second LDS array: wave
//      ballot + popcount prefix, one scan over the (pass, wave) totals
//   4. only next_pow2(count) keys go through lds_sort_asc_1024 - at most N / 2, usually far fewer
//   5. the first K are refined in fp64 and written; rows behind them are zeros
// No atomics: the same arguments give the same bits.  HBM traffic: N rows read, K rows written.
// LDS at N = 16384: 64 KiB of values + at most 64 KiB of keys.
#include "pca_common.h"
#include "select_keys.hpp"
#include "lds_sort.hpp"

#include <math.h>
#include <stdint.h>

namespace pca {
namespace {

constexpr int PEAK_THREADS = 1024, PEAK_WAVES = PEAK_THREADS / 64, PEAK_PASSES = 16;
// 8-byte LDS slots behind the keys: the waves' minima, the (pass, wave) counts, the total
constexpr int PEAK_SMALL_SLOTS = PEAK_WAVES + PEAK_PASSES * PEAK_WAVES / 2 + 1;

// fp64 parabola through (x-, a), (x0, b), (x+, c), b the peak: each result rounded to fp32 once.  Contraction
// is off so that the fp64 intermediates are those of the plain expressions.
__device__ __forceinline__ void refine_peak(float a, float b, float c, float xm, float x0, float xp,
                                            float* f_hat, float* v_hat) {
#pragma clang fp contract(off)
  *f_hat = x0;
  *v_hat = b;
  if (!(isfinite(a) && isfinite(b) && isfinite(c))) return;
  const double da = a, db = b, dc = c;
  const double den = (da - db) + (dc - db);              // < 0 at a peak: b > a, b >= c
  const double delta = 0.5 * (da - dc) / den;            // in (-1/2, 1/2]
  const double step = delta >= 0.0 ? (double)xp - (double)x0 : (double)x0 - (double)xm;
  *f_hat = (float)((double)x0 + delta * step);
  *v_hat = (float)(db - 0.25 * (da - dc) * delta);
}

__global__ __launch_bounds__(PEAK_THREADS) void k_peak_points(
    const float* __restrict__ X, const int32_t* __restrict__ lengths_in, int F, int Nt, int din,
    PcaPeakSpec spec, int K, float* __restrict__ out, int32_t* __restrict__ lengths_out,
    int32_t* __restrict__ count_out, int32_t* __restrict__ sel, int vals_slots, int key_slots) {
  // all of it dynamic: a static array would count against the 160 KiB the launcher asks for
  extern __shared__ uint64_t lds64[];
  float* vals = reinterpret_cast<float*>(lds64);               // [N] the value column
  uint64_t* keys = lds64 + vals_slots;                         // [next_pow2(most peaks a set can hold)]
  uint64_t* s_red = keys + key_slots;                          // [PEAK_WAVES]
  int* s_cnt = reinterpret_cast<int*>(s_red + PEAK_WAVES);     // peaks per (pass, wave), then their offsets
  int& s_total = s_cnt[PEAK_PASSES * PEAK_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = F * Nt;
  int Tv = Nt;                                                 // valid frames of this set
  if (lengths_in != nullptr) {
    Tv = lengths_in[b] / F;
    Tv = Tv < 1 ? 1 : (Tv > Nt ? Nt : Tv);
  }
  const int Nv = Tv * F;
  const float* __restrict__ xb = X + (int64_t)b * N * din;

  // 1. stage the values; min of (desc_key, p) over the valid points
  uint64_t best = ~0ull;
  for (int p = tid; p < Nv; p += PEAK_THREADS) {
    const float v = xb[(int64_t)p * din + (din - 1)];
    vals[p] = v;
    const uint64_t k = ((uint64_t)desc_key(v) << 32) | (uint32_t)p;
    best = k < best ? k : best;
  }
  for (int d = 32; d > 0; d >>= 1) {
    const uint64_t o = __shfl_xor(best, d);
    best = o < best ? o : best;
  }
  if (lane == 0) s_red[wave] = best;
  for (int i = tid; i < PEAK_PASSES * PEAK_WAVES; i += PEAK_THREADS) s_cnt[i] = 0;
  __syncthreads();
  best = s_red[0];
  for (int w = 1; w < PEAK_WAVES; ++w) best = s_red[w] < best ? s_red[w] : best;
  const int p_first = (int)(uint32_t)best;                     // first point in max-K order (Nv >= F >= 3)
  const float vmax = vals[p_first];                            // NaN only when every valid value is NaN
  const bool rel_on = spec.rel_floor < INFINITY;
  const float rel_cut = vmax - spec.rel_floor;

  // 2. + 3a. test this thread's points; count the survivors per (pass, wave)
  const int rf = spec.radius_f, rt = spec.radius_t;
  uint32_t flags = 0;
#pragma unroll 1
  for (int u = 0; u * PEAK_THREADS < Nv; ++u) {
    const int p = u * PEAK_THREADS + tid;
    bool peak = false;
    if (p < Nv) {
      const int t = p / F, f = p - t * F;
      const float v = vals[p];
      peak = f >= 1 && f <= F - 2 && v == v && v >= spec.abs_floor && (!rel_on || v >= rel_cut) &&
             !(vals[p - 1] >= v) && !(vals[p + 1] > v);
      if (peak) {
        const int f0 = f - rf < 0 ? 0 : f - rf, f1 = f + rf > F - 1 ? F - 1 : f + rf;
        const int t0 = t - rt < 0 ? 0 : t - rt, t1 = t + rt > Tv - 1 ? Tv - 1 : t + rt;
        for (int tt = t0; tt <= t1 && peak; ++tt) {
          const int row = tt * F;
          for (int q = row + f0; q <= row + f1; ++q) {
            const float w = vals[q];
            if (w > v || (w == v && q < p)) {                  // (value, -index) order; NaN loses
              peak = false;
              break;
            }
          }
        }
      }
    }
    const uint64_t m = __ballot(peak);
    if (peak) flags |= 1u << u;
    if (lane == 0) s_cnt[u * PEAK_WAVES + wave] = __popcll(m);
  }
  __syncthreads();
  // 3b. exclusive scan of the 256 (pass, wave) totals by wave 0, four entries per lane
  if (tid < 64) {
    const int a0 = s_cnt[4 * tid], a1 = s_cnt[4 * tid + 1], a2 = s_cnt[4 * tid + 2],
              a3 = s_cnt[4 * tid + 3];
    const int s = a0 + a1 + a2 + a3;
    int inc = s;
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d);
      if (tid >= d) inc += o;
    }
    const int ex = inc - s;
    s_cnt[4 * tid] = ex;
    s_cnt[4 * tid + 1] = ex + a0;
    s_cnt[4 * tid + 2] = ex + a0 + a1;
    s_cnt[4 * tid + 3] = ex + a0 + a1 + a2;
    if (tid == 63) s_total = inc;
  }
  __syncthreads();
  const int count = s_total;
  // 3c. the survivors' keys, in point order
#pragma unroll 1
  for (int u = 0; u * PEAK_THREADS < Nv; ++u) {
    const bool peak = (flags >> u) & 1u;
    const uint64_t m = __ballot(peak);
    if (peak) {
      const int p = u * PEAK_THREADS + tid;
      const int at = s_cnt[u * PEAK_WAVES + wave] + __popcll(m & ((1ull << lane) - 1ull));
      keys[at] = ((uint64_t)desc_key(vals[p]) << 32) | (uint32_t)p;
    }
  }
  // 4. sort next_pow2(count) keys
  if (count > 1) {
    int Np = 2;
    while (Np < count) Np <<= 1;
    for (int i = count + tid; i < Np; i += PEAK_THREADS) keys[i] = ~0ull;
    __syncthreads();
    lds_sort_asc_1024(keys, Np, tid);
  } else {
    __syncthreads();
  }
  // 5. refine and write the first min(count, K); a set without peaks yields its first point, unrefined
  const int n_out = count < 1 ? 1 : (count > K ? K : count);
  if (tid == 0) {
    lengths_out[b] = n_out;
    if (count_out != nullptr) count_out[b] = count;
  }
  for (int q = tid; q < K; q += PEAK_THREADS) {
    float* o = out + ((int64_t)b * K + q) * din;
    int p = -1;
    float x0 = 0.f, tm = 0.f, v = 0.f;
    if (q < n_out) {
      p = count > 0 ? (int)(uint32_t)keys[q] : p_first;
      const float* r = xb + (int64_t)p * din;
      x0 = r[0];
      tm = din == 3 ? r[1] : 0.f;
      v = vals[p];
      if (spec.refine && count > 0)                            // a peak has both frequency neighbours
        refine_peak(vals[p - 1], v, vals[p + 1], r[-din], x0, r[din], &x0, &v);
    }
    o[0] = x0;
    if (din == 3) o[1] = tm;
    o[din - 1] = v;
    if (sel != nullptr) sel[(int64_t)b * K + q] = p;
  }
}

}  // namespace
}  // namespace pca

extern "C" int pca_peak_points(const float* X, const int32_t* lengths_in, int B, int F, int Nt, int din,
                               const PcaPeakSpec* spec, int K, float* out, int32_t* lengths_out,
                               int32_t* count_out, int32_t* sel, void* stream) {
  // the shape first, so that a bad argument is named whatever the pointers are
  PCA_REQUIRE(B > 0, "peak_points: B=%d", B);
  PCA_REQUIRE(F >= 3, "peak_points: F=%d (a peak needs both frequency neighbours: F >= 3)", F);
  PCA_REQUIRE(Nt >= 1, "peak_points: Nt=%d", Nt);
  PCA_REQUIRE(din == 2 || din == 3, "peak_points: din=%d (2 or 3)", din);
  PCA_REQUIRE(din == 3 || Nt == 1, "peak_points: din=2 rows carry no time: Nt=%d must be 1", Nt);
  const int64_t N = (int64_t)F * Nt;
  PCA_REQUIRE(N <= 16384, "peak_points: N = F*Nt = %lld points per set (max 16384)", (long long)N);
  PCA_REQUIRE(K >= 1 && K <= N, "peak_points: K=%d outside [1, %lld]", K, (long long)N);
  PCA_REQUIRE(spec != nullptr, "peak_points: spec is null");
  PCA_REQUIRE(spec->radius_f >= 1 && spec->radius_f <= 16, "peak_points: radius_f=%d outside [1, 16]",
              spec->radius_f);
  PCA_REQUIRE(spec->radius_t >= 0 && spec->radius_t <= 4, "peak_points: radius_t=%d outside [0, 4]",
              spec->radius_t);
  PCA_REQUIRE(spec->rel_floor >= 0.0f, "peak_points: rel_floor=%g (>= 0, +inf = off)",
              (double)spec->rel_floor);
  PCA_REQUIRE(spec->abs_floor == spec->abs_floor, "peak_points: abs_floor is NaN (-inf = off)");
  PCA_REQUIRE(spec->refine == 0 || spec->refine == 1, "peak_points: refine=%d (0 or 1)", spec->refine);
  PCA_REQUIRE(X && out && lengths_out, "peak_points: null pointer (X, out, lengths_out)");
  const char* x0 = reinterpret_cast<const char*>(X);
  const char* o0 = reinterpret_cast<const char*>(out);
  PCA_REQUIRE(o0 + (int64_t)B * K * din * 4 <= x0 || x0 + (int64_t)B * N * din * 4 <= o0,
              "peak_points: out overlaps X");
  PCA_TRY(pca::no_stale_pack("pca_peak_points", false));
  // LDS: the values (padded to whole 8-byte slots), then next_pow2(most peaks) keys; a frame holds at
  // most ceil((F - 2) / 2) peaks
  const int64_t most = (int64_t)((F - 1) / 2) * Nt;
  int Np = 2;
  while (Np < most) Np <<= 1;
  const int vals_slots = (int)((N + 1) / 2);
  pca::allow_lds160<pca::k_peak_points>();
  hipLaunchKernelGGL(pca::k_peak_points, dim3((unsigned)B), dim3(pca::PEAK_THREADS),
                     (size_t)(vals_slots + Np + pca::PEAK_SMALL_SLOTS) * sizeof(uint64_t),
                     pca::as_stream(stream), X, lengths_in, F, Nt, din, *spec, K, out, lengths_out, count_out,
                     sel, vals_slots, Np);
  return pca::check_launch("k_peak_points");
}
