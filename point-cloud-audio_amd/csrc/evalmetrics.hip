// Held-out metrics of a whole [n_rows, C] logit buffer in one call: per-row loss, prediction and rank of
// the label, the counters, the confusion matrix and the fp64 loss sum.
//
//   k_eval_metrics_lane  : C <= 64.  A workgroup of 128 lanes stages 128 consecutive rows into LDS with
//                          coalesced loads (row stride C | 1 words: odd, so the 32 lanes of a half-wave
//                          that then read column j of 32 different rows hit 32 different banks); each
//                          lane walks ITS row twice (maximum / argmax, then sum-exp and rank) with no
//                          cross-lane step.  The confusion matrix is an int32 histogram in LDS that
//                          lives across the workgroup's row blocks and is flushed once, non-zero cells only.
//   k_eval_metrics_wave  : C > 64.  A wave per row, C a loop bound; confusion cells by integer atomics.
//   k_eval_metrics_merge : one workgroup adds the workgroups' partials in index order
//
// replaces: Code/settransformer.py:121-130 (per test batch: criterion(...).item(), argmax, compare, sum
//           and a second .item()).
//
// No floating-point atomics.  Workgroup g owns the row blocks g, g + G, g + 2G, ... (G depends on n_rows
// and C only); a lane adds its rows' losses in fp64 in that order, the lanes are summed by a fixed
// butterfly, the waves in wave order, and the merge kernel sums the G partials in a fixed pattern: the same
// call gives the same bits whatever order the workgroups run in.  Everything else is integer adds.
#include "pca_common.h"

#include <cmath>

namespace pca {
namespace {

constexpr int kLaneRows = 128;         // rows per block = lanes per workgroup of the C <= 64 kernel
constexpr int kLaneMaxC = 64;
constexpr int kWaveWaves = 4;          // rows in flight per workgroup of the C > 64 kernel
constexpr int kMaxGrid = 1024;         // workgroups (= partials) of either kernel
constexpr int kMergeThreads = 256;

// torch.argmax order of two (value, index) candidates, as k_eval_tally (train_ops.hip) and
// k_clip_aggregate (clip.hip): NaN is the maximum, equal values (and two NaNs) go to the lower index
__device__ inline bool argmax_before(float a, int ia, float b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na != nb) return na;
  if (!na && a != b) return a > b;
  return ia < ib;
}

__device__ inline double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ inline long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct RowOut {
  float* loss;
  int64_t* pred;
  int32_t* rank;
};

// what one scored / skipped row adds to its owner's accumulators
struct Acc {
  double loss = 0.0;
  int scored = 0, top1 = 0, topk = 0, skipped = 0;
};

// a row's results: outputs and accumulators (ok = the label is a class)
__device__ inline void finish_row(const RowOut& o, int64_t r, bool ok, float m, float s, float lv,
                                  int am, int rank, int topk, Acc& a) {
  const float loss = ok ? logf(s) + (m - lv) : 0.f;
  if (o.loss) o.loss[r] = loss;
  if (o.pred) o.pred[r] = am;
  if (o.rank) o.rank[r] = ok ? rank : -1;
  if (ok) {
    a.loss += (double)loss;
    a.scored += 1;
    a.top1 += rank == 0;
    a.topk += rank < topk;
  } else {
    a.skipped += 1;
  }
}

// the workgroup's partial: lanes by butterfly, waves in wave order (red: one slot per wave)
template <int WAVES>
__device__ inline void write_partial(const Acc& a, int g, int G, double* part_loss,
                                     long long* part_cnt, double* red_d, long long* red_c) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const double d = wave_sum_f64(a.loss);
  const long long c0 = wave_sum_i64(a.scored), c1 = wave_sum_i64(a.top1);
  const long long c2 = wave_sum_i64(a.topk), c3 = wave_sum_i64(a.skipped);
  if (lane == 0) {
    red_d[w] = d;
    red_c[4 * w] = c0; red_c[4 * w + 1] = c1; red_c[4 * w + 2] = c2; red_c[4 * w + 3] = c3;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sd = red_d[0];
    for (int k = 1; k < WAVES; ++k) sd += red_d[k];
    part_loss[g] = sd;
    for (int q = 0; q < 4; ++q) {
      long long sc = 0;
      for (int k = 0; k < WAVES; ++k) sc += red_c[4 * k + q];
      part_cnt[(size_t)q * G + g] = sc;
    }
  }
}

__global__ __launch_bounds__(kLaneRows) void k_eval_metrics_lane(
    const float* __restrict__ logits, const int64_t* __restrict__ labels, int64_t n_rows, int C,
    int topk, int vec, RowOut out, unsigned long long* __restrict__ confusion,
    double* __restrict__ part_loss, long long* __restrict__ part_cnt) {
  extern __shared__ float smem[];
  __shared__ double red_d[kLaneRows / 64];
  __shared__ long long red_c[4 * (kLaneRows / 64)];
  const int S = C | 1;
  float* tile = smem;                                           // [kLaneRows][S]
  int* hist = reinterpret_cast<int*>(smem + kLaneRows * S);     // [C][C], with confusion only
  const int tid = threadIdx.x;
  const int64_t n_blocks = (n_rows + kLaneRows - 1) / kLaneRows;

  if (confusion) {
    for (int i = tid; i < C * C; i += kLaneRows) hist[i] = 0;
  }
  Acc acc;
  for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const int64_t r0 = b * kLaneRows;
    const int nr = n_rows - r0 < kLaneRows ? (int)(n_rows - r0) : kLaneRows;
    const unsigned total = (unsigned)nr * (unsigned)C;
    const float* __restrict__ src = logits + r0 * C;            // the block's rows are contiguous
    __syncthreads();                                            // the previous block's rows are read
    for (unsigned e = 4u * tid; e < total; e += 4u * kLaneRows) {
      float v[4];
      const unsigned left = total - e;
      if (vec && left >= 4u) {                                  // r0 * C and e are multiples of 4
        const float4 q = *reinterpret_cast<const float4*>(src + e);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (unsigned)k < left ? src[e + k] : 0.f;
      }
      unsigned row = e / (unsigned)C, col = e - row * (unsigned)C;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if ((unsigned)k < left) tile[row * S + col] = v[k];
        if (++col == (unsigned)C) { col = 0; ++row; }
      }
    }
    __syncthreads();

    if (tid < nr) {
      const float* row = tile + tid * S;
      const int64_t lab64 = labels[r0 + tid];
      const bool ok = lab64 >= 0 && lab64 < C;
      const int lab = ok ? (int)lab64 : 0;
      float m = row[0];
      int am = 0;
#pragma unroll 4
      for (int j = 1; j < C; ++j) {
        const float v = row[j];
        if (argmax_before(v, j, m, am)) { m = v; am = j; }
      }
      const float lv = row[lab];
      float s = 0.f;
      int rank = 0;
#pragma unroll 4
      for (int j = 0; j < C; ++j) {
        const float v = row[j];
        s += expf(v - m);
        rank += (j != lab && argmax_before(v, j, lv, lab)) ? 1 : 0;
      }
      finish_row(out, r0 + tid, ok, m, s, lv, am, rank, topk, acc);
      if (confusion && ok) atomicAdd(&hist[lab * C + am], 1);
    }
  }
  __syncthreads();
  if (confusion) {
    for (int i = tid; i < C * C; i += kLaneRows) {
      const int h = hist[i];
      if (h) atomicAdd(confusion + i, (unsigned long long)h);
    }
  }
  if (part_loss) write_partial<kLaneRows / 64>(acc, blockIdx.x, gridDim.x, part_loss, part_cnt, red_d, red_c);
}

__global__ __launch_bounds__(64 * kWaveWaves) void k_eval_metrics_wave(
    const float* __restrict__ logits, const int64_t* __restrict__ labels, int64_t n_rows, int C,
    int topk, RowOut out, unsigned long long* __restrict__ confusion,
    double* __restrict__ part_loss, long long* __restrict__ part_cnt) {
  __shared__ double red_d[kWaveWaves];
  __shared__ long long red_c[4 * kWaveWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  Acc acc;                                                      // lane 0 of a wave holds the wave's
  for (int64_t r = (int64_t)blockIdx.x * kWaveWaves + w; r < n_rows;
       r += (int64_t)gridDim.x * kWaveWaves) {
    const float* __restrict__ x = logits + r * C;
    float m = -INFINITY;
    int am = 0x7fffffff;
    for (int j = lane; j < C; j += 64) {
      const float v = x[j];
      if (argmax_before(v, j, m, am)) { m = v; am = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(m, o, 64);
      const int oa = __shfl_xor(am, o, 64);
      if (argmax_before(om, oa, m, am)) { m = om; am = oa; }
    }
    const int64_t lab64 = labels[r];
    const bool ok = lab64 >= 0 && lab64 < C;
    const int lab = ok ? (int)lab64 : 0;
    const float lv = x[lab];
    float s = 0.f;
    int rank = 0;
    for (int j = lane; j < C; j += 64) {
      const float v = x[j];
      s += expf(v - m);
      rank += (j != lab && argmax_before(v, j, lv, lab)) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s += __shfl_xor(s, o, 64);
      rank += __shfl_xor(rank, o, 64);
    }
    if (lane == 0) {
      finish_row(out, r, ok, m, s, lv, am, rank, topk, acc);
      if (confusion && ok) atomicAdd(confusion + (size_t)lab * C + am, 1ull);
    }
  }
  if (part_loss) write_partial<kWaveWaves>(acc, blockIdx.x, gridDim.x, part_loss, part_cnt, red_d, red_c);
}

// loss_sum[0] += sum of part_loss[0 .. G), counts[q] += sum of part_cnt[q][0 .. G): thread t takes t,
// t + 256, ... in that order, then the butterfly, then the waves in wave order
__global__ __launch_bounds__(kMergeThreads) void k_eval_metrics_merge(
    const double* __restrict__ part_loss, const long long* __restrict__ part_cnt, int G,
    double* __restrict__ loss_sum, unsigned long long* __restrict__ counts) {
  __shared__ double red_d[kMergeThreads / 64];
  __shared__ long long red_c[4 * (kMergeThreads / 64)];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double d = 0.0;
  long long c[4] = {0, 0, 0, 0};
  for (int i = tid; i < G; i += kMergeThreads) {
    d += part_loss[i];
#pragma unroll
    for (int q = 0; q < 4; ++q) c[q] += part_cnt[(size_t)q * G + i];
  }
  d = wave_sum_f64(d);
#pragma unroll
  for (int q = 0; q < 4; ++q) c[q] = wave_sum_i64(c[q]);
  if (lane == 0) {
    red_d[w] = d;
#pragma unroll
    for (int q = 0; q < 4; ++q) red_c[4 * w + q] = c[q];
  }
  __syncthreads();
  if (tid == 0) {
    double sd = red_d[0];
    for (int k = 1; k < kMergeThreads / 64; ++k) sd += red_d[k];
    if (loss_sum) loss_sum[0] += sd;
    if (counts) {
      for (int q = 0; q < 4; ++q) {
        long long sc = 0;
        for (int k = 0; k < kMergeThreads / 64; ++k) sc += red_c[4 * k + q];
        if (sc) atomicAdd(counts + q, (unsigned long long)sc);
      }
    }
  }
}

inline int grid_of(int64_t n_rows, int C) {
  const int64_t blocks = C <= kLaneMaxC ? cdiv(n_rows, kLaneRows) : cdiv(n_rows, kWaveWaves);
  return (int)(blocks < kMaxGrid ? blocks : kMaxGrid);
}

}  // namespace
}  // namespace pca

extern "C" {

size_t pca_eval_metrics_ws_bytes(int64_t n_rows) {
  if (n_rows <= 0) return 0;
  const int64_t g = pca::cdiv(n_rows, pca::kWaveWaves);         // the larger of the two grids
  return pca::align256((size_t)(g < pca::kMaxGrid ? g : pca::kMaxGrid) * 5 * sizeof(double));
}

int pca_eval_metrics(const float* logits, const int64_t* labels, int64_t n_rows, int C, int topk,
                     float* row_loss, int64_t* row_pred, int32_t* row_rank, int64_t* counts, int slot,
                     int64_t* confusion, double* loss_sum, void* ws, void* stream) {
  PCA_REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 40) && C >= 1 && topk >= 1,
              "eval_metrics: n_rows=%lld C=%d topk=%d", (long long)n_rows, C, topk);
  PCA_REQUIRE((logits && labels) || n_rows == 0, "eval_metrics: null pointer");
  PCA_REQUIRE(slot >= 0, "eval_metrics: slot=%d", slot);
  const bool sums = counts != nullptr || loss_sum != nullptr;
  PCA_REQUIRE(!sums || ws != nullptr || n_rows == 0,
              "eval_metrics: counts / loss_sum need the workspace of pca_eval_metrics_ws_bytes");
  if (n_rows == 0) return PCA_OK;
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counter width");
  hipStream_t st = pca::as_stream(stream);
  const int G = pca::grid_of(n_rows, C);
  double* part_loss = sums ? reinterpret_cast<double*>(ws) : nullptr;
  long long* part_cnt = sums ? reinterpret_cast<long long*>(part_loss + G) : nullptr;
  auto* conf = reinterpret_cast<unsigned long long*>(confusion);
  const pca::RowOut out{row_loss, row_pred, row_rank};
  if (C <= pca::kLaneMaxC) {
    const size_t lds = (size_t)pca::kLaneRows * (C | 1) * sizeof(float) +
                       (confusion ? (size_t)C * C * sizeof(int) : 0);       // 49 KB at most
    const int vec = (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
    hipLaunchKernelGGL(pca::k_eval_metrics_lane, dim3(G), dim3(pca::kLaneRows), lds, st, logits,
                       labels, n_rows, C, topk, vec, out, conf, part_loss, part_cnt);
    PCA_TRY(pca::check_launch("k_eval_metrics_lane"));
  } else {
    hipLaunchKernelGGL(pca::k_eval_metrics_wave, dim3(G), dim3(64 * pca::kWaveWaves), 0, st, logits,
                       labels, n_rows, C, topk, out, conf, part_loss, part_cnt);
    PCA_TRY(pca::check_launch("k_eval_metrics_wave"));
  }
  if (sums) {
    hipLaunchKernelGGL(pca::k_eval_metrics_merge, dim3(1), dim3(pca::kMergeThreads), 0, st, part_loss,
                       part_cnt, G, loss_sum,
                       counts ? reinterpret_cast<unsigned long long*>(counts + 4 * (int64_t)slot)
                              : nullptr);
    PCA_TRY(pca::check_launch("k_eval_metrics_merge"));
  }
  return PCA_OK;
}
}
