// The d = 128 weight-gradient engine (the peer of wgrad64.hip / wgrad256.hip): job tables in bwd_defer.hpp.
//
//   k_wgrad128     dW[128 x 128] += G^T.A over a row range (G = dZ|dQp|dKp.., A = O|X|H..), several jobs per
//                  launch: both operands come from row-major [point][feature] LDS images through
//                  ds_read_tr16_b64 (hardware transpose); the result leaves as a per-workgroup slab summed in
//                  a fixed order afterwards, or as fp32 atomics; column sums of G (bias gradients) ride along,
//                  and so do slab sums that are due now (rider rows).
//   k_wgrad128_step  the same body over the two deferred lists of a step (bf16 and fp32 operands) in one launch.
//   k_mab0_small_ride  the bf16 list of a step beside layer 1's few-queries backward (body:
//                  mab0_bwd_small_body.hpp), which needs the memory system as little as the list needs it.
//   k_wgrad_small  layer 1: dW[128 x dq] += G^T.X with dq <= 4 (body: terminal_bodies.hpp).
#include "bwd_defer.hpp"
#include "mab0_bwd_small_body.hpp"
#include "mfma_common.hpp"
#include "terminal_bodies.hpp"
#include "slab_sum_body.hpp"
#include <mutex>
#include <type_traits>

namespace pca {

namespace {

// ---------------------------------------------------------------------------------
// dW[DG x DA] += G[rows, DG]^T . A[rows, DA]  (+ db[DG] += column sums of G)
// ---------------------------------------------------------------------------------

// eight consecutive elements of an operand row as they were loaded: converted to bf16 only when the
// tile goes to LDS, so that a fetch is requests and nothing else and stays in flight until then
template <typename T> struct Raw8;
template <> struct Raw8<__bf16> { bf16x8 v; };
template <> struct Raw8<float> { float4 lo, hi; };
__device__ __forceinline__ void load_raw(Raw8<__bf16>& r, const __bf16* p) {
  r.v = *reinterpret_cast<const bf16x8*>(p);
}
__device__ __forceinline__ void load_raw(Raw8<float>& r, const float* p) {
  r.lo = reinterpret_cast<const float4*>(p)[0];
  r.hi = reinterpret_cast<const float4*>(p)[1];
}
__device__ __forceinline__ void zero_raw(Raw8<__bf16>& r) {
#pragma unroll
  for (int k = 0; k < 8; ++k) r.v[k] = (__bf16)0.f;
}
__device__ __forceinline__ void zero_raw(Raw8<float>& r) {
  r.lo = float4{0.f, 0.f, 0.f, 0.f};
  r.hi = float4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ bf16x8 to_bf16(const Raw8<__bf16>& r) { return r.v; }
__device__ __forceinline__ bf16x8 to_bf16(const Raw8<float>& r) {
  bf16x8 v;
  v[0] = (__bf16)r.lo.x; v[1] = (__bf16)r.lo.y; v[2] = (__bf16)r.lo.z; v[3] = (__bf16)r.lo.w;
  v[4] = (__bf16)r.hi.x; v[5] = (__bf16)r.hi.y; v[6] = (__bf16)r.hi.z; v[7] = (__bf16)r.hi.w;
  return v;
}
// one thread's share of a fetched 32-row tile pair: two 8-element chunks of G and of A, and the ReLU
// mask words of the G chunks (job.mask)
template <typename GT, typename AT>
struct WgradStage {
  Raw8<GT> g[2];
  Raw8<AT> a[2];
  uint32_t mk[2][2];
};

// One job's row range [blockIdx.x * rows_per_wg, ...) of dW += G^T.A (the body of k_wgrad128 and of the
// job rows of k_wgrad128_step).  `lds`: 64 KiB - 2 x 2 staging tiles per group during the loop, the fp32
// [128][128] result afterwards.
// Software-pipelined: DEPTH 32-row tile pairs per group are in flight as loads into register sets that
// rotate (unrolled by DEPTH: the sets are named statically) while the current one is consumed from
// LDS; two LDS buffers -> one barrier per tile.  A tile's wait is the counted one the compiler derives
// from the program order of the loads (the DEPTH - 1 later tiles stay in flight across the barrier),
// which is why the steady loop below holds no conditional load: steps whose tiles lie wholly inside
// the range for every group fetch unguarded (one uniform test per tile), and only the last steps of a
// range and a ragged last tile go through the guarded fetch with its zero fill.
// NG row groups of four waves each (NG = 2 for the long B*N-row jobs: twice the loads in flight
// per CU): group q takes the 32-row tiles q, q + NG, ...; the groups' [128][128] blocks are summed in
// LDS.
template <typename GT, typename AT, int NG, int DEPTH>
__device__ __forceinline__ void wgrad128_body(const WgradJob& job, int rows_per_wg, char* lds) {
  constexpr int D = 128, NT = 256 * NG;
  const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3, grp = tid >> 8;
  const int gtid = tid & 255;
  char (*sG)[32 * 256] = reinterpret_cast<char (*)[32 * 256]>(lds + grp * (4 * 32 * 256));
  char (*sA)[32 * 256] = reinterpret_cast<char (*)[32 * 256]>(lds + grp * (4 * 32 * 256) + 2 * 32 * 256);
  const GT* __restrict__ G = reinterpret_cast<const GT*>(job.G);
  const AT* __restrict__ A = reinterpret_cast<const AT*>(job.A);
  const int64_t M = job.M;
  const int r = lane & 15, g = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  if (r0 >= M) return;
  const int64_t r1 = (r0 + rows_per_wg < M) ? r0 + rows_per_wg : M;
  // steps (uniform over the groups: a group whose tile lies beyond r1 multiplies zeros), and how many
  // of them have every group's tile wholly inside [r0, r1)
  const int nrows = (int)(r1 - r0);
  const int nt = (nrows + 32 * NG - 1) / (32 * NG), nfull = nrows / (32 * NG);
  // wave w owns the 64 x 64 output block (G features 64*(w>>1).., A features 64*(w&1)..):
  // 4 + 4 transposed fragments feed 16 MFMAs per 32-row tile
  const int gt0 = 4 * (wave >> 1), at0 = 4 * (wave & 1);
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // column sums of G, columns 8*(tid&15)..

  // the loop, once per kind of job (with / without mask words: a load that only one kind issues
  // would make the other kind's counted waits count it too)
  auto run = [&](auto has_mask) {
    constexpr bool MASK = decltype(has_mask)::value;
    using Stage = WgradStage<GT, AT>;
    // features 8 ch .. 8 ch + 7 of row R: two nibbles (bit 4 t + e of lane (r, g) <-> feature
    // 16 t + 4 g + e, t = ch / 2) of the words of lanes g0 = 2 (ch & 1) and g0 + 1.  Only
    // requested with the tile; applied when the tile goes to LDS (the loads stay in flight meanwhile)
    auto fetch_row = [&](Stage& s, int e, int64_t R, int ch) {
      load_raw(s.g[e], G + R * D + ch * 8);
      load_raw(s.a[e], A + R * D + ch * 8);
      if (MASK) {
        const uint32_t* mw = job.mask + (R >> 4) * 64 + (R & 15) + 32 * (ch & 1);
        s.mk[e][0] = mw[0];
        s.mk[e][1] = mw[16];
      }
    };
    auto fetch_full = [&](Stage& s, int t) {          // step t < nfull: every row exists
      const int64_t base = r0 + 32 * ((int64_t)t * NG + grp);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int c = gtid + e * 256;
        fetch_row(s, e, base + (c >> 4), c & 15);
      }
    };
    auto fetch_any = [&](Stage& s, int t) {           // rows at and beyond r1 read as zeros
      if (t < nfull) {
        fetch_full(s, t);
      } else if (t < nt) {
        const int64_t base = r0 + 32 * ((int64_t)t * NG + grp);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int c = gtid + e * 256;
          if (base + (c >> 4) < r1) {
            fetch_row(s, e, base + (c >> 4), c & 15);
          } else {
            zero_raw(s.g[e]);
            zero_raw(s.a[e]);
          }
        }
      }
    };
    int buf = 0;
    // step t: set s (tile t) goes to LDS, then takes the loads of tile t + DEPTH
    auto step = [&](Stage& s, int t, auto full) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int c = gtid + e * 256;
        const int row = c >> 4, ch = c & 15;
        bf16x8 vg = to_bf16(s.g[e]);
        const bf16x8 va = to_bf16(s.a[e]);
        if (MASK) {
          const uint32_t n0 = s.mk[e][0] >> (4 * (ch >> 1)), n1 = s.mk[e][1] >> (4 * (ch >> 1));
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (!((n0 >> k) & 1u)) vg[k] = (__bf16)0.f;
            if (!((n1 >> k) & 1u)) vg[4 + k] = (__bf16)0.f;
          }
        }
        *reinterpret_cast<bf16x8*>(sG[buf] + tr_off(row, ch)) = vg;
        *reinterpret_cast<bf16x8*>(sA[buf] + tr_off(row, ch)) = va;
        if (job.db != nullptr) {
#pragma unroll
          for (int k = 0; k < 8; ++k) bs[k] += (float)vg[k];
        }
      }
      __syncthreads();
      if (decltype(full)::value) fetch_full(s, t + DEPTH);
      else fetch_any(s, t + DEPTH);
      __builtin_amdgcn_sched_barrier(0);      // the requests leave before this step's LDS reads and MFMAs
      bf16x8 ga[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) ga[i] = tr_frag(sG[buf], gt0 + i, lane);
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const bf16x8 ab = tr_frag(sA[buf], at0 + tt, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][tt] = mfma32(ga[i], ab, acc[i][tt]);
      }
      buf ^= 1;
    };
    Stage st[DEPTH];
#pragma unroll
    for (int u = 0; u < DEPTH; ++u)
#pragma unroll
      for (int e = 0; e < 2; ++e) st[u].mk[e][0] = st[u].mk[e][1] = ~0u;
    int t = 0;
    if (2 * DEPTH <= nfull) {
      // steady: the prologue and every fetch of the loop are full tiles, so the loop is entered
      // with all DEPTH sets requested in order and its waits count exactly
#pragma unroll
      for (int u = 0; u < DEPTH; ++u) {
        fetch_full(st[u], u);
        __builtin_amdgcn_sched_barrier(0);    // (the scheduler would request the first tile last)
      }
      for (; t + 2 * DEPTH <= nfull; t += DEPTH) {
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) step(st[u], t + u, std::true_type{});
      }
    } else {
#pragma unroll
      for (int u = 0; u < DEPTH; ++u) fetch_any(st[u], u);
    }
    for (; t < nt; t += DEPTH) {                      // the last steps and the ragged tile
#pragma unroll
      for (int u = 0; u < DEPTH; ++u)
        if (t + u < nt) step(st[u], t + u, std::false_type{});
    }
  };
  if (job.mask != nullptr) run(std::true_type{});
  else run(std::false_type{});

  // The atomics cost per cache-line transaction, not per lane: stage the [128][128] block in
  // LDS and add it with fully coalesced instructions (64 consecutive floats per wave) instead
  // of 16-float row fragments straight from the accumulator layout.
  __syncthreads();
  float* res = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int q = NG - 1; q >= 0; --q) {       // last group stores, the others add on top
    if (grp == q) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int grow = 16 * (gt0 + i) + 4 * g + e;
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            float* dst = &res[grow * D + 16 * (at0 + t) + r];
            *dst = (q == NG - 1) ? acc[i][t][e] : *dst + acc[i][t][e];
          }
        }
    }
    __syncthreads();
  }
  // slab mode: this workgroup's [rows][128] block (+ its 128 bias sums) as plain stores
  const int n1 = (job.g_hi - job.g_lo) * D;
  float* slab = job.slab == nullptr
                    ? nullptr
                    : job.slab + (int64_t)blockIdx.x * (n1 + (job.db != nullptr ? D : 0));
  if (slab != nullptr)
    for (int i = tid; i < n1; i += NT) slab[i] = res[job.g_lo * D + i];
  else
    for (int i = job.g_lo * D + tid; i < job.g_hi * D; i += NT) atomicAdd(&job.dW[i], res[i]);
  if (job.db != nullptr) {
    // threads with equal (tid & 15) hold partial sums of the same 8 columns
    __syncthreads();
    float* red = reinterpret_cast<float*>(lds);         // [16 NG groups][128 columns]
#pragma unroll
    for (int k = 0; k < 8; ++k) red[(tid >> 4) * D + (tid & 15) * 8 + k] = bs[k];
    __syncthreads();
    if (tid < D) {
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < 16 * NG; ++q) t += red[q * D + tid];
      if (slab != nullptr) slab[n1 + tid] = t;
      else atomicAdd(&job.db[tid], t);
    }
  }
}

// tile pairs in flight per row group: three for bf16 operands (96 KB per 512-thread workgroup beside
// the 64 accumulator registers), one for fp32 ones (their register sets are twice as large, and the
// fp32 jobs of a step are two steps long: two in flight measured the same k_wgrad128_step time)
template <typename GT, typename AT>
constexpr int wgrad128_depth() {
  return std::is_same<GT, __bf16>::value && std::is_same<AT, __bf16>::value ? 3 : 1;
}

// blockIdx.y selects the job; behind the jobs `sw_rows` rows of the layer-1 fc_v job (as in k_wgrad128_step
// below: NG blocks of rows per workgroup), then the rider rows
template <typename GT, typename AT, int NG>
__global__ __launch_bounds__(256 * NG) void k_wgrad128(const WgradJobs jobs, int rows_per_wg,
                                                       const SmallWgradArgs w, int sw_rows,
                                                       const SlabSumJobs riders) {
  __shared__ __attribute__((aligned(16))) char lds[4 * 32 * 256 * 2];
  if ((int)blockIdx.y >= jobs.n + sw_rows) {          // rider rows: partial sums that are due now
    slab_sum_body(riders.j[blockIdx.y - jobs.n - sw_rows], blockIdx.x, threadIdx.x,
                  reinterpret_cast<float4*>(lds));
    return;
  }
  if ((int)blockIdx.y >= jobs.n) {
    const int wg = ((int)blockIdx.y - jobs.n) * (int)gridDim.x + (int)blockIdx.x;
    if ((int64_t)wg * NG * w.rows_per_wg < w.M)      // (uniform per workgroup)
      wgrad_small_rows<float, 256 * NG>(w.G, w.X, w.M, w.dq, w.rows_per_wg, w.x_head_stride, w.dW, w.db, wg,
                                        w.slab, reinterpret_cast<float (*)[5]>(lds));
    return;
  }
  wgrad128_body<GT, AT, NG, wgrad128_depth<GT, AT>()>(jobs.j[blockIdx.y], rows_per_wg, lds);
}

// The two deferred lists of a step in one launch: rows [0, bf.n) of blockIdx.y are the bf16 jobs (the
// long ones, so they are placed first), then the fp32 jobs, then the rider rows.  Each list has its own
// rows per workgroup; a row whose blockIdx.x lies beyond its range leaves at once.  The operand type
// is uniform per workgroup, and both lists run two row groups.
// Behind the fp32 jobs, `sw_rows` rows of the layer-1 fc_v job (its workgroup = row * gridDim.x + blockIdx.x,
// so the rows are as wide as the grid; each half of a workgroup takes one block of rows_per_wg rows, the
// partition and the slabs of the 256-thread launch): it reads what layer 1's few-queries backward wrote, like
// the fp32 jobs, and its partials are summed with theirs in k_terminal1.
__global__ __launch_bounds__(512) void k_wgrad128_step(const WgradJobs bf, int rpw_bf,
                                                       const WgradJobs f32, int rpw_f32,
                                                       const SmallWgradArgs w, int sw_rows,
                                                       const SlabSumJobs riders) {
  __shared__ __attribute__((aligned(16))) char lds[4 * 32 * 256 * 2];
  const int y = blockIdx.y;
  if (y < bf.n) {
    wgrad128_body<__bf16, __bf16, 2, wgrad128_depth<__bf16, __bf16>()>(bf.j[y], rpw_bf, lds);
  } else if (y < bf.n + f32.n) {
    wgrad128_body<float, float, 2, wgrad128_depth<float, float>()>(f32.j[y - bf.n], rpw_f32, lds);
  } else if (y < bf.n + f32.n + sw_rows) {
    const int wg = (y - bf.n - f32.n) * (int)gridDim.x + (int)blockIdx.x;
    if ((int64_t)wg * 2 * w.rows_per_wg < w.M)       // (uniform per workgroup; two blocks of rows each)
      wgrad_small_rows<float, 512>(w.G, w.X, w.M, w.dq, w.rows_per_wg, w.x_head_stride, w.dW, w.db, wg,
                                   w.slab, reinterpret_cast<float (*)[5]>(lds));
  } else {
    // (32 loads in flight: when the bf16 list ran in k_mab0_small_ride nothing hides these chains)
    slab_sum_body<32>(riders.j[y - bf.n - f32.n - sw_rows], blockIdx.x, threadIdx.x,
                      reinterpret_cast<float4*>(lds));
  }
}

// The bf16 list of a step and layer 1's few-queries backward (one 512-thread workgroup per set: the
// partition of two 256-thread workgroups of k_mab0_bwd_small, see mab0_bwd_small_body.hpp) in one launch:
// the list's operands are ready before that backward runs and it does not read what the list writes, the
// list streams on three quarters of the compute units, and the set rows are a latency chain that moves
// about 1 MB.  blockIdx.y selects the row: the jobs, and `set_rows` rows of sets as wide as the job rows
// (set = row * gridDim.x + blockIdx.x; a workgroup that leaves at once still takes a compute unit's whole
// LDS and register file while it does, so the grid holds as few of them as the two extents allow); which
// kind is dispatched first is RIDE_SETS_FIRST (measured: DESIGN 4.4.4).  No workgroup waits for another.
constexpr bool RIDE_SETS_FIRST = false;
constexpr int RIDE_SET_LDS = 512 * 4 * 4 + PCA_POINT_CHUNK * 4 * 4 + MID_SMALL_FUSE_LDS;
constexpr int RIDE_LDS = RIDE_SET_LDS > 4 * 32 * 256 * 2 ? RIDE_SET_LDS : 4 * 32 * 256 * 2;
__global__ __launch_bounds__(512) void k_mab0_small_ride(const WgradJobs bf, int rpw_bf,
                                                         const Mab0SmallArgs sets, int B, int set_rows) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int y = RIDE_SETS_FIRST ? (int)blockIdx.y - set_rows : (int)blockIdx.y;
  if (y >= 0 && y < bf.n) {
    wgrad128_body<__bf16, __bf16, 2, wgrad128_depth<__bf16, __bf16>()>(bf.j[y], rpw_bf, lds);
    return;
  }
  const int b = (RIDE_SETS_FIRST ? (int)blockIdx.y : y - bf.n) * (int)gridDim.x + (int)blockIdx.x;
  if (b < B) {
    float (*sD)[4] = reinterpret_cast<float (*)[4]>(lds);
    float* sX = reinterpret_cast<float*>(lds + 512 * 4 * 4);
    mab0_bwd_small_body<true, 512>(sets, b, 0, 1, sD, sX, lds + 512 * 4 * 4 + PCA_POINT_CHUNK * 4 * 4);
  }
}

// layer 1: dW[D x dq] += dQp^T . X with dq <= 4 (fp32 X), db += colsum(dQp).
// 256 threads = 128 features x 2 row phases; 128 rows per workgroup, loads unrolled.
template <typename GT>
__global__ __launch_bounds__(256) void k_wgrad_small(const GT* __restrict__ G,
                                                     const float* __restrict__ X, int64_t M,
                                                     int dq, int rows_per_wg,
                                                     int64_t x_head_stride,   // A = X + (f/32)*stride
                                                     float* __restrict__ dW,
                                                     float* __restrict__ db) {
  wgrad_small_body<GT>(G, X, M, dq, rows_per_wg, x_head_stride, dW, db, blockIdx.x);
}

}  // namespace

int wgrad128_launch(const WgradJobs& jobs, bool g_bf16, bool a_bf16, int rows_per_wg, hipStream_t st,
                    const SlabSumJobs* riders_in, const SmallWgradArgs* sw) {
  const SlabSumJobs riders = riders_in != nullptr ? *riders_in : SlabSumJobs{};
  PCA_REQUIRE(sw == nullptr || wgrad_max_rows(jobs) > 0, "wgrad128: the small job rides with a list that has rows");
  if (wgrad_max_rows(jobs) == 0) return slab_sum_jobs(riders, st);
  unsigned gx, gy;
  int sw_rows = 0;
  PCA_TRY(wgrad128_shape(jobs, rows_per_wg, riders, sw, &gx, &gy, &sw_rows));
  const bool two = rows_per_wg >= 128;       // (two row groups per workgroup: wgrad128_shape)
  const SmallWgradArgs w = sw != nullptr ? *sw : SmallWgradArgs{};
  const dim3 grid(gx, gy);
  if (g_bf16 && a_bf16) {
    if (two) hipLaunchKernelGGL((k_wgrad128<__bf16, __bf16, 2>), grid, dim3(512), 0, st, jobs, rows_per_wg, w, sw_rows, riders);
    else hipLaunchKernelGGL((k_wgrad128<__bf16, __bf16, 1>), grid, dim3(256), 0, st, jobs, rows_per_wg, w, sw_rows, riders);
  } else if (g_bf16) {
    if (two) hipLaunchKernelGGL((k_wgrad128<__bf16, float, 2>), grid, dim3(512), 0, st, jobs, rows_per_wg, w, sw_rows, riders);
    else hipLaunchKernelGGL((k_wgrad128<__bf16, float, 1>), grid, dim3(256), 0, st, jobs, rows_per_wg, w, sw_rows, riders);
  } else if (!a_bf16) {
    if (two) hipLaunchKernelGGL((k_wgrad128<float, float, 2>), grid, dim3(512), 0, st, jobs, rows_per_wg, w, sw_rows, riders);
    else hipLaunchKernelGGL((k_wgrad128<float, float, 1>), grid, dim3(256), 0, st, jobs, rows_per_wg, w, sw_rows, riders);
  } else {
    set_error("wgrad128: fp32 G with bf16 A is not instantiated");
    return PCA_EUNSUPPORTED;
  }
  return check_launch("k_wgrad128");
}

int wgrad128_launch_step(const WgradJobs& bf, int rpw_bf, const WgradJobs& f32, int rpw_f32,
                         const WgradStepShape& shape, hipStream_t st, const SmallWgradArgs* sw) {
  hipLaunchKernelGGL(k_wgrad128_step, dim3(shape.gx, shape.gy), dim3(512), 0, st, bf, rpw_bf, f32, rpw_f32,
                     sw != nullptr ? *sw : SmallWgradArgs{}, shape.sw_rows, shape.riders);
  return check_launch("k_wgrad128_step");
}

int mab0_small_ride_launch(const WgradJobs& bf, int rpw_bf, const Mab0SmallArgs& sets, int B,
                           hipStream_t st) {
  PCA_REQUIRE(bf.n > 0 && wgrad_max_rows(bf) > 0 && rpw_bf >= 128,
              "mab0_small_ride: a bf16 list with rows, two row groups");
  PCA_REQUIRE(B > 0 && sets.R == 64 && sets.dk >= 1 && sets.dk <= 4 && sets.slabs != nullptr,
              "mab0_small_ride: R=%d dk=%d", sets.R, sets.dk);
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_mab0_small_ride),
                              hipFuncAttributeMaxDynamicSharedMemorySize, RIDE_LDS);
  });
  const unsigned gj = (unsigned)cdiv(wgrad_max_rows(bf), rpw_bf);
  const int set_rows = (int)cdiv(B, gj);
  hipLaunchKernelGGL(k_mab0_small_ride, dim3(gj, (unsigned)(bf.n + set_rows)), dim3(512), RIDE_LDS, st, bf,
                     rpw_bf, sets, B, set_rows);
  return check_launch("k_mab0_small_ride");
}

int wgrad128_defer(BwdDefer* defer, const WgradJobs& jobs, bool bf16, int rows_per_wg,
                   hipStream_t st) {
  if (defer == nullptr) return wgrad128_launch(jobs, bf16, bf16, rows_per_wg, st);
  WgradJobs& L = bf16 ? defer->wg_bf16 : defer->wg_f32;
  if (L.n + jobs.n > 16) {                 // table full: run what has been collected
    PCA_TRY(wgrad128_launch(L, bf16, bf16, bf16 ? 512 : 64, st));
    L.n = 0;
  }
  for (int i = 0; i < jobs.n; ++i) L.j[L.n++] = jobs.j[i];
  return PCA_OK;
}

int wgrad_small_f32_launch(const float* G, const float* X, int64_t M, int dq,
                           int64_t x_head_stride, float* dW, float* db, hipStream_t st,
                           BwdDefer* defer) {
  if (defer != nullptr && !defer->has_sw) {
    defer->sw = SmallWgradArgs{G, X, M, dq, 64, x_head_stride, dW, db, nullptr};
    defer->has_sw = 1;
    return PCA_OK;
  }
  hipLaunchKernelGGL((k_wgrad_small<float>), dim3((unsigned)cdiv(M, 64)), dim3(256), 0, st, G, X, M,
                     dq, 64, x_head_stride, dW, db);
  return check_launch("k_wgrad_small<float>");
}

// the same with bf16 G over one input (no head stride), 128 rows per workgroup: never deferred
int wgrad_small_bf16_launch(const __bf16* G, const float* X, int64_t M, int dq, float* dW, float* db,
                            hipStream_t st) {
  hipLaunchKernelGGL((k_wgrad_small<__bf16>), dim3((unsigned)cdiv(M, 128)), dim3(256), 0, st,
                     G, X, M, dq, 128, (int64_t)0, dW, db);
  return check_launch("k_wgrad_small");
}

}  // namespace pca
