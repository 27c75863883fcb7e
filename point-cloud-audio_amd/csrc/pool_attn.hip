// The pooling attention of one PMA block, returned to the caller (a diagnostic on the parity side).
//
// Replaces: nothing the reference returns - it is the `A` that set_transformer-master/modules.py:21-27
// builds inside MAB.forward and drops:  Q = fc_q(S), K = fc_k(X), heads split along the features,
// A = softmax(Q_j K_j^T / sqrt(d)) over the keys.  The fused forward kernels never build it and the exact
// chain keeps it in a workspace; this file computes it on its own, in fp32 whatever the mode.
//
// With few queries the projected keys [B, N, d] need not exist: for row r = (seed s, head j)
//   u_r = Wk_j^T q_{s,j} / sqrt(d)  in R^d,   c_r = q_{s,j} . bk_j / sqrt(d),
//   score[b, r, n] = X[b, n, :] . u_r + c_r,
// u and c being the same for every set.  Three launches:
//   k_pa_prep    u [R, d] and c [R] (R = k h), once per call; sums in fp64, rounded to fp32 once
//   k_pa_scores  one workgroup per 64-point tile of a set: the tile of X goes through LDS once, coalesced, and
//                serves all R rows (lane = point, wave = rows w, w + 4, ...; u in scalar registers); the raw
//                scores go to `attn`, the tile's (max, sum of exp) per row to the workspace
//   k_pa_norm    one workgroup per 256 points of a set: merges the tile statistics of every row in tile
//                order, normalises `attn` in place, writes zeros beyond lengths[b] and the key
// so a row of any length works: nothing of size N lives in LDS.  HBM traffic: X read once (B N d 4 bytes, the
// bound), attn written, read and written again (3 B R N 4 bytes).  No atomics; every output element has one
// owner; sums run in a fixed order: the same call gives the same bits.
#include "pca_common.h"

#include <math.h>

namespace pca {
namespace {

constexpr int PA_TILE = 64;      // points per scores tile: one per lane
constexpr int PA_ROWS = 4;       // rows a wave carries through one pass over its tile
constexpr int PA_CHUNK = 256;    // points per workgroup of the normalising launch
constexpr int PA_PASS = 64;      // rows whose statistics the normalising launch holds at a time

inline int pa_tiles(int N) { return (int)cdiv(N, PA_TILE); }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// butterfly: every lane ends with the same sum, added in the same order on every call
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid: R workgroups of 256 threads.  q = fc_q(S)[s, head j's features]; u_r = sum_f q[f] Wk[f, :] / sqrt(d).
// A wave per query feature (lanes over the d inputs, coalesced, butterfly sum), then a thread per column of u:
// its dh loads do not depend on one another, so they are in flight together.
__global__ __launch_bounds__(256) void k_pa_prep(const float* __restrict__ S, const float* __restrict__ wq,
                                                 const float* __restrict__ bq, const float* __restrict__ wk,
                                                 const float* __restrict__ bk, int d, int h,
                                                 float* __restrict__ u, float* __restrict__ c) {
  __shared__ double q[256];                       // dh <= d <= 256
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int s = r / h, j = r - s * h, dh = d / h;
  const double scale = 1.0 / sqrt((double)d);
  for (int fl = w; fl < dh; fl += 4) {
    const int f = j * dh + fl;
    double acc = 0.0;
    for (int i = lane; i < d; i += 64) acc += (double)S[(int64_t)s * d + i] * (double)wq[(int64_t)f * d + i];
    acc = wave_sum_f64(acc) + (double)bq[f];
    if (lane == 0) q[fl] = (double)(float)acc;    // the query as the reference holds it: an fp32 tensor
  }
  __syncthreads();
  if (tid < d) {
    double acc = 0.0;
    for (int f = 0; f < dh; ++f) acc += q[f] * (double)wk[(int64_t)(j * dh + f) * d + tid];
    u[(int64_t)r * d + tid] = (float)(acc * scale);
  }
  if (w == 3) {                                    // (d <= 192 leaves this wave idle above)
    double acc = 0.0;
    for (int f = lane; f < dh; f += 64) acc += q[f] * (double)bk[j * dh + f];
    acc = wave_sum_f64(acc);
    if (lane == 0) c[r] = (float)(acc * scale);
  }
}

// sc[q] = x . u_q for NR rows of u that lie 4 rows (4 d floats) apart; x: one row of the tile in LDS.  Four
// partial sums per row (one per float4 component), joined pairwise.
template <int NR>
__device__ __forceinline__ void pa_dot4(const float* __restrict__ xr, const float* __restrict__ u, int d,
                                        float* sc) {
  float4 acc[NR];
#pragma unroll
  for (int q = 0; q < NR; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int col = 0; col < d; col += 4) {
    const float4 x = *reinterpret_cast<const float4*>(xr + col);
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      const float4 uv = *reinterpret_cast<const float4*>(u + (int64_t)4 * q * d + col);
      acc[q].x = fmaf(x.x, uv.x, acc[q].x);
      acc[q].y = fmaf(x.y, uv.y, acc[q].y);
      acc[q].z = fmaf(x.z, uv.z, acc[q].z);
      acc[q].w = fmaf(x.w, uv.w, acc[q].w);
    }
  }
#pragma unroll
  for (int q = 0; q < NR; ++q) sc[q] = (acc[q].x + acc[q].y) + (acc[q].z + acc[q].w);
}

// grid: B * T workgroups of 256 threads (T = tiles per set); LDS: PA_TILE rows of `ds` floats + a spare float4.
// VEC: d % 4 == 0 and X 16-byte aligned - float4 loads, LDS rows d + 4 apart (ds_read_b128 of 16 lanes then
// covers all 64 banks); otherwise scalar loads and an odd row stride.
template <bool VEC>
__global__ __launch_bounds__(256) void k_pa_scores(const float* __restrict__ X,
                                                   const int32_t* __restrict__ lengths,
                                                   const float* __restrict__ u, const float* __restrict__ c,
                                                   int N, int d, int R, int T, int ds,
                                                   float* __restrict__ attn, float* __restrict__ part) {
  extern __shared__ float4 pa_lds4[];
  float* xs = reinterpret_cast<float*>(pa_lds4);
  const int b = blockIdx.x / T, t = blockIdx.x - b * T;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int len = lengths != nullptr ? lengths[b] : N;
  len = len < 0 ? 0 : (len > N ? N : len);
  const int n0 = t * PA_TILE;
  if (n0 >= len) return;                          // (the whole workgroup: a padding tile has no statistics)
  const int cnt = len - n0 < PA_TILE ? len - n0 : PA_TILE;
  const float* __restrict__ src = X + ((int64_t)b * N + n0) * d;   // cnt rows, contiguous
  if (VEC) {
    // Eight 16-byte loads of a thread are issued before the first is stored (32 KiB in flight per
    // workgroup).  Straight-line code - a load past the tile's rows re-reads element 0, a store past the tile
    // goes to the spare slot behind it - because a guarded store would take its load into the guard with it.
    const int d4 = d >> 2, total = cnt * d4, full = PA_TILE * d4;
    const float4* __restrict__ src4 = reinterpret_cast<const float4*>(src);
    const int step_row = 256 / d4, step_col = 256 - step_row * d4;   // element i + 256 lies this far on
    int row = tid / d4, col = tid - row * d4;
    for (int base = tid; base < full; base += 256 * 8) {
      float4 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int i = base + 256 * q;
        v[q] = src4[i < total ? i : 0];
      }
      // (an empty statement every loaded value passes through: all eight loads come before it, all eight
      //  stores after it - left alone, the compiler pairs each load with its store, one in flight at a time)
#pragma unroll
      for (int q = 0; q < 8; ++q) asm volatile("" : "+v"(v[q].x), "+v"(v[q].y), "+v"(v[q].z), "+v"(v[q].w));
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int i = base + 256 * q;
        *reinterpret_cast<float4*>(xs + (i < full ? row * ds + 4 * col : PA_TILE * ds)) = v[q];
        row += step_row;
        col += step_col;
        if (col >= d4) {
          col -= d4;
          ++row;
        }
      }
    }
  } else {
    const int total = cnt * d;
    for (int i = tid; i < total; i += 256) {
      const int row = i / d, col = i - row * d;
      xs[row * ds + col] = src[i];
    }
  }
  __syncthreads();
  const bool valid = lane < cnt;
  const float* __restrict__ xr = xs + (valid ? lane : 0) * ds;     // (an idle lane re-reads row 0: written)
  for (int r0 = w; r0 < R; r0 += 4 * PA_ROWS) {
    float sc[PA_ROWS];
    if (VEC) {
      const int left = (R - r0 + 3) >> 2;          // rows r0, r0 + 4, ... still to do (wave-uniform)
      if (left >= 4) pa_dot4<4>(xr, u + (int64_t)r0 * d, d, sc);
      else if (left == 3) pa_dot4<3>(xr, u + (int64_t)r0 * d, d, sc);
      else if (left == 2) pa_dot4<2>(xr, u + (int64_t)r0 * d, d, sc);
      else pa_dot4<1>(xr, u + (int64_t)r0 * d, d, sc);
    } else {
#pragma unroll
      for (int q = 0; q < PA_ROWS; ++q) sc[q] = 0.f;
      for (int col = 0; col < d; ++col) {
        const float x = xr[col];
#pragma unroll
        for (int q = 0; q < PA_ROWS; ++q) {
          const int r = r0 + 4 * q;
          if (r < R) sc[q] = fmaf(x, u[(int64_t)r * d + col], sc[q]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < PA_ROWS; ++q) {
      const int r = r0 + 4 * q;
      if (r >= R) break;                          // (wave-uniform)
      const float s = sc[q] + c[r];
      const float m = wave_max(valid ? s : -INFINITY);
      const float l = wave_sum(valid ? expf(s - m) : 0.f);
      const int64_t row = (int64_t)b * R + r;
      if (valid) attn[row * N + n0 + lane] = s;
      if (lane == 0) {
        part[(row * T + t) * 2] = m;
        part[(row * T + t) * 2 + 1] = l;
      }
    }
  }
}

// grid: B * ceil(N / PA_CHUNK) workgroups of 256 threads; thread = point, all R rows.
__global__ __launch_bounds__(256) void k_pa_norm(const int32_t* __restrict__ lengths,
                                                 const float* __restrict__ part, int N, int R, int T,
                                                 int chunks, float* __restrict__ attn,
                                                 float* __restrict__ key) {
  __shared__ float sM[PA_PASS], sL[PA_PASS];
  const int b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int len = lengths != nullptr ? lengths[b] : N;
  len = len < 0 ? 0 : (len > N ? N : len);
  const int Tv = (len + PA_TILE - 1) / PA_TILE;    // tiles that hold statistics
  const int n = ch * PA_CHUNK + tid;
  float ksum = 0.f;
  for (int p0 = 0; p0 < R; p0 += PA_PASS) {
    const int pr = R - p0 < PA_PASS ? R - p0 : PA_PASS;
    // the row's maximum and sum from its tiles: a lane walks tiles lane, lane + 64, ... in order, the lanes'
    // sums meet in the butterfly.  One tile: M = m_0 and L = l_0 exactly.
    for (int i = w; i < pr; i += 4) {
      const float* __restrict__ pp = part + ((int64_t)b * R + p0 + i) * T * 2;
      float m = -INFINITY;
      for (int t = lane; t < Tv; t += 64) m = fmaxf(m, pp[2 * t]);
      m = wave_max(m);
      float l = 0.f;
      for (int t = lane; t < Tv; t += 64) l += pp[2 * t + 1] * expf(pp[2 * t] - m);
      l = wave_sum(l);
      if (lane == 0) {
        sM[i] = m;
        sL[i] = l;
      }
    }
    __syncthreads();
    float* a = attn + ((int64_t)b * R + p0) * N + n;
    if (n < len) {
      int i = 0;
      for (; i + 8 <= pr; i += 8) {                // eight rows' loads in flight, then their stores
        float sv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) sv[q] = a[(int64_t)(i + q) * N];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float v = expf(sv[q] - sM[i + q]) / sL[i + q];
          a[(int64_t)(i + q) * N] = v;
          ksum += v;                               // rows in order r = 0 .. R - 1
        }
      }
      for (; i < pr; ++i) {
        const float v = expf(a[(int64_t)i * N] - sM[i]) / sL[i];
        a[(int64_t)i * N] = v;
        ksum += v;
      }
    } else if (n < N) {                            // beyond lengths[b]: exact zeros, nothing read
      for (int i = 0; i < pr; ++i) a[(int64_t)i * N] = 0.f;
    }
    __syncthreads();
  }
  if (key != nullptr && n < N) key[(int64_t)b * N + n] = ksum / (float)R;
}

int pa_validate(const pca_mab_shape* s) {
  PCA_REQUIRE(s != nullptr, "pma_attention: null shape");
  PCA_REQUIRE(s->B > 0 && s->nq > 0 && s->nk > 0 && s->d > 0 && s->h > 0,
              "pma_attention: non-positive extent (B=%d nq=%d nk=%d d=%d h=%d)", s->B, s->nq, s->nk, s->d,
              s->h);
  PCA_REQUIRE(s->q_shared == 1, "pma_attention: the queries are the shared seeds (q_shared=%d)", s->q_shared);
  PCA_REQUIRE(s->dq == s->d && s->dk == s->d, "pma_attention: dq=%d dk=%d must equal d=%d", s->dq, s->dk,
              s->d);
  PCA_REQUIRE(s->k_dtype == PCA_F32, "pma_attention: fp32 keys only");
  PCA_REQUIRE(s->ln == 0, "pma_attention: no LayerNorm variant");
  PCA_REQUIRE(s->d % s->h == 0, "pma_attention: d=%d not divisible by h=%d", s->d, s->h);
  PCA_REQUIRE(s->d <= 256, "pma_attention: d=%d (max 256)", s->d);
  const int64_t R = (int64_t)s->nq * s->h;
  PCA_REQUIRE(R <= (1 << 20) && (int64_t)s->B * R * pa_tiles(s->nk) <= (int64_t)1 << 40,
              "pma_attention: %lld rows per set", (long long)R);
  PCA_REQUIRE((int64_t)s->B * cdiv(s->nk, PA_TILE) < ((int64_t)1 << 31),
              "pma_attention: B=%d nk=%d exceeds the launch grid", s->B, s->nk);
  return PCA_OK;
}

}  // namespace

size_t pma_attention_ws_bytes(const pca_mab_shape& s) {
  const size_t R = (size_t)s.nq * s.h;
  return align256(R * s.d * sizeof(float)) + align256(R * sizeof(float)) +
         align256((size_t)s.B * R * pa_tiles(s.nk) * 2 * sizeof(float));
}

int pma_attention(const pca_mab_shape& s, const float* S, const float* X, const pca_mab_params& p,
                  float* attn, float* key, void* ws, hipStream_t st) {
  PCA_TRY(pa_validate(&s));
  PCA_REQUIRE(S && X && attn && ws, "pma_attention: null pointer");
  PCA_REQUIRE(p.wq && p.bq && p.wk && p.bk, "pma_attention: null parameter");
  const int R = s.nq * s.h, N = s.nk, d = s.d, T = pa_tiles(N);
  Carver cv(ws);
  float* u = cv.take<float>((size_t)R * d);
  float* c = cv.take<float>((size_t)R);
  float* part = cv.take<float>((size_t)s.B * R * T * 2);
  hipLaunchKernelGGL(k_pa_prep, dim3((unsigned)R), dim3(256), 0, st, S, p.wq, p.bq, p.wk, p.bk, d, s.h, u, c);
  PCA_TRY(check_launch("k_pa_prep"));
  const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  const int ds = vec ? d + 4 : (d | 1);
  const size_t lds = ((size_t)PA_TILE * ds + 4) * sizeof(float);    // the tile + a spare float4: <= 66,576 bytes
  allow_lds160<k_pa_scores<true>, k_pa_scores<false>>();
  const dim3 grid((unsigned)((int64_t)s.B * T));
  if (vec)
    hipLaunchKernelGGL(k_pa_scores<true>, grid, dim3(256), lds, st, X, s.k_lengths, u, c, N, d, R, T, ds, attn,
                       part);
  else
    hipLaunchKernelGGL(k_pa_scores<false>, grid, dim3(256), lds, st, X, s.k_lengths, u, c, N, d, R, T, ds,
                       attn, part);
  PCA_TRY(check_launch("k_pa_scores"));
  const int chunks = (int)cdiv(N, PA_CHUNK);
  hipLaunchKernelGGL(k_pa_norm, dim3((unsigned)((int64_t)s.B * chunks)), dim3(256), 0, st, s.k_lengths, part, N,
                     R, T, chunks, attn, key);
  return check_launch("k_pa_norm");
}

}  // namespace pca

extern "C" {

size_t pca_pma_attention_ws_bytes(const pca_mab_shape* s) {
  if (pca::pa_validate(s) != PCA_OK) return 0;
  return pca::pma_attention_ws_bytes(*s);
}

int pca_pma_attention(const pca_mab_shape* s, const float* S, const float* X, const pca_mab_params* p,
                      float* attn, float* key, void* ws, void* stream) {
  PCA_TRY(pca::pa_validate(s));
  PCA_REQUIRE(p != nullptr, "pma_attention: null parameters");
  PCA_TRY(pca::no_stale_pack("pca_pma_attention", false));
  return pca::pma_attention(*s, S, X, *p, attn, key, ws, pca::as_stream(stream));
}
}
