// The preparation launch of a step as a plan: prep_plan (host code only) turns the weight-image jobs, the
// query-side jobs and a deferred pack into a short table of SEGMENTS over one flat block index, so that the
// launch has no empty workgroup and its deepest chains are dispatched first:
//   query-side items (live rows and, where WvT is asked for, the PREP_SPARE transposers; two to three round
//   trips deep), pack items (step / base -> idx -> labels, spec), image tiles, element items, clears.
// Image jobs are grouped by source: a group is one fp32 [rows][cols] source with up to three (dst, mode)
// targets, and an item of it is a tile of 32 source rows x all columns, read ONCE with 16-byte loads, held in
// LDS and written to every target with 16-byte stores (prep_tile_body).  Jobs whose shape or alignment does
// not fit a tile keep the element body (four elements per thread), as items of the same plan.
// k_prep_all (mab0_bf16.hip), k_prep_jobs (mab1_bf16.hip) and k_mab0_prep run the same plan and bodies.
#pragma once
#include "weight_images.hpp"
#include "mfma_common.hpp"
#include "pack_body.hpp"

namespace pca {

constexpr int PREP_SPARE = 16;            // transposer workgroups of a query-side job that asks for WvT / WoT
constexpr int PREP_TILE_ROWS = 32;        // source rows of an image tile: one aligned perm32 group of modes 2 / 3
constexpr int PREP_TILE_MAXC = 256;       // widest source a tile holds
constexpr int PREP_TILE_PAD = 4;          // floats: rows stay 16-byte aligned, 32 lanes over a column read 32 banks
constexpr int PREP_TILE_LDS = PREP_TILE_ROWS * (PREP_TILE_MAXC + PREP_TILE_PAD);   // floats
constexpr int PREP_CLEAR_WORDS = 8 * 256; // 16-bit words of a clear item (a 16-byte store per thread)
constexpr int PREP_ELEMS_PER_ITEM = 4 * 256;       // elements of an element item (four loads in flight per thread)

enum PrepKind : int { PREP_QUERY = 0, PREP_PACK = 1, PREP_TILES = 2, PREP_ELEMS = 3, PREP_CLEAR = 4 };

struct PrepSeg {
  int kind;       // PrepKind
  int job;        // index into Mab0PrepJobs (query), PrepPlan::grp (tiles) or PrepJobs (elements, clear)
  int first;      // first block of the segment; it ends where the next one begins
};
constexpr int PREP_MAXSEG = 36;           // <= 3 query jobs + 1 pack + 32 image / clear jobs
struct PrepGroup {
  short job[3];   // indices into PrepJobs: one source, rows and cols; dst and mode of each target
  short n;
};
struct PrepPlan {
  int first[PREP_MAXSEG];   // first block of segment i (INT_MAX behind the last): read in one batch by the search
  short kind[PREP_MAXSEG];  // PrepKind
  short job[PREP_MAXSEG];   // index into Mab0PrepJobs (query), grp (tiles) or PrepJobs (elements, clear)
  PrepGroup grp[32];
  int nseg, ngrp;
  int blocks;               // the grid
  int lds_floats;           // dynamic LDS of the query-side items (a Qp row)
};

// a job whose images are written by tiles: whole 32-row tiles, 16-byte loads and stores
inline bool prep_job_tiled(const PrepJob& j) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(j.src) | reinterpret_cast<uintptr_t>(j.dst);
  return j.mode >= 0 && j.mode <= 3 && j.rows > 0 && j.cols > 0 && j.rows % PREP_TILE_ROWS == 0 &&
         j.cols % 8 == 0 && j.cols <= PREP_TILE_MAXC && (j.mode != 1 || j.cols % 32 == 0) && (a & 15) == 0;
}
// clear items work on 16-byte groups of the destination: word w lies in group (w + lead) / 8
inline int prep_clear_lead(const void* dst) { return (int)((reinterpret_cast<uintptr_t>(dst) & 15) / 2); }

// workgroups of a query-side job: its live rows, the spare transposers, then the PAD items that zero the
// padding rows [h m, Rp) of Gb / GtP (256 elements each; they depend on nothing, so they are items of their own
// and not a loop behind the chain of the job's first row)
__host__ __device__ inline int prep_query_rows(const Mab0PrepJob& a) { return a.d > 128 ? a.m * a.h : a.m; }
__host__ __device__ inline int prep_query_spare(const Mab0PrepJob& a) { return a.WvT != nullptr ? PREP_SPARE : 0; }
inline int prep_query_pads(const Mab0PrepJob& a) {
  if (a.Gf == nullptr || a.Gb == nullptr) return 0;
  return (int)cdiv((int64_t)(a.Rp - a.h * a.m) * a.dk, 256);
}
inline int prep_query_blocks(const Mab0PrepJob& a) {
  return prep_query_rows(a) + prep_query_spare(a) + prep_query_pads(a);
}

// tiles = false: every image job keeps the element body (prep_plan_launch: launches of more than one round)
inline void prep_plan(const PrepJobs& W, const Mab0PrepJobs& Q, const PackJob& P, PrepPlan* out, bool tiles = true) {
  PrepPlan pl{};
  int at = 0;
  auto seg = [&](int kind, int job, int64_t blocks) {
    if (blocks <= 0) return;
    pl.first[pl.nseg] = at;
    pl.kind[pl.nseg] = (short)kind;
    pl.job[pl.nseg++] = (short)job;
    at += (int)blocks;
  };
  for (int i = 0; i < Q.n; ++i) {
    seg(PREP_QUERY, i, prep_query_blocks(Q.j[i]));
    pl.lds_floats = Q.j[i].d > pl.lds_floats ? Q.j[i].d : pl.lds_floats;
  }
  if (P.kind != 0) seg(PREP_PACK, 0, pack_blocks(P));
  for (int i = 0; i < W.n; ++i) {
    const PrepJob& j = W.j[i];
    if (!tiles || !prep_job_tiled(j)) continue;
    int g = 0;
    for (; g < pl.ngrp; ++g) {
      const PrepJob& h = W.j[pl.grp[g].job[0]];
      if (pl.grp[g].n < 3 && h.src == j.src && h.rows == j.rows && h.cols == j.cols) break;
    }
    if (g == pl.ngrp) pl.grp[pl.ngrp++] = PrepGroup{};
    pl.grp[g].job[pl.grp[g].n++] = (short)i;
  }
  for (int g = 0; g < pl.ngrp; ++g) seg(PREP_TILES, g, W.j[pl.grp[g].job[0]].rows / PREP_TILE_ROWS);
  for (int i = 0; i < W.n; ++i) {
    const PrepJob& j = W.j[i];
    if (j.mode >= 0 && j.mode <= 3 && !(tiles && prep_job_tiled(j))) seg(PREP_ELEMS, i, cdiv((int64_t)j.rows * j.cols, PREP_ELEMS_PER_ITEM));
  }
  for (int i = 0; i < W.n; ++i) {
    const PrepJob& j = W.j[i];
    const int64_t n = (int64_t)j.rows * j.cols;
    if (j.mode == 4 && n > 0) seg(PREP_CLEAR, i, cdiv(n + prep_clear_lead(j.dst), PREP_CLEAR_WORDS));
  }
  pl.blocks = at;
  for (int i = pl.nseg; i < PREP_MAXSEG; ++i) pl.first[i] = 0x7fffffff;
  *out = pl;
}

#if defined(__HIPCC__)
// ---- device bodies ---------------------------------------------------------------------------------------
// the segment of a block: uniform over the workgroup.  The firsts are one batch of scalar loads and a count,
// not a loop of dependent ones; kind and job follow in a second trip.
__device__ __forceinline__ PrepSeg prep_find_seg(const PrepPlan& pl, int blk) {
  int s = -1;
#pragma unroll
  for (int i = 0; i < PREP_MAXSEG; ++i) s += blk >= pl.first[i] ? 1 : 0;
  return PrepSeg{pl.kind[s], pl.job[s], pl.first[s]};
}

// four elements per thread, their loads requested together: block x of job jb (shapes and alignments a tile
// does not take, and every image of a plan without tiles)
__device__ __forceinline__ void prep_elems_body(const PrepJob& jb, int x) {
  const int rows = jb.rows, cols = jb.cols, mode = jb.mode;
  float v[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int idx = x * PREP_ELEMS_PER_ITEM + u * 256 + threadIdx.x;
    v[u] = 0.f;
    if (idx >= rows * cols) continue;
    if (mode <= 1) {
      const int n = idx / cols, k = idx - n * cols;
      const int kk = mode == 1 ? (k & ~31) + perm32(k & 31) : k;
      v[u] = jb.src[(int64_t)n * cols + kk];
    } else {
      const int n = idx / rows, k = idx - n * rows;
      const int kk = mode == 2 ? (k & ~31) + perm32(k & 31) : k;
      v[u] = jb.src[(int64_t)kk * cols + n];
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int idx = x * PREP_ELEMS_PER_ITEM + u * 256 + threadIdx.x;
    if (idx < rows * cols) jb.dst[idx] = (__bf16)v[u];
  }
}

// clear job: words [0, rows * cols) of dst, and not a byte more.  Thread t of block x owns the 16-byte group
// 256 x + t of the destination; a group that lies wholly inside the range is one store, the head and the tail
// groups are written word by word.
__device__ __forceinline__ void prep_clear_body(const PrepJob& jb, int x) {
  const int64_t n = (int64_t)jb.rows * jb.cols;
  const int lead = (int)((reinterpret_cast<uintptr_t>(jb.dst) & 15) / 2);
  const int64_t w0 = ((int64_t)x * 256 + threadIdx.x) * 8 - lead;
  if (w0 >= n) return;
  if (w0 >= 0 && w0 + 8 <= n) {
    *reinterpret_cast<uint4*>(jb.dst + w0) = uint4{0u, 0u, 0u, 0u};
    return;
  }
#pragma unroll
  for (int u = 0; u < 8; ++u)
    if (w0 + u >= 0 && w0 + u < n) jb.dst[w0 + u] = (__bf16)0.f;
}

__device__ __forceinline__ bf16x8 prep_cvt8(const float (&x)[8]) {
  bf16x8 o;
#pragma unroll
  for (int u = 0; u < 8; ++u) o[u] = (__bf16)x[u];
  return o;
}

// Tile `tile` of group g: source rows [32 tile, 32 tile + 32) x all columns.  All loads of the tile are
// requested before the first use; `lds` holds PREP_TILE_LDS floats.
//   modes 0 / 1 (row-major): a thread writes 8 consecutive outputs of a row; with the K permutation these
//     are two runs of 4 source columns (perm32: 4g .. 4g+3 and 16+4g .. 16+4g+3 of the 32-block).
//   modes 2 / 3 (transposed): the tile's rows are positions [32 tile, 32 tile + 32) of the target's K axis -
//     one aligned perm32 group - so target row n gets 64 contiguous bytes, 16 per thread; the 32 lanes of a
//     half wave read 32 consecutive columns of one LDS row.
struct PrepTargets {
  __bf16* dst[3];
  int mode[3];
  int n;
};
__device__ __forceinline__ void prep_tile_body(const float* src, int rows, int cols, PrepTargets g, int tile,
                                            float* lds) {
  const int ld = cols + PREP_TILE_PAD;
  const int tid = threadIdx.x;
  const int nv = 8 * cols;                  // float4s of the tile (<= 8 per thread)
  const float4* s4 = reinterpret_cast<const float4*>(src + (int64_t)tile * PREP_TILE_ROWS * cols);
  float4 v[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int i = tid + 256 * u;
    v[u] = i < nv ? s4[i] : float4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int e = 4 * (tid + 256 * u);
    if (e < 4 * nv) {
      const int r = e / cols, c = e - r * cols;
      *reinterpret_cast<float4*>(lds + r * ld + c) = v[u];
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    if (t >= g.n) break;
    const int mode = g.mode[t];
    __bf16* const dst = g.dst[t];
    if (mode <= 1) {
      const int cpr = cols / 8;
      for (int c = tid; c < PREP_TILE_ROWS * cpr; c += 256) {
        const int r = c / cpr, k0 = 8 * (c - r * cpr);
        const float* p = lds + r * ld;
        const int o0 = mode == 1 ? (k0 & ~31) + ((k0 & 31) >> 1) : k0;        // perm32(8g) = 4g
        const int o1 = mode == 1 ? o0 + 16 : k0 + 4;
        const float4 a = *reinterpret_cast<const float4*>(p + o0);
        const float4 b = *reinterpret_cast<const float4*>(p + o1);
        const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        *reinterpret_cast<bf16x8*>(dst + (int64_t)(tile * PREP_TILE_ROWS + r) * cols + k0) = prep_cvt8(x);
      }
    } else {
      for (int c = tid; c < 4 * cols; c += 256) {
        const int q = c / cols, n = c - q * cols;
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int p = 8 * q + u;
          x[u] = lds[(mode == 2 ? perm32(p) : p) * ld + n];
        }
        *reinterpret_cast<bf16x8*>(dst + (int64_t)n * rows + tile * PREP_TILE_ROWS + 8 * q) = prep_cvt8(x);
      }
    }
  }
}

// an image / clear item of the plan (segment s, block x of it); TILES = false: of a plan without tiles
template <bool TILES = true>
__device__ __forceinline__ void prep_image_item(const PrepJobs& W, const PrepPlan& pl, const PrepSeg& s, int x,
                                                float* lds) {
  if (TILES && s.kind == PREP_TILES) {
    const PrepGroup g = pl.grp[s.job];
    const PrepJob j0 = W.j[g.job[0]];
    PrepTargets t{};
    t.n = g.n;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const PrepJob jb = W.j[g.job[i < g.n ? i : 0]];
      t.dst[i] = jb.dst;
      t.mode[i] = jb.mode;
    }
    prep_tile_body(j0.src, j0.rows, j0.cols, t, x, lds);
  } else if (s.kind == PREP_ELEMS) prep_elems_body(W.j[s.job], x);
  else if (s.kind == PREP_CLEAR) prep_clear_body(W.j[s.job], x);
}
#endif

}  // namespace pca
