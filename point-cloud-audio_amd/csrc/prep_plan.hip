// Host views of the preparation plan (prep_plan.hpp) for tests/test_prep_plan_host.py and
// tests/test_gpu_prep_images.py; not part of the documented ABI.
#include "prep_plan.hpp"

// The plan of a made-up job set, as integers; no device, every pointer is an address that nothing reads.
// in:  [0] query jobs (<= 3), [1] image / clear jobs (<= 32), [2] pack kind (0 none, 2, 3), [3] the pack's sets B,
//      [4] its blocks per set bx; then per query job (m, d, h, WvT asked for, dk, bf16 G images asked for: their
//      padding rows [h m, Rp) are zeroed by pad items), then per image / clear job
//      (source id, source misalignment in bytes, destination misalignment in bytes, rows, cols, mode).
//      Jobs with the same source id and misalignment share a source pointer.
// out: [0] blocks (the grid), [1] segments, [2] groups, [3] floats of dynamic LDS; then per segment
//      (kind, job, first block), then per group (targets, job 0, job 1, job 2; -1: none).
// Returns PCA_EINVAL when `out` is too short.
extern "C" int pca_debug_prep_plan(const int64_t* in, int n_in, int64_t* out, int n_out) {
  using namespace pca;
  PCA_REQUIRE(in != nullptr && out != nullptr && n_in >= 5, "pca_debug_prep_plan: null or short input");
  const int nq = (int)in[0], nw = (int)in[1];
  PCA_REQUIRE(nq >= 0 && nq <= 3 && nw >= 0 && nw <= 32 && n_in >= 5 + 6 * nq + 6 * nw,
              "pca_debug_prep_plan: table sizes");
  Mab0PrepJobs Q{};
  PrepJobs W{};
  PackJob P{};
  P.kind = (int)in[2]; P.B = (int)in[3]; P.bx = (int)in[4];
  const int64_t* q = in + 5;
  for (int i = 0; i < nq; ++i, q += 6) {
    Mab0PrepJob a{};
    a.m = (int)q[0]; a.d = (int)q[1]; a.h = (int)q[2]; a.dk = (int)q[4];
    a.Rp = (int)cdiv(a.h * a.m, 32) * 32;
    if (q[5]) {
      a.Gf = reinterpret_cast<float*>((uintptr_t)0x400000000ull + ((uintptr_t)i << 24));
      a.Gb = reinterpret_cast<__bf16*>((uintptr_t)0x500000000ull + ((uintptr_t)i << 24));
    }
    a.WvT = q[3] ? reinterpret_cast<float*>((uintptr_t)0x300000000ull + ((uintptr_t)i << 24)) : nullptr;
    Q.j[Q.n++] = a;
  }
  for (int i = 0; i < nw; ++i, q += 6) {
    PCA_REQUIRE(q[1] >= 0 && q[1] < 16 && q[2] >= 0 && q[2] < 16 && q[2] % 2 == 0, "pca_debug_prep_plan: misalignment");
    const float* src = reinterpret_cast<const float*>((uintptr_t)0x100000000ull + ((uintptr_t)q[0] << 24) + q[1]);
    __bf16* dst = reinterpret_cast<__bf16*>((uintptr_t)0x200000000ull + ((uintptr_t)i << 24) + q[2]);
    W.j[W.n++] = PrepJob{q[5] == 4 ? nullptr : src, dst, (int)q[3], (int)q[4], (int)q[5]};
  }
  PrepPlan pl;
  prep_plan(W, Q, P, &pl);
  const int need = 4 + 3 * pl.nseg + 4 * pl.ngrp;
  PCA_REQUIRE(n_out >= need, "pca_debug_prep_plan: out holds %d words, the plan %d", n_out, need);
  int64_t* o = out;
  *o++ = pl.blocks; *o++ = pl.nseg; *o++ = pl.ngrp; *o++ = pl.lds_floats;
  for (int i = 0; i < pl.nseg; ++i) { *o++ = pl.kind[i]; *o++ = pl.job[i]; *o++ = pl.first[i]; }
  for (int g = 0; g < pl.ngrp; ++g) {
    *o++ = pl.grp[g].n;
    for (int t = 0; t < 3; ++t) *o++ = t < pl.grp[g].n ? pl.grp[g].job[t] : -1;
  }
  return PCA_OK;
}

// n image / clear jobs (src[i], dst[i], rows[i], cols[i], mode[i]; device pointers, src unused in mode 4) through
// prep_jobs_launch: the plan's tiles, element items and clears as a step runs them.
extern "C" int pca_debug_prep_images(const void* const* src, void* const* dst, const int* rows, const int* cols,
                                     const int* mode, int n, hipStream_t st) {
  using namespace pca;
  PCA_REQUIRE(src != nullptr && dst != nullptr && rows != nullptr && cols != nullptr && mode != nullptr && n >= 0 &&
                  n <= 32,
              "pca_debug_prep_images: null table or more than 32 jobs");
  PrepJobs W{};
  for (int i = 0; i < n; ++i) {
    PCA_REQUIRE(mode[i] >= 0 && mode[i] <= 4 && rows[i] >= 0 && cols[i] >= 0 && dst[i] != nullptr &&
                    (mode[i] == 4 || src[i] != nullptr) && (int64_t)rows[i] * cols[i] < (int64_t)1 << 31,
                "pca_debug_prep_images: job %d", i);
    W.j[W.n++] = PrepJob{reinterpret_cast<const float*>(src[i]), reinterpret_cast<__bf16*>(dst[i]), rows[i], cols[i],
                         mode[i]};
  }
  return prep_jobs_launch(W, st);
}
