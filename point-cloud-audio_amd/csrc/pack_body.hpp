// Point-set packing (Code/dataset.py:50-54, 160-166) as a device body that runs either in the
// k_pack_2d / k_pack_3d launches of features.hip or as RIDER ROWS of the training step's k_prep_all
// launch (mab0_bf16.hip): the pack of a captured step is independent of the parameter-only
// preparation that opens the step, so the two share one launch (round 3: k_pack_* leaves the step's
// kernel table; pca_pack_defer in include/pca_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pca {

struct PackJob {
  int kind;                       // 0 none, 2 = 2-D (ESC_pc), 3 = 3-D (ESC_pc_temp)
  const float* spec;
  int64_t stride_f, stride_t, stride_s;
  const float *farr, *tarr;
  const int64_t* idx;             // index sequence (see pca_pack_points_*_seq)
  const int32_t *step_dev, *base_dev, *nt_valid;
  const int64_t* labels;
  int64_t* labels_out;
  int32_t* lengths_out;
  float* out;
  int B, F, Nt;
  int bx;                         // 256-thread blocks per set
};
inline int pack_blocks(const PackJob& j) { return j.bx * j.B; }

// block = set * bx + x : the work of workgroup (x, set) of k_pack_2d / k_pack_3d
__device__ __forceinline__ void pack_body(const PackJob& a, int block) {
  // The chain is cursor -> idx[b] -> labels / nt_valid / spec.  Requests are ordered by what they depend on:
  // the cursor's two words and the axis values (farr / tarr: no item in their index) go out together, then
  // idx, then everything behind the item as one batch.
  const int b = block / a.bx, x = block - b * a.bx;
  const int e = x * 256 + threadIdx.x;               // 2-D: bin f; 3-D: point index t*F + f (time-major)
  const bool lead = x == 0 && threadIdx.x == 0;
  const bool want_label = lead && a.labels != nullptr && a.labels_out != nullptr;
  // device cursor: batch number (step - base) of a pre-staged index sequence, so that a
  // captured step needs no per-step index upload
  int32_t step = 0, base = 0;
  if (a.step_dev != nullptr) {
    step = a.step_dev[0];
    base = a.base_dev[0];
  }
  if (a.kind == 2) {
    const bool live = e < a.F;
    const float fa = live ? a.farr[e] : 0.f;
    const int64_t item = a.idx[(int64_t)(step - base) * a.B + b];
    const int64_t lab = want_label ? a.labels[item] : 0;
    const float sp = live ? a.spec[e * a.stride_f + item * a.stride_t] : 0.f;
    if (want_label) a.labels_out[b] = lab;
    if (live) reinterpret_cast<float2*>(a.out)[(int64_t)b * a.F + e] = float2{fa, sp};
    return;
  }
  // variable-size sets: chunk s holds nt_valid[s] <= Nt frames; time-major point order makes
  // its points a prefix of the padded set, the padding rows are written as zeros
  const int Nt = a.Nt, F = a.F;
  const bool live = e < F * Nt;
  const int t = e / F, f = e - t * F;
  const float fa = live ? a.farr[f] : 0.f;
  const float ta = live ? a.tarr[t] : 0.f;
  const int64_t item = a.idx[(int64_t)(step - base) * a.B + b];
  const int64_t lab = want_label ? a.labels[item] : 0;
  const int ntv = a.nt_valid != nullptr ? a.nt_valid[item] : Nt;
  const int nt = ntv < Nt ? ntv : Nt;
  const bool ok = live && t < nt;
  // (spec is read for valid frames only, as before: the one request that waits for nt_valid)
  const float sp = ok ? a.spec[f * a.stride_f + t * a.stride_t + item * a.stride_s] : 0.f;
  if (lead) {
    if (want_label) a.labels_out[b] = lab;
    if (a.lengths_out != nullptr) a.lengths_out[b] = nt * F;
  }
  if (!live) return;
  float* o = a.out + ((int64_t)b * F * Nt + e) * 3;
  o[0] = ok ? fa : 0.f;
  o[1] = ok ? ta : 0.f;
  o[2] = sp;
}

// hand-off of a deferred pack (features.hip; thread-local: the one hand-off between public calls)
bool pack_stream_ok(hipStream_t st);  // the pending pack (if any) was submitted on `st`
bool pack_take(PackJob* out);          // true: *out is the pending pack, now the caller's to launch
int pack_flush(hipStream_t st);        // launches a pending pack on its own (no-op without one)

}  // namespace pca
