// Weight images: the bf16 / fp8 / transposed-fp32 copies of the parameters the fused kernels read, the job
// tables that convert a whole step's images in one launch, and the table (WeightImages) through which a
// block finds an image its caller has already made.  Kernels: mab1_bf16.hip (prep_*), mab0_bf16.hip
// (the query-side preparation, prep_all_launch); the plan and the image bodies they run: prep_plan.hpp.
#pragma once
#include "pca_common.h"

namespace pca {

// fp32 weight [rows][cols] -> bf16 image; mode 0 natural, 1 K-permuted, 2 transposed +
// K-permuted ([cols][rows]), 3 transposed natural
int prep_weight2(const float* src0, __bf16* dst0, int mode0, const float* src1, __bf16* dst1,
                 int mode1, int rows, int cols, hipStream_t st);
int prep_weight(const float* src, __bf16* dst, int rows, int cols, int mode, hipStream_t st);
// fp8 e4m3 image of s * W (mode 0 natural / 1 K-permuted), s a power of two; inv_scale[0] = 1 / s
int prep_weight_f8(const float* src, void* dst, int rows, int cols, int mode, float* inv_scale,
                   hipStream_t st);
// dst[c][r] = src[r][c]  (fp32): gives the per-set row-GEMM kernels coalesced weight reads
int transpose_f32(const float* src, float* dst, int rows, int cols, hipStream_t st);

// the query side (Qp, G: parameters only) of a few-queries block
struct Mab0PrepJob {
  const float *I, *Wq, *bq, *Wk;
  int m, d, dq, dk, h, Rp;
  float sl2e;
  float *Qp, *Gf;
  __bf16 *Gb, *GtP;
  // epilogue weights transposed to [in][out] fp32 by spare workgroups of the same launch
  // (null when the epilogue runs elsewhere, e.g. inside k_mid_fwd)
  const float *Wv, *Wo;
  float *WvT, *WoT;
};
struct Mab0PrepJobs {
  Mab0PrepJob j[3];
  int n;
};
int mab0_prep_launch(const Mab0PrepJobs& J, hipStream_t st);

// ---- batched weight-image preparation (one launch per step) -----------------------------
// bf16 images of one ISAB's weights, owned by the caller (the ST engine) for a whole step
struct IsabImg {
  __bf16 *Wv0, *Wo0, *Wk1, *Wv1;                     // natural: k_mid_fwd
  __bf16 *WqB, *WoP;                                 // k_mab1_fwd (natural Wq, K-permuted Wo)
  __bf16 *Wk1T, *Wv1T, *Wo0TP, *Wv0TP, *Wv0T;        // k_mid_bwd
  __bf16 *WoTP, *WqTP;                               // k_mab1_bwd
};
struct PrepJob {
  const float* src;
  __bf16* dst;
  int rows, cols, mode;      // modes of prep_weight; 4: dst[0 .. rows * cols) = 0 (src unused)
};
struct PrepJobs {
  PrepJob j[32];
  int n;
};
int prep_jobs_launch(const PrepJobs& jobs, hipStream_t st);
// Weight images prepared ahead by the caller (the ST engine: every bf16 image the d = 256 blocks of a
// training step will ask for, in ONE launch at the start of the step instead of one ~5 us launch per
// block and direction).  Given a table, weight_image1 / 2 redirect *dst to a registered image of
// (src, mode, rows, cols) instead of converting into *dst; anything not registered - everything, with a
// null table - is converted as before, so a table can only save launches, never change results.
struct WeightImages {
  struct E { const float* src; int mode, rows, cols; __bf16* img; } e[24];
  int n;
  // fp8 mode: e4m3 images of s * W (prep_weight_f8) with their inverse scales, one launch for all
  struct F8 { const float* src; int mode, rows, cols; uint8_t* img; float* inv; } f8[8];
  int nf8;
};
struct PrepF8Jobs {
  WeightImages::F8 j[8];
  int n;
};
int prep_f8_jobs_launch(const PrepF8Jobs& J, hipStream_t st);
// the registered fp8 image of (src, mode) - *dst and *inv are redirected to it - or a conversion into
// *dst / *inv on the spot
int weight_image_f8(const WeightImages* t, const float* src, void** dst, int rows, int cols, int mode,
                    float** inv, hipStream_t st);
int weight_image1(const WeightImages* t, const float* src, __bf16** dst, int rows, int cols, int mode,
                  hipStream_t st);
int weight_image2(const WeightImages* t, const float* src0, __bf16** dst0, int mode0, const float* src1,
                  __bf16** dst1, int mode1, int rows, int cols, hipStream_t st);
int mab1_fwd_wo_mode(const pca_mab_shape& s);        // image mode of fc_o the mab1 forward asks for
// the weight images AND the query-side tensors of a step in ONE launch (both depend on the
// parameters only; the launch is a plan of segments over one flat block index: prep_plan.hpp)
int prep_all_launch(const PrepJobs& W, const Mab0PrepJobs& Q, hipStream_t st);

}  // namespace pca
