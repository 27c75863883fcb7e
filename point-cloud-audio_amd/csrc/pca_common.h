// Internal helpers shared by the HIP translation units of libpca_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdarg.h>

#include "pca_hip.h"

namespace pca {

// thread-local error string (the only mutable global state of the library)
void set_error(const char* fmt, ...);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return PCA_ELAUNCH;
  }
  return PCA_OK;
}

#define PCA_REQUIRE(cond, ...)        \
  do {                                \
    if (!(cond)) {                    \
      ::pca::set_error(__VA_ARGS__);  \
      return PCA_EINVAL;              \
    }                                 \
  } while (0)

#define PCA_TRY(expr)                 \
  do {                                \
    int _rc = (expr);                 \
    if (_rc != PCA_OK) return _rc;    \
  } while (0)

inline size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// log2(e): the softmax kernels work in the log2 domain (v_exp_f32 is 2^x)
constexpr float LOG2E = 1.4426950408889634f;

// Allow each of the kernels 160 KiB of dynamic LDS (a CU's whole LDS; HIP's default cap is 64 KiB): at the
// first call per process, result ignored.
// (Once per process, not per device: per-device state would change behaviour and belongs in a change of its own.)
template <auto... Kernels>
inline void allow_lds160() {
  static const bool once = [] {
    ((void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernels),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), ...);
    return true;
  }();
  (void)once;
}

// A/B switch read from the environment: on unless the variable starts with '0'.  Callers that read a
// switch once per process keep the result in a `static const bool`; the ones tests flip in-process call
// this every time.
inline bool env_not_zero(const char* name) {
  const char* e = getenv(name);
  return !(e != nullptr && e[0] == '0');
}

// bump allocator over a caller-provided block
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* p) : base(reinterpret_cast<char*>(p)) {}
  template <typename T>
  T* take(size_t count) {
    T* r = reinterpret_cast<T*>(base + off);
    off += align256(count * sizeof(T));
    return r;
  }
};

// ---- measurement hook (see pca_prof_start in pca_hip.h) -------------------------
// Usage in a launcher:  ProfScope ps(PCA_K_X, stream, flops, bytes);  <launch>;  ps.end();
struct ProfScope {
  int slot = -1;
  hipStream_t st;
  ProfScope(int kernel_id, hipStream_t stream, double flops, double bytes);
  void end();
};

// ---- the deferred pack (documented in include/pca_hip.h, "Per-thread state") ------------------------
// The one hand-off BETWEEN public calls: allowed to be pending at the entry of its documented consumers
// only (pack_allowed), never when a public pca_* call returns.  PCA_EINVAL naming the stale pack (armed and
// never consumed) otherwise.
bool pack_pending();
int no_stale_pack(const char* where, bool pack_allowed);

// ---- internal launchers used across translation units -------------------
int gemm_f32(const pca_gemm_desc& g, const float* A, const float* B, const float* bias,
             float* C, hipStream_t st);
// same contract, operands rounded to bf16 on the way into the MFMA (gemm_bf16.hip)
int gemm_bf16(const pca_gemm_desc& g, const float* A, const float* B, const float* bias,
              float* C, hipStream_t st);
// same contract, operands as hi + lo bf16 pairs (three MFMAs per K step): fp32-level results
int gemm_bf16_hl(const pca_gemm_desc& g, const float* A, const float* B, const float* bias,
                 float* C, hipStream_t st);
int softmax_rows(float* X, int64_t rows, int n, float scale, hipStream_t st,
                 const int32_t* lengths = nullptr, int64_t rows_per_set = 0);
int layernorm_fwd(const float* X, const float* w, const float* b, float* Y, float* mean,
                  float* rstd, int64_t rows, int d, hipStream_t st);
int layernorm_bwd(const float* dY, const float* X, const float* mean, const float* rstd,
                  const float* w, float* dX, float* dw, float* db, int64_t rows, int d,
                  hipStream_t st);
int softmax_bwd_rows(const float* A, float* dA, int64_t rows, int n, float scale,
                     hipStream_t st);
int colsum_parts(const float* X, int64_t rows, int cols, float* part, int* nparts, hipStream_t st);
int colsum(const float* X, int64_t rows, int cols, float* out, int accumulate,
           hipStream_t st);
// Y = O + relu(Z)
int add_relu(const float* O, const float* Z, float* Y, int64_t n, hipStream_t st);
// dZ = dY * [Z > 0]
int relu_bwd(const float* dY, const float* Z, float* dZ, int64_t n, hipStream_t st);
int relu_bwd_copy(const float* dY, const float* Z, float* dZ, float* dO, int64_t n, hipStream_t st);
// dst[r, :] = src[(r % src_rows), :]   (broadcast copy when src_rows < rows)
int copy_rows(const float* src, int64_t src_rows, float* dst, int64_t rows, int64_t cols,
              hipStream_t st);
int fill_zero(float* dst, int64_t n, hipStream_t st);
// the pooling attention of a q_shared block (pool_attn.hip; contracts: pca_pma_attention in pca_hip.h)
size_t pma_attention_ws_bytes(const pca_mab_shape& s);
int pma_attention(const pca_mab_shape& s, const float* S, const float* X, const pca_mab_params& p,
                  float* attn, float* key, void* ws, hipStream_t st);

}  // namespace pca
