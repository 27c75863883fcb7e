// Forward passes of the paper's two fixed-input baselines, for the evaluation sweeps
// (DESIGN.md section 7):
//   FB        baseline_ff(layer_dims, C):   Code/models.py:47-88  (eval mode: dropout is identity)
//             frame x[F] -> [Linear + LeakyReLU(0.01)] * (nd - 1) -> Linear -> softmax
//   CNN_temp  CNN_classifier(Nt, Nf, dims): Code/models.py:91-119
//             chunk x[Nt][Nf] -> Conv2d(1, 1, (Nt, kw)) valid + bias -> [L0]
//             -> [Linear + LeakyReLU(0.01)] * (nd - 1) -> Linear (logits)
// with the optional in-launch sub-sampling of the reference's Experiment 2:
//   Code/utils.py:86-108      pc_maxK_replace / pc_randK_replace          (FB)
//   Code/dataset.py:101-135   ESC_baseline_temporal_maxK "max" / "rand"  (CNN_temp)
// All but K cells of every set are zeroed.  The kept cells are those pca_subsample_points selects
// for the same (seed, draw + draw_dev[0], batch slot, set): the same keys (select_keys.hpp), the
// same cell order p = t*F + f and the same bitonic sort.  The zero-filled input exists only in LDS.
//
// One workgroup (16 waves) per set, one launch per batch:
//   1. selection: (key, p) pairs sorted in LDS; the K-th smallest pair is the threshold, so a
//      cell is kept iff its own pair is <= it (pairs are unique: their low word is p);
//   2. the zero-filled input is loaded into LDS (aliasing the sort keys);
//   3. CNN_temp: the valid convolution, one output column per thread;
//   4. every Linear: one output row per wave and pass, lanes stride the row (coalesced weight
//      reads), a fixed butterfly reduction; activations stay in two LDS buffers;
//   5. FB: softmax over the classes (nn.Softmax() inside the model, Code/models.py:75).
// fp32 FMA throughout (parity mode); no atomics, so a launch is bitwise reproducible.  Weights
// are read from L2 by every workgroup: a set costs one pass over them (2.6 MB FB, 0.63 MB
// CNN_temp at the shipped shapes).
#include "pca_common.h"
#include "select_keys.hpp"

#include <stdint.h>

#include <mutex>

namespace pca {
namespace {

constexpr int kMaxLinear = 16;        // Linear layers (hidden + head) a launch supports
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr size_t kMaxLds = 160 * 1024;

struct BaseNet {
  int cnn;                      // 0 FB, 1 CNN_temp
  int F, Nt;                    // cells of a set: N = F * Nt (FB: Nt = 1)
  int kw, L0;                   // CNN_temp: conv width and output width L0 = F + 1 - kw
  int nl;                       // Linear layers
  int din[kMaxLinear], dout[kMaxLinear];
  int64_t woff[kMaxLinear];     // weight [dout][din] at woff, bias [dout] right after it
  int hmax;                     // widest activation after the input (L0, hidden widths, C)
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// y[o] = act(b[o] + sum_i W[o][i] x[i]) for o < dout; x, y in LDS
__device__ __forceinline__ void dense(const float* __restrict__ W, const float* x, float* y,
                                      int din, int dout, bool leaky, int wave, int lane) {
  const float* __restrict__ bias = W + (int64_t)din * dout;
  for (int o = wave; o < dout; o += kWaves) {
    const float* __restrict__ w = W + (int64_t)o * din;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int i = lane;
    for (; i + 192 < din; i += 256) {
      a0 = fmaf(w[i], x[i], a0);
      a1 = fmaf(w[i + 64], x[i + 64], a1);
      a2 = fmaf(w[i + 128], x[i + 128], a2);
      a3 = fmaf(w[i + 192], x[i + 192], a3);
    }
    for (; i < din; i += 64) a0 = fmaf(w[i], x[i], a0);
    float s = wave_sum((a0 + a1) + (a2 + a3));
    if (lane == 0) {
      s += bias[o];
      y[o] = (leaky && !(s > 0.f)) ? s * 0.01f : s;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_baseline_fwd(
    const float* __restrict__ spec, int64_t stride_f, int64_t stride_t, int64_t stride_s,
    const int64_t* __restrict__ idx, const float* __restrict__ W, BaseNet net, int K, int mode,
    uint64_t seed, uint64_t draw, const int32_t* __restrict__ draw_dev, int Np, int C,
    float* __restrict__ out, int32_t* __restrict__ sel, const int64_t* __restrict__ labels,
    int64_t* __restrict__ labels_out) {
  extern __shared__ uint64_t lds[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int F = net.F, N = F * net.Nt;
  const int64_t set = idx[b];
  if (labels != nullptr && labels_out != nullptr && tid == 0) labels_out[b] = labels[set];
  const float* __restrict__ base = spec + set * stride_s;
  const bool select = mode != PCA_SEL_ALL;
  if (draw_dev != nullptr) draw += (uint64_t)(uint32_t)draw_dev[0];   // device-side counter
  const uint64_t stream = select_stream(seed, draw, set, b);
  // input region: the sort keys (Np u64), then the zero-filled input (N floats) over them
  const size_t in_bytes = select ? (size_t)Np * 8 : (size_t)N * 4;
  float* xin = reinterpret_cast<float*>(lds);
  float* h0 = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + ((in_bytes + 15) & ~size_t(15)));
  float* h1 = h0 + ((net.hmax + 3) & ~3);

  uint64_t thr = ~0ull;
  if (select) {
    for (int p = tid; p < Np; p += kThreads) {
      uint64_t k = ~0ull;
      if (p < N) {
        const int t = p / F, f = p - t * F;
        const uint32_t hi = mode == PCA_SEL_MAXK ? desc_key(base[f * stride_f + t * stride_t])
                                                 : rand_key(stream, p);
        k = ((uint64_t)hi << 32) | (uint32_t)p;
      }
      lds[p] = k;
    }
    __syncthreads();
    for (int k = 2; k <= Np; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (Np >> 1); t += kThreads) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int l = i | j;
          const uint64_t a = lds[i], c = lds[l];
          const bool up = (i & k) == 0;
          if ((a > c) == up) {
            lds[i] = c;
            lds[l] = a;
          }
        }
        __syncthreads();
      }
    }
    thr = lds[K - 1];
    if (sel != nullptr)
      for (int q = tid; q < K; q += kThreads) sel[(int64_t)b * K + q] = (int32_t)(uint32_t)lds[q];
    __syncthreads();                                   // keys are overwritten next
  }
  for (int p = tid; p < N; p += kThreads) {
    const int t = p / F, f = p - t * F;
    const float v = base[f * stride_f + t * stride_t];
    bool keep = true;
    if (select) {
      const uint32_t hi = mode == PCA_SEL_MAXK ? desc_key(v) : rand_key(stream, p);
      keep = (((uint64_t)hi << 32) | (uint32_t)p) <= thr;
    }
    xin[p] = keep ? v : 0.f;
  }
  __syncthreads();

  const float* cur = xin;
  float* nxt = h0;
  if (net.cnn) {
    // y[l] = bias + sum_{t, k} Wc[t][k] x[t][l + k]   (cell p = t*F + f)
    const int kw = net.kw, Nt = net.Nt;
    for (int l = tid; l < net.L0; l += kThreads) {
      float acc = 0.f;
      for (int t = 0; t < Nt; ++t)
        for (int k = 0; k < kw; ++k) acc = fmaf(W[t * kw + k], xin[t * F + l + k], acc);
      h0[l] = acc + W[Nt * kw];
    }
    __syncthreads();
    cur = h0;
    nxt = h1;
  }
  for (int li = 0; li < net.nl; ++li) {
    dense(W + net.woff[li], cur, nxt, net.din[li], net.dout[li], li + 1 < net.nl, wave, lane);
    __syncthreads();
    const float* done = nxt;
    nxt = (nxt == h0) ? h1 : h0;
    cur = done;
  }
  // cur: the C outputs of the head
  float* o = out + (int64_t)b * C;
  if (net.cnn) {
    for (int c = tid; c < C; c += kThreads) o[c] = cur[c];
  } else if (wave == 0) {
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, cur[c]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(cur[c] - m);
    s = wave_sum(s);
    for (int c = lane; c < C; c += 64) o[c] = expf(cur[c] - m) / s;
  }
}

// shapes -> BaseNet; PCA_EINVAL with a message for anything the kernel cannot run
int make_net(int cnn, int F, int Nt, int Nf, const int* dims, int nd, int C, BaseNet* net,
             int64_t* n_params) {
  const char* who = cnn ? "cnn_temp_forward" : "fb_forward";
  PCA_REQUIRE(dims != nullptr, "%s: null layer_dims", who);
  PCA_REQUIRE(nd >= 1 && nd <= kMaxLinear - 1, "%s: %d layer_dims entries (1 .. %d)", who, nd,
              kMaxLinear - 1);
  PCA_REQUIRE(C >= 1, "%s: %d classes", who, C);
  for (int i = 0; i < nd; ++i) PCA_REQUIRE(dims[i] >= 1, "%s: layer_dims[%d] = %d", who, i, dims[i]);
  *net = BaseNet{};
  net->cnn = cnn;
  net->F = F;
  net->Nt = cnn ? Nt : 1;
  int64_t off = 0;
  int hmax = C;
  if (cnn) {
    PCA_REQUIRE(Nt >= 1, "%s: Nt = %d", who, Nt);
    PCA_REQUIRE(F == Nf, "%s: the chunks have F = %d bins, the model Nf = %d", who, F, Nf);
    net->kw = Nf + 1 - dims[0];
    PCA_REQUIRE(net->kw >= 1, "%s: conv width Nf + 1 - layer_dims[0] = %d", who, net->kw);
    net->L0 = dims[0];
    off = (int64_t)Nt * net->kw + 1;                 // cnn.weight [1, 1, Nt, kw], cnn.bias [1]
    hmax = hmax > dims[0] ? hmax : dims[0];
  } else {
    PCA_REQUIRE(F == dims[0], "%s: frames have F = %d bins, layer_dims[0] = %d", who, F, dims[0]);
  }
  net->nl = nd;
  for (int i = 0; i < nd; ++i) {
    const int di = dims[i], doo = i + 1 < nd ? dims[i + 1] : C;
    net->din[i] = di;
    net->dout[i] = doo;
    net->woff[i] = off;
    off += (int64_t)di * doo + doo;
    hmax = hmax > doo ? hmax : doo;
  }
  net->hmax = hmax;
  *n_params = off;
  return PCA_OK;
}

int launch(const char* who, const float* spec, int64_t sf, int64_t st, int64_t ss,
           const int64_t* idx, int B, const BaseNet& net, int C, const float* weights,
           int64_t n_weights, int64_t n_params, int K, int mode, uint64_t seed, uint64_t draw,
           const int32_t* draw_dev, float* out, int32_t* sel, const int64_t* labels,
           int64_t* labels_out, void* stream) {
  PCA_REQUIRE(spec && idx && weights && out, "%s: null pointer", who);
  PCA_REQUIRE(B > 0, "%s: B = %d", who, B);
  PCA_REQUIRE(n_weights == n_params, "%s: %lld weights given, the model has %lld", who,
              (long long)n_weights, (long long)n_params);
  PCA_REQUIRE(mode == PCA_SEL_MAXK || mode == PCA_SEL_RANDK || mode == PCA_SEL_ALL,
              "%s: mode = %d", who, mode);
  const int64_t N = (int64_t)net.F * net.Nt;
  PCA_REQUIRE(net.F >= 1 && N <= (1 << 24), "%s: %lld cells per set", who, (long long)N);
  int Np = 2;
  if (mode != PCA_SEL_ALL) {
    PCA_REQUIRE(N <= 16384, "%s: %lld cells per set with selection on (max 16384)", who,
                (long long)N);
    PCA_REQUIRE(K >= 1 && K <= N, "%s: K = %d outside [1, %lld]", who, K, (long long)N);
    while (Np < N) Np <<= 1;
  }
  const size_t in_bytes = mode != PCA_SEL_ALL ? (size_t)Np * 8 : (size_t)N * 4;
  const size_t lds = ((in_bytes + 15) & ~size_t(15)) + 2 * (size_t)((net.hmax + 3) & ~3) * 4;
  PCA_REQUIRE(lds <= kMaxLds, "%s: %zu bytes of LDS per set (max %zu): input or layers too wide",
              who, lds, kMaxLds);
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_baseline_fwd),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
  });
  hipLaunchKernelGGL(k_baseline_fwd, dim3((unsigned)B), dim3(kThreads), lds, as_stream(stream),
                     spec, sf, st, ss, idx, weights, net, K, mode, seed, draw, draw_dev, Np, C,
                     out, sel, labels, labels_out);
  return check_launch(who);
}

}  // namespace
}  // namespace pca

extern "C" {

int64_t pca_baseline_param_count(int cnn, int Nt, int Nf, const int* layer_dims_host, int n_dims,
                                 int nclasses) {
  pca::BaseNet net;
  int64_t n = 0;
  const int F = cnn ? Nf : (layer_dims_host && n_dims > 0 ? layer_dims_host[0] : 0);
  if (pca::make_net(cnn ? 1 : 0, F, Nt, Nf, layer_dims_host, n_dims, nclasses, &net, &n) != PCA_OK)
    return -1;
  return n;
}

int pca_fb_forward(const float* spec, int64_t stride_f, int64_t stride_s, const int64_t* idx,
                   int B, int F, const int* layer_dims_host, int n_dims, int nclasses,
                   const float* weights, int64_t n_weights, int K, int mode, uint64_t seed,
                   uint64_t draw, const int32_t* draw_dev, float* probs, int32_t* sel,
                   const int64_t* labels, int64_t* labels_out, void* stream) {
  pca::BaseNet net;
  int64_t n = 0;
  PCA_TRY(pca::make_net(0, F, 1, 0, layer_dims_host, n_dims, nclasses, &net, &n));
  return pca::launch("fb_forward", spec, stride_f, 0, stride_s, idx, B, net, nclasses, weights,
                     n_weights, n, K, mode, seed, draw, draw_dev, probs, sel, labels, labels_out,
                     stream);
}

int pca_cnn_temp_forward(const float* spec, int64_t stride_f, int64_t stride_t, int64_t stride_s,
                         const int64_t* idx, int B, int F, int Nt, int Nf,
                         const int* layer_dims_host, int n_dims, int nclasses,
                         const float* weights, int64_t n_weights, int K, int mode, uint64_t seed,
                         uint64_t draw, const int32_t* draw_dev, float* logits, int32_t* sel,
                         const int64_t* labels, int64_t* labels_out, void* stream) {
  pca::BaseNet net;
  int64_t n = 0;
  PCA_TRY(pca::make_net(1, F, Nt, Nf, layer_dims_host, n_dims, nclasses, &net, &n));
  return pca::launch("cnn_temp_forward", spec, stride_f, stride_t, stride_s, idx, B, net,
                     nclasses, weights, n_weights, n, K, mode, seed, draw, draw_dev, logits, sel,
                     labels, labels_out, stream);
}
}
