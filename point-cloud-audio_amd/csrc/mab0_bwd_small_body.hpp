// The layer-1 few-queries backward (dk <= 4, fp32 VALU) as a device function: the body of k_mab0_bwd_small
// (mab0_bwd_bf16.hip) and of the set rows of k_mab0_small_ride (wgrad128.hip), which runs it beside the bf16
// weight-gradient jobs of the step.
#pragma once
#include "bwd_defer.hpp"
#include "mfma_common.hpp"
#include "mid_bwd_body.hpp"

namespace pca {

// sink of the mid chain run in the prologue: dT (fp32) and Delta stay in LDS
constexpr int MID_SMALL_FUSE_IMG = (64 * 4 + 64) * 4;       // dTf [64][4] + Delta [64]
constexpr int MID_SMALL_FUSE_LDS = MID_SMALL_FUSE_IMG + MID_BWD_SMALL_LDS;
struct MidSinkSmall {
  float *sdTf, *sDel;       // [64][4], [64]
  __device__ __forceinline__ void dTb(int, int, int, bf16x4) const {}
  __device__ __forceinline__ void dTt(int, int, int, int, bf16x4) const {}
  __device__ __forceinline__ void dTf(int row, int c, float v) const { sdTf[row * 4 + c] = v; }
  __device__ __forceinline__ void stat(int row, float delta, float) const { sDel[row] = delta; }
};

struct Mab0SmallArgs {
  const float *X, *Gf, *dTf, *LSE, *Delta;
  int N, R, Rp, dk;
  float* DG;
  const int32_t* lengths;
  float* slabs;
  MidBwdArgs mid;
};

// layer 1 (dk <= 4): thread = (query row r, point partition); accumulates DG only.  The
// set's points are staged in LDS chunk by chunk (coalesced) and re-read from there.
// Set b; `ny` workgroups of NT threads share the rows of the set, this one (`y`) owns rows [row0, row0 + Rb)
// with NT / Rb point partitions: (NT, ny) = (256, 2) and (512, 1) give every (row, partition) the same
// points in the same order and the same order of the final sum, hence the same bits.
// MID (R == 64, an ISAB's first few-queries block): dTf / Delta are not read; every workgroup of a set
// runs the set's mid chain in `smid` (MID_SMALL_FUSE_LDS bytes).
// sD: [NT][4] floats, sX: PCA_POINT_CHUNK * 4 floats (16-byte aligned).
template <bool MID, int NT>
__device__ __forceinline__ void mab0_bwd_small_body(const Mab0SmallArgs& a, int b, unsigned y, unsigned ny,
                                                    float (*sD)[4], float* sX, char* smid) {
  constexpr int CH = PCA_POINT_CHUNK;
  const float* __restrict__ X = a.X;
  const float* __restrict__ Gf = a.Gf;
  const int N = a.N, R = a.R, dk = a.dk;
  const int tid = threadIdx.x;
  const int Rb = R / ny, row0 = y * Rb;
  const int parts = NT / Rb;
  const int rl = tid % Rb, part = tid / Rb;
  const int r = row0 + rl;
  constexpr float LN2 = 0.6931471805599453f;
  float gk[4], dt[4], acc[4];
  f32x2 acc2[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
  int len = N;
  if (a.lengths != nullptr) len = a.lengths[b] < N ? a.lengths[b] : N;
  float xr[4096 / NT];
  float lse, del;
  PCA_MID_STAMPS_DECL;       // (phase stamps of the fused mid chain: diagnostic builds only)
  if constexpr (MID) {
    // the first chunk of points, G and the statistics are in flight while the mid chain runs
#pragma unroll
    for (int c = 0; c < 4; ++c) gk[c] = c < dk ? Gf[r * dk + c] : 0.f;
    lse = a.LSE[(int64_t)b * R + r];
    if (len > 0) fetch_points<NT>(X + (int64_t)b * N * dk, len < CH ? len : CH, dk, xr);
    float* const sdTf = reinterpret_cast<float*>(smid);
    float* const sDelta = sdTf + 64 * 4;
    char* const base = smid + MID_SMALL_FUSE_IMG;
    mid_bwd_body<true, NT>(a.mid, b, mid_bwd_lds(base), y == 0, MidSinkSmall{sdTf, sDelta} PCA_MID_STAMPS_ARG);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) dt[c] = c < dk ? sdTf[r * 4 + c] : 0.f;
    del = sDelta[r];
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      gk[c] = c < dk ? Gf[r * dk + c] : 0.f;
      dt[c] = c < dk ? a.dTf[((int64_t)b * R + r) * dk + c] : 0.f;
    }
    lse = a.LSE[(int64_t)b * R + r];
    del = a.Delta[(int64_t)b * a.Rp + r];
    if (len > 0) fetch_points<NT>(X + (int64_t)b * N * dk, len < CH ? len : CH, dk, xr);
  }
  PCA_MID_STAMP(6);
  for (int n0 = 0; n0 < len; n0 += CH) {
    const int cn = (len - n0 < CH) ? len - n0 : CH;
    // [pair of points][component][2] (as k_mab0_attn_small): two points per packed-fp32 instruction;
    // unused components and the odd point of the chunk are zero; the next chunk's loads are in flight
    // while this one is worked on
    const int nfull = cn >> 1;       // pairs of two real points; an odd chunk ends in a half-filled one
    commit_points<NT>(xr, cn, dk, sX);
    if (n0 + CH < len)
      fetch_points<NT>(X + ((int64_t)b * N + n0 + CH) * dk, (len - n0 - CH < CH) ? len - n0 - CH : CH, dk,
                       xr);
    // half: the pair's second point is the chunk's zero padding.  Its score is 0 whatever the row, so
    // exp2(0 - lse) is +inf for a row whose scores all lie below -128 and inf * (x = 0) is NaN: its dS is
    // dropped, not multiplied by zero (k_mab0_attn_small masks the same point to -inf)
    auto pair = [&](int q, bool half) {
      const float4 lo = *reinterpret_cast<const float4*>(&sX[q * 8]);
      const float4 hi = *reinterpret_cast<const float4*>(&sX[q * 8 + 4]);
      const f32x2 x0 = {lo.x, lo.y}, x1 = {lo.z, lo.w}, x2 = {hi.x, hi.y}, x3 = {hi.z, hi.w};
      const f32x2 sc = gk[0] * x0 + gk[1] * x1 + gk[2] * x2 + gk[3] * x3;
      const f32x2 da = dt[0] * x0 + dt[1] * x1 + dt[2] * x2 + dt[3] * x3;
      const f32x2 pe = {__builtin_amdgcn_exp2f(sc[0] - lse), __builtin_amdgcn_exp2f(sc[1] - lse)};
      f32x2 ds = (LN2 * pe) * (da - del);
      if (half) ds[1] = 0.f;
      acc2[0] += ds * x0; acc2[1] += ds * x1; acc2[2] += ds * x2; acc2[3] += ds * x3;
    };
    if (part < parts) {
#pragma unroll 4
      for (int q = part; q < nfull; q += parts) pair(q, false);
      if ((cn & 1) && nfull % parts == part) pair(nfull, true);
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = acc2[c][0] + acc2[c][1];
#pragma unroll
  for (int c = 0; c < 4; ++c) sD[tid][c] = acc[c];
  __syncthreads();
  if (tid < Rb) {
    for (int c = 0; c < dk; ++c) {
      float v = 0.f;
      for (int p = 0; p < parts; ++p) v += sD[p * Rb + tid][c];
      // slabs != nullptr: per-set partial [b][R][dk] (summed in a fixed order by the caller)
      if (a.slabs != nullptr) a.slabs[((int64_t)b * R + row0 + tid) * dk + c] = v;
      else atomicAdd(&a.DG[(row0 + tid) * dk + c], v);
    }
  }
  if constexpr (MID) PCA_MID_STAMPS_WRITE(a.mid, b, y == 0);
}

// The bf16 weight-gradient list of a step (placed: bwd_defer_ride) and the layer-1 few-queries backward with
// its mid chain (R == 64, dk <= 4, per-set slabs) over B sets in ONE launch: k_mab0_small_ride, wgrad128.hip.
int mab0_small_ride_launch(const WgradJobs& bf16_jobs, int rows_per_wg, const Mab0SmallArgs& sets, int B,
                           hipStream_t st);

}  // namespace pca
