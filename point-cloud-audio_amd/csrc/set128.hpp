// Set-resident kernels of the d = 128 / 4 heads / m = 16 / k = 1 train step (BASELINE configs[1]):
// a PAIR of workgroups carries a whole set through ISAB -> ISAB -> PMA (set_transformer-master/
// modules.py:51-53, 62-63 with :19-33 inside; Code/models.py:34-44), each its half of the set's
// [N, 128] activations resident in LDS.  The sets are dense, or padded with a length per set
// (Set128FwdArgs::lengths): the padding is masked out of the three attentions over the points, and the
// pair protocol - barriers, flags, hand-off payloads - is the same whatever the lengths are.
// Declarations shared by set128_fwd.hip and the ST engine.
#pragma once
#include "bwd_defer.hpp"

namespace pca {

// everything one ISAB of the set-resident forward reads and writes (pointers into the engine's
// weight images, the blocks' saved areas and the parameter vector; layouts are those the per-block
// kernels use, so the backward kernels read what this forward saved)
struct Set128Layer {
  // mab0 = MAB(I, X): few shared queries
  const float* Gf;        // [64][dk] fp32, sl2e folded in      (layer 1: dk = din <= 4)
  const __bf16* Gb;       // [64][128] bf16                      (layer 2)
  const float* Qp0;       // [16][128] fc_q(I)
  const __bf16* Wv0;      // [128][128] natural bf16 image       (layer 2)
  const float* Wv0f;      // [128][dk] fp32                      (layer 1)
  const float *bv0, *bo0;
  const __bf16* Wo0;      // natural
  float *T, *LSE;         // saved: [B][64][dk], [B][64]
  float *O0, *Z0, *H;     // [B][16][128] fp32
  // mab1 = MAB(X, H): many queries
  const __bf16 *Wk1, *Wv1;   // natural
  const float *bk1, *bv1;
  __bf16 *KpP, *VpP, *Kt, *Vt;
  const __bf16* WqB;      // natural                              (layer 2)
  const float* WqF;       // [128][dq] fp32                       (layer 1)
  const float* bq1;
  const __bf16* WoP;      // K-permuted
  const float* bo1;
  __bf16 *QpS, *OS, *Y;   // saved Qp (layer 2 only), saved O, the layer's output [B][N][128] (null:
                          // not stored - layer 2 when the PMA backward runs in the tail)
  uint32_t* mask;         // ReLU mask words, mab1_mask_index<128> layout
};

struct Set128FwdArgs {
  const float* X;         // [B][N][din] fp32
  int B, N, din;
  float scale_log2e;
  Set128Layer L[2];
  // pair exchange (scratch; `flags` is zeroed by the step's preparation launch):
  uint32_t* flags;        // [4] header (word 0 counts spin timeouts) + [B][2 exchanges][2 halves]
  float* ex2;             // [B][2][8192 + 1024] layer-2 attention partials (T as float4 [8][4][64], m / l)
  const __bf16* Gpma;     // [>= 16][128] bf16, rows >= 4 zero
  float *TpP, *MpP, *LpP; // PMA attention partials [B][Sp][4][128], [B][Sp][4] x 2 (read by k_pma_head1)
  int Sp;                 // 2 or 4
  // fuse_head != 0: the stages of k_pma_head1 (PMA epilogue, classifier, cross-entropy forward and
  // backward, PMA backward epilogue) run in this launch's tail on workgroup 0 of the pair, which gets
  // the partner's PMA partial through exP [B][2][528]; TpP / MpP / LpP are then not written
  int fuse_head;
  float* exP;
  PmaHeadArgs head;
  // pma_bwd != 0 (needs fuse_head): the PMA's attention backward runs in the tail as well (k_mab0_bwd's
  // arithmetic on the resident Y2 rows).  Hand-off 3 is then symmetric - both halves publish their
  // partial and run the head stages on the same merge, half 0 alone writes the head's outputs - and
  // each half writes dY2 of its rows and its S / 2 dG slabs - the same values k_mab0_bwd wrote
  int pma_bwd;
  __bf16* dY2;            // [B][N][128] bf16 (written, not accumulated)
  float* pma_slabs;       // [B][S][4][128], slab b S + sp over the points [sp N / S, (sp + 1) N / S)
  int pma_S;              // k_mab0_bwd's point splits per set (mab0_bwd_splits): 2, or 4 at N = 512
  // variable-length sets: device int32 [B], 1 <= lengths[b] <= N (pca_hip.h, "variable-size sets"), or null for
  // dense sets.  The points at and beyond lengths[b] are no keys of the three attentions over the points
  // (both ISABs' few-queries blocks, the PMA) and get exact-zero dY2 rows from the tail's PMA backward; their
  // rows of the many-queries blocks are computed from the (finite) padding and stored, as k_mab1_fwd does.
  // (Last member: the dense instantiations read every other argument at the offset it always had.)
  const int32_t* lengths;
};

// bytes of `flags` (the block the preparation launch clears) / of the whole exchange area
size_t set128_flag_bytes(int B);
size_t set128_fwd_ws_bytes(int B);
// N = 256 or 512 (each half a multiple of 128 points); din <= 4; 2 B workgroups resident at once
bool set128_shape_ok(int B, int N, int din, int d, int h, int m, int k);
int set128_fwd_launch(const Set128FwdArgs& a, hipStream_t st);

}  // namespace pca
