// What the ranking models (csrc/din.hip, csrc/dien.hip) share: the limits, the gather / scatter of the history and candidate
// rows, z = [v, q, v * q] and its backward, the tower (Linear + Dice / PReLU layers, the output layer, BCE over the live
// candidates) and the K-sliced weight-gradient GEMMs with their fixed-order sum.  The kernels live in csrc/din.hip only.
#pragma once
#include "gemm.hpp"
#include "seqrec.hpp"

namespace hiprec {

constexpr int kDinMaxDim = 128, kDinMaxLen = 256, kDinMaxDnn = 512, kDinMaxLayers = 3;
constexpr int64_t kDinMaxRows = 1ll << 24;     // B T and B C
constexpr int kDinSplitRows = 256;             // a K-slice of a weight-gradient GEMM is at least this long

// The tower over N candidate rows: its widths, where its parameters sit in the flat buffers (in[0] = the width of z) and in
// the running buffer, and its workspace.  dA / dB hold N x the widest layer (z included), sums 2 x that width, cs
// 2 * colsum_ws_floats(N, that width); the training-only buffers may be NULL in an eval forward.
struct DinTower {
  int L, act, W[kDinMaxLayers], in[kDinMaxLayers], bn[kDinMaxLayers];
  int64_t dw[kDinMaxLayers], db[kDinMaxLayers], da[kDinMaxLayers], ow, ob;
  float *x[kDinMaxLayers], *y[kDinMaxLayers], *mean, *var, *logit, *dlogit, *dA, *dB, *sums, *cs;
};

// rows [B T, D] = E[seq], q [N, D] = E[cand] (zero rows for ids that are not 1 .. n_items), the live flags lv / lc, the
// status word of an id out of range
int din_gather(const float* E, int64_t n_items, int D, const int64_t* seq, const int64_t* cand, int64_t BT, int64_t N,
               float* rows, float* q, uint8_t* lv, uint8_t* lc, hiprec_stats* stats, hipStream_t st);
// lv = mask != 0, lc = 1: the flags of a stage entry on explicit rows
int din_flags(const uint8_t* mask, uint8_t* lv, int64_t BT, uint8_t* lc, int64_t N, hipStream_t st);
// row atomics into g_item: drows [B T, D] at seq's ids, dqa + dqb [N, D] at cand's, live rows only
int din_scatter(const float* drows, const float* dqa, const float* dqb, const int64_t* seq, const int64_t* cand,
                const uint8_t* lv, const uint8_t* lc, int64_t BT, int64_t N, int D, float* g_item, hipStream_t st);
int din_fill(float* p, int64_t n, float v, hipStream_t st);
int din_add(float* dst, const float* src, int64_t n, hipStream_t st);
// z = [v, q, v * q] [N, 3 D]; its backward: dv = dz[:, :D] + dz[:, 2D:] * q, dq = dz[:, D:2D] + dz[:, 2D:] * v
int din_z(const float* v, const float* q, int64_t N, int D, float* z, hipStream_t st);
int din_z_bwd(const float* dz, const float* v, const float* q, int64_t N, int D, float* dv, float* dq, hipStream_t st);

// The layers over z [N, in[0]].  train: Dice reads the batch statistics of the live rows (and moves `running` when
// update_running), the logits go to t.logit; else Dice reads `running` and the logits go to logits_out, 0 in dead rows.
int din_tower_forward(const DinTower& t, const float* w_flat, float* running, int update_running, bool train,
                      const float* z, const uint8_t* lc, int64_t N, float* logits_out, hiprec_stats* stats,
                      hipStream_t st);
// BCE-with-logits over the live rows (the loss partials into scratch, the step advanced, t.logit copied to logits_out
// when given), then the backward of every layer: the tower's gradients into g_flat, *dz = d z [N, in[0]] (t.dA or t.dB)
int din_tower_backward(const DinTower& t, const float* w_flat, float* g_flat, const float* z, const uint8_t* lc,
                       const float* label, int64_t N, float* logits_out, Scratch* scratch, hiprec_stats* stats,
                       hipStream_t st, float** dz);

// C_i [M, N] = A[k_i .. k_i+1)^T B[k_i .. k_i+1) for up to `want` K-slices of at least kDinSplitRows rows: problems of the
// caller's grouped launch, each a block per tile with plain stores; returns the number of slices, which the caller adds
// in order (din_slab_sum)
int din_add_wgrad_slices(GemmGroup& g, int want, int M, int N, int K, const float* A, int lda, const float* Bm, int ldb,
                         float* parts);

#if defined(__HIPCC__)
// element `at` summed over n parts `stride` apart: eight running sums (part k into sum k % 8, so that eight loads are in
// flight at a time), folded as a tree.  The association depends on n alone: the same bits on every run.
__device__ __forceinline__ float din_slab_sum(const float* slabs, int n, int64_t stride, int64_t at) {
  float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < n; k += 8) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = k + i < n ? slabs[(k + i) * stride + at] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] += v[i];
  }
  return ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
}
#endif

}  // namespace hiprec
