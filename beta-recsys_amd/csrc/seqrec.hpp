// What the sequence models (csrc/sasrec.hip, csrc/tisasrec.hip) share: the limits, the device helpers of their attention
// kernels, and the host launchers of the stages that are the same in both -- norm / count prep, embed, LayerNorm, the
// feed-forward GEMM groups, the BCE loss -- whose kernels live in csrc/seqrec.hip only.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace hiprec {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kSeqMaxDim = 128;
constexpr int kSeqMaxLen = 256;
constexpr int kSeqNormParts = 256;   // first-level partial sums of ||item_emb||^2
constexpr int kSeqAux = 2 + kSeqNormParts;   // [0] count of pos != 0, [1] ||item_emb||, [2..] the partial sums

// v_mfma_f32_16x16x4_f32 on operands in LDS: element (i, k) of A at A[i * sai + k * sak], element (k, j) of B at
// B[k * sbk + j * sbj]; lane l feeds A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15]; the result has
// col = lane & 15, row = 4 * (lane >> 4) + reg.
__device__ __forceinline__ f32x4 mma16(f32x4 acc, const float* A, int sai, int sak, const float* B, int sbk, int sbj,
                                       int K) {
  const int l = lane_id();
  const float* ap = A + (l & 15) * sai + (l >> 4) * sak;
  const float* bp = B + (l >> 4) * sbk + (l & 15) * sbj;
  for (int k = 0; k < K; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k * sak], bp[k * sbk], acc, 0, 0, 0);
  return acc;
}

// rows [r0, r0 + rows) x HD columns of src (leading dimension ld) into dst[rows][HD + 1]; rows >= limit are 0
template <int HD>
__device__ __forceinline__ void load_tile(float* dst, const float* __restrict__ src, int64_t ld, int r0, int rows,
                                          int limit, float scale) {
  for (int e = threadIdx.x; e < rows * HD; e += kBlock) {
    const int r = e / HD, c = e - r * HD;
    dst[r * (HD + 1) + c] = (r0 + r < limit) ? src[static_cast<int64_t>(r0 + r) * ld + c] * scale : 0.f;
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

template <typename F>
static int by_head_width(int hd, F&& f) {
  if (hd == 16) return f(std::integral_constant<int, 16>{});
  if (hd == 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, 64>{});
}

// n_items, n_blocks, heads, maxlen, dim and the head width of either shape struct; `model` names it in the message
int seq_check_shape(const char* model, int64_t n_items, int n_blocks, int heads, int maxlen, int dim);
// what both *_grad entry points require of a call; `need` = the model's workspace bytes for this batch
int seq_check_call(const void* w_flat, const void* g_flat, const void* seq, const void* pos, const void* neg,
                   int64_t batch, int seq_len, int maxlen, int heads, const void* feats_out, const void* stats,
                   const void* scratch, size_t scratch_bytes, const void* workspace, size_t workspace_bytes,
                   size_t need);

// training only: aux[0] = count(pos != 0); with l2 != 0 also aux[1] = ||W||_2 and g += l2 * W / ||W|| (2 launches)
int seq_prep(const float* W, float* g, int64_t n_w, const int64_t* pos, int64_t M, float l2, float* aux,
             hipStream_t st);
// x = (E[seq] * sqrt(D) + P[t]) * keep * (seq != 0); P == NULL: no positional row
int seq_embed(const float* E, const float* P, const int64_t* seq, int64_t M, int T, int D, int64_t n_items,
              float sqrt_d, const uint8_t* keep, float ks, float* x, hiprec_stats* stats, hipStream_t st);
int seq_ln_fwd(const float* a, const float* b, const int64_t* seq, float* xsum, const float* gamma, const float* beta,
               float* y, float* mean, float* rstd, int64_t M, int D, hipStream_t st);
// LayerNorm backward + its two column sums (d gamma from dyx, d beta from the summed dy); cs holds
// 2 * colsum_ws_floats(M, D) floats
int seq_ln_bwd(const float* dy_a, const float* dy_b, const float* a, const float* b, const float* gamma,
               const float* mean, const float* rstd, const float* dx_extra, const float* dx_extra2, const int64_t* seq,
               const uint8_t* keep, float ks, float* dx, float* dx_keep, float* dyx, float* dyt, float* g_gamma,
               float* g_beta, float* cs, int64_t M, int D, hipStream_t st);
// h1 = drop1(relu(conv1(f))), z = drop2(conv2(h1)): two launches; keep1 / keep2 may be NULL
int seq_ffn_fwd(int M, int D, const float* f, const float* c1_w, const float* c1_b, const float* c2_w,
                const float* c2_b, const uint8_t* keep1, const uint8_t* keep2, float ks, float* h1, float* z,
                hipStream_t st);
// from dz (already through keep2): d conv2, dh = the hidden gradient through keep1 and the ReLU, d conv1, df
int seq_ffn_bwd(int M, int D, const float* dz, const float* f, const float* h1, const float* c1_w, const float* c2_w,
                const uint8_t* keep1, float ks, float* dh, float* df, float* g_c1_w, float* g_c1_b, float* g_c2_w,
                float* g_c2_b, float* cs, hipStream_t st);
// BCE-with-logits over pos != 0: the loss partials, dfeats, row atomics into g_item
int seq_loss(const float* feats, const float* E, const int64_t* pos, const int64_t* neg, int64_t M, int D,
             int64_t n_items, const float* aux, float l2, float* dfeats, float* g_item, Scratch* scratch,
             hiprec_stats* stats, hipStream_t st);

}  // namespace hiprec
