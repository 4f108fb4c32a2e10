// BERT4Rec (Sun et al., CIKM 2019; no counterpart in the reference, the definition is include/hiprec.h's): zero_grad +
// forward + cloze loss + backward of BERT4RecEngine.train_single_batch as a fixed sequence of launches, no host sync.
// Activations are [M = B * T, D] row-major, row m = b * T + t.  Post-LN, bidirectional, key-padding mask from seq.
//
//   embed               raw = E[seq] + P[t] (0 at padding) -> LN_e -> dropout
//   per block           in_proj (one GEMM, q | k | v from x) -> attention over ALL keys with seq != 0 per (sequence,
//                       head) on the fp32 MFMA, probabilities never leave LDS -> out_proj + dropout1 (GEMM epilogue) ->
//                       y = LN_a(x + mha) -> fc1 (GEMM, pre-activation kept) -> GELU -> fc2 + dropout2 (GEMM epilogue) ->
//                       x' = LN_f(y + z)
//   head                gather of the n_lab labelled rows -> dense (GEMM) -> GELU -> LN_h
//   loss                cross-entropy over items 1 .. n_items against the tied table E, + out_bias: a block owns 32 rows of
//                       h in LDS and streams E through LDS in tiles of 64 items (score tile on the fp32 MFMA, running
//                       max / sum per row); no [n_lab, n_items] buffer exists.  Loss partials in a fixed order.
//   backward            cross-entropy in two kernels that recompute p = exp(score - lse): the row-tile owner writes dh,
//                       the item-tile owner writes d E[1 .. n_items] and d out_bias with plain stores into the zeroed
//                       gradient (no atomics); head backward; scatter into the feature gradient; then the chain in
//                       reverse: LayerNorm backward (seq_ln_bwd: dx; d gamma / d beta through the fixed-order column
//                       sums), GELU backward, dgrad / wgrad / bias GEMM groups (the weight gradients in up to 8 slabs of
//                       the batch with plain stores, folded in slab order: the same bits from run to run), attention
//                       backward in two kernels from the saved log-sum-exp (one owns a query tile and writes dQ, the
//                       other owns a key tile and writes dK and dV: no atomics), embed backward (row atomics into the
//                       item rows, [MASK] included, after the cross-entropy's plain stores; pos_emb in a fixed order).
//
// Saved per block: x, the projected [M, 3D] q | k | v, the attention output, mha (through dropout1), y, the fc1
// pre-activation [M, F], z (through dropout2), two (mean, rstd) pairs and the log-sum-exp per (sequence, head, query).
// Saved once: raw and LN_e's (mean, rstd); of the head Xc, the dense pre-activation, its GELU, h, LN_h's (mean, rstd)
// and the cross-entropy's log-sum-exp per labelled row.  Recomputed: attention scores and probabilities, GELU(fc1) in
// the backward, every cross-entropy score and probability (twice).  A query with no open key stores a large finite
// log-sum-exp; its probabilities are zero because every key of it is closed.
#include <vector>

#include "gemm.hpp"
#include "seqrec.hpp"

namespace hiprec {

constexpr int kB4rMaxFfn = 512;
constexpr int kB4rQT = 32;                  // query (or key) rows a block owns
constexpr int kB4rSLd = kSeqMaxLen + 4;     // leading dimension of the score rows in LDS
constexpr float kB4rClosedLse = 3.0e38f;    // log-sum-exp of a row with no open key: exp(s - it) == 0 for every finite s
constexpr int kB4rSlabs = 8;                // batch slabs of a weight-gradient GEMM

// ---- elementwise -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_f32(float z) { return 0.5f * z * (1.0f + erff(z * 0.70710678118654752440f)); }

__device__ __forceinline__ float gelu_grad_f32(float z) {
  return 0.5f * (1.0f + erff(z * 0.70710678118654752440f)) + z * 0.39894228040143267794f * expf(-0.5f * z * z);
}

__global__ __launch_bounds__(kBlock) void b4r_gelu_fwd_kernel(const float* __restrict__ pre, float* __restrict__ act,
                                                              int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) act[i] = gelu_f32(pre[i]);
}

// d pre = d act * gelu'(pre), in place on d
__global__ __launch_bounds__(kBlock) void b4r_gelu_bwd_kernel(float* d, const float* __restrict__ pre, int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride)
    d[i] = d[i] * gelu_grad_f32(pre[i]);
}

// out = keep ? (a + b) * ks : 0; b may be NULL
__global__ __launch_bounds__(kBlock) void b4r_keep_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          const uint8_t* __restrict__ keep, float ks,
                                                          float* __restrict__ out, int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    float v = a[i];
    if (b) v += b[i];
    out[i] = keep[i] ? v * ks : 0.f;
  }
}

// out[i] = sum over the slabs, in slab order
__global__ __launch_bounds__(kBlock) void b4r_fold_kernel(float* __restrict__ out, const float* __restrict__ part,
                                                          int64_t n, int slabs) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    float s = part[i];
    for (int k = 1; k < slabs; ++k) s += part[k * n + i];
    out[i] = s;
  }
}

// Xc[r] = x[lab_pos[r]]; a position outside [0, M) or a label outside [1, n_items] raises the status and gathers zeros
__global__ __launch_bounds__(kBlock) void b4r_gather_kernel(const float* __restrict__ x,
                                                            const int64_t* __restrict__ lab_pos,
                                                            const int64_t* __restrict__ lab_item, int64_t n_lab,
                                                            int64_t M, int64_t n_items, int D, float* __restrict__ xc,
                                                            hiprec_stats* stats) {
  const int64_t n = n_lab * D, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t r = i / D;
    const int d = static_cast<int>(i - r * D);
    const int64_t m = lab_pos[r], it = lab_item[r];
    const bool ok = m >= 0 && m < M;
    if (d == 0 && (!ok || it < 1 || it > n_items)) atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
    xc[i] = ok ? x[m * D + d] : 0.f;
  }
}

// dx[lab_pos[r]] = dxc[r] into a zeroed dx: lab_pos is ascending and unique, so plain stores suffice
__global__ __launch_bounds__(kBlock) void b4r_scatter_kernel(const float* __restrict__ dxc,
                                                             const int64_t* __restrict__ lab_pos, int64_t n_lab,
                                                             int64_t M, int D, float* __restrict__ dx) {
  const int64_t n = n_lab * D, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t r = i / D;
    const int64_t m = lab_pos[r];
    if (m >= 0 && m < M) dx[m * D + (i - r * D)] = dxc[i];
  }
}

// no labelled position: the loss is 0, the step still counts
__global__ void b4r_empty_loss_kernel(Scratch* scratch, hiprec_stats* stats) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    scratch->n_partials = 1;
    scratch->partials[0] = make_float4(0.f, 0.f, 0.f, 0.f);
    advance_step(stats);
  }
}

// d item_emb[seq] += dx (row atomics, id 0 skipped, [MASK] = n_items + 1 included), d pos_emb[t] += sum_b dx: one
// thread per (t, d) walks the batch in order, so the positional gradient is the same from run to run
__global__ __launch_bounds__(kBlock) void b4r_embed_bwd_kernel(const float* __restrict__ dx,
                                                               const int64_t* __restrict__ seq, int64_t B, int T, int D,
                                                               int64_t max_id, float* __restrict__ g_item,
                                                               float* __restrict__ g_pos) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= T * D) return;
  const int t = e / D, d = e - t * D;
  float acc = 0.f;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t m = b * T + t;
    const int64_t id = seq[m];
    if (id <= 0 || id > max_id) continue;
    const float gv = dx[m * D + d];
    atomic_add_f32(g_item + id * D + d, gv);
    acc += gv;
  }
  g_pos[e] += acc;
}

// ---- bidirectional attention per (sequence, head) ----------------------------------------------------------------------
// grid (B * H, ceil(T / 32)).  qkv [M, 3D]: q | k | v.  Key j is open when seq[b, j] != 0.  keep (optional)
// [B * H, T, T] bytes on the probabilities.
template <int HD>
__global__ __launch_bounds__(kBlock) void b4r_attn_fwd_kernel(const float* __restrict__ qkv,
                                                              const int64_t* __restrict__ seq, int T, int H, int D,
                                                              const uint8_t* __restrict__ keep, float ks,
                                                              float* __restrict__ O, float* __restrict__ lse) {
  __shared__ float Qs[kB4rQT][HD + 1];
  __shared__ float Ks[64][HD + 1];
  __shared__ float S[kB4rQT][kB4rSLd];
  __shared__ uint8_t s_open[kSeqMaxLen];
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int q0 = blockIdx.y * kB4rQT;
  const int lane = lane_id(), wave = wave_in_block();
  const int64_t ld = 3 * D;
  const float* base = qkv + static_cast<int64_t>(b) * T * ld + h * HD;
  const float scale = 1.0f / sqrtf(static_cast<float>(HD));
  for (int j = threadIdx.x; j < kSeqMaxLen; j += kBlock)
    s_open[j] = (j < T && seq[static_cast<int64_t>(b) * T + j] != 0) ? 1 : 0;
  load_tile<HD>(&Qs[0][0], base, ld, q0, kB4rQT, T, scale);
  const int n_chunks = (T + 63) / 64;
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * 64;
    __syncthreads();
    load_tile<HD>(&Ks[0][0], base + D, ld, j0, 64, T, 1.f);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int tile = wave * 2 + u, rt = tile >> 2, ct = tile & 3;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = mma16(acc, &Qs[rt * 16][0], HD + 1, 1, &Ks[ct * 16][0], 1, HD + 1, HD);
#pragma unroll
      for (int r = 0; r < 4; ++r) S[rt * 16 + 4 * (lane >> 4) + r][j0 + ct * 16 + (lane & 15)] = acc[r];
    }
  }
  __syncthreads();
  const int width = n_chunks * 64;
  for (int rr = 0; rr < kB4rQT / kWavesPerBlock; ++rr) {
    const int row = wave * (kB4rQT / kWavesPerBlock) + rr, i = q0 + row;
    if (i >= T) {                       // a row past the sequence: finite zeros for the product below
      for (int j = lane; j < width; j += 64) S[row][j] = 0.f;
      continue;
    }
    float mx = -INFINITY;
    for (int j = lane; j < width; j += 64)
      if (s_open[j]) mx = fmaxf(mx, S[row][j]);
    mx = wave_max(mx);
    const bool any = mx > -INFINITY;    // no open key: every probability is 0, nothing below subtracts infinities
    const float m = any ? mx : 0.f;
    float sum = 0.f;
    for (int j = lane; j < width; j += 64) {
      const float e = s_open[j] ? expf(S[row][j] - m) : 0.f;
      S[row][j] = e;
      sum += e;
    }
    sum = wave_sum(sum);
    const float inv = any ? 1.0f / sum : 0.f;
    const uint8_t* kp = keep ? keep + (static_cast<int64_t>(bh) * T + i) * T : nullptr;
    for (int j = lane; j < width; j += 64) {
      float p = S[row][j] * inv;
      if (kp && j < T) p = kp[j] ? p * ks : 0.f;
      S[row][j] = p;
    }
    if (lane == 0) lse[static_cast<int64_t>(bh) * T + i] = any ? m + logf(sum) : kB4rClosedLse;
  }
  constexpr int kColTiles = HD / 16, kTiles = 2 * kColTiles;
  f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * 64;
    __syncthreads();
    load_tile<HD>(&Ks[0][0], base + 2 * D, ld, j0, 64, T, 1.f);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = wave + kWavesPerBlock * u;
      if (t < kTiles) {
        const int rt = t / kColTiles, ct = t - rt * kColTiles;
        acc[u] = mma16(acc[u], &S[rt * 16][j0], kB4rSLd, 1, &Ks[0][ct * 16], HD + 1, 1, 64);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int t = wave + kWavesPerBlock * u;
    if (t < kTiles) {
      const int rt = t / kColTiles, ct = t - rt * kColTiles;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = q0 + rt * 16 + 4 * (lane >> 4) + r;
        if (i < T) O[(static_cast<int64_t>(b) * T + i) * D + h * HD + ct * 16 + (lane & 15)] = acc[u][r];
      }
    }
  }
}

// backward, query side: a block owns 32 queries and walks all keys in chunks of 64.  P = exp(S - lse) on open keys,
// dP = dO V^T through the keep bytes, dS = P * (dP - delta) with delta = rowsum(dO * O); dQ = dS K / sqrt(hd).
// Writes delta [B * H, T] for the key-side kernel and the q third of dqkv [M, 3D].
template <int HD>
__global__ __launch_bounds__(kBlock) void b4r_attn_bwd_q_kernel(const float* __restrict__ qkv,
                                                                const int64_t* __restrict__ seq,
                                                                const float* __restrict__ dO,
                                                                const float* __restrict__ O,
                                                                const float* __restrict__ lse, int T, int H, int D,
                                                                const uint8_t* __restrict__ keep, float ks,
                                                                float* __restrict__ delta, float* __restrict__ dqkv) {
  __shared__ float Qs[kB4rQT][HD + 1];
  __shared__ float Gs[kB4rQT][HD + 1];
  __shared__ float Ks[64][HD + 1];
  __shared__ float Vs[64][HD + 1];
  __shared__ float DS[kB4rQT][65];
  __shared__ float s_lse[kB4rQT], s_delta[kB4rQT];
  __shared__ uint8_t s_open[kSeqMaxLen];
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int q0 = blockIdx.y * kB4rQT;
  const int lane = lane_id(), wave = wave_in_block();
  const int64_t ld = 3 * D;
  const float* base = qkv + static_cast<int64_t>(b) * T * ld + h * HD;
  const float* g_base = dO + static_cast<int64_t>(b) * T * D + h * HD;
  const float* o_base = O + static_cast<int64_t>(b) * T * D + h * HD;
  const float scale = 1.0f / sqrtf(static_cast<float>(HD));
  for (int j = threadIdx.x; j < kSeqMaxLen; j += kBlock)
    s_open[j] = (j < T && seq[static_cast<int64_t>(b) * T + j] != 0) ? 1 : 0;
  load_tile<HD>(&Qs[0][0], base, ld, q0, kB4rQT, T, scale);
  load_tile<HD>(&Gs[0][0], g_base, D, q0, kB4rQT, T, 1.f);
  __syncthreads();
  {
    const int row = threadIdx.x >> 3, part = threadIdx.x & 7, i = q0 + row;    // 8 threads per row
    float s = 0.f;
    if (i < T)
      for (int c = part; c < HD; c += 8) s += Gs[row][c] * o_base[static_cast<int64_t>(i) * D + c];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (part == 0) {
      s_delta[row] = s;
      s_lse[row] = i < T ? lse[static_cast<int64_t>(bh) * T + i] : 0.f;
      if (i < T) delta[static_cast<int64_t>(bh) * T + i] = s;
    }
  }
  const int n_chunks = (T + 63) / 64;
  constexpr int kColTiles = HD / 16, kTiles = 2 * kColTiles;
  f32x4 acc_q[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * 64;
    __syncthreads();
    load_tile<HD>(&Ks[0][0], base + D, ld, j0, 64, T, 1.f);
    load_tile<HD>(&Vs[0][0], base + 2 * D, ld, j0, 64, T, 1.f);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int tile = wave * 2 + u, rt = tile >> 2, ct = tile & 3;
      f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
      s = mma16(s, &Qs[rt * 16][0], HD + 1, 1, &Ks[ct * 16][0], 1, HD + 1, HD);
      dp = mma16(dp, &Gs[rt * 16][0], HD + 1, 1, &Vs[ct * 16][0], 1, HD + 1, HD);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rt * 16 + 4 * (lane >> 4) + r, col = ct * 16 + (lane & 15);
        const int i = q0 + row, j = j0 + col;
        float ds = 0.f;
        if (i < T && s_open[j]) {
          const float p = expf(s[r] - s_lse[row]);
          float d = dp[r];
          if (keep) d = keep[(static_cast<int64_t>(bh) * T + i) * T + j] ? d * ks : 0.f;
          ds = p * (d - s_delta[row]);
        }
        DS[row][col] = ds;
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = wave + kWavesPerBlock * u;
      if (t < kTiles) {
        const int rt = t / kColTiles, ct = t - rt * kColTiles;
        acc_q[u] = mma16(acc_q[u], &DS[rt * 16][0], 65, 1, &Ks[0][ct * 16], HD + 1, 1, 64);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int t = wave + kWavesPerBlock * u;
    if (t < kTiles) {
      const int rt = t / kColTiles, ct = t - rt * kColTiles;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = q0 + rt * 16 + 4 * (lane >> 4) + r;
        if (i < T) dqkv[(static_cast<int64_t>(b) * T + i) * ld + h * HD + ct * 16 + (lane & 15)] = acc_q[u][r] * scale;
      }
    }
  }
}

// backward, key side: a block owns 32 keys and walks ALL queries in chunks of 32.  S^T = K Q^T,
// dK = dS^T (q / sqrt(hd)), dV = (P through the keep bytes)^T dO, each summed in a fixed order: no atomics.  A closed
// key receives exactly zero.
template <int HD>
__global__ __launch_bounds__(kBlock) void b4r_attn_bwd_kv_kernel(const float* __restrict__ qkv,
                                                                 const int64_t* __restrict__ seq,
                                                                 const float* __restrict__ dO,
                                                                 const float* __restrict__ lse,
                                                                 const float* __restrict__ delta, int T, int H, int D,
                                                                 const uint8_t* __restrict__ keep, float ks,
                                                                 float* __restrict__ dqkv) {
  __shared__ float Ks[kB4rQT][HD + 1];
  __shared__ float Vs[kB4rQT][HD + 1];
  __shared__ float Qc[32][HD + 1];
  __shared__ float Gc[32][HD + 1];
  __shared__ float PT[kB4rQT][33];
  __shared__ float DST[kB4rQT][33];
  __shared__ float s_lse[32], s_delta[32];
  __shared__ uint8_t s_open[kB4rQT];
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int j0 = blockIdx.y * kB4rQT;
  const int lane = lane_id(), wave = wave_in_block();
  const int64_t ld = 3 * D;
  const float* base = qkv + static_cast<int64_t>(b) * T * ld + h * HD;
  const float* g_base = dO + static_cast<int64_t>(b) * T * D + h * HD;
  const float scale = 1.0f / sqrtf(static_cast<float>(HD));
  if (threadIdx.x < kB4rQT) {
    const int j = j0 + threadIdx.x;
    s_open[threadIdx.x] = (j < T && seq[static_cast<int64_t>(b) * T + j] != 0) ? 1 : 0;
  }
  load_tile<HD>(&Ks[0][0], base + D, ld, j0, kB4rQT, T, 1.f);
  load_tile<HD>(&Vs[0][0], base + 2 * D, ld, j0, kB4rQT, T, 1.f);
  constexpr int kColTiles = HD / 16, kTiles = 2 * kColTiles;
  f32x4 acc_k[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  f32x4 acc_v[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int i0 = 0; i0 < T; i0 += 32) {
    __syncthreads();
    load_tile<HD>(&Qc[0][0], base, ld, i0, 32, T, scale);
    load_tile<HD>(&Gc[0][0], g_base, D, i0, 32, T, 1.f);
    if (threadIdx.x < 32) {
      const int i = i0 + threadIdx.x;
      s_lse[threadIdx.x] = i < T ? lse[static_cast<int64_t>(bh) * T + i] : 0.f;
      s_delta[threadIdx.x] = i < T ? delta[static_cast<int64_t>(bh) * T + i] : 0.f;
    }
    __syncthreads();
    {
      const int rt = wave >> 1, ct = wave & 1;       // 2 x 2 tiles of the [32 keys, 32 queries] block, one per wave
      f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
      s = mma16(s, &Ks[rt * 16][0], HD + 1, 1, &Qc[ct * 16][0], 1, HD + 1, HD);
      dp = mma16(dp, &Vs[rt * 16][0], HD + 1, 1, &Gc[ct * 16][0], 1, HD + 1, HD);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rt * 16 + 4 * (lane >> 4) + r, col = ct * 16 + (lane & 15);
        const int j = j0 + row, i = i0 + col;
        float ds = 0.f, pd = 0.f;
        if (i < T && s_open[row]) {
          const float p = expf(s[r] - s_lse[col]);
          float d = dp[r];
          pd = p;
          if (keep) {
            const bool kept = keep[(static_cast<int64_t>(bh) * T + i) * T + j] != 0;
            d = kept ? d * ks : 0.f;
            pd = kept ? p * ks : 0.f;
          }
          ds = p * (d - s_delta[col]);
        }
        PT[row][col] = pd;
        DST[row][col] = ds;
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = wave + kWavesPerBlock * u;
      if (t < kTiles) {
        const int rt = t / kColTiles, ct = t - rt * kColTiles;
        acc_k[u] = mma16(acc_k[u], &DST[rt * 16][0], 33, 1, &Qc[0][ct * 16], HD + 1, 1, 32);
        acc_v[u] = mma16(acc_v[u], &PT[rt * 16][0], 33, 1, &Gc[0][ct * 16], HD + 1, 1, 32);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int t = wave + kWavesPerBlock * u;
    if (t < kTiles) {
      const int rt = t / kColTiles, ct = t - rt * kColTiles;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + rt * 16 + 4 * (lane >> 4) + r;
        if (j < T) {
          float* out = dqkv + (static_cast<int64_t>(b) * T + j) * ld + h * HD + ct * 16 + (lane & 15);
          out[D] = acc_k[u][r];
          out[2 * D] = acc_v[u][r];
        }
      }
    }
  }
}

// ---- cross-entropy over the catalogue with tied embeddings ---------------------------------------------------------------
// Tiles: 32 labelled rows of h x 64 items.  Column c of item tile jt is item 64 jt + 1 + c (row 0 of E is padding and
// the last row is [MASK]: neither is a class).  Ragged edges are masked by index: a row past n_lab is zeros with weight 0,
// a column past n_items has logit -inf.
constexpr int kCeRows = 32, kCeItems = 64, kCeLd = kSeqMaxDim + 1;

__device__ __forceinline__ void ce_load_rows(float (*Hs)[kCeLd], const float* __restrict__ h, int64_t r0, int64_t n_lab,
                                             int D) {
  for (int e = threadIdx.x; e < kCeRows * D; e += kBlock) {
    const int r = e / D, c = e - r * D;
    Hs[r][c] = r0 + r < n_lab ? h[(r0 + r) * D + c] : 0.f;
  }
}

__device__ __forceinline__ void ce_load_items(float (*Es)[kCeLd], float* s_bias, const float* __restrict__ E,
                                              const float* __restrict__ out_bias, int64_t j0, int64_t n_items, int D) {
  for (int e = threadIdx.x; e < kCeItems * D; e += kBlock) {
    const int r = e / D, c = e - r * D;
    const int64_t j = j0 + 1 + r;
    Es[r][c] = j <= n_items ? E[j * D + c] : 0.f;
  }
  if (threadIdx.x < kCeItems) {
    const int64_t j = j0 + 1 + threadIdx.x;
    s_bias[threadIdx.x] = j <= n_items ? out_bias[j] : -INFINITY;
  }
}

// S[r][c] = <h_r, E_c> + out_bias_c on the fp32 MFMA: 2 x 4 tiles of 16 x 16, two per wave
__device__ __forceinline__ void ce_scores(float (*S)[kCeItems + 1], const float (*Hs)[kCeLd], const float (*Es)[kCeLd],
                                          const float* s_bias, int D) {
  const int lane = lane_id(), wave = wave_in_block();
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int tile = wave * 2 + u, rt = tile >> 2, ct = tile & 3;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = mma16(acc, &Hs[rt * 16][0], kCeLd, 1, &Es[ct * 16][0], 1, kCeLd, D);
    const int col = ct * 16 + (lane & 15);
    const float bias = s_bias[col];
#pragma unroll
    for (int r = 0; r < 4; ++r) S[rt * 16 + 4 * (lane >> 4) + r][col] = acc[r] + bias;
  }
}

// per labelled row of the tile: its log-sum-exp, its label and its weight 1 / n_lab (0 past n_lab or for a bad label)
__device__ __forceinline__ void ce_load_meta(float* s_lse, int64_t* s_lab, float* s_w, const float* __restrict__ lse,
                                             const int64_t* __restrict__ lab_item, int64_t r0, int64_t n_lab,
                                             int64_t n_items, float inv) {
  if (threadIdx.x < kCeRows) {
    const int64_t r = r0 + threadIdx.x;
    const bool in = r < n_lab;
    const int64_t lab = in ? lab_item[r] : 0;
    s_lse[threadIdx.x] = in ? lse[r] : 0.f;
    s_lab[threadIdx.x] = lab;
    s_w[threadIdx.x] = (lab >= 1 && lab <= n_items) ? inv : 0.f;
  }
}

// S <- G = (p - [item == label]) * weight, p = exp(score - lse)
__device__ __forceinline__ void ce_probs_to_grad(float (*S)[kCeItems + 1], const float* s_lse, const int64_t* s_lab,
                                                 const float* s_w, int64_t j0) {
  for (int e = threadIdx.x; e < kCeRows * kCeItems; e += kBlock) {
    const int r = e >> 6, c = e & 63;
    const float w = s_w[r];
    float g = 0.f;
    if (w != 0.f) {
      const float p = expf(S[r][c] - s_lse[r]);
      g = (p - (s_lab[r] == j0 + 1 + c ? 1.f : 0.f)) * w;
    }
    S[r][c] = g;
  }
}

// forward: grid (row tiles, item splits).  Block (x, y) streams the item tiles [y * tiles_per_split, ...) past its rows
// and leaves per row the running maximum, the sum of exp(score - maximum) and the label's logit (0 when the label is in
// another split) at part_*[y * n_lab + row]; b4r_ce_combine_kernel folds the splits in order.
__global__ __launch_bounds__(kBlock) void b4r_ce_fwd_kernel(const float* __restrict__ h, const float* __restrict__ E,
                                                            const float* __restrict__ out_bias,
                                                            const int64_t* __restrict__ lab_item, int64_t n_lab,
                                                            int64_t n_items, int D, int64_t tiles_per_split,
                                                            float* __restrict__ part_m, float* __restrict__ part_l,
                                                            float* __restrict__ part_pick) {
  __shared__ float Hs[kCeRows][kCeLd];
  __shared__ float Es[kCeItems][kCeLd];
  __shared__ float S[kCeRows][kCeItems + 1];
  __shared__ float s_bias[kCeItems];
  __shared__ int64_t s_lab[kCeRows];
  constexpr int kPer = kCeRows / kWavesPerBlock;    // rows a wave reduces
  const int lane = lane_id(), wave = wave_in_block();
  const int64_t n_tiles = (n_lab + kCeRows - 1) / kCeRows, n_item_tiles = (n_items + kCeItems - 1) / kCeItems;
  const int64_t jt_lo = blockIdx.y * tiles_per_split;
  const int64_t jt_hi = jt_lo + tiles_per_split < n_item_tiles ? jt_lo + tiles_per_split : n_item_tiles;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t r0 = tile * kCeRows;
    __syncthreads();
    ce_load_rows(Hs, h, r0, n_lab, D);
    if (threadIdx.x < kCeRows) {        // a label outside 1 .. n_items (or past n_lab) is kept as 0: never picked
      const int64_t lab = r0 + threadIdx.x < n_lab ? lab_item[r0 + threadIdx.x] : 0;
      s_lab[threadIdx.x] = lab >= 1 && lab <= n_items ? lab : 0;
    }
    float m[kPer], l[kPer], pick[kPer];
#pragma unroll
    for (int rr = 0; rr < kPer; ++rr) {
      m[rr] = -INFINITY;
      l[rr] = 0.f;
      pick[rr] = 0.f;
    }
    for (int64_t jt = jt_lo; jt < jt_hi; ++jt) {
      const int64_t j0 = jt * kCeItems;
      __syncthreads();
      ce_load_items(Es, s_bias, E, out_bias, j0, n_items, D);
      __syncthreads();
      ce_scores(S, Hs, Es, s_bias, D);
      __syncthreads();
#pragma unroll
      for (int rr = 0; rr < kPer; ++rr) {
        const int row = wave * kPer + rr;
        const float s = S[row][lane];
        // a split's first tile starts inside the catalogue, so the running maximum is finite from that tile on: -inf
        // never meets -inf
        const float mn = fmaxf(m[rr], wave_max(s));
        l[rr] = l[rr] * expf(m[rr] - mn) + wave_sum(expf(s - mn));
        m[rr] = mn;
        const int64_t c = s_lab[row] - 1 - j0;
        if (c >= 0 && c < kCeItems) pick[rr] = S[row][c];
      }
    }
#pragma unroll
    for (int rr = 0; rr < kPer; ++rr) {
      const int64_t r = r0 + wave * kPer + rr;
      if (r < n_lab && lane == 0) {
        const int64_t at = static_cast<int64_t>(blockIdx.y) * n_lab + r;
        part_m[at] = m[rr];
        part_l[at] = l[rr];
        part_pick[at] = pick[rr];
      }
    }
  }
}

// lse [n_lab] from the splits' (maximum, sum) pairs in split order, the loss partial of every block in a fixed order;
// block 0 advances the step counter
__global__ __launch_bounds__(kBlock) void b4r_ce_combine_kernel(const float* __restrict__ part_m,
                                                                const float* __restrict__ part_l,
                                                                const float* __restrict__ part_pick,
                                                                const int64_t* __restrict__ lab_item, int64_t n_lab,
                                                                int64_t n_items, int splits, float* __restrict__ lse,
                                                                Scratch* scratch, hiprec_stats* stats) {
  __shared__ float s_red[kBlock];
  float loss = 0.f;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; r < n_lab; r += stride) {
    float m = part_m[r];
    for (int s = 1; s < splits; ++s) m = fmaxf(m, part_m[s * n_lab + r]);
    float l = 0.f, pick = 0.f;
    for (int s = 0; s < splits; ++s) {
      l += part_l[s * n_lab + r] * expf(part_m[s * n_lab + r] - m);
      pick += part_pick[s * n_lab + r];
    }
    const float v = m + logf(l);
    lse[r] = v;
    const int64_t lab = lab_item[r];
    if (lab >= 1 && lab <= n_items) loss += v - pick;
  }
  s_red[threadIdx.x] = loss;
  __syncthreads();
  for (int r = kBlock / 2; r > 0; r >>= 1) {
    if (static_cast<int>(threadIdx.x) < r) s_red[threadIdx.x] += s_red[threadIdx.x + r];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0) {
      scratch->n_partials = gridDim.x;
      advance_step(stats);
    }
    scratch->partials[blockIdx.x] = make_float4(s_red[0] / static_cast<float>(n_lab), 0.f, 0.f, 0.f);
  }
}

// backward, row side: grid (row tiles, item splits).  The owner of 32 labelled rows streams its split of the catalogue
// and writes sum_j G_j E_j over that split into slab blockIdx.y of dh [splits, n_lab, D]; b4r_fold_kernel adds the slabs
// in split order (one split: dh itself)
__global__ __launch_bounds__(kBlock) void b4r_ce_bwd_h_kernel(const float* __restrict__ h, const float* __restrict__ E,
                                                              const float* __restrict__ out_bias,
                                                              const int64_t* __restrict__ lab_item,
                                                              const float* __restrict__ lse, int64_t n_lab,
                                                              int64_t n_items, int D, int64_t tiles_per_split,
                                                              float* __restrict__ dh) {
  __shared__ float Hs[kCeRows][kCeLd];
  __shared__ float Es[kCeItems][kCeLd];
  __shared__ float S[kCeRows][kCeItems + 1];
  __shared__ float s_bias[kCeItems];
  __shared__ float s_lse[kCeRows], s_w[kCeRows];
  __shared__ int64_t s_lab[kCeRows];
  const int lane = lane_id(), wave = wave_in_block();
  const int64_t n_tiles = (n_lab + kCeRows - 1) / kCeRows, n_item_tiles = (n_items + kCeItems - 1) / kCeItems;
  const float inv = 1.0f / static_cast<float>(n_lab);
  const int col_tiles = D / 16, tiles = 2 * col_tiles;     // of the [32, D] output, up to 16: four per wave
  const int64_t jt_lo = blockIdx.y * tiles_per_split;
  const int64_t jt_hi = jt_lo + tiles_per_split < n_item_tiles ? jt_lo + tiles_per_split : n_item_tiles;
  dh += static_cast<int64_t>(blockIdx.y) * n_lab * D;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t r0 = tile * kCeRows;
    __syncthreads();
    ce_load_rows(Hs, h, r0, n_lab, D);
    ce_load_meta(s_lse, s_lab, s_w, lse, lab_item, r0, n_lab, n_items, inv);
    f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int64_t jt = jt_lo; jt < jt_hi; ++jt) {
      const int64_t j0 = jt * kCeItems;
      __syncthreads();
      ce_load_items(Es, s_bias, E, out_bias, j0, n_items, D);
      __syncthreads();
      ce_scores(S, Hs, Es, s_bias, D);
      __syncthreads();
      ce_probs_to_grad(S, s_lse, s_lab, s_w, j0);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = wave + kWavesPerBlock * u;
        if (t < tiles) {
          const int rt = t / col_tiles, ct = t - rt * col_tiles;
          acc[u] = mma16(acc[u], &S[rt * 16][0], kCeItems + 1, 1, &Es[0][ct * 16], kCeLd, 1, kCeItems);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = wave + kWavesPerBlock * u;
      if (t < tiles) {
        const int rt = t / col_tiles, ct = t - rt * col_tiles;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t i = r0 + rt * 16 + 4 * (lane >> 4) + r;
          if (i < n_lab) dh[i * D + ct * 16 + (lane & 15)] = acc[u][r];
        }
      }
    }
  }
}

// backward, item side: the owner of 64 items walks all row tiles and writes d E_j = sum_r G_rj h_r and
// d out_bias_j = sum_r G_rj with plain stores, rows in ascending order
__global__ __launch_bounds__(kBlock) void b4r_ce_bwd_e_kernel(const float* __restrict__ h, const float* __restrict__ E,
                                                              const float* __restrict__ out_bias,
                                                              const int64_t* __restrict__ lab_item,
                                                              const float* __restrict__ lse, int64_t n_lab,
                                                              int64_t n_items, int D, float* __restrict__ g_item,
                                                              float* __restrict__ g_out_bias) {
  __shared__ float Hs[kCeRows][kCeLd];
  __shared__ float Es[kCeItems][kCeLd];
  __shared__ float S[kCeRows][kCeItems + 1];
  __shared__ float s_bias[kCeItems];
  __shared__ float s_lse[kCeRows], s_w[kCeRows];
  __shared__ int64_t s_lab[kCeRows];
  const int lane = lane_id(), wave = wave_in_block();
  const int64_t n_tiles = (n_lab + kCeRows - 1) / kCeRows, n_item_tiles = (n_items + kCeItems - 1) / kCeItems;
  const float inv = 1.0f / static_cast<float>(n_lab);
  const int col_tiles = D / 16, tiles = 4 * col_tiles;     // of the [64, D] output, up to 32: eight per wave
  for (int64_t jt = blockIdx.x; jt < n_item_tiles; jt += gridDim.x) {
    const int64_t j0 = jt * kCeItems;
    __syncthreads();
    ce_load_items(Es, s_bias, E, out_bias, j0, n_items, D);
    f32x4 acc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    for (int64_t tile = 0; tile < n_tiles; ++tile) {
      const int64_t r0 = tile * kCeRows;
      __syncthreads();
      ce_load_rows(Hs, h, r0, n_lab, D);
      ce_load_meta(s_lse, s_lab, s_w, lse, lab_item, r0, n_lab, n_items, inv);
      __syncthreads();
      ce_scores(S, Hs, Es, s_bias, D);
      __syncthreads();
      ce_probs_to_grad(S, s_lse, s_lab, s_w, j0);
      __syncthreads();
      if (threadIdx.x < kCeItems) {
#pragma unroll 8
        for (int r = 0; r < kCeRows; ++r) bsum += S[r][threadIdx.x];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = wave + kWavesPerBlock * u;
        if (t < tiles) {
          const int it = t / col_tiles, ct = t - it * col_tiles;
          acc[u] = mma16(acc[u], &S[0][it * 16], 1, kCeItems + 1, &Hs[0][ct * 16], kCeLd, 1, kCeRows);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int t = wave + kWavesPerBlock * u;
      if (t < tiles) {
        const int it = t / col_tiles, ct = t - it * col_tiles;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t j = j0 + 1 + it * 16 + 4 * (lane >> 4) + r;
          if (j <= n_items) g_item[j * D + ct * 16 + (lane & 15)] = acc[u][r];
        }
      }
    }
    if (threadIdx.x < kCeItems && j0 + 1 + threadIdx.x <= n_items) g_out_bias[j0 + 1 + threadIdx.x] = bsum;
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------
struct B4rParams {      // pointers into a flat buffer laid out in state_dict() order
  float *item_emb, *pos_emb, *ln_e_w, *ln_e_b, *hd_w, *hd_b, *ln_h_w, *ln_h_b, *out_bias;
  std::vector<float*> in_w, in_b, out_w, out_b, ln_a_w, ln_a_b, f1_w, f1_b, f2_w, f2_b, ln_f_w, ln_f_b;
};

static int64_t b4r_n_params(const hiprec_bert4rec_shape& s) {
  const int64_t D = s.dim, F = s.ffn_dim;
  return (s.n_items + 2) * D + static_cast<int64_t>(s.maxlen) * D + 2 * D +
         s.n_blocks * (4 * D * D + 4 * D + 2 * D + 2 * D * F + F + D + 2 * D) + D * D + D + 2 * D + s.n_items + 1;
}

static B4rParams b4r_params(float* base, const hiprec_bert4rec_shape& s) {
  B4rParams p;
  const int64_t D = s.dim, F = s.ffn_dim;
  const int nb = s.n_blocks;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += n; return r; };
  p.item_emb = take((s.n_items + 2) * D);
  p.pos_emb = take(static_cast<int64_t>(s.maxlen) * D);
  p.ln_e_w = take(D);
  p.ln_e_b = take(D);
  for (int k = 0; k < nb; ++k) {
    p.in_w.push_back(take(3 * D * D)); p.in_b.push_back(take(3 * D));
    p.out_w.push_back(take(D * D)); p.out_b.push_back(take(D));
  }
  for (int k = 0; k < nb; ++k) { p.ln_a_w.push_back(take(D)); p.ln_a_b.push_back(take(D)); }
  for (int k = 0; k < nb; ++k) {
    p.f1_w.push_back(take(F * D)); p.f1_b.push_back(take(F));
    p.f2_w.push_back(take(D * F)); p.f2_b.push_back(take(D));
  }
  for (int k = 0; k < nb; ++k) { p.ln_f_w.push_back(take(D)); p.ln_f_b.push_back(take(D)); }
  p.hd_w = take(D * D);
  p.hd_b = take(D);
  p.ln_h_w = take(D);
  p.ln_h_b = take(D);
  p.out_bias = take(s.n_items + 1);
  return p;
}

struct B4rWorkspace {
  std::vector<float*> x, qkv, o, mha, y, pre, z, mean_a, rstd_a, mean_f, rstd_f, lse;
  float *raw, *mean_e, *rstd_e, *feats, *xc, *hpre, *hact, *hh, *mean_h, *rstd_h, *lse_ce, *dh;
  float *ce_m, *ce_l, *ce_pick, *dh_part;     // per (item split, labelled row)
  float *t[8], *tf[2], *dqkv, *delta, *cs, *part;
  int64_t floats;
};

// The cross-entropy's row-side kernels cut the catalogue into splits so that about kCeTargetBlocks blocks run: with
// r row tiles, min(kCeMaxSplits, ceil(kCeTargetBlocks / r), item tiles) of them.
constexpr int kCeMaxSplits = 16, kCeTargetBlocks = 1024;

static int b4r_splits(int64_t row_tiles, int64_t item_tiles, int64_t* tiles_per_split) {
  int64_t s = (kCeTargetBlocks + row_tiles - 1) / row_tiles;
  if (s > kCeMaxSplits) s = kCeMaxSplits;
  if (s > item_tiles) s = item_tiles;
  if (s < 1) s = 1;
  *tiles_per_split = (item_tiles + s - 1) / s;
  return static_cast<int>((item_tiles + *tiles_per_split - 1) / *tiles_per_split);      // no split is empty
}

// the most (split, labelled row) pairs a call on M positions can have: splits * n_lab <= 16 n_lab while n_lab <= 2048,
// and <= (kCeTargetBlocks / r + 1) * 32 r <= 32 kCeTargetBlocks + n_lab + 32 beyond
static int64_t b4r_split_rows(int64_t M) {
  const int64_t a = kCeMaxSplits * M, b = 32 * kCeTargetBlocks + M + 32;
  return a < b ? a : b;
}

// nothing here depends on n_items: the cross-entropy keeps no score of any (row, item) pair in global memory
static B4rWorkspace b4r_carve(float* base, const hiprec_bert4rec_shape& s, int64_t B, int T) {
  B4rWorkspace w;
  const int64_t D = s.dim, F = s.ffn_dim, M = B * T, MD = M * D, MF = M * F, MH = M * s.heads;
  const int wide = static_cast<int>(3 * D > F ? 3 * D : F);
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += (n + 3) / 4 * 4; return r; };
  for (int k = 0; k < s.n_blocks; ++k) {
    w.x.push_back(take(MD)); w.qkv.push_back(take(3 * MD)); w.o.push_back(take(MD)); w.mha.push_back(take(MD));
    w.y.push_back(take(MD)); w.pre.push_back(take(MF)); w.z.push_back(take(MD));
    w.mean_a.push_back(take(M)); w.rstd_a.push_back(take(M)); w.mean_f.push_back(take(M)); w.rstd_f.push_back(take(M));
    w.lse.push_back(take(MH));
  }
  w.raw = take(MD); w.mean_e = take(M); w.rstd_e = take(M); w.feats = take(MD);
  w.xc = take(MD); w.hpre = take(MD); w.hact = take(MD); w.hh = take(MD); w.mean_h = take(M); w.rstd_h = take(M);
  w.lse_ce = take(M); w.dh = take(MD);
  const int64_t split_rows = b4r_split_rows(M);
  w.ce_m = take(split_rows); w.ce_l = take(split_rows); w.ce_pick = take(split_rows); w.dh_part = take(split_rows * D);
  for (int i = 0; i < 8; ++i) w.t[i] = take(MD);
  for (int i = 0; i < 2; ++i) w.tf[i] = take(MF);
  w.dqkv = take(3 * MD);
  w.delta = take(MH);
  w.cs = take(2 * colsum_ws_floats(static_cast<int>(M), wide));
  w.part = take(kB4rSlabs * wide * D);
  w.floats = c - base;
  return w;
}

static int b4r_check_shape(const hiprec_bert4rec_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  if (int rc = seq_check_shape("BERT4Rec", s->n_items, s->n_blocks, s->heads, s->maxlen, s->dim)) return rc;
  HIPREC_REQUIRE(s->ffn_dim >= 1 && s->ffn_dim <= kB4rMaxFfn, "BERT4Rec needs ffn_dim in 1 .. %d (got %d)", kB4rMaxFfn,
                 s->ffn_dim);
  return 0;
}

static void b4r_set_keep(GemmProblem& p, const uint8_t* keep, int ld, float ks) {
  if (keep) { p.keep = keep; p.ldk = ld; p.keep_scale = ks; }
}

static int b4r_gelu_fwd(const float* pre, float* act, int64_t n, hipStream_t st) {
  b4r_gelu_fwd_kernel<<<grid_for_threads(n), kBlock, 0, st>>>(pre, act, n);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

static int b4r_gelu_bwd(float* d, const float* pre, int64_t n, hipStream_t st) {
  b4r_gelu_bwd_kernel<<<grid_for_threads(n), kBlock, 0, st>>>(d, pre, n);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// C[rows, cols] = A^T B over K batch rows, as problems of g: one with plain stores into the zeroed gradient, or (long K)
// up to kB4rSlabs slabs of K into `part`, which b4r_fold adds up in slab order afterwards.  Returns the slab count.
static int b4r_add_wgrad(GemmGroup& g, int rows, int cols, int K, const float* A, int lda, const float* Bm, int ldb,
                         float* out, float* part) {
  int slabs = (K + 511) / 512;
  if (slabs > kB4rSlabs) slabs = kB4rSlabs;
  if (slabs <= 1) {
    g.p[g.n++] = make_gemm(kTNm, rows, cols, K, A, lda, Bm, ldb, out, cols, nullptr, 0, nullptr, 0, false);
    return 1;
  }
  const int per = ((K + slabs - 1) / slabs + 15) / 16 * 16;
  int s = 0;
  for (int k0 = 0; k0 < K; k0 += per, ++s)
    g.p[g.n++] = make_gemm(kTNm, rows, cols, K - k0 < per ? K - k0 : per, A + static_cast<int64_t>(k0) * lda, lda,
                           Bm + static_cast<int64_t>(k0) * ldb, ldb, part + static_cast<int64_t>(s) * rows * cols, cols,
                           nullptr, 0, nullptr, 0, false);
  return s;
}

static int b4r_fold(float* out, const float* part, int64_t n, int slabs, hipStream_t st) {
  if (slabs <= 1) return 0;
  b4r_fold_kernel<<<grid_for_threads(n), kBlock, 0, st>>>(out, part, n, slabs);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// h = LN_h(gelu(dense(x))) on n rows; pre / act [n, D], mean / rstd [n]
static int b4r_head_fwd(const B4rParams& w, int n, int D, const float* x, float* pre, float* act, float* out,
                        float* mean, float* rstd, hipStream_t st) {
  GemmGroup g{};
  g.n = 1;
  g.p[0] = make_gemm(kNT, n, D, D, x, D, w.hd_w, D, pre, D, w.hd_b, 0, nullptr, 0, false);
  if (int rc = launch_group(g, st)) return rc;
  if (int rc = b4r_gelu_fwd(pre, act, static_cast<int64_t>(n) * D, st)) return rc;
  return seq_ln_fwd(act, nullptr, nullptr, nullptr, w.ln_h_w, w.ln_h_b, out, mean, rstd, n, D, st);
}

static int b4r_run(const hiprec_bert4rec_shape& s, float* w_flat, float* g_flat, const int64_t* seq, int64_t n_lab,
                   const int64_t* lab_pos, const int64_t* lab_item, int64_t B, int T, const uint8_t* const* keep, float ks,
                   float* feats_out, hiprec_stats* stats, Scratch* scratch, float* ws_base, hipStream_t st) {
  const int D = s.dim, H = s.heads, nb = s.n_blocks, hd = D / H, F = s.ffn_dim;
  const int64_t M = B * T, MD = M * D, MF = M * F;
  const int Mi = static_cast<int>(M), Ni = static_cast<int>(n_lab);
  const bool train = g_flat != nullptr;
  const B4rParams w = b4r_params(w_flat, s);
  const B4rWorkspace a = b4r_carve(ws_base, s, B, T);
  auto kp = [&](int i) -> const uint8_t* { return keep ? keep[i] : nullptr; };
  const dim3 attn_grid(static_cast<unsigned>(B * H), static_cast<unsigned>((T + kB4rQT - 1) / kB4rQT));

  // ---- forward ----
  if (int rc = seq_embed(w.item_emb, w.pos_emb, seq, M, T, D, s.n_items + 1, 1.0f, nullptr, ks, a.raw, stats, st)) return rc;
  if (int rc = seq_ln_fwd(a.raw, nullptr, nullptr, nullptr, w.ln_e_w, w.ln_e_b, kp(0) ? a.t[0] : a.x[0], a.mean_e,
                          a.rstd_e, M, D, st))
    return rc;
  if (kp(0)) {
    b4r_keep_kernel<<<grid_for_threads(MD), kBlock, 0, st>>>(a.t[0], nullptr, kp(0), ks, a.x[0], MD);
    HIPREC_TRY(hipGetLastError());
  }
  for (int k = 0; k < nb; ++k) {
    GemmGroup g{};
    g.n = 1;
    g.p[0] = make_gemm(kNT, Mi, 3 * D, D, a.x[k], D, w.in_w[k], D, a.qkv[k], 3 * D, w.in_b[k], 0, nullptr, 0, false);
    if (int rc = launch_group(g, st)) return rc;
    if (int rc = by_head_width(hd, [&](auto hw) {
          b4r_attn_fwd_kernel<decltype(hw)::value><<<attn_grid, kBlock, 0, st>>>(a.qkv[k], seq, T, H, D, kp(1 + 3 * k),
                                                                                 ks, a.o[k], a.lse[k]);
          HIPREC_TRY(hipGetLastError());
          return 0;
        }))
      return rc;
    g = GemmGroup{};
    g.n = 1;
    g.p[0] = make_gemm(kNT, Mi, D, D, a.o[k], D, w.out_w[k], D, a.mha[k], D, w.out_b[k], 0, nullptr, 0, false);
    b4r_set_keep(g.p[0], kp(2 + 3 * k), D, ks);
    if (int rc = launch_group(g, st)) return rc;
    if (int rc = seq_ln_fwd(a.x[k], a.mha[k], nullptr, nullptr, w.ln_a_w[k], w.ln_a_b[k], a.y[k], a.mean_a[k],
                            a.rstd_a[k], M, D, st))
      return rc;
    g = GemmGroup{};
    g.n = 1;
    g.p[0] = make_gemm(kNT, Mi, F, D, a.y[k], D, w.f1_w[k], D, a.pre[k], F, w.f1_b[k], 0, nullptr, 0, false);
    if (int rc = launch_group(g, st)) return rc;
    if (int rc = b4r_gelu_fwd(a.pre[k], a.tf[0], MF, st)) return rc;
    g = GemmGroup{};
    g.n = 1;
    g.p[0] = make_gemm(kNT, Mi, D, F, a.tf[0], F, w.f2_w[k], F, a.z[k], D, w.f2_b[k], 0, nullptr, 0, false);
    b4r_set_keep(g.p[0], kp(3 + 3 * k), D, ks);
    if (int rc = launch_group(g, st)) return rc;
    const bool last = k + 1 == nb;
    if (int rc = seq_ln_fwd(a.y[k], a.z[k], nullptr, nullptr, w.ln_f_w[k], w.ln_f_b[k],
                            last ? (train ? a.feats : feats_out) : a.x[k + 1], a.mean_f[k], a.rstd_f[k], M, D, st))
      return rc;
  }
  if (!train) return 0;
  if (n_lab == 0) {     // loss 0, every gradient stays exactly zero
    b4r_empty_loss_kernel<<<1, 64, 0, st>>>(scratch, stats);
    HIPREC_TRY(hipGetLastError());
    return 0;
  }

  // ---- head and cross-entropy ----
  const B4rParams g = b4r_params(g_flat, s);
  float *S1 = a.t[0], *S1k = a.t[1], *S2 = a.t[2], *S3 = a.t[3], *S3k = a.t[4], *X1 = a.t[5], *U1 = a.t[6], *U2 = a.t[7];
  const int64_t ND = n_lab * D;
  b4r_gather_kernel<<<grid_for_threads(ND), kBlock, 0, st>>>(a.feats, lab_pos, lab_item, n_lab, M, s.n_items, D, a.xc,
                                                             stats);
  HIPREC_TRY(hipGetLastError());
  if (int rc = b4r_head_fwd(w, Ni, D, a.xc, a.hpre, a.hact, a.hh, a.mean_h, a.rstd_h, st)) return rc;
  const int64_t row_tiles = (n_lab + kCeRows - 1) / kCeRows, item_tiles = (s.n_items + kCeItems - 1) / kCeItems;
  const int item_grid = static_cast<int>(item_tiles < (1 << 20) ? item_tiles : (1 << 20));
  int64_t tiles_per_split = 0;
  const int splits = b4r_splits(row_tiles, item_tiles, &tiles_per_split);
  const dim3 row_grid(static_cast<unsigned>(row_tiles < kMaxBlocks ? row_tiles : kMaxBlocks), static_cast<unsigned>(splits));
  b4r_ce_fwd_kernel<<<row_grid, kBlock, 0, st>>>(a.hh, w.item_emb, w.out_bias, lab_item, n_lab, s.n_items, D,
                                                 tiles_per_split, a.ce_m, a.ce_l, a.ce_pick);
  HIPREC_TRY(hipGetLastError());
  b4r_ce_combine_kernel<<<grid_for_threads(n_lab), kBlock, 0, st>>>(a.ce_m, a.ce_l, a.ce_pick, lab_item, n_lab, s.n_items,
                                                                    splits, a.lse_ce, scratch, stats);
  HIPREC_TRY(hipGetLastError());
  b4r_ce_bwd_h_kernel<<<row_grid, kBlock, 0, st>>>(a.hh, w.item_emb, w.out_bias, lab_item, a.lse_ce, n_lab, s.n_items, D,
                                                   tiles_per_split, splits > 1 ? a.dh_part : a.dh);
  HIPREC_TRY(hipGetLastError());
  if (int rc = b4r_fold(a.dh, a.dh_part, ND, splits, st)) return rc;
  b4r_ce_bwd_e_kernel<<<item_grid, kBlock, 0, st>>>(a.hh, w.item_emb, w.out_bias, lab_item, a.lse_ce, n_lab, s.n_items,
                                                    D, g.item_emb, g.out_bias);
  HIPREC_TRY(hipGetLastError());
  // LN_h backward -> S1 = d gelu(dense); GELU backward in place; X1 = d Xc
  if (int rc = seq_ln_bwd(a.dh, nullptr, a.hact, nullptr, w.ln_h_w, a.mean_h, a.rstd_h, nullptr, nullptr, nullptr,
                          nullptr, ks, S1, nullptr, U1, U2, g.ln_h_w, g.ln_h_b, a.cs, n_lab, D, st))
    return rc;
  if (int rc = b4r_gelu_bwd(S1, a.hpre, ND, st)) return rc;
  {
    GemmGroup q{};
    q.p[q.n++] = make_gemm(kNN, Ni, D, D, S1, D, w.hd_w, D, X1, D, nullptr, 0, nullptr, 0, false);
    const int slabs = b4r_add_wgrad(q, D, D, Ni, S1, D, a.xc, D, g.hd_w, a.part);
    q.p[q.n++] = make_colsum(S1, Ni, D, D, g.hd_b, a.cs);
    if (int rc = launch_group(q, st)) return rc;
    if (int rc = launch_colsum_reduce(q, st)) return rc;
    if (int rc = b4r_fold(g.hd_w, a.part, static_cast<int64_t>(D) * D, slabs, st)) return rc;
  }
  HIPREC_TRY(hipMemsetAsync(S3, 0, sizeof(float) * MD, st));
  b4r_scatter_kernel<<<grid_for_threads(ND), kBlock, 0, st>>>(X1, lab_pos, n_lab, M, D, S3);
  HIPREC_TRY(hipGetLastError());

  // ---- the blocks in reverse: (dA, dB) = the two summands of the gradient of a block's output ----
  const float *dA = S3, *dB = nullptr;
  for (int k = nb - 1; k >= 0; --k) {
    // LN_f: S1 = gradient of y + z, S1k = the same through dropout2
    if (int rc = seq_ln_bwd(dA, dB, a.y[k], a.z[k], w.ln_f_w[k], a.mean_f[k], a.rstd_f[k], nullptr, nullptr, nullptr,
                            kp(3 + 3 * k), ks, S1, S1k, U1, U2, g.ln_f_w[k], g.ln_f_b[k], a.cs, M, D, st))
      return rc;
    const float* dz = kp(3 + 3 * k) ? S1k : S1;
    if (int rc = b4r_gelu_fwd(a.pre[k], a.tf[0], MF, st)) return rc;
    {
      GemmGroup q{};
      q.p[q.n++] = make_gemm(kNN, Mi, F, D, dz, D, w.f2_w[k], F, a.tf[1], F, nullptr, 0, nullptr, 0, false);
      const int slabs = b4r_add_wgrad(q, D, F, Mi, dz, D, a.tf[0], F, g.f2_w[k], a.part);
      q.p[q.n++] = make_colsum(dz, Mi, D, D, g.f2_b[k], a.cs);
      if (int rc = launch_group(q, st)) return rc;
      if (int rc = launch_colsum_reduce(q, st)) return rc;
      if (int rc = b4r_fold(g.f2_w[k], a.part, static_cast<int64_t>(D) * F, slabs, st)) return rc;
    }
    if (int rc = b4r_gelu_bwd(a.tf[1], a.pre[k], MF, st)) return rc;
    {
      GemmGroup q{};
      q.p[q.n++] = make_gemm(kNN, Mi, D, F, a.tf[1], F, w.f1_w[k], D, S2, D, nullptr, 0, nullptr, 0, false);
      const int slabs = b4r_add_wgrad(q, F, D, Mi, a.tf[1], F, a.y[k], D, g.f1_w[k], a.part);
      q.p[q.n++] = make_colsum(a.tf[1], Mi, F, F, g.f1_b[k], a.cs);
      if (int rc = launch_group(q, st)) return rc;
      if (int rc = launch_colsum_reduce(q, st)) return rc;
      if (int rc = b4r_fold(g.f1_w[k], a.part, static_cast<int64_t>(D) * F, slabs, st)) return rc;
    }
    // LN_a: dy = d(fc1 input) + the residual's gradient; S3 = gradient of x + mha, S3k = the same through dropout1
    if (int rc = seq_ln_bwd(S2, S1, a.x[k], a.mha[k], w.ln_a_w[k], a.mean_a[k], a.rstd_a[k], nullptr, nullptr, nullptr,
                            kp(2 + 3 * k), ks, S3, S3k, U1, U2, g.ln_a_w[k], g.ln_a_b[k], a.cs, M, D, st))
      return rc;
    const float* dm = kp(2 + 3 * k) ? S3k : S3;
    {
      GemmGroup q{};
      q.p[q.n++] = make_gemm(kNN, Mi, D, D, dm, D, w.out_w[k], D, S2, D, nullptr, 0, nullptr, 0, false);
      const int slabs = b4r_add_wgrad(q, D, D, Mi, dm, D, a.o[k], D, g.out_w[k], a.part);
      q.p[q.n++] = make_colsum(dm, Mi, D, D, g.out_b[k], a.cs);
      if (int rc = launch_group(q, st)) return rc;
      if (int rc = launch_colsum_reduce(q, st)) return rc;
      if (int rc = b4r_fold(g.out_w[k], a.part, static_cast<int64_t>(D) * D, slabs, st)) return rc;
    }
    if (int rc = by_head_width(hd, [&](auto hw) {
          constexpr int HD = decltype(hw)::value;
          b4r_attn_bwd_q_kernel<HD><<<attn_grid, kBlock, 0, st>>>(a.qkv[k], seq, S2, a.o[k], a.lse[k], T, H, D,
                                                                  kp(1 + 3 * k), ks, a.delta, a.dqkv);
          HIPREC_TRY(hipGetLastError());
          b4r_attn_bwd_kv_kernel<HD><<<attn_grid, kBlock, 0, st>>>(a.qkv[k], seq, S2, a.lse[k], a.delta, T, H, D,
                                                                   kp(1 + 3 * k), ks, a.dqkv);
          HIPREC_TRY(hipGetLastError());
          return 0;
        }))
      return rc;
    {
      GemmGroup q{};
      q.p[q.n++] = make_gemm(kNN, Mi, D, 3 * D, a.dqkv, 3 * D, w.in_w[k], D, X1, D, nullptr, 0, nullptr, 0, false);
      const int slabs = b4r_add_wgrad(q, 3 * D, D, Mi, a.dqkv, 3 * D, a.x[k], D, g.in_w[k], a.part);
      q.p[q.n++] = make_colsum(a.dqkv, Mi, 3 * D, 3 * D, g.in_b[k], a.cs);
      if (int rc = launch_group(q, st)) return rc;
      if (int rc = launch_colsum_reduce(q, st)) return rc;
      if (int rc = b4r_fold(g.in_w[k], a.part, static_cast<int64_t>(3) * D * D, slabs, st)) return rc;
    }
    dA = S3;        // the residual's share of d x[k] ...
    dB = X1;        // ... and the attention's
  }
  // embedding: dropout, LN_e (padding rows get exactly zero), the two tables
  if (kp(0)) {
    b4r_keep_kernel<<<grid_for_threads(MD), kBlock, 0, st>>>(dA, dB, kp(0), ks, S2, MD);
    HIPREC_TRY(hipGetLastError());
    dA = S2;
    dB = nullptr;
  }
  if (int rc = seq_ln_bwd(dA, dB, a.raw, nullptr, w.ln_e_w, a.mean_e, a.rstd_e, nullptr, nullptr, seq, nullptr, ks, S1,
                          nullptr, U1, U2, g.ln_e_w, g.ln_e_b, a.cs, M, D, st))
    return rc;
  b4r_embed_bwd_kernel<<<(T * D + kBlock - 1) / kBlock, kBlock, 0, st>>>(S1, seq, B, T, D, s.n_items + 1, g.item_emb,
                                                                         g.pos_emb);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_bert4rec_shape_bytes(void) { return sizeof(hiprec_bert4rec_shape); }

extern "C" int64_t hiprec_bert4rec_param_floats(const hiprec_bert4rec_shape* shape) {
  if (b4r_check_shape(shape)) return -1;
  return b4r_n_params(*shape);
}

extern "C" size_t hiprec_bert4rec_workspace_bytes(const hiprec_bert4rec_shape* shape, int64_t batch, int32_t seq_len) {
  if (b4r_check_shape(shape) || batch <= 0 || seq_len <= 0) return 0;
  return sizeof(float) * static_cast<size_t>(b4r_carve(nullptr, *shape, batch, seq_len).floats);
}

extern "C" int hiprec_bert4rec_grad(const hiprec_bert4rec_shape* shape, const float* w_flat, float* g_flat,
                                    const int64_t* seq, int64_t n_lab, const int64_t* lab_pos, const int64_t* lab_item,
                                    int64_t batch, int32_t seq_len, const uint8_t* const* keep, float keep_scale,
                                    float* feats_out, hiprec_stats* stats, void* scratch, size_t scratch_bytes,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = b4r_check_shape(shape)) return rc;
  // seq stands in for the two id arrays the shared check wants of a training call: the labels are checked below
  if (int rc = seq_check_call(w_flat, g_flat, seq, seq, seq, batch, seq_len, shape->maxlen, shape->heads, feats_out, stats,
                              scratch, scratch_bytes, workspace, workspace_bytes,
                              hiprec_bert4rec_workspace_bytes(shape, batch, seq_len)))
    return rc;
  if (g_flat) {
    HIPREC_REQUIRE(n_lab >= 0 && n_lab <= batch * seq_len, "n_lab outside [0, batch x sequence length]");
    HIPREC_REQUIRE(n_lab == 0 || (lab_pos && lab_item), "labelled positions without their arrays");
  }
  return b4r_run(*shape, const_cast<float*>(w_flat), g_flat, seq, g_flat ? n_lab : 0, lab_pos, lab_item, batch, seq_len,
                 keep, keep_scale, feats_out, stats, static_cast<Scratch*>(scratch), static_cast<float*>(workspace),
                 static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_bert4rec_head(const hiprec_bert4rec_shape* shape, const float* w_flat, const float* rows, int64_t n,
                                    float* out, float* tmp, size_t tmp_floats, void* stream) {
  if (int rc = b4r_check_shape(shape)) return rc;
  HIPREC_REQUIRE(w_flat && rows && out && tmp, "NULL pointer");
  HIPREC_REQUIRE(n >= 1 && n < (1ll << 24), "bad row count");
  const int64_t nd = (n * shape->dim + 3) / 4 * 4, n4 = (n + 3) / 4 * 4;
  HIPREC_REQUIRE(tmp_floats >= static_cast<size_t>(2 * nd + 2 * n4), "head scratch %zu floats < %lld", tmp_floats,
                 static_cast<long long>(2 * nd + 2 * n4));
  const B4rParams w = b4r_params(const_cast<float*>(w_flat), *shape);
  return b4r_head_fwd(w, static_cast<int>(n), shape->dim, rows, tmp, tmp + nd, out, tmp + 2 * nd, tmp + 2 * nd + n4,
                      static_cast<hipStream_t>(stream));
}
