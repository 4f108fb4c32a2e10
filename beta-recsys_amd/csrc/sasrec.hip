// SASRec (beta_rec/models/sasrec.py): zero_grad + forward + loss + backward of SASRecEngine.train_single_batch as a
// fixed sequence of launches, no host sync.  Activations are [M = B * T, D] row-major, row m = b * T + t.
//
//   prep (2 launches)   count of pos != 0; ||item_emb||_2 in two fixed-order levels and its dense gradient
//   embed               x0 = (E[seq] * sqrt(D) + P[t]) * keep * (seq != 0)
//   per block           LN_a -> in_proj (grouped GEMM: Q rows from LN_a(x), K / V rows from x) -> causal attention per
//                       (sequence, head) on the fp32 MFMA, probabilities never leave LDS -> out_proj (GEMM) ->
//                       LN_f(Q + mha) -> conv1 + dropout + ReLU (GEMM epilogue) -> conv2 + dropout (GEMM epilogue);
//                       the next LayerNorm adds the residual and applies the timeline mask on its way in
//   loss                last LayerNorm, two dot products per token, BCE-with-logits over pos != 0, d feats, row atomics
//   backward            the same chain in reverse: LayerNorm backward (dx; dy * xhat and dy go through the fixed-order
//                       column sums of gemm.hpp), dgrad / wgrad / bias GEMM groups, attention backward in two kernels
//                       that recompute the probabilities from the saved log-sum-exp (one owns a query tile and writes
//                       dQ, the other owns a key tile and writes dK and dV: no atomics), embed backward
//
// Saved per block: x, LN_a(x), the projected [M, 3D] q | k | v, the attention output, mha, LN_f's output, the FFN's
// hidden activation, two (mean, rstd) pairs and the log-sum-exp per (sequence, head, query).  Recomputed: scores and
// probabilities.  The GEMM is the grouped exact-fp32 MFMA GEMM of ncf.hip.
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "gemm.hpp"

namespace hiprec {

using sas_f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kSasMaxDim = 128;
constexpr int kSasMaxLen = 256;
constexpr int kSasNormParts = 256;   // first-level partial sums of ||item_emb||^2
constexpr int kSasAux = 2 + kSasNormParts;   // [0] count of pos != 0, [1] ||item_emb||, [2..] the partial sums

// ---- prep: count(pos != 0) and the first level of sum(W^2) ------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void sas_prep_kernel(const float* __restrict__ W, int64_t n_w,
                                                          const int64_t* __restrict__ pos, int64_t M, int with_norm,
                                                          float* __restrict__ aux) {
  __shared__ float s_red[kBlock];
  float s = 0.f;
  if (with_norm) {
    const int64_t per = (n_w + kSasNormParts - 1) / kSasNormParts;
    const int64_t lo = per * blockIdx.x, hi = min(n_w, lo + per);
    for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) s += W[i] * W[i];
  }
  s_red[threadIdx.x] = s;
  __syncthreads();
  for (int r = kBlock / 2; r > 0; r >>= 1) {
    if (static_cast<int>(threadIdx.x) < r) s_red[threadIdx.x] += s_red[threadIdx.x + r];
    __syncthreads();
  }
  if (threadIdx.x == 0) aux[2 + blockIdx.x] = s_red[0];
  if (blockIdx.x != 0) return;
  __syncthreads();
  float c = 0.f;                                   // integers up to 2^24 are exact in fp32; M < 2^24 is required
  for (int64_t m = threadIdx.x; m < M; m += kBlock) c += pos[m] != 0 ? 1.f : 0.f;
  s_red[threadIdx.x] = c;
  __syncthreads();
  for (int r = kBlock / 2; r > 0; r >>= 1) {
    if (static_cast<int>(threadIdx.x) < r) s_red[threadIdx.x] += s_red[threadIdx.x + r];
    __syncthreads();
  }
  if (threadIdx.x == 0) aux[0] = s_red[0];
}

// second level, in a fixed order; g += l2 * W / ||W|| (0 where ||W|| == 0, as torch.norm's backward gives)
__global__ __launch_bounds__(kBlock) void sas_norm_grad_kernel(const float* __restrict__ W, float* __restrict__ g,
                                                               int64_t n_w, float l2, float* __restrict__ aux) {
  __shared__ float s_red[kBlock];
  s_red[threadIdx.x] = aux[2 + threadIdx.x];
  __syncthreads();
  for (int r = kBlock / 2; r > 0; r >>= 1) {
    if (static_cast<int>(threadIdx.x) < r) s_red[threadIdx.x] += s_red[threadIdx.x + r];
    __syncthreads();
  }
  const float norm = sqrtf(s_red[0]);
  const float coef = norm > 0.f ? l2 / norm : 0.f;
  if (blockIdx.x == 0 && threadIdx.x == 0) aux[1] = norm;
  if (g == nullptr) return;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n_w; i += stride) g[i] += coef * W[i];
}

// ---- embed ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void sas_embed_kernel(const float* __restrict__ E, const float* __restrict__ P,
                                                           const int64_t* __restrict__ seq, int64_t M, int T, int D,
                                                           int64_t n_items, float sqrt_d,
                                                           const uint8_t* __restrict__ keep, float ks,
                                                           float* __restrict__ x, hiprec_stats* stats) {
  const int64_t n = M * D, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t m = i / D;
    const int d = static_cast<int>(i - m * D);
    const int64_t id = seq[m];
    float v = 0.f;
    if (id < 0 || id > n_items) {
      if (d == 0) atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
    } else if (id != 0) {
      v = E[id * D + d] * sqrt_d + P[static_cast<int64_t>(m % T) * D + d];
      if (keep) v = keep[i] ? v * ks : 0.f;
    }
    x[i] = v;
  }
}

// d item_emb[seq] += dx * keep * sqrt(D) (row atomics, id 0 skipped), d pos_emb[t] += sum_b dx * keep: one thread per
// (t, d) walks the batch in order, so the positional gradient is the same from run to run
__global__ __launch_bounds__(kBlock) void sas_embed_bwd_kernel(const float* __restrict__ dx,
                                                               const int64_t* __restrict__ seq, int64_t B, int T, int D,
                                                               int64_t n_items, float sqrt_d,
                                                               const uint8_t* __restrict__ keep, float ks,
                                                               float* __restrict__ g_item, float* __restrict__ g_pos) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= T * D) return;
  const int t = e / D, d = e - t * D;
  float acc = 0.f;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t m = b * T + t;
    const int64_t id = seq[m];
    if (id <= 0 || id > n_items) continue;
    float gv = dx[m * D + d];
    if (keep) gv = keep[m * D + d] ? gv * ks : 0.f;
    atomic_add_f32(g_item + id * D + d, gv * sqrt_d);
    acc += gv;
  }
  g_pos[e] += acc;
}

// ---- LayerNorm (eps 1e-8, biased variance), one wave per row, D <= 128 -----------------------------------------------
// x = (a + b) * (seq != 0); xsum (optional) receives x; y = (x - mean) * rstd * gamma + beta
__global__ __launch_bounds__(kBlock) void sas_ln_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            const int64_t* __restrict__ seq, float* __restrict__ xsum,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ y,
                                                            float* __restrict__ mean, float* __restrict__ rstd,
                                                            int64_t M, int D) {
  const int lane = lane_id();
  const float inv_d = 1.f / static_cast<float>(D);
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); row < M;
       row += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const bool live = !seq || seq[row] != 0;
    float v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      float t = 0.f;
      if (d < D && live) {
        t = a[row * D + d];
        if (b) t += b[row * D + d];
      }
      v[h] = t;
      if (xsum && d < D) xsum[row * D + d] = t;
    }
    const float mu = wave_sum(v[0] + v[1]) * inv_d;
    const float c0 = lane < D ? v[0] - mu : 0.f, c1 = lane + 64 < D ? v[1] - mu : 0.f;
    const float var = wave_sum(c0 * c0 + c1 * c1) * inv_d;
    const float r = 1.0f / sqrtf(var + 1e-8f);
    if (lane < D) y[row * D + lane] = c0 * r * gamma[lane] + beta[lane];
    if (lane + 64 < D) y[row * D + lane + 64] = c1 * r * gamma[lane + 64] + beta[lane + 64];
    if (lane == 0) {
      mean[row] = mu;
      rstd[row] = r;
    }
  }
}

// dy = dy_a + dy_b; x = a + b; dx = (rstd * (g - mean(g) - xhat * mean(g * xhat)) + dx_extra) * (seq != 0) with
// g = dy * gamma; dx_keep (optional) = dx through the keep bytes; dyx = dy * xhat and dyt = dy feed the column sums
__global__ __launch_bounds__(kBlock) void sas_ln_bwd_kernel(
    const float* __restrict__ dy_a, const float* __restrict__ dy_b, const float* __restrict__ a,
    const float* __restrict__ b, const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ dx_extra, const int64_t* __restrict__ seq,
    const uint8_t* __restrict__ keep, float ks, float* __restrict__ dx, float* __restrict__ dx_keep,
    float* __restrict__ dyx, float* __restrict__ dyt, int64_t M, int D) {
  const int lane = lane_id();
  const float inv_d = 1.f / static_cast<float>(D);
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); row < M;
       row += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const bool live = !seq || seq[row] != 0;
    const float mu = mean[row], r = rstd[row];
    float xh[2], gg[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      xh[h] = 0.f;
      gg[h] = 0.f;
      if (d < D) {
        const int64_t i = row * D + d;
        float x = a[i];
        if (b) x += b[i];
        float dy = dy_a[i];
        if (dy_b) dy += dy_b[i];
        xh[h] = (x - mu) * r;
        gg[h] = dy * gamma[d];
        dyx[i] = dy * xh[h];
        if (dyt) dyt[i] = dy;
      }
    }
    const float m1 = wave_sum(gg[0] + gg[1]) * inv_d;
    const float m2 = wave_sum(gg[0] * xh[0] + gg[1] * xh[1]) * inv_d;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      if (d < D) {
        const int64_t i = row * D + d;
        float v = r * (gg[h] - m1 - xh[h] * m2);
        if (dx_extra) v += dx_extra[i];
        if (!live) v = 0.f;
        dx[i] = v;
        if (dx_keep) dx_keep[i] = keep[i] ? v * ks : 0.f;
      }
    }
  }
}

// ---- causal attention per (sequence, head) ----------------------------------------------------------------------------
// v_mfma_f32_16x16x4_f32 on operands in LDS: element (i, k) of A at A[i * sai + k * sak], element (k, j) of B at
// B[k * sbk + j * sbj]; lane l feeds A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15]; the result has
// col = lane & 15, row = 4 * (lane >> 4) + reg.
__device__ __forceinline__ sas_f32x4 sas_mma16(sas_f32x4 acc, const float* A, int sai, int sak, const float* B, int sbk,
                                               int sbj, int K) {
  const int l = lane_id();
  const float* ap = A + (l & 15) * sai + (l >> 4) * sak;
  const float* bp = B + (l >> 4) * sbk + (l & 15) * sbj;
  for (int k = 0; k < K; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k * sak], bp[k * sbk], acc, 0, 0, 0);
  return acc;
}

constexpr int kSasQT = 32;                 // query (or key) rows a block owns
constexpr int kSasSLd = kSasMaxLen + 4;    // leading dimension of the score rows in LDS

// rows [r0, r0 + rows) x HD columns starting at src (leading dimension ld) into dst[rows][HD + 1]; rows >= limit are 0
template <int HD>
__device__ __forceinline__ void sas_load_tile(float (*dst)[HD + 1], const float* __restrict__ src, int64_t ld, int r0,
                                              int rows, int limit, float scale) {
  for (int e = threadIdx.x; e < rows * HD; e += kBlock) {
    const int r = e / HD, c = e - r * HD;
    dst[r][c] = (r0 + r < limit) ? src[static_cast<int64_t>(r0 + r) * ld + c] * scale : 0.f;
  }
}

__device__ __forceinline__ float sas_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// grid (B * H, ceil(T / 32)).  qkv [M, 3D]: q | k | v.  keep (optional) [B * H, T, T] bytes on the probabilities.
template <int HD>
__global__ __launch_bounds__(kBlock) void sas_attn_fwd_kernel(const float* __restrict__ qkv, int T, int H, int D,
                                                              const uint8_t* __restrict__ keep, float ks,
                                                              float* __restrict__ O, float* __restrict__ lse) {
  __shared__ float Qs[kSasQT][HD + 1];
  __shared__ float Ks[64][HD + 1];
  __shared__ float S[kSasQT][kSasSLd];
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int q0 = blockIdx.y * kSasQT;
  const int lane = lane_id(), wave = wave_in_block();
  const int64_t ld = 3 * D;
  const float* base = qkv + static_cast<int64_t>(b) * T * ld + h * HD;
  const float scale = 1.0f / sqrtf(static_cast<float>(HD));
  sas_load_tile<HD>(Qs, base, ld, q0, kSasQT, T, scale);
  const int n_keys = min(T, q0 + kSasQT);
  const int n_chunks = (n_keys + 63) / 64;
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * 64;
    __syncthreads();
    sas_load_tile<HD>(Ks, base + D, ld, j0, 64, n_keys, 1.f);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int tile = wave * 2 + u, rt = tile >> 2, ct = tile & 3;
      sas_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = sas_mma16(acc, &Qs[rt * 16][0], HD + 1, 1, &Ks[ct * 16][0], 1, HD + 1, HD);
#pragma unroll
      for (int r = 0; r < 4; ++r) S[rt * 16 + 4 * (lane >> 4) + r][j0 + ct * 16 + (lane & 15)] = acc[r];
    }
  }
  __syncthreads();
  const int width = n_chunks * 64;
  for (int rr = 0; rr < kSasQT / kWavesPerBlock; ++rr) {
    const int row = wave * (kSasQT / kWavesPerBlock) + rr, i = q0 + row;
    if (i >= T) {                       // a row past the sequence: finite zeros for the product below
      for (int j = lane; j < width; j += 64) S[row][j] = 0.f;
      continue;
    }
    float mx = -INFINITY;
    for (int j = lane; j <= i; j += 64) mx = fmaxf(mx, S[row][j]);
    mx = sas_wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j <= i; j += 64) {
      const float e = expf(S[row][j] - mx);
      S[row][j] = e;
      sum += e;
    }
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
    const uint8_t* kp = keep ? keep + (static_cast<int64_t>(bh) * T + i) * T : nullptr;
    for (int j = lane; j < width; j += 64) {
      float p = 0.f;
      if (j <= i) {
        p = S[row][j] * inv;
        if (kp) p = kp[j] ? p * ks : 0.f;
      }
      S[row][j] = p;
    }
    if (lane == 0) lse[static_cast<int64_t>(bh) * T + i] = mx + logf(sum);
  }
  constexpr int kColTiles = HD / 16, kTiles = 2 * kColTiles;
  sas_f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * 64;
    __syncthreads();
    sas_load_tile<HD>(Ks, base + 2 * D, ld, j0, 64, n_keys, 1.f);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = wave + kWavesPerBlock * u;
      if (t < kTiles) {
        const int rt = t / kColTiles, ct = t - rt * kColTiles;
        acc[u] = sas_mma16(acc[u], &S[rt * 16][j0], kSasSLd, 1, &Ks[0][ct * 16], HD + 1, 1, 64);
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

// backward, query side: a block owns 32 queries and walks the keys 0 .. i in chunks of 64.  P = exp(S - lse),
// dP = dO V^T through the keep bytes, dS = P * (dP - delta) with delta = rowsum(dO * O); dQ = dS K / sqrt(hd).
// Writes delta [B * H, T] for the key-side kernel and the q third of dqkv [M, 3D].
template <int HD>
__global__ __launch_bounds__(kBlock) void sas_attn_bwd_q_kernel(const float* __restrict__ qkv,
                                                                const float* __restrict__ dO,
                                                                const float* __restrict__ O,
                                                                const float* __restrict__ lse, int T, int H, int D,
                                                                const uint8_t* __restrict__ keep, float ks,
                                                                float* __restrict__ delta, float* __restrict__ dqkv) {
  __shared__ float Qs[kSasQT][HD + 1];
  __shared__ float Gs[kSasQT][HD + 1];
  __shared__ float Ks[64][HD + 1];
  __shared__ float Vs[64][HD + 1];
  __shared__ float DS[kSasQT][65];
  __shared__ float s_lse[kSasQT], s_delta[kSasQT];
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int q0 = blockIdx.y * kSasQT;
  const int lane = lane_id(), wave = wave_in_block();
  const int64_t ld = 3 * D;
  const float* base = qkv + static_cast<int64_t>(b) * T * ld + h * HD;
  const float* g_base = dO + static_cast<int64_t>(b) * T * D + h * HD;
  const float* o_base = O + static_cast<int64_t>(b) * T * D + h * HD;
  const float scale = 1.0f / sqrtf(static_cast<float>(HD));
  sas_load_tile<HD>(Qs, base, ld, q0, kSasQT, T, scale);
  sas_load_tile<HD>(Gs, g_base, D, q0, kSasQT, T, 1.f);
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
  const int n_keys = min(T, q0 + kSasQT);
  const int n_chunks = (n_keys + 63) / 64;
  constexpr int kColTiles = HD / 16, kTiles = 2 * kColTiles;
  sas_f32x4 acc_q[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * 64;
    __syncthreads();
    sas_load_tile<HD>(Ks, base + D, ld, j0, 64, n_keys, 1.f);
    sas_load_tile<HD>(Vs, base + 2 * D, ld, j0, 64, n_keys, 1.f);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int tile = wave * 2 + u, rt = tile >> 2, ct = tile & 3;
      sas_f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
      s = sas_mma16(s, &Qs[rt * 16][0], HD + 1, 1, &Ks[ct * 16][0], 1, HD + 1, HD);
      dp = sas_mma16(dp, &Gs[rt * 16][0], HD + 1, 1, &Vs[ct * 16][0], 1, HD + 1, HD);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rt * 16 + 4 * (lane >> 4) + r, col = ct * 16 + (lane & 15);
        const int i = q0 + row, j = j0 + col;
        float ds = 0.f;
        if (i < T && j <= i) {
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
        acc_q[u] = sas_mma16(acc_q[u], &DS[rt * 16][0], 65, 1, &Ks[0][ct * 16], HD + 1, 1, 64);
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

// backward, key side: a block owns 32 keys and walks the queries j .. T - 1 in chunks of 32.  S^T = K Q^T,
// dK = dS^T (q / sqrt(hd)), dV = (P through the keep bytes)^T dO, each summed in a fixed order: no atomics.
template <int HD>
__global__ __launch_bounds__(kBlock) void sas_attn_bwd_kv_kernel(const float* __restrict__ qkv,
                                                                 const float* __restrict__ dO,
                                                                 const float* __restrict__ lse,
                                                                 const float* __restrict__ delta, int T, int H, int D,
                                                                 const uint8_t* __restrict__ keep, float ks,
                                                                 float* __restrict__ dqkv) {
  __shared__ float Ks[kSasQT][HD + 1];
  __shared__ float Vs[kSasQT][HD + 1];
  __shared__ float Qc[32][HD + 1];
  __shared__ float Gc[32][HD + 1];
  __shared__ float PT[kSasQT][33];
  __shared__ float DST[kSasQT][33];
  __shared__ float s_lse[32], s_delta[32];
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int j0 = blockIdx.y * kSasQT;
  const int lane = lane_id(), wave = wave_in_block();
  const int64_t ld = 3 * D;
  const float* base = qkv + static_cast<int64_t>(b) * T * ld + h * HD;
  const float* g_base = dO + static_cast<int64_t>(b) * T * D + h * HD;
  const float scale = 1.0f / sqrtf(static_cast<float>(HD));
  sas_load_tile<HD>(Ks, base + D, ld, j0, kSasQT, T, 1.f);
  sas_load_tile<HD>(Vs, base + 2 * D, ld, j0, kSasQT, T, 1.f);
  constexpr int kColTiles = HD / 16, kTiles = 2 * kColTiles;
  sas_f32x4 acc_k[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  sas_f32x4 acc_v[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int i0 = j0; i0 < T; i0 += 32) {
    __syncthreads();
    sas_load_tile<HD>(Qc, base, ld, i0, 32, T, scale);
    sas_load_tile<HD>(Gc, g_base, D, i0, 32, T, 1.f);
    if (threadIdx.x < 32) {
      const int i = i0 + threadIdx.x;
      s_lse[threadIdx.x] = i < T ? lse[static_cast<int64_t>(bh) * T + i] : 0.f;
      s_delta[threadIdx.x] = i < T ? delta[static_cast<int64_t>(bh) * T + i] : 0.f;
    }
    __syncthreads();
    {
      const int rt = wave >> 1, ct = wave & 1;       // 2 x 2 tiles of the [32 keys, 32 queries] block, one per wave
      sas_f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
      s = sas_mma16(s, &Ks[rt * 16][0], HD + 1, 1, &Qc[ct * 16][0], 1, HD + 1, HD);
      dp = sas_mma16(dp, &Vs[rt * 16][0], HD + 1, 1, &Gc[ct * 16][0], 1, HD + 1, HD);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rt * 16 + 4 * (lane >> 4) + r, col = ct * 16 + (lane & 15);
        const int j = j0 + row, i = i0 + col;
        float ds = 0.f, pd = 0.f;
        if (i < T && j <= i) {
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
        acc_k[u] = sas_mma16(acc_k[u], &DST[rt * 16][0], 33, 1, &Qc[0][ct * 16], HD + 1, 1, 32);
        acc_v[u] = sas_mma16(acc_v[u], &PT[rt * 16][0], 33, 1, &Gc[0][ct * 16], HD + 1, 1, 32);
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

// ---- loss: BCE-with-logits over the tokens with pos != 0, d feats, row atomics into d item_emb -----------------------
__global__ __launch_bounds__(kBlock) void sas_loss_kernel(const float* __restrict__ feats, const float* __restrict__ E,
                                                          const int64_t* __restrict__ pos,
                                                          const int64_t* __restrict__ neg, int64_t M, int D,
                                                          int64_t n_items, const float* __restrict__ aux, float l2,
                                                          float* __restrict__ dfeats, float* __restrict__ g_item,
                                                          Scratch* scratch, hiprec_stats* stats) {
  __shared__ float s_loss[kWavesPerBlock];
  const int lane = lane_id(), wave = wave_in_block();
  const float inv = 1.0f / aux[0];
  float loss = 0.f;
  for (int64_t m = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave; m < M;
       m += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const int64_t p = pos[m], n = neg[m];
    const bool ok = p >= 0 && p <= n_items && n >= 0 && n <= n_items;
    if (!ok && lane == 0) atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
    if (!ok || p == 0) {
      if (lane < D) dfeats[m * D + lane] = 0.f;
      if (lane + 64 < D) dfeats[m * D + lane + 64] = 0.f;
      continue;
    }
    float f[2], ep[2], en[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      f[h] = d < D ? feats[m * D + d] : 0.f;
      ep[h] = d < D ? E[p * D + d] : 0.f;
      en[h] = d < D ? E[n * D + d] : 0.f;
    }
    const float pl = wave_sum(f[0] * ep[0] + f[1] * ep[1]);
    const float nl = wave_sum(f[0] * en[0] + f[1] * en[1]);
    float sig_neg_pl, sig_nl;
    loss += neg_logsigmoid(pl, &sig_neg_pl);      // BCEWithLogits(x, 1) = softplus(-x)
    loss += neg_logsigmoid(-nl, &sig_nl);         // BCEWithLogits(x, 0) = softplus(x)
    const float dpl = -sig_neg_pl * inv, dnl = sig_nl * inv;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      if (d < D) {
        dfeats[m * D + d] = dpl * ep[h] + dnl * en[h];
        atomic_add_f32(g_item + p * D + d, dpl * f[h]);
        if (n != 0) atomic_add_f32(g_item + n * D + d, dnl * f[h]);
      }
    }
  }
  if (lane == 0) s_loss[wave] = loss;
  lds_barrier();
  if (threadIdx.x == 0) {
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < kWavesPerBlock; ++i) l += s_loss[i];
    l *= inv;
    if (blockIdx.x == 0) {
      if (l2 != 0.f) l += l2 * aux[1];
      scratch->n_partials = gridDim.x;
      advance_step(stats);
    }
    scratch->partials[blockIdx.x] = make_float4(l, 0.f, 0.f, 0.f);
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------
struct SasParams {      // pointers into a flat buffer laid out in state_dict() order
  float *item_emb, *pos_emb, *last_w, *last_b;
  std::vector<float*> ln_a_w, ln_a_b, in_w, in_b, out_w, out_b, ln_f_w, ln_f_b, c1_w, c1_b, c2_w, c2_b;
};

static int64_t sas_n_params(const hiprec_sasrec_shape& s) {
  const int64_t D = s.dim;
  return (s.n_items + 1) * D + static_cast<int64_t>(s.maxlen) * D + s.n_blocks * (6 * D * D + 10 * D) + 2 * D;
}

static SasParams sas_params(float* base, const hiprec_sasrec_shape& s) {
  SasParams p;
  const int64_t D = s.dim;
  const int nb = s.n_blocks;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += n; return r; };
  p.item_emb = take((s.n_items + 1) * D);
  p.pos_emb = take(static_cast<int64_t>(s.maxlen) * D);
  for (int k = 0; k < nb; ++k) { p.ln_a_w.push_back(take(D)); p.ln_a_b.push_back(take(D)); }
  for (int k = 0; k < nb; ++k) {
    p.in_w.push_back(take(3 * D * D)); p.in_b.push_back(take(3 * D));
    p.out_w.push_back(take(D * D)); p.out_b.push_back(take(D));
  }
  for (int k = 0; k < nb; ++k) { p.ln_f_w.push_back(take(D)); p.ln_f_b.push_back(take(D)); }
  for (int k = 0; k < nb; ++k) {
    p.c1_w.push_back(take(D * D)); p.c1_b.push_back(take(D));
    p.c2_w.push_back(take(D * D)); p.c2_b.push_back(take(D));
  }
  p.last_w = take(D);
  p.last_b = take(D);
  return p;
}

struct SasWorkspace {
  std::vector<float*> x, qn, qkv, o, mha, f, h1, mean_a, rstd_a, mean_f, rstd_f, lse, delta;
  float *x_last, *feats, *mean_l, *rstd_l, *z, *t[8], *dqkv, *aux, *cs;
  int64_t floats;
};

static SasWorkspace sas_carve(float* base, const hiprec_sasrec_shape& s, int64_t B, int T) {
  SasWorkspace w;
  const int64_t M = B * T, MD = M * s.dim, MH = M * s.heads;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += (n + 3) / 4 * 4; return r; };
  for (int k = 0; k < s.n_blocks; ++k) {
    w.x.push_back(take(MD)); w.qn.push_back(take(MD)); w.qkv.push_back(take(3 * MD)); w.o.push_back(take(MD));
    w.mha.push_back(take(MD)); w.f.push_back(take(MD)); w.h1.push_back(take(MD));
    w.mean_a.push_back(take(M)); w.rstd_a.push_back(take(M)); w.mean_f.push_back(take(M)); w.rstd_f.push_back(take(M));
    w.lse.push_back(take(MH)); w.delta.push_back(take(MH));
  }
  w.x_last = take(MD); w.feats = take(MD); w.mean_l = take(M); w.rstd_l = take(M); w.z = take(MD);
  for (int i = 0; i < 8; ++i) w.t[i] = take(MD);
  w.dqkv = take(3 * MD);
  w.aux = take(kSasAux);
  w.cs = take(2 * colsum_ws_floats(static_cast<int>(M), 3 * s.dim));
  w.floats = c - base;
  return w;
}

static int sas_check_shape(const hiprec_sasrec_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  HIPREC_REQUIRE(s->n_items > 0 && s->n_blocks >= 1 && s->heads >= 1 && s->maxlen >= 1, "bad SASRec shape");
  HIPREC_REQUIRE(s->dim <= kSasMaxDim && s->dim % s->heads == 0, "SASRec needs emb_dim <= %d and a multiple of num_heads",
                 kSasMaxDim);
  const int hd = s->dim / s->heads;
  HIPREC_REQUIRE(hd == 16 || hd == 32 || hd == 64, "SASRec needs a head width of 16, 32 or 64 (got %d)", hd);
  HIPREC_REQUIRE(s->maxlen <= kSasMaxLen, "SASRec needs maxlen <= %d (got %d)", kSasMaxLen, s->maxlen);
  return 0;
}

static int sas_ln_fwd(const float* a, const float* b, const int64_t* seq, float* xsum, const float* gamma,
                      const float* beta, float* y, float* mean, float* rstd, int64_t M, int D, hipStream_t st) {
  sas_ln_fwd_kernel<<<grid_for_waves(M), kBlock, 0, st>>>(a, b, seq, xsum, gamma, beta, y, mean, rstd, M, D);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// LayerNorm backward + its two column sums (d gamma from dyx, d beta from the summed dy)
static int sas_ln_bwd(const float* dy_a, const float* dy_b, const float* a, const float* b, const float* gamma,
                      const float* mean, const float* rstd, const float* dx_extra, const int64_t* seq,
                      const uint8_t* keep, float ks, float* dx, float* dx_keep, float* dyx, float* dyt, float* g_gamma,
                      float* g_beta, float* cs, int64_t M, int D, hipStream_t st) {
  sas_ln_bwd_kernel<<<grid_for_waves(M), kBlock, 0, st>>>(dy_a, dy_b, a, b, gamma, mean, rstd, dx_extra, seq, keep, ks,
                                                           dx, keep ? dx_keep : nullptr, dyx, dy_b ? dyt : nullptr, M, D);
  HIPREC_TRY(hipGetLastError());
  GemmGroup g{};
  g.n = 2;
  g.p[0] = make_colsum(dyx, static_cast<int>(M), D, D, g_gamma, cs);
  g.p[1] = make_colsum(dy_b ? dyt : dy_a, static_cast<int>(M), D, D, g_beta, cs + colsum_ws_floats(static_cast<int>(M), D));
  if (int rc = launch_group(g, st)) return rc;
  return launch_colsum_reduce(g, st);
}

template <typename F>
static int sas_by_head_width(int hd, F&& f) {
  if (hd == 16) return f(std::integral_constant<int, 16>{});
  if (hd == 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, 64>{});
}

static int sas_run(const hiprec_sasrec_shape& s, float* w_flat, float* g_flat, const int64_t* seq, const int64_t* pos,
                   const int64_t* neg, int64_t B, int T, float l2, const uint8_t* const* keep, float ks,
                   float* feats_out, hiprec_stats* stats, Scratch* scratch, float* ws_base, hipStream_t st) {
  const int D = s.dim, H = s.heads, nb = s.n_blocks, hd = D / H;
  const int64_t M = B * T;
  const int Mi = static_cast<int>(M);
  const bool train = g_flat != nullptr;
  const SasParams w = sas_params(w_flat, s);
  const SasWorkspace a = sas_carve(ws_base, s, B, T);
  const float sqrt_d = sqrtf(static_cast<float>(D));
  const int64_t n_table = (s.n_items + 1) * D;
  auto kp = [&](int i) -> const uint8_t* { return keep ? keep[i] : nullptr; };
  const dim3 attn_grid(static_cast<unsigned>(B * H), static_cast<unsigned>((T + kSasQT - 1) / kSasQT));

  if (train) {
    sas_prep_kernel<<<kSasNormParts, kBlock, 0, st>>>(w.item_emb, n_table, pos, M, l2 != 0.f, a.aux);
    HIPREC_TRY(hipGetLastError());
    if (l2 != 0.f) {
      sas_norm_grad_kernel<<<grid_for_threads(n_table), kBlock, 0, st>>>(w.item_emb, g_flat, n_table, l2, a.aux);
      HIPREC_TRY(hipGetLastError());
    }
  }
  sas_embed_kernel<<<grid_for_threads(M * D), kBlock, 0, st>>>(w.item_emb, w.pos_emb, seq, M, T, D, s.n_items, sqrt_d,
                                                               kp(0), ks, a.x[0], stats);
  HIPREC_TRY(hipGetLastError());
  if (int rc = sas_ln_fwd(a.x[0], nullptr, nullptr, nullptr, w.ln_a_w[0], w.ln_a_b[0], a.qn[0], a.mean_a[0],
                          a.rstd_a[0], M, D, st))
    return rc;
  for (int k = 0; k < nb; ++k) {
    {
      GemmGroup g{};
      g.n = 2;
      g.p[0] = make_gemm(kNT, Mi, D, D, a.qn[k], D, w.in_w[k], D, a.qkv[k], 3 * D, w.in_b[k], 0, nullptr, 0, false);
      g.p[1] = make_gemm(kNT, Mi, 2 * D, D, a.x[k], D, w.in_w[k] + D * D, D, a.qkv[k] + D, 3 * D, w.in_b[k] + D, 0,
                         nullptr, 0, false);
      if (int rc = launch_group(g, st)) return rc;
    }
    if (int rc = sas_by_head_width(hd, [&](auto hw) {
          sas_attn_fwd_kernel<decltype(hw)::value><<<attn_grid, kBlock, 0, st>>>(a.qkv[k], T, H, D, kp(1 + 3 * k), ks,
                                                                                 a.o[k], a.lse[k]);
          HIPREC_TRY(hipGetLastError());
          return 0;
        }))
      return rc;
    {
      GemmGroup g{};
      g.n = 1;
      g.p[0] = make_gemm(kNT, Mi, D, D, a.o[k], D, w.out_w[k], D, a.mha[k], D, w.out_b[k], 0, nullptr, 0, false);
      if (int rc = launch_group(g, st)) return rc;
    }
    if (int rc = sas_ln_fwd(a.qn[k], a.mha[k], nullptr, nullptr, w.ln_f_w[k], w.ln_f_b[k], a.f[k], a.mean_f[k],
                            a.rstd_f[k], M, D, st))
      return rc;
    {
      GemmGroup g{};
      g.n = 1;
      g.p[0] = make_gemm(kNT, Mi, D, D, a.f[k], D, w.c1_w[k], D, a.h1[k], D, w.c1_b[k], 1, nullptr, 0, false);
      if (kp(2 + 3 * k)) { g.p[0].keep = kp(2 + 3 * k); g.p[0].ldk = D; g.p[0].keep_scale = ks; }
      if (int rc = launch_group(g, st)) return rc;
    }
    {
      GemmGroup g{};
      g.n = 1;
      g.p[0] = make_gemm(kNT, Mi, D, D, a.h1[k], D, w.c2_w[k], D, a.z, D, w.c2_b[k], 0, nullptr, 0, false);
      if (kp(3 + 3 * k)) { g.p[0].keep = kp(3 + 3 * k); g.p[0].ldk = D; g.p[0].keep_scale = ks; }
      if (int rc = launch_group(g, st)) return rc;
    }
    const bool last = k + 1 == nb;
    if (int rc = sas_ln_fwd(a.f[k], a.z, seq, last ? a.x_last : a.x[k + 1], last ? w.last_w : w.ln_a_w[k + 1],
                            last ? w.last_b : w.ln_a_b[k + 1], last ? (train ? a.feats : feats_out) : a.qn[k + 1],
                            last ? a.mean_l : a.mean_a[k + 1], last ? a.rstd_l : a.rstd_a[k + 1], M, D, st))
      return rc;
  }
  if (!train) return 0;

  const SasParams g = sas_params(g_flat, s);
  float *T1 = a.t[0], *T2 = a.t[1], *T3 = a.t[2], *T4 = a.t[3], *T5 = a.t[4], *T6 = a.t[5], *T7 = a.t[6], *T8 = a.t[7];
  sas_loss_kernel<<<grid_for_waves(M), kBlock, 0, st>>>(a.feats, w.item_emb, pos, neg, M, D, s.n_items, a.aux, l2, T1,
                                                        g.item_emb, scratch, stats);
  HIPREC_TRY(hipGetLastError());
  // T2: gradient of a block's masked output; T3: the same through that block's dropout2 keep bytes
  if (int rc = sas_ln_bwd(T1, nullptr, a.x_last, nullptr, w.last_w, a.mean_l, a.rstd_l, nullptr, seq, kp(3 * nb), ks,
                          T2, T3, T6, T8, g.last_w, g.last_b, a.cs, M, D, st))
    return rc;
  for (int k = nb - 1; k >= 0; --k) {
    const float* dz = kp(3 + 3 * k) ? T3 : T2;
    {
      GemmGroup q{};
      q.n = 3;
      q.p[0] = make_gemm(kNN, Mi, D, D, dz, D, w.c2_w[k], D, T4, D, nullptr, 0, a.h1[k], D, false);
      if (kp(2 + 3 * k)) { q.p[0].keep = kp(2 + 3 * k); q.p[0].ldk = D; q.p[0].keep_scale = ks; }
      q.p[1] = make_gemm(kTNm, D, D, Mi, dz, D, a.h1[k], D, g.c2_w[k], D, nullptr, 0, nullptr, 0, true);
      q.p[2] = make_colsum(dz, Mi, D, D, g.c2_b[k], a.cs);
      if (int rc = launch_group(q, st)) return rc;
      if (int rc = launch_colsum_reduce(q, st)) return rc;
    }
    {
      GemmGroup q{};
      q.n = 3;
      q.p[0] = make_gemm(kNN, Mi, D, D, T4, D, w.c1_w[k], D, T5, D, nullptr, 0, nullptr, 0, false);
      q.p[1] = make_gemm(kTNm, D, D, Mi, T4, D, a.f[k], D, g.c1_w[k], D, nullptr, 0, nullptr, 0, true);
      q.p[2] = make_colsum(T4, Mi, D, D, g.c1_b[k], a.cs);
      if (int rc = launch_group(q, st)) return rc;
      if (int rc = launch_colsum_reduce(q, st)) return rc;
    }
    // LN_f: dy = d(FFN input) + the residual's gradient; T7 = gradient of Q + mha
    if (int rc = sas_ln_bwd(T5, T2, a.qn[k], a.mha[k], w.ln_f_w[k], a.mean_f[k], a.rstd_f[k], nullptr, nullptr, nullptr,
                            ks, T7, nullptr, T6, T8, g.ln_f_w[k], g.ln_f_b[k], a.cs, M, D, st))
      return rc;
    {
      GemmGroup q{};
      q.n = 3;
      q.p[0] = make_gemm(kNN, Mi, D, D, T7, D, w.out_w[k], D, T1, D, nullptr, 0, nullptr, 0, false);
      q.p[1] = make_gemm(kTNm, D, D, Mi, T7, D, a.o[k], D, g.out_w[k], D, nullptr, 0, nullptr, 0, true);
      q.p[2] = make_colsum(T7, Mi, D, D, g.out_b[k], a.cs);
      if (int rc = launch_group(q, st)) return rc;
      if (int rc = launch_colsum_reduce(q, st)) return rc;
    }
    if (int rc = sas_by_head_width(hd, [&](auto hw) {
          constexpr int HD = decltype(hw)::value;
          sas_attn_bwd_q_kernel<HD><<<attn_grid, kBlock, 0, st>>>(a.qkv[k], T1, a.o[k], a.lse[k], T, H, D,
                                                                  kp(1 + 3 * k), ks, a.delta[k], a.dqkv);
          HIPREC_TRY(hipGetLastError());
          sas_attn_bwd_kv_kernel<HD><<<attn_grid, kBlock, 0, st>>>(a.qkv[k], T1, a.lse[k], a.delta[k], T, H, D,
                                                                   kp(1 + 3 * k), ks, a.dqkv);
          HIPREC_TRY(hipGetLastError());
          return 0;
        }))
      return rc;
    {
      GemmGroup q{};
      q.n = 5;
      q.p[0] = make_gemm(kNN, Mi, D, D, a.dqkv, 3 * D, w.in_w[k], D, T4, D, nullptr, 0, nullptr, 0, false);
      q.p[1] = make_gemm(kNN, Mi, D, 2 * D, a.dqkv + D, 3 * D, w.in_w[k] + D * D, D, T5, D, nullptr, 0, nullptr, 0, false);
      q.p[2] = make_gemm(kTNm, D, D, Mi, a.dqkv, 3 * D, a.qn[k], D, g.in_w[k], D, nullptr, 0, nullptr, 0, true);
      q.p[3] = make_gemm(kTNm, 2 * D, D, Mi, a.dqkv + D, 3 * D, a.x[k], D, g.in_w[k] + D * D, D, nullptr, 0, nullptr, 0,
                         true);
      q.p[4] = make_colsum(a.dqkv, Mi, 3 * D, 3 * D, g.in_b[k], a.cs);
      if (int rc = launch_group(q, st)) return rc;
      if (int rc = launch_colsum_reduce(q, st)) return rc;
    }
    // LN_a: dy = d(q projection input) + the residual's gradient (x = Q + mha); the K / V path enters x directly
    if (int rc = sas_ln_bwd(T4, T7, a.x[k], nullptr, w.ln_a_w[k], a.mean_a[k], a.rstd_a[k], T5, k > 0 ? seq : nullptr,
                            k > 0 ? kp(3 * k) : nullptr, ks, T2, T3, T6, T8, g.ln_a_w[k], g.ln_a_b[k], a.cs, M, D, st))
      return rc;
  }
  sas_embed_bwd_kernel<<<(T * D + kBlock - 1) / kBlock, kBlock, 0, st>>>(T2, seq, B, T, D, s.n_items, sqrt_d, kp(0), ks,
                                                                         g.item_emb, g.pos_emb);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_sasrec_shape_bytes(void) { return sizeof(hiprec_sasrec_shape); }

extern "C" int64_t hiprec_sasrec_param_floats(const hiprec_sasrec_shape* shape) {
  if (sas_check_shape(shape)) return -1;
  return sas_n_params(*shape);
}

extern "C" size_t hiprec_sasrec_workspace_bytes(const hiprec_sasrec_shape* shape, int64_t batch, int32_t seq_len) {
  if (sas_check_shape(shape) || batch <= 0 || seq_len <= 0) return 0;
  return sizeof(float) * static_cast<size_t>(sas_carve(nullptr, *shape, batch, seq_len).floats);
}

extern "C" int hiprec_sasrec_grad(const hiprec_sasrec_shape* shape, const float* w_flat, float* g_flat,
                                  const int64_t* seq, const int64_t* pos, const int64_t* neg, int64_t batch,
                                  int32_t seq_len, float l2_emb, const uint8_t* const* keep, float keep_scale,
                                  float* feats_out, hiprec_stats* stats, void* scratch, size_t scratch_bytes,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = sas_check_shape(shape)) return rc;
  HIPREC_REQUIRE(w_flat && seq && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(batch >= 1 && seq_len >= 1 && seq_len <= shape->maxlen, "bad batch / sequence length (maxlen %d)",
                 shape->maxlen);
  HIPREC_REQUIRE(batch * seq_len < (1ll << 24), "batch x sequence length must stay below 2^24");
  HIPREC_REQUIRE(batch * shape->heads <= 65535ll * 1024, "batch too large");
  if (g_flat) {
    HIPREC_REQUIRE(pos && neg && scratch, "training needs pos, neg and the scratch block");
    if (scratch_bytes < kScratchBytes) {
      set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
      return HIPREC_E_SCRATCH;
    }
  } else {
    HIPREC_REQUIRE(feats_out, "forward only needs a feature buffer");
  }
  const size_t need = hiprec_sasrec_workspace_bytes(shape, batch, seq_len);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  return sas_run(*shape, const_cast<float*>(w_flat), g_flat, seq, pos, neg, batch, seq_len, l2_emb, keep, keep_scale,
                 feats_out, stats, static_cast<Scratch*>(scratch), static_cast<float*>(workspace),
                 static_cast<hipStream_t>(stream));
}
