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
// probabilities.  The GEMM is the grouped exact-fp32 MFMA GEMM of ncf.hip.  Prep, embed, LayerNorm, the feed-forward
// GEMM groups, the loss and the attention's MFMA / tile helpers are shared with TiSASRec: csrc/seqrec.hpp, seqrec.hip.
#include <vector>

#include "gemm.hpp"
#include "seqrec.hpp"

namespace hiprec {

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

// ---- causal attention per (sequence, head) ----------------------------------------------------------------------------
constexpr int kSasQT = 32;                 // query (or key) rows a block owns
constexpr int kSasSLd = kSeqMaxLen + 4;    // leading dimension of the score rows in LDS

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
  load_tile<HD>(&Qs[0][0], base, ld, q0, kSasQT, T, scale);
  const int n_keys = min(T, q0 + kSasQT);
  const int n_chunks = (n_keys + 63) / 64;
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * 64;
    __syncthreads();
    load_tile<HD>(&Ks[0][0], base + D, ld, j0, 64, n_keys, 1.f);
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
  for (int rr = 0; rr < kSasQT / kWavesPerBlock; ++rr) {
    const int row = wave * (kSasQT / kWavesPerBlock) + rr, i = q0 + row;
    if (i >= T) {                       // a row past the sequence: finite zeros for the product below
      for (int j = lane; j < width; j += 64) S[row][j] = 0.f;
      continue;
    }
    float mx = -INFINITY;
    for (int j = lane; j <= i; j += 64) mx = fmaxf(mx, S[row][j]);
    mx = wave_max(mx);
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
  f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * 64;
    __syncthreads();
    load_tile<HD>(&Ks[0][0], base + 2 * D, ld, j0, 64, n_keys, 1.f);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = wave + kWavesPerBlock * u;
      if (t < kTiles) {
        const int rt = t / kColTiles, ct = t - rt * kColTiles;
        acc[u] = mma16(acc[u], &S[rt * 16][j0], kSasSLd, 1, &Ks[0][ct * 16], HD + 1, 1, 64);
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
  load_tile<HD>(&Qs[0][0], base, ld, q0, kSasQT, T, scale);
  load_tile<HD>(&Gs[0][0], g_base, D, q0, kSasQT, T, 1.f);
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
  f32x4 acc_q[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * 64;
    __syncthreads();
    load_tile<HD>(&Ks[0][0], base + D, ld, j0, 64, n_keys, 1.f);
    load_tile<HD>(&Vs[0][0], base + 2 * D, ld, j0, 64, n_keys, 1.f);
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
  load_tile<HD>(&Ks[0][0], base + D, ld, j0, kSasQT, T, 1.f);
  load_tile<HD>(&Vs[0][0], base + 2 * D, ld, j0, kSasQT, T, 1.f);
  constexpr int kColTiles = HD / 16, kTiles = 2 * kColTiles;
  f32x4 acc_k[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  f32x4 acc_v[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int i0 = j0; i0 < T; i0 += 32) {
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
  w.aux = take(kSeqAux);
  w.cs = take(2 * colsum_ws_floats(static_cast<int>(M), 3 * s.dim));
  w.floats = c - base;
  return w;
}

static int sas_check_shape(const hiprec_sasrec_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  return seq_check_shape("SASRec", s->n_items, s->n_blocks, s->heads, s->maxlen, s->dim);
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

  if (train)
    if (int rc = seq_prep(w.item_emb, g_flat, n_table, pos, M, l2, a.aux, st)) return rc;
  if (int rc = seq_embed(w.item_emb, w.pos_emb, seq, M, T, D, s.n_items, sqrt_d, kp(0), ks, a.x[0], stats, st)) return rc;
  if (int rc = seq_ln_fwd(a.x[0], nullptr, nullptr, nullptr, w.ln_a_w[0], w.ln_a_b[0], a.qn[0], a.mean_a[0],
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
    if (int rc = by_head_width(hd, [&](auto hw) {
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
    if (int rc = seq_ln_fwd(a.qn[k], a.mha[k], nullptr, nullptr, w.ln_f_w[k], w.ln_f_b[k], a.f[k], a.mean_f[k],
                            a.rstd_f[k], M, D, st))
      return rc;
    if (int rc = seq_ffn_fwd(Mi, D, a.f[k], w.c1_w[k], w.c1_b[k], w.c2_w[k], w.c2_b[k], kp(2 + 3 * k), kp(3 + 3 * k), ks,
                             a.h1[k], a.z, st))
      return rc;
    const bool last = k + 1 == nb;
    if (int rc = seq_ln_fwd(a.f[k], a.z, seq, last ? a.x_last : a.x[k + 1], last ? w.last_w : w.ln_a_w[k + 1],
                            last ? w.last_b : w.ln_a_b[k + 1], last ? (train ? a.feats : feats_out) : a.qn[k + 1],
                            last ? a.mean_l : a.mean_a[k + 1], last ? a.rstd_l : a.rstd_a[k + 1], M, D, st))
      return rc;
  }
  if (!train) return 0;

  const SasParams g = sas_params(g_flat, s);
  float *T1 = a.t[0], *T2 = a.t[1], *T3 = a.t[2], *T4 = a.t[3], *T5 = a.t[4], *T6 = a.t[5], *T7 = a.t[6], *T8 = a.t[7];
  if (int rc = seq_loss(a.feats, w.item_emb, pos, neg, M, D, s.n_items, a.aux, l2, T1, g.item_emb, scratch, stats, st))
    return rc;
  // T2: gradient of a block's masked output; T3: the same through that block's dropout2 keep bytes
  if (int rc = seq_ln_bwd(T1, nullptr, a.x_last, nullptr, w.last_w, a.mean_l, a.rstd_l, nullptr, nullptr, seq,
                          kp(3 * nb), ks, T2, T3, T6, T8, g.last_w, g.last_b, a.cs, M, D, st))
    return rc;
  for (int k = nb - 1; k >= 0; --k) {
    if (int rc = seq_ffn_bwd(Mi, D, kp(3 + 3 * k) ? T3 : T2, a.f[k], a.h1[k], w.c1_w[k], w.c2_w[k], kp(2 + 3 * k), ks, T4,
                             T5, g.c1_w[k], g.c1_b[k], g.c2_w[k], g.c2_b[k], a.cs, st))
      return rc;
    // LN_f: dy = d(FFN input) + the residual's gradient; T7 = gradient of Q + mha
    if (int rc = seq_ln_bwd(T5, T2, a.qn[k], a.mha[k], w.ln_f_w[k], a.mean_f[k], a.rstd_f[k], nullptr, nullptr, nullptr,
                            nullptr, ks, T7, nullptr, T6, T8, g.ln_f_w[k], g.ln_f_b[k], a.cs, M, D, st))
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
    if (int rc = by_head_width(hd, [&](auto hw) {
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
    if (int rc = seq_ln_bwd(T4, T7, a.x[k], nullptr, w.ln_a_w[k], a.mean_a[k], a.rstd_a[k], T5, nullptr,
                            k > 0 ? seq : nullptr, k > 0 ? kp(3 * k) : nullptr, ks, T2, T3, T6, T8, g.ln_a_w[k],
                            g.ln_a_b[k], a.cs, M, D, st))
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
  if (int rc = seq_check_call(w_flat, g_flat, seq, pos, neg, batch, seq_len, shape->maxlen, shape->heads, feats_out,
                              stats, scratch, scratch_bytes, workspace, workspace_bytes,
                              hiprec_sasrec_workspace_bytes(shape, batch, seq_len)))
    return rc;
  return sas_run(*shape, const_cast<float*>(w_flat), g_flat, seq, pos, neg, batch, seq_len, l2_emb, keep, keep_scale,
                 feats_out, stats, static_cast<Scratch*>(scratch), static_cast<float*>(workspace),
                 static_cast<hipStream_t>(stream));
}
