// HSTU (Zhai et al., "Actions Speak Louder than Words", ICML 2024): zero_grad + forward + loss + backward of
// HSTUEngine.train_single_batch as a fixed sequence of launches, no host sync.  Activations are [M = B * T, D] row-major,
// row m = b * T + t; N = maxlen is the config constant of the 1 / N and of the pos_w offset, T <= N the batch's length.
//
//   bucket prep         once per step: bucket[b, i, j] (a byte, j <= i) from time_seq and the host's threshold table, by
//                       integer comparisons only; shared by all heads, all blocks, forward and backward
//   per block           xn = LN(x) -> pre = xn W_uvqk (grouped GEMM) -> u | v | q | k = SiLU(pre) -> pointwise attention
//                       AV = (SiLU(q k^T + pos_w + ts_w) / N under the causal and padding masks) v -> Y = LN_noaffine(AV) * u
//                       through the keep bytes -> z = Y W_o^T + b_o (GEMM); the next LayerNorm adds the residual and
//                       applies the padding mask on its way in (seq_ln_fwd)
//   attention forward   a workgroup owns (sequence, head, 32 queries) and walks the keys in chunks of 64: q k^T on the fp32
//                       MFMA, bias + SiLU + 1 / N + masks in registers, the 32 x 64 weights through LDS into A v, whose
//                       accumulators stay in registers over all chunks.  No row statistic exists: nothing couples the keys.
//   attention backward  S is recomputed; one kernel owns a query tile (dq, and this tile's share of d pos_w by diagonal and
//                       of d ts_w by bucket, reduced in LDS by one owner thread per entry scanning in a fixed order), the
//                       other owns a key tile (dk, dv).  No atomics; the per-workgroup slabs of the bias gradients are
//                       folded over (sequence, head, tile) in a fixed two-level order.
//   the rest            prep, embed, LayerNorm, loss (seqrec.hpp), embed backward (SASRec's), the grouped GEMM with
//                       fixed-order column sums; weight gradients in up to 8 slabs of the rows, folded in slab order.
//
// Every gradient but item_emb.weight (row atomics) is the same bits on every run.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "gemm.hpp"
#include "seqrec.hpp"

namespace hiprec {
namespace {

constexpr int kHstuQT = 32;            // query rows (or key rows, in the key-side backward) a workgroup owns
constexpr int kHstuKC = 64;            // keys per chunk of the query-side kernels
constexpr int kHstuALd = 68;           // leading dimension of the 32 x 64 weight tile: 16-byte rows, conflict-free MFMA reads
constexpr int kHstuMaxBlocks = 16;
constexpr int kHstuMaxBuckets = 255;
constexpr int kHstuSlabs = 8;          // row slabs of a weight-gradient GEMM
constexpr int kHstuFoldSegs = 64;      // first-level segments of the bias-gradient fold
constexpr float kHstuEps = 1e-6f;
constexpr double kHstuLogBase = 0.301;
constexpr int64_t kHstuMaxTime = 1ll << 62;

struct HstuThr {
  int64_t v[kHstuMaxBuckets];          // v[k - 1] = the smallest d with floor(ln(d) / 0.301) >= k
};

__device__ __forceinline__ float hstu_silu(float x, float* dsilu) {
  const float sg = sigmoid_f32(x);
  *dsilu = sg * (1.f + x * (1.f - sg));
  return x * sg;
}

// ---- bucket prep: grid (B, T), block (b, i) covers the keys j <= i ------------------------------------------------------
__global__ __launch_bounds__(kBlock) void hstu_bucket_kernel(const int64_t* __restrict__ ts, const int64_t* __restrict__ seq,
                                                             HstuThr thr, int nbk, int T, uint8_t* __restrict__ bucket,
                                                             hiprec_stats* stats) {
  __shared__ uint64_t s_thr[kHstuMaxBuckets + 1];
  const int b = blockIdx.x, i = blockIdx.y;
  for (int k = threadIdx.x; k < nbk; k += kBlock) s_thr[k] = static_cast<uint64_t>(thr.v[k]);
  __syncthreads();
  const int64_t* row = ts + static_cast<int64_t>(b) * T;
  if (threadIdx.x == 0 && seq[static_cast<int64_t>(b) * T + i] != 0 && (row[i] < 0 || row[i] >= kHstuMaxTime))
    atomicOr(&stats->status, HIPREC_STATUS_ROW_OOB);
  const int64_t te = row[min(i + 1, T - 1)];
  uint8_t* out = bucket + (static_cast<int64_t>(b) * T + i) * T;
  for (int j = threadIdx.x; j <= i; j += kBlock) {
    const int64_t tj = row[j];
    const uint64_t d = te >= tj ? static_cast<uint64_t>(te) - static_cast<uint64_t>(tj)
                                : static_cast<uint64_t>(tj) - static_cast<uint64_t>(te);
    int lo = 0, hi = nbk;              // the count of thresholds <= d (the table is non-decreasing)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_thr[mid] <= d) lo = mid + 1; else hi = mid;
    }
    out[j] = static_cast<uint8_t>(lo);
  }
}

// ---- SiLU of the fused projection ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void hstu_silu_fwd_kernel(const float* __restrict__ pre, float* __restrict__ act,
                                                               int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const float x = pre[i];
    act[i] = x * sigmoid_f32(x);
  }
}

// d pre = d act * SiLU'(pre), in place
__global__ __launch_bounds__(kBlock) void hstu_silu_bwd_kernel(float* __restrict__ dact, const float* __restrict__ pre,
                                                               int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    float ds;
    hstu_silu(pre[i], &ds);
    dact[i] *= ds;
  }
}

__global__ void hstu_clamp_count_kernel(float* aux) {
  if (threadIdx.x == 0 && blockIdx.x == 0) aux[0] = fmaxf(aux[0], 1.f);   // no label: loss 0 and a zero gradient
}

// ---- gated norm: Y = LayerNorm_noaffine(AV over W = H * dv columns) * U through the keep bytes, one wave per row -----------
__global__ __launch_bounds__(kBlock) void hstu_gate_fwd_kernel(const float* __restrict__ av, const float* __restrict__ act,
                                                               int64_t ld, const uint8_t* __restrict__ keep, float ks,
                                                               float* __restrict__ y, float* __restrict__ mean,
                                                               float* __restrict__ rstd, int64_t M, int W) {
  const int lane = lane_id();
  const float inv_w = 1.f / static_cast<float>(W);
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); row < M;
       row += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const float v0 = lane < W ? av[row * W + lane] : 0.f, v1 = lane + 64 < W ? av[row * W + lane + 64] : 0.f;
    const float mu = wave_sum(v0 + v1) * inv_w;
    const float c0 = lane < W ? v0 - mu : 0.f, c1 = lane + 64 < W ? v1 - mu : 0.f;
    const float r = 1.0f / sqrtf(wave_sum(c0 * c0 + c1 * c1) * inv_w + kHstuEps);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      if (d < W) {
        float o = (h ? c1 : c0) * r * act[row * ld + d];
        if (keep) o = keep[row * W + d] ? o * ks : 0.f;
        y[row * W + d] = o;
      }
    }
    if (lane == 0) {
      mean[row] = mu;
      rstd[row] = r;
    }
  }
}

// from dY: dU = g * n into the u columns of dact, dAV = rstd * (dn - mean(dn) - n * mean(dn * n)) with g = dY through the
// keep bytes, n = (AV - mean) * rstd, dn = g * U
__global__ __launch_bounds__(kBlock) void hstu_gate_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ av,
                                                               const float* __restrict__ act, int64_t ld,
                                                               const uint8_t* __restrict__ keep, float ks,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, float* __restrict__ dav,
                                                               float* __restrict__ dact, int64_t M, int W) {
  const int lane = lane_id();
  const float inv_w = 1.f / static_cast<float>(W);
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); row < M;
       row += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const float mu = mean[row], r = rstd[row];
    float n[2] = {0.f, 0.f}, dn[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      if (d < W) {
        float g = dy[row * W + d];
        if (keep) g = keep[row * W + d] ? g * ks : 0.f;
        n[h] = (av[row * W + d] - mu) * r;
        dn[h] = g * act[row * ld + d];
        dact[row * ld + d] = g * n[h];
      }
    }
    const float m1 = wave_sum(dn[0] + dn[1]) * inv_w;
    const float m2 = wave_sum(dn[0] * n[0] + dn[1] * n[1]) * inv_w;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      if (d < W) dav[row * W + d] = r * (dn[h] - m1 - n[h] * m2);
    }
  }
}

// ---- pointwise attention ------------------------------------------------------------------------------------------------
// act [M, 2 H (DV + DQ)]: u | v | q | k, each head-major.  The columns of one head:
template <int DQ, int DV>
struct HstuCols {
  int64_t ld;
  int v, q, k;
  __host__ __device__ HstuCols(int H, int h) : ld(2ll * H * (DQ + DV)), v(H * DV + h * DV), q(2 * H * DV + h * DQ),
                                               k(2 * H * DV + H * DQ + h * DQ) {}
};

// the pos_w window of offsets d = i - j in [0, n) as s_pos[d] = pos_w[N - 1 - d] (0 past the sequence), and ts_w
__device__ __forceinline__ void hstu_stage_bias(float* s_pos, int n, int T, int N, const float* __restrict__ pos_w,
                                                float* s_ts, const float* __restrict__ ts_w, int nbk) {
  for (int e = threadIdx.x; e < n; e += kBlock) s_pos[e] = e < T ? pos_w[N - 1 - e] : 0.f;
  if (ts_w)
    for (int e = threadIdx.x; e <= nbk; e += kBlock) s_ts[e] = ts_w[e];
}

// grid (B * H, ceil(T / 32)).  AV [M, H * DV].
template <int DQ, int DV>
__global__ __launch_bounds__(kBlock) void hstu_attn_fwd_kernel(const float* __restrict__ act,
                                                               const float* __restrict__ pos_w,
                                                               const float* __restrict__ ts_w, int nbk,
                                                               const int64_t* __restrict__ seq,
                                                               const uint8_t* __restrict__ bucket, int T, int H, int N,
                                                               float* __restrict__ AV) {
  __shared__ float Qs[kHstuQT][DQ + 1];
  __shared__ float Ks[kHstuKC][DQ + 1];
  __shared__ float Vs[kHstuKC][DV + 1];
  __shared__ float As[kHstuQT][kHstuALd];
  __shared__ float s_pos[kSeqMaxLen + kHstuQT], s_ts[kHstuMaxBuckets + 1];
  __shared__ uint8_t s_vq[kHstuQT], s_vk[kHstuKC];
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int q0 = blockIdx.y * kHstuQT;
  const int lane = lane_id(), wave = wave_in_block();
  const HstuCols<DQ, DV> c(H, h);
  const float* base = act + static_cast<int64_t>(b) * T * c.ld;
  const int64_t* sq = seq + static_cast<int64_t>(b) * T;
  const uint8_t* bk = bucket + static_cast<int64_t>(b) * T * T;
  const float inv_n = 1.0f / static_cast<float>(N);
  const int n_keys = min(T, q0 + kHstuQT);
  const int n_chunks = (n_keys + kHstuKC - 1) / kHstuKC;
  load_tile<DQ>(&Qs[0][0], base + c.q, c.ld, q0, kHstuQT, T, 1.f);
  hstu_stage_bias(s_pos, q0 + kHstuQT, T, N, pos_w, s_ts, ts_w, nbk);
  if (threadIdx.x < kHstuQT) s_vq[threadIdx.x] = q0 + threadIdx.x < T && sq[q0 + threadIdx.x] != 0;
  constexpr int kColTiles = DV / 16, kTiles = 2 * kColTiles;
  f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * kHstuKC;
    __syncthreads();
    load_tile<DQ>(&Ks[0][0], base + c.k, c.ld, j0, kHstuKC, n_keys, 1.f);
    load_tile<DV>(&Vs[0][0], base + c.v, c.ld, j0, kHstuKC, n_keys, 1.f);
    if (threadIdx.x < kHstuKC) s_vk[threadIdx.x] = j0 + threadIdx.x < n_keys && sq[j0 + threadIdx.x] != 0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int tile = wave * 2 + u, rt = tile >> 2, ct = tile & 3;
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      s = mma16(s, &Qs[rt * 16][0], DQ + 1, 1, &Ks[ct * 16][0], 1, DQ + 1, DQ);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rt * 16 + 4 * (lane >> 4) + r, col = ct * 16 + (lane & 15);
        const int i = q0 + row, j = j0 + col;
        float a = 0.f;
        if (j <= i && s_vq[row] && s_vk[col]) {
          float x = s[r] + s_pos[i - j];
          if (ts_w) x += s_ts[bk[static_cast<int64_t>(i) * T + j]];
          a = x * sigmoid_f32(x) * inv_n;
        }
        As[row][col] = a;
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = wave + kWavesPerBlock * u;
      if (t < kTiles) {
        const int rt = t / kColTiles, ct = t - rt * kColTiles;
        acc[u] = mma16(acc[u], &As[rt * 16][0], kHstuALd, 1, &Vs[0][ct * 16], DV + 1, 1, kHstuKC);
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
        if (i < T) AV[(static_cast<int64_t>(b) * T + i) * (H * DV) + h * DV + ct * 16 + (lane & 15)] = acc[u][r];
      }
    }
  }
}

// backward, query side: a block owns 32 queries and walks the keys in chunks of 64.  dA = dAV v^T,
// dS = dA * SiLU'(S) / N under the masks, dq = dS k.  The block's share of d pos_w (entry d = i - j) and of d ts_w (entry
// = the bucket) is reduced from the dS tile in LDS: one owner thread per diagonal / per bucket scans the tile in a fixed
// order.  part [blocks, T + nbk + 1] receives the share (T entries without ts_w).
template <int DQ, int DV>
__global__ __launch_bounds__(kBlock) void hstu_attn_bwd_q_kernel(const float* __restrict__ act,
                                                                 const float* __restrict__ pos_w,
                                                                 const float* __restrict__ ts_w, int nbk,
                                                                 const int64_t* __restrict__ seq,
                                                                 const uint8_t* __restrict__ bucket,
                                                                 const float* __restrict__ dAV, int T, int H, int N,
                                                                 float* __restrict__ dact, float* __restrict__ part) {
  __shared__ float Qs[kHstuQT][DQ + 1];
  __shared__ float Gs[kHstuQT][DV + 1];
  __shared__ float Ks[kHstuKC][DQ + 1];
  __shared__ float Vs[kHstuKC][DV + 1];
  __shared__ __attribute__((aligned(16))) float DS[kHstuQT][kHstuALd];
  __shared__ __attribute__((aligned(16))) uint8_t Bk[kHstuQT][kHstuKC];
  __shared__ float s_pos[kSeqMaxLen + kHstuQT], s_dpos[kSeqMaxLen + kHstuQT];
  __shared__ float s_ts[kHstuMaxBuckets + 1], s_dts[kHstuMaxBuckets + 1];
  __shared__ uint8_t s_vq[kHstuQT], s_vk[kHstuKC];
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int q0 = blockIdx.y * kHstuQT;
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_in_block();
  const HstuCols<DQ, DV> c(H, h);
  const float* base = act + static_cast<int64_t>(b) * T * c.ld;
  const int64_t* sq = seq + static_cast<int64_t>(b) * T;
  const uint8_t* bk = bucket + static_cast<int64_t>(b) * T * T;
  const float inv_n = 1.0f / static_cast<float>(N);
  const int n_keys = min(T, q0 + kHstuQT);
  const int n_chunks = (n_keys + kHstuKC - 1) / kHstuKC;
  load_tile<DQ>(&Qs[0][0], base + c.q, c.ld, q0, kHstuQT, T, 1.f);
  load_tile<DV>(&Gs[0][0], dAV + static_cast<int64_t>(b) * T * (H * DV) + h * DV, H * DV, q0, kHstuQT, T, 1.f);
  hstu_stage_bias(s_pos, q0 + kHstuQT, T, N, pos_w, s_ts, ts_w, nbk);
  for (int e = tid; e < kSeqMaxLen + kHstuQT; e += kBlock) s_dpos[e] = 0.f;
  s_dts[tid] = 0.f;
  if (tid < kHstuQT) s_vq[tid] = q0 + tid < T && sq[q0 + tid] != 0;
  constexpr int kColTiles = DQ / 16, kTiles = 2 * kColTiles;
  f32x4 acc_q[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * kHstuKC;
    __syncthreads();
    load_tile<DQ>(&Ks[0][0], base + c.k, c.ld, j0, kHstuKC, n_keys, 1.f);
    load_tile<DV>(&Vs[0][0], base + c.v, c.ld, j0, kHstuKC, n_keys, 1.f);
    if (tid < kHstuKC) s_vk[tid] = j0 + tid < n_keys && sq[j0 + tid] != 0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int tile = wave * 2 + u, rt = tile >> 2, ct = tile & 3;
      f32x4 s = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
      s = mma16(s, &Qs[rt * 16][0], DQ + 1, 1, &Ks[ct * 16][0], 1, DQ + 1, DQ);
      da = mma16(da, &Gs[rt * 16][0], DV + 1, 1, &Vs[ct * 16][0], 1, DV + 1, DV);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rt * 16 + 4 * (lane >> 4) + r, col = ct * 16 + (lane & 15);
        const int i = q0 + row, j = j0 + col;
        float ds = 0.f;
        uint8_t bkt = 0;
        if (j <= i && s_vq[row] && s_vk[col]) {
          float x = s[r] + s_pos[i - j];
          if (ts_w) {
            bkt = bk[static_cast<int64_t>(i) * T + j];
            x += s_ts[bkt];
          }
          float dsilu;
          hstu_silu(x, &dsilu);
          ds = da[r] * dsilu * inv_n;
        }
        DS[row][col] = ds;
        Bk[row][col] = bkt;
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = wave + kWavesPerBlock * u;
      if (t < kTiles) {
        const int rt = t / kColTiles, ct = t - rt * kColTiles;
        acc_q[u] = mma16(acc_q[u], &DS[rt * 16][0], kHstuALd, 1, &Ks[0][ct * 16], DQ + 1, 1, kHstuKC);
      }
    }
    // d pos_w: thread t owns the diagonal d = q0 - j0 + 31 - t of this chunk, i.e. the entries (r, r - 31 + t)
    if (tid < kHstuQT + kHstuKC - 1) {
      const int d = q0 - j0 + kHstuQT - 1 - tid;
      if (d >= 0) {
        float sum = 0.f;
        const int r_lo = max(0, kHstuQT - 1 - tid), r_hi = min(kHstuQT, kHstuQT + kHstuKC - 1 - tid);
#pragma unroll 1
        for (int r = r_lo; r < r_hi; ++r) sum += DS[r][r - (kHstuQT - 1) + tid];      // the rows whose column is in the tile
        s_dpos[d] += sum;
      }
    }
    // d ts_w: thread k owns bucket k and scans the tile row by row, four entries per read
    if (ts_w && tid <= nbk) {
      float sum = 0.f;
#pragma unroll 1
      for (int r = 0; r < kHstuQT; ++r) {      // one row per trip: the bytes are uniform, unrolled rows would all sit in SGPRs
        const uint32_t* b4 = reinterpret_cast<const uint32_t*>(&Bk[r][0]);
        const float4* d4 = reinterpret_cast<const float4*>(&DS[r][0]);
#pragma unroll 4
        for (int q = 0; q < kHstuKC / 4; ++q) {
          const uint32_t bb = b4[q];
          const float4 dv = d4[q];
          sum += (bb & 255u) == static_cast<uint32_t>(tid) ? dv.x : 0.f;
          sum += ((bb >> 8) & 255u) == static_cast<uint32_t>(tid) ? dv.y : 0.f;
          sum += ((bb >> 16) & 255u) == static_cast<uint32_t>(tid) ? dv.z : 0.f;
          sum += (bb >> 24) == static_cast<uint32_t>(tid) ? dv.w : 0.f;
        }
      }
      s_dts[tid] += sum;
    }
  }
  __syncthreads();
  const int E = T + (ts_w ? nbk + 1 : 0);
  float* slab = part + (static_cast<int64_t>(bh) * gridDim.y + blockIdx.y) * E;
  for (int e = tid; e < T; e += kBlock) slab[e] = s_dpos[e];
  if (ts_w && tid <= nbk) slab[T + tid] = s_dts[tid];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int t = wave + kWavesPerBlock * u;
    if (t < kTiles) {
      const int rt = t / kColTiles, ct = t - rt * kColTiles;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = q0 + rt * 16 + 4 * (lane >> 4) + r;
        if (i < T) dact[(static_cast<int64_t>(b) * T + i) * c.ld + c.q + ct * 16 + (lane & 15)] = acc_q[u][r];
      }
    }
  }
}

// backward, key side: a block owns 32 keys and walks the queries j .. T - 1 in chunks of 32.  S^T = k q^T,
// dk = dS^T q, dv = A^T dAV, each summed in a fixed order: no atomics.
template <int DQ, int DV>
__global__ __launch_bounds__(kBlock) void hstu_attn_bwd_kv_kernel(const float* __restrict__ act,
                                                                  const float* __restrict__ pos_w,
                                                                  const float* __restrict__ ts_w, int nbk,
                                                                  const int64_t* __restrict__ seq,
                                                                  const uint8_t* __restrict__ bucket,
                                                                  const float* __restrict__ dAV, int T, int H, int N,
                                                                  float* __restrict__ dact) {
  __shared__ float Ks[kHstuQT][DQ + 1];
  __shared__ float Vs[kHstuQT][DV + 1];
  __shared__ float Qc[kHstuQT][DQ + 1];
  __shared__ float Gc[kHstuQT][DV + 1];
  __shared__ float AT[kHstuQT][kHstuQT + 1];
  __shared__ float DST[kHstuQT][kHstuQT + 1];
  __shared__ float s_pos[kSeqMaxLen], s_ts[kHstuMaxBuckets + 1];
  __shared__ uint8_t s_vk[kHstuQT], s_vq[kHstuQT];
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int j0 = blockIdx.y * kHstuQT;
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_in_block();
  const HstuCols<DQ, DV> c(H, h);
  const float* base = act + static_cast<int64_t>(b) * T * c.ld;
  const float* g_base = dAV + static_cast<int64_t>(b) * T * (H * DV) + h * DV;
  const int64_t* sq = seq + static_cast<int64_t>(b) * T;
  const uint8_t* bk = bucket + static_cast<int64_t>(b) * T * T;
  const float inv_n = 1.0f / static_cast<float>(N);
  load_tile<DQ>(&Ks[0][0], base + c.k, c.ld, j0, kHstuQT, T, 1.f);
  load_tile<DV>(&Vs[0][0], base + c.v, c.ld, j0, kHstuQT, T, 1.f);
  hstu_stage_bias(s_pos, kSeqMaxLen, T, N, pos_w, s_ts, ts_w, nbk);
  if (tid < kHstuQT) s_vk[tid] = j0 + tid < T && sq[j0 + tid] != 0;
  constexpr int kColK = DQ / 16, kColV = DV / 16;
  f32x4 acc_k[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  f32x4 acc_v[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int i0 = j0; i0 < T; i0 += kHstuQT) {
    __syncthreads();
    load_tile<DQ>(&Qc[0][0], base + c.q, c.ld, i0, kHstuQT, T, 1.f);
    load_tile<DV>(&Gc[0][0], g_base, H * DV, i0, kHstuQT, T, 1.f);
    if (tid < kHstuQT) s_vq[tid] = i0 + tid < T && sq[i0 + tid] != 0;
    __syncthreads();
    {
      const int rt = wave >> 1, ct = wave & 1;       // 2 x 2 tiles of the [32 keys, 32 queries] block, one per wave
      f32x4 s = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
      s = mma16(s, &Ks[rt * 16][0], DQ + 1, 1, &Qc[ct * 16][0], 1, DQ + 1, DQ);
      da = mma16(da, &Vs[rt * 16][0], DV + 1, 1, &Gc[ct * 16][0], 1, DV + 1, DV);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rt * 16 + 4 * (lane >> 4) + r, col = ct * 16 + (lane & 15);
        const int j = j0 + row, i = i0 + col;
        float a = 0.f, ds = 0.f;
        if (j <= i && s_vk[row] && s_vq[col]) {
          float x = s[r] + s_pos[i - j];
          if (ts_w) x += s_ts[bk[static_cast<int64_t>(i) * T + j]];
          float dsilu;
          a = hstu_silu(x, &dsilu) * inv_n;
          ds = da[r] * dsilu * inv_n;
        }
        AT[row][col] = a;
        DST[row][col] = ds;
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = wave + kWavesPerBlock * u;
      if (t < 2 * kColK) {
        const int rt = t / kColK, ct = t - rt * kColK;
        acc_k[u] = mma16(acc_k[u], &DST[rt * 16][0], kHstuQT + 1, 1, &Qc[0][ct * 16], DQ + 1, 1, kHstuQT);
      }
      if (t < 2 * kColV) {
        const int rt = t / kColV, ct = t - rt * kColV;
        acc_v[u] = mma16(acc_v[u], &AT[rt * 16][0], kHstuQT + 1, 1, &Gc[0][ct * 16], DV + 1, 1, kHstuQT);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int t = wave + kWavesPerBlock * u;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (t < 2 * kColK) {
        const int rt = t / kColK, ct = t - rt * kColK, j = j0 + rt * 16 + 4 * (lane >> 4) + r;
        if (j < T) dact[(static_cast<int64_t>(b) * T + j) * c.ld + c.k + ct * 16 + (lane & 15)] = acc_k[u][r];
      }
      if (t < 2 * kColV) {
        const int rt = t / kColV, ct = t - rt * kColV, j = j0 + rt * 16 + 4 * (lane >> 4) + r;
        if (j < T) dact[(static_cast<int64_t>(b) * T + j) * c.ld + c.v + ct * 16 + (lane & 15)] = acc_v[u][r];
      }
    }
  }
}

// the bias gradients from the n_slabs slabs of E = T (+ nbk + 1) entries: 64 segments of consecutive slabs each summed in
// order, then the segments in order.  Entry d < T goes to d pos_w[N - 1 - d], entry T + k to d ts_w[k].  4 entries / block.
__global__ __launch_bounds__(kBlock) void hstu_bias_fold_kernel(const float* __restrict__ part, int64_t n_slabs, int E, int T,
                                                                int N, float* __restrict__ dpos, float* __restrict__ dts) {
  __shared__ float s_seg[kHstuFoldSegs][4];
  const int e = blockIdx.x * 4 + (threadIdx.x & 3), seg = threadIdx.x >> 2;
  const int64_t per = (n_slabs + kHstuFoldSegs - 1) / kHstuFoldSegs;
  const int64_t lo = per * seg, hi = min(n_slabs, lo + per);
  float s = 0.f;
  if (e < E)
    for (int64_t k = lo; k < hi; ++k) s += part[k * E + e];
  s_seg[seg][threadIdx.x & 3] = s;
  __syncthreads();
  if (seg != 0 || e >= E) return;
  float total = 0.f;
  for (int k = 0; k < kHstuFoldSegs; ++k) total += s_seg[k][threadIdx.x & 3];
  if (e < T) dpos[N - 1 - e] = total; else dts[e - T] = total;
}

__global__ __launch_bounds__(kBlock) void hstu_fold_kernel(float* __restrict__ out, const float* __restrict__ part, int64_t n,
                                                           int slabs) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    float s = part[i];
    for (int k = 1; k < slabs; ++k) s += part[k * n + i];
    out[i] = s;
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------
struct HstuBlock {
  float *ln_w, *ln_b, *uvqk, *pos_w, *ts_w, *o_w, *o_b;
};
struct HstuParams {      // pointers into a flat buffer laid out in state_dict() order
  float *item_emb, *pos_emb, *last_w, *last_b;
  HstuBlock blk[kHstuMaxBlocks];
};

struct HstuDims {
  int D, H, dq, dv, W, Wt, N, nb, nbk;
  bool time;
  explicit HstuDims(const hiprec_hstu_shape& s)
      : D(s.dim), H(s.heads), dq(s.attention_dim), dv(s.linear_dim), W(s.heads * s.linear_dim),
        Wt(2 * s.heads * (s.attention_dim + s.linear_dim)), N(s.maxlen), nb(s.n_blocks), nbk(s.num_buckets),
        time(s.rel_bias == HIPREC_HSTU_BIAS_POS_TIME) {}
};

int64_t hstu_walk_params(float* base, const hiprec_hstu_shape& s, HstuParams* p) {
  const HstuDims d(s);
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += n; return r; };
  HstuParams q{};
  q.item_emb = take((s.n_items + 1) * d.D);
  q.pos_emb = take(static_cast<int64_t>(d.N) * d.D);
  for (int k = 0; k < d.nb; ++k) {
    HstuBlock& b = q.blk[k];
    b.ln_w = take(d.D);
    b.ln_b = take(d.D);
    b.uvqk = take(static_cast<int64_t>(d.D) * d.Wt);
    b.pos_w = take(2 * d.N - 1);
    b.ts_w = d.time ? take(d.nbk + 1) : nullptr;
    b.o_w = take(static_cast<int64_t>(d.D) * d.W);
    b.o_b = take(d.D);
  }
  q.last_w = take(d.D);
  q.last_b = take(d.D);
  if (p) *p = q;
  return c - base;
}

struct HstuSaved {
  float *x, *xn, *pre, *act, *av, *y, *mean_a, *rstd_a, *mean_g, *rstd_g;
};
struct HstuWorkspace {
  HstuSaved sv[kHstuMaxBlocks];
  float *x_last, *feats, *mean_l, *rstd_l, *z, *t[5], *dy, *dav, *dact, *aux, *cs, *part, *bpart;
  uint8_t* bucket;
  int64_t floats;
};

int64_t hstu_slabs(int64_t B, int T, int H) { return B * H * ((T + kHstuQT - 1) / kHstuQT); }
int hstu_bias_entries(int T, int nbk, bool time) { return T + (time ? nbk + 1 : 0); }

HstuWorkspace hstu_carve(float* base, const hiprec_hstu_shape& s, int64_t B, int T) {
  HstuWorkspace w{};
  const HstuDims d(s);
  const int64_t M = B * T, MD = M * d.D, MW = M * d.W, MT = M * d.Wt;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += (n + 3) / 4 * 4; return r; };
  for (int k = 0; k < d.nb; ++k)
    w.sv[k] = HstuSaved{take(MD), take(MD), take(MT), take(MT), take(MW), take(MW), take(M), take(M), take(M), take(M)};
  w.x_last = take(MD); w.feats = take(MD); w.mean_l = take(M); w.rstd_l = take(M); w.z = take(MD);
  for (int i = 0; i < 5; ++i) w.t[i] = take(MD);
  w.dy = take(MW); w.dav = take(MW); w.dact = take(MT);
  w.aux = take(kSeqAux);
  w.cs = take(2 * colsum_ws_floats(static_cast<int>(M), d.D));
  w.part = take(static_cast<int64_t>(kHstuSlabs) * d.D * d.Wt);
  w.bpart = take(hstu_slabs(B, T, d.H) * hstu_bias_entries(T, d.nbk, d.time));
  w.bucket = reinterpret_cast<uint8_t*>(take(d.time ? (M * T + 3) / 4 : 0));
  w.floats = c - base;
  return w;
}

bool hstu_width_ok(int w) { return w == 16 || w == 32 || w == 64; }

int hstu_check_attention(int heads, int dq, int dv, int maxlen, int nbk) {
  HIPREC_REQUIRE(heads >= 1, "HSTU needs num_heads >= 1 (got %d)", heads);
  HIPREC_REQUIRE(hstu_width_ok(dq), "HSTU needs attention_dim in (16, 32, 64) (got %d)", dq);
  HIPREC_REQUIRE(hstu_width_ok(dv), "HSTU needs linear_dim in (16, 32, 64) (got %d)", dv);
  HIPREC_REQUIRE(heads * dq <= kSeqMaxDim && heads * dv <= kSeqMaxDim,
                 "HSTU needs num_heads * attention_dim <= %d and num_heads * linear_dim <= %d", kSeqMaxDim, kSeqMaxDim);
  HIPREC_REQUIRE(maxlen >= 1 && maxlen <= kSeqMaxLen, "HSTU needs 1 <= maxlen <= %d (got %d)", kSeqMaxLen, maxlen);
  HIPREC_REQUIRE(nbk >= 1 && nbk <= kHstuMaxBuckets, "HSTU needs 1 <= num_buckets <= %d (got %d)", kHstuMaxBuckets, nbk);
  return 0;
}

int hstu_check_shape(const hiprec_hstu_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  HIPREC_REQUIRE(s->n_items >= 1 && s->n_items < (1ll << 31) - 1, "HSTU needs 1 <= n_items < 2^31 - 1");
  HIPREC_REQUIRE(s->dim >= 16 && s->dim <= kSeqMaxDim && s->dim % 16 == 0,
                 "HSTU needs emb_dim a multiple of 16 in 16 .. %d (got %d)", kSeqMaxDim, s->dim);
  HIPREC_REQUIRE(s->n_blocks >= 1 && s->n_blocks <= kHstuMaxBlocks, "HSTU needs 1 <= num_blocks <= %d (got %d)",
                 kHstuMaxBlocks, s->n_blocks);
  HIPREC_REQUIRE(s->rel_bias == HIPREC_HSTU_BIAS_POS_TIME || s->rel_bias == HIPREC_HSTU_BIAS_POS,
                 "HSTU needs rel_bias pos_time or pos (got %d)", s->rel_bias);
  return hstu_check_attention(s->heads, s->attention_dim, s->linear_dim, s->maxlen, s->num_buckets);
}

// B * T < 2^24 (the row counts are exact in fp32) also keeps every grid dimension and B * H far below 2^31
bool hstu_batch_ok(int64_t B, int T, int maxlen) { return B >= 1 && T >= 1 && T <= maxlen && B * T < (1ll << 24); }

int hstu_thresholds(int nbk, int64_t* out) {
  HIPREC_REQUIRE(out && nbk >= 1 && nbk <= kHstuMaxBuckets, "threshold table: 1 <= num_buckets <= %d and a buffer",
                 kHstuMaxBuckets);
  auto bucket_of = [](int64_t d) { return std::floor(std::log(static_cast<double>(d)) / kHstuLogBase); };
  for (int k = 1; k <= nbk; ++k) {
    const double edge = std::exp(kHstuLogBase * k);
    if (edge >= static_cast<double>(kHstuMaxTime)) {      // no time gap below 2^62 reaches this bucket
      out[k - 1] = INT64_MAX;
      continue;
    }
    int64_t c = std::max<int64_t>(1, static_cast<int64_t>(std::ceil(edge)));
    while (c > 1 && bucket_of(c - 1) >= k) --c;           // the formula itself decides at the candidate's neighbours
    while (bucket_of(c) < k) ++c;
    out[k - 1] = c;
  }
  return 0;
}

int hstu_buckets(const int64_t* ts, const int64_t* seq, int64_t B, int T, int nbk, uint8_t* bucket, hiprec_stats* stats,
                 hipStream_t st) {
  HstuThr thr;
  std::memset(&thr, 0, sizeof(thr));
  if (int rc = hstu_thresholds(nbk, thr.v)) return rc;
  hstu_bucket_kernel<<<dim3(static_cast<unsigned>(B), static_cast<unsigned>(T)), kBlock, 0, st>>>(ts, seq, thr, nbk, T,
                                                                                                 bucket, stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

template <typename F>
int hstu_by_widths(int dq, int dv, F&& f) {
  return by_head_width(dq, [&](auto a) { return by_head_width(dv, [&](auto b) { return f(a, b); }); });
}

struct HstuAttn {        // what the three attention launches share
  const float *act, *pos_w, *ts_w;
  const int64_t* seq;
  const uint8_t* bucket;
  int64_t B;
  int T, H, dq, dv, N, nbk;
  dim3 grid() const { return dim3(static_cast<unsigned>(B * H), static_cast<unsigned>((T + kHstuQT - 1) / kHstuQT)); }
};

int hstu_attn_fwd(const HstuAttn& a, float* av, hipStream_t st) {
  return hstu_by_widths(a.dq, a.dv, [&](auto q, auto v) {
    hstu_attn_fwd_kernel<decltype(q)::value, decltype(v)::value><<<a.grid(), kBlock, 0, st>>>(
        a.act, a.pos_w, a.ts_w, a.nbk, a.seq, a.bucket, a.T, a.H, a.N, av);
    HIPREC_TRY(hipGetLastError());
    return 0;
  });
}

// dq | dk | dv into their columns of dact [M, Wt]; dpos [2 N - 1] and dts [nbk + 1] receive plain stores at the entries
// a pair can reach (offsets j - i in -(T - 1) .. 0, every bucket)
int hstu_attn_bwd(const HstuAttn& a, const float* dav, float* dact, float* dpos, float* dts, float* bpart, hipStream_t st) {
  if (int rc = hstu_by_widths(a.dq, a.dv, [&](auto q, auto v) {
        constexpr int DQ = decltype(q)::value, DV = decltype(v)::value;
        hstu_attn_bwd_q_kernel<DQ, DV><<<a.grid(), kBlock, 0, st>>>(a.act, a.pos_w, a.ts_w, a.nbk, a.seq, a.bucket, dav,
                                                                    a.T, a.H, a.N, dact, bpart);
        HIPREC_TRY(hipGetLastError());
        hstu_attn_bwd_kv_kernel<DQ, DV><<<a.grid(), kBlock, 0, st>>>(a.act, a.pos_w, a.ts_w, a.nbk, a.seq, a.bucket, dav,
                                                                     a.T, a.H, a.N, dact);
        HIPREC_TRY(hipGetLastError());
        return 0;
      }))
    return rc;
  const int E = hstu_bias_entries(a.T, a.nbk, a.ts_w != nullptr);
  hstu_bias_fold_kernel<<<(E + 3) / 4, kBlock, 0, st>>>(bpart, hstu_slabs(a.B, a.T, a.H), E, a.T, a.N, dpos, dts);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// C[rows, cols] = A^T B over K rows, as problems of g: one with plain stores into the zeroed gradient, or (long K) up to
// kHstuSlabs slabs of K into `part`, which hstu_fold adds up in slab order afterwards.  Returns the slab count.
int hstu_add_wgrad(GemmGroup& g, int rows, int cols, int K, const float* A, int lda, const float* Bm, int ldb, float* out,
                   float* part) {
  const int slabs = std::min(kHstuSlabs, (K + 511) / 512);
  if (slabs <= 1) {
    g.p[g.n++] = make_gemm(kTNm, rows, cols, K, A, lda, Bm, ldb, out, cols, nullptr, 0, nullptr, 0, false);
    return 1;
  }
  const int per = ((K + slabs - 1) / slabs + 15) / 16 * 16;
  int s = 0;
  for (int k0 = 0; k0 < K; k0 += per, ++s)
    g.p[g.n++] = make_gemm(kTNm, rows, cols, std::min(per, K - k0), A + static_cast<int64_t>(k0) * lda, lda,
                           Bm + static_cast<int64_t>(k0) * ldb, ldb, part + static_cast<int64_t>(s) * rows * cols, cols,
                           nullptr, 0, nullptr, 0, false);
  return s;
}

int hstu_fold(float* out, const float* part, int64_t n, int slabs, hipStream_t st) {
  if (slabs <= 1) return 0;
  hstu_fold_kernel<<<grid_for_threads(n), kBlock, 0, st>>>(out, part, n, slabs);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

int hstu_run(const hiprec_hstu_shape& s, float* w_flat, float* g_flat, const int64_t* seq, const int64_t* time_seq,
             const int64_t* pos, const int64_t* neg, int64_t B, int T, float l2, const uint8_t* const* keep, float ks,
             float* feats_out, hiprec_stats* stats, Scratch* scratch, float* ws_base, hipStream_t st) {
  const HstuDims d(s);
  const int D = d.D, W = d.W, Wt = d.Wt, nb = d.nb;
  const int64_t M = B * T;
  const int Mi = static_cast<int>(M);
  const bool train = g_flat != nullptr;
  HstuParams w, g;
  hstu_walk_params(w_flat, s, &w);
  const HstuWorkspace a = hstu_carve(ws_base, s, B, T);
  const float sqrt_d = sqrtf(static_cast<float>(D));
  auto kp = [&](int i) -> const uint8_t* { return keep ? keep[i] : nullptr; };
  auto attn = [&](int k) {
    return HstuAttn{a.sv[k].act, w.blk[k].pos_w, w.blk[k].ts_w, seq, a.bucket, B, T, d.H, d.dq, d.dv, d.N, d.nbk};
  };

  if (train) {
    if (int rc = seq_prep(w.item_emb, g_flat, (s.n_items + 1) * D, pos, M, l2, a.aux, st)) return rc;
    hstu_clamp_count_kernel<<<1, kWave, 0, st>>>(a.aux);
    HIPREC_TRY(hipGetLastError());
  }
  if (d.time)
    if (int rc = hstu_buckets(time_seq, seq, B, T, d.nbk, a.bucket, stats, st)) return rc;
  if (int rc = seq_embed(w.item_emb, w.pos_emb, seq, M, T, D, s.n_items, sqrt_d, kp(0), ks, a.sv[0].x, stats, st))
    return rc;
  if (int rc = seq_ln_fwd(a.sv[0].x, nullptr, nullptr, nullptr, w.blk[0].ln_w, w.blk[0].ln_b, a.sv[0].xn, a.sv[0].mean_a,
                          a.sv[0].rstd_a, M, D, st, kHstuEps))
    return rc;
  for (int k = 0; k < nb; ++k) {
    const HstuSaved& v = a.sv[k];
    const HstuBlock& q = w.blk[k];
    GemmGroup p{};
    p.n = 1;
    p.p[0] = make_gemm(kNN, Mi, Wt, D, v.xn, D, q.uvqk, Wt, v.pre, Wt, nullptr, 0, nullptr, 0, false);
    if (int rc = launch_group(p, st)) return rc;
    hstu_silu_fwd_kernel<<<grid_for_threads(M * Wt), kBlock, 0, st>>>(v.pre, v.act, M * Wt);
    HIPREC_TRY(hipGetLastError());
    if (int rc = hstu_attn_fwd(attn(k), v.av, st)) return rc;
    hstu_gate_fwd_kernel<<<grid_for_waves(M), kBlock, 0, st>>>(v.av, v.act, Wt, kp(1 + k), ks, v.y, v.mean_g, v.rstd_g, M,
                                                               W);
    HIPREC_TRY(hipGetLastError());
    p = GemmGroup{};
    p.n = 1;
    p.p[0] = make_gemm(kNT, Mi, D, W, v.y, W, q.o_w, W, a.z, D, q.o_b, 0, nullptr, 0, false);
    if (int rc = launch_group(p, st)) return rc;
    // x' = (x + z) * valid on the way into the next LayerNorm
    const bool last = k + 1 == nb;
    if (int rc = seq_ln_fwd(v.x, a.z, seq, last ? a.x_last : a.sv[k + 1].x, last ? w.last_w : w.blk[k + 1].ln_w,
                            last ? w.last_b : w.blk[k + 1].ln_b, last ? (train ? a.feats : feats_out) : a.sv[k + 1].xn,
                            last ? a.mean_l : a.sv[k + 1].mean_a, last ? a.rstd_l : a.sv[k + 1].rstd_a, M, D, st,
                            kHstuEps))
      return rc;
  }
  if (!train) return 0;
  if (feats_out) HIPREC_TRY(hipMemcpyAsync(feats_out, a.feats, sizeof(float) * M * D, hipMemcpyDeviceToDevice, st));

  hstu_walk_params(g_flat, s, &g);
  float *T1 = a.t[0], *T2 = a.t[1], *T3 = a.t[2], *T6 = a.t[3], *T8 = a.t[4];
  if (int rc = seq_loss(a.feats, w.item_emb, pos, neg, M, D, s.n_items, a.aux, l2, T1, g.item_emb, scratch, stats, st))
    return rc;
  // T2: the gradient of a block's masked output x + z
  if (int rc = seq_ln_bwd(T1, nullptr, a.x_last, nullptr, w.last_w, a.mean_l, a.rstd_l, nullptr, nullptr, seq, nullptr, ks,
                          T2, nullptr, T6, T8, g.last_w, g.last_b, a.cs, M, D, st))
    return rc;
  for (int k = nb - 1; k >= 0; --k) {
    const HstuSaved& v = a.sv[k];
    const HstuBlock &q = w.blk[k], &gq = g.blk[k];
    {
      GemmGroup p{};
      p.p[p.n++] = make_gemm(kNN, Mi, W, D, T2, D, q.o_w, W, a.dy, W, nullptr, 0, nullptr, 0, false);
      const int slabs = hstu_add_wgrad(p, D, W, Mi, T2, D, v.y, W, gq.o_w, a.part);
      p.p[p.n++] = make_colsum(T2, Mi, D, D, gq.o_b, a.cs);
      if (int rc = launch_group(p, st)) return rc;
      if (int rc = launch_colsum_reduce(p, st)) return rc;
      if (int rc = hstu_fold(gq.o_w, a.part, static_cast<int64_t>(D) * W, slabs, st)) return rc;
    }
    hstu_gate_bwd_kernel<<<grid_for_waves(M), kBlock, 0, st>>>(a.dy, v.av, v.act, Wt, kp(1 + k), ks, v.mean_g, v.rstd_g,
                                                               a.dav, a.dact, M, W);
    HIPREC_TRY(hipGetLastError());
    if (int rc = hstu_attn_bwd(attn(k), a.dav, a.dact, gq.pos_w, gq.ts_w, a.bpart, st)) return rc;
    hstu_silu_bwd_kernel<<<grid_for_threads(M * Wt), kBlock, 0, st>>>(a.dact, v.pre, M * Wt);
    HIPREC_TRY(hipGetLastError());
    {
      GemmGroup p{};
      p.p[p.n++] = make_gemm(kNT, Mi, D, Wt, a.dact, Wt, q.uvqk, Wt, T1, D, nullptr, 0, nullptr, 0, false);
      const int slabs = hstu_add_wgrad(p, D, Wt, Mi, v.xn, D, a.dact, Wt, gq.uvqk, a.part);
      if (int rc = launch_group(p, st)) return rc;
      if (int rc = hstu_fold(gq.uvqk, a.part, static_cast<int64_t>(D) * Wt, slabs, st)) return rc;
    }
    // LN: dy = d xn, plus the residual's gradient T2; block k > 0 reads a masked sum
    if (int rc = seq_ln_bwd(T1, nullptr, v.x, nullptr, q.ln_w, v.mean_a, v.rstd_a, T2, nullptr, k > 0 ? seq : nullptr,
                            nullptr, ks, T3, nullptr, T6, T8, gq.ln_w, gq.ln_b, a.cs, M, D, st))
      return rc;
    std::swap(T2, T3);
  }
  return seq_embed_bwd(T2, seq, B, T, D, s.n_items, sqrt_d, kp(0), ks, g.item_emb, g.pos_emb, st);
}

int hstu_check_call(const hiprec_hstu_shape* shape, const void* w_flat, const void* seq, const void* time_seq, int64_t batch,
                    int seq_len, const void* stats, const void* workspace, size_t workspace_bytes) {
  if (int rc = hstu_check_shape(shape)) return rc;
  HIPREC_REQUIRE(w_flat && seq && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(time_seq || shape->rel_bias == HIPREC_HSTU_BIAS_POS, "HSTU: rel_bias pos_time needs time_seq");
  HIPREC_REQUIRE(hstu_batch_ok(batch, seq_len, shape->maxlen),
                 "HSTU: bad batch / sequence length (maxlen %d; batch x length below 2^24)", shape->maxlen);
  const size_t need = hiprec_hstu_workspace_bytes(shape, batch, seq_len);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  return 0;
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_hstu_shape_bytes(void) { return sizeof(hiprec_hstu_shape); }

extern "C" int64_t hiprec_hstu_param_floats(const hiprec_hstu_shape* shape) {
  if (hstu_check_shape(shape)) return -1;
  return hstu_walk_params(nullptr, *shape, nullptr);
}

extern "C" size_t hiprec_hstu_workspace_bytes(const hiprec_hstu_shape* shape, int64_t batch, int32_t seq_len) {
  if (hstu_check_shape(shape) || !hstu_batch_ok(batch, seq_len, shape->maxlen)) return 0;
  return sizeof(float) * static_cast<size_t>(hstu_carve(nullptr, *shape, batch, seq_len).floats);
}

extern "C" int hiprec_hstu_time_thresholds(int32_t num_buckets, int64_t* out) { return hstu_thresholds(num_buckets, out); }

extern "C" int hiprec_hstu_grad(const hiprec_hstu_shape* shape, const float* w_flat, float* g_flat, const int64_t* seq,
                                const int64_t* time_seq, const int64_t* pos, const int64_t* neg, int64_t batch,
                                int32_t seq_len, float l2_emb, const uint8_t* const* keep, float keep_scale,
                                float* feats_out, hiprec_stats* stats, void* scratch, size_t scratch_bytes, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (int rc = hstu_check_call(shape, w_flat, seq, time_seq, batch, seq_len, stats, workspace, workspace_bytes)) return rc;
  HIPREC_REQUIRE(g_flat && pos && neg && scratch, "training needs the gradient buffer, pos, neg and the scratch block");
  if (scratch_bytes < kScratchBytes) {
    set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
    return HIPREC_E_SCRATCH;
  }
  return hstu_run(*shape, const_cast<float*>(w_flat), g_flat, seq, time_seq, pos, neg, batch, seq_len, l2_emb, keep,
                  keep_scale, feats_out, stats, static_cast<Scratch*>(scratch), static_cast<float*>(workspace),
                  static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_hstu_feats(const hiprec_hstu_shape* shape, const float* w_flat, const int64_t* seq,
                                 const int64_t* time_seq, int64_t batch, int32_t seq_len, float* feats_out,
                                 hiprec_stats* stats, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = hstu_check_call(shape, w_flat, seq, time_seq, batch, seq_len, stats, workspace, workspace_bytes)) return rc;
  HIPREC_REQUIRE(feats_out, "the eval forward needs the feats buffer");
  return hstu_run(*shape, const_cast<float*>(w_flat), nullptr, seq, time_seq, nullptr, nullptr, batch, seq_len, 0.f, nullptr,
                  1.0f, feats_out, stats, nullptr, static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_hstu_buckets(const int64_t* time_seq, const int64_t* seq, int64_t batch, int32_t seq_len,
                                   int32_t num_buckets, uint8_t* bucket, hiprec_stats* stats, void* stream) {
  HIPREC_REQUIRE(time_seq && seq && bucket && stats, "NULL pointer");
  HIPREC_REQUIRE(hstu_batch_ok(batch, seq_len, kSeqMaxLen), "HSTU buckets: bad batch / sequence length");
  return hstu_buckets(time_seq, seq, batch, seq_len, num_buckets, bucket, stats, static_cast<hipStream_t>(stream));
}

extern "C" int64_t hiprec_hstu_attention_scratch_floats(int64_t batch, int32_t seq_len, int32_t heads, int32_t num_buckets) {
  if (heads < 1 || !hstu_batch_ok(batch, seq_len, kSeqMaxLen) || num_buckets < 1 || num_buckets > kHstuMaxBuckets)
    return -1;
  return hstu_slabs(batch, seq_len, heads) * hstu_bias_entries(seq_len, num_buckets, true);
}

extern "C" int hiprec_hstu_attention(const float* act, const float* pos_w, const float* ts_w, const int64_t* seq,
                                     const uint8_t* bucket, const float* dav, int64_t batch, int32_t seq_len, int32_t heads,
                                     int32_t attention_dim, int32_t linear_dim, int32_t maxlen, int32_t num_buckets,
                                     float* av, float* dact, float* dpos_w, float* dts_w, float* scratch,
                                     size_t scratch_floats, void* stream) {
  if (int rc = hstu_check_attention(heads, attention_dim, linear_dim, maxlen, num_buckets)) return rc;
  HIPREC_REQUIRE(act && pos_w && seq && (av || dav) && (bucket || !ts_w), "NULL pointer");
  HIPREC_REQUIRE(hstu_batch_ok(batch, seq_len, maxlen), "HSTU attention: bad batch / sequence length (maxlen %d)",
                 maxlen);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const HstuAttn a{act, pos_w, ts_w, seq, bucket, batch, seq_len, heads, attention_dim, linear_dim, maxlen, num_buckets};
  if (av)
    if (int rc = hstu_attn_fwd(a, av, st)) return rc;
  if (!dav) return 0;
  HIPREC_REQUIRE(dact && dpos_w && scratch && (dts_w || !ts_w), "the attention backward needs dact, dpos_w, dts_w and scratch");
  const int64_t need = hiprec_hstu_attention_scratch_floats(batch, seq_len, heads, num_buckets);
  HIPREC_REQUIRE(scratch_floats >= static_cast<size_t>(need), "attention scratch %zu floats < %lld", scratch_floats,
                 static_cast<long long>(need));
  return hstu_attn_bwd(a, dav, dact, dpos_w, dts_w, scratch, st);
}
