// ComiRec-DR (Cen et al., KDD 2020; the capsule routing of MIND, Li et al., CIKM 2019): zero_grad + forward + loss + backward
// of one step as a fixed sequence of launches, no host sync.  The contract is in include/hiprec.h; B sequences of T slots,
// K interests of width D, R routing iterations, S shared samples.
//
//   project   uh[b, t, k, :] = routing.weight[t, k] e[b, t].  The matrix differs for every position, so this is T GEMMs whose
//             M dimension is the batch: a workgroup owns one position, 32 sequences and 64 of the K D output columns; the 32
//             rows e[., t] are gathered straight from the table into LDS once, routing.weight[t] passes through LDS in
//             K-slabs of 32, the product runs on v_mfma_f32_16x16x4_f32.  Padding rows are zeros and are not read; a tile of
//             padding only (the early positions of a left-padded batch) stores zeros without a product.
//   route     one workgroup per sequence, all R iterations in one launch.  Logits and couplings [K, T] live in LDS (16 KB),
//             s / v [K, D] too (4 KB); uh is streamed from memory 2 R - 1 times and never held: LDS does not grow with T D.
//             Weighted sum: a thread owns one of the K D columns (coalesced over the columns); when K D < 256 the positions
//             are dealt to 256 / (K D) thread groups whose partial sums are folded in group order.  Squash: a wave per
//             interest.  Logit update: 16 lanes per position, 16 positions per trip, its K dot products by a 4-step shuffle sum.
//             Padded positions are skipped in both passes (their coupling is 0).
//   readout   one wave per row: k* = argmax_k <v[k], E[target]>, readout = v[k*], z_0; one wave per sample: its row of the
//             table and its logQ shift, which rides in the logit GEMM as the column bias
//   logits    Z [B, S] = readout O^T + ob through the grouped GEMM
//   loss      one wave per row (GRU4Rec's softmax stage): accidental-hit mask, log-sum-exp over z_0 and the row, the loss
//             term into the block's partial, d Z written over Z, d z_0 beside it
//   d logits  one grouped launch: d readout = dZ O, dO = dZ^T readout (a block per tile walks the whole batch: no split-K)
//   squash'   one wave per row: d v[k*] -> d s, with s recovered from v and n; target and sample rows into d item_emb
//   rows      the rows that chose interest k, ascending, as K lists (ballot + popcount, one wave per interest)
//   d weight  d routing.weight[t, k] = sum over list k of c[b, k, t] (d s_b outer e[b, t]): a workgroup owns (t, k) and a
//             64 x 64 tile and walks the list in slabs of 32 rows; the left operand c d s is formed while it is staged, so no
//             [B, T, K, D] gradient exists, and because the rows are listed per interest a row is multiplied once, not K times
//   d e       d e[b, t] = c[b, k*, t] routing.weight[t, k*]^T d s_b: a workgroup owns (t, k) and one slab of the list; the
//             result leaves the accumulators as row atomics into d item_emb
//
// 10 launches when training, 2 in the eval forward.  The only float atomics are the rows of d item_emb.weight; d
// routing.weight is the same bits on every run.  A separate kernel merges the K top-k lists of a sequence (recommend_next).
#include <algorithm>

#include "gemm.hpp"
#include "seqrec.hpp"

namespace hiprec {
namespace {

constexpr int kCrMaxDim = 128, kCrMaxLen = 256, kCrMaxInterest = 8, kCrMaxIters = 4, kCrMaxSample = 8192;
constexpr int64_t kCrMaxRows = 1ll << 24;      // batch x maxlen
constexpr int kCrPM = 32;                      // project: sequences of a workgroup
constexpr int kCrPN = 64;                      // project: output columns of a workgroup
constexpr int kCrPK = 32;                      // project: K-slab of routing.weight[t] in LDS
constexpr int kCrLdE = kCrMaxDim + 1;
constexpr int kCrSlab = 32;                    // backward: rows of one interest's list per slab
constexpr int kCrLdT = 80;                     // 64-wide LDS tiles read along the slab: 16 mod 32 banks apart
constexpr int kCrLdW = kCrMaxDim + 16;
constexpr int kCrMaxTopk = 128;                // HIPREC_TOPK_MAX_K

struct CrDims {
  int64_t n_items;
  int D, T, K, R;
};

// ---- project ---------------------------------------------------------------------------------------------------------------
// grid (T, ceil(B / 32), ceil(K D / 64)).  ids [B, T] index `table` (rows 0 .. max_id); a row is live when mask says so (mask
// given) or when its id is not 0; the z == 0 blocks leave that decision in live [B, T] for the routing.
__global__ __launch_bounds__(kBlock) void comirec_project_kernel(const float* __restrict__ table, int64_t max_id,
                                                                 const int64_t* __restrict__ ids,
                                                                 const uint8_t* __restrict__ mask,
                                                                 const float* __restrict__ W, int B, int T, int KD, int D,
                                                                 float* __restrict__ uh, uint8_t* __restrict__ live,
                                                                 hiprec_stats* stats) {
  __shared__ float Es[kCrPM][kCrLdE];
  __shared__ float Ws[kCrPN][kCrPK + 1];
  __shared__ int64_t s_id[kCrPM];
  const int t = blockIdx.x, b0 = blockIdx.y * kCrPM, n0 = blockIdx.z * kCrPN;
  const int lane = lane_id(), wave = wave_in_block();
  if (threadIdx.x < kCrPM) {
    const int b = b0 + threadIdx.x;
    int64_t id = -1;      // -1: a row of zeros
    if (b < B) {
      const int64_t m = static_cast<int64_t>(b) * T + t, raw = ids[m];
      if (raw < 0 || raw > max_id) {
        atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
      } else if (mask ? mask[m] != 0 : raw != 0) {
        id = raw;
      }
      if (blockIdx.z == 0) live[m] = id >= 0;
    }
    s_id[threadIdx.x] = id;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kCrPM * D; e += kBlock) {
    const int r = e / D, c = e - r * D;
    const int64_t id = s_id[r];
    Es[r][c] = id >= 0 ? table[id * D + c] : 0.f;
  }
  const bool work = __syncthreads_or(s_id[threadIdx.x & (kCrPM - 1)] >= 0);
  f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  if (work) {
    const float* Wt = W + static_cast<int64_t>(t) * KD * D;
    for (int k0 = 0; k0 < D; k0 += kCrPK) {
      __syncthreads();
      for (int e = threadIdx.x; e < kCrPN * kCrPK; e += kBlock) {
        const int c = e / kCrPK, kk = e - c * kCrPK;
        Ws[c][kk] = (n0 + c < KD && k0 + kk < D) ? Wt[static_cast<int64_t>(n0 + c) * D + k0 + kk] : 0.f;
      }
      __syncthreads();
      const int kw = min(kCrPK, D - k0);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int tile = wave * 2 + u, rt = tile >> 2, ct = tile & 3;
        acc[u] = mma16(acc[u], &Es[rt * 16][k0], kCrLdE, 1, &Ws[ct * 16][0], 1, kCrPK + 1, kw);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int tile = wave * 2 + u, rt = tile >> 2, ct = tile & 3;
    const int col = n0 + ct * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + rt * 16 + 4 * (lane >> 4) + r;
      if (b < B && col < KD) uh[(static_cast<int64_t>(b) * T + t) * KD + col] = acc[u][r];
    }
  }
}

// ---- route -----------------------------------------------------------------------------------------------------------------
// grid B.  uh [B, T, K, D], live [B, T]; v_out [B, K, D], c_out [B, K, T], n_out [B, K] of the last iteration.
__global__ __launch_bounds__(kBlock) void comirec_route_kernel(const float* __restrict__ uh, const uint8_t* __restrict__ live,
                                                               int T, int K, int D, int R, float* __restrict__ v_out,
                                                               float* __restrict__ c_out, float* __restrict__ n_out) {
  __shared__ float bl[kCrMaxInterest][kCrMaxLen];      // routing logits
  __shared__ float cl[kCrMaxInterest][kCrMaxLen];      // couplings
  __shared__ float part[kBlock];
  __shared__ float sv[kCrMaxInterest * kCrMaxDim];     // s, then v
  __shared__ float nn[kCrMaxInterest];
  const int b = blockIdx.x, KD = K * D, tid = threadIdx.x;
  const int lane = lane_id(), wave = wave_in_block();
  const float* u = uh + static_cast<int64_t>(b) * T * KD;
  const uint8_t* lv = live + static_cast<int64_t>(b) * T;
  for (int k = 0; k < K; ++k)
    for (int t = tid; t < T; t += kBlock) bl[k][t] = 0.f;
  // the weighted sum's split: CW columns in a pass, G groups of positions (G > 1 only when every column fits one pass)
  const int CW = min(KD, kBlock), G = kBlock / CW, g = tid / CW, c0 = tid - g * CW;
  for (int r = 0; r < R; ++r) {
    __syncthreads();
    for (int t = tid; t < T; t += kBlock) {
      float m = -INFINITY, z = 0.f;
#pragma unroll 1
      for (int k = 0; k < K; ++k) m = fmaxf(m, bl[k][t]);
#pragma unroll 1
      for (int k = 0; k < K; ++k) {
        const float e = expf(bl[k][t] - m);
        cl[k][t] = e;
        z += e;
      }
      const float inv = lv[t] ? 1.f / z : 0.f;
#pragma unroll 1
      for (int k = 0; k < K; ++k) cl[k][t] *= inv;
    }
    __syncthreads();
    if (g < G) {
#pragma unroll 1
      for (int j = 0; j < kCrMaxInterest * kCrMaxDim / kBlock; ++j) {
        const int col = c0 + j * CW;
        if (col >= KD) break;
        const float* ck = cl[col / D];
        float a = 0.f;
        for (int t = g; t < T; t += G) {
          const float cc = ck[t];
          if (cc != 0.f) a = fmaf(cc, u[static_cast<int64_t>(t) * KD + col], a);
        }
        if (G > 1) part[tid] = a; else sv[col] = a;
      }
    }
    __syncthreads();
    if (G > 1 && tid < KD) {
      float a = 0.f;
      for (int gg = 0; gg < G; ++gg) a += part[gg * CW + tid];
      sv[tid] = a;
    }
    __syncthreads();
    for (int k = wave; k < K; k += kWavesPerBlock) {
      float q = 0.f;
      for (int d = lane; d < D; d += kWave) q = fmaf(sv[k * D + d], sv[k * D + d], q);
      const float n = wave_sum(q);
      const float f = n / (1.f + n) / sqrtf(n + 1e-9f);
      for (int d = lane; d < D; d += kWave) sv[k * D + d] *= f;
      if (lane == 0) nn[k] = n;
    }
    __syncthreads();
    if (r == R - 1) break;
    const int grp = tid >> 4, l16 = tid & 15;
    for (int t = grp; t < T; t += kBlock / 16) {      // 16 positions per trip, the K pairs of one in turn
      if (!lv[t]) continue;
      for (int k = 0; k < K; ++k) {
        float a = 0.f;
        for (int d = l16; d < D; d += 16) a = fmaf(u[static_cast<int64_t>(t) * KD + k * D + d], sv[k * D + d], a);
        a += __shfl_xor(a, 8, 16);
        a += __shfl_xor(a, 4, 16);
        a += __shfl_xor(a, 2, 16);
        a += __shfl_xor(a, 1, 16);
        if (l16 == 0) bl[k][t] += a;
      }
    }
  }
  for (int e = tid; e < KD; e += kBlock) v_out[static_cast<int64_t>(b) * KD + e] = sv[e];
  for (int k = 0; k < K; ++k)
    for (int t = tid; t < T; t += kBlock) c_out[(static_cast<int64_t>(b) * K + k) * T + t] = cl[k][t];
  if (tid < K) n_out[static_cast<int64_t>(b) * K + tid] = nn[tid];
}

// ---- readout, loss, squash' ------------------------------------------------------------------------------------------------
// waves [0, B): k*, readout and z_0 of a row (k* = -1: no label); waves [B, B + S): a sample's row of the table and its shift
__global__ __launch_bounds__(kBlock) void comirec_readout_kernel(const float* __restrict__ E, int64_t n_items,
                                                                 const float* __restrict__ v,
                                                                 const int64_t* __restrict__ target,
                                                                 const int64_t* __restrict__ samples,
                                                                 const float* __restrict__ log_q, int B, int S, int K, int D,
                                                                 int* __restrict__ kstar, float* __restrict__ readout,
                                                                 float* __restrict__ z0, float* __restrict__ O,
                                                                 float* __restrict__ ob, hiprec_stats* stats) {
  const int lane = lane_id();
  for (int w = blockIdx.x * kWavesPerBlock + wave_in_block(); w < B + S; w += gridDim.x * kWavesPerBlock) {
    if (w < B) {
      const int64_t id = target[w];
      const bool ok = id >= 1 && id <= n_items;
      if (lane == 0 && (id < 0 || id > n_items)) atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
      int best = -1;
      float bz = 0.f;
      if (ok) {
        const float e0 = lane < D ? E[id * D + lane] : 0.f, e1 = lane + kWave < D ? E[id * D + lane + kWave] : 0.f;
        for (int k = 0; k < K; ++k) {
          const float* vk = v + (static_cast<int64_t>(w) * K + k) * D;
          float a = lane < D ? vk[lane] * e0 : 0.f;
          if (lane + kWave < D) a = fmaf(vk[lane + kWave], e1, a);
          const float z = wave_sum(a);
          if (best < 0 || z > bz) {      // the lowest k on a tie
            best = k;
            bz = z;
          }
        }
      }
      if (lane == 0) {
        kstar[w] = best;
        z0[w] = ok ? bz - (log_q ? log_q[id] : 0.f) : 0.f;
      }
      for (int d = lane; d < D; d += kWave)
        readout[static_cast<int64_t>(w) * D + d] = ok ? v[(static_cast<int64_t>(w) * K + best) * D + d] : 0.f;
    } else {
      const int j = w - B;
      const int64_t id = samples[j];
      const bool ok = id >= 1 && id <= n_items;
      if (lane == 0) {
        if (!ok) atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
        ob[j] = (ok && log_q) ? -log_q[id] : 0.f;
      }
      for (int d = lane; d < D; d += kWave) O[static_cast<int64_t>(j) * D + d] = ok ? E[id * D + d] : 0.f;
    }
  }
}

// One wave per row of Z [B, S]; d Z is written over Z.  loss = mean over the labelled rows of logsumexp(z) - z_0, where a
// sample equal to the row's target is left out.
__global__ __launch_bounds__(kBlock) void comirec_loss_kernel(float* __restrict__ Z, const float* __restrict__ z0,
                                                              const int* __restrict__ kstar,
                                                              const int64_t* __restrict__ target,
                                                              const int64_t* __restrict__ samples, int B, int S,
                                                              float* __restrict__ dz0, Scratch* scratch, hiprec_stats* stats) {
  __shared__ float s_cnt[kWavesPerBlock];
  const int lane = lane_id(), wave = wave_in_block();
  float cnt = 0.f;      // every block counts the labelled rows itself (exact: B < 2^24)
  for (int i = threadIdx.x; i < B; i += kBlock) cnt += kstar[i] >= 0 ? 1.f : 0.f;
  cnt = wave_sum(cnt);
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  cnt = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
  const float inv = cnt > 0.f ? 1.f / cnt : 0.f;
  float loss_w = 0.f;
  for (int i = blockIdx.x * kWavesPerBlock + wave; i < B; i += gridDim.x * kWavesPerBlock) {
    float* row = Z + static_cast<int64_t>(i) * S;
    if (kstar[i] < 0) {
      for (int j = lane; j < S; j += kWave) row[j] = 0.f;
      if (lane == 0) dz0[i] = 0.f;
      continue;
    }
    const int64_t tg = target[i];
    const float a0 = z0[i];
    float m = a0;
    for (int j = lane; j < S; j += kWave)
      if (samples[j] != tg) m = fmaxf(m, row[j]);
    m = wave_max(m);
    float zs = 0.f;
    for (int j = lane; j < S; j += kWave)
      if (samples[j] != tg) zs += expf(row[j] - m);
    const float e0 = expf(a0 - m), Zs = wave_sum(zs) + e0;
    loss_w += m + logf(Zs) - a0;
    for (int j = lane; j < S; j += kWave) row[j] = samples[j] != tg ? expf(row[j] - m) / Zs * inv : 0.f;
    if (lane == 0) dz0[i] = (e0 / Zs - 1.f) * inv;
  }
  publish_partials<kWavesPerBlock>(loss_w * inv, 0.f, 0.f, 1.0f, scratch);
  if (blockIdx.x == 0 && threadIdx.x == 0) advance_step(stats);
}

// waves [0, B): d v[k*] = d readout + d z_0 E[target] through the squash to d s [B, D] (s = v / f(n), v = s f(n),
// f = n / (1 + n) / sqrt(n + 1e-9)), and d z_0 readout into the target's row; waves [B, B + S): dO[j] into the sample's row
__global__ __launch_bounds__(kBlock) void comirec_squash_bwd_kernel(const float* __restrict__ E, int64_t n_items,
                                                                    const float* __restrict__ readout,
                                                                    const float* __restrict__ dread,
                                                                    const float* __restrict__ dz0,
                                                                    const float* __restrict__ nsq,
                                                                    const int* __restrict__ kstar,
                                                                    const int64_t* __restrict__ target,
                                                                    const int64_t* __restrict__ samples,
                                                                    const float* __restrict__ dO, int B, int S, int K, int D,
                                                                    float* __restrict__ ds, float* __restrict__ g_item) {
  const int lane = lane_id();
  for (int w = blockIdx.x * kWavesPerBlock + wave_in_block(); w < B + S; w += gridDim.x * kWavesPerBlock) {
    if (w < B) {
      const int k = kstar[w];
      float* out = ds + static_cast<int64_t>(w) * D;
      if (k < 0) {
        for (int d = lane; d < D; d += kWave) out[d] = 0.f;
        continue;
      }
      const int64_t id = target[w];
      const float g0 = dz0[w], n = nsq[static_cast<int64_t>(w) * K + k];
      const float f = n / (1.f + n) / sqrtf(n + 1e-9f);
      float vv[2], dv[2], dot = 0.f;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int d = lane + h * kWave;
        vv[h] = dv[h] = 0.f;
        if (d < D) {
          vv[h] = readout[static_cast<int64_t>(w) * D + d];
          dv[h] = fmaf(g0, E[id * D + d], dread[static_cast<int64_t>(w) * D + d]);
          const float gt = g0 * vv[h];
          if (gt != 0.f) atomic_add_f32(g_item + id * D + d, gt);
          dot = fmaf(vv[h], dv[h], dot);
        }
      }
      // d s = f d v + 2 f'(n) <s, d v> s with s = v / f: 2 (f' / f) / f <v, d v> v.  An interest the routing has starved
      // (c ~ e^-50) can still be the nearest one when every other score is negative: below n = 1e-18 the second term is
      // under 1e-13 |d v| and is dropped, because f^2 is no float32 number any more.
      const float vdv = wave_sum(dot);
      const float coef = n > 1e-18f ? 2.f * (1.f / (n * (1.f + n)) - 0.5f / (n + 1e-9f)) / f * vdv : 0.f;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int d = lane + h * kWave;
        if (d < D) out[d] = fmaf(coef, vv[h], f * dv[h]);
      }
    } else {
      const int j = w - B;
      const int64_t id = samples[j];
      if (id < 1 || id > n_items) continue;
      for (int d = lane; d < D; d += kWave) {
        const float gv = dO[static_cast<int64_t>(j) * D + d];
        if (gv != 0.f) atomic_add_f32(g_item + id * D + d, gv);
      }
    }
  }
}

// ---- backward of the routing's last weighted sum and of the projection -----------------------------------------------------
// one block; wave w lists the rows with k* == w, w + 4 in ascending order: list [K, B], count [K]
__global__ __launch_bounds__(kBlock) void comirec_rows_kernel(const int* __restrict__ kstar, int B, int K,
                                                              int* __restrict__ list, int* __restrict__ count) {
  const int lane = lane_id();
  for (int k = wave_in_block(); k < K; k += kWavesPerBlock) {
    int n = 0;
    for (int b0 = 0; b0 < B; b0 += kWave) {
      const int b = b0 + lane;
      const bool hit = b < B && kstar[b] == k;
      const uint64_t m = __ballot(hit);
      if (hit) list[static_cast<int64_t>(k) * B + n + __popcll(m & ((1ull << lane) - 1ull))] = b;
      n += __popcll(m);
    }
    if (lane == 0) count[k] = n;
  }
}

// grid (T K, ceil(D / 64), ceil(D / 64)): the tile [i0, i0 + 64) x [j0, j0 + 64) of d routing.weight[t, k]
__global__ __launch_bounds__(kBlock) void comirec_wgrad_kernel(const float* __restrict__ E, const int64_t* __restrict__ seq,
                                                               const float* __restrict__ c, const float* __restrict__ ds,
                                                               const int* __restrict__ list, const int* __restrict__ count,
                                                               int B, int T, int K, int D, float* __restrict__ gW) {
  __shared__ float As[kCrSlab][kCrLdT];      // c d s: [row of the slab][i]
  __shared__ float Xs[kCrSlab][kCrLdT];      // e: [row of the slab][j]
  const int t = blockIdx.x / K, k = blockIdx.x - t * K, i0 = blockIdx.y * 64, j0 = blockIdx.z * 64;
  const int lane = lane_id(), wave = wave_in_block();
  const int n = count[k];
  const int* rows = list + static_cast<int64_t>(k) * B;
  f32x4 acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int r0 = 0; r0 < n; r0 += kCrSlab) {
    __syncthreads();
    int any = 0;
    for (int e = threadIdx.x; e < kCrSlab * 64; e += kBlock) {
      const int rr = e >> 6, cc = e & 63;
      float a = 0.f, x = 0.f;
      if (r0 + rr < n) {
        const int b = rows[r0 + rr];
        const float coef = c[(static_cast<int64_t>(b) * K + k) * T + t];
        if (coef != 0.f) {      // a live position: its id is in the table
          if (i0 + cc < D) a = coef * ds[static_cast<int64_t>(b) * D + i0 + cc];
          if (j0 + cc < D) x = E[seq[static_cast<int64_t>(b) * T + t] * D + j0 + cc];
          any = 1;
        }
      }
      As[rr][cc] = a;
      Xs[rr][cc] = x;
    }
    if (!__syncthreads_or(any)) continue;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      acc[u] = mma16(acc[u], &As[0][wave * 16], 1, kCrLdT, &Xs[0][u * 16], kCrLdT, 1, kCrSlab);
  }
  float* out = gW + (static_cast<int64_t>(t) * K + k) * D * D;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int j = j0 + u * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + wave * 16 + 4 * (lane >> 4) + r;
      if (i < D && j < D) out[static_cast<int64_t>(i) * D + j] = acc[u][r];
    }
  }
}

// grid (T K, ceil(B / 32)): slab y of list k at position t; rows of d e leave as atomics into d item_emb
__global__ __launch_bounds__(kBlock) void comirec_dgrad_kernel(const float* __restrict__ W, const int64_t* __restrict__ seq,
                                                               const float* __restrict__ c, const float* __restrict__ ds,
                                                               const int* __restrict__ list, const int* __restrict__ count,
                                                               int B, int T, int K, int D, float* __restrict__ g_item) {
  __shared__ float As[kCrSlab][kCrLdE];      // c d s: [row of the slab][i]
  __shared__ float Ws[kCrPK][kCrLdW];        // routing.weight[t, k][i slab][j]
  __shared__ int64_t s_id[kCrSlab];
  __shared__ float s_c[kCrSlab];
  const int t = blockIdx.x / K, k = blockIdx.x - t * K, r0 = blockIdx.y * kCrSlab;
  const int lane = lane_id(), wave = wave_in_block();
  const int n = count[k];
  if (r0 >= n) return;
  const int* rows = list + static_cast<int64_t>(k) * B;
  if (threadIdx.x < kCrSlab) {
    float coef = 0.f;
    int64_t id = 0;
    if (r0 + threadIdx.x < n) {
      const int b = rows[r0 + threadIdx.x];
      coef = c[(static_cast<int64_t>(b) * K + k) * T + t];
      if (coef != 0.f) id = seq[static_cast<int64_t>(b) * T + t];
    }
    s_c[threadIdx.x] = coef;
    s_id[threadIdx.x] = id;
  }
  if (!__syncthreads_or(threadIdx.x < kCrSlab && s_c[threadIdx.x] != 0.f)) return;
  for (int e = threadIdx.x; e < kCrSlab * D; e += kBlock) {
    const int rr = e / D, i = e - rr * D;
    const float coef = s_c[rr];
    As[rr][i] = coef != 0.f ? coef * ds[static_cast<int64_t>(rows[r0 + rr]) * D + i] : 0.f;
  }
  const float* Wk = W + (static_cast<int64_t>(t) * K + k) * D * D;
  const int rt = wave >> 1, n_ct = D / 16;
  f32x4 acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i0 = 0; i0 < D; i0 += kCrPK) {
    __syncthreads();
    for (int e = threadIdx.x; e < kCrPK * D; e += kBlock) {
      const int ii = e / D, j = e - ii * D;
      Ws[ii][j] = i0 + ii < D ? Wk[static_cast<int64_t>(i0 + ii) * D + j] : 0.f;
    }
    __syncthreads();
    const int kw = min(kCrPK, D - i0);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ct = (wave & 1) + 2 * u;
      if (ct < n_ct) acc[u] = mma16(acc[u], &As[rt * 16][i0], kCrLdE, 1, &Ws[0][ct * 16], kCrLdW, 1, kw);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int ct = (wave & 1) + 2 * u;
    if (ct >= n_ct) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t id = s_id[rt * 16 + 4 * (lane >> 4) + r];
      if (id > 0 && acc[u][r] != 0.f) atomic_add_f32(g_item + id * D + ct * 16 + (lane & 15), acc[u][r]);
    }
  }
}

// ---- multi-interest top-k merge ------------------------------------------------------------------------------------------
// One wave per sequence.  items / scores [n K, k]: per interest the k best, best first (ties to the lower id), -1 / -inf
// tails.  Lane l < K holds the head of list l; every turn the best head (highest score, then lowest id) is taken unless the
// item was taken before (lane e keeps the e-th and (e + 64)-th taken item), and every list whose head is that item moves on.
__global__ __launch_bounds__(kBlock) void comirec_merge_kernel(const int64_t* __restrict__ items,
                                                               const float* __restrict__ scores, int64_t n, int K, int k,
                                                               int64_t* __restrict__ out_items,
                                                               float* __restrict__ out_scores) {
  const int lane = lane_id();
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); q < n;
       q += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    int head = 0, taken = 0;
    long long kept0 = -1, kept1 = -1;
    while (taken < k) {
      float sc = -INFINITY;
      long long it = -1;
      if (lane < K && head < k) {
        const int64_t at = (q * K + lane) * k + head;
        it = items[at];
        if (it >= 0) sc = scores[at];
      }
      float bs = sc;
      long long bi = it;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float os = __shfl_xor(bs, o, kWave);
        const long long oi = __shfl_xor(bi, o, kWave);
        if (oi >= 0 && (bi < 0 || os > bs || (os == bs && oi < bi))) {
          bs = os;
          bi = oi;
        }
      }
      if (bi < 0) break;      // every list is used up
      const bool dup = (lane < taken && kept0 == bi) || (lane + kWave < taken && kept1 == bi);
      if (lane < K && it == bi) ++head;
      if (__ballot(dup) == 0ull) {
        if (lane == taken) kept0 = bi;
        if (lane + kWave == taken) kept1 = bi;
        if (lane == 0) {
          out_items[q * k + taken] = bi;
          out_scores[q * k + taken] = bs;
        }
        ++taken;
      }
    }
    for (int e = taken + lane; e < k; e += kWave) {
      out_items[q * k + e] = -1;
      out_scores[q * k + e] = -INFINITY;
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
int comirec_check_shape(const hiprec_comirec_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  HIPREC_REQUIRE(s->n_items >= 1 && s->n_items < (1ll << 31), "ComiRec needs 1 <= n_items < 2^31, got %lld",
                 static_cast<long long>(s->n_items));
  HIPREC_REQUIRE(s->dim >= 16 && s->dim <= kCrMaxDim && s->dim % 16 == 0,
                 "ComiRec needs emb_dim a multiple of 16 in 16 .. %d (got %d)", kCrMaxDim, s->dim);
  HIPREC_REQUIRE(s->n_interest >= 1 && s->n_interest <= kCrMaxInterest, "ComiRec needs 1 <= num_interest <= %d (got %d)",
                 kCrMaxInterest, s->n_interest);
  HIPREC_REQUIRE(s->maxlen >= 1 && s->maxlen <= kCrMaxLen, "ComiRec needs 1 <= maxlen <= %d (got %d)", kCrMaxLen, s->maxlen);
  HIPREC_REQUIRE(s->routing_iters >= 1 && s->routing_iters <= kCrMaxIters, "ComiRec needs 1 <= routing_iters <= %d (got %d)",
                 kCrMaxIters, s->routing_iters);
  return 0;
}

CrDims comirec_dims(const hiprec_comirec_shape& s) { return CrDims{s.n_items, s.dim, s.maxlen, s.n_interest, s.routing_iters}; }

bool comirec_batch_ok(const CrDims& q, int64_t B, int64_t S) {
  return B >= 1 && B * q.T <= kCrMaxRows && S >= 0 && S <= kCrMaxSample;
}

struct CrWorkspace {
  float *uh, *v, *c, *nsq, *readout, *z0, *dz0, *O, *ob, *Z, *dread, *dO, *ds;
  int *kstar, *list, *count;
  uint8_t* live;
  int64_t floats;
};

CrWorkspace comirec_carve(float* base, const CrDims& q, int64_t B, int64_t S) {
  CrWorkspace w{};
  float* p = base;
  auto take = [&](int64_t n) { float* r = p; p += (n + 3) / 4 * 4; return r; };
  const int64_t KD = static_cast<int64_t>(q.K) * q.D;
  w.uh = take(B * q.T * KD);
  w.v = take(B * KD);
  w.c = take(B * q.K * q.T);
  w.nsq = take(B * q.K);
  w.live = reinterpret_cast<uint8_t*>(take((B * q.T + 3) / 4));
  w.readout = take(B * q.D);
  w.z0 = take(B);
  w.dz0 = take(B);
  w.kstar = reinterpret_cast<int*>(take(B));
  w.O = take(S * q.D);
  w.ob = take(S);
  w.Z = take(B * S);
  w.dread = take(B * q.D);
  w.dO = take(S * q.D);
  w.ds = take(B * q.D);
  w.list = reinterpret_cast<int*>(take(B * q.K));
  w.count = reinterpret_cast<int*>(take(kCrMaxInterest));
  w.floats = p - base;
  return w;
}

int comirec_project(const float* table, int64_t max_id, const int64_t* ids, const uint8_t* mask, const float* W, int B,
                    int T, int K, int D, float* uh, uint8_t* live, hiprec_stats* stats, hipStream_t st) {
  const int KD = K * D;
  const dim3 grid(T, (B + kCrPM - 1) / kCrPM, (KD + kCrPN - 1) / kCrPN);
  HIPREC_REQUIRE(grid.y <= 65535u, "ComiRec: a call takes at most %d sequences", 65535 * kCrPM);
  comirec_project_kernel<<<grid, kBlock, 0, st>>>(table, max_id, ids, mask, W, B, T, KD, D, uh, live, stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// rows + d routing.weight + d e from d s [B, D], k* [B] and c [B, K, T]
int comirec_backward(const float* W, const float* E, const int64_t* seq, const float* c, const float* ds, const int* kstar,
                     int B, int T, int K, int D, int* list, int* count, float* gW, float* g_item, hipStream_t st) {
  HIPREC_REQUIRE((B + kCrSlab - 1) / kCrSlab <= 65535, "ComiRec: a call takes at most %d sequences", 65535 * kCrSlab);
  comirec_rows_kernel<<<1, kBlock, 0, st>>>(kstar, B, K, list, count);
  HIPREC_TRY(hipGetLastError());
  const int dt = (D + 63) / 64;
  comirec_wgrad_kernel<<<dim3(T * K, dt, dt), kBlock, 0, st>>>(E, seq, c, ds, list, count, B, T, K, D, gW);
  HIPREC_TRY(hipGetLastError());
  comirec_dgrad_kernel<<<dim3(T * K, (B + kCrSlab - 1) / kCrSlab), kBlock, 0, st>>>(W, seq, c, ds, list, count, B, T, K, D,
                                                                                    g_item);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

int comirec_run(const CrDims& q, float* w_flat, float* g_flat, const int64_t* seq, const int64_t* target,
                const int64_t* samples, int B, int S, const float* log_q, float* interests_out, int32_t* kstar_out,
                hiprec_stats* stats, Scratch* scratch, float* ws_base, hipStream_t st) {
  const int T = q.T, K = q.K, D = q.D;
  const CrWorkspace a = comirec_carve(ws_base, q, B, S);
  float* E = w_flat;
  float* W = w_flat + (q.n_items + 1) * D;
  const bool train = g_flat != nullptr;
  if (int rc = comirec_project(E, q.n_items, seq, nullptr, W, B, T, K, D, a.uh, a.live, stats, st)) return rc;
  float* v = (!train && interests_out) ? interests_out : a.v;
  comirec_route_kernel<<<B, kBlock, 0, st>>>(a.uh, a.live, T, K, D, q.R, v, a.c, a.nsq);
  HIPREC_TRY(hipGetLastError());
  if (!train) return 0;
  if (interests_out) HIPREC_TRY(hipMemcpyAsync(interests_out, v, sizeof(float) * static_cast<size_t>(B) * K * D, hipMemcpyDeviceToDevice, st));

  comirec_readout_kernel<<<grid_for_waves(B + S), kBlock, 0, st>>>(E, q.n_items, v, target, samples, log_q, B, S, K, D,
                                                                   a.kstar, a.readout, a.z0, a.O, a.ob, stats);
  HIPREC_TRY(hipGetLastError());
  if (kstar_out) HIPREC_TRY(hipMemcpyAsync(kstar_out, a.kstar, sizeof(int) * B, hipMemcpyDeviceToDevice, st));
  {
    GemmGroup p{};
    p.n = 1;
    p.p[0] = make_gemm(kNT, B, S, D, a.readout, D, a.O, D, a.Z, S, a.ob, 0, nullptr, 0, false);
    if (int rc = launch_group(p, st)) return rc;
  }
  comirec_loss_kernel<<<grid_for_waves(B), kBlock, 0, st>>>(a.Z, a.z0, a.kstar, target, samples, B, S, a.dz0, scratch, stats);
  HIPREC_TRY(hipGetLastError());
  {
    GemmGroup p{};
    p.n = 2;
    p.p[0] = make_gemm(kNN, B, D, S, a.Z, S, a.O, D, a.dread, D, nullptr, 0, nullptr, 0, false);
    p.p[1] = make_gemm(kTNm, S, D, B, a.Z, S, a.readout, D, a.dO, D, nullptr, 0, nullptr, 0, false);
    if (int rc = launch_group(p, st)) return rc;
  }
  float* g_item = g_flat;
  float* gW = g_flat + (q.n_items + 1) * D;
  comirec_squash_bwd_kernel<<<grid_for_waves(B + S), kBlock, 0, st>>>(E, q.n_items, a.readout, a.dread, a.dz0, a.nsq, a.kstar,
                                                                      target, samples, a.dO, B, S, K, D, a.ds, g_item);
  HIPREC_TRY(hipGetLastError());
  return comirec_backward(W, E, seq, a.c, a.ds, a.kstar, B, T, K, D, a.list, a.count, gW, g_item, st);
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_comirec_shape_bytes(void) { return sizeof(hiprec_comirec_shape); }

extern "C" int64_t hiprec_comirec_param_floats(const hiprec_comirec_shape* shape) {
  if (comirec_check_shape(shape)) return -1;
  const CrDims q = comirec_dims(*shape);
  return (q.n_items + 1) * q.D + static_cast<int64_t>(q.T) * q.K * q.D * q.D;
}

extern "C" size_t hiprec_comirec_workspace_bytes(const hiprec_comirec_shape* shape, int64_t batch, int32_t n_sample) {
  if (comirec_check_shape(shape)) return 0;
  const CrDims q = comirec_dims(*shape);
  if (!comirec_batch_ok(q, batch, n_sample)) return 0;
  return sizeof(float) * static_cast<size_t>(comirec_carve(nullptr, q, batch, n_sample).floats);
}

extern "C" int hiprec_comirec_grad(const hiprec_comirec_shape* shape, const float* w_flat, float* g_flat, const int64_t* seq,
                                   const int64_t* target, const int64_t* samples, int64_t batch, int32_t n_sample,
                                   const float* log_q, float* interests_out, int32_t* kstar_out, hiprec_stats* stats,
                                   void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  if (int rc = comirec_check_shape(shape)) return rc;
  const CrDims q = comirec_dims(*shape);
  HIPREC_REQUIRE(w_flat && seq && stats && workspace, "NULL pointer");
  if (!g_flat) n_sample = 0;
  HIPREC_REQUIRE(comirec_batch_ok(q, batch, n_sample),
                 "ComiRec needs batch >= 1, batch * maxlen <= 2^24 and 0 <= n_sample <= %d (got %lld, %d)", kCrMaxSample,
                 static_cast<long long>(batch), n_sample);
  if (g_flat) {
    HIPREC_REQUIRE(n_sample >= 1, "ComiRec: the sampled softmax needs 1 <= n_sample <= %d", kCrMaxSample);
    HIPREC_REQUIRE(target && samples && scratch, "training needs the targets, the samples and the scratch block");
    if (scratch_bytes < kScratchBytes) {
      set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
      return HIPREC_E_SCRATCH;
    }
  } else {
    HIPREC_REQUIRE(interests_out, "the eval forward needs the interests buffer");
  }
  const size_t need = hiprec_comirec_workspace_bytes(shape, batch, n_sample);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  return comirec_run(q, const_cast<float*>(w_flat), g_flat, seq, target, samples, static_cast<int>(batch), n_sample, log_q,
                     interests_out, kstar_out, stats, static_cast<Scratch*>(scratch), static_cast<float*>(workspace),
                     static_cast<hipStream_t>(stream));
}

static int comirec_stage_ok(int64_t batch, int32_t seq_len, int32_t n_interest, int32_t dim) {
  HIPREC_REQUIRE(dim >= 16 && dim <= kCrMaxDim && dim % 16 == 0 && n_interest >= 1 && n_interest <= kCrMaxInterest &&
                     seq_len >= 1 && seq_len <= kCrMaxLen && batch >= 1 && batch * seq_len <= kCrMaxRows,
                 "ComiRec stage: dim a multiple of 16 up to %d, 1 .. %d interests, seq_len up to %d, batch * seq_len <= 2^24",
                 kCrMaxDim, kCrMaxInterest, kCrMaxLen);
  return 0;
}

extern "C" int hiprec_comirec_project(const float* weight, const float* rows, int64_t n_rows, const int64_t* ids,
                                      const uint8_t* mask, int64_t batch, int32_t seq_len, int32_t n_interest, int32_t dim,
                                      float* uh, uint8_t* live, hiprec_stats* stats, void* stream) {
  if (int rc = comirec_stage_ok(batch, seq_len, n_interest, dim)) return rc;
  HIPREC_REQUIRE(weight && rows && ids && uh && live && stats && n_rows >= 1, "NULL pointer");
  return comirec_project(rows, n_rows - 1, ids, mask, weight, static_cast<int>(batch), seq_len, n_interest, dim, uh, live,
                         stats, static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_comirec_route(const float* uh, const uint8_t* live, int64_t batch, int32_t seq_len, int32_t n_interest,
                                    int32_t dim, int32_t iters, float* interests, float* c, float* nsq, void* stream) {
  if (int rc = comirec_stage_ok(batch, seq_len, n_interest, dim)) return rc;
  HIPREC_REQUIRE(iters >= 1 && iters <= kCrMaxIters, "ComiRec needs 1 <= routing_iters <= %d (got %d)", kCrMaxIters, iters);
  HIPREC_REQUIRE(uh && live && interests && c && nsq, "NULL pointer");
  comirec_route_kernel<<<static_cast<int>(batch), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      uh, live, seq_len, n_interest, dim, iters, interests, c, nsq);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_comirec_backward(const hiprec_comirec_shape* shape, const float* w_flat, float* g_flat,
                                       const int64_t* seq, const float* c, const float* ds, const int32_t* kstar,
                                       int64_t batch, int32_t* lists, void* stream) {
  if (int rc = comirec_check_shape(shape)) return rc;
  const CrDims q = comirec_dims(*shape);
  HIPREC_REQUIRE(w_flat && g_flat && seq && c && ds && kstar && lists, "NULL pointer");
  HIPREC_REQUIRE(comirec_batch_ok(q, batch, 0), "ComiRec needs batch >= 1 and batch * maxlen <= 2^24");
  const int64_t off = (q.n_items + 1) * q.D;
  return comirec_backward(w_flat + off, w_flat, seq, c, ds, kstar, static_cast<int>(batch), q.T, q.K, q.D,
                          lists + kCrMaxInterest, lists, g_flat + off, g_flat, static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_comirec_merge(const int64_t* items, const float* scores, int64_t n, int32_t n_interest, int32_t k,
                                    int64_t* out_items, float* out_scores, void* stream) {
  HIPREC_REQUIRE(items && scores && out_items && out_scores, "NULL pointer");
  HIPREC_REQUIRE(n >= 1 && n_interest >= 1 && n_interest <= kCrMaxInterest && k >= 1 && k <= kCrMaxTopk,
                 "ComiRec merge: 1 .. %d interests and 1 <= k <= %d", kCrMaxInterest, kCrMaxTopk);
  comirec_merge_kernel<<<grid_for_waves(n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(items, scores, n, n_interest, k,
                                                                                          out_items, out_scores);
  HIPREC_TRY(hipGetLastError());
  return 0;
}
