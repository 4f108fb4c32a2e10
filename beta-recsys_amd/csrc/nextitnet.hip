// NextItNet (Yuan et al., WSDM 2019; no counterpart in the reference, the definition is include/hiprec.h's): zero_grad +
// forward + loss + backward of one training step as a fixed sequence of launches, no host sync.
// Activations are [M = B * T, D] row-major, row m = b * T + t.  All matrix products are exact fp32 on
// v_mfma_f32_16x16x4_f32 with both operands in LDS.
//
//   embed               x_0 = E[seq] (seq_embed without scale or positional row; row 0 of E is zero)
//   convolution         nin_conv_kernel<false>: a workgroup owns kNinTimeTile positions of ONE sequence and all D output
//                       columns.  Tap j is one pass over the same accumulators: the input rows t - (k-1-j) d of this
//                       sequence are staged in LDS (zeros where that is < 0: a row of the neighbouring sequence is never
//                       read) and the tap's D x D slab streams through LDS kNinColChunk output columns at a time.  The
//                       epilogue puts the [32, D] tile + bias into LDS and a wave per row computes mean / rstd, the affine,
//                       the ReLU and (conv2) the residual add; stored: the pre-norm row, (mean, rstd) and the output.
//   input gradient      nin_conv_kernel<true>: the same kernel with the shift sign flipped (rows s + (k-1-j) d, zeros past
//                       T - 1) and the slab read through swapped strides (W_j^T); its epilogue adds the residual's
//                       gradient.  In front of it nin_ln_bwd_kernel (a wave per row) goes through the ReLU mask and the
//                       LayerNorm; d gamma, d beta, d conv-bias are fixed-order two-level column sums.
//   weight gradient     nin_wgrad_kernel: block (tap, slab) walks the row tiles slab, slab + slabs, ... of the flattened
//                       [M, D] rows; the x rows are shifted by the tap and masked where t - shift < 0; the [D, D] partial
//                       stays in accumulators and goes to part[slab][tap]; nin_wfold_kernel adds the slabs in slab order
//                       into conv.weight's [D, D, 1, k] layout.  No atomics.
//   final_layer         grouped GEMM (forward; dgrad + wgrad + bias column sum in one launch)
//   loss                nin_labels_kernel (one block) compacts the labelled rows in ascending order and counts them on the
//                       device; cross-entropy over items 1 .. n_items against the tied table in 32 x 64 tiles with a
//                       running max / sum, the catalogue cut into splits that are folded in order; the backward recomputes
//                       p = exp(score - lse) twice: the row-tile owner writes d f, the item-tile owner writes
//                       d E[1 .. n_items] with plain stores.  No [n_lab, n_items] buffer exists.  Every grid is sized by
//                       the most rows a batch can label and the surplus tiles fall out on the device's count.
//   embed backward      row atomics into d E (after the loss's plain stores), id 0 skipped
//   weight decay        g += l2 * w over the whole flat buffer
//
// Every gradient except item_emb.weight is the same bits on every run.
#include <algorithm>

#include "gemm.hpp"
#include "nextitnet.hpp"
#include "seqrec.hpp"

namespace hiprec {
namespace {

constexpr int kNinLd = kSeqMaxDim + 1;      // LDS row stride of every [rows, D] tile (odd: rows 16 apart hit 16 banks)

struct NinTaps {
  int n;                          // kernel_size
  int shift[kNinMaxKernel];       // (k - 1 - j) * dilation, clamped to T (a tap that far back reads nothing)
};

// ---- the shifted-row product ---------------------------------------------------------------------------------------------
// out[b, t, n] = sum_j sum_kk in[b, t -/+ shift_j, kk] * W[n * sn + kk * sk + j]
//   BWD = false: -, (sn, sk) = (D k, k): the causal convolution; epilogue bias + LayerNorm + ReLU (+ resid)
//   BWD = true : +, (sn, sk) = (k, D k): its transpose, the input gradient; epilogue + add
// grid = B * ceil(T / kNinTimeTile).  LDS: Xs [32][kNinLd] the shifted rows of one tap, Bs [32][kNinLd] the chunk of the
// slab as Bs[n][kk]; Bs holds the output tile in the forward's epilogue.  Wave w owns row tile w & 1 and column tile
// w >> 1 of every chunk: acc[c] is its tile of chunk c.
template <bool BWD>
__global__ __launch_bounds__(kBlock) void nin_conv_kernel(
    const float* __restrict__ in, const float* __restrict__ W, int T, int D, NinTaps taps,
    const float* __restrict__ bias, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ resid, float* __restrict__ pre, float* __restrict__ mean, float* __restrict__ rstd,
    float* __restrict__ out) {
  __shared__ float Xs[kNinTimeTile * kNinLd];
  __shared__ float Bs[kNinColChunk * kNinLd];
  constexpr int kMaxChunks = kSeqMaxDim / kNinColChunk;
  const int tiles_t = (T + kNinTimeTile - 1) / kNinTimeTile;
  const int64_t b = blockIdx.x / tiles_t;
  const int t0 = static_cast<int>(blockIdx.x - b * tiles_t) * kNinTimeTile;
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_in_block();
  const int rt = wave & 1, ctl = wave >> 1, n_chunks = (D + kNinColChunk - 1) / kNinColChunk;
  const int ksz = taps.n, sn = BWD ? ksz : D * ksz, sk = BWD ? D * ksz : ksz;
  const float* src = in + b * T * D;
  f32x4 acc[kMaxChunks];
#pragma unroll
  for (int c = 0; c < kMaxChunks; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int j = 0; j < ksz; ++j) {
    const int lo = BWD ? t0 + taps.shift[j] : t0 - taps.shift[j];      // the input row of the tile's first position
    if (lo + kNinTimeTile - 1 < 0 || lo >= T) continue;                 // block-uniform: the whole tap reads zeros
    __syncthreads();
    for (int e = tid; e < kNinTimeTile * D; e += kBlock) {
      const int r = e / D, c = e - r * D, tt = lo + r;
      Xs[r * kNinLd + c] = (tt >= 0 && tt < T && t0 + r < T) ? src[static_cast<int64_t>(tt) * D + c] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c) {
      if (c >= n_chunks) break;
      const int n0 = c * kNinColChunk;
      __syncthreads();
      for (int e = tid; e < kNinColChunk * D; e += kBlock) {
        // consecutive threads walk the dimension that is closest in memory
        const int nl = BWD ? e % kNinColChunk : e / D, kk = BWD ? e / kNinColChunk : e - nl * D;
        const int n = n0 + nl;
        Bs[nl * kNinLd + kk] = n < D ? W[static_cast<int64_t>(n) * sn + static_cast<int64_t>(kk) * sk + j] : 0.f;
      }
      __syncthreads();
      if (n0 + ctl * 16 < D)
        acc[c] = mma16(acc[c], Xs + rt * 16 * kNinLd, kNinLd, 1, Bs + ctl * 16 * kNinLd, 1, kNinLd, D);
    }
  }

  const int64_t m0 = b * T + t0;
  if (BWD) {
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c) {
      const int col = c * kNinColChunk + ctl * 16 + (lane & 15);
      if (c >= n_chunks || col >= D) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = rt * 16 + 4 * (lane >> 4) + q;
        if (t0 + r < T) {
          const int64_t at = (m0 + r) * D + col;
          out[at] = resid ? acc[c][q] + resid[at] : acc[c][q];
        }
      }
    }
    return;
  }
  __syncthreads();      // every wave is done with Bs as an operand
#pragma unroll
  for (int c = 0; c < kMaxChunks; ++c) {
    const int col = c * kNinColChunk + ctl * 16 + (lane & 15);
    if (c >= n_chunks || col >= D) continue;
    const float bv = bias[col];
#pragma unroll
    for (int q = 0; q < 4; ++q) Bs[(rt * 16 + 4 * (lane >> 4) + q) * kNinLd + col] = acc[c][q] + bv;
  }
  __syncthreads();
  const float inv_d = 1.f / static_cast<float>(D);
  for (int r = wave; r < kNinTimeTile; r += kWavesPerBlock) {
    if (t0 + r >= T) break;
    const int64_t m = m0 + r;
    const float v0 = lane < D ? Bs[r * kNinLd + lane] : 0.f, v1 = lane + 64 < D ? Bs[r * kNinLd + lane + 64] : 0.f;
    const float mu = wave_sum(v0 + v1) * inv_d;
    const float c0 = lane < D ? v0 - mu : 0.f, c1 = lane + 64 < D ? v1 - mu : 0.f;
    const float var = wave_sum(c0 * c0 + c1 * c1) * inv_d;
    const float rs = 1.0f / sqrtf(var + 1e-8f);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      if (d >= D) continue;
      float y = fmaxf((h ? c1 : c0) * rs * gamma[d] + beta[d], 0.f);
      if (resid) y += resid[m * D + d];
      out[m * D + d] = y;
      if (pre) pre[m * D + d] = h ? v1 : v0;
    }
    if (pre && lane == 0) {
      mean[m] = mu;
      rstd[m] = rs;
    }
  }
}

// y = relu(xhat gamma + beta) with xhat = (pre - mean) rstd: dy through the ReLU mask and the LayerNorm.  One wave per row.
// d pre = rstd (g - mean(g) - xhat mean(g xhat)), g = dym gamma; dyx = dym xhat and dyt = dym feed the column sums.
__global__ __launch_bounds__(kBlock) void nin_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ pre,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ dpre,
                                                            float* __restrict__ dyx, float* __restrict__ dyt, int64_t M,
                                                            int D) {
  const int lane = lane_id();
  const float inv_d = 1.f / static_cast<float>(D);
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); row < M;
       row += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const float mu = mean[row], r = rstd[row];
    float xh[2] = {0.f, 0.f}, gg[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      if (d >= D) continue;
      const int64_t i = row * D + d;
      const float c = pre[i] - mu, g = gamma[d];
      xh[h] = c * r;
      const float dym = (c * r * g + beta[d] > 0.f) ? dy[i] : 0.f;
      gg[h] = dym * g;
      dyx[i] = dym * xh[h];
      dyt[i] = dym;
    }
    const float m1 = wave_sum(gg[0] + gg[1]) * inv_d;
    const float m2 = wave_sum(gg[0] * xh[0] + gg[1] * xh[1]) * inv_d;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      if (d < D) dpre[row * D + d] = r * (gg[h] - m1 - xh[h] * m2);
    }
  }
}

// d W_j[o, i] = sum_m dc[m, o] * x[m - shift_j, i] over the rows with t - shift_j >= 0.  grid = (k, slabs); block (j, q) walks
// the row tiles q, q + slabs, ... and leaves its [D, D] partial at part[(q k + j) D D].  Wave w owns the 16 x 16 tiles
// w, w + 4, ... of the output (up to 16 of them).
__global__ __launch_bounds__(kBlock) void nin_wgrad_kernel(const float* __restrict__ dc, const float* __restrict__ x,
                                                           int64_t M, int T, int D, NinTaps taps,
                                                           float* __restrict__ part) {
  __shared__ float Ds[kNinWgradRows * kNinLd];
  __shared__ float Xs[kNinWgradRows * kNinLd];
  constexpr int kOwn = (kSeqMaxDim / 16) * (kSeqMaxDim / 16) / kWavesPerBlock;
  const int j = blockIdx.x, q = blockIdx.y, slabs = gridDim.y, shift = taps.shift[j];
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_in_block(), nct = D / 16, tiles = nct * nct;
  const int64_t n_rt = (M + kNinWgradRows - 1) / kNinWgradRows;
  f32x4 acc[kOwn];
#pragma unroll
  for (int u = 0; u < kOwn; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (shift < T) {
    for (int64_t tile = q; tile < n_rt; tile += slabs) {
      const int64_t m0 = tile * kNinWgradRows;
      __syncthreads();
      for (int e = tid; e < kNinWgradRows * D; e += kBlock) {
        const int r = e / D, c = e - r * D;
        const int64_t m = m0 + r;
        const bool in = m < M;
        Ds[r * kNinLd + c] = in ? dc[m * D + c] : 0.f;
        Xs[r * kNinLd + c] = (in && static_cast<int>(m % T) >= shift) ? x[(m - shift) * D + c] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kOwn; ++u) {
        const int t = wave + kWavesPerBlock * u;
        if (t < tiles) {
          const int ot = t / nct, it = t - ot * nct;
          acc[u] = mma16(acc[u], Ds + ot * 16, 1, kNinLd, Xs + it * 16, kNinLd, 1, kNinWgradRows);
        }
      }
    }
  }
  float* dst = part + (static_cast<int64_t>(q) * taps.n + j) * D * D;
#pragma unroll
  for (int u = 0; u < kOwn; ++u) {
    const int t = wave + kWavesPerBlock * u;
    if (t >= tiles) continue;
    const int ot = t / nct, it = t - ot * nct;
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[(ot * 16 + 4 * (lane >> 4) + r) * D + it * 16 + (lane & 15)] = acc[u][r];
  }
}

// g[(o D + i) k + j] = the slabs' partials of (j, o, i), added in slab order
__global__ __launch_bounds__(kBlock) void nin_wfold_kernel(const float* __restrict__ part, int D, int ksz, int slabs,
                                                           float* __restrict__ g) {
  const int n = D * D * ksz;
  for (int e = blockIdx.x * kBlock + threadIdx.x; e < n; e += gridDim.x * kBlock) {
    const int j = e % ksz, oi = e / ksz;
    float v = 0.f;
    for (int q = 0; q < slabs; ++q) v += part[(static_cast<int64_t>(q) * ksz + j) * D * D + oi];
    g[e] = v;
  }
}

// ---- the labelled rows -----------------------------------------------------------------------------------------------------
// Candidates: every row ("all", n_c = M) or row b T + T - 1 of every sequence ("last", n_c = B).  A candidate whose pos
// is in 1 .. n_items is labelled (anything else but 0 raises the status).  One block: thread i counts and then writes
// the candidates [i per, (i + 1) per), so rows[] is ascending.  meta[0] = n_lab; slot[c] = the candidate's place in
// rows[], -1 when it is not labelled.
__global__ __launch_bounds__(kBlock) void nin_labels_kernel(const int64_t* __restrict__ pos, int64_t n_c, int T, int last,
                                                            int64_t n_items, int* __restrict__ meta,
                                                            int* __restrict__ rows, int* __restrict__ labs,
                                                            int* __restrict__ slot, hiprec_stats* stats) {
  __shared__ int s_off[kBlock + 1];
  const int tid = threadIdx.x;
  const int64_t per = (n_c + kBlock - 1) / kBlock, c0 = tid * per, c1 = c0 + per < n_c ? c0 + per : n_c;
  int cnt = 0;
  bool bad = false;
  for (int64_t c = c0; c < c1; ++c) {
    const int64_t p = pos[last ? c * T + T - 1 : c];
    if (p >= 1 && p <= n_items) ++cnt;
    else if (p != 0) bad = true;
  }
  if (bad) atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
  s_off[tid + 1] = cnt;
  __syncthreads();
  if (tid == 0) {
    s_off[0] = 0;
    for (int i = 1; i <= kBlock; ++i) s_off[i] += s_off[i - 1];
    meta[0] = s_off[kBlock];
  }
  __syncthreads();
  int at = s_off[tid];
  for (int64_t c = c0; c < c1; ++c) {
    const int64_t m = last ? c * T + T - 1 : c, p = pos[m];
    if (p >= 1 && p <= n_items) {
      rows[at] = static_cast<int>(m);
      labs[at] = static_cast<int>(p);
      slot[c] = at++;
    } else {
      slot[c] = -1;
    }
  }
}

// ---- cross-entropy over the catalogue with the tied table ------------------------------------------------------------------
// Tiles: kNinCeRows labelled rows of f x kNinCeItems items.  Column c of item tile jt is item 64 jt + 1 + c.  A row past
// n_lab is zeros with weight 0, a column past n_items has score -inf.
__device__ __forceinline__ void nin_ce_load_rows(float (*Hs)[kNinLd], const float* __restrict__ f,
                                                 const int* __restrict__ rows, int r0, int n_lab, int D) {
  for (int e = threadIdx.x; e < kNinCeRows * D; e += kBlock) {
    const int r = e / D, c = e - r * D;
    Hs[r][c] = r0 + r < n_lab ? f[static_cast<int64_t>(rows[r0 + r]) * D + c] : 0.f;
  }
}

__device__ __forceinline__ void nin_ce_load_items(float (*Es)[kNinLd], const float* __restrict__ E, int64_t j0,
                                                  int64_t n_items, int D) {
  for (int e = threadIdx.x; e < kNinCeItems * D; e += kBlock) {
    const int r = e / D, c = e - r * D;
    const int64_t j = j0 + 1 + r;
    Es[r][c] = j <= n_items ? E[j * D + c] : 0.f;
  }
}

// S[r][c] = <f_r, E_c>: 2 x 4 tiles of 16 x 16, two per wave
__device__ __forceinline__ void nin_ce_scores(float (*S)[kNinCeItems + 1], const float (*Hs)[kNinLd],
                                              const float (*Es)[kNinLd], int64_t j0, int64_t n_items, int D) {
  const int lane = lane_id(), wave = wave_in_block();
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int tile = wave * 2 + u, rt = tile >> 2, ct = tile & 3;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = mma16(acc, &Hs[rt * 16][0], kNinLd, 1, &Es[ct * 16][0], 1, kNinLd, D);
    const int col = ct * 16 + (lane & 15);
    const bool in = j0 + 1 + col <= n_items;
#pragma unroll
    for (int r = 0; r < 4; ++r) S[rt * 16 + 4 * (lane >> 4) + r][col] = in ? acc[r] : -INFINITY;
  }
}

// per labelled row of the tile: its log-sum-exp and label; S <- G = (p - [item == label]) / n_lab, p = exp(score - lse)
__device__ __forceinline__ void nin_ce_grad(float (*S)[kNinCeItems + 1], float* s_lse, int* s_lab,
                                            const float* __restrict__ lse, const int* __restrict__ labs, int r0,
                                            int n_lab, int64_t j0) {
  if (threadIdx.x < kNinCeRows) {
    const int r = r0 + threadIdx.x;
    s_lse[threadIdx.x] = r < n_lab ? lse[r] : 0.f;
    s_lab[threadIdx.x] = r < n_lab ? labs[r] : 0;      // 0: past n_lab, weight 0
  }
  __syncthreads();
  const float inv = 1.0f / static_cast<float>(n_lab);
  for (int e = threadIdx.x; e < kNinCeRows * kNinCeItems; e += kBlock) {
    const int r = e >> 6, c = e & 63;
    float g = 0.f;
    if (s_lab[r] != 0) g = (expf(S[r][c] - s_lse[r]) - (s_lab[r] == j0 + 1 + c ? 1.f : 0.f)) * inv;
    S[r][c] = g;
  }
}

// forward: grid (row tiles of the most rows a batch can label, item splits).  Block (x, y) streams the item tiles
// [y tiles_per_split, ...) past its rows and leaves per row the running maximum, the sum of exp(score - maximum) and the
// label's score (0 when the label is in another split) at part_*[y n_max + row].
__global__ __launch_bounds__(kBlock) void nin_ce_fwd_kernel(const float* __restrict__ f, const float* __restrict__ E,
                                                            const int* __restrict__ meta, const int* __restrict__ rows,
                                                            const int* __restrict__ labs, int64_t n_max, int64_t n_items,
                                                            int D, int64_t tiles_per_split, float* __restrict__ part_m,
                                                            float* __restrict__ part_l, float* __restrict__ part_pick) {
  __shared__ float Hs[kNinCeRows][kNinLd];
  __shared__ float Es[kNinCeItems][kNinLd];
  __shared__ float S[kNinCeRows][kNinCeItems + 1];
  __shared__ int s_lab[kNinCeRows];
  constexpr int kPer = kNinCeRows / kWavesPerBlock;
  const int lane = lane_id(), wave = wave_in_block(), n_lab = meta[0];
  const int n_tiles = (n_lab + kNinCeRows - 1) / kNinCeRows;
  const int64_t n_item_tiles = (n_items + kNinCeItems - 1) / kNinCeItems;
  const int64_t jt_lo = blockIdx.y * tiles_per_split;
  const int64_t jt_hi = jt_lo + tiles_per_split < n_item_tiles ? jt_lo + tiles_per_split : n_item_tiles;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int r0 = tile * kNinCeRows;
    __syncthreads();
    nin_ce_load_rows(Hs, f, rows, r0, n_lab, D);
    if (threadIdx.x < kNinCeRows) s_lab[threadIdx.x] = r0 + threadIdx.x < n_lab ? labs[r0 + threadIdx.x] : 0;
    float m[kPer], l[kPer], pick[kPer];
#pragma unroll
    for (int rr = 0; rr < kPer; ++rr) {
      m[rr] = -INFINITY;
      l[rr] = 0.f;
      pick[rr] = 0.f;
    }
    for (int64_t jt = jt_lo; jt < jt_hi; ++jt) {
      const int64_t j0 = jt * kNinCeItems;
      __syncthreads();
      nin_ce_load_items(Es, E, j0, n_items, D);
      __syncthreads();
      nin_ce_scores(S, Hs, Es, j0, n_items, D);
      __syncthreads();
#pragma unroll
      for (int rr = 0; rr < kPer; ++rr) {
        const int row = wave * kPer + rr;
        const float s = S[row][lane];
        // a split's first tile starts inside the catalogue, so the running maximum is finite from that tile on
        const float mn = fmaxf(m[rr], wave_max(s));
        l[rr] = l[rr] * expf(m[rr] - mn) + wave_sum(expf(s - mn));
        m[rr] = mn;
        const int64_t c = s_lab[row] - 1 - j0;
        if (s_lab[row] != 0 && c >= 0 && c < kNinCeItems) pick[rr] = S[row][c];
      }
    }
#pragma unroll
    for (int rr = 0; rr < kPer; ++rr) {
      const int r = r0 + wave * kPer + rr;
      if (r < n_lab && lane == 0) {
        const int64_t at = static_cast<int64_t>(blockIdx.y) * n_max + r;
        part_m[at] = m[rr];
        part_l[at] = l[rr];
        part_pick[at] = pick[rr];
      }
    }
  }
}

// lse [n_lab] from the splits' (maximum, sum) pairs in split order, the loss partial of every block in a fixed order with
// the weight 1 / max(n_lab, 1); block 0 advances the step counter
__global__ __launch_bounds__(kBlock) void nin_ce_combine_kernel(const float* __restrict__ part_m,
                                                                const float* __restrict__ part_l,
                                                                const float* __restrict__ part_pick,
                                                                const int* __restrict__ meta, int64_t n_max, int splits,
                                                                float* __restrict__ lse, Scratch* scratch,
                                                                hiprec_stats* stats) {
  __shared__ float s_red[kBlock];
  const int n_lab = meta[0];
  float loss = 0.f;
  for (int r = blockIdx.x * kBlock + threadIdx.x; r < n_lab; r += gridDim.x * kBlock) {
    float m = part_m[r];
    for (int s = 1; s < splits; ++s) m = fmaxf(m, part_m[s * n_max + r]);
    float l = 0.f, pick = 0.f;
    for (int s = 0; s < splits; ++s) {
      l += part_l[s * n_max + r] * expf(part_m[s * n_max + r] - m);
      pick += part_pick[s * n_max + r];
    }
    const float v = m + logf(l);
    lse[r] = v;
    loss += v - pick;
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
    scratch->partials[blockIdx.x] = make_float4(s_red[0] / static_cast<float>(n_lab > 1 ? n_lab : 1), 0.f, 0.f, 0.f);
  }
}

// backward, row side: the owner of 32 labelled rows streams its split of the catalogue and writes sum_j G_j E_j over that
// split into slab blockIdx.y of dh [splits, n_max, D]
__global__ __launch_bounds__(kBlock) void nin_ce_bwd_f_kernel(const float* __restrict__ f, const float* __restrict__ E,
                                                              const int* __restrict__ meta, const int* __restrict__ rows,
                                                              const int* __restrict__ labs, const float* __restrict__ lse,
                                                              int64_t n_max, int64_t n_items, int D,
                                                              int64_t tiles_per_split, float* __restrict__ dh) {
  __shared__ float Hs[kNinCeRows][kNinLd];
  __shared__ float Es[kNinCeItems][kNinLd];
  __shared__ float S[kNinCeRows][kNinCeItems + 1];
  __shared__ float s_lse[kNinCeRows];
  __shared__ int s_lab[kNinCeRows];
  const int lane = lane_id(), wave = wave_in_block(), n_lab = meta[0];
  const int n_tiles = (n_lab + kNinCeRows - 1) / kNinCeRows;
  const int64_t n_item_tiles = (n_items + kNinCeItems - 1) / kNinCeItems;
  const int col_tiles = D / 16, tiles = 2 * col_tiles;      // of the [32, D] output, up to 16: four per wave
  const int64_t jt_lo = blockIdx.y * tiles_per_split;
  const int64_t jt_hi = jt_lo + tiles_per_split < n_item_tiles ? jt_lo + tiles_per_split : n_item_tiles;
  dh += static_cast<int64_t>(blockIdx.y) * n_max * D;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int r0 = tile * kNinCeRows;
    __syncthreads();
    nin_ce_load_rows(Hs, f, rows, r0, n_lab, D);
    f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int64_t jt = jt_lo; jt < jt_hi; ++jt) {
      const int64_t j0 = jt * kNinCeItems;
      __syncthreads();
      nin_ce_load_items(Es, E, j0, n_items, D);
      __syncthreads();
      nin_ce_scores(S, Hs, Es, j0, n_items, D);
      __syncthreads();
      nin_ce_grad(S, s_lse, s_lab, lse, labs, r0, n_lab, j0);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = wave + kWavesPerBlock * u;
        if (t < tiles) {
          const int rt = t / col_tiles, ct = t - rt * col_tiles;
          acc[u] = mma16(acc[u], &S[rt * 16][0], kNinCeItems + 1, 1, &Es[0][ct * 16], kNinLd, 1, kNinCeItems);
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
          const int i = r0 + rt * 16 + 4 * (lane >> 4) + r;
          if (i < n_lab) dh[static_cast<int64_t>(i) * D + ct * 16 + (lane & 15)] = acc[u][r];
        }
      }
    }
  }
}

// d f [M, D]: a labelled row receives its splits' partials in split order, every other row 0
__global__ __launch_bounds__(kBlock) void nin_df_kernel(const float* __restrict__ dh, const int* __restrict__ slot,
                                                        int64_t M, int T, int last, int D, int64_t n_max, int splits,
                                                        float* __restrict__ df) {
  const int64_t n = M * D, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t m = i / D;
    const int d = static_cast<int>(i - m * D);
    int r = -1;
    if (!last) r = slot[m];
    else if (m % T == T - 1) r = slot[m / T];
    float v = 0.f;
    if (r >= 0)
      for (int s = 0; s < splits; ++s) v += dh[(s * n_max + r) * D + d];
    df[i] = v;
  }
}

// backward, item side: the owner of 64 items walks all row tiles and writes d E_j = sum_r G_rj f_r with plain stores, rows
// in ascending order
__global__ __launch_bounds__(kBlock) void nin_ce_bwd_e_kernel(const float* __restrict__ f, const float* __restrict__ E,
                                                              const int* __restrict__ meta, const int* __restrict__ rows,
                                                              const int* __restrict__ labs, const float* __restrict__ lse,
                                                              int64_t n_items, int D, float* __restrict__ g_item) {
  __shared__ float Hs[kNinCeRows][kNinLd];
  __shared__ float Es[kNinCeItems][kNinLd];
  __shared__ float S[kNinCeRows][kNinCeItems + 1];
  __shared__ float s_lse[kNinCeRows];
  __shared__ int s_lab[kNinCeRows];
  const int lane = lane_id(), wave = wave_in_block(), n_lab = meta[0];
  const int n_tiles = (n_lab + kNinCeRows - 1) / kNinCeRows;
  const int64_t n_item_tiles = (n_items + kNinCeItems - 1) / kNinCeItems;
  const int col_tiles = D / 16, tiles = 4 * col_tiles;      // of the [64, D] output, up to 32: eight per wave
  for (int64_t jt = blockIdx.x; jt < n_item_tiles; jt += gridDim.x) {
    const int64_t j0 = jt * kNinCeItems;
    __syncthreads();
    nin_ce_load_items(Es, E, j0, n_items, D);
    f32x4 acc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int tile = 0; tile < n_tiles; ++tile) {
      const int r0 = tile * kNinCeRows;
      __syncthreads();
      nin_ce_load_rows(Hs, f, rows, r0, n_lab, D);
      __syncthreads();
      nin_ce_scores(S, Hs, Es, j0, n_items, D);
      __syncthreads();
      nin_ce_grad(S, s_lse, s_lab, lse, labs, r0, n_lab, j0);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = wave + kWavesPerBlock * u;
        if (t < tiles) {
          const int it = t / col_tiles, ct = t - it * col_tiles;
          acc[u] = mma16(acc[u], &S[0][it * 16], 1, kNinCeItems + 1, &Hs[0][ct * 16], kNinLd, 1, kNinCeRows);
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
  }
}

// d E[seq[m]] += dx[m] by row atomics; id 0 (and an id outside the table, which the embed has flagged) is skipped
__global__ __launch_bounds__(kBlock) void nin_embed_bwd_kernel(const float* __restrict__ dx,
                                                               const int64_t* __restrict__ seq, int64_t M, int D,
                                                               int64_t n_items, float* __restrict__ g_item) {
  const int64_t n = M * D, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t m = i / D, id = seq[m];
    if (id >= 1 && id <= n_items) atomic_add_f32(g_item + id * D + (i - m * D), dx[i]);
  }
}

__global__ __launch_bounds__(kBlock) void nin_l2_kernel(const float* __restrict__ w, float* __restrict__ g, int64_t n,
                                                        float l2) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) g[e] = fmaf(l2, w[e], g[e]);
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct NinConv {
  float *w, *b, *ln_w, *ln_b;
};
struct NinParams {      // pointers into a flat buffer laid out in state_dict() order
  float* item_emb;
  NinConv conv[kNinMaxBlocks][2];
  float *final_w, *final_b;
};

int64_t nin_n_params(const hiprec_nextitnet_shape& s) {
  const int64_t D = s.dim;
  return (s.n_items + 1) * D + s.n_blocks * 2 * (D * D * s.kernel_size + 3 * D) + D * D + D;
}

NinParams nin_params(float* base, const hiprec_nextitnet_shape& s) {
  NinParams p{};
  const int64_t D = s.dim;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += n; return r; };
  p.item_emb = take((s.n_items + 1) * D);
  for (int r = 0; r < s.n_blocks; ++r)
    for (int h = 0; h < 2; ++h) {
      NinConv& q = p.conv[r][h];
      q.w = take(D * D * s.kernel_size);
      q.b = take(D);
      q.ln_w = take(D);
      q.ln_b = take(D);
    }
  p.final_w = take(D * D);
  p.final_b = take(D);
  return p;
}

// the taps of a convolution at `dil` on sequences of T positions; the shifts are clamped to T (no row that far back)
NinTaps nin_taps(int ksz, int64_t dil, int T) {
  NinTaps t{};
  t.n = ksz;
  for (int j = 0; j < ksz; ++j) t.shift[j] = static_cast<int>(std::min<int64_t>(T, (ksz - 1 - j) * dil));
  return t;
}

int nin_slabs(int64_t M) {
  return static_cast<int>(std::min<int64_t>(kNinMaxSlabs, (M + kNinWgradRows - 1) / kNinWgradRows));
}

int nin_ce_splits(int64_t row_tiles, int64_t item_tiles, int64_t* tiles_per_split) {
  int64_t s = (kNinCeTargetBlocks + row_tiles - 1) / row_tiles;
  s = std::max<int64_t>(1, std::min<int64_t>({s, kNinCeMaxSplits, item_tiles}));
  *tiles_per_split = (item_tiles + s - 1) / s;
  return static_cast<int>((item_tiles + *tiles_per_split - 1) / *tiles_per_split);      // no split is empty
}

// the most (split, labelled row) pairs a call with n_c candidates can have, whatever n_items is
int64_t nin_split_rows(int64_t n_c) {
  return std::min<int64_t>(kNinCeMaxSplits * n_c, static_cast<int64_t>(kNinCeRows) * kNinCeTargetBlocks + n_c + kNinCeRows);
}

struct NinSaved {
  float *pre, *mean, *rstd;
};
struct NinWorkspace {
  float* x[kNinMaxBlocks + 1];
  float* h[kNinMaxBlocks];
  NinSaved sv[kNinMaxBlocks][2];
  float *f, *df, *dxa, *dxb, *dh, *dc, *dyx, *dyt, *cs[3], *wpart, *lse, *ce_m, *ce_l, *ce_pick, *dh_part;
  int *meta, *rows, *labs, *slot;
  int64_t floats;
};

// nothing here depends on n_items
NinWorkspace nin_carve(float* base, const hiprec_nextitnet_shape& s, int64_t B, int T) {
  NinWorkspace w{};
  const int64_t M = B * T, D = s.dim, MD = M * D, n_c = s.loss_last ? B : M;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += (n + 3) / 4 * 4; return r; };
  for (int r = 0; r <= s.n_blocks; ++r) w.x[r] = take(MD);
  for (int r = 0; r < s.n_blocks; ++r) {
    w.h[r] = take(MD);
    for (int h = 0; h < 2; ++h) w.sv[r][h] = NinSaved{take(MD), take(M), take(M)};
  }
  w.f = take(MD);
  w.df = take(MD);
  w.dxa = take(MD);
  w.dxb = take(MD);
  w.dh = take(MD);
  w.dc = take(MD);
  w.dyx = take(MD);
  w.dyt = take(MD);
  for (int i = 0; i < 3; ++i) w.cs[i] = take(colsum_ws_floats(static_cast<int>(M), s.dim));
  w.wpart = take(static_cast<int64_t>(nin_slabs(M)) * s.kernel_size * D * D);
  w.lse = take(n_c);
  const int64_t sr = nin_split_rows(n_c);
  w.ce_m = take(sr);
  w.ce_l = take(sr);
  w.ce_pick = take(sr);
  w.dh_part = take(sr * D);
  w.meta = reinterpret_cast<int*>(take(4));
  w.rows = reinterpret_cast<int*>(take(n_c));
  w.labs = reinterpret_cast<int*>(take(n_c));
  w.slot = reinterpret_cast<int*>(take(n_c));
  w.floats = c - base;
  return w;
}

int nin_check_shape(const hiprec_nextitnet_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  HIPREC_REQUIRE(s->n_items >= 1 && s->n_items < (1ll << 31) - 1, "NextItNet needs 1 <= n_items < 2^31 - 1");
  HIPREC_REQUIRE(s->dim >= 16 && s->dim <= kSeqMaxDim && s->dim % 16 == 0,
                 "NextItNet needs emb_dim a multiple of 16 up to %d (got %d)", kSeqMaxDim, s->dim);
  HIPREC_REQUIRE(s->maxlen >= 1 && s->maxlen <= kSeqMaxLen, "NextItNet needs 1 <= maxlen <= %d (got %d)", kSeqMaxLen,
                 s->maxlen);
  HIPREC_REQUIRE(s->kernel_size >= 1 && s->kernel_size <= kNinMaxKernel, "NextItNet needs 1 <= kernel_size <= %d (got %d)",
                 kNinMaxKernel, s->kernel_size);
  HIPREC_REQUIRE(s->n_blocks >= 1 && s->n_blocks <= kNinMaxBlocks,
                 "NextItNet needs 1 <= len(dilations) * block_num <= %d (got %d)", kNinMaxBlocks, s->n_blocks);
  for (int r = 0; r < s->n_blocks; ++r)
    HIPREC_REQUIRE(s->dilation[r] >= 1, "NextItNet needs every dilation >= 1 (block %d has %d)", r, s->dilation[r]);
  return 0;
}

bool nin_batch_ok(const hiprec_nextitnet_shape& s, int64_t B, int T) {
  return B >= 1 && T >= 1 && T <= s.maxlen && B * T < (1ll << 24);
}

int nin_conv_fwd(const float* in, const NinConv& q, int64_t B, int T, int D, const NinTaps& taps, const float* resid,
                 const NinSaved* sv, float* out, hipStream_t st) {
  const int64_t blocks = B * ((T + kNinTimeTile - 1) / kNinTimeTile);
  nin_conv_kernel<false><<<static_cast<unsigned>(blocks), kBlock, 0, st>>>(
      in, q.w, T, D, taps, q.b, q.ln_w, q.ln_b, resid, sv ? sv->pre : nullptr, sv ? sv->mean : nullptr,
      sv ? sv->rstd : nullptr, out);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// backward of out = relu(LN(conv(in))) from dy = d out: d conv.{weight, bias}, d ln.{weight, bias} and din = conv^T(d pre)
// + add
int nin_conv_bwd(const float* dy, const float* in, const NinConv& w, const NinConv& g, const NinSaved& sv, int64_t B, int T,
                 int D, const NinTaps& taps, const float* add, float* din, const NinWorkspace& a, hipStream_t st) {
  const int64_t M = B * T;
  const int Mi = static_cast<int>(M);
  nin_ln_bwd_kernel<<<grid_for_waves(M), kBlock, 0, st>>>(dy, sv.pre, sv.mean, sv.rstd, w.ln_w, w.ln_b, a.dc, a.dyx, a.dyt,
                                                          M, D);
  HIPREC_TRY(hipGetLastError());
  GemmGroup p{};
  p.n = 3;
  p.p[0] = make_colsum(a.dyx, Mi, D, D, g.ln_w, a.cs[0]);
  p.p[1] = make_colsum(a.dyt, Mi, D, D, g.ln_b, a.cs[1]);
  p.p[2] = make_colsum(a.dc, Mi, D, D, g.b, a.cs[2]);
  if (int rc = launch_group(p, st)) return rc;
  if (int rc = launch_colsum_reduce(p, st)) return rc;
  const int slabs = nin_slabs(M);
  nin_wgrad_kernel<<<dim3(taps.n, slabs), kBlock, 0, st>>>(a.dc, in, M, T, D, taps, a.wpart);
  HIPREC_TRY(hipGetLastError());
  nin_wfold_kernel<<<grid_for_threads(static_cast<int64_t>(D) * D * taps.n), kBlock, 0, st>>>(a.wpart, D, taps.n, slabs,
                                                                                              g.w);
  HIPREC_TRY(hipGetLastError());
  const int64_t blocks = B * ((T + kNinTimeTile - 1) / kNinTimeTile);
  nin_conv_kernel<true><<<static_cast<unsigned>(blocks), kBlock, 0, st>>>(a.dc, w.w, T, D, taps, nullptr, nullptr, nullptr,
                                                                           add, nullptr, nullptr, nullptr, din);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

int nin_run(const hiprec_nextitnet_shape& s, float* w_flat, float* g_flat, const int64_t* seq, const int64_t* pos,
            int64_t B, int T, float l2, float* feats_out, hiprec_stats* stats, Scratch* scratch, float* ws_base,
            hipStream_t st) {
  const bool train = g_flat != nullptr;
  const int D = s.dim, R = s.n_blocks, ksz = s.kernel_size;
  const int64_t M = B * T;
  const int Mi = static_cast<int>(M);
  const NinParams w = nin_params(w_flat, s);
  const NinWorkspace a = nin_carve(ws_base, s, B, T);

  if (int rc = seq_embed(w.item_emb, nullptr, seq, M, T, D, s.n_items, 1.0f, nullptr, 1.0f, a.x[0], stats, st)) return rc;
  for (int r = 0; r < R; ++r) {
    const NinTaps t1 = nin_taps(ksz, s.dilation[r], T), t2 = nin_taps(ksz, 2ll * s.dilation[r], T);
    if (int rc = nin_conv_fwd(a.x[r], w.conv[r][0], B, T, D, t1, nullptr, train ? &a.sv[r][0] : nullptr, a.h[r], st))
      return rc;
    if (int rc = nin_conv_fwd(a.h[r], w.conv[r][1], B, T, D, t2, a.x[r], train ? &a.sv[r][1] : nullptr, a.x[r + 1], st))
      return rc;
  }
  {
    GemmGroup g{};
    g.n = 1;
    if (train)
      g.p[0] = make_gemm(kNT, Mi, D, D, a.x[R], D, w.final_w, D, a.f, D, w.final_b, 0, nullptr, 0, false);
    else      // the last position of every sequence alone
      g.p[0] = make_gemm(kNT, static_cast<int>(B), D, D, a.x[R] + static_cast<int64_t>(T - 1) * D, T * D, w.final_w, D,
                         feats_out, D, w.final_b, 0, nullptr, 0, false);
    if (int rc = launch_group(g, st)) return rc;
  }
  if (!train) return 0;

  const NinParams g = nin_params(g_flat, s);
  const int64_t n_c = s.loss_last ? B : M;
  const int64_t row_tiles = (n_c + kNinCeRows - 1) / kNinCeRows, item_tiles = (s.n_items + kNinCeItems - 1) / kNinCeItems;
  int64_t tps = 0;
  const int splits = nin_ce_splits(row_tiles, item_tiles, &tps);
  const dim3 ce_grid(static_cast<unsigned>(std::min<int64_t>(row_tiles, kNinCeTargetBlocks)), splits);
  nin_labels_kernel<<<1, kBlock, 0, st>>>(pos, n_c, T, s.loss_last, s.n_items, a.meta, a.rows, a.labs, a.slot, stats);
  HIPREC_TRY(hipGetLastError());
  nin_ce_fwd_kernel<<<ce_grid, kBlock, 0, st>>>(a.f, w.item_emb, a.meta, a.rows, a.labs, n_c, s.n_items, D, tps, a.ce_m,
                                                a.ce_l, a.ce_pick);
  HIPREC_TRY(hipGetLastError());
  nin_ce_combine_kernel<<<grid_for_threads(n_c), kBlock, 0, st>>>(a.ce_m, a.ce_l, a.ce_pick, a.meta, n_c, splits, a.lse,
                                                                  scratch, stats);
  HIPREC_TRY(hipGetLastError());
  nin_ce_bwd_f_kernel<<<ce_grid, kBlock, 0, st>>>(a.f, w.item_emb, a.meta, a.rows, a.labs, a.lse, n_c, s.n_items, D, tps,
                                                  a.dh_part);
  HIPREC_TRY(hipGetLastError());
  nin_df_kernel<<<grid_for_threads(M * D), kBlock, 0, st>>>(a.dh_part, a.slot, M, T, s.loss_last, D, n_c, splits, a.df);
  HIPREC_TRY(hipGetLastError());
  nin_ce_bwd_e_kernel<<<static_cast<unsigned>(std::min<int64_t>(item_tiles, 65535)), kBlock, 0, st>>>(
      a.f, w.item_emb, a.meta, a.rows, a.labs, a.lse, s.n_items, D, g.item_emb);
  HIPREC_TRY(hipGetLastError());
  {
    GemmGroup p{};
    p.n = 3;
    p.p[0] = make_gemm(kNN, Mi, D, D, a.df, D, w.final_w, D, a.dxa, D, nullptr, 0, nullptr, 0, false);
    p.p[1] = make_gemm(kTNm, D, D, Mi, a.df, D, a.x[R], D, g.final_w, D, nullptr, 0, nullptr, 0, false);
    p.p[2] = make_colsum(a.df, Mi, D, D, g.final_b, a.cs[0]);
    if (int rc = launch_group(p, st)) return rc;
    if (int rc = launch_colsum_reduce(p, st)) return rc;
  }
  float *dx = a.dxa, *dx_next = a.dxb;
  for (int r = R - 1; r >= 0; --r) {
    const NinTaps t1 = nin_taps(ksz, s.dilation[r], T), t2 = nin_taps(ksz, 2ll * s.dilation[r], T);
    if (int rc = nin_conv_bwd(dx, a.h[r], w.conv[r][1], g.conv[r][1], a.sv[r][1], B, T, D, t2, nullptr, a.dh, a, st))
      return rc;
    if (int rc = nin_conv_bwd(a.dh, a.x[r], w.conv[r][0], g.conv[r][0], a.sv[r][0], B, T, D, t1, dx, dx_next, a, st))
      return rc;
    std::swap(dx, dx_next);
  }
  nin_embed_bwd_kernel<<<grid_for_threads(M * D), kBlock, 0, st>>>(dx, seq, M, D, s.n_items, g.item_emb);
  HIPREC_TRY(hipGetLastError());
  if (l2 != 0.f) {
    const int64_t n = nin_n_params(s);
    nin_l2_kernel<<<grid_for_threads(n), kBlock, 0, st>>>(w_flat, g_flat, n, l2);
    HIPREC_TRY(hipGetLastError());
  }
  return 0;
}

int nin_check_call(const hiprec_nextitnet_shape* shape, const void* w_flat, const void* seq, int64_t batch, int seq_len,
                   const void* stats, const void* workspace, size_t workspace_bytes) {
  if (int rc = nin_check_shape(shape)) return rc;
  HIPREC_REQUIRE(w_flat && seq && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(nin_batch_ok(*shape, batch, seq_len),
                 "NextItNet: batch %lld x sequence length %d must be >= 1 x 1, within maxlen %d and below 2^24 positions",
                 static_cast<long long>(batch), seq_len, shape->maxlen);
  const size_t need = hiprec_nextitnet_workspace_bytes(shape, batch, seq_len);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  return 0;
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_nextitnet_shape_bytes(void) { return sizeof(hiprec_nextitnet_shape); }

extern "C" int64_t hiprec_nextitnet_param_floats(const hiprec_nextitnet_shape* shape) {
  if (nin_check_shape(shape)) return -1;
  return nin_n_params(*shape);
}

extern "C" size_t hiprec_nextitnet_workspace_bytes(const hiprec_nextitnet_shape* shape, int64_t batch, int32_t seq_len) {
  if (nin_check_shape(shape) || !nin_batch_ok(*shape, batch, seq_len)) return 0;
  return sizeof(float) * static_cast<size_t>(nin_carve(nullptr, *shape, batch, seq_len).floats);
}

extern "C" int hiprec_nextitnet_grad(const hiprec_nextitnet_shape* shape, const float* w_flat, float* g_flat,
                                     const int64_t* seq, const int64_t* pos, int64_t batch, int32_t seq_len, float l2,
                                     hiprec_stats* stats, void* scratch, size_t scratch_bytes, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (int rc = nin_check_call(shape, w_flat, seq, batch, seq_len, stats, workspace, workspace_bytes)) return rc;
  HIPREC_REQUIRE(g_flat && pos && scratch, "training needs the gradient buffer, pos and the scratch block");
  if (scratch_bytes < kScratchBytes) {
    set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
    return HIPREC_E_SCRATCH;
  }
  return nin_run(*shape, const_cast<float*>(w_flat), g_flat, seq, pos, batch, seq_len, l2, nullptr, stats,
                 static_cast<Scratch*>(scratch), static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_nextitnet_feats(const hiprec_nextitnet_shape* shape, const float* w_flat, const int64_t* seq,
                                      int64_t batch, int32_t seq_len, float* feats_out, hiprec_stats* stats,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = nin_check_call(shape, w_flat, seq, batch, seq_len, stats, workspace, workspace_bytes)) return rc;
  HIPREC_REQUIRE(feats_out, "the eval forward needs the feats buffer");
  return nin_run(*shape, const_cast<float*>(w_flat), nullptr, seq, nullptr, batch, seq_len, 0.f, feats_out, stats, nullptr,
                 static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_nextitnet_conv(const float* x, const float* weight, const float* bias, const float* ln_weight,
                                     const float* ln_bias, const float* resid, int64_t batch, int32_t seq_len,
                                     int32_t dim, int32_t kernel_size, int32_t dilation, float* out, void* stream) {
  HIPREC_REQUIRE(x && weight && bias && ln_weight && ln_bias && out, "NULL pointer");
  HIPREC_REQUIRE(dim >= 16 && dim <= kSeqMaxDim && dim % 16 == 0 && kernel_size >= 1 && kernel_size <= kNinMaxKernel &&
                     dilation >= 1 && batch >= 1 && seq_len >= 1 && seq_len <= kSeqMaxLen &&
                     batch * seq_len < (1ll << 24),
                 "NextItNet convolution: shape outside the model's limits");
  const NinConv q{const_cast<float*>(weight), const_cast<float*>(bias), const_cast<float*>(ln_weight),
                  const_cast<float*>(ln_bias)};
  return nin_conv_fwd(x, q, batch, seq_len, dim, nin_taps(kernel_size, dilation, seq_len), resid, nullptr, out,
                      static_cast<hipStream_t>(stream));
}
