// Caser (Tang and Wang, WSDM 2018): zero_grad + forward + loss + backward of one training step as a fixed sequence of
// launches, no host sync.  The contract is in include/hiprec.h; F = n_v d + n_h L is the width of fc1's input.
//
//   pack                the conv_h filters of every height h, zero padded for the MFMA: Wp_h [pad16(n_h)][pad4(h dS)]
//                       with Wp_h[f][i dS + k] = conv_h.{h-1}.weight[f, i, k] (dS: the LDS row stride of the forward)
//   convolution forward a workgroup owns kCaserSeqTile sequences.  Their L x d rows are gathered into LDS ONCE, row
//                       m = b L + t at Es[m dS]; because consecutive rows of a sequence are dS apart, the window of height
//                       h that starts at row m IS the contiguous run Es[m dS .. (m + h) dS): the filter bank of one height
//                       is a plain [rows, h dS] x [h dS, n_h] product on v_mfma_f32_16x16x4_f32 with overlapping A rows
//                       (im2col that costs no copy; the sum over the h filter rows happens in the accumulator, so neither
//                       the h row products nor pre are ever written anywhere).  One height at a time: bias, ac_conv, the
//                       16 x 16 tiles into a [rows, n_h] LDS tile, max over t with the arg-max (lowest t on a tie) in one
//                       byte per (b, h, f).  The vertical filters are [n_v, L] x [L, d] per sequence on the same tile.
//   fc1                 the grouped GEMM (bias and relu in its epilogue) into x[:, :d]; one pass applies tanh / sigm and
//                       gathers the user rows into x[:, d:]
//   scores and loss     the targets are counted first (the two means need their counts); then one wave per batch row:
//                       x, the T + N rows of W2, the scores, softplus, dx in registers; d W2, d b2, d user_embeddings by
//                       row atomics
//   fc1 backward        dz = dx[:, :d] * ac_fc'(z) in place; dgrad (the dropout keep bytes in its epilogue), wgrad
//                       (one block per tile walks the whole batch: no split-K atomics) and the fixed-order bias column sum
//   convolution backward per batch row: G[b, h, f] = d out_h * ac_conv'(out_h) and d E = G scattered through the arg-max
//                       onto the filter rows + conv_v^T d out_v, by row atomics into item_embeddings (never row 0);
//                       d conv_h and d conv_v as per-slab partials (the batch is cut into at most kCaserMaxSlabs slabs)
//                       that one launch folds in slab order
//   weight decay        g += l2 * w over the whole flat buffer
//
// Every gradient except the three tables (user_embeddings, item_embeddings, W2 / b2) is the same bits on every run.
#include <algorithm>

#include "caser.hpp"
#include "gemm.hpp"

namespace hiprec {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kCaserMaxRowTiles = (kCaserSeqTile * kCaserMaxLen + 15) / 16;
constexpr size_t kCaserLds = 72 * 1024;      // the convolution forward at the limits needs 68 120 B

__host__ __device__ inline int pad_to(int n, int q) { return (n + q - 1) / q * q; }
// LDS row stride of the gathered item rows: >= d and = 2 (mod 4).  The A operand's lanes 0 .. 15 read rows dS apart and
// lanes 16 .. 31 the same rows one float on: with dS = 2 x odd the 32 lanes of a half wave hit 32 different banks.
__host__ __device__ inline int caser_row_stride(int d) { return d + ((6 - d % 4) % 4); }

__device__ __forceinline__ float caser_act(int kind, float v) {
  switch (kind) {
    case HIPREC_CASER_AC_RELU: return fmaxf(v, 0.f);
    case HIPREC_CASER_AC_TANH: return tanhf(v);
    case HIPREC_CASER_AC_SIGM: return sigmoid_f32(v);
    default: return v;
  }
}

// the activation's derivative from its OUTPUT y
__device__ __forceinline__ float caser_dact(int kind, float y) {
  switch (kind) {
    case HIPREC_CASER_AC_RELU: return y > 0.f ? 1.f : 0.f;
    case HIPREC_CASER_AC_TANH: return 1.f - y * y;
    case HIPREC_CASER_AC_SIGM: return y * (1.f - y);
    default: return 1.f;
  }
}

struct CaserDims {
  int64_t n_users, n_items;
  int d, L, T, N, nv, nh, ac_conv, ac_fc;
  int dS, nhp, F;
};

// offsets (floats) inside the conv_h block of the flat buffer: conv_h.{h-1}.weight [n_h, h, d], then its bias [n_h]
__host__ __device__ inline int64_t caser_off_w(int nh, int d, int h) {
  return static_cast<int64_t>(nh) * d * ((h - 1) * h / 2) + static_cast<int64_t>(nh) * (h - 1);
}
__host__ __device__ inline int64_t caser_off_b(int nh, int d, int h) {
  return caser_off_w(nh, d, h) + static_cast<int64_t>(nh) * h * d;
}
// offset of Wp_h inside the packed copy
__host__ __device__ inline int64_t caser_off_p(int nhp, int dS, int h) {
  int64_t o = 0;
  for (int q = 1; q < h; ++q) o += static_cast<int64_t>(nhp) * ((q * dS + 3) / 4 * 4);
  return o;
}

__global__ __launch_bounds__(kBlock) void caser_pack_kernel(const float* __restrict__ conv_h, CaserDims s,
                                                            float* __restrict__ wp) {
  const int64_t total = caser_off_p(s.nhp, s.dS, s.L + 1), stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e0 = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e0 < total; e0 += stride) {
    int64_t e = e0;
    int h = 1, Kh = pad_to(s.dS, 4);
    while (e >= static_cast<int64_t>(s.nhp) * Kh) {
      e -= static_cast<int64_t>(s.nhp) * Kh;
      ++h;
      Kh = pad_to(h * s.dS, 4);
    }
    const int f = static_cast<int>(e / Kh), kk = static_cast<int>(e - static_cast<int64_t>(f) * Kh);
    const int i = kk / s.dS, k = kk - i * s.dS;
    float v = 0.f;
    if (f < s.nh && i < h && k < s.d) v = conv_h[caser_off_w(s.nh, s.d, h) + (static_cast<int64_t>(f) * h + i) * s.d + k];
    wp[e0] = v;
  }
}

// NR row tiles that share one column tile's B operand: acc[r] += Es[rows of tile rt0 + r] x Wp_h[columns of tile ct]
template <int NR>
__device__ __forceinline__ void caser_mma(f32x4 (&acc)[NR], const float* Es, int dS, const float* __restrict__ Wp, int Kh,
                                          int rt0, int n_rt, int ct) {
  const int l = lane_id();
  const float* ap = Es + (rt0 * 16 + (l & 15)) * dS + (l >> 4);
  const float* bp = Wp + static_cast<int64_t>(ct * 16 + (l & 15)) * Kh + (l >> 4);
#pragma unroll 4
  for (int k = 0; k < Kh; k += 4) {
    const float b = bp[k];
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (rt0 + r < n_rt) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[r * 16 * dS + k], b, acc[r], 0, 0, 0);
  }
}

template <int NR>
__device__ __forceinline__ void caser_conv_item(const float* Es, int dS, const float* __restrict__ Wp, int Kh, int rt0,
                                                int n_rt, int ct, const float* __restrict__ bias, int nh, int ac,
                                                float* Ps, int ldp) {
  f32x4 acc[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
  caser_mma<NR>(acc, Es, dS, Wp, Kh, rt0, n_rt, ct);
  const int l = lane_id(), f = ct * 16 + (l & 15);
  if (f >= nh) return;
  const float bf = bias[f];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    if (rt0 + r >= n_rt) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) Ps[((rt0 + r) * 16 + 4 * (l >> 4) + q) * ldp + f] = caser_act(ac, acc[r][q] + bf);
  }
}

// grid = ceil(B / kCaserSeqTile).  LDS: Es [(16 n_rt + L + 1)][dS] (the rows behind the tile are zero: the windows that
// hang over a sequence's end read them or the next sequence and are never pooled), Ps [16 n_rt][n_h + 1].
// o [B, F] = [out_v | out_h] through the keep bytes, craw [B, n_h L] = out_h before the dropout, am = its arg-max.
__global__ __launch_bounds__(kBlock) void caser_conv_fwd_kernel(
    const float* __restrict__ E, const float* __restrict__ conv_v, const float* __restrict__ conv_h,
    const float* __restrict__ wp, const int64_t* __restrict__ seq, int64_t B, CaserDims s, int n_rt, int nr,
    const uint8_t* __restrict__ keep, float ks, float* __restrict__ o, float* __restrict__ craw,
    uint8_t* __restrict__ am, hiprec_stats* stats) {
  extern __shared__ float caser_lds[];
  const int d = s.d, L = s.L, dS = s.dS, nh = s.nh, nv = s.nv, F = s.F;
  const int rows_alloc = n_rt * 16 + L + 1, R = kCaserSeqTile * L, ldp = nh + 1;
  float* Es = caser_lds;
  float* Ps = Es + rows_alloc * dS;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * kCaserSeqTile;
  const int tid = threadIdx.x, wave = wave_in_block();
  for (int e = tid; e < rows_alloc * dS; e += kBlock) {
    const int m = e / dS, k = e - m * dS;
    float v = 0.f;
    if (m < R && k < d) {
      const int bl = m / L;
      if (b0 + bl < B) {
        const int64_t id = seq[(b0 + bl) * L + (m - bl * L)];
        if (id >= 1 && id <= s.n_items)
          v = E[id * d + k];
        else if (id != 0 && k == 0)
          atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
      }
    }
    Es[e] = v;
  }
  __syncthreads();
  // the vertical filters: out_v[b, c, j] = bias[c] + sum_l w[c, l] E[b, l, j], no activation
  for (int e = tid; e < kCaserSeqTile * nv * d; e += kBlock) {
    const int bl = e / (nv * d), r = e - bl * nv * d, c = r / d, j = r - c * d;
    if (b0 + bl >= B) break;
    float v = conv_v[nv * L + c];
    for (int l = 0; l < L; ++l) v = fmaf(conv_v[c * L + l], Es[(bl * L + l) * dS + j], v);
    const int64_t at = (b0 + bl) * F + r;
    if (keep) v = keep[at] ? v * ks : 0.f;
    o[at] = v;
  }
  const int n_ct = s.nhp / 16, n_rg = (n_rt + nr - 1) / nr;
  for (int h = 1; h <= L; ++h) {
    const int Kh = pad_to(h * dS, 4);
    const float* Wp = wp + caser_off_p(s.nhp, dS, h);
    const float* bias = conv_h + caser_off_b(nh, d, h);
    for (int item = wave; item < n_ct * n_rg; item += kWavesPerBlock) {
      const int ct = item % n_ct, rt0 = item / n_ct * nr;
      switch (nr) {
        case 1: caser_conv_item<1>(Es, dS, Wp, Kh, rt0, n_rt, ct, bias, nh, s.ac_conv, Ps, ldp); break;
        case 2: caser_conv_item<2>(Es, dS, Wp, Kh, rt0, n_rt, ct, bias, nh, s.ac_conv, Ps, ldp); break;
        case 3: caser_conv_item<3>(Es, dS, Wp, Kh, rt0, n_rt, ct, bias, nh, s.ac_conv, Ps, ldp); break;
        default: caser_conv_item<kCaserMaxRowTiles>(Es, dS, Wp, Kh, rt0, n_rt, ct, bias, nh, s.ac_conv, Ps, ldp); break;
      }
    }
    __syncthreads();
    for (int e = tid; e < kCaserSeqTile * nh; e += kBlock) {
      const int bl = e / nh, f = e - bl * nh;
      if (b0 + bl >= B) break;
      float best = Ps[(bl * L) * ldp + f];
      int arg = 0;
      for (int t = 1; t <= L - h; ++t) {
        const float v = Ps[(bl * L + t) * ldp + f];
        if (v > best) {
          best = v;
          arg = t;
        }
      }
      const int col = (h - 1) * nh + f;
      craw[(b0 + bl) * (nh * L) + col] = best;
      am[(b0 + bl) * (nh * L) + col] = static_cast<uint8_t>(arg);
      const int64_t at = (b0 + bl) * F + nv * d + col;
      if (keep) best = keep[at] ? best * ks : 0.f;
      o[at] = best;
    }
    __syncthreads();
  }
}

// x [B, 2d]: ac_fc on the fc1 half where the GEMM's epilogue has not applied it (tanh, sigm), the user rows into the other
__global__ __launch_bounds__(kBlock) void caser_x_kernel(float* __restrict__ x, const float* __restrict__ U,
                                                         const int64_t* __restrict__ users, int64_t B, CaserDims s,
                                                         hiprec_stats* stats) {
  const int d = s.d;
  const int64_t n = B * 2 * d, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  const bool act = s.ac_fc == HIPREC_CASER_AC_TANH || s.ac_fc == HIPREC_CASER_AC_SIGM;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
    const int64_t b = e / (2 * d);
    const int j = static_cast<int>(e - b * 2 * d);
    if (j < d) {
      if (act) x[e] = caser_act(s.ac_fc, x[e]);
    } else {
      const int64_t u = users[b];
      float v = 0.f;
      if (u >= 0 && u < s.n_users)
        v = U[u * d + (j - d)];
      else if (j == d)
        atomicOr(&stats->status, HIPREC_STATUS_USER_OOB);
      x[e] = v;
    }
  }
}

// cnt[0] = targets of pos in 1 .. n_items, cnt[1] = the same of neg (zeroed by the caller)
__global__ __launch_bounds__(kBlock) void caser_count_kernel(const int64_t* __restrict__ pos,
                                                             const int64_t* __restrict__ neg, int64_t n_pos,
                                                             int64_t n_neg, int64_t n_items, int* __restrict__ cnt) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  int c0 = 0, c1 = 0;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n_pos + n_neg; e += stride) {
    const int64_t id = e < n_pos ? pos[e] : neg[e - n_pos];
    const bool ok = id >= 1 && id <= n_items;
    if (e < n_pos) c0 += ok;
    else c1 += ok;
  }
  if (c0) atomicAdd(cnt, c0);
  if (c1) atomicAdd(cnt + 1, c1);
}

// one wave per batch row; lane holds x[lane + 64 q], q < 4 (2d <= 256).  g_* == NULL never happens here (training only).
__global__ __launch_bounds__(kBlock) void caser_loss_kernel(
    const float* __restrict__ x, const float* __restrict__ W2, const float* __restrict__ b2,
    const int64_t* __restrict__ users, const int64_t* __restrict__ pos, const int64_t* __restrict__ neg,
    const int* __restrict__ cnt, int64_t B, CaserDims s, float* __restrict__ dx, float* __restrict__ g_U,
    float* __restrict__ g_W2, float* __restrict__ g_b2, Scratch* scratch, hiprec_stats* stats) {
  const int lane = lane_id(), d = s.d, d2 = 2 * s.d, T = s.T, N = s.N;
  const int n_p = cnt[0], n_n = cnt[1];
  const float inv_p = n_p > 0 ? 1.0f / static_cast<float>(n_p) : 0.f;
  const float inv_n = n_n > 0 ? 1.0f / static_cast<float>(n_n) : 0.f;
  float loss_w = 0.f;
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); b < B;
       b += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    float xv[4], dxl[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = lane + 64 * q;
      xv[q] = j < d2 ? x[b * d2 + j] : 0.f;
    }
    for (int k = 0; k < T + N; ++k) {
      const bool is_pos = k < T;
      const int64_t item = is_pos ? pos[b * T + k] : neg[b * N + (k - T)];
      if (item == 0) continue;
      if (item < 0 || item > s.n_items) {
        if (lane == 0) atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
        continue;
      }
      const float* wr = W2 + item * d2;
      float wv[4], part = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = lane + 64 * q;
        wv[q] = j < d2 ? wr[j] : 0.f;
        part = fmaf(xv[q], wv[q], part);
      }
      const float sc = wave_sum(part) + b2[item];
      float sg, ds;
      if (is_pos) {      // softplus(-s) = -log sigmoid(s); d/ds = -sigmoid(-s)
        loss_w += neg_logsigmoid(sc, &sg) * inv_p;
        ds = -sg * inv_p;
      } else {           // softplus(s) = -log sigmoid(-s); d/ds = sigmoid(s)
        loss_w += neg_logsigmoid(-sc, &sg) * inv_n;
        ds = sg * inv_n;
      }
      float* gr = g_W2 + item * d2;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = lane + 64 * q;
        if (j < d2) {
          atomic_add_f32(gr + j, ds * xv[q]);
          dxl[q] = fmaf(ds, wv[q], dxl[q]);
        }
      }
      if (lane == 0) atomic_add_f32(g_b2 + item, ds);
    }
    const int64_t u = users[b];
    const bool u_ok = u >= 0 && u < s.n_users;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = lane + 64 * q;
      if (j < d2) {
        dx[b * d2 + j] = dxl[q];
        if (j >= d && u_ok && dxl[q] != 0.f) atomic_add_f32(g_U + u * d + (j - d), dxl[q]);
      }
    }
  }
  publish_partials<kWavesPerBlock>(loss_w, 0.f, 0.f, 1.0f, scratch);
  if (blockIdx.x == 0 && threadIdx.x == 0) advance_step(stats);
}

// dz = dx[:, :d] * ac_fc'(z), in place (x[:, :d] = z)
__global__ __launch_bounds__(kBlock) void caser_dz_kernel(float* __restrict__ dx, const float* __restrict__ x, int64_t B,
                                                          CaserDims s) {
  const int d = s.d;
  const int64_t n = B * d, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
    const int64_t b = e / d, at = b * 2 * d + (e - b * d);
    dx[at] *= caser_dact(s.ac_fc, x[at]);
  }
}

// One workgroup per batch row.  G [B, n_h L] = d out_h * ac_conv'(out_h); d E[b, l, :] = sum over (h, f, i) with
// arg-max + i = l of G conv_h.{h-1}.weight[f, i, :] + sum_c conv_v.weight[c, l] d out_v[b, c, :], added to
// g_E[seq[b, l]] by row atomics (ids 0 and out of range are skipped).
// LDS: gs / ts [n_h L], acc [parts][L][d] with parts = kBlock / d column groups that each own every parts-th (h, f).
__global__ __launch_bounds__(kBlock) void caser_conv_bwd_kernel(
    const float* __restrict__ dO, const float* __restrict__ craw, const uint8_t* __restrict__ am,
    const float* __restrict__ conv_v, const float* __restrict__ conv_h, const int64_t* __restrict__ seq, int64_t B,
    CaserDims s, float* __restrict__ G, float* __restrict__ g_E) {
  __shared__ float gs[kCaserMaxNh * kCaserMaxLen];
  __shared__ int ts[kCaserMaxNh * kCaserMaxLen];
  __shared__ float acc[kBlock * kCaserMaxLen];
  const int d = s.d, L = s.L, nh = s.nh, nv = s.nv, F = s.F, nc = nh * L;
  const int tid = threadIdx.x, parts = kBlock / d, part = tid / d, k = tid - part * d;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    for (int e = tid; e < nc; e += kBlock) {
      const int h = e / nh + 1;
      const float g = dO[b * F + nv * d + e] * caser_dact(s.ac_conv, craw[b * nc + e]);
      G[b * nc + e] = g;
      gs[e] = g;
      ts[e] = min(static_cast<int>(am[b * nc + e]), L - h);
    }
    for (int e = tid; e < parts * L * d; e += kBlock) acc[e] = 0.f;
    __syncthreads();
    if (part < parts) {
      float* mine = acc + part * L * d + k;
      for (int e = part; e < nc; e += parts) {
        const float g = gs[e];
        if (g == 0.f) continue;
        const int h = e / nh + 1, f = e - (h - 1) * nh, t = ts[e];
        const float* w = conv_h + caser_off_w(nh, d, h) + static_cast<int64_t>(f) * h * d + k;
        for (int i = 0; i < h; ++i) mine[(t + i) * d] = fmaf(g, w[i * d], mine[(t + i) * d]);
      }
    }
    __syncthreads();
    for (int e = tid; e < L * d; e += kBlock) {
      const int l = e / d, j = e - l * d;
      const int64_t id = seq[b * L + l];
      if (id < 1 || id > s.n_items) continue;
      float v = 0.f;
      for (int p = 0; p < parts; ++p) v += acc[p * L * d + e];
      for (int c = 0; c < nv; ++c) v = fmaf(conv_v[c * L + l], dO[b * F + c * d + j], v);
      if (v != 0.f) atomic_add_f32(g_E + id * d + j, v);
    }
    __syncthreads();
  }
}

// d conv_h of one (slab, height, filter): part[slab][.] laid out like the conv_h block of the flat buffer.
// grid = (n_h L, slabs).  The slab's rows go through LDS kCaserChunk at a time; a thread owns up to 5 of the h d elements.
__global__ __launch_bounds__(kBlock) void caser_dconvh_kernel(const float* __restrict__ G, const uint8_t* __restrict__ am,
                                                              const float* __restrict__ E,
                                                              const int64_t* __restrict__ seq, int64_t B, int slab_rows,
                                                              CaserDims s, int64_t part_floats,
                                                              float* __restrict__ part) {
  __shared__ float gs[kCaserChunk];
  __shared__ int ts[kCaserChunk];
  __shared__ int ids[kCaserChunk * kCaserMaxLen];
  constexpr int kOwn = (kCaserMaxLen * kCaserMaxDim + kBlock - 1) / kBlock;
  const int d = s.d, L = s.L, nh = s.nh, nc = nh * L;
  const int col = blockIdx.x, h = col / nh + 1, f = col - (h - 1) * nh, tid = threadIdx.x, n_el = h * d;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * slab_rows, r1 = r0 + slab_rows < B ? r0 + slab_rows : B;
  float a[kOwn], bias = 0.f;
#pragma unroll
  for (int q = 0; q < kOwn; ++q) a[q] = 0.f;
  for (int64_t c0 = r0; c0 < r1; c0 += kCaserChunk) {
    const int n = r1 - c0 < kCaserChunk ? static_cast<int>(r1 - c0) : kCaserChunk;
    __syncthreads();
    for (int e = tid; e < n; e += kBlock) {
      gs[e] = G[(c0 + e) * nc + col];
      ts[e] = min(static_cast<int>(am[(c0 + e) * nc + col]), L - h);
    }
    for (int e = tid; e < n * L; e += kBlock) {
      const int64_t id = seq[c0 * L + e];
      ids[e] = (id >= 1 && id <= s.n_items) ? static_cast<int>(id) : 0;
    }
    __syncthreads();
    for (int r = 0; r < n; ++r) {
      const float g = gs[r];
      if (g == 0.f) continue;
      if (tid == 0) bias += g;
      const int t = ts[r];
#pragma unroll
      for (int q = 0; q < kOwn; ++q) {
        const int e = tid + q * kBlock;
        if (e < n_el) {
          const int i = e / d, k = e - i * d, id = ids[r * L + t + i];
          if (id) a[q] = fmaf(g, E[static_cast<int64_t>(id) * d + k], a[q]);
        }
      }
    }
  }
  float* out = part + static_cast<int64_t>(blockIdx.y) * part_floats;
#pragma unroll
  for (int q = 0; q < kOwn; ++q) {
    const int e = tid + q * kBlock;
    if (e < n_el) out[caser_off_w(nh, d, h) + static_cast<int64_t>(f) * n_el + e] = a[q];
  }
  if (tid == 0) out[caser_off_b(nh, d, h) + f] = bias;
}

// d conv_v of one (slab, filter c): wave w takes l = w, w + 4, ... and l = L is the bias; part[slab][c L + l | n_v L + c]
// grid = (n_v, slabs)
__global__ __launch_bounds__(kBlock) void caser_dconvv_kernel(const float* __restrict__ dO, const float* __restrict__ E,
                                                              const int64_t* __restrict__ seq, int64_t B, int slab_rows,
                                                              CaserDims s, float* __restrict__ part) {
  const int d = s.d, L = s.L, nv = s.nv, F = s.F, c = blockIdx.x, lane = lane_id();
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * slab_rows, r1 = r0 + slab_rows < B ? r0 + slab_rows : B;
  float* out = part + static_cast<int64_t>(blockIdx.y) * (nv * (L + 1));
  for (int l = wave_in_block(); l <= L; l += kWavesPerBlock) {
    float v = 0.f;
    for (int64_t b = r0; b < r1; ++b) {
      const float* go = dO + b * F + c * d;
      if (l == L) {
        for (int j = lane; j < d; j += kWave) v += go[j];
      } else {
        const int64_t id = seq[b * L + l];
        if (id < 1 || id > s.n_items) continue;
        for (int j = lane; j < d; j += kWave) v = fmaf(go[j], E[id * d + j], v);
      }
    }
    v = wave_sum(v);
    if (lane == 0) out[l == L ? nv * L + c : c * L + l] = v;
  }
}

// g[e] = the slabs' partials of element e, added in slab order
__global__ __launch_bounds__(kBlock) void caser_fold_kernel(const float* __restrict__ part, int64_t n, int slabs,
                                                            float* __restrict__ g) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
    float v = part[e];
    for (int q = 1; q < slabs; ++q) v += part[q * n + e];
    g[e] = v;
  }
}

__global__ __launch_bounds__(kBlock) void caser_l2_kernel(const float* __restrict__ w, float* __restrict__ g, int64_t n,
                                                          float l2) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) g[e] = fmaf(l2, w[e], g[e]);
}

// scores[b, k] = <x[b], W2[items[b, k]]> + b2[items[b, k]]: one wave per pair
__global__ __launch_bounds__(kBlock) void caser_score_kernel(const float* __restrict__ x, const float* __restrict__ W2,
                                                             const float* __restrict__ b2,
                                                             const int64_t* __restrict__ items, int64_t B, int K, int d2,
                                                             int64_t n_items, float* __restrict__ scores,
                                                             hiprec_stats* stats) {
  const int lane = lane_id();
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); p < B * K;
       p += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const int64_t b = p / K, item = items[p];
    if (item < 1 || item > n_items) {
      if (lane == 0) {
        atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
        scores[p] = 0.f;
      }
      continue;
    }
    float part = 0.f;
    for (int j = lane; j < d2; j += kWave) part = fmaf(x[b * d2 + j], W2[item * d2 + j], part);
    const float sc = wave_sum(part) + b2[item];
    if (lane == 0) scores[p] = sc;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
struct CaserParams {      // pointers into a flat buffer laid out in state_dict() order
  float *U, *E, *conv_v, *conv_h, *fc1_w, *fc1_b, *W2, *b2;
};

CaserDims caser_dims(const hiprec_caser_shape& s) {
  CaserDims q{};
  q.n_users = s.n_users; q.n_items = s.n_items;
  q.d = s.dim; q.L = s.L; q.T = s.T; q.N = s.N; q.nv = s.n_v; q.nh = s.n_h; q.ac_conv = s.ac_conv; q.ac_fc = s.ac_fc;
  q.dS = caser_row_stride(s.dim);
  q.nhp = pad_to(s.n_h, 16);
  q.F = s.n_v * s.dim + s.n_h * s.L;
  return q;
}

int64_t caser_convh_floats(const CaserDims& q) { return caser_off_w(q.nh, q.d, q.L + 1); }

int64_t caser_n_params(const CaserDims& q) {
  const int64_t d = q.d;
  return q.n_users * d + (q.n_items + 1) * d + q.nv * q.L + q.nv + caser_convh_floats(q) + d * q.F + d +
         (q.n_items + 1) * 2 * d + (q.n_items + 1);
}

CaserParams caser_params(float* base, const CaserDims& q) {
  CaserParams p{};
  const int64_t d = q.d;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += n; return r; };
  p.U = take(q.n_users * d);
  p.E = take((q.n_items + 1) * d);
  p.conv_v = take(q.nv * q.L + q.nv);
  p.conv_h = take(caser_convh_floats(q));
  p.fc1_w = take(d * q.F);
  p.fc1_b = take(d);
  p.W2 = take((q.n_items + 1) * 2 * d);
  p.b2 = take(q.n_items + 1);
  return p;
}

int caser_slabs(int64_t B) {
  return static_cast<int>(std::min<int64_t>(kCaserMaxSlabs, (B + kCaserSlabRows - 1) / kCaserSlabRows));
}

struct CaserWorkspace {
  float *wp, *o, *craw, *x, *dx, *dO, *G, *part_h, *part_v, *cs;
  uint8_t* am;
  int* cnt;
  int64_t floats;
};

CaserWorkspace caser_carve(float* base, const CaserDims& q, int64_t B) {
  CaserWorkspace w{};
  const int64_t nc = static_cast<int64_t>(q.nh) * q.L, slabs = caser_slabs(B);
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += (n + 3) / 4 * 4; return r; };
  w.wp = take(caser_off_p(q.nhp, q.dS, q.L + 1));
  w.o = take(B * q.F);
  w.craw = take(B * nc);
  w.am = reinterpret_cast<uint8_t*>(take((B * nc + 3) / 4));
  w.x = take(B * 2 * q.d);
  w.cnt = reinterpret_cast<int*>(take(4));
  w.dx = take(B * 2 * q.d);
  w.dO = take(B * q.F);
  w.G = take(B * nc);
  w.part_h = take(slabs * caser_convh_floats(q));
  w.part_v = take(slabs * q.nv * (q.L + 1));
  w.cs = take(colsum_ws_floats(static_cast<int>(B), q.d));
  w.floats = c - base;
  return w;
}

int caser_check_shape(const hiprec_caser_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  HIPREC_REQUIRE(s->n_users >= 1 && s->n_items >= 1, "Caser needs n_users >= 1 and n_items >= 1, got %lld and %lld",
                 static_cast<long long>(s->n_users), static_cast<long long>(s->n_items));
  HIPREC_REQUIRE(s->n_items < (1ll << 31) - 1 && s->n_users < (1ll << 31), "Caser needs n_users and n_items below 2^31");
  HIPREC_REQUIRE(s->dim >= 1 && s->dim <= kCaserMaxDim, "Caser needs 1 <= emb_dim <= %d (got %d)", kCaserMaxDim, s->dim);
  HIPREC_REQUIRE(s->L >= 1 && s->L <= kCaserMaxLen, "Caser needs 1 <= L <= %d (got %d)", kCaserMaxLen, s->L);
  HIPREC_REQUIRE(s->n_v >= 1 && s->n_v <= kCaserMaxNv, "Caser needs 1 <= n_v <= %d (got %d)", kCaserMaxNv, s->n_v);
  HIPREC_REQUIRE(s->n_h >= 1 && s->n_h <= kCaserMaxNh, "Caser needs 1 <= n_h <= %d (got %d)", kCaserMaxNh, s->n_h);
  HIPREC_REQUIRE(s->T >= 1 && s->T <= kCaserMaxT, "Caser needs 1 <= T <= %d (got %d)", kCaserMaxT, s->T);
  HIPREC_REQUIRE(s->N >= 1 && s->N <= kCaserMaxN, "Caser needs 1 <= neg_samples <= %d (got %d)", kCaserMaxN, s->N);
  HIPREC_REQUIRE(s->ac_conv >= 0 && s->ac_conv <= HIPREC_CASER_AC_IDEN, "Caser: unknown ac_conv %d", s->ac_conv);
  HIPREC_REQUIRE(s->ac_fc >= 0 && s->ac_fc <= HIPREC_CASER_AC_IDEN, "Caser: unknown ac_fc %d", s->ac_fc);
  return 0;
}

bool caser_batch_ok(const CaserDims& q, int64_t B) { return B >= 1 && B * q.F < (1ll << 31) && B < (1ll << 24); }

int caser_run(const CaserDims& q, float* w_flat, float* g_flat, const int64_t* seq, const int64_t* users,
              const int64_t* pos, const int64_t* neg, int64_t B, const uint8_t* keep, float ks, float l2, float* x_out,
              hiprec_stats* stats, Scratch* scratch, float* ws_base, hipStream_t st) {
  const bool train = g_flat != nullptr;
  const int d = q.d, L = q.L, F = q.F, Bi = static_cast<int>(B), nc = q.nh * L;
  const CaserParams w = caser_params(w_flat, q);
  const CaserWorkspace a = caser_carve(ws_base, q, B);
  if (!train) keep = nullptr;

  static std::atomic<uint64_t> lds_ok{0};
  if (int rc = allow_dynamic_lds({reinterpret_cast<const void*>(&caser_conv_fwd_kernel)}, kCaserLds, lds_ok,
                                 "Caser's convolution forward"))
    return rc;
  const int n_rt = (kCaserSeqTile * L + 15) / 16, n_ct = q.nhp / 16;
  // row tiles per wave item: as few as keep all four waves busy, so that a column tile's B operand is shared where it can be
  const int groups = std::max(1, std::min(n_rt, kWavesPerBlock / n_ct));
  int nr = (n_rt + groups - 1) / groups;
  if (nr > 3) nr = kCaserMaxRowTiles;
  const size_t lds = sizeof(float) * (static_cast<size_t>(n_rt * 16 + L + 1) * q.dS + static_cast<size_t>(n_rt) * 16 * (q.nh + 1));
  HIPREC_REQUIRE(lds <= kCaserLds, "Caser: the convolution tile needs %zu B of LDS", lds);

  caser_pack_kernel<<<grid_for_threads(caser_off_p(q.nhp, q.dS, L + 1)), kBlock, 0, st>>>(w.conv_h, q, a.wp);
  HIPREC_TRY(hipGetLastError());
  const int tiles = static_cast<int>((B + kCaserSeqTile - 1) / kCaserSeqTile);
  caser_conv_fwd_kernel<<<tiles, kBlock, lds, st>>>(w.E, w.conv_v, w.conv_h, a.wp, seq, B, q, n_rt, nr, keep, ks, a.o,
                                                    a.craw, a.am, stats);
  HIPREC_TRY(hipGetLastError());
  float* x = train ? a.x : x_out;
  {
    GemmGroup g{};
    g.n = 1;
    g.p[0] = make_gemm(kNT, Bi, d, F, a.o, F, w.fc1_w, F, x, 2 * d, w.fc1_b, q.ac_fc == HIPREC_CASER_AC_RELU ? 1 : 0,
                       nullptr, 0, false);
    if (int rc = launch_group(g, st)) return rc;
  }
  caser_x_kernel<<<grid_for_threads(B * 2 * d), kBlock, 0, st>>>(x, w.U, users, B, q, stats);
  HIPREC_TRY(hipGetLastError());
  if (!train) return 0;

  const CaserParams g = caser_params(g_flat, q);
  HIPREC_TRY(hipMemsetAsync(a.cnt, 0, 4 * sizeof(int), st));
  caser_count_kernel<<<grid_for_threads(B * (q.T + q.N)), kBlock, 0, st>>>(pos, neg, B * q.T, B * q.N, q.n_items, a.cnt);
  HIPREC_TRY(hipGetLastError());
  caser_loss_kernel<<<grid_for_waves(B), kBlock, 0, st>>>(x, w.W2, w.b2, users, pos, neg, a.cnt, B, q, a.dx, g.U, g.W2,
                                                          g.b2, scratch, stats);
  HIPREC_TRY(hipGetLastError());
  caser_dz_kernel<<<grid_for_threads(B * d), kBlock, 0, st>>>(a.dx, x, B, q);
  HIPREC_TRY(hipGetLastError());
  {
    GemmGroup p{};
    p.n = 3;
    p.p[0] = make_gemm(kNN, Bi, F, d, a.dx, 2 * d, w.fc1_w, F, a.dO, F, nullptr, 0, nullptr, 0, false);
    if (keep) { p.p[0].keep = keep; p.p[0].ldk = F; p.p[0].keep_scale = ks; }
    p.p[1] = make_gemm(kTNm, d, F, Bi, a.dx, 2 * d, a.o, F, g.fc1_w, F, nullptr, 0, nullptr, 0, false);
    p.p[2] = make_colsum(a.dx, Bi, d, 2 * d, g.fc1_b, a.cs);
    if (int rc = launch_group(p, st)) return rc;
    if (int rc = launch_colsum_reduce(p, st)) return rc;
  }
  caser_conv_bwd_kernel<<<static_cast<int>(std::min<int64_t>(B, 65535)), kBlock, 0, st>>>(a.dO, a.craw, a.am, w.conv_v,
                                                                                          w.conv_h, seq, B, q, a.G, g.E);
  HIPREC_TRY(hipGetLastError());
  const int slabs = caser_slabs(B), slab_rows = static_cast<int>((B + slabs - 1) / slabs);
  const int64_t ch = caser_convh_floats(q), cv = q.nv * (L + 1);
  caser_dconvh_kernel<<<dim3(nc, slabs), kBlock, 0, st>>>(a.G, a.am, w.E, seq, B, slab_rows, q, ch, a.part_h);
  HIPREC_TRY(hipGetLastError());
  caser_dconvv_kernel<<<dim3(q.nv, slabs), kBlock, 0, st>>>(a.dO, w.E, seq, B, slab_rows, q, a.part_v);
  HIPREC_TRY(hipGetLastError());
  caser_fold_kernel<<<grid_for_threads(ch), kBlock, 0, st>>>(a.part_h, ch, slabs, g.conv_h);
  HIPREC_TRY(hipGetLastError());
  caser_fold_kernel<<<grid_for_threads(cv), kBlock, 0, st>>>(a.part_v, cv, slabs, g.conv_v);
  HIPREC_TRY(hipGetLastError());
  if (l2 != 0.f) {
    const int64_t n = caser_n_params(q);
    caser_l2_kernel<<<grid_for_threads(n), kBlock, 0, st>>>(w_flat, g_flat, n, l2);
    HIPREC_TRY(hipGetLastError());
  }
  return 0;
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_caser_shape_bytes(void) { return sizeof(hiprec_caser_shape); }

extern "C" int64_t hiprec_caser_param_floats(const hiprec_caser_shape* shape) {
  if (caser_check_shape(shape)) return -1;
  return caser_n_params(caser_dims(*shape));
}

extern "C" size_t hiprec_caser_workspace_bytes(const hiprec_caser_shape* shape, int64_t batch) {
  if (caser_check_shape(shape)) return 0;
  const CaserDims q = caser_dims(*shape);
  if (!caser_batch_ok(q, batch)) return 0;
  return sizeof(float) * static_cast<size_t>(caser_carve(nullptr, q, batch).floats);
}

extern "C" int hiprec_caser_grad(const hiprec_caser_shape* shape, const float* w_flat, float* g_flat, const int64_t* seq,
                                 const int64_t* users, const int64_t* pos, const int64_t* neg, int64_t batch,
                                 const uint8_t* keep, float keep_scale, float l2, float* x_out, hiprec_stats* stats,
                                 void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  if (int rc = caser_check_shape(shape)) return rc;
  const CaserDims q = caser_dims(*shape);
  HIPREC_REQUIRE(w_flat && seq && users && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(caser_batch_ok(q, batch), "Caser: batch %lld is empty or too large", static_cast<long long>(batch));
  if (g_flat) {
    HIPREC_REQUIRE(pos && neg && scratch, "training needs the targets and the scratch block");
    if (scratch_bytes < kScratchBytes) {
      set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
      return HIPREC_E_SCRATCH;
    }
  } else {
    HIPREC_REQUIRE(x_out, "the eval-mode forward needs the x buffer");
  }
  const size_t need = hiprec_caser_workspace_bytes(shape, batch);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  return caser_run(q, const_cast<float*>(w_flat), g_flat, seq, users, pos, neg, batch, keep, keep_scale, l2, x_out, stats,
                   static_cast<Scratch*>(scratch), static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_caser_score(const hiprec_caser_shape* shape, const float* w_flat, const float* x,
                                  const int64_t* items, int64_t batch, int32_t n_candidates, float* scores,
                                  hiprec_stats* stats, void* stream) {
  if (int rc = caser_check_shape(shape)) return rc;
  HIPREC_REQUIRE(w_flat && x && items && scores && stats, "NULL pointer");
  HIPREC_REQUIRE(batch >= 1 && n_candidates >= 1, "Caser: empty batch or candidate list");
  const CaserDims q = caser_dims(*shape);
  const CaserParams w = caser_params(const_cast<float*>(w_flat), q);
  caser_score_kernel<<<grid_for_waves(batch * n_candidates), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      x, w.W2, w.b2, items, batch, n_candidates, 2 * q.d, q.n_items, scores, stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}
