// SGL training step for gfx950.
//
// Replaces beta_rec/models/sgl.py:277-394 (SGL.forward: three LightGCN propagations -- norm_adj and two augmented
// sub-graphs -- each mean-pooled over L + 1 hops), :82-145 (calc_ssl_loss_v2: InfoNCE of the batch's view-1 rows
// against EVERY view-2 row of their side), :188-226 (create_bpr_loss: BPR sum + regs / 2 * squares of the hop-0 rows),
// autograd's backward through all of it, and :464-527 (create_sgl_mat: D^-1/2 A D^-1/2 of the kept interactions).
//
// The reference materialises normalize(sub1[users]) @ normalize(sub2).T as a [B, n] matrix per side, and autograd keeps
// its exp, its row sums and their gradients.  Here the scores only ever exist as 16 x 16 MFMA tiles in registers: the
// forward sums exp((s - 1) / temp) per batch row (cosines are <= 1, so the shift 1 / temp is exact and no running
// maximum is needed), the backward recomputes p = exp((s - 1) / temp - logsum) from the stored log-sum, once with a
// batch tile resident (dQn, one owner per batch row) and once with a node tile resident (dKn, one owner per node row,
// plain stores, the positive's one-hot subtracted from the probability tile before the product).
//
// Everything is held as the hop SUM P = E_0 + ... + E_L; the 1 / (L + 1) of the mean enters as `scale` where a row is
// read, and every d buffer is the gradient with respect to P, which enters the backward propagation at every hop.
//
// LDS tiles are [rows][DP + 4] floats, DP = dim rounded up to 16 with zeros: DP / 4 is even, so the row stride is 4 x
// an odd number and the 16 rows x 4 k-columns one MFMA operand load touches fall into 64 different banks.
#include <algorithm>

#include "common.hpp"
#include "seqrec.hpp"
#include "spmm.hpp"

namespace hiprec {

constexpr int kSglTB = HIPREC_SGL_TILE_B;   // batch rows per tile (2 MFMA row blocks)
constexpr int kSglTN = HIPREC_SGL_TILE_N;   // node rows per tile (one 16-column block per wave)
constexpr int kSglPS = kSglTN + 4;          // row stride of the probability tile
static_assert(kSglTB == 32 && kSglTN == 16 * kWavesPerBlock, "tile geometry is wired into the kernels");

__host__ __device__ inline int sgl_dp(int dim) { return (dim + 15) & ~15; }
static size_t sgl_lds_bytes(int dim, bool with_p) {
  return sizeof(float) * (static_cast<size_t>(kSglTB + kSglTN) * (sgl_dp(dim) + 4) + (with_p ? kSglTB * kSglPS : 0));
}

// one side of the InfoNCE term: batch ids `idx` into the n rows that start at row `off` of the [n_rows, dim] tables
struct SglSide {
  const int64_t* idx;
  int64_t off, n;
};

// ---- sub-graph values --------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sgl_edge_kept(int64_t r, int32_t c, int64_t e, const int32_t* edge_inter,
                                              const uint8_t* keep, const uint8_t* ku, const uint8_t* ki, int64_t n_users) {
  if (keep) return keep[edge_inter[e]] != 0;
  if (ku == nullptr) return true;
  const int64_t u = r < n_users ? r : c, i = (r < n_users ? c : r) - n_users;
  return (ku[u] & ki[i]) != 0;
}

__global__ __launch_bounds__(kBlock) void sgl_degree_kernel(hiprec_csr s, const int32_t* __restrict__ edge_inter,
                                                            const uint8_t* __restrict__ keep,
                                                            const uint8_t* __restrict__ ku,
                                                            const uint8_t* __restrict__ ki, int64_t n_users,
                                                            float* __restrict__ deg) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; r < s.n_rows; r += stride) {
    int n = 0;
    for (int64_t e = s.rowptr[r]; e < s.rowptr[r + 1]; ++e)
      n += sgl_edge_kept(r, s.col[e], e, edge_inter, keep, ku, ki, n_users) ? 1 : 0;
    deg[r] = static_cast<float>(n);   // the row owns its count: a plain store
  }
}

__global__ __launch_bounds__(kBlock) void sgl_values_kernel(hiprec_csr s, const int32_t* __restrict__ edge_inter,
                                                            const uint8_t* __restrict__ keep,
                                                            const uint8_t* __restrict__ ku,
                                                            const uint8_t* __restrict__ ki, int64_t n_users,
                                                            const float* __restrict__ deg, float* __restrict__ val) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; r < s.n_rows; r += stride) {
    const float dr = deg[r] > 0.f ? 1.0f / sqrtf(deg[r]) : 0.f;
    for (int64_t e = s.rowptr[r]; e < s.rowptr[r + 1]; ++e) {
      const int32_t c = s.col[e];
      const bool k = sgl_edge_kept(r, c, e, edge_inter, keep, ku, ki, n_users);
      const float dc = deg[c] > 0.f ? 1.0f / sqrtf(deg[c]) : 0.f;
      val[e] = k ? dr * dc : 0.f;
    }
  }
}

// ---- row kernels: one wave per row -------------------------------------------------------------------------------
// x = scale * P[r]; inv[r] = 1 / |x|; P[r] = x / |x| in place
__global__ __launch_bounds__(kBlock) void sgl_normalize_kernel(float* __restrict__ x, float* __restrict__ inv,
                                                               int64_t n_rows, int D, float scale) {
  const int lane = lane_id();
  const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t r = wave0; r < n_rows; r += n_waves) {
    float v[4], ss = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane + kWave * k;
      v[k] = c < D ? x[r * D + c] * scale : 0.f;
      ss += v[k] * v[k];
    }
    const float nrm = sqrtf(wave_sum(ss));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane + kWave * k;
      if (c < D) x[r * D + c] = v[k] / nrm;
    }
    if (lane == 0) inv[r] = 1.0f / nrm;
  }
}

// d[r] = scale * inv[r] * (d[r] - xn[r] <xn[r], d[r]>) in place, rows [r0, r0 + n)
__global__ __launch_bounds__(kBlock) void sgl_norm_bwd_kernel(float* __restrict__ d, const float* __restrict__ xn,
                                                              const float* __restrict__ inv, int64_t r0, int64_t n, int D,
                                                              float scale) {
  const int lane = lane_id();
  const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t t = wave0; t < n; t += n_waves) {
    const int64_t r = r0 + t;
    float g[4], x[4], dot = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane + kWave * k;
      g[k] = c < D ? d[r * D + c] : 0.f;
      x[k] = c < D ? xn[r * D + c] : 0.f;
      dot += g[k] * x[k];
    }
    dot = wave_sum(dot);
    const float w = scale * inv[r];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane + kWave * k;
      if (c < D) d[r * D + c] = (g[k] - x[k] * dot) * w;
    }
  }
}

// the batch rows of view 1: d1[row] += scale * inv1[row] * (dq[b] - xn1[row] <xn1[row], dq[b]>), row atomics (a user
// may sit in several batch rows)
__global__ __launch_bounds__(kBlock) void sgl_norm_bwd_scatter_kernel(const float* __restrict__ dq, SglSide side,
                                                                      int64_t batch, const float* __restrict__ xn,
                                                                      const float* __restrict__ inv,
                                                                      float* __restrict__ d, int D, float scale) {
  const int lane = lane_id();
  const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t b = wave0; b < batch; b += n_waves) {
    const int64_t id = side.idx[b];
    if (static_cast<uint64_t>(id) >= static_cast<uint64_t>(side.n)) continue;   // flagged by the loss stage
    const int64_t r = side.off + id;
    float g[4], x[4], dot = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane + kWave * k;
      g[k] = c < D ? dq[b * D + c] : 0.f;
      x[k] = c < D ? xn[r * D + c] : 0.f;
      dot += g[k] * x[k];
    }
    dot = wave_sum(dot);
    const float w = scale * inv[r];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane + kWave * k;
      if (c < D) atomic_add_f32(d + r * D + c, (g[k] - x[k] * dot) * w);
    }
  }
}

__global__ __launch_bounds__(kBlock) void sgl_add_kernel(float* __restrict__ y, const float* __restrict__ x, int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) y[i] += x[i];
}

// ---- InfoNCE tiles -----------------------------------------------------------------------------------------------
// rows of `src` ([*, D], row ids from row_of, < 0 = no such row) into dst[rows][stride], zero beyond D up to DP
template <typename F>
__device__ __forceinline__ void sgl_load_rows(float* dst, int stride, int DP, const float* __restrict__ src, int D,
                                              int rows, F&& row_of) {
  for (int e = threadIdx.x; e < rows * DP; e += kBlock) {
    const int r = e / DP, c = e - r * DP;
    const int64_t g = row_of(r);
    dst[r * stride + c] = (g >= 0 && c < D) ? src[g * D + c] : 0.f;
  }
}

// S = Q K^T for this wave's 16 node columns and both 16-row blocks of the batch tile: s[rb] holds
// (row = rb * 16 + 4 * (lane >> 4) + reg, col = wave * 16 + (lane & 15))
__device__ __forceinline__ void sgl_scores(const float* Qs, const float* Ks, int stride, int DP, f32x4 (&s)[2]) {
  const float* kb = Ks + wave_in_block() * 16 * stride;
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) s[rb] = mma16(f32x4{0.f, 0.f, 0.f, 0.f}, Qs + rb * 16 * stride, stride, 1, kb, 1, stride, DP);
}

// partial[b * n_splits + split] = sum over this split's node tiles of exp((s_bj - 1) / temp)
__global__ __launch_bounds__(kBlock) void sgl_nce_fwd_kernel(const float* __restrict__ xq, const float* __restrict__ xk,
                                                             SglSide side, int64_t batch, int D, float inv_temp,
                                                             int tiles_per_split, int n_splits,
                                                             float* __restrict__ partial) {
  extern __shared__ float smem[];
  __shared__ float s_red[kWavesPerBlock][kSglTB];
  const int DP = sgl_dp(D), stride = DP + 4;
  float* Qs = smem;
  float* Ks = smem + kSglTB * stride;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * kSglTB;
  const int split = blockIdx.y;
  const int lane = lane_id(), w = wave_in_block();
  sgl_load_rows(Qs, stride, DP, xq, D, kSglTB, [&](int r) -> int64_t {
    if (b0 + r >= batch) return -1;
    const int64_t id = side.idx[b0 + r];
    return static_cast<uint64_t>(id) < static_cast<uint64_t>(side.n) ? side.off + id : -1;
  });
  const int64_t n_tiles = (side.n + kSglTN - 1) / kSglTN;
  const int64_t t_end = min(n_tiles, static_cast<int64_t>(split + 1) * tiles_per_split);
  float rs[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int64_t t = static_cast<int64_t>(split) * tiles_per_split; t < t_end; ++t) {
    const int64_t j0 = t * kSglTN;
    __syncthreads();   // the previous tile's MFMA reads of Ks are done (and Qs is written, first round)
    sgl_load_rows(Ks, stride, DP, xk, D, kSglTN, [&](int r) -> int64_t { return j0 + r < side.n ? side.off + j0 + r : -1; });
    __syncthreads();
    f32x4 s[2];
    sgl_scores(Qs, Ks, stride, DP, s);
    const bool live = j0 + w * 16 + (lane & 15) < side.n;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) rs[rb][q] += live ? expf((s[rb][q] - 1.f) * inv_temp) : 0.f;
  }
  // the 16 columns of a row sit in the 16 lanes of one DPP row; then the four waves in a fixed order
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = rs[rb][q];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      v += __shfl_xor(v, 8, 64);
      if ((lane & 15) == 0) s_red[w][rb * 16 + 4 * (lane >> 4) + q] = v;
    }
  __syncthreads();
  if (threadIdx.x < kSglTB && b0 + threadIdx.x < batch) {
    const int r = threadIdx.x;
    partial[(b0 + r) * n_splits + split] = (s_red[0][r] + s_red[1][r]) + (s_red[2][r] + s_red[3][r]);
  }
}

// one wave per batch row: logsum[b] = log(sum of the partials, in order); row_loss[b] = ssl_reg * (logsum - (pos - 1) / temp)
__global__ __launch_bounds__(kBlock) void sgl_nce_combine_kernel(const float* __restrict__ xq, const float* __restrict__ xk,
                                                                 SglSide side, int64_t batch, int D, float inv_temp,
                                                                 float ssl_reg, int n_splits,
                                                                 const float* __restrict__ partial,
                                                                 float* __restrict__ logsum, float* __restrict__ row_loss) {
  const int lane = lane_id();
  const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t b = wave0; b < batch; b += n_waves) {
    const int64_t id = side.idx[b];
    if (static_cast<uint64_t>(id) >= static_cast<uint64_t>(side.n)) {
      if (lane == 0) {
        logsum[b] = 0.f;
        row_loss[b] = 0.f;
      }
      continue;
    }
    const int64_t r = side.off + id;
    float dot = 0.f;
    for (int c = lane; c < D; c += kWave) dot += xq[r * D + c] * xk[r * D + c];
    dot = wave_sum(dot);
    if (lane == 0) {
      float z = 0.f;
      for (int s = 0; s < n_splits; ++s) z += partial[b * n_splits + s];
      const float lz = logf(z);
      logsum[b] = lz;
      row_loss[b] = ssl_reg * (lz - (dot - 1.f) * inv_temp);
    }
  }
}

// dq[b] = c * (sum_j p_bj K_j - K_idx(b)): a block owns kSglTB batch rows and streams every node tile past them.
// NCBW: 16-column blocks of the output per wave (DP <= 64 * NCBW)
template <int NCBW>
__global__ __launch_bounds__(kBlock) void sgl_nce_dq_kernel(const float* __restrict__ xq, const float* __restrict__ xk,
                                                            SglSide side, int64_t batch, int D, float inv_temp, float coef,
                                                            const float* __restrict__ logsum, float* __restrict__ dq) {
  extern __shared__ float smem[];
  __shared__ float s_lse[kSglTB];
  const int DP = sgl_dp(D), stride = DP + 4;
  float* Qs = smem;
  float* Ks = smem + kSglTB * stride;
  float* Ps = Ks + kSglTN * stride;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * kSglTB;
  const int lane = lane_id(), w = wave_in_block();
  auto row_id = [&](int r) -> int64_t {
    if (b0 + r >= batch) return -1;
    const int64_t id = side.idx[b0 + r];
    return static_cast<uint64_t>(id) < static_cast<uint64_t>(side.n) ? side.off + id : -1;
  };
  sgl_load_rows(Qs, stride, DP, xq, D, kSglTB, row_id);
  if (threadIdx.x < kSglTB) s_lse[threadIdx.x] = b0 + threadIdx.x < batch ? logsum[b0 + threadIdx.x] : 0.f;
  f32x4 acc[2][NCBW];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int t = 0; t < NCBW; ++t) acc[rb][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t n_tiles = (side.n + kSglTN - 1) / kSglTN;
  for (int64_t t = 0; t < n_tiles; ++t) {
    const int64_t j0 = t * kSglTN;
    __syncthreads();   // the previous product's reads of Ks and Ps are done
    sgl_load_rows(Ks, stride, DP, xk, D, kSglTN, [&](int r) -> int64_t { return j0 + r < side.n ? side.off + j0 + r : -1; });
    __syncthreads();
    f32x4 s[2];
    sgl_scores(Qs, Ks, stride, DP, s);
    const bool live = j0 + w * 16 + (lane & 15) < side.n;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = rb * 16 + 4 * (lane >> 4) + q;
        Ps[row * kSglPS + w * 16 + (lane & 15)] = live ? expf((s[rb][q] - 1.f) * inv_temp - s_lse[row]) : 0.f;
      }
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < NCBW; ++tt) {
      const int cb = w + kWavesPerBlock * tt;
      if (cb * 16 < DP) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
          acc[rb][tt] = mma16(acc[rb][tt], Ps + rb * 16 * kSglPS, kSglPS, 1, Ks + cb * 16, stride, 1, kSglTN);
      }
    }
  }
#pragma unroll
  for (int tt = 0; tt < NCBW; ++tt) {
    const int d = (w + kWavesPerBlock * tt) * 16 + (lane & 15);
    if (d >= D) continue;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = rb * 16 + 4 * (lane >> 4) + q;
        if (b0 + row >= batch) continue;
        const int64_t g = row_id(row);
        dq[(b0 + row) * D + d] = g >= 0 ? coef * (acc[rb][tt][q] - xk[g * D + d]) : 0.f;
      }
  }
}

// dk[j] = c * sum_b (p_bj - [j == idx_b]) Q_b: a block owns kSglTN node rows and streams every batch tile past them;
// each of its rows is stored once
template <int NCBW>
__global__ __launch_bounds__(kBlock) void sgl_nce_dk_kernel(const float* __restrict__ xq, const float* __restrict__ xk,
                                                            SglSide side, int64_t batch, int D, float inv_temp, float coef,
                                                            const float* __restrict__ logsum, float* __restrict__ dk) {
  extern __shared__ float smem[];
  __shared__ float s_lse[kSglTB];
  __shared__ int64_t s_id[kSglTB];
  const int DP = sgl_dp(D), stride = DP + 4;
  float* Qs = smem;
  float* Ks = smem + kSglTB * stride;
  float* Ps = Ks + kSglTN * stride;
  const int64_t j0 = static_cast<int64_t>(blockIdx.x) * kSglTN;
  const int lane = lane_id(), w = wave_in_block();
  sgl_load_rows(Ks, stride, DP, xk, D, kSglTN, [&](int r) -> int64_t { return j0 + r < side.n ? side.off + j0 + r : -1; });
  f32x4 acc[4][NCBW];
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int t = 0; t < NCBW; ++t) acc[jb][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t jcol = j0 + w * 16 + (lane & 15);
  for (int64_t b0 = 0; b0 < batch; b0 += kSglTB) {
    __syncthreads();   // the previous product's reads of Qs and Ps are done
    if (threadIdx.x < kSglTB) {
      const int64_t b = b0 + threadIdx.x;
      int64_t id = b < batch ? side.idx[b] : -1;
      if (static_cast<uint64_t>(id) >= static_cast<uint64_t>(side.n)) id = -1;
      s_id[threadIdx.x] = id;
      s_lse[threadIdx.x] = id >= 0 ? logsum[b] : 0.f;
    }
    sgl_load_rows(Qs, stride, DP, xq, D, kSglTB, [&](int r) -> int64_t {
      if (b0 + r >= batch) return -1;
      const int64_t id = side.idx[b0 + r];
      return static_cast<uint64_t>(id) < static_cast<uint64_t>(side.n) ? side.off + id : -1;
    });
    __syncthreads();
    f32x4 s[2];
    sgl_scores(Qs, Ks, stride, DP, s);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = rb * 16 + 4 * (lane >> 4) + q;
        const int64_t id = s_id[row];
        float pv = (id >= 0 && jcol < side.n) ? expf((s[rb][q] - 1.f) * inv_temp - s_lse[row]) : 0.f;
        if (id >= 0 && id == jcol) pv -= 1.f;   // the positive, before the product: duplicates need no special case
        Ps[row * kSglPS + w * 16 + (lane & 15)] = pv;
      }
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < NCBW; ++tt) {
      const int cb = w + kWavesPerBlock * tt;
      if (cb * 16 < DP) {
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)   // A = P^T: element (node, batch row) at Ps[batch row][node]
          acc[jb][tt] = mma16(acc[jb][tt], Ps + jb * 16, 1, kSglPS, Qs + cb * 16, stride, 1, kSglTB);
      }
    }
  }
#pragma unroll
  for (int tt = 0; tt < NCBW; ++tt) {
    const int d = (w + kWavesPerBlock * tt) * 16 + (lane & 15);
    if (d >= D) continue;
#pragma unroll
    for (int jb = 0; jb < 4; ++jb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t j = j0 + jb * 16 + 4 * (lane >> 4) + q;
        if (j < side.n) dk[(side.off + j) * D + d] = coef * acc[jb][tt][q];
      }
  }
}

// ---- BPR stage: one wave per triple ------------------------------------------------------------------------------
template <int NPL>
__global__ __launch_bounds__(kBlock) void sgl_bpr_kernel(hiprec_sgl_plan p, const float* __restrict__ pool,
                                                         float* __restrict__ d0, const int64_t* __restrict__ users,
                                                         const int64_t* __restrict__ pos, const int64_t* __restrict__ neg,
                                                         int64_t batch, float scale, float* __restrict__ row_bpr,
                                                         float* __restrict__ row_emb, hiprec_stats* stats) {
  const int lane = lane_id();
  const int D = p.dim;
  const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t t = wave0; t < batch; t += n_waves) {
    const int64_t u = users[t], ip = pos[t], in = neg[t];
    const bool u_ok = static_cast<uint64_t>(u) < static_cast<uint64_t>(p.n_users);
    const bool i_ok = static_cast<uint64_t>(ip) < static_cast<uint64_t>(p.n_items) &&
                      static_cast<uint64_t>(in) < static_cast<uint64_t>(p.n_items);
    if (!(u_ok && i_ok)) {
      if (lane == 0) {
        atomicOr(&stats->status, (u_ok ? 0u : HIPREC_STATUS_USER_OOB) | (i_ok ? 0u : HIPREC_STATUS_ITEM_OOB));
        row_bpr[t] = 0.f;
        row_emb[t] = 0.f;
      }
      continue;
    }
    const int64_t ru = u * D, rp = (p.n_users + ip) * D, rn = (p.n_users + in) * D;
    float ue[NPL], pe[NPL], ne[NPL], u0[NPL], p0[NPL], n0[NPL];
    float x = 0.f, sq = 0.f;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int c = lane + kWave * k;
      const bool ok = c < D;
      ue[k] = ok ? pool[ru + c] * scale : 0.f;
      pe[k] = ok ? pool[rp + c] * scale : 0.f;
      ne[k] = ok ? pool[rn + c] * scale : 0.f;
      u0[k] = ok ? p.e0[ru + c] : 0.f;
      p0[k] = ok ? p.e0[rp + c] : 0.f;
      n0[k] = ok ? p.e0[rn + c] : 0.f;
      x += ue[k] * (pe[k] - ne[k]);
      sq += u0[k] * u0[k] + p0[k] * p0[k] + n0[k] * n0[k];
    }
    x = wave_sum(x);
    sq = wave_sum(sq);
    float sg;   // sigmoid(-x) = -d softplus(-x) / dx
    const float loss = neg_logsigmoid(x, &sg);
    if (lane == 0) {
      row_bpr[t] = loss;
      row_emb[t] = 0.5f * p.regs * sq;
    }
    const float gs = sg * scale;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int c = lane + kWave * k;
      if (c < D) {
        atomic_add_f32(d0 + ru + c, -gs * (pe[k] - ne[k]));
        atomic_add_f32(d0 + rp + c, -gs * ue[k]);
        atomic_add_f32(d0 + rn + c, gs * ue[k]);
        atomic_add_f32(p.g + ru + c, p.regs * u0[k]);
        atomic_add_f32(p.g + rp + c, p.regs * p0[k]);
        atomic_add_f32(p.g + rn + c, p.regs * n0[k]);
      }
    }
  }
}

// one block: the three loss parts summed in a fixed order, the step's partial for the optimizer sweep, the step counter
__global__ __launch_bounds__(kBlock) void sgl_finish_kernel(const float* __restrict__ rows, int64_t batch, int n_ssl,
                                                            float* __restrict__ parts, hiprec_stats* stats,
                                                            Scratch* scratch) {
  __shared__ double s_sum[4][kBlock];
  for (int a = 0; a < 4; ++a) {
    double v = 0.0;
    if (a < 2 + n_ssl)
      for (int64_t i = threadIdx.x; i < batch; i += kBlock) v += rows[a * batch + i];
    s_sum[a][threadIdx.x] = v;
  }
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s)
      for (int a = 0; a < 4; ++a) s_sum[a][threadIdx.x] += s_sum[a][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double ssl = s_sum[2][0] + s_sum[3][0];
    parts[0] = static_cast<float>(s_sum[0][0]);
    parts[1] = static_cast<float>(s_sum[1][0]);
    parts[2] = static_cast<float>(ssl);
    parts[3] = static_cast<float>(s_sum[0][0] + s_sum[1][0] + ssl);
    scratch->partials[0] = make_float4(parts[3], parts[1], 0.f, 0.f);
    scratch->n_partials = 1;
    advance_step(stats);
  }
}

__global__ __launch_bounds__(kBlock) void sgl_predict_kernel(const float* __restrict__ pool, int64_t n_users,
                                                             int64_t n_items, int D, float scale,
                                                             const int64_t* __restrict__ users,
                                                             const int64_t* __restrict__ items, int64_t n,
                                                             float* __restrict__ scores, hiprec_stats* stats) {
  const int lane = lane_id();
  const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t t = wave0; t < n; t += n_waves) {
    const int64_t u = users[t], i = items[t];
    if (static_cast<uint64_t>(u) >= static_cast<uint64_t>(n_users) ||
        static_cast<uint64_t>(i) >= static_cast<uint64_t>(n_items)) {
      if (lane == 0) {
        atomicOr(&stats->status, HIPREC_STATUS_ROW_OOB);
        scores[t] = __builtin_nanf("");
      }
      continue;
    }
    float dot = 0.f;
    for (int c = lane; c < D; c += kWave) dot += (pool[u * D + c] * scale) * (pool[(n_users + i) * D + c] * scale);
    dot = wave_sum(dot);
    if (lane == 0) scores[t] = dot;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------
static int64_t sgl_ws_floats(int64_t n_rows, int dim) { return 8 * n_rows * dim + 2 * n_rows; }
static int64_t sgl_batch_floats(int64_t batch, int dim) {
  return batch * (2 + 4 + 2 * HIPREC_SGL_MAX_SPLITS + 2 * static_cast<int64_t>(dim));
}

struct SglWs {
  float *pool, *x1, *x2, *d0, *d1, *d2, *ping, *pong, *inv1, *inv2;
};

static SglWs sgl_ws(const hiprec_sgl_plan* p) {
  const int64_t nd = p->a.n_rows * p->dim;
  float* w = p->ws;
  return SglWs{w, w + nd, w + 2 * nd, w + 3 * nd, w + 4 * nd, w + 5 * nd, w + 6 * nd, w + 7 * nd, w + 8 * nd,
               w + 8 * nd + p->a.n_rows};
}

static int check_sgl_plan(const hiprec_sgl_plan* p, bool train) {
  HIPREC_REQUIRE(p != nullptr, "NULL plan");
  HIPREC_REQUIRE(p->a.rowptr && p->a.n_rows > 0 && p->a.nnz >= 0 && (p->a.nnz == 0 || (p->a.col && p->a.val)),
                 "bad CSR a");
  HIPREC_REQUIRE(p->n_users > 0 && p->n_items > 0, "bad sizes");
  HIPREC_REQUIRE(p->a.n_rows == p->n_users + p->n_items, "graph size != n_users + n_items");
  HIPREC_REQUIRE(p->n_layers >= 0 && p->n_layers <= HIPREC_SGL_MAX_LAYERS, "SGL n_layers %d: 0 .. %d are supported",
                 p->n_layers, HIPREC_SGL_MAX_LAYERS);
  HIPREC_REQUIRE(p->dim >= 1 && p->dim <= 256, "SGL emb_dim %d: 1 .. 256 are supported", p->dim);
  HIPREC_REQUIRE(p->e0 != nullptr && p->ws != nullptr, "NULL e0 / ws");
  HIPREC_REQUIRE(p->ws_floats >= sgl_ws_floats(p->a.n_rows, p->dim), "ws holds %lld floats, %lld are needed",
                 (long long)p->ws_floats, (long long)sgl_ws_floats(p->a.n_rows, p->dim));
  if (!train) return 0;
  HIPREC_REQUIRE(p->g != nullptr, "NULL g");
  HIPREC_REQUIRE(p->at.rowptr && p->at.n_rows == p->a.n_rows && p->at.nnz == p->a.nnz &&
                     (p->a.nnz == 0 || (p->at.col && p->at.val)),
                 "bad CSR at / a and at differ");
  HIPREC_REQUIRE(p->ssl_sides >= 0 && p->ssl_sides <= 3, "bad ssl_sides %d", p->ssl_sides);
  HIPREC_REQUIRE(p->n_splits >= 0 && p->n_splits <= HIPREC_SGL_MAX_SPLITS, "n_splits %d: 0 .. %d", p->n_splits,
                 HIPREC_SGL_MAX_SPLITS);
  if (p->ssl_sides) {
    HIPREC_REQUIRE(p->ssl_temp > 0.f, "ssl_temp must be positive");
    HIPREC_REQUIRE(p->s.rowptr && p->s.n_rows == p->a.n_rows && p->s.nnz >= 0 && (p->s.nnz == 0 || p->s.col),
                   "bad sub-graph CSR s");
    for (int v = 0; v < 2; ++v)
      for (int l = 0; l < p->n_layers; ++l)
        HIPREC_REQUIRE(p->s.nnz == 0 || p->sub_val[v][l] != nullptr, "NULL sub_val[%d][%d]", v, l);
  }
  return 0;
}

static hiprec_csr sgl_layer_graph(const hiprec_sgl_plan* p, int view, int l, bool transposed) {
  if (view == 0) return transposed ? p->at : p->a;
  hiprec_csr g = p->s;   // symmetric: its own transpose
  g.val = p->sub_val[view - 1][l];
  g.eid = nullptr;
  return g;
}

// pool = E_0 + ... + E_L of one view
static int sgl_forward_view(const hiprec_sgl_plan* p, int view, float* pool, hipStream_t st) {
  const SglWs w = sgl_ws(p);
  const int64_t nd = p->a.n_rows * p->dim;
  HIPREC_TRY(hipMemcpyAsync(pool, p->e0, sizeof(float) * nd, hipMemcpyDeviceToDevice, st));
  const float* cur = p->e0;
  for (int l = 0; l < p->n_layers; ++l) {
    const hiprec_csr g = sgl_layer_graph(p, view, l, false);
    float* nxt = (l & 1) ? w.pong : w.ping;
    if (int rc = launch_spmm(&g, nullptr, 1.f, cur, nxt, pool, p->dim, st, false)) return rc;
    cur = nxt;
  }
  return 0;
}

// g += sum_l (M_0^T ... M_{l-1}^T) d: d enters at every hop, dE_l = d + M_l^T dE_{l+1}
static int sgl_backward_view(const hiprec_sgl_plan* p, int view, const float* d, hipStream_t st) {
  const SglWs w = sgl_ws(p);
  const int64_t nd = p->a.n_rows * p->dim;
  const float* t = d;
  for (int l = p->n_layers - 1; l >= 0; --l) {
    const hiprec_csr g = sgl_layer_graph(p, view, l, true);
    float* dst = l == 0 ? p->g : ((l & 1) ? w.pong : w.ping);
    if (l != 0) HIPREC_TRY(hipMemcpyAsync(dst, d, sizeof(float) * nd, hipMemcpyDeviceToDevice, st));
    // the SpMM only ever ADDS into its output, so with y_is_zero it accumulates onto what is there
    if (int rc = launch_spmm(&g, nullptr, 1.f, t, dst, nullptr, p->dim, st, true)) return rc;
    t = dst;
  }
  sgl_add_kernel<<<grid_for_threads(nd), kBlock, 0, st>>>(p->g, d, nd);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

static std::atomic<uint64_t> g_sgl_lds_ok{0};

static int sgl_allow_lds() {
  return allow_dynamic_lds({reinterpret_cast<const void*>(&sgl_nce_fwd_kernel),
                            reinterpret_cast<const void*>(&sgl_nce_dq_kernel<1>),
                            reinterpret_cast<const void*>(&sgl_nce_dq_kernel<2>),
                            reinterpret_cast<const void*>(&sgl_nce_dq_kernel<4>),
                            reinterpret_cast<const void*>(&sgl_nce_dk_kernel<1>),
                            reinterpret_cast<const void*>(&sgl_nce_dk_kernel<2>),
                            reinterpret_cast<const void*>(&sgl_nce_dk_kernel<4>)},
                           sgl_lds_bytes(256, true), g_sgl_lds_ok, "SGL's InfoNCE tiles");
}

// forward + backward of one side's InfoNCE term; row_loss gets the per-row loss
static int sgl_nce_side(const hiprec_sgl_plan* p, const SglWs& w, SglSide side, int64_t batch, float* logsum,
                        float* row_loss, float* partial, float* dq, hipStream_t st) {
  const int D = p->dim;
  const float inv_temp = 1.0f / p->ssl_temp, coef = p->ssl_reg / p->ssl_temp;
  const int64_t b_tiles = (batch + kSglTB - 1) / kSglTB, n_tiles = (side.n + kSglTN - 1) / kSglTN;
  // enough blocks to fill the part (256 CUs, two resident blocks each at the common widths)
  int64_t want = p->n_splits > 0 ? p->n_splits : (512 + b_tiles - 1) / b_tiles;
  want = std::max<int64_t>(1, std::min<int64_t>({want, n_tiles, HIPREC_SGL_MAX_SPLITS}));
  const int tps = static_cast<int>((n_tiles + want - 1) / want);
  const int n_splits = static_cast<int>((n_tiles + tps - 1) / tps);
  HIPREC_REQUIRE(b_tiles < (1ll << 31) && n_tiles < (1ll << 31), "batch / side too large for one launch");
  sgl_nce_fwd_kernel<<<dim3(static_cast<unsigned>(b_tiles), n_splits), kBlock, sgl_lds_bytes(D, false), st>>>(
      w.x1, w.x2, side, batch, D, inv_temp, tps, n_splits, partial);
  HIPREC_TRY(hipGetLastError());
  sgl_nce_combine_kernel<<<grid_for_waves(batch), kBlock, 0, st>>>(w.x1, w.x2, side, batch, D, inv_temp, p->ssl_reg,
                                                                  n_splits, partial, logsum, row_loss);
  HIPREC_TRY(hipGetLastError());
  const size_t lds = sgl_lds_bytes(D, true);
  const int gq = static_cast<int>(b_tiles), gk = static_cast<int>(n_tiles);
  if (D <= 64) {
    sgl_nce_dq_kernel<1><<<gq, kBlock, lds, st>>>(w.x1, w.x2, side, batch, D, inv_temp, coef, logsum, dq);
    sgl_nce_dk_kernel<1><<<gk, kBlock, lds, st>>>(w.x1, w.x2, side, batch, D, inv_temp, coef, logsum, w.d2);
  } else if (D <= 128) {
    sgl_nce_dq_kernel<2><<<gq, kBlock, lds, st>>>(w.x1, w.x2, side, batch, D, inv_temp, coef, logsum, dq);
    sgl_nce_dk_kernel<2><<<gk, kBlock, lds, st>>>(w.x1, w.x2, side, batch, D, inv_temp, coef, logsum, w.d2);
  } else {
    sgl_nce_dq_kernel<4><<<gq, kBlock, lds, st>>>(w.x1, w.x2, side, batch, D, inv_temp, coef, logsum, dq);
    sgl_nce_dk_kernel<4><<<gk, kBlock, lds, st>>>(w.x1, w.x2, side, batch, D, inv_temp, coef, logsum, w.d2);
  }
  HIPREC_TRY(hipGetLastError());
  const float scale = 1.0f / static_cast<float>(p->n_layers + 1);
  sgl_norm_bwd_scatter_kernel<<<grid_for_waves(batch), kBlock, 0, st>>>(dq, side, batch, w.x1, w.inv1, w.d1, D, scale);
  sgl_norm_bwd_kernel<<<grid_for_waves(side.n), kBlock, 0, st>>>(w.d2, w.x2, w.inv2, side.off, side.n, D, scale);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_sgl_plan_bytes(void) { return sizeof(hiprec_sgl_plan); }
extern "C" int32_t hiprec_sgl_tile_b(void) { return kSglTB; }
extern "C" int32_t hiprec_sgl_tile_n(void) { return kSglTN; }
extern "C" int64_t hiprec_sgl_ws_floats(int64_t n_rows, int32_t dim) { return sgl_ws_floats(n_rows, dim); }
extern "C" int64_t hiprec_sgl_batch_ws_floats(int64_t batch, int32_t dim) { return sgl_batch_floats(batch, dim); }

extern "C" int hiprec_sgl_sub_values(const hiprec_csr* s, const int32_t* edge_inter, const uint8_t* keep,
                                     const uint8_t* keep_user, const uint8_t* keep_item, int64_t n_users, float* deg,
                                     float* val, void* stream) {
  HIPREC_REQUIRE(s && s->rowptr && s->n_rows > 0 && s->nnz >= 0 && (s->nnz == 0 || s->col), "bad CSR s");
  HIPREC_REQUIRE(deg && (s->nnz == 0 || val), "NULL deg / val");
  HIPREC_REQUIRE(keep == nullptr || edge_inter != nullptr || s->nnz == 0, "keep bytes need edge_inter");
  HIPREC_REQUIRE((keep_user == nullptr) == (keep_item == nullptr), "keep_user and keep_item go together");
  HIPREC_REQUIRE(n_users > 0 && n_users < s->n_rows, "bad n_users");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = grid_for_threads(s->n_rows);
  sgl_degree_kernel<<<grid, kBlock, 0, st>>>(*s, edge_inter, keep, keep_user, keep_item, n_users, deg);
  sgl_values_kernel<<<grid, kBlock, 0, st>>>(*s, edge_inter, keep, keep_user, keep_item, n_users, deg, val);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_sgl_propagate(const hiprec_sgl_plan* plan, void* stream) {
  if (int rc = check_sgl_plan(plan, false)) return rc;
  return sgl_forward_view(plan, 0, sgl_ws(plan).pool, static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_sgl_predict(const hiprec_sgl_plan* plan, const int64_t* users, const int64_t* items, int64_t n,
                                  float* scores, hiprec_stats* stats, void* stream) {
  if (int rc = check_sgl_plan(plan, false)) return rc;
  if (n == 0) return 0;
  HIPREC_REQUIRE(n > 0 && users && items && scores && stats, "NULL pointer");
  sgl_predict_kernel<<<grid_for_waves(n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      sgl_ws(plan).pool, plan->n_users, plan->n_items, plan->dim, 1.0f / static_cast<float>(plan->n_layers + 1), users,
      items, n, scores, stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_sgl_grad(const hiprec_sgl_plan* plan, const int64_t* users, const int64_t* pos, const int64_t* neg,
                               int64_t batch, float* parts, hiprec_stats* stats, void* scratch, size_t scratch_bytes,
                               void* stream) {
  if (int rc = check_sgl_plan(plan, true)) return rc;
  const hiprec_sgl_plan* p = plan;
  HIPREC_REQUIRE(batch > 0 && users && pos && neg && parts && stats && scratch, "NULL pointer / empty batch");
  HIPREC_REQUIRE(p->batch_ws && p->batch_ws_floats >= sgl_batch_floats(batch, p->dim),
                 "batch_ws holds %lld floats, %lld are needed", (long long)p->batch_ws_floats,
                 (long long)sgl_batch_floats(batch, p->dim));
  if (scratch_bytes < kScratchBytes) {
    set_error("scratch too small: %zu < %zu", scratch_bytes, kScratchBytes);
    return HIPREC_E_SCRATCH;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const SglWs w = sgl_ws(p);
  const int D = p->dim;
  const int64_t N = p->a.n_rows, nd = N * D;
  const float scale = 1.0f / static_cast<float>(p->n_layers + 1);
  float* logsum = p->batch_ws;               // [2][batch]
  float* rows = logsum + 2 * batch;          // [4][batch]: bpr, emb, ssl user side, ssl item side
  float* partial = rows + 4 * batch;         // [batch][n_splits] of the side at work
  float* dq = partial + 2 * batch * HIPREC_SGL_MAX_SPLITS;   // [batch][dim] of the side at work
  const bool ssl = p->ssl_sides != 0;

  // d0 and d1 collect row atomics; d2 is stored row by row on the sides that take part, the other side stays zero
  HIPREC_TRY(hipMemsetAsync(w.d0, 0, sizeof(float) * (ssl ? 2 : 1) * nd, st));
  if (ssl && p->ssl_sides != 3) HIPREC_TRY(hipMemsetAsync(w.d2, 0, sizeof(float) * nd, st));

  if (int rc = sgl_forward_view(p, 0, w.pool, st)) return rc;
  int n_ssl = 0;
  if (ssl) {
    if (int rc = sgl_allow_lds()) return rc;
    if (int rc = sgl_forward_view(p, 1, w.x1, st)) return rc;
    if (int rc = sgl_forward_view(p, 2, w.x2, st)) return rc;
    sgl_normalize_kernel<<<grid_for_waves(N), kBlock, 0, st>>>(w.x1, w.inv1, N, D, scale);
    sgl_normalize_kernel<<<grid_for_waves(N), kBlock, 0, st>>>(w.x2, w.inv2, N, D, scale);
    HIPREC_TRY(hipGetLastError());
    if (p->ssl_sides & 1) {
      if (int rc = sgl_nce_side(p, w, SglSide{users, 0, p->n_users}, batch, logsum, rows + (2 + n_ssl) * batch, partial,
                                dq, st))
        return rc;
      ++n_ssl;
    }
    if (p->ssl_sides & 2) {
      if (int rc = sgl_nce_side(p, w, SglSide{pos, p->n_users, p->n_items}, batch, logsum + batch,
                                rows + (2 + n_ssl) * batch, partial, dq, st))
        return rc;
      ++n_ssl;
    }
  }
  const int grid = grid_for_waves(batch);
  if (D <= 64)
    sgl_bpr_kernel<1><<<grid, kBlock, 0, st>>>(*p, w.pool, w.d0, users, pos, neg, batch, scale, rows, rows + batch, stats);
  else if (D <= 128)
    sgl_bpr_kernel<2><<<grid, kBlock, 0, st>>>(*p, w.pool, w.d0, users, pos, neg, batch, scale, rows, rows + batch, stats);
  else
    sgl_bpr_kernel<4><<<grid, kBlock, 0, st>>>(*p, w.pool, w.d0, users, pos, neg, batch, scale, rows, rows + batch, stats);
  sgl_finish_kernel<<<1, kBlock, 0, st>>>(rows, batch, n_ssl, parts, stats, static_cast<Scratch*>(scratch));
  HIPREC_TRY(hipGetLastError());

  if (int rc = sgl_backward_view(p, 0, w.d0, st)) return rc;
  if (ssl) {
    if (int rc = sgl_backward_view(p, 1, w.d1, st)) return rc;
    if (int rc = sgl_backward_view(p, 2, w.d2, st)) return rc;
  }
  return 0;
}
