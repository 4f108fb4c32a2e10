// EASE (Steck, "Embarrassingly Shallow Autoencoders for Sparse Data", WWW 2019) for gfx950: the closed-form item
// autoencoder.  No counterpart in the reference.
//
//   X binary [n_users, n_items]     G = X^T X + reg I     P = G^-1     B[i, j] = -P[i, j] / P[j, j],  B[j, j] = 0
//
// Three stages, none with a float atomic; every rounded value has one owner and a fixed order of operations, so the same
// input gives the same bits whatever the grid.
//
//   gram     one block per item row i (block-stride): the distinct users of column i, their distinct items, counted in an
//            integer accumulator (LDS, or the block's slice of the workspace when the row does not fit: knn.hip's scheme
//            without the touched list, because the whole row is written anyway).  Plain fp32 stores, reg on the diagonal.
//   invert   right-looking blocked Cholesky A = L L^T in place (lower triangle, panels of HIPREC_EASE_PANEL columns) that
//            carries the forward substitution W = L^-1 along in the workspace, then P = W^T W over the lower triangle.
//            Per panel k, four launches:
//              potrf   the diagonal block in one wave's registers, sqrtf and operator/ (correctly rounded in every build)
//              trsm    L21 = A21 L11^-T by substitution, one lane per row (no explicit inverse of the diagonal block)
//              solve   W[k, :] = L11^-1 R[k, :] by substitution, one lane per column (R starts as I and lives in W)
//              update  A22 -= L21 L21^T over the lower-triangle tiles and R[i > k, :] -= L21 W[k, :], both on
//                      v_mfma_f32_16x16x4_f32: a 64 x 64 tile per block, 32 x 32 per wave in four accumulators that start
//                      from zero (a k-ordered fmaf chain of the panel's 64 products), subtracted from C once.
//            and one last launch for P = W^T W (lower tiles; tile (I, J) sums k from the first row of tile I to n, each
//            64 rows on their own and the chunks in order).
//            A pivot that is not positive and finite sets HIPREC_STATUS_NOT_SPD; every later launch reads the word first
//            and does nothing.
//   finish   B from the lower triangle of P, both triangles written, the diagonal +0; P's upper triangle is mirrored so
//            the caller may keep the inverse.
//
// Bounds: every tile load and store is guarded by the row and column being < n; LDS tiles are padded with zeros (the
// diagonal block with the identity), so a ragged last panel runs the same code.  Only the last panel can be ragged and it
// has nothing below it: the MFMA updates always have K = HIPREC_EASE_PANEL.
//
// LDS: [row][k] operand tiles use a row stride of 4 mod 64 floats and [k][column] tiles one of 16 mod 64, so the 64 lanes
// of an MFMA operand load (16 rows x 4 k, or 4 k x 16 columns) fall into different banks.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace hiprec {
namespace {

using ease_f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kEaseNb = HIPREC_EASE_PANEL;       // panel width = K of every update
constexpr int kEaseTile = HIPREC_EASE_TILE;      // rows and columns of a block's output tile
constexpr int kEaseSub = kEaseTile / 2;          // ... of a wave's
constexpr int kEaseRk = kEaseNb + 4;             // stride of a [row][k] tile
constexpr int kEaseKc = kEaseTile + 16;          // stride of a [k][column] tile
constexpr int kEaseSq = kEaseNb + 1;             // stride of the substitution tiles
constexpr int kEaseGramBlocks = 1024;
static_assert(kEaseNb == 64 && kEaseTile == 64 && kWavesPerBlock == 4, "four waves, 32 x 32 each; one lane per panel row");
static_assert(kEaseNb % HIPREC_EASE_MFMA == 0 && kEaseSub == 2 * HIPREC_EASE_MFMA, "a wave holds 2 x 2 MFMA tiles");

__device__ __forceinline__ bool ease_stopped(const hiprec_stats* stats) {
  return (*reinterpret_cast<const volatile uint32_t*>(&stats->status) & HIPREC_STATUS_NOT_SPD) != 0;
}

// ---------------------------------------------------------------- gram
struct EaseGramArgs {
  const int64_t* bt_ptr;
  const int64_t* bt_idx;
  const int64_t* b_ptr;
  const int64_t* b_idx;
  float* G;
  unsigned* ws;
  hiprec_stats* stats;
  int64_t n_users, n_items;
  float reg;
};

template <bool WS>
__global__ __launch_bounds__(kBlock) void ease_gram_kernel(const EaseGramArgs a) {
  extern __shared__ unsigned ease_lds[];
  const int tid = static_cast<int>(threadIdx.x), lane = lane_id(), wv = wave_in_block();
  unsigned* acc = WS ? a.ws + static_cast<size_t>(blockIdx.x) * a.n_items : ease_lds;   // (WS: zeroed by the entry point)
  if constexpr (!WS) {
    for (int64_t j = tid; j < a.n_items; j += kBlock) acc[j] = 0;
  }
  __syncthreads();
  for (int64_t i = blockIdx.x; i < a.n_items; i += gridDim.x) {
    // one wave per user of column i, its lanes over the user's row (rows are unique: every pair counts once)
    for (int64_t e = a.bt_ptr[i] + wv; e < a.bt_ptr[i + 1]; e += kWavesPerBlock) {
      const int64_t v = a.bt_idx[e];
      if (v < 0 || v >= a.n_users) {
        if (lane == 0) atomicOr(&a.stats->status, HIPREC_STATUS_USER_OOB);
        continue;
      }
      for (int64_t t = a.b_ptr[v] + lane; t < a.b_ptr[v + 1]; t += kWave) {
        const int64_t j = a.b_idx[t];
        if (j < 0 || j >= a.n_items) {
          atomicOr(&a.stats->status, HIPREC_STATUS_ITEM_OOB);
          continue;
        }
        atomicAdd(&acc[j], 1u);
      }
    }
    __syncthreads();
    float* out = a.G + i * a.n_items;
    for (int64_t j = tid; j < a.n_items; j += kBlock) {
      const float c = static_cast<float>(acc[j]);   // < 2^24: exact
      out[j] = j == i ? c + a.reg : c;
      acc[j] = 0;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- invert
// The diagonal block of panel k0 (nb columns) as a 64 x 64 lower-triangular LDS tile, the identity outside nb
__device__ __forceinline__ void ease_load_diag(float* Ls, const float* A, int64_t n, int64_t k0, int nb) {
  for (int e = threadIdx.x; e < kEaseNb * kEaseNb; e += kBlock) {
    const int r = e / kEaseNb, c = e - r * kEaseNb;
    Ls[r * kEaseSq + c] = (r < nb && c <= r) ? A[(k0 + r) * n + k0 + c] : (r == c ? 1.f : 0.f);
  }
}

__global__ __launch_bounds__(kBlock) void ease_identity_kernel(float* W, int64_t n) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kBlock)
    W[i * n + i] = 1.f;
}

// A11 = L11 L11^T by ONE wave without LDS or barriers: lane i holds row i of the (identity-padded) block in 64
// registers; step j takes the pivot and column j from the other lanes by v_readlane.  Right-looking, the same operations
// in the same order as the textbook loop: L[i][j] = A[i][j] / sqrt(A[j][j]), then A[i][k] = fma(-L[i][j], L[k][j], A[i][k]).
// A lane's entries right of its diagonal are scratch (never read by another lane, never stored).
__global__ __launch_bounds__(kWave) void ease_potrf_kernel(float* A, int64_t n, int64_t k0, int nb, hiprec_stats* stats) {
  if (ease_stopped(stats)) return;
  const int i = static_cast<int>(threadIdx.x);
  float* row = A + (k0 + i) * n + k0;               // (dereferenced only when i < nb)
  float a[kEaseNb];
#pragma unroll
  for (int c = 0; c < kEaseNb; ++c) a[c] = (i < nb && c <= i) ? row[c] : (c == i ? 1.f : 0.f);
#pragma unroll
  for (int j = 0; j < kEaseNb; ++j) {
    const float piv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a[j]), j));
    if (!(piv > 0.f) || !(piv < INFINITY)) {        // uniform: one scalar value
      if (i == 0) atomicOr(&stats->status, HIPREC_STATUS_NOT_SPD);
      return;                                       // A keeps the block unfactorised
    }
    const float d = sqrtf(piv);
    const float lj = i == j ? d : a[j] / d;
    a[j] = lj;
#pragma unroll
    for (int k = j + 1; k < kEaseNb; ++k) {
      const float lkj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, lj), k));
      a[k] = __builtin_fmaf(-lj, lkj, a[k]);
    }
  }
  if (i < nb) {
#pragma unroll
    for (int c = 0; c < kEaseNb; ++c)
      if (c <= i) row[c] = a[c];
  }
}

// Forward substitution against the lower-triangular LDS tile Ls, the right-hand side in registers: for j ascending
// x_j = s_j / L[j][j], then s_k = fma(-x_j, L[k][j], s_k) for every k > j.  Each s_k subtracts its products in ascending j,
// as a dot-product loop would, but the 63 - j updates of a step are independent of each other.
__device__ __forceinline__ void ease_substitute(float (&s)[kEaseNb], const float* Ls) {
#pragma unroll
  for (int j = 0; j < kEaseNb; ++j) {
    const float x = s[j] / Ls[j * kEaseSq + j];
    s[j] = x;
#pragma unroll
    for (int k = j + 1; k < kEaseNb; ++k) s[k] = __builtin_fmaf(-x, Ls[k * kEaseSq + j], s[k]);
  }
}

// L21 = A21 L11^-T: block b owns rows k0 + 64 + 64 b ...; lane r of wave 0 substitutes along its row
// (x_j = (a_j - sum_{q < j} x_q L11[j][q]) / L11[j][j])
__global__ __launch_bounds__(kBlock) void ease_trsm_kernel(float* A, int64_t n, int64_t k0, const hiprec_stats* stats) {
  __shared__ float Ls[kEaseNb * kEaseSq];
  __shared__ float T[kEaseTile * kEaseSq];
  if (ease_stopped(stats)) return;
  const int tid = static_cast<int>(threadIdx.x);
  const int64_t r0 = k0 + kEaseNb + static_cast<int64_t>(blockIdx.x) * kEaseTile;
  ease_load_diag(Ls, A, n, k0, kEaseNb);
  for (int e = tid; e < kEaseTile * kEaseNb; e += kBlock) {
    const int r = e / kEaseNb, c = e - r * kEaseNb;
    T[r * kEaseSq + c] = (r0 + r < n) ? A[(r0 + r) * n + k0 + c] : 0.f;
  }
  __syncthreads();
  if (tid < kEaseTile) {
    float s[kEaseNb];
#pragma unroll
    for (int c = 0; c < kEaseNb; ++c) s[c] = T[tid * kEaseSq + c];
    ease_substitute(s, Ls);
#pragma unroll
    for (int c = 0; c < kEaseNb; ++c) T[tid * kEaseSq + c] = s[c];
  }
  __syncthreads();
  for (int e = tid; e < kEaseTile * kEaseNb; e += kBlock) {
    const int r = e / kEaseNb, c = e - r * kEaseNb;
    if (r0 + r < n) A[(r0 + r) * n + k0 + c] = T[r * kEaseSq + c];
  }
}

// W[k0 .. k0 + nb, 0 .. k0 + nb) = L11^-1 R[same]: block b owns 64 columns; lane c of wave 0 substitutes down its column
// (rows >= nb of the padded tile are zeros over an identity: they stay zeros and are not stored)
__global__ __launch_bounds__(kBlock) void ease_solve_kernel(const float* A, float* W, int64_t n, int64_t k0, int nb,
                                                            const hiprec_stats* stats) {
  __shared__ float Ls[kEaseNb * kEaseSq];
  __shared__ float T[kEaseNb * kEaseSq];
  if (ease_stopped(stats)) return;
  const int tid = static_cast<int>(threadIdx.x);
  const int64_t c0 = static_cast<int64_t>(blockIdx.x) * kEaseTile, c_end = k0 + nb;
  ease_load_diag(Ls, A, n, k0, nb);
  for (int e = tid; e < kEaseNb * kEaseTile; e += kBlock) {
    const int r = e / kEaseTile, c = e - r * kEaseTile;
    T[r * kEaseSq + c] = (r < nb && c0 + c < c_end) ? W[(k0 + r) * n + c0 + c] : 0.f;
  }
  __syncthreads();
  if (tid < kEaseTile) {
    float s[kEaseNb];
#pragma unroll
    for (int r = 0; r < kEaseNb; ++r) s[r] = T[r * kEaseSq + tid];
    ease_substitute(s, Ls);
#pragma unroll
    for (int r = 0; r < kEaseNb; ++r) T[r * kEaseSq + tid] = s[r];
  }
  __syncthreads();
  for (int e = tid; e < kEaseNb * kEaseTile; e += kBlock) {
    const int r = e / kEaseTile, c = e - r * kEaseTile;
    if (r < nb && c0 + c < c_end) W[(k0 + r) * n + c0 + c] = T[r * kEaseSq + c];
  }
}

// The wave's 32 x 32 part of C (rows row0 ..., columns col0 ... of a matrix with n columns), guarded; C/D map of the
// 16 x 16 MFMA: column = lane & 15, row = 4 (lane >> 4) + register
template <typename F>
__device__ __forceinline__ void ease_each_entry(int64_t row0, int64_t col0, F f) {
  const int l = lane_id();
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int q = 0; q < 4; ++q) f(ti, tj, q, row0 + ti * 16 + 4 * (l >> 4) + q, col0 + tj * 16 + (l & 15));
}

// Both updates of panel k0 (a full panel: rows exist below it).  blockIdx.x = I, the tile row below the panel.
//   blockIdx.y <  m:  A22 tile (I, J = y), J <= I:       C -= L21[I] L21[J]^T      (lower part only on the diagonal)
//   blockIdx.y >= m:  R tile (I, J = y - m), columns 64 J ... < k0 + 64:   C -= L21[I] W[k0 ..., J]
__global__ __launch_bounds__(kBlock) void ease_update_kernel(float* A, float* W, int64_t n, int64_t k0, int m,
                                                             const hiprec_stats* stats) {
  __shared__ float As[kEaseTile * kEaseRk];
  __shared__ float Bs[kEaseNb * kEaseKc];     // [column][k] (stride kEaseRk) for A22, [k][column] (stride kEaseKc) for R
  if (ease_stopped(stats)) return;
  const int I = blockIdx.x;
  const bool syrk = static_cast<int>(blockIdx.y) < m;
  const int J = syrk ? blockIdx.y : blockIdx.y - m;
  if (syrk && J > I) return;
  const int tid = static_cast<int>(threadIdx.x), l = lane_id(), w = wave_in_block();
  const int64_t k1 = k0 + kEaseNb, row0 = k1 + static_cast<int64_t>(I) * kEaseTile;
  const int64_t col0 = syrk ? k1 + static_cast<int64_t>(J) * kEaseTile : static_cast<int64_t>(J) * kEaseTile;
  float* C = syrk ? A : W;
  for (int e = tid; e < kEaseTile * kEaseNb; e += kBlock) {
    const int r = e / kEaseNb, c = e - r * kEaseNb;
    As[r * kEaseRk + c] = (row0 + r < n) ? A[(row0 + r) * n + k0 + c] : 0.f;
    if (syrk) Bs[r * kEaseRk + c] = (col0 + r < n) ? A[(col0 + r) * n + k0 + c] : 0.f;
    else Bs[r * kEaseKc + c] = (col0 + c < n) ? W[(k0 + r) * n + col0 + c] : 0.f;      // (k0 + r < n: a full panel)
  }
  __syncthreads();
  const int wr = w >> 1, wc = w & 1;
  if (syrk && I == J && wc > wr) return;       // strictly above the diagonal
  const int64_t wrow = row0 + wr * kEaseSub, wcol = col0 + wc * kEaseSub;
  ease_f32x4 acc[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = ease_f32x4{0.f, 0.f, 0.f, 0.f};
  const float* ap = As + (wr * kEaseSub + (l & 15)) * kEaseRk + (l >> 4);
  const int sc = syrk ? kEaseRk : 1, sk = syrk ? 1 : kEaseKc;
  const float* bp = Bs + (wc * kEaseSub + (l & 15)) * sc + (l >> 4) * sk;
  for (int k = 0; k < kEaseNb; k += 4) {
    const float a0 = ap[k], a1 = ap[k + 16 * kEaseRk];
    const float b0 = bp[k * sk], b1 = bp[k * sk + 16 * sc];
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
  }
  // one subtraction per panel: C is large against the products, so a chain through C would round at C's magnitude once
  // per k (n times in all) where this rounds there once per panel
  const bool lower_only = syrk && I == J;
  ease_each_entry(wrow, wcol, [&](int ti, int tj, int q, int64_t r, int64_t c) {
    if (r < n && c < n && (!lower_only || c <= r)) C[r * n + c] = C[r * n + c] - acc[ti][tj][q];
  });
}

// P = W^T W, lower tiles into A: tile (I, J <= I) sums k over the rows of W from 64 I to n, 64 at a time (W is lower
// triangular with exact zeros above the diagonal, so the rows before 64 I add nothing)
__global__ __launch_bounds__(kBlock) void ease_wtw_kernel(float* A, const float* W, int64_t n, const hiprec_stats* stats) {
  __shared__ float Wa[kEaseNb * kEaseKc];
  __shared__ float Wb[kEaseNb * kEaseKc];
  if (ease_stopped(stats)) return;
  const int I = blockIdx.x, J = blockIdx.y;
  if (J > I) return;
  const int tid = static_cast<int>(threadIdx.x), l = lane_id(), w = wave_in_block();
  const int wr = w >> 1, wc = w & 1;
  const int64_t row0 = static_cast<int64_t>(I) * kEaseTile, col0 = static_cast<int64_t>(J) * kEaseTile;
  const bool idle = I == J && wc > wr;         // (stays for the barriers)
  ease_f32x4 acc[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = ease_f32x4{0.f, 0.f, 0.f, 0.f};
  const float* ap = Wa + (l >> 4) * kEaseKc + wr * kEaseSub + (l & 15);
  const float* bp = Wb + (l >> 4) * kEaseKc + wc * kEaseSub + (l & 15);
  for (int64_t kb = row0; kb < n; kb += kEaseNb) {
    __syncthreads();                           // the chunk before is consumed
    for (int e = tid; e < kEaseNb * kEaseTile; e += kBlock) {
      const int r = e / kEaseTile, c = e - r * kEaseTile;
      const bool in = kb + r < n;
      Wa[r * kEaseKc + c] = (in && row0 + c < n) ? W[(kb + r) * n + row0 + c] : 0.f;
      Wb[r * kEaseKc + c] = (in && col0 + c < n) ? W[(kb + r) * n + col0 + c] : 0.f;
    }
    __syncthreads();
    if (!idle) {
      ease_f32x4 part[2][2];                   // the chunk on its own, then one addition: as in the update above
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) part[ti][tj] = ease_f32x4{0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < kEaseNb; k += 4) {
        const float a0 = ap[k * kEaseKc], a1 = ap[k * kEaseKc + 16];
        const float b0 = bp[k * kEaseKc], b1 = bp[k * kEaseKc + 16];
        part[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, part[0][0], 0, 0, 0);
        part[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, part[0][1], 0, 0, 0);
        part[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, part[1][0], 0, 0, 0);
        part[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, part[1][1], 0, 0, 0);
      }
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) acc[ti][tj] += part[ti][tj];
    }
  }
  if (idle) return;
  ease_each_entry(row0 + wr * kEaseSub, col0 + wc * kEaseSub, [&](int ti, int tj, int q, int64_t r, int64_t c) {
    if (r < n && c < n && c <= r) A[r * n + c] = acc[ti][tj][q];
  });
}

// ---------------------------------------------------------------- finish
__global__ __launch_bounds__(kBlock) void ease_finish_kernel(float* P, int64_t n, float* B, const hiprec_stats* stats) {
  if (ease_stopped(stats)) return;
  const int64_t total = n * n;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < total;
       e += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t i = e / n, j = e - i * n;
    if (j > i) continue;
    if (i == j) {
      B[e] = 0.f;
      continue;
    }
    const float p = P[e];
    B[e] = -p / P[j * n + j];
    B[j * n + i] = -p / P[i * n + i];
    P[j * n + i] = p;
  }
}

// ---------------------------------------------------------------- host side
bool ease_sizes_ok(int64_t n_users, int64_t n_items) {
  return n_users >= 1 && n_users < HIPREC_EASE_MAX_USERS && n_items >= 1 && n_items <= HIPREC_EASE_MAX_ITEMS;
}

bool ease_gram_in_lds(int64_t n_items, int32_t lds_cap) {
  const int64_t cap = (lds_cap == 0 || lds_cap > HIPREC_EASE_LDS_CAP) ? HIPREC_EASE_LDS_CAP : lds_cap;
  return n_items <= cap;
}

// blocks of the workspace form: at most n / 2, so that their slices fit the [n, n] fp32 workspace of the inversion
int64_t ease_gram_ws_blocks(int64_t n_items) {
  return std::min<int64_t>(std::max<int64_t>(n_items / 2, 1), kEaseGramBlocks);
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_ease_workspace_bytes(int64_t n_users, int64_t n_items) {
  if (!ease_sizes_ok(n_users, n_items)) return static_cast<size_t>(-1);
  const size_t n = static_cast<size_t>(n_items);
  const size_t inverse = n * n * sizeof(float);
  const size_t gram = static_cast<size_t>(ease_gram_ws_blocks(n_items)) * n * sizeof(unsigned);
  return (std::max(inverse, gram) + 7) / 8 * 8;
}

extern "C" int hiprec_ease_gram(const int64_t* bt_ptr, const int64_t* bt_idx, const int64_t* b_ptr, const int64_t* b_idx,
                                int64_t n_users, int64_t n_items, float reg, float* G, int32_t lds_cap, void* workspace,
                                size_t workspace_bytes, hiprec_stats* stats, void* stream) {
  HIPREC_REQUIRE(ease_sizes_ok(n_users, n_items) && lds_cap >= 0,
                 "ease_gram: bad sizes (n_users=%lld n_items=%lld lds_cap=%d; n_users < 2^24 keeps an fp32 count exact)",
                 (long long)n_users, (long long)n_items, lds_cap);
  HIPREC_REQUIRE(reg > 0.f && std::isfinite(reg), "ease_gram: reg=%g must be finite and > 0", (double)reg);
  HIPREC_REQUIRE(stats != nullptr, "ease_gram: NULL stats");
  HIPREC_REQUIRE(bt_ptr && bt_idx && b_ptr && b_idx && G, "ease_gram: NULL pointer");
  const bool in_lds = ease_gram_in_lds(n_items, lds_cap);
  const int64_t ws_blocks = ease_gram_ws_blocks(n_items);
  const size_t need = in_lds ? 0 : static_cast<size_t>(ws_blocks) * static_cast<size_t>(n_items) * sizeof(unsigned);
  HIPREC_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need), "ease_gram: workspace %zu B < %zu B",
                 workspace_bytes, need);
  EaseGramArgs a{bt_ptr, bt_idx, b_ptr, b_idx, G, static_cast<unsigned*>(workspace), stats, n_users, n_items, reg};
  auto s = static_cast<hipStream_t>(stream);
  if (in_lds) {
    const unsigned grid = static_cast<unsigned>(std::min<int64_t>(n_items, kEaseGramBlocks));
    ease_gram_kernel<false><<<grid, kBlock, sizeof(unsigned) * static_cast<size_t>(n_items), s>>>(a);
  } else {
    HIPREC_TRY(hipMemsetAsync(workspace, 0, need, s));
    ease_gram_kernel<true><<<static_cast<unsigned>(ws_blocks), kBlock, 0, s>>>(a);
  }
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_ease_invert(float* A, int64_t n, void* workspace, size_t workspace_bytes, hiprec_stats* stats,
                                  void* stream) {
  HIPREC_REQUIRE(n >= 1 && n <= HIPREC_EASE_MAX_ITEMS, "ease_invert: bad size (n=%lld; 1..%d)", (long long)n,
                 HIPREC_EASE_MAX_ITEMS);
  HIPREC_REQUIRE(stats != nullptr, "ease_invert: NULL stats");
  HIPREC_REQUIRE(A != nullptr, "ease_invert: NULL pointer");
  const size_t need = static_cast<size_t>(n) * static_cast<size_t>(n) * sizeof(float);
  HIPREC_REQUIRE(workspace != nullptr && workspace_bytes >= need, "ease_invert: workspace %zu B < %zu B", workspace_bytes,
                 need);
  HIPREC_REQUIRE(static_cast<void*>(A) != workspace, "ease_invert: the workspace is the matrix itself");
  auto s = static_cast<hipStream_t>(stream);
  float* W = static_cast<float*>(workspace);
  HIPREC_TRY(hipMemsetAsync(W, 0, need, s));
  ease_identity_kernel<<<grid_for_threads(n), kBlock, 0, s>>>(W, n);
  HIPREC_TRY(hipGetLastError());
  for (int64_t k0 = 0; k0 < n; k0 += kEaseNb) {
    const int nb = static_cast<int>(std::min<int64_t>(kEaseNb, n - k0));
    const int64_t below = n - k0 - nb;                                   // > 0 only behind a full panel
    const unsigned m = static_cast<unsigned>((below + kEaseTile - 1) / kEaseTile);
    ease_potrf_kernel<<<1, kWave, 0, s>>>(A, n, k0, nb, stats);
    if (m > 0) ease_trsm_kernel<<<m, kBlock, 0, s>>>(A, n, k0, stats);
    ease_solve_kernel<<<static_cast<unsigned>((k0 + nb + kEaseTile - 1) / kEaseTile), kBlock, 0, s>>>(A, W, n, k0, nb,
                                                                                                      stats);
    if (m > 0) {
      const unsigned r_tiles = static_cast<unsigned>(k0 / kEaseTile + 1);
      ease_update_kernel<<<dim3(m, m + r_tiles), kBlock, 0, s>>>(A, W, n, k0, static_cast<int>(m), stats);
    }
    HIPREC_TRY(hipGetLastError());
  }
  const unsigned t = static_cast<unsigned>((n + kEaseTile - 1) / kEaseTile);
  ease_wtw_kernel<<<dim3(t, t), kBlock, 0, s>>>(A, W, n, stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_ease_finish(float* P, int64_t n, float* B, hiprec_stats* stats, void* stream) {
  HIPREC_REQUIRE(n >= 1 && n <= HIPREC_EASE_MAX_ITEMS, "ease_finish: bad size (n=%lld; 1..%d)", (long long)n,
                 HIPREC_EASE_MAX_ITEMS);
  HIPREC_REQUIRE(stats != nullptr, "ease_finish: NULL stats");
  HIPREC_REQUIRE(P != nullptr && B != nullptr, "ease_finish: NULL pointer");
  HIPREC_REQUIRE(P != B, "ease_finish: B must not be P");
  ease_finish_kernel<<<grid_for_threads(n * n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(P, n, B, stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}
