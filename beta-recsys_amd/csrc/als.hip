// Implicit ALS (WRMF, Hu, Koren and Volinsky 2008) for gfx950: exact alternating least squares.
//
// No counterpart in the reference.  A half-sweep solves, for every row u of one side,
//   A_u = G + reg I + sum_{i in N(u)} alpha r_ui y_i y_i^T        b_u = sum_{i in N(u)} (1 + alpha r_ui) y_i
//   x_u = A_u^{-1} b_u
// with G = Y^T Y of the OTHER side's table.  Three stages, none with a float atomic:
//   gram    G = F^T F: block b reduces the 64-row tiles b, b + slots, ... on the fp32 MFMA (rows are the K dimension)
//           into its own slot; a second launch adds the slots in slot order and also writes G + reg I.
//   solve   one 256-thread block owns one row at a time (block-stride loop over a host-provided order, longest first).
//           The row's neighbours are staged into LDS 64 at a time through its CSR row; the lower-triangle 16 x 16 tiles of
//           sum w y y^T stay in MFMA accumulators across all chunks (36 tiles at D = 128, nine per wave) and b is
//           accumulated per column in the same loop.  Only after the last chunk the tiles are spilled to LDS, G + reg I
//           is added, and the block factors A = L L^T in place.  b rides along as one more row of the matrix, so the
//           forward substitution L z = b happens inside the factorisation; one backward substitution follows.
//   loss    per-row fp64 partials of  x^T G x + sum_{i in N(u)} [c (1 - s)^2 - s^2] + reg |x|^2,  folded in a fixed order.
//
// Order of every sum: neighbours in CSR order, four per MFMA (bit for bit a k-ordered fmaf chain), chunks in order; a
// chunk's last group is padded with zero rows of zero weight, which add nothing.  So a row's bits depend on the tables
// and its list, not on the grid, the chunk size or the block that took it.
//
// Square root and division: D of each per row.  sqrtf() and operator/ compile to the correctly rounded sequences in
// every build of this library (no fast-math flag is ever passed); the hardware approximations would be the largest
// error of the factorisation.
//
// LDS: the matrix and the staging tile use row strides of 16 mod 64 floats, so the 64 lanes of an MFMA operand load
// (16 consecutive floats of 4 rows) and of a trailing-update row segment fall into different banks.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace hiprec {

using als_f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kAlsChunk = HIPREC_ALS_CHUNK;
constexpr int kAlsMaxDim = HIPREC_ALS_MAX_DIM;
static_assert(kAlsChunk % 4 == 0 && kAlsChunk <= kBlock, "a chunk is whole MFMA k-groups, one index per thread");
static_assert(kAlsMaxDim % 16 == 0 && kAlsMaxDim <= 2 * kWave && kAlsMaxDim < kBlock, "one thread per column");

__host__ __device__ constexpr int als_pad16(int x) { return (x + 15) & ~15; }
__host__ __device__ constexpr int als_stride(int dp) { return ((dp + 63) & ~63) + 16; }
__host__ __device__ constexpr int als_tiles(int nt) { return nt * (nt + 1) / 2; }
__host__ __device__ constexpr int als_tiles_per_wave(int nt) {
  return (als_tiles(nt) + kWavesPerBlock - 1) / kWavesPerBlock;
}

// floats of LDS of the solve kernel: matrix [DP + 1][S] (row DP is b), staging tile [chunk][S], column [DP + 16],
// reciprocal diagonal [DP], z [DP], the chunk's weights alpha r and 1 + alpha r, the chunk's ids
__host__ __device__ constexpr int als_solve_lds_floats(int dp) {
  return (dp + 1) * als_stride(dp) + kAlsChunk * als_stride(dp) + (dp + 16) + dp + dp + 3 * kAlsChunk;
}

// this wave's lower-triangle tiles: tile t = wave + 4 i is block row ta[i], block column tb[i] (ta = -1: none)
template <int NT>
__device__ __forceinline__ void als_my_tiles(int (&ta)[als_tiles_per_wave(NT)], int (&tb)[als_tiles_per_wave(NT)]) {
  const int w = wave_in_block();
#pragma unroll
  for (int i = 0; i < als_tiles_per_wave(NT); ++i) {
    const int t = w + kWavesPerBlock * i;
    int r = 0;
    while ((r + 1) * (r + 2) / 2 <= t) ++r;
    ta[i] = t < als_tiles(NT) ? r : -1;
    tb[i] = t - r * (r + 1) / 2;
  }
}

// acc += sum over the `rows` (a multiple of 4) staged rows k of w_k y_k y_k^T, lower-triangle tiles only
template <int NT, bool WEIGHTED>
__device__ __forceinline__ void als_syrk(als_f32x4 (&acc)[als_tiles_per_wave(NT)],
                                         const int (&ta)[als_tiles_per_wave(NT)],
                                         const int (&tb)[als_tiles_per_wave(NT)], const float* Ys, const float* ws,
                                         int rows) {
  constexpr int S = als_stride(NT * 16);
  const int l = lane_id();
  const float* yp = Ys + (l >> 4) * S + (l & 15);
  for (int k = 0; k < rows; k += 4) {
    const float wk = WEIGHTED ? ws[k + (l >> 4)] : 1.f;
#pragma unroll
    for (int i = 0; i < als_tiles_per_wave(NT); ++i) {
      if (ta[i] >= 0) {
        float a = yp[k * S + ta[i] * 16];
        const float b = yp[k * S + tb[i] * 16];
        if constexpr (WEIGHTED) a *= wk;
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[i], 0, 0, 0);
      }
    }
  }
}

// rows [0, rows4) of the staging tile from table rows src(k) (nullptr = a zero row), 16-byte loads when the rows are
// 16-byte aligned; columns >= D and rows without a source are zeros
template <int NT, typename RowOf>
__device__ __forceinline__ void als_stage(float* Ys, int rows4, int D, bool vec, RowOf src) {
  constexpr int DP = NT * 16, S = als_stride(DP);
  if (vec) {
    for (int e = threadIdx.x; e < rows4 * (DP / 4); e += kBlock) {
      const int k = e / (DP / 4), c = (e - k * (DP / 4)) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const float* row = src(k);
      if (row != nullptr && c < D) v = *reinterpret_cast<const float4*>(row + c);   // D % 4 == 0: all four inside
      *reinterpret_cast<float4*>(Ys + k * S + c) = v;
    }
  } else {
    for (int e = threadIdx.x; e < rows4 * DP; e += kBlock) {
      const int k = e / DP, c = e - k * DP;
      const float* row = src(k);
      Ys[k * S + c] = (row != nullptr && c < D) ? row[c] : 0.f;
    }
  }
}

__host__ __device__ inline bool als_vec_ok(const float* table, int D) {
  return D % 4 == 0 && (reinterpret_cast<uintptr_t>(table) & 15) == 0;
}

// ---- gram --------------------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(kBlock) void als_gram_kernel(const float* __restrict__ F, int64_t n, int D,
                                                          float* __restrict__ slots) {
  extern __shared__ float smem[];
  constexpr int DP = NT * 16, TPW = als_tiles_per_wave(NT);
  float* Ys = smem;
  int ta[TPW], tb[TPW];
  als_my_tiles<NT>(ta, tb);
  als_f32x4 acc[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) acc[i] = als_f32x4{0.f, 0.f, 0.f, 0.f};
  const bool vec = als_vec_ok(F, D);
  const int64_t n_tiles = (n + kAlsChunk - 1) / kAlsChunk;
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t r0 = t * kAlsChunk;
    const int cnt = static_cast<int>(std::min<int64_t>(kAlsChunk, n - r0));
    const int rows4 = (cnt + 3) & ~3;
    __syncthreads();   // the previous tile's operand loads are done
    als_stage<NT>(Ys, rows4, D, vec, [&](int k) { return k < cnt ? F + (r0 + k) * D : nullptr; });
    __syncthreads();
    als_syrk<NT, false>(acc, ta, tb, Ys, nullptr, rows4);
  }
  float* slot = slots + static_cast<int64_t>(blockIdx.x) * DP * DP;
  const int l = lane_id();
#pragma unroll
  for (int i = 0; i < TPW; ++i)
    if (ta[i] >= 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) slot[(ta[i] * 16 + 4 * (l >> 4) + q) * DP + tb[i] * 16 + (l & 15)] = acc[i][q];
    }
}

// G[r][c] = sum of the slots' entry [max(r, c)][min(r, c)] in slot order; G_reg = G + reg I
__global__ __launch_bounds__(kBlock) void als_gram_fold_kernel(const float* __restrict__ slots, int n_slots, int D, int DP,
                                                               float reg, float* __restrict__ G, float* __restrict__ Greg) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= D * D) return;
  const int r = e / D, c = e - r * D;
  const float* src = slots + std::max(r, c) * DP + std::min(r, c);
  const int64_t step = static_cast<int64_t>(DP) * DP;
  float v = 0.f;
  int s = 0;
  for (; s + 8 <= n_slots; s += 8) {   // eight loads in flight before their adds; the order of the adds is the slots'
    float x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) x[q] = src[(s + q) * step];
#pragma unroll
    for (int q = 0; q < 8; ++q) v += x[q];
  }
  for (; s < n_slots; ++s) v += src[s * step];
  G[e] = v;
  Greg[e] = r == c ? v + reg : v;
}

// ---- solve -------------------------------------------------------------------------------------------------------------
struct AlsSolve {
  const int64_t* ptr;
  const int64_t* idx;
  const float* val;
  const int64_t* order;
  int64_t n_rows;
  const float* other;
  int64_t n_other;
  const float* greg;
  float* out;
  int32_t* failed;
  hiprec_stats* stats;
  float alpha;
  int D;
};

template <int NT>
__global__ __launch_bounds__(kBlock) void als_solve_kernel(AlsSolve s) {
  extern __shared__ float smem[];
  constexpr int DP = NT * 16, S = als_stride(DP), TPW = als_tiles_per_wave(NT);
  float* A = smem;                      // [DP + 1][S], row DP is b / z
  float* Ys = A + (DP + 1) * S;         // [chunk][S]
  float* col = Ys + kAlsChunk * S;      // column j of L by logical row (row D is b's)
  float* dinv = col + DP + 16;          // 1 / L[j][j]
  float* zs = dinv + DP;
  float* s_w = zs + DP;                 // alpha r
  float* s_c = s_w + kAlsChunk;         // 1 + alpha r
  int* s_id = reinterpret_cast<int*>(s_c + kAlsChunk);
  const int tid = threadIdx.x, l = lane_id(), D = s.D;
  const int ty = tid >> 4, tx = tid & 15;
  const bool vec = als_vec_ok(s.other, D);
  int ta[TPW], tb[TPW];
  als_my_tiles<NT>(ta, tb);

  for (int64_t p = blockIdx.x; p < s.n_rows; p += gridDim.x) {
    const int64_t row = s.order != nullptr ? s.order[p] : p;
    if (row < 0 || row >= s.n_rows) {   // (uniform)
      if (tid == 0) atomicOr(&s.stats->status, HIPREC_STATUS_ROW_OOB);
      continue;
    }
    const int64_t beg = s.ptr[row], end = s.ptr[row + 1];
    float* dst = s.out + row * D;
    if (end <= beg) {
      if (tid < D) dst[tid] = 0.f;
      continue;
    }
    als_f32x4 acc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) acc[i] = als_f32x4{0.f, 0.f, 0.f, 0.f};
    float bacc = 0.f;
    for (int64_t c0 = beg; c0 < end; c0 += kAlsChunk) {
      const int cnt = static_cast<int>(std::min<int64_t>(kAlsChunk, end - c0));
      const int rows4 = (cnt + 3) & ~3;
      __syncthreads();   // the previous chunk's (or row's) LDS reads are done
      if (tid < kAlsChunk) {
        int id = -1;
        float w = 0.f;
        if (tid < cnt) {
          const int64_t v = s.idx[c0 + tid];
          if (v >= 0 && v < s.n_other) {
            id = static_cast<int>(v);
            w = s.alpha * s.val[c0 + tid];
          } else {
            atomicOr(&s.stats->status, HIPREC_STATUS_ITEM_OOB);
          }
        }
        s_id[tid] = id;
        s_w[tid] = w;
        s_c[tid] = id >= 0 ? 1.f + w : 0.f;
      }
      __syncthreads();
      als_stage<NT>(Ys, rows4, D, vec, [&](int k) {
        const int id = s_id[k];
        return id >= 0 ? s.other + static_cast<int64_t>(id) * D : nullptr;
      });
      __syncthreads();
      als_syrk<NT, true>(acc, ta, tb, Ys, s_w, rows4);
      if (tid < DP) {
        for (int k = 0; k < cnt; ++k) bacc = __builtin_fmaf(s_c[k], Ys[k * S + tid], bacc);
      }
    }
    // A = tiles + (G + reg I); b behind it
#pragma unroll
    for (int i = 0; i < TPW; ++i)
      if (ta[i] >= 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = ta[i] * 16 + 4 * (l >> 4) + q, c = tb[i] * 16 + (l & 15);
          A[r * S + c] = acc[i][q] + ((r < D && c < D) ? s.greg[r * D + c] : 0.f);
        }
      }
    if (tid < DP) A[DP * S + tid] = bacc;
    __syncthreads();

    // A = L L^T in place, right-looking; logical row D (physical row DP) is b, which the same updates turn into z
    bool bad = false;
    for (int j = 0; j < D; ++j) {
      const float piv = A[j * S + j];
      if (!(piv > 0.f) || !(piv < INFINITY)) {   // every thread reads the same value: uniform
        bad = true;
        break;
      }
      const float rinv = 1.f / sqrtf(piv);
      if (tid == 0) dinv[j] = rinv;
      {
        const int i = j + 1 + tid;
        if (i <= D) {
          float* e = A + (i == D ? DP : i) * S + j;
          const float v = *e * rinv;
          *e = v;
          col[i] = v;
        }
      }
      __syncthreads();
      for (int i = j + 1 + ty; i <= D; i += 16) {
        float* arow = A + (i == D ? DP : i) * S;
        const float lij = col[i];
        const int kmax = i < D ? i : D - 1;
        for (int k = j + 1 + tx; k <= kmax; k += 16) arow[k] = __builtin_fmaf(-lij, col[k], arow[k]);
      }
      __syncthreads();
    }
    if (bad) {
      if (tid == 0) atomicAdd(s.failed, 1);
      continue;
    }
    // L^T x = z
    if (tid < D) zs[tid] = A[DP * S + tid];
    __syncthreads();
    for (int j = D - 1; j >= 0; --j) {
      const float xj = zs[j] * dinv[j];
      if (tid < j) zs[tid] = __builtin_fmaf(-A[j * S + tid], xj, zs[tid]);
      if (tid == j) dst[j] = xj;
      __syncthreads();
    }
  }
}

// ---- loss --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double als_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

// part[u] = {x^T G x + sum over the row of [c (1 - s)^2 - s^2], |x|^2}: one wave per row
__global__ __launch_bounds__(kBlock) void als_loss_rows_kernel(const int64_t* __restrict__ ptr,
                                                               const int64_t* __restrict__ idx,
                                                               const float* __restrict__ val, int64_t n_users,
                                                               const float* __restrict__ X, const float* __restrict__ Y,
                                                               int64_t n_items, int D, const float* __restrict__ G,
                                                               float alpha, double2* __restrict__ part,
                                                               hiprec_stats* stats) {
  const int l = lane_id();
  const bool in0 = l < D, in1 = l + kWave < D;
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); u < n_users;
       u += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const float x0 = in0 ? X[u * D + l] : 0.f, x1 = in1 ? X[u * D + l + kWave] : 0.f;
    double g0 = 0.0, g1 = 0.0;
    for (int e = 0; e < D; ++e) {   // G is symmetric bit for bit: row e is column e
      const float xe = __shfl(e < kWave ? x0 : x1, e & (kWave - 1), kWave);
      if (in0) g0 += static_cast<double>(G[e * D + l]) * xe;
      if (in1) g1 += static_cast<double>(G[e * D + l + kWave]) * xe;
    }
    const double quad = als_wave_sum(g0 * x0 + g1 * x1);
    const double sq = als_wave_sum(static_cast<double>(x0) * x0 + static_cast<double>(x1) * x1);
    double frame = 0.0;
    for (int64_t p = ptr[u]; p < ptr[u + 1]; ++p) {
      const int64_t i = idx[p];
      if (i < 0 || i >= n_items) {
        if (l == 0) atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
        continue;
      }
      const float y0 = in0 ? Y[i * D + l] : 0.f, y1 = in1 ? Y[i * D + l + kWave] : 0.f;
      const double sc = als_wave_sum(static_cast<double>(x0) * y0 + static_cast<double>(x1) * y1);
      const double c = 1.0 + static_cast<double>(alpha) * static_cast<double>(val[p]);
      frame += c * (1.0 - sc) * (1.0 - sc) - sc * sc;
    }
    if (l == 0) part[u] = make_double2(quad + frame, sq);
  }
}

// out[0] = sum of the partials + reg (|X|^2 + trace G), out[1] = the regulariser: thread t adds rows t, t + 256, ...,
// then a tree over the threads -- the same order every run
__global__ __launch_bounds__(kBlock) void als_loss_fold_kernel(const double2* __restrict__ part, int64_t n_users,
                                                               const float* __restrict__ G, int D, float reg,
                                                               double* __restrict__ out) {
  __shared__ double s_a[kBlock];
  __shared__ double s_b[kBlock];
  double a = 0.0, b = 0.0;
  for (int64_t u = threadIdx.x; u < n_users; u += kBlock) {
    const double2 v = part[u];
    a += v.x;
    b += v.y;
  }
  s_a[threadIdx.x] = a;
  s_b[threadIdx.x] = b;
  __syncthreads();
  for (int h = kBlock / 2; h > 0; h >>= 1) {
    if (static_cast<int>(threadIdx.x) < h) {
      s_a[threadIdx.x] += s_a[threadIdx.x + h];
      s_b[threadIdx.x] += s_b[threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double tr = 0.0;
    for (int d = 0; d < D; ++d) tr += static_cast<double>(G[d * D + d]);
    const double r = static_cast<double>(reg) * (s_b[0] + tr);
    out[0] = s_a[0] + r;
    out[1] = r;
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------
static bool als_dim_ok(int32_t dim) { return dim >= 1 && dim <= kAlsMaxDim; }
static bool als_count_ok(int64_t n) { return n >= 1 && n < (1ll << 31); }
static int als_gram_slots(int64_t n) {
  return static_cast<int>(std::min<int64_t>((n + kAlsChunk - 1) / kAlsChunk, HIPREC_ALS_GRAM_SLOTS));
}
static size_t als_gram_bytes(int64_t n, int32_t dim) {
  const size_t dp = als_pad16(dim);
  return sizeof(float) * dp * dp * static_cast<size_t>(als_gram_slots(n));
}

template <int NT>
static int als_launch_gram(const float* F, int64_t n, int D, float* slots, int grid, hipStream_t st) {
  const size_t lds = sizeof(float) * kAlsChunk * als_stride(NT * 16);
  als_gram_kernel<NT><<<grid, kBlock, lds, st>>>(F, n, D, slots);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

template <int NT>
static int als_launch_solve(const AlsSolve& a, int grid, hipStream_t st) {
  constexpr size_t lds = sizeof(float) * als_solve_lds_floats(NT * 16);
  if constexpr (lds > 64 * 1024) {
    static std::atomic<uint64_t> lds_ok{0};   // per instantiation: the limit is an attribute of the function
    if (int rc = allow_dynamic_lds({reinterpret_cast<const void*>(&als_solve_kernel<NT>)}, lds, lds_ok,
                                   "the ALS row solve"))
      return rc;
  }
  als_solve_kernel<NT><<<grid, kBlock, lds, st>>>(a);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_als_workspace_bytes(int64_t n_users, int64_t n_items, int32_t dim) {
  if (!als_count_ok(n_users) || !als_count_ok(n_items) || !als_dim_ok(dim)) return static_cast<size_t>(-1);
  return als_gram_bytes(std::max(n_users, n_items), dim) + sizeof(double2) * static_cast<size_t>(n_users);
}

static int als_gram_dispatch(int nt, const float* F, int64_t n, int D, float* slots, int grid, hipStream_t st) {
#define ALS_GRAM_CALL(N) als_launch_gram<N>(F, n, D, slots, grid, st)
  switch (nt) {
    case 1: return ALS_GRAM_CALL(1);
    case 2: return ALS_GRAM_CALL(2);
    case 3: return ALS_GRAM_CALL(3);
    case 4: return ALS_GRAM_CALL(4);
    case 5: return ALS_GRAM_CALL(5);
    case 6: return ALS_GRAM_CALL(6);
    case 7: return ALS_GRAM_CALL(7);
    default: return ALS_GRAM_CALL(8);
  }
#undef ALS_GRAM_CALL
}

static int als_solve_dispatch(int nt, const AlsSolve& a, int grid, hipStream_t st) {
  switch (nt) {
    case 1: return als_launch_solve<1>(a, grid, st);
    case 2: return als_launch_solve<2>(a, grid, st);
    case 3: return als_launch_solve<3>(a, grid, st);
    case 4: return als_launch_solve<4>(a, grid, st);
    case 5: return als_launch_solve<5>(a, grid, st);
    case 6: return als_launch_solve<6>(a, grid, st);
    case 7: return als_launch_solve<7>(a, grid, st);
    default: return als_launch_solve<8>(a, grid, st);
  }
}

extern "C" int hiprec_als_gram(const float* F, int64_t n, int32_t dim, float reg, float* G, float* G_reg, void* workspace,
                               size_t workspace_bytes, void* stream) {
  HIPREC_REQUIRE(als_count_ok(n) && als_dim_ok(dim), "als_gram: bad shape (n=%lld dim=%d; dim is 1..%d)", (long long)n, dim,
                 kAlsMaxDim);
  HIPREC_REQUIRE(std::isfinite(reg), "als_gram: reg=%g is not finite", (double)reg);
  HIPREC_REQUIRE(F && G && G_reg, "als_gram: NULL pointer");
  const size_t need = als_gram_bytes(n, dim);
  HIPREC_REQUIRE(workspace != nullptr && workspace_bytes >= need, "als_gram: workspace %zu B < %zu B", workspace_bytes,
                 need);
  auto st = static_cast<hipStream_t>(stream);
  const int slots = als_gram_slots(n), DP = als_pad16(dim);
  if (int rc = als_gram_dispatch(DP / 16, F, n, dim, static_cast<float*>(workspace), slots, st)) return rc;
  als_gram_fold_kernel<<<(dim * dim + kBlock - 1) / kBlock, kBlock, 0, st>>>(static_cast<const float*>(workspace), slots,
                                                                           dim, DP, reg, G, G_reg);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_als_solve_rows(const int64_t* ptr, const int64_t* idx, const float* val, const int64_t* order,
                                     int64_t n_rows, const float* other, int64_t n_other, int32_t dim,
                                     const float* G_reg, float alpha, float* out, int32_t blocks, int32_t* failed,
                                     hiprec_stats* stats, void* stream) {
  HIPREC_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31) && als_count_ok(n_other) && als_dim_ok(dim),
                 "als_solve_rows: bad shape (n_rows=%lld n_other=%lld dim=%d; dim is 1..%d)", (long long)n_rows,
                 (long long)n_other, dim, kAlsMaxDim);
  HIPREC_REQUIRE(alpha >= 0.f && std::isfinite(alpha), "als_solve_rows: alpha=%g must be finite and >= 0", (double)alpha);
  HIPREC_REQUIRE(blocks >= 0 && blocks <= HIPREC_ALS_MAX_BLOCKS, "als_solve_rows: blocks=%d outside 0..%d", blocks,
                 HIPREC_ALS_MAX_BLOCKS);
  HIPREC_REQUIRE(failed != nullptr, "als_solve_rows: NULL failed counter");
  HIPREC_REQUIRE(stats != nullptr, "als_solve_rows: NULL stats");
  HIPREC_REQUIRE(ptr && other && G_reg && out, "als_solve_rows: NULL pointer");
  if (n_rows == 0) return 0;
  HIPREC_REQUIRE(idx && val, "als_solve_rows: NULL pointer");
  const AlsSolve a{ptr, idx, val, order, n_rows, other, n_other, G_reg, out, failed, stats, alpha, dim};
  const int grid = static_cast<int>(std::min<int64_t>(n_rows, blocks > 0 ? blocks : HIPREC_ALS_MAX_BLOCKS));
  return als_solve_dispatch(als_pad16(dim) / 16, a, grid, static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_als_loss(const int64_t* ptr, const int64_t* idx, const float* val, int64_t n_users, const float* X,
                               const float* Y, int64_t n_items, int32_t dim, const float* G, float alpha, float reg,
                               void* workspace, size_t workspace_bytes, double* out, hiprec_stats* stats, void* stream) {
  HIPREC_REQUIRE(als_count_ok(n_users) && als_count_ok(n_items) && als_dim_ok(dim),
                 "als_loss: bad shape (n_users=%lld n_items=%lld dim=%d; dim is 1..%d)", (long long)n_users,
                 (long long)n_items, dim, kAlsMaxDim);
  HIPREC_REQUIRE(alpha >= 0.f && std::isfinite(alpha) && std::isfinite(reg), "als_loss: alpha=%g / reg=%g", (double)alpha,
                 (double)reg);
  HIPREC_REQUIRE(stats != nullptr, "als_loss: NULL stats");
  HIPREC_REQUIRE(ptr && idx && val && X && Y && G && out, "als_loss: NULL pointer");
  const size_t need = hiprec_als_workspace_bytes(n_users, n_items, dim);
  HIPREC_REQUIRE(workspace != nullptr && workspace_bytes >= need, "als_loss: workspace %zu B < %zu B", workspace_bytes,
                 need);
  auto st = static_cast<hipStream_t>(stream);
  // the partials live behind the Gram slots, so G (not the slots) is all this call needs from hiprec_als_gram
  double2* part = reinterpret_cast<double2*>(static_cast<char*>(workspace) + als_gram_bytes(std::max(n_users, n_items), dim));
  als_loss_rows_kernel<<<grid_for_waves(n_users), kBlock, 0, st>>>(ptr, idx, val, n_users, X, Y, n_items, dim, G, alpha,
                                                                  part, stats);
  HIPREC_TRY(hipGetLastError());
  als_loss_fold_kernel<<<1, kBlock, 0, st>>>(part, n_users, G, dim, reg, out);
  HIPREC_TRY(hipGetLastError());
  return 0;
}
