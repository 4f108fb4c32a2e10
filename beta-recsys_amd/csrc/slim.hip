// SLIM (Ning and Karypis, "SLIM: Sparse Linear Methods for Top-N Recommender Systems", ICDM 2011) for gfx950: the sparse
// linear item model by cyclic coordinate descent.  No counterpart in the reference.
//
//   G = X^T X     A = G + l2 I (hiprec_ease_gram with reg = l2)     per item j, w = W[:, j] minimises
//   1/2 w^T A w - G[:, j]^T w + l1 sum |w_k|     subject to w_j = 0 and, in positive mode, w >= 0
//
// One workgroup per column j.  w and q = A w live in LDS (or in the block's slice of the workspace when 2 n floats do not
// fit: the same code, the same bits).  A is symmetric, so column k is the contiguous row k and G[k, j] is A[j, k] for
// k != j: the only strided access is the store of the finished column.
//
// A sweep visits k = 0 .. n-1 in ascending order (Gauss-Seidel), skipping k = j.  Most coordinates do not move, so a
// coordinate does not cost a barrier: every wave of the block evaluates the same chunk of 64 candidates redundantly, one
// candidate per lane, from the same LDS values with the same operations, so the four waves agree on every decision
// without talking.  __ballot finds the lowest lane that moves; its axpy q += d A[:, k] runs across the block (thread t
// owns the entries t, t + 256, ...: consecutive axpys need no barrier between them); each lane keeps its own candidate's
// q in a register and applies the same axpy term to it, then the lanes above the mover are evaluated again.  That is
// exactly the ascending order.  Barriers: one after a chunk's first read when the chunk has a move (so no wave writes q
// while another still reads the chunk), one at the end of such a chunk.  A chunk without a move has none.
//
// Every rounded operation is one IEEE operation in a fixed order: contraction to an fma is switched off for this file
// (the pragma below; the __f*_rn intrinsics are plain operators in HIP and would be contracted all the same), and the
// division is the correctly rounded one.  So the bits are a function of A, the parameters and j alone, and
// tests/slim_numpy.py in float32 restates them operation by operation.
//
// Bounds: a lane is live only for k < n; the axpy and the column store run over i < n; the workspace slice of block b is
// [b * 2 n, (b + 1) * 2 n) floats behind the n floats of the diagonal.  Every loop is bounded: a chunk retires at least
// one lane per move (at most 64), a sweep has ceil(n / 64) chunks, a column at most max_sweeps sweeps.  A value that is
// not finite (NaN or inf in A, a zero diagonal) ends the column at once and sets HIPREC_STATUS_NOT_FINITE.
#include <algorithm>
#include <cmath>

#include "common.hpp"

#pragma clang fp contract(off)

namespace hiprec {
namespace {

constexpr int kSlimWsBlocks = 1024;     // blocks of the workspace form (block-stride over the columns)

struct SlimArgs {
  const float* A;
  const float* diag;
  float* W;
  int32_t* sweeps;
  float* ws;
  hiprec_stats* stats;
  int64_t n;
  float l1, tol;
  int32_t max_sweeps;
};

__global__ __launch_bounds__(kBlock) void slim_diag_kernel(const float* A, int64_t n, float* diag) {
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; k < n;
       k += static_cast<int64_t>(gridDim.x) * kBlock)
    diag[k] = A[k * n + k];
}

// The coordinate's new value from (w_k, q_k, b_k = G_kj, A_kk); `fin` is false when the step or A_kk is not finite (an
// infinite A_kk would quietly pin w_k instead).
template <bool POSITIVE>
__device__ __forceinline__ float slim_step(float wk, float qk, float bk, float akk, float l1, bool& fin) {
  if constexpr (POSITIVE) {
    const float g = (qk - bk) + l1;
    const float t = wk - g / akk;
    fin = fabsf(t) < INFINITY && fabsf(akk) < INFINITY;
    return t > 0.f ? t : 0.f;                         // (-0 and NaN become +0; NaN is reported through fin)
  } else {
    const float r = bk - (qk - akk * wk);
    const float m = fabsf(r) - l1;
    const float v = m / akk;
    fin = fabsf(v) < INFINITY && fabsf(akk) < INFINITY;
    return m > 0.f ? copysignf(v, r) : 0.f;
  }
}

template <bool WS, bool POSITIVE>
__global__ __launch_bounds__(kBlock) void slim_fit_kernel(const SlimArgs a) {
  extern __shared__ float slim_lds[];
  const int tid = static_cast<int>(threadIdx.x), lane = lane_id();
  const int n = static_cast<int>(a.n);                // <= HIPREC_EASE_MAX_ITEMS: element indices fit an int
  float* w = WS ? a.ws + static_cast<size_t>(blockIdx.x) * 2 * static_cast<size_t>(n) : slim_lds;
  float* q = w + n;
  for (int j = static_cast<int>(blockIdx.x); j < n; j += static_cast<int>(gridDim.x)) {
    for (int i = tid; i < n; i += kBlock) {
      w[i] = 0.f;
      q[i] = 0.f;
    }
    __syncthreads();
    const float* b = a.A + static_cast<int64_t>(j) * n;                    // G[:, j] off the diagonal (A is symmetric)
    int sweep = 0;
    bool converged = false, bad = false;
    while (sweep < a.max_sweeps && !bad) {
      ++sweep;
      float dmax = 0.f;
      for (int c0 = 0; c0 < n && !bad; c0 += kWave) {
        const int k = c0 + lane;
        const bool live = k < n && k != j;
        float wk = 0.f, qk = 0.f, bk = 0.f, akk = 1.f;
        if (live) {
          wk = w[k];
          qk = q[k];
          bk = b[k];
          akk = a.diag[k];
        }
        bool moved = false;
        unsigned long long todo = ~0ull;              // the lanes of this chunk not yet passed by the sweep
        while (todo) {
          bool fin = true;
          const float wn = slim_step<POSITIVE>(wk, qk, bk, akk, a.l1, fin);
          const unsigned long long m = __ballot(live && (!fin || wn != wk)) & todo;
          if (m == 0) break;
          const int src = __ffsll(m) - 1;             // the lowest coordinate that moves: uniform across the block
          const float wn_s = __shfl(wn, src), wk_s = __shfl(wk, src);
          if (__shfl(fin ? 1 : 0, src) == 0) {
            bad = true;
            break;
          }
          const float d = wn_s - wk_s;
          const int ks = c0 + src;
          if (!moved) {
            __syncthreads();                          // every wave has read this chunk's w and q
            moved = true;
          }
          const float* row = a.A + static_cast<int64_t>(ks) * n;
#pragma unroll 4
          for (int i = tid; i < n; i += kBlock) q[i] = q[i] + d * row[i];
          if (live) qk = qk + d * row[k];
          if (lane == src) wk = wn_s;
          if (tid == src) w[ks] = wn_s;
          dmax = fmaxf(dmax, fabsf(d));
          todo = src == kWave - 1 ? 0ull : (~0ull << (src + 1));
        }
        if (moved && !bad) __syncthreads();           // the chunk's axpys are complete before the next chunk is read
      }
      if (!bad && dmax <= a.tol) {
        converged = true;
        break;
      }
    }
    __syncthreads();
    for (int i = tid; i < n; i += kBlock) a.W[static_cast<int64_t>(i) * n + j] = w[i];    // (w[j] was never written: +0)
    if (tid == 0) {
      a.sweeps[j] = converged ? sweep : -sweep;
      if (bad) atomicOr(&a.stats->status, HIPREC_STATUS_NOT_FINITE);
    }
    __syncthreads();
  }
}

bool slim_size_ok(int64_t n) { return n >= 1 && n <= HIPREC_EASE_MAX_ITEMS; }

bool slim_in_lds(int64_t n, int32_t lds_cap) {
  const int64_t cap = (lds_cap == 0 || lds_cap > HIPREC_SLIM_LDS_CAP) ? HIPREC_SLIM_LDS_CAP : lds_cap;
  return n <= cap;
}

int64_t slim_ws_blocks(int64_t n) { return std::min<int64_t>(n, kSlimWsBlocks); }

size_t slim_diag_floats(int64_t n) { return (static_cast<size_t>(n) + 3) / 4 * 4; }

size_t slim_need(int64_t n, int32_t lds_cap) {
  size_t floats = slim_diag_floats(n);
  if (!slim_in_lds(n, lds_cap)) floats += static_cast<size_t>(slim_ws_blocks(n)) * 2 * static_cast<size_t>(n);
  return (floats * sizeof(float) + 7) / 8 * 8;
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_slim_workspace_bytes(int64_t n, int32_t lds_cap) {
  if (!slim_size_ok(n) || lds_cap < 0) return static_cast<size_t>(-1);
  return slim_need(n, lds_cap);
}

extern "C" int hiprec_slim_fit(const float* A, int64_t n, float l1, int32_t positive_only, float tol, int32_t max_sweeps,
                               float* W, int32_t* sweeps_out, int32_t lds_cap, void* workspace, size_t workspace_bytes,
                               hiprec_stats* stats, void* stream) {
  HIPREC_REQUIRE(slim_size_ok(n) && lds_cap >= 0, "slim_fit: bad sizes (n=%lld lds_cap=%d; n in 1..%d)", (long long)n,
                 lds_cap, HIPREC_EASE_MAX_ITEMS);
  HIPREC_REQUIRE(l1 >= 0.f && std::isfinite(l1), "slim_fit: l1=%g must be finite and >= 0", (double)l1);
  HIPREC_REQUIRE(tol >= 0.f && std::isfinite(tol), "slim_fit: tol=%g must be finite and >= 0", (double)tol);
  HIPREC_REQUIRE(max_sweeps >= 1 && max_sweeps <= HIPREC_SLIM_MAX_SWEEPS, "slim_fit: max_sweeps=%d must be in 1..%d",
                 max_sweeps, HIPREC_SLIM_MAX_SWEEPS);
  HIPREC_REQUIRE(positive_only == 0 || positive_only == 1, "slim_fit: positive_only=%d must be 0 or 1", positive_only);
  HIPREC_REQUIRE(stats != nullptr, "slim_fit: NULL stats");
  HIPREC_REQUIRE(A != nullptr && W != nullptr && sweeps_out != nullptr, "slim_fit: NULL pointer");
  HIPREC_REQUIRE(A != W, "slim_fit: W must not be A");
  const size_t need = slim_need(n, lds_cap);
  HIPREC_REQUIRE(workspace != nullptr && workspace_bytes >= need, "slim_fit: workspace %zu B < %zu B", workspace_bytes,
                 need);
  auto s = static_cast<hipStream_t>(stream);
  float* diag = static_cast<float*>(workspace);
  slim_diag_kernel<<<grid_for_threads(n), kBlock, 0, s>>>(A, n, diag);
  HIPREC_TRY(hipGetLastError());
  SlimArgs a{A, diag, W, sweeps_out, diag + slim_diag_floats(n), stats, n, l1, tol, max_sweeps};
  if (slim_in_lds(n, lds_cap)) {
    const unsigned grid = static_cast<unsigned>(n);                   // one block per column: the hardware balances them
    const size_t lds = 2 * sizeof(float) * static_cast<size_t>(n);    // <= 64 KiB: HIPREC_SLIM_LDS_CAP
    if (positive_only)
      slim_fit_kernel<false, true><<<grid, kBlock, lds, s>>>(a);
    else
      slim_fit_kernel<false, false><<<grid, kBlock, lds, s>>>(a);
  } else {
    const unsigned grid = static_cast<unsigned>(slim_ws_blocks(n));
    if (positive_only)
      slim_fit_kernel<true, true><<<grid, kBlock, 0, s>>>(a);
    else
      slim_fit_kernel<true, false><<<grid, kBlock, 0, s>>>(a);
  }
  HIPREC_TRY(hipGetLastError());
  return 0;
}
