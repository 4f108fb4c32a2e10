// LCFN training step for gfx950.
//
// Replaces beta_rec/models/lcfn.py:55-87 (LCFN.forward: per layer and per side torch.matmul(P, torch.diag(f)) -- an
// [n, F] product and an [F, F] diagonal matrix built anew in every step --, P^T X, the [n, D] x [D, D] transform and the
// sigmoid), :171-205 (loss_comput: BPR mean over the concatenated rows + lamda x unsquared norms) and autograd's backward
// through all of it.
//
// A layer is X_k = sigmoid(P diag(f_k) P^T X_{k-1} W_k).  Here it is three launches that serve the user side and the
// item side together (split grids):
//   project   T  = P^T X        every block reduces its row tiles into an [F, D] partial on the fp32 MFMA and writes
//                               it to its own workspace slot (backward: X is dX (.) X_k (.) (1 - X_k), applied on load)
//   mid       M  = (f (.) T) W  sums the slots in slot order (no float atomics), scales, multiplies by W (backward: by
//                               W^T, then scales; df and the operands of dW when the filters are trained)
//   expand    X' = sigmoid(P M) one row tile per block, stored into column block k of the [n, (L + 1) D] all-embeddings
//                               table (backward: G_{k-1} + P (f (.) dA))
// so the [n, F] operand is read twice per layer and direction and nothing of size [n, F] or [n, n] is ever written.
//
// The loss stage gathers the three all-rows of a triple with one wave, scatters the BPR gradient into the hop-gradient
// table with row atomics and leaves per-triple partials; one block folds them (fixed order, double) into the BPR mean and
// the three batch norms, and only then can lamda x / ||x|| be scattered.
//
// LDS tiles: the project stage reads both of its tiles k-major (16 consecutive floats per k), so their row stride is
// 16 mod 64 floats; the expand stage reads P row-major (4 consecutive floats of 16 rows), so its stride is 4 x an odd
// number: either way the 64 lanes of one MFMA operand load fall into 64 different banks.
#include <algorithm>

#include "common.hpp"
#include "seqrec.hpp"

namespace hiprec {

constexpr int kLcfnTile = HIPREC_LCFN_TILE_ROWS;
constexpr int kLcfnMidRows = HIPREC_LCFN_MID_ROWS;
constexpr int kLcfnNorms = 16;   // 3 batch norms + 3 per layer, rounded up
static_assert(kLcfnTile == 32, "two MFMA row blocks per expand tile are wired into the kernels");
static_assert(3 + 3 * HIPREC_LCFN_MAX_LAYERS <= kLcfnNorms, "norm slots");
static_assert(HIPREC_LCFN_MAX_DIM <= 16 * 2 * kWavesPerBlock, "expand: two column blocks per wave");
static_assert(HIPREC_LCFN_MAX_FREQ <= 16 * 4 * kWavesPerBlock, "project: four frequency blocks per wave");

__host__ __device__ inline int lcfn_pad16(int x) { return (x + 15) & ~15; }
__host__ __device__ inline int lcfn_kmajor_stride(int x) { return ((x + 63) & ~63) + 16; }

// ---- project: slot[b] = sum over this block's row tiles of P_tile^T X_tile ------------------------------------------
struct LcfnProj {
  const float* P;      // [n, F]
  int64_t n;
  int F, slots;
  float* slot;         // [slots][F][D]
  const float* x;      // column block of the all-embeddings table, leading dimension ld
  const float* gx;     // backward: the same column block of the hop-gradient table
  int64_t ld;
};

template <int NFB, int NDB, bool BWD>
__global__ __launch_bounds__(kBlock) void lcfn_project_kernel(LcfnProj su, LcfnProj si, int D) {
  extern __shared__ float smem[];
  const bool item = static_cast<int>(blockIdx.x) >= su.slots;
  const LcfnProj s = item ? si : su;
  const int b = static_cast<int>(blockIdx.x) - (item ? su.slots : 0);
  const int F = s.F, FP = lcfn_pad16(F), DP = lcfn_pad16(D);
  const int sp = lcfn_kmajor_stride(FP), sx = lcfn_kmajor_stride(DP);
  float* Ps = smem;
  float* Xs = smem + kLcfnTile * sp;
  const int lane = lane_id(), w = wave_in_block();
  f32x4 acc[NFB][NDB];
#pragma unroll
  for (int i = 0; i < NFB; ++i)
#pragma unroll
    for (int j = 0; j < NDB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t n_tiles = (s.n + kLcfnTile - 1) / kLcfnTile;
  for (int64_t t = b; t < n_tiles; t += s.slots) {
    const int64_t r0 = t * kLcfnTile;
    __syncthreads();   // the previous tile's MFMA reads are done
    for (int e = threadIdx.x; e < kLcfnTile * FP; e += kBlock) {
      const int r = e / FP, c = e - r * FP;
      Ps[r * sp + c] = (r0 + r < s.n && c < F) ? s.P[(r0 + r) * F + c] : 0.f;
    }
    for (int e = threadIdx.x; e < kLcfnTile * DP; e += kBlock) {
      const int r = e / DP, c = e - r * DP;
      float v = 0.f;
      if (r0 + r < s.n && c < D) {
        v = s.x[(r0 + r) * s.ld + c];
        if constexpr (BWD) v = s.gx[(r0 + r) * s.ld + c] * v * (1.f - v);
      }
      Xs[r * sx + c] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NFB; ++i) {
      const int fb = w + kWavesPerBlock * i;
      if (fb * 16 < FP) {
#pragma unroll
        for (int j = 0; j < NDB; ++j)
          if (j * 16 < DP)   // A = P^T: element (f, row) at Ps[row][f]
            acc[i][j] = mma16(acc[i][j], Ps + fb * 16, 1, sp, Xs + j * 16, sx, 1, kLcfnTile);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NFB; ++i)
#pragma unroll
    for (int j = 0; j < NDB; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int f = (w + kWavesPerBlock * i) * 16 + 4 * (lane >> 4) + q, d = j * 16 + (lane & 15);
        if (f < F && d < D) s.slot[(static_cast<int64_t>(b) * F + f) * D + d] = acc[i][j][q];
      }
}

// ---- mid: the [F, D] stage -------------------------------------------------------------------------------------------
struct LcfnMid {
  const float* slot;   // [slots][F][D]
  int slots, F, blocks;
  const float* filt;   // f_k [F]
  float* t;            // T_k [F][D]: written by the forward, read by the backward when the filters are trained
  float* out;          // [FP][DP], zero beyond F / D: M_k (forward), f_k (.) dA (backward)
  float* dm;           // backward, filters trained: dM [F][D]
  float* gf;           // backward, filters trained: the gradient slot of f_k
  const float* norm;   // backward, filters trained: ||f_k||
};

template <bool BWD>
__global__ __launch_bounds__(kBlock) void lcfn_mid_kernel(LcfnMid mu, LcfnMid mi, int D, const float* __restrict__ W,
                                                          float lamda, int train) {
  __shared__ float s_a[kLcfnMidRows][HIPREC_LCFN_MAX_DIM];
  __shared__ float s_p[kLcfnMidRows][HIPREC_LCFN_MAX_DIM];
  const bool item = static_cast<int>(blockIdx.x) >= mu.blocks;
  const LcfnMid m = item ? mi : mu;
  const int f0 = (static_cast<int>(blockIdx.x) - (item ? mu.blocks : 0)) * kLcfnMidRows;
  const int F = m.F, DP = lcfn_pad16(D);
  for (int e = threadIdx.x; e < kLcfnMidRows * D; e += kBlock) {
    const int fr = e / D, d = e - fr * D, f = f0 + fr;
    float v = 0.f;
    if (f < F) {
      // slot order: same bits every run.  Eight loads are issued before their adds: one load per add made every
      // iteration wait out a cache miss (45 us of a 155 us step at 6040 x 3706, 189 slots)
      const float* src = m.slot + static_cast<int64_t>(f) * D + d;
      const int64_t step = static_cast<int64_t>(F) * D;
      int s = 0;
      for (; s + 8 <= m.slots; s += 8) {
        float x[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) x[q] = src[(s + q) * step];
#pragma unroll
        for (int q = 0; q < 8; ++q) v += x[q];
      }
      for (; s < m.slots; ++s) v += src[s * step];
      if constexpr (!BWD) {
        m.t[f * D + d] = v;
        v *= m.filt[f];
      } else if (train) {
        m.dm[f * D + d] = v;
      }
    }
    s_a[fr][d] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kLcfnMidRows * DP; e += kBlock) {
    const int fr = e / DP, j = e - fr * DP, f = f0 + fr;
    float o = 0.f;
    if (f < F && j < D) {
      if constexpr (BWD) {
        for (int d = 0; d < D; ++d) o += s_a[fr][d] * W[j * D + d];   // dA = dM W^T
      } else {
        for (int d = 0; d < D; ++d) o += s_a[fr][d] * W[d * D + j];   // M = (f (.) T) W
      }
    }
    if constexpr (BWD) {
      if (j < D) s_p[fr][j] = (train && f < F) ? o * m.t[f * D + j] : 0.f;
      o = f < F ? o * m.filt[f] : 0.f;
    }
    m.out[static_cast<int64_t>(f) * DP + j] = o;   // f < FP: the grid covers exactly FP rows
  }
  if constexpr (BWD) {
    if (train) {
      __syncthreads();
      const int f = f0 + static_cast<int>(threadIdx.x);
      if (threadIdx.x < kLcfnMidRows && f < F) {
        float df = 0.f;
        for (int j = 0; j < D; ++j) df += s_p[threadIdx.x][j];
        const float nrm = *m.norm;
        m.gf[f] = df + (nrm > 0.f ? lamda * m.filt[f] / nrm : 0.f);   // the slot's only writer
      }
    }
  }
}

// filters trained: dW[d][j] = sum over both sides and f of (f_f T[f][d]) dM[f][j] + lamda W[d][j] / ||W||
__global__ __launch_bounds__(kBlock) void lcfn_dw_kernel(const float* __restrict__ t_u, const float* __restrict__ dm_u,
                                                         const float* __restrict__ f_u, int F_u,
                                                         const float* __restrict__ t_i, const float* __restrict__ dm_i,
                                                         const float* __restrict__ f_i, int F_i, int D,
                                                         const float* __restrict__ W, const float* __restrict__ norm,
                                                         float lamda, float* __restrict__ gW) {
  const int d = blockIdx.x, j = threadIdx.x;
  if (j >= D) return;
  float v = 0.f;
  for (int f = 0; f < F_u; ++f) v += (f_u[f] * t_u[f * D + d]) * dm_u[f * D + j];
  for (int f = 0; f < F_i; ++f) v += (f_i[f] * t_i[f * D + d]) * dm_i[f * D + j];
  const float nrm = *norm;
  gW[d * D + j] = v + (nrm > 0.f ? lamda * W[d * D + j] / nrm : 0.f);
}

// ---- expand: one row tile per block ---------------------------------------------------------------------------------
struct LcfnExp {
  const float* P;      // [n, F]
  int64_t n;
  int F, tiles;
  const float* m;      // [FP][DP] from the mid stage
  float* out;          // leading dimension ldo
  const float* add;    // MODE 1: a second addend (leading dimension lda), or NULL
  int64_t ldo, lda;
};

// MODE 0: out = sigmoid(P m).  MODE 1: out += P m (+ add)
template <int MODE>
__global__ __launch_bounds__(kBlock) void lcfn_expand_kernel(LcfnExp eu, LcfnExp ei, int D) {
  extern __shared__ float smem[];
  const bool item = static_cast<int>(blockIdx.x) >= eu.tiles;
  const LcfnExp s = item ? ei : eu;
  const int64_t r0 = static_cast<int64_t>(static_cast<int>(blockIdx.x) - (item ? eu.tiles : 0)) * kLcfnTile;
  const int F = s.F, FP = lcfn_pad16(F), DP = lcfn_pad16(D), sp = FP + 4;
  const int lane = lane_id(), w = wave_in_block();
  for (int e = threadIdx.x; e < kLcfnTile * FP; e += kBlock) {
    const int r = e / FP, c = e - r * FP;
    smem[r * sp + c] = (r0 + r < s.n && c < F) ? s.P[(r0 + r) * F + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int cb = w + kWavesPerBlock * tt;
    if (cb * 16 >= DP) continue;
    const int col = cb * 16 + (lane & 15);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      const f32x4 acc = mma16(f32x4{0.f, 0.f, 0.f, 0.f}, smem + rb * 16 * sp, sp, 1, s.m + cb * 16, DP, 1, FP);
      if (col >= D) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t row = r0 + rb * 16 + 4 * (lane >> 4) + q;
        if (row >= s.n) continue;
        float* o = s.out + row * s.ldo + col;   // the element's only writer
        if constexpr (MODE == 0) {
          *o = sigmoid_f32(acc[q]);
        } else {
          *o = *o + (acc[q] + (s.add ? s.add[row * s.lda + col] : 0.f));
        }
      }
    }
  }
}

// X_0 = the tables themselves, as column block 0 of the all-embeddings tables
__global__ __launch_bounds__(kBlock) void lcfn_hop0_kernel(const float* __restrict__ w, float* __restrict__ all_u,
                                                           float* __restrict__ all_i, int64_t n_users, int64_t n_items,
                                                           int D, int W) {
  const int64_t total = (n_users + n_items) * D, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < total; e += stride) {
    const int64_t r = e / D;
    const int c = static_cast<int>(e - r * D);
    if (r < n_users)
      all_u[r * W + c] = w[e];
    else
      all_i[(r - n_users) * W + c] = w[e];
  }
}

// ---- loss stage: one wave per triple --------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void lcfn_loss_kernel(const float* __restrict__ all_u, const float* __restrict__ all_i,
                                                           float* __restrict__ g_u, float* __restrict__ g_i,
                                                           int64_t n_users, int64_t n_items, int W, int D,
                                                           const int64_t* __restrict__ users,
                                                           const int64_t* __restrict__ pos,
                                                           const int64_t* __restrict__ neg, int64_t batch, float inv_batch,
                                                           float* __restrict__ rows, hiprec_stats* stats) {
  const int lane = lane_id();
  const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t t = wave0; t < batch; t += n_waves) {
    const int64_t u = users[t], ip = pos[t], in = neg[t];
    const bool u_ok = static_cast<uint64_t>(u) < static_cast<uint64_t>(n_users);
    const bool i_ok = static_cast<uint64_t>(ip) < static_cast<uint64_t>(n_items) &&
                      static_cast<uint64_t>(in) < static_cast<uint64_t>(n_items);
    if (!(u_ok && i_ok)) {
      if (lane == 0) {
        atomicOr(&stats->status, (u_ok ? 0u : HIPREC_STATUS_USER_OOB) | (i_ok ? 0u : HIPREC_STATUS_ITEM_OOB));
        for (int a = 0; a < 4; ++a) rows[a * batch + t] = 0.f;
      }
      continue;
    }
    const int64_t ru = u * W, rp = ip * W, rn = in * W;
    float x = 0.f, squ = 0.f, sqp = 0.f, sqn = 0.f;
    for (int c = lane; c < W; c += kWave) {
      const float a = all_u[ru + c], p = all_i[rp + c], n = all_i[rn + c];
      x += a * (p - n);
      if (c < D) {   // the regulariser's rows are the hop-0 rows: column block 0
        squ += a * a;
        sqp += p * p;
        sqn += n * n;
      }
    }
    x = wave_sum(x);
    squ = wave_sum(squ);
    sqp = wave_sum(sqp);
    sqn = wave_sum(sqn);
    float sg;   // sigmoid(-x)
    const float loss = neg_logsigmoid(x, &sg);
    if (lane == 0) {
      rows[t] = loss;
      rows[batch + t] = squ;
      rows[2 * batch + t] = sqp;
      rows[3 * batch + t] = sqn;
    }
    const float gs = sg * inv_batch;
    for (int c = lane; c < W; c += kWave) {
      const float a = all_u[ru + c], p = all_i[rp + c], n = all_i[rn + c];
      atomic_add_f32(g_u + ru + c, -gs * (p - n));
      atomic_add_f32(g_i + rp + c, -gs * a);
      atomic_add_f32(g_i + rn + c, gs * a);
    }
  }
}

__device__ __forceinline__ double lcfn_block_sum(double v, double* s) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int k = kBlock / 2; k > 0; k >>= 1) {
    if (static_cast<int>(threadIdx.x) < k) s[threadIdx.x] += s[threadIdx.x + k];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();
  return r;
}

// one block: the per-triple partials folded in a fixed order into the BPR mean and the three batch norms; the norms of
// the filters and transformers; the step's loss for the optimizer sweep; the step counter
__global__ __launch_bounds__(kBlock) void lcfn_finish_kernel(const float* __restrict__ rows, int64_t batch, float inv_batch,
                                                             const float* __restrict__ tail, int F_u, int F_i, int D,
                                                             int L, float lamda, float* __restrict__ norm,
                                                             float* __restrict__ parts, hiprec_stats* stats,
                                                             Scratch* scratch) {
  __shared__ double s_red[kBlock];
  double sums[4];
  for (int a = 0; a < 4; ++a) {
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < batch; i += kBlock) v += rows[a * batch + i];
    sums[a] = lcfn_block_sum(v, s_red);
  }
  double reg = sqrt(sums[1]) + sqrt(sums[2]) + sqrt(sums[3]);
  if (threadIdx.x == 0)
    for (int a = 0; a < 3; ++a) norm[a] = static_cast<float>(sqrt(sums[1 + a]));
  for (int t = 0; t < 3 * L; ++t) {
    const int kind = t / L, k = t - kind * L;
    const int len = kind == 0 ? F_u : (kind == 1 ? F_i : D * D);
    const float* x = tail + (kind == 0 ? k * F_u : (kind == 1 ? L * F_u + k * F_i : L * (F_u + F_i) + k * D * D));
    double v = 0.0;
    for (int i = threadIdx.x; i < len; i += kBlock) v += static_cast<double>(x[i]) * x[i];
    const double nrm = sqrt(lcfn_block_sum(v, s_red));
    reg += nrm;
    if (threadIdx.x == 0) norm[3 + t] = static_cast<float>(nrm);
  }
  if (threadIdx.x == 0) {
    const double bpr = sums[0] * inv_batch;
    reg *= lamda;
    parts[0] = static_cast<float>(bpr);
    parts[1] = static_cast<float>(reg);
    parts[2] = static_cast<float>(bpr + reg);
    scratch->partials[0] = make_float4(parts[2], parts[1], 0.f, 0.f);
    scratch->n_partials = 1;
    advance_step(stats);
  }
}

// g[row] += lamda x / ||x|| for the three gathered batch matrices (a repeated row once per occurrence); norm 0 -> 0
__global__ __launch_bounds__(kBlock) void lcfn_reg_kernel(const float* __restrict__ w, float* __restrict__ g,
                                                          int64_t n_users, int64_t n_items, int D,
                                                          const int64_t* __restrict__ users,
                                                          const int64_t* __restrict__ pos,
                                                          const int64_t* __restrict__ neg, int64_t batch, float lamda,
                                                          const float* __restrict__ norm) {
  const int lane = lane_id();
  const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  const float cu = norm[0] > 0.f ? lamda / norm[0] : 0.f;
  const float cp = norm[1] > 0.f ? lamda / norm[1] : 0.f;
  const float cn = norm[2] > 0.f ? lamda / norm[2] : 0.f;
  for (int64_t t = wave0; t < batch; t += n_waves) {
    const int64_t u = users[t], ip = pos[t], in = neg[t];
    if (static_cast<uint64_t>(u) >= static_cast<uint64_t>(n_users) ||
        static_cast<uint64_t>(ip) >= static_cast<uint64_t>(n_items) ||
        static_cast<uint64_t>(in) >= static_cast<uint64_t>(n_items))
      continue;   // flagged by the loss stage
    const int64_t ru = u * D, rp = (n_users + ip) * D, rn = (n_users + in) * D;
    for (int c = lane; c < D; c += kWave) {
      atomic_add_f32(g + ru + c, cu * w[ru + c]);
      atomic_add_f32(g + rp + c, cp * w[rp + c]);
      atomic_add_f32(g + rn + c, cn * w[rn + c]);
    }
  }
}

__global__ __launch_bounds__(kBlock) void lcfn_predict_kernel(const float* __restrict__ all_u,
                                                              const float* __restrict__ all_i, int64_t n_users,
                                                              int64_t n_items, int W, const int64_t* __restrict__ users,
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
    for (int c = lane; c < W; c += kWave) dot += all_u[u * W + c] * all_i[i * W + c];
    dot = wave_sum(dot);
    if (lane == 0) scores[t] = dot;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
static int64_t lcfn_tiles(int64_t n) { return (n + kLcfnTile - 1) / kLcfnTile; }
static int lcfn_slots(int64_t n, int n_slots) {
  const int cap = n_slots > 0 ? std::min<int>(n_slots, HIPREC_LCFN_MAX_SLOTS) : HIPREC_LCFN_MAX_SLOTS;
  return static_cast<int>(std::min<int64_t>(lcfn_tiles(n), cap));
}

struct LcfnWs {
  float *all_u, *all_i, *g_u, *g_i, *slot_u, *slot_i, *t, *mid_u, *mid_i, *dm_u, *dm_i, *norm;
  int slots_u, slots_i;
};

// offsets (in floats) of the twelve regions of ws, and in [12] their total
static void lcfn_offsets(int64_t U, int64_t I, int Fu, int Fi, int D, int L, int n_slots, int64_t (&off)[13]) {
  const int64_t W = static_cast<int64_t>(L + 1) * D;
  const int64_t DP = lcfn_pad16(D);
  const int64_t size[12] = {U * W, I * W, U * W, I * W,
                            static_cast<int64_t>(lcfn_slots(U, n_slots)) * Fu * D,
                            static_cast<int64_t>(lcfn_slots(I, n_slots)) * Fi * D,
                            static_cast<int64_t>(L) * (Fu + Fi) * D, lcfn_pad16(Fu) * DP, lcfn_pad16(Fi) * DP,
                            static_cast<int64_t>(Fu) * D, static_cast<int64_t>(Fi) * D, kLcfnNorms};
  off[0] = 0;
  for (int i = 0; i < 12; ++i) off[i + 1] = off[i] + size[i];
}

static int64_t lcfn_ws_floats(int64_t U, int64_t I, int Fu, int Fi, int D, int L, int n_slots) {
  int64_t off[13];
  lcfn_offsets(U, I, Fu, Fi, D, L, n_slots, off);
  return off[12];
}
static int64_t lcfn_batch_floats(int64_t batch) { return 4 * batch; }

static LcfnWs lcfn_ws(const hiprec_lcfn_plan* p) {
  int64_t off[13];
  lcfn_offsets(p->n_users, p->n_items, p->f_user, p->f_item, p->dim, p->layer, p->n_slots, off);
  float* b = p->ws;
  return LcfnWs{b + off[0], b + off[1], b + off[2], b + off[3], b + off[4], b + off[5], b + off[6], b + off[7],
                b + off[8], b + off[9], b + off[10], b + off[11], lcfn_slots(p->n_users, p->n_slots),
                lcfn_slots(p->n_items, p->n_slots)};
}

struct LcfnTail {
  float *fu, *fi, *W;   // of layer k (0-based), in w or in g
};
static LcfnTail lcfn_tail(float* flat, const hiprec_lcfn_plan* p, int k) {
  float* t = flat + (p->n_users + p->n_items) * p->dim;
  return LcfnTail{t + static_cast<int64_t>(k) * p->f_user, t + static_cast<int64_t>(p->layer) * p->f_user + static_cast<int64_t>(k) * p->f_item,
                  t + static_cast<int64_t>(p->layer) * (p->f_user + p->f_item) + static_cast<int64_t>(k) * p->dim * p->dim};
}

static int check_lcfn_plan(const hiprec_lcfn_plan* p, bool train) {
  HIPREC_REQUIRE(p != nullptr, "NULL plan");
  HIPREC_REQUIRE(p->n_users > 0 && p->n_items > 0, "bad sizes");
  HIPREC_REQUIRE(p->dim >= 1 && p->dim <= HIPREC_LCFN_MAX_DIM, "LCFN emb_dim %d: 1 .. %d are supported", p->dim,
                 HIPREC_LCFN_MAX_DIM);
  HIPREC_REQUIRE(p->f_user >= 1 && p->f_user <= HIPREC_LCFN_MAX_FREQ && p->f_item >= 1 && p->f_item <= HIPREC_LCFN_MAX_FREQ,
                 "LCFN frequencies %d / %d: 1 .. %d are supported", p->f_user, p->f_item, HIPREC_LCFN_MAX_FREQ);
  HIPREC_REQUIRE(p->layer >= 1 && p->layer <= HIPREC_LCFN_MAX_LAYERS, "LCFN layer %d: 1 .. %d are supported", p->layer,
                 HIPREC_LCFN_MAX_LAYERS);
  HIPREC_REQUIRE((p->layer + 1) * p->dim <= HIPREC_LCFN_MAX_WIDTH, "LCFN (layer + 1) * emb_dim = %d: at most %d",
                 (p->layer + 1) * p->dim, HIPREC_LCFN_MAX_WIDTH);
  HIPREC_REQUIRE(p->n_slots >= 0, "bad n_slots %d", p->n_slots);
  HIPREC_REQUIRE(lcfn_tiles(p->n_users) + lcfn_tiles(p->n_items) < (1ll << 31), "tables too large for one launch");
  HIPREC_REQUIRE(p->P && p->Q && p->w && p->ws, "NULL P / Q / w / ws");
  const int64_t need = lcfn_ws_floats(p->n_users, p->n_items, p->f_user, p->f_item, p->dim, p->layer, p->n_slots);
  HIPREC_REQUIRE(p->ws_floats >= need, "ws holds %lld floats, %lld are needed", (long long)p->ws_floats, (long long)need);
  if (train) HIPREC_REQUIRE(p->g != nullptr, "NULL g");
  return 0;
}

template <bool BWD>
static int lcfn_launch_project(const LcfnProj& su, const LcfnProj& si, int D, hipStream_t st) {
  const int FP = lcfn_pad16(std::max(su.F, si.F)), DP = lcfn_pad16(D);
  const size_t lds = sizeof(float) * kLcfnTile * (lcfn_kmajor_stride(FP) + lcfn_kmajor_stride(DP));
  const int grid = su.slots + si.slots;
  const int nfb = FP <= 64 ? 1 : (FP <= 128 ? 2 : 4), ndb = DP <= 16 ? 1 : (DP <= 64 ? 4 : 8);
#define LCFN_PROJECT(A, B)                                                                     \
  if (nfb == A && ndb == B) {                                                                  \
    lcfn_project_kernel<A, B, BWD><<<grid, kBlock, lds, st>>>(su, si, D);                      \
    HIPREC_TRY(hipGetLastError());                                                             \
    return 0;                                                                                  \
  }
  LCFN_PROJECT(1, 1) LCFN_PROJECT(1, 4) LCFN_PROJECT(1, 8) LCFN_PROJECT(2, 1) LCFN_PROJECT(2, 4) LCFN_PROJECT(2, 8)
  LCFN_PROJECT(4, 1) LCFN_PROJECT(4, 4) LCFN_PROJECT(4, 8)
#undef LCFN_PROJECT
  set_error("LCFN project: no kernel for F %d, D %d", FP, DP);
  return HIPREC_E_BADARG;
}

static size_t lcfn_expand_lds(int Fu, int Fi) {
  return sizeof(float) * kLcfnTile * (lcfn_pad16(std::max(Fu, Fi)) + 4);
}

// [X_0 | ... | X_L] of both sides
static int lcfn_forward(const hiprec_lcfn_plan* p, const LcfnWs& w, hipStream_t st) {
  const int D = p->dim, L = p->layer, W = (L + 1) * D;
  lcfn_hop0_kernel<<<grid_for_threads((p->n_users + p->n_items) * D), kBlock, 0, st>>>(p->w, w.all_u, w.all_i, p->n_users,
                                                                                        p->n_items, D, W);
  HIPREC_TRY(hipGetLastError());
  for (int k = 1; k <= L; ++k) {
    const LcfnTail tl = lcfn_tail(p->w, p, k - 1);
    float* t_u = w.t + static_cast<int64_t>(k - 1) * (p->f_user + p->f_item) * D;
    float* t_i = t_u + static_cast<int64_t>(p->f_user) * D;
    const LcfnProj pu{p->P, p->n_users, p->f_user, w.slots_u, w.slot_u, w.all_u + (k - 1) * D, nullptr, W};
    const LcfnProj pi{p->Q, p->n_items, p->f_item, w.slots_i, w.slot_i, w.all_i + (k - 1) * D, nullptr, W};
    if (int rc = lcfn_launch_project<false>(pu, pi, D, st)) return rc;
    const LcfnMid mu{w.slot_u, w.slots_u, p->f_user, lcfn_pad16(p->f_user) / kLcfnMidRows, tl.fu, t_u, w.mid_u, nullptr,
                     nullptr, nullptr};
    const LcfnMid mi{w.slot_i, w.slots_i, p->f_item, lcfn_pad16(p->f_item) / kLcfnMidRows, tl.fi, t_i, w.mid_i, nullptr,
                     nullptr, nullptr};
    lcfn_mid_kernel<false><<<mu.blocks + mi.blocks, kBlock, 0, st>>>(mu, mi, D, tl.W, p->lamda, 0);
    HIPREC_TRY(hipGetLastError());
    const LcfnExp eu{p->P, p->n_users, p->f_user, static_cast<int>(lcfn_tiles(p->n_users)), w.mid_u, w.all_u + k * D,
                     nullptr, W, 0};
    const LcfnExp ei{p->Q, p->n_items, p->f_item, static_cast<int>(lcfn_tiles(p->n_items)), w.mid_i, w.all_i + k * D,
                     nullptr, W, 0};
    lcfn_expand_kernel<0><<<eu.tiles + ei.tiles, kBlock, lcfn_expand_lds(p->f_user, p->f_item), st>>>(eu, ei, D);
    HIPREC_TRY(hipGetLastError());
  }
  return 0;
}

// from the hop-gradient tables G = dloss / d[X_0 | ... | X_L]: dX = G_L; for k = L .. 1: dM = P^T (dX (.) X_k (.) (1 - X_k)),
// dA = dM W_k^T, dX = G_{k-1} + P (f_k (.) dA) -- accumulated in place in G's column block k - 1, for k = 1 into g
static int lcfn_backward(const hiprec_lcfn_plan* p, const LcfnWs& w, hipStream_t st) {
  const int D = p->dim, L = p->layer, W = (L + 1) * D;
  const int train = p->train_filters != 0;
  for (int k = L; k >= 1; --k) {
    const LcfnTail tl = lcfn_tail(p->w, p, k - 1), gl = lcfn_tail(p->g, p, k - 1);
    float* t_u = w.t + static_cast<int64_t>(k - 1) * (p->f_user + p->f_item) * D;
    float* t_i = t_u + static_cast<int64_t>(p->f_user) * D;
    const LcfnProj pu{p->P, p->n_users, p->f_user, w.slots_u, w.slot_u, w.all_u + k * D, w.g_u + k * D, W};
    const LcfnProj pi{p->Q, p->n_items, p->f_item, w.slots_i, w.slot_i, w.all_i + k * D, w.g_i + k * D, W};
    if (int rc = lcfn_launch_project<true>(pu, pi, D, st)) return rc;
    const LcfnMid mu{w.slot_u, w.slots_u, p->f_user, lcfn_pad16(p->f_user) / kLcfnMidRows, tl.fu, t_u, w.mid_u, w.dm_u,
                     gl.fu, w.norm + 3 + (k - 1)};
    const LcfnMid mi{w.slot_i, w.slots_i, p->f_item, lcfn_pad16(p->f_item) / kLcfnMidRows, tl.fi, t_i, w.mid_i, w.dm_i,
                     gl.fi, w.norm + 3 + L + (k - 1)};
    lcfn_mid_kernel<true><<<mu.blocks + mi.blocks, kBlock, 0, st>>>(mu, mi, D, tl.W, p->lamda, train);
    HIPREC_TRY(hipGetLastError());
    if (train) {
      lcfn_dw_kernel<<<D, kBlock, 0, st>>>(t_u, w.dm_u, tl.fu, p->f_user, t_i, w.dm_i, tl.fi, p->f_item, D, tl.W,
                                           w.norm + 3 + 2 * L + (k - 1), p->lamda, gl.W);
      HIPREC_TRY(hipGetLastError());
    }
    const bool last = k == 1;
    const LcfnExp eu{p->P, p->n_users, p->f_user, static_cast<int>(lcfn_tiles(p->n_users)), w.mid_u,
                     last ? p->g : w.g_u + (k - 1) * D, last ? w.g_u : nullptr, last ? D : W, W};
    const LcfnExp ei{p->Q, p->n_items, p->f_item, static_cast<int>(lcfn_tiles(p->n_items)), w.mid_i,
                     last ? p->g + p->n_users * D : w.g_i + (k - 1) * D, last ? w.g_i : nullptr, last ? D : W, W};
    lcfn_expand_kernel<1><<<eu.tiles + ei.tiles, kBlock, lcfn_expand_lds(p->f_user, p->f_item), st>>>(eu, ei, D);
    HIPREC_TRY(hipGetLastError());
  }
  return 0;
}

}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_lcfn_plan_bytes(void) { return sizeof(hiprec_lcfn_plan); }
extern "C" int32_t hiprec_lcfn_tile_rows(void) { return kLcfnTile; }
extern "C" int32_t hiprec_lcfn_max_slots(void) { return HIPREC_LCFN_MAX_SLOTS; }
extern "C" int32_t hiprec_lcfn_loss_triples_per_block(void) { return kWavesPerBlock; }
extern "C" int64_t hiprec_lcfn_ws_floats(int64_t n_users, int64_t n_items, int32_t f_user, int32_t f_item, int32_t dim,
                                         int32_t layer, int32_t n_slots) {
  if (n_users <= 0 || n_items <= 0 || f_user <= 0 || f_item <= 0 || dim <= 0 || layer <= 0 || n_slots < 0) return 0;
  return lcfn_ws_floats(n_users, n_items, f_user, f_item, dim, layer, n_slots);
}
extern "C" int64_t hiprec_lcfn_batch_ws_floats(int64_t batch) { return lcfn_batch_floats(batch); }

extern "C" int hiprec_lcfn_propagate(const hiprec_lcfn_plan* plan, void* stream) {
  if (int rc = check_lcfn_plan(plan, false)) return rc;
  return lcfn_forward(plan, lcfn_ws(plan), static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_lcfn_predict(const hiprec_lcfn_plan* plan, const int64_t* users, const int64_t* items, int64_t n,
                                   float* scores, hiprec_stats* stats, void* stream) {
  if (int rc = check_lcfn_plan(plan, false)) return rc;
  if (n == 0) return 0;
  HIPREC_REQUIRE(n > 0 && users && items && scores && stats, "NULL pointer");
  const LcfnWs w = lcfn_ws(plan);
  lcfn_predict_kernel<<<grid_for_waves(n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      w.all_u, w.all_i, plan->n_users, plan->n_items, (plan->layer + 1) * plan->dim, users, items, n, scores, stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_lcfn_grad(const hiprec_lcfn_plan* plan, const int64_t* users, const int64_t* pos, const int64_t* neg,
                                int64_t batch, float* parts, hiprec_stats* stats, void* scratch, size_t scratch_bytes,
                                void* stream) {
  if (int rc = check_lcfn_plan(plan, true)) return rc;
  const hiprec_lcfn_plan* p = plan;
  HIPREC_REQUIRE(batch > 0 && users && pos && neg && parts && stats && scratch, "NULL pointer / empty batch");
  HIPREC_REQUIRE(p->batch_ws && p->batch_ws_floats >= lcfn_batch_floats(batch), "batch_ws holds %lld floats, %lld are needed",
                 (long long)p->batch_ws_floats, (long long)lcfn_batch_floats(batch));
  if (scratch_bytes < kScratchBytes) {
    set_error("scratch too small: %zu < %zu", scratch_bytes, kScratchBytes);
    return HIPREC_E_SCRATCH;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LcfnWs w = lcfn_ws(p);
  const int D = p->dim, L = p->layer, W = (L + 1) * D;
  const float inv_batch = 1.0f / static_cast<float>(batch);
  // the hop-gradient tables collect row atomics (g_u and g_i are adjacent)
  HIPREC_TRY(hipMemsetAsync(w.g_u, 0, sizeof(float) * (p->n_users + p->n_items) * W, st));
  if (int rc = lcfn_forward(p, w, st)) return rc;
  const int grid = grid_for_waves(batch);
  lcfn_loss_kernel<<<grid, kBlock, 0, st>>>(w.all_u, w.all_i, w.g_u, w.g_i, p->n_users, p->n_items, W, D, users, pos, neg,
                                            batch, inv_batch, p->batch_ws, stats);
  lcfn_finish_kernel<<<1, kBlock, 0, st>>>(p->batch_ws, batch, inv_batch, p->w + (p->n_users + p->n_items) * D, p->f_user,
                                           p->f_item, D, L, p->lamda, w.norm, parts, stats,
                                           static_cast<Scratch*>(scratch));
  lcfn_reg_kernel<<<grid, kBlock, 0, st>>>(p->w, p->g, p->n_users, p->n_items, D, users, pos, neg, batch, p->lamda, w.norm);
  HIPREC_TRY(hipGetLastError());
  return lcfn_backward(p, w, st);
}
