// BUIR training step for gfx950.
//
// Replaces beta_rec/models/buir.py:56-77 (BUIR_NB.forward / get_loss: two LightGCN encoders, one shared predictor, the
// symmetric cosine loss), :149-178 (LGCN_Encoder.forward: L hops of norm_adj, mean over hops 0 .. L), :215-233
// (train_single_batch), autograd's backward through all of it, :48-54 (_update_target, the optional moving target) and
// :79-100 (predict).
//
// The reference never calls _update_target, so its target encoder stays the initial online encoder and the pooled target
// table P_tg is a constant: it lives in the workspace and is not propagated again.  A step runs L SpMMs forward (the online
// pool P_on) and L backward, where the reference runs 2 L + L.  With update_target the raw tables follow T <- m T + (1 - m)
// O after the optimizer (bu_ema_kernel) and, the pool being linear, P_tg <- m P_tg + (1 - m) P_on in the pass of the next
// forward that writes each pooled online row (bu_finish_pool_kernel) -- still no target propagation.
//
// The SpMM is launch_spmm of csrc/lightgcn.hip (edge slices, atomics into the hop buffer and into the running hop sum): a
// row has no single owner wave there, so the (L + 1)-term mean is finished by one elementwise pass after the last hop.
//
// Everything per batch is ONE kernel, bu_tile_kernel: a block takes TILE_B batch rows, stacks their user and item rows into
// a 2 TILE_B x D tile X in LDS (the paired target rows, already normalised, in a second tile), computes Y = X W^T + b on
// v_mfma_f32_16x16x4_f32 with W staged through LDS in 16-wide K-slabs, the row norms, the two cosines and the block's loss
// partial, overwrites the target tile with dY (torch's normalize backward; the clamp makes the denominator a constant
// below 1e-12), computes dX = dY W on the MFMA and adds it into the [n, D] gradient table with row atomics, and leaves
// dW = dY^T X and db = sum dY as per-block partials that bu_fold_kernel adds up in block order.  Y and dY never leave
// the CU.  Then the backward chain of csrc/simgcl.hip runs over the gradient table with A^T:
// g_E0 = (1 / (L + 1)) sum_{k = 0 .. L} (A^T)^k G, by Horner's rule.
#include <algorithm>

#include "common.hpp"
#include "seqrec.hpp"
#include "spmm.hpp"

namespace hiprec {

constexpr int kBuTB = HIPREC_BUIR_TILE_B;   // batch rows per block
constexpr int kBuRows = 2 * kBuTB;          // stacked rows: users, then items (4 MFMA row blocks)
constexpr int kBuRB = kBuRows / 16;
constexpr int kBuKS = 16;                   // K-slab of W in LDS
constexpr int kBuWS = kBuKS + 4;            // row stride of a forward slab
static_assert(kBuTB == 32 && kBuRB == 4, "tile geometry is wired into the kernels");
static_assert(HIPREC_BUIR_MAX_DIM == 4 * kWave, "a wave holds a row in four registers per lane");

__host__ __device__ inline int bu_dp(int dim) { return (dim + 15) & ~15; }
// n_tiles row tiles [kBuRows][DP + 4] and one slab: [DP][kBuWS] forward (>= [kBuKS][DP + 4], the transposed one)
static size_t bu_lds_bytes(int dim, int n_tiles) {
  const size_t DP = bu_dp(dim);
  return sizeof(float) * (n_tiles * kBuRows * (DP + 4) + DP * kBuWS);
}

// acc[rb][tt] += (Xs W^T)[16 rb .., 16 (w + 4 tt) ..]: W [D, D] row-major from global, one 16-wide K-slab at a time
template <int NCBW>
__device__ __forceinline__ void bu_linear(const float* Xs, int stride, float* Ws, const float* __restrict__ W, int D,
                                          int DP, f32x4 (&acc)[kBuRB][NCBW]) {
  const int w = wave_in_block();
  for (int k0 = 0; k0 < DP; k0 += kBuKS) {
    __syncthreads();   // the previous slab's reads are done (first round: the tiles are written)
    for (int e = threadIdx.x; e < DP * kBuKS; e += kBlock) {
      const int n = e / kBuKS, kk = e - n * kBuKS;
      Ws[n * kBuWS + kk] = (n < D && k0 + kk < D) ? W[static_cast<int64_t>(n) * D + k0 + kk] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < NCBW; ++tt) {
      const int cb = w + kWavesPerBlock * tt;
      if (cb * 16 < DP) {
#pragma unroll
        for (int rb = 0; rb < kBuRB; ++rb)   // B = W^T: element (k, j) at Ws[j][k]
          acc[rb][tt] = mma16(acc[rb][tt], Xs + rb * 16 * stride + k0, stride, 1, Ws + cb * 16 * kBuWS, 1, kBuWS, kBuKS);
      }
    }
  }
}

// acc[rb][tt] += (As W)[16 rb .., 16 (w + 4 tt) ..]: slabs of 16 ROWS of W
template <int NCBW>
__device__ __forceinline__ void bu_linear_t(const float* As, int stride, float* Ws, const float* __restrict__ W, int D,
                                            int DP, f32x4 (&acc)[kBuRB][NCBW]) {
  const int w = wave_in_block();
  for (int o0 = 0; o0 < DP; o0 += kBuKS) {
    __syncthreads();
    for (int e = threadIdx.x; e < kBuKS * DP; e += kBlock) {
      const int oo = e / DP, i = e - oo * DP;
      Ws[oo * stride + i] = (o0 + oo < D && i < D) ? W[static_cast<int64_t>(o0 + oo) * D + i] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < NCBW; ++tt) {
      const int cb = w + kWavesPerBlock * tt;
      if (cb * 16 < DP) {
#pragma unroll
        for (int rb = 0; rb < kBuRB; ++rb)
          acc[rb][tt] = mma16(acc[rb][tt], As + rb * 16 * stride + o0, stride, 1, Ws + cb * 16, stride, 1, kBuKS);
      }
    }
  }
}

// ---- the mean over hops 0 .. L, and the deferred moving-average update of the pooled target -------------------------
// pool holds E_0 + A E_0 + .. + A^L E_0; pool <- pool / (L + 1); ptg (when given) <- m ptg + (1 - m) pool
__global__ __launch_bounds__(kBlock) void bu_finish_pool_kernel(float* __restrict__ pool, float* __restrict__ ptg,
                                                                int64_t n, float inv, float m, float omm) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const float p = pool[i] * inv;
    pool[i] = p;
    if (ptg) ptg[i] = m * ptg[i] + omm * p;
  }
}

// buir.py:48-54 on the raw tables: two rounded products and their rounded sum, as ATen computes t * m + o * (1 - m)
__global__ __launch_bounds__(kBlock) void bu_ema_kernel(const float* __restrict__ o, float* __restrict__ t, int64_t n,
                                                        float m, float omm) {
#pragma clang fp contract(off)
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const float a = t[i] * m, b = o[i] * omm;
    t[i] = a + b;
  }
}

// ---- the fused batch tile ------------------------------------------------------------------------------------------
struct BuTileArgs {
  const float *P_on, *P_tg, *W, *b;
  const int64_t *users, *pos;
  int64_t batch, n_users, n_items;
  int D;
  float inv_batch;   // the batch mean
  float g_scale;     // 1 / (L + 1): takes the gradient from the pooled row to the hop sum
  float* G;          // [n, D], zero on entry
  float *part_w, *part_b;   // [blocks][D * D], [blocks][D]
  Scratch* scratch;
  hiprec_stats* stats;
};

template <int NCBW>
__global__ __launch_bounds__(kBlock) void bu_tile_kernel(BuTileArgs a) {
  extern __shared__ float smem[];
  __shared__ float s_red[2][kWavesPerBlock][kBuRows];
  __shared__ float s_coef[kBuRows], s_cy[kBuRows], s_loss[kBuRows];
  __shared__ long long s_node[kBuRows];   // node row of a stacked row, -1: none (beyond the batch, or a flagged id)
  const int D = a.D, DP = bu_dp(D), stride = DP + 4;
  float* Xs = smem;
  float* Ts = Xs + kBuRows * stride;
  float* Ws = Ts + kBuRows * stride;
  const int lane = lane_id(), w = wave_in_block();
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * kBuTB;

  // gather: one wave per stacked row.  Row r < TILE_B is x_u paired with t_i, row TILE_B + r is x_i paired with t_u; the
  // target row is normalised here (F.normalize's clamp) and the padding up to DP is zero in both tiles.
  for (int r = w; r < kBuRows; r += kWavesPerBlock) {
    const int side = r >= kBuTB ? 1 : 0;
    const int64_t t = b0 + (r - side * kBuTB);
    long long xn = -1, tn = -1;
    if (t < a.batch) {
      const int64_t u = a.users[t], i = a.pos[t];
      const bool u_ok = static_cast<uint64_t>(u) < static_cast<uint64_t>(a.n_users);
      const bool i_ok = static_cast<uint64_t>(i) < static_cast<uint64_t>(a.n_items);
      if (u_ok && i_ok) {
        xn = side ? a.n_users + i : u;
        tn = side ? u : a.n_users + i;
      } else if (lane == 0 && side == 0) {
        atomicOr(&a.stats->status, (u_ok ? 0u : HIPREC_STATUS_USER_OOB) | (i_ok ? 0u : HIPREC_STATUS_ITEM_OOB));
      }
    }
    float tv[4], ss = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane + kWave * k;
      const bool ok = c < D;
      const float xv = (ok && xn >= 0) ? a.P_on[xn * D + c] : 0.f;
      tv[k] = (ok && tn >= 0) ? a.P_tg[tn * D + c] : 0.f;
      ss += tv[k] * tv[k];
      if (c < DP) Xs[r * stride + c] = xv;
    }
    const float inv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane + kWave * k;
      if (c < DP) Ts[r * stride + c] = tv[k] * inv;
    }
    if (lane == 0) s_node[r] = xn;
  }

  // Y = X W^T + b in registers: (row = 16 rb + 4 (lane >> 4) + q, col = 16 (w + 4 tt) + (lane & 15))
  f32x4 acc[kBuRB][NCBW];
#pragma unroll
  for (int rb = 0; rb < kBuRB; ++rb)
#pragma unroll
    for (int tt = 0; tt < NCBW; ++tt) acc[rb][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
  bu_linear<NCBW>(Xs, stride, Ws, a.W, D, DP, acc);

  float ss[kBuRB][4], dt[kBuRB][4];
#pragma unroll
  for (int rb = 0; rb < kBuRB; ++rb)
#pragma unroll
    for (int q = 0; q < 4; ++q) ss[rb][q] = dt[rb][q] = 0.f;
#pragma unroll
  for (int tt = 0; tt < NCBW; ++tt) {
    const int cb = w + kWavesPerBlock * tt;
    if (cb * 16 < DP) {
      const int col = cb * 16 + (lane & 15);
      const bool ok = col < D;
      const float bias = ok ? a.b[col] : 0.f;
#pragma unroll
      for (int rb = 0; rb < kBuRB; ++rb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = rb * 16 + 4 * (lane >> 4) + q;
          const float y = ok ? acc[rb][tt][q] + bias : 0.f;
          acc[rb][tt][q] = y;
          ss[rb][q] += y * y;
          dt[rb][q] += y * Ts[row * stride + col];
        }
    }
  }
  // the 16 columns of a row sit in the 16 lanes of one DPP row; then the four waves in a fixed order
#pragma unroll
  for (int rb = 0; rb < kBuRB; ++rb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = ss[rb][q], p = dt[rb][q];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        v += __shfl_xor(v, o, 64);
        p += __shfl_xor(p, o, 64);
      }
      if ((lane & 15) == 0) {
        s_red[0][w][rb * 16 + 4 * (lane >> 4) + q] = v;
        s_red[1][w][rb * 16 + 4 * (lane >> 4) + q] = p;
      }
    }
  __syncthreads();
  if (threadIdx.x < kBuRows) {
    const int r = threadIdx.x;
    const float sq = (s_red[0][0][r] + s_red[0][1][r]) + (s_red[0][2][r] + s_red[0][3][r]);
    const float dot = (s_red[1][0][r] + s_red[1][1][r]) + (s_red[1][2][r] + s_red[1][3][r]);
    const float nrm = sqrtf(sq), den = fmaxf(nrm, 1e-12f);
    const float c = dot / den;   // n(y) . n(t)
    const bool live = s_node[r] >= 0;
    s_loss[r] = live ? (2.f - 2.f * c) * a.inv_batch : 0.f;
    // d loss / d y = coef (n(t) - [|y| >= 1e-12] c n(y)): below the clamp the denominator is a constant
    s_coef[r] = live ? -2.f * a.inv_batch / den : 0.f;
    s_cy[r] = nrm >= 1e-12f ? c / den : 0.f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {   // the loss once per block, in row order
    float l = 0.f;
    for (int r = 0; r < kBuRows; ++r) l += s_loss[r];
    a.scratch->partials[blockIdx.x] = make_float4(l, 0.f, 0.f, 0.f);
    if (blockIdx.x == 0) a.scratch->n_partials = gridDim.x;
  }
  // dY over the target tile: every element is read and rewritten by the lane that holds its y
#pragma unroll
  for (int tt = 0; tt < NCBW; ++tt) {
    const int cb = w + kWavesPerBlock * tt;
    if (cb * 16 < DP) {
      const int col = cb * 16 + (lane & 15);
#pragma unroll
      for (int rb = 0; rb < kBuRB; ++rb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = rb * 16 + 4 * (lane >> 4) + q;
          const int at = row * stride + col;
          Ts[at] = s_coef[row] * (Ts[at] - s_cy[row] * acc[rb][tt][q]);
          acc[rb][tt][q] = 0.f;
        }
    }
  }

  // dX = dY W, scattered into the gradient table (a node may sit in many rows of many blocks: atomics)
  bu_linear_t<NCBW>(Ts, stride, Ws, a.W, D, DP, acc);
#pragma unroll
  for (int tt = 0; tt < NCBW; ++tt) {
    const int col = (w + kWavesPerBlock * tt) * 16 + (lane & 15);
    if (col >= D) continue;
#pragma unroll
    for (int rb = 0; rb < kBuRB; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const long long node = s_node[rb * 16 + 4 * (lane >> 4) + q];
        if (node >= 0) atomic_add_f32(a.G + node * D + col, acc[rb][tt][q] * a.g_scale);
      }
  }

  // dW = dY^T X and db = sum of dY's rows: this block's partials (both tiles are read-only from here on)
  float* pw = a.part_w + static_cast<int64_t>(blockIdx.x) * D * D;
  const int nb = DP / 16;
  for (int t = w; t < nb * nb; t += kWavesPerBlock) {
    const int ob = t / nb, ib = t - ob * nb;
    const f32x4 d = mma16(f32x4{0.f, 0.f, 0.f, 0.f}, Ts + ob * 16, 1, stride, Xs + ib * 16, stride, 1, kBuRows);
    const int i = ib * 16 + (lane & 15);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int o = ob * 16 + 4 * (lane >> 4) + q;
      if (o < D && i < D) pw[o * D + i] = d[q];
    }
  }
  for (int o = threadIdx.x; o < D; o += kBlock) {
    float s = 0.f;
    for (int r = 0; r < kBuRows; ++r) s += Ts[r * stride + o];
    a.part_b[static_cast<int64_t>(blockIdx.x) * D + o] = s;
  }
}

// second level of dW / db: element e of [D * D | D] summed over the blocks in block order; counts the step
__global__ __launch_bounds__(kBlock) void bu_fold_kernel(const float* __restrict__ part_w, const float* __restrict__ part_b,
                                                         int n_blocks, int D, float* __restrict__ g_w,
                                                         float* __restrict__ g_b, hiprec_stats* stats) {
  const int dd = D * D;
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e < dd + D) {
    const bool is_w = e < dd;
    const float* src = is_w ? part_w + e : part_b + (e - dd);
    const int64_t step = is_w ? dd : D;
    float s = 0.f;
    for (int k = 0; k < n_blocks; ++k) s += src[k * step];
    if (is_w) g_w[e] = s; else g_b[e - dd] = s;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) advance_step(stats);
}

// ---- projection and predict ----------------------------------------------------------------------------------------
// out[r] = P[r] W^T + b for kBuRows node rows per block
template <int NCBW>
__global__ __launch_bounds__(kBlock) void bu_project_kernel(const float* __restrict__ P, const float* __restrict__ W,
                                                            const float* __restrict__ b, int64_t n, int D,
                                                            float* __restrict__ out) {
  extern __shared__ float smem[];
  const int DP = bu_dp(D), stride = DP + 4;
  float* Xs = smem;
  float* Ws = Xs + kBuRows * stride;
  const int lane = lane_id(), w = wave_in_block();
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kBuRows;
  for (int e = threadIdx.x; e < kBuRows * DP; e += kBlock) {
    const int r = e / DP, c = e - r * DP;
    Xs[r * stride + c] = (r0 + r < n && c < D) ? P[(r0 + r) * D + c] : 0.f;
  }
  f32x4 acc[kBuRB][NCBW];
#pragma unroll
  for (int rb = 0; rb < kBuRB; ++rb)
#pragma unroll
    for (int tt = 0; tt < NCBW; ++tt) acc[rb][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
  bu_linear<NCBW>(Xs, stride, Ws, W, D, DP, acc);
#pragma unroll
  for (int tt = 0; tt < NCBW; ++tt) {
    const int col = (w + kWavesPerBlock * tt) * 16 + (lane & 15);
    if (col >= D) continue;
    const float bias = b[col];
#pragma unroll
    for (int rb = 0; rb < kBuRB; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t r = r0 + rb * 16 + 4 * (lane >> 4) + q;
        if (r < n) out[r * D + col] = acc[rb][tt][q] + bias;
      }
  }
}

// scores[t] = PW[u] . P[U + i] + P[u] . PW[U + i]: one wave per pair
__global__ __launch_bounds__(kBlock) void bu_predict_kernel(const float* __restrict__ P, const float* __restrict__ PW,
                                                            int64_t n_users, int64_t n_items, int D,
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
    const int64_t ru = u * D, ri = (n_users + i) * D;
    float dot = 0.f;
    for (int c = lane; c < D; c += kWave) dot += PW[ru + c] * P[ri + c] + P[ru + c] * PW[ri + c];
    dot = wave_sum(dot);
    if (lane == 0) scores[t] = dot;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------
// pooled online | pooled target | gradient table | two hop buffers
static int64_t bu_ws_floats(int64_t n_rows, int dim) { return 5 * n_rows * dim; }
static int64_t bu_blocks(int64_t batch) { return (batch + kBuTB - 1) / kBuTB; }
static int64_t bu_batch_floats(int64_t batch, int dim) { return bu_blocks(batch) * (static_cast<int64_t>(dim) * dim + dim); }

struct BuWs {
  float *p_on, *p_tg, *G, *ha, *hb;
};
static BuWs bu_ws(const hiprec_buir_plan* p) {
  const int64_t nd = (p->n_users + p->n_items) * p->dim;
  float* w = p->ws;
  return BuWs{w, w + nd, w + 2 * nd, w + 3 * nd, w + 4 * nd};
}

// level 0: the shape; 1: + graph and workspace; 2: + the training buffers
static int check_bu_plan(const hiprec_buir_plan* p, int level) {
  HIPREC_REQUIRE(p != nullptr, "NULL plan");
  HIPREC_REQUIRE(p->n_users > 0 && p->n_items > 0, "bad sizes");
  HIPREC_REQUIRE(p->n_layers >= 1 && p->n_layers <= HIPREC_BUIR_MAX_LAYERS, "BUIR n_layers %d: 1 .. %d are supported",
                 p->n_layers, HIPREC_BUIR_MAX_LAYERS);
  HIPREC_REQUIRE(p->dim >= 1 && p->dim <= HIPREC_BUIR_MAX_DIM, "BUIR emb_dim %d: 1 .. %d are supported", p->dim,
                 HIPREC_BUIR_MAX_DIM);
  if (level < 1) return 0;
  HIPREC_REQUIRE(p->online && p->w && p->b, "NULL online / w / b");
  HIPREC_REQUIRE(p->a.rowptr && p->a.n_rows > 0 && p->a.nnz >= 0 && (p->a.nnz == 0 || (p->a.col && p->a.val)),
                 "bad CSR a");
  HIPREC_REQUIRE(p->a.n_rows == p->n_users + p->n_items, "graph size != n_users + n_items");
  HIPREC_REQUIRE(p->a.n_rows < (1ll << 31) - 1, "more than 2^31 - 2 nodes");
  HIPREC_REQUIRE(p->ws != nullptr && p->ws_floats >= bu_ws_floats(p->a.n_rows, p->dim),
                 "ws holds %lld floats, %lld are needed", (long long)p->ws_floats,
                 (long long)bu_ws_floats(p->a.n_rows, p->dim));
  if (level < 2) return 0;
  HIPREC_REQUIRE(p->at.rowptr && p->at.n_rows == p->a.n_rows && p->at.nnz == p->a.nnz &&
                     (p->a.nnz == 0 || (p->at.col && p->at.val)),
                 "bad CSR at / a and at differ");
  HIPREC_REQUIRE(p->g_online && p->g_w && p->g_b, "NULL gradient slot");
  return 0;
}

static std::atomic<uint64_t> g_bu_lds_ok{0};

static int bu_allow_lds() {
  return allow_dynamic_lds({reinterpret_cast<const void*>(&bu_tile_kernel<1>),
                            reinterpret_cast<const void*>(&bu_tile_kernel<2>),
                            reinterpret_cast<const void*>(&bu_tile_kernel<4>),
                            reinterpret_cast<const void*>(&bu_project_kernel<1>),
                            reinterpret_cast<const void*>(&bu_project_kernel<2>),
                            reinterpret_cast<const void*>(&bu_project_kernel<4>)},
                           bu_lds_bytes(HIPREC_BUIR_MAX_DIM, 2), g_bu_lds_ok, "BUIR's batch tiles");
}

// out = mean(E_0 .. A^L E_0) of `table`; ptg (optional): the deferred moving-average update rides in the finishing pass
static int bu_pool(const hiprec_buir_plan* p, const float* table, float* out, float* ptg, hipStream_t st) {
  const BuWs w = bu_ws(p);
  const int64_t nd = p->a.n_rows * p->dim;
  if (out != table) HIPREC_TRY(hipMemcpyAsync(out, table, sizeof(float) * nd, hipMemcpyDeviceToDevice, st));
  const float* cur = table;
  for (int hop = 0; hop < p->n_layers; ++hop) {
    float* nxt = (hop & 1) ? w.hb : w.ha;
    if (int rc = launch_spmm(&p->a, nullptr, 1.f, cur, nxt, out, p->dim, st, false)) return rc;
    cur = nxt;
  }
  bu_finish_pool_kernel<<<grid_for_threads(nd), kBlock, 0, st>>>(out, ptg, nd, 1.0f / static_cast<float>(p->n_layers + 1),
                                                                 p->momentum, p->one_minus_momentum);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

static int bu_project(const hiprec_buir_plan* p, const float* P, float* out, hipStream_t st) {
  if (int rc = bu_allow_lds()) return rc;
  const int64_t n = p->a.n_rows;
  const int D = p->dim;
  const int64_t blocks = (n + kBuRows - 1) / kBuRows;
  const size_t lds = bu_lds_bytes(D, 1);
  const unsigned grid = static_cast<unsigned>(blocks);
  if (D <= 64) bu_project_kernel<1><<<grid, kBlock, lds, st>>>(P, p->w, p->b, n, D, out);
  else if (D <= 128) bu_project_kernel<2><<<grid, kBlock, lds, st>>>(P, p->w, p->b, n, D, out);
  else bu_project_kernel<4><<<grid, kBlock, lds, st>>>(P, p->w, p->b, n, D, out);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_buir_plan_bytes(void) { return sizeof(hiprec_buir_plan); }
extern "C" int32_t hiprec_buir_tile_b(void) { return kBuTB; }
extern "C" int32_t hiprec_buir_max_dim(void) { return HIPREC_BUIR_MAX_DIM; }
extern "C" int32_t hiprec_buir_max_layers(void) { return HIPREC_BUIR_MAX_LAYERS; }
extern "C" int64_t hiprec_buir_ws_floats(int64_t n_rows, int32_t dim) { return bu_ws_floats(n_rows, dim); }
extern "C" int64_t hiprec_buir_batch_ws_floats(int64_t batch, int32_t dim) { return bu_batch_floats(batch, dim); }

extern "C" int hiprec_buir_pool(const hiprec_buir_plan* plan, const float* table, float* out, float* proj, void* stream) {
  if (int rc = check_bu_plan(plan, 1)) return rc;
  HIPREC_REQUIRE(table != nullptr && out != nullptr, "NULL table / out");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = bu_pool(plan, table, out, nullptr, st)) return rc;
  return proj ? bu_project(plan, out, proj, st) : 0;
}

extern "C" int hiprec_buir_ema(const hiprec_buir_plan* plan, void* stream) {
  if (int rc = check_bu_plan(plan, 0)) return rc;
  HIPREC_REQUIRE(plan->online && plan->target, "NULL online / target");
  const int64_t nd = (plan->n_users + plan->n_items) * plan->dim;
  bu_ema_kernel<<<grid_for_threads(nd), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      plan->online, plan->target, nd, plan->momentum, plan->one_minus_momentum);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_buir_predict(const hiprec_buir_plan* plan, const int64_t* users, const int64_t* items, int64_t n,
                                   float* scores, hiprec_stats* stats, void* stream) {
  if (int rc = check_bu_plan(plan, 0)) return rc;
  if (n == 0) return 0;
  if (int rc = check_bu_plan(plan, 1)) return rc;
  HIPREC_REQUIRE(n > 0 && users && items && scores && stats, "NULL pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const BuWs w = bu_ws(plan);
  if (int rc = bu_pool(plan, plan->online, w.p_on, nullptr, st)) return rc;
  if (int rc = bu_project(plan, w.p_on, w.ha, st)) return rc;   // the hop buffers are free once the pool is finished
  bu_predict_kernel<<<grid_for_waves(n), kBlock, 0, st>>>(w.p_on, w.ha, plan->n_users, plan->n_items, plan->dim, users,
                                                          items, n, scores, stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_buir_grad(const hiprec_buir_plan* plan, const int64_t* users, const int64_t* pos,
                                const int64_t* neg, int64_t batch, hiprec_stats* stats, void* scratch,
                                size_t scratch_bytes, void* stream) {
  if (int rc = check_bu_plan(plan, 2)) return rc;
  (void)neg;   // buir.py:226-228 unpacks the negatives and never uses them
  const hiprec_buir_plan* p = plan;
  HIPREC_REQUIRE(batch > 0 && users && pos && stats && scratch, "NULL pointer / empty batch");
  const int64_t blocks = bu_blocks(batch);
  HIPREC_REQUIRE(blocks <= kMaxBlocks, "BUIR batch %lld: at most %d rows per step", (long long)batch, kMaxBlocks * kBuTB);
  HIPREC_REQUIRE(p->batch_ws && p->batch_ws_floats >= bu_batch_floats(batch, p->dim),
                 "batch_ws holds %lld floats, %lld are needed", (long long)p->batch_ws_floats,
                 (long long)bu_batch_floats(batch, p->dim));
  if (scratch_bytes < kScratchBytes) {
    set_error("scratch too small: %zu < %zu", scratch_bytes, kScratchBytes);
    return HIPREC_E_SCRATCH;
  }
  if (int rc = bu_allow_lds()) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const BuWs w = bu_ws(p);
  const int D = p->dim, L = p->n_layers;
  const int64_t nd = p->a.n_rows * D;

  // forward: the online pool (L SpMMs); the target pool is in the workspace already
  if (int rc = bu_pool(p, p->online, w.p_on, p->apply_pending ? w.p_tg : nullptr, st)) return rc;
  HIPREC_TRY(hipMemsetAsync(w.G, 0, sizeof(float) * nd, st));

  BuTileArgs a;
  a.P_on = w.p_on;
  a.P_tg = w.p_tg;
  a.W = p->w;
  a.b = p->b;
  a.users = users;
  a.pos = pos;
  a.batch = batch;
  a.n_users = p->n_users;
  a.n_items = p->n_items;
  a.D = D;
  a.inv_batch = 1.0f / static_cast<float>(batch);
  a.g_scale = 1.0f / static_cast<float>(L + 1);
  a.G = w.G;
  a.part_w = p->batch_ws;
  a.part_b = p->batch_ws + blocks * D * D;
  a.scratch = static_cast<Scratch*>(scratch);
  a.stats = stats;
  const size_t lds = bu_lds_bytes(D, 2);
  const unsigned grid = static_cast<unsigned>(blocks);
  if (D <= 64) bu_tile_kernel<1><<<grid, kBlock, lds, st>>>(a);
  else if (D <= 128) bu_tile_kernel<2><<<grid, kBlock, lds, st>>>(a);
  else bu_tile_kernel<4><<<grid, kBlock, lds, st>>>(a);
  HIPREC_TRY(hipGetLastError());
  bu_fold_kernel<<<(D * D + D + kBlock - 1) / kBlock, kBlock, 0, st>>>(a.part_w, a.part_b, static_cast<int>(blocks), D,
                                                                     p->g_w, p->g_b, stats);
  HIPREC_TRY(hipGetLastError());

  // backward (G carries the 1 / (L + 1) of the mean): h = G; (L - 1) x: h = G + A^T h; g = G + A^T h
  const float* h = w.G;
  for (int k = 1; k < L; ++k) {
    float* nxt = (k & 1) ? w.ha : w.hb;
    HIPREC_TRY(hipMemcpyAsync(nxt, w.G, sizeof(float) * nd, hipMemcpyDeviceToDevice, st));
    // the SpMM only ever ADDS into its output, so with y_is_zero it accumulates onto what is there
    if (int rc = launch_spmm(&p->at, nullptr, 1.f, h, nxt, nullptr, D, st, true)) return rc;
    h = nxt;
  }
  HIPREC_TRY(hipMemcpyAsync(p->g_online, w.G, sizeof(float) * nd, hipMemcpyDeviceToDevice, st));
  return launch_spmm(&p->at, nullptr, 1.f, h, p->g_online, nullptr, D, st, true);
}
