// Collaborative Memory Network (CMN) training step -- SURVEY.md §8f rank 4, the model PairwiseGMF (pgmf.hip) pre-trains.
//
//   beta_rec/models/cmn.py:69-121    forward: two-hop neighbourhood attention + a 2D -> D -> 1 output module
//   beta_rec/models/vlml.py:59-124   apply_attention_memory / the hop loop (masked softmax over the list only)
//   beta_rec/models/cmn.py:153-200   train_single_batch: mean(-log(sigmoid(s+ - s-) + 1e-12)) + lambda ||W||_2 ;
//                                    backward ; clip_grad_norm_ ; optimizer.step()
//
// Flat layout (named_parameters() order), weights and the dense gradient alike:
//   [user_memory M U*D | item_memory E I*D | user_output C U*D | W D*D | b D | Wd D*2D | bd D | w D]
//
// A query (u, i, list) is:  z0 = M[u] + E[i];  hop k: a_j = z.M[n_j], p = softmax(a), o = sum_j p_j C[n_j];
// z1 = relu(W z0 + b + o0);  h = relu(Wd [M[u]*E[i] ; o1] + bd);  s = w.h.  A list is (pointer to ids, length): rows
// of a padded [B, Lpad] matrix or rows of an item -> users CSR, the same kernel either way.
//
// The step is
//   cmn_sample_kernel   one 256-thread block per SAMPLE (both of its queries, so the loss needs no second launch).
//                       A list of any length is streamed in rounds of 4 waves x (64 / G) rows, G = lanes per row
//                       (the smallest power of two >= D / 4: a lane holds four columns, read as one float4 when D is
//                       a multiple of 4), with an online softmax per lane group merged per wave and per block.
//                       Probabilities are RECOMPUTED in the backward (the rows have to be read again anyway):
//                         forward hop 0, forward hop 1                      (reads M and C rows)
//                         backward pass 1: dz1 = sum_j da1_j M[n_j]         (reads, no atomics)
//                         backward pass 2: da0 / dz0, and per row ONE add into dM[n_j] (da1_j z1 + da0_j z0) and ONE
//                         into dC[n_j] (p1_j do1 + p0_j do0): only the four scalars per row depend on the row, so
//                         they are shuffled from the row-parallel layout to a lane = column layout in which every
//                         atomic wave-instruction covers whole contiguous row segments (256 B for D >= 64).
//                       The dense layers' gradients are NOT accumulated here: the per-query vectors t, z0, dh,
//                       [M[u]*E[i] ; o1] and ds*h go to the workspace ...
//   gemm group          ... and are contracted by the exact-fp32 MFMA GEMM of gemm.hpp: dW = T^T Z0, dWd = DH^T X,
//                       db / dbd / dw as two-level fixed-order column sums
//   cmn_finish_kernel   + the gradient and the value of lambda ||W||_2
//   clip + sweep        pgmf.hip / optim.hip
#include "gemm.hpp"

namespace hiprec {

constexpr int kCmnMaxDim = 256;
constexpr int kCmnMaxBlocks = 1024;   // one scratch partial per block + one for the L2 term
constexpr int kCmnFinishThreads = 1024;

struct CmnArgs {
  hiprec_cmn_tables w, g;
  const int64_t *users, *pos, *neg;
  // padded form: nbr[side] is [batch, lpad[side]], len[side] is [batch]; CSR form: rowptr / col (nbr / len NULL)
  const int64_t* nbr[2];
  const int64_t* len[2];
  int64_t lpad[2];
  const int64_t *rowptr, *col;
  int64_t batch;
  float inv_batch;
  int backward;        // 0: forward only (scores out, no loss, no step)
  int n_sides;         // 1: the positive query only (forward(evaluation=True))
  float* scores[2];    // forward only
  float* ws;           // [2 * batch] rows of T, Z0, DH, DSH (D each) and X (2D)
  hiprec_stats* stats;
  Scratch* scratch;
  int G;               // lanes per row
};

struct CmnSide {
  float z0[kCmnMaxDim], o0[kCmnMaxDim], z1[kCmnMaxDim], o1[kCmnMaxDim], x0[kCmnMaxDim], h[kCmnMaxDim];
};

struct CmnShared {
  CmnSide side[2];
  float wave_o[kWavesPerBlock][kCmnMaxDim];
  float wave_m[kWavesPerBlock], wave_l[kWavesPerBlock];
  float dh[kCmnMaxDim], dx[2 * kCmnMaxDim], dz[kCmnMaxDim], t[kCmnMaxDim];
  float score[2];
};

template <bool VEC>
__device__ __forceinline__ int cmn_col(int sub, int k, int G) {
  return VEC ? 4 * sub + k : sub + G * k;
}

// the lane's four columns of a row (zeros beyond D)
template <bool VEC>
__device__ __forceinline__ void cmn_load_row(const float* __restrict__ row, int sub, int G, int D, float (&x)[4]) {
  if constexpr (VEC) {
    if (4 * sub < D) {
      const float4 v = *reinterpret_cast<const float4*>(row + 4 * sub);
      x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
      x[0] = x[1] = x[2] = x[3] = 0.f;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = sub + G * k;
      x[k] = c < D ? row[c] : 0.f;
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void cmn_load_lds(const float* v, int sub, int G, int D, float (&x)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = cmn_col<VEC>(sub, k, G);
    x[k] = c < D ? v[c] : 0.f;
  }
}

__device__ __forceinline__ float cmn_dot4(const float (&a)[4], const float (&b)[4]) {
  return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
}

// sum over the G lanes of a group (G a power of two; every lane of the group gets the total)
__device__ __forceinline__ float cmn_group_sum(float v, int G) {
  if (G == kWave) return wave_sum(v);
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sum over the groups of a wave (offsets G .. 32): lanes of group 0 (and every other) hold the wave's total
__device__ __forceinline__ float cmn_across_groups(float v, int G) {
  for (int o = G; o < kWave; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ float cmn_wave_max(float v) {
  for (int o = 1; o < kWave; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// dot of two LDS vectors, computed by every wave on its own (wave-uniform result)
__device__ __forceinline__ float cmn_lds_dot(const float* a, const float* b, int D) {
  float s = 0.f;
  for (int c = lane_id(); c < D; c += kWave) s += a[c] * b[c];
  return wave_sum(s);
}

// One neighbour id of a list, checked: -1 (and the status word raised) when it is no user.
__device__ __forceinline__ int cmn_neighbor(const int64_t* __restrict__ ids, int64_t j, int64_t n_users,
                                            hiprec_stats* stats) {
  const int64_t n = ids[j];
  if (static_cast<uint64_t>(n) >= static_cast<uint64_t>(n_users)) {
    atomicOr(&stats->status, HIPREC_STATUS_USER_OOB);
    return -1;
  }
  return static_cast<int>(n);
}

// One attention hop over a list: o = sum_j softmax_j(z . M[n_j]) C[n_j] into `o` (LDS), the softmax's maximum and
// denominator returned (block-uniform).  Online softmax per lane group, merged per wave, then per block.
template <bool VEC>
__device__ __forceinline__ void cmn_attend(const CmnArgs& a, CmnShared& sh, const int64_t* __restrict__ ids, int64_t L,
                                           const float* z, float* o, float* m_out, float* l_out) {
  const int D = a.w.dim, G = a.G, R = kWave / G;
  const int lane = lane_id(), wv = wave_in_block();
  const int sub = lane & (G - 1), grp = lane / G;
  float zr[4];
  cmn_load_lds<VEC>(z, sub, G, D, zr);
  float m = -INFINITY, l = 0.f, acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t j = static_cast<int64_t>(wv) * R + grp; j < L; j += static_cast<int64_t>(kWavesPerBlock) * R) {
    const int n = cmn_neighbor(ids, j, a.w.n_users, a.stats);
    if (n < 0) continue;
    float mr[4], cr[4];
    cmn_load_row<VEC>(a.w.user_memory + static_cast<int64_t>(n) * D, sub, G, D, mr);
    cmn_load_row<VEC>(a.w.user_output + static_cast<int64_t>(n) * D, sub, G, D, cr);
    const float s = cmn_group_sum(cmn_dot4(zr, mr), G);
    const float m_new = fmaxf(m, s);
    const float keep = expf(m - m_new);   // exp(-inf) = 0 on the group's first row
    const float e = expf(s - m_new);
    l = l * keep + e;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = acc[k] * keep + e * cr[k];
    m = m_new;
  }
  // per wave
  const float m_w = cmn_wave_max(m);
  const float f = (l > 0.f) ? expf(m - m_w) : 0.f;
  const float l_w = cmn_across_groups(l * f, G);
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = cmn_across_groups(acc[k] * f, G);
  if (grp == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = cmn_col<VEC>(sub, k, G);
      if (c < D) sh.wave_o[wv][c] = acc[k];
    }
  }
  if (lane == 0) {
    sh.wave_m[wv] = m_w;
    sh.wave_l[wv] = l_w;
  }
  __syncthreads();
  float m_b = sh.wave_m[0];
#pragma unroll
  for (int i = 1; i < kWavesPerBlock; ++i) m_b = fmaxf(m_b, sh.wave_m[i]);
  float fw[kWavesPerBlock], l_b = 0.f;
#pragma unroll
  for (int i = 0; i < kWavesPerBlock; ++i) {
    fw[i] = sh.wave_l[i] > 0.f ? expf(sh.wave_m[i] - m_b) : 0.f;
    l_b += sh.wave_l[i] * fw[i];
  }
  for (int c = threadIdx.x; c < D; c += kBlock) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kWavesPerBlock; ++i)
      if (fw[i] > 0.f) s += sh.wave_o[i][c] * fw[i];
    o[c] = s / l_b;
  }
  *m_out = m_b;
  *l_out = l_b;
  __syncthreads();
}

// out[r] = relu(sum_c W[r, c] v[c] + bias[r] (+ add[r])), r < n_rows: a wave per row, lanes over the columns
__device__ __forceinline__ void cmn_matvec_rows(const float* __restrict__ W, const float* __restrict__ bias, int n_rows,
                                                int n_cols, const float* v, const float* add, float* out) {
  const int lane = lane_id();
  for (int r = wave_in_block(); r < n_rows; r += kWavesPerBlock) {
    const float* row = W + static_cast<int64_t>(r) * n_cols;
    float s = 0.f;
    for (int c = lane; c < n_cols; c += kWave) s += row[c] * v[c];
    s = wave_sum(s);
    if (lane == 0) out[r] = fmaxf(s + bias[r] + (add ? add[r] : 0.f), 0.f);
  }
}

// out[c] = sum_r W[r, c] v[r], c < n_cols: a thread per column (coalesced across the block)
__device__ __forceinline__ void cmn_matvec_cols(const float* __restrict__ W, int n_rows, int n_cols, const float* v,
                                                float* out) {
  for (int c = threadIdx.x; c < n_cols; c += kBlock) {
    float s0 = 0.f, s1 = 0.f;
    int r = 0;
    for (; r + 1 < n_rows; r += 2) {
      s0 += W[static_cast<int64_t>(r) * n_cols + c] * v[r];
      s1 += W[static_cast<int64_t>(r + 1) * n_cols + c] * v[r + 1];
    }
    if (r < n_rows) s0 += W[static_cast<int64_t>(r) * n_cols + c] * v[r];
    out[c] = s0 + s1;
  }
}

struct CmnHopStats {
  float m0, l0, m1, l1;
};

// forward of one query; returns the score (block-uniform)
template <bool VEC>
__device__ __forceinline__ float cmn_forward_query(const CmnArgs& a, CmnShared& sh, CmnSide& sd, int64_t u, int64_t i,
                                                   const int64_t* __restrict__ ids, int64_t L, CmnHopStats* hs) {
  const int D = a.w.dim;
  for (int c = threadIdx.x; c < D; c += kBlock) {
    const float mu = a.w.user_memory[u * D + c], ei = a.w.item_memory[i * D + c];
    sd.z0[c] = mu + ei;
    sd.x0[c] = mu * ei;
  }
  __syncthreads();
  cmn_attend<VEC>(a, sh, ids, L, sd.z0, sd.o0, &hs->m0, &hs->l0);
  cmn_matvec_rows(a.w.hop_w, a.w.hop_b, D, D, sd.z0, sd.o0, sd.z1);
  __syncthreads();
  cmn_attend<VEC>(a, sh, ids, L, sd.z1, sd.o1, &hs->m1, &hs->l1);
  // h = relu(Wd [x0 ; o1] + bd): the two halves of a row of Wd against x0 and o1
  {
    const int lane = lane_id();
    for (int r = wave_in_block(); r < D; r += kWavesPerBlock) {
      const float* row = a.w.dense_w + static_cast<int64_t>(r) * 2 * D;
      float s = 0.f;
      for (int c = lane; c < D; c += kWave) s += row[c] * sd.x0[c] + row[D + c] * sd.o1[c];
      s = wave_sum(s);
      if (lane == 0) sd.h[r] = fmaxf(s + a.w.dense_b[r], 0.f);
    }
  }
  __syncthreads();
  float s = 0.f;
  for (int c = lane_id(); c < D; c += kWave) s += a.w.out_w[c] * sd.h[c];
  return wave_sum(s);
}

// One streaming pass of the backward over a list.  SCATTER = false (pass 1): dz1 = sum_j da1_j M[n_j] into sh.dz.
// SCATTER = true (pass 2): dz0 += sum_j da0_j M[n_j] (added to sh.dz, which holds W^T t on entry) and the row adds.
// do1 = sh.dx + D, do0 = sh.t; delta_k = do_k . o_k.
template <bool VEC, bool SCATTER>
__device__ __forceinline__ void cmn_backward_pass(const CmnArgs& a, CmnShared& sh, const CmnSide& sd,
                                                  const int64_t* __restrict__ ids, int64_t L, const CmnHopStats& hs,
                                                  float delta1, float delta0) {
  const int D = a.w.dim, G = a.G, R = kWave / G;
  const int lane = lane_id(), wv = wave_in_block();
  const int sub = lane & (G - 1), grp = lane / G;
  const float* do1 = sh.dx + D;
  float z1r[4], d1r[4], z0r[4], d0r[4];
  cmn_load_lds<VEC>(sd.z1, sub, G, D, z1r);
  cmn_load_lds<VEC>(do1, sub, G, D, d1r);
  if constexpr (SCATTER) {
    cmn_load_lds<VEC>(sd.z0, sub, G, D, z0r);
    cmn_load_lds<VEC>(sh.t, sub, G, D, d0r);
  }
  // lane = column layout of the scatter: Dp lanes per row, 64 / Dp rows per wave instruction
  const int Dp = D >= kWave ? kWave : (1 << (32 - __builtin_clz(D - 1)));   // D >= 4
  const int rows_per_instr = kWave / Dp;
  const int c0 = lane & (Dp - 1), rsel = lane / Dp;
  float z1c[4], z0c[4], d1c[4], d0c[4];
  if constexpr (SCATTER) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + kWave * k;
      const bool in = c < D && (k == 0 || Dp == kWave);
      z1c[k] = in ? sd.z1[c] : 0.f;
      z0c[k] = in ? sd.z0[c] : 0.f;
      d1c[k] = in ? do1[c] : 0.f;
      d0c[k] = in ? sh.t[c] : 0.f;
    }
  }
  const float inv_l1 = 1.f / hs.l1, inv_l0 = 1.f / hs.l0;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t stride = static_cast<int64_t>(kWavesPerBlock) * R;
  // every wave runs the same number of rounds of its R groups; a group beyond the list idles (the shuffles of the
  // scatter need the whole wave)
  for (int64_t base = static_cast<int64_t>(wv) * R; base < L; base += stride) {
    const int64_t j = base + grp;
    int n = -1;
    float da1 = 0.f, da0 = 0.f, p1 = 0.f, p0 = 0.f;
    if (j < L) n = cmn_neighbor(ids, j, a.w.n_users, a.stats);
    if (n >= 0) {
      float mr[4], cr[4];
      cmn_load_row<VEC>(a.w.user_memory + static_cast<int64_t>(n) * D, sub, G, D, mr);
      cmn_load_row<VEC>(a.w.user_output + static_cast<int64_t>(n) * D, sub, G, D, cr);
      const float a1 = cmn_group_sum(cmn_dot4(z1r, mr), G);
      const float dp1 = cmn_group_sum(cmn_dot4(d1r, cr), G);
      p1 = expf(a1 - hs.m1) * inv_l1;
      da1 = p1 * (dp1 - delta1);
      if constexpr (SCATTER) {
        const float a0 = cmn_group_sum(cmn_dot4(z0r, mr), G);
        const float dp0 = cmn_group_sum(cmn_dot4(d0r, cr), G);
        p0 = expf(a0 - hs.m0) * inv_l0;
        da0 = p0 * (dp0 - delta0);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += da0 * mr[k];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += da1 * mr[k];
      }
    }
    if constexpr (SCATTER) {
      for (int r0 = 0; r0 < R; r0 += rows_per_instr) {
        const int r = r0 + rsel;              // the group whose row this lane adds a column of
        const int src = (r < R ? r : 0) * G;
        const int nn = __shfl(n, src);
        const float s_da1 = __shfl(da1, src), s_da0 = __shfl(da0, src);
        const float s_p1 = __shfl(p1, src), s_p0 = __shfl(p0, src);
        if (r < R && nn >= 0) {
          float* gm = a.g.user_memory + static_cast<int64_t>(nn) * D;
          float* gc = a.g.user_output + static_cast<int64_t>(nn) * D;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int c = c0 + kWave * k;
            if (c < D && (k == 0 || Dp == kWave)) {
              atomic_add_f32(gm + c, s_da1 * z1c[k] + s_da0 * z0c[k]);
              atomic_add_f32(gc + c, s_p1 * d1c[k] + s_p0 * d0c[k]);
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = cmn_across_groups(acc[k], G);
  if (grp == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = cmn_col<VEC>(sub, k, G);
      if (c < D) sh.wave_o[wv][c] = acc[k];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += kBlock) {
    const float s = (sh.wave_o[0][c] + sh.wave_o[1][c]) + (sh.wave_o[2][c] + sh.wave_o[3][c]);
    sh.dz[c] = SCATTER ? sh.dz[c] + s : s;
  }
  __syncthreads();
}

// backward of one query whose score received the gradient ds; q = its row in the workspace
template <bool VEC>
__device__ __forceinline__ void cmn_backward_query(const CmnArgs& a, CmnShared& sh, const CmnSide& sd, int64_t u,
                                                   int64_t i, const int64_t* __restrict__ ids, int64_t L,
                                                   const CmnHopStats& hs, float ds, int64_t q, int64_t Q) {
  const int D = a.w.dim;
  float* T = a.ws + q * D;
  float* Z0 = a.ws + (Q + q) * D;
  float* DH = a.ws + (2 * Q + q) * D;
  float* DSH = a.ws + (3 * Q + q) * D;
  float* X = a.ws + 4 * Q * D + q * 2 * D;
  for (int c = threadIdx.x; c < D; c += kBlock) {
    const float h = sd.h[c];
    const float dh = h > 0.f ? ds * a.w.out_w[c] : 0.f;
    sh.dh[c] = dh;
    DH[c] = dh;
    DSH[c] = ds * h;
    X[c] = sd.x0[c];
    X[D + c] = sd.o1[c];
    Z0[c] = sd.z0[c];
  }
  __syncthreads();
  cmn_matvec_cols(a.w.dense_w, D, 2 * D, sh.dh, sh.dx);   // dx[:D] -> M[u] * E[i], dx[D:] = do1
  __syncthreads();
  const float delta1 = cmn_lds_dot(sh.dx + D, sd.o1, D);
  cmn_backward_pass<VEC, false>(a, sh, sd, ids, L, hs, delta1, 0.f);
  for (int c = threadIdx.x; c < D; c += kBlock) {
    const float t = sd.z1[c] > 0.f ? sh.dz[c] : 0.f;
    sh.t[c] = t;
    T[c] = t;
  }
  __syncthreads();
  cmn_matvec_cols(a.w.hop_w, D, D, sh.t, sh.dz);          // dz0 = W^T t
  __syncthreads();
  const float delta0 = cmn_lds_dot(sh.t, sd.o0, D);
  cmn_backward_pass<VEC, true>(a, sh, sd, ids, L, hs, delta1, delta0);
  for (int c = threadIdx.x; c < D; c += kBlock) {
    const float mu = a.w.user_memory[u * D + c], ei = a.w.item_memory[i * D + c];
    const float dz0 = sh.dz[c], dx0 = sh.dx[c];
    atomic_add_f32(a.g.user_memory + u * D + c, dx0 * ei + dz0);
    atomic_add_f32(a.g.item_memory + i * D + c, dx0 * mu + dz0);
  }
  __syncthreads();
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void cmn_sample_kernel(CmnArgs a) {
  __shared__ CmnShared sh;
  const int D = a.w.dim;
  const int64_t Q = 2 * a.batch;
  const bool stepper = a.backward && blockIdx.x == 0 && threadIdx.x == 0;
  StepState step_state{};
  if (stepper) step_state = step_load(a.stats);

  float loss_acc = 0.f;
  for (int64_t b = blockIdx.x; b < a.batch; b += gridDim.x) {
    const int64_t u = a.users[b];
    const int64_t item[2] = {a.pos[b], a.n_sides > 1 ? a.neg[b] : 0};
    const bool u_ok = static_cast<uint64_t>(u) < static_cast<uint64_t>(a.w.n_users);
    const bool i_ok = static_cast<uint64_t>(item[0]) < static_cast<uint64_t>(a.w.n_items) &&
                      static_cast<uint64_t>(item[1]) < static_cast<uint64_t>(a.w.n_items);
    const int64_t* ids[2] = {nullptr, nullptr};
    int64_t L[2] = {0, 0};
    bool l_ok = true;
    if (u_ok && i_ok) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (s >= a.n_sides) continue;
        if (a.rowptr) {
          const int64_t lo = a.rowptr[item[s]];
          ids[s] = a.col + lo;
          L[s] = a.rowptr[item[s] + 1] - lo;
          l_ok = l_ok && L[s] >= 1;
        } else {
          ids[s] = a.nbr[s] + b * a.lpad[s];
          L[s] = a.len[s][b];
          l_ok = l_ok && L[s] >= 1 && L[s] <= a.lpad[s];
        }
      }
    }
    if (!(u_ok && i_ok && l_ok)) {      // block-uniform
      if (threadIdx.x == 0)
        atomicOr(&a.stats->status, (u_ok ? 0u : HIPREC_STATUS_USER_OOB) | (i_ok ? 0u : HIPREC_STATUS_ITEM_OOB) |
                                       (l_ok ? 0u : HIPREC_STATUS_ROW_OOB));
      if (a.backward) {                 // the contractions read every row of the workspace
        for (int s = 0; s < 2; ++s) {
          const int64_t q = s * a.batch + b;
          for (int c = threadIdx.x; c < D; c += kBlock) {
            for (int part = 0; part < 4; ++part) a.ws[(part * Q + q) * D + c] = 0.f;
            a.ws[4 * Q * D + q * 2 * D + c] = 0.f;
            a.ws[4 * Q * D + q * 2 * D + D + c] = 0.f;
          }
        }
      } else {
        if (threadIdx.x == 0) {
          a.scores[0][b] = 0.f;
          if (a.n_sides > 1) a.scores[1][b] = 0.f;
        }
      }
      continue;
    }
    CmnHopStats hs[2];
    float score[2] = {0.f, 0.f};
    score[0] = cmn_forward_query<VEC>(a, sh, sh.side[0], u, item[0], ids[0], L[0], &hs[0]);
    if (a.n_sides > 1) score[1] = cmn_forward_query<VEC>(a, sh, sh.side[1], u, item[1], ids[1], L[1], &hs[1]);
    if (!a.backward) {
      if (threadIdx.x == 0) {
        a.scores[0][b] = score[0];
        if (a.n_sides > 1) a.scores[1][b] = score[1];
      }
      __syncthreads();
      continue;
    }
    // the engine's bpr_loss: -log(sigmoid(x) + 1e-12); d loss / d x = -(y (1 - y)) / (y + eps) / B
    const float x = score[0] - score[1];
    const float y = sigmoid_f32(x);
    loss_acc += -logf(y + 1e-12f);
    const float dx = -(a.inv_batch / (y + 1e-12f)) * ((1.f - y) * y);
    cmn_backward_query<VEC>(a, sh, sh.side[0], u, item[0], ids[0], L[0], hs[0], dx, b, Q);
    cmn_backward_query<VEC>(a, sh, sh.side[1], u, item[1], ids[1], L[1], hs[1], -dx, a.batch + b, Q);
  }
  if (!a.backward) return;
  // every wave holds the block's loss; only wave 0 contributes it
  publish_partials<kWavesPerBlock>(wave_in_block() == 0 ? loss_acc : 0.f, 0.f, 0.f, a.inv_batch, a.scratch);
  if (stepper) step_store_advanced(a.stats, step_state);
}

// One block.  g.hop_w += lambda * W / ||W||_2 (sqrt backward then pow backward, 0/0 -> NaN as autograd gives);
// loss partial += lambda * ||W||_2.  Fixed-order sum of squares.
__global__ __launch_bounds__(kCmnFinishThreads) void cmn_finish_kernel(hiprec_cmn_tables w, hiprec_cmn_tables g,
                                                                       float l2_lambda, Scratch* scratch) {
  __shared__ float s_sq[kCmnFinishThreads];
  const int n = w.dim * w.dim;
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += kCmnFinishThreads) s += w.hop_w[i] * w.hop_w[i];
  s_sq[threadIdx.x] = s;
  __syncthreads();
  for (int r = kCmnFinishThreads / 2; r > 0; r >>= 1) {
    if (static_cast<int>(threadIdx.x) < r) s_sq[threadIdx.x] += s_sq[threadIdx.x + r];
    __syncthreads();
  }
  const float l2 = sqrtf(s_sq[0]);
  const float coef = l2_lambda / (2.f * l2);
  for (int i = threadIdx.x; i < n; i += kCmnFinishThreads) g.hop_w[i] += coef * (2.f * w.hop_w[i]);
  if (threadIdx.x == 0) {
    const uint32_t np = scratch->n_partials;
    scratch->partials[np] = make_float4(l2_lambda * l2, 0.f, 0.f, 0.f);
    scratch->n_partials = np + 1;
  }
}

inline int cmn_lanes_per_row(int dim) {
  int g = 1;
  while (4 * g < dim) g <<= 1;
  return g;
}

inline int64_t cmn_ws_floats(int dim, int64_t max_batch) {
  const int64_t Q = 2 * max_batch;
  return 6 * Q * dim + 3 * colsum_ws_floats(static_cast<int>(Q), dim);
}

static int cmn_check_tables(const hiprec_cmn_tables* w, const hiprec_cmn_tables* g) {
  HIPREC_REQUIRE(w, "NULL tables");
  HIPREC_REQUIRE(w->user_memory && w->item_memory && w->user_output && w->hop_w && w->hop_b && w->dense_w &&
                     w->dense_b && w->out_w,
                 "NULL tensor pointer");
  HIPREC_REQUIRE(w->n_users > 0 && w->n_items > 0 && w->n_users < (1ll << 31) && w->dim >= 4 && w->dim <= kCmnMaxDim,
                 "CMN needs 4 <= dim <= %d (got %d) and fewer than 2^31 users", kCmnMaxDim, w->dim);
  if (g) {
    HIPREC_REQUIRE(g->user_memory && g->item_memory && g->user_output && g->hop_w && g->hop_b && g->dense_w &&
                       g->dense_b && g->out_w,
                   "NULL gradient pointer");
    HIPREC_REQUIRE(w->n_users == g->n_users && w->n_items == g->n_items && w->dim == g->dim,
                   "weight / gradient shapes differ");
  }
  return 0;
}

static int cmn_launch(CmnArgs& a, const hiprec_cmn_tables* w, const hiprec_cmn_tables* g, float l2_lambda,
                      void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = cmn_check_tables(w, g)) return rc;
  HIPREC_REQUIRE(a.stats, "NULL stats");
  HIPREC_REQUIRE(a.batch >= 0 && a.batch < (1ll << 29), "bad batch");
  HIPREC_REQUIRE(a.batch == 0 || (a.users && a.pos), "NULL index arrays");
  a.w = *w;
  a.backward = g != nullptr;
  if (g) {
    a.g = *g;
    a.n_sides = 2;
    HIPREC_REQUIRE(a.batch == 0 || a.neg, "NULL index arrays");
    HIPREC_REQUIRE(scratch && workspace, "NULL scratch/workspace");
    if (scratch_bytes < kScratchBytes) {
      set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
      return HIPREC_E_SCRATCH;
    }
    const size_t need = sizeof(float) * static_cast<size_t>(cmn_ws_floats(w->dim, a.batch));
    HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
    a.scratch = static_cast<Scratch*>(scratch);
    a.ws = static_cast<float*>(workspace);
  } else {
    HIPREC_REQUIRE(a.scores[0], "forward only needs a score buffer");
    a.n_sides = a.scores[1] ? 2 : 1;
    HIPREC_REQUIRE(a.n_sides == 1 || a.batch == 0 || a.neg, "NULL index arrays");
  }
  a.G = cmn_lanes_per_row(w->dim);
  auto s = static_cast<hipStream_t>(stream);
  if (a.batch == 0 && !g) return 0;
  const int grid = static_cast<int>(a.batch < 1 ? 1 : (a.batch > kCmnMaxBlocks ? kCmnMaxBlocks : a.batch));
  const bool vec = (w->dim & 3) == 0;
  if (vec) cmn_sample_kernel<true><<<grid, kBlock, 0, s>>>(a);
  else cmn_sample_kernel<false><<<grid, kBlock, 0, s>>>(a);
  HIPREC_TRY(hipGetLastError());
  if (!g) return 0;
  if (a.batch > 0) {
    const int D = w->dim, Q = static_cast<int>(2 * a.batch);
    const int64_t QD = static_cast<int64_t>(Q) * D;
    float* cs = a.ws + 6 * QD;
    const int64_t cs_n = colsum_ws_floats(Q, D);
    GemmGroup grp{};
    grp.n = 5;
    grp.p[0] = make_gemm(kTNm, D, D, Q, a.ws, D, a.ws + QD, D, g->hop_w, D, nullptr, 0, nullptr, 0, true);
    grp.p[1] = make_gemm(kTNm, D, 2 * D, Q, a.ws + 2 * QD, D, a.ws + 4 * QD, 2 * D, g->dense_w, 2 * D, nullptr, 0,
                         nullptr, 0, true);
    grp.p[2] = make_colsum(a.ws, Q, D, D, g->hop_b, cs);
    grp.p[3] = make_colsum(a.ws + 2 * QD, Q, D, D, g->dense_b, cs + cs_n);
    grp.p[4] = make_colsum(a.ws + 3 * QD, Q, D, D, g->out_w, cs + 2 * cs_n);
    if (int rc = launch_group(grp, s)) return rc;
    if (int rc = launch_colsum_reduce(grp, s)) return rc;
  }
  if (l2_lambda != 0.f) {
    cmn_finish_kernel<<<1, kCmnFinishThreads, 0, s>>>(*w, *g, l2_lambda, a.scratch);
    HIPREC_TRY(hipGetLastError());
  }
  return 0;
}

}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_cmn_tables_bytes(void) { return sizeof(hiprec_cmn_tables); }

extern "C" size_t hiprec_cmn_workspace_bytes(int32_t dim, int64_t max_batch) {
  if (dim <= 0 || max_batch <= 0) return 0;
  return sizeof(float) * static_cast<size_t>(cmn_ws_floats(dim, max_batch));
}

extern "C" int hiprec_cmn_grad_padded(const hiprec_cmn_tables* w, const hiprec_cmn_tables* g, const int64_t* users,
                                      const int64_t* pos, const int64_t* neg, const int64_t* pos_nbr,
                                      const int64_t* pos_len, int64_t pos_lpad, const int64_t* neg_nbr,
                                      const int64_t* neg_len, int64_t neg_lpad, int64_t batch, float inv_batch,
                                      float l2_lambda, float* pos_scores, float* neg_scores, hiprec_stats* stats,
                                      void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  CmnArgs a{};
  const bool two = g || neg_scores;
  HIPREC_REQUIRE(batch == 0 || (pos_nbr && pos_len && pos_lpad >= 1), "NULL / empty positive neighbourhoods");
  HIPREC_REQUIRE(batch == 0 || !two || (neg_nbr && neg_len && neg_lpad >= 1), "NULL / empty negative neighbourhoods");
  a.users = users; a.pos = pos; a.neg = neg;
  a.nbr[0] = pos_nbr; a.len[0] = pos_len; a.lpad[0] = pos_lpad;
  a.nbr[1] = neg_nbr; a.len[1] = neg_len; a.lpad[1] = neg_lpad;
  a.batch = batch; a.inv_batch = inv_batch;
  a.scores[0] = pos_scores; a.scores[1] = neg_scores;
  a.stats = stats;
  return cmn_launch(a, w, g, l2_lambda, scratch, scratch_bytes, workspace, workspace_bytes, stream);
}

extern "C" int hiprec_cmn_grad_csr(const hiprec_cmn_tables* w, const hiprec_cmn_tables* g, const int64_t* users,
                                   const int64_t* pos, const int64_t* neg, const int64_t* rowptr, const int64_t* col,
                                   int64_t batch, float inv_batch, float l2_lambda, float* pos_scores,
                                   float* neg_scores, hiprec_stats* stats, void* scratch, size_t scratch_bytes,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  CmnArgs a{};
  HIPREC_REQUIRE(rowptr && col, "NULL CSR (one row per item, n_items + 1 row pointers)");
  a.users = users; a.pos = pos; a.neg = neg;
  a.rowptr = rowptr; a.col = col;
  a.batch = batch; a.inv_batch = inv_batch;
  a.scores[0] = pos_scores; a.scores[1] = neg_scores;
  a.stats = stats;
  return cmn_launch(a, w, g, l2_lambda, scratch, scratch_bytes, workspace, workspace_bytes, stream);
}

// cmnEngine.train_an_epoch (cmn.py:202-267) over resident (user, pos, neg) arrays in visiting order, the lists taken
// from the item -> users CSR: every batch is hiprec_cmn_grad_csr + hiprec_clip_opt_dense_step, enqueued back to back.
extern "C" int hiprec_cmn_epoch(const hiprec_cmn_tables* w, const hiprec_cmn_tables* g, const int64_t* users,
                                const int64_t* pos, const int64_t* neg, const int64_t* rowptr, const int64_t* col,
                                int64_t n_triples, int64_t batch, float l2_lambda, float max_norm, int kind, double lr,
                                double beta1, double beta2, double eps, float* flat_w, float* flat_g, float* flat_m,
                                float* flat_v, int64_t n_flat, hiprec_stats* stats, void* scratch, size_t scratch_bytes,
                                void* workspace, size_t workspace_bytes, void* clip_workspace,
                                size_t clip_workspace_bytes, void* stream) {
  HIPREC_REQUIRE(n_triples >= 0 && batch > 0, "bad n_triples/batch");
  HIPREC_REQUIRE(g, "the epoch needs the gradient tables");
  HIPREC_REQUIRE(flat_w && flat_g && n_flat > 0, "the dense optimizer needs the flat buffers");
  if (int rc = hiprec_stats_begin_epoch(stats, stream)) return rc;
  for (int64_t off = 0; off < n_triples; off += batch) {
    const int64_t b = (n_triples - off < batch) ? (n_triples - off) : batch;
    if (int rc = hiprec_cmn_grad_csr(w, g, users + off, pos + off, neg + off, rowptr, col, b,
                                     1.0f / static_cast<float>(b), l2_lambda, nullptr, nullptr, stats, scratch,
                                     scratch_bytes, workspace, workspace_bytes, stream))
      return rc;
    if (int rc = hiprec_clip_opt_dense_step(kind, flat_w, flat_g, flat_m, flat_v, n_flat, lr, beta1, beta2, eps, stats,
                                            scratch, -1, max_norm, clip_workspace, clip_workspace_bytes, stream))
      return rc;
  }
  return 0;
}
