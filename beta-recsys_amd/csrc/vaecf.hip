// VAECF (Mult-VAE): the variational autoencoder of beta_rec/models/vaecf.py.
//
//   vaecf.py:26-43    parameters: encoder.fc{l} [h_l, h_{l-1}] (h_{-1} = n_items), enc_mu / enc_logvar [Z, h_last],
//                     decoder.fc{l} over [Z, h_last, ..., h_0, n_items]; the activation follows every layer but the last
//   vaecf.py:45-64    forward: (mu, logvar) = encode(x), z = mu + eps exp(0.5 logvar), x_ = softmax / sigmoid(decoder(z))
//   vaecf.py:66-87    loss: mean_b(beta kld_b - ll_b), EPS = 1e-10 inside the logs
//   vaecf.py:134-142  train_single_batch: zero_grad, forward, loss, backward, step
//
// The reference works on a dense [B, n_items] batch; here a batch is CSR (row_ptr, items, values) and no [B, n_items]
// buffer exists.  One step:
//   1 first layer     h0[b] = act(b0 + sum_{i in row b} v_bi W0[:, i]), one wave per row        vc_first_kernel
//                     (W0 gathered as it lies, or from a transposed shadow refreshed by vc_transpose_kernel)
//   2 middle layers   the other encoder layers, enc_mu | enc_logvar (one launch), the decoder up to Hd [B, h_0]: the
//                     grouped GEMM of csrc/ncf.hip (relu in its epilogue, the other activations in vc_act_kernel)
//   3 reparameterise  z = mu + eps exp(0.5 logvar)                                               vc_reparam_kernel
//   4 last layer + likelihood + backward over 64 x 64 tiles of (rows, items):
//       pass A (mult)  each tile's logits Hd W_L^T + b_L, an online log-sum-exp per row and item split   vc_dense_kernel<true>
//       sparse pass    one wave per row: the splits' log-sum-exps combined in split order, then over the row's nonzeros
//                      ll_b, c_b and the sparse correction of dlogit, which goes to dHd (plain stores: the row is the
//                      wave's), dW_L and db_L (atomics)                                           vc_sparse_kernel
//       pass B         each tile's logits again, the dense (x = 0) part of dlogit left in LDS, and from there dHd, dW_L
//                      and db_L with atomics; for bern / gaus / pois also the dense part of ll    vc_dense_kernel<false>
//   5 backward        decoder layers (grouped GEMM), the latent stage (KL, dmu, dlogvar and the loss partials)
//                     vc_latent_kernel, the encoder layers, and the first layer's dW0[:, i] += v_bi dpre0[b] over the
//                     nonzeros only                                                              vc_first_bwd_kernel
// Saved for the backward: every layer's activation (act' is taken from it), (mu | logvar), z.
#include <algorithm>

#include "gemm.hpp"

namespace hiprec {
namespace {

constexpr int kVcMaxZ = 256;        // z_dim
constexpr int kVcMaxHidden = 512;   // every hidden width (csrc/topk.hip ranks rows of Hd: its MAX_DIM)
constexpr int kVcMaxLayers = 3;     // hidden layers
constexpr int kVcNpl = kVcMaxHidden / kWave;   // columns of a hidden row per lane
constexpr int kVcTile = 64;         // rows and items of one tile of the fused last layer
constexpr int kVcKc = 32;           // its K chunk
constexpr int kVcMaxSplits = 64;    // item splits of the last layer (each leaves one (max, sum) pair per row)
constexpr int kVcChunk = 8192;      // rows per pass of the inference encoder
constexpr float kVcEps = 1e-10f;    // vaecf.py:24

__device__ __forceinline__ bool vc_in_range(int64_t i, int64_t n) {
  return static_cast<uint64_t>(i) < static_cast<uint64_t>(n);
}

__device__ __forceinline__ float vc_act(float x, int act) {
  switch (act) {
    case HIPREC_VAECF_ACT_SIGMOID: return 1.0f / (1.0f + expf(-x));
    case HIPREC_VAECF_ACT_TANH: return tanhf(x);
    case HIPREC_VAECF_ACT_RELU: return x > 0.f ? x : 0.f;
    default: return fminf(fmaxf(x, 0.f), 6.0f);
  }
}

// the derivative, taken from the activation's value
__device__ __forceinline__ float vc_act_grad(float h, int act) {
  switch (act) {
    case HIPREC_VAECF_ACT_SIGMOID: return h * (1.0f - h);
    case HIPREC_VAECF_ACT_TANH: return 1.0f - h * h;
    case HIPREC_VAECF_ACT_RELU: return h > 0.f ? 1.0f : 0.f;
    default: return (h > 0.f && h < 6.0f) ? 1.0f : 0.f;
  }
}

// a row's extent in the CSR arrays; a row_ptr that does not fit them sets the status bit and yields an empty row
__device__ __forceinline__ void vc_row_extent(const int64_t* __restrict__ row_ptr, int64_t b, int64_t nnz, int lane,
                                              hiprec_stats* stats, int64_t* s, int64_t* e) {
  *s = row_ptr[b];
  *e = row_ptr[b + 1];
  if (*s < 0 || *e < *s || *e > nnz) {
    if (lane == 0 && stats) atomicOr(&stats->status, HIPREC_STATUS_ROW_OOB);
    *s = *e = 0;
  }
}

// ---- 1. the sparse first layer ----------------------------------------------------------------------------------------
// W0[h, i] is read at W[h * sh + i * si]: (sh, si) = (n_items, 1) for the parameter as it lies, (1, H) for the shadow.
__global__ __launch_bounds__(kBlock) void vc_first_kernel(const int64_t* __restrict__ row_ptr,
                                                          const int64_t* __restrict__ items,
                                                          const float* __restrict__ values, int64_t n_rows, int64_t nnz,
                                                          const float* __restrict__ W, int64_t sh, int64_t si,
                                                          const float* __restrict__ bias, int H, int64_t I, int act,
                                                          float* __restrict__ H0, hiprec_stats* stats) {
  const int lane = lane_id();
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); b < n_rows;
       b += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    int64_t s, e;
    vc_row_extent(row_ptr, b, nnz, lane, stats, &s, &e);
    float acc[kVcNpl];
#pragma unroll
    for (int k = 0; k < kVcNpl; ++k) {
      const int h = lane + kWave * k;
      acc[k] = h < H ? bias[h] : 0.f;
    }
    for (int64_t base = s; base < e; base += kWave) {
      const int64_t idx = base + lane;
      const bool in = idx < e;
      long long it = in ? items[idx] : 0;
      float v = in ? values[idx] : 0.f;
      if (in && !vc_in_range(it, I)) {
        atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
        it = 0;
        v = 0.f;
      }
      const int cnt = e - base < kWave ? static_cast<int>(e - base) : kWave;
      for (int q = 0; q < cnt; ++q) {
        const long long iq = __shfl(it, q);
        const float vq = __shfl(v, q);
        if (vq == 0.f) continue;
#pragma unroll
        for (int k = 0; k < kVcNpl; ++k) {
          const int h = lane + kWave * k;
          if (h < H) acc[k] = fmaf(vq, W[h * sh + iq * si], acc[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kVcNpl; ++k) {
      const int h = lane + kWave * k;
      if (h < H) H0[b * H + h] = vc_act(acc[k], act);
    }
  }
}

// dpre0 = (d + add) act'(h0), left in d; dW0[:, i] += v_bi dpre0[b] over the nonzeros (gW is [H, n_items])
__global__ __launch_bounds__(kBlock) void vc_first_bwd_kernel(const int64_t* __restrict__ row_ptr,
                                                              const int64_t* __restrict__ items,
                                                              const float* __restrict__ values, int64_t n_rows,
                                                              int64_t nnz, float* __restrict__ d,
                                                              const float* __restrict__ add,
                                                              const float* __restrict__ H0, int H, int64_t I, int act,
                                                              float* __restrict__ gW) {
  const int lane = lane_id();
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); b < n_rows;
       b += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    int64_t s, e;
    vc_row_extent(row_ptr, b, nnz, lane, nullptr, &s, &e);
    float dp[kVcNpl];
#pragma unroll
    for (int k = 0; k < kVcNpl; ++k) {
      const int h = lane + kWave * k;
      dp[k] = 0.f;
      if (h < H) {
        dp[k] = (d[b * H + h] + (add ? add[b * H + h] : 0.f)) * vc_act_grad(H0[b * H + h], act);
        d[b * H + h] = dp[k];
      }
    }
    for (int64_t base = s; base < e; base += kWave) {
      const int64_t idx = base + lane;
      const bool in = idx < e;
      long long it = in ? items[idx] : 0;
      float v = in ? values[idx] : 0.f;
      if (!vc_in_range(it, I)) {   // the forward has raised the status
        it = 0;
        v = 0.f;
      }
      const int cnt = e - base < kWave ? static_cast<int>(e - base) : kWave;
      for (int q = 0; q < cnt; ++q) {
        const long long iq = __shfl(it, q);
        const float vq = __shfl(v, q);
        if (vq == 0.f) continue;
#pragma unroll
        for (int k = 0; k < kVcNpl; ++k) {
          const int h = lane + kWave * k;
          if (h < H) atomic_add_f32(gW + h * I + iq, vq * dp[k]);
        }
      }
    }
  }
}

// WT[i, h] = W[h, i] through a 32 x 33 LDS tile
__global__ __launch_bounds__(kBlock) void vc_transpose_kernel(const float* __restrict__ W, int H, int64_t I,
                                                              float* __restrict__ WT) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t tiles_i = (I + 31) / 32, tiles_h = (H + 31) / 32;
  for (int64_t t = blockIdx.x; t < tiles_i * tiles_h; t += gridDim.x) {
    const int64_t i0 = (t / tiles_h) * 32;
    const int h0 = static_cast<int>(t % tiles_h) * 32;
    for (int r = ty; r < 32; r += 8)
      tile[r][tx] = (h0 + r < H && i0 + tx < I) ? W[static_cast<int64_t>(h0 + r) * I + i0 + tx] : 0.f;
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
      if (i0 + r < I && h0 + tx < H) WT[(i0 + r) * H + h0 + tx] = tile[tx][r];
    __syncthreads();
  }
}

// ---- 2. activations the GEMM epilogue does not offer --------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void vc_act_kernel(float* __restrict__ a, int64_t n, int act) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) a[e] = vc_act(a[e], act);
}

// d = (d + add) act'(h)
__global__ __launch_bounds__(kBlock) void vc_act_bwd_kernel(float* __restrict__ d, const float* __restrict__ add,
                                                            const float* __restrict__ h, int64_t n, int act) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride)
    d[e] = (d[e] + (add ? add[e] : 0.f)) * vc_act_grad(h[e], act);
}

// ---- 3. reparameterisation, and the latent stage of the backward ------------------------------------------------------
// z = mu + eps exp(0.5 logvar) (vaecf.py:56-59); ML is [B, 2Z] = (mu | logvar)
__global__ __launch_bounds__(kBlock) void vc_reparam_kernel(const float* __restrict__ ML, const float* __restrict__ eps,
                                                            int64_t B, int Z, float* __restrict__ z) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < B * Z; e += stride) {
    const int64_t b = e / Z;
    const int c = static_cast<int>(e - b * Z);
    z[e] = ML[b * 2 * Z + c] + eps[e] * expf(0.5f * ML[b * 2 * Z + Z + c]);
  }
}

// One wave per row: kld_b = -0.5 sum(1 + 2 log(std) - mu^2 - std^2) (vaecf.py:83-85), dmu = dz + beta / B mu,
// dlogvar = dz eps 0.5 std + beta / B 0.5 (std^2 - 1); the row's ll (the sparse pass's part + the dense parts of every
// item split, in split order) joins the loss partials: stats.loss = mean ll, stats.reg = mean kld.
__global__ __launch_bounds__(kBlock) void vc_latent_kernel(const float* __restrict__ ML, const float* __restrict__ eps,
                                                           const float* __restrict__ dz, int64_t B, int Z, float beta_b,
                                                           float inv_b, const float* __restrict__ ll,
                                                           const float* __restrict__ ll0, int n_splits,
                                                           float* __restrict__ dML, hiprec_stats* stats,
                                                           Scratch* scratch) {
  const int lane = lane_id();
  const bool stepper = blockIdx.x == 0 && threadIdx.x == 0;
  StepState step_state{};
  if (stepper) step_state = step_load(stats);
  float ll_w = 0.f, kl_lane = 0.f;
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); b < B;
       b += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    for (int c = lane; c < Z; c += kWave) {
      const float mu = ML[b * 2 * Z + c], lv = ML[b * 2 * Z + Z + c], ep = eps[b * Z + c], g = dz[b * Z + c];
      const float sd = expf(0.5f * lv);
      kl_lane += -0.5f * (1.0f + 2.0f * logf(sd) - mu * mu - sd * sd);
      dML[b * 2 * Z + c] = g + beta_b * mu;
      dML[b * 2 * Z + Z + c] = g * ep * 0.5f * sd + beta_b * 0.5f * (sd * sd - 1.0f);
    }
    float row = ll[b];
    if (ll0)
      for (int sp = 0; sp < n_splits; ++sp) row += ll0[sp * B + b];
    ll_w += row;
  }
  publish_partials<kWavesPerBlock>(ll_w, kl_lane, 0.f, inv_b, scratch);
  if (stepper) step_store_advanced(stats, step_state);
}

// ---- 4. the fused last layer ------------------------------------------------------------------------------------------
// the log-sum-exp of row b from the (max, sum) pairs the item splits left, combined in split order
__device__ __forceinline__ float vc_combine_lse(const float* __restrict__ parts, int n_splits, int64_t B, int64_t b) {
  float M = -INFINITY;
  for (int sp = 0; sp < n_splits; ++sp) M = fmaxf(M, parts[(sp * B + b) * 2]);
  float S = 0.f;
  for (int sp = 0; sp < n_splits; ++sp) {
    const float m = parts[(sp * B + b) * 2];
    if (m > -INFINITY) S += parts[(sp * B + b) * 2 + 1] * expf(m - M);
  }
  return M + logf(S);
}

struct VcDense {
  const float* Hd;     // [B, H]
  const float* W;      // [I, H]: the decoder's last weight
  const float* bias;   // [I]
  int H, lik, n_splits;
  int64_t B, I, n_tiles;
  float* parts;        // pass A: [n_splits, B, 2] (max, sum)
  const float* lse;    // pass B, mult: [B]
  const float* c;      // pass B, mult: [B]
  float inv_b;
  float* ll0;          // pass B, not mult: [n_splits, B] the dense part of ll
  float *dHd, *gW, *gb;
};

// grid (row blocks, item splits); a block walks the item tiles split, split + n_splits, ... of its 64 rows
template <bool PASS_A>
__global__ __launch_bounds__(kBlock) void vc_dense_kernel(VcDense a) {
  __shared__ float As[kVcTile][kVcKc + 1];                   // Hd[b0 + r, k0 + k]
  __shared__ float Bs[kVcTile][kVcKc + 1];                   // W[j0 + j, k0 + k]
  __shared__ __align__(16) float Dm[kVcTile][kVcTile + 4];   // dlogit[row][item]
  __shared__ __align__(16) float Dt[kVcTile][kVcTile + 4];   // dlogit[item][row]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int H = a.H;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * kVcTile;
  const int split = blockIdx.y;
  float m[4], s[4], lse[4], cb[4], ll0[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = -INFINITY;
    s[r] = 0.f;
    ll0[r] = 0.f;
    const int64_t b = b0 + ty * 4 + r;
    const bool mult = !PASS_A && a.lik == HIPREC_VAECF_LIK_MULT && b < a.B;
    lse[r] = mult ? a.lse[b] : 0.f;
    cb[r] = mult ? a.c[b] : 0.f;
  }
  for (int64_t t = split; t < a.n_tiles; t += a.n_splits) {
    const int64_t j0 = t * kVcTile;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < H; k0 += kVcKc) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < kVcTile * kVcKc / kBlock; ++i) {
        const int e = i * kBlock + tid, r = e / kVcKc, k = e % kVcKc;
        const bool kin = k0 + k < H;
        As[r][k] = (kin && b0 + r < a.B) ? a.Hd[(b0 + r) * H + k0 + k] : 0.f;
        Bs[r][k] = (kin && j0 + r < a.I) ? a.W[(j0 + r) * H + k0 + k] : 0.f;
      }
      __syncthreads();
#pragma unroll 8
      for (int k = 0; k < kVcKc; ++k) {
        float av[4], bv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) av[r] = As[ty * 4 + r][k];
#pragma unroll
        for (int c = 0; c < 4; ++c) bv[c] = Bs[tx * 4 + c][k];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(av[r], bv[c], acc[r][c]);
      }
    }
    float bj[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t j = j0 + tx * 4 + c;
      bj[c] = j < a.I ? a.bias[j] : 0.f;
    }
    if constexpr (PASS_A) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float tm = -INFINITY;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (j0 + tx * 4 + c < a.I) tm = fmaxf(tm, acc[r][c] + bj[c]);
        if (tm > -INFINITY) {
          const float nm = fmaxf(m[r], tm);
          float ns = m[r] > -INFINITY ? s[r] * expf(m[r] - nm) : 0.f;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (j0 + tx * 4 + c < a.I) ns += expf(acc[r][c] + bj[c] - nm);
          m[r] = nm;
          s[r] = ns;
        }
      }
    } else {
      // the dense (x = 0) part of d loss / d logit, and of ll where it is not zero
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool row_in = b0 + ty * 4 + r < a.B;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float d = 0.f;
          if (row_in && j0 + tx * 4 + c < a.I) {
            const float x = acc[r][c] + bj[c];
            if (a.lik == HIPREC_VAECF_LIK_MULT) {
              d = expf(x - lse[r]) * cb[r] * a.inv_b;
            } else {
              const float p = 1.0f / (1.0f + expf(-x)), dp = p * (1.0f - p);
              if (a.lik == HIPREC_VAECF_LIK_BERN) {
                const float q = 1.0f - p + kVcEps;
                ll0[r] += logf(q);
                d = dp / q * a.inv_b;
              } else if (a.lik == HIPREC_VAECF_LIK_GAUS) {
                ll0[r] -= p * p;
                d = 2.0f * p * dp * a.inv_b;
              } else {
                ll0[r] -= p;
                d = dp * a.inv_b;
              }
            }
          }
          Dm[ty * 4 + r][tx * 4 + c] = d;
          Dt[tx * 4 + c][ty * 4 + r] = d;
        }
      }
      __syncthreads();
      if (tid < kVcTile && j0 + tid < a.I) {   // db_L
        float sum = 0.f;
        for (int r = 0; r < kVcTile; ++r) sum += Dt[tid][r];
        atomic_add_f32(a.gb + j0 + tid, sum);
      }
      const int k = tid & (kVcKc - 1), g = tid >> 5;
      for (int k0 = 0; k0 < H; k0 += kVcKc) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kVcTile * kVcKc / kBlock; ++i) {
          const int e = i * kBlock + tid, r = e / kVcKc, kk = e % kVcKc;
          const bool kin = k0 + kk < H;
          As[r][kk] = (kin && b0 + r < a.B) ? a.Hd[(b0 + r) * H + k0 + kk] : 0.f;
          Bs[r][kk] = (kin && j0 + r < a.I) ? a.W[(j0 + r) * H + k0 + kk] : 0.f;
        }
        __syncthreads();
        float accH[8] = {}, accW[8] = {};   // dHd[row i * 8 + g][k], dW_L[item i * 8 + g][k]
        for (int j4 = 0; j4 < kVcTile; j4 += 4) {
          const float w0 = Bs[j4][k], w1 = Bs[j4 + 1][k], w2 = Bs[j4 + 2][k], w3 = Bs[j4 + 3][k];
          const float h0 = As[j4][k], h1 = As[j4 + 1][k], h2 = As[j4 + 2][k], h3 = As[j4 + 3][k];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const float4 d = *reinterpret_cast<const float4*>(&Dm[i * 8 + g][j4]);
            accH[i] = fmaf(d.x, w0, fmaf(d.y, w1, fmaf(d.z, w2, fmaf(d.w, w3, accH[i]))));
            const float4 u = *reinterpret_cast<const float4*>(&Dt[i * 8 + g][j4]);
            accW[i] = fmaf(u.x, h0, fmaf(u.y, h1, fmaf(u.z, h2, fmaf(u.w, h3, accW[i]))));
          }
        }
        if (k0 + k < H) {
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int64_t row = b0 + i * 8 + g, item = j0 + i * 8 + g;
            if (row < a.B) atomic_add_f32(a.dHd + row * H + k0 + k, accH[i]);
            if (item < a.I) atomic_add_f32(a.gW + item * H + k0 + k, accW[i]);
          }
        }
      }
    }
  }
  // the block's per-row results: the 16 threads that share a row leave their parts in LDS, one thread adds them in order
  __syncthreads();
  if constexpr (PASS_A) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      Dm[ty * 4 + r][tx * 2] = m[r];
      Dm[ty * 4 + r][tx * 2 + 1] = s[r];
    }
    __syncthreads();
    if (tid < kVcTile && b0 + tid < a.B) {
      float M = -INFINITY, S = 0.f;
      for (int q = 0; q < 16; ++q) M = fmaxf(M, Dm[tid][q * 2]);
      for (int q = 0; q < 16; ++q)
        if (Dm[tid][q * 2] > -INFINITY) S += Dm[tid][q * 2 + 1] * expf(Dm[tid][q * 2] - M);
      a.parts[(split * a.B + b0 + tid) * 2] = M;
      a.parts[(split * a.B + b0 + tid) * 2 + 1] = S;
    }
  } else if (a.ll0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) Dm[ty * 4 + r][tx] = ll0[r];
    __syncthreads();
    if (tid < kVcTile && b0 + tid < a.B) {
      float sum = 0.f;
      for (int q = 0; q < 16; ++q) sum += Dm[tid][q];
      a.ll0[split * a.B + b0 + tid] = sum;
    }
  }
}

struct VcSparse {
  const int64_t *row_ptr, *items;
  const float* values;
  int64_t B, nnz, I;
  const float *Hd, *W, *bias;
  int H, lik, n_splits;
  const float* parts;
  float inv_b;
  float *lse, *c, *ll;   // [B] each
  float *dHd, *gW, *gb;
};

// One wave per row.  Per 64 nonzeros: each lane scores its own nonzero (logit, p, its part of ll_b / c_b and the
// correction `corr` of d loss / d logit at (b, i)), then the wave walks them with the lanes over the hidden columns:
// dHd[b] += corr W_L[i] (registers, stored once), dW_L[i] += corr Hd[b] and db_L[i] += corr (atomics).
__global__ __launch_bounds__(kBlock) void vc_sparse_kernel(VcSparse a, hiprec_stats* stats) {
  const int lane = lane_id();
  const int H = a.H;
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); b < a.B;
       b += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    int64_t s, e;
    vc_row_extent(a.row_ptr, b, a.nnz, lane, stats, &s, &e);
    float lse = 0.f;
    if (a.lik == HIPREC_VAECF_LIK_MULT) lse = vc_combine_lse(a.parts, a.n_splits, a.B, b);
    float hd[kVcNpl], dh[kVcNpl];
#pragma unroll
    for (int k = 0; k < kVcNpl; ++k) {
      const int h = lane + kWave * k;
      hd[k] = h < H ? a.Hd[b * H + h] : 0.f;
      dh[k] = 0.f;
    }
    float ll = 0.f, c = 0.f;
    for (int64_t base = s; base < e; base += kWave) {
      const int64_t idx = base + lane;
      const bool in = idx < e;
      long long it = in ? a.items[idx] : 0;
      const float v = in ? a.values[idx] : 0.f;
      float corr = 0.f;
      if (in && !vc_in_range(it, a.I)) {
        atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
        it = 0;
      } else if (in && v != 0.f) {
        float x = a.bias[it];
        const float* __restrict__ w = a.W + it * H;
        for (int h = 0; h < H; ++h) x = fmaf(a.Hd[b * H + h], w[h], x);
        if (a.lik == HIPREC_VAECF_LIK_MULT) {
          const float p = expf(x - lse), r = p / (p + kVcEps);
          ll += v * logf(p + kVcEps);
          c += v * r;
          corr = -v * r * a.inv_b;
        } else {
          const float p = 1.0f / (1.0f + expf(-x)), dp = p * (1.0f - p);
          if (a.lik == HIPREC_VAECF_LIK_BERN) {
            const float q = 1.0f - p + kVcEps;
            ll += v * (logf(p + kVcEps) - logf(q));
            corr = -v * dp * (1.0f / (p + kVcEps) + 1.0f / q) * a.inv_b;
          } else if (a.lik == HIPREC_VAECF_LIK_GAUS) {
            ll += v * (2.0f * p - v);
            corr = -2.0f * v * dp * a.inv_b;
          } else {
            ll += v * logf(p + kVcEps);
            corr = -v * dp / (p + kVcEps) * a.inv_b;
          }
        }
      }
      const int cnt = e - base < kWave ? static_cast<int>(e - base) : kWave;
      for (int q = 0; q < cnt; ++q) {
        const long long iq = __shfl(it, q);
        const float cq = __shfl(corr, q);
        if (cq == 0.f) continue;
#pragma unroll
        for (int k = 0; k < kVcNpl; ++k) {
          const int h = lane + kWave * k;
          if (h < H) {
            dh[k] = fmaf(cq, a.W[iq * H + h], dh[k]);
            atomic_add_f32(a.gW + iq * H + h, cq * hd[k]);
          }
        }
        if (lane == 0) atomic_add_f32(a.gb + iq, cq);
      }
    }
#pragma unroll
    for (int k = 0; k < kVcNpl; ++k) {
      const int h = lane + kWave * k;
      if (h < H) a.dHd[b * H + h] = dh[k];
    }
    ll = wave_sum(ll);
    c = wave_sum(c);
    if (lane == 0) {
      a.lse[b] = lse;
      a.c[b] = c;
      a.ll[b] = ll;
    }
  }
}

// ---- inference ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void vc_lse_kernel(const float* __restrict__ parts, int n_splits, int64_t n,
                                                        float* __restrict__ lse) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; b < n; b += stride)
    lse[b] = vc_combine_lse(parts, n_splits, n, b);
}

// out[k] = softmax / sigmoid of the decoder's last layer at (rows[k], items[k]); one wave per pair
__global__ __launch_bounds__(kBlock) void vc_pair_kernel(const float* __restrict__ Hd, int64_t n_rows,
                                                         const float* __restrict__ W, const float* __restrict__ bias,
                                                         int H, int64_t I, const int64_t* __restrict__ rows,
                                                         const int64_t* __restrict__ items, int64_t n,
                                                         const float* __restrict__ lse, float* __restrict__ out,
                                                         hiprec_stats* stats) {
  const int lane = lane_id();
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); q < n;
       q += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const int64_t r = rows[q], i = items[q];
    const bool r_ok = vc_in_range(r, n_rows), i_ok = vc_in_range(i, I);
    if (!(r_ok && i_ok)) {
      if (lane == 0) {
        atomicOr(&stats->status, (r_ok ? 0u : HIPREC_STATUS_ROW_OOB) | (i_ok ? 0u : HIPREC_STATUS_ITEM_OOB));
        out[q] = __builtin_nanf("");
      }
      continue;
    }
    float x = 0.f;
    for (int h = lane; h < H; h += kWave) x = fmaf(Hd[r * H + h], W[i * H + h], x);
    x = wave_sum(x) + bias[i];
    if (lane == 0) out[q] = lse ? expf(x - lse[r]) : 1.0f / (1.0f + expf(-x));
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
struct VcParams {   // pointers into a flat buffer laid out in state_dict() order
  int n, Z;
  int h[kVcMaxLayers];
  int dd[kVcMaxLayers + 1];   // the decoder's input widths: Z, h[n - 1], ..., h[0]
  int64_t I;
  float *we[kVcMaxLayers], *be[kVcMaxLayers], *wmu, *bmu, *wlv, *blv, *wd[kVcMaxLayers + 1], *bd[kVcMaxLayers + 1];
  int64_t floats;
};

VcParams vc_params(float* base, const hiprec_vaecf_shape& s) {
  VcParams p{};
  p.n = s.n_hidden;
  p.Z = s.z_dim;
  p.I = s.n_items;
  for (int l = 0; l < p.n; ++l) p.h[l] = s.hidden[l];
  p.dd[0] = p.Z;
  for (int l = 1; l <= p.n; ++l) p.dd[l] = p.h[p.n - l];
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += n; return r; };
  for (int l = 0; l < p.n; ++l) {
    p.we[l] = take(static_cast<int64_t>(p.h[l]) * (l == 0 ? p.I : p.h[l - 1]));
    p.be[l] = take(p.h[l]);
  }
  p.wmu = take(static_cast<int64_t>(p.Z) * p.h[p.n - 1]);
  p.bmu = take(p.Z);
  p.wlv = take(static_cast<int64_t>(p.Z) * p.h[p.n - 1]);
  p.blv = take(p.Z);
  for (int l = 0; l <= p.n; ++l) {
    const int64_t out = l < p.n ? p.dd[l + 1] : p.I;
    p.wd[l] = take(out * p.dd[l]);
    p.bd[l] = take(out);
  }
  p.floats = c - base;
  return p;
}

int vc_splits(int64_t B, int64_t I) {
  const int64_t tiles = (I + kVcTile - 1) / kVcTile, row_blocks = (B + kVcTile - 1) / kVcTile;
  const int64_t want = std::max<int64_t>(1, (1024 + row_blocks - 1) / row_blocks);
  return static_cast<int>(std::min<int64_t>({tiles, want, kVcMaxSplits}));
}

struct VcWorkspace {
  float *He[kVcMaxLayers], *Hdec[kVcMaxLayers], *ML, *Zb, *dML, *GA, *GB, *parts, *lse, *c, *ll, *ll0, *cs[2], *WT;
  int64_t floats;
};

VcWorkspace vc_carve(float* base, const hiprec_vaecf_shape& s, int64_t B) {
  VcWorkspace w{};
  const VcParams p = vc_params(nullptr, s);
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += (n + 3) / 4 * 4; return r; };
  int widest = 2 * p.Z;
  for (int l = 0; l < p.n; ++l) widest = std::max(widest, p.h[l]);
  for (int l = 0; l < p.n; ++l) {
    w.He[l] = take(B * p.h[l]);
    w.Hdec[l] = take(B * p.dd[l + 1]);
  }
  w.ML = take(B * 2 * p.Z);
  w.Zb = take(B * p.Z);
  w.dML = take(B * 2 * p.Z);
  w.GA = take(B * widest);
  w.GB = take(B * widest);
  const int splits = vc_splits(B, p.I);
  w.parts = take(2 * splits * B);
  w.lse = take(B);
  w.c = take(B);
  w.ll = take(B);
  w.ll0 = take(splits * B);
  for (int k = 0; k < 2; ++k) w.cs[k] = take(colsum_ws_floats(static_cast<int>(B), widest));
  w.WT = s.w0_shadow ? take(p.I * p.h[0]) : nullptr;
  w.floats = c - base;
  return w;
}

int vc_check_shape(const hiprec_vaecf_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  HIPREC_REQUIRE(s->n_users >= 1 && s->n_items >= 1, "VAECF needs n_users >= 1 and n_items >= 1");
  HIPREC_REQUIRE(s->z_dim >= 1 && s->z_dim <= kVcMaxZ, "VAECF needs 1 <= z_dim <= %d (got %d)", kVcMaxZ, s->z_dim);
  HIPREC_REQUIRE(s->n_hidden >= 1 && s->n_hidden <= kVcMaxLayers, "VAECF needs 1 .. %d hidden layers (got %d)",
                 kVcMaxLayers, s->n_hidden);
  for (int l = 0; l < s->n_hidden; ++l)
    HIPREC_REQUIRE(s->hidden[l] >= 1 && s->hidden[l] <= kVcMaxHidden, "VAECF needs hidden widths in 1 .. %d (got %d)",
                   kVcMaxHidden, s->hidden[l]);
  HIPREC_REQUIRE(s->act >= HIPREC_VAECF_ACT_SIGMOID && s->act <= HIPREC_VAECF_ACT_RELU6, "unknown activation %d", s->act);
  HIPREC_REQUIRE(s->likelihood >= HIPREC_VAECF_LIK_MULT && s->likelihood <= HIPREC_VAECF_LIK_POIS,
                 "unknown likelihood %d", s->likelihood);
  return 0;
}

// the grouped GEMM indexes its operands with ints: every [rows, width] operand of a step must stay below 2^31 elements
bool vc_rows_ok(int64_t rows) {
  return rows >= 1 && rows < (1ll << 24) && rows * std::max(kVcMaxHidden, 2 * kVcMaxZ) < (1ll << 31);
}

int vc_launch_act(float* a, int64_t n, int act, hipStream_t st) {
  vc_act_kernel<<<grid_for_threads(n), kBlock, 0, st>>>(a, n, act);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// out = act(X W^T + b) for one Linear layer of B rows
int vc_linear(const float* X, int in, const float* W, const float* b, float* out, int n_out, int64_t B, int act,
              hipStream_t st) {
  GemmGroup g{};
  const bool relu = act == HIPREC_VAECF_ACT_RELU;
  g.p[g.n++] = make_gemm(kNT, static_cast<int>(B), n_out, in, X, in, W, in, out, n_out, b, relu ? 1 : 0, nullptr, 0, false);
  if (int rc = launch_group(g, st)) return rc;
  return relu ? 0 : vc_launch_act(out, B * n_out, act, st);
}

struct VcBatch {
  const int64_t *row_ptr, *items;
  const float* values;
  int64_t B, nnz;
};

// stages 1 and 2 up to (mu | logvar) (n_lat = 2) or mu alone (n_lat = 1, into `lat` with the leading dimension ld_lat)
int vc_encode(const hiprec_vaecf_shape& s, const VcParams& w, const VcWorkspace& a, const VcBatch& x, float* lat,
              int ld_lat, int n_lat, hiprec_stats* stats, hipStream_t st) {
  const int H0 = w.h[0], n = w.n, Z = w.Z;
  const int R = static_cast<int>(x.B);
  if (s.w0_shadow) {
    const int64_t tiles = ((w.I + 31) / 32) * ((H0 + 31) / 32);
    vc_transpose_kernel<<<static_cast<int>(std::min<int64_t>(tiles, kMaxBlocks)), kBlock, 0, st>>>(w.we[0], H0, w.I, a.WT);
    HIPREC_TRY(hipGetLastError());
  }
  vc_first_kernel<<<grid_for_waves(x.B), kBlock, 0, st>>>(x.row_ptr, x.items, x.values, x.B, x.nnz,
                                                          s.w0_shadow ? a.WT : w.we[0], s.w0_shadow ? 1 : w.I,
                                                          s.w0_shadow ? H0 : 1, w.be[0], H0, w.I, s.act, a.He[0], stats);
  HIPREC_TRY(hipGetLastError());
  for (int l = 1; l < n; ++l)
    if (int rc = vc_linear(a.He[l - 1], w.h[l - 1], w.we[l], w.be[l], a.He[l], w.h[l], x.B, s.act, st)) return rc;
  const int hl = w.h[n - 1];
  GemmGroup g{};
  g.p[g.n++] = make_gemm(kNT, R, Z, hl, a.He[n - 1], hl, w.wmu, hl, lat, ld_lat, w.bmu, 0, nullptr, 0, false);
  if (n_lat == 2)
    g.p[g.n++] = make_gemm(kNT, R, Z, hl, a.He[n - 1], hl, w.wlv, hl, lat + Z, ld_lat, w.blv, 0, nullptr, 0, false);
  return launch_group(g, st);
}

// the decoder up to its last hidden activation: z [B, Z] -> Hd [B, h_0] (`out`, or the workspace's when NULL)
int vc_decode_hidden(const hiprec_vaecf_shape& s, const VcParams& w, const VcWorkspace& a, const float* z, int64_t B,
                     float* out, hipStream_t st) {
  const float* X = z;
  for (int l = 0; l < w.n; ++l) {
    float* Y = (l == w.n - 1 && out) ? out : a.Hdec[l];
    if (int rc = vc_linear(X, w.dd[l], w.wd[l], w.bd[l], Y, w.dd[l + 1], B, s.act, st)) return rc;
    X = Y;
  }
  return 0;
}

template <bool PASS_A>
int vc_launch_dense(const VcDense& d, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>((d.B + kVcTile - 1) / kVcTile), static_cast<unsigned>(d.n_splits));
  vc_dense_kernel<PASS_A><<<grid, kBlock, 0, st>>>(d);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

int vc_train(const hiprec_vaecf_shape& s, float* w_flat, float* g_flat, const VcBatch& x, const float* noise, float beta,
             hiprec_stats* stats, Scratch* scratch, float* ws_base, hipStream_t st) {
  const VcParams w = vc_params(w_flat, s), g = vc_params(g_flat, s);
  const VcWorkspace a = vc_carve(ws_base, s, x.B);
  const int n = w.n, Z = w.Z, H0 = w.h[0], R = static_cast<int>(x.B);
  const int64_t B = x.B;
  const bool mult = s.likelihood == HIPREC_VAECF_LIK_MULT;
  const float inv_b = 1.0f / static_cast<float>(B);

  if (int rc = vc_encode(s, w, a, x, a.ML, 2 * Z, 2, stats, st)) return rc;
  vc_reparam_kernel<<<grid_for_threads(B * Z), kBlock, 0, st>>>(a.ML, noise, B, Z, a.Zb);
  HIPREC_TRY(hipGetLastError());
  if (int rc = vc_decode_hidden(s, w, a, a.Zb, B, nullptr, st)) return rc;
  const float* Hd = a.Hdec[n - 1];

  // the fused last layer: dHd lands in GA
  VcDense d{};
  d.Hd = Hd; d.W = w.wd[n]; d.bias = w.bd[n];
  d.H = H0; d.lik = s.likelihood; d.n_splits = vc_splits(B, w.I);
  d.B = B; d.I = w.I; d.n_tiles = (w.I + kVcTile - 1) / kVcTile;
  d.parts = a.parts; d.lse = a.lse; d.c = a.c; d.inv_b = inv_b;
  d.ll0 = mult ? nullptr : a.ll0;
  d.dHd = a.GA; d.gW = g.wd[n]; d.gb = g.bd[n];
  if (mult)
    if (int rc = vc_launch_dense<true>(d, st)) return rc;
  VcSparse sp{};
  sp.row_ptr = x.row_ptr; sp.items = x.items; sp.values = x.values;
  sp.B = B; sp.nnz = x.nnz; sp.I = w.I;
  sp.Hd = Hd; sp.W = w.wd[n]; sp.bias = w.bd[n];
  sp.H = H0; sp.lik = s.likelihood; sp.n_splits = d.n_splits;
  sp.parts = a.parts; sp.inv_b = inv_b;
  sp.lse = a.lse; sp.c = a.c; sp.ll = a.ll;
  sp.dHd = a.GA; sp.gW = g.wd[n]; sp.gb = g.bd[n];
  vc_sparse_kernel<<<grid_for_waves(B), kBlock, 0, st>>>(sp, stats);
  HIPREC_TRY(hipGetLastError());
  if (int rc = vc_launch_dense<false>(d, st)) return rc;

  // the decoder's hidden layers, last to first: GA holds d loss / d (the layer's activation)
  float *GA = a.GA, *GB = a.GB;
  for (int l = n - 1; l >= 0; --l) {
    const int out = w.dd[l + 1], in = w.dd[l];
    const float* X = l == 0 ? a.Zb : a.Hdec[l - 1];
    vc_act_bwd_kernel<<<grid_for_threads(B * out), kBlock, 0, st>>>(GA, nullptr, a.Hdec[l], B * out, s.act);
    HIPREC_TRY(hipGetLastError());
    GemmGroup q{};
    q.p[q.n++] = make_gemm(kTNm, out, in, R, GA, out, X, in, g.wd[l], in, nullptr, 0, nullptr, 0, true);
    q.p[q.n++] = make_colsum(GA, R, out, out, g.bd[l], a.cs[0]);
    q.p[q.n++] = make_gemm(kNN, R, in, out, GA, out, w.wd[l], in, GB, in, nullptr, 0, nullptr, 0, false);
    if (int rc = launch_group(q, st)) return rc;
    if (int rc = launch_colsum_reduce(q, st)) return rc;
    std::swap(GA, GB);
  }
  // GA = dz
  vc_latent_kernel<<<grid_for_waves(B), kBlock, 0, st>>>(a.ML, noise, GA, B, Z, beta * inv_b, inv_b, a.ll,
                                                         mult ? nullptr : a.ll0, d.n_splits, a.dML, stats, scratch);
  HIPREC_TRY(hipGetLastError());
  {
    const int hl = w.h[n - 1];
    GemmGroup q{};
    q.p[q.n++] = make_gemm(kTNm, Z, hl, R, a.dML, 2 * Z, a.He[n - 1], hl, g.wmu, hl, nullptr, 0, nullptr, 0, true);
    q.p[q.n++] = make_gemm(kTNm, Z, hl, R, a.dML + Z, 2 * Z, a.He[n - 1], hl, g.wlv, hl, nullptr, 0, nullptr, 0, true);
    q.p[q.n++] = make_colsum(a.dML, R, Z, 2 * Z, g.bmu, a.cs[0]);
    q.p[q.n++] = make_colsum(a.dML + Z, R, Z, 2 * Z, g.blv, a.cs[1]);
    q.p[q.n++] = make_gemm(kNN, R, hl, Z, a.dML, 2 * Z, w.wmu, hl, GA, hl, nullptr, 0, nullptr, 0, false);
    q.p[q.n++] = make_gemm(kNN, R, hl, Z, a.dML + Z, 2 * Z, w.wlv, hl, GB, hl, nullptr, 0, nullptr, 0, false);
    if (int rc = launch_group(q, st)) return rc;
    if (int rc = launch_colsum_reduce(q, st)) return rc;
  }
  // the encoder: d loss / d He[n - 1] = GA + GB
  const float* add = GB;
  for (int l = n - 1; l >= 1; --l) {
    const int out = w.h[l], in = w.h[l - 1];
    vc_act_bwd_kernel<<<grid_for_threads(B * out), kBlock, 0, st>>>(GA, add, a.He[l], B * out, s.act);
    HIPREC_TRY(hipGetLastError());
    GemmGroup q{};
    q.p[q.n++] = make_gemm(kTNm, out, in, R, GA, out, a.He[l - 1], in, g.we[l], in, nullptr, 0, nullptr, 0, true);
    q.p[q.n++] = make_colsum(GA, R, out, out, g.be[l], a.cs[0]);
    q.p[q.n++] = make_gemm(kNN, R, in, out, GA, out, w.we[l], in, GB, in, nullptr, 0, nullptr, 0, false);
    if (int rc = launch_group(q, st)) return rc;
    if (int rc = launch_colsum_reduce(q, st)) return rc;
    std::swap(GA, GB);
    add = nullptr;
  }
  vc_first_bwd_kernel<<<grid_for_waves(B), kBlock, 0, st>>>(x.row_ptr, x.items, x.values, B, x.nnz, GA, add, a.He[0], H0,
                                                            w.I, s.act, g.we[0]);
  HIPREC_TRY(hipGetLastError());
  GemmGroup q{};
  q.p[q.n++] = make_colsum(GA, R, H0, H0, g.be[0], a.cs[0]);
  if (int rc = launch_group(q, st)) return rc;
  return launch_colsum_reduce(q, st);
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_vaecf_shape_bytes(void) { return sizeof(hiprec_vaecf_shape); }

extern "C" int64_t hiprec_vaecf_param_floats(const hiprec_vaecf_shape* shape) {
  if (vc_check_shape(shape)) return -1;
  return vc_params(nullptr, *shape).floats;
}

extern "C" size_t hiprec_vaecf_workspace_bytes(const hiprec_vaecf_shape* shape, int64_t batch, int64_t nnz) {
  if (vc_check_shape(shape)) return 0;
  if (nnz < 0 || !vc_rows_ok(batch)) {
    set_error("a VAECF step of %lld rows is beyond the grouped GEMM's 2^31 elements per operand",
              static_cast<long long>(batch));
    return 0;
  }
  return sizeof(float) * static_cast<size_t>(vc_carve(nullptr, *shape, batch).floats);
}

extern "C" size_t hiprec_vaecf_encode_workspace_bytes(const hiprec_vaecf_shape* shape, int64_t n_rows) {
  if (vc_check_shape(shape) || n_rows < 1) return 0;
  return sizeof(float) * static_cast<size_t>(vc_carve(nullptr, *shape, std::min<int64_t>(n_rows, kVcChunk)).floats);
}

extern "C" size_t hiprec_vaecf_decode_workspace_bytes(const hiprec_vaecf_shape* shape, int64_t n_rows) {
  if (vc_check_shape(shape) || n_rows < 1) return 0;
  return sizeof(float) * static_cast<size_t>((2 * vc_splits(n_rows, shape->n_items) + 1) * n_rows);
}

extern "C" int hiprec_vaecf_grad(const hiprec_vaecf_shape* shape, const float* w_flat, float* g_flat,
                                 const int64_t* row_ptr, const int64_t* items, const float* values, int64_t batch,
                                 int64_t nnz, const float* noise, float beta, hiprec_stats* stats, void* scratch,
                                 size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = vc_check_shape(shape)) return rc;
  HIPREC_REQUIRE(w_flat && g_flat && row_ptr && noise && stats && scratch && workspace, "NULL pointer");
  HIPREC_REQUIRE(batch >= 1 && nnz >= 0, "bad batch / nnz");
  HIPREC_REQUIRE(nnz == 0 || (items && values), "NULL items / values");
  if (scratch_bytes < kScratchBytes) {
    set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
    return HIPREC_E_SCRATCH;
  }
  const size_t need = hiprec_vaecf_workspace_bytes(shape, batch, nnz);
  HIPREC_REQUIRE(need > 0, "unsupported batch %lld", static_cast<long long>(batch));
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  const VcBatch x{row_ptr, items, values, batch, nnz};
  return vc_train(*shape, const_cast<float*>(w_flat), g_flat, x, noise, beta, stats, static_cast<Scratch*>(scratch),
                  static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_vaecf_encode(const hiprec_vaecf_shape* shape, const float* w_flat, const int64_t* row_ptr,
                                   const int64_t* items, const float* values, int64_t n_rows, int64_t nnz, float* mu,
                                   float* hd, hiprec_stats* stats, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  if (int rc = vc_check_shape(shape)) return rc;
  HIPREC_REQUIRE(n_rows >= 0 && nnz >= 0, "bad n_rows / nnz");
  if (n_rows == 0) return 0;
  HIPREC_REQUIRE(w_flat && row_ptr && mu && hd && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(nnz == 0 || (items && values), "NULL items / values");
  const size_t need = hiprec_vaecf_encode_workspace_bytes(shape, n_rows);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const VcParams w = vc_params(const_cast<float*>(w_flat), *shape);
  const VcWorkspace a = vc_carve(static_cast<float*>(workspace), *shape, std::min<int64_t>(n_rows, kVcChunk));
  for (int64_t off = 0; off < n_rows; off += kVcChunk) {
    const int64_t m = std::min<int64_t>(n_rows - off, kVcChunk);
    const VcBatch x{row_ptr + off, items, values, m, nnz};
    float* mu_c = mu + off * w.Z;
    if (int rc = vc_encode(*shape, w, a, x, mu_c, w.Z, 1, stats, st)) return rc;
    if (int rc = vc_decode_hidden(*shape, w, a, mu_c, m, hd + off * w.h[0], st)) return rc;
  }
  return 0;
}

extern "C" int hiprec_vaecf_decode_at(const hiprec_vaecf_shape* shape, const float* w_flat, const float* hd,
                                      int64_t n_rows, const int64_t* rows, const int64_t* items, int64_t n, float* out,
                                      float* lse_out, hiprec_stats* stats, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  if (int rc = vc_check_shape(shape)) return rc;
  HIPREC_REQUIRE(n_rows >= 1 && n >= 0, "bad n_rows / n");
  HIPREC_REQUIRE(w_flat && hd && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(n == 0 || (rows && items && out), "NULL pair arrays");
  HIPREC_REQUIRE(vc_rows_ok(n_rows), "too many rows for one pass");
  const size_t need = hiprec_vaecf_decode_workspace_bytes(shape, n_rows);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const VcParams w = vc_params(const_cast<float*>(w_flat), *shape);
  float* lse = nullptr;
  if (shape->likelihood == HIPREC_VAECF_LIK_MULT) {
    VcDense d{};
    d.Hd = hd; d.W = w.wd[w.n]; d.bias = w.bd[w.n];
    d.H = w.h[0]; d.lik = shape->likelihood; d.n_splits = vc_splits(n_rows, w.I);
    d.B = n_rows; d.I = w.I; d.n_tiles = (w.I + kVcTile - 1) / kVcTile;
    d.parts = static_cast<float*>(workspace);
    lse = d.parts + 2 * static_cast<int64_t>(d.n_splits) * n_rows;
    if (int rc = vc_launch_dense<true>(d, st)) return rc;
    vc_lse_kernel<<<grid_for_threads(n_rows), kBlock, 0, st>>>(d.parts, d.n_splits, n_rows, lse);
    HIPREC_TRY(hipGetLastError());
    if (lse_out) HIPREC_TRY(hipMemcpyAsync(lse_out, lse, sizeof(float) * n_rows, hipMemcpyDeviceToDevice, st));
  }
  if (n == 0) return 0;
  vc_pair_kernel<<<grid_for_waves(n), kBlock, 0, st>>>(hd, n_rows, w.wd[w.n], w.bd[w.n], w.h[0], w.I, rows, items, n, lse,
                                                       out, stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}
