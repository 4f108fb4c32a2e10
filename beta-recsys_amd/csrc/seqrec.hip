// The stages SASRec (csrc/sasrec.hip) and TiSASRec (csrc/tisasrec.hip) have in common, once: the kernels of the norm /
// count prep, the embed, LayerNorm forward and backward and the BCE loss, their launchers, the feed-forward GEMM groups
// and the argument checks of the two C entry points (declared in seqrec.hpp).  Activations are [M = B * T, D] row-major.
#include "seqrec.hpp"

#include "gemm.hpp"

namespace hiprec {
namespace {

// ---- prep: count(pos != 0) and the first level of sum(W^2) ------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void seq_prep_kernel(const float* __restrict__ W, int64_t n_w,
                                                          const int64_t* __restrict__ pos, int64_t M, int with_norm,
                                                          float* __restrict__ aux) {
  __shared__ float s_red[kBlock];
  float s = 0.f;
  if (with_norm) {
    const int64_t per = (n_w + kSeqNormParts - 1) / kSeqNormParts;
    const int64_t lo = per * blockIdx.x, hi = min(n_w, lo + per);
    for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) s += W[i] * W[i];
  }
  s_red[threadIdx.x] = s;
  __syncthreads();
  for (int r = kBlock / 2; r > 0; r >>= 1) {
    if (static_cast<int>(threadIdx.x) < r) s_red[threadIdx.x] += s_red[threadIdx.x + r];
    __syncthreads();
  }
  if (threadIdx.x == 0) aux[2 + blockIdx.x] = s_red[0];
  if (blockIdx.x != 0) return;
  __syncthreads();
  float c = 0.f;                                   // integers up to 2^24 are exact in fp32; M < 2^24 is required
  for (int64_t m = threadIdx.x; m < M; m += kBlock) c += pos[m] != 0 ? 1.f : 0.f;
  s_red[threadIdx.x] = c;
  __syncthreads();
  for (int r = kBlock / 2; r > 0; r >>= 1) {
    if (static_cast<int>(threadIdx.x) < r) s_red[threadIdx.x] += s_red[threadIdx.x + r];
    __syncthreads();
  }
  if (threadIdx.x == 0) aux[0] = s_red[0];
}

// second level, in a fixed order; g += l2 * W / ||W|| (0 where ||W|| == 0, as torch.norm's backward gives)
__global__ __launch_bounds__(kBlock) void seq_norm_grad_kernel(const float* __restrict__ W, float* __restrict__ g,
                                                               int64_t n_w, float l2, float* __restrict__ aux) {
  __shared__ float s_red[kBlock];
  s_red[threadIdx.x] = aux[2 + threadIdx.x];
  __syncthreads();
  for (int r = kBlock / 2; r > 0; r >>= 1) {
    if (static_cast<int>(threadIdx.x) < r) s_red[threadIdx.x] += s_red[threadIdx.x + r];
    __syncthreads();
  }
  const float norm = sqrtf(s_red[0]);
  const float coef = norm > 0.f ? l2 / norm : 0.f;
  if (blockIdx.x == 0 && threadIdx.x == 0) aux[1] = norm;
  if (g == nullptr) return;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n_w; i += stride) g[i] += coef * W[i];
}

// ---- embed: x0 = (E[seq] * sqrt(D) + P[t]) * keep * (seq != 0); P == NULL: no positional row -------------------------
__global__ __launch_bounds__(kBlock) void seq_embed_kernel(const float* __restrict__ E, const float* __restrict__ P,
                                                           const int64_t* __restrict__ seq, int64_t M, int T, int D,
                                                           int64_t n_items, float sqrt_d,
                                                           const uint8_t* __restrict__ keep, float ks,
                                                           float* __restrict__ x, hiprec_stats* stats) {
  const int64_t n = M * D, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t m = i / D;
    const int d = static_cast<int>(i - m * D);
    const int64_t id = seq[m];
    float v = 0.f;
    if (id < 0 || id > n_items) {
      if (d == 0) atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
    } else if (id != 0) {
      const float e = E[id * D + d];       // with P: one fused multiply-add, never a product rounded before the sum
      v = P ? fmaf(e, sqrt_d, P[static_cast<int64_t>(m % T) * D + d]) : e * sqrt_d;
      if (keep) v = keep[i] ? v * ks : 0.f;
    }
    x[i] = v;
  }
}

// ---- LayerNorm (eps 1e-8, biased variance), one wave per row, D <= 128 -----------------------------------------------
// x = (a + b) * (seq != 0); xsum (optional) receives x; y = (x - mean) * rstd * gamma + beta
__global__ __launch_bounds__(kBlock) void seq_ln_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            const int64_t* __restrict__ seq, float* __restrict__ xsum,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ y,
                                                            float* __restrict__ mean, float* __restrict__ rstd,
                                                            int64_t M, int D) {
  const int lane = lane_id();
  const float inv_d = 1.f / static_cast<float>(D);
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); row < M;
       row += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const bool live = !seq || seq[row] != 0;
    float v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      float t = 0.f;
      if (d < D && live) {
        t = a[row * D + d];
        if (b) t += b[row * D + d];
      }
      v[h] = t;
      if (xsum && d < D) xsum[row * D + d] = t;
    }
    const float mu = wave_sum(v[0] + v[1]) * inv_d;
    const float c0 = lane < D ? v[0] - mu : 0.f, c1 = lane + 64 < D ? v[1] - mu : 0.f;
    const float var = wave_sum(c0 * c0 + c1 * c1) * inv_d;
    const float r = 1.0f / sqrtf(var + 1e-8f);
    if (lane < D) y[row * D + lane] = c0 * r * gamma[lane] + beta[lane];
    if (lane + 64 < D) y[row * D + lane + 64] = c1 * r * gamma[lane + 64] + beta[lane + 64];
    if (lane == 0) {
      mean[row] = mu;
      rstd[row] = r;
    }
  }
}

// dy = dy_a + dy_b; x = a + b; dx = (rstd * (g - mean(g) - xhat * mean(g * xhat)) + dx_extra + dx_extra2) * (seq != 0) with
// g = dy * gamma; dx_keep (optional) = dx through the keep bytes; dyx = dy * xhat and dyt = dy feed the column sums
__global__ __launch_bounds__(kBlock) void seq_ln_bwd_kernel(
    const float* __restrict__ dy_a, const float* __restrict__ dy_b, const float* __restrict__ a,
    const float* __restrict__ b, const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ dx_extra, const float* __restrict__ dx_extra2,
    const int64_t* __restrict__ seq, const uint8_t* __restrict__ keep, float ks, float* __restrict__ dx,
    float* __restrict__ dx_keep, float* __restrict__ dyx, float* __restrict__ dyt, int64_t M, int D) {
  const int lane = lane_id();
  const float inv_d = 1.f / static_cast<float>(D);
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); row < M;
       row += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const bool live = !seq || seq[row] != 0;
    const float mu = mean[row], r = rstd[row];
    float xh[2], gg[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      xh[h] = 0.f;
      gg[h] = 0.f;
      if (d < D) {
        const int64_t i = row * D + d;
        float x = a[i];
        if (b) x += b[i];
        float dy = dy_a[i];
        if (dy_b) dy += dy_b[i];
        xh[h] = (x - mu) * r;
        gg[h] = dy * gamma[d];
        dyx[i] = dy * xh[h];
        if (dyt) dyt[i] = dy;
      }
    }
    const float m1 = wave_sum(gg[0] + gg[1]) * inv_d;
    const float m2 = wave_sum(gg[0] * xh[0] + gg[1] * xh[1]) * inv_d;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      if (d < D) {
        const int64_t i = row * D + d;
        float v = r * (gg[h] - m1 - xh[h] * m2);
        if (dx_extra) v += dx_extra[i];
        if (dx_extra2) v += dx_extra2[i];
        if (!live) v = 0.f;
        dx[i] = v;
        if (dx_keep) dx_keep[i] = keep[i] ? v * ks : 0.f;
      }
    }
  }
}

// ---- loss: BCE-with-logits over the tokens with pos != 0, d feats, row atomics into d item_emb -----------------------
__global__ __launch_bounds__(kBlock) void seq_loss_kernel(const float* __restrict__ feats, const float* __restrict__ E,
                                                          const int64_t* __restrict__ pos,
                                                          const int64_t* __restrict__ neg, int64_t M, int D,
                                                          int64_t n_items, const float* __restrict__ aux, float l2,
                                                          float* __restrict__ dfeats, float* __restrict__ g_item,
                                                          Scratch* scratch, hiprec_stats* stats) {
  __shared__ float s_loss[kWavesPerBlock];
  const int lane = lane_id(), wave = wave_in_block();
  const float inv = 1.0f / aux[0];
  float loss = 0.f;
  for (int64_t m = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave; m < M;
       m += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const int64_t p = pos[m], n = neg[m];
    const bool ok = p >= 0 && p <= n_items && n >= 0 && n <= n_items;
    if (!ok && lane == 0) atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
    if (!ok || p == 0) {
      if (lane < D) dfeats[m * D + lane] = 0.f;
      if (lane + 64 < D) dfeats[m * D + lane + 64] = 0.f;
      continue;
    }
    float f[2], ep[2], en[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      f[h] = d < D ? feats[m * D + d] : 0.f;
      ep[h] = d < D ? E[p * D + d] : 0.f;
      en[h] = d < D ? E[n * D + d] : 0.f;
    }
    const float pl = wave_sum(f[0] * ep[0] + f[1] * ep[1]);
    const float nl = wave_sum(f[0] * en[0] + f[1] * en[1]);
    float sig_neg_pl, sig_nl;
    loss += neg_logsigmoid(pl, &sig_neg_pl);      // BCEWithLogits(x, 1) = softplus(-x)
    loss += neg_logsigmoid(-nl, &sig_nl);         // BCEWithLogits(x, 0) = softplus(x)
    const float dpl = -sig_neg_pl * inv, dnl = sig_nl * inv;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      if (d < D) {
        dfeats[m * D + d] = dpl * ep[h] + dnl * en[h];
        atomic_add_f32(g_item + p * D + d, dpl * f[h]);
        if (n != 0) atomic_add_f32(g_item + n * D + d, dnl * f[h]);
      }
    }
  }
  if (lane == 0) s_loss[wave] = loss;
  lds_barrier();
  if (threadIdx.x == 0) {
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < kWavesPerBlock; ++i) l += s_loss[i];
    l *= inv;
    if (blockIdx.x == 0) {
      if (l2 != 0.f) l += l2 * aux[1];
      scratch->n_partials = gridDim.x;
      advance_step(stats);
    }
    scratch->partials[blockIdx.x] = make_float4(l, 0.f, 0.f, 0.f);
  }
}

}  // namespace

// ---- host side --------------------------------------------------------------------------------------------------------
int seq_check_shape(const char* model, int64_t n_items, int n_blocks, int heads, int maxlen, int dim) {
  HIPREC_REQUIRE(n_items > 0 && n_blocks >= 1 && heads >= 1 && maxlen >= 1, "bad %s shape", model);
  HIPREC_REQUIRE(dim <= kSeqMaxDim && dim % heads == 0, "%s needs emb_dim <= %d and a multiple of num_heads", model,
                 kSeqMaxDim);
  const int hd = dim / heads;
  HIPREC_REQUIRE(hd == 16 || hd == 32 || hd == 64, "%s needs a head width of 16, 32 or 64 (got %d)", model, hd);
  HIPREC_REQUIRE(maxlen <= kSeqMaxLen, "%s needs maxlen <= %d (got %d)", model, kSeqMaxLen, maxlen);
  return 0;
}

int seq_check_call(const void* w_flat, const void* g_flat, const void* seq, const void* pos, const void* neg,
                   int64_t batch, int seq_len, int maxlen, int heads, const void* feats_out, const void* stats,
                   const void* scratch, size_t scratch_bytes, const void* workspace, size_t workspace_bytes,
                   size_t need) {
  HIPREC_REQUIRE(w_flat && seq && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(batch >= 1 && seq_len >= 1 && seq_len <= maxlen, "bad batch / sequence length (maxlen %d)", maxlen);
  HIPREC_REQUIRE(batch * seq_len < (1ll << 24), "batch x sequence length must stay below 2^24");
  HIPREC_REQUIRE(batch * heads <= 65535ll * 1024, "batch too large");
  if (g_flat) {
    HIPREC_REQUIRE(pos && neg && scratch, "training needs pos, neg and the scratch block");
    if (scratch_bytes < kScratchBytes) {
      set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
      return HIPREC_E_SCRATCH;
    }
  } else {
    HIPREC_REQUIRE(feats_out, "forward only needs a feature buffer");
  }
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  return 0;
}

int seq_prep(const float* W, float* g, int64_t n_w, const int64_t* pos, int64_t M, float l2, float* aux,
             hipStream_t st) {
  seq_prep_kernel<<<kSeqNormParts, kBlock, 0, st>>>(W, n_w, pos, M, l2 != 0.f, aux);
  HIPREC_TRY(hipGetLastError());
  if (l2 != 0.f) {
    seq_norm_grad_kernel<<<grid_for_threads(n_w), kBlock, 0, st>>>(W, g, n_w, l2, aux);
    HIPREC_TRY(hipGetLastError());
  }
  return 0;
}

int seq_embed(const float* E, const float* P, const int64_t* seq, int64_t M, int T, int D, int64_t n_items,
              float sqrt_d, const uint8_t* keep, float ks, float* x, hiprec_stats* stats, hipStream_t st) {
  seq_embed_kernel<<<grid_for_threads(M * D), kBlock, 0, st>>>(E, P, seq, M, T, D, n_items, sqrt_d, keep, ks, x, stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

int seq_ln_fwd(const float* a, const float* b, const int64_t* seq, float* xsum, const float* gamma, const float* beta,
               float* y, float* mean, float* rstd, int64_t M, int D, hipStream_t st) {
  seq_ln_fwd_kernel<<<grid_for_waves(M), kBlock, 0, st>>>(a, b, seq, xsum, gamma, beta, y, mean, rstd, M, D);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

int seq_ln_bwd(const float* dy_a, const float* dy_b, const float* a, const float* b, const float* gamma,
               const float* mean, const float* rstd, const float* dx_extra, const float* dx_extra2, const int64_t* seq,
               const uint8_t* keep, float ks, float* dx, float* dx_keep, float* dyx, float* dyt, float* g_gamma,
               float* g_beta, float* cs, int64_t M, int D, hipStream_t st) {
  seq_ln_bwd_kernel<<<grid_for_waves(M), kBlock, 0, st>>>(dy_a, dy_b, a, b, gamma, mean, rstd, dx_extra, dx_extra2, seq,
                                                           keep, ks, dx, keep ? dx_keep : nullptr, dyx,
                                                           dy_b ? dyt : nullptr, M, D);
  HIPREC_TRY(hipGetLastError());
  GemmGroup g{};
  g.n = 2;
  g.p[0] = make_colsum(dyx, static_cast<int>(M), D, D, g_gamma, cs);
  g.p[1] = make_colsum(dy_b ? dyt : dy_a, static_cast<int>(M), D, D, g_beta, cs + colsum_ws_floats(static_cast<int>(M), D));
  if (int rc = launch_group(g, st)) return rc;
  return launch_colsum_reduce(g, st);
}

static void set_keep(GemmProblem& p, const uint8_t* keep, int D, float ks) {
  if (keep) { p.keep = keep; p.ldk = D; p.keep_scale = ks; }
}

int seq_ffn_fwd(int M, int D, const float* f, const float* c1_w, const float* c1_b, const float* c2_w,
                const float* c2_b, const uint8_t* keep1, const uint8_t* keep2, float ks, float* h1, float* z,
                hipStream_t st) {
  GemmGroup g{};
  g.n = 1;
  g.p[0] = make_gemm(kNT, M, D, D, f, D, c1_w, D, h1, D, c1_b, 1, nullptr, 0, false);
  set_keep(g.p[0], keep1, D, ks);
  if (int rc = launch_group(g, st)) return rc;
  g = GemmGroup{};
  g.n = 1;
  g.p[0] = make_gemm(kNT, M, D, D, h1, D, c2_w, D, z, D, c2_b, 0, nullptr, 0, false);
  set_keep(g.p[0], keep2, D, ks);
  return launch_group(g, st);
}

int seq_ffn_bwd(int M, int D, const float* dz, const float* f, const float* h1, const float* c1_w, const float* c2_w,
                const uint8_t* keep1, float ks, float* dh, float* df, float* g_c1_w, float* g_c1_b, float* g_c2_w,
                float* g_c2_b, float* cs, hipStream_t st) {
  GemmGroup q{};
  q.n = 3;
  q.p[0] = make_gemm(kNN, M, D, D, dz, D, c2_w, D, dh, D, nullptr, 0, h1, D, false);
  set_keep(q.p[0], keep1, D, ks);
  q.p[1] = make_gemm(kTNm, D, D, M, dz, D, h1, D, g_c2_w, D, nullptr, 0, nullptr, 0, true);
  q.p[2] = make_colsum(dz, M, D, D, g_c2_b, cs);
  if (int rc = launch_group(q, st)) return rc;
  if (int rc = launch_colsum_reduce(q, st)) return rc;
  q = GemmGroup{};
  q.n = 3;
  q.p[0] = make_gemm(kNN, M, D, D, dh, D, c1_w, D, df, D, nullptr, 0, nullptr, 0, false);
  q.p[1] = make_gemm(kTNm, D, D, M, dh, D, f, D, g_c1_w, D, nullptr, 0, nullptr, 0, true);
  q.p[2] = make_colsum(dh, M, D, D, g_c1_b, cs);
  if (int rc = launch_group(q, st)) return rc;
  return launch_colsum_reduce(q, st);
}

int seq_loss(const float* feats, const float* E, const int64_t* pos, const int64_t* neg, int64_t M, int D,
             int64_t n_items, const float* aux, float l2, float* dfeats, float* g_item, Scratch* scratch,
             hiprec_stats* stats, hipStream_t st) {
  seq_loss_kernel<<<grid_for_waves(M), kBlock, 0, st>>>(feats, E, pos, neg, M, D, n_items, aux, l2, dfeats, g_item,
                                                        scratch, stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

}  // namespace hiprec
