// UltraGCN: two embedding tables trained with a weighted BCE over one positive and N sampled negatives
// per sample plus an item-item constraint over K precomputed neighbours -- no propagation at all.
//
//   beta_rec/models/ultragcn.py:72-100    get_omegas: wp = w1 + w2 bu[u] bi[p], wn = w3 + w4 bu[u] bi[n] (w3 when w4 <= 0)
//   beta_rec/models/ultragcn.py:102-134   cal_loss_L: sum_b [ wp bce(s(u,p), 1) + negative_weight mean_n(wn bce(s(u,n), 0)) ]
//   beta_rec/models/ultragcn.py:136-151   cal_loss_I: sum_b sum_k -sim[p,k] log sigmoid(s(u, nbr[p,k]))
//   beta_rec/models/ultragcn.py:153-157   norm_loss: (||U||^2 + ||V||^2) / 2 over EVERY row, every step
//   beta_rec/models/ultragcn.py:159-165   forward: L + gamma norm_loss + lambda I;   s(u,i) = <U[u], V[i]>
//   beta_rec/models/ultragcn.py:167-179   predict: the plain dot product
//
// Layout in HBM: one flat fp32 buffer [user_embeds U*D | item_embeds I*D] for the weights and one of the same shape for
// the dense gradient.  The step is
//   ug_grad_kernel              one BLOCK per sample: the user row sits in the registers of all four waves, which share
//                               the sample's 1 + N + K item terms (four rows in flight per wave); an item row's gradient
//                               is one 256-B atomic wave-instruction per 64 columns; the user row's gradient -- the sum
//                               over all terms -- is added up in registers, across the waves in LDS, and leaves the block
//                               once.  Block 0 also folds the per-block sums of w^2 that the previous sweep (or
//                               hiprec_sumsq) left into the loss value of the gamma term.
//   opt_dense_decay_kernel      the optimizer sweep (optim.hip's arithmetic) with gamma * w added to the gradient on the
//                               fly and the per-block sums of the NEW w^2 emitted for the next step's loss
// Atomic-rate bound: the step adds B (2 + N + K) 4D bytes by float atomics.
#include "common.hpp"

namespace hiprec {

constexpr int kUgMaxNpl = 4;   // dim <= 256: columns lane, lane+64, ...
constexpr int kUgUnroll = 4;   // item rows in flight per wave

__device__ __forceinline__ bool ug_in_range(int64_t i, int64_t n) {
  return static_cast<uint64_t>(i) < static_cast<uint64_t>(n);
}

template <int NPL>
__global__ __launch_bounds__(kBlock) void ug_grad_kernel(
    hiprec_ultragcn_tables w, hiprec_ultragcn_tables g, hiprec_ultragcn_params p,
    const int64_t* __restrict__ users, const int64_t* __restrict__ pos, const int64_t* __restrict__ neg,
    int64_t batch, int n_neg, const double* __restrict__ sumsq_ws, hiprec_stats* stats, Scratch* scratch) {
  __shared__ float s_gu[kWavesPerBlock][NPL * kWave];
  __shared__ double s_sq[kBlock];
  const int lane = lane_id();
  const int wv = wave_in_block();
  const int D = w.dim;

  const bool stepper = blockIdx.x == 0 && threadIdx.x == 0;
  StepState step_state{};
  if (stepper) step_state = step_load(stats);

  const int K = (p.lambda_ != 0.f && p.ii_neighbor != nullptr) ? p.n_neighbors : 0;
  const int n_terms = 1 + n_neg + K;
  const float neg_scale = p.negative_weight / static_cast<float>(n_neg);

  float loss_acc = 0.f;
  for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
    const int64_t u = users[b], pi = pos[b];
    const bool u_ok = ug_in_range(u, w.n_users), p_ok = ug_in_range(pi, w.n_items);
    if (!(u_ok && p_ok)) {  // block-uniform: the whole sample is dropped
      if (threadIdx.x == 0)
        atomicOr(&stats->status, (u_ok ? 0u : HIPREC_STATUS_USER_OOB) | (p_ok ? 0u : HIPREC_STATUS_ITEM_OOB));
      continue;
    }
    const float* ur = w.user_embeds + u * D;
    const float bu = p.beta_u[u];
    float uu[NPL], gu[NPL];
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int c = lane + kWave * k;
      uu[k] = c < D ? ur[c] : 0.f;
      gu[k] = 0.f;
    }
    // term 0 = the positive, 1 .. N = the negatives, N+1 .. N+K = the neighbours of the positive
    for (int t0 = wv * kUgUnroll; t0 < n_terms; t0 += kWavesPerBlock * kUgUnroll) {
      int64_t id[kUgUnroll];
      float sim[kUgUnroll];
#pragma unroll
      for (int j = 0; j < kUgUnroll; ++j) {
        const int t = t0 + j;
        id[j] = -1;
        sim[j] = 0.f;
        if (t == 0) {
          id[j] = pi;
        } else if (t <= n_neg) {
          id[j] = neg[b * n_neg + (t - 1)];
        } else if (t < n_terms) {
          const int64_t q = pi * p.n_neighbors + (t - 1 - n_neg);
          id[j] = p.ii_neighbor[q];
          sim[j] = p.ii_sim[q];
        }
      }
      float row[kUgUnroll][NPL], bi[kUgUnroll];
      bool ok[kUgUnroll];
#pragma unroll
      for (int j = 0; j < kUgUnroll; ++j) {
        ok[j] = ug_in_range(id[j], w.n_items);
        if (!ok[j] && t0 + j < n_terms && lane == 0) atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
        const int64_t r = ok[j] ? id[j] : 0;
        bi[j] = p.beta_i[r];
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
          const int c = lane + kWave * k;
          row[j][k] = c < D ? w.item_embeds[r * D + c] : 0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < kUgUnroll; ++j) {
        if (!ok[j]) continue;  // wave-uniform (past the last term, or an id out of range)
        const int t = t0 + j;
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < NPL; ++k) dot += uu[k] * row[j][k];
        const float s = wave_sum(dot);
        // every term is weight * softplus(-sign * s): bce(s, 1) = softplus(-s), bce(s, 0) = softplus(s),
        // -log(sigmoid(s)) = softplus(-s)
        float weight, sign = 1.f;
        if (t == 0) {
          weight = p.w1 + p.w2 * (bu * bi[j]);
        } else if (t <= n_neg) {
          weight = neg_scale * (p.w4 > 0.f ? p.w3 + p.w4 * (bu * bi[j]) : p.w3);
          sign = -1.f;
        } else {
          weight = p.lambda_ * sim[j];
        }
        float sg;  // sigmoid(-sign * s)
        loss_acc += weight * neg_logsigmoid(sign * s, &sg);
        const float coef = -sign * (weight * sg);  // d term / d s
        if (coef == 0.f) continue;                 // padded neighbours (sim 0): no gradient
        float* gr = g.item_embeds + id[j] * D;
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
          const int c = lane + kWave * k;
          gu[k] += coef * row[j][k];
          if (c < D) atomic_add_f32(gr + c, coef * uu[k]);
        }
      }
    }
    // the user row's gradient: registers -> LDS -> one atomic per column for the whole sample
#pragma unroll
    for (int k = 0; k < NPL; ++k) s_gu[wv][lane + kWave * k] = gu[k];
    lds_barrier();
    for (int c = threadIdx.x; c < D; c += kBlock) {
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < kWavesPerBlock; ++i) sum += s_gu[i][c];
      atomic_add_f32(g.user_embeds + u * D + c, sum);
    }
    lds_barrier();
  }

  // gamma / 2 * sum w^2 (the weights BEFORE this step's update): per-block sums in a fixed order
  if (blockIdx.x == 0 && sumsq_ws != nullptr) {
    int n = static_cast<int>(sumsq_ws[0]);
    n = n < 0 ? 0 : (n > kMaxBlocks ? kMaxBlocks : n);  // never read past the workspace, whatever it holds
    double t = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) t += sumsq_ws[1 + i];
    s_sq[threadIdx.x] = t;
    __syncthreads();
    for (int r = kBlock / 2; r > 0; r >>= 1) {
      if (static_cast<int>(threadIdx.x) < r) s_sq[threadIdx.x] += s_sq[threadIdx.x + r];
      __syncthreads();
    }
    if (wv == 0) loss_acc += p.gamma * (static_cast<float>(s_sq[0]) / 2.f);
  }
  publish_partials<kWavesPerBlock>(loss_acc, 0.f, 0.f, 1.f, scratch);
  if (stepper) step_store_advanced(stats, step_state);
}

// scores[k] = <U[u_k], V[i_k]>   (UltraGCN.predict, ultragcn.py:167-179)
__global__ __launch_bounds__(kBlock) void ug_predict_kernel(hiprec_ultragcn_tables w, const int64_t* __restrict__ users,
                                                            const int64_t* __restrict__ items, int64_t n,
                                                            float* __restrict__ scores, hiprec_stats* stats) {
  const int lane = lane_id();
  const int D = w.dim;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); t < n;
       t += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const int64_t u = users[t], i = items[t];
    const bool u_ok = ug_in_range(u, w.n_users), i_ok = ug_in_range(i, w.n_items);
    if (!(u_ok && i_ok)) {
      if (lane == 0) {
        atomicOr(&stats->status, (u_ok ? 0u : HIPREC_STATUS_USER_OOB) | (i_ok ? 0u : HIPREC_STATUS_ITEM_OOB));
        scores[t] = __builtin_nanf("");
      }
      continue;
    }
    float dot = 0.f;
    for (int c = lane; c < D; c += kWave) dot += w.user_embeds[u * D + c] * w.item_embeds[i * D + c];
    dot = wave_sum(dot);
    if (lane == 0) scores[t] = dot;
  }
}

// ws[0] = number of partials, ws[1 + b] = sum of x^2 over block b's grid-stride share (the layout the decay sweep of
// optim.hip emits for the updated weights)
__global__ __launch_bounds__(kBlock) void sumsq_kernel(const float* __restrict__ x, int64_t n, double* __restrict__ ws) {
  __shared__ double s_p[kBlock];
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  const int64_t n4 = n >> 2;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  double total = 0.0;
  for (int64_t i = tid; i < n4; i += stride) {
    const float4 v = x4[i];
    total += static_cast<double>((v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w));
  }
  for (int64_t i = (n4 << 2) + tid; i < n; i += stride) total += static_cast<double>(x[i] * x[i]);
  s_p[threadIdx.x] = total;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s) s_p[threadIdx.x] += s_p[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ws[1 + blockIdx.x] = s_p[0];
    if (blockIdx.x == 0) ws[0] = static_cast<double>(gridDim.x);
  }
}

// The dense optimizer sweep of csrc/optim.hip (the same opt_update, step_scalars and finalize_partials, so the same bits
// from the same gradient) for a loss that carries decay / 2 * sum w^2 over EVERY element (ultragcn.py:153-162): an
// element's gradient is g + decay * w, formed as it is consumed instead of in a pass of its own over the tables, and
// block b leaves the sum of the squares of ITS updated weights in sumsq_ws[1 + b] (fp32 per thread, fp64 across the
// block, a fixed order; sumsq_ws[0] = number of blocks) for the next step's loss value.  A raised status word (an id out
// of range in the preceding gradient kernel, whose gradient is then incomplete) turns the sweep into a no-op: the tables
// stay as they were.  A kernel of its own rather than one more template flag on opt_dense_kernel: the sweeps every other
// model runs stay byte for byte what they were.
template <int KIND>
__global__ __launch_bounds__(kBlock) void opt_dense_decay_kernel(float* __restrict__ w, float* __restrict__ g,
                                                                 float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                                 OptScalars s, float decay, hiprec_stats* stats,
                                                                 const Scratch* scratch, double* __restrict__ sumsq_ws) {
  __shared__ double s_sq[kBlock];
  if (stats->status != 0u) return;
  float step_size, bc2_sqrt;
  step_scalars<KIND>(s, stats, &step_size, &bc2_sqrt);
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  const int64_t n4 = n >> 2;
  float4* w4 = reinterpret_cast<float4*>(w);
  float4* g4 = reinterpret_cast<float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  float sq = 0.f;
  for (int64_t i = tid; i < n4; i += stride) {
    float4 wv = w4[i], gv = g4[i];
    float4 mv = make_float4(0, 0, 0, 0), vv = make_float4(0, 0, 0, 0);
    if constexpr (KIND == HIPREC_OPT_ADAM) mv = m4[i];
    if constexpr (KIND != HIPREC_OPT_SGD) vv = v4[i];
    gv.x = __builtin_fmaf(decay, wv.x, gv.x);
    gv.y = __builtin_fmaf(decay, wv.y, gv.y);
    gv.z = __builtin_fmaf(decay, wv.z, gv.z);
    gv.w = __builtin_fmaf(decay, wv.w, gv.w);
    opt_update<KIND>(wv.x, gv.x, mv.x, vv.x, s, step_size, bc2_sqrt);
    opt_update<KIND>(wv.y, gv.y, mv.y, vv.y, s, step_size, bc2_sqrt);
    opt_update<KIND>(wv.z, gv.z, mv.z, vv.z, s, step_size, bc2_sqrt);
    opt_update<KIND>(wv.w, gv.w, mv.w, vv.w, s, step_size, bc2_sqrt);
    sq += (wv.x * wv.x + wv.y * wv.y) + (wv.z * wv.z + wv.w * wv.w);
    w4[i] = wv;
    g4[i] = gv;
    if constexpr (KIND == HIPREC_OPT_ADAM) m4[i] = mv;
    if constexpr (KIND != HIPREC_OPT_SGD) v4[i] = vv;
  }
  for (int64_t i = (n4 << 2) + tid; i < n; i += stride) {  // scalar tail (< 4 elements)
    float wv = w[i], gv = __builtin_fmaf(decay, w[i], g[i]), mv = 0.f, vv = 0.f;
    if constexpr (KIND == HIPREC_OPT_ADAM) mv = m[i];
    if constexpr (KIND != HIPREC_OPT_SGD) vv = v[i];
    opt_update<KIND>(wv, gv, mv, vv, s, step_size, bc2_sqrt);
    sq += wv * wv;
    w[i] = wv;
    g[i] = gv;
    if constexpr (KIND == HIPREC_OPT_ADAM) m[i] = mv;
    if constexpr (KIND != HIPREC_OPT_SGD) v[i] = vv;
  }
  s_sq[threadIdx.x] = static_cast<double>(sq);
  __syncthreads();
  for (int r = kBlock / 2; r > 0; r >>= 1) {
    if (static_cast<int>(threadIdx.x) < r) s_sq[threadIdx.x] += s_sq[threadIdx.x + r];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    sumsq_ws[1 + blockIdx.x] = s_sq[0];
    if (blockIdx.x == 0) sumsq_ws[0] = static_cast<double>(gridDim.x);
  }
  if (blockIdx.x == 0 && scratch) finalize_partials(stats, scratch);
}

// g += gamma * w: the gamma term's gradient for callers that want the WHOLE gradient in memory (backward_only); the
// training step never runs this, its sweep adds the term on the fly.
__global__ __launch_bounds__(kBlock) void decay_grad_kernel(float* __restrict__ g, const float* __restrict__ w, int64_t n,
                                                            float gamma) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride)
    g[i] = __builtin_fmaf(gamma, w[i], g[i]);
}

inline int check_ug_tables(const hiprec_ultragcn_tables* w, const char* name) {
  HIPREC_REQUIRE(w != nullptr, "%s is NULL", name);
  HIPREC_REQUIRE(w->user_embeds && w->item_embeds, "%s: NULL tensor pointer", name);
  HIPREC_REQUIRE(w->n_users > 0 && w->n_items > 0 && w->dim > 0 && w->dim <= kUgMaxNpl * kWave,
                 "%s: UltraGCN needs positive sizes and dim <= %d (got %d)", name, kUgMaxNpl * kWave, w->dim);
  return 0;
}

}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_sumsq_workspace_bytes(void) { return sizeof(double) * (1 + kMaxBlocks); }

extern "C" int hiprec_sumsq(const float* x, int64_t n, void* workspace, size_t workspace_bytes, void* stream) {
  HIPREC_REQUIRE(n >= 0, "negative n");
  HIPREC_REQUIRE(workspace && (n == 0 || x), "NULL pointer");
  HIPREC_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0, "the buffer must be 16-byte aligned");
  HIPREC_REQUIRE(workspace_bytes >= hiprec_sumsq_workspace_bytes(), "workspace %zu B < %zu B", workspace_bytes,
                 hiprec_sumsq_workspace_bytes());
  sumsq_kernel<<<grid_for_threads((n + 3) / 4), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      x, n, static_cast<double*>(workspace));
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_opt_dense_step_decay(int kind, float* w, float* g, float* m, float* v, int64_t n, double lr,
                                           double beta1, double beta2, double eps, hiprec_stats* stats,
                                           const void* scratch, float decay, void* sumsq_workspace,
                                           size_t sumsq_workspace_bytes, void* stream) {
  HIPREC_REQUIRE(sumsq_workspace != nullptr, "NULL sums-of-squares workspace");
  HIPREC_REQUIRE(sumsq_workspace_bytes >= hiprec_sumsq_workspace_bytes(), "workspace %zu B < %zu B",
                 sumsq_workspace_bytes, hiprec_sumsq_workspace_bytes());
  HIPREC_REQUIRE(w && g && stats, "NULL w/g/stats");
  HIPREC_REQUIRE(n >= 0, "negative n");
  HIPREC_REQUIRE((reinterpret_cast<uintptr_t>(w) & 15) == 0 && (reinterpret_cast<uintptr_t>(g) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(m) & 15) == 0 && (reinterpret_cast<uintptr_t>(v) & 15) == 0,
                 "flat buffers must be 16-byte aligned");
  const OptScalars s{lr,
                     static_cast<float>(lr),
                     static_cast<float>(beta2),
                     static_cast<float>(1.0 - beta1),
                     static_cast<float>(1.0 - beta2),
                     static_cast<float>(eps)};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = grid_for_threads((n + 3) / 4);
  const auto* sc = static_cast<const Scratch*>(scratch);
  auto* sq = static_cast<double*>(sumsq_workspace);
  switch (kind) {
    case HIPREC_OPT_SGD:
      opt_dense_decay_kernel<HIPREC_OPT_SGD><<<grid, kBlock, 0, st>>>(w, g, m, v, n, s, decay, stats, sc, sq);
      break;
    case HIPREC_OPT_ADAM:
      HIPREC_REQUIRE(m && v, "adam needs exp_avg / exp_avg_sq buffers");
      opt_dense_decay_kernel<HIPREC_OPT_ADAM><<<grid, kBlock, 0, st>>>(w, g, m, v, n, s, decay, stats, sc, sq);
      break;
    case HIPREC_OPT_RMSPROP:
      HIPREC_REQUIRE(v, "rmsprop needs a square_avg buffer");
      opt_dense_decay_kernel<HIPREC_OPT_RMSPROP><<<grid, kBlock, 0, st>>>(w, g, m, v, n, s, decay, stats, sc, sq);
      break;
    default:
      set_error("unknown optimizer kind %d", kind);
      return HIPREC_E_UNSUPPORTED;
  }
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_decay_grad(float* g, const float* w, int64_t n, float gamma, void* stream) {
  HIPREC_REQUIRE(n >= 0, "negative n");
  HIPREC_REQUIRE(n == 0 || (g && w), "NULL pointer");
  if (n == 0) return 0;
  decay_grad_kernel<<<grid_for_threads(n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(g, w, n, gamma);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_ultragcn_grad(const hiprec_ultragcn_tables* w, const hiprec_ultragcn_tables* g,
                                    const hiprec_ultragcn_params* params, const int64_t* users, const int64_t* pos,
                                    const int64_t* neg, int64_t batch, int32_t n_neg, const void* sumsq_workspace,
                                    hiprec_stats* stats, void* scratch, size_t scratch_bytes, void* stream) {
  if (int rc = check_ug_tables(w, "w")) return rc;
  if (int rc = check_ug_tables(g, "g")) return rc;
  HIPREC_REQUIRE(w->n_users == g->n_users && w->n_items == g->n_items && w->dim == g->dim,
                 "weight / gradient shapes differ");
  HIPREC_REQUIRE(params != nullptr, "NULL params");
  HIPREC_REQUIRE(params->beta_u && params->beta_i, "NULL beta_u / beta_i");
  HIPREC_REQUIRE(params->n_neighbors >= 0, "negative n_neighbors");
  HIPREC_REQUIRE(params->n_neighbors == 0 || params->lambda_ == 0.f || (params->ii_neighbor && params->ii_sim),
                 "NULL neighbour tables with lambda != 0");
  HIPREC_REQUIRE(params->w2 > 0.f, "w2 <= 0 has no meaning in the reference (pow_weight is never bound)");
  HIPREC_REQUIRE(stats && scratch, "NULL stats/scratch");
  HIPREC_REQUIRE(batch >= 0 && n_neg >= 1, "batch must be >= 0 and n_neg >= 1");
  HIPREC_REQUIRE(batch == 0 || (users && pos && neg), "NULL index arrays");
  HIPREC_REQUIRE(params->gamma == 0.f || sumsq_workspace, "gamma != 0 needs the sums of squares of the weights");
  if (scratch_bytes < kScratchBytes) {
    set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
    return HIPREC_E_SCRATCH;
  }
  const int grid = static_cast<int>(batch < 1 ? 1 : (batch > kMaxBlocks ? kMaxBlocks : batch));
  auto s = static_cast<hipStream_t>(stream);
  const double* sq = params->gamma == 0.f ? nullptr : static_cast<const double*>(sumsq_workspace);
#define HIPREC_UG_LAUNCH(NPL)                                                                                     \
  ug_grad_kernel<NPL><<<grid, kBlock, 0, s>>>(*w, *g, *params, users, pos, neg, batch, n_neg, sq, stats,          \
                                              static_cast<Scratch*>(scratch))
  switch ((w->dim + kWave - 1) / kWave) {
    case 1: HIPREC_UG_LAUNCH(1); break;
    case 2: HIPREC_UG_LAUNCH(2); break;
    case 3: HIPREC_UG_LAUNCH(3); break;
    default: HIPREC_UG_LAUNCH(4); break;
  }
#undef HIPREC_UG_LAUNCH
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_ultragcn_predict(const hiprec_ultragcn_tables* w, const int64_t* users, const int64_t* items,
                                       int64_t n, float* scores, hiprec_stats* stats, void* stream) {
  if (int rc = check_ug_tables(w, "w")) return rc;
  HIPREC_REQUIRE(n >= 0, "negative n");
  if (n == 0) return 0;
  HIPREC_REQUIRE(users && items && scores && stats, "NULL pointer");
  ug_predict_kernel<<<grid_for_waves(n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(*w, users, items, n, scores,
                                                                                       stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// UltraGCNEngine.train_an_epoch (ultragcn.py:218-236) over resident arrays in visiting order: every batch is
// hiprec_ultragcn_grad + hiprec_opt_dense_step_decay, enqueued back to back from C.
extern "C" int hiprec_ultragcn_epoch(const hiprec_ultragcn_tables* w, const hiprec_ultragcn_tables* g,
                                     const hiprec_ultragcn_params* params, const int64_t* users, const int64_t* pos,
                                     const int64_t* neg, int64_t n_samples, int64_t batch, int32_t n_neg, int kind,
                                     double lr, double beta1, double beta2, double eps, float* flat_w, float* flat_g,
                                     float* flat_m, float* flat_v, int64_t n_flat, void* sumsq_workspace,
                                     size_t sumsq_workspace_bytes, hiprec_stats* stats, void* scratch,
                                     size_t scratch_bytes, void* stream) {
  HIPREC_REQUIRE(n_samples >= 0 && batch > 0 && n_neg >= 1, "bad n_samples/batch/n_neg");
  HIPREC_REQUIRE(flat_w && flat_g && n_flat > 0, "the dense optimizer needs the flat buffers");
  HIPREC_REQUIRE(params != nullptr, "NULL params");
  // the weights may have come from anywhere (construction, load_state_dict): one reduction per epoch, then every
  // sweep hands the sums of its new weights to the next step
  if (int rc = hiprec_sumsq(flat_w, n_flat, sumsq_workspace, sumsq_workspace_bytes, stream)) return rc;
  if (int rc = hiprec_stats_begin_epoch(stats, stream)) return rc;
  for (int64_t off = 0; off < n_samples; off += batch) {
    const int64_t b = (n_samples - off < batch) ? (n_samples - off) : batch;
    if (int rc = hiprec_ultragcn_grad(w, g, params, users + off, pos + off, neg + off * n_neg, b, n_neg,
                                      sumsq_workspace, stats, scratch, scratch_bytes, stream))
      return rc;
    if (int rc = hiprec_opt_dense_step_decay(kind, flat_w, flat_g, flat_m, flat_v, n_flat, lr, beta1, beta2, eps, stats,
                                             scratch, params->gamma, sumsq_workspace, sumsq_workspace_bytes, stream))
      return rc;
  }
  return 0;
}
