// MixGCF training step for gfx950.
//
// Replaces beta_rec/models/mixgcf.py:46-67 (GraphConv.forward: per hop edge dropout + torch.sparse.mm + message
// dropout, every hop's output kept), :222-251 (negative_sampling: K * n_negs candidates gathered at all L + 1 hops,
// mixed with the positive, scored against the user, per-hop argmax), :253-286 (create_bpr_loss: pooling, K-pair
// softplus, L2 on the hop-0 rows) and the backward the reference never runs (its train_single_batch returns the loss
// tensor and stops): a different gradient for every hop's table, then L transposed SpMMs down to the parameters.
//
// Layout: L + 1 tables of [N, D], hop 0 being the parameter buffer itself.  The SpMM (spmm.hpp::launch_spmm, the
// gather CSR form of lightgcn.hip) reads and writes row-major [N, D]; an interleaved [N, L + 1, D] would need a
// strided form of it and a copy of the parameters per step, for a sampler whose rows are 256 B segments either way.
//
// The sampler + loss + scatter kernel follows lightgcn_loss_kernel: one wave per batch row, one lane per column
// (NPL columns per lane), the user's and the positive's hop rows in registers.  Candidates stream through: all hop
// rows of candidate j + 1 are requested before candidate j's L + 1 wave reductions.
#include "common.hpp"
#include "spmm.hpp"

namespace hiprec {

__global__ __launch_bounds__(kBlock) void mixgcf_mask_kernel(float* __restrict__ x, const uint8_t* __restrict__ keep,
                                                             float scale, int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride)
    x[i] = keep[i] ? x[i] * scale : 0.f;
}

__device__ __forceinline__ float mixgcf_coef(int pool, int l, int L) {
  if (pool == HIPREC_MIXGCF_POOL_MEAN) return 1.0f / static_cast<float>(L + 1);
  if (pool == HIPREC_MIXGCF_POOL_FINAL) return l == L ? 1.f : 0.f;
  return 1.f;
}

// score(a, b) = sum_l coef_l <s_l, b_l> with s_l = a_l (concat) or pool(a) (mean / sum / final: the same for every l),
// which is <pool(a), pool(b)> for the pooled forms and the concatenated dot product for concat.
// HMAX: hop tables held in registers (L + 1 <= HMAX); NPL: columns per lane (dim <= 64 * NPL).
// Per row: pass 1 finds the per-hop argmax of every k and x_k = s_neg_k - s_pos; the K-pair softplus needs every x_k
// before any gradient, so pass 2 scatters.  With K == 1 the winning mixed rows are still in registers; with K > 1 the
// winners (L + 1 rows per k, against n_negs * (L + 1) in pass 1) are gathered again.  Lane k * (L + 1) + l keeps
// choice[k][l], lane k keeps x_k: K * (L + 1) <= 64.
template <int NPL, int HMAX>
__global__ __launch_bounds__(kBlock) void mixgcf_loss_kernel(
    hiprec_mixgcf_plan p, const int64_t* __restrict__ users, const int64_t* __restrict__ pos,
    const int64_t* __restrict__ neg, int64_t neg_stride, int64_t batch, const float* __restrict__ seeds,
    int32_t* __restrict__ choice, float inv_batch, hiprec_stats* stats, Scratch* scratch) {
  const int lane = lane_id();
  const int D = p.dim, L = p.n_hops, H = L + 1, K = p.k_neg;
  const int n_c = p.rns ? 1 : p.n_negs;
  const bool concat = p.pool == HIPREC_MIXGCF_POOL_CONCAT;
  const int64_t ND = p.a.n_rows * D;
  const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  auto tab = [&](int l) -> const float* { return l == 0 ? p.e0 : p.zero_ws + static_cast<int64_t>(l - 1) * ND; };
  auto gtab = [&](int l) -> float* { return l == 0 ? p.g : p.zero_ws + static_cast<int64_t>(L + l - 1) * ND; };
  float coef[HMAX];
#pragma unroll
  for (int l = 0; l < HMAX; ++l) coef[l] = l < H ? mixgcf_coef(p.pool, l, L) : 0.f;
  const float cr = p.l2 * inv_batch;  // d reg / d row = l2 * row / B
  float loss_acc = 0.f, reg_acc = 0.f;
  const bool stepper = blockIdx.x == 0 && threadIdx.x == 0;
  StepState ss{};
  if (stepper) ss = step_load(stats);

  for (int64_t t = wave0; t < batch; t += n_waves) {
    const int64_t u = users[t], ip = pos[t];
    const int64_t* __restrict__ cand = neg + t * neg_stride;
    const bool u_ok = static_cast<uint64_t>(u) < static_cast<uint64_t>(p.n_users);
    bool bad = false;
    for (int i = lane; i < K * n_c; i += kWave) bad |= static_cast<uint64_t>(cand[i]) >= static_cast<uint64_t>(p.n_items);
    const bool i_ok = static_cast<uint64_t>(ip) < static_cast<uint64_t>(p.n_items) && __ballot(bad) == 0;
    if (!(u_ok && i_ok)) {
      if (lane == 0)
        atomicOr(&stats->status, (u_ok ? 0u : HIPREC_STATUS_USER_OOB) | (i_ok ? 0u : HIPREC_STATUS_ITEM_OOB));
      continue;
    }
    const int64_t ru = u * D, rp = (p.n_users + ip) * D;
    float uh[HMAX][NPL], ph[HMAX][NPL], pu[NPL], pp[NPL];
#pragma unroll
    for (int l = 0; l < HMAX; ++l) {
#pragma unroll
      for (int k = 0; k < NPL; ++k) {
        const int c = lane + kWave * k;
        const bool in = l < H && c < D;
        uh[l][k] = in ? tab(l)[ru + c] : 0.f;
        ph[l][k] = in ? tab(l)[rp + c] : 0.f;
      }
    }
    float sp = 0.f;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      pu[k] = 0.f;
      pp[k] = 0.f;
      float cdot = 0.f;
#pragma unroll
      for (int l = 0; l < HMAX; ++l) {
        pu[k] += coef[l] * uh[l][k];
        pp[k] += coef[l] * ph[l][k];
        cdot += uh[l][k] * ph[l][k];
      }
      sp += concat ? cdot : pu[k] * pp[k];
      reg_acc += uh[0][k] * uh[0][k] + ph[0][k] * ph[0][k];
    }
    sp = wave_sum(sp);
    auto sv = [&](int l, int k) { return concat ? uh[l][k] : pu[k]; };
    auto load_cand = [&](float (&dst)[HMAX][NPL], int64_t item) {
      const int64_t rc = (p.n_users + item) * D;
#pragma unroll
      for (int l = 0; l < HMAX; ++l) {
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
          const int c = lane + kWave * k;
          dst[l][k] = (l < H && c < D) ? tab(l)[rc + c] : 0.f;
        }
      }
    };

    // ---- pass 1: the sampler
    float bm[HMAX][NPL];  // best mixed row per hop of the current k
    float xv = 0.f;       // lane k: x_k
    int ch = 0;           // lane k * H + l: choice[k][l]
    for (int kk = 0; kk < K; ++kk) {
      float seed[HMAX];
#pragma unroll
      for (int l = 0; l < HMAX; ++l) seed[l] = (seeds && l < H) ? seeds[(t * K + kk) * H + l] : 0.f;
      float best[HMAX];
      int bj[HMAX];
#pragma unroll
      for (int l = 0; l < HMAX; ++l) {
        best[l] = 0.f;
        bj[l] = 0;
      }
      float cn[HMAX][NPL];
      load_cand(cn, cand[kk * n_c]);
      for (int j = 0; j < n_c; ++j) {
        float m[HMAX][NPL];
#pragma unroll
        for (int l = 0; l < HMAX; ++l)
#pragma unroll
          for (int k = 0; k < NPL; ++k) m[l][k] = cn[l][k];
        if (j + 1 < n_c) load_cand(cn, cand[kk * n_c + j + 1]);
        float dot[HMAX];
#pragma unroll
        for (int l = 0; l < HMAX; ++l) {
          dot[l] = 0.f;
#pragma unroll
          for (int k = 0; k < NPL; ++k) {
            m[l][k] = seed[l] * ph[l][k] + (1.f - seed[l]) * m[l][k];
            dot[l] += sv(l, k) * m[l][k];
          }
        }
#pragma unroll
        for (int l = 0; l < HMAX; ++l) {
          if (l < H) {
            const float d = wave_sum(dot[l]);
            if (j == 0 || d > best[l]) {  // ties keep the lowest j
              best[l] = d;
              bj[l] = j;
#pragma unroll
              for (int k = 0; k < NPL; ++k) bm[l][k] = m[l][k];
            }
          }
        }
      }
      float sn = 0.f;
#pragma unroll
      for (int l = 0; l < HMAX; ++l) {
        if (l < H) {
          sn += coef[l] * best[l];
          if (lane == kk * H + l) ch = bj[l];
        }
      }
      if (lane == kk) xv = sn - sp;
#pragma unroll
      for (int k = 0; k < NPL; ++k) reg_acc += bm[0][k] * bm[0][k];
    }
    if (choice && lane < K * H) choice[t * K * H + lane] = ch;

    // ---- log(1 + sum_k exp(x_k)), shifted by max(0, max_k x_k)
    float mx = 0.f;
    for (int kk = 0; kk < K; ++kk)
      mx = fmaxf(mx, __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, xv), kk)));
    float z = expf(-mx);
    for (int kk = 0; kk < K; ++kk)
      z += expf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, xv), kk)) - mx);
    loss_acc += mx + logf(z);
    const float inv_z = inv_batch / z;

    // ---- pass 2: the gradient
    float du[HMAX][NPL], dq[NPL], p0acc[NPL], a_l[HMAX];
    float gsum = 0.f;
#pragma unroll
    for (int l = 0; l < HMAX; ++l) {
      a_l[l] = 0.f;
#pragma unroll
      for (int k = 0; k < NPL; ++k) du[l][k] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      dq[k] = 0.f;
      p0acc[k] = 0.f;
    }
    for (int kk = 0; kk < K; ++kk) {
      const float gk =
          expf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, xv), kk)) - mx) * inv_z;
      gsum += gk;
      float seed[HMAX];
      int64_t rc[HMAX];
#pragma unroll
      for (int l = 0; l < HMAX; ++l) {
        seed[l] = (seeds && l < H) ? seeds[(t * K + kk) * H + l] : 0.f;
        const int j = l < H ? __builtin_amdgcn_readlane(ch, kk * H + l) : 0;
        rc[l] = (p.n_users + cand[kk * n_c + j]) * D;
      }
      if (K > 1) {  // (K == 1: bm still holds the winners)
#pragma unroll
        for (int l = 0; l < HMAX; ++l) {
#pragma unroll
          for (int k = 0; k < NPL; ++k) {
            const int c = lane + kWave * k;
            const float cv = (l < H && c < D) ? tab(l)[rc[l] + c] : 0.f;
            bm[l][k] = seed[l] * ph[l][k] + (1.f - seed[l]) * cv;
          }
        }
      }
#pragma unroll
      for (int l = 0; l < HMAX; ++l) {
        if (l < H) {
          a_l[l] += gk * (seed[l] - 1.f);
          const bool live = coef[l] != 0.f || l == 0;
#pragma unroll
          for (int k = 0; k < NPL; ++k) {
            const int c = lane + kWave * k;
            float dn = gk * coef[l] * sv(l, k);
            if (l == 0) {
              dn += cr * bm[0][k];
              p0acc[k] += seed[0] * bm[0][k];
            }
            if (concat) du[l][k] += gk * bm[l][k];
            else dq[k] += gk * coef[l] * bm[l][k];
            if (live && c < D) atomic_add_f32(gtab(l) + rc[l] + c, (1.f - seed[l]) * dn);
          }
        }
      }
    }
#pragma unroll
    for (int l = 0; l < HMAX; ++l) {
      if (l < H && (coef[l] != 0.f || l == 0)) {
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
          const int c = lane + kWave * k;
          float gu = concat ? du[l][k] - gsum * ph[l][k] : coef[l] * (dq[k] - gsum * pp[k]);
          float gp = coef[l] * sv(l, k) * a_l[l];
          if (l == 0) {
            gu += cr * uh[0][k];
            gp += cr * (ph[0][k] + p0acc[k]);
          }
          if (c < D) {
            atomic_add_f32(gtab(l) + ru + c, gu);
            atomic_add_f32(gtab(l) + rp + c, gp);
          }
        }
      }
    }
  }
  if (stepper) step_store_advanced(stats, ss);
  const float reg_w = wave_sum(reg_acc);
  publish_partials<kWavesPerBlock>(loss_acc + 0.5f * p.l2 * reg_w, 0.f, 0.f, inv_batch, scratch);
}

__global__ __launch_bounds__(kBlock) void mixgcf_predict_kernel(hiprec_mixgcf_plan p, const int64_t* __restrict__ users,
                                                                const int64_t* __restrict__ items, int64_t n,
                                                                float* __restrict__ scores, hiprec_stats* stats) {
  const int lane = lane_id();
  const int D = p.dim, L = p.n_hops;
  const bool concat = p.pool == HIPREC_MIXGCF_POOL_CONCAT;
  const int64_t ND = p.a.n_rows * D;
  const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t t = wave0; t < n; t += n_waves) {
    const int64_t u = users[t], i = items[t];
    if (static_cast<uint64_t>(u) >= static_cast<uint64_t>(p.n_users) ||
        static_cast<uint64_t>(i) >= static_cast<uint64_t>(p.n_items)) {
      if (lane == 0) {
        atomicOr(&stats->status, HIPREC_STATUS_ROW_OOB);
        scores[t] = __builtin_nanf("");
      }
      continue;
    }
    float dot = 0.f;
    for (int c = lane; c < D; c += kWave) {
      float su = 0.f, si = 0.f, cd = 0.f;
      for (int l = 0; l <= L; ++l) {
        const float* tb = l == 0 ? p.e0 : p.zero_ws + static_cast<int64_t>(l - 1) * ND;
        const float a = tb[u * D + c], b = tb[(p.n_users + i) * D + c];
        const float w = mixgcf_coef(p.pool, l, L);
        su += w * a;
        si += w * b;
        cd += a * b;
      }
      dot += concat ? cd : su * si;
    }
    dot = wave_sum(dot);
    if (lane == 0) scores[t] = dot;
  }
}

static int check_mix_plan(const hiprec_mixgcf_plan* p, bool train) {
  HIPREC_REQUIRE(p != nullptr, "NULL plan");
  HIPREC_REQUIRE(p->a.rowptr && p->a.n_rows > 0 && p->a.nnz >= 0 && (p->a.nnz == 0 || (p->a.col && p->a.val)),
                 "bad CSR a");
  HIPREC_REQUIRE(p->n_users > 0 && p->n_items > 0 && p->dim > 0, "bad sizes");
  HIPREC_REQUIRE(p->a.n_rows == p->n_users + p->n_items, "graph size != n_users + n_items");
  HIPREC_REQUIRE(p->n_hops >= 0 && p->n_hops <= HIPREC_MIXGCF_MAX_HOPS, "MixGCF context_hops %d: 0 .. %d are supported",
                 p->n_hops, HIPREC_MIXGCF_MAX_HOPS);
  if (p->dim > 256) {
    set_error("MixGCF embedding dim %d > 256 is not supported", p->dim);
    return HIPREC_E_UNSUPPORTED;
  }
  HIPREC_REQUIRE(p->pool >= HIPREC_MIXGCF_POOL_CONCAT && p->pool <= HIPREC_MIXGCF_POOL_FINAL, "bad pool %d", p->pool);
  HIPREC_REQUIRE(p->e0 != nullptr, "NULL e0");
  HIPREC_REQUIRE(p->n_hops == 0 ||
                     (p->zero_ws && p->zero_ws_floats >= 2 * static_cast<int64_t>(p->n_hops) * p->a.n_rows * p->dim),
                 "zero_ws holds %lld floats, 2 * n_hops * n_rows * dim are needed", (long long)p->zero_ws_floats);
  if (train) {
    HIPREC_REQUIRE(p->at.rowptr && p->at.n_rows == p->a.n_rows && p->at.nnz == p->a.nnz &&
                       (p->a.nnz == 0 || (p->at.col && p->at.val)),
                   "bad CSR at / a and at differ");
    HIPREC_REQUIRE(p->g != nullptr, "NULL g");
    HIPREC_REQUIRE(p->k_neg >= 1 && (p->rns || p->n_negs >= 1), "k_neg and n_negs must be >= 1");
    HIPREC_REQUIRE(static_cast<int64_t>(p->k_neg) * (p->n_hops + 1) <= kWave,
                   "MixGCF K * (context_hops + 1) = %lld > 64 is not supported",
                   (long long)p->k_neg * (p->n_hops + 1));
    for (int l = 0; l < p->n_hops; ++l)
      HIPREC_REQUIRE(p->edge_keep[l] == nullptr || p->at.eid != nullptr || p->a.nnz == 0,
                     "edge dropout needs at.eid (the transposed graph's map to the forward edges)");
  }
  return 0;
}

static float* mix_hop(const hiprec_mixgcf_plan* p, int l) {  // l >= 1
  return p->zero_ws + static_cast<int64_t>(l - 1) * p->a.n_rows * p->dim;
}

static float* mix_dhop(const hiprec_mixgcf_plan* p, int l) {
  return l == 0 ? p->g : p->zero_ws + static_cast<int64_t>(p->n_hops + l - 1) * p->a.n_rows * p->dim;
}

static int mix_mask(float* x, const uint8_t* keep, float scale, int64_t n, hipStream_t st) {
  mixgcf_mask_kernel<<<grid_for_threads(n), kBlock, 0, st>>>(x, keep, scale, n);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// zeroed: the caller cleared the hop tables already
static int mix_propagate(const hiprec_mixgcf_plan* p, bool train, hipStream_t st, bool zeroed) {
  const int64_t n = p->a.n_rows * p->dim;
  const float* cur = p->e0;
  for (int l = 0; l < p->n_hops; ++l) {
    float* nxt = mix_hop(p, l + 1);
    const uint8_t* ek = train ? p->edge_keep[l] : nullptr;
    if (int rc = launch_spmm(&p->a, ek, p->edge_scale, cur, nxt, nullptr, p->dim, st, zeroed)) return rc;
    if (train && p->mess_keep[l])
      if (int rc = mix_mask(nxt, p->mess_keep[l], p->mess_scale, n, st)) return rc;
    cur = nxt;
  }
  return 0;
}

}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_mixgcf_plan_bytes(void) { return sizeof(hiprec_mixgcf_plan); }

extern "C" int hiprec_mixgcf_propagate(const hiprec_mixgcf_plan* plan, int32_t train, void* stream) {
  if (int rc = check_mix_plan(plan, false)) return rc;
  return mix_propagate(plan, train != 0, static_cast<hipStream_t>(stream), false);
}

extern "C" int hiprec_mixgcf_predict(const hiprec_mixgcf_plan* plan, const int64_t* users, const int64_t* items,
                                     int64_t n, float* scores, hiprec_stats* stats, void* stream) {
  if (int rc = check_mix_plan(plan, false)) return rc;
  if (n == 0) return 0;
  HIPREC_REQUIRE(n > 0 && users && items && scores && stats, "NULL pointer");
  mixgcf_predict_kernel<<<grid_for_waves(n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(*plan, users, items, n,
                                                                                          scores, stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

template <int HMAX>
static int launch_mix_loss(const hiprec_mixgcf_plan& p, const int64_t* users, const int64_t* pos, const int64_t* neg,
                           int64_t neg_stride, int64_t batch, const float* seeds, int32_t* choice, float inv_batch,
                           hiprec_stats* stats, Scratch* scratch, hipStream_t st) {
  const int grid = grid_for_waves(batch);
  if (p.dim <= 64)
    mixgcf_loss_kernel<1, HMAX><<<grid, kBlock, 0, st>>>(p, users, pos, neg, neg_stride, batch, seeds, choice, inv_batch,
                                                         stats, scratch);
  else if (p.dim <= 128)
    mixgcf_loss_kernel<2, HMAX><<<grid, kBlock, 0, st>>>(p, users, pos, neg, neg_stride, batch, seeds, choice, inv_batch,
                                                         stats, scratch);
  else
    mixgcf_loss_kernel<4, HMAX><<<grid, kBlock, 0, st>>>(p, users, pos, neg, neg_stride, batch, seeds, choice, inv_batch,
                                                         stats, scratch);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_mixgcf_grad(const hiprec_mixgcf_plan* plan, const int64_t* users, const int64_t* pos,
                                  const int64_t* neg, int64_t neg_stride, int64_t batch, const float* seeds,
                                  int32_t* choice, float inv_batch, hiprec_stats* stats, void* scratch,
                                  size_t scratch_bytes, void* stream) {
  if (int rc = check_mix_plan(plan, true)) return rc;
  HIPREC_REQUIRE(batch > 0 && users && pos && neg && stats && scratch, "NULL pointer / empty batch");
  const hiprec_mixgcf_plan* p = plan;
  const int64_t need = p->rns ? p->k_neg : static_cast<int64_t>(p->k_neg) * p->n_negs;
  HIPREC_REQUIRE(neg_stride >= need, "neg rows hold %lld ids, %lld are needed", (long long)neg_stride, (long long)need);
  HIPREC_REQUIRE(p->rns || seeds, "NULL seeds");
  if (scratch_bytes < kScratchBytes) {
    set_error("scratch too small: %zu < %zu", scratch_bytes, kScratchBytes);
    return HIPREC_E_SCRATCH;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int L = p->n_hops;
  const int64_t n = p->a.n_rows * p->dim;
  // ONE fill for every hop table and every hop's gradient table of the step
  if (L > 0) HIPREC_TRY(hipMemsetAsync(p->zero_ws, 0, sizeof(float) * 2 * L * n, st));
  if (int rc = mix_propagate(p, true, st, true)) return rc;
  const float* sd = p->rns ? nullptr : seeds;
  int rc = L + 1 <= 4 ? launch_mix_loss<4>(*p, users, pos, neg, neg_stride, batch, sd, choice, inv_batch, stats,
                                           static_cast<Scratch*>(scratch), st)
                      : launch_mix_loss<HIPREC_MIXGCF_MAX_HOPS + 1>(*p, users, pos, neg, neg_stride, batch, sd, choice,
                                                                     inv_batch, stats, static_cast<Scratch*>(scratch), st);
  if (rc) return rc;
  // dE_l = G_l + A_l^T (mask_l (.) dE_{l+1}): the SpMM only ever ADDS into its output (atomic flushes), so with
  // y_is_zero it accumulates onto the G_l the loss kernel scattered; hop 0 ends in the flat gradient buffer
  for (int l = L - 1; l >= 0; --l) {
    float* cur = mix_dhop(p, l + 1);
    if (p->mess_keep[l])
      if (int r2 = mix_mask(cur, p->mess_keep[l], p->mess_scale, n, st)) return r2;
    if (int r2 = launch_spmm(&p->at, p->edge_keep[l], p->edge_scale, cur, mix_dhop(p, l), nullptr, p->dim, st, true))
      return r2;
  }
  return 0;
}
