// TVBR: the time-aware variational basket model of the grocery family (beta_rec/models/tvbr.py), VBCAR's temporal
// successor.
//
//   tvbr.py:65-119    parameters: user_emb, item_emb [.,D], time_embdding [T+1,T+1], user_mean / user_std / item_mean /
//                     item_std [.,D], four one-layer encoders time2{mean,std}_{u,i}: Linear(D + T+1 + F, D) + act
//   tvbr.py:121-187   encode: h = act(W [table[id] | time row | fea[id]] + b), once with the row of t (prior) and once
//                     with the row of t+1 (posterior); std = exp(0.5 h)
//   tvbr.py:189-240   reparameterize(mean, std) treats std as a log-variance: z = mean + eps exp(0.5 std);
//                     kl_div(prior, posterior) with var = std^2 + 1e-10, a mean over the rows of its own group
//   tvbr.py:242-369   forward: the Triple2vec scores on e = [z | emb[id]], rec / (3 config batch), kl = -0.5 sum of six
//
// Only the time columns of the concatenated input differ between the prior and the posterior run of a Linear, so
//   pre = base + Tb[.],   base = [table[id] | 0 | fea[id]] W^T + b  (once per row),   Tb = time_embdding W_t^T  [T+1, D]
// with W_t the time-column block of W: half the encoder GEMM work, and no [rows, D + T+1 + F] concatenation per run.
// The gathered rows keep ZEROED time columns, so W is used whole through its leading dimension (forward and weight
// gradient alike; the weight gradient's time columns come out exactly zero and get dTb^T time_embdding afterwards).
//
// One step, rows Ru = B (1 + n_neg) users ([pos_u | neg_u]) and Ri = 2 B (1 + n_neg) items ([pos_i_1 | pos_i_2 | neg_i_1
// | neg_i_2]), each row with its own t; encoders e = 0..3 = mean_u, std_u, mean_i, std_i:
//   1 gather        X_e = [table_e[id] | 0 | fea[id]]                         tv_gather_kernel
//   2 GEMM          base_e = X_e W_e^T + b_e  and  Tb_e = time W_t,e^T         (8 problems, one grouped launch)
//   3 activation    h_e(prior) = act(base_e + Tb_e[t]), h_e(post) = act(base_e + Tb_e[t+1])      tv_act_kernel
//   4 loss stage    one wave per triple: z, scores, logsigmoid, KL; d h of all four activations of every row written
//                   with plain stores, the user_emb / item_emb halves added with row atomics     tv_loss_kernel
//   5 activation'   d pre = d h act'(h) (from h; prelu from base + Tb), d base = d post + d prior in place, dTb reduced
//                   in registers over a wave's run of equal t and in LDS over the block before any atomic, the prelu
//                   slope's gradient one atomic per wave                                           tv_bwd_kernel
//   6 GEMM          dW_e = d base_e^T X_e, db_e = colsum, d table rows = d base_e W_e[:, :D]       (12 problems)
//   7 scatter       the four tables' row gradients, 256-byte row atomics                            tv_scatter_kernel
//   8 time path     dW_t,e = dTb_e^T time (4 problems), d time = sum_e dTb_e W_t,e                  tv_time_grad_kernel
#include <algorithm>

#include "gemm.hpp"

namespace hiprec {
namespace {

constexpr int kTvMaxDim = 128;      // emb_dim: two columns per lane
constexpr int kTvMaxFea = 1 << 16;  // feature width
constexpr int kTvMaxTime = 255;     // time_step
constexpr int kTvNpl = kTvMaxDim / kWave;
constexpr int kTvChunk = 8192;      // rows per pass of the eval-mode encoder
constexpr int kTvBwdRows = 8;       // stage 5: rows a wave walks at least, and at most this many blocks per side
constexpr int kTvBwdMaxBlocks = 256;
constexpr int kTvBwdUnroll = 4;     // ... of which it keeps this many in flight
constexpr float kTvEsp = 1e-10f;    // tvbr.py:34

__device__ __forceinline__ bool tv_in_range(int64_t i, int64_t n) {
  return static_cast<uint64_t>(i) < static_cast<uint64_t>(n);
}

// Which id and which t a row of a side has.  Training: the six id arrays and the two t arrays of the reference's batch.
// Eval mode (fixed_t >= 0): ids[0] holds the ids of the one side in use, every row at fixed_t.
struct TvRows {
  const int64_t* ids[6];
  const int64_t *pos_t, *neg_t;
  int64_t B, Bn, fixed_t;
};

__device__ __forceinline__ int64_t tv_id(const TvRows& a, int side, int64_t r) {
  if (a.fixed_t >= 0) return a.ids[0][r];
  if (side == 0) return r < a.B ? a.ids[0][r] : a.ids[3][r - a.B];
  if (r < a.B) return a.ids[1][r];
  if (r < 2 * a.B) return a.ids[2][r - a.B];
  r -= 2 * a.B;
  return r < a.Bn ? a.ids[4][r] : a.ids[5][r - a.Bn];
}

__device__ __forceinline__ int64_t tv_time(const TvRows& a, int side, int64_t r) {
  if (a.fixed_t >= 0) return a.fixed_t;
  if (side == 0) return r < a.B ? a.pos_t[r] : a.neg_t[r - a.B];
  if (r < 2 * a.B) return a.pos_t[r < a.B ? r : r - a.B];
  r -= 2 * a.B;
  return a.neg_t[r < a.Bn ? r : r - a.Bn];
}

// ---- 1. gather --------------------------------------------------------------------------------------------------------
// Row r of X[side][kind] = [table[side][kind][id] | T1 zeros | fea[side][id]].  An id outside its table sets the side's
// status bit and leaves a zero row.  enc_out (eval mode): the id's user_emb / item_emb row goes to the second half of
// its output row.
struct TvGather {
  TvRows rows;
  int64_t R[2], n_ids[2];
  const float* fea[2];
  const float* tab[2][2];
  float* X[2][2];
  int F[2];
  int D, T1, kinds;
  const float* emb;
  float* enc_out;
};

__global__ __launch_bounds__(kBlock) void tv_gather_kernel(TvGather a, hiprec_stats* stats) {
  const int lane = lane_id();
  const int64_t n_rows = a.R[0] + a.R[1];
  const int D = a.D, T1 = a.T1;
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); q < n_rows;
       q += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const int side = q < a.R[0] ? 0 : 1;
    const int64_t r = side ? q - a.R[0] : q;
    const int64_t id = tv_id(a.rows, side, r);
    const bool ok = tv_in_range(id, a.n_ids[side]);
    if (!ok && lane == 0) atomicOr(&stats->status, side == 0 ? HIPREC_STATUS_USER_OOB : HIPREC_STATUS_ITEM_OOB);
    const int F = a.F[side];
    const int64_t K = static_cast<int64_t>(D) + T1 + F, src_row = ok ? id : 0;
    const float* __restrict__ f = a.fea[side] + src_row * F;
    for (int kind = 0; kind < a.kinds; ++kind) {
      const float* __restrict__ tab = a.tab[side][kind] + src_row * D;
      float* __restrict__ dst = a.X[side][kind] + r * K;
      for (int c = lane; c < D; c += kWave) dst[c] = ok ? tab[c] : 0.f;
      for (int c = lane; c < T1; c += kWave) dst[D + c] = 0.f;
      for (int c = lane; c < F; c += kWave) dst[D + T1 + c] = ok ? f[c] : 0.f;
    }
    if (a.enc_out) {
      float* e = a.enc_out + r * 2 * D + D;
      for (int c = lane; c < D; c += kWave) e[c] = ok ? a.emb[id * D + c] : __builtin_nanf("");
    }
  }
}

// ---- 3 / 5. the activation and its derivative ----------------------------------------------------------------------------
__device__ __forceinline__ float tv_act(int act, float x, float slope) {
  switch (act) {
    case HIPREC_TVBR_ACT_TANH: return tanhf(x);
    case HIPREC_TVBR_ACT_HARDTANH: return fminf(fmaxf(x, -1.0f), 1.0f);
    case HIPREC_TVBR_ACT_LOGSIGMOID: return fminf(x, 0.f) - log1pf(expf(-fabsf(x)));
    case HIPREC_TVBR_ACT_SIGMOID: return 1.0f / (1.0f + expf(-x));
    case HIPREC_TVBR_ACT_RELU: return x > 0.f ? x : 0.f;
    case HIPREC_TVBR_ACT_LRELU: return x > 0.f ? x : 0.01f * x;
    default: return x > 0.f ? x : slope * x;   // prelu
  }
}

// from the output h where h determines it; prelu (any slope, zero and negative ones too) from the pre-activation
__device__ __forceinline__ float tv_act_grad(int act, float h, float pre, float slope) {
  switch (act) {
    case HIPREC_TVBR_ACT_TANH: return 1.0f - h * h;
    case HIPREC_TVBR_ACT_HARDTANH: return fabsf(h) < 1.0f ? 1.0f : 0.f;
    case HIPREC_TVBR_ACT_LOGSIGMOID: return 1.0f - expf(h);
    case HIPREC_TVBR_ACT_SIGMOID: return h * (1.0f - h);
    case HIPREC_TVBR_ACT_RELU: return h > 0.f ? 1.0f : 0.f;
    case HIPREC_TVBR_ACT_LRELU: return h > 0.f ? 1.0f : 0.01f;
    default: return pre > 0.f ? 1.0f : slope;
  }
}

// h(prior)[r, d] = act(base[r, d] + Tb[t_r, d]) and h(post)[r, d] = act(base[r, d] + Tb[t_r + 1, d]); a t outside
// [0, T) sets HIPREC_STATUS_TIME_OOB and leaves a zero row.  hpri may be NULL (eval mode wants the posterior only).
struct TvActJob {
  const float *base, *Tb, *slope;
  float *hpri, *hpost;
  int64_t R;
  int side, ldh;
};
struct TvAct {
  int n;
  TvActJob job[4];
  TvRows rows;
  int D, T, act;
};

__global__ __launch_bounds__(kBlock) void tv_act_kernel(TvAct a, hiprec_stats* stats) {
  const int D = a.D;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int j = 0; j < a.n; ++j) {
    const TvActJob& jb = a.job[j];
    const float slope = jb.slope ? load_scalar_param(jb.slope) : 0.f;
    const int64_t n = jb.R * D;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
      const int64_t r = e / D;
      const int d = static_cast<int>(e - r * D);
      const int64_t t = tv_time(a.rows, jb.side, r);
      float hp = 0.f, hq = 0.f;
      if (tv_in_range(t, a.T)) {
        const float b = jb.base[e];
        hp = tv_act(a.act, b + jb.Tb[t * D + d], slope);
        hq = tv_act(a.act, b + jb.Tb[(t + 1) * D + d], slope);
      } else if (d == 0) {
        atomicOr(&stats->status, HIPREC_STATUS_TIME_OOB);
      }
      if (jb.hpri) jb.hpri[r * jb.ldh + d] = hp;
      jb.hpost[r * jb.ldh + d] = hq;
    }
  }
}

// ---- 4. the loss stage --------------------------------------------------------------------------------------------------
// H / dH of a side: four planes [R, D] at stride P: 0 mean(prior), 1 mean(post), 2 std-encoder(prior), 3 std-encoder(post)
struct TvLoss {
  const float *H_u, *H_i;
  float *dH_u, *dH_i;
  int64_t P_u, P_i;
  const float* noise;           // [3B (1 + n_neg), D]: pos_u, pos_i_1, pos_i_2, neg_u, neg_i_1, neg_i_2
  const float *emb_u, *emb_i;
  float *g_emb_u, *g_emb_i;
  TvRows rows;
  int64_t B, U, I;
  int n_neg, D, T;
  float alpha, scale, inv_scale;
};

// lane's columns c = lane + 64 k of one encoded row
struct TvRow {
  float dm[kTvNpl];    // mean(post) - mean(prior)
  float v1[kTvNpl];    // std(prior)^2 + esp
  float sp2[kTvNpl];   // std(prior)^2
  float sq[kTvNpl];    // std(post) = exp(0.5 h)
  float se[kTvNpl];    // eps exp(0.5 std(post)): reparameterize is handed std as if it were a log-variance
  float z[kTvNpl], t[kTvNpl];
};

__device__ __forceinline__ void tv_load_row(const float* __restrict__ H, int64_t P, int64_t r,
                                            const float* __restrict__ noise, int64_t nr, const float* __restrict__ emb,
                                            int64_t id, int D, int lane, TvRow& v) {
#pragma unroll
  for (int k = 0; k < kTvNpl; ++k) {
    const int c = lane + kWave * k;
    const bool in = c < D;
    const int64_t o = r * D + c;
    const float mp = in ? H[o] : 0.f, mq = in ? H[P + o] : 0.f;
    const float hp = in ? H[2 * P + o] : 0.f, hq = in ? H[3 * P + o] : 0.f;
    const float eps = in ? noise[nr * D + c] : 0.f;
    v.t[k] = in ? emb[id * D + c] : 0.f;
    const float sp = expf(0.5f * hp);
    v.sq[k] = expf(0.5f * hq);
    v.sp2[k] = sp * sp;
    v.v1[k] = v.sp2[k] + kTvEsp;
    v.dm[k] = mq - mp;
    v.se[k] = expf(0.5f * v.sq[k]) * eps;
    v.z[k] = mq + v.se[k];
  }
}

__device__ __forceinline__ float tv_dot(const TvRow& a, const TvRow& b) {
  float d = 0.f;
#pragma unroll
  for (int k = 0; k < kTvNpl; ++k) d += a.z[k] * b.z[k] + a.t[k] * b.t[k];
  return d;
}

// With dz / dt = d rec / d (z | table half) of the row: its KL term (kl_w = -0.5 / rows of its mean, divided by
// `scale` so that the partials' common factor gives kl_loss) joins kl_lane, the derivative with respect to the row's
// four activations is stored, and the table half goes to the gradient with row atomics.
__device__ __forceinline__ void tv_finish_row(float* __restrict__ dH, int64_t P, int64_t r, float* __restrict__ g_emb,
                                              int64_t id, int D, int lane, const TvRow& v, const float* dz,
                                              const float* dt, float oma, float akl, float kl_w, float& kl_lane) {
#pragma unroll
  for (int k = 0; k < kTvNpl; ++k) {
    const int c = lane + kWave * k;
    if (c < D) {
      const float sq2 = v.sq[k] * v.sq[k];
      const float v2 = sq2 + kTvEsp, r2 = 1.0f / v2, dm = v.dm[k], v1 = v.v1[k];
      // log(v2 / v1) - 1 + v1 / v2 = x - log1p(x) at x = (v1 - v2) / v2: the reference's three terms of magnitude 1
      // cancel where prior and posterior are close (its own fp32 kl_loss is up to 4e-5 of its value off); this form
      // keeps the error relative to x
      const float x = (v1 - v2) * r2;
      kl_lane += kl_w * 0.5f * (x - log1pf(x) + dm * r2 * dm);
      const float g_m = akl * dm * r2, rec = oma * dz[k];
      const int64_t o = r * D + c;
      dH[o] = -g_m;
      dH[P + o] = rec + g_m;
      dH[2 * P + o] = akl * 0.5f * (r2 - 1.0f / v1) * v.sp2[k];
      dH[3 * P + o] = rec * v.se[k] * 0.25f * v.sq[k] + akl * 0.5f * (r2 - v1 * r2 * r2 - dm * dm * r2 * r2) * sq2;
      atomic_add_f32(g_emb + id * D + c, oma * dt[k]);
    }
  }
}

__device__ __forceinline__ void tv_zero_row(float* __restrict__ dH, int64_t P, int64_t r, int D, int lane) {
  for (int c = lane; c < D; c += kWave) {
    const int64_t o = r * D + c;
    dH[o] = dH[P + o] = dH[2 * P + o] = dH[3 * P + o] = 0.f;
  }
}

__global__ __launch_bounds__(kBlock) void tv_loss_kernel(TvLoss a, hiprec_stats* stats, Scratch* scratch) {
  const int lane = lane_id();
  const int D = a.D, n_neg = a.n_neg;
  const int64_t B = a.B, Bn = B * n_neg;
  const float oma = 1.0f - a.alpha;
  // kl_loss = -0.5 sum of six means, NOT divided by the batch (tvbr.py:365)
  const float klm_pos = -0.5f / static_cast<float>(B), klm_neg = n_neg ? -0.5f / static_cast<float>(Bn) : 0.f;
  const float akl_pos = a.alpha * klm_pos, akl_neg = a.alpha * klm_neg;
  const float klw_pos = klm_pos * a.inv_scale, klw_neg = klm_neg * a.inv_scale;

  const bool stepper = blockIdx.x == 0 && threadIdx.x == 0;
  StepState step_state{};
  if (stepper) step_state = step_load(stats);

  float gen = 0.f, kl_lane = 0.f;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); t < B;
       t += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const int64_t u = a.rows.ids[0][t], i1 = a.rows.ids[1][t], i2 = a.rows.ids[2][t];
    const bool u_ok = tv_in_range(u, a.U), i_ok = tv_in_range(i1, a.I) && tv_in_range(i2, a.I);
    const bool t_ok = tv_in_range(a.rows.pos_t[t], a.T);
    if (!(u_ok && i_ok && t_ok)) {  // the whole triple is dropped; its rows of d h are still this wave's to write
      if (lane == 0)
        atomicOr(&stats->status, (u_ok ? 0u : HIPREC_STATUS_USER_OOB) | (i_ok ? 0u : HIPREC_STATUS_ITEM_OOB) |
                                     (t_ok ? 0u : HIPREC_STATUS_TIME_OOB));
      tv_zero_row(a.dH_u, a.P_u, t, D, lane);
      tv_zero_row(a.dH_i, a.P_i, t, D, lane);
      tv_zero_row(a.dH_i, a.P_i, B + t, D, lane);
      for (int j = 0; j < n_neg; ++j) {
        const int64_t qn = t * n_neg + j;
        tv_zero_row(a.dH_u, a.P_u, B + qn, D, lane);
        tv_zero_row(a.dH_i, a.P_i, 2 * B + qn, D, lane);
        tv_zero_row(a.dH_i, a.P_i, 2 * B + Bn + qn, D, lane);
      }
      continue;
    }
    TvRow pu, p1, p2;
    tv_load_row(a.H_u, a.P_u, t, a.noise, t, a.emb_u, u, D, lane, pu);
    tv_load_row(a.H_i, a.P_i, t, a.noise, B + t, a.emb_i, i1, D, lane, p1);
    tv_load_row(a.H_i, a.P_i, B + t, a.noise, 2 * B + t, a.emb_i, i2, D, lane, p2);
    // positives: each vector against the SUM of the other two (tvbr.py:338-358)
    float xu = 0.f, x1 = 0.f, x2 = 0.f;
#pragma unroll
    for (int k = 0; k < kTvNpl; ++k) {
      xu += pu.z[k] * (p1.z[k] + p2.z[k]) + pu.t[k] * (p1.t[k] + p2.t[k]);
      x1 += p1.z[k] * (pu.z[k] + p2.z[k]) + p1.t[k] * (pu.t[k] + p2.t[k]);
      x2 += p2.z[k] * (pu.z[k] + p1.z[k]) + p2.t[k] * (pu.t[k] + p1.t[k]);
    }
    xu = wave_sum(xu);
    x1 = wave_sum(x1);
    x2 = wave_sum(x2);
    float su, s1, s2;
    gen += neg_logsigmoid(xu, &su);
    gen += neg_logsigmoid(x1, &s1);
    gen += neg_logsigmoid(x2, &s2);
    const float au = -su * a.scale, a1 = -s1 * a.scale, a2 = -s2 * a.scale;
    float dzu[kTvNpl], dtu[kTvNpl], dz1[kTvNpl], dt1[kTvNpl], dz2[kTvNpl], dt2[kTvNpl];
#pragma unroll
    for (int k = 0; k < kTvNpl; ++k) {
      dzu[k] = au * (p1.z[k] + p2.z[k]) + a1 * p1.z[k] + a2 * p2.z[k];
      dtu[k] = au * (p1.t[k] + p2.t[k]) + a1 * p1.t[k] + a2 * p2.t[k];
      dz1[k] = au * pu.z[k] + a1 * (pu.z[k] + p2.z[k]) + a2 * p2.z[k];
      dt1[k] = au * pu.t[k] + a1 * (pu.t[k] + p2.t[k]) + a2 * p2.t[k];
      dz2[k] = au * pu.z[k] + a1 * p1.z[k] + a2 * (pu.z[k] + p1.z[k]);
      dt2[k] = au * pu.t[k] + a1 * p1.t[k] + a2 * (pu.t[k] + p1.t[k]);
    }
    // negatives: each against the triple's OWN vector of its kind (tvbr.py:343-361); the three of one j share a t
    for (int j = 0; j < n_neg; ++j) {
      const int64_t qn = t * n_neg + j;
      const bool tn_ok = tv_in_range(a.rows.neg_t[qn], a.T);
      if (!tn_ok && lane == 0) atomicOr(&stats->status, HIPREC_STATUS_TIME_OOB);
#pragma unroll
      for (int kind = 0; kind < 3; ++kind) {
        const bool user = kind == 0;
        const int64_t id = a.rows.ids[3 + kind][qn];
        const int64_t r = user ? B + qn : 2 * B + (kind == 2 ? Bn : 0) + qn;
        const int64_t nr = 3 * B + kind * Bn + qn;
        float* dH = user ? a.dH_u : a.dH_i;
        const int64_t P = user ? a.P_u : a.P_i;
        const bool id_ok = tv_in_range(id, user ? a.U : a.I);
        if (!(id_ok && tn_ok)) {
          if (!id_ok && lane == 0) atomicOr(&stats->status, user ? HIPREC_STATUS_USER_OOB : HIPREC_STATUS_ITEM_OOB);
          tv_zero_row(dH, P, r, D, lane);
          continue;
        }
        const TvRow& p = kind == 0 ? pu : (kind == 1 ? p1 : p2);
        float* dzp = kind == 0 ? dzu : (kind == 1 ? dz1 : dz2);
        float* dtp = kind == 0 ? dtu : (kind == 1 ? dt1 : dt2);
        TvRow nv;
        tv_load_row(user ? a.H_u : a.H_i, P, r, a.noise, nr, user ? a.emb_u : a.emb_i, id, D, lane, nv);
        const float y = wave_sum(tv_dot(nv, p));
        float sy;  // neg_logsigmoid(-y) = -logsigmoid(-y), and sigmoid(y) next to it
        gen += neg_logsigmoid(-y, &sy);
        const float b = sy * a.scale;
        float dzn[kTvNpl], dtn[kTvNpl];
#pragma unroll
        for (int k = 0; k < kTvNpl; ++k) {
          dzp[k] += b * nv.z[k];
          dtp[k] += b * nv.t[k];
          dzn[k] = b * p.z[k];
          dtn[k] = b * p.t[k];
        }
        tv_finish_row(dH, P, r, user ? a.g_emb_u : a.g_emb_i, id, D, lane, nv, dzn, dtn, oma, akl_neg, klw_neg, kl_lane);
      }
    }
    tv_finish_row(a.dH_u, a.P_u, t, a.g_emb_u, u, D, lane, pu, dzu, dtu, oma, akl_pos, klw_pos, kl_lane);
    tv_finish_row(a.dH_i, a.P_i, t, a.g_emb_i, i1, D, lane, p1, dz1, dt1, oma, akl_pos, klw_pos, kl_lane);
    tv_finish_row(a.dH_i, a.P_i, B + t, a.g_emb_i, i2, D, lane, p2, dz2, dt2, oma, akl_pos, klw_pos, kl_lane);
  }
  publish_partials<kWavesPerBlock>(gen, kl_lane, 0.f, a.scale, scratch);   // loss = rec_loss, reg = kl_loss
  if (stepper) step_store_advanced(stats, step_state);
}

// ---- 5. activation backward, d base and the dTb reduction ---------------------------------------------------------------
// Blocks [0, nb[0]) walk the user rows, the rest the item rows; a wave owns a contiguous stretch of its side's rows and
// both encoders (mean, std) of each.  d base = d pre(prior) + d pre(post) replaces plane 2 * kind of dH.
// dTb[t] += d pre(prior) and dTb[t + 1] += d pre(post) for ARBITRARY per-row t: a wave adds the rows of a run of equal t
// in registers and sends a finished run off with atomics; the run each wave still holds at the end meets the other
// waves' in LDS, where runs of the same t are added before the block's one set of atomics.  In the epoch loop every
// row of a step shares one t: each block then sends ONE row pair per encoder.
struct TvBwd {
  const float* H[2];
  float* dH[2];
  int64_t P[2], R[2];
  const float* base[4];
  const float* Tb[4];
  float* dTb[4];
  const float* slope[4];
  float* g_slope[4];
  int nb[2];
  TvRows rows;
  int D, T, act;
};

__device__ __forceinline__ void tv_flush_run(const TvBwd& a, int side, int64_t t, int lane,
                                             float (&acc)[2][2][kTvNpl]) {
#pragma unroll
  for (int kind = 0; kind < 2; ++kind)
#pragma unroll
    for (int pp = 0; pp < 2; ++pp)
#pragma unroll
      for (int k = 0; k < kTvNpl; ++k) {
        const int c = lane + kWave * k;
        if (c < a.D) atomic_add_f32(a.dTb[2 * side + kind] + (t + pp) * a.D + c, acc[kind][pp][k]);
        acc[kind][pp][k] = 0.f;
      }
}

__global__ __launch_bounds__(kBlock) void tv_bwd_kernel(TvBwd a) {
  __shared__ float s_acc[kWavesPerBlock][2][2][kTvMaxDim];
  __shared__ long long s_t[kWavesPerBlock];
  const int lane = lane_id(), wv = wave_in_block(), D = a.D;
  const int side = static_cast<int>(blockIdx.x) < a.nb[0] ? 0 : 1;
  const int blk = side ? static_cast<int>(blockIdx.x) - a.nb[0] : static_cast<int>(blockIdx.x);
  const int64_t R = a.R[side], P = a.P[side];
  const int64_t n_waves = static_cast<int64_t>(a.nb[side]) * kWavesPerBlock;
  const int64_t per = (R + n_waves - 1) / n_waves;
  const int64_t first = (static_cast<int64_t>(blk) * kWavesPerBlock + wv) * per;
  const int64_t r0 = first < R ? first : R, r1 = r0 + per < R ? r0 + per : R;
  const float* __restrict__ H = a.H[side];
  float* __restrict__ dH = a.dH[side];
  const bool prelu = a.act == HIPREC_TVBR_ACT_PRELU;
  float slope[2] = {0.f, 0.f}, dslope[2] = {0.f, 0.f};
  if (prelu) {
    slope[0] = load_scalar_param(a.slope[2 * side]);
    slope[1] = load_scalar_param(a.slope[2 * side + 1]);
  }
  float acc[2][2][kTvNpl] = {};
  int64_t cur_t = -1;
  // kTvBwdUnroll rows are loaded together (a row's loads depend on nothing but r), then taken in order
  for (int64_t rb = r0; rb < r1; rb += kTvBwdUnroll) {
    int64_t tt[kTvBwdUnroll];
    float gp[kTvBwdUnroll][2][kTvNpl], gq[kTvBwdUnroll][2][kTvNpl], hp[kTvBwdUnroll][2][kTvNpl],
        hq[kTvBwdUnroll][2][kTvNpl];
#pragma unroll
    for (int j = 0; j < kTvBwdUnroll; ++j) {
      const int64_t r = rb + j < r1 ? rb + j : r1 - 1;
      tt[j] = tv_time(a.rows, side, r);
#pragma unroll
      for (int kind = 0; kind < 2; ++kind)
#pragma unroll
        for (int k = 0; k < kTvNpl; ++k) {
          const int c = lane + kWave * k;
          const int64_t op = 2 * kind * P + r * D + (c < D ? c : 0), oq = op + P;
          gp[j][kind][k] = dH[op];
          gq[j][kind][k] = dH[oq];
          hp[j][kind][k] = H[op];
          hq[j][kind][k] = H[oq];
        }
    }
#pragma unroll
    for (int j = 0; j < kTvBwdUnroll; ++j) {
      const int64_t r = rb + j, t = tt[j];
      if (r >= r1) break;
      const bool t_ok = tv_in_range(t, a.T);   // a row with a bad t was dropped by the loss stage: its d h is zero
      if (t_ok && t != cur_t) {
        if (cur_t >= 0) tv_flush_run(a, side, cur_t, lane, acc);
        cur_t = t;
      }
#pragma unroll
      for (int kind = 0; kind < 2; ++kind) {
        const int e = 2 * side + kind;
#pragma unroll
        for (int k = 0; k < kTvNpl; ++k) {
          const int c = lane + kWave * k;
          if (c >= D) continue;
          const int64_t o = r * D + c, op = 2 * kind * P + o;
          if (!t_ok) {
            dH[op] = 0.f;
            continue;
          }
          float pre_p = 0.f, pre_q = 0.f;
          if (prelu) {
            const float b = a.base[e][o];
            pre_p = b + a.Tb[e][t * D + c];
            pre_q = b + a.Tb[e][(t + 1) * D + c];
          }
          const float dp = gp[j][kind][k] * tv_act_grad(a.act, hp[j][kind][k], pre_p, slope[kind]);
          const float dq = gq[j][kind][k] * tv_act_grad(a.act, hq[j][kind][k], pre_q, slope[kind]);
          if (prelu)
            dslope[kind] += (pre_p > 0.f ? 0.f : gp[j][kind][k] * pre_p) + (pre_q > 0.f ? 0.f : gq[j][kind][k] * pre_q);
          dH[op] = dp + dq;
          acc[kind][0][k] += dp;
          acc[kind][1][k] += dq;
        }
      }
    }
  }
  if (prelu) {   // one atomic per wave and slope
#pragma unroll
    for (int kind = 0; kind < 2; ++kind) {
      const float s = wave_sum(dslope[kind]);
      if (lane == 0 && r1 > r0) atomic_add_f32(a.g_slope[2 * side + kind], s);
    }
  }
  // the waves' last runs meet in LDS
  if (lane == 0) s_t[wv] = cur_t;
#pragma unroll
  for (int kind = 0; kind < 2; ++kind)
#pragma unroll
    for (int pp = 0; pp < 2; ++pp)
#pragma unroll
      for (int k = 0; k < kTvNpl; ++k) s_acc[wv][kind][pp][lane + kWave * k] = acc[kind][pp][k];
  lds_barrier();
  for (int i = threadIdx.x; i < 4 * D; i += kBlock) {
    const int kp = i / D, c = i - kp * D, kind = kp >> 1, pp = kp & 1;
    for (int w = 0; w < kWavesPerBlock; ++w) {
      const long long t = s_t[w];
      if (t < 0) continue;
      bool first = true;
      for (int v = 0; v < w; ++v) first = first && s_t[v] != t;
      if (!first) continue;
      float s = 0.f;
      for (int v = w; v < kWavesPerBlock; ++v)
        if (s_t[v] == t) s += s_acc[v][kind][pp][c];
      atomic_add_f32(a.dTb[2 * side + kind] + (t + pp) * D + c, s);
    }
  }
}

// ---- 7. the four tables' row gradients -------------------------------------------------------------------------------------
struct TvScatter {
  const float* dtab[4];
  float* g_tab[4];
  int64_t R[2], n_ids[2];
  TvRows rows;
  int D;
};

__global__ __launch_bounds__(kBlock) void tv_scatter_kernel(TvScatter a) {
  const int lane = lane_id();
  const int64_t n_rows = a.R[0] + a.R[1];
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); q < n_rows;
       q += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const int side = q < a.R[0] ? 0 : 1;
    const int64_t r = side ? q - a.R[0] : q;
    const int64_t id = tv_id(a.rows, side, r);
    if (!tv_in_range(id, a.n_ids[side])) continue;   // flagged by the gather
    for (int kind = 0; kind < 2; ++kind)
      for (int c = lane; c < a.D; c += kWave)
        atomic_add_f32(a.g_tab[2 * side + kind] + id * a.D + c, a.dtab[2 * side + kind][r * a.D + c]);
  }
}

// ---- 8. d time_embdding[tau, k] = sum_e sum_d dTb_e[tau, d] W_e[d, D + k]: the only writer of that gradient --------------
struct TvTimeGrad {
  const float* dTb[4];
  const float* W[4];
  int K[4];
  float* g_time;
  int D, T1;
};

// One block per (time row tau, 64 columns k).  The row's four dTb slices go to LDS first; a row that is exactly zero
// there -- in the epoch loop every time row but t and t + 1 -- writes zeros and is done (no loads of W, an exactly zero
// gradient whatever W holds).  Otherwise lanes run over k (coalesced rows of W), the four waves split the columns d and
// meet in LDS.
__global__ __launch_bounds__(kBlock) void tv_time_grad_kernel(TvTimeGrad a) {
  __shared__ float s_d[4][kTvMaxDim];
  __shared__ float s_part[kWavesPerBlock][kWave];
  const int tau = blockIdx.x, k0 = blockIdx.y * kWave, lane = lane_id(), wv = wave_in_block();
  const int D = a.D, T1 = a.T1;
  int any = 0;
  for (int i = threadIdx.x; i < 4 * D; i += kBlock) {
    const int e = i / D, c = i - e * D;
    const float v = a.dTb[e][tau * D + c];
    s_d[e][c] = v;
    any |= v != 0.f;
  }
  const bool live = __syncthreads_or(any);
  const int k = k0 + lane < T1 ? k0 + lane : T1 - 1;
  float s = 0.f;
  if (live) {
    for (int e = 0; e < 4; ++e) {
      const float* __restrict__ w = a.W[e] + D + k;
      const int64_t ldw = a.K[e];
#pragma unroll 8
      for (int c = wv; c < D; c += kWavesPerBlock) s += s_d[e][c] * w[c * ldw];
    }
  }
  s_part[wv][lane] = s;
  __syncthreads();
  if (wv == 0 && k0 + lane < T1)
    a.g_time[tau * T1 + k0 + lane] = (s_part[0][lane] + s_part[1][lane]) + (s_part[2][lane] + s_part[3][lane]);
}

// scores[k] = <eu[k], ei[k]> over `width` columns (TVBR.predict, tvbr.py:402-412)
__global__ __launch_bounds__(kBlock) void tv_rowdot_kernel(const float* __restrict__ eu, const float* __restrict__ ei,
                                                           int64_t n, int width, float* __restrict__ scores) {
  const int lane = lane_id();
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); q < n;
       q += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    float d = 0.f;
    for (int c = lane; c < width; c += kWave) d += eu[q * width + c] * ei[q * width + c];
    d = wave_sum(d);
    if (lane == 0) scores[q] = d;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// pointers into a flat buffer laid out in state_dict() order; encoders e = 0..3 = time2mean_u, time2std_u, time2mean_i,
// time2std_i; tab[e] = user_mean, user_std, item_mean, item_std; slope[e] = the PReLU weight (prelu only)
struct TvParams {
  float* emb[2];
  float* time;
  float *tab[4], *W[4], *b[4], *slope[4];
};

int tv_K(const hiprec_tvbr_shape& s, int side) { return s.emb_dim + s.time_step + 1 + (side == 0 ? s.fea_u : s.fea_i); }

int64_t tv_n_params(const hiprec_tvbr_shape& s) {
  const int64_t D = s.emb_dim, T1 = s.time_step + 1, UI = s.n_users + s.n_items;
  int64_t n = 3 * UI * D + T1 * T1;
  for (int e = 0; e < 4; ++e) n += D * tv_K(s, e >> 1) + D + (s.act == HIPREC_TVBR_ACT_PRELU ? 1 : 0);
  return n;
}

TvParams tv_params(float* base, const hiprec_tvbr_shape& s) {
  TvParams p{};
  const int64_t D = s.emb_dim, T1 = s.time_step + 1;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += n; return r; };
  p.emb[0] = take(s.n_users * D);
  p.emb[1] = take(s.n_items * D);
  p.time = take(T1 * T1);
  p.tab[0] = take(s.n_users * D);
  p.tab[1] = take(s.n_users * D);
  p.tab[2] = take(s.n_items * D);
  p.tab[3] = take(s.n_items * D);
  for (int e = 0; e < 4; ++e) {
    p.W[e] = take(D * tv_K(s, e >> 1));
    p.b[e] = take(D);
    p.slope[e] = s.act == HIPREC_TVBR_ACT_PRELU ? take(1) : nullptr;
  }
  return p;
}

struct TvWorkspace {
  float *Tb[4], *dTb[4];               // dTb[0..3] contiguous: one memset
  float *X[4], *base[4], *dtab[4], *cs[4];
  float *H[2], *dH[2];
  int64_t P[2], dTb_floats, floats;
};

TvWorkspace tv_carve(float* base, const hiprec_tvbr_shape& s, int64_t B, int n_neg) {
  TvWorkspace w{};
  const int64_t D = s.emb_dim, T1 = s.time_step + 1;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += (n + 3) / 4 * 4; return r; };
  for (int e = 0; e < 4; ++e) w.Tb[e] = take(T1 * D);
  for (int e = 0; e < 4; ++e) w.dTb[e] = take(T1 * D);
  w.dTb_floats = 4 * ((T1 * D + 3) / 4 * 4);
  for (int side = 0; side < 2; ++side) {
    const int64_t R = (side + 1) * B * (1 + n_neg), K = tv_K(s, side);
    w.P[side] = (R * D + 3) / 4 * 4;
    w.H[side] = take(4 * w.P[side]);
    w.dH[side] = take(4 * w.P[side]);
    for (int kind = 0; kind < 2; ++kind) {
      const int e = 2 * side + kind;
      w.X[e] = take(R * K);
      w.base[e] = take(R * D);
      w.dtab[e] = take(R * D);
      w.cs[e] = take(colsum_ws_floats(static_cast<int>(R), static_cast<int>(D)));
    }
  }
  w.floats = c - base;
  return w;
}

int tv_check_shape(const hiprec_tvbr_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  HIPREC_REQUIRE(s->n_users >= 1 && s->n_items >= 1, "TVBR needs n_users >= 1 and n_items >= 1");
  HIPREC_REQUIRE(s->emb_dim >= 1 && s->emb_dim <= kTvMaxDim, "TVBR needs 1 <= emb_dim <= %d (got %d)", kTvMaxDim,
                 s->emb_dim);
  HIPREC_REQUIRE(s->time_step >= 1 && s->time_step <= kTvMaxTime, "TVBR needs 1 <= time_step <= %d (got %d)", kTvMaxTime,
                 s->time_step);
  HIPREC_REQUIRE(s->fea_u >= 1 && s->fea_u <= kTvMaxFea && s->fea_i >= 1 && s->fea_i <= kTvMaxFea,
                 "TVBR needs feature widths in 1 .. %d (got %d and %d)", kTvMaxFea, s->fea_u, s->fea_i);
  HIPREC_REQUIRE(s->act >= HIPREC_TVBR_ACT_TANH && s->act <= HIPREC_TVBR_ACT_PRELU, "unknown activation %d", s->act);
  return 0;
}

// the grouped GEMM indexes its operands with ints: every [rows, width] operand of a step must stay below 2^31 elements
bool tv_rows_ok(const hiprec_tvbr_shape& s, int64_t rows) {
  const int64_t widest = std::max(tv_K(s, 0), tv_K(s, 1));
  return rows >= 1 && rows < (1ll << 24) && rows * widest < (1ll << 31);
}

int tv_launch_act(const TvAct& a, hiprec_stats* stats, hipStream_t st) {
  int64_t n = 0;
  for (int j = 0; j < a.n; ++j) n = std::max(n, a.job[j].R * a.D);
  tv_act_kernel<<<grid_for_threads(n), kBlock, 0, st>>>(a, stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

int tv_train(const hiprec_tvbr_shape& s, float* w_flat, float* g_flat, const float* fea_u, const float* fea_i,
             const TvRows& rows, int n_neg, const float* noise, float alpha, float scale, hiprec_stats* stats,
             Scratch* scratch, float* ws_base, hipStream_t st) {
  const int D = s.emb_dim, T = s.time_step, T1 = T + 1;
  const int64_t B = rows.B, Bn = rows.Bn;
  const int64_t R[2] = {B + Bn, 2 * (B + Bn)};
  const int K[2] = {tv_K(s, 0), tv_K(s, 1)};
  const TvParams w = tv_params(w_flat, s), g = tv_params(g_flat, s);
  const TvWorkspace a = tv_carve(ws_base, s, B, n_neg);
  HIPREC_TRY(hipMemsetAsync(a.dTb[0], 0, sizeof(float) * a.dTb_floats, st));

  TvGather ga{};
  ga.rows = rows;
  ga.fea[0] = fea_u; ga.fea[1] = fea_i;
  ga.F[0] = s.fea_u; ga.F[1] = s.fea_i;
  ga.n_ids[0] = s.n_users; ga.n_ids[1] = s.n_items;
  ga.D = D; ga.T1 = T1; ga.kinds = 2;
  for (int e = 0; e < 4; ++e) {
    ga.tab[e >> 1][e & 1] = w.tab[e];
    ga.X[e >> 1][e & 1] = a.X[e];
  }
  ga.R[0] = R[0]; ga.R[1] = R[1];
  tv_gather_kernel<<<grid_for_waves(R[0] + R[1]), kBlock, 0, st>>>(ga, stats);
  HIPREC_TRY(hipGetLastError());

  {
    GemmGroup q{};
    for (int e = 0; e < 4; ++e) {
      const int side = e >> 1, Rs = static_cast<int>(R[side]), Ks = K[side];
      q.p[q.n++] = make_gemm(kNT, Rs, D, Ks, a.X[e], Ks, w.W[e], Ks, a.base[e], D, w.b[e], 0, nullptr, 0, false);
      q.p[q.n++] = make_gemm(kNT, T1, D, T1, w.time, T1, w.W[e] + D, Ks, a.Tb[e], D, nullptr, 0, nullptr, 0, false);
    }
    if (int rc = launch_group(q, st)) return rc;
  }

  TvAct ac{};
  ac.rows = rows; ac.D = D; ac.T = T; ac.act = s.act;
  for (int e = 0; e < 4; ++e) {
    const int side = e >> 1, kind = e & 1;
    TvActJob& jb = ac.job[ac.n++];
    jb.base = a.base[e]; jb.Tb = a.Tb[e]; jb.slope = w.slope[e];
    jb.hpri = a.H[side] + 2 * kind * a.P[side];
    jb.hpost = jb.hpri + a.P[side];
    jb.R = R[side]; jb.side = side; jb.ldh = D;
  }
  if (int rc = tv_launch_act(ac, stats, st)) return rc;

  TvLoss lo{};
  lo.H_u = a.H[0]; lo.H_i = a.H[1];
  lo.dH_u = a.dH[0]; lo.dH_i = a.dH[1];
  lo.P_u = a.P[0]; lo.P_i = a.P[1];
  lo.noise = noise;
  lo.emb_u = w.emb[0]; lo.emb_i = w.emb[1];
  lo.g_emb_u = g.emb[0]; lo.g_emb_i = g.emb[1];
  lo.rows = rows;
  lo.B = B; lo.U = s.n_users; lo.I = s.n_items;
  lo.n_neg = n_neg; lo.D = D; lo.T = T;
  lo.alpha = alpha; lo.scale = scale; lo.inv_scale = 1.0f / scale;
  tv_loss_kernel<<<grid_for_waves(B), kBlock, 0, st>>>(lo, stats, scratch);
  HIPREC_TRY(hipGetLastError());

  TvBwd bw{};
  bw.rows = rows; bw.D = D; bw.T = T; bw.act = s.act;
  for (int side = 0; side < 2; ++side) {
    bw.H[side] = a.H[side]; bw.dH[side] = a.dH[side];
    bw.P[side] = a.P[side]; bw.R[side] = R[side];
    const int64_t nb = (R[side] + kTvBwdRows * kWavesPerBlock - 1) / (kTvBwdRows * kWavesPerBlock);
    bw.nb[side] = static_cast<int>(std::min<int64_t>(std::max<int64_t>(nb, 1), kTvBwdMaxBlocks));
  }
  for (int e = 0; e < 4; ++e) {
    bw.base[e] = a.base[e]; bw.Tb[e] = a.Tb[e]; bw.dTb[e] = a.dTb[e];
    bw.slope[e] = w.slope[e]; bw.g_slope[e] = g.slope[e];
  }
  tv_bwd_kernel<<<bw.nb[0] + bw.nb[1], kBlock, 0, st>>>(bw);
  HIPREC_TRY(hipGetLastError());

  {
    GemmGroup q{};
    for (int e = 0; e < 4; ++e) {
      const int side = e >> 1, Rs = static_cast<int>(R[side]), Ks = K[side];
      const float* dbase = a.dH[side] + 2 * (e & 1) * a.P[side];
      q.p[q.n++] = make_gemm(kTNm, D, Ks, Rs, dbase, D, a.X[e], Ks, g.W[e], Ks, nullptr, 0, nullptr, 0, true);
      q.p[q.n++] = make_colsum(dbase, Rs, D, D, g.b[e], a.cs[e]);
      q.p[q.n++] = make_gemm(kNN, Rs, D, D, dbase, D, w.W[e], Ks, a.dtab[e], D, nullptr, 0, nullptr, 0, false);
    }
    if (int rc = launch_group(q, st)) return rc;
    if (int rc = launch_colsum_reduce(q, st)) return rc;
  }

  TvScatter sc{};
  sc.rows = rows; sc.D = D;
  sc.R[0] = R[0]; sc.R[1] = R[1];
  sc.n_ids[0] = s.n_users; sc.n_ids[1] = s.n_items;
  for (int e = 0; e < 4; ++e) {
    sc.dtab[e] = a.dtab[e];
    sc.g_tab[e] = g.tab[e];
  }
  tv_scatter_kernel<<<grid_for_waves(R[0] + R[1]), kBlock, 0, st>>>(sc);
  HIPREC_TRY(hipGetLastError());

  {  // after the weight gradients: their time columns hold exact zeros (X's are zero) that this launch builds on
    GemmGroup q{};
    for (int e = 0; e < 4; ++e)
      q.p[q.n++] = make_gemm(kTNm, D, T1, T1, a.dTb[e], D, w.time, T1, g.W[e] + D, K[e >> 1], nullptr, 0, nullptr, 0,
                             true);
    if (int rc = launch_group(q, st)) return rc;
  }
  TvTimeGrad tg{};
  for (int e = 0; e < 4; ++e) {
    tg.dTb[e] = a.dTb[e];
    tg.W[e] = w.W[e];
    tg.K[e] = K[e >> 1];
  }
  tg.g_time = g.time; tg.D = D; tg.T1 = T1;
  tv_time_grad_kernel<<<dim3(T1, (T1 + kWave - 1) / kWave), kBlock, 0, st>>>(tg);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

int64_t tv_encode_ws_floats(const hiprec_tvbr_shape& s, int64_t n) {
  const int64_t rows = std::min<int64_t>(n, kTvChunk), K = std::max(tv_K(s, 0), tv_K(s, 1));
  const int64_t D = s.emb_dim, T1 = s.time_step + 1;
  return (rows * K + 3) / 4 * 4 + (rows * D + 3) / 4 * 4 + (T1 * D + 3) / 4 * 4;
}

// out[k] = [posterior mean of ids[k] at t = time_step | emb[ids[k]]] for one side, kTvChunk rows per pass
int tv_encode(const hiprec_tvbr_shape& s, const TvParams& w, const float* fea, const int64_t* ids, int64_t n, int side,
              float* out, hiprec_stats* stats, float* ws, hipStream_t st) {
  const int D = s.emb_dim, T = s.time_step, T1 = T + 1, K = tv_K(s, side), e = 2 * side;
  const int64_t max_rows = std::min<int64_t>(n, kTvChunk);
  float* X = ws;
  float* base = X + (max_rows * K + 3) / 4 * 4;
  float* Tb = base + (max_rows * D + 3) / 4 * 4;
  for (int64_t off = 0; off < n; off += kTvChunk) {
    const int64_t m = std::min<int64_t>(n - off, kTvChunk);
    TvRows rows{};
    rows.ids[0] = ids + off;
    rows.fixed_t = T - 1;            // the posterior run reads time row t + 1 = time_step (tvbr.py:380-387)
    TvGather ga{};
    ga.rows = rows;
    ga.R[side] = m;
    ga.n_ids[side] = side == 0 ? s.n_users : s.n_items;
    ga.fea[side] = fea;
    ga.tab[side][0] = w.tab[e];
    ga.X[side][0] = X;
    ga.F[side] = side == 0 ? s.fea_u : s.fea_i;
    ga.D = D; ga.T1 = T1; ga.kinds = 1;
    ga.emb = w.emb[side];
    ga.enc_out = out + off * 2 * D;
    tv_gather_kernel<<<grid_for_waves(m), kBlock, 0, st>>>(ga, stats);
    HIPREC_TRY(hipGetLastError());
    GemmGroup q{};
    q.p[q.n++] = make_gemm(kNT, static_cast<int>(m), D, K, X, K, w.W[e], K, base, D, w.b[e], 0, nullptr, 0, false);
    if (off == 0)
      q.p[q.n++] = make_gemm(kNT, T1, D, T1, w.time, T1, w.W[e] + D, K, Tb, D, nullptr, 0, nullptr, 0, false);
    if (int rc = launch_group(q, st)) return rc;
    TvAct ac{};
    ac.rows = rows; ac.D = D; ac.T = T; ac.act = s.act; ac.n = 1;
    ac.job[0].base = base; ac.job[0].Tb = Tb; ac.job[0].slope = w.slope[e];
    ac.job[0].hpri = nullptr; ac.job[0].hpost = out + off * 2 * D;
    ac.job[0].R = m; ac.job[0].side = side; ac.job[0].ldh = 2 * D;
    if (int rc = tv_launch_act(ac, stats, st)) return rc;
  }
  return 0;
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_tvbr_shape_bytes(void) { return sizeof(hiprec_tvbr_shape); }

extern "C" int64_t hiprec_tvbr_param_floats(const hiprec_tvbr_shape* shape) {
  if (tv_check_shape(shape)) return -1;
  return tv_n_params(*shape);
}

extern "C" size_t hiprec_tvbr_workspace_bytes(const hiprec_tvbr_shape* shape, int64_t batch, int32_t n_neg) {
  if (tv_check_shape(shape) || batch < 1 || n_neg < 0) return 0;
  if (!tv_rows_ok(*shape, 2 * batch * (1 + static_cast<int64_t>(n_neg)))) {
    set_error("a TVBR step of %lld triples x %d negatives is beyond the grouped GEMM's 2^31 elements per operand",
              static_cast<long long>(batch), n_neg);
    return 0;
  }
  return sizeof(float) * static_cast<size_t>(tv_carve(nullptr, *shape, batch, n_neg).floats);
}

extern "C" size_t hiprec_tvbr_encode_workspace_bytes(const hiprec_tvbr_shape* shape, int64_t n, int32_t pairs) {
  if (tv_check_shape(shape) || n < 1) return 0;
  const int64_t rows = std::min<int64_t>(n, kTvChunk);
  int64_t floats = tv_encode_ws_floats(*shape, n);
  if (pairs) floats += 2 * rows * 2 * shape->emb_dim;
  return sizeof(float) * static_cast<size_t>(floats);
}

extern "C" int hiprec_tvbr_grad(const hiprec_tvbr_shape* shape, const float* w_flat, float* g_flat,
                                const float* user_fea, const float* item_fea, const int64_t* pos_u,
                                const int64_t* pos_i1, const int64_t* pos_i2, const int64_t* neg_u,
                                const int64_t* neg_i1, const int64_t* neg_i2, const int64_t* pos_t,
                                const int64_t* neg_t, int64_t batch, int32_t n_neg, const float* noise, float alpha,
                                float scale, hiprec_stats* stats, void* scratch, size_t scratch_bytes, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (int rc = tv_check_shape(shape)) return rc;
  HIPREC_REQUIRE(w_flat && g_flat && user_fea && item_fea && noise && stats && scratch && workspace, "NULL pointer");
  HIPREC_REQUIRE(batch >= 1 && n_neg >= 0, "bad batch / n_neg");
  HIPREC_REQUIRE(scale > 0.f, "scale must be positive");
  HIPREC_REQUIRE(pos_u && pos_i1 && pos_i2 && pos_t, "NULL positive index arrays");
  HIPREC_REQUIRE(n_neg == 0 || (neg_u && neg_i1 && neg_i2 && neg_t), "NULL negative index arrays");
  if (scratch_bytes < kScratchBytes) {
    set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
    return HIPREC_E_SCRATCH;
  }
  const size_t need = hiprec_tvbr_workspace_bytes(shape, batch, n_neg);
  HIPREC_REQUIRE(need > 0, "unsupported batch %lld x n_neg %d", static_cast<long long>(batch), n_neg);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  TvRows rows{};
  rows.ids[0] = pos_u; rows.ids[1] = pos_i1; rows.ids[2] = pos_i2;
  rows.ids[3] = neg_u; rows.ids[4] = neg_i1; rows.ids[5] = neg_i2;
  rows.pos_t = pos_t; rows.neg_t = neg_t;
  rows.B = batch; rows.Bn = batch * n_neg; rows.fixed_t = -1;
  return tv_train(*shape, const_cast<float*>(w_flat), g_flat, user_fea, item_fea, rows, n_neg, noise, alpha, scale,
                  stats, static_cast<Scratch*>(scratch), static_cast<float*>(workspace),
                  static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_tvbr_encode(const hiprec_tvbr_shape* shape, const float* w_flat, const float* fea,
                                  const int64_t* ids, int64_t n, int32_t side, float* out, hiprec_stats* stats,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = tv_check_shape(shape)) return rc;
  HIPREC_REQUIRE(n >= 0 && (side == 0 || side == 1), "bad n / side");
  if (n == 0) return 0;
  HIPREC_REQUIRE(w_flat && fea && ids && out && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(tv_rows_ok(*shape, std::min<int64_t>(n, kTvChunk)), "feature rows too wide for one pass");
  const size_t need = hiprec_tvbr_encode_workspace_bytes(shape, n, 0);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  return tv_encode(*shape, tv_params(const_cast<float*>(w_flat), *shape), fea, ids, n, side, out, stats,
                   static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_tvbr_predict(const hiprec_tvbr_shape* shape, const float* w_flat, const float* user_fea,
                                   const float* item_fea, const int64_t* users, const int64_t* items, int64_t n,
                                   float* scores, hiprec_stats* stats, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  if (int rc = tv_check_shape(shape)) return rc;
  HIPREC_REQUIRE(n >= 0, "negative n");
  if (n == 0) return 0;
  HIPREC_REQUIRE(w_flat && user_fea && item_fea && users && items && scores && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(tv_rows_ok(*shape, std::min<int64_t>(n, kTvChunk)), "feature rows too wide for one pass");
  const size_t need = hiprec_tvbr_encode_workspace_bytes(shape, n, 1);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const TvParams w = tv_params(const_cast<float*>(w_flat), *shape);
  const int D2 = 2 * shape->emb_dim;
  float* ws = static_cast<float*>(workspace);
  float* eu = ws + tv_encode_ws_floats(*shape, n);
  float* ei = eu + std::min<int64_t>(n, kTvChunk) * D2;
  for (int64_t off = 0; off < n; off += kTvChunk) {
    const int64_t m = std::min<int64_t>(n - off, kTvChunk);
    if (int rc = tv_encode(*shape, w, user_fea, users + off, m, 0, eu, stats, ws, st)) return rc;
    if (int rc = tv_encode(*shape, w, item_fea, items + off, m, 1, ei, stats, ws, st)) return rc;
    tv_rowdot_kernel<<<grid_for_waves(m), kBlock, 0, st>>>(eu, ei, m, D2, scores + off);
    HIPREC_TRY(hipGetLastError());
  }
  return 0;
}
