// VBCAR: the variational basket encoder of the grocery family (beta_rec/models/vbcar.py).
//
//   vbcar.py:37-46    parameters: user_emb [U,D], item_emb [I,D], fc_{u,i}_1_mu [L,F], fc_{u,i}_2_mu [2D,L] (+ biases)
//   vbcar.py:55-76    encode: (mu | s) = fc_2(act(fc_1(fea[id]))),  z = mu + exp(0.5 s) * eps
//   vbcar.py:78-109   kl_div against N(0, 1): var1 = s^2 + 1e-10 from the RAW second half (not from exp(0.5 s))
//   vbcar.py:111-178  forward: the Triple2vec scores on e = [z | emb[id]] (2D wide) + six KL means
//   vbcar.py:219-227  train_single_batch: zero_grad, forward, backward, step
//
// One step, rows Ru = B (1 + n_neg) users ([pos_u | neg_u]) and Ri = 2 B (1 + n_neg) items
// ([pos_i_1 | pos_i_2 | neg_i_1 | neg_i_2]), every GEMM stage ONE grouped launch of csrc/ncf.hip's kernel for the user
// and the item problem together:
//   1 gather        X = fea[id]                                     vb_gather_kernel
//   2 GEMM          pre = X W1^T + b1                               (2 problems)
//   3 activation    h = act(pre), in place                          vb_act_kernel<ACT, false>
//   4 GEMM          out = h W2^T + b2 = (mu | s)                    (2 problems)
//   5 loss stage    one wave per triple: z, scores, logsigmoid, KL; d_out written with plain stores (a row of d_out
//                   belongs to exactly one triple), the table halves added to g_flat with fp32 row atomics (a table
//                   row is shared by every occurrence of its id)   vb_loss_kernel
//   6 GEMM          dh = d_out W2, dW2 = d_out^T h, db2 = colsum    (6 problems)
//   7 activation'   dpre = dh * act'(h), in place                   vb_act_kernel<ACT, true>
//   8 GEMM          dW1 = dpre^T X, db1 = colsum                    (4 problems; the features get no gradient)
// Saved for the backward: X, h and out (act' is taken from h: tanh 1 - h^2, sigmoid h (1 - h), (l)relu by h's sign).
#include <algorithm>

#include "gemm.hpp"

namespace hiprec {
namespace {

constexpr int kVbMaxDim = 128;      // emb_dim: two columns of each half per lane
constexpr int kVbMaxLate = 512;     // late_dim
constexpr int kVbMaxFea = 1 << 16;  // feature width
constexpr int kVbNpl = kVbMaxDim / kWave;
constexpr int kVbChunk = 8192;      // rows per pass of the eval-mode encoder
constexpr int kVbMaxSeg = 6;
constexpr float kVbEsp = 1e-10f;    // vbcar.py:23

__device__ __forceinline__ bool vb_in_range(int64_t i, int64_t n) {
  return static_cast<uint64_t>(i) < static_cast<uint64_t>(n);
}

// ---- 1. gather --------------------------------------------------------------------------------------------------------
// A list of id segments, each bound for consecutive rows of its side's X.  An id outside its table sets the side's status
// bit and leaves a zero row.  enc_out (the eval-mode encoder): the id's table row goes to the second half of its output
// row as well.
struct VbSeg {
  const int64_t* ids;
  int64_t n, row0;
  int side;
};
struct VbGather {
  int n_seg;
  VbSeg seg[kVbMaxSeg];
  const float* fea[2];
  const float* emb[2];
  float* X[2];
  int F[2];
  int64_t n_ids[2];
  float* enc_out;
  int D;
};

__global__ __launch_bounds__(kBlock) void vb_gather_kernel(VbGather a, int64_t n_rows, hiprec_stats* stats) {
  const int lane = lane_id();
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); q < n_rows;
       q += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    int sg = 0;
    int64_t k = q;
    while (sg + 1 < a.n_seg && k >= a.seg[sg].n) k -= a.seg[sg++].n;
    const int side = a.seg[sg].side;
    const int64_t id = a.seg[sg].ids[k], row = a.seg[sg].row0 + k;
    const bool ok = vb_in_range(id, a.n_ids[side]);
    if (!ok && lane == 0) atomicOr(&stats->status, side == 0 ? HIPREC_STATUS_USER_OOB : HIPREC_STATUS_ITEM_OOB);
    const int F = a.F[side];
    const float* __restrict__ src = a.fea[side] + (ok ? id : 0) * F;
    float* __restrict__ dst = a.X[side] + row * F;
    if ((F & 3) == 0) {  // rows of both sides start 16-byte aligned
      const float4* s4 = reinterpret_cast<const float4*>(src);
      float4* d4 = reinterpret_cast<float4*>(dst);
      for (int c = lane; c < F / 4; c += kWave) d4[c] = ok ? s4[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (int c = lane; c < F; c += kWave) dst[c] = ok ? src[c] : 0.f;
    }
    if (a.enc_out) {
      float* e = a.enc_out + row * 2 * a.D + a.D;
      for (int c = lane; c < a.D; c += kWave) e[c] = ok ? a.emb[side][id * a.D + c] : __builtin_nanf("");
    }
  }
}

// ---- 3 / 7. the activation and its derivative (taken from h) ---------------------------------------------------------
template <int ACT>
__device__ __forceinline__ float vb_act(float x) {
  if constexpr (ACT == HIPREC_VBCAR_ACT_TANH) return tanhf(x);
  if constexpr (ACT == HIPREC_VBCAR_ACT_SIGMOID) return 1.0f / (1.0f + expf(-x));
  if constexpr (ACT == HIPREC_VBCAR_ACT_RELU) return x > 0.f ? x : 0.f;
  if constexpr (ACT == HIPREC_VBCAR_ACT_LRELU) return x > 0.f ? x : 0.01f * x;
  return x;
}

template <int ACT>
__device__ __forceinline__ float vb_act_grad(float h) {
  if constexpr (ACT == HIPREC_VBCAR_ACT_TANH) return 1.0f - h * h;
  if constexpr (ACT == HIPREC_VBCAR_ACT_SIGMOID) return h * (1.0f - h);
  if constexpr (ACT == HIPREC_VBCAR_ACT_RELU) return h > 0.f ? 1.0f : 0.f;
  if constexpr (ACT == HIPREC_VBCAR_ACT_LRELU) return h > 0.f ? 1.0f : 0.01f;
  return 1.0f;
}

// both sides in one launch: elements [0, n0) of (a0, h0) and [0, n1) of (a1, h1); the buffers are 16-byte aligned and
// padded to whole float4s by the workspace carve
template <int ACT, bool BWD>
__global__ __launch_bounds__(kBlock) void vb_act_kernel(float* __restrict__ a0, const float* __restrict__ h0, int64_t n0,
                                                        float* __restrict__ a1, const float* __restrict__ h1,
                                                        int64_t n1) {
  const int64_t q0 = (n0 + 3) / 4, q1 = (n1 + 3) / 4, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < q0 + q1; e += stride) {
    const bool first = e < q0;
    const int64_t i = first ? e : e - q0;
    float4* a = reinterpret_cast<float4*>(first ? a0 : a1) + i;
    float4 v = *a;
    if constexpr (BWD) {
      const float4 h = reinterpret_cast<const float4*>(first ? h0 : h1)[i];
      v.x *= vb_act_grad<ACT>(h.x);
      v.y *= vb_act_grad<ACT>(h.y);
      v.z *= vb_act_grad<ACT>(h.z);
      v.w *= vb_act_grad<ACT>(h.w);
    } else {
      v.x = vb_act<ACT>(v.x);
      v.y = vb_act<ACT>(v.y);
      v.z = vb_act<ACT>(v.z);
      v.w = vb_act<ACT>(v.w);
    }
    *a = v;
  }
}

template <bool BWD>
int vb_launch_act(int act, float* a0, const float* h0, int64_t n0, float* a1, const float* h1, int64_t n1,
                  hipStream_t st) {
  const int grid = grid_for_threads((n0 + 3) / 4 + (n1 + 3) / 4);
  switch (act) {
    case HIPREC_VBCAR_ACT_NONE:
      return 0;
    case HIPREC_VBCAR_ACT_TANH:
      vb_act_kernel<HIPREC_VBCAR_ACT_TANH, BWD><<<grid, kBlock, 0, st>>>(a0, h0, n0, a1, h1, n1);
      break;
    case HIPREC_VBCAR_ACT_SIGMOID:
      vb_act_kernel<HIPREC_VBCAR_ACT_SIGMOID, BWD><<<grid, kBlock, 0, st>>>(a0, h0, n0, a1, h1, n1);
      break;
    case HIPREC_VBCAR_ACT_RELU:
      vb_act_kernel<HIPREC_VBCAR_ACT_RELU, BWD><<<grid, kBlock, 0, st>>>(a0, h0, n0, a1, h1, n1);
      break;
    default:
      vb_act_kernel<HIPREC_VBCAR_ACT_LRELU, BWD><<<grid, kBlock, 0, st>>>(a0, h0, n0, a1, h1, n1);
  }
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// ---- 5. the loss stage --------------------------------------------------------------------------------------------------
struct VbLoss {
  const float *out_u, *out_i;   // [Ru, 2D], [Ri, 2D]: (mu | s)
  float *dout_u, *dout_i;
  const float* noise;           // [3B (1 + n_neg), D]: pos_u, pos_i_1, pos_i_2, neg_u, neg_i_1, neg_i_2
  const float *emb_u, *emb_i;
  float *g_emb_u, *g_emb_i;
  const int64_t *pos_u, *pos_i1, *pos_i2, *neg_u, *neg_i1, *neg_i2;
  int64_t B, U, I;
  int n_neg, D;
  float alpha, scale;
};

// lane's columns c = lane + 64 k of one encoded row: z = mu + exp(0.5 s) eps and the table row next to it
struct VbRow {
  float mu[kVbNpl], s[kVbNpl], se[kVbNpl], z[kVbNpl], t[kVbNpl];
};

__device__ __forceinline__ void vb_load_row(const float* __restrict__ out, int64_t r, const float* __restrict__ noise,
                                            int64_t nr, const float* __restrict__ emb, int64_t id, int D, int lane,
                                            VbRow& v) {
#pragma unroll
  for (int k = 0; k < kVbNpl; ++k) {
    const int c = lane + kWave * k;
    const bool in = c < D;
    v.mu[k] = in ? out[r * 2 * D + c] : 0.f;
    v.s[k] = in ? out[r * 2 * D + D + c] : 0.f;
    const float eps = in ? noise[nr * D + c] : 0.f;
    v.t[k] = in ? emb[id * D + c] : 0.f;
    v.se[k] = expf(0.5f * v.s[k]) * eps;
    v.z[k] = v.mu[k] + v.se[k];
  }
}

__device__ __forceinline__ float vb_dot(const VbRow& a, const VbRow& b) {
  float d = 0.f;
#pragma unroll
  for (int k = 0; k < kVbNpl; ++k) d += a.z[k] * b.z[k] + a.t[k] * b.t[k];
  return d;
}

// With dz / dt = d GEN / d (z | table half) of the row: its KL term (weight kl_w = 1 / rows of its mean) joins kl_lane,
// d_out = (1 - alpha) d GEN + alpha scale kl_w d KL is stored, and the table half goes to the gradient with row atomics.
__device__ __forceinline__ void vb_finish_row(float* __restrict__ dout, int64_t r, float* __restrict__ g_emb, int64_t id,
                                              int D, int lane, const VbRow& v, const float* dz, const float* dt,
                                              float oma, float akl, float kl_w, float& kl_lane) {
#pragma unroll
  for (int k = 0; k < kVbNpl; ++k) {
    const int c = lane + kWave * k;
    if (c < D) {
      const float mu = v.mu[k], s = v.s[k];
      const float var1 = s * s + kVbEsp;
      kl_lane += kl_w * 0.5f * (logf(1.0f / var1) - 1.0f + var1 + mu * mu);
      dout[r * 2 * D + c] = oma * dz[k] + akl * mu;
      dout[r * 2 * D + D + c] = oma * dz[k] * 0.5f * v.se[k] + akl * (s - s / var1);
      atomic_add_f32(g_emb + id * D + c, oma * dt[k]);
    }
  }
}

__device__ __forceinline__ void vb_zero_row(float* __restrict__ dout, int64_t r, int D, int lane) {
  for (int c = lane; c < 2 * D; c += kWave) dout[r * 2 * D + c] = 0.f;
}

__global__ __launch_bounds__(kBlock) void vb_loss_kernel(VbLoss a, hiprec_stats* stats, Scratch* scratch) {
  const int lane = lane_id();
  const int D = a.D, n_neg = a.n_neg;
  const int64_t B = a.B, Bn = B * n_neg;
  const float oma = 1.0f - a.alpha;
  const float kl_pos = 1.0f / static_cast<float>(B), kl_neg = n_neg ? 1.0f / static_cast<float>(Bn) : 0.f;
  const float akl_pos = a.alpha * a.scale * kl_pos, akl_neg = a.alpha * a.scale * kl_neg;

  const bool stepper = blockIdx.x == 0 && threadIdx.x == 0;
  StepState step_state{};
  if (stepper) step_state = step_load(stats);

  float gen = 0.f, kl_lane = 0.f;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); t < B;
       t += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const int64_t u = a.pos_u[t], i1 = a.pos_i1[t], i2 = a.pos_i2[t];
    const bool u_ok = vb_in_range(u, a.U), i_ok = vb_in_range(i1, a.I) && vb_in_range(i2, a.I);
    if (!(u_ok && i_ok)) {  // the whole triple is dropped; its rows of d_out are still this wave's to write
      if (lane == 0)
        atomicOr(&stats->status, (u_ok ? 0u : HIPREC_STATUS_USER_OOB) | (i_ok ? 0u : HIPREC_STATUS_ITEM_OOB));
      vb_zero_row(a.dout_u, t, D, lane);
      vb_zero_row(a.dout_i, t, D, lane);
      vb_zero_row(a.dout_i, B + t, D, lane);
      for (int j = 0; j < n_neg; ++j) {
        const int64_t qn = t * n_neg + j;
        vb_zero_row(a.dout_u, B + qn, D, lane);
        vb_zero_row(a.dout_i, 2 * B + qn, D, lane);
        vb_zero_row(a.dout_i, 2 * B + Bn + qn, D, lane);
      }
      continue;
    }
    VbRow pu, p1, p2;
    vb_load_row(a.out_u, t, a.noise, t, a.emb_u, u, D, lane, pu);
    vb_load_row(a.out_i, t, a.noise, B + t, a.emb_i, i1, D, lane, p1);
    vb_load_row(a.out_i, B + t, a.noise, 2 * B + t, a.emb_i, i2, D, lane, p2);
    // positives: each vector against the SUM of the other two (vbcar.py:137-159)
    float xu = 0.f, x1 = 0.f, x2 = 0.f;
#pragma unroll
    for (int k = 0; k < kVbNpl; ++k) {
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
    float dzu[kVbNpl], dtu[kVbNpl], dz1[kVbNpl], dt1[kVbNpl], dz2[kVbNpl], dt2[kVbNpl];
#pragma unroll
    for (int k = 0; k < kVbNpl; ++k) {
      dzu[k] = au * (p1.z[k] + p2.z[k]) + a1 * p1.z[k] + a2 * p2.z[k];
      dtu[k] = au * (p1.t[k] + p2.t[k]) + a1 * p1.t[k] + a2 * p2.t[k];
      dz1[k] = au * pu.z[k] + a1 * (pu.z[k] + p2.z[k]) + a2 * p2.z[k];
      dt1[k] = au * pu.t[k] + a1 * (pu.t[k] + p2.t[k]) + a2 * p2.t[k];
      dz2[k] = au * pu.z[k] + a1 * p1.z[k] + a2 * (pu.z[k] + p1.z[k]);
      dt2[k] = au * pu.t[k] + a1 * p1.t[k] + a2 * (pu.t[k] + p1.t[k]);
    }
    // negatives: each against the triple's OWN vector of its kind (vbcar.py:142-162)
    for (int j = 0; j < n_neg; ++j) {
      const int64_t qn = t * n_neg + j;
#pragma unroll
      for (int kind = 0; kind < 3; ++kind) {
        const bool user = kind == 0;
        const int64_t id = user ? a.neg_u[qn] : (kind == 1 ? a.neg_i1[qn] : a.neg_i2[qn]);
        const int64_t r = user ? B + qn : 2 * B + (kind == 2 ? Bn : 0) + qn;
        const int64_t nr = 3 * B + kind * Bn + qn;
        float* dout = user ? a.dout_u : a.dout_i;
        if (!vb_in_range(id, user ? a.U : a.I)) {
          if (lane == 0) atomicOr(&stats->status, user ? HIPREC_STATUS_USER_OOB : HIPREC_STATUS_ITEM_OOB);
          vb_zero_row(dout, r, D, lane);
          continue;
        }
        const VbRow& p = kind == 0 ? pu : (kind == 1 ? p1 : p2);
        float* dzp = kind == 0 ? dzu : (kind == 1 ? dz1 : dz2);
        float* dtp = kind == 0 ? dtu : (kind == 1 ? dt1 : dt2);
        VbRow nv;
        vb_load_row(user ? a.out_u : a.out_i, r, a.noise, nr, user ? a.emb_u : a.emb_i, id, D, lane, nv);
        const float y = wave_sum(vb_dot(nv, p));
        float sy;  // neg_logsigmoid(-y) = -logsigmoid(-y), and sigmoid(y) next to it
        gen += neg_logsigmoid(-y, &sy);
        const float b = sy * a.scale;
        float dzn[kVbNpl], dtn[kVbNpl];
#pragma unroll
        for (int k = 0; k < kVbNpl; ++k) {
          dzp[k] += b * nv.z[k];
          dtp[k] += b * nv.t[k];
          dzn[k] = b * p.z[k];
          dtn[k] = b * p.t[k];
        }
        vb_finish_row(dout, r, user ? a.g_emb_u : a.g_emb_i, id, D, lane, nv, dzn, dtn, oma, akl_neg, kl_neg, kl_lane);
      }
    }
    vb_finish_row(a.dout_u, t, a.g_emb_u, u, D, lane, pu, dzu, dtu, oma, akl_pos, kl_pos, kl_lane);
    vb_finish_row(a.dout_i, t, a.g_emb_i, i1, D, lane, p1, dz1, dt1, oma, akl_pos, kl_pos, kl_lane);
    vb_finish_row(a.dout_i, B + t, a.g_emb_i, i2, D, lane, p2, dz2, dt2, oma, akl_pos, kl_pos, kl_lane);
  }
  publish_partials<kWavesPerBlock>(gen, kl_lane, 0.f, a.scale, scratch);   // loss = GEN, reg = KLD
  if (stepper) step_store_advanced(stats, step_state);
}

// scores[k] = <eu[k], ei[k]> over `width` columns (VBCAR.predict, vbcar.py:185-192)
__global__ __launch_bounds__(kBlock) void vb_rowdot_kernel(const float* __restrict__ eu, const float* __restrict__ ei,
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
struct VbParams {   // pointers into a flat buffer laid out in state_dict() order; [0] = user side, [1] = item side
  float* emb[2];
  float *w1[2], *b1[2], *w2[2], *b2[2];
};

int64_t vb_n_params(const hiprec_vbcar_shape& s) {
  const int64_t D = s.emb_dim, L = s.late_dim;
  return (s.n_users + s.n_items) * D + L * (s.fea_u + s.fea_i) + 2 * L + 2 * (2 * D * L + 2 * D);
}

VbParams vb_params(float* base, const hiprec_vbcar_shape& s) {
  VbParams p{};
  const int64_t D = s.emb_dim, L = s.late_dim;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += n; return r; };
  p.emb[0] = take(s.n_users * D);
  p.emb[1] = take(s.n_items * D);
  for (int side = 0; side < 2; ++side) {
    p.w1[side] = take(L * (side == 0 ? s.fea_u : s.fea_i));
    p.b1[side] = take(L);
    p.w2[side] = take(2 * D * L);
    p.b2[side] = take(2 * D);
  }
  return p;
}

struct VbWorkspace {
  float *X[2], *H[2], *O[2], *dO[2], *dH[2], *cs2[2], *cs1[2];
  int64_t floats;
};

VbWorkspace vb_carve(float* base, const hiprec_vbcar_shape& s, int64_t B, int n_neg) {
  VbWorkspace w{};
  const int64_t D = s.emb_dim, L = s.late_dim;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += (n + 3) / 4 * 4; return r; };
  for (int side = 0; side < 2; ++side) {
    const int64_t R = (side + 1) * B * (1 + n_neg), F = side == 0 ? s.fea_u : s.fea_i;
    w.X[side] = take(R * F);
    w.H[side] = take(R * L);
    w.O[side] = take(R * 2 * D);
    w.dO[side] = take(R * 2 * D);
    w.dH[side] = take(R * L);
    w.cs2[side] = take(colsum_ws_floats(static_cast<int>(R), static_cast<int>(2 * D)));
    w.cs1[side] = take(colsum_ws_floats(static_cast<int>(R), static_cast<int>(L)));
  }
  w.floats = c - base;
  return w;
}

int vb_check_shape(const hiprec_vbcar_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  HIPREC_REQUIRE(s->n_users >= 1 && s->n_items >= 1, "VBCAR needs n_users >= 1 and n_items >= 1");
  HIPREC_REQUIRE(s->emb_dim >= 1 && s->emb_dim <= kVbMaxDim, "VBCAR needs 1 <= emb_dim <= %d (got %d)", kVbMaxDim,
                 s->emb_dim);
  HIPREC_REQUIRE(s->late_dim >= 1 && s->late_dim <= kVbMaxLate, "VBCAR needs 1 <= late_dim <= %d (got %d)", kVbMaxLate,
                 s->late_dim);
  HIPREC_REQUIRE(s->fea_u >= 1 && s->fea_u <= kVbMaxFea && s->fea_i >= 1 && s->fea_i <= kVbMaxFea,
                 "VBCAR needs feature widths in 1 .. %d (got %d and %d)", kVbMaxFea, s->fea_u, s->fea_i);
  HIPREC_REQUIRE(s->act >= HIPREC_VBCAR_ACT_NONE && s->act <= HIPREC_VBCAR_ACT_LRELU, "unknown activation %d", s->act);
  return 0;
}

// the grouped GEMM indexes its operands with ints: every [rows, width] operand of a step must stay below 2^31 elements
bool vb_rows_ok(const hiprec_vbcar_shape& s, int64_t rows) {
  const int64_t widest = std::max<int64_t>({s.fea_u, s.fea_i, s.late_dim, 2 * s.emb_dim});
  return rows >= 1 && rows < (1ll << 24) && rows * widest < (1ll << 31);
}

// (mu | s) of `rows` gathered rows of each side: stages 1-4.  n_out: columns of fc_2 that are computed (2D in training,
// D in the eval-mode encoder, whose O has the leading dimension 2D all the same).
int vb_forward(const hiprec_vbcar_shape& s, const VbParams& w, const VbGather& ga, const int64_t rows[2],
               float* const H[2], float* const O[2], int n_out, hiprec_stats* stats, hipStream_t st) {
  const int L = s.late_dim, D = s.emb_dim;
  vb_gather_kernel<<<grid_for_waves(rows[0] + rows[1]), kBlock, 0, st>>>(ga, rows[0] + rows[1], stats);
  HIPREC_TRY(hipGetLastError());
  GemmGroup g1{}, g2{};
  for (int side = 0; side < 2; ++side) {
    if (rows[side] == 0) continue;
    const int R = static_cast<int>(rows[side]), F = ga.F[side];
    g1.p[g1.n++] = make_gemm(kNT, R, L, F, ga.X[side], F, w.w1[side], F, H[side], L, w.b1[side], 0, nullptr, 0, false);
    g2.p[g2.n++] = make_gemm(kNT, R, n_out, L, H[side], L, w.w2[side], L, O[side], 2 * D, w.b2[side], 0, nullptr, 0,
                             false);
  }
  if (int rc = launch_group(g1, st)) return rc;
  if (int rc = vb_launch_act<false>(s.act, H[0], nullptr, rows[0] * L, H[1], nullptr, rows[1] * L, st)) return rc;
  return launch_group(g2, st);
}

int vb_train(const hiprec_vbcar_shape& s, float* w_flat, float* g_flat, const float* fea_u, const float* fea_i,
             const int64_t* const ids[6], int64_t B, int n_neg, const float* noise, float alpha, float scale,
             hiprec_stats* stats, Scratch* scratch, float* ws_base, hipStream_t st) {
  const int L = s.late_dim, D = s.emb_dim;
  const int64_t Bn = B * n_neg;
  const int64_t rows[2] = {B + Bn, 2 * (B + Bn)};
  const VbParams w = vb_params(w_flat, s), g = vb_params(g_flat, s);
  const VbWorkspace a = vb_carve(ws_base, s, B, n_neg);

  VbGather ga{};
  ga.seg[ga.n_seg++] = VbSeg{ids[0], B, 0, 0};
  ga.seg[ga.n_seg++] = VbSeg{ids[1], B, 0, 1};
  ga.seg[ga.n_seg++] = VbSeg{ids[2], B, B, 1};
  if (n_neg > 0) {
    ga.seg[ga.n_seg++] = VbSeg{ids[3], Bn, B, 0};
    ga.seg[ga.n_seg++] = VbSeg{ids[4], Bn, 2 * B, 1};
    ga.seg[ga.n_seg++] = VbSeg{ids[5], Bn, 2 * B + Bn, 1};
  }
  ga.fea[0] = fea_u; ga.fea[1] = fea_i;
  ga.F[0] = s.fea_u; ga.F[1] = s.fea_i;
  ga.n_ids[0] = s.n_users; ga.n_ids[1] = s.n_items;
  ga.D = D;
  for (int side = 0; side < 2; ++side) ga.X[side] = a.X[side];
  if (int rc = vb_forward(s, w, ga, rows, a.H, a.O, 2 * D, stats, st)) return rc;

  VbLoss lo{};
  lo.out_u = a.O[0]; lo.out_i = a.O[1];
  lo.dout_u = a.dO[0]; lo.dout_i = a.dO[1];
  lo.noise = noise;
  lo.emb_u = w.emb[0]; lo.emb_i = w.emb[1];
  lo.g_emb_u = g.emb[0]; lo.g_emb_i = g.emb[1];
  lo.pos_u = ids[0]; lo.pos_i1 = ids[1]; lo.pos_i2 = ids[2];
  lo.neg_u = ids[3]; lo.neg_i1 = ids[4]; lo.neg_i2 = ids[5];
  lo.B = B; lo.U = s.n_users; lo.I = s.n_items;
  lo.n_neg = n_neg; lo.D = D;
  lo.alpha = alpha; lo.scale = scale;
  vb_loss_kernel<<<grid_for_waves(B), kBlock, 0, st>>>(lo, stats, scratch);
  HIPREC_TRY(hipGetLastError());

  {
    GemmGroup q{};
    for (int side = 0; side < 2; ++side) {
      const int R = static_cast<int>(rows[side]);
      q.p[q.n++] = make_gemm(kNN, R, L, 2 * D, a.dO[side], 2 * D, w.w2[side], L, a.dH[side], L, nullptr, 0, nullptr, 0,
                             false);
      q.p[q.n++] = make_gemm(kTNm, 2 * D, L, R, a.dO[side], 2 * D, a.H[side], L, g.w2[side], L, nullptr, 0, nullptr, 0,
                             true);
      q.p[q.n++] = make_colsum(a.dO[side], R, 2 * D, 2 * D, g.b2[side], a.cs2[side]);
    }
    if (int rc = launch_group(q, st)) return rc;
    if (int rc = launch_colsum_reduce(q, st)) return rc;
  }
  if (int rc = vb_launch_act<true>(s.act, a.dH[0], a.H[0], rows[0] * L, a.dH[1], a.H[1], rows[1] * L, st)) return rc;
  {
    GemmGroup q{};
    for (int side = 0; side < 2; ++side) {
      const int R = static_cast<int>(rows[side]), F = ga.F[side];
      q.p[q.n++] = make_gemm(kTNm, L, F, R, a.dH[side], L, a.X[side], F, g.w1[side], F, nullptr, 0, nullptr, 0, true);
      q.p[q.n++] = make_colsum(a.dH[side], R, L, L, g.b1[side], a.cs1[side]);
    }
    if (int rc = launch_group(q, st)) return rc;
    if (int rc = launch_colsum_reduce(q, st)) return rc;
  }
  return 0;
}

int64_t vb_encode_ws_floats(const hiprec_vbcar_shape& s, int64_t n) {
  const int64_t rows = std::min<int64_t>(n, kVbChunk), F = std::max(s.fea_u, s.fea_i);
  return (rows * F + 3) / 4 * 4 + (rows * s.late_dim + 3) / 4 * 4;
}

// out[k] = [mu(ids[k]) | emb[ids[k]]] for one side, kVbChunk rows per pass
int vb_encode(const hiprec_vbcar_shape& s, const VbParams& w, const float* fea, const int64_t* ids, int64_t n, int side,
              float* out, hiprec_stats* stats, float* ws, hipStream_t st) {
  const int D = s.emb_dim, F = side == 0 ? s.fea_u : s.fea_i;
  for (int64_t off = 0; off < n; off += kVbChunk) {
    const int64_t m = std::min<int64_t>(n - off, kVbChunk);
    float* X = ws;
    float* H = ws + (m * F + 3) / 4 * 4;
    VbGather ga{};
    ga.n_seg = 1;
    ga.seg[0] = VbSeg{ids + off, m, 0, side};
    ga.fea[side] = fea;
    ga.emb[side] = w.emb[side];
    ga.F[side] = F;
    ga.n_ids[side] = side == 0 ? s.n_users : s.n_items;
    ga.X[side] = X;
    ga.enc_out = out + off * 2 * D;
    ga.D = D;
    int64_t rows[2] = {0, 0};
    float *Hs[2] = {nullptr, nullptr}, *Os[2] = {nullptr, nullptr};
    rows[side] = m;
    Hs[side] = H;
    Os[side] = out + off * 2 * D;
    if (int rc = vb_forward(s, w, ga, rows, Hs, Os, D, stats, st)) return rc;
  }
  return 0;
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_vbcar_shape_bytes(void) { return sizeof(hiprec_vbcar_shape); }

extern "C" int64_t hiprec_vbcar_param_floats(const hiprec_vbcar_shape* shape) {
  if (vb_check_shape(shape)) return -1;
  return vb_n_params(*shape);
}

extern "C" size_t hiprec_vbcar_workspace_bytes(const hiprec_vbcar_shape* shape, int64_t batch, int32_t n_neg) {
  if (vb_check_shape(shape) || batch < 1 || n_neg < 0) return 0;
  if (!vb_rows_ok(*shape, 2 * batch * (1 + static_cast<int64_t>(n_neg)))) {
    set_error("a VBCAR step of %lld triples x %d negatives is beyond the grouped GEMM's 2^31 elements per operand",
              static_cast<long long>(batch), n_neg);
    return 0;
  }
  return sizeof(float) * static_cast<size_t>(vb_carve(nullptr, *shape, batch, n_neg).floats);
}

extern "C" size_t hiprec_vbcar_encode_workspace_bytes(const hiprec_vbcar_shape* shape, int64_t n, int32_t pairs) {
  if (vb_check_shape(shape) || n < 1) return 0;
  const int64_t rows = std::min<int64_t>(n, kVbChunk);
  int64_t floats = vb_encode_ws_floats(*shape, n);
  if (pairs) floats += 2 * rows * 2 * shape->emb_dim;
  return sizeof(float) * static_cast<size_t>(floats);
}

extern "C" int hiprec_vbcar_grad(const hiprec_vbcar_shape* shape, const float* w_flat, float* g_flat,
                                 const float* user_fea, const float* item_fea, const int64_t* pos_u,
                                 const int64_t* pos_i1, const int64_t* pos_i2, const int64_t* neg_u,
                                 const int64_t* neg_i1, const int64_t* neg_i2, int64_t batch, int32_t n_neg,
                                 const float* noise, float alpha, float scale, hiprec_stats* stats, void* scratch,
                                 size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = vb_check_shape(shape)) return rc;
  HIPREC_REQUIRE(w_flat && g_flat && user_fea && item_fea && noise && stats && scratch && workspace, "NULL pointer");
  HIPREC_REQUIRE(batch >= 1 && n_neg >= 0, "bad batch / n_neg");
  HIPREC_REQUIRE(pos_u && pos_i1 && pos_i2, "NULL positive index arrays");
  HIPREC_REQUIRE(n_neg == 0 || (neg_u && neg_i1 && neg_i2), "NULL negative index arrays");
  if (scratch_bytes < kScratchBytes) {
    set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
    return HIPREC_E_SCRATCH;
  }
  const size_t need = hiprec_vbcar_workspace_bytes(shape, batch, n_neg);
  HIPREC_REQUIRE(need > 0, "unsupported batch %lld x n_neg %d", static_cast<long long>(batch), n_neg);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  const int64_t* const ids[6] = {pos_u, pos_i1, pos_i2, neg_u, neg_i1, neg_i2};
  return vb_train(*shape, const_cast<float*>(w_flat), g_flat, user_fea, item_fea, ids, batch, n_neg, noise, alpha, scale,
                  stats, static_cast<Scratch*>(scratch), static_cast<float*>(workspace),
                  static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_vbcar_encode(const hiprec_vbcar_shape* shape, const float* w_flat, const float* fea,
                                   const int64_t* ids, int64_t n, int32_t side, float* out, hiprec_stats* stats,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = vb_check_shape(shape)) return rc;
  HIPREC_REQUIRE(n >= 0 && (side == 0 || side == 1), "bad n / side");
  if (n == 0) return 0;
  HIPREC_REQUIRE(w_flat && fea && ids && out && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(vb_rows_ok(*shape, std::min<int64_t>(n, kVbChunk)), "feature rows too wide for one pass");
  const size_t need = hiprec_vbcar_encode_workspace_bytes(shape, n, 0);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  return vb_encode(*shape, vb_params(const_cast<float*>(w_flat), *shape), fea, ids, n, side, out, stats,
                   static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_vbcar_predict(const hiprec_vbcar_shape* shape, const float* w_flat, const float* user_fea,
                                    const float* item_fea, const int64_t* users, const int64_t* items, int64_t n,
                                    float* scores, hiprec_stats* stats, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (int rc = vb_check_shape(shape)) return rc;
  HIPREC_REQUIRE(n >= 0, "negative n");
  if (n == 0) return 0;
  HIPREC_REQUIRE(w_flat && user_fea && item_fea && users && items && scores && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(vb_rows_ok(*shape, std::min<int64_t>(n, kVbChunk)), "feature rows too wide for one pass");
  const size_t need = hiprec_vbcar_encode_workspace_bytes(shape, n, 1);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const VbParams w = vb_params(const_cast<float*>(w_flat), *shape);
  const int D2 = 2 * shape->emb_dim;
  float* ws = static_cast<float*>(workspace);
  float* eu = ws + vb_encode_ws_floats(*shape, n);
  float* ei = eu + std::min<int64_t>(n, kVbChunk) * D2;
  for (int64_t off = 0; off < n; off += kVbChunk) {
    const int64_t m = std::min<int64_t>(n - off, kVbChunk);
    if (int rc = vb_encode(*shape, w, user_fea, users + off, m, 0, eu, stats, ws, st)) return rc;
    if (int rc = vb_encode(*shape, w, item_fea, items + off, m, 1, ei, stats, ws, st)) return rc;
    vb_rowdot_kernel<<<grid_for_waves(m), kBlock, 0, st>>>(eu, ei, m, D2, scores + off);
    HIPREC_TRY(hipGetLastError());
  }
  return 0;
}
