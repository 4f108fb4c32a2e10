// GRU4Rec (Hidasi et al., ICLR 2016; Hidasi and Karatzoglou, CIKM 2018): zero_grad + forward + loss + backward of one
// session-parallel step as a fixed sequence of launches, no host sync.  The contract is in include/hiprec.h; B slots,
// S extra samples, N = B + S candidates, L layers of widths H_l, in_l the width of layer l's input.
//
//   gather        x_0 = table[in_items] through the embed keep bytes (table: Wy when constrained, else E); per layer
//                 hp_l = the stored state read through the reset byte; when training the candidate rows O [N, H_last] =
//                 Wy[cand] and ob [N] = By[cand] - shift (the logQ shift is a per-column constant, so it rides in the
//                 score GEMM's bias)
//   cell forward  per layer: the grouped GEMM does Gi = x W_ih^T + b_ih and Gh = hp W_hh^T + b_hh as two problems of one
//                 grid; one elementwise launch forms r, z, n and h, applies the hidden dropout, stores the new state and
//                 leaves r | z | n in Gi for the backward (Gh keeps W_hn hp + b_hn)
//   scores        R [B, N] = h_last O^T + ob through the grouped GEMM
//   loss          one wave per row of R: maximum, sums and the diagonal in registers, the loss term into the block's
//                 partial, d R written over R
//   loss backward one grouped launch: d h_last = dR O, dO = dR^T h_last (one block per tile walks the whole batch: no
//                 split-K atomics), the column sums of dR per 128-row slab; a second launch folds the slabs in order
//   cell backward per layer from the top: gate derivatives elementwise over Gi / Gh, then one grouped launch for
//                 d W_ih = dGi^T x, d W_hh = dGh^T hp, both bias sums and dx = dGi W_ih, and the slab fold
//   scatter       the N candidate rows of dO / d ob into d Wy / d By and the B input rows of dx_0 (through the embed keep
//                 bytes) into d Wy or d E, by row atomics: ids repeat
//
// 6 + 5 L launches when training, 1 + 2 L in the eval step, whatever B, S and n_items are.  Every gradient except the
// tables (Wy, By, E) is the same bits on every run.  The score block R is kept in the workspace (B N floats): the GEMM
// that fills it and the two that read d R are the project's exact-fp32 MFMA GEMM, and at the limits it is 48 MB.
#include <algorithm>

#include "gemm.hpp"
#include "gru4rec.hpp"

namespace hiprec {
namespace {

struct Gru4recDims {
  int64_t n_items;
  int L, H[kGru4recMaxLayers], in[kGru4recMaxLayers];
  int D;        // emb_dim, 0 when constrained
  int loss;
};

struct Gru4recLayer {
  float *wih, *whh, *bih, *bhh;
};
struct Gru4recParams {      // pointers into a flat buffer laid out in state_dict() order
  float *Wy, *By, *E;
  Gru4recLayer l[kGru4recMaxLayers];
};

struct Gru4recGather {
  const float* table;             // Wy or E: the rows of x_0
  const float *Wy, *By, *log_p;
  const int64_t *in_items, *targets, *samples;
  const uint8_t *reset, *keep_e;
  float ks_e, logq, alpha;
  int B, S, L, in0, HL;
  int H[kGru4recMaxLayers];
  float* state[kGru4recMaxLayers];
  float* hp[kGru4recMaxLayers];
  float *x0, *O, *ob, *dob;
  int train;
};

__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}

__global__ __launch_bounds__(kBlock) void gru4rec_gather_kernel(Gru4recGather a, int64_t n_items, hiprec_stats* stats) {
  const int64_t t0 = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  const int B = a.B;
  for (int64_t e = t0; e < static_cast<int64_t>(B) * a.in0; e += stride) {
    const int b = static_cast<int>(e / a.in0), k = static_cast<int>(e - static_cast<int64_t>(b) * a.in0);
    const int64_t id = a.in_items[b];
    float v = 0.f;
    if (id >= 0 && id < n_items) {
      v = a.table[id * a.in0 + k];
      if (a.keep_e) v = a.keep_e[e] ? v * a.ks_e : 0.f;
    } else if (k == 0) {
      atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
    }
    a.x0[e] = v;
  }
  for (int l = 0; l < a.L; ++l) {
    const int H = a.H[l];
    for (int64_t e = t0; e < static_cast<int64_t>(B) * H; e += stride) {
      const int b = static_cast<int>(e / H);
      a.hp[l][e] = (a.reset && a.reset[b]) ? 0.f : a.state[l][e];
    }
  }
  if (!a.train) return;
  const int N = B + a.S, HL = a.HL;
  for (int64_t e = t0; e < static_cast<int64_t>(N) * HL; e += stride) {
    const int j = static_cast<int>(e / HL), k = static_cast<int>(e - static_cast<int64_t>(j) * HL);
    const int64_t id = j < B ? a.targets[j] : a.samples[j - B];
    const bool ok = id >= 0 && id < n_items;
    a.O[e] = ok ? a.Wy[id * HL + k] : 0.f;
    if (k == 0) {
      float bias = 0.f;
      if (ok) {
        bias = a.By[id];
        if (a.log_p) bias -= a.logq * a.log_p[id] * (j < B ? 1.f : a.alpha);
      } else {
        atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
      }
      a.ob[j] = bias;
      a.dob[j] = 0.f;
    }
  }
}

// Gi, Gh [B, 3H] hold the two halves of the gate pre-activations (biases included).  h = (1 - z) n + z hp; out = h through
// the keep bytes goes to `act` (what the next layer and the loss read) and to the stored state.  With `save` Gi receives
// r | z | n (Gh's n block stays W_hn hp + b_hn: the backward needs it for d r).
__global__ __launch_bounds__(kBlock) void gru4rec_cell_kernel(float* __restrict__ Gi, const float* __restrict__ Gh,
                                                              const float* __restrict__ hp, int B, int H,
                                                              const uint8_t* __restrict__ keep, float ks, int save,
                                                              float* __restrict__ act, float* __restrict__ state) {
  const int64_t n = static_cast<int64_t>(B) * H, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
    const int64_t b = e / H, k = e - b * H, g = b * 3 * H + k;
    const float r = sigmoid_f32(Gi[g] + Gh[g]);
    const float z = sigmoid_f32(Gi[g + H] + Gh[g + H]);
    const float c = tanhf(Gi[g + 2 * H] + r * Gh[g + 2 * H]);
    const float prev = hp[e];
    float h = c + z * (prev - c);
    if (keep) h = keep[e] ? h * ks : 0.f;
    if (save) {
      Gi[g] = r;
      Gi[g + H] = z;
      Gi[g + 2 * H] = c;
    }
    act[e] = h;
    state[e] = h;
  }
}

// d out [B, H] -> d Gi (over Gi) and d Gh (over Gh); no gradient goes to hp
__global__ __launch_bounds__(kBlock) void gru4rec_cell_bwd_kernel(float* __restrict__ Gi, float* __restrict__ Gh,
                                                                  const float* __restrict__ hp,
                                                                  const float* __restrict__ d_out, int B, int H,
                                                                  const uint8_t* __restrict__ keep, float ks) {
  const int64_t n = static_cast<int64_t>(B) * H, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
    const int64_t b = e / H, k = e - b * H, g = b * 3 * H + k;
    float dh = d_out[e];
    if (keep) dh = keep[e] ? dh * ks : 0.f;
    const float r = Gi[g], z = Gi[g + H], c = Gi[g + 2 * H], ghn = Gh[g + 2 * H];
    const float dc = dh * (1.f - z) * (1.f - c * c);      // d (W_in x + b_in + r ghn)
    const float dz = dh * (hp[e] - c) * z * (1.f - z);
    const float dr = dc * ghn * r * (1.f - r);
    Gi[g] = dr;
    Gi[g + H] = dz;
    Gi[g + 2 * H] = dc;
    Gh[g] = dr;
    Gh[g + H] = dz;
    Gh[g + 2 * H] = dc * r;
  }
}

__device__ __forceinline__ float elu_f32(float v, float alpha) { return v > 0.f ? v : alpha * expm1f(v); }

// One wave per row i of R [B, N] (ld N); d R is written over R.  The diagonal entry stays as it came until the row's
// last store, so every lane may read it at the top.
__global__ __launch_bounds__(kBlock) void gru4rec_loss_kernel(float* __restrict__ R, int B, int N, int loss, float bpreg,
                                                              float alpha, Scratch* scratch, hiprec_stats* stats) {
  const int lane = lane_id();
  float loss_w = 0.f;
  for (int i = blockIdx.x * kWavesPerBlock + wave_in_block(); i < B; i += gridDim.x * kWavesPerBlock) {
    float* row = R + static_cast<int64_t>(i) * N;
    const float raw_ii = row[i];
    if (loss == HIPREC_GRU4REC_XE) {
      float m = -INFINITY;
      for (int j = lane; j < N; j += kWave) m = fmaxf(m, row[j]);
      m = wave_max(m);
      float zs = 0.f;
      for (int j = lane; j < N; j += kWave) zs += expf(row[j] - m);
      const float Z = wave_sum(zs), p_i = expf(raw_ii - m) / Z;
      loss_w -= logf(p_i + 1e-24f);
      const float c = p_i / (p_i + 1e-24f);
      for (int j = lane; j < N; j += kWave) {
        const float p = expf(row[j] - m) / Z;
        row[j] = c * (j == i ? p - 1.f : p);
      }
    } else {
      const bool elu = alpha > 0.f;
      const float r_ii = elu ? elu_f32(raw_ii, alpha) : raw_ii;
      float m = -INFINITY;
      for (int j = lane; j < N; j += kWave) {
        if (j == i) continue;
        float v = row[j];
        if (elu) {
          v = elu_f32(v, alpha);
          row[j] = v;      // R' replaces R; elu'(R) = R' + alpha where R <= 0
        }
        m = fmaxf(m, v);
      }
      m = wave_max(m);
      float zs = 0.f, as = 0.f, bs = 0.f;
      for (int j = lane; j < N; j += kWave) {
        if (j == i) continue;
        const float v = row[j], ex = expf(v - m);
        zs += ex;
        as = fmaf(sigmoid_f32(r_ii - v), ex, as);
        bs = fmaf(v * v, ex, bs);
      }
      const float Z = wave_sum(zs), A = wave_sum(as) / Z, Q = wave_sum(bs) / Z;
      loss_w += -logf(A + 1e-24f) + bpreg * Q;
      const float inv_a = 1.f / (A + 1e-24f);
      float dii = 0.f;
      for (int j = lane; j < N; j += kWave) {
        if (j == i) continue;
        const float v = row[j], s = expf(v - m) / Z, u = sigmoid_f32(r_ii - v), du = u * (1.f - u);
        // d/dR'_j of sum_k f_k s_k = f'_j s_j + s_j (f_j - sum_k f_k s_k)
        float d = -inv_a * s * (u - A - du) + bpreg * s * (2.f * v + v * v - Q);
        if (elu && v <= 0.f) d *= v + alpha;
        row[j] = d;
        dii = fmaf(s, du, dii);
      }
      dii = -inv_a * wave_sum(dii);
      if (elu && raw_ii <= 0.f) dii *= r_ii + alpha;
      if (lane == 0) row[i] = dii;
    }
  }
  publish_partials<kWavesPerBlock>(loss_w, 0.f, 0.f, 1.0f, scratch);
  if (blockIdx.x == 0 && threadIdx.x == 0) advance_step(stats);
}

// one wave per row: candidate j's dO row and d ob into g_Wy / g_By, slot b's dx_0 row through the keep bytes into g_table
__global__ __launch_bounds__(kBlock) void gru4rec_scatter_kernel(
    const float* __restrict__ dO, const float* __restrict__ dob, const float* __restrict__ dx0,
    const int64_t* __restrict__ in_items, const int64_t* __restrict__ targets, const int64_t* __restrict__ samples,
    const uint8_t* __restrict__ keep_e, float ks_e, int B, int S, int HL, int in0, int64_t n_items,
    float* __restrict__ g_Wy, float* __restrict__ g_By, float* __restrict__ g_table) {
  const int lane = lane_id(), N = B + S;
  for (int w = blockIdx.x * kWavesPerBlock + wave_in_block(); w < N + B; w += gridDim.x * kWavesPerBlock) {
    if (w < N) {
      const int64_t id = w < B ? targets[w] : samples[w - B];
      if (id < 0 || id >= n_items) continue;
      for (int k = lane; k < HL; k += kWave) {
        const float v = dO[static_cast<int64_t>(w) * HL + k];
        if (v != 0.f) atomic_add_f32(g_Wy + id * HL + k, v);
      }
      if (lane == 0 && dob[w] != 0.f) atomic_add_f32(g_By + id, dob[w]);
    } else {
      const int b = w - N;
      const int64_t id = in_items[b];
      if (id < 0 || id >= n_items) continue;
      for (int k = lane; k < in0; k += kWave) {
        const int64_t at = static_cast<int64_t>(b) * in0 + k;
        float v = dx0[at];
        if (keep_e) v = keep_e[at] ? v * ks_e : 0.f;
        if (v != 0.f) atomic_add_f32(g_table + id * in0 + k, v);
      }
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
Gru4recDims gru4rec_dims(const hiprec_gru4rec_shape& s) {
  Gru4recDims q{};
  q.n_items = s.n_items;
  q.L = s.n_layers;
  q.D = s.emb_dim;
  q.loss = s.loss;
  for (int l = 0; l < q.L; ++l) q.H[l] = s.hidden[l];
  for (int l = 0; l < q.L; ++l) q.in[l] = l ? q.H[l - 1] : (q.D ? q.D : q.H[q.L - 1]);
  return q;
}

int64_t gru4rec_n_params(const Gru4recDims& q) {
  int64_t n = q.n_items * q.H[q.L - 1] + q.n_items + q.n_items * q.D;
  for (int l = 0; l < q.L; ++l) n += 3ll * q.H[l] * (q.in[l] + q.H[l]) + 6ll * q.H[l];
  return n;
}

Gru4recParams gru4rec_params(float* base, const Gru4recDims& q) {
  Gru4recParams p{};
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += n; return r; };
  p.Wy = take(q.n_items * q.H[q.L - 1]);
  p.By = take(q.n_items);
  p.E = q.D ? take(q.n_items * q.D) : nullptr;
  for (int l = 0; l < q.L; ++l) {
    p.l[l].wih = take(3ll * q.H[l] * q.in[l]);
    p.l[l].whh = take(3ll * q.H[l] * q.H[l]);
    p.l[l].bih = take(3ll * q.H[l]);
    p.l[l].bhh = take(3ll * q.H[l]);
  }
  return p;
}

struct Gru4recWorkspace {
  float *x0, *O, *ob, *dob, *R, *dO, *da, *db, *cs;
  float *hp[kGru4recMaxLayers], *Gi[kGru4recMaxLayers], *Gh[kGru4recMaxLayers], *act[kGru4recMaxLayers];
  int64_t floats;
};

Gru4recWorkspace gru4rec_carve(float* base, const Gru4recDims& q, int64_t B, int64_t S) {
  Gru4recWorkspace w{};
  const int64_t N = B + S, HL = q.H[q.L - 1];
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += (n + 3) / 4 * 4; return r; };
  int wide = q.in[0];
  w.x0 = take(B * q.in[0]);
  for (int l = 0; l < q.L; ++l) {
    w.hp[l] = take(B * q.H[l]);
    w.Gi[l] = take(B * 3 * q.H[l]);
    w.Gh[l] = take(B * 3 * q.H[l]);
    w.act[l] = take(B * q.H[l]);
    wide = std::max(wide, q.H[l]);
  }
  w.O = take(N * HL);
  w.ob = take(N);
  w.dob = take(N);
  w.R = take(B * N);
  w.dO = take(N * HL);
  w.da = take(B * wide);
  w.db = take(B * wide);
  // the fixed-order column sums: d R [B, N] once, then d Gi and d Gh [B, 3 H_l] of one layer at a time
  w.cs = take(std::max(colsum_ws_floats(static_cast<int>(B), static_cast<int>(N)),
                       2 * colsum_ws_floats(static_cast<int>(B), 3 * kGru4recMaxHidden)));
  w.floats = c - base;
  return w;
}

int gru4rec_check_shape(const hiprec_gru4rec_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  HIPREC_REQUIRE(s->n_items >= 1 && s->n_items < (1ll << 31), "GRU4Rec needs 1 <= n_items < 2^31, got %lld",
                 static_cast<long long>(s->n_items));
  HIPREC_REQUIRE(s->n_layers >= 1 && s->n_layers <= kGru4recMaxLayers, "GRU4Rec needs 1 <= len(layers) <= %d (got %d)",
                 kGru4recMaxLayers, s->n_layers);
  for (int l = 0; l < s->n_layers; ++l)
    HIPREC_REQUIRE(s->hidden[l] >= 1 && s->hidden[l] <= kGru4recMaxHidden,
                   "GRU4Rec needs 1 <= layers[%d] <= %d (got %d)", l, kGru4recMaxHidden, s->hidden[l]);
  HIPREC_REQUIRE(s->emb_dim >= 0 && s->emb_dim <= kGru4recMaxDim, "GRU4Rec needs embedding <= %d (got %d)",
                 kGru4recMaxDim, s->emb_dim);
  HIPREC_REQUIRE(s->loss == HIPREC_GRU4REC_BPRMAX || s->loss == HIPREC_GRU4REC_XE, "GRU4Rec: unknown loss %d", s->loss);
  return 0;
}

bool gru4rec_batch_ok(int64_t B, int64_t S) { return B >= 1 && B <= kGru4recMaxBatch && S >= 0 && S <= kGru4recMaxSample; }

int gru4rec_run(const Gru4recDims& q, float* w_flat, float* g_flat, float* const* state, const int64_t* in_items,
                const int64_t* targets, const uint8_t* reset, const int64_t* samples, int B, int S, const float* log_p,
                float logq, float sample_alpha, float bpreg, float elu_param, const uint8_t* const* keep, float ks_e,
                float ks_h, float* h_out, hiprec_stats* stats, Scratch* scratch, float* ws_base, hipStream_t st) {
  const bool train = g_flat != nullptr;
  const int L = q.L, HL = q.H[L - 1], N = B + S, in0 = q.in[0];
  const Gru4recParams w = gru4rec_params(w_flat, q);
  const Gru4recWorkspace a = gru4rec_carve(ws_base, q, B, S);
  if (!train) keep = nullptr;
  const uint8_t* keep_e = keep ? keep[0] : nullptr;

  Gru4recGather ga{};
  ga.table = q.D ? w.E : w.Wy;
  ga.Wy = w.Wy; ga.By = w.By;
  ga.log_p = (q.loss == HIPREC_GRU4REC_XE && logq != 0.f) ? log_p : nullptr;
  ga.in_items = in_items; ga.targets = targets; ga.samples = samples; ga.reset = reset; ga.keep_e = keep_e;
  ga.ks_e = ks_e; ga.logq = logq; ga.alpha = sample_alpha;
  ga.B = B; ga.S = S; ga.L = L; ga.in0 = in0; ga.HL = HL;
  for (int l = 0; l < L; ++l) {
    ga.H[l] = q.H[l];
    ga.state[l] = state[l];
    ga.hp[l] = a.hp[l];
  }
  ga.x0 = a.x0; ga.O = a.O; ga.ob = a.ob; ga.dob = a.dob;
  ga.train = train ? 1 : 0;
  const int64_t most = std::max<int64_t>(static_cast<int64_t>(B) * std::max(in0, kGru4recMaxHidden),
                                         train ? static_cast<int64_t>(N) * HL : 0);
  gru4rec_gather_kernel<<<grid_for_threads(most), kBlock, 0, st>>>(ga, q.n_items, stats);
  HIPREC_TRY(hipGetLastError());

  const float* x = a.x0;
  for (int l = 0; l < L; ++l) {
    const int H = q.H[l];
    GemmGroup g{};
    g.n = 2;
    g.p[0] = make_gemm(kNT, B, 3 * H, q.in[l], x, q.in[l], w.l[l].wih, q.in[l], a.Gi[l], 3 * H, w.l[l].bih, 0, nullptr, 0, false);
    g.p[1] = make_gemm(kNT, B, 3 * H, H, a.hp[l], H, w.l[l].whh, H, a.Gh[l], 3 * H, w.l[l].bhh, 0, nullptr, 0, false);
    if (int rc = launch_group(g, st)) return rc;
    float* out = (!train && l == L - 1) ? h_out : a.act[l];
    gru4rec_cell_kernel<<<grid_for_threads(static_cast<int64_t>(B) * H), kBlock, 0, st>>>(
        a.Gi[l], a.Gh[l], a.hp[l], B, H, keep ? keep[1 + l] : nullptr, ks_h, train ? 1 : 0, out, state[l]);
    HIPREC_TRY(hipGetLastError());
    x = out;
  }
  if (!train) return 0;

  const Gru4recParams g = gru4rec_params(g_flat, q);
  const float* h_last = a.act[L - 1];
  {
    GemmGroup p{};
    p.n = 1;
    p.p[0] = make_gemm(kNT, B, N, HL, h_last, HL, a.O, HL, a.R, N, a.ob, 0, nullptr, 0, false);
    if (int rc = launch_group(p, st)) return rc;
  }
  gru4rec_loss_kernel<<<grid_for_waves(B), kBlock, 0, st>>>(a.R, B, N, q.loss, bpreg, elu_param, scratch, stats);
  HIPREC_TRY(hipGetLastError());
  {
    GemmGroup p{};
    p.n = 3;
    p.p[0] = make_gemm(kNN, B, HL, N, a.R, N, a.O, HL, a.da, HL, nullptr, 0, nullptr, 0, false);
    p.p[1] = make_gemm(kTNm, N, HL, B, a.R, N, h_last, HL, a.dO, HL, nullptr, 0, nullptr, 0, false);
    p.p[2] = make_colsum(a.R, B, N, N, a.dob, a.cs);
    p.p[2].ws = a.cs;      // the two-level form for a single slab too: the launch count does not depend on B
    if (int rc = launch_group(p, st)) return rc;
    if (int rc = launch_colsum_reduce(p, st)) return rc;
  }
  float *d_out = a.da, *d_in = a.db;
  for (int l = L - 1; l >= 0; --l) {
    const int H = q.H[l], in = q.in[l];
    gru4rec_cell_bwd_kernel<<<grid_for_threads(static_cast<int64_t>(B) * H), kBlock, 0, st>>>(
        a.Gi[l], a.Gh[l], a.hp[l], d_out, B, H, keep ? keep[1 + l] : nullptr, ks_h);
    HIPREC_TRY(hipGetLastError());
    const float* xl = l ? a.act[l - 1] : a.x0;
    GemmGroup p{};
    p.n = 5;
    p.p[0] = make_gemm(kTNm, 3 * H, in, B, a.Gi[l], 3 * H, xl, in, g.l[l].wih, in, nullptr, 0, nullptr, 0, false);
    p.p[1] = make_gemm(kTNm, 3 * H, H, B, a.Gh[l], 3 * H, a.hp[l], H, g.l[l].whh, H, nullptr, 0, nullptr, 0, false);
    p.p[2] = make_colsum(a.Gi[l], B, 3 * H, 3 * H, g.l[l].bih, a.cs);
    p.p[3] = make_colsum(a.Gh[l], B, 3 * H, 3 * H, g.l[l].bhh, a.cs + colsum_ws_floats(B, 3 * kGru4recMaxHidden));
    p.p[2].ws = a.cs;
    p.p[3].ws = a.cs + colsum_ws_floats(B, 3 * kGru4recMaxHidden);
    p.p[4] = make_gemm(kNN, B, in, 3 * H, a.Gi[l], 3 * H, w.l[l].wih, in, d_in, in, nullptr, 0, nullptr, 0, false);
    if (int rc = launch_group(p, st)) return rc;
    if (int rc = launch_colsum_reduce(p, st)) return rc;
    std::swap(d_out, d_in);
  }
  gru4rec_scatter_kernel<<<grid_for_waves(N + B), kBlock, 0, st>>>(a.dO, a.dob, d_out, in_items, targets, samples, keep_e,
                                                                  ks_e, B, S, HL, in0, q.n_items, g.Wy, g.By,
                                                                  q.D ? g.E : g.Wy);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_gru4rec_shape_bytes(void) { return sizeof(hiprec_gru4rec_shape); }

extern "C" int64_t hiprec_gru4rec_param_floats(const hiprec_gru4rec_shape* shape) {
  if (gru4rec_check_shape(shape)) return -1;
  return gru4rec_n_params(gru4rec_dims(*shape));
}

extern "C" size_t hiprec_gru4rec_workspace_bytes(const hiprec_gru4rec_shape* shape, int64_t batch, int32_t n_sample) {
  if (gru4rec_check_shape(shape)) return 0;
  if (!gru4rec_batch_ok(batch, n_sample)) return 0;
  return sizeof(float) * static_cast<size_t>(gru4rec_carve(nullptr, gru4rec_dims(*shape), batch, n_sample).floats);
}

extern "C" int hiprec_gru4rec_grad(const hiprec_gru4rec_shape* shape, const float* w_flat, float* g_flat,
                                   float* const* state, const int64_t* in_items, const int64_t* targets,
                                   const uint8_t* reset, const int64_t* samples, int64_t batch, int32_t n_sample,
                                   const float* log_p, float logq, float sample_alpha, float bpreg, float elu_param,
                                   const uint8_t* const* keep, float ks_embed, float ks_hidden, float* h_out,
                                   hiprec_stats* stats, void* scratch, size_t scratch_bytes, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (int rc = gru4rec_check_shape(shape)) return rc;
  const Gru4recDims q = gru4rec_dims(*shape);
  HIPREC_REQUIRE(w_flat && state && in_items && stats && workspace, "NULL pointer");
  for (int l = 0; l < q.L; ++l) HIPREC_REQUIRE(state[l], "GRU4Rec: the state of layer %d is NULL", l);
  if (!g_flat) n_sample = 0;
  HIPREC_REQUIRE(gru4rec_batch_ok(batch, n_sample), "GRU4Rec needs 1 <= batch <= %d and 0 <= n_sample <= %d (got %lld, %d)",
                 kGru4recMaxBatch, kGru4recMaxSample, static_cast<long long>(batch), n_sample);
  if (g_flat) {
    HIPREC_REQUIRE(batch + n_sample >= 2, "GRU4Rec: a row needs a negative: batch + n_sample >= 2");
    HIPREC_REQUIRE(targets && scratch && (samples || n_sample == 0), "training needs the targets, the samples and the scratch block");
    HIPREC_REQUIRE(!(q.loss == HIPREC_GRU4REC_XE && logq != 0.f) || log_p, "a logQ shift needs log_p");
    if (scratch_bytes < kScratchBytes) {
      set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
      return HIPREC_E_SCRATCH;
    }
  } else {
    HIPREC_REQUIRE(h_out, "the eval step needs the h_out buffer");
  }
  const size_t need = hiprec_gru4rec_workspace_bytes(shape, batch, n_sample);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  return gru4rec_run(q, const_cast<float*>(w_flat), g_flat, state, in_items, targets, reset, samples,
                     static_cast<int>(batch), n_sample, log_p, logq, sample_alpha, bpreg, elu_param, keep, ks_embed,
                     ks_hidden, h_out, stats, static_cast<Scratch*>(scratch), static_cast<float*>(workspace),
                     static_cast<hipStream_t>(stream));
}
