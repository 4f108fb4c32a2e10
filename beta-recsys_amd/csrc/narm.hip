// NARM (beta_rec/models/narm.py): zero_grad + forward + loss + backward of one NARMEngine.train_an_epoch iteration as a
// fixed sequence of launches, no host sync.  Activations are time-major as collate_fn makes the batch: row m = t * B + b.
//
//   embed               X = E[seq] * keep_input (seq_embed of seqrec.hip without a positional row)
//   per GRU layer       Gi = X W_ih^T + b_ih for all T * B rows (one GEMM, outside the recurrence); the recurrence: a
//                       workgroup owns 16 sessions and walks t itself, W_hh stays in LDS for all steps, h W_hh^T on the
//                       fp32 MFMA with the three gates of one (session, unit) in one lane, the gate nonlinearities fused,
//                       every session stops at its own length
//   attention           q1 = gru_out a_1^T, q2 = h_T a_2^T (GEMMs); one wave per session: alpha = v_t . sigmoid(q1 +
//                       [seq > 0] q2) (NO softmax over t), c_local = sum_t alpha gru_out, c_t = drop([c_local, h_T])
//   scores              the factored order: query = c_t b.weight [B, D], scores = query E^T [B, I] -- [I, 2H] never exists
//   cross-entropy       one launch: per row the log-sum-exp over I, the loss partial, dscores in place
//   backward            dquery = dscores E, d emb[1:] = dscores[:, 1:]^T query WRITTEN (row 0 is the padding row and stays
//                       0), d b, d c_t through the hidden keep bytes; attention backward per session; the recurrence in
//                       reverse time with W_hh resident the same way, writing dGi and the n third of dGh per step;
//                       d W_hh, d W_ih, the bias column sums and dX are GEMMs / reductions over the T * B rows afterwards;
//                       dX of the first layer goes through the input keep bytes into emb with row atomics
//
// Saved per layer: the gates r | z | n | (W_hn h + b_hn) [T * B, 4H], gru_out [T * B, H] and h_T; Gi is dropped and its
// buffer becomes dGi.
// W_hh residency: the forward needs 3 * pad16(H) rows of pad4(H) + 1 floats next to two 16-session state tiles, the
// backward 3 * pad4(H) rows of pad16(H) + 1 floats next to the dGh tile and the dh tile; what of that does not fit the
// 160 KB of LDS (H above 108 forward, above 100 backward) is read from the packed copy in global memory (192 KB at
// H = 128: it stays in L2) -- the leading rows stay resident.
#include <algorithm>
#include <vector>

#include "gemm.hpp"
#include "seqrec.hpp"

namespace hiprec {
namespace {

constexpr int kNarmTile = 16;              // sessions of one recurrence workgroup: one MFMA row tile
constexpr int kNarmMaxHidden = 128, kNarmMaxDim = 128, kNarmMaxLayers = 4;
constexpr size_t kNarmLds = 160 * 1024;    // gfx950: LDS per workgroup

inline int pad_to(int n, int q) { return (n + q - 1) / q * q; }

// W_hh [3H, H] twice, zero padded: Wf [3 * Hp][Kp] (forward: rows = gate outputs in 16-tiles, K = inputs) and
// Wb [3 * Kp][Hp] (backward: K = gate outputs, columns = inputs in 16-tiles)
__global__ __launch_bounds__(kBlock) void narm_pack_kernel(const float* __restrict__ W, int H, int Hp, int Kp,
                                                           float* __restrict__ Wf, float* __restrict__ Wb) {
  const int n = 3 * Hp * Kp, stride = gridDim.x * kBlock;
  for (int e = blockIdx.x * kBlock + threadIdx.x; e < n; e += stride) {
    {
      const int row = e / Kp, k = e - row * Kp, g = row / Hp, j = row - g * Hp;
      Wf[e] = (j < H && k < H) ? W[(g * H + j) * H + k] : 0.f;
    }
    {
      const int row = e / Hp, j = e - row * Hp, g = row / Kp, k = row - g * Kp;
      Wb[e] = (k < H && j < H) ? W[(g * H + k) * H + j] : 0.f;
    }
  }
}

// mma16 of seqrec.hpp (same operand layout, A's k stride 1) for the recurrences' long dependent chains: the operands of
// kNarmUnroll k-steps are loaded before their MFMAs issue, so a step pays one LDS / L2 round trip per group instead of
// one per MFMA (the plain loop made a GRU step 10 us at H = 100: 150 load -> MFMA round trips per wave).
constexpr int kNarmUnroll = 5;

__device__ __forceinline__ f32x4 mma16_grouped(f32x4 acc, const float* A, int sai, const float* B, int sbk, int sbj,
                                               int K) {
  const int l = lane_id();
  const float* ap = A + (l & 15) * sai + (l >> 4);
  const float* bp = B + (l >> 4) * sbk + (l & 15) * sbj;
  int k = 0;
  for (; k + 4 * kNarmUnroll <= K; k += 4 * kNarmUnroll) {
    float a[kNarmUnroll], b[kNarmUnroll];
#pragma unroll
    for (int u = 0; u < kNarmUnroll; ++u) {
      a[u] = ap[k + 4 * u];
      b[u] = bp[(k + 4 * u) * sbk];
    }
#pragma unroll
    for (int u = 0; u < kNarmUnroll; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u], acc, 0, 0, 0);
  }
  for (; k < K; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k], bp[k * sbk], acc, 0, 0, 0);
  return acc;
}

// three products that share the A operand (the r, z and n gates of one column tile): B_g(k, j) at Bg[k + j * sbj]
__device__ __forceinline__ void mma16_gates(f32x4 (&acc)[3], const float* A, int sai, const float* B0, const float* B1,
                                            const float* B2, int sbj, int K) {
  const int l = lane_id();
  const float* ap = A + (l & 15) * sai + (l >> 4);
  const int bo = (l >> 4) + (l & 15) * sbj;
  int k = 0;
  for (; k + 4 * kNarmUnroll <= K; k += 4 * kNarmUnroll) {
    float a[kNarmUnroll], b0[kNarmUnroll], b1[kNarmUnroll], b2[kNarmUnroll];
#pragma unroll
    for (int u = 0; u < kNarmUnroll; ++u) {
      a[u] = ap[k + 4 * u];
      b0[u] = B0[bo + k + 4 * u];
      b1[u] = B1[bo + k + 4 * u];
      b2[u] = B2[bo + k + 4 * u];
    }
#pragma unroll
    for (int u = 0; u < kNarmUnroll; ++u) {
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b0[u], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b1[u], acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b2[u], acc[2], 0, 0, 0);
    }
  }
  for (; k < K; k += 4) {
    const float a = ap[k];
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, B0[bo + k], acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, B1[bo + k], acc[1], 0, 0, 0);
    acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, B2[bo + k], acc[2], 0, 0, 0);
  }
}

__device__ __forceinline__ int narm_len(const int64_t* lens, int64_t b, int64_t B, int T) {
  if (b >= B) return 0;
  const int64_t l = lens[b];
  return l < 0 ? 0 : (l > T ? T : static_cast<int>(l));
}

// ---- GRU forward recurrence --------------------------------------------------------------------------------------------
// grid = ceil(B / 16).  LDS: Ws [rows_res][Kp + 1] (the leading rows of Wf), hb [2][16][Hp + 1], s_len [16].
// out [T * B, H] (0 at t >= lens[b]), hT [B, H], gates [T * B, 4H] (training only)
__global__ __launch_bounds__(kBlock) void narm_gru_fwd_kernel(const float* __restrict__ Wf,
                                                              const float* __restrict__ b_hh,
                                                              const float* __restrict__ Gi,
                                                              const int64_t* __restrict__ lens, int64_t B, int T, int H,
                                                              int Hp, int Kp, int rows_res, float* __restrict__ out,
                                                              float* __restrict__ hT, float* __restrict__ gates) {
  extern __shared__ float narm_lds[];
  const int ldw = Kp + 1, ldh = Hp + 1;
  float* Ws = narm_lds;
  float* hb = Ws + rows_res * ldw;
  int* s_len = reinterpret_cast<int*>(hb + 2 * kNarmTile * ldh);
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * kNarmTile;
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_in_block();
  for (int e = tid; e < rows_res * Kp; e += kBlock) {
    const int r = e / Kp, c = e - r * Kp;
    Ws[r * ldw + c] = Wf[e];
  }
  for (int e = tid; e < 2 * kNarmTile * ldh; e += kBlock) hb[e] = 0.f;
  if (tid < kNarmTile) s_len[tid] = narm_len(lens, b0 + tid, B, T);
  __syncthreads();
  int tmax = 0;
#pragma unroll
  for (int i = 0; i < kNarmTile; ++i) tmax = max(tmax, s_len[i]);
  const int n_ct = Hp / 16, col = lane & 15, row0 = 4 * (lane >> 4);
  const int64_t H3 = 3 * static_cast<int64_t>(H), H4 = 4 * static_cast<int64_t>(H);
  for (int t = 0; t < tmax; ++t) {
    const float* hc = hb + (t & 1) * kNarmTile * ldh;
    float* hn = hb + ((t + 1) & 1) * kNarmTile * ldh;
    for (int ct = wave; ct < n_ct; ct += kWavesPerBlock) {
      const int j = ct * 16 + col;
      const bool j_ok = j < H;
      float gi[3][4];
      bool live[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = row0 + r;
        live[r] = t < s_len[i] && j_ok;
        const int64_t m = static_cast<int64_t>(t) * B + b0 + i;
#pragma unroll
        for (int g = 0; g < 3; ++g) gi[g][r] = live[r] ? Gi[m * H3 + g * H + j] : 0.f;
      }
      f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      if (2 * Hp + ct * 16 + 16 <= rows_res) {      // the tile's rows of all three gates are resident
        const float* w0 = Ws + ct * 16 * ldw;
        mma16_gates(acc, hc, ldh, w0, w0 + Hp * ldw, w0 + 2 * Hp * ldw, ldw, Kp);
      } else {
#pragma unroll
        for (int g = 0; g < 3; ++g) {
          const int wrow = g * Hp + ct * 16;
          if (wrow + 16 <= rows_res)
            acc[g] = mma16_grouped(acc[g], hc, ldh, Ws + wrow * ldw, 1, ldw, Kp);
          else
            acc[g] = mma16_grouped(acc[g], hc, ldh, Wf + static_cast<int64_t>(wrow) * Kp, 1, Kp, Kp);
        }
      }
      const float br = j_ok ? b_hh[j] : 0.f, bz = j_ok ? b_hh[H + j] : 0.f, bn = j_ok ? b_hh[2 * H + j] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = row0 + r;
        const float h_old = hc[i * ldh + j];
        float h_new = h_old;
        const int64_t m = static_cast<int64_t>(t) * B + b0 + i;
        if (live[r]) {
          const float rr = sigmoid_f32(gi[0][r] + (acc[0][r] + br));
          const float zz = sigmoid_f32(gi[1][r] + (acc[1][r] + bz));
          const float hp = acc[2][r] + bn;
          const float nn = tanhf(gi[2][r] + rr * hp);
          h_new = (1.f - zz) * nn + zz * h_old;
          out[m * H + j] = h_new;
          if (gates) {
            float* gp = gates + m * H4 + j;
            gp[0] = rr;
            gp[H] = zz;
            gp[2 * H] = nn;
            gp[3 * H] = hp;
          }
        } else if (j_ok && b0 + i < B) {
          out[m * H + j] = 0.f;
        }
        hn[i * ldh + j] = h_new;
      }
    }
    lds_barrier();
  }
  const float* hf = hb + (tmax & 1) * kNarmTile * ldh;
  for (int e = tid; e < kNarmTile * H; e += kBlock) {
    const int i = e / H, j = e - i * H;
    if (b0 + i >= B) continue;
    hT[(b0 + i) * H + j] = hf[i * ldh + j];
    for (int t = tmax; t < T; ++t) out[(static_cast<int64_t>(t) * B + b0 + i) * H + j] = 0.f;
  }
}

// ---- GRU backward recurrence -------------------------------------------------------------------------------------------
// Reverse time.  d h enters as dout_a (+ dout_b) at every step and dhT_a (+ dhT_b) at step lens[b] - 1 (NULL: none).
// LDS: Ws [rows_res][Hp + 1] (the leading rows of Wb), dG [16][3 Kp + 1] (dGh of the tile), dh [16][Hp + 1], s_len.
// Writes dGi [T * B, 3H] and dGhn [T * B, H] (the n third of dGh; its r and z thirds equal dGi's), 0 beyond a length.
__global__ __launch_bounds__(kBlock) void narm_gru_bwd_kernel(
    const float* __restrict__ Wb, const float* __restrict__ gates, const float* __restrict__ out,
    const float* __restrict__ dout_a, const float* __restrict__ dout_b, const float* __restrict__ dhT_a,
    const float* __restrict__ dhT_b, const int64_t* __restrict__ lens, int64_t B, int T, int H, int Hp, int Kp,
    int rows_res, float* __restrict__ dGi, float* __restrict__ dGhn) {
  extern __shared__ float narm_lds[];
  const int ldw = Hp + 1, ldg = 3 * Kp + 1, ldh = Hp + 1;
  float* Ws = narm_lds;
  float* dG = Ws + rows_res * ldw;
  float* dh = dG + kNarmTile * ldg;
  int* s_len = reinterpret_cast<int*>(dh + kNarmTile * ldh);
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * kNarmTile;
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_in_block();
  for (int e = tid; e < rows_res * Hp; e += kBlock) {
    const int r = e / Hp, c = e - r * Hp;
    Ws[r * ldw + c] = Wb[e];
  }
  for (int e = tid; e < kNarmTile * ldg; e += kBlock) dG[e] = 0.f;
  for (int e = tid; e < kNarmTile * ldh; e += kBlock) dh[e] = 0.f;
  if (tid < kNarmTile) s_len[tid] = narm_len(lens, b0 + tid, B, T);
  __syncthreads();
  int tmax = 0;
#pragma unroll
  for (int i = 0; i < kNarmTile; ++i) tmax = max(tmax, s_len[i]);
  const int n_ct = Hp / 16, col = lane & 15, row0 = 4 * (lane >> 4);
  const int64_t H3 = 3 * static_cast<int64_t>(H), H4 = 4 * static_cast<int64_t>(H);
  const int k_all = 3 * Kp;
  // What phase one of step t reads from global memory does not depend on the carry, so it is fetched into registers one
  // step ahead, behind the MFMAs of step t + 1: the loop no longer waits out an HBM / L2 round trip at every step.
  constexpr int kOwn = kNarmTile * kNarmMaxHidden / kBlock;     // elements of the tile a thread owns, at most
  float p_d[kOwn], p_r[kOwn], p_z[kOwn], p_n[kOwn], p_hp[kOwn], p_h[kOwn];
  auto fetch = [&](int t) {
#pragma unroll
    for (int n = 0; n < kOwn; ++n) {
      const int e = tid + n * kBlock;
      p_d[n] = p_r[n] = p_z[n] = p_n[n] = p_hp[n] = p_h[n] = 0.f;
      if (t < 0 || e >= kNarmTile * Kp) continue;
      const int i = e / Kp, j = e - i * Kp;
      if (j >= H || t >= s_len[i]) continue;                     // t < s_len[i] implies b0 + i < B
      const int64_t b = b0 + i, m = static_cast<int64_t>(t) * B + b;
      float d = dout_a[m * H + j];
      if (dout_b) d += dout_b[m * H + j];
      if (t == s_len[i] - 1 && dhT_a) {
        d += dhT_a[b * H + j];
        if (dhT_b) d += dhT_b[b * H + j];
      }
      const float* gp = gates + m * H4 + j;
      p_d[n] = d;
      p_r[n] = gp[0];
      p_z[n] = gp[H];
      p_n[n] = gp[2 * H];
      p_hp[n] = gp[3 * H];
      p_h[n] = t > 0 ? out[(m - B) * H + j] : 0.f;
    }
  };
  fetch(tmax - 1);
  for (int t = tmax - 1; t >= 0; --t) {
#pragma unroll
    for (int n = 0; n < kOwn; ++n) {
      const int e = tid + n * kBlock;
      if (e >= kNarmTile * Kp) continue;
      const int i = e / Kp, j = e - i * Kp;
      const int64_t b = b0 + i, m = static_cast<int64_t>(t) * B + b;
      float d_r = 0.f, d_z = 0.f, d_n = 0.f, d_hn = 0.f;
      if (j < H && b < B) {
        if (t < s_len[i]) {
          const float d = dh[i * ldh + j] + p_d[n];
          const float rr = p_r[n], zz = p_z[n], nn = p_n[n];
          d_n = d * (1.f - zz) * (1.f - nn * nn);
          d_z = d * (p_h[n] - nn) * zz * (1.f - zz);
          d_r = d_n * p_hp[n] * rr * (1.f - rr);
          d_hn = d_n * rr;
          dh[i * ldh + j] = d * zz;
        }
        float* o = dGi + m * H3 + j;
        o[0] = d_r;
        o[H] = d_z;
        o[2 * H] = d_n;
        dGhn[m * H + j] = d_hn;
      }
      dG[i * ldg + j] = d_r;
      dG[i * ldg + Kp + j] = d_z;
      dG[i * ldg + 2 * Kp + j] = d_hn;
    }
    lds_barrier();
    fetch(t - 1);
    for (int ct = wave; ct < n_ct; ct += kWavesPerBlock) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = mma16_grouped(acc, dG, ldg, Ws + ct * 16, ldw, 1, rows_res);
      if (rows_res < k_all)
        acc = mma16_grouped(acc, dG + rows_res, ldg, Wb + static_cast<int64_t>(rows_res) * Hp + ct * 16, Hp, 1,
                            k_all - rows_res);
#pragma unroll
      for (int r = 0; r < 4; ++r) dh[(row0 + r) * ldh + ct * 16 + col] += acc[r];
    }
    lds_barrier();
  }
  for (int e = tid; e < kNarmTile * H; e += kBlock) {
    const int i = e / H, j = e - i * H;
    if (b0 + i >= B) continue;
    for (int t = tmax; t < T; ++t) {
      const int64_t m = static_cast<int64_t>(t) * B + b0 + i;
      float* o = dGi + m * H3 + j;
      o[0] = 0.f;
      o[H] = 0.f;
      o[2 * H] = 0.f;
      dGhn[m * H + j] = 0.f;
    }
  }
}

// ---- attention: one wave per session, H <= 128 = two values per lane ----------------------------------------------------
// alpha [T * B]; ct [B, 2H] = ([c_local, h_T]) through the hidden keep bytes
__global__ __launch_bounds__(kBlock) void narm_attn_fwd_kernel(
    const float* __restrict__ out, const float* __restrict__ hT, const float* __restrict__ q1,
    const float* __restrict__ q2, const float* __restrict__ v, const int64_t* __restrict__ seq,
    const int64_t* __restrict__ lens, const uint8_t* __restrict__ keep, float ks, int64_t B, int T, int H,
    float* __restrict__ alpha, float* __restrict__ ct) {
  const int lane = lane_id();
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); b < B;
       b += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const int len = narm_len(lens, b, B, T);
    float q[2], vv[2], c[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = lane + 64 * h;
      q[h] = j < H ? q2[b * H + j] : 0.f;
      vv[h] = j < H ? v[j] : 0.f;
    }
    for (int t = 0; t < len; ++t) {
      const int64_t m = static_cast<int64_t>(t) * B + b;
      const bool on = seq[m] > 0;
      float o[2], part = 0.f;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        o[h] = 0.f;
        if (j < H) {
          o[h] = out[m * H + j];
          part += vv[h] * sigmoid_f32(q1[m * H + j] + (on ? q[h] : 0.f));
        }
      }
      const float a = wave_sum(part);
      if (lane == 0) alpha[m] = a;
      c[0] += a * o[0];
      c[1] += a * o[1];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = lane + 64 * h;
      if (j < H) {
        const int64_t i0 = b * 2 * H + j, i1 = i0 + H;
        float x0 = c[h], x1 = hT[b * H + j];
        if (keep) {
          x0 = keep[i0] ? x0 * ks : 0.f;
          x1 = keep[i1] ? x1 * ks : 0.f;
        }
        ct[i0] = x0;
        ct[i1] = x1;
      }
    }
  }
}

// dct [B, 2H] (already through the keep bytes).  Writes dgo = alpha * dc_local, dq1, vs = dalpha * sigmoid(..) (the rows
// whose column sum is d v_t), all [T * B, H] and 0 beyond a length; dq2 [B, H]; dhT = the h_T half of dct [B, H].
__global__ __launch_bounds__(kBlock) void narm_attn_bwd_kernel(
    const float* __restrict__ out, const float* __restrict__ q1, const float* __restrict__ q2,
    const float* __restrict__ v, const float* __restrict__ alpha, const float* __restrict__ dct,
    const int64_t* __restrict__ seq, const int64_t* __restrict__ lens, int64_t B, int T, int H, float* __restrict__ dgo,
    float* __restrict__ dq1, float* __restrict__ vs, float* __restrict__ dq2, float* __restrict__ dhT) {
  const int lane = lane_id();
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); b < B;
       b += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const int len = narm_len(lens, b, B, T);
    float q[2], vv[2], dc[2], acc[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = lane + 64 * h;
      q[h] = j < H ? q2[b * H + j] : 0.f;
      vv[h] = j < H ? v[j] : 0.f;
      dc[h] = j < H ? dct[b * 2 * H + j] : 0.f;
      if (j < H) dhT[b * H + j] = dct[b * 2 * H + H + j];
    }
    for (int t = 0; t < T; ++t) {
      const int64_t m = static_cast<int64_t>(t) * B + b;
      if (t >= len) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int j = lane + 64 * h;
          if (j < H) {
            dgo[m * H + j] = 0.f;
            dq1[m * H + j] = 0.f;
            vs[m * H + j] = 0.f;
          }
        }
        continue;
      }
      const bool on = seq[m] > 0;
      float s[2] = {0.f, 0.f}, part = 0.f;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        if (j < H) {
          part += dc[h] * out[m * H + j];
          s[h] = sigmoid_f32(q1[m * H + j] + (on ? q[h] : 0.f));
        }
      }
      const float da = wave_sum(part), a = alpha[m];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        if (j < H) {
          const float dpre = da * vv[h] * s[h] * (1.f - s[h]);
          dgo[m * H + j] = a * dc[h];
          vs[m * H + j] = da * s[h];
          dq1[m * H + j] = dpre;
          if (on) acc[h] += dpre;
        }
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = lane + 64 * h;
      if (j < H) dq2[b * H + j] = acc[h];
    }
  }
}

// ---- cross-entropy over the whole catalogue: a block per row, any I -----------------------------------------------------
__device__ __forceinline__ float block_reduce(float v, float* s_red, bool is_max) {
  v = is_max ? wave_max(v) : wave_sum(v);
  __syncthreads();
  if (lane_id() == 0) s_red[wave_in_block()] = v;
  __syncthreads();
  float r = s_red[0];
#pragma unroll
  for (int i = 1; i < kWavesPerBlock; ++i) r = is_max ? fmaxf(r, s_red[i]) : r + s_red[i];
  return r;
}

// scores [B, I] -> dscores = (softmax - onehot) / B in place; the block's loss partial; block 0 advances the step
__global__ __launch_bounds__(kBlock) void narm_ce_kernel(float* __restrict__ scores, const int64_t* __restrict__ target,
                                                         int64_t B, int64_t I, Scratch* scratch, hiprec_stats* stats) {
  __shared__ float s_red[kWavesPerBlock];
  const float inv_b = 1.0f / static_cast<float>(B);
  float loss = 0.f;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    float* row = scores + b * I;
    float mx = -INFINITY;
    for (int64_t i = threadIdx.x; i < I; i += kBlock) mx = fmaxf(mx, row[i]);
    mx = block_reduce(mx, s_red, true);
    float sum = 0.f;
    for (int64_t i = threadIdx.x; i < I; i += kBlock) sum += expf(row[i] - mx);
    sum = block_reduce(sum, s_red, false);
    const float lse = mx + logf(sum);
    const int64_t tg = target[b];
    const bool ok = tg >= 0 && tg < I;
    if (!ok && threadIdx.x == 0) atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
    if (ok) loss += lse - row[tg];       // every thread reads it before anyone overwrites the row
    __syncthreads();
    for (int64_t i = threadIdx.x; i < I; i += kBlock) {
      float p = expf(row[i] - lse);
      if (i == tg) p -= 1.f;
      row[i] = ok ? p * inv_b : 0.f;
    }
  }
  if (threadIdx.x == 0) {
    scratch->partials[blockIdx.x] = make_float4(loss * inv_b, 0.f, 0.f, 0.f);
    if (blockIdx.x == 0) {
      scratch->n_partials = gridDim.x;
      advance_step(stats);
    }
  }
}

// d emb[seq] += dX through the input keep bytes: row atomics; id 0, ids out of range and t >= lens[b] are skipped
__global__ __launch_bounds__(kBlock) void narm_embed_bwd_kernel(const float* __restrict__ dX,
                                                                const int64_t* __restrict__ seq,
                                                                const int64_t* __restrict__ lens, int64_t B, int T, int D,
                                                                int64_t I, const uint8_t* __restrict__ keep, float ks,
                                                                float* __restrict__ g_emb) {
  const int64_t n = static_cast<int64_t>(T) * B * D, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
    const int64_t m = e / D;
    const int d = static_cast<int>(e - m * D);
    const int64_t t = m / B, b = m - t * B;
    const int64_t id = seq[m];
    if (id <= 0 || id >= I || t >= lens[b]) continue;
    float gv = dX[e];
    if (keep) gv = keep[e] ? gv * ks : 0.f;
    if (gv != 0.f) atomic_add_f32(g_emb + id * D + d, gv);
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
struct NarmParams {      // pointers into a flat buffer laid out in state_dict() order
  float *emb, *a1, *a2, *vt, *bw;
  float *w_ih[kNarmMaxLayers], *w_hh[kNarmMaxLayers], *b_ih[kNarmMaxLayers], *b_hh[kNarmMaxLayers];
};

int64_t narm_n_params(const hiprec_narm_shape& s) {
  const int64_t D = s.emb_dim, H = s.hidden;
  int64_t n = s.n_items * D;
  for (int l = 0; l < s.n_layers; ++l) n += 3 * H * (l == 0 ? D : H) + 3 * H * H + 6 * H;
  return n + 2 * H * H + H + 2 * H * D;
}

NarmParams narm_params(float* base, const hiprec_narm_shape& s) {
  NarmParams p{};
  const int64_t D = s.emb_dim, H = s.hidden;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += n; return r; };
  p.emb = take(s.n_items * D);
  for (int l = 0; l < s.n_layers; ++l) {
    p.w_ih[l] = take(3 * H * (l == 0 ? D : H));
    p.w_hh[l] = take(3 * H * H);
    p.b_ih[l] = take(3 * H);
    p.b_hh[l] = take(3 * H);
  }
  p.a1 = take(H * H);
  p.a2 = take(H * H);
  p.vt = take(H);
  p.bw = take(2 * H * D);
  return p;
}

struct NarmWorkspace {
  float *x, *gi, *q1, *q2, *alpha, *ct, *query, *scores;
  float *out[kNarmMaxLayers], *gates[kNarmMaxLayers], *hT[kNarmMaxLayers], *wf[kNarmMaxLayers], *wb[kNarmMaxLayers];
  float *dquery, *dct, *dgo, *dq1, *vs, *dq2, *dhT, *dgo2, *dhT2, *dgi, *dghn, *dx, *cs;
  int64_t floats;
};

NarmWorkspace narm_carve(float* base, const hiprec_narm_shape& s, int64_t B, int T, bool train) {
  NarmWorkspace w{};
  const int64_t H = s.hidden, D = s.emb_dim, M = B * T, Hp = pad_to(s.hidden, 16), Kp = pad_to(s.hidden, 4);
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += (n + 3) / 4 * 4; return r; };
  w.x = take(M * D);
  w.gi = take(M * 3 * H);
  for (int l = 0; l < s.n_layers; ++l) {
    w.out[l] = take(M * H);
    w.hT[l] = take(B * H);
    w.wf[l] = take(3 * Hp * Kp);
    w.wb[l] = take(3 * Hp * Kp);
    if (train) w.gates[l] = take(M * 4 * H);
  }
  w.q1 = take(M * H);
  w.q2 = take(B * H);
  w.alpha = take(M);
  w.ct = take(B * 2 * H);
  w.query = take(B * D);
  if (train) {
    w.scores = take(B * s.n_items);
    w.dquery = take(B * D);
    w.dct = take(B * 2 * H);
    w.dgo = take(M * H);
    w.dq1 = take(M * H);
    w.vs = take(M * H);
    w.dq2 = take(B * H);
    w.dhT = take(B * H);
    w.dgo2 = w.q1;      // q1 is last read by the attention backward, which runs before the GEMM that writes dgo2
    w.dhT2 = take(B * H);
    w.dgi = w.gi;       // Gi is last read by the last forward recurrence: the backward works from the saved gates
    w.dghn = take(M * H);
    w.dx = take(M * std::max(D, H));
    w.cs = take(3 * colsum_ws_floats(static_cast<int>(M), static_cast<int>(3 * H)));
  }
  w.floats = c - base;
  return w;
}

int narm_check_shape(const hiprec_narm_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  HIPREC_REQUIRE(s->n_items >= 2, "NARM needs n_items >= 2 (the padding id is counted), got %lld",
                 static_cast<long long>(s->n_items));
  HIPREC_REQUIRE(s->hidden >= 1 && s->hidden <= kNarmMaxHidden, "NARM needs 1 <= hidden_size <= %d (got %d)",
                 kNarmMaxHidden, s->hidden);
  HIPREC_REQUIRE(s->emb_dim >= 1 && s->emb_dim <= kNarmMaxDim, "NARM needs 1 <= embedding_dim <= %d (got %d)",
                 kNarmMaxDim, s->emb_dim);
  HIPREC_REQUIRE(s->n_layers >= 1 && s->n_layers <= kNarmMaxLayers, "NARM needs 1 <= n_layers <= %d (got %d)",
                 kNarmMaxLayers, s->n_layers);
  return 0;
}

// rows of the packed W_hh that stay in LDS (a multiple of `quantum`) and the dynamic LDS of the launch
void narm_residency(int row_floats, int rows_all, int other_floats, int quantum, int* rows_res, size_t* bytes) {
  const size_t fixed = sizeof(float) * other_floats + sizeof(int) * kNarmTile;
  int rows = static_cast<int>((kNarmLds - fixed) / (sizeof(float) * row_floats));
  rows = std::min(rows_all, rows / quantum * quantum);
  *rows_res = rows;
  *bytes = fixed + sizeof(float) * static_cast<size_t>(rows) * row_floats;
}

int narm_run(const hiprec_narm_shape& s, float* w_flat, float* g_flat, const int64_t* seq, const int64_t* lens,
             const int64_t* target, int64_t B, int T, const uint8_t* const* keep, float ks_in, float ks_hid,
             float* query_out, hiprec_stats* stats, Scratch* scratch, float* ws_base, hipStream_t st) {
  const int H = s.hidden, D = s.emb_dim, L = s.n_layers, Hp = pad_to(H, 16), Kp = pad_to(H, 4);
  const int64_t M = B * T, I = s.n_items;
  const int Mi = static_cast<int>(M), Bi = static_cast<int>(B), Ii = static_cast<int>(I);
  const bool train = g_flat != nullptr;
  const NarmParams w = narm_params(w_flat, s);
  const NarmWorkspace a = narm_carve(ws_base, s, B, T, train);
  const uint8_t* keep_in = train && keep ? keep[0] : nullptr;
  const uint8_t* keep_hid = train && keep ? keep[1] : nullptr;
  const int tiles = static_cast<int>((B + kNarmTile - 1) / kNarmTile);

  static std::atomic<uint64_t> lds_ok{0};
  if (int rc = allow_dynamic_lds({reinterpret_cast<const void*>(&narm_gru_fwd_kernel),
                                  reinterpret_cast<const void*>(&narm_gru_bwd_kernel)},
                                 kNarmLds, lds_ok, "NARM's GRU recurrence"))
    return rc;
  int res_f, res_b;
  size_t lds_f, lds_b;
  narm_residency(Kp + 1, 3 * Hp, 2 * kNarmTile * (Hp + 1), 16, &res_f, &lds_f);
  narm_residency(Hp + 1, 3 * Kp, kNarmTile * (3 * Kp + 1) + kNarmTile * (Hp + 1), 4, &res_b, &lds_b);

  if (int rc = seq_embed(w.emb, nullptr, seq, M, T, D, I - 1, 1.0f, keep_in, ks_in, a.x, stats, st)) return rc;
  for (int l = 0; l < L; ++l) {
    const int din = l == 0 ? D : H;
    const float* xin = l == 0 ? a.x : a.out[l - 1];
    narm_pack_kernel<<<grid_for_threads(3 * Hp * Kp), kBlock, 0, st>>>(w.w_hh[l], H, Hp, Kp, a.wf[l], a.wb[l]);
    HIPREC_TRY(hipGetLastError());
    GemmGroup g{};
    g.n = 1;
    g.p[0] = make_gemm(kNT, Mi, 3 * H, din, xin, din, w.w_ih[l], din, a.gi, 3 * H, w.b_ih[l], 0, nullptr, 0, false);
    if (int rc = launch_group(g, st)) return rc;
    narm_gru_fwd_kernel<<<tiles, kBlock, lds_f, st>>>(a.wf[l], w.b_hh[l], a.gi, lens, B, T, H, Hp, Kp, res_f, a.out[l],
                                                      a.hT[l], train ? a.gates[l] : nullptr);
    HIPREC_TRY(hipGetLastError());
  }
  const float* top = a.out[L - 1];
  const float* hT = a.hT[L - 1];
  {
    GemmGroup g{};
    g.n = 2;
    g.p[0] = make_gemm(kNT, Mi, H, H, top, H, w.a1, H, a.q1, H, nullptr, 0, nullptr, 0, false);
    g.p[1] = make_gemm(kNT, Bi, H, H, hT, H, w.a2, H, a.q2, H, nullptr, 0, nullptr, 0, false);
    if (int rc = launch_group(g, st)) return rc;
  }
  narm_attn_fwd_kernel<<<grid_for_waves(B), kBlock, 0, st>>>(top, hT, a.q1, a.q2, w.vt, seq, lens, keep_hid, ks_hid, B, T,
                                                             H, a.alpha, a.ct);
  HIPREC_TRY(hipGetLastError());
  float* query = train ? a.query : query_out;
  {
    GemmGroup g{};
    g.n = 1;
    g.p[0] = make_gemm(kNN, Bi, D, 2 * H, a.ct, 2 * H, w.bw, D, query, D, nullptr, 0, nullptr, 0, false);
    if (int rc = launch_group(g, st)) return rc;
  }
  if (!train) return 0;

  const NarmParams g = narm_params(g_flat, s);
  {
    GemmGroup q{};
    q.n = 1;
    q.p[0] = make_gemm(kNT, Bi, Ii, D, query, D, w.emb, D, a.scores, Ii, nullptr, 0, nullptr, 0, false);
    if (int rc = launch_group(q, st)) return rc;
  }
  narm_ce_kernel<<<static_cast<int>(std::min<int64_t>(B, kMaxBlocks)), kBlock, 0, st>>>(a.scores, target, B, I, scratch,
                                                                                        stats);
  HIPREC_TRY(hipGetLastError());
  HIPREC_TRY(hipMemsetAsync(a.dquery, 0, sizeof(float) * B * D, st));
  {
    // d emb[1:] is WRITTEN here (the padding row's gradient stays 0); the lookup's row atomics come last
    GemmGroup q{};
    q.n = 2;
    q.p[0] = make_gemm(kNN, Bi, D, Ii, a.scores, Ii, w.emb, D, a.dquery, D, nullptr, 0, nullptr, 0, true);
    q.p[1] = make_gemm(kTNm, Ii - 1, D, Bi, a.scores + 1, Ii, query, D, g.emb + D, D, nullptr, 0, nullptr, 0, false);
    if (int rc = launch_group(q, st)) return rc;
  }
  {
    GemmGroup q{};
    q.n = 2;
    q.p[0] = make_gemm(kNT, Bi, 2 * H, D, a.dquery, D, w.bw, D, a.dct, 2 * H, nullptr, 0, nullptr, 0, false);
    if (keep_hid) { q.p[0].keep = keep_hid; q.p[0].ldk = 2 * H; q.p[0].keep_scale = ks_hid; }
    q.p[1] = make_gemm(kTNm, 2 * H, D, Bi, a.ct, 2 * H, a.dquery, D, g.bw, D, nullptr, 0, nullptr, 0, true);
    if (int rc = launch_group(q, st)) return rc;
  }
  narm_attn_bwd_kernel<<<grid_for_waves(B), kBlock, 0, st>>>(top, a.q1, a.q2, w.vt, a.alpha, a.dct, seq, lens, B, T, H,
                                                             a.dgo, a.dq1, a.vs, a.dq2, a.dhT);
  HIPREC_TRY(hipGetLastError());
  {
    GemmGroup q{};
    q.n = 5;
    q.p[0] = make_gemm(kNN, Mi, H, H, a.dq1, H, w.a1, H, a.dgo2, H, nullptr, 0, nullptr, 0, false);
    q.p[1] = make_gemm(kTNm, H, H, Mi, a.dq1, H, top, H, g.a1, H, nullptr, 0, nullptr, 0, true);
    q.p[2] = make_gemm(kNN, Bi, H, H, a.dq2, H, w.a2, H, a.dhT2, H, nullptr, 0, nullptr, 0, false);
    q.p[3] = make_gemm(kTNm, H, H, Bi, a.dq2, H, hT, H, g.a2, H, nullptr, 0, nullptr, 0, true);
    q.p[4] = make_colsum(a.vs, Mi, H, H, g.vt, a.cs);
    if (int rc = launch_group(q, st)) return rc;
    if (int rc = launch_colsum_reduce(q, st)) return rc;
  }
  const int64_t cs_part = colsum_ws_floats(Mi, 3 * H);
  for (int l = L - 1; l >= 0; --l) {
    const bool is_top = l == L - 1;
    const int din = l == 0 ? D : H;
    const float* xin = l == 0 ? a.x : a.out[l - 1];
    narm_gru_bwd_kernel<<<tiles, kBlock, lds_b, st>>>(a.wb[l], a.gates[l], a.out[l], is_top ? a.dgo : a.dx,
                                                      is_top ? a.dgo2 : nullptr, is_top ? a.dhT : nullptr,
                                                      is_top ? a.dhT2 : nullptr, lens, B, T, H, Hp, Kp, res_b, a.dgi,
                                                      a.dghn);
    HIPREC_TRY(hipGetLastError());
    GemmGroup q{};
    int n = 0;
    q.p[n++] = make_gemm(kNN, Mi, din, 3 * H, a.dgi, 3 * H, w.w_ih[l], din, a.dx, din, nullptr, 0, nullptr, 0, false);
    q.p[n++] = make_gemm(kTNm, 3 * H, din, Mi, a.dgi, 3 * H, xin, din, g.w_ih[l], din, nullptr, 0, nullptr, 0, true);
    q.p[n++] = make_colsum(a.dgi, Mi, 3 * H, 3 * H, g.b_ih[l], a.cs);
    q.p[n++] = make_colsum(a.dgi, Mi, 2 * H, 3 * H, g.b_hh[l], a.cs + cs_part);
    q.p[n++] = make_colsum(a.dghn, Mi, H, H, g.b_hh[l] + 2 * H, a.cs + 2 * cs_part);
    if (T > 1) {      // h_{t-1} of row (t, b) is gru_out's row (t - 1, b); h_0 = 0 contributes nothing
      const int Mr = static_cast<int>(M - B);
      q.p[n++] = make_gemm(kTNm, 2 * H, H, Mr, a.dgi + B * 3 * H, 3 * H, a.out[l], H, g.w_hh[l], H, nullptr, 0, nullptr,
                           0, true);
      q.p[n++] = make_gemm(kTNm, H, H, Mr, a.dghn + B * H, H, a.out[l], H, g.w_hh[l] + 2 * H * H, H, nullptr, 0, nullptr,
                           0, true);
    }
    q.n = n;
    if (int rc = launch_group(q, st)) return rc;
    if (int rc = launch_colsum_reduce(q, st)) return rc;
  }
  narm_embed_bwd_kernel<<<grid_for_threads(M * D), kBlock, 0, st>>>(a.dx, seq, lens, B, T, D, I, keep_in, ks_in, g.emb);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_narm_shape_bytes(void) { return sizeof(hiprec_narm_shape); }

extern "C" int64_t hiprec_narm_param_floats(const hiprec_narm_shape* shape) {
  if (narm_check_shape(shape)) return -1;
  return narm_n_params(*shape);
}

extern "C" size_t hiprec_narm_workspace_bytes(const hiprec_narm_shape* shape, int64_t batch, int32_t seq_len) {
  if (narm_check_shape(shape) || batch <= 0 || seq_len <= 0) return 0;
  return sizeof(float) * static_cast<size_t>(narm_carve(nullptr, *shape, batch, seq_len, true).floats);
}

extern "C" int hiprec_narm_grad(const hiprec_narm_shape* shape, const float* w_flat, float* g_flat, const int64_t* seq,
                                const int64_t* lens, const int64_t* target, int64_t batch, int32_t seq_len,
                                const uint8_t* const* keep, float keep_scale_input, float keep_scale_hidden,
                                float* query_out, hiprec_stats* stats, void* scratch, size_t scratch_bytes,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = narm_check_shape(shape)) return rc;
  HIPREC_REQUIRE(w_flat && seq && lens && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(batch >= 1 && seq_len >= 1, "bad batch / sequence length");
  HIPREC_REQUIRE(batch * seq_len < (1ll << 24), "batch x sequence length must stay below 2^24");
  HIPREC_REQUIRE(shape->n_items < (1ll << 31) && batch < (1ll << 24), "batch or catalogue too large");
  if (g_flat) {
    HIPREC_REQUIRE(target && scratch, "training needs the targets and the scratch block");
    if (scratch_bytes < kScratchBytes) {
      set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
      return HIPREC_E_SCRATCH;
    }
  } else {
    HIPREC_REQUIRE(query_out, "the eval-mode forward needs a query buffer");
  }
  const size_t need = hiprec_narm_workspace_bytes(shape, batch, seq_len);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  return narm_run(*shape, const_cast<float*>(w_flat), g_flat, seq, lens, target, batch, seq_len, keep, keep_scale_input,
                  keep_scale_hidden, query_out, stats, static_cast<Scratch*>(scratch), static_cast<float*>(workspace),
                  static_cast<hipStream_t>(stream));
}
