// FMLP-Rec (Zhou et al., WWW 2022; no counterpart in the reference, the definition is include/hiprec.h's): zero_grad +
// forward + loss + backward of one training step as a fixed sequence of launches, no host sync.
// Activations are [M = B * T, D] row-major, row m = b * T + t, T = maxlen.  Post-LN, padded positions are not masked.
//
//   embed               raw = E[seq] + P[t] (P[t] alone at padding) -> LN_e (eps 1e-12) -> dropout
//   filter              fml_filter_fwd_kernel: a workgroup owns kFmlSlab = 16 channels of ONE sequence.  The [T, 16] slab
//                       of x and the table of T (cos, sin) pairs sit in LDS.  Product 1 (the rfft): a wave owns 16
//                       frequencies x 16 channels; its A operand is the DFT basis, never stored: lane (k, t) reads
//                       table[(k t) mod T] and advances the index by (4 k) mod T per MFMA step; two accumulators (cos,
//                       sin) share the x operand.  The epilogue multiplies by the complex weight, folds 1 / sqrt(T) and
//                       the multiplicity m_k of the bin in, and leaves (Pr, Pi) in LDS.  Product 2 (the irfft): a wave
//                       owns 16 positions x 16 channels, the basis again from the table, two MFMAs per step into one
//                       accumulator; the epilogue applies the keep bytes.  The spectrum never reaches memory.
//   filter backward     fml_filter_bwd_kernel: grid (D / 16, P), P = min(B, kFmlParts); workgroup (slab, p) walks the
//                       sequences p, p + P, ... in order.  Per sequence it stages x and dy, runs product 1 on both with
//                       ONE table read per step (four accumulators: X recomputed, G), adds X conj-times G to the weight
//                       gradient it keeps in registers, leaves the spectrum of dx in LDS and runs product 2.  Its weight
//                       gradient goes to part[p]; fml_fold_kernel adds the P partials in order.  No atomics.
//   per block           fl = drop(filter(x)); h = LN_1(x + fl); pre = fc1(h) (GEMM); GELU; z = drop(fc2(.)) (GEMM
//                       epilogue); x' = LN_2(h + z).  LayerNorm through seq_ln_fwd / seq_ln_bwd without the padding mask.
//   loss                the last position of every sequence is gathered into [B, D]; BCE-with-logits over the rows with
//                       pos != 0 (seq_loss) with the count clamped to 1 on the device: a batch without a label gives
//                       loss 0 and a zero gradient.
//   backward            the chain in reverse: LayerNorm backward (fixed-order column sums), GELU backward, dgrad / wgrad /
//                       bias GEMM groups (weight gradients in up to 8 slabs of the batch, folded in slab order), the
//                       filter backward, embed backward (row atomics into the item rows, pos_emb in a fixed order).
//
// Every gradient except item_emb.weight is the same bits on every run.
#include <algorithm>
#include <cmath>

#include "gemm.hpp"
#include "seqrec.hpp"

namespace hiprec {
namespace {

constexpr int kFmlSlab = 16;                                 // channels a filter workgroup owns
constexpr int kFmlMaxBins = kSeqMaxLen / 2 + 1;              // F at maxlen 256
constexpr int kFmlBinRows = (kFmlMaxBins + 15) / 16 * 16;    // spectrum rows in LDS: whole bin tiles
constexpr int kFmlOwnBins = (kFmlBinRows / 16 + kWavesPerBlock - 1) / kWavesPerBlock;   // bin tiles a wave owns
constexpr int kFmlParts = 64;                                // workgroups per slab of the filter backward
constexpr int kFmlMaxBlocks = 16;
constexpr int kFmlMaxFfn = 512;
constexpr int kFmlSlabs = 8;                                 // batch slabs of a weight-gradient GEMM
constexpr float kFmlEps = 1e-12f;

// ---- the filter ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 fml_mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// rows [0, T4) x 16 channels of one sequence (src at its first row and channel) into dst[T4][16]; rows >= T are 0
__device__ __forceinline__ void fml_stage(float* dst, const float* __restrict__ src, int T, int T4, int D) {
  for (int e = threadIdx.x; e < T4 * kFmlSlab; e += kBlock) {
    const int r = e >> 4, c = e & 15;
    dst[e] = r < T ? src[static_cast<int64_t>(r) * D + c] : 0.f;
  }
}

// Product 1 on bin tile kt: re[n] = sum_t cos(theta) in_n[t], im[n] = sum_t sin(theta) in_n[t], theta = 2 pi (k t mod T) / T,
// as a [16 bins, 16 channels] MFMA tile.  Lane l feeds basis element (k = 16 kt + (l & 15), t = (l >> 4) + 4 step).
template <int NIN>
__device__ __forceinline__ void fml_analyse(const float2* tw, const float* in0, const float* in1, int T, int T4, int kt,
                                            f32x4 (&re)[NIN], f32x4 (&im)[NIN]) {
  const int l = lane_id(), kf = kt * 16 + (l & 15), off = (l >> 4) * kFmlSlab + (l & 15);
  int idx = (kf * (l >> 4)) % T;
  const int inc = (4 * kf) % T;
#pragma unroll
  for (int n = 0; n < NIN; ++n) re[n] = im[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < T4; t += 4) {
    const float2 w = tw[idx];
    const float a = in0[off + t * kFmlSlab];
    re[0] = fml_mfma(w.x, a, re[0]);
    im[0] = fml_mfma(w.y, a, im[0]);
    if (NIN == 2) {
      const float g = in1[off + t * kFmlSlab];
      re[NIN - 1] = fml_mfma(w.x, g, re[NIN - 1]);
      im[NIN - 1] = fml_mfma(w.y, g, im[NIN - 1]);
    }
    idx += inc;
    if (idx >= T) idx -= T;
  }
}

// Product 2 on time tile tt: out[t] = sum_k cos(theta) sp[k].x + sin(theta) sp[k].y over the F4 spectrum rows (zeros past F)
__device__ __forceinline__ f32x4 fml_synthesise(const float2* tw, const float2* sp, int T, int F4, int tt) {
  const int l = lane_id(), tr = tt * 16 + (l & 15);
  int idx = (tr * (l >> 4)) % T;
  const int inc = (4 * tr) % T;
  const float2* bp = sp + (l >> 4) * kFmlSlab + (l & 15);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < F4; k += 4) {
    const float2 w = tw[idx], p = bp[k * kFmlSlab];
    acc = fml_mfma(w.x, p.x, acc);
    acc = fml_mfma(w.y, p.y, acc);
    idx += inc;
    if (idx >= T) idx -= T;
  }
  return acc;
}

// the multiplicity of bin k in the inverse transform times s = 1 / sqrt(T): DC and (T even) Nyquist count once
__device__ __forceinline__ float fml_bin_scale(int k, int T, float s) { return (k == 0 || 2 * k == T) ? s : 2.f * s; }

// y = keep(filter(x)).  grid (B, D / 16).  W [F, D] complex, twiddle [T] (cos, sin) of 2 pi j / T.
__global__ __launch_bounds__(kBlock) void fml_filter_fwd_kernel(const float* __restrict__ x, const float2* __restrict__ W,
                                                                const float2* __restrict__ twiddle, int T, int D,
                                                                const uint8_t* __restrict__ keep, float ks,
                                                                float* __restrict__ y) {
  __shared__ float xs[kSeqMaxLen * kFmlSlab];
  __shared__ float2 sp[kFmlBinRows * kFmlSlab];
  __shared__ float2 tw[kSeqMaxLen];
  const int F = T / 2 + 1, T4 = (T + 3) & ~3, F4 = (F + 3) & ~3, nkt = (F + 15) / 16, ntt = (T + 15) / 16;
  const int lane = lane_id(), wave = wave_in_block(), d0 = blockIdx.y * kFmlSlab;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * T;
  const float s = 1.0f / sqrtf(static_cast<float>(T));
  for (int j = threadIdx.x; j < T; j += kBlock) tw[j] = twiddle[j];
  fml_stage(xs, x + row0 * D + d0, T, T4, D);
  __syncthreads();
  for (int kt = wave; kt < nkt; kt += kWavesPerBlock) {
    f32x4 re[1], im[1];
    fml_analyse<1>(tw, xs, nullptr, T, T4, kt, re, im);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = kt * 16 + 4 * (lane >> 4) + r;
      float2 p = make_float2(0.f, 0.f);
      if (k < F) {
        const float2 w = W[static_cast<int64_t>(k) * D + d0 + (lane & 15)];
        const float xr = s * re[0][r], xi = -s * im[0][r], m = fml_bin_scale(k, T, s);
        p = make_float2(m * (xr * w.x - xi * w.y), -m * (xr * w.y + xi * w.x));
      }
      sp[k * kFmlSlab + (lane & 15)] = p;
    }
  }
  __syncthreads();
  for (int tt = wave; tt < ntt; tt += kWavesPerBlock) {
    const f32x4 acc = fml_synthesise(tw, sp, T, F4, tt);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = tt * 16 + 4 * (lane >> 4) + r;
      if (t < T) {
        const int64_t at = (row0 + t) * D + d0 + (lane & 15);
        y[at] = keep ? (keep[at] ? acc[r] * ks : 0.f) : acc[r];
      }
    }
  }
}

// dx = filter^T(dy) and this workgroup's share of dW.  grid (D / 16, P); part [P, F, D] complex.
__global__ __launch_bounds__(kBlock) void fml_filter_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                const float2* __restrict__ W,
                                                                const float2* __restrict__ twiddle, int64_t B, int T, int D,
                                                                float* __restrict__ dx, float2* __restrict__ part) {
  __shared__ float xs[kSeqMaxLen * kFmlSlab];
  __shared__ float gs[kSeqMaxLen * kFmlSlab];
  __shared__ float2 sp[kFmlBinRows * kFmlSlab];
  __shared__ float2 tw[kSeqMaxLen];
  const int F = T / 2 + 1, T4 = (T + 3) & ~3, F4 = (F + 3) & ~3, nkt = (F + 15) / 16, ntt = (T + 15) / 16;
  const int lane = lane_id(), wave = wave_in_block(), d0 = blockIdx.x * kFmlSlab;
  const float s = 1.0f / sqrtf(static_cast<float>(T));
  for (int j = threadIdx.x; j < T; j += kBlock) tw[j] = twiddle[j];
  float2 wv[kFmlOwnBins][4], dw[kFmlOwnBins][4];
#pragma unroll
  for (int u = 0; u < kFmlOwnBins; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = (wave + kWavesPerBlock * u) * 16 + 4 * (lane >> 4) + r;
      wv[u][r] = k < F ? W[static_cast<int64_t>(k) * D + d0 + (lane & 15)] : make_float2(0.f, 0.f);
      dw[u][r] = make_float2(0.f, 0.f);
    }
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    const int64_t row0 = b * T;
    __syncthreads();      // the sequence before is through with xs, gs and sp
    fml_stage(xs, x + row0 * D + d0, T, T4, D);
    fml_stage(gs, dy + row0 * D + d0, T, T4, D);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kFmlOwnBins; ++u) {
      const int kt = wave + kWavesPerBlock * u;
      if (kt >= nkt) continue;
      f32x4 re[2], im[2];
      fml_analyse<2>(tw, xs, gs, T, T4, kt, re, im);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = kt * 16 + 4 * (lane >> 4) + r;
        float2 p = make_float2(0.f, 0.f);
        if (k < F) {
          const float m = fml_bin_scale(k, T, s);
          const float xr = s * re[0][r], xi = -s * im[0][r], gr = m * re[1][r], gi = -m * im[1][r];
          dw[u][r].x += xr * gr + xi * gi;
          dw[u][r].y += xr * gi - xi * gr;
          p = make_float2(s * (gr * wv[u][r].x + gi * wv[u][r].y), -s * (gi * wv[u][r].x - gr * wv[u][r].y));
        }
        sp[k * kFmlSlab + (lane & 15)] = p;
      }
    }
    __syncthreads();
    for (int tt = wave; tt < ntt; tt += kWavesPerBlock) {
      const f32x4 acc = fml_synthesise(tw, sp, T, F4, tt);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = tt * 16 + 4 * (lane >> 4) + r;
        if (t < T) dx[(row0 + t) * D + d0 + (lane & 15)] = acc[r];
      }
    }
  }
  float2* dst = part + static_cast<int64_t>(blockIdx.y) * F * D;
#pragma unroll
  for (int u = 0; u < kFmlOwnBins; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = (wave + kWavesPerBlock * u) * 16 + 4 * (lane >> 4) + r;
      if (k < F) dst[static_cast<int64_t>(k) * D + d0 + (lane & 15)] = dw[u][r];
    }
}

// ---- elementwise -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float fml_gelu(float z) { return 0.5f * z * (1.0f + erff(z * 0.70710678118654752440f)); }

__device__ __forceinline__ float fml_gelu_grad(float z) {
  return 0.5f * (1.0f + erff(z * 0.70710678118654752440f)) + z * 0.39894228040143267794f * expf(-0.5f * z * z);
}

__global__ __launch_bounds__(kBlock) void fml_gelu_fwd_kernel(const float* __restrict__ pre, float* __restrict__ act,
                                                              int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) act[i] = fml_gelu(pre[i]);
}

// d pre = d act * gelu'(pre), in place on d
__global__ __launch_bounds__(kBlock) void fml_gelu_bwd_kernel(float* d, const float* __restrict__ pre, int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride)
    d[i] = d[i] * fml_gelu_grad(pre[i]);
}

// out = keep ? (a + b) * ks : 0; b may be NULL
__global__ __launch_bounds__(kBlock) void fml_keep_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          const uint8_t* __restrict__ keep, float ks,
                                                          float* __restrict__ out, int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    float v = a[i];
    if (b) v += b[i];
    out[i] = keep[i] ? v * ks : 0.f;
  }
}

// out[i] = the slabs' partials of i, added in slab order
__global__ __launch_bounds__(kBlock) void fml_fold_kernel(float* __restrict__ out, const float* __restrict__ part,
                                                          int64_t n, int slabs) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    float s = part[i];
    for (int k = 1; k < slabs; ++k) s += part[k * n + i];
    out[i] = s;
  }
}

// raw = E[seq] + P[t]; padding (and an id outside the table, which raises the status) carries P[t] alone
__global__ __launch_bounds__(kBlock) void fml_embed_kernel(const float* __restrict__ E, const float* __restrict__ P,
                                                           const int64_t* __restrict__ seq, int64_t M, int T, int D,
                                                           int64_t n_items, float* __restrict__ raw, hiprec_stats* stats) {
  const int64_t n = M * D, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t m = i / D, id = seq[m];
    const int d = static_cast<int>(i - m * D);
    float v = P[static_cast<int64_t>(m % T) * D + d];
    if (id < 0 || id > n_items) {
      if (d == 0) atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
    } else if (id != 0) {
      v += E[id * D + d];
    }
    raw[i] = v;
  }
}

// d item_emb[seq] += dx (row atomics, id 0 skipped), d pos_emb[t] = sum_b dx over every sequence: one thread per (t, d)
// walks the batch in order, so the positional gradient is the same from run to run
__global__ __launch_bounds__(kBlock) void fml_embed_bwd_kernel(const float* __restrict__ dx,
                                                               const int64_t* __restrict__ seq, int64_t B, int T, int D,
                                                               int64_t n_items, float* __restrict__ g_item,
                                                               float* __restrict__ g_pos) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= T * D) return;
  const int t = e / D, d = e - t * D;
  float acc = 0.f;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t m = b * T + t, id = seq[m];
    const float gv = dx[m * D + d];
    if (id >= 1 && id <= n_items) atomic_add_f32(g_item + id * D + d, gv);
    acc += gv;
  }
  g_pos[e] = acc;
}

// f[b] = x[b, T - 1]
__global__ __launch_bounds__(kBlock) void fml_last_rows_kernel(const float* __restrict__ x, int64_t B, int T, int D,
                                                               float* __restrict__ f) {
  const int64_t n = B * D, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t b = i / D;
    f[i] = x[(b * T + T - 1) * D + (i - b * D)];
  }
}

// dx[b, T - 1] = df[b], every other row 0
__global__ __launch_bounds__(kBlock) void fml_spread_last_kernel(const float* __restrict__ df, int64_t M, int T, int D,
                                                                 float* __restrict__ dx) {
  const int64_t n = M * D, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t m = i / D;
    dx[i] = (m % T == T - 1) ? df[(m / T) * D + (i - m * D)] : 0.f;
  }
}

// aux[0] = max(1, count(pos != 0)) (one block; integers up to 2^24 are exact in fp32), aux[1] = 0: what seq_loss divides by
__global__ __launch_bounds__(kBlock) void fml_count_kernel(const int64_t* __restrict__ pos, int64_t B,
                                                           float* __restrict__ aux) {
  __shared__ float s_red[kBlock];
  float c = 0.f;
  for (int64_t b = threadIdx.x; b < B; b += kBlock) c += pos[b] != 0 ? 1.f : 0.f;
  s_red[threadIdx.x] = c;
  __syncthreads();
  for (int r = kBlock / 2; r > 0; r >>= 1) {
    if (static_cast<int>(threadIdx.x) < r) s_red[threadIdx.x] += s_red[threadIdx.x + r];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    aux[0] = fmaxf(s_red[0], 1.f);
    aux[1] = 0.f;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct FmlBlock {
  float *filt, *ln1_w, *ln1_b, *f1_w, *f1_b, *f2_w, *f2_b, *ln2_w, *ln2_b;
};
struct FmlParams {      // pointers into a flat buffer laid out in state_dict() order
  float *item_emb, *pos_emb, *ln_e_w, *ln_e_b;
  FmlBlock blk[kFmlMaxBlocks];
};

int fml_bins(int T) { return T / 2 + 1; }

int64_t fml_n_params(const hiprec_fmlprec_shape& s) {
  const int64_t D = s.dim, H = s.ffn_dim, F = fml_bins(s.maxlen);
  return (s.n_items + 1) * D + s.maxlen * D + 2 * D + s.n_blocks * (2 * F * D + 2 * D + H * D + H + D * H + D + 2 * D);
}

FmlParams fml_params(float* base, const hiprec_fmlprec_shape& s) {
  FmlParams p{};
  const int64_t D = s.dim, H = s.ffn_dim, F = fml_bins(s.maxlen);
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += n; return r; };
  p.item_emb = take((s.n_items + 1) * D);
  p.pos_emb = take(s.maxlen * D);
  p.ln_e_w = take(D);
  p.ln_e_b = take(D);
  for (int k = 0; k < s.n_blocks; ++k) {
    FmlBlock& q = p.blk[k];
    q.filt = take(2 * F * D);
    q.ln1_w = take(D);
    q.ln1_b = take(D);
    q.f1_w = take(H * D);
    q.f1_b = take(H);
    q.f2_w = take(D * H);
    q.f2_b = take(D);
    q.ln2_w = take(D);
    q.ln2_b = take(D);
  }
  return p;
}

int fml_parts(int64_t B) { return static_cast<int>(std::min<int64_t>(B, kFmlParts)); }

struct FmlSaved {
  float *x, *fl, *h, *pre, *z, *mean1, *rstd1, *mean2, *rstd2;
};
struct FmlWorkspace {
  FmlSaved sv[kFmlMaxBlocks];
  float *raw, *mean_e, *rstd_e, *out, *f, *df, *aux, *t[8], *tf[2], *cs, *part, *fpart;
  int64_t floats;
};

FmlWorkspace fml_carve(float* base, const hiprec_fmlprec_shape& s, int64_t B) {
  FmlWorkspace w{};
  const int64_t T = s.maxlen, D = s.dim, H = s.ffn_dim, M = B * T, MD = M * D, MH = M * H;
  const int wide = static_cast<int>(std::max(D, H));
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += (n + 3) / 4 * 4; return r; };
  for (int k = 0; k < s.n_blocks; ++k)
    w.sv[k] = FmlSaved{take(MD), take(MD), take(MD), take(MH), take(MD), take(M), take(M), take(M), take(M)};
  w.raw = take(MD);
  w.mean_e = take(M);
  w.rstd_e = take(M);
  w.out = take(MD);
  w.f = take(B * D);
  w.df = take(B * D);
  w.aux = take(kSeqAux);
  for (int i = 0; i < 8; ++i) w.t[i] = take(MD);
  for (int i = 0; i < 2; ++i) w.tf[i] = take(MH);
  w.cs = take(2 * colsum_ws_floats(static_cast<int>(M), wide));
  w.part = take(static_cast<int64_t>(kFmlSlabs) * wide * D);
  w.fpart = take(static_cast<int64_t>(fml_parts(B)) * 2 * fml_bins(s.maxlen) * D);
  w.floats = c - base;
  return w;
}

int fml_check_shape(const hiprec_fmlprec_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  HIPREC_REQUIRE(s->n_items >= 1 && s->n_items < (1ll << 31) - 1, "FMLP-Rec needs 1 <= n_items < 2^31 - 1");
  HIPREC_REQUIRE(s->dim >= 16 && s->dim <= kSeqMaxDim && s->dim % 16 == 0,
                 "FMLP-Rec needs emb_dim a multiple of 16 in 16 .. %d (got %d)", kSeqMaxDim, s->dim);
  HIPREC_REQUIRE(s->maxlen >= 1 && s->maxlen <= kSeqMaxLen, "FMLP-Rec needs 1 <= maxlen <= %d (got %d)", kSeqMaxLen,
                 s->maxlen);
  HIPREC_REQUIRE(s->n_blocks >= 1 && s->n_blocks <= kFmlMaxBlocks, "FMLP-Rec needs 1 <= num_blocks <= %d (got %d)",
                 kFmlMaxBlocks, s->n_blocks);
  HIPREC_REQUIRE(s->ffn_dim >= 16 && s->ffn_dim <= kFmlMaxFfn && s->ffn_dim % 16 == 0,
                 "FMLP-Rec needs ffn_dim a multiple of 16 in 16 .. %d (got %d)", kFmlMaxFfn, s->ffn_dim);
  return 0;
}

bool fml_batch_ok(const hiprec_fmlprec_shape& s, int64_t B) { return B >= 1 && B * s.maxlen <= (1ll << 24); }

int fml_filter_fwd(const float* x, const float* W, const float* twiddle, int64_t B, int T, int D, const uint8_t* keep,
                   float ks, float* y, hipStream_t st) {
  fml_filter_fwd_kernel<<<dim3(static_cast<unsigned>(B), D / kFmlSlab), kBlock, 0, st>>>(
      x, reinterpret_cast<const float2*>(W), reinterpret_cast<const float2*>(twiddle), T, D, keep, ks, y);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// dx [B, T, D] and dW [F, D, 2] (plain stores) from dy = the gradient of filter(x); part holds fml_parts(B) partials of dW
int fml_filter_bwd(const float* x, const float* dy, const float* W, const float* twiddle, int64_t B, int T, int D, float* dx,
                   float* dW, float* part, hipStream_t st) {
  const int P = fml_parts(B);
  fml_filter_bwd_kernel<<<dim3(D / kFmlSlab, P), kBlock, 0, st>>>(x, dy, reinterpret_cast<const float2*>(W),
                                                                  reinterpret_cast<const float2*>(twiddle), B, T, D, dx,
                                                                  reinterpret_cast<float2*>(part));
  HIPREC_TRY(hipGetLastError());
  const int64_t n = 2ll * fml_bins(T) * D;
  fml_fold_kernel<<<grid_for_threads(n), kBlock, 0, st>>>(dW, part, n, P);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

void fml_set_keep(GemmProblem& p, const uint8_t* keep, int ld, float ks) {
  if (keep) { p.keep = keep; p.ldk = ld; p.keep_scale = ks; }
}

int fml_gelu_fwd(const float* pre, float* act, int64_t n, hipStream_t st) {
  fml_gelu_fwd_kernel<<<grid_for_threads(n), kBlock, 0, st>>>(pre, act, n);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// C[rows, cols] = A^T B over K batch rows, as problems of g: one with plain stores into the zeroed gradient, or (long K)
// up to kFmlSlabs slabs of K into `part`, which fml_fold adds up in slab order afterwards.  Returns the slab count.
int fml_add_wgrad(GemmGroup& g, int rows, int cols, int K, const float* A, int lda, const float* Bm, int ldb, float* out,
                  float* part) {
  const int slabs = std::min(kFmlSlabs, (K + 511) / 512);
  if (slabs <= 1) {
    g.p[g.n++] = make_gemm(kTNm, rows, cols, K, A, lda, Bm, ldb, out, cols, nullptr, 0, nullptr, 0, false);
    return 1;
  }
  const int per = ((K + slabs - 1) / slabs + 15) / 16 * 16;
  int s = 0;
  for (int k0 = 0; k0 < K; k0 += per, ++s)
    g.p[g.n++] = make_gemm(kTNm, rows, cols, std::min(per, K - k0), A + static_cast<int64_t>(k0) * lda, lda,
                           Bm + static_cast<int64_t>(k0) * ldb, ldb, part + static_cast<int64_t>(s) * rows * cols, cols,
                           nullptr, 0, nullptr, 0, false);
  return s;
}

int fml_fold(float* out, const float* part, int64_t n, int slabs, hipStream_t st) {
  if (slabs <= 1) return 0;
  fml_fold_kernel<<<grid_for_threads(n), kBlock, 0, st>>>(out, part, n, slabs);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

int fml_run(const hiprec_fmlprec_shape& s, float* w_flat, float* g_flat, const int64_t* seq, const int64_t* pos,
            const int64_t* neg, int64_t B, const float* twiddle, const uint8_t* const* keep, float ks, float* feats_out,
            hiprec_stats* stats, Scratch* scratch, float* ws_base, hipStream_t st) {
  const bool train = g_flat != nullptr;
  const int T = s.maxlen, D = s.dim, H = s.ffn_dim, nb = s.n_blocks;
  const int64_t M = B * T, MD = M * D, MH = M * H;
  const int Mi = static_cast<int>(M);
  const FmlParams w = fml_params(w_flat, s);
  const FmlWorkspace a = fml_carve(ws_base, s, B);
  auto kp = [&](int i) -> const uint8_t* { return keep ? keep[i] : nullptr; };

  // ---- forward ----
  fml_embed_kernel<<<grid_for_threads(MD), kBlock, 0, st>>>(w.item_emb, w.pos_emb, seq, M, T, D, s.n_items, a.raw, stats);
  HIPREC_TRY(hipGetLastError());
  if (int rc = seq_ln_fwd(a.raw, nullptr, nullptr, nullptr, w.ln_e_w, w.ln_e_b, kp(0) ? a.t[0] : a.sv[0].x, a.mean_e,
                          a.rstd_e, M, D, st, kFmlEps))
    return rc;
  if (kp(0)) {
    fml_keep_kernel<<<grid_for_threads(MD), kBlock, 0, st>>>(a.t[0], nullptr, kp(0), ks, a.sv[0].x, MD);
    HIPREC_TRY(hipGetLastError());
  }
  for (int k = 0; k < nb; ++k) {
    const FmlSaved& v = a.sv[k];
    const FmlBlock& q = w.blk[k];
    if (int rc = fml_filter_fwd(v.x, q.filt, twiddle, B, T, D, kp(1 + 2 * k), ks, v.fl, st)) return rc;
    if (int rc = seq_ln_fwd(v.x, v.fl, nullptr, nullptr, q.ln1_w, q.ln1_b, v.h, v.mean1, v.rstd1, M, D, st, kFmlEps))
      return rc;
    GemmGroup g{};
    g.n = 1;
    g.p[0] = make_gemm(kNT, Mi, H, D, v.h, D, q.f1_w, D, v.pre, H, q.f1_b, 0, nullptr, 0, false);
    if (int rc = launch_group(g, st)) return rc;
    if (int rc = fml_gelu_fwd(v.pre, a.tf[0], MH, st)) return rc;
    g = GemmGroup{};
    g.n = 1;
    g.p[0] = make_gemm(kNT, Mi, D, H, a.tf[0], H, q.f2_w, H, v.z, D, q.f2_b, 0, nullptr, 0, false);
    fml_set_keep(g.p[0], kp(2 + 2 * k), D, ks);
    if (int rc = launch_group(g, st)) return rc;
    if (int rc = seq_ln_fwd(v.h, v.z, nullptr, nullptr, q.ln2_w, q.ln2_b, k + 1 == nb ? a.out : a.sv[k + 1].x, v.mean2,
                            v.rstd2, M, D, st, kFmlEps))
      return rc;
  }
  float* f = train ? a.f : feats_out;
  fml_last_rows_kernel<<<grid_for_threads(B * D), kBlock, 0, st>>>(a.out, B, T, D, f);
  HIPREC_TRY(hipGetLastError());
  if (!train) return 0;
  if (feats_out) HIPREC_TRY(hipMemcpyAsync(feats_out, f, sizeof(float) * B * D, hipMemcpyDeviceToDevice, st));

  // ---- loss on the B last-position rows ----
  const FmlParams g = fml_params(g_flat, s);
  float *S1 = a.t[0], *S1k = a.t[1], *S2 = a.t[2], *S3 = a.t[3], *S3k = a.t[4], *X1 = a.t[5], *U1 = a.t[6], *U2 = a.t[7];
  fml_count_kernel<<<1, kBlock, 0, st>>>(pos, B, a.aux);
  HIPREC_TRY(hipGetLastError());
  if (int rc = seq_loss(f, w.item_emb, pos, neg, B, D, s.n_items, a.aux, 0.f, a.df, g.item_emb, scratch, stats, st))
    return rc;
  fml_spread_last_kernel<<<grid_for_threads(MD), kBlock, 0, st>>>(a.df, M, T, D, S3);
  HIPREC_TRY(hipGetLastError());

  // ---- the blocks in reverse: (dA, dB) = the two summands of the gradient of a block's output ----
  const float *dA = S3, *dB = nullptr;
  for (int k = nb - 1; k >= 0; --k) {
    const FmlSaved& v = a.sv[k];
    const FmlBlock &q = w.blk[k], &gq = g.blk[k];
    // LN_2: S1 = gradient of h + z, S1k = the same through the feed-forward dropout
    if (int rc = seq_ln_bwd(dA, dB, v.h, v.z, q.ln2_w, v.mean2, v.rstd2, nullptr, nullptr, nullptr, kp(2 + 2 * k), ks, S1,
                            S1k, U1, U2, gq.ln2_w, gq.ln2_b, a.cs, M, D, st))
      return rc;
    const float* dz = kp(2 + 2 * k) ? S1k : S1;
    if (int rc = fml_gelu_fwd(v.pre, a.tf[0], MH, st)) return rc;
    {
      GemmGroup p{};
      p.p[p.n++] = make_gemm(kNN, Mi, H, D, dz, D, q.f2_w, H, a.tf[1], H, nullptr, 0, nullptr, 0, false);
      const int slabs = fml_add_wgrad(p, D, H, Mi, dz, D, a.tf[0], H, gq.f2_w, a.part);
      p.p[p.n++] = make_colsum(dz, Mi, D, D, gq.f2_b, a.cs);
      if (int rc = launch_group(p, st)) return rc;
      if (int rc = launch_colsum_reduce(p, st)) return rc;
      if (int rc = fml_fold(gq.f2_w, a.part, static_cast<int64_t>(D) * H, slabs, st)) return rc;
    }
    fml_gelu_bwd_kernel<<<grid_for_threads(MH), kBlock, 0, st>>>(a.tf[1], v.pre, MH);
    HIPREC_TRY(hipGetLastError());
    {
      GemmGroup p{};
      p.p[p.n++] = make_gemm(kNN, Mi, D, H, a.tf[1], H, q.f1_w, D, S2, D, nullptr, 0, nullptr, 0, false);
      const int slabs = fml_add_wgrad(p, H, D, Mi, a.tf[1], H, v.h, D, gq.f1_w, a.part);
      p.p[p.n++] = make_colsum(a.tf[1], Mi, H, H, gq.f1_b, a.cs);
      if (int rc = launch_group(p, st)) return rc;
      if (int rc = launch_colsum_reduce(p, st)) return rc;
      if (int rc = fml_fold(gq.f1_w, a.part, static_cast<int64_t>(D) * H, slabs, st)) return rc;
    }
    // LN_1: dy = d(fc1 input) + the residual's gradient; S3 = gradient of x + fl, S3k = the same through the filter dropout
    if (int rc = seq_ln_bwd(S2, S1, v.x, v.fl, q.ln1_w, v.mean1, v.rstd1, nullptr, nullptr, nullptr, kp(1 + 2 * k), ks, S3,
                            S3k, U1, U2, gq.ln1_w, gq.ln1_b, a.cs, M, D, st))
      return rc;
    if (int rc = fml_filter_bwd(v.x, kp(1 + 2 * k) ? S3k : S3, q.filt, twiddle, B, T, D, X1, gq.filt, a.fpart, st))
      return rc;
    dA = S3;        // the residual's share of d x[k] ...
    dB = X1;        // ... and the filter's
  }
  // embedding: dropout, LN_e, the two tables
  if (kp(0)) {
    fml_keep_kernel<<<grid_for_threads(MD), kBlock, 0, st>>>(dA, dB, kp(0), ks, S2, MD);
    HIPREC_TRY(hipGetLastError());
    dA = S2;
    dB = nullptr;
  }
  if (int rc = seq_ln_bwd(dA, dB, a.raw, nullptr, w.ln_e_w, a.mean_e, a.rstd_e, nullptr, nullptr, nullptr, nullptr, ks, S1,
                          nullptr, U1, U2, g.ln_e_w, g.ln_e_b, a.cs, M, D, st))
    return rc;
  fml_embed_bwd_kernel<<<(T * D + kBlock - 1) / kBlock, kBlock, 0, st>>>(S1, seq, B, T, D, s.n_items, g.item_emb,
                                                                         g.pos_emb);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

int fml_check_call(const hiprec_fmlprec_shape* shape, const void* w_flat, const void* seq, int64_t batch,
                   const void* twiddle, const void* stats, const void* workspace, size_t workspace_bytes) {
  if (int rc = fml_check_shape(shape)) return rc;
  HIPREC_REQUIRE(w_flat && seq && twiddle && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(fml_batch_ok(*shape, batch), "FMLP-Rec: batch %lld must be >= 1 and batch x maxlen %d at most 2^24",
                 static_cast<long long>(batch), shape->maxlen);
  const size_t need = hiprec_fmlprec_workspace_bytes(shape, batch);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  return 0;
}

bool fml_filter_shape_ok(int64_t batch, int seq_len, int dim) {
  return dim >= 16 && dim <= kSeqMaxDim && dim % 16 == 0 && seq_len >= 1 && seq_len <= kSeqMaxLen && batch >= 1 &&
         batch * seq_len <= (1ll << 24);
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_fmlprec_shape_bytes(void) { return sizeof(hiprec_fmlprec_shape); }

extern "C" int64_t hiprec_fmlprec_param_floats(const hiprec_fmlprec_shape* shape) {
  if (fml_check_shape(shape)) return -1;
  return fml_n_params(*shape);
}

extern "C" size_t hiprec_fmlprec_workspace_bytes(const hiprec_fmlprec_shape* shape, int64_t batch) {
  if (fml_check_shape(shape) || !fml_batch_ok(*shape, batch)) return 0;
  return sizeof(float) * static_cast<size_t>(fml_carve(nullptr, *shape, batch).floats);
}

extern "C" int hiprec_fmlprec_twiddle(int32_t seq_len, float* out) {
  HIPREC_REQUIRE(out && seq_len >= 1 && seq_len <= kSeqMaxLen, "twiddle table: 1 <= seq_len <= %d and a buffer", kSeqMaxLen);
  const double two_pi = 6.283185307179586476925286766559;
  for (int j = 0; j < seq_len; ++j) {
    double c = std::cos(two_pi * j / seq_len), sn = std::sin(two_pi * j / seq_len);
    if (j == 0 || 2 * j == seq_len) sn = 0.0;                     // the axes are exact: the imaginary part of the DC and
    if (4 * j == seq_len || 4 * j == 3 * seq_len) c = 0.0;        // Nyquist bins is 0, not the rounding of sin(pi)
    out[2 * j] = static_cast<float>(c);
    out[2 * j + 1] = static_cast<float>(sn);
  }
  return 0;
}

extern "C" int hiprec_fmlprec_grad(const hiprec_fmlprec_shape* shape, const float* w_flat, float* g_flat,
                                   const int64_t* seq, const int64_t* pos, const int64_t* neg, int64_t batch,
                                   const float* twiddle, const uint8_t* const* keep, float keep_scale, float* feats_out,
                                   hiprec_stats* stats, void* scratch, size_t scratch_bytes, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (int rc = fml_check_call(shape, w_flat, seq, batch, twiddle, stats, workspace, workspace_bytes)) return rc;
  HIPREC_REQUIRE(g_flat && pos && neg && scratch, "training needs the gradient buffer, pos, neg and the scratch block");
  if (scratch_bytes < kScratchBytes) {
    set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
    return HIPREC_E_SCRATCH;
  }
  return fml_run(*shape, const_cast<float*>(w_flat), g_flat, seq, pos, neg, batch, twiddle, keep, keep_scale, feats_out,
                 stats, static_cast<Scratch*>(scratch), static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_fmlprec_feats(const hiprec_fmlprec_shape* shape, const float* w_flat, const int64_t* seq,
                                    int64_t batch, const float* twiddle, float* feats_out, hiprec_stats* stats,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = fml_check_call(shape, w_flat, seq, batch, twiddle, stats, workspace, workspace_bytes)) return rc;
  HIPREC_REQUIRE(feats_out, "the eval forward needs the feats buffer");
  return fml_run(*shape, const_cast<float*>(w_flat), nullptr, seq, nullptr, nullptr, batch, twiddle, nullptr, 1.0f,
                 feats_out, stats, nullptr, static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int64_t hiprec_fmlprec_filter_scratch_floats(int64_t batch, int32_t seq_len, int32_t dim) {
  if (!fml_filter_shape_ok(batch, seq_len, dim)) return -1;
  return static_cast<int64_t>(fml_parts(batch)) * 2 * fml_bins(seq_len) * dim;
}

extern "C" int hiprec_fmlprec_filter(const float* x, const float* weight, const float* twiddle, const uint8_t* keep,
                                     float keep_scale, const float* dy, int64_t batch, int32_t seq_len, int32_t dim,
                                     float* y, float* dx, float* dw, float* scratch, size_t scratch_floats, void* stream) {
  HIPREC_REQUIRE(x && weight && twiddle && (y || dy), "NULL pointer");
  HIPREC_REQUIRE(fml_filter_shape_ok(batch, seq_len, dim), "FMLP-Rec filter: shape outside the model's limits");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (y)
    if (int rc = fml_filter_fwd(x, weight, twiddle, batch, seq_len, dim, keep, keep_scale, y, st)) return rc;
  if (!dy) return 0;
  HIPREC_REQUIRE(dx && dw && scratch, "the filter backward needs dx, dw and the scratch buffer");
  const int64_t need = hiprec_fmlprec_filter_scratch_floats(batch, seq_len, dim);
  HIPREC_REQUIRE(scratch_floats >= static_cast<size_t>(need), "filter scratch %zu floats < %lld", scratch_floats,
                 static_cast<long long>(need));
  return fml_filter_bwd(x, dy, weight, twiddle, batch, seq_len, dim, dx, dw, scratch, st);
}
