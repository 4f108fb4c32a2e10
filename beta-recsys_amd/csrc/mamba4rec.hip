// Mamba4Rec (Liu et al., 2024; no counterpart in the reference, the definition is include/hiprec.h's): zero_grad + forward +
// loss + backward of one training step as a fixed sequence of launches, no host sync.
// Activations are [M = B * T, .] row-major, row m = b * T + t, T = maxlen, sequences left-padded; start[b] is the first slot
// with seq != 0 (T for an empty row).  D = dim, Di = expand * D, N = d_state, R = dt_rank, Kc = d_conv.
//
//   embed               raw = drop(E[seq]) (seq_embed without a positional table) -> LN_e (eps 1e-12)
//   per layer           xm = x masked; [xi | z] = xm in_proj^T (GEMM); u = silu(conv(xi) + bias) (mb_conv_fwd_kernel);
//                       [dt | Bm | Cm] = u x_proj^T (GEMM, odd widths: the grouped GEMM checks every element's bounds, no
//                       padding needed); dtp = dt dt_proj^T + bias (GEMM); yg = scan(...) * silu(z); mo = drop(yg out_proj^T)
//                       (GEMM epilogue); h = LN_1(mo + x) (nb == 1: LN_1(mo)); the GELU feed-forward; x' = LN_2(h + z2).
//   selective scan      time in lanes.  A workgroup is 4 waves on ONE sequence and kMbSlab = 16 channels, a wave owns
//                       kMbCW = 4 of them at once: lane l holds the K = ceil(T / 64) consecutive positions l K .. l K + K - 1
//                       of each (delta, u, y as [4][K] registers, loaded as one float4 per position).  Bm and Cm of the
//                       sequence are staged through LDS in chunks of kMbNC = 16 states as [n][i * 64 + l] with a row pitch
//                       of 257 floats: lanes read consecutive words, the staging threads (consecutive n) hit different
//                       banks.  Per (channel, state): the lane composes its K steps into (a, b), the wave runs the
//                       inclusive scan of (a1, b1) o (a2, b2) = (a1 a2, a2 b1 + b2) by __shfl_up in 6 rounds, the lane
//                       replays its steps from the carry and adds Cm_t[n] h_t into its y registers: the sum over n never
//                       crosses lanes.  softplus, + D u, * silu(z) and the padding mask are prologue and epilogue.
//   scan backward       the same ownership, states outermost and the wave's 4 channels inside: h is recomputed, h_{t-1}
//                       is the replay's previous value, g_t = Cm_t dy_t + a_{t+1} g_{t+1} is the mirrored scan by
//                       __shfl_down.  d delta, du, y stay in [4][K] registers, dBm / dCm of the state in 2 K registers,
//                       folded across the 4 waves through LDS in wave order (one barrier per state, two buffers) into the
//                       slab's partial [slab][b][2 N][T]; mb_bc_fold_kernel adds the slabs in order.  dA and dD are one
//                       wave reduction each into the wave's LDS slots; workgroup (p, slab) walks the sequences p, p + P, ...
//                       (P = min(B, 128)) and leaves one partial, mb_fold_kernel adds the P partials in order
//                       (d A_log = dA * A).  Nothing of shape [B, T, Di, N] exists.
//   conv backward       mb_conv_bwd_kernel: workgroup (slab of 16 channels, p) walks its sequences; xi and d pre sit in LDS,
//                       d weight / d bias in registers, folded over the 16 time groups and then over the P partials in order.
//   backward            the chain in reverse; every weight gradient is a kTNm problem of the grouped GEMM in up to 8 batch
//                       slabs folded in slab order; bias gradients are two-level column sums.
//
// No float atomics in this file: every gradient except item_emb.weight (seq_loss, seq_embed_bwd) is the same bits on every run.
#include <algorithm>
#include <cmath>

#include "gemm.hpp"
#include "seqrec.hpp"

namespace hiprec {
namespace {

constexpr int kMbCW = 4;                              // channels a wave owns at once
constexpr int kMbSlab = kMbCW * kWavesPerBlock;       // channels of a scan workgroup
constexpr int kMbNC = 16;                             // states staged per chunk
constexpr int kMbPitch = kSeqMaxLen + 1;              // row pitch of a staged state
constexpr int kMbParts = 128;                         // workgroups per slab of the scan / conv backward
constexpr int kMbConvSlab = 16;
constexpr int kMbMaxState = 64, kMbMaxRank = 32, kMbMaxConv = 4, kMbMaxBlocks = 16, kMbMaxFfn = 512;
constexpr int kMbSlabs = 8;                           // batch slabs of a weight-gradient GEMM
constexpr float kMbEps = 1e-12f;
constexpr float kMbLog2e = 1.44269504088896340736f;

__device__ __forceinline__ float mb_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float mb_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }   // F.softplus's threshold

// ---- the selective scan ------------------------------------------------------------------------------------------------
// K positions x 4 channels of one lane: p at (first row of the sequence, first channel of the wave); 0 outside [lo, T)
template <int K>
__device__ __forceinline__ void mb_load(const float* __restrict__ p, int64_t ld, int t0, int lo, int T,
                                        float (&v)[kMbCW][K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int t = t0 + i;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t >= lo && t < T) q = *reinterpret_cast<const float4*>(p + static_cast<int64_t>(t) * ld);
    v[0][i] = q.x; v[1][i] = q.y; v[2][i] = q.z; v[3][i] = q.w;
  }
}

template <int K>
__device__ __forceinline__ void mb_store(float* __restrict__ p, int64_t ld, int t0, int T, const float (&v)[kMbCW][K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int t = t0 + i;
    if (t < T) *reinterpret_cast<float4*>(p + static_cast<int64_t>(t) * ld) = make_float4(v[0][i], v[1][i], v[2][i], v[3][i]);
  }
}

// states [n0, n0 + nc) of one sequence's Bm and Cm (at its first row, leading dimension ld) into sB / sC [j][i * 64 + l]
template <int K>
__device__ __forceinline__ void mb_stage(float* sB, float* sC, const float* __restrict__ Bm, const float* __restrict__ Cm,
                                         int64_t ld, int T, int n0, int nc) {
  for (int e = threadIdx.x; e < T * nc; e += kBlock) {
    const int t = e / nc, j = e - t * nc;
    const int at = j * kMbPitch + (t % K) * kWave + t / K;
    sB[at] = Bm[static_cast<int64_t>(t) * ld + n0 + j];
    sC[at] = Cm[static_cast<int64_t>(t) * ld + n0 + j];
  }
}

// h of the lane's K positions for one (channel, state) from the steps (a, b): in-lane composition, inclusive wave scan,
// replay from the carry.  hp receives h_{t-1}.
template <int K>
__device__ __forceinline__ void mb_scan_steps(const float (&a)[K], const float (&b)[K], int lane, float (&h)[K],
                                              float (&hp)[K]) {
  float ca = 1.f, cb = 0.f;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    cb = a[i] * cb + b[i];
    ca = ca * a[i];
  }
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const float pa = __shfl_up(ca, off, kWave), pb = __shfl_up(cb, off, kWave);
    if (lane >= off) {
      cb = ca * pb + cb;
      ca = pa * ca;
    }
  }
  float carry = __shfl_up(cb, 1, kWave);
  if (lane == 0) carry = 0.f;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    hp[i] = carry;
    carry = a[i] * carry + b[i];
    h[i] = carry;
  }
}

// out = (scan + D u) * silu(z), 0 at padded slots.  grid (B, Di / 16).  u, dtp, out [M, Di]; z with ldz; Bm, Cm with ldbc.
template <int K>
__global__ __launch_bounds__(kBlock) void mb_scan_fwd_kernel(const float* __restrict__ u, const float* __restrict__ dtp,
                                                             const float* __restrict__ z, int ldz,
                                                             const float* __restrict__ A, const float* __restrict__ Bm,
                                                             const float* __restrict__ Cm, int ldbc,
                                                             const float* __restrict__ Dp, const int32_t* __restrict__ start,
                                                             int T, int Di, int N, float* __restrict__ out) {
  __shared__ float sB[kMbNC * kMbPitch];
  __shared__ float sC[kMbNC * kMbPitch];
  const int lane = lane_id(), wave = wave_in_block(), t0 = lane * K;
  const int d0 = blockIdx.y * kMbSlab + wave * kMbCW;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * T;
  const int lo = start[blockIdx.x];
  float delta[kMbCW][K], uu[kMbCW][K], y[kMbCW][K];
  mb_load<K>(dtp + row0 * Di + d0, Di, t0, lo, T, delta);
  mb_load<K>(u + row0 * Di + d0, Di, t0, lo, T, uu);
  bool valid[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    valid[i] = t0 + i >= lo && t0 + i < T;
#pragma unroll
    for (int c = 0; c < kMbCW; ++c) {
      delta[c][i] = mb_softplus(delta[c][i]);
      y[c][i] = 0.f;
    }
  }
  for (int n0 = 0; n0 < N; n0 += kMbNC) {
    const int nc = min(kMbNC, N - n0);
    if (n0) lds_barrier();       // the chunk before has been read
    mb_stage<K>(sB, sC, Bm + row0 * ldbc, Cm + row0 * ldbc, ldbc, T, n0, nc);
    lds_barrier();
    for (int j = 0; j < nc; ++j) {
      float Bv[K], Cv[K];
#pragma unroll
      for (int i = 0; i < K; ++i) {
        Bv[i] = valid[i] ? sB[j * kMbPitch + i * kWave + lane] : 0.f;
        Cv[i] = valid[i] ? sC[j * kMbPitch + i * kWave + lane] : 0.f;
      }
#pragma unroll
      for (int c = 0; c < kMbCW; ++c) {
        const float A2 = A[static_cast<int64_t>(d0 + c) * N + n0 + j] * kMbLog2e;
        float a[K], b[K], h[K], hp[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
          a[i] = valid[i] ? exp2f(delta[c][i] * A2) : 1.f;
          b[i] = delta[c][i] * Bv[i] * uu[c][i];
        }
        mb_scan_steps<K>(a, b, lane, h, hp);
#pragma unroll
        for (int i = 0; i < K; ++i) y[c][i] += Cv[i] * h[i];
      }
    }
  }
  float zz[kMbCW][K];
  mb_load<K>(z + row0 * ldz + d0, ldz, t0, lo, T, zz);
#pragma unroll
  for (int c = 0; c < kMbCW; ++c) {
    const float dv = Dp[d0 + c];
#pragma unroll
    for (int i = 0; i < K; ++i)
      y[c][i] = valid[i] ? (y[c][i] + dv * uu[c][i]) * (zz[c][i] * mb_sigmoid(zz[c][i])) : 0.f;
  }
  mb_store<K>(out + row0 * Di + d0, Di, t0, T, y);
}

// grid (P, Di / 16).  du, ddtp [M, Di]; dz with lddz; partBC [Di / 16][B][2 N][T]; partA [P][Di * N]; partD [P][Di].
template <int K>
__global__ __launch_bounds__(kBlock) void mb_scan_bwd_kernel(
    const float* __restrict__ u, const float* __restrict__ dtp, const float* __restrict__ z, int ldz,
    const float* __restrict__ A, const float* __restrict__ Bm, const float* __restrict__ Cm, int ldbc,
    const float* __restrict__ Dp, const int32_t* __restrict__ start, const float* __restrict__ dout, int64_t B, int T,
    int Di, int N, float* __restrict__ du, float* __restrict__ ddtp, float* __restrict__ dz, int lddz,
    float* __restrict__ partBC, float* __restrict__ partA, float* __restrict__ partD) {
  __shared__ float sB[kMbNC * kMbPitch];
  __shared__ float sC[kMbNC * kMbPitch];
  __shared__ float xw[2][kWavesPerBlock][2][kSeqMaxLen];
  __shared__ float sA[kWavesPerBlock][kMbCW][kMbMaxState];
  __shared__ float sD[kWavesPerBlock][kMbCW];
  const int lane = lane_id(), wave = wave_in_block(), t0 = lane * K;
  const int d0 = blockIdx.y * kMbSlab + wave * kMbCW;
#pragma unroll
  for (int c = 0; c < kMbCW; ++c) {
    sA[wave][c][lane] = 0.f;          // only this wave touches its slots
    if (lane == 0) sD[wave][c] = 0.f;
  }
  int par = 0;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t row0 = b * T;
    const int lo = start[b];
    float delta[kMbCW][K], uu[kMbCW][K], dy[kMbCW][K], y[kMbCW][K], dl[kMbCW][K], dus[kMbCW][K];
    mb_load<K>(dtp + row0 * Di + d0, Di, t0, lo, T, delta);
    mb_load<K>(u + row0 * Di + d0, Di, t0, lo, T, uu);
    mb_load<K>(dout + row0 * Di + d0, Di, t0, lo, T, dy);
    mb_load<K>(z + row0 * ldz + d0, ldz, t0, lo, T, y);
    bool valid[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
      valid[i] = t0 + i >= lo && t0 + i < T;
#pragma unroll
      for (int c = 0; c < kMbCW; ++c) {
        delta[c][i] = mb_softplus(delta[c][i]);
        dy[c][i] = dy[c][i] * (y[c][i] * mb_sigmoid(y[c][i]));      // 0 outside [lo, T): dout was loaded as 0
        y[c][i] = 0.f;
        dl[c][i] = 0.f;
        dus[c][i] = 0.f;
      }
    }
    float* pbc = partBC + (static_cast<int64_t>(blockIdx.y) * B + b) * 2 * N * T;
    for (int n0 = 0; n0 < N; n0 += kMbNC) {
      const int nc = min(kMbNC, N - n0);
      // no barrier in front: every wave passed the barrier of the state before, after its last read of sB / sC
      mb_stage<K>(sB, sC, Bm + row0 * ldbc, Cm + row0 * ldbc, ldbc, T, n0, nc);
      lds_barrier();
      for (int j = 0; j < nc; ++j) {
        float Bv[K], Cv[K], dB[K], dC[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
          Bv[i] = valid[i] ? sB[j * kMbPitch + i * kWave + lane] : 0.f;
          Cv[i] = valid[i] ? sC[j * kMbPitch + i * kWave + lane] : 0.f;
          dB[i] = 0.f;
          dC[i] = 0.f;
        }
#pragma unroll
        for (int c = 0; c < kMbCW; ++c) {
          const float An = A[static_cast<int64_t>(d0 + c) * N + n0 + j], A2 = An * kMbLog2e;
          float a[K], bb[K], h[K], hp[K], g[K];
#pragma unroll
          for (int i = 0; i < K; ++i) {
            a[i] = valid[i] ? exp2f(delta[c][i] * A2) : 1.f;
            bb[i] = delta[c][i] * Bv[i] * uu[c][i];
          }
          mb_scan_steps<K>(a, bb, lane, h, hp);
          // g_t = Cm_t dy_t + a_{t+1} g_{t+1}: the mirrored scan
          float an = __shfl_down(a[0], 1, kWave);
          if (lane == kWave - 1) an = 1.f;
          float al[K];
#pragma unroll
          for (int i = 0; i < K; ++i) al[i] = i + 1 < K ? a[i + 1 < K ? i + 1 : i] : an;
          float ca = 1.f, cb = 0.f;
#pragma unroll
          for (int i = K - 1; i >= 0; --i) {
            cb = Cv[i] * dy[c][i] + al[i] * cb;
            ca = al[i] * ca;
          }
#pragma unroll
          for (int off = 1; off < kWave; off <<= 1) {
            const float pa = __shfl_down(ca, off, kWave), pb = __shfl_down(cb, off, kWave);
            if (lane + off < kWave) {
              cb = cb + ca * pb;
              ca = ca * pa;
            }
          }
          float gin = __shfl_down(cb, 1, kWave);
          if (lane == kWave - 1) gin = 0.f;
#pragma unroll
          for (int i = K - 1; i >= 0; --i) {
            gin = Cv[i] * dy[c][i] + al[i] * gin;
            g[i] = valid[i] ? gin : 0.f;
          }
          float da = 0.f;
#pragma unroll
          for (int i = 0; i < K; ++i) {
            const float gah = g[i] * a[i] * hp[i];
            y[c][i] += Cv[i] * h[i];
            dl[c][i] += g[i] * Bv[i] * uu[c][i] + An * gah;
            dus[c][i] += g[i] * delta[c][i] * Bv[i];
            dB[i] += g[i] * delta[c][i] * uu[c][i];
            dC[i] += dy[c][i] * h[i];
            da += delta[c][i] * gah;
          }
          da = wave_sum(da);
          if (lane == 0) sA[wave][c][n0 + j] += da;
        }
#pragma unroll
        for (int i = 0; i < K; ++i)
          if (t0 + i < T) {
            xw[par][wave][0][t0 + i] = dB[i];
            xw[par][wave][1][t0 + i] = dC[i];
          }
        lds_barrier();
        if (static_cast<int>(threadIdx.x) < T) {
          const int t = threadIdx.x;
          const float sb = ((xw[par][0][0][t] + xw[par][1][0][t]) + xw[par][2][0][t]) + xw[par][3][0][t];
          const float sc = ((xw[par][0][1][t] + xw[par][1][1][t]) + xw[par][2][1][t]) + xw[par][3][1][t];
          pbc[static_cast<int64_t>(n0 + j) * T + t] = sb;
          pbc[static_cast<int64_t>(N + n0 + j) * T + t] = sc;
        }
        par ^= 1;
      }
    }
    // epilogue: + D u, dz, the softplus derivative
    float zz[kMbCW][K], go[kMbCW][K];
    mb_load<K>(z + row0 * ldz + d0, ldz, t0, lo, T, zz);
    mb_load<K>(dout + row0 * Di + d0, Di, t0, lo, T, go);
#pragma unroll
    for (int c = 0; c < kMbCW; ++c) {
      const float dv = Dp[d0 + c];
      float dd = 0.f;
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const float s = mb_sigmoid(zz[c][i]);
        dd += dy[c][i] * uu[c][i];
        dus[c][i] += dv * dy[c][i];
        zz[c][i] = go[c][i] * (y[c][i] + dv * uu[c][i]) * (s * (1.f + zz[c][i] * (1.f - s)));    // dz; 0 outside [lo, T)
      }
      dd = wave_sum(dd);
      if (lane == 0) sD[wave][c] += dd;
    }
    mb_load<K>(dtp + row0 * Di + d0, Di, t0, lo, T, go);
#pragma unroll
    for (int c = 0; c < kMbCW; ++c)
#pragma unroll
      for (int i = 0; i < K; ++i) dl[c][i] = valid[i] ? dl[c][i] * (go[c][i] > 20.f ? 1.f : mb_sigmoid(go[c][i])) : 0.f;
    mb_store<K>(du + row0 * Di + d0, Di, t0, T, dus);
    mb_store<K>(ddtp + row0 * Di + d0, Di, t0, T, dl);
    mb_store<K>(dz + row0 * lddz + d0, lddz, t0, T, zz);
  }
#pragma unroll
  for (int c = 0; c < kMbCW; ++c) {
    if (lane < N) partA[(static_cast<int64_t>(blockIdx.x) * Di + d0 + c) * N + lane] = sA[wave][c][lane];
    if (lane == 0) partD[static_cast<int64_t>(blockIdx.x) * Di + d0 + c] = sD[wave][c];
  }
}

// dBm / dCm [b, t, n] (leading dimension ld) = the channel slabs' partials [slab][b][2 N][T], added in slab order
__global__ __launch_bounds__(kBlock) void mb_bc_fold_kernel(const float* __restrict__ part, int slabs, int64_t B, int T, int N,
                                                            float* __restrict__ dB, float* __restrict__ dC, int ld) {
  const int64_t n = B * 2 * N * T, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
    const int t = static_cast<int>(e % T);
    const int n2 = static_cast<int>((e / T) % (2 * N));
    const int64_t b = e / (static_cast<int64_t>(T) * 2 * N);
    float s = part[e];
    for (int k = 1; k < slabs; ++k) s += part[k * n + e];
    float* dst = n2 < N ? dB + n2 : dC + (n2 - N);
    dst[(b * T + t) * ld] = s;
  }
}

// ---- conv + SiLU ---------------------------------------------------------------------------------------------------------
// pre[t] = bias + sum_s w[Kc - 1 - s] xi[t - s] over t - s >= start (zeros before: never the neighbouring sequence's row)
__global__ __launch_bounds__(kBlock) void mb_conv_fwd_kernel(const float* __restrict__ xi, int ldx,
                                                             const float* __restrict__ w, const float* __restrict__ bias,
                                                             const int32_t* __restrict__ start, int64_t M, int T, int Di,
                                                             int Kc, float* __restrict__ u) {
  const int64_t n = M * Di, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t m = i / Di, b = m / T;
    const int d = static_cast<int>(i - m * Di), t = static_cast<int>(m - b * T), lo = start[b];
    float acc = bias[d];
    for (int s = 0; s < Kc; ++s)
      if (t - s >= lo) acc += w[d * Kc + Kc - 1 - s] * xi[(m - s) * ldx + d];
    u[i] = acc * mb_sigmoid(acc);
  }
}

// dxi and this workgroup's share of d weight / d bias from du = du_a + du_b.  grid (Di / 16, P); partW [P][Di * Kc],
// partB [P][Di].  Thread (c = tid & 15, tg = tid >> 4) owns channel c at the positions tg, tg + 16, ...
__global__ __launch_bounds__(kBlock) void mb_conv_bwd_kernel(const float* __restrict__ xi, int ldx,
                                                             const float* __restrict__ w, const float* __restrict__ bias,
                                                             const int32_t* __restrict__ start,
                                                             const float* __restrict__ du_a, const float* __restrict__ du_b,
                                                             int64_t B, int T, int Di, int Kc, float* __restrict__ dxi,
                                                             int lddx, float* __restrict__ partW, float* __restrict__ partB) {
  __shared__ float xs[kSeqMaxLen][kMbConvSlab];
  __shared__ float ds[kSeqMaxLen][kMbConvSlab];
  __shared__ float red[kBlock / kMbConvSlab][kMbConvSlab][kMbMaxConv + 1];
  const int c = threadIdx.x & (kMbConvSlab - 1), tg = threadIdx.x / kMbConvSlab, d = blockIdx.x * kMbConvSlab + c;
  constexpr int kGroups = kBlock / kMbConvSlab;
  float wv[kMbMaxConv], gw[kMbMaxConv], gb = 0.f;      // wv[s] multiplies xi[t - s]
#pragma unroll
  for (int s = 0; s < kMbMaxConv; ++s) {
    wv[s] = s < Kc ? w[d * Kc + Kc - 1 - s] : 0.f;
    gw[s] = 0.f;
  }
  const float bv = bias[d];
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    const int64_t row0 = b * T;
    const int lo = start[b];
    lds_barrier();       // the sequence before is through with xs and ds
    for (int t = tg; t < T; t += kGroups) xs[t][c] = t >= lo ? xi[(row0 + t) * ldx + d] : 0.f;
    lds_barrier();
    for (int t = tg; t < T; t += kGroups) {
      float pre = bv;
#pragma unroll
      for (int s = 0; s < kMbMaxConv; ++s)
        if (s < Kc && t - s >= 0) pre += wv[s] * xs[t - s][c];
      const float sg = mb_sigmoid(pre);
      float g = du_a[(row0 + t) * Di + d];
      if (du_b) g += du_b[(row0 + t) * Di + d];
      g *= sg * (1.f + pre * (1.f - sg));
      ds[t][c] = g;
      gb += g;
#pragma unroll
      for (int s = 0; s < kMbMaxConv; ++s)
        if (s < Kc && t - s >= 0) gw[s] += g * xs[t - s][c];
    }
    lds_barrier();
    for (int t = tg; t < T; t += kGroups) {
      float v = 0.f;
#pragma unroll
      for (int s = 0; s < kMbMaxConv; ++s)
        if (s < Kc && t + s < T) v += wv[s] * ds[t + s][c];
      dxi[(row0 + t) * lddx + d] = t >= lo ? v : 0.f;
    }
  }
#pragma unroll
  for (int s = 0; s < kMbMaxConv; ++s) red[tg][c][s] = gw[s];
  red[tg][c][kMbMaxConv] = gb;
  lds_barrier();
  if (tg <= Kc) {       // thread (c, s = tg) adds the 16 time groups in order; s == Kc is the bias
    const int s = tg == Kc ? kMbMaxConv : tg;
    float v = red[0][c][s];
    for (int k = 1; k < kGroups; ++k) v += red[k][c][s];
    if (tg == Kc) partB[static_cast<int64_t>(blockIdx.y) * Di + d] = v;
    else partW[(static_cast<int64_t>(blockIdx.y) * Di + d) * Kc + Kc - 1 - s] = v;
  }
}

// ---- elementwise ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float mb_gelu(float z) { return 0.5f * z * (1.0f + erff(z * 0.70710678118654752440f)); }

__device__ __forceinline__ float mb_gelu_grad(float z) {
  return 0.5f * (1.0f + erff(z * 0.70710678118654752440f)) + z * 0.39894228040143267794f * expf(-0.5f * z * z);
}

// act = keep(gelu(pre)); keep may be NULL
__global__ __launch_bounds__(kBlock) void mb_gelu_fwd_kernel(const float* __restrict__ pre, const uint8_t* __restrict__ keep,
                                                             float ks, float* __restrict__ act, int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const float v = mb_gelu(pre[i]);
    act[i] = keep ? (keep[i] ? v * ks : 0.f) : v;
  }
}

// d pre = d act * gelu'(pre), in place on d
__global__ __launch_bounds__(kBlock) void mb_gelu_bwd_kernel(float* d, const float* __restrict__ pre, int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride)
    d[i] = d[i] * mb_gelu_grad(pre[i]);
}

// start[b] = the first slot with seq != 0, T for a row of padding
__global__ __launch_bounds__(kBlock) void mb_start_kernel(const int64_t* __restrict__ seq, int64_t B, int T,
                                                          int32_t* __restrict__ start) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; b < B; b += stride) {
    int t = 0;
    while (t < T && seq[b * T + t] == 0) ++t;
    start[b] = t;
  }
}

// out = x at the slots from start on, 0 at padding
__global__ __launch_bounds__(kBlock) void mb_mask_kernel(const float* __restrict__ x, const int32_t* __restrict__ start,
                                                         int64_t M, int T, int D, float* __restrict__ out) {
  const int64_t n = M * D, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t m = i / D, b = m / T;
    out[i] = static_cast<int>(m - b * T) >= start[b] ? x[i] : 0.f;
  }
}

// A = -exp(A_log)
__global__ __launch_bounds__(kBlock) void mb_neg_exp_kernel(const float* __restrict__ a_log, float* __restrict__ A, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) A[i] = -expf(a_log[i]);
}

// out[i] = the partials of i added in order, times mul[i] (mul may be NULL)
__global__ __launch_bounds__(kBlock) void mb_fold_kernel(float* __restrict__ out, const float* __restrict__ part,
                                                         const float* __restrict__ mul, int64_t n, int parts) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    float s = part[i];
    for (int k = 1; k < parts; ++k) s += part[k * n + i];
    out[i] = mul ? s * mul[i] : s;
  }
}

// f[b] = x[b, T - 1]
__global__ __launch_bounds__(kBlock) void mb_last_rows_kernel(const float* __restrict__ x, int64_t B, int T, int D,
                                                              float* __restrict__ f) {
  const int64_t n = B * D, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t b = i / D;
    f[i] = x[(b * T + T - 1) * D + (i - b * D)];
  }
}

// dx[b, T - 1] = df[b], every other row 0
__global__ __launch_bounds__(kBlock) void mb_spread_last_kernel(const float* __restrict__ df, int64_t M, int T, int D,
                                                                float* __restrict__ dx) {
  const int64_t n = M * D, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t m = i / D;
    dx[i] = (m % T == T - 1) ? df[(m / T) * D + (i - m * D)] : 0.f;
  }
}

// aux[0] = max(1, count(pos != 0)) (one block; integers up to 2^24 are exact in fp32), aux[1] = 0: what seq_loss divides by
__global__ __launch_bounds__(kBlock) void mb_count_kernel(const int64_t* __restrict__ pos, int64_t B, float* __restrict__ aux) {
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

// ---- host side: the scan and conv stages -------------------------------------------------------------------------------
int mb_parts(int64_t B) { return static_cast<int>(std::min<int64_t>(B, kMbParts)); }

int64_t mb_scan_scratch(int64_t B, int T, int Di, int N) {
  return static_cast<int64_t>(Di / kMbSlab) * B * 2 * N * T + static_cast<int64_t>(mb_parts(B)) * Di * (N + 1);
}

bool mb_scan_shape_ok(int64_t B, int T, int Di, int N) {
  return B >= 1 && T >= 1 && T <= kSeqMaxLen && B * T <= (1ll << 24) && Di >= 16 && Di <= 2 * kSeqMaxDim && Di % 16 == 0 &&
         N >= 1 && N <= kMbMaxState;
}

int mb_scan_fwd(const float* u, const float* dtp, const float* z, int ldz, const float* A, const float* Bm, const float* Cm,
                int ldbc, const float* Dp, const int32_t* start, int64_t B, int T, int Di, int N, float* out,
                hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(B), Di / kMbSlab);
  switch ((T + kWave - 1) / kWave) {
    case 1: mb_scan_fwd_kernel<1><<<grid, kBlock, 0, st>>>(u, dtp, z, ldz, A, Bm, Cm, ldbc, Dp, start, T, Di, N, out); break;
    case 2: mb_scan_fwd_kernel<2><<<grid, kBlock, 0, st>>>(u, dtp, z, ldz, A, Bm, Cm, ldbc, Dp, start, T, Di, N, out); break;
    case 3: mb_scan_fwd_kernel<3><<<grid, kBlock, 0, st>>>(u, dtp, z, ldz, A, Bm, Cm, ldbc, Dp, start, T, Di, N, out); break;
    default: mb_scan_fwd_kernel<4><<<grid, kBlock, 0, st>>>(u, dtp, z, ldz, A, Bm, Cm, ldbc, Dp, start, T, Di, N, out); break;
  }
  HIPREC_TRY(hipGetLastError());
  return 0;
}

int mb_fold(float* out, const float* part, const float* mul, int64_t n, int parts, hipStream_t st) {
  mb_fold_kernel<<<grid_for_threads(n), kBlock, 0, st>>>(out, part, mul, n, parts);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// du, ddtp [M, Di], dz (lddz), dBm / dCm (lddbc) and plain stores into dA (times a_mul if given) and dD; scratch holds
// mb_scan_scratch(...) floats
int mb_scan_bwd(const float* u, const float* dtp, const float* z, int ldz, const float* A, const float* Bm, const float* Cm,
                int ldbc, const float* Dp, const int32_t* start, const float* dout, int64_t B, int T, int Di, int N, float* du,
                float* ddtp, float* dz, int lddz, float* dA, const float* a_mul, float* dBm, float* dCm, int lddbc, float* dD,
                float* scratch, hipStream_t st) {
  const int P = mb_parts(B), slabs = Di / kMbSlab;
  float* partBC = scratch;
  float* partA = partBC + static_cast<int64_t>(slabs) * B * 2 * N * T;
  float* partD = partA + static_cast<int64_t>(P) * Di * N;
  const dim3 grid(P, slabs);
#define MB_BWD(KK)                                                                                                      \
  mb_scan_bwd_kernel<KK><<<grid, kBlock, 0, st>>>(u, dtp, z, ldz, A, Bm, Cm, ldbc, Dp, start, dout, B, T, Di, N, du, ddtp, dz, \
                                                  lddz, partBC, partA, partD)
  switch ((T + kWave - 1) / kWave) {
    case 1: MB_BWD(1); break;
    case 2: MB_BWD(2); break;
    case 3: MB_BWD(3); break;
    default: MB_BWD(4); break;
  }
#undef MB_BWD
  HIPREC_TRY(hipGetLastError());
  mb_bc_fold_kernel<<<grid_for_threads(B * 2 * N * T), kBlock, 0, st>>>(partBC, slabs, B, T, N, dBm, dCm, lddbc);
  HIPREC_TRY(hipGetLastError());
  if (int rc = mb_fold(dA, partA, a_mul, static_cast<int64_t>(Di) * N, P, st)) return rc;
  return mb_fold(dD, partD, nullptr, Di, P, st);
}

// ---- host side: the model -------------------------------------------------------------------------------------------------
struct MbLayer {
  float *in_w, *conv_w, *conv_b, *x_w, *dt_w, *dt_b, *a_log, *dp, *out_w, *ln1_w, *ln1_b, *f1_w, *f1_b, *f2_w, *f2_b, *ln2_w,
      *ln2_b;
};
struct MbParams {      // pointers into a flat buffer laid out in state_dict() order
  float *item_emb, *ln_e_w, *ln_e_b;
  MbLayer blk[kMbMaxBlocks];
};

struct MbDims {
  int T, D, Di, N, R, Kc, H, W;      // W = R + 2 N
};
MbDims mb_dims(const hiprec_mamba4rec_shape& s) {
  return MbDims{s.maxlen, s.dim, s.expand * s.dim, s.d_state, s.dt_rank, s.d_conv, s.ffn_dim, s.dt_rank + 2 * s.d_state};
}

int64_t mb_layer_floats(const MbDims& d) {
  const int64_t D = d.D, Di = d.Di;
  return 2 * Di * D + Di * d.Kc + Di + d.W * Di + Di * d.R + Di + Di * d.N + Di + D * Di + 2 * D + d.H * D + d.H + D * d.H + D +
         2 * D;
}

int64_t mb_n_params(const hiprec_mamba4rec_shape& s) {
  return (s.n_items + 1) * s.dim + 2 * s.dim + s.n_blocks * mb_layer_floats(mb_dims(s));
}

MbParams mb_params(float* base, const hiprec_mamba4rec_shape& s) {
  MbParams p{};
  const MbDims d = mb_dims(s);
  const int64_t D = d.D, Di = d.Di, H = d.H;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += n; return r; };
  p.item_emb = take((s.n_items + 1) * D);
  p.ln_e_w = take(D);
  p.ln_e_b = take(D);
  for (int k = 0; k < s.n_blocks; ++k) {
    MbLayer& q = p.blk[k];
    q.in_w = take(2 * Di * D);
    q.conv_w = take(Di * d.Kc);
    q.conv_b = take(Di);
    q.x_w = take(d.W * Di);
    q.dt_w = take(Di * d.R);
    q.dt_b = take(Di);
    q.a_log = take(Di * d.N);
    q.dp = take(Di);
    q.out_w = take(D * Di);
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

struct MbSaved {
  float *x, *xz, *u, *dbc, *dtp, *yg, *mo, *h, *pre, *z2, *mean1, *rstd1, *mean2, *rstd2, *A;
};
struct MbWorkspace {
  MbSaved sv[kMbMaxBlocks];
  float *raw, *mean_e, *rstd_e, *out, *f, *df, *aux, *gpos, *t[8], *xm, *tf[2], *dyg, *ddtp, *du_s, *du_x, *dxz, *ddbc, *cs,
      *part, *cpart, *spart;
  int32_t* start;
  int64_t floats;
};

int64_t mb_wgrad_floats(const MbDims& d) {
  const int64_t D = d.D, Di = d.Di;
  return std::max({2 * Di * D, static_cast<int64_t>(d.W) * Di, Di * d.R, static_cast<int64_t>(d.H) * D});
}

MbWorkspace mb_carve(float* base, const hiprec_mamba4rec_shape& s, int64_t B) {
  MbWorkspace w{};
  const MbDims d = mb_dims(s);
  const int64_t M = B * d.T, MD = M * d.D, MH = M * d.H, MI = M * d.Di, MW = M * d.W;
  const int wide = std::max({d.D, d.H, d.Di});
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += (n + 3) / 4 * 4; return r; };
  for (int k = 0; k < s.n_blocks; ++k)
    w.sv[k] = MbSaved{take(MD), take(2 * MI), take(MI), take(MW), take(MI), take(MI), take(MD), take(MD), take(MH), take(MD),
                      take(M), take(M), take(M), take(M), take(static_cast<int64_t>(d.Di) * d.N)};
  w.raw = take(MD);
  w.mean_e = take(M);
  w.rstd_e = take(M);
  w.out = take(MD);
  w.f = take(B * d.D);
  w.df = take(B * d.D);
  w.aux = take(kSeqAux);
  w.gpos = take(static_cast<int64_t>(d.T) * d.D);
  w.start = reinterpret_cast<int32_t*>(take(B));
  for (int i = 0; i < 8; ++i) w.t[i] = take(MD);
  w.xm = take(MD);
  for (int i = 0; i < 2; ++i) w.tf[i] = take(MH);
  w.dyg = take(MI);
  w.ddtp = take(MI);
  w.du_s = take(MI);
  w.du_x = take(MI);
  w.dxz = take(2 * MI);
  w.ddbc = take(MW);
  w.cs = take(2 * colsum_ws_floats(static_cast<int>(M), wide));
  w.part = take(kMbSlabs * mb_wgrad_floats(d));
  w.cpart = take(static_cast<int64_t>(mb_parts(B)) * d.Di * (d.Kc + 1));
  w.spart = take(mb_scan_scratch(B, d.T, d.Di, d.N));
  w.floats = c - base;
  return w;
}

int mb_check_shape(const hiprec_mamba4rec_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  HIPREC_REQUIRE(s->n_items >= 1 && s->n_items < (1ll << 31) - 1, "Mamba4Rec needs 1 <= n_items < 2^31 - 1");
  HIPREC_REQUIRE(s->dim >= 16 && s->dim <= kSeqMaxDim && s->dim % 16 == 0,
                 "Mamba4Rec needs emb_dim a multiple of 16 in 16 .. %d (got %d)", kSeqMaxDim, s->dim);
  HIPREC_REQUIRE(s->maxlen >= 1 && s->maxlen <= kSeqMaxLen, "Mamba4Rec needs 1 <= maxlen <= %d (got %d)", kSeqMaxLen,
                 s->maxlen);
  HIPREC_REQUIRE(s->n_blocks >= 1 && s->n_blocks <= kMbMaxBlocks, "Mamba4Rec needs 1 <= num_blocks <= %d (got %d)",
                 kMbMaxBlocks, s->n_blocks);
  HIPREC_REQUIRE(s->ffn_dim >= 16 && s->ffn_dim <= kMbMaxFfn && s->ffn_dim % 16 == 0,
                 "Mamba4Rec needs ffn_dim a multiple of 16 in 16 .. %d (got %d)", kMbMaxFfn, s->ffn_dim);
  HIPREC_REQUIRE(s->expand == 1 || s->expand == 2, "Mamba4Rec needs expand 1 or 2 (got %d)", s->expand);
  HIPREC_REQUIRE(s->d_state >= 1 && s->d_state <= kMbMaxState, "Mamba4Rec needs 1 <= d_state <= %d (got %d)", kMbMaxState,
                 s->d_state);
  HIPREC_REQUIRE(s->d_conv >= 2 && s->d_conv <= kMbMaxConv, "Mamba4Rec needs 2 <= d_conv <= %d (got %d)", kMbMaxConv,
                 s->d_conv);
  HIPREC_REQUIRE(s->dt_rank >= 1 && s->dt_rank <= kMbMaxRank, "Mamba4Rec needs 1 <= dt_rank <= %d (got %d)", kMbMaxRank,
                 s->dt_rank);
  return 0;
}

bool mb_batch_ok(const hiprec_mamba4rec_shape& s, int64_t B) { return B >= 1 && B * s.maxlen <= (1ll << 24); }

void mb_set_keep(GemmProblem& p, const uint8_t* keep, int ld, float ks) {
  if (keep) { p.keep = keep; p.ldk = ld; p.keep_scale = ks; }
}

// C[rows, cols] = A^T B over K batch rows, as problems of g: one with plain stores into the zeroed gradient, or (long K)
// up to kMbSlabs slabs of K into `part`, which mb_fold adds up in slab order afterwards.  Returns the slab count.
int mb_add_wgrad(GemmGroup& g, int rows, int cols, int K, const float* A, int lda, const float* Bm, int ldb, float* out,
                 float* part) {
  const int slabs = std::min(kMbSlabs, (K + 511) / 512);
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

// one Linear's backward as ONE grouped launch: dX [M, K] = dZ W (dX may be NULL), dW [N, K] = dZ^T X in slabs, d bias (may
// be NULL) = the column sums of dZ.  dZ [M, N] (lddz), W [N, K], X [M, K] (ldx); dxkeep: the keep bytes of dX's epilogue.
int mb_linear_bwd(int M, int N, int K, const float* dZ, int lddz, const float* W, const float* X, int ldx, float* dX,
                  int lddx, const uint8_t* dxkeep, float ks, float* gW, float* gb, float* part, float* cs, hipStream_t st) {
  GemmGroup p{};
  if (dX) {
    p.p[p.n] = make_gemm(kNN, M, K, N, dZ, lddz, W, K, dX, lddx, nullptr, 0, nullptr, 0, false);
    mb_set_keep(p.p[p.n++], dxkeep, lddx, ks);
  }
  const int slabs = mb_add_wgrad(p, N, K, M, dZ, lddz, X, ldx, gW, part);
  if (gb) p.p[p.n++] = make_colsum(dZ, M, N, lddz, gb, cs);
  if (int rc = launch_group(p, st)) return rc;
  if (gb)
    if (int rc = launch_colsum_reduce(p, st)) return rc;
  if (slabs > 1) return mb_fold(gW, part, nullptr, static_cast<int64_t>(N) * K, slabs, st);
  return 0;
}

int mb_linear_fwd(int M, int N, int K, const float* X, int ldx, const float* W, const float* bias, float* Z, int ldz,
                  const uint8_t* keep, float ks, hipStream_t st) {
  GemmGroup g{};
  g.n = 1;
  g.p[0] = make_gemm(kNT, M, N, K, X, ldx, W, K, Z, ldz, bias, 0, nullptr, 0, false);
  mb_set_keep(g.p[0], keep, ldz, ks);
  return launch_group(g, st);
}

int mb_run(const hiprec_mamba4rec_shape& s, float* w_flat, float* g_flat, const int64_t* seq, const int64_t* pos,
           const int64_t* neg, int64_t B, const uint8_t* const* keep, float ks, float* feats_out, hiprec_stats* stats,
           Scratch* scratch, float* ws_base, hipStream_t st) {
  const bool train = g_flat != nullptr;
  const MbDims d = mb_dims(s);
  const int T = d.T, D = d.D, Di = d.Di, N = d.N, R = d.R, Kc = d.Kc, H = d.H, W = d.W, nb = s.n_blocks;
  const int64_t M = B * T, MD = M * D, MH = M * H;
  const int Mi = static_cast<int>(M), P = mb_parts(B);
  const MbParams w = mb_params(w_flat, s);
  const MbWorkspace a = mb_carve(ws_base, s, B);
  auto kp = [&](int i) -> const uint8_t* { return (train && keep) ? keep[i] : nullptr; };

  // ---- forward ----
  mb_start_kernel<<<grid_for_threads(B), kBlock, 0, st>>>(seq, B, T, a.start);
  HIPREC_TRY(hipGetLastError());
  if (int rc = seq_embed(w.item_emb, nullptr, seq, M, T, D, s.n_items, 1.0f, kp(0), ks, a.raw, stats, st)) return rc;
  if (int rc = seq_ln_fwd(a.raw, nullptr, nullptr, nullptr, w.ln_e_w, w.ln_e_b, a.sv[0].x, a.mean_e, a.rstd_e, M, D, st,
                          kMbEps))
    return rc;
  for (int k = 0; k < nb; ++k) {
    const MbSaved& v = a.sv[k];
    const MbLayer& q = w.blk[k];
    mb_mask_kernel<<<grid_for_threads(MD), kBlock, 0, st>>>(v.x, a.start, M, T, D, a.xm);
    HIPREC_TRY(hipGetLastError());
    if (int rc = mb_linear_fwd(Mi, 2 * Di, D, a.xm, D, q.in_w, nullptr, v.xz, 2 * Di, nullptr, ks, st)) return rc;
    mb_conv_fwd_kernel<<<grid_for_threads(M * Di), kBlock, 0, st>>>(v.xz, 2 * Di, q.conv_w, q.conv_b, a.start, M, T, Di, Kc,
                                                                     v.u);
    HIPREC_TRY(hipGetLastError());
    if (int rc = mb_linear_fwd(Mi, W, Di, v.u, Di, q.x_w, nullptr, v.dbc, W, nullptr, ks, st)) return rc;
    if (int rc = mb_linear_fwd(Mi, Di, R, v.dbc, W, q.dt_w, q.dt_b, v.dtp, Di, nullptr, ks, st)) return rc;
    mb_neg_exp_kernel<<<(Di * N + kBlock - 1) / kBlock, kBlock, 0, st>>>(q.a_log, v.A, Di * N);
    HIPREC_TRY(hipGetLastError());
    if (int rc = mb_scan_fwd(v.u, v.dtp, v.xz + Di, 2 * Di, v.A, v.dbc + R, v.dbc + R + N, W, q.dp, a.start, B, T, Di, N,
                             v.yg, st))
      return rc;
    if (int rc = mb_linear_fwd(Mi, D, Di, v.yg, Di, q.out_w, nullptr, v.mo, D, kp(1 + 3 * k), ks, st)) return rc;
    if (int rc = seq_ln_fwd(v.mo, nb > 1 ? v.x : nullptr, nullptr, nullptr, q.ln1_w, q.ln1_b, v.h, v.mean1, v.rstd1, M, D, st,
                            kMbEps))
      return rc;
    if (int rc = mb_linear_fwd(Mi, H, D, v.h, D, q.f1_w, q.f1_b, v.pre, H, nullptr, ks, st)) return rc;
    mb_gelu_fwd_kernel<<<grid_for_threads(MH), kBlock, 0, st>>>(v.pre, kp(2 + 3 * k), ks, a.tf[0], MH);
    HIPREC_TRY(hipGetLastError());
    if (int rc = mb_linear_fwd(Mi, D, H, a.tf[0], H, q.f2_w, q.f2_b, v.z2, D, kp(3 + 3 * k), ks, st)) return rc;
    if (int rc = seq_ln_fwd(v.h, v.z2, nullptr, nullptr, q.ln2_w, q.ln2_b, k + 1 == nb ? a.out : a.sv[k + 1].x, v.mean2,
                            v.rstd2, M, D, st, kMbEps))
      return rc;
  }
  float* f = train ? a.f : feats_out;
  mb_last_rows_kernel<<<grid_for_threads(B * D), kBlock, 0, st>>>(a.out, B, T, D, f);
  HIPREC_TRY(hipGetLastError());
  if (!train) return 0;
  if (feats_out) HIPREC_TRY(hipMemcpyAsync(feats_out, f, sizeof(float) * B * D, hipMemcpyDeviceToDevice, st));

  // ---- loss on the B last-slot rows ----
  const MbParams g = mb_params(g_flat, s);
  float *S1 = a.t[0], *S1k = a.t[1], *S2 = a.t[2], *S3 = a.t[3], *S3k = a.t[4], *X1 = a.t[5], *U1 = a.t[6], *U2 = a.t[7];
  mb_count_kernel<<<1, kBlock, 0, st>>>(pos, B, a.aux);
  HIPREC_TRY(hipGetLastError());
  if (int rc = seq_loss(f, w.item_emb, pos, neg, B, D, s.n_items, a.aux, 0.f, a.df, g.item_emb, scratch, stats, st))
    return rc;
  mb_spread_last_kernel<<<grid_for_threads(MD), kBlock, 0, st>>>(a.df, M, T, D, S3);
  HIPREC_TRY(hipGetLastError());

  // ---- the layers in reverse: (dA, dB) = the two summands of the gradient of a layer's output ----
  const float *dA = S3, *dB = nullptr;
  for (int k = nb - 1; k >= 0; --k) {
    const MbSaved& v = a.sv[k];
    const MbLayer &q = w.blk[k], &gq = g.blk[k];
    // LN_2: S1 = gradient of h + z2, S1k = the same through the feed-forward's output dropout
    if (int rc = seq_ln_bwd(dA, dB, v.h, v.z2, q.ln2_w, v.mean2, v.rstd2, nullptr, nullptr, nullptr, kp(3 + 3 * k), ks, S1,
                            S1k, U1, U2, gq.ln2_w, gq.ln2_b, a.cs, M, D, st))
      return rc;
    const float* dz2 = kp(3 + 3 * k) ? S1k : S1;
    mb_gelu_fwd_kernel<<<grid_for_threads(MH), kBlock, 0, st>>>(v.pre, kp(2 + 3 * k), ks, a.tf[0], MH);
    HIPREC_TRY(hipGetLastError());
    if (int rc = mb_linear_bwd(Mi, D, H, dz2, D, q.f2_w, a.tf[0], H, a.tf[1], H, kp(2 + 3 * k), ks, gq.f2_w, gq.f2_b, a.part,
                               a.cs, st))
      return rc;
    mb_gelu_bwd_kernel<<<grid_for_threads(MH), kBlock, 0, st>>>(a.tf[1], v.pre, MH);
    HIPREC_TRY(hipGetLastError());
    if (int rc = mb_linear_bwd(Mi, H, D, a.tf[1], H, q.f1_w, v.h, D, S2, D, nullptr, ks, gq.f1_w, gq.f1_b, a.part, a.cs, st))
      return rc;
    // LN_1: dy = d(fc1 input) + the residual's gradient; S3 = gradient of mo + x, S3k = the same through the Mamba dropout
    if (int rc = seq_ln_bwd(S2, S1, v.mo, nb > 1 ? v.x : nullptr, q.ln1_w, v.mean1, v.rstd1, nullptr, nullptr, nullptr,
                            kp(1 + 3 * k), ks, S3, S3k, U1, U2, gq.ln1_w, gq.ln1_b, a.cs, M, D, st))
      return rc;
    const float* dmo = kp(1 + 3 * k) ? S3k : S3;
    if (int rc = mb_linear_bwd(Mi, D, Di, dmo, D, q.out_w, v.yg, Di, a.dyg, Di, nullptr, ks, gq.out_w, nullptr, a.part, a.cs,
                               st))
      return rc;
    if (int rc = mb_scan_bwd(v.u, v.dtp, v.xz + Di, 2 * Di, v.A, v.dbc + R, v.dbc + R + N, W, q.dp, a.start, a.dyg, B, T, Di,
                             N, a.du_s, a.ddtp, a.dxz + Di, 2 * Di, gq.a_log, v.A, a.ddbc + R, a.ddbc + R + N, W, gq.dp,
                             a.spart, st))
      return rc;
    // dt_proj: its input gradient is the first R columns of d [dt | Bm | Cm]
    if (int rc = mb_linear_bwd(Mi, Di, R, a.ddtp, Di, q.dt_w, v.dbc, W, a.ddbc, W, nullptr, ks, gq.dt_w, gq.dt_b, a.part, a.cs,
                               st))
      return rc;
    if (int rc = mb_linear_bwd(Mi, W, Di, a.ddbc, W, q.x_w, v.u, Di, a.du_x, Di, nullptr, ks, gq.x_w, nullptr, a.part, a.cs,
                               st))
      return rc;
    float* cpw = a.cpart;
    float* cpb = cpw + static_cast<int64_t>(P) * Di * Kc;
    mb_conv_bwd_kernel<<<dim3(Di / kMbConvSlab, P), kBlock, 0, st>>>(v.xz, 2 * Di, q.conv_w, q.conv_b, a.start, a.du_s, a.du_x,
                                                                     B, T, Di, Kc, a.dxz, 2 * Di, cpw, cpb);
    HIPREC_TRY(hipGetLastError());
    if (int rc = mb_fold(gq.conv_w, cpw, nullptr, static_cast<int64_t>(Di) * Kc, P, st)) return rc;
    if (int rc = mb_fold(gq.conv_b, cpb, nullptr, Di, P, st)) return rc;
    mb_mask_kernel<<<grid_for_threads(MD), kBlock, 0, st>>>(v.x, a.start, M, T, D, a.xm);
    HIPREC_TRY(hipGetLastError());
    if (int rc = mb_linear_bwd(Mi, 2 * Di, D, a.dxz, 2 * Di, q.in_w, a.xm, D, U1, D, nullptr, ks, gq.in_w, nullptr, a.part,
                               a.cs, st))
      return rc;
    mb_mask_kernel<<<grid_for_threads(MD), kBlock, 0, st>>>(U1, a.start, M, T, D, X1);
    HIPREC_TRY(hipGetLastError());
    if (nb > 1) {
      dA = S3;        // the residual's share of d x[k] ...
      dB = X1;        // ... and the Mamba layer's
    } else {
      dA = X1;
      dB = nullptr;
    }
  }
  // embedding: LN_e, then the dropout inside the table's backward
  if (int rc = seq_ln_bwd(dA, dB, a.raw, nullptr, w.ln_e_w, a.mean_e, a.rstd_e, nullptr, nullptr, nullptr, nullptr, ks, S1,
                          nullptr, U1, U2, g.ln_e_w, g.ln_e_b, a.cs, M, D, st))
    return rc;
  return seq_embed_bwd(S1, seq, B, T, D, s.n_items, 1.0f, kp(0), ks, g.item_emb, a.gpos, st);
}

int mb_check_call(const hiprec_mamba4rec_shape* shape, const void* w_flat, const void* seq, int64_t batch, const void* stats,
                  const void* workspace, size_t workspace_bytes) {
  if (int rc = mb_check_shape(shape)) return rc;
  HIPREC_REQUIRE(w_flat && seq && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(mb_batch_ok(*shape, batch), "Mamba4Rec: batch %lld must be >= 1 and batch x maxlen %d at most 2^24",
                 static_cast<long long>(batch), shape->maxlen);
  const size_t need = hiprec_mamba4rec_workspace_bytes(shape, batch);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  return 0;
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_mamba4rec_shape_bytes(void) { return sizeof(hiprec_mamba4rec_shape); }

extern "C" int64_t hiprec_mamba4rec_param_floats(const hiprec_mamba4rec_shape* shape) {
  if (mb_check_shape(shape)) return -1;
  return mb_n_params(*shape);
}

extern "C" size_t hiprec_mamba4rec_workspace_bytes(const hiprec_mamba4rec_shape* shape, int64_t batch) {
  if (mb_check_shape(shape) || !mb_batch_ok(*shape, batch)) return 0;
  return sizeof(float) * static_cast<size_t>(mb_carve(nullptr, *shape, batch).floats);
}

extern "C" int hiprec_mamba4rec_grad(const hiprec_mamba4rec_shape* shape, const float* w_flat, float* g_flat,
                                     const int64_t* seq, const int64_t* pos, const int64_t* neg, int64_t batch,
                                     const uint8_t* const* keep, float keep_scale, float* feats_out, hiprec_stats* stats,
                                     void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (int rc = mb_check_call(shape, w_flat, seq, batch, stats, workspace, workspace_bytes)) return rc;
  HIPREC_REQUIRE(g_flat && pos && neg && scratch, "training needs the gradient buffer, pos, neg and the scratch block");
  if (scratch_bytes < kScratchBytes) {
    set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
    return HIPREC_E_SCRATCH;
  }
  return mb_run(*shape, const_cast<float*>(w_flat), g_flat, seq, pos, neg, batch, keep, keep_scale, feats_out, stats,
                static_cast<Scratch*>(scratch), static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_mamba4rec_feats(const hiprec_mamba4rec_shape* shape, const float* w_flat, const int64_t* seq,
                                      int64_t batch, float* feats_out, hiprec_stats* stats, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  if (int rc = mb_check_call(shape, w_flat, seq, batch, stats, workspace, workspace_bytes)) return rc;
  HIPREC_REQUIRE(feats_out, "the eval forward needs the feats buffer");
  return mb_run(*shape, const_cast<float*>(w_flat), nullptr, seq, nullptr, nullptr, batch, nullptr, 1.0f, feats_out, stats,
                nullptr, static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int64_t hiprec_mamba4rec_scan_scratch_floats(int64_t batch, int32_t seq_len, int32_t d_inner, int32_t d_state) {
  if (!mb_scan_shape_ok(batch, seq_len, d_inner, d_state)) return -1;
  return mb_scan_scratch(batch, seq_len, d_inner, d_state);
}

extern "C" int hiprec_mamba4rec_scan(const float* u, const float* dt_pre, const float* z, const float* A, const float* Bm,
                                     const float* Cm, const float* D, const int32_t* start, const float* dout, int64_t batch,
                                     int32_t seq_len, int32_t d_inner, int32_t d_state, float* out, float* du, float* ddt_pre,
                                     float* dz, float* dA, float* dBm, float* dCm, float* dD, float* scratch,
                                     size_t scratch_floats, void* stream) {
  HIPREC_REQUIRE(u && dt_pre && z && A && Bm && Cm && D && start && (out || dout), "NULL pointer");
  HIPREC_REQUIRE(mb_scan_shape_ok(batch, seq_len, d_inner, d_state), "Mamba4Rec scan: shape outside the model's limits");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (out)
    if (int rc = mb_scan_fwd(u, dt_pre, z, d_inner, A, Bm, Cm, d_state, D, start, batch, seq_len, d_inner, d_state, out, st))
      return rc;
  if (!dout) return 0;
  HIPREC_REQUIRE(du && ddt_pre && dz && dA && dBm && dCm && dD && scratch, "the scan backward needs every gradient buffer");
  const int64_t need = mb_scan_scratch(batch, seq_len, d_inner, d_state);
  HIPREC_REQUIRE(scratch_floats >= static_cast<size_t>(need), "scan scratch %zu floats < %lld", scratch_floats,
                 static_cast<long long>(need));
  return mb_scan_bwd(u, dt_pre, z, d_inner, A, Bm, Cm, d_state, D, start, dout, batch, seq_len, d_inner, d_state, du, ddt_pre,
                     dz, d_inner, dA, nullptr, dBm, dCm, d_state, dD, scratch, st);
}
