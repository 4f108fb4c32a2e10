// Deep Interest Network (Zhou et al., KDD 2018): zero_grad + forward + loss + backward of one ranking step as a fixed
// sequence of launches, no host sync.  The contract is in include/hiprec.h; B sequences of T slots, C candidates per
// sequence, N = B C candidate rows, D = dim, H1 / H2 the widths of the activation unit, W_l those of the tower.
//
// The unit's first layer is split: att.0.weight = [Wq | We | Wd | Wp] and
//   att.0 [q, e, q - e, q * e] = (Wq + Wd) q + (We - Wd) e + Wp (q * e),
// so U = E[seq] (We - Wd)^T + b0 [B T, H1] and V = E[cand] (Wq + Wd)^T [N, H1] are two problems of ONE grouped GEMM launch
// and only the last term, a product of depth D, is per (candidate, position) pair.
//
//   prep      the folded weights We - Wd, Wq + Wd and zero-padded copies of Wp [H1p, D + 4], att.1.weight [H2p, H1p + 4]
//             and the unit's vectors (H1p / H2p: the widths rounded up to the 16 of the MFMA tile)
//   gather    E[seq], E[cand] as rows, the live flags, the status word of an id out of range
//   unit fwd  a workgroup owns one sequence and kDinSlice candidates.  History rows are staged into LDS in chunks of R <= 64
//             positions and reused by every candidate of the workgroup; Wp and att.1.weight are copied into LDS once per
//             workgroup when they fit beside the chunk (every shape but the widest), else the MFMA reads the padded copies
//             through L2.  A wave owns one tile of 16 positions: pre1 = U + V + (e * q) Wp^T on v_mfma_f32_16x16x4_f32 with
//             the e * q operand formed while it is read from LDS, the activation on the accumulators, h1 through LDS into
//             the operand layout of the [16, H1] x [H1, H2] product, activation, the H2 -> 1 dot by a 16-lane shuffle sum,
//             scale and mask; pooled accumulates from the staged rows.  x, pre1, h1, h2 never reach memory.
//   tower     z = [pooled, q, pooled * q]; Linear layers through the grouped GEMM; Dice / PReLU as column kernels (a block
//             owns 16 columns, 16 row groups, the groups' partial sums are folded in a fixed order); BCE one lane per row
//   unit bwd  a workgroup walks whole sequences (b = block, block + grid, ...; grid <= kDinSlabs).  It recomputes h1 and
//             pre2, then d pre2, d att.1.weight += d pre2^T h1 (MFMA over the chunk's positions, the tiles dealt to the four
//             waves, accumulators live across every candidate and sequence of the workgroup), d h1, d pre1, d Wp likewise,
//             d (e * q).  d U and d V leave by plain read-modify-write of rows only this workgroup touches, d e is summed over
//             the candidates in LDS and leaves as one row atomic per (sequence, position).  The weight partials go to the
//             workgroup's slab; a later kernel folds the slabs in order and unfolds d (We - Wd), d (Wq + Wd), which the
//             grouped GEMM made from d U and d V, into d att.0.weight.
//
// The only float atomics are rows of d item_emb.weight; every other gradient is the same bits on every run.
#include <algorithm>

#include "din.hpp"

namespace hiprec {
namespace {

constexpr int kDinMaxAtt = 128;
constexpr int kDinTile = 16;                   // positions of a wave's MFMA tile
constexpr int kDinMaxChunk = 64;               // staged positions: one tile per wave
constexpr int kDinSlice = 4;                   // forward: candidates of a workgroup
constexpr int kDinSlabs = 256;                 // backward: workgroups, each with a slab of weight partials
constexpr int kDinColTiles = kDinMaxAtt / 16;  // column tiles a wave walks per product
constexpr int kDinWTiles = kDinColTiles * kDinColTiles / kWavesPerBlock;   // weight-gradient tiles of a wave
constexpr int kDinSplitE = 8, kDinSplitQ = 3;  // K-slices of the two folded-weight gradient GEMMs (one grouped launch)
constexpr size_t kDinLdsBudget = 160 * 1024;
constexpr float kDiceEps = 1e-8f, kDiceMomentum = 0.1f;
constexpr int kColW = 16, kColG = 16;          // column kernels: columns and row groups of a block
constexpr int kColFly = 8;                     // ... rows a thread has in flight

struct DinDims {
  int64_t n_items;
  int D, T, H1, H2, att_act, dnn_act, L, W[kDinMaxLayers];
  int H1p, H2p;
};

// offsets into the flat parameter buffer (state_dict() order)
struct DinOff {
  int64_t a0w, a0b, a0a, a1w, a1b, a1a, a2w, a2b, dw[kDinMaxLayers], db[kDinMaxLayers], da[kDinMaxLayers], ow, ob, total;
  int in[kDinMaxLayers], bn[kDinMaxLayers], bn_total;
};

DinOff din_offsets(const DinDims& q) {
  DinOff o{};
  int64_t p = (q.n_items + 1) * q.D;
  auto take = [&](int64_t n) { int64_t r = p; p += n; return r; };
  o.a0w = take(static_cast<int64_t>(q.H1) * 4 * q.D); o.a0b = take(q.H1); o.a0a = take(q.H1);
  o.a1w = take(static_cast<int64_t>(q.H2) * q.H1); o.a1b = take(q.H2); o.a1a = take(q.H2);
  o.a2w = take(q.H2); o.a2b = take(1);
  int in = 3 * q.D, bn = 0;
  for (int l = 0; l < q.L; ++l) {
    o.in[l] = in;
    o.dw[l] = take(static_cast<int64_t>(q.W[l]) * in); o.db[l] = take(q.W[l]); o.da[l] = take(q.W[l]);
    o.bn[l] = bn;
    bn += 2 * q.W[l];
    in = q.W[l];
  }
  o.ow = take(in); o.ob = take(1);
  o.total = p;
  o.bn_total = bn;
  return o;
}

// ---- the activation unit ---------------------------------------------------------------------------------------------------
struct DinUnit {
  int T, C, D, H1, H2, H1p, H2p, R, act;
  int ldE, ldH, ldG, ldWp, ldW1, wp_lds, w1_lds;
  float scale;
  const float *WpP, *W1P, *w2P, *b1P, *al1P, *al2P, *b2;      // padded copies (prep) and att.2.bias
  const float *rows, *q, *U, *V;                              // E[seq] [B T, D], E[cand] [N, D], U [B T, H1], V [N, H1]
  const uint8_t *lv, *lc;                                     // live positions [B T], live candidates [N]
};

__device__ __forceinline__ float din_act(float x, float alpha, int kind) {
  return kind ? (x > 0.f ? x : alpha * x) : 1.f / (1.f + expf(-x));
}
// d act / d pre from the pre-activation and the activation
__device__ __forceinline__ float din_dact(float x, float h, float alpha, int kind) {
  return kind ? (x > 0.f ? 1.f : alpha) : h * (1.f - h);
}

__device__ __forceinline__ f32x4 din_zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// the LDS every unit kernel starts with: vectors, then the weights (when resident), then the chunk buffers
struct DinLds {
  float *w2, *b1, *al2, *al1, *qs, *dps, *as, *at, *ls, *red, *Es, *Hs, *dEs, *G1, *G2;
  const float *Wp, *W1;
};

__device__ __forceinline__ DinLds din_carve(float* base, const DinUnit& u, bool bwd) {
  DinLds s;
  float* p = base;
  auto take = [&](int n) { float* r = p; p += n; return r; };
  s.w2 = take(u.H2p); s.b1 = take(u.H2p); s.al2 = take(u.H2p); s.al1 = take(u.H1p);
  s.qs = take(u.D); s.dps = take(u.D);
  s.as = take(kDinMaxChunk); s.at = take(kDinMaxChunk); s.ls = take(kDinMaxChunk);
  s.red = take(kWavesPerBlock * kDinColTiles * 16);
  s.Es = take(u.R * u.ldE); s.Hs = take(u.R * u.ldH);
  s.dEs = s.G1 = s.G2 = nullptr;
  if (bwd) { s.dEs = take(u.R * u.ldE); s.G1 = take(u.R * u.ldH); s.G2 = take(u.R * u.ldG); }
  float* wp = u.wp_lds ? take(u.H1p * u.ldWp) : nullptr;
  float* w1 = u.w1_lds ? take(u.H2p * u.ldW1) : nullptr;
  for (int e = threadIdx.x; e < u.H2p; e += kBlock) { s.w2[e] = u.w2P[e]; s.b1[e] = u.b1P[e]; s.al2[e] = u.al2P[e]; }
  for (int e = threadIdx.x; e < u.H1p; e += kBlock) s.al1[e] = u.al1P[e];
  if (wp) for (int e = threadIdx.x; e < u.H1p * u.ldWp; e += kBlock) wp[e] = u.WpP[e];
  if (w1) for (int e = threadIdx.x; e < u.H2p * u.ldW1; e += kBlock) w1[e] = u.W1P[e];
  s.Wp = wp ? wp : u.WpP;
  s.W1 = w1 ? w1 : u.W1P;
  return s;
}

// rows [t0, t0 + R) of sequence b into Es (dead and out-of-range positions are zero rows), their live flags into ls
__device__ __forceinline__ void din_stage(const DinUnit& u, const DinLds& s, int64_t b, int t0) {
  for (int t = threadIdx.x; t < u.R; t += kBlock) s.ls[t] = (t0 + t < u.T && u.lv[b * u.T + t0 + t]) ? 1.f : 0.f;
  for (int e = threadIdx.x; e < u.R * u.D; e += kBlock) {
    const int t = e / u.D, d = e - t * u.D;
    const bool ok = t0 + t < u.T && u.lv[b * u.T + t0 + t];
    s.Es[t * u.ldE + d] = ok ? u.rows[(b * u.T + t0 + t) * u.D + d] : 0.f;
  }
}

// A wave's tile of 16 positions [r0, r0 + 16): h1 = act(U + V + (e * q) Wp^T) into Hs, with KEEP the pre-activation into G1
template <bool KEEP>
__device__ __forceinline__ void din_layer1(const DinUnit& u, const DinLds& s, int64_t b, int64_t n, int t0, int r0) {
  const int l = lane_id(), li = l & 15, lk = l >> 4;
  const float* ap = s.Es + (r0 + li) * u.ldE + lk;
  for (int tc = 0; tc < u.H1p / 16; ++tc) {
    const float* bp = s.Wp + (tc * 16 + li) * u.ldWp + lk;
    f32x4 acc = din_zero4();
    for (int k = 0; k < u.D; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k] * s.qs[k + lk], bp[k], acc, 0, 0, 0);
    const int j = tc * 16 + li;
    const float vj = j < u.H1 ? u.V[n * u.H1 + j] : 0.f, al = s.al1[j];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = r0 + 4 * lk + r;
      const float uj = (j < u.H1 && t0 + t < u.T) ? u.U[(b * u.T + t0 + t) * u.H1 + j] : 0.f;
      const float pre = acc[r] + uj + vj;
      s.Hs[t * u.ldH + j] = din_act(pre, al, u.act);
      if (KEEP) s.G1[t * u.ldH + j] = pre;
    }
  }
}

// pre2 tile tc of the wave's positions: h1 [16, H1p] x att.1.weight^T
__device__ __forceinline__ f32x4 din_layer2_tile(const DinUnit& u, const DinLds& s, int r0, int tc) {
  const int l = lane_id(), li = l & 15, lk = l >> 4;
  const float* ap = s.Hs + (r0 + li) * u.ldH + lk;
  const float* bp = s.W1 + (tc * 16 + li) * u.ldW1 + lk;
  f32x4 acc = din_zero4();
  for (int k = 0; k < u.H1p; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k], bp[k], acc, 0, 0, 0);
  return acc;
}

// grid B * ceil(C / kDinSlice).  pooled [N, D], a [N, T]
__global__ __launch_bounds__(kBlock) void din_unit_fwd_kernel(DinUnit u, float* __restrict__ pooled, float* __restrict__ a) {
  extern __shared__ float din_lds[];
  const DinLds s = din_carve(din_lds, u, false);
  const int n_slice = (u.C + kDinSlice - 1) / kDinSlice;
  const int64_t b = blockIdx.x / n_slice;
  const int c0 = (blockIdx.x % n_slice) * kDinSlice;
  const int l = lane_id(), li = l & 15, lk = l >> 4, r0 = wave_in_block() * kDinTile;
  const float b2 = u.b2[0];
  float pool[kDinSlice];
#pragma unroll
  for (int ci = 0; ci < kDinSlice; ++ci) pool[ci] = 0.f;
  for (int t0 = 0; t0 < u.T; t0 += u.R) {
    __syncthreads();
    din_stage(u, s, b, t0);
#pragma unroll
    for (int ci = 0; ci < kDinSlice; ++ci) {
      const int c = c0 + ci;
      if (c >= u.C) break;
      const int64_t n = b * u.C + c;
      if (!u.lc[n]) {      // a dead slot: a = 0, pooled = 0
        for (int t = threadIdx.x; t < u.R; t += kBlock)
          if (t0 + t < u.T) a[n * u.T + t0 + t] = 0.f;
        continue;
      }
      __syncthreads();
      for (int d = threadIdx.x; d < u.D; d += kBlock) s.qs[d] = u.q[n * u.D + d];
      __syncthreads();
      if (r0 < u.R) din_layer1<false>(u, s, b, n, t0, r0);
      __syncthreads();
      if (r0 < u.R) {
        float part[4] = {0.f, 0.f, 0.f, 0.f};
        for (int tc = 0; tc < u.H2p / 16; ++tc) {
          const f32x4 acc = din_layer2_tile(u, s, r0, tc);
          const int j = tc * 16 + li;
          const float w = s.w2[j], bj = s.b1[j], al = s.al2[j];
#pragma unroll
          for (int r = 0; r < 4; ++r) part[r] = fmaf(din_act(acc[r] + bj, al, u.act), w, part[r]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = part[r];
          v += __shfl_xor(v, 8, 16);
          v += __shfl_xor(v, 4, 16);
          v += __shfl_xor(v, 2, 16);
          v += __shfl_xor(v, 1, 16);
          const int t = r0 + 4 * lk + r;
          if (li == 0) s.as[t] = s.ls[t] != 0.f ? (v + b2) * u.scale : 0.f;
        }
      }
      __syncthreads();
      for (int t = threadIdx.x; t < u.R; t += kBlock)
        if (t0 + t < u.T) a[n * u.T + t0 + t] = s.as[t];
      if (static_cast<int>(threadIdx.x) < u.D) {
        float p = pool[ci];
        for (int t = 0; t < u.R; ++t) p = fmaf(s.as[t], s.Es[t * u.ldE + threadIdx.x], p);
        pool[ci] = p;
      }
    }
  }
#pragma unroll
  for (int ci = 0; ci < kDinSlice; ++ci)
    if (c0 + ci < u.C && static_cast<int>(threadIdx.x) < u.D) pooled[(b * u.C + c0 + ci) * u.D + threadIdx.x] = pool[ci];
}

// Slab of one backward workgroup: d Wp [H1, D], d att.1.weight [H2, H1], d att.1.bias, d alpha2, d att.2.weight [H2],
// d alpha1 [H1], d att.2.bias [1]
struct DinSlab {
  int64_t wp, w1, b1, al2, w2, al1, b2, floats;
};
__host__ __device__ inline DinSlab din_slab(int D, int H1, int H2) {
  DinSlab o;
  o.wp = 0;
  o.w1 = o.wp + static_cast<int64_t>(H1) * D;
  o.b1 = o.w1 + static_cast<int64_t>(H2) * H1;
  o.al2 = o.b1 + H2;
  o.w2 = o.al2 + H2;
  o.al1 = o.w2 + H2;
  o.b2 = o.al1 + H1;
  o.floats = (o.b2 + 1 + 3) / 4 * 4;
  return o;
}

// a wave's per-lane column partials -> out[0 .. width): lane groups by shuffle, waves through LDS, both in a fixed order
__device__ __forceinline__ void din_fold_columns(const float (&p)[kDinColTiles], float* red, float* out, int width) {
  const int l = lane_id(), wave = wave_in_block();
  __syncthreads();
#pragma unroll
  for (int tc = 0; tc < kDinColTiles; ++tc) {
    float v = p[tc];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (l < 16) red[(wave * kDinColTiles + tc) * 16 + l] = v;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < width; j += kBlock) {
    float t = 0.f;
    for (int w = 0; w < kWavesPerBlock; ++w) t += red[w * kDinColTiles * 16 + j];
    out[j] = t;
  }
}

// grid min(B, kDinSlabs).  a [N, T] of the forward, dpooled [N, D]; dU [B T, H1], dV [N, H1] and dq [N, D] are ADDED to
// (rows of this workgroup's sequences only); d e goes to de_out [B T, D] by plain stores when given, else as row atomics
// into g_item at seq's ids.
__global__ __launch_bounds__(kBlock) void din_unit_bwd_kernel(DinUnit u, int64_t B, const float* __restrict__ a,
                                                              const float* __restrict__ dpooled,
                                                              const int64_t* __restrict__ seq, float* __restrict__ dU,
                                                              float* __restrict__ dV, float* __restrict__ dq,
                                                              float* __restrict__ g_item, float* __restrict__ de_out,
                                                              float* __restrict__ slabs) {
  extern __shared__ float din_lds[];
  const DinLds s = din_carve(din_lds, u, true);
  const int l = lane_id(), li = l & 15, lk = l >> 4, wave = wave_in_block(), r0 = wave * kDinTile;
  const int n1 = u.H1p / 16, n2 = u.H2p / 16, nd = u.D / 16;
  f32x4 accW1[kDinWTiles], accWp[kDinWTiles];
#pragma unroll
  for (int i = 0; i < kDinWTiles; ++i) accW1[i] = accWp[i] = din_zero4();
  float p_w2[kDinColTiles], p_b1[kDinColTiles], p_al2[kDinColTiles], p_al1[kDinColTiles], p_b2 = 0.f;
#pragma unroll
  for (int i = 0; i < kDinColTiles; ++i) p_w2[i] = p_b1[i] = p_al2[i] = p_al1[i] = 0.f;

  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    for (int t0 = 0; t0 < u.T; t0 += u.R) {
      __syncthreads();
      din_stage(u, s, b, t0);
      for (int e = threadIdx.x; e < u.R * u.ldE; e += kBlock) s.dEs[e] = 0.f;
      for (int c = 0; c < u.C; ++c) {
        const int64_t n = b * u.C + c;
        if (!u.lc[n]) continue;
        __syncthreads();
        for (int d = threadIdx.x; d < u.D; d += kBlock) {
          s.qs[d] = u.q[n * u.D + d];
          s.dps[d] = dpooled[n * u.D + d];
        }
        __syncthreads();
        if (static_cast<int>(threadIdx.x) < u.R) {      // d a_t = <d pooled, e_t> / sqrt(D) on the live positions
          const int t = threadIdx.x;
          float da = 0.f, at = 0.f;
          if (s.ls[t] != 0.f) {
            for (int d = 0; d < u.D; ++d) da = fmaf(s.dps[d], s.Es[t * u.ldE + d], da);
            da *= u.scale;
            at = a[n * u.T + t0 + t];
          }
          s.as[t] = da;
          s.at[t] = at;
          p_b2 += da;
        }
        if (r0 < u.R) din_layer1<true>(u, s, b, n, t0, r0);
        __syncthreads();
        if (r0 < u.R) {      // pre2 -> d pre2 into G2, the column partials of att.1.bias, att.2.weight, alpha2
#pragma unroll
          for (int tc = 0; tc < kDinColTiles; ++tc) {
            if (tc >= n2) break;
            const f32x4 acc = din_layer2_tile(u, s, r0, tc);
            const int j = tc * 16 + li;
            const float w = s.w2[j], bj = s.b1[j], al = s.al2[j];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int t = r0 + 4 * lk + r;
              const float pre = acc[r] + bj, h = din_act(pre, al, u.act), da = s.as[t], dh = da * w;
              const float dp = dh * din_dact(pre, h, al, u.act);
              s.G2[t * u.ldG + j] = dp;
              p_w2[tc] = fmaf(da, h, p_w2[tc]);
              p_b1[tc] += dp;
              if (u.act) p_al2[tc] = fmaf(dh, fminf(pre, 0.f), p_al2[tc]);
            }
          }
        }
        __syncthreads();
        // d att.1.weight += d pre2^T h1 over the chunk's positions
#pragma unroll
        for (int i = 0; i < kDinWTiles; ++i) {
          const int tile = wave + kWavesPerBlock * i;
          if (tile >= n2 * n1) break;
          const int t2 = tile / n1, t1 = tile - t2 * n1;
          const float* ap = s.G2 + lk * u.ldG + t2 * 16 + li;
          const float* bp = s.Hs + lk * u.ldH + t1 * 16 + li;
          for (int k = 0; k < u.R; k += 4)
            accW1[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k * u.ldG], bp[k * u.ldH], accW1[i], 0, 0, 0);
        }
        if (r0 < u.R) {      // d h1 = d pre2 att.1.weight -> d pre1 over G1's pre-activations
          const float* ap = s.G2 + (r0 + li) * u.ldG + lk;
#pragma unroll
          for (int tc = 0; tc < kDinColTiles; ++tc) {
            if (tc >= n1) break;
            const float* bp = s.W1 + lk * u.ldW1 + tc * 16 + li;
            f32x4 acc = din_zero4();
            for (int k = 0; k < u.H2p; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k], bp[k * u.ldW1], acc, 0, 0, 0);
            const int j = tc * 16 + li;
            const float al = s.al1[j];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int at = (r0 + 4 * lk + r) * u.ldH + j;
              const float pre = s.G1[at];
              s.G1[at] = acc[r] * din_dact(pre, s.Hs[at], al, u.act);
              if (u.act) p_al1[tc] = fmaf(acc[r], fminf(pre, 0.f), p_al1[tc]);
            }
          }
        }
        __syncthreads();
        for (int j = threadIdx.x; j < u.H1; j += kBlock) {      // d V[n] += the column sums of d pre1
          float t = 0.f;
          for (int r = 0; r < u.R; ++r) t += s.G1[r * u.ldH + j];
          dV[n * u.H1 + j] += t;
        }
        for (int e = threadIdx.x; e < u.R * u.H1; e += kBlock) {      // d U[b, t] += d pre1
          const int t = e / u.H1, j = e - t * u.H1;
          if (t0 + t < u.T) dU[(b * u.T + t0 + t) * u.H1 + j] += s.G1[t * u.ldH + j];
        }
        // d Wp += d pre1^T (e * q)
#pragma unroll
        for (int i = 0; i < kDinWTiles; ++i) {
          const int tile = wave + kWavesPerBlock * i;
          if (tile >= n1 * nd) break;
          const int t1 = tile / nd, td = tile - t1 * nd;
          const float* ap = s.G1 + lk * u.ldH + t1 * 16 + li;
          const float* bp = s.Es + lk * u.ldE + td * 16 + li;
          const float qd = s.qs[td * 16 + li];
          for (int k = 0; k < u.R; k += 4)
            accWp[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k * u.ldH], bp[k * u.ldE] * qd, accWp[i], 0, 0, 0);
        }
        if (r0 < u.R) {      // d (e * q) = d pre1 Wp: d e in LDS, the terms of d q over the freed h1
          const float* ap = s.G1 + (r0 + li) * u.ldH + lk;
          for (int td = 0; td < nd; ++td) {
            const float* bp = s.Wp + lk * u.ldWp + td * 16 + li;
            f32x4 acc = din_zero4();
            for (int k = 0; k < u.H1p; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k], bp[k * u.ldWp], acc, 0, 0, 0);
            const int d = td * 16 + li;
            const float qd = s.qs[d], dpd = s.dps[d];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int t = r0 + 4 * lk + r;
              s.dEs[t * u.ldE + d] += fmaf(acc[r], qd, s.at[t] * dpd);
              s.Hs[t * u.ldH + d] = acc[r] * s.Es[t * u.ldE + d];
            }
          }
        }
        __syncthreads();
        for (int d = threadIdx.x; d < u.D; d += kBlock) {
          float t = 0.f;
          for (int r = 0; r < u.R; ++r) t += s.Hs[r * u.ldH + d];
          dq[n * u.D + d] += t;
        }
      }
      __syncthreads();
      for (int e = threadIdx.x; e < u.R * u.D; e += kBlock) {
        const int t = e / u.D, d = e - t * u.D;
        if (t0 + t >= u.T) continue;
        const int64_t m = b * u.T + t0 + t;
        const float v = s.dEs[t * u.ldE + d];
        if (de_out) de_out[m * u.D + d] = v;
        else if (s.ls[t] != 0.f && v != 0.f) atomic_add_f32(g_item + seq[m] * u.D + d, v);
      }
    }
  }

  const DinSlab o = din_slab(u.D, u.H1, u.H2);
  float* slab = slabs + static_cast<int64_t>(blockIdx.x) * o.floats;
#pragma unroll
  for (int i = 0; i < kDinWTiles; ++i) {
    const int tile = wave + kWavesPerBlock * i;
    if (tile < n2 * n1) {
      const int t2 = tile / n1, t1 = tile - t2 * n1, j1 = t1 * 16 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j2 = t2 * 16 + 4 * lk + r;
        if (j2 < u.H2 && j1 < u.H1) slab[o.w1 + static_cast<int64_t>(j2) * u.H1 + j1] = accW1[i][r];
      }
    }
    if (tile < n1 * nd) {
      const int t1 = tile / nd, td = tile - t1 * nd, d = td * 16 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = t1 * 16 + 4 * lk + r;
        if (j < u.H1) slab[o.wp + static_cast<int64_t>(j) * u.D + d] = accWp[i][r];
      }
    }
  }
  din_fold_columns(p_b1, s.red, slab + o.b1, u.H2);
  din_fold_columns(p_al2, s.red, slab + o.al2, u.H2);
  din_fold_columns(p_w2, s.red, slab + o.w2, u.H2);
  din_fold_columns(p_al1, s.red, slab + o.al1, u.H1);
  __syncthreads();
  s.red[threadIdx.x] = p_b2;      // threads beyond R hold 0
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < kDinMaxChunk; ++i) t += s.red[i];
    slab[o.b2] = t;
  }
}

// ---- prep, gather, z, the folds ----------------------------------------------------------------------------------------------
struct DinPrep {
  const float *a0w, *a0a, *a1w, *a1b, *a1a, *a2w;
  float *Wfe, *Wfq, *WpP, *W1P, *w2P, *b1P, *al1P, *al2P;
  int D, H1, H2, H1p, H2p;
};
__global__ __launch_bounds__(kBlock) void din_prep_kernel(DinPrep p) {
  const int ldWp = p.D + 4, ldW1 = p.H1p + 4;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < p.H1 * p.D) {
    const int j = i / p.D, d = i - j * p.D;
    const float* row = p.a0w + static_cast<int64_t>(j) * 4 * p.D;
    p.Wfq[i] = row[d] + row[2 * p.D + d];
    p.Wfe[i] = row[p.D + d] - row[2 * p.D + d];
  }
  if (i < p.H1p * ldWp) {
    const int j = i / ldWp, d = i - j * ldWp;
    p.WpP[i] = (j < p.H1 && d < p.D) ? p.a0w[static_cast<int64_t>(j) * 4 * p.D + 3 * p.D + d] : 0.f;
  }
  if (i < p.H2p * ldW1) {
    const int j = i / ldW1, k = i - j * ldW1;
    p.W1P[i] = (j < p.H2 && k < p.H1) ? p.a1w[static_cast<int64_t>(j) * p.H1 + k] : 0.f;
  }
  if (i < p.H2p) {
    p.w2P[i] = i < p.H2 ? p.a2w[i] : 0.f;
    p.b1P[i] = i < p.H2 ? p.a1b[i] : 0.f;
    p.al2P[i] = i < p.H2 ? p.a1a[i] : 0.f;
  }
  if (i < p.H1p) p.al1P[i] = i < p.H1 ? p.a0a[i] : 0.f;
}

// one wave per row: rows [0, BT) = E[seq], rows [BT, BT + N) = E[cand]; live = an id in 1 .. n_items
__global__ __launch_bounds__(kBlock) void din_gather_kernel(const float* __restrict__ E, int64_t n_items, int D,
                                                            const int64_t* __restrict__ seq,
                                                            const int64_t* __restrict__ cand, int64_t BT, int64_t N,
                                                            float* __restrict__ rows, float* __restrict__ q,
                                                            uint8_t* __restrict__ lv, uint8_t* __restrict__ lc,
                                                            hiprec_stats* stats) {
  const int lane = lane_id();
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); w < BT + N;
       w += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const bool is_seq = w < BT;
    const int64_t m = is_seq ? w : w - BT, id = is_seq ? seq[m] : cand[m];
    const bool ok = id >= 1 && id <= n_items;
    if (lane == 0) {
      if (id < 0 || id > n_items) atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
      (is_seq ? lv : lc)[m] = ok;
    }
    float* out = (is_seq ? rows : q) + m * D;
    for (int d = lane; d < D; d += kWave) out[d] = ok ? E[id * D + d] : 0.f;
  }
}

__global__ __launch_bounds__(kBlock) void din_fill_kernel(float* p, int64_t n, float v) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * kBlock)
    p[i] = v;
}
__global__ __launch_bounds__(kBlock) void din_add_kernel(float* dst, const float* src, int64_t n) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * kBlock)
    dst[i] += src[i];
}
__global__ __launch_bounds__(kBlock) void din_flags_kernel(const uint8_t* mask, uint8_t* lv, int64_t BT, uint8_t* lc, int64_t N) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < BT + N; i += static_cast<int64_t>(gridDim.x) * kBlock) {
    if (i < BT) lv[i] = mask[i] != 0;
    else lc[i - BT] = 1;
  }
}

// z = [pooled, q, pooled * q]
__global__ __launch_bounds__(kBlock) void din_z_kernel(const float* __restrict__ pooled, const float* __restrict__ q,
                                                       int64_t N, int D, float* __restrict__ z) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < N * D; i += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t n = i / D;
    const int d = static_cast<int>(i - n * D);
    const float p = pooled[i], qq = q[i];
    float* row = z + n * 3 * D;
    row[d] = p;
    row[D + d] = qq;
    row[2 * D + d] = p * qq;
  }
}
// d pooled = dz[:, :D] + dz[:, 2D:] * q, d q = dz[:, D:2D] + dz[:, 2D:] * pooled
__global__ __launch_bounds__(kBlock) void din_z_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ pooled,
                                                           const float* __restrict__ q, int64_t N, int D,
                                                           float* __restrict__ dpooled, float* __restrict__ dq) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < N * D; i += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t n = i / D;
    const int d = static_cast<int>(i - n * D);
    const float* row = dz + n * 3 * D;
    dpooled[i] = fmaf(row[2 * D + d], q[i], row[d]);
    dq[i] = fmaf(row[2 * D + d], pooled[i], row[D + d]);
  }
}

// The slabs' sums in slab order and the unfolding of d (Wq + Wd), d (We - Wd) into d att.0.weight = [dq' | de' | dq' - de' | d Wp]
struct DinUnfold {
  const float *slabs, *gWfe, *gWfq;
  float *a0w, *a0a, *a1w, *a1b, *a1a, *a2w, *a2b;
  int n_slabs, D, H1, H2, n_e, n_q;      // n_e / n_q: K-slices of d (We - Wd) / d (Wq + Wd), each [H1, D]
};
__global__ __launch_bounds__(kBlock) void din_unfold_kernel(DinUnfold p) {
  const DinSlab o = din_slab(p.D, p.H1, p.H2);
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i < static_cast<int64_t>(p.H1) * p.D) {
    const int64_t j = i / p.D, d = i - j * p.D;
    float* row = p.a0w + j * 4 * p.D;
    const int64_t hd = static_cast<int64_t>(p.H1) * p.D;
    const float gq = din_slab_sum(p.gWfq, p.n_q, hd, i), ge = din_slab_sum(p.gWfe, p.n_e, hd, i);
    row[d] = gq;
    row[p.D + d] = ge;
    row[2 * p.D + d] = gq - ge;
    row[3 * p.D + d] = din_slab_sum(p.slabs, p.n_slabs, o.floats, o.wp + i);
  }
  if (i < static_cast<int64_t>(p.H2) * p.H1) p.a1w[i] = din_slab_sum(p.slabs, p.n_slabs, o.floats, o.w1 + i);
  if (i < p.H2) {
    p.a1b[i] = din_slab_sum(p.slabs, p.n_slabs, o.floats, o.b1 + i);
    p.a1a[i] = din_slab_sum(p.slabs, p.n_slabs, o.floats, o.al2 + i);
    p.a2w[i] = din_slab_sum(p.slabs, p.n_slabs, o.floats, o.w2 + i);
  }
  if (i < p.H1) p.a0a[i] = din_slab_sum(p.slabs, p.n_slabs, o.floats, o.al1 + i);
  if (i == 0) p.a2b[0] = din_slab_sum(p.slabs, p.n_slabs, o.floats, o.b2);
}

// one wave per row: d E[seq] rows (from d U) and d E[cand] rows (from d V and d q) into g_item as row atomics
__global__ __launch_bounds__(kBlock) void din_scatter_kernel(const float* __restrict__ drows, const float* __restrict__ dqv,
                                                             const float* __restrict__ dq, const int64_t* __restrict__ seq,
                                                             const int64_t* __restrict__ cand,
                                                             const uint8_t* __restrict__ lv, const uint8_t* __restrict__ lc,
                                                             int64_t BT, int64_t N, int D, float* __restrict__ g_item) {
  const int lane = lane_id();
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); w < BT + N;
       w += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const bool is_seq = w < BT;
    const int64_t m = is_seq ? w : w - BT;
    if (!(is_seq ? lv[m] : lc[m])) continue;
    const int64_t id = is_seq ? seq[m] : cand[m];
    for (int d = lane; d < D; d += kWave) {
      const float v = is_seq ? drows[m * D + d] : dqv[m * D + d] + dq[m * D + d];
      if (v != 0.f) atomic_add_f32(g_item + id * D + d, v);
    }
  }
}

// ---- the tower's column kernels ----------------------------------------------------------------------------------------------
// A block owns kColW columns; its kColG row groups each sum every kColG-th row, the groups' partials are added in order.
__device__ __forceinline__ float din_live_count(const uint8_t* live, int64_t N) {
  __shared__ float s_cnt[kWavesPerBlock];
  float cnt = 0.f;      // exact: N <= 2^24
  for (int64_t i = threadIdx.x; i < N; i += kBlock) cnt += live[i] ? 1.f : 0.f;
  cnt = wave_sum(cnt);
  if (lane_id() == 0) s_cnt[wave_in_block()] = cnt;
  __syncthreads();
  return (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}
__device__ __forceinline__ float din_group_sum(float (*red)[kColW + 1], float v) {
  const int c = threadIdx.x & (kColW - 1), g = threadIdx.x / kColW;
  __syncthreads();
  red[g][c] = v;
  __syncthreads();
  float t = 0.f;
  for (int k = 0; k < kColG; ++k) t += red[k][c];
  return t;
}

// Dice's batch statistics over the live rows: mean and the biased variance of every column, the running buffers updated
// BatchNorm1d's way (momentum 0.1, the unbiased variance) when `running` is given.  One live row has no variance: status.
__global__ __launch_bounds__(kBlock) void din_bn_stats_kernel(const float* __restrict__ x, const uint8_t* __restrict__ live,
                                                              int64_t N, int W, float* __restrict__ mean,
                                                              float* __restrict__ var, float* running, hiprec_stats* stats) {
  __shared__ float red[kColG][kColW + 1];
  const int c = threadIdx.x & (kColW - 1), g = threadIdx.x / kColW, col = blockIdx.x * kColW + c;
  const float n = din_live_count(live, N);
  const bool ok = col < W;
  float sum = 0.f;
  if (ok) {
    for (int64_t r0 = g; r0 < N; r0 += kColG * kColFly) {      // kColFly independent loads, then added in row order
      float v[kColFly];
#pragma unroll
      for (int i = 0; i < kColFly; ++i) {
        const int64_t r = r0 + i * kColG;
        v[i] = (r < N && live[r]) ? x[r * W + col] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < kColFly; ++i) sum += v[i];
    }
  }
  const float t_sum = din_group_sum(red, sum), mu = n > 0.f ? t_sum / n : 0.f;
  float sq = 0.f;
  if (ok) {
    for (int64_t r0 = g; r0 < N; r0 += kColG * kColFly) {
      float v[kColFly];
#pragma unroll
      for (int i = 0; i < kColFly; ++i) {
        const int64_t r = r0 + i * kColG;
        v[i] = (r < N && live[r]) ? x[r * W + col] - mu : 0.f;
      }
#pragma unroll
      for (int i = 0; i < kColFly; ++i) sq = fmaf(v[i], v[i], sq);
    }
  }
  const float t_sq = din_group_sum(red, sq), vr = n > 0.f ? t_sq / n : 0.f;
  if (g == 0 && ok) {
    mean[col] = mu;
    var[col] = vr;
    if (running && n > 1.f) {
      running[col] = (1.f - kDiceMomentum) * running[col] + kDiceMomentum * mu;
      running[W + col] = (1.f - kDiceMomentum) * running[W + col] + kDiceMomentum * (vr * n / (n - 1.f));
    }
  }
  if (n == 1.f && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&stats->status, HIPREC_STATUS_BATCH_STATS);
}

// y = x (alpha + p (1 - alpha)), p = sigmoid((x - mean) / sqrt(var + eps)) (kind 0, Dice); y = prelu(x) (kind 1)
__global__ __launch_bounds__(kBlock) void din_act_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                             const float* __restrict__ var, const float* __restrict__ alpha,
                                                             int64_t N, int W, int kind, float* __restrict__ y) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < N * W; i += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int col = static_cast<int>(i % W);
    const float xv = x[i], al = alpha[col];
    if (kind) {
      y[i] = xv > 0.f ? xv : al * xv;
    } else {
      const float p = sigmoid_f32((xv - mean[col]) / sqrtf(var[col] + kDiceEps));
      y[i] = xv * fmaf(p, 1.f - al, al);
    }
  }
}

// The backward column sums over the live rows: d alpha (stored into g_alpha) and, for Dice, S1 = sum gh, S2 = sum gh xhat
// with gh = dy x (1 - alpha) p (1 - p) the gradient that reaches xhat.  sums [2, W].
__global__ __launch_bounds__(kBlock) void din_act_bwd_stats_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                   const float* __restrict__ mean,
                                                                   const float* __restrict__ var,
                                                                   const float* __restrict__ alpha,
                                                                   const uint8_t* __restrict__ live, int64_t N, int W,
                                                                   int kind, float* __restrict__ sums,
                                                                   float* __restrict__ g_alpha) {
  __shared__ float red[kColG][kColW + 1];
  const int c = threadIdx.x & (kColW - 1), g = threadIdx.x / kColW, col = blockIdx.x * kColW + c;
  const bool ok = col < W;
  float s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (ok) {
    const float al = alpha[col], mu = kind ? 0.f : mean[col], rstd = kind ? 0.f : 1.f / sqrtf(var[col] + kDiceEps);
    for (int64_t r0 = g; r0 < N; r0 += kColG * kColFly) {
      float xs[kColFly], ds[kColFly];
#pragma unroll
      for (int i = 0; i < kColFly; ++i) {      // dead rows count as d y = 0: every term below is then 0
        const int64_t r = r0 + i * kColG;
        const bool on = r < N && live[r];
        xs[i] = on ? x[r * W + col] : 0.f;
        ds[i] = on ? dy[r * W + col] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < kColFly; ++i) {
      const float xv = xs[i], d = ds[i];
      if (kind) {
        s3 = fmaf(d, fminf(xv, 0.f), s3);
      } else {
        const float xh = (xv - mu) * rstd, p = sigmoid_f32(xh), gh = d * xv * (1.f - al) * p * (1.f - p);
        s1 += gh;
        s2 = fmaf(gh, xh, s2);
        s3 = fmaf(d * (1.f - p), xv, s3);
      }
      }
    }
  }
  const float t3 = din_group_sum(red, s3);
  if (g == 0 && ok) g_alpha[col] = t3;
  if (kind) return;
  const float t1 = din_group_sum(red, s1), t2 = din_group_sum(red, s2);
  if (g == 0 && ok) {
    sums[col] = t1;
    sums[W + col] = t2;
  }
}

// d x over d y in place; dead rows get 0
__global__ __launch_bounds__(kBlock) void din_act_bwd_kernel(const float* __restrict__ x, float* __restrict__ dy,
                                                             const float* __restrict__ mean, const float* __restrict__ var,
                                                             const float* __restrict__ alpha,
                                                             const uint8_t* __restrict__ live, const float* __restrict__ sums,
                                                             int64_t N, int W, int kind) {
  const float n = kind ? 1.f : din_live_count(live, N), inv_n = n > 0.f ? 1.f / n : 0.f;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < N * W; i += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t r = i / W;
    const int col = static_cast<int>(i - r * W);
    float out = 0.f;
    if (live[r]) {
      const float xv = x[i], d = dy[i], al = alpha[col];
      if (kind) {
        out = xv > 0.f ? d : al * d;
      } else {
        const float rstd = 1.f / sqrtf(var[col] + kDiceEps), xh = (xv - mean[col]) * rstd, p = sigmoid_f32(xh);
        const float gh = d * xv * (1.f - al) * p * (1.f - p);
        out = fmaf(d, fmaf(p, 1.f - al, al), rstd * (gh - inv_n * (sums[col] + xh * sums[W + col])));
      }
    }
    dy[i] = out;
  }
}

// BCE-with-logits over the live candidates, one lane per row: the loss partial, d logit = (sigmoid(z) - y) / n; a dead
// slot's logit is set to 0.
__global__ __launch_bounds__(kBlock) void din_bce_kernel(float* __restrict__ logit, const float* __restrict__ label,
                                                         const uint8_t* __restrict__ live, int64_t N,
                                                         float* __restrict__ dlogit, Scratch* scratch, hiprec_stats* stats) {
  const float n = din_live_count(live, N), inv = n > 0.f ? 1.f / n : 0.f;
  float loss = 0.f;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < N; i += static_cast<int64_t>(gridDim.x) * kBlock) {
    float d = 0.f;
    if (live[i]) {
      const float z = logit[i], y = label[i];
      float sig_neg;
      const float nls = neg_logsigmoid(z, &sig_neg);      // -log sigmoid(z), sigmoid(-z)
      loss += nls + (1.f - y) * z;
      d = ((1.f - sig_neg) - y) * inv;
    } else {
      logit[i] = 0.f;
    }
    dlogit[i] = d;
  }
  publish_partials<kWavesPerBlock>(wave_sum(loss), 0.f, 0.f, inv, scratch);
  if (blockIdx.x == 0 && threadIdx.x == 0) advance_step(stats);
}

__global__ __launch_bounds__(kBlock) void din_mask_logits_kernel(float* __restrict__ logit, const uint8_t* __restrict__ live,
                                                                 int64_t N) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < N; i += static_cast<int64_t>(gridDim.x) * kBlock)
    if (!live[i]) logit[i] = 0.f;
}

}  // namespace

// ---- what csrc/dien.hip shares (din.hpp) ----------------------------------------------------------------------------------
int din_gather(const float* E, int64_t n_items, int D, const int64_t* seq, const int64_t* cand, int64_t BT, int64_t N,
               float* rows, float* q, uint8_t* lv, uint8_t* lc, hiprec_stats* stats, hipStream_t st) {
  din_gather_kernel<<<grid_for_waves(BT + N), kBlock, 0, st>>>(E, n_items, D, seq, cand, BT, N, rows, q, lv, lc, stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}
int din_flags(const uint8_t* mask, uint8_t* lv, int64_t BT, uint8_t* lc, int64_t N, hipStream_t st) {
  din_flags_kernel<<<grid_for_threads(BT + N), kBlock, 0, st>>>(mask, lv, BT, lc, N);
  HIPREC_TRY(hipGetLastError());
  return 0;
}
int din_scatter(const float* drows, const float* dqa, const float* dqb, const int64_t* seq, const int64_t* cand,
                const uint8_t* lv, const uint8_t* lc, int64_t BT, int64_t N, int D, float* g_item, hipStream_t st) {
  din_scatter_kernel<<<grid_for_waves(BT + N), kBlock, 0, st>>>(drows, dqa, dqb, seq, cand, lv, lc, BT, N, D, g_item);
  HIPREC_TRY(hipGetLastError());
  return 0;
}
int din_fill(float* p, int64_t n, float v, hipStream_t st) {
  din_fill_kernel<<<grid_for_threads(n), kBlock, 0, st>>>(p, n, v);
  HIPREC_TRY(hipGetLastError());
  return 0;
}
int din_add(float* dst, const float* src, int64_t n, hipStream_t st) {
  din_add_kernel<<<grid_for_threads(n), kBlock, 0, st>>>(dst, src, n);
  HIPREC_TRY(hipGetLastError());
  return 0;
}
int din_z(const float* v, const float* q, int64_t N, int D, float* z, hipStream_t st) {
  din_z_kernel<<<grid_for_threads(N * D), kBlock, 0, st>>>(v, q, N, D, z);
  HIPREC_TRY(hipGetLastError());
  return 0;
}
int din_z_bwd(const float* dz, const float* v, const float* q, int64_t N, int D, float* dv, float* dq, hipStream_t st) {
  din_z_bwd_kernel<<<grid_for_threads(N * D), kBlock, 0, st>>>(dz, v, q, N, D, dv, dq);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

int din_tower_forward(const DinTower& t, const float* w_flat, float* bn, int update_running, bool train, const float* z,
                      const uint8_t* lc, int64_t N, float* logits_out, hiprec_stats* stats, hipStream_t st) {
  const int Ni = static_cast<int>(N);
  const float* in = z;
  int moff = 0;
  for (int l = 0; l < t.L; ++l) {
    const int W = t.W[l];
    GemmGroup g{};
    g.n = 1;
    g.p[0] = make_gemm(kNT, Ni, W, t.in[l], in, t.in[l], w_flat + t.dw[l], t.in[l], t.x[l], W, w_flat + t.db[l], 0, nullptr, 0,
                       false);
    if (int rc = launch_group(g, st)) return rc;
    const float *mean = t.mean + moff, *var = t.var + moff;
    if (t.act == 0) {
      if (train) {
        din_bn_stats_kernel<<<(W + kColW - 1) / kColW, kBlock, 0, st>>>(t.x[l], lc, N, W, t.mean + moff, t.var + moff,
                                                                        update_running ? bn + t.bn[l] : nullptr, stats);
        HIPREC_TRY(hipGetLastError());
      } else {
        mean = bn + t.bn[l];
        var = bn + t.bn[l] + W;
      }
    }
    din_act_fwd_kernel<<<grid_for_threads(N * W), kBlock, 0, st>>>(t.x[l], mean, var, w_flat + t.da[l], N, W, t.act, t.y[l]);
    HIPREC_TRY(hipGetLastError());
    in = t.y[l];
    moff += W;
  }
  const int WL = t.W[t.L - 1];
  float* logit = train ? t.logit : logits_out;
  GemmGroup g{};
  g.n = 1;
  g.p[0] = make_gemm(kNT, Ni, 1, WL, in, WL, w_flat + t.ow, WL, logit, 1, w_flat + t.ob, 0, nullptr, 0, false);
  if (int rc = launch_group(g, st)) return rc;
  if (!train) {
    din_mask_logits_kernel<<<grid_for_threads(N), kBlock, 0, st>>>(logit, lc, N);
    HIPREC_TRY(hipGetLastError());
  }
  return 0;
}

int din_tower_backward(const DinTower& t, const float* w_flat, float* g_flat, const float* z, const uint8_t* lc,
                       const float* label, int64_t N, float* logits_out, Scratch* scratch, hiprec_stats* stats,
                       hipStream_t st, float** dz) {
  const int Ni = static_cast<int>(N), WL = t.W[t.L - 1];
  const float* in = t.y[t.L - 1];
  int moff = 0;
  for (int l = 0; l < t.L; ++l) moff += t.W[l];
  din_bce_kernel<<<grid_for_threads(N), kBlock, 0, st>>>(t.logit, label, lc, N, t.dlogit, scratch, stats);
  HIPREC_TRY(hipGetLastError());
  if (logits_out) HIPREC_TRY(hipMemcpyAsync(logits_out, t.logit, sizeof(float) * N, hipMemcpyDeviceToDevice, st));
  // the output layer: d y_L = d logit out.weight, d out.weight = d logit^T y_L, d out.bias = sum d logit
  float *dcur = t.dA, *dnext = t.dB;
  {
    GemmGroup g{};
    g.n = 3;
    g.p[0] = make_gemm(kNN, Ni, WL, 1, t.dlogit, 1, w_flat + t.ow, WL, dcur, WL, nullptr, 0, nullptr, 0, false);
    g.p[1] = make_gemm(kTNm, 1, WL, Ni, t.dlogit, 1, in, WL, g_flat + t.ow, WL, nullptr, 0, nullptr, 0, false);
    g.p[2] = make_colsum(t.dlogit, Ni, 1, 1, g_flat + t.ob, t.cs);
    if (int rc = launch_group(g, st)) return rc;
    if (int rc = launch_colsum_reduce(g, st)) return rc;
  }
  for (int l = t.L - 1; l >= 0; --l) {
    const int W = t.W[l], K = t.in[l];
    moff -= W;
    const float* lin = l ? t.y[l - 1] : z;
    din_act_bwd_stats_kernel<<<(W + kColW - 1) / kColW, kBlock, 0, st>>>(t.x[l], dcur, t.mean + moff, t.var + moff,
                                                                         w_flat + t.da[l], lc, N, W, t.act, t.sums,
                                                                         g_flat + t.da[l]);
    HIPREC_TRY(hipGetLastError());
    din_act_bwd_kernel<<<grid_for_threads(N * W), kBlock, 0, st>>>(t.x[l], dcur, t.mean + moff, t.var + moff, w_flat + t.da[l],
                                                                   lc, t.sums, N, W, t.act);
    HIPREC_TRY(hipGetLastError());
    GemmGroup g{};
    g.n = 3;
    g.p[0] = make_gemm(kNN, Ni, K, W, dcur, W, w_flat + t.dw[l], K, dnext, K, nullptr, 0, nullptr, 0, false);
    g.p[1] = make_gemm(kTNm, W, K, Ni, dcur, W, lin, K, g_flat + t.dw[l], K, nullptr, 0, nullptr, 0, false);
    g.p[2] = make_colsum(dcur, Ni, W, W, g_flat + t.db[l], t.cs);
    if (int rc = launch_group(g, st)) return rc;
    if (int rc = launch_colsum_reduce(g, st)) return rc;
    std::swap(dcur, dnext);
  }
  *dz = dcur;
  return 0;
}

int din_add_wgrad_slices(GemmGroup& g, int want, int M, int N, int K, const float* A, int lda, const float* Bm, int ldb,
                         float* parts) {
  const int n = std::max(1, std::min(want, K / kDinSplitRows));
  const int len = ((K + n - 1) / n + 3) / 4 * 4;
  for (int i = 0; i < n; ++i) {
    const int k0 = i * len, kn = std::min(len, K - k0);
    g.p[g.n++] = make_gemm(kTNm, M, N, kn, A + static_cast<int64_t>(k0) * lda, lda, Bm + static_cast<int64_t>(k0) * ldb, ldb,
                           parts + static_cast<int64_t>(i) * M * N, N, nullptr, 0, nullptr, 0, false);
  }
  return n;
}

namespace {

// ---- host side ----------------------------------------------------------------------------------------------------------
int din_check_shape(const hiprec_din_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  HIPREC_REQUIRE(s->n_items >= 1 && s->n_items < (1ll << 31), "DIN needs 1 <= n_items < 2^31, got %lld",
                 static_cast<long long>(s->n_items));
  HIPREC_REQUIRE(s->dim >= 16 && s->dim <= kDinMaxDim && s->dim % 16 == 0,
                 "DIN needs emb_dim a multiple of 16 in 16 .. %d (got %d)", kDinMaxDim, s->dim);
  HIPREC_REQUIRE(s->maxlen >= 1 && s->maxlen <= kDinMaxLen, "DIN needs 1 <= maxlen <= %d (got %d)", kDinMaxLen, s->maxlen);
  HIPREC_REQUIRE(s->att_h1 >= 1 && s->att_h1 <= kDinMaxAtt && s->att_h2 >= 1 && s->att_h2 <= kDinMaxAtt,
                 "DIN needs two att_hidden widths in 1 .. %d (got %d, %d)", kDinMaxAtt, s->att_h1, s->att_h2);
  HIPREC_REQUIRE(s->n_dnn >= 1 && s->n_dnn <= kDinMaxLayers, "DIN needs 1 .. %d dnn_hidden widths (got %d)", kDinMaxLayers,
                 s->n_dnn);
  for (int l = 0; l < s->n_dnn; ++l)
    HIPREC_REQUIRE(s->dnn[l] >= 1 && s->dnn[l] <= kDinMaxDnn, "DIN needs dnn_hidden widths in 1 .. %d (got %d)", kDinMaxDnn,
                   s->dnn[l]);
  HIPREC_REQUIRE((s->att_act == 0 || s->att_act == 1) && (s->dnn_act == 0 || s->dnn_act == 1),
                 "DIN: att_activation is sigmoid (0) or prelu (1), dnn_activation dice (0) or prelu (1)");
  return 0;
}

DinDims din_dims(const hiprec_din_shape& s) {
  DinDims q{};
  q.n_items = s.n_items; q.D = s.dim; q.T = s.maxlen; q.H1 = s.att_h1; q.H2 = s.att_h2;
  q.att_act = s.att_act; q.dnn_act = s.dnn_act; q.L = s.n_dnn;
  for (int l = 0; l < q.L; ++l) q.W[l] = s.dnn[l];
  q.H1p = (q.H1 + 15) / 16 * 16;
  q.H2p = (q.H2 + 15) / 16 * 16;
  return q;
}

// the chunk and what is resident in LDS: the largest chunk of 64 / 32 / 16 positions (no longer than the sequence) beside
// which the buffers fit, then Wp, then att.1.weight while there is room
size_t din_plan_lds(const DinDims& q, bool bwd, DinUnit* u) {
  u->T = q.T; u->D = q.D; u->H1 = q.H1; u->H2 = q.H2; u->H1p = q.H1p; u->H2p = q.H2p; u->act = q.att_act;
  u->ldE = q.D + 4; u->ldH = std::max(q.H1p, q.D) + 4; u->ldG = q.H2p + 4; u->ldWp = q.D + 4; u->ldW1 = q.H1p + 4;
  u->scale = 1.0f / sqrtf(static_cast<float>(q.D));
  const size_t fixed = 3 * q.H2p + q.H1p + 2 * q.D + 3 * kDinMaxChunk + kWavesPerBlock * kDinColTiles * 16;
  const size_t budget = kDinLdsBudget / sizeof(float);
  size_t use = 0;
  for (int R = kDinMaxChunk; R >= kDinTile; R /= 2) {
    u->R = R;
    use = fixed + static_cast<size_t>(R) * (u->ldE + u->ldH) * (bwd ? 2 : 1) + (bwd ? static_cast<size_t>(R) * u->ldG : 0);
    if (use <= budget && (R == kDinTile || R / 2 < q.T)) break;
  }
  const size_t wp = static_cast<size_t>(q.H1p) * u->ldWp, w1 = static_cast<size_t>(q.H2p) * u->ldW1;
  u->wp_lds = use + wp <= budget;
  if (u->wp_lds) use += wp;
  u->w1_lds = use + w1 <= budget;
  if (u->w1_lds) use += w1;
  return use * sizeof(float);
}

struct DinWs {
  float *Wfe, *Wfq, *WpP, *W1P, *w2P, *b1P, *al1P, *al2P;
  float *rows, *q, *U, *V, *a, *pooled, *z, *x[kDinMaxLayers], *y[kDinMaxLayers], *mean, *var, *logit;
  float *dlogit, *dA, *dB, *sums, *dpooled, *dq, *dU, *dV, *drows, *dqv, *gWfe, *gWfq, *slabs, *cs;
  uint8_t *lv, *lc;
  int64_t zero_floats;      // dU and dV: cleared in one launch
  int64_t floats;
};

DinWs din_carve_ws(float* base, const DinDims& q, int64_t B, int64_t C, bool train) {
  DinWs w{};
  float* p = base;
  auto take = [&](int64_t n) { float* r = p; p += (n + 3) / 4 * 4; return r; };
  const int64_t BT = B * q.T, N = B * C;
  const int ldWp = q.D + 4, ldW1 = q.H1p + 4;
  w.Wfe = take(static_cast<int64_t>(q.H1) * q.D); w.Wfq = take(static_cast<int64_t>(q.H1) * q.D);
  w.WpP = take(static_cast<int64_t>(q.H1p) * ldWp); w.W1P = take(static_cast<int64_t>(q.H2p) * ldW1);
  w.w2P = take(q.H2p); w.b1P = take(q.H2p); w.al2P = take(q.H2p); w.al1P = take(q.H1p);
  w.rows = take(BT * q.D); w.q = take(N * q.D);
  w.lv = reinterpret_cast<uint8_t*>(take((BT + 3) / 4)); w.lc = reinterpret_cast<uint8_t*>(take((N + 3) / 4));
  w.U = take(BT * q.H1); w.V = take(N * q.H1); w.a = take(N * q.T); w.pooled = take(N * q.D);
  w.z = take(N * 3 * q.D);
  int wide = 3 * q.D, sumw = 0;
  for (int l = 0; l < q.L; ++l) {
    w.x[l] = take(N * q.W[l]); w.y[l] = take(N * q.W[l]);
    wide = std::max(wide, q.W[l]);
    sumw += q.W[l];
  }
  w.mean = take(sumw); w.var = take(sumw);
  w.logit = take(N);
  if (train) {
    w.dlogit = take(N);
    w.dA = take(N * wide); w.dB = take(N * wide); w.sums = take(2 * wide);
    w.dpooled = take(N * q.D); w.dq = take(N * q.D);
    w.dU = take(BT * q.H1); w.dV = take(N * q.H1);
    w.zero_floats = (w.dV - w.dU) + (N * q.H1 + 3) / 4 * 4;
    w.drows = take(BT * q.D); w.dqv = take(N * q.D);
    w.gWfe = take(static_cast<int64_t>(kDinSplitE) * q.H1 * q.D); w.gWfq = take(static_cast<int64_t>(kDinSplitQ) * q.H1 * q.D);
    w.slabs = take(kDinSlabs * din_slab(q.D, q.H1, q.H2).floats);
    w.cs = take(2 * colsum_ws_floats(static_cast<int>(std::max(BT, N)), std::max(wide, q.H1)));
  }
  w.floats = p - base;
  return w;
}

bool din_batch_ok(const DinDims& q, int64_t B, int64_t C) {
  return B >= 1 && C >= 1 && B * q.T <= kDinMaxRows && B * C <= kDinMaxRows && B * ((C + kDinSlice - 1) / kDinSlice) < (1ll << 31);
}

std::atomic<uint64_t> din_lds_ok{0};

int din_allow_lds() {
  return allow_dynamic_lds({reinterpret_cast<const void*>(&din_unit_fwd_kernel), reinterpret_cast<const void*>(&din_unit_bwd_kernel)},
                           kDinLdsBudget, din_lds_ok, "the DIN activation unit");
}

int din_prep(const DinDims& q, const DinOff& o, const float* w_flat, const DinWs& a, hipStream_t st) {
  DinPrep p{w_flat + o.a0w, w_flat + o.a0a, w_flat + o.a1w, w_flat + o.a1b, w_flat + o.a1a, w_flat + o.a2w,
            a.Wfe, a.Wfq, a.WpP, a.W1P, a.w2P, a.b1P, a.al1P, a.al2P, q.D, q.H1, q.H2, q.H1p, q.H2p};
  const int n = std::max(q.H1p * (q.D + 4), q.H2p * (q.H1p + 4));
  din_prep_kernel<<<(n + kBlock - 1) / kBlock, kBlock, 0, st>>>(p);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// U, V in one grouped launch, then the fused unit: pooled [N, D], a [N, T]
int din_unit_forward(const DinDims& q, const DinOff& o, const float* w_flat, const DinWs& a, int64_t B, int64_t C,
                     float* pooled, float* att, hipStream_t st) {
  const int BT = static_cast<int>(B * q.T), N = static_cast<int>(B * C);
  GemmGroup g{};
  g.n = 2;
  g.p[0] = make_gemm(kNT, BT, q.H1, q.D, a.rows, q.D, a.Wfe, q.D, a.U, q.H1, w_flat + o.a0b, 0, nullptr, 0, false);
  g.p[1] = make_gemm(kNT, N, q.H1, q.D, a.q, q.D, a.Wfq, q.D, a.V, q.H1, nullptr, 0, nullptr, 0, false);
  if (int rc = launch_group(g, st)) return rc;
  DinUnit u{};
  const size_t lds = din_plan_lds(q, false, &u);
  if (int rc = din_allow_lds()) return rc;
  u.C = static_cast<int>(C);
  u.WpP = a.WpP; u.W1P = a.W1P; u.w2P = a.w2P; u.b1P = a.b1P; u.al1P = a.al1P; u.al2P = a.al2P; u.b2 = w_flat + o.a2b;
  u.rows = a.rows; u.q = a.q; u.U = a.U; u.V = a.V; u.lv = a.lv; u.lc = a.lc;
  const int64_t grid = B * ((C + kDinSlice - 1) / kDinSlice);
  din_unit_fwd_kernel<<<static_cast<int>(grid), kBlock, lds, st>>>(u, pooled, att);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// After the fused backward: d (We - Wd), d (Wq + Wd), d att.0.bias and the rows d U (We - Wd), d V (Wq + Wd) in one grouped
// launch, then the fold of the slabs and slices into the unit's gradients, which start at g_att (att.0.weight)
int din_unit_finish(const DinDims& q, const DinOff& o, const DinWs& a, int64_t BT, int64_t N, int n_slabs, float* g_att,
                    float* drows, float* dqv, hipStream_t st) {
  const int BTi = static_cast<int>(BT), Ni = static_cast<int>(N), D = q.D;
  GemmGroup g{};
  const int n_e = din_add_wgrad_slices(g, kDinSplitE, q.H1, D, BTi, a.dU, q.H1, a.rows, D, a.gWfe);
  const int n_q = din_add_wgrad_slices(g, kDinSplitQ, q.H1, D, Ni, a.dV, q.H1, a.q, D, a.gWfq);
  g.p[g.n++] = make_gemm(kNN, BTi, D, q.H1, a.dU, q.H1, a.Wfe, D, drows, D, nullptr, 0, nullptr, 0, false);
  g.p[g.n++] = make_gemm(kNN, Ni, D, q.H1, a.dV, q.H1, a.Wfq, D, dqv, D, nullptr, 0, nullptr, 0, false);
  g.p[g.n++] = make_colsum(a.dU, BTi, q.H1, q.H1, g_att + (o.a0b - o.a0w), a.cs);
  static_assert(kDinSplitE + kDinSplitQ + 3 <= kMaxGroup, "one grouped launch");
  if (int rc = launch_group(g, st)) return rc;
  if (int rc = launch_colsum_reduce(g, st)) return rc;
  DinUnfold f{a.slabs, a.gWfe, a.gWfq, g_att, g_att + (o.a0a - o.a0w), g_att + (o.a1w - o.a0w), g_att + (o.a1b - o.a0w),
              g_att + (o.a1a - o.a0w), g_att + (o.a2w - o.a0w), g_att + (o.a2b - o.a0w), n_slabs, D, q.H1, q.H2, n_e, n_q};
  const int nf = std::max(q.H1 * D, q.H2 * q.H1);
  din_unfold_kernel<<<(nf + kBlock - 1) / kBlock, kBlock, 0, st>>>(f);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

DinTower din_tower_of(const DinDims& q, const DinOff& o, const DinWs& a) {
  DinTower t{};
  t.L = q.L; t.act = q.dnn_act; t.ow = o.ow; t.ob = o.ob;
  for (int l = 0; l < q.L; ++l) {
    t.W[l] = q.W[l]; t.in[l] = o.in[l]; t.bn[l] = o.bn[l]; t.dw[l] = o.dw[l]; t.db[l] = o.db[l]; t.da[l] = o.da[l];
    t.x[l] = a.x[l]; t.y[l] = a.y[l];
  }
  t.mean = a.mean; t.var = a.var; t.logit = a.logit; t.dlogit = a.dlogit; t.dA = a.dA; t.dB = a.dB; t.sums = a.sums; t.cs = a.cs;
  return t;
}

int din_run(const DinDims& q, const float* w_flat, float* g_flat, float* bn, int update_running, const int64_t* seq,
            const int64_t* cand, const float* label, int64_t B, int64_t C, float* logits_out, hiprec_stats* stats,
            Scratch* scratch, float* ws_base, hipStream_t st) {
  const bool train = g_flat != nullptr;
  const DinOff o = din_offsets(q);
  const DinWs a = din_carve_ws(ws_base, q, B, C, train);
  const int64_t BT = B * q.T, N = B * C;
  const int D = q.D;
  if (int rc = din_prep(q, o, w_flat, a, st)) return rc;
  if (int rc = din_gather(w_flat, q.n_items, D, seq, cand, BT, N, a.rows, a.q, a.lv, a.lc, stats, st)) return rc;
  if (int rc = din_unit_forward(q, o, w_flat, a, B, C, a.pooled, a.a, st)) return rc;
  if (int rc = din_z(a.pooled, a.q, N, D, a.z, st)) return rc;

  const DinTower tw = din_tower_of(q, o, a);
  if (int rc = din_tower_forward(tw, w_flat, bn, update_running, train, a.z, a.lc, N, logits_out, stats, st)) return rc;
  if (!train) return 0;
  float* dcur = nullptr;
  if (int rc = din_tower_backward(tw, w_flat, g_flat, a.z, a.lc, label, N, logits_out, scratch, stats, st, &dcur)) return rc;
  if (int rc = din_z_bwd(dcur, a.pooled, a.q, N, D, a.dpooled, a.dq, st)) return rc;
  if (int rc = din_fill(a.dU, a.zero_floats, 0.f, st)) return rc;

  DinUnit u{};
  const size_t lds = din_plan_lds(q, true, &u);
  u.C = static_cast<int>(C);
  u.WpP = a.WpP; u.W1P = a.W1P; u.w2P = a.w2P; u.b1P = a.b1P; u.al1P = a.al1P; u.al2P = a.al2P; u.b2 = w_flat + o.a2b;
  u.rows = a.rows; u.q = a.q; u.U = a.U; u.V = a.V; u.lv = a.lv; u.lc = a.lc;
  const int n_slabs = static_cast<int>(std::min<int64_t>(B, kDinSlabs));
  din_unit_bwd_kernel<<<n_slabs, kBlock, lds, st>>>(u, B, a.a, a.dpooled, seq, a.dU, a.dV, a.dq, g_flat, nullptr, a.slabs);
  HIPREC_TRY(hipGetLastError());
  if (int rc = din_unit_finish(q, o, a, BT, N, n_slabs, g_flat + o.a0w, a.drows, a.dqv, st)) return rc;
  return din_scatter(a.drows, a.dqv, a.dq, seq, cand, a.lv, a.lc, BT, N, D, g_flat, st);
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_din_shape_bytes(void) { return sizeof(hiprec_din_shape); }

extern "C" int64_t hiprec_din_param_floats(const hiprec_din_shape* shape) {
  if (din_check_shape(shape)) return -1;
  return din_offsets(din_dims(*shape)).total;
}

extern "C" int hiprec_din_tiles(const hiprec_din_shape* shape, int32_t* out) {
  if (int rc = din_check_shape(shape)) return rc;
  HIPREC_REQUIRE(out, "NULL pointer");
  const DinDims q = din_dims(*shape);
  DinUnit f{}, b{};
  din_plan_lds(q, false, &f);
  din_plan_lds(q, true, &b);
  out[0] = kDinTile; out[1] = f.R; out[2] = b.R; out[3] = kDinSlice; out[4] = kDinSlabs;
  out[5] = f.wp_lds + 2 * f.w1_lds; out[6] = b.wp_lds + 2 * b.w1_lds;
  return 0;
}

extern "C" size_t hiprec_din_workspace_bytes(const hiprec_din_shape* shape, int64_t batch, int64_t n_cand, int32_t train) {
  if (din_check_shape(shape)) return 0;
  const DinDims q = din_dims(*shape);
  if (!din_batch_ok(q, batch, n_cand)) return 0;
  return sizeof(float) * static_cast<size_t>(din_carve_ws(nullptr, q, batch, n_cand, train != 0).floats);
}

extern "C" int hiprec_din_grad(const hiprec_din_shape* shape, const float* w_flat, float* g_flat, float* running,
                               int32_t update_running, const int64_t* seq, const int64_t* cand, const float* label,
                               int64_t batch, int64_t n_cand, float* logits_out, hiprec_stats* stats, void* scratch,
                               size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = din_check_shape(shape)) return rc;
  const DinDims q = din_dims(*shape);
  HIPREC_REQUIRE(w_flat && running && seq && cand && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(din_batch_ok(q, batch, n_cand), "DIN needs batch >= 1, n_cand >= 1, batch * maxlen <= 2^24 and batch * n_cand <= 2^24 "
                 "(got %lld, %lld)", static_cast<long long>(batch), static_cast<long long>(n_cand));
  if (g_flat) {
    HIPREC_REQUIRE(label && scratch, "training needs the labels and the scratch block");
    if (scratch_bytes < kScratchBytes) {
      set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
      return HIPREC_E_SCRATCH;
    }
  } else {
    HIPREC_REQUIRE(logits_out, "the eval forward needs the logits buffer");
  }
  const size_t need = hiprec_din_workspace_bytes(shape, batch, n_cand, g_flat != nullptr);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  return din_run(q, w_flat, g_flat, running, update_running, seq, cand, label, batch, n_cand, logits_out, stats,
                 static_cast<Scratch*>(scratch), static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_din_attention(const hiprec_din_shape* shape, const float* w_flat, const float* e, const float* q_rows,
                                    const uint8_t* mask, int64_t batch, int64_t n_cand, float* pooled, float* a,
                                    const float* dpooled, float* g_att, float* de, float* dq, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  if (int rc = din_check_shape(shape)) return rc;
  const DinDims q = din_dims(*shape);
  HIPREC_REQUIRE(w_flat && e && q_rows && mask && pooled && a && workspace, "NULL pointer");
  HIPREC_REQUIRE(din_batch_ok(q, batch, n_cand), "DIN needs batch >= 1, n_cand >= 1, batch * maxlen <= 2^24 and batch * n_cand <= 2^24");
  const bool bwd = dpooled != nullptr;
  HIPREC_REQUIRE(!bwd || (g_att && de && dq), "the stage's backward needs g_att, de and dq");
  const size_t need = hiprec_din_workspace_bytes(shape, batch, n_cand, bwd);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const DinOff o = din_offsets(q);
  DinWs w = din_carve_ws(static_cast<float*>(workspace), q, batch, n_cand, bwd);
  const int64_t BT = batch * q.T, N = batch * n_cand;
  if (int rc = din_prep(q, o, w_flat, w, st)) return rc;
  if (int rc = din_flags(mask, w.lv, BT, w.lc, N, st)) return rc;
  w.rows = const_cast<float*>(e);
  w.q = const_cast<float*>(q_rows);
  if (int rc = din_unit_forward(q, o, w_flat, w, batch, n_cand, pooled, a, st)) return rc;
  if (!bwd) return 0;
  // the stage's backward from d pooled alone: the unit's parameters into g_att, d e [B T, D] and d q [N, D] as rows
  if (int rc = din_fill(w.dU, w.zero_floats, 0.f, st)) return rc;
  if (int rc = din_fill(dq, N * q.D, 0.f, st)) return rc;
  DinUnit u{};
  const size_t lds = din_plan_lds(q, true, &u);
  u.C = static_cast<int>(n_cand);
  u.WpP = w.WpP; u.W1P = w.W1P; u.w2P = w.w2P; u.b1P = w.b1P; u.al1P = w.al1P; u.al2P = w.al2P; u.b2 = w_flat + o.a2b;
  u.rows = w.rows; u.q = w.q; u.U = w.U; u.V = w.V; u.lv = w.lv; u.lc = w.lc;
  const int n_slabs = static_cast<int>(std::min<int64_t>(batch, kDinSlabs));
  din_unit_bwd_kernel<<<n_slabs, kBlock, lds, st>>>(u, batch, a, dpooled, nullptr, w.dU, w.dV, dq, nullptr, w.drows, w.slabs);
  HIPREC_TRY(hipGetLastError());
  const int D = q.D;
  if (int rc = din_unit_finish(q, o, w, BT, N, n_slabs, g_att, de, w.dqv, st)) return rc;      // the GEMM's part of d e
  if (int rc = din_add(de, w.drows, BT * D, st)) return rc;      // the part summed on chip
  return din_add(dq, w.dqv, N * D, st);
}
