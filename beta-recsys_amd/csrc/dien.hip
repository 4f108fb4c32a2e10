// Deep Interest Evolution Network (Zhou et al., AAAI 2019): zero_grad + forward + loss + backward of one ranking step as a
// fixed sequence of launches, no host sync.  The contract is in include/hiprec.h; B sequences of T slots, C candidates per
// sequence, N = B C candidate rows, D = dim = the hidden width of both recurrent layers.
//
// ONE recurrence kernel template serves both layers.  A workgroup owns a tile of kDienTile = 16 rows and walks the T
// positions itself.  A row is a (sequence, candidate) pair, row n = b C + c, so the candidates of a sequence are
// neighbours; the interest extractor is the case C = 1, g = 1.  Per step:
//   * the projected input x W_ih^T + b (a grouped GEMM over all B T positions, outside the recurrence; for the evolution
//     layer on h1 [B T, D]: once per sequence, never per candidate) is staged into LDS once per SEQUENCE of the tile
//     (at most ceil(15 / C) + 1 of them), one step ahead and double buffered, and read from there by every candidate row;
//   * h W_hh^T runs on v_mfma_f32_16x16x4_f32: wave w owns the column tiles w, w + 4, ... and keeps the r, u and n
//     accumulators of one (row, unit) in one lane, the gate arithmetic is done on them;
//   * W_hh [3D, D] stays in LDS for all positions: the leading rows_res rows (all of them up to D = 96); the tail rows
//     (part of the n gate at D = 112, 128) are read through L2 from the parameter buffer itself, which needs no packing
//     because D is a multiple of 16.  The same row-major copy serves the backward (read transposed);
//   * a step at which no row of the tile is live (padding, dead candidates) skips the MFMAs.
// The evolution workgroup first computes its rows' attention: scores h1[b, t] . (att.weight q) (att.weight q is a
// grouped GEMM), a 16-lane group per row, then the masked softmax over the positions in LDS; a [N, T] reaches memory
// only when training or when the stage entry asks.
//
// Saved, not recomputed (training): per (row, position) the gates r | u | n | U_n h [4D] and the state before the
// position [D]: 5 D floats for every (sequence, position) of the extractor and every (row, position) of the evolution
// layer, plus a [N, T].  The reverse-time backward (same template) reads them one step ahead of the carry, keeps W_hh
// resident the same way, and per step forms the gate gradients, d a[b, c, t] (a 16-lane shuffle sum) and the carried d h
// (MFMA [16, 3D] x [3D, D]).  It overwrites the saved gates with d (W_hh h) = d r | d u | d (U_n h), so that d W_hh is a
// GEMM over the saved rows afterwards.  The gradient of the shared projected input is the sum over a sequence's
// candidates: the rows of a sequence inside the tile are added in row order in LDS; a sequence whose candidates straddle
// tiles leaves one partial per tile in ordered slabs, which a fold kernel adds in tile order.  After the walk the softmax
// backward gives d s, d (att.weight q) per row and the attention's share of d h1 (per sequence, same fold).
// d W_hh, d W_ih, the biases, d att.weight are K-sliced GEMMs / two-level column sums, added in slice order.
//
// The only float atomics are rows of d item_emb.weight; every other gradient is the same bits on every run.
#include <algorithm>

#include "din.hpp"

namespace hiprec {
namespace {

constexpr int kDienTile = 16;                 // rows of a recurrence workgroup: one MFMA row tile
constexpr int kDienOwn = kDinMaxDim / 16;     // units of a row that one lane of its 16-lane group owns
constexpr int kDienStage = (3 * kDinMaxDim + kBlock - 1) / kBlock;   // staged floats of one sequence per thread
constexpr size_t kDienLds = 160 * 1024;
constexpr int kDienSplitHH = 6, kDienSplitIH = 3, kDienSplitAtt = 3, kDienSplitIH1 = 6;   // K-slices of the weight-gradient GEMMs
constexpr int kDienCountBlocks = 8;           // partial counts of the auxiliary terms
constexpr int64_t kDienMaxSaved = 1ll << 24;  // B C T when training: rows of the saved gates

struct DienDims {
  int64_t n_items;
  int D, T;
  float aux_w;
  DinTower tw;      // widths and offsets only; dien_carve_ws adds the workspace
};

struct DienOff {
  int64_t xw_ih, xw_hh, xb, att, vw_ih, vw_hh, vb, total;
  int bn_total;
};

DienOff dien_offsets(DienDims& q) {
  DienOff o{};
  const int64_t D = q.D;
  int64_t p = (q.n_items + 1) * D;
  auto take = [&](int64_t n) { int64_t r = p; p += n; return r; };
  o.xw_ih = take(3 * D * D); o.xw_hh = take(3 * D * D); o.xb = take(3 * D);
  o.att = take(D * D);
  o.vw_ih = take(3 * D * D); o.vw_hh = take(3 * D * D); o.vb = take(3 * D);
  int in = 3 * q.D, bn = 0;
  DinTower& t = q.tw;
  for (int l = 0; l < t.L; ++l) {
    t.in[l] = in;
    t.dw[l] = take(static_cast<int64_t>(t.W[l]) * in); t.db[l] = take(t.W[l]); t.da[l] = take(t.W[l]);
    t.bn[l] = bn;
    bn += 2 * t.W[l];
    in = t.W[l];
  }
  t.ow = take(in); t.ob = take(1);
  o.total = p;
  o.bn_total = bn;
  return o;
}

// ---- the recurrence ----------------------------------------------------------------------------------------------------------
struct DienRec {
  int T, C, D, nslot, rows_res, ldA;
  int64_t R, B;                   // rows = B C
  const float *Whh, *Gi;          // [3D, D]; the projected input [B T, 3D]
  const uint8_t *lv, *lc;         // live positions [B T]; live rows [R] (NULL: every row)
  const float *h1, *aq;           // evolution: [B T, D], att.weight q [R, D]
  float* a;                       // evolution: [R, T], written by the forward (NULL: not), read by the backward
  float *hseq, *hT;               // extractor: the state after every position [B T, D]; evolution: the last state [R, D]
  float *hprev, *gates;           // training: the state before every position [R T, D], r | u | n | U_n h [R T, 4D]
  const float *dhT, *inj[3];      // backward: evolution d hT [R, D]; extractor up to three [B T, D] added at live positions
  float *partG, *partH, *daq;     // backward: [slabs][B T, 3D], [slabs][B T, D], [R, D]
};

// sequences that a tile of 16 consecutive rows can touch, at most
inline int dien_slots(int C) { return std::min(kDienTile, (kDienTile - 2 + C) / C + 1); }
// tiles that hold rows of one sequence, at most: the slabs of the per-sequence sums (1: no sequence straddles two tiles)
inline int dien_slabs(int C) { return kDienTile % C == 0 ? 1 : (C + kDienTile - 2) / kDienTile + 1; }

// floats of LDS beside the resident rows of W_hh
inline size_t dien_lds_fixed(int D, int T, int nslot, bool evolve, bool bwd) {
  const size_t ldh = D + 1, ldA = T | 1;
  size_t n = 3 * kDienTile + T + (static_cast<size_t>(nslot) * T + 3) / 4;      // slot, lo, hi, any; the live bytes
  if (bwd) n += kDienTile * (4 * D + 1) + kDienTile * ldh + (evolve ? 2 * kDienTile * ldA : 0);
  else n += 2 * kDienTile * ldh + 2 * static_cast<size_t>(nslot) * 3 * D + (evolve ? kDienTile * ldA : 0);
  return n;
}
inline int dien_rows_res(int D, int T, int nslot, bool evolve, bool bwd) {
  const size_t room = kDienLds / sizeof(float) - dien_lds_fixed(D, T, nslot, evolve, bwd);
  return std::min<int>(3 * D, static_cast<int>(room / (D + 1)) / 16 * 16);
}

struct DienTile {
  int *slot, *lo, *hi, *any;
  uint8_t* lv;
  int64_t n0, b_first;
  int nseq;
};

// The tile's bookkeeping at `base`: slot[i] = the sequence slot of row i (-1: a dead row), lo / hi[s] = the rows of slot s,
// lv[s T + t] = the live flags of slot s, any[t] = some row of the tile is live at t
__device__ __forceinline__ DienTile dien_tile_setup(const DienRec& p, float* base) {
  DienTile k;
  k.slot = reinterpret_cast<int*>(base);
  k.lo = k.slot + kDienTile; k.hi = k.lo + kDienTile; k.any = k.hi + kDienTile;
  k.lv = reinterpret_cast<uint8_t*>(k.any + p.T);
  k.n0 = static_cast<int64_t>(blockIdx.x) * kDienTile;
  const int64_t last = min(k.n0 + kDienTile - 1, p.R - 1);
  k.b_first = k.n0 / p.C;
  k.nseq = static_cast<int>(last / p.C - k.b_first) + 1;
  const int tid = threadIdx.x;
  if (tid < kDienTile) {
    const int64_t row = k.n0 + tid;
    k.slot[tid] = (row < p.R && (!p.lc || p.lc[row])) ? static_cast<int>(row / p.C - k.b_first) : -1;
  }
  if (tid < k.nseq) {
    const int64_t b = k.b_first + tid;
    k.lo[tid] = static_cast<int>(max(b * p.C, k.n0) - k.n0);
    k.hi[tid] = static_cast<int>(min((b + 1) * p.C, last + 1) - k.n0);
  }
  for (int e = tid; e < k.nseq * p.T; e += kBlock) k.lv[e] = p.lv[k.b_first * p.T + e] != 0;
  __syncthreads();
  for (int t = tid; t < p.T; t += kBlock) {
    int any = 0;
    for (int i = 0; i < kDienTile; ++i) any |= (k.slot[i] >= 0 && k.lv[k.slot[i] * p.T + t]);
    k.any[t] = any;
  }
  __syncthreads();
  return k;
}

// acc += A [16, K] B [K, 16] on v_mfma_f32_16x16x4_f32: the lane feeds A(l & 15, k + (l >> 4)) = ap[k] and
// B(k + (l >> 4), l & 15) = bp[k * sbk]; K is a multiple of 16 and the operands of four k-steps are loaded before their
// MFMAs issue, so the dependent chain pays one LDS / L2 round trip per group
__device__ __forceinline__ f32x4 dien_mma(f32x4 acc, const float* ap, const float* bp, int sbk, int K) {
  for (int k = 0; k < K; k += 16) {
    float a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u] = ap[k + 4 * u];
      b[u] = bp[(k + 4 * u) * sbk];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u], acc, 0, 0, 0);
  }
  return acc;
}

__device__ __forceinline__ float dien_sum16(float v) {
  v += __shfl_xor(v, 8, 16);
  v += __shfl_xor(v, 4, 16);
  v += __shfl_xor(v, 2, 16);
  v += __shfl_xor(v, 1, 16);
  return v;
}

// grid ceil(R / 16).  LDS: Ws [rows_res][D + 1], hb [2][16][D + 1], gis [2][nslot][3D], as [16][ldA] (evolution), the tile's
// bookkeeping
template <bool EVOLVE>
__global__ __launch_bounds__(kBlock) void dien_rec_fwd_kernel(DienRec p) {
  extern __shared__ float dien_lds[];
  const int D = p.D, T = p.T, D3 = 3 * D, ldw = D + 1, ldh = D + 1, ldA = p.ldA;
  float* Ws = dien_lds;
  float* hb = Ws + p.rows_res * ldw;
  float* gis = hb + 2 * kDienTile * ldh;
  float* as = gis + 2 * p.nslot * D3;
  const DienTile k = dien_tile_setup(p, as + (EVOLVE ? kDienTile * ldA : 0));
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_in_block();
  for (int e = tid; e < p.rows_res * D; e += kBlock) {
    const int r = e / D, c = e - r * D;
    Ws[r * ldw + c] = p.Whh[e];
  }
  for (int e = tid; e < 2 * kDienTile * ldh; e += kBlock) hb[e] = 0.f;

  if (EVOLVE) {      // the attention of the tile's rows: a 16-lane group per row
    const int i = tid >> 4, l16 = tid & 15, sl = k.slot[i];
    const int64_t row = k.n0 + i;
    float aqr[kDienOwn];
#pragma unroll
    for (int n = 0; n < kDienOwn; ++n) {
      const int j = l16 + 16 * n;
      aqr[n] = (sl >= 0 && j < D) ? p.aq[row * D + j] : 0.f;
    }
    for (int t = 0; t < T; ++t) {
      float part = 0.f;
      if (sl >= 0 && k.lv[sl * T + t]) {
        const float* hr = p.h1 + ((k.b_first + sl) * T + t) * D;
#pragma unroll
        for (int n = 0; n < kDienOwn; ++n) {
          const int j = l16 + 16 * n;
          if (j < D) part = fmaf(hr[j], aqr[n], part);
        }
      }
      part = dien_sum16(part);
      if (l16 == 0) as[i * ldA + t] = part;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int t = l16; t < T; t += 16)
      if (sl >= 0 && k.lv[sl * T + t]) m = fmaxf(m, as[i * ldA + t]);
    m = fmaxf(m, __shfl_xor(m, 8, 16));
    m = fmaxf(m, __shfl_xor(m, 4, 16));
    m = fmaxf(m, __shfl_xor(m, 2, 16));
    m = fmaxf(m, __shfl_xor(m, 1, 16));
    float sum = 0.f;
    for (int t = l16; t < T; t += 16) {
      const float e = (sl >= 0 && k.lv[sl * T + t]) ? expf(as[i * ldA + t] - m) : 0.f;
      as[i * ldA + t] = e;
      sum += e;
    }
    sum = dien_sum16(sum);
    for (int t = l16; t < T; t += 16) {
      const float v = sum > 0.f ? as[i * ldA + t] / sum : 0.f;
      as[i * ldA + t] = v;
      if (p.a && row < p.R) p.a[row * T + t] = v;
    }
  }

  // the projected input of position t, one row per sequence of the tile: loaded a step ahead, stored behind the MFMAs
  float st[kDienTile][kDienStage];
  auto stage_load = [&](int t) {
#pragma unroll
    for (int s = 0; s < kDienTile; ++s) {
      if (s >= k.nseq) break;
      const bool on = t < T && k.lv[s * T + t];
      const float* src = p.Gi + ((k.b_first + s) * T + (t < T ? t : 0)) * D3;
#pragma unroll
      for (int n = 0; n < kDienStage; ++n) {
        const int c = tid + n * kBlock;
        st[s][n] = (on && c < D3) ? src[c] : 0.f;
      }
    }
  };
  auto stage_store = [&](int buf) {
    float* dst = gis + buf * p.nslot * D3;
#pragma unroll
    for (int s = 0; s < kDienTile; ++s) {
      if (s >= k.nseq) break;
#pragma unroll
      for (int n = 0; n < kDienStage; ++n) {
        const int c = tid + n * kBlock;
        if (c < D3) dst[s * D3 + c] = st[s][n];
      }
    }
  };
  stage_load(0);
  stage_store(0);
  __syncthreads();

  const int n_ct = D / 16, col = lane & 15, lk = lane >> 4, row0 = 4 * lk;
  for (int t = 0; t < T; ++t) {
    const float* hc = hb + (t & 1) * kDienTile * ldh;
    float* hn = hb + ((t + 1) & 1) * kDienTile * ldh;
    const float* gi = gis + (t & 1) * p.nslot * D3;
    const bool any = k.any[t] != 0;
    stage_load(t + 1);
    for (int ct = wave; ct < n_ct; ct += kWavesPerBlock) {
      const int j = ct * 16 + col;
      f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      if (any) {
        const float* ap = hc + col * ldh + lk;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
          const int wrow = g * D + ct * 16;
          if (wrow + 16 <= p.rows_res) acc[g] = dien_mma(acc[g], ap, Ws + (wrow + col) * ldw + lk, 1, D);
          else acc[g] = dien_mma(acc[g], ap, p.Whh + static_cast<int64_t>(wrow + col) * D + lk, 1, D);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = row0 + r, sl = k.slot[i];
        const int64_t row = k.n0 + i, m = row * T + t;
        const float h_old = hc[i * ldh + j];
        float h_new = h_old;
        if (sl >= 0 && k.lv[sl * T + t]) {
          const float* gr = gi + sl * D3 + j;
          const float rr = sigmoid_f32(gr[0] + acc[0][r]);
          const float uu = sigmoid_f32(gr[D] + acc[1][r]);
          const float hp = acc[2][r];
          const float nn = tanhf(fmaf(rr, hp, gr[2 * D]));
          const float gu = EVOLVE ? as[i * ldA + t] * uu : uu;
          h_new = fmaf(gu, nn, (1.f - gu) * h_old);
          if (p.gates) {
            float* gp = p.gates + m * 4 * D + j;
            gp[0] = rr;
            gp[D] = uu;
            gp[2 * D] = nn;
            gp[3 * D] = hp;
          }
        }
        hn[i * ldh + j] = h_new;
        if (row < p.R) {
          if (p.hprev) p.hprev[m * D + j] = h_old;
          if (!EVOLVE) p.hseq[m * D + j] = h_new;
        }
      }
    }
    stage_store((t + 1) & 1);
    lds_barrier();
  }
  if (EVOLVE) {
    const float* hf = hb + (T & 1) * kDienTile * ldh;
    for (int e = tid; e < kDienTile * D; e += kBlock) {
      const int i = e / D, j = e - i * D;
      if (k.n0 + i < p.R) p.hT[(k.n0 + i) * D + j] = hf[i * ldh + j];
    }
  }
}

// Reverse time.  LDS: Ws [rows_res][D + 1] (the leading rows of W_hh, read as B(k, j) = W[k][j]), dG [16][4D + 1] = d r | d u |
// d (U_n h) | d n of the tile, dh [16][D + 1], as / das [16][ldA] (evolution: a and d a, then d s), the tile's bookkeeping
template <bool EVOLVE>
__global__ __launch_bounds__(kBlock) void dien_rec_bwd_kernel(DienRec p) {
  extern __shared__ float dien_lds[];
  const int D = p.D, T = p.T, D3 = 3 * D, ldw = D + 1, ldh = D + 1, ldg = 4 * D + 1, ldA = p.ldA;
  const int64_t BT = p.B * T;
  float* Ws = dien_lds;
  float* dG = Ws + p.rows_res * ldw;
  float* dh = dG + kDienTile * ldg;
  float* as = dh + kDienTile * ldh;
  float* das = as + (EVOLVE ? kDienTile * ldA : 0);
  const DienTile k = dien_tile_setup(p, das + (EVOLVE ? kDienTile * ldA : 0));
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_in_block();
  const int i = tid >> 4, l16 = tid & 15, sl = k.slot[i];      // the lane's row and its units l16, l16 + 16, ...
  const int64_t row = k.n0 + i, b = k.b_first + (sl >= 0 ? sl : 0);
  for (int e = tid; e < p.rows_res * D; e += kBlock) {
    const int r = e / D, c = e - r * D;
    Ws[r * ldw + c] = p.Whh[e];
  }
#pragma unroll
  for (int n = 0; n < kDienOwn; ++n) {
    const int j = l16 + 16 * n;
    if (j < D) dh[i * ldh + j] = (EVOLVE && sl >= 0) ? p.dhT[row * D + j] : 0.f;
  }
  if (EVOLVE)
    for (int t = l16; t < T; t += 16) as[i * ldA + t] = row < p.R ? p.a[row * T + t] : 0.f;
  __syncthreads();

  // what a step reads from memory does not depend on the carry: fetched one step ahead, behind the MFMAs
  float p_d[kDienOwn], p_r[kDienOwn], p_u[kDienOwn], p_n[kDienOwn], p_hp[kDienOwn], p_h[kDienOwn];
  auto fetch = [&](int t) {
    const bool live = t >= 0 && sl >= 0 && k.lv[sl * T + t];
    const int64_t m = row * T + (t >= 0 ? t : 0);
#pragma unroll
    for (int n = 0; n < kDienOwn; ++n) {
      const int j = l16 + 16 * n;
      p_d[n] = p_r[n] = p_u[n] = p_n[n] = p_hp[n] = p_h[n] = 0.f;
      if (!live || j >= D) continue;
      const float* gp = p.gates + m * 4 * D + j;
      p_r[n] = gp[0];
      p_u[n] = gp[D];
      p_n[n] = gp[2 * D];
      p_hp[n] = gp[3 * D];
      p_h[n] = p.hprev[m * D + j];
      if (!EVOLVE) {
        float d = 0.f;
#pragma unroll
        for (int s = 0; s < 3; ++s)
          if (p.inj[s]) d += p.inj[s][m * D + j];
        p_d[n] = d;
      }
    }
  };
  fetch(T - 1);
  const int n_ct = D / 16, col = lane & 15, lk = lane >> 4, row0 = 4 * lk;
  for (int t = T - 1; t >= 0; --t) {
    const bool live = sl >= 0 && k.lv[sl * T + t];
    const float g = EVOLVE ? as[i * ldA + t] : 1.f;
    const int64_t m = row * T + t;
    float dap = 0.f;
#pragma unroll
    for (int n = 0; n < kDienOwn; ++n) {
      const int j = l16 + 16 * n;
      if (j >= D) continue;
      float d_r = 0.f, d_u = 0.f, d_n = 0.f, d_hp = 0.f;
      if (live) {
        const float d = dh[i * ldh + j] + p_d[n];
        const float rr = p_r[n], uu = p_u[n], nn = p_n[n], gu = g * uu;
        const float d_gu = d * (nn - p_h[n]);
        dap = fmaf(d_gu, uu, dap);
        d_n = d * gu * (1.f - nn * nn);
        d_u = d_gu * g * uu * (1.f - uu);
        d_r = d_n * p_hp[n] * rr * (1.f - rr);
        d_hp = d_n * rr;
        dh[i * ldh + j] = d * (1.f - gu);
      }
      float* o = dG + i * ldg + j;
      o[0] = d_r;
      o[D] = d_u;
      o[2 * D] = d_hp;
      o[3 * D] = d_n;
      if (row < p.R) {      // over the saved gates: d (W_hh h) of this (row, position), zero where it is dead
        float* gp = p.gates + m * 4 * D + j;
        gp[0] = d_r;
        gp[D] = d_u;
        gp[2 * D] = d_hp;
      }
    }
    if (EVOLVE) {
      dap = dien_sum16(dap);
      if (l16 == 0) das[i * ldA + t] = dap;
    }
    lds_barrier();
    fetch(t - 1);
    if (k.any[t]) {      // d h += d (W_hh h) W_hh
      for (int ct = wave; ct < n_ct; ct += kWavesPerBlock) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = dien_mma(acc, dG + col * ldg + lk, Ws + lk * ldw + ct * 16 + col, ldw, p.rows_res);
        if (p.rows_res < D3)
          acc = dien_mma(acc, dG + col * ldg + p.rows_res + lk,
                         p.Whh + static_cast<int64_t>(p.rows_res + lk) * D + ct * 16 + col, D, D3 - p.rows_res);
#pragma unroll
        for (int r = 0; r < 4; ++r) dh[(row0 + r) * ldh + ct * 16 + col] += acc[r];
      }
    }
    // the gradient of the projected input: the rows of every sequence of the tile added in row order
    for (int s = 0; s < k.nseq; ++s) {
      const int64_t bs = k.b_first + s, slab = blockIdx.x - bs * p.C / kDienTile;
      float* out = p.partG + ((slab * BT) + bs * T + t) * D3;
      for (int c = tid; c < D3; c += kBlock) {
        const float* src = dG + (c < 2 * D ? c : c + D);
        float sum = 0.f;
        for (int r = k.lo[s]; r < k.hi[s]; ++r) sum += src[r * ldg];
        out[c] = sum;
      }
    }
    lds_barrier();
  }
  if (!EVOLVE) return;

  // the softmax backward: d s = a (d a - <a, d a>) per row; then d (att.weight q) per row and the attention's d h1 per sequence
  float* aqs = dG;      // [16][D + 1]
  {
    float dot = 0.f;
    for (int t = l16; t < T; t += 16) dot = fmaf(as[i * ldA + t], das[i * ldA + t], dot);
    dot = dien_sum16(dot);
    for (int t = l16; t < T; t += 16) das[i * ldA + t] = as[i * ldA + t] * (das[i * ldA + t] - dot);
#pragma unroll
    for (int n = 0; n < kDienOwn; ++n) {
      const int j = l16 + 16 * n;
      if (j < D) aqs[i * ldh + j] = sl >= 0 ? p.aq[row * D + j] : 0.f;
    }
  }
  __syncthreads();
  {
    float acc[kDienOwn];
#pragma unroll
    for (int n = 0; n < kDienOwn; ++n) acc[n] = 0.f;
    for (int t = 0; t < T; ++t) {
      if (sl < 0 || !k.lv[sl * T + t]) continue;
      const float ds = das[i * ldA + t];
      const float* hr = p.h1 + (b * T + t) * D;
#pragma unroll
      for (int n = 0; n < kDienOwn; ++n) {
        const int j = l16 + 16 * n;
        if (j < D) acc[n] = fmaf(ds, hr[j], acc[n]);
      }
    }
#pragma unroll
    for (int n = 0; n < kDienOwn; ++n) {
      const int j = l16 + 16 * n;
      if (j < D && row < p.R) p.daq[row * D + j] = acc[n];
    }
  }
  for (int s = 0; s < k.nseq; ++s) {
    const int64_t bs = k.b_first + s, slab = blockIdx.x - bs * p.C / kDienTile;
    float* out = p.partH + ((slab * BT) + bs * T) * D;
    for (int e = tid; e < T * D; e += kBlock) {
      const int t = e / D, j = e - t * D;
      float sum = 0.f;
      for (int r = k.lo[s]; r < k.hi[s]; ++r) sum = fmaf(das[r * ldA + t], aqs[r * ldh + j], sum);
      out[e] = sum;
    }
  }
}

// out [B T, W] = the slabs of every sequence added in tile order (dien_rec_bwd_kernel left one per tile that holds its rows)
__global__ __launch_bounds__(kBlock) void dien_seq_fold_kernel(const float* __restrict__ part, int64_t B, int T, int C, int W,
                                                               float* __restrict__ out) {
  const int64_t BT = B * T, n = BT * W;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t b = e / (static_cast<int64_t>(T) * W);
    const int slabs = static_cast<int>((b * C + C - 1) / kDienTile - b * C / kDienTile) + 1;
    float sum = 0.f;
    for (int s = 0; s < slabs; ++s) sum += part[s * BT * W + e];
    out[e] = sum;
  }
}

// out[i] = the n K-slices of a weight gradient added in slice order
__global__ __launch_bounds__(kBlock) void dien_slice_fold_kernel(const float* __restrict__ parts, int n, int64_t count,
                                                                 float* __restrict__ out) {
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < count; e += static_cast<int64_t>(gridDim.x) * kBlock)
    out[e] = din_slab_sum(parts, n, count, e);
}

// ---- the auxiliary loss --------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool dien_id_ok(int64_t id, int64_t n_items) { return id >= 1 && id <= n_items; }

// cnt[block] = the block's number of auxiliary terms (an exact integer in fp32); an id of neg out of range raises the status
__global__ __launch_bounds__(kBlock) void dien_aux_count_kernel(const int64_t* __restrict__ seq, const int64_t* __restrict__ neg,
                                                                int64_t B, int T, int64_t n_items, float* __restrict__ cnt,
                                                                hiprec_stats* stats) {
  __shared__ float s_cnt[kWavesPerBlock];
  float c = 0.f;
  for (int64_t m = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; m < B * T; m += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t ng = neg[m];
    if (ng < 0 || ng > n_items) atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
    if (m % T < T - 1 && dien_id_ok(seq[m], n_items) && dien_id_ok(seq[m + 1], n_items) && dien_id_ok(neg[m + 1], n_items)) c += 1.f;
  }
  c = wave_sum(c);
  if (lane_id() == 0) s_cnt[wave_in_block()] = c;
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

// One wave per (sequence, position): softplus(-<h1[t], E[seq[t + 1]]>) + softplus(<h1[t], E[neg[t + 1]]>), the mean over the
// terms times aux_w.  dh1 [B T, D] is written everywhere (0 where there is no term), the two item rows get row atomics,
// loss_part[block] the block's share of the loss.
__global__ __launch_bounds__(kBlock) void dien_aux_kernel(const float* __restrict__ E, const float* __restrict__ h1,
                                                          const int64_t* __restrict__ seq, const int64_t* __restrict__ neg,
                                                          int64_t B, int T, int D, int64_t n_items, float aux_w,
                                                          const float* __restrict__ cnt, int n_cnt, float* __restrict__ dh1,
                                                          float* __restrict__ g_item, float* __restrict__ loss_part) {
  __shared__ float s_loss[kWavesPerBlock];
  float total = 0.f;
  for (int s = 0; s < n_cnt; ++s) total += cnt[s];
  const float scale = total > 0.f ? aux_w / total : 0.f;
  const int lane = lane_id();
  float loss = 0.f;
  for (int64_t m = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); m < B * T;
       m += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const bool on = m % T < T - 1 && dien_id_ok(seq[m], n_items) && dien_id_ok(seq[m + 1], n_items) &&
                    dien_id_ok(neg[m + 1], n_items);
    if (!on) {
      for (int d = lane; d < D; d += kWave) dh1[m * D + d] = 0.f;
      continue;
    }
    const int64_t ip = seq[m + 1], in = neg[m + 1];
    float h[2], ep[2], en[2], sp = 0.f, sn = 0.f;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int d = lane + kWave * n;
      h[n] = d < D ? h1[m * D + d] : 0.f;
      ep[n] = d < D ? E[ip * D + d] : 0.f;
      en[n] = d < D ? E[in * D + d] : 0.f;
      sp = fmaf(h[n], ep[n], sp);
      sn = fmaf(h[n], en[n], sn);
    }
    sp = wave_sum(sp);
    sn = wave_sum(sn);
    float sig_neg_p, sig_n;
    loss += neg_logsigmoid(sp, &sig_neg_p) + neg_logsigmoid(-sn, &sig_n);      // sigmoid(-sp), sigmoid(sn)
    const float dp = -sig_neg_p * scale, dn = sig_n * scale;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int d = lane + kWave * n;
      if (d >= D) continue;
      dh1[m * D + d] = fmaf(dp, ep[n], dn * en[n]);
      atomic_add_f32(g_item + ip * D + d, dp * h[n]);
      atomic_add_f32(g_item + in * D + d, dn * h[n]);
    }
  }
  if (lane == 0) s_loss[wave_in_block()] = loss;      // wave-uniform
  __syncthreads();
  if (threadIdx.x == 0) loss_part[blockIdx.x] = ((s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3])) * scale;
}

// after the BCE: the auxiliary loss joins the step's loss partials, its blocks added in order
__global__ __launch_bounds__(kWave) void dien_aux_loss_kernel(const float* __restrict__ loss_part, int n, Scratch* scratch) {
  float t = 0.f;
  for (int s = lane_id(); s < n; s += kWave) t += loss_part[s];
  t = wave_sum(t);
  if (lane_id() == 0) scratch->partials[0].x += t;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
int dien_check_shape(const hiprec_dien_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  HIPREC_REQUIRE(s->n_items >= 1 && s->n_items < (1ll << 31), "DIEN needs 1 <= n_items < 2^31, got %lld",
                 static_cast<long long>(s->n_items));
  HIPREC_REQUIRE(s->dim >= 16 && s->dim <= kDinMaxDim && s->dim % 16 == 0,
                 "DIEN needs emb_dim a multiple of 16 in 16 .. %d (got %d)", kDinMaxDim, s->dim);
  HIPREC_REQUIRE(s->maxlen >= 1 && s->maxlen <= kDinMaxLen, "DIEN needs 1 <= maxlen <= %d (got %d)", kDinMaxLen, s->maxlen);
  HIPREC_REQUIRE(s->n_dnn >= 1 && s->n_dnn <= kDinMaxLayers, "DIEN needs 1 .. %d dnn_hidden widths (got %d)", kDinMaxLayers,
                 s->n_dnn);
  for (int l = 0; l < s->n_dnn; ++l)
    HIPREC_REQUIRE(s->dnn[l] >= 1 && s->dnn[l] <= kDinMaxDnn, "DIEN needs dnn_hidden widths in 1 .. %d (got %d)", kDinMaxDnn,
                   s->dnn[l]);
  HIPREC_REQUIRE(s->dnn_act == 0 || s->dnn_act == 1, "DIEN: dnn_activation is dice (0) or prelu (1)");
  HIPREC_REQUIRE(s->aux_weight >= 0.f, "DIEN needs aux_weight >= 0");
  return 0;
}

DienDims dien_dims(const hiprec_dien_shape& s) {
  DienDims q{};
  q.n_items = s.n_items; q.D = s.dim; q.T = s.maxlen; q.aux_w = s.aux_weight;
  q.tw.L = s.n_dnn; q.tw.act = s.dnn_act;
  for (int l = 0; l < s.n_dnn; ++l) q.tw.W[l] = s.dnn[l];
  return q;
}

struct DienWs {
  float *rows, *q, *Gi1, *h1, *aq, *Gi2, *hT, *z;
  uint8_t *lv, *lc;
  // training
  float *hprev1, *gates1, *a, *hprev2, *gates2, *dhT, *dqz, *daq, *dqa, *partG, *dGi2, *partH, *dh1a, *dh1p, *dh1x, *dGi1,
      *drows, *sWhh2, *sWih2, *sAtt, *sWhh1, *sWih1, *cnt, *lossp, *cs;
  int64_t floats;
};

DienWs dien_carve_ws(float* base, DienDims& q, int64_t B, int64_t C, bool train, bool stage) {
  DienWs w{};
  float* p = base;
  auto take = [&](int64_t n) { float* r = p; p += (n + 3) / 4 * 4; return r; };
  const int64_t D = q.D, T = q.T, BT = B * T, N = B * C, NT = N * T, slabs = dien_slabs(static_cast<int>(C));
  w.lv = reinterpret_cast<uint8_t*>(take((BT + 3) / 4)); w.lc = reinterpret_cast<uint8_t*>(take((N + 3) / 4));
  w.aq = take(N * D); w.Gi2 = take(BT * 3 * D);
  if (!stage) {
    w.rows = take(BT * D); w.q = take(N * D); w.Gi1 = take(BT * 3 * D); w.h1 = take(BT * D); w.hT = take(N * D);
    w.z = take(N * 3 * D);
  }
  DinTower& t = q.tw;
  int wide = 3 * q.D;
  if (!stage) {
    int sumw = 0;
    for (int l = 0; l < t.L; ++l) {
      t.x[l] = take(N * t.W[l]); t.y[l] = take(N * t.W[l]);
      wide = std::max(wide, t.W[l]);
      sumw += t.W[l];
    }
    t.mean = take(sumw); t.var = take(sumw); t.logit = take(N);
  }
  if (train) {
    if (!stage) {
      t.dlogit = take(N); t.dA = take(N * wide); t.dB = take(N * wide); t.sums = take(2 * wide);
      w.hprev1 = take(BT * D); w.gates1 = take(BT * 4 * D); w.a = take(NT); w.dhT = take(N * D); w.dqz = take(N * D);
      w.dqa = take(N * D); w.dh1a = take(BT * D); w.dh1p = take(BT * D); w.dh1x = take(BT * D); w.dGi1 = take(BT * 3 * D);
      w.drows = take(BT * D);
      w.sWhh1 = take(kDienSplitHH * 3 * D * D); w.sWih1 = take(kDienSplitIH1 * 3 * D * D);
      w.cnt = take(kDienCountBlocks); w.lossp = take(kMaxBlocks);
    }
    w.hprev2 = take(NT * D); w.gates2 = take(NT * 4 * D); w.daq = take(N * D);
    w.partG = take(slabs * BT * 3 * D); w.partH = take(slabs * BT * D);
    if (slabs > 1) { w.dGi2 = take(BT * 3 * D); if (stage) w.dh1a = take(BT * D); }
    w.sWhh2 = take(kDienSplitHH * 3 * D * D); w.sWih2 = take(kDienSplitIH * 3 * D * D); w.sAtt = take(kDienSplitAtt * D * D);
    w.cs = take(2 * colsum_ws_floats(static_cast<int>(std::max(BT, N)), wide));
    t.cs = w.cs;
  }
  w.floats = p - base;
  return w;
}

// the workspace of hiprec_dien_extract: the extractor's share of the step's
DienWs dien_carve_extract(float* base, const DienDims& q, int64_t B, bool train) {
  DienWs w{};
  float* p = base;
  auto take = [&](int64_t n) { float* r = p; p += (n + 3) / 4 * 4; return r; };
  const int64_t D = q.D, BT = B * q.T;
  w.lv = reinterpret_cast<uint8_t*>(take((BT + 3) / 4)); w.Gi1 = take(BT * 3 * D);
  if (train) {
    w.hprev1 = take(BT * D); w.gates1 = take(BT * 4 * D); w.dGi1 = take(BT * 3 * D);
    w.sWhh1 = take(kDienSplitHH * 3 * D * D); w.sWih1 = take(kDienSplitIH1 * 3 * D * D);
    w.cs = take(2 * colsum_ws_floats(static_cast<int>(BT), 3 * q.D));
  }
  w.floats = p - base;
  return w;
}

bool dien_batch_ok(const DienDims& q, int64_t B, int64_t C, bool train) {
  if (B < 1 || C < 1 || B * q.T > kDinMaxRows || B * C > kDinMaxRows) return false;
  return !train || B * C * q.T <= kDienMaxSaved;
}

std::atomic<uint64_t> dien_lds_ok{0};

int dien_allow_lds() {
  return allow_dynamic_lds({reinterpret_cast<const void*>(&dien_rec_fwd_kernel<false>),
                            reinterpret_cast<const void*>(&dien_rec_fwd_kernel<true>),
                            reinterpret_cast<const void*>(&dien_rec_bwd_kernel<false>),
                            reinterpret_cast<const void*>(&dien_rec_bwd_kernel<true>)},
                           kDienLds, dien_lds_ok, "the DIEN recurrence");
}

template <bool EVOLVE>
int dien_launch_rec(DienRec r, bool bwd, hipStream_t st) {
  if (int rc = dien_allow_lds()) return rc;
  r.nslot = dien_slots(r.C);
  r.ldA = r.T | 1;
  r.rows_res = dien_rows_res(r.D, r.T, r.nslot, EVOLVE, bwd);
  const size_t lds = sizeof(float) * (dien_lds_fixed(r.D, r.T, r.nslot, EVOLVE, bwd) + static_cast<size_t>(r.rows_res) * (r.D + 1));
  const int grid = static_cast<int>((r.R + kDienTile - 1) / kDienTile);
  if (bwd) dien_rec_bwd_kernel<EVOLVE><<<grid, kBlock, lds, st>>>(r);
  else dien_rec_fwd_kernel<EVOLVE><<<grid, kBlock, lds, st>>>(r);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

int dien_fold_slices(const float* parts, int n, int64_t count, float* out, hipStream_t st) {
  dien_slice_fold_kernel<<<grid_for_threads(count), kBlock, 0, st>>>(parts, n, count, out);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// att.weight q and the evolution layer's projected input (one grouped launch), then the evolution recurrence with its attention
int dien_evolve_forward(const DienDims& q, const DienOff& o, const float* w_flat, const DienWs& a, const float* h1,
                        const float* qrows, int64_t B, int64_t C, bool train, float* hT, float* att, hipStream_t st) {
  const int D = q.D, BT = static_cast<int>(B * q.T), N = static_cast<int>(B * C);
  GemmGroup g{};
  g.n = 2;
  g.p[0] = make_gemm(kNT, N, D, D, qrows, D, w_flat + o.att, D, a.aq, D, nullptr, 0, nullptr, 0, false);
  g.p[1] = make_gemm(kNT, BT, 3 * D, D, h1, D, w_flat + o.vw_ih, D, a.Gi2, 3 * D, w_flat + o.vb, 0, nullptr, 0, false);
  if (int rc = launch_group(g, st)) return rc;
  DienRec r{};
  r.T = q.T; r.C = static_cast<int>(C); r.D = D; r.R = B * C; r.B = B;
  r.Whh = w_flat + o.vw_hh; r.Gi = a.Gi2; r.lv = a.lv; r.lc = a.lc; r.h1 = h1; r.aq = a.aq; r.a = att; r.hT = hT;
  r.hprev = train ? a.hprev2 : nullptr; r.gates = train ? a.gates2 : nullptr;
  return dien_launch_rec<true>(r, false, st);
}

// From d hT: the evolution recurrence in reverse, the folds, and one grouped launch for d evolve.*, d att.weight, the
// projection's d h1 (into dh1p) and d q (into dqa).  g_att: the gradient span that starts at att.weight.  *dh1a = the
// attention's d h1.
int dien_evolve_backward(const DienDims& q, const DienOff& o, const float* w_flat, const DienWs& a, const float* h1,
                         const float* qrows, const float* att, const float* dhT, int64_t B, int64_t C, float* g_att,
                         float* dh1p, float* dqa, const float** dh1a, hipStream_t st) {
  const int D = q.D, T = q.T, BT = static_cast<int>(B * T), N = static_cast<int>(B * C), NT = N * T;
  const bool folded = dien_slabs(static_cast<int>(C)) > 1;
  float* dGi2 = folded ? a.dGi2 : a.partG;
  float* dh1_att = folded ? a.dh1a : a.partH;
  DienRec r{};
  r.T = T; r.C = static_cast<int>(C); r.D = D; r.R = B * C; r.B = B;
  r.Whh = w_flat + o.vw_hh; r.lv = a.lv; r.lc = a.lc; r.h1 = h1; r.aq = a.aq; r.a = const_cast<float*>(att);
  r.hprev = a.hprev2; r.gates = a.gates2; r.dhT = dhT; r.partG = a.partG; r.partH = a.partH; r.daq = a.daq;
  if (int rc = dien_launch_rec<true>(r, true, st)) return rc;
  if (folded) {
    dien_seq_fold_kernel<<<grid_for_threads(static_cast<int64_t>(BT) * 3 * D), kBlock, 0, st>>>(a.partG, B, T, r.C, 3 * D, dGi2);
    HIPREC_TRY(hipGetLastError());
    dien_seq_fold_kernel<<<grid_for_threads(static_cast<int64_t>(BT) * D), kBlock, 0, st>>>(a.partH, B, T, r.C, D, dh1_att);
    HIPREC_TRY(hipGetLastError());
  }
  *dh1a = dh1_att;
  GemmGroup g{};
  const int n_hh = din_add_wgrad_slices(g, kDienSplitHH, 3 * D, D, NT, a.gates2, 4 * D, a.hprev2, D, a.sWhh2);
  const int n_ih = din_add_wgrad_slices(g, kDienSplitIH, 3 * D, D, BT, dGi2, 3 * D, h1, D, a.sWih2);
  const int n_at = din_add_wgrad_slices(g, kDienSplitAtt, D, D, N, a.daq, D, qrows, D, a.sAtt);
  g.p[g.n++] = make_gemm(kNN, BT, D, 3 * D, dGi2, 3 * D, w_flat + o.vw_ih, D, dh1p, D, nullptr, 0, nullptr, 0, false);
  g.p[g.n++] = make_gemm(kNN, N, D, D, a.daq, D, w_flat + o.att, D, dqa, D, nullptr, 0, nullptr, 0, false);
  g.p[g.n++] = make_colsum(dGi2, BT, 3 * D, 3 * D, g_att + (o.vb - o.att), a.cs);
  static_assert(kDienSplitHH + kDienSplitIH + kDienSplitAtt + 3 <= kMaxGroup, "one grouped launch");
  if (int rc = launch_group(g, st)) return rc;
  if (int rc = launch_colsum_reduce(g, st)) return rc;
  const int64_t DD = static_cast<int64_t>(D) * D;
  if (int rc = dien_fold_slices(a.sWhh2, n_hh, 3 * DD, g_att + (o.vw_hh - o.att), st)) return rc;
  if (int rc = dien_fold_slices(a.sWih2, n_ih, 3 * DD, g_att + (o.vw_ih - o.att), st)) return rc;
  return dien_fold_slices(a.sAtt, n_at, DD, g_att, st);
}

DienRec dien_extract_rec(const DienDims& q, const DienOff& o, const float* w_flat, const DienWs& a, int64_t B, bool train) {
  DienRec x{};
  x.T = q.T; x.C = 1; x.D = q.D; x.R = B; x.B = B;
  x.Whh = w_flat + o.xw_hh; x.Gi = a.Gi1; x.lv = a.lv;
  x.hprev = train ? a.hprev1 : nullptr; x.gates = train ? a.gates1 : nullptr;
  return x;
}

// the extractor's projected input (one GEMM over all B T positions), then its recurrence: h1 [B T, D] = the state after every
// position
int dien_extract_forward(const DienDims& q, const DienOff& o, const float* w_flat, const DienWs& a, const float* rows, int64_t B,
                         bool train, float* h1, hipStream_t st) {
  const int D = q.D, BT = static_cast<int>(B * q.T);
  GemmGroup g{};
  g.n = 1;
  g.p[0] = make_gemm(kNT, BT, 3 * D, D, rows, D, w_flat + o.xw_ih, D, a.Gi1, 3 * D, w_flat + o.xb, 0, nullptr, 0, false);
  if (int rc = launch_group(g, st)) return rc;
  DienRec x = dien_extract_rec(q, o, w_flat, a, B, train);
  x.hseq = h1;
  return dien_launch_rec<false>(x, false, st);
}

// From up to three d h1 [B T, D] (added at the live positions while they are read): the extractor's recurrence in reverse and
// one grouped launch for d extractor.* (into g_ext, the gradient span that starts at extractor.weight_ih) and d rows [B T, D]
int dien_extract_backward(const DienDims& q, const DienOff& o, const float* w_flat, const DienWs& a, const float* rows,
                          const float* dh1a, const float* dh1b, const float* dh1c, int64_t B, float* g_ext, float* drows,
                          hipStream_t st) {
  const int D = q.D, BT = static_cast<int>(B * q.T);
  DienRec x = dien_extract_rec(q, o, w_flat, a, B, true);
  x.inj[0] = dh1a; x.inj[1] = dh1b; x.inj[2] = dh1c; x.partG = a.dGi1;
  if (int rc = dien_launch_rec<false>(x, true, st)) return rc;
  GemmGroup g{};
  const int n_hh = din_add_wgrad_slices(g, kDienSplitHH, 3 * D, D, BT, a.gates1, 4 * D, a.hprev1, D, a.sWhh1);
  const int n_ih = din_add_wgrad_slices(g, kDienSplitIH1, 3 * D, D, BT, a.dGi1, 3 * D, rows, D, a.sWih1);
  g.p[g.n++] = make_gemm(kNN, BT, D, 3 * D, a.dGi1, 3 * D, w_flat + o.xw_ih, D, drows, D, nullptr, 0, nullptr, 0, false);
  g.p[g.n++] = make_colsum(a.dGi1, BT, 3 * D, 3 * D, g_ext + (o.xb - o.xw_ih), a.cs);
  static_assert(kDienSplitHH + kDienSplitIH1 + 2 <= kMaxGroup, "one grouped launch");
  if (int rc = launch_group(g, st)) return rc;
  if (int rc = launch_colsum_reduce(g, st)) return rc;
  const int64_t DD3 = 3ll * D * D;
  if (int rc = dien_fold_slices(a.sWhh1, n_hh, DD3, g_ext + (o.xw_hh - o.xw_ih), st)) return rc;
  return dien_fold_slices(a.sWih1, n_ih, DD3, g_ext, st);
}

int dien_run(DienDims& q, const DienOff& o, const float* w_flat, float* g_flat, float* bn, int update_running,
             const int64_t* seq, const int64_t* neg, const int64_t* cand, const float* label, int64_t B, int64_t C,
             float* logits_out, hiprec_stats* stats, Scratch* scratch, float* ws_base, hipStream_t st) {
  const bool train = g_flat != nullptr;
  const DienWs a = dien_carve_ws(ws_base, q, B, C, train, false);
  const DinTower& tw = q.tw;
  const int D = q.D, T = q.T;
  const int64_t BT = B * T, N = B * C;
  if (int rc = din_gather(w_flat, q.n_items, D, seq, cand, BT, N, a.rows, a.q, a.lv, a.lc, stats, st)) return rc;
  if (int rc = dien_extract_forward(q, o, w_flat, a, a.rows, B, train, a.h1, st)) return rc;
  if (int rc = dien_evolve_forward(q, o, w_flat, a, a.h1, a.q, B, C, train, a.hT, train ? a.a : nullptr, st)) return rc;
  if (int rc = din_z(a.hT, a.q, N, D, a.z, st)) return rc;
  if (int rc = din_tower_forward(tw, w_flat, bn, update_running, train, a.z, a.lc, N, logits_out, stats, st)) return rc;
  if (!train) return 0;

  const int n_cnt = static_cast<int>(std::min<int64_t>(kDienCountBlocks, (BT + kBlock - 1) / kBlock));
  dien_aux_count_kernel<<<n_cnt, kBlock, 0, st>>>(seq, neg, B, T, q.n_items, a.cnt, stats);
  HIPREC_TRY(hipGetLastError());
  const int n_aux = std::min(grid_for_waves(BT), 512);
  dien_aux_kernel<<<n_aux, kBlock, 0, st>>>(w_flat, a.h1, seq, neg, B, T, D, q.n_items, q.aux_w, a.cnt, n_cnt, a.dh1x, g_flat,
                                           a.lossp);
  HIPREC_TRY(hipGetLastError());
  float* dz = nullptr;
  if (int rc = din_tower_backward(tw, w_flat, g_flat, a.z, a.lc, label, N, logits_out, scratch, stats, st, &dz)) return rc;
  dien_aux_loss_kernel<<<1, kWave, 0, st>>>(a.lossp, n_aux, scratch);
  HIPREC_TRY(hipGetLastError());
  if (int rc = din_z_bwd(dz, a.hT, a.q, N, D, a.dhT, a.dqz, st)) return rc;
  const float* dh1a = nullptr;
  if (int rc = dien_evolve_backward(q, o, w_flat, a, a.h1, a.q, a.a, a.dhT, B, C, g_flat + o.att, a.dh1p, a.dqa, &dh1a, st))
    return rc;

  if (int rc = dien_extract_backward(q, o, w_flat, a, a.rows, dh1a, a.dh1p, a.dh1x, B, g_flat + o.xw_ih, a.drows, st)) return rc;
  return din_scatter(a.drows, a.dqz, a.dqa, seq, cand, a.lv, a.lc, BT, N, D, g_flat, st);
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_dien_shape_bytes(void) { return sizeof(hiprec_dien_shape); }

extern "C" int64_t hiprec_dien_param_floats(const hiprec_dien_shape* shape) {
  if (dien_check_shape(shape)) return -1;
  DienDims q = dien_dims(*shape);
  return dien_offsets(q).total;
}

extern "C" int hiprec_dien_tiles(const hiprec_dien_shape* shape, int64_t n_cand, int32_t* out) {
  if (int rc = dien_check_shape(shape)) return rc;
  HIPREC_REQUIRE(out && n_cand >= 1 && n_cand <= kDinMaxRows, "NULL pointer or n_cand out of range");
  const int D = shape->dim, T = shape->maxlen, C = static_cast<int>(n_cand);
  out[0] = kDienTile; out[1] = dien_slots(C); out[2] = dien_slabs(C); out[3] = kDienSplitHH;
  out[4] = dien_rows_res(D, T, kDienTile, false, false); out[5] = dien_rows_res(D, T, dien_slots(C), true, false);
  out[6] = dien_rows_res(D, T, kDienTile, false, true); out[7] = dien_rows_res(D, T, dien_slots(C), true, true);
  return 0;
}

extern "C" size_t hiprec_dien_workspace_bytes(const hiprec_dien_shape* shape, int64_t batch, int64_t n_cand, int32_t mode) {
  if (dien_check_shape(shape) || mode < 0 || mode > 5) return 0;
  DienDims q = dien_dims(*shape);
  if (mode & 4) {
    if (!dien_batch_ok(q, batch, 1, (mode & 1) != 0)) return 0;
    return sizeof(float) * static_cast<size_t>(dien_carve_extract(nullptr, q, batch, (mode & 1) != 0).floats);
  }
  if (!dien_batch_ok(q, batch, n_cand, (mode & 1) != 0)) return 0;
  return sizeof(float) * static_cast<size_t>(dien_carve_ws(nullptr, q, batch, n_cand, (mode & 1) != 0, (mode & 2) != 0).floats);
}

static int dien_call(const hiprec_dien_shape* shape, const float* w_flat, float* g_flat, float* running, int32_t update_running,
                     const int64_t* seq, const int64_t* neg, const int64_t* cand, const float* label, int64_t batch,
                     int64_t n_cand, float* logits_out, hiprec_stats* stats, void* scratch, void* workspace,
                     size_t workspace_bytes, void* stream) {
  if (int rc = dien_check_shape(shape)) return rc;
  DienDims q = dien_dims(*shape);
  HIPREC_REQUIRE(w_flat && running && seq && cand && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(dien_batch_ok(q, batch, n_cand, g_flat != nullptr),
                 "DIEN needs batch >= 1, n_cand >= 1, batch * maxlen <= 2^24, batch * n_cand <= 2^24 and, training, batch * "
                 "n_cand * maxlen <= 2^24 (got %lld, %lld)", static_cast<long long>(batch), static_cast<long long>(n_cand));
  const size_t need = hiprec_dien_workspace_bytes(shape, batch, n_cand, g_flat != nullptr);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  const DienOff o = dien_offsets(q);
  return dien_run(q, o, w_flat, g_flat, running, update_running, seq, neg, cand, label, batch, n_cand, logits_out, stats,
                  static_cast<Scratch*>(scratch), static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_dien_grad(const hiprec_dien_shape* shape, const float* w_flat, float* g_flat, float* running,
                                int32_t update_running, const int64_t* seq, const int64_t* neg_seq, const int64_t* cand,
                                const float* label, int64_t batch, int64_t n_cand, float* logits_out, hiprec_stats* stats,
                                void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  HIPREC_REQUIRE(g_flat && neg_seq && label && scratch, "training needs the gradient buffer, neg_seq, the labels and the scratch block");
  if (scratch_bytes < kScratchBytes) {
    set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
    return HIPREC_E_SCRATCH;
  }
  return dien_call(shape, w_flat, g_flat, running, update_running, seq, neg_seq, cand, label, batch, n_cand, logits_out, stats,
                   scratch, workspace, workspace_bytes, stream);
}

extern "C" int hiprec_dien_score(const hiprec_dien_shape* shape, const float* w_flat, float* running, const int64_t* seq,
                                 const int64_t* cand, int64_t batch, int64_t n_cand, float* logits_out, hiprec_stats* stats,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  HIPREC_REQUIRE(logits_out, "scoring needs the logits buffer");
  return dien_call(shape, w_flat, nullptr, running, 0, seq, nullptr, cand, nullptr, batch, n_cand, logits_out, stats, nullptr,
                   workspace, workspace_bytes, stream);
}

extern "C" int hiprec_dien_evolve(const hiprec_dien_shape* shape, const float* w_flat, const float* h1, const float* q_rows,
                                  const uint8_t* mask, int64_t batch, int64_t n_cand, float* hT, float* a, const float* dhT,
                                  float* g_att, float* dh1, float* dq, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = dien_check_shape(shape)) return rc;
  DienDims q = dien_dims(*shape);
  const bool bwd = dhT != nullptr;
  HIPREC_REQUIRE(w_flat && h1 && q_rows && mask && hT && a && workspace, "NULL pointer");
  HIPREC_REQUIRE(dien_batch_ok(q, batch, n_cand, bwd), "DIEN: batch or n_cand out of range");
  HIPREC_REQUIRE(!bwd || (g_att && dh1 && dq), "the stage's backward needs g_att, dh1 and dq");
  const size_t need = hiprec_dien_workspace_bytes(shape, batch, n_cand, bwd ? 3 : 2);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const DienOff o = dien_offsets(q);
  const DienWs w = dien_carve_ws(static_cast<float*>(workspace), q, batch, n_cand, bwd, true);
  const int64_t BT = batch * q.T, N = batch * n_cand;
  if (int rc = din_flags(mask, w.lv, BT, w.lc, N, st)) return rc;
  if (int rc = dien_evolve_forward(q, o, w_flat, w, h1, q_rows, batch, n_cand, bwd, hT, a, st)) return rc;
  if (!bwd) return 0;
  const float* dh1a = nullptr;
  if (int rc = dien_evolve_backward(q, o, w_flat, w, h1, q_rows, a, dhT, batch, n_cand, g_att, dh1, dq, &dh1a, st)) return rc;
  return din_add(dh1, dh1a, BT * q.D, st);
}

extern "C" int hiprec_dien_extract(const hiprec_dien_shape* shape, const float* w_flat, const float* x, const uint8_t* mask,
                                   int64_t batch, float* h1, const float* dh1, float* g_ext, float* dx, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (int rc = dien_check_shape(shape)) return rc;
  DienDims q = dien_dims(*shape);
  const bool bwd = dh1 != nullptr;
  HIPREC_REQUIRE(w_flat && x && mask && h1 && workspace, "NULL pointer");
  HIPREC_REQUIRE(dien_batch_ok(q, batch, 1, bwd), "DIEN: batch out of range");
  HIPREC_REQUIRE(!bwd || (g_ext && dx), "the stage's backward needs g_ext and dx");
  const size_t need = hiprec_dien_workspace_bytes(shape, batch, 1, bwd ? 5 : 4);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const DienOff o = dien_offsets(q);
  const DienWs w = dien_carve_extract(static_cast<float*>(workspace), q, batch, bwd);
  if (int rc = din_flags(mask, w.lv, batch * q.T, nullptr, 0, st)) return rc;
  if (int rc = dien_extract_forward(q, o, w_flat, w, x, batch, bwd, h1, st)) return rc;
  if (!bwd) return 0;
  return dien_extract_backward(q, o, w_flat, w, x, dh1, nullptr, nullptr, batch, g_ext, dx, st);
}
