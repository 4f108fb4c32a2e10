// TiSASRec (beta_rec/models/tisasrec.py): zero_grad + forward + loss + backward of TiSASRecEngine.train_single_batch
// as a fixed sequence of launches, no host sync.  Activations are [M = B * T, D] row-major, row m = b * T + t.
//
// What differs from SASRec (csrc/sasrec.hip): no positional row on x and no output projection; three separate
// Linear(D, D) for Q / K / V; the absolute positions enter as keys and values (K' = K + drop(PK), V' = V + drop(PV),
// folded into the projected k | v once per block); and every (query i, key j) pair carries a row of two small tables
// [time_span + 1, D] selected by the integer time_matrix[b, i, j]:
//     S[i, j] = Q_i . (K'_j + drop(EK[tm[i, j]])) / sqrt(hd)        O_i = sum_j P[i, j] (V'_j + drop(EV[tm[i, j]]))
// The gathered [B, T, T, D] tensors of the reference are never made: the head's slice of one table sits in LDS
// (stride hd + 1, so that lanes gathering different rows hit different banks) next to the block's score rows.
//
//   forward   per (sequence, head, query tile): Q K'^T on the fp32 MFMA, + the gathered dot products, softmax (a
//             padded QUERY row is skipped: zeros, as nothing downstream reads it), P V' on the MFMA + the gathered sum
//   backward  per (sequence, head), ONE LAUNCH PER QUERY TILE in ascending order: dP and S are rebuilt row-complete in
//             LDS (first with EV resident, then with EK), then dQ, this tile's part of dK' / dV' (stored for the keys
//             the tile is the first to reach, added for the earlier ones: a (sequence, head) owns its columns, and the
//             launches are ordered, so there is no atomic and no race) and this tile's part of the two time tables'
//             gradient: the table slice in LDS becomes the accumulator, thread (column c, residue g) owns the rows
//             t = g mod (256 / hd) and scans the tile's (i, j) pairs in order.  Per-sequence slabs [B, span + 1, D]
//             are then summed over b by one thread per element, in order.
//
// LayerNorm, the loss stage, the norm prep, the embed, the feed-forward GEMM groups and the attention's MFMA / tile
// helpers are shared with SASRec: csrc/seqrec.hpp, csrc/seqrec.hip.
#include <vector>

#include "gemm.hpp"
#include "seqrec.hpp"

namespace hiprec {
namespace {

constexpr int kTisMaxSpan = 256;     // (span + 1) x (64 + 1) fp32 = 66.8 KB of the 160 KB LDS
constexpr int kTisSLd = kSeqMaxLen + 4;   // leading dimension of the score rows in LDS
constexpr int kTisFixedKeep = 5;          // embedding, abs-pos-K, abs-pos-V, time-K, time-V

// ---- time matrix ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void tis_check_tm_kernel(const int32_t* __restrict__ tm, int64_t n, int span,
                                                              hiprec_stats* stats) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  bool bad = false;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int32_t t = tm[i];
    bad |= t < 0 || t > span;
  }
  if (bad) atomicOr(&stats->status, HIPREC_STATUS_ROW_OOB);
}

// an entry outside [0, span] has raised the status word already (tis_check_tm_kernel); it never indexes out of range
__device__ __forceinline__ int tis_row(int32_t t, int span) { return min(max(t, 0), span); }

__global__ __launch_bounds__(kBlock) void tis_time_relation_kernel(const int64_t* __restrict__ ts, int64_t B, int T,
                                                                   int span, int32_t* __restrict__ out) {
  const int64_t n = B * T * T, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
    const int64_t bi = e / T;
    const int j = static_cast<int>(e - bi * T);
    const int64_t b = bi / T;
    const int64_t d = ts[bi] - ts[b * T + j];
    const int64_t a = d < 0 ? -d : d;
    out[e] = static_cast<int32_t>(a > span ? span : a);
  }
}

// d item_emb[seq] += dx * keep * sqrt(D) (row atomics, id 0 skipped); there is no positional row to differentiate
__global__ __launch_bounds__(kBlock) void tis_embed_bwd_kernel(const float* __restrict__ dx,
                                                               const int64_t* __restrict__ seq, int64_t M, int D,
                                                               int64_t n_items, float sqrt_d,
                                                               const uint8_t* __restrict__ keep, float ks,
                                                               float* __restrict__ g_item) {
  const int64_t n = M * D, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t m = i / D;
    const int64_t id = seq[m];
    if (id <= 0 || id > n_items) continue;
    float gv = dx[i];
    if (keep) gv = keep[i] ? gv * ks : 0.f;
    atomic_add_f32(g_item + id * D + (i - m * D), gv * sqrt_d);
  }
}

// k | v of qkv [M, 3D] += the dropped-out absolute-position rows: K' = K + PK[t] * keep, V' = V + PV[t] * keep
__global__ __launch_bounds__(kBlock) void tis_pos_fwd_kernel(float* __restrict__ qkv, const float* __restrict__ PK,
                                                             const float* __restrict__ PV, int64_t M, int T, int D,
                                                             const uint8_t* __restrict__ keep_k,
                                                             const uint8_t* __restrict__ keep_v, float ks) {
  const int64_t n = M * D, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t m = i / D;
    const int d = static_cast<int>(i - m * D);
    const int64_t p = static_cast<int64_t>(m % T) * D + d;
    float pk = PK[p], pv = PV[p];
    if (keep_k) pk = keep_k[i] ? pk * ks : 0.f;
    if (keep_v) pv = keep_v[i] ? pv * ks : 0.f;
    qkv[m * 3 * D + D + d] += pk;
    qkv[m * 3 * D + 2 * D + d] += pv;
  }
}

// d PK[t] += sum_b dK'[b, t] * keep, d PV likewise: one thread per (t, d) walks the batch in order
__global__ __launch_bounds__(kBlock) void tis_pos_bwd_kernel(const float* __restrict__ dqkv, int64_t B, int T, int D,
                                                             const uint8_t* __restrict__ keep_k,
                                                             const uint8_t* __restrict__ keep_v, float ks,
                                                             float* __restrict__ g_pk, float* __restrict__ g_pv) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= T * D) return;
  const int t = e / D, d = e - t * D;
  float ak = 0.f, av = 0.f;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t m = b * T + t;
    float gk = dqkv[m * 3 * D + D + d], gv = dqkv[m * 3 * D + 2 * D + d];
    if (keep_k) gk = keep_k[m * D + d] ? gk * ks : 0.f;
    if (keep_v) gv = keep_v[m * D + d] ? gv * ks : 0.f;
    ak += gk;
    av += gv;
  }
  g_pk[e] += ak;
  g_pv[e] += av;
}

// the time tables' gradient: the per-sequence slabs [B, rows * D] summed over b in order, one thread per element
__global__ __launch_bounds__(kBlock) void tis_table_reduce_kernel(const float* __restrict__ slab_k,
                                                                  const float* __restrict__ slab_v, int64_t B,
                                                                  int64_t n, float* __restrict__ g_k,
                                                                  float* __restrict__ g_v) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= n) return;
  float ak = 0.f, av = 0.f;
  for (int64_t b = 0; b < B; ++b) {
    ak += slab_k[b * n + e];
    av += slab_v[b * n + e];
  }
  g_k[e] += ak;
  g_v[e] += av;
}

// ---- time-interval-aware causal attention ------------------------------------------------------------------------------
// the head's slice of a [span + 1, D] table into tab[span + 1][HD + 1]
template <int HD>
__device__ __forceinline__ void tis_load_table(float* tab, const float* __restrict__ E, int D, int h, int span) {
  for (int e = threadIdx.x; e < (span + 1) * HD; e += kBlock) {
    const int r = e / HD, c = e - r * HD;
    tab[r * (HD + 1) + c] = E[static_cast<int64_t>(r) * D + h * HD + c];
  }
}

// sum_c a[c] * row[c] over the head's HD columns, through HD keep bytes (16-byte aligned) when kp != NULL
template <int HD>
__device__ __forceinline__ float tis_dot(const float* a, const float* row, const uint8_t* __restrict__ kp, float ks) {
  float s = 0.f;
  if (kp == nullptr) {
#pragma unroll
    for (int c = 0; c < HD; ++c) s += a[c] * row[c];
    return s;
  }
  const uint4* kv = reinterpret_cast<const uint4*>(kp);
#pragma unroll
  for (int q = 0; q < HD / 16; ++q) {
    const uint4 w = kv[q];
    const uint32_t words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if ((words[k >> 2] >> (8 * (k & 3))) & 0xffu) s += a[q * 16 + k] * row[q * 16 + k];
  }
  return s * ks;
}

template <int HD>
struct TisTile {
  static constexpr int kQT = HD == 64 ? 16 : 32;      // query rows a block owns: 16 at hd 64, so that the table slice,
  static constexpr int kRowTiles = kQT / 16;          // two row-complete buffers and the tiles fit 160 KB at span 256
  static constexpr int kColTiles = HD / 16;
  static constexpr int kGroups = kBlock / HD;         // residue classes of table rows in the table-gradient scan
};

static size_t tis_fwd_lds(int hd, int span) {
  const int qt = hd == 64 ? 16 : 32;
  return sizeof(float) * (static_cast<size_t>(qt + 64) * (hd + 1) + static_cast<size_t>(qt) * kTisSLd +
                          static_cast<size_t>(span + 1) * (hd + 1));
}

static size_t tis_bwd_lds(int hd, int span) {
  const int qt = hd == 64 ? 16 : 32;
  return sizeof(float) * (static_cast<size_t>(2 * qt + 64) * (hd + 1) + 2 * static_cast<size_t>(qt) * kTisSLd +
                          static_cast<size_t>(span + 1) * (hd + 1) + 3 * qt) +
         sizeof(uint16_t) * static_cast<size_t>(qt) * kSeqMaxLen;
}

// grid (B * H, ceil(T / QT)).  qkv [M, 3D]: q | k' | v'.  keep_a [H * B, T, T] (the reference's head-major layout),
// keep_tk / keep_tv [B, T, T, D].  lse [B * H, T] with bh = b * H + h.
template <int HD>
__global__ __launch_bounds__(kBlock) void tis_attn_fwd_kernel(
    const float* __restrict__ qkv, const int64_t* __restrict__ seq, const int32_t* __restrict__ tm,
    const float* __restrict__ EK, const float* __restrict__ EV, int B, int T, int H, int D, int span,
    const uint8_t* __restrict__ keep_a, const uint8_t* __restrict__ keep_tk, const uint8_t* __restrict__ keep_tv,
    float ks, float* __restrict__ O, float* __restrict__ lse) {
  constexpr int QT = TisTile<HD>::kQT, LD = HD + 1;
  extern __shared__ float tis_smem[];
  float* Qs = tis_smem;                 // [QT][LD]; the gathered part of O later
  float* Ks = Qs + QT * LD;             // [64][LD]
  float* S = Ks + 64 * LD;              // [QT][kTisSLd]
  float* tab = S + QT * kTisSLd;        // [span + 1][LD]
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int q0 = blockIdx.y * QT;
  const int lane = lane_id(), wave = wave_in_block();
  const int64_t ld = 3 * D;
  const float* base = qkv + static_cast<int64_t>(b) * T * ld + h * HD;
  const int64_t* seq_b = seq + static_cast<int64_t>(b) * T;
  const int32_t* tm_b = tm + static_cast<int64_t>(b) * T * T;
  const float scale = 1.0f / sqrtf(static_cast<float>(HD));
  load_tile<HD>(Qs, base, ld, q0, QT, T, scale);
  tis_load_table<HD>(tab, EK, D, h, span);
  const int n_keys = min(T, q0 + QT);
  const int n_chunks = (n_keys + 63) / 64;
  const int width = n_chunks * 64;
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * 64;
    __syncthreads();
    load_tile<HD>(Ks, base + D, ld, j0, 64, n_keys, 1.f);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < TisTile<HD>::kRowTiles; ++u) {
      const int tile = wave * TisTile<HD>::kRowTiles + u, rt = tile >> 2, ct = tile & 3;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = mma16(acc, Qs + rt * 16 * LD, LD, 1, Ks + ct * 16 * LD, 1, LD, HD);
#pragma unroll
      for (int r = 0; r < 4; ++r) S[(rt * 16 + 4 * (lane >> 4) + r) * kTisSLd + j0 + ct * 16 + (lane & 15)] = acc[r];
    }
  }
  __syncthreads();
  // + Q_i . drop(EK[tm[i, j]]) / sqrt(hd): one (i, j) pair per thread, the keys of a row across the lanes
  for (int e = threadIdx.x; e < QT * n_keys; e += kBlock) {
    const int r = e / n_keys, j = e - r * n_keys, i = q0 + r;
    if (i >= T || j > i || seq_b[i] == 0) continue;
    const int t = tis_row(tm_b[static_cast<int64_t>(i) * T + j], span);
    const uint8_t* kp =
        keep_tk ? keep_tk + ((static_cast<int64_t>(b) * T + i) * T + j) * D + h * HD : nullptr;
    S[r * kTisSLd + j] += tis_dot<HD>(Qs + r * LD, tab + t * LD, kp, ks);
  }
  __syncthreads();
  for (int rr = 0; rr < QT / kWavesPerBlock; ++rr) {
    const int row = wave * (QT / kWavesPerBlock) + rr, i = q0 + row;
    float* Sr = S + row * kTisSLd;
    if (i >= T || seq_b[i] == 0) {      // past the sequence, or a padded query: zeros (nothing reads its output)
      for (int j = lane; j < width; j += 64) Sr[j] = 0.f;
      if (i < T && lane == 0) lse[static_cast<int64_t>(bh) * T + i] = 0.f;
      continue;
    }
    float mx = -INFINITY;
    for (int j = lane; j <= i; j += 64) mx = fmaxf(mx, Sr[j]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j <= i; j += 64) {
      const float ex = expf(Sr[j] - mx);
      Sr[j] = ex;
      sum += ex;
    }
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
    const uint8_t* kp = keep_a ? keep_a + ((static_cast<int64_t>(h) * B + b) * T + i) * T : nullptr;
    for (int j = lane; j < width; j += 64) {
      float p = 0.f;
      if (j <= i) {
        p = Sr[j] * inv;
        if (kp) p = kp[j] ? p * ks : 0.f;
      }
      Sr[j] = p;
    }
    if (lane == 0) lse[static_cast<int64_t>(bh) * T + i] = mx + logf(sum);
  }
  __syncthreads();
  tis_load_table<HD>(tab, EV, D, h, span);
  constexpr int kTiles = TisTile<HD>::kRowTiles * TisTile<HD>::kColTiles;    // <= 4: one per wave
  const int rt = wave / TisTile<HD>::kColTiles, ct = wave - rt * TisTile<HD>::kColTiles;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * 64;
    __syncthreads();
    load_tile<HD>(Ks, base + 2 * D, ld, j0, 64, n_keys, 1.f);
    __syncthreads();
    if (wave < kTiles) acc = mma16(acc, S + rt * 16 * kTisSLd + j0, kTisSLd, 1, Ks + ct * 16, LD, 1, 64);
  }
  // + sum_j P[i, j] drop(EV[tm[i, j]]): lane = column, the rows over the 256 / HD groups, j in order
  {
    const int c = threadIdx.x % HD, g = threadIdx.x / HD;
    for (int r = g; r < QT; r += TisTile<HD>::kGroups) {
      const int i = q0 + r;
      float o = 0.f;
      if (i < T && seq_b[i] != 0) {
        const float* Sr = S + r * kTisSLd;
        const int32_t* tr = tm_b + static_cast<int64_t>(i) * T;
        const uint8_t* kp = keep_tv ? keep_tv + (static_cast<int64_t>(b) * T + i) * T * D + h * HD + c : nullptr;
        for (int j = 0; j <= i; ++j) {
          float v = tab[tis_row(tr[j], span) * LD + c];
          if (kp) v = kp[static_cast<int64_t>(j) * D] ? v * ks : 0.f;
          o += Sr[j] * v;
        }
      }
      Qs[r * LD + c] = o;
    }
  }
  __syncthreads();
  if (wave < kTiles) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rt * 16 + 4 * (lane >> 4) + r, col = ct * 16 + (lane & 15), i = q0 + row;
      if (i < T) O[(static_cast<int64_t>(b) * T + i) * D + h * HD + col] = acc[r] + Qs[row * LD + col];
    }
  }
}

// backward of one query tile (blockIdx.x = sequence * H + head; tile = the launch's).  Writes the q third of dqkv
// [M, 3D] for the tile's rows, stores (keys >= q0) or adds (keys < q0) the tile's part of the k' | v' thirds, and adds
// the tile's part of the two time-table gradients to this sequence's slab [span + 1, D] (columns of this head).
template <int HD>
__global__ __launch_bounds__(kBlock) void tis_attn_bwd_kernel(
    const float* __restrict__ qkv, const float* __restrict__ dO, const float* __restrict__ O,
    const float* __restrict__ lse, const int64_t* __restrict__ seq, const int32_t* __restrict__ tm,
    const float* __restrict__ EK, const float* __restrict__ EV, int B, int T, int H, int D, int span, int tile,
    const uint8_t* __restrict__ keep_a, const uint8_t* __restrict__ keep_tk, const uint8_t* __restrict__ keep_tv,
    float ks, float* __restrict__ dqkv, float* __restrict__ slab_k, float* __restrict__ slab_v) {
  constexpr int QT = TisTile<HD>::kQT, LD = HD + 1, G = TisTile<HD>::kGroups;
  extern __shared__ float tis_smem[];
  float* Qs = tis_smem;                    // [QT][LD] q / sqrt(hd)
  float* Gs = Qs + QT * LD;                // [QT][LD] dO
  float* Ks = Gs + QT * LD;                // [64][LD] a chunk of k' or v'; the gathered part of dQ at the end
  float* DS = Ks + 64 * LD;                // [QT][kTisSLd] dP, then dS
  float* PD = DS + QT * kTisSLd;           // [QT][kTisSLd] S, then P through the attention keep bytes
  float* tab = PD + QT * kTisSLd;          // [span + 1][LD] EV, EK, then the accumulator of each table's gradient
  float* s_lse = tab + (span + 1) * LD;    // [QT]
  float* s_delta = s_lse + QT;             // [QT]
  float* s_live = s_delta + QT;            // [QT] 1 = a real query row of the sequence
  uint16_t* tms = reinterpret_cast<uint16_t*>(s_live + QT);   // [QT][kSeqMaxLen] table rows of the tile's pairs
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int q0 = tile * QT;
  const int lane = lane_id(), wave = wave_in_block();
  const int64_t ld = 3 * D;
  const float* base = qkv + static_cast<int64_t>(b) * T * ld + h * HD;
  const float* g_base = dO + static_cast<int64_t>(b) * T * D + h * HD;
  const float* o_base = O + static_cast<int64_t>(b) * T * D + h * HD;
  const int64_t* seq_b = seq + static_cast<int64_t>(b) * T;
  const int32_t* tm_b = tm + static_cast<int64_t>(b) * T * T;
  const float scale = 1.0f / sqrtf(static_cast<float>(HD));
  const int n_keys = min(T, q0 + QT);
  const int n_chunks = (n_keys + 63) / 64;
  const int width = n_chunks * 64;
  load_tile<HD>(Qs, base, ld, q0, QT, T, scale);
  load_tile<HD>(Gs, g_base, D, q0, QT, T, 1.f);
  tis_load_table<HD>(tab, EV, D, h, span);
  for (int e = threadIdx.x; e < QT * n_keys; e += kBlock) {
    const int r = e / n_keys, j = e - r * n_keys, i = q0 + r;
    tms[r * kSeqMaxLen + j] = i < T ? static_cast<uint16_t>(tis_row(tm_b[static_cast<int64_t>(i) * T + j], span)) : 0;
  }
  __syncthreads();
  if (threadIdx.x < QT * 8) {                 // delta = rowsum(dO * O), 8 threads per row
    const int row = threadIdx.x >> 3, part = threadIdx.x & 7, i = q0 + row;
    float s = 0.f;
    if (i < T)
      for (int c = part; c < HD; c += 8) s += Gs[row * LD + c] * o_base[static_cast<int64_t>(i) * D + c];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (part == 0) {
      const bool live = i < T && seq_b[i] != 0;
      s_delta[row] = s;
      s_lse[row] = live ? lse[static_cast<int64_t>(bh) * T + i] : 0.f;
      s_live[row] = live ? 1.f : 0.f;
    }
  }
  // pass 1 (EV resident): dP[i, j] = dO_i . (V'_j + drop(EV[tm[i, j]]))
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * 64;
    __syncthreads();
    load_tile<HD>(Ks, base + 2 * D, ld, j0, 64, n_keys, 1.f);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < TisTile<HD>::kRowTiles; ++u) {
      const int tl = wave * TisTile<HD>::kRowTiles + u, rt = tl >> 2, ct = tl & 3;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = mma16(acc, Gs + rt * 16 * LD, LD, 1, Ks + ct * 16 * LD, 1, LD, HD);
#pragma unroll
      for (int r = 0; r < 4; ++r) DS[(rt * 16 + 4 * (lane >> 4) + r) * kTisSLd + j0 + ct * 16 + (lane & 15)] = acc[r];
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < QT * n_keys; e += kBlock) {
    const int r = e / n_keys, j = e - r * n_keys, i = q0 + r;
    if (j > i || s_live[r] == 0.f) continue;
    const uint8_t* kp =
        keep_tv ? keep_tv + ((static_cast<int64_t>(b) * T + i) * T + j) * D + h * HD : nullptr;
    DS[r * kTisSLd + j] += tis_dot<HD>(Gs + r * LD, tab + tms[r * kSeqMaxLen + j] * LD, kp, ks);
  }
  __syncthreads();
  // pass 2 (EK resident): S, P = exp(S - lse), dS = P * (dP through the keep bytes - delta)
  tis_load_table<HD>(tab, EK, D, h, span);
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * 64;
    __syncthreads();
    load_tile<HD>(Ks, base + D, ld, j0, 64, n_keys, 1.f);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < TisTile<HD>::kRowTiles; ++u) {
      const int tl = wave * TisTile<HD>::kRowTiles + u, rt = tl >> 2, ct = tl & 3;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = mma16(acc, Qs + rt * 16 * LD, LD, 1, Ks + ct * 16 * LD, 1, LD, HD);
#pragma unroll
      for (int r = 0; r < 4; ++r) PD[(rt * 16 + 4 * (lane >> 4) + r) * kTisSLd + j0 + ct * 16 + (lane & 15)] = acc[r];
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < QT * width; e += kBlock) {
    const int r = e / width, j = e - r * width, i = q0 + r;
    float ds = 0.f, pd = 0.f;
    if (j <= i && s_live[r] != 0.f) {
      const uint8_t* kp =
          keep_tk ? keep_tk + ((static_cast<int64_t>(b) * T + i) * T + j) * D + h * HD : nullptr;
      const float s = PD[r * kTisSLd + j] + tis_dot<HD>(Qs + r * LD, tab + tms[r * kSeqMaxLen + j] * LD, kp, ks);
      const float p = expf(s - s_lse[r]);
      float d = DS[r * kTisSLd + j];
      pd = p;
      if (keep_a) {
        const bool kept = keep_a[((static_cast<int64_t>(h) * B + b) * T + i) * T + j] != 0;
        d = kept ? d * ks : 0.f;
        pd = kept ? p * ks : 0.f;
      }
      ds = p * (d - s_delta[r]);
    }
    DS[r * kTisSLd + j] = ds;
    PD[r * kTisSLd + j] = pd;
  }
  // pass 3: dQ = dS (K' + drop(EK[tm])) / sqrt(hd); this tile's dK' = dS^T q / sqrt(hd) and dV' = P^T dO
  constexpr int kTiles = TisTile<HD>::kRowTiles * TisTile<HD>::kColTiles;    // <= 4: one per wave
  const int qrt = wave / TisTile<HD>::kColTiles, qct = wave - qrt * TisTile<HD>::kColTiles;
  f32x4 acc_q = {0.f, 0.f, 0.f, 0.f};
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * 64;
    __syncthreads();
    load_tile<HD>(Ks, base + D, ld, j0, 64, n_keys, 1.f);
    __syncthreads();
    if (wave < kTiles) acc_q = mma16(acc_q, DS + qrt * 16 * kTisSLd + j0, kTisSLd, 1, Ks + qct * 16, LD, 1, 64);
    for (int tl = wave; tl < 4 * TisTile<HD>::kColTiles; tl += kWavesPerBlock) {
      const int jt = tl / TisTile<HD>::kColTiles, ct = tl - jt * TisTile<HD>::kColTiles;
      f32x4 ak = {0.f, 0.f, 0.f, 0.f}, av = {0.f, 0.f, 0.f, 0.f};
      ak = mma16(ak, DS + j0 + jt * 16, 1, kTisSLd, Qs + ct * 16, LD, 1, QT);
      av = mma16(av, PD + j0 + jt * 16, 1, kTisSLd, Gs + ct * 16, LD, 1, QT);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + jt * 16 + 4 * (lane >> 4) + r;
        if (j < n_keys) {
          float* out = dqkv + (static_cast<int64_t>(b) * T + j) * ld + h * HD + ct * 16 + (lane & 15);
          if (j >= q0) {
            out[D] = ak[r];
            out[2 * D] = av[r];
          } else {
            out[D] += ak[r];
            out[2 * D] += av[r];
          }
        }
      }
    }
  }
  __syncthreads();
  {
    const int c = threadIdx.x % HD, g = threadIdx.x / HD;
    for (int r = g; r < QT; r += G) {
      const int i = q0 + r;
      float o = 0.f;
      if (s_live[r] != 0.f) {
        const uint8_t* kp = keep_tk ? keep_tk + (static_cast<int64_t>(b) * T + i) * T * D + h * HD + c : nullptr;
        for (int j = 0; j <= i; ++j) {
          float v = tab[tms[r * kSeqMaxLen + j] * LD + c];
          if (kp) v = kp[static_cast<int64_t>(j) * D] ? v * ks : 0.f;
          o += DS[r * kTisSLd + j] * v;
        }
      }
      Ks[r * LD + c] = o;
    }
  }
  __syncthreads();
  if (wave < kTiles) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = qrt * 16 + 4 * (lane >> 4) + r, col = qct * 16 + (lane & 15), i = q0 + row;
      if (i < T) dqkv[(static_cast<int64_t>(b) * T + i) * ld + h * HD + col] = (acc_q[r] + Ks[row * LD + col]) * scale;
    }
  }
  // pass 4: the time tables' gradients.  The slice becomes the accumulator (this sequence's slab so far); thread
  // (column c, residue g) owns the rows t = g mod G and scans the tile's pairs in (i, j) order: no atomics.
  for (int which = 0; which < 2; ++which) {
    float* slab = (which == 0 ? slab_k : slab_v) + static_cast<int64_t>(b) * (span + 1) * D + h * HD;
    const float* coef = which == 0 ? DS : PD;        // dS / sqrt(hd) rides in Qs; P through the keep bytes
    const float* vec = which == 0 ? Qs : Gs;
    const uint8_t* keep_t = which == 0 ? keep_tk : keep_tv;
    __syncthreads();
    for (int e = threadIdx.x; e < (span + 1) * HD; e += kBlock) {
      const int r = e / HD, c = e - r * HD;
      tab[r * LD + c] = slab[static_cast<int64_t>(r) * D + c];
    }
    __syncthreads();
    const int c = threadIdx.x % HD, g = threadIdx.x / HD;
    for (int r = 0; r < QT; ++r) {
      if (s_live[r] == 0.f) continue;
      const int i = q0 + r;
      const float vr = vec[r * LD + c];
      const uint8_t* kp = keep_t ? keep_t + (static_cast<int64_t>(b) * T + i) * T * D + h * HD + c : nullptr;
      for (int j = 0; j <= i; ++j) {
        const int t = tms[r * kSeqMaxLen + j];
        if ((t & (G - 1)) != g) continue;
        float v = coef[r * kTisSLd + j] * vr;
        if (kp) v = kp[static_cast<int64_t>(j) * D] ? v * ks : 0.f;
        tab[t * LD + c] += v;
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < (span + 1) * HD; e += kBlock) {
      const int r = e / HD, cc = e - r * HD;
      slab[static_cast<int64_t>(r) * D + cc] = tab[r * LD + cc];
    }
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------
struct TisParams {      // pointers into a flat buffer laid out in state_dict() order
  float *item_emb, *pos_k, *pos_v, *time_k, *time_v, *last_w, *last_b;
  std::vector<float*> ln_a_w, ln_a_b, q_w, q_b, k_w, k_b, v_w, v_b, ln_f_w, ln_f_b, c1_w, c1_b, c2_w, c2_b;
};

static int64_t tis_n_params(const hiprec_tisasrec_shape& s) {
  const int64_t D = s.dim;
  return (s.n_items + 1) * D + 2 * static_cast<int64_t>(s.maxlen) * D + 2 * static_cast<int64_t>(s.time_span + 1) * D +
         s.n_blocks * (5 * D * D + 9 * D) + 2 * D;
}

static TisParams tis_params(float* base, const hiprec_tisasrec_shape& s) {
  TisParams p;
  const int64_t D = s.dim;
  const int nb = s.n_blocks;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += n; return r; };
  p.item_emb = take((s.n_items + 1) * D);
  p.pos_k = take(static_cast<int64_t>(s.maxlen) * D);
  p.pos_v = take(static_cast<int64_t>(s.maxlen) * D);
  p.time_k = take(static_cast<int64_t>(s.time_span + 1) * D);
  p.time_v = take(static_cast<int64_t>(s.time_span + 1) * D);
  for (int k = 0; k < nb; ++k) { p.ln_a_w.push_back(take(D)); p.ln_a_b.push_back(take(D)); }
  for (int k = 0; k < nb; ++k) {
    p.q_w.push_back(take(D * D)); p.q_b.push_back(take(D));
    p.k_w.push_back(take(D * D)); p.k_b.push_back(take(D));
    p.v_w.push_back(take(D * D)); p.v_b.push_back(take(D));
  }
  for (int k = 0; k < nb; ++k) { p.ln_f_w.push_back(take(D)); p.ln_f_b.push_back(take(D)); }
  for (int k = 0; k < nb; ++k) {
    p.c1_w.push_back(take(D * D)); p.c1_b.push_back(take(D));
    p.c2_w.push_back(take(D * D)); p.c2_b.push_back(take(D));
  }
  p.last_w = take(D);
  p.last_b = take(D);
  return p;
}

struct TisWorkspace {
  std::vector<float*> x, qn, qkv, o, f, h1, mean_a, rstd_a, mean_f, rstd_f, lse;
  float *x_last, *feats, *mean_l, *rstd_l, *z, *t[8], *dqkv, *aux, *cs, *slab_k, *slab_v;
  int64_t cs_each, slab_floats, floats;
};

static TisWorkspace tis_carve(float* base, const hiprec_tisasrec_shape& s, int64_t B, int T) {
  TisWorkspace w;
  const int64_t M = B * T, MD = M * s.dim, MH = M * s.heads;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += (n + 3) / 4 * 4; return r; };
  for (int k = 0; k < s.n_blocks; ++k) {
    w.x.push_back(take(MD)); w.qn.push_back(take(MD)); w.qkv.push_back(take(3 * MD)); w.o.push_back(take(MD));
    w.f.push_back(take(MD)); w.h1.push_back(take(MD));
    w.mean_a.push_back(take(M)); w.rstd_a.push_back(take(M)); w.mean_f.push_back(take(M)); w.rstd_f.push_back(take(M));
    w.lse.push_back(take(MH));
  }
  w.x_last = take(MD); w.feats = take(MD); w.mean_l = take(M); w.rstd_l = take(M); w.z = take(MD);
  for (int i = 0; i < 8; ++i) w.t[i] = take(MD);
  w.dqkv = take(3 * MD);
  w.aux = take(kSeqAux);
  w.cs_each = colsum_ws_floats(static_cast<int>(M), s.dim);
  w.cs = take(3 * w.cs_each);
  w.slab_floats = B * static_cast<int64_t>(s.time_span + 1) * s.dim;     // one [span + 1, D] slab per sequence
  w.slab_k = take(w.slab_floats);
  w.slab_v = take(w.slab_floats);
  w.floats = c - base;
  return w;
}

static int tis_check_shape(const hiprec_tisasrec_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  if (int rc = seq_check_shape("TiSASRec", s->n_items, s->n_blocks, s->heads, s->maxlen, s->dim)) return rc;
  HIPREC_REQUIRE(s->time_span >= 1, "bad TiSASRec shape");
  HIPREC_REQUIRE(s->time_span <= kTisMaxSpan, "TiSASRec needs time_span <= %d (got %d)", kTisMaxSpan, s->time_span);
  return 0;
}

static std::atomic<uint64_t> g_tis_lds_done[3][2];      // [head width][forward / backward], a bit per device

// the kernel's dynamic-LDS limit, raised once per device to what the largest supported time_span needs
static int tis_allow_lds(const void* kernel, int hd, int hw, int dir) {
  const size_t most = dir == 0 ? tis_fwd_lds(hd, kTisMaxSpan) : tis_bwd_lds(hd, kTisMaxSpan);
  return allow_dynamic_lds({kernel}, most, g_tis_lds_done[hw][dir], "TiSASRec's attention");
}

static int tis_run(const hiprec_tisasrec_shape& s, float* w_flat, float* g_flat, const int64_t* seq,
                   const int32_t* tm, const int64_t* pos, const int64_t* neg, int64_t B, int T, float l2,
                   const uint8_t* const* keep, float ks, float* feats_out, hiprec_stats* stats, Scratch* scratch,
                   float* ws_base, hipStream_t st) {
  const int D = s.dim, H = s.heads, nb = s.n_blocks, hd = D / H, span = s.time_span;
  const int hw = hd == 16 ? 0 : hd == 32 ? 1 : 2;
  const int64_t M = B * T;
  const int Mi = static_cast<int>(M), Bi = static_cast<int>(B);
  const bool train = g_flat != nullptr;
  const TisParams w = tis_params(w_flat, s);
  const TisWorkspace a = tis_carve(ws_base, s, B, T);
  const float sqrt_d = sqrtf(static_cast<float>(D));
  const int64_t n_table = (s.n_items + 1) * D;
  auto kp = [&](int i) -> const uint8_t* { return keep ? keep[i] : nullptr; };
  const int qt = hd == 64 ? 16 : 32, n_tiles = (T + qt - 1) / qt;
  const dim3 attn_grid(static_cast<unsigned>(B * H), static_cast<unsigned>(n_tiles));
  const size_t fwd_lds = tis_fwd_lds(hd, span), bwd_lds = tis_bwd_lds(hd, span);

  tis_check_tm_kernel<<<grid_for_threads(M * T), kBlock, 0, st>>>(tm, M * T, span, stats);
  HIPREC_TRY(hipGetLastError());
  if (train)
    if (int rc = seq_prep(w.item_emb, g_flat, n_table, pos, M, l2, a.aux, st)) return rc;
  if (int rc = seq_embed(w.item_emb, nullptr, seq, M, T, D, s.n_items, sqrt_d, kp(0), ks, a.x[0], stats, st)) return rc;
  if (int rc = seq_ln_fwd(a.x[0], nullptr, nullptr, nullptr, w.ln_a_w[0], w.ln_a_b[0], a.qn[0], a.mean_a[0],
                          a.rstd_a[0], M, D, st))
    return rc;
  for (int k = 0; k < nb; ++k) {
    const int ka = kTisFixedKeep + 3 * k;      // this block's attention, dropout1, dropout2 keep bytes
    {
      GemmGroup g{};
      g.n = 3;
      g.p[0] = make_gemm(kNT, Mi, D, D, a.qn[k], D, w.q_w[k], D, a.qkv[k], 3 * D, w.q_b[k], 0, nullptr, 0, false);
      g.p[1] = make_gemm(kNT, Mi, D, D, a.x[k], D, w.k_w[k], D, a.qkv[k] + D, 3 * D, w.k_b[k], 0, nullptr, 0, false);
      g.p[2] = make_gemm(kNT, Mi, D, D, a.x[k], D, w.v_w[k], D, a.qkv[k] + 2 * D, 3 * D, w.v_b[k], 0, nullptr, 0,
                         false);
      if (int rc = launch_group(g, st)) return rc;
    }
    tis_pos_fwd_kernel<<<grid_for_threads(M * D), kBlock, 0, st>>>(a.qkv[k], w.pos_k, w.pos_v, M, T, D, kp(1), kp(2),
                                                                   ks);
    HIPREC_TRY(hipGetLastError());
    if (int rc = by_head_width(hd, [&](auto hwc) {
          constexpr int HD = decltype(hwc)::value;
          if (int rc2 = tis_allow_lds(reinterpret_cast<const void*>(&tis_attn_fwd_kernel<HD>), HD, hw, 0))
            return rc2;
          tis_attn_fwd_kernel<HD><<<attn_grid, kBlock, fwd_lds, st>>>(a.qkv[k], seq, tm, w.time_k, w.time_v, Bi, T, H, D,
                                                                      span, kp(ka), kp(3), kp(4), ks, a.o[k], a.lse[k]);
          HIPREC_TRY(hipGetLastError());
          return 0;
        }))
      return rc;
    if (int rc = seq_ln_fwd(a.qn[k], a.o[k], nullptr, nullptr, w.ln_f_w[k], w.ln_f_b[k], a.f[k], a.mean_f[k],
                            a.rstd_f[k], M, D, st))
      return rc;
    if (int rc = seq_ffn_fwd(Mi, D, a.f[k], w.c1_w[k], w.c1_b[k], w.c2_w[k], w.c2_b[k], kp(ka + 1), kp(ka + 2), ks, a.h1[k],
                             a.z, st))
      return rc;
    const bool last = k + 1 == nb;
    if (int rc = seq_ln_fwd(a.f[k], a.z, seq, last ? a.x_last : a.x[k + 1], last ? w.last_w : w.ln_a_w[k + 1],
                            last ? w.last_b : w.ln_a_b[k + 1], last ? (train ? a.feats : feats_out) : a.qn[k + 1],
                            last ? a.mean_l : a.mean_a[k + 1], last ? a.rstd_l : a.rstd_a[k + 1], M, D, st))
      return rc;
  }
  if (!train) return 0;

  const TisParams g = tis_params(g_flat, s);
  float *T1 = a.t[0], *T2 = a.t[1], *T3 = a.t[2], *T4 = a.t[3], *T5 = a.t[4], *T6 = a.t[5], *T7 = a.t[6], *T8 = a.t[7];
  HIPREC_TRY(hipMemsetAsync(a.slab_k, 0, sizeof(float) * 2 * ((a.slab_floats + 3) / 4 * 4), st));
  if (int rc = seq_loss(a.feats, w.item_emb, pos, neg, M, D, s.n_items, a.aux, l2, T1, g.item_emb, scratch, stats, st))
    return rc;
  // T2: gradient of a block's masked output; T3: the same through that block's dropout2 keep bytes
  if (int rc = seq_ln_bwd(T1, nullptr, a.x_last, nullptr, w.last_w, a.mean_l, a.rstd_l, nullptr, nullptr, seq,
                          kp(kTisFixedKeep + 3 * (nb - 1) + 2), ks, T2, T3, T6, T8, g.last_w, g.last_b, a.cs, M, D, st))
    return rc;
  for (int k = nb - 1; k >= 0; --k) {
    const int ka = kTisFixedKeep + 3 * k;
    if (int rc = seq_ffn_bwd(Mi, D, kp(ka + 2) ? T3 : T2, a.f[k], a.h1[k], w.c1_w[k], w.c2_w[k], kp(ka + 1), ks, T4, T5,
                             g.c1_w[k], g.c1_b[k], g.c2_w[k], g.c2_b[k], a.cs, st))
      return rc;
    // LN_f: dy = d(FFN input) + the residual's gradient; T7 = gradient of LN_a(x) + O, which is dO as well
    if (int rc = seq_ln_bwd(T5, T2, a.qn[k], a.o[k], w.ln_f_w[k], a.mean_f[k], a.rstd_f[k], nullptr, nullptr, nullptr,
                            nullptr, ks, T7, nullptr, T6, T8, g.ln_f_w[k], g.ln_f_b[k], a.cs, M, D, st))
      return rc;
    if (int rc = by_head_width(hd, [&](auto hwc) {
          constexpr int HD = decltype(hwc)::value;
          if (int rc2 = tis_allow_lds(reinterpret_cast<const void*>(&tis_attn_bwd_kernel<HD>), HD, hw, 1))
            return rc2;
          for (int tile = 0; tile < n_tiles; ++tile) {     // in order: a later tile adds to what the earlier ones stored
            tis_attn_bwd_kernel<HD><<<static_cast<unsigned>(B * H), kBlock, bwd_lds, st>>>(
                a.qkv[k], T7, a.o[k], a.lse[k], seq, tm, w.time_k, w.time_v, Bi, T, H, D, span, tile, kp(ka), kp(3),
                kp(4), ks, a.dqkv, a.slab_k, a.slab_v);
            HIPREC_TRY(hipGetLastError());
          }
          return 0;
        }))
      return rc;
    tis_pos_bwd_kernel<<<(T * D + kBlock - 1) / kBlock, kBlock, 0, st>>>(a.dqkv, B, T, D, kp(1), kp(2), ks, g.pos_k,
                                                                         g.pos_v);
    HIPREC_TRY(hipGetLastError());
    {
      GemmGroup q{};
      q.n = 9;
      q.p[0] = make_gemm(kNN, Mi, D, D, a.dqkv, 3 * D, w.q_w[k], D, T4, D, nullptr, 0, nullptr, 0, false);
      q.p[1] = make_gemm(kNN, Mi, D, D, a.dqkv + D, 3 * D, w.k_w[k], D, T5, D, nullptr, 0, nullptr, 0, false);
      q.p[2] = make_gemm(kNN, Mi, D, D, a.dqkv + 2 * D, 3 * D, w.v_w[k], D, T1, D, nullptr, 0, nullptr, 0, false);
      q.p[3] = make_gemm(kTNm, D, D, Mi, a.dqkv, 3 * D, a.qn[k], D, g.q_w[k], D, nullptr, 0, nullptr, 0, true);
      q.p[4] = make_gemm(kTNm, D, D, Mi, a.dqkv + D, 3 * D, a.x[k], D, g.k_w[k], D, nullptr, 0, nullptr, 0, true);
      q.p[5] = make_gemm(kTNm, D, D, Mi, a.dqkv + 2 * D, 3 * D, a.x[k], D, g.v_w[k], D, nullptr, 0, nullptr, 0, true);
      q.p[6] = make_colsum(a.dqkv, Mi, D, 3 * D, g.q_b[k], a.cs);
      q.p[7] = make_colsum(a.dqkv + D, Mi, D, 3 * D, g.k_b[k], a.cs + a.cs_each);
      q.p[8] = make_colsum(a.dqkv + 2 * D, Mi, D, 3 * D, g.v_b[k], a.cs + 2 * a.cs_each);
      if (int rc = launch_group(q, st)) return rc;
      if (int rc = launch_colsum_reduce(q, st)) return rc;
    }
    // LN_a: dy = d(q projection input) + the residual's gradient; the K / V paths enter x directly
    if (int rc = seq_ln_bwd(T4, T7, a.x[k], nullptr, w.ln_a_w[k], a.mean_a[k], a.rstd_a[k], T5, T1,
                            k > 0 ? seq : nullptr, k > 0 ? kp(ka - 1) : nullptr, ks, T2, T3, T6, T8, g.ln_a_w[k],
                            g.ln_a_b[k], a.cs, M, D, st))
      return rc;
  }
  tis_embed_bwd_kernel<<<grid_for_threads(M * D), kBlock, 0, st>>>(T2, seq, M, D, s.n_items, sqrt_d, kp(0), ks,
                                                                   g.item_emb);
  HIPREC_TRY(hipGetLastError());
  const int64_t n_tab = static_cast<int64_t>(span + 1) * D;
  tis_table_reduce_kernel<<<static_cast<unsigned>((n_tab + kBlock - 1) / kBlock), kBlock, 0, st>>>(
      a.slab_k, a.slab_v, B, n_tab, g.time_k, g.time_v);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_tisasrec_shape_bytes(void) { return sizeof(hiprec_tisasrec_shape); }

extern "C" int64_t hiprec_tisasrec_param_floats(const hiprec_tisasrec_shape* shape) {
  if (tis_check_shape(shape)) return -1;
  return tis_n_params(*shape);
}

extern "C" size_t hiprec_tisasrec_workspace_bytes(const hiprec_tisasrec_shape* shape, int64_t batch, int32_t seq_len) {
  if (tis_check_shape(shape) || batch <= 0 || seq_len <= 0) return 0;
  return sizeof(float) * static_cast<size_t>(tis_carve(nullptr, *shape, batch, seq_len).floats);
}

extern "C" int hiprec_tisasrec_grad(const hiprec_tisasrec_shape* shape, const float* w_flat, float* g_flat,
                                    const int64_t* seq, const int32_t* time_matrix, const int64_t* pos,
                                    const int64_t* neg, int64_t batch, int32_t seq_len, float l2_emb,
                                    const uint8_t* const* keep, float keep_scale, float* feats_out, hiprec_stats* stats,
                                    void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (int rc = tis_check_shape(shape)) return rc;
  HIPREC_REQUIRE(time_matrix, "NULL pointer");
  if (int rc = seq_check_call(w_flat, g_flat, seq, pos, neg, batch, seq_len, shape->maxlen, shape->heads, feats_out,
                              stats, scratch, scratch_bytes, workspace, workspace_bytes,
                              hiprec_tisasrec_workspace_bytes(shape, batch, seq_len)))
    return rc;
  return tis_run(*shape, const_cast<float*>(w_flat), g_flat, seq, time_matrix, pos, neg, batch, seq_len, l2_emb, keep,
                 keep_scale, feats_out, stats, static_cast<Scratch*>(scratch), static_cast<float*>(workspace),
                 static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_time_relation(const int64_t* time_seq, int64_t batch, int32_t seq_len, int32_t time_span,
                                    int32_t* out, void* stream) {
  HIPREC_REQUIRE(time_seq && out, "NULL pointer");
  HIPREC_REQUIRE(batch >= 1 && seq_len >= 1 && time_span >= 0, "bad batch / sequence length / time span");
  const int64_t n = batch * seq_len * seq_len;
  tis_time_relation_kernel<<<grid_for_threads(n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(time_seq, batch, seq_len,
                                                                                               time_span, out);
  HIPREC_TRY(hipGetLastError());
  return 0;
}
