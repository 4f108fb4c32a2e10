// ETA (Chen et al., 2021): SimHash retrieval over a long history and a multi-head target attention over the retrieved
// positions, then DIN's tower (csrc/din.hpp).  The contract is in include/hiprec.h; B sequences of T slots, C candidates per
// sequence, N = B C pairs, D = dim, m = hash_bits (Wd = m / 32 code words), k = top_k, H heads of dh = D / H.
//
//   retrieve  a workgroup owns one sequence and all its candidates.  hash.weight [m, D] stays in LDS; the history is walked in
//             chunks of 64 positions, each gathered into LDS once (from the table or from explicit rows).  A wave owns a tile
//             of 16 positions: two 16 x 16 accumulators of v_mfma_f32_16x16x4_f32 over D are the projections onto 32 hash
//             vectors, __ballot of their signs gives, per accumulator register, the 16-bit half words of four positions, and
//             lanes 0 .. 15 put the halves of their position together.  No float leaves the product.  Codes go to the
//             workspace and stay in LDS when T Wd words fit beside the rest; the candidates' codes are made the same way.
//             Then a wave per candidate: XOR + popcount against every live position into an integer histogram of the m + 1
//             distances (LDS counters), the threshold distance and the number of ties it may take from one walk of the
//             histogram, and a second walk over the positions from the most recent end that takes everything below the
//             threshold and the first `ties` at it.  The slot of a taken position is known from ballots alone (the total is
//             min(k, live)), so sel leaves ascending in t with no sort.  The selection is a function of the codes alone.
//   compact   the same workgroup ORs every selection into a bitmap of T bits; a prefix over its words gives the sequence's
//             distinct selected positions and, for every sel slot, its rank among them.  A one-block scan turns the
//             per-sequence counts into batch-wide row offsets: the compact row list (no host sync; the launches that follow
//             are sized by the bound B min(T, C k), the rows past the end are zero).
//   project   [Wk; Wv] over the compact rows and Wq over the N candidate rows: two problems of ONE grouped GEMM launch
//             (csrc/ncf.hip); Wo after the attention.  No [B, T, D] projection exists.
//   attend    a wave per pair.  Lanes over the <= k slots: the H scores of a slot against its compact row; per head a
//             masked softmax across the wave; lanes over D: the weighted sum.  p is saved.
//   backward  two passes, no atomics: the pair's wave forms dp, ds = p (dp - sum p dp) and dQp and saves ds; then a wave per
//             compact row walks the sequence's candidates in order, finds itself in each ascending rank row by binary search
//             and sums dVp = sum p dO, dKp = sum ds Qp / sqrt(dh) in that order.  d e = [dKp | dVp] [Wk; Wv] and d q = dQp Wq
//             are problems of one grouped launch with the K-sliced weight-gradient GEMMs, which are added in slice order.
//
// The only float atomics are rows of d item_emb.weight (din_scatter); every other gradient is the same bits on every run.
#include <algorithm>

#include "din.hpp"

namespace hiprec {
namespace {

constexpr int kEtaMaxLen = 4096, kEtaMaxBits = 128, kEtaMaxK = 128;
constexpr int kEtaChunk = 64;                    // staged positions: a tile of 16 per wave
constexpr int kEtaMaxWords = kEtaMaxLen / 32;    // words of the selection bitmap
constexpr int kEtaSplitKV = 6, kEtaSplitQ = 3, kEtaSplitO = 3;      // K-slices of the weight-gradient GEMMs
constexpr size_t kEtaLdsBudget = 152 * 1024;      // dynamic LDS; the retrieval kernel's static arrays take 5 KB more

struct EtaDims {
  int64_t n_items;
  int D, T, m, Wd, k, H, dh, dnn_act, L, W[kDinMaxLayers];
};

// offsets into the flat parameter buffer (state_dict() order; hash.weight is a buffer beside it)
struct EtaOff {
  int64_t qw, qb, kw, kb, vw, vb, ow, ob, dw[kDinMaxLayers], db[kDinMaxLayers], da[kDinMaxLayers], outw, outb, total;
  int in[kDinMaxLayers], bn[kDinMaxLayers];
};

EtaOff eta_offsets(const EtaDims& q) {
  EtaOff o{};
  int64_t p = (q.n_items + 1) * q.D;
  auto take = [&](int64_t n) { int64_t r = p; p += n; return r; };
  const int64_t DD = static_cast<int64_t>(q.D) * q.D;
  o.qw = take(DD); o.qb = take(q.D); o.kw = take(DD); o.kb = take(q.D);
  o.vw = take(DD); o.vb = take(q.D); o.ow = take(DD); o.ob = take(q.D);
  int in = 3 * q.D, bn = 0;
  for (int l = 0; l < q.L; ++l) {
    o.in[l] = in;
    o.dw[l] = take(static_cast<int64_t>(q.W[l]) * in); o.db[l] = take(q.W[l]); o.da[l] = take(q.W[l]);
    o.bn[l] = bn;
    bn += 2 * q.W[l];
    in = q.W[l];
  }
  o.outw = take(in); o.outb = take(1);
  o.total = p;
  return o;
}

// ---- retrieval ---------------------------------------------------------------------------------------------------------------
struct EtaRetrieve {
  int T, C, D, m, Wd, k, U, ldE, codes_lds;
  int64_t n_items;
  const float *hash, *E, *e, *q;      // the table (with seq / cand) or explicit rows e [B T, D], q [N, D] (with mask)
  const int64_t *seq, *cand;
  const uint8_t* mask;
  uint32_t *codes_e, *codes_q;        // [B T, Wd], [N, Wd]
  int32_t *sel, *rank, *upos, *count; // [N, k], [N, k], [B, U], [B]
  hiprec_stats* stats;
};

__device__ __forceinline__ void eta_wave_sync() {      // LDS traffic of one wave, in order
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Codes of the 64 staged rows in Es: the wave's 16 rows x 32 hash vectors per word, signs packed by ballot.  Rows
// [0, n_rows) are stored at out[row * Wd + word] (and at lds_out likewise when given).
__device__ __forceinline__ void eta_hash_chunk(const float* Hs, const float* Es, int ldE, int D, int Wd, int n_rows,
                                               uint32_t* out, uint32_t* lds_out) {
  const int l = lane_id(), li = l & 15, lk = l >> 4, r0 = wave_in_block() * 16;
  const float* ap = Es + (r0 + li) * ldE + lk;
  for (int wd = 0; wd < Wd; ++wd) {
    const float* b0 = Hs + (wd * 32 + li) * ldE + lk;
    const float* b1 = b0 + 16 * ldE;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < D; kk += 4) {
      const float a = ap[kk];
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0[kk], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1[kk], acc1, 0, 0, 0);
    }
    // register r of lane (lk, li) is the projection of row 4 lk + r onto hash vector li of the tile: the ballot's 16-bit
    // segment lk is that row's half word
    uint32_t word = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const unsigned long long m0 = __ballot(acc0[r] >= 0.f), m1 = __ballot(acc1[r] >= 0.f);
      const int sh = 16 * ((l >> 2) & 3);
      const uint32_t w = static_cast<uint32_t>((m0 >> sh) & 0xffffull) | (static_cast<uint32_t>((m1 >> sh) & 0xffffull) << 16);
      if ((l & 3) == r) word = w;
    }
    const int row = r0 + l;      // lanes 0 .. 15: row 4 (l >> 2) + (l & 3) = l of the tile
    if (l < 16 && row < n_rows) {
      out[static_cast<int64_t>(row) * Wd + wd] = word;
      if (lds_out) lds_out[row * Wd + wd] = word;
    }
  }
}

__device__ __forceinline__ int eta_ham(const uint32_t* cp, const uint32_t (&cq)[4], int Wd) {
  int h = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w)
    if (w < Wd) h += __popc(cq[w] ^ cp[w]);
  return h;
}

// One wave, one candidate: the k live positions with the smallest (distance, -t) into sel_out, ascending in t, -1 behind
// them; the taken positions OR-ed into selbits.
__device__ __forceinline__ void eta_select(const EtaRetrieve& p, const uint32_t* cp, const uint32_t* livebits,
                                           const uint32_t* cqp, int* hist, uint32_t* selbits, int32_t* sel_out) {
  const int lane = lane_id(), T = p.T, Wd = p.Wd, k = p.k;
  uint32_t cq[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) cq[w] = w < Wd ? cqp[w] : 0u;
  for (int i = lane; i <= p.m; i += kWave) hist[i] = 0;
  eta_wave_sync();
  for (int base = 0; base < T; base += kWave) {
    const int t = base + lane;
    if (t < T && ((livebits[t >> 5] >> (t & 31)) & 1u)) atomicAdd(&hist[eta_ham(cp + static_cast<int64_t>(t) * Wd, cq, Wd)], 1);
  }
  eta_wave_sync();
  // the threshold: the smallest distance at which k positions are reached; `need` ties are taken at it
  int cum = 0, thr = p.m + 1, need = 0;
  for (int d = 0; d <= p.m; ++d) {
    const int h = hist[d];
    if (cum + h >= k) { thr = d; need = k - cum; break; }
    cum += h;
  }
  const int n_sel = thr > p.m ? cum : k;      // fewer than k live positions: all of them
  int taken = 0, ties = 0;
  for (int base = (T - 1) / kWave * kWave; base >= 0 && taken < n_sel; base -= kWave) {
    const int t = base + lane;
    const bool live = t < T && ((livebits[t >> 5] >> (t & 31)) & 1u);
    const int ham = live ? eta_ham(cp + static_cast<int64_t>(t) * Wd, cq, Wd) : 0;
    const unsigned long long above = ~((2ull << lane) - 1ull);      // the lanes of more recent positions
    const bool tie = live && ham == thr;
    const unsigned long long tm = __ballot(tie);
    const bool tie_take = tie && ties + __popcll(tm & above) < need;
    const bool s = (live && ham < thr) || tie_take;
    const unsigned long long sm = __ballot(s);
    const int slot = n_sel - 1 - (taken + __popcll(sm & above));
    if (s && slot >= 0) sel_out[slot] = t;
    taken += __popcll(sm);
    ties += __popcll(__ballot(tie_take));
    if (lane == 0 && sm) {
      atomicOr(&selbits[base >> 5], static_cast<uint32_t>(sm));
      atomicOr(&selbits[(base >> 5) + 1], static_cast<uint32_t>(sm >> 32));
    }
  }
  for (int j = n_sel + lane; j < k; j += kWave) sel_out[j] = -1;
}

// From the bitmap of a sequence's selected positions: its distinct positions ascending into upos, their number into count,
// and the rank of every sel slot among them (-1 for an empty slot or a position outside the history).  Whole workgroup.
__device__ __forceinline__ void eta_compact(int64_t b, int T, int CK, int U, const uint32_t* selbits, int* pre,
                                            const int32_t* sel, int32_t* rank, int32_t* upos, int32_t* count) {
  const int nW = (T + 63) / 64 * 2;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int i = 0; i < nW; ++i) { pre[i] = run; run += __popc(selbits[i]); }
    count[b] = run;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nW; i += kBlock) {
    uint32_t bits = selbits[i];
    int r = pre[i];
    while (bits) {
      if (r < U) upos[b * U + r] = i * 32 + __ffs(bits) - 1;
      ++r;
      bits &= bits - 1;
    }
  }
  for (int s = threadIdx.x; s < CK; s += kBlock) {
    const int t = sel[b * CK + s];
    rank[b * CK + s] = (t < 0 || t >= T) ? -1 : pre[t >> 5] + __popc(selbits[t >> 5] & ((1u << (t & 31)) - 1u));
  }
}

// grid B.  Dynamic LDS: hash.weight [m, ldE], the chunk [64, ldE], then the codes [T, Wd] when they fit.
__global__ __launch_bounds__(kBlock) void eta_retrieve_kernel(EtaRetrieve p) {
  extern __shared__ float eta_lds[];
  __shared__ uint32_t livebits[kEtaMaxWords], selbits[kEtaMaxWords];
  __shared__ int pre[kEtaMaxWords], hist[kWavesPerBlock][kEtaMaxBits + 4];
  __shared__ int64_t src[kEtaChunk];
  float* Hs = eta_lds;
  float* Es = Hs + p.m * p.ldE;
  uint32_t* lds_codes = p.codes_lds ? reinterpret_cast<uint32_t*>(Es + kEtaChunk * p.ldE) : nullptr;
  const int64_t b = blockIdx.x;
  const int T = p.T, D = p.D, Wd = p.Wd, C = p.C;
  for (int e = threadIdx.x; e < p.m * D; e += kBlock) {
    const int j = e / D, d = e - j * D;
    Hs[j * p.ldE + d] = p.hash[e];
  }
  for (int i = threadIdx.x; i < kEtaMaxWords; i += kBlock) livebits[i] = selbits[i] = 0u;
  uint32_t* gcodes = p.codes_e + b * T * Wd;
  // the history, a chunk at a time: where each row comes from (-1: a zero row), the live bits, the rows, the codes
  for (int t0 = 0; t0 < T; t0 += kEtaChunk) {
    __syncthreads();
    if (threadIdx.x < kEtaChunk) {
      const int t = t0 + threadIdx.x;
      int64_t from = -1;
      bool live = false;
      if (t < T) {
        if (p.e) {
          from = (b * T + t) * D;
          live = p.mask[b * T + t] != 0;
        } else {
          const int64_t id = p.seq[b * T + t];
          live = id >= 1 && id <= p.n_items;
          if (id >= 0 && id <= p.n_items) from = id * D;
          else if (p.stats) atomicOr(&p.stats->status, HIPREC_STATUS_ITEM_OOB);
        }
      }
      src[threadIdx.x] = from;
      const unsigned long long lm = __ballot(live);      // wave 0 holds the chunk's 64 positions
      if (threadIdx.x == 0) {
        livebits[t0 >> 5] = static_cast<uint32_t>(lm);
        livebits[(t0 >> 5) + 1] = static_cast<uint32_t>(lm >> 32);
      }
    }
    __syncthreads();
    const float* from = p.e ? p.e : p.E;
    for (int e = threadIdx.x; e < kEtaChunk * D; e += kBlock) {
      const int r = e / D, d = e - r * D;
      Es[r * p.ldE + d] = src[r] >= 0 ? from[src[r] + d] : 0.f;
    }
    __syncthreads();
    eta_hash_chunk(Hs, Es, p.ldE, D, Wd, min(kEtaChunk, T - t0), gcodes + static_cast<int64_t>(t0) * Wd,
                   lds_codes ? lds_codes + t0 * Wd : nullptr);
  }
  // the candidates' codes, the same way
  uint32_t* qcodes = p.codes_q + b * C * Wd;
  for (int c0 = 0; c0 < C; c0 += kEtaChunk) {
    __syncthreads();
    if (threadIdx.x < kEtaChunk) {
      const int c = c0 + threadIdx.x;
      int64_t from = -1;
      if (c < C) {
        if (p.q) {
          from = (b * C + c) * D;
        } else {
          const int64_t id = p.cand[b * C + c];
          if (id >= 0 && id <= p.n_items) from = id * D;
          else if (p.stats) atomicOr(&p.stats->status, HIPREC_STATUS_ITEM_OOB);
        }
      }
      src[threadIdx.x] = from;
    }
    __syncthreads();
    const float* from = p.q ? p.q : p.E;
    for (int e = threadIdx.x; e < kEtaChunk * D; e += kBlock) {
      const int r = e / D, d = e - r * D;
      Es[r * p.ldE + d] = src[r] >= 0 ? from[src[r] + d] : 0.f;
    }
    __syncthreads();
    eta_hash_chunk(Hs, Es, p.ldE, D, Wd, min(kEtaChunk, C - c0), qcodes + static_cast<int64_t>(c0) * Wd, nullptr);
  }
  __syncthreads();      // the codes this workgroup wrote are visible to all of its waves
  const uint32_t* cp = lds_codes ? lds_codes : gcodes;
  const int wave = wave_in_block();
  for (int c = wave; c < C; c += kWavesPerBlock) {
    int32_t* out = p.sel + (b * C + c) * p.k;
    bool dead = false;
    if (!p.q) {
      const int64_t id = p.cand[b * C + c];
      dead = id < 1 || id > p.n_items;
    }
    if (dead) {
      for (int j = lane_id(); j < p.k; j += kWave) out[j] = -1;
      continue;
    }
    eta_select(p, cp, livebits, qcodes + c * Wd, hist[wave], selbits, out);
  }
  eta_compact(b, T, C * p.k, p.U, selbits, pre, p.sel, p.rank, p.upos, p.count);
}

// grid B: the compaction alone, from an explicit sel [N, k]
__global__ __launch_bounds__(kBlock) void eta_compact_kernel(int T, int CK, int U, const int32_t* __restrict__ sel,
                                                             int32_t* __restrict__ rank, int32_t* __restrict__ upos,
                                                             int32_t* __restrict__ count) {
  __shared__ uint32_t selbits[kEtaMaxWords];
  __shared__ int pre[kEtaMaxWords];
  const int64_t b = blockIdx.x;
  for (int i = threadIdx.x; i < kEtaMaxWords; i += kBlock) selbits[i] = 0u;
  __syncthreads();
  for (int s = threadIdx.x; s < CK; s += kBlock) {
    const int t = sel[b * CK + s];
    if (t >= 0 && t < T) atomicOr(&selbits[t >> 5], 1u << (t & 31));
  }
  eta_compact(b, T, CK, U, selbits, pre, sel, rank, upos, count);
}

// one block: off[b] = the sequences' counts summed below b, off[B] = the rows of the compact list
__global__ __launch_bounds__(kBlock) void eta_offsets_kernel(const int32_t* __restrict__ count, int64_t B,
                                                             int32_t* __restrict__ off) {
  __shared__ int part[kBlock];
  const int64_t per = (B + kBlock - 1) / kBlock, lo = per * threadIdx.x < B ? per * threadIdx.x : B, hi = lo + per < B ? lo + per : B;
  int s = 0;
  for (int64_t i = lo; i < hi; ++i) s += count[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int i = 0; i < kBlock; ++i) { const int v = part[i]; part[i] = run; run += v; }
    off[B] = run;
  }
  __syncthreads();
  int run = part[threadIdx.x];
  for (int64_t i = lo; i < hi; ++i) { off[i] = run; run += count[i]; }
}

// a thread per slot of the bound B U: the compact rows' sequence, source position b T + t and item id; -1 / 0 past the end
__global__ __launch_bounds__(kBlock) void eta_rowid_kernel(int64_t B, int T, int U, const int32_t* __restrict__ count,
                                                           const int32_t* __restrict__ off, const int32_t* __restrict__ upos,
                                                           const int64_t* __restrict__ seq, int32_t* __restrict__ row_src,
                                                           int32_t* __restrict__ row_b, int64_t* __restrict__ row_id) {
  const int64_t R = off[B];
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; w < B * U; w += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t b = w / U;
    const int i = static_cast<int>(w - b * U);
    if (i < count[b]) {
      const int64_t r = off[b] + i, at = b * T + upos[w];
      row_src[r] = static_cast<int32_t>(at);
      row_b[r] = static_cast<int32_t>(b);
      row_id[r] = seq ? seq[at] : 0;
    }
    if (w >= R) {
      row_src[w] = -1;
      row_b[w] = -1;
      row_id[w] = 0;
    }
  }
}

// the stage entry's rows: a wave per compact row copies e[row_src] (a zero row past the end), every row and pair is live
__global__ __launch_bounds__(kBlock) void eta_rows_kernel(const float* __restrict__ e, const int32_t* __restrict__ row_src,
                                                          int64_t R, int D, float* __restrict__ rows, uint8_t* __restrict__ lv,
                                                          uint8_t* __restrict__ lc, int64_t N) {
  const int lane = lane_id();
  const int64_t n_lc = (N + kWave - 1) / kWave, end = R > n_lc ? R : n_lc;
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); w < end;
       w += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    if (w < R) {
      const int64_t at = row_src[w];
      for (int d = lane; d < D; d += kWave) rows[w * D + d] = at >= 0 ? e[at * D + d] : 0.f;
      if (lane == 0) lv[w] = at >= 0;
    }
    if (w * kWave + lane < N) lc[w * kWave + lane] = 1;
  }
}
// ... and their gradient back: de [B T, D] (zero on entry) receives row r at row_src[r]; a position is one row at most
__global__ __launch_bounds__(kBlock) void eta_rows_back_kernel(const float* __restrict__ dE, const int32_t* __restrict__ row_src,
                                                               int64_t R, int D, float* __restrict__ de) {
  const int lane = lane_id();
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); w < R;
       w += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const int64_t at = row_src[w];
    if (at < 0) continue;
    for (int d = lane; d < D; d += kWave) de[at * D + d] = dE[w * D + d];
  }
}

// ---- the attention -----------------------------------------------------------------------------------------------------------
struct EtaAttn {
  int C, D, H, dh, k;
  int64_t N;
  float scale;
  const int32_t *rank, *off;      // [N, k], [B + 1]
  const float* KV;                // [rows, 2 D]: Kp | Vp
};

__device__ __forceinline__ float eta_wave_max(float v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, kWave));
  return v;
}

// A wave per pair; dynamic LDS per wave: D floats, k row indices, H k floats.
// Forward: x = Qp, against Kp -> scores -> softmax p (saved to P) -> out = O = sum p Vp.
// Backward: x = dO, against Vp -> dp -> ds = p (dp - sum p dp) (saved to S) -> out = dQp = scale sum ds Kp.
template <bool BWD>
__global__ __launch_bounds__(kBlock) void eta_pair_kernel(EtaAttn a, const float* __restrict__ x, float* __restrict__ P,
                                                          float* __restrict__ S, float* __restrict__ out) {
  extern __shared__ float eta_lds[];
  const int lane = lane_id(), D = a.D, H = a.H, dh = a.dh, k = a.k, ld = 2 * D;
  float* xs = eta_lds + wave_in_block() * (D + k + H * k);
  int* rowi = reinterpret_cast<int*>(xs + D);
  float* sc = xs + D + k;
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const bool on = n < a.N;
  if (on) {
    const int base = a.off[n / a.C];
    for (int d = lane; d < D; d += kWave) xs[d] = x[n * D + d];
    for (int j = lane; j < k; j += kWave) {
      const int r = a.rank[n * k + j];
      rowi[j] = r < 0 ? -1 : base + r;
    }
  }
  __syncthreads();
  if (on) {
    for (int j = lane; j < k; j += kWave) {
      const int r = rowi[j];
      const float* row = a.KV + static_cast<int64_t>(max(r, 0)) * ld + (BWD ? D : 0);
      for (int h = 0; h < H; ++h) {
        float s = 0.f;
        if (r >= 0)
          for (int d = h * dh; d < (h + 1) * dh; ++d) s = fmaf(xs[d], row[d], s);
        sc[h * k + j] = BWD ? s : (r >= 0 ? s * a.scale : -INFINITY);
      }
    }
  }
  __syncthreads();
  if (on) {
    for (int h = 0; h < H; ++h) {
      float* pr = P + (n * H + h) * k;
      const int j0 = lane, j1 = lane + kWave;
      if (BWD) {
        const float d0 = j0 < k ? sc[h * k + j0] : 0.f, d1 = j1 < k ? sc[h * k + j1] : 0.f;
        const float p0 = j0 < k ? pr[j0] : 0.f, p1 = j1 < k ? pr[j1] : 0.f;
        const float t = wave_sum(fmaf(p0, d0, p1 * d1));
        if (j0 < k) S[(n * H + h) * k + j0] = sc[h * k + j0] = p0 * (d0 - t);
        if (j1 < k) S[(n * H + h) * k + j1] = sc[h * k + j1] = p1 * (d1 - t);
      } else {
        const float s0 = j0 < k ? sc[h * k + j0] : -INFINITY, s1 = j1 < k ? sc[h * k + j1] : -INFINITY;
        const float mx = eta_wave_max(fmaxf(s0, s1));
        const float e0 = s0 == -INFINITY ? 0.f : expf(s0 - mx), e1 = s1 == -INFINITY ? 0.f : expf(s1 - mx);
        const float sum = wave_sum(e0 + e1), inv = sum > 0.f ? 1.f / sum : 0.f;
        if (j0 < k) pr[j0] = sc[h * k + j0] = e0 * inv;
        if (j1 < k) pr[j1] = sc[h * k + j1] = e1 * inv;
      }
    }
  }
  __syncthreads();
  if (on) {
    for (int d = lane; d < D; d += kWave) {
      const float* w = sc + (d / dh) * k;
      const float* col = a.KV + (BWD ? 0 : D) + d;
      float acc = 0.f;
      for (int j = 0; j < k; ++j) {
        const int r = rowi[j];
        if (r >= 0) acc = fmaf(w[j], col[static_cast<int64_t>(r) * ld], acc);
      }
      out[n * D + d] = BWD ? acc * a.scale : acc;
    }
  }
}

// A wave per compact row (of the bound; a row past the end gets zeros): dKV[r] = [sum ds Qp scale | sum p dO] over the
// pairs of the row's sequence that selected it, in candidate order.
__global__ __launch_bounds__(kBlock) void eta_row_bwd_kernel(EtaAttn a, int64_t R, const int32_t* __restrict__ row_b,
                                                             const float* __restrict__ P, const float* __restrict__ S,
                                                             const float* __restrict__ Qp, const float* __restrict__ dO,
                                                             float* __restrict__ dKV) {
  const int lane = lane_id(), D = a.D, H = a.H, dh = a.dh, k = a.k;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); r < R;
       r += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const int64_t b = row_b[r];
    float aK[2] = {0.f, 0.f}, aV[2] = {0.f, 0.f};
    if (b >= 0) {
      const int i = static_cast<int>(r - a.off[b]);
      for (int c = 0; c < a.C; ++c) {
        const int64_t n = b * a.C + c;
        const int32_t* rk = a.rank + n * k;
        int lo = 0, hi = k;      // the first slot that is empty or ranks at least i
        while (lo < hi) {
          const int mid = (lo + hi) >> 1, v = rk[mid];
          if (v < 0 || v >= i) hi = mid;
          else lo = mid + 1;
        }
        if (lo >= k || rk[lo] != i) continue;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int d = lane + u * kWave;
          if (d >= D) break;
          const int64_t at = (n * H + d / dh) * k + lo;
          aK[u] = fmaf(S[at], Qp[n * D + d], aK[u]);
          aV[u] = fmaf(P[at], dO[n * D + d], aV[u]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int d = lane + u * kWave;
      if (d >= D) break;
      dKV[r * 2 * D + d] = aK[u] * a.scale;
      dKV[r * 2 * D + D + d] = aV[u];
    }
  }
}

// [Wk; Wv] and [bk; bv] stacked for the one problem over the compact rows
__global__ __launch_bounds__(kBlock) void eta_stack_kernel(const float* __restrict__ kw, const float* __restrict__ kb,
                                                           const float* __restrict__ vw, const float* __restrict__ vb, int D,
                                                           float* __restrict__ Wkv, float* __restrict__ bkv) {
  const int i = blockIdx.x * kBlock + threadIdx.x, DD = D * D;
  if (i < DD) { Wkv[i] = kw[i]; Wkv[DD + i] = vw[i]; }
  if (i < D) { bkv[i] = kb[i]; bkv[D + i] = vb[i]; }
}

// the K-slices of the four weight gradients, added in slice order
__global__ __launch_bounds__(kBlock) void eta_fold_kernel(const float* __restrict__ gq, int nq, const float* __restrict__ gkv,
                                                          int nkv, const float* __restrict__ go, int no, int D,
                                                          float* __restrict__ qw, float* __restrict__ kw,
                                                          float* __restrict__ vw, float* __restrict__ ow) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x, DD = static_cast<int64_t>(D) * D;
  if (i >= DD) return;
  qw[i] = din_slab_sum(gq, nq, DD, i);
  kw[i] = din_slab_sum(gkv, nkv, 2 * DD, i);
  vw[i] = din_slab_sum(gkv, nkv, 2 * DD, DD + i);
  ow[i] = din_slab_sum(go, no, DD, i);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
int eta_check_shape(const hiprec_eta_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  HIPREC_REQUIRE(s->n_items >= 1 && s->n_items < (1ll << 31), "ETA needs 1 <= n_items < 2^31, got %lld",
                 static_cast<long long>(s->n_items));
  HIPREC_REQUIRE(s->dim >= 16 && s->dim <= kDinMaxDim && s->dim % 16 == 0,
                 "ETA needs emb_dim a multiple of 16 in 16 .. %d (got %d)", kDinMaxDim, s->dim);
  HIPREC_REQUIRE(s->maxlen >= 1 && s->maxlen <= kEtaMaxLen, "ETA needs 1 <= maxlen <= %d (got %d)", kEtaMaxLen, s->maxlen);
  HIPREC_REQUIRE(s->hash_bits >= 32 && s->hash_bits <= kEtaMaxBits && s->hash_bits % 32 == 0,
                 "ETA needs hash_bits in {32, 64, 96, 128} (got %d)", s->hash_bits);
  HIPREC_REQUIRE(s->top_k >= 1 && s->top_k <= kEtaMaxK, "ETA needs 1 <= top_k <= %d (got %d)", kEtaMaxK, s->top_k);
  HIPREC_REQUIRE(s->num_heads >= 1 && s->dim % s->num_heads == 0 && s->dim / s->num_heads >= 4,
                 "ETA needs num_heads dividing emb_dim with at least 4 dimensions a head (got %d for %d)", s->num_heads, s->dim);
  HIPREC_REQUIRE(s->n_dnn >= 1 && s->n_dnn <= kDinMaxLayers, "ETA needs 1 .. %d dnn_hidden widths (got %d)", kDinMaxLayers,
                 s->n_dnn);
  for (int l = 0; l < s->n_dnn; ++l)
    HIPREC_REQUIRE(s->dnn[l] >= 1 && s->dnn[l] <= kDinMaxDnn, "ETA needs dnn_hidden widths in 1 .. %d (got %d)", kDinMaxDnn,
                   s->dnn[l]);
  HIPREC_REQUIRE(s->dnn_act == 0 || s->dnn_act == 1, "ETA: dnn_activation is dice (0) or prelu (1)");
  return 0;
}

EtaDims eta_dims(const hiprec_eta_shape& s) {
  EtaDims q{};
  q.n_items = s.n_items; q.D = s.dim; q.T = s.maxlen; q.m = s.hash_bits; q.Wd = s.hash_bits / 32; q.k = s.top_k;
  q.H = s.num_heads; q.dh = s.dim / s.num_heads; q.dnn_act = s.dnn_act; q.L = s.n_dnn;
  for (int l = 0; l < q.L; ++l) q.W[l] = s.dnn[l];
  return q;
}

bool eta_batch_ok(const EtaDims& q, int64_t B, int64_t C) {
  return B >= 1 && C >= 1 && C <= kDinMaxRows && B * q.T <= kDinMaxRows && B * C * q.k <= kDinMaxRows;
}

// rows of a sequence's compact list at most
int eta_rows_per_seq(const EtaDims& q, int64_t C) { return static_cast<int>(std::min<int64_t>(q.T, C * q.k)); }

// the retrieval kernel's dynamic LDS; *codes_lds: the codes stay on chip
size_t eta_retrieve_lds(const EtaDims& q, int* codes_lds) {
  const size_t fixed = static_cast<size_t>(q.m + kEtaChunk) * (q.D + 4) * sizeof(float);
  const size_t codes = static_cast<size_t>(q.T) * q.Wd * sizeof(uint32_t);
  *codes_lds = fixed + codes <= kEtaLdsBudget;
  return fixed + (*codes_lds ? codes : 0);
}
size_t eta_pair_lds(const EtaDims& q) { return sizeof(float) * kWavesPerBlock * (q.D + q.k + q.H * q.k); }

struct EtaWs {
  float *Wkv, *bkv, *rows, *q, *KV, *Qp, *P, *O, *v, *z, *x[kDinMaxLayers], *y[kDinMaxLayers], *mean, *var, *logit;
  float *dlogit, *dA, *dB, *sums, *dv, *dqz, *dO, *dQp, *S, *dKV, *dE, *dqa, *gkv, *gq, *go, *cs, *cs_q, *cs_k, *cs_v, *cs_o;
  uint32_t *codes_e, *codes_q;
  int32_t *sel, *rank, *upos, *count, *off, *row_src, *row_b;
  int64_t* row_id;
  uint8_t *lv, *lc;
  int64_t floats;
};

EtaWs eta_carve_ws(float* base, const EtaDims& q, int64_t B, int64_t C, bool train) {
  EtaWs w{};
  float* p = base;
  auto take = [&](int64_t n) { float* r = p; p += (n + 3) / 4 * 4; return r; };
  auto take_i = [&](int64_t n) { return reinterpret_cast<int32_t*>(take(n)); };
  const int64_t N = B * C, NK = N * q.k, R = B * eta_rows_per_seq(q, C), D = q.D, DD = D * D;
  w.Wkv = take(2 * DD); w.bkv = take(2 * D);
  w.codes_e = reinterpret_cast<uint32_t*>(take(B * q.T * q.Wd)); w.codes_q = reinterpret_cast<uint32_t*>(take(N * q.Wd));
  w.sel = take_i(NK); w.rank = take_i(NK); w.upos = take_i(R); w.count = take_i(B); w.off = take_i(B + 1);
  w.row_src = take_i(R); w.row_b = take_i(R); w.row_id = reinterpret_cast<int64_t*>(take(2 * R));
  w.lv = reinterpret_cast<uint8_t*>(take((R + 3) / 4)); w.lc = reinterpret_cast<uint8_t*>(take((N + 3) / 4));
  w.rows = take(R * D); w.q = take(N * D); w.KV = take(R * 2 * D); w.Qp = take(N * D);
  w.P = take(NK * q.H); w.O = take(N * D); w.v = take(N * D); w.z = take(N * 3 * D);
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
    w.dv = take(N * D); w.dqz = take(N * D); w.dO = take(N * D); w.dQp = take(N * D); w.S = take(NK * q.H);
    w.dKV = take(R * 2 * D); w.dE = take(R * D); w.dqa = take(N * D);
    w.gkv = take(kEtaSplitKV * 2 * DD); w.gq = take(kEtaSplitQ * DD); w.go = take(kEtaSplitO * DD);
    w.cs = take(2 * colsum_ws_floats(static_cast<int>(N), wide));
    w.cs_q = take(colsum_ws_floats(static_cast<int>(N), q.D)); w.cs_o = take(colsum_ws_floats(static_cast<int>(N), q.D));
    w.cs_k = take(colsum_ws_floats(static_cast<int>(R), q.D)); w.cs_v = take(colsum_ws_floats(static_cast<int>(R), q.D));
  }
  w.floats = p - base;
  return w;
}

std::atomic<uint64_t> eta_lds_ok{0};

int eta_allow_lds() {
  return allow_dynamic_lds({reinterpret_cast<const void*>(&eta_retrieve_kernel), reinterpret_cast<const void*>(&eta_pair_kernel<false>),
                            reinterpret_cast<const void*>(&eta_pair_kernel<true>)},
                           kEtaLdsBudget, eta_lds_ok, "the ETA retrieval and attention");
}

// codes, sel and the compaction of one batch, from the table (E, seq, cand) or from explicit rows (e, qrows, mask)
int eta_retrieve(const EtaDims& q, const float* hash, const float* E, const int64_t* seq, const int64_t* cand, const float* e,
                 const float* qrows, const uint8_t* mask, int64_t B, int64_t C, uint32_t* codes_e, uint32_t* codes_q,
                 int32_t* sel, const EtaWs& a, hiprec_stats* stats, hipStream_t st) {
  if (int rc = eta_allow_lds()) return rc;
  EtaRetrieve p{};
  p.T = q.T; p.C = static_cast<int>(C); p.D = q.D; p.m = q.m; p.Wd = q.Wd; p.k = q.k; p.U = eta_rows_per_seq(q, C);
  p.ldE = q.D + 4; p.n_items = q.n_items;
  const size_t lds = eta_retrieve_lds(q, &p.codes_lds);
  p.hash = hash; p.E = E; p.e = e; p.q = qrows; p.seq = seq; p.cand = cand; p.mask = mask;
  p.codes_e = codes_e; p.codes_q = codes_q; p.sel = sel; p.rank = a.rank; p.upos = a.upos; p.count = a.count; p.stats = stats;
  eta_retrieve_kernel<<<static_cast<int>(B), kBlock, lds, st>>>(p);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

// after the compaction: the row offsets and what every compact row is
int eta_row_list(const EtaDims& q, const int64_t* seq, int64_t B, int64_t C, const EtaWs& a, hipStream_t st) {
  const int U = eta_rows_per_seq(q, C);
  eta_offsets_kernel<<<1, kBlock, 0, st>>>(a.count, B, a.off);
  HIPREC_TRY(hipGetLastError());
  eta_rowid_kernel<<<grid_for_threads(B * U), kBlock, 0, st>>>(B, q.T, U, a.count, a.off, a.upos, seq, a.row_src, a.row_b,
                                                              a.row_id);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

EtaAttn eta_attn_of(const EtaDims& q, int64_t B, int64_t C, const EtaWs& a) {
  EtaAttn t{};
  t.C = static_cast<int>(C); t.D = q.D; t.H = q.H; t.dh = q.dh; t.k = q.k; t.N = B * C;
  t.scale = 1.0f / sqrtf(static_cast<float>(q.dh));
  t.rank = a.rank; t.off = a.off; t.KV = a.KV;
  return t;
}

// v [N, D] from the compact rows a.rows and the candidate rows qrows
int eta_attend_forward(const EtaDims& q, const EtaOff& o, const float* w_flat, const EtaWs& a, const float* qrows, int64_t B,
                       int64_t C, float* v, hipStream_t st) {
  const int D = q.D, N = static_cast<int>(B * C), R = static_cast<int>(B * eta_rows_per_seq(q, C));
  eta_stack_kernel<<<(D * D + kBlock - 1) / kBlock, kBlock, 0, st>>>(w_flat + o.kw, w_flat + o.kb, w_flat + o.vw, w_flat + o.vb, D,
                                                                      a.Wkv, a.bkv);
  HIPREC_TRY(hipGetLastError());
  GemmGroup g{};
  g.n = 2;
  g.p[0] = make_gemm(kNT, R, 2 * D, D, a.rows, D, a.Wkv, D, a.KV, 2 * D, a.bkv, 0, nullptr, 0, false);
  g.p[1] = make_gemm(kNT, N, D, D, qrows, D, w_flat + o.qw, D, a.Qp, D, w_flat + o.qb, 0, nullptr, 0, false);
  if (int rc = launch_group(g, st)) return rc;
  if (int rc = eta_allow_lds()) return rc;
  const EtaAttn t = eta_attn_of(q, B, C, a);
  eta_pair_kernel<false><<<(N + kWavesPerBlock - 1) / kWavesPerBlock, kBlock, eta_pair_lds(q), st>>>(t, a.Qp, a.P, nullptr, a.O);
  HIPREC_TRY(hipGetLastError());
  GemmGroup g2{};
  g2.n = 1;
  g2.p[0] = make_gemm(kNT, N, D, D, a.O, D, w_flat + o.ow, D, v, D, w_flat + o.ob, 0, nullptr, 0, false);
  return launch_group(g2, st);
}

// from dv [N, D]: the eight gradients of att.* into g_att (laid out like that span of the flat buffer, zero on entry),
// a.dE [rows, D] and a.dqa [N, D]
int eta_attend_backward(const EtaDims& q, const EtaOff& o, const float* w_flat, const EtaWs& a, const float* qrows,
                        const float* dv, int64_t B, int64_t C, float* g_att, hipStream_t st) {
  const int D = q.D, N = static_cast<int>(B * C), R = static_cast<int>(B * eta_rows_per_seq(q, C));
  const int64_t base = o.qw;
  GemmGroup g{};
  g.p[g.n++] = make_gemm(kNN, N, D, D, dv, D, w_flat + o.ow, D, a.dO, D, nullptr, 0, nullptr, 0, false);
  const int n_o = din_add_wgrad_slices(g, kEtaSplitO, D, D, N, dv, D, a.O, D, a.go);
  g.p[g.n++] = make_colsum(dv, N, D, D, g_att + (o.ob - base), a.cs_o);
  if (int rc = launch_group(g, st)) return rc;
  if (int rc = launch_colsum_reduce(g, st)) return rc;
  const EtaAttn t = eta_attn_of(q, B, C, a);
  eta_pair_kernel<true><<<(N + kWavesPerBlock - 1) / kWavesPerBlock, kBlock, eta_pair_lds(q), st>>>(t, a.dO, a.P, a.S, a.dQp);
  HIPREC_TRY(hipGetLastError());
  eta_row_bwd_kernel<<<grid_for_waves(R), kBlock, 0, st>>>(t, R, a.row_b, a.P, a.S, a.Qp, a.dO, a.dKV);
  HIPREC_TRY(hipGetLastError());
  GemmGroup h{};
  h.p[h.n++] = make_gemm(kNN, R, D, 2 * D, a.dKV, 2 * D, a.Wkv, D, a.dE, D, nullptr, 0, nullptr, 0, false);
  h.p[h.n++] = make_gemm(kNN, N, D, D, a.dQp, D, w_flat + o.qw, D, a.dqa, D, nullptr, 0, nullptr, 0, false);
  const int n_kv = din_add_wgrad_slices(h, kEtaSplitKV, 2 * D, D, R, a.dKV, 2 * D, a.rows, D, a.gkv);
  const int n_q = din_add_wgrad_slices(h, kEtaSplitQ, D, D, N, a.dQp, D, qrows, D, a.gq);
  h.p[h.n++] = make_colsum(a.dQp, N, D, D, g_att + (o.qb - base), a.cs_q);
  h.p[h.n++] = make_colsum(a.dKV, R, D, 2 * D, g_att + (o.kb - base), a.cs_k);
  h.p[h.n++] = make_colsum(a.dKV + D, R, D, 2 * D, g_att + (o.vb - base), a.cs_v);
  static_assert(kEtaSplitKV + kEtaSplitQ + 5 <= kMaxGroup && kEtaSplitO + 2 <= kMaxGroup, "one grouped launch each");
  if (int rc = launch_group(h, st)) return rc;
  if (int rc = launch_colsum_reduce(h, st)) return rc;
  eta_fold_kernel<<<(D * D + kBlock - 1) / kBlock, kBlock, 0, st>>>(a.gq, n_q, a.gkv, n_kv, a.go, n_o, D, g_att + (o.qw - base),
                                                                     g_att + (o.kw - base), g_att + (o.vw - base),
                                                                     g_att + (o.ow - base));
  HIPREC_TRY(hipGetLastError());
  return 0;
}

DinTower eta_tower_of(const EtaDims& q, const EtaOff& o, const EtaWs& a) {
  DinTower t{};
  t.L = q.L; t.act = q.dnn_act; t.ow = o.outw; t.ob = o.outb;
  for (int l = 0; l < q.L; ++l) {
    t.W[l] = q.W[l]; t.in[l] = o.in[l]; t.bn[l] = o.bn[l]; t.dw[l] = o.dw[l]; t.db[l] = o.db[l]; t.da[l] = o.da[l];
    t.x[l] = a.x[l]; t.y[l] = a.y[l];
  }
  t.mean = a.mean; t.var = a.var; t.logit = a.logit; t.dlogit = a.dlogit; t.dA = a.dA; t.dB = a.dB; t.sums = a.sums; t.cs = a.cs;
  return t;
}

int eta_run(const EtaDims& q, const float* w_flat, const float* hash, float* g_flat, float* bn, int update_running,
            const int64_t* seq, const int64_t* cand, const float* label, int64_t B, int64_t C, float* logits_out,
            hiprec_stats* stats, Scratch* scratch, float* ws_base, hipStream_t st) {
  const bool train = g_flat != nullptr;
  const EtaOff o = eta_offsets(q);
  const EtaWs a = eta_carve_ws(ws_base, q, B, C, train);
  const int64_t N = B * C, R = B * eta_rows_per_seq(q, C);
  const int D = q.D;
  if (int rc = eta_retrieve(q, hash, w_flat, seq, cand, nullptr, nullptr, nullptr, B, C, a.codes_e, a.codes_q, a.sel, a, stats, st))
    return rc;
  if (int rc = eta_row_list(q, seq, B, C, a, st)) return rc;
  if (int rc = din_gather(w_flat, q.n_items, D, a.row_id, cand, R, N, a.rows, a.q, a.lv, a.lc, stats, st)) return rc;
  if (int rc = eta_attend_forward(q, o, w_flat, a, a.q, B, C, a.v, st)) return rc;
  if (int rc = din_z(a.v, a.q, N, D, a.z, st)) return rc;
  const DinTower tw = eta_tower_of(q, o, a);
  if (int rc = din_tower_forward(tw, w_flat, bn, update_running, train, a.z, a.lc, N, logits_out, stats, st)) return rc;
  if (!train) return 0;
  float* dz = nullptr;
  if (int rc = din_tower_backward(tw, w_flat, g_flat, a.z, a.lc, label, N, logits_out, scratch, stats, st, &dz)) return rc;
  if (int rc = din_z_bwd(dz, a.v, a.q, N, D, a.dv, a.dqz, st)) return rc;
  if (int rc = eta_attend_backward(q, o, w_flat, a, a.q, a.dv, B, C, g_flat + o.qw, st)) return rc;
  return din_scatter(a.dE, a.dqa, a.dqz, a.row_id, cand, a.lv, a.lc, R, N, D, g_flat, st);
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_eta_shape_bytes(void) { return sizeof(hiprec_eta_shape); }

extern "C" int64_t hiprec_eta_param_floats(const hiprec_eta_shape* shape) {
  if (eta_check_shape(shape)) return -1;
  return eta_offsets(eta_dims(*shape)).total;
}

extern "C" int hiprec_eta_tiles(const hiprec_eta_shape* shape, int64_t n_cand, int32_t* out) {
  if (int rc = eta_check_shape(shape)) return rc;
  HIPREC_REQUIRE(out && n_cand >= 1 && n_cand <= kDinMaxRows, "hiprec_eta_tiles needs out and 1 <= n_cand <= 2^24");
  const EtaDims q = eta_dims(*shape);
  int codes_lds = 0;
  eta_retrieve_lds(q, &codes_lds);
  out[0] = kEtaChunk; out[1] = q.Wd; out[2] = codes_lds; out[3] = eta_rows_per_seq(q, n_cand); out[4] = kWavesPerBlock;
  out[5] = kEtaSplitKV;
  return 0;
}

extern "C" size_t hiprec_eta_workspace_bytes(const hiprec_eta_shape* shape, int64_t batch, int64_t n_cand, int32_t train) {
  if (eta_check_shape(shape)) return 0;
  const EtaDims q = eta_dims(*shape);
  if (!eta_batch_ok(q, batch, n_cand)) return 0;
  return sizeof(float) * static_cast<size_t>(eta_carve_ws(nullptr, q, batch, n_cand, train != 0).floats);
}

#define ETA_BATCH_MSG "ETA needs batch >= 1, n_cand >= 1, batch * maxlen <= 2^24 and batch * n_cand * top_k <= 2^24"

extern "C" int hiprec_eta_grad(const hiprec_eta_shape* shape, const float* w_flat, const float* hash_weight, float* g_flat,
                               float* running, int32_t update_running, const int64_t* seq, const int64_t* cand,
                               const float* label, int64_t batch, int64_t n_cand, float* logits_out, hiprec_stats* stats,
                               void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = eta_check_shape(shape)) return rc;
  const EtaDims q = eta_dims(*shape);
  HIPREC_REQUIRE(w_flat && hash_weight && running && seq && cand && stats && workspace, "NULL pointer");
  HIPREC_REQUIRE(eta_batch_ok(q, batch, n_cand), ETA_BATCH_MSG " (got %lld, %lld)", static_cast<long long>(batch),
                 static_cast<long long>(n_cand));
  if (g_flat) {
    HIPREC_REQUIRE(label && scratch, "training needs the labels and the scratch block");
    if (scratch_bytes < kScratchBytes) {
      set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
      return HIPREC_E_SCRATCH;
    }
  } else {
    HIPREC_REQUIRE(logits_out, "the eval forward needs the logits buffer");
  }
  const size_t need = hiprec_eta_workspace_bytes(shape, batch, n_cand, g_flat != nullptr);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  return eta_run(q, w_flat, hash_weight, g_flat, running, update_running, seq, cand, label, batch, n_cand, logits_out, stats,
                 static_cast<Scratch*>(scratch), static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_eta_retrieve(const hiprec_eta_shape* shape, const float* hash_weight, const float* e, const float* q_rows,
                                   const uint8_t* mask, int64_t batch, int64_t n_cand, uint32_t* codes_e, uint32_t* codes_q,
                                   int32_t* sel, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = eta_check_shape(shape)) return rc;
  const EtaDims q = eta_dims(*shape);
  HIPREC_REQUIRE(hash_weight && e && q_rows && mask && codes_e && codes_q && sel && workspace, "NULL pointer");
  HIPREC_REQUIRE(eta_batch_ok(q, batch, n_cand), ETA_BATCH_MSG);
  const size_t need = hiprec_eta_workspace_bytes(shape, batch, n_cand, 0);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  const EtaWs a = eta_carve_ws(static_cast<float*>(workspace), q, batch, n_cand, false);
  return eta_retrieve(q, hash_weight, nullptr, nullptr, nullptr, e, q_rows, mask, batch, n_cand, codes_e, codes_q, sel, a, nullptr,
                      static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_eta_attention(const hiprec_eta_shape* shape, const float* w_flat, const float* e, const float* q_rows,
                                    const int32_t* sel, int64_t batch, int64_t n_cand, float* v, const float* dv, float* g_att,
                                    float* de, float* dq, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = eta_check_shape(shape)) return rc;
  const EtaDims q = eta_dims(*shape);
  HIPREC_REQUIRE(w_flat && e && q_rows && sel && v && workspace, "NULL pointer");
  HIPREC_REQUIRE(eta_batch_ok(q, batch, n_cand), ETA_BATCH_MSG);
  const bool bwd = dv != nullptr;
  HIPREC_REQUIRE(!bwd || (g_att && de && dq), "the stage's backward needs g_att, de and dq");
  const size_t need = hiprec_eta_workspace_bytes(shape, batch, n_cand, bwd);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const EtaOff o = eta_offsets(q);
  EtaWs a = eta_carve_ws(static_cast<float*>(workspace), q, batch, n_cand, bwd);
  const int U = eta_rows_per_seq(q, n_cand);
  const int64_t N = batch * n_cand, R = batch * U;
  eta_compact_kernel<<<static_cast<int>(batch), kBlock, 0, st>>>(q.T, static_cast<int>(n_cand) * q.k, U, sel, a.rank, a.upos, a.count);
  HIPREC_TRY(hipGetLastError());
  if (int rc = eta_row_list(q, nullptr, batch, n_cand, a, st)) return rc;
  eta_rows_kernel<<<grid_for_waves(std::max(R, N / kWave + 1)), kBlock, 0, st>>>(e, a.row_src, R, q.D, a.rows, a.lv, a.lc, N);
  HIPREC_TRY(hipGetLastError());
  if (int rc = eta_attend_forward(q, o, w_flat, a, q_rows, batch, n_cand, v, st)) return rc;
  if (!bwd) return 0;
  if (int rc = eta_attend_backward(q, o, w_flat, a, q_rows, dv, batch, n_cand, g_att, st)) return rc;
  if (int rc = din_fill(de, batch * q.T * q.D, 0.f, st)) return rc;
  eta_rows_back_kernel<<<grid_for_waves(R), kBlock, 0, st>>>(a.dE, a.row_src, R, q.D, de);
  HIPREC_TRY(hipGetLastError());
  HIPREC_TRY(hipMemcpyAsync(dq, a.dqa, sizeof(float) * N * q.D, hipMemcpyDeviceToDevice, st));
  return 0;
}
