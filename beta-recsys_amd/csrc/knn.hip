// ItemKNN / UserKNN (models/itemKNN.py, models/userKNN.py): sparse set intersection, a small selection and a weighted
// scatter.  No optimizer, no GEMM, no autograd.
//
// The overlap walk serves both models: a row's overlap with every other row is "for each column c of my row, for each
// row r of the transposed matrix at c, add B[r, c]".  Overlaps are integers and are accumulated as integers, so their
// sum does not depend on the order the block's lanes arrive in; everything that is rounded (overlap / sqrt(mass) in
// fp64, the fp32 / fp64 score sums) has one owner and a fixed order.  No device-scope atomics anywhere: the only
// atomics are the block's own integer adds into its own accumulator.
//
//   knn_item_sim_kernel     one block per row i of S: overlaps of column i with every column, scaled, rounded to fp32,
//                           written with plain stores (the whole row: zeros where nothing overlaps).
//   knn_item_scores_kernel  one block per query user: one thread per column adds S[i, j] over the user's items in
//                           ascending order (coalesced across the column tile), then the output stage.
//   knn_user_kernel         one block per query user, fused: overlaps with all users -> sim in fp64 -> the k best by
//                           (fp64 value, lower id) -> for each neighbour, best first, acc[j] += sim * B[v, j] with a
//                           barrier between neighbours (a neighbour's row has distinct items) -> own items to -inf ->
//                           the output stage.
//   output stage            pick pair items out of the row, and / or the top K of the row under a seen mask: K rounds of
//                           a block-wide minimum over topk.hip's 64-bit keys (score bits made orderable, item id in the
//                           low word: ties to the lower id, -0 == +0); a round takes the best key behind the one before.
//
// Accumulator placement: the block's dense accumulator lives in LDS while it has at most lds_cap entries (at most
// HIPREC_KNN_LDS_CAP: 56 KB of the 64 KB a block gets without asking for more), else in the block's slice of the
// caller's workspace.  The workspace form relies on its slice being zero between uses and restores that through the list
// of entries it touched (kept behind the accumulator in the slice), never by sweeping the slice; the entry point zeroes
// the workspace once per call.  The LDS form sweeps: LDS is cheap to clear.  Both forms run the same arithmetic in the
// same order, so the result does not depend on the placement.
#include "common.hpp"

namespace hiprec {
namespace {

constexpr int kKnnMaxBlocks = 1024;          // blocks (= workspace slices) per launch; rows / queries beyond are strided
constexpr uint64_t kKnnNone = ~0ull;         // no candidate: worse than every key

// topk.hip's key encoding (that file's measured evidence is stamped by its hash, so it is restated, not shared)
__device__ __forceinline__ uint64_t knn_key(float score, uint32_t item) {
  if (score == 0.0f) score = 0.0f;  // -0 ties with +0
  uint32_t u = __float_as_uint(score);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending-orderable
  return (static_cast<uint64_t>(~u) << 32) | item;  // smaller key == better candidate
}

__device__ __forceinline__ float knn_key_score(uint64_t key) {
  const uint32_t u = ~static_cast<uint32_t>(key >> 32);
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

__device__ __forceinline__ uint64_t dbits(double x) { return static_cast<uint64_t>(__double_as_longlong(x)); }
__device__ __forceinline__ double bits_d(uint64_t b) { return __longlong_as_double(static_cast<long long>(b)); }

// Block-wide minimum of a 64-bit key, uniform over the block.  `red`: kWavesPerBlock words of LDS, free again on return.
__device__ __forceinline__ uint64_t block_min_u64(uint64_t v, uint64_t* red) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const uint64_t o = __shfl_xor(static_cast<unsigned long long>(v), off, kWave);
    v = o < v ? o : v;
  }
  if (lane_id() == 0) red[wave_in_block()] = v;
  __syncthreads();
  uint64_t r = red[0];
#pragma unroll
  for (int w = 1; w < kWavesPerBlock; ++w) r = red[w] < r ? red[w] : r;
  __syncthreads();
  return r;
}

// A neighbour candidate: the complement of the fp64 bits of a positive sim (larger sim = smaller inv), then the id.
struct SimKey {
  uint64_t inv;
  uint32_t id;
};

__device__ __forceinline__ bool sim_better(const SimKey& a, const SimKey& b) {
  return a.inv < b.inv || (a.inv == b.inv && a.id < b.id);
}

__device__ __forceinline__ SimKey block_best_sim(SimKey v, uint64_t* red, uint32_t* red_id) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    SimKey o;
    o.inv = __shfl_xor(static_cast<unsigned long long>(v.inv), off, kWave);
    o.id = __shfl_xor(v.id, off, kWave);
    if (sim_better(o, v)) v = o;
  }
  if (lane_id() == 0) {
    red[wave_in_block()] = v.inv;
    red_id[wave_in_block()] = v.id;
  }
  __syncthreads();
  SimKey r{red[0], red_id[0]};
#pragma unroll
  for (int w = 1; w < kWavesPerBlock; ++w) {
    const SimKey o{red[w], red_id[w]};
    if (sim_better(o, r)) r = o;
  }
  __syncthreads();
  return r;
}

// What the output stage is asked for (shared by both score kernels)
struct KnnOut {
  const int64_t* pair_ptr;     // [n_query + 1] or nullptr
  const int64_t* pair_items;
  void* out_pick;              // float (ItemKNN) / double (UserKNN)
  const int64_t* seen_ptr;     // [n_users + 1] or nullptr
  const int64_t* seen_idx;
  int64_t* out_items;          // [n_query, topk]
  float* out_scores;
  hiprec_stats* stats;
  int32_t topk;
};

// The fp32 score row of the ItemKNN kernel
struct FloatRow {
  float* p;
  using value_t = float;
  __device__ __forceinline__ float value(int64_t j) const { return p[j]; }
  __device__ __forceinline__ float score(int64_t j) const { return p[j]; }
  __device__ __forceinline__ void mask(int64_t j) const { p[j] = -INFINITY; }
};

// The fp64 score row of the UserKNN kernel: fp64 bits in the block's 64-bit accumulator.  WS: an entry that leaves
// zero is entered into the touched list first (an entry is written by one thread between two barriers).
template <bool WS>
struct DoubleRow {
  uint64_t* acc;
  int32_t* touched;
  unsigned* n_touched;
  unsigned cap;
  using value_t = double;
  __device__ __forceinline__ void note(int64_t j) const {
    if constexpr (WS) {
      if (acc[j] == 0) {
        const unsigned pos = atomicAdd(n_touched, 1u);
        if (pos < cap) touched[pos] = static_cast<int32_t>(j);  // (distinct entries: never more than the slice holds)
      }
    }
  }
  __device__ __forceinline__ double value(int64_t j) const { return bits_d(acc[j]); }
  __device__ __forceinline__ float score(int64_t j) const { return static_cast<float>(bits_d(acc[j])); }
  __device__ __forceinline__ void mask(int64_t j) const {
    note(j);
    acc[j] = dbits(-INFINITY);
  }
};

// The output stage for query q (user `user`, or -1: out of range) over a finished score row.  Called by the whole
// block; the row is complete and visible (a barrier lies behind its last write).  Masks the seen items IN the row.
template <typename Row>
__device__ __forceinline__ void knn_output_stage(const Row& row, const KnnOut& o, int64_t q, int64_t user,
                                                 int64_t n_items, uint64_t* red) {
  using T = typename Row::value_t;
  const int tid = static_cast<int>(threadIdx.x);
  if (o.pair_ptr != nullptr) {
    T* out = static_cast<T*>(o.out_pick);
    for (int64_t p = o.pair_ptr[q] + tid; p < o.pair_ptr[q + 1]; p += kBlock) {
      const int64_t item = o.pair_items[p];
      const bool ok = item >= 0 && item < n_items;
      if (!ok) atomicOr(&o.stats->status, HIPREC_STATUS_ITEM_OOB);
      out[p] = (ok && user >= 0) ? row.value(item) : static_cast<T>(0);
    }
  }
  if (o.topk <= 0) return;
  int64_t* items = o.out_items + q * o.topk;
  float* scores = o.out_scores + q * o.topk;
  if (user < 0) {
    for (int r = tid; r < o.topk; r += kBlock) items[r] = -1, scores[r] = -INFINITY;
    return;
  }
  __syncthreads();  // the picks have read the row
  if (o.seen_ptr != nullptr) {
    for (int64_t e = o.seen_ptr[user] + tid; e < o.seen_ptr[user + 1]; e += kBlock) {
      const int64_t j = o.seen_idx[e];
      if (j >= 0 && j < n_items) row.mask(j);
    }
    __syncthreads();
  }
  uint64_t prev = 0;
  for (int r = 0; r < o.topk; ++r) {
    uint64_t best = kKnnNone;
    for (int64_t j = tid; j < n_items; j += kBlock) {
      const float s = row.score(j);
      if (s == -INFINITY) continue;  // masked (seen, or the user's own items in UserKNN): never returned
      const uint64_t key = knn_key(s, static_cast<uint32_t>(j));
      if ((r == 0 || key > prev) && key < best) best = key;
    }
    best = block_min_u64(best, red);
    if (best == kKnnNone) {  // fewer than topk candidates: the tail
      for (int t = r + tid; t < o.topk; t += kBlock) items[t] = -1, scores[t] = -INFINITY;
      break;
    }
    if (tid == 0) {
      items[r] = static_cast<int64_t>(best & 0xffffffffull);
      scores[r] = knn_key_score(best);
    }
    prev = best;
  }
}

// ---------------------------------------------------------------- ItemKNN: the similarity matrix
struct KnnSimArgs {
  const int64_t* bt_ptr;
  const int64_t* bt_idx;
  const int64_t* b_ptr;
  const int64_t* b_idx;
  const float* b_val;
  const double* cnt;
  float* S;
  void* ws;
  int64_t n_users, n_items, lds, slice_bytes;
};

template <bool WS>
__global__ __launch_bounds__(kBlock) void knn_item_sim_kernel(const KnnSimArgs a) {
  extern __shared__ uint64_t knn_lds[];
  __shared__ unsigned s_touched;
  const int tid = static_cast<int>(threadIdx.x), lane = lane_id(), wv = wave_in_block();
  char* slice = WS ? static_cast<char*>(a.ws) + static_cast<size_t>(blockIdx.x) * a.slice_bytes : nullptr;
  unsigned* acc = WS ? reinterpret_cast<unsigned*>(slice) : reinterpret_cast<unsigned*>(knn_lds);
  int32_t* touched = WS ? reinterpret_cast<int32_t*>(slice) + a.n_items : nullptr;
  if constexpr (!WS) {
    for (int64_t j = tid; j < a.n_items; j += kBlock) acc[j] = 0;
  }
  if (tid == 0) s_touched = 0;
  __syncthreads();

  for (int64_t i = blockIdx.x; i < a.n_items; i += gridDim.x) {
    // one wave per user of column i, its lanes over the user's row
    for (int64_t e = a.bt_ptr[i] + wv; e < a.bt_ptr[i + 1]; e += kWavesPerBlock) {
      const int64_t v = a.bt_idx[e];
      if (v < 0 || v >= a.n_users) continue;
      for (int64_t t = a.b_ptr[v] + lane; t < a.b_ptr[v + 1]; t += kWave) {
        const int64_t j = a.b_idx[t];
        if (j < 0 || j >= a.n_items) continue;
        const unsigned old = atomicAdd(&acc[j], static_cast<unsigned>(a.b_val[t]));
        if constexpr (WS) {
          if (old == 0) {
            const unsigned pos = atomicAdd(&s_touched, 1u);
            if (pos < static_cast<unsigned>(a.n_items)) touched[pos] = static_cast<int32_t>(j);
          }
        }
      }
    }
    __syncthreads();
    float* out = a.S + i * a.lds;
    if constexpr (WS) {
      for (int64_t j = tid; j < a.n_items; j += kBlock) out[j] = 0.f;
      __syncthreads();
      const unsigned n = s_touched;
      for (unsigned t = tid; t < n; t += kBlock) {
        const int32_t j = touched[t];
        out[j] = static_cast<float>(static_cast<double>(acc[j]) / sqrt(a.cnt[j]));
        acc[j] = 0;
      }
      __syncthreads();
      if (tid == 0) s_touched = 0;
    } else {
      for (int64_t j = tid; j < a.n_items; j += kBlock) {
        const unsigned ov = acc[j];
        out[j] = ov != 0 ? static_cast<float>(static_cast<double>(ov) / sqrt(a.cnt[j])) : 0.f;
        acc[j] = 0;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- ItemKNN: score rows
struct KnnItemArgs {
  const int64_t* b_ptr;
  const int64_t* b_idx;
  const float* S;
  const int64_t* query;
  void* ws;
  KnnOut out;
  int64_t n_users, n_items, lds, n_query;
};

template <bool WS>
__global__ __launch_bounds__(kBlock) void knn_item_scores_kernel(const KnnItemArgs a) {
  extern __shared__ uint64_t knn_lds[];
  __shared__ uint64_t s_red[kWavesPerBlock];
  const int tid = static_cast<int>(threadIdx.x);
  FloatRow row{WS ? static_cast<float*>(a.ws) + static_cast<size_t>(blockIdx.x) * a.n_items
                  : reinterpret_cast<float*>(knn_lds)};
  for (int64_t q = blockIdx.x; q < a.n_query; q += gridDim.x) {
    int64_t user = a.query[q];
    if (user < 0 || user >= a.n_users) {
      if (tid == 0) atomicOr(&a.out.stats->status, HIPREC_STATUS_USER_OOB);
      user = -1;
    } else {
      const int64_t r0 = a.b_ptr[user], r1 = a.b_ptr[user + 1];
      for (int64_t j = tid; j < a.n_items; j += kBlock) {
        float acc = 0.f;  // (S >= +0, so 0 + S[i0, j] is S[i0, j] to the bit: the reference starts from the row itself)
        int64_t e = r0;
        for (; e + 8 <= r1; e += 8) {  // eight loads in flight, added in the same ascending order
          float s[8];
#pragma unroll
          for (int t = 0; t < 8; ++t) s[t] = a.S[a.b_idx[e + t] * a.lds + j];
#pragma unroll
          for (int t = 0; t < 8; ++t) acc = acc + s[t];
        }
        for (; e < r1; ++e) acc = acc + a.S[a.b_idx[e] * a.lds + j];
        row.p[j] = acc;
      }
    }
    __syncthreads();
    knn_output_stage(row, a.out, q, user, a.n_items, s_red);
    __syncthreads();  // the row is free for the next query
  }
}

// ---------------------------------------------------------------- UserKNN: fused
struct KnnUserArgs {
  const int64_t* b_ptr;
  const int64_t* b_idx;
  const float* b_val;
  const int64_t* bt_ptr;
  const int64_t* bt_idx;
  const float* bt_val;
  const double* cu;
  const int64_t* query;
  int64_t* out_nb_ids;
  double* out_nb_sims;
  void* ws;
  KnnOut out;
  int64_t n_users, n_items, n_acc, n_query, slice_bytes;
  int32_t k;
};

template <bool WS>
__global__ __launch_bounds__(kBlock) void knn_user_kernel(const KnnUserArgs a) {
  extern __shared__ uint64_t knn_lds[];
  __shared__ uint64_t s_red[kWavesPerBlock];
  __shared__ uint32_t s_red_id[kWavesPerBlock];
  __shared__ int32_t s_nb_id[HIPREC_KNN_MAX_K];
  __shared__ double s_nb_sim[HIPREC_KNN_MAX_K];
  __shared__ unsigned s_touched;
  const int tid = static_cast<int>(threadIdx.x), lane = lane_id(), wv = wave_in_block();
  char* slice = WS ? static_cast<char*>(a.ws) + static_cast<size_t>(blockIdx.x) * a.slice_bytes : nullptr;
  uint64_t* acc = WS ? reinterpret_cast<uint64_t*>(slice) : knn_lds;
  int32_t* touched = WS ? reinterpret_cast<int32_t*>(acc + a.n_acc) : nullptr;
  if constexpr (!WS) {
    for (int64_t e = tid; e < a.n_acc; e += kBlock) acc[e] = 0;
  }
  if (tid == 0) s_touched = 0;
  __syncthreads();
  const DoubleRow<WS> row{acc, touched, &s_touched, static_cast<unsigned>(a.n_acc)};
  const int k = a.k;

  for (int64_t q = blockIdx.x; q < a.n_query; q += gridDim.x) {
    const int64_t user = a.query[q];
    if (user < 0 || user >= a.n_users) {  // (uniform over the block)
      if (tid == 0) atomicOr(&a.out.stats->status, HIPREC_STATUS_USER_OOB);
      if (a.out_nb_ids != nullptr)
        for (int r = tid; r < k; r += kBlock) a.out_nb_ids[q * k + r] = -1, a.out_nb_sims[q * k + r] = 0.0;
      knn_output_stage(row, a.out, q, -1, a.n_items, s_red);
      continue;
    }
    const int64_t r0 = a.b_ptr[user], r1 = a.b_ptr[user + 1];

    // 1. overlaps with every user, as integers: one wave per item of the query user, its lanes over the item's users
    for (int64_t e = r0 + wv; e < r1; e += kWavesPerBlock) {
      const int64_t j = a.b_idx[e];
      if (j < 0 || j >= a.n_items) continue;
      for (int64_t t = a.bt_ptr[j] + lane; t < a.bt_ptr[j + 1]; t += kWave) {
        const int64_t v = a.bt_idx[t];
        if (v < 0 || v >= a.n_users) continue;
        const unsigned long long old = atomicAdd(reinterpret_cast<unsigned long long*>(&acc[v]),
                                                 static_cast<unsigned long long>(a.bt_val[t]));
        if constexpr (WS) {
          if (old == 0) {
            const unsigned pos = atomicAdd(&s_touched, 1u);
            if (pos < static_cast<unsigned>(a.n_acc)) touched[pos] = static_cast<int32_t>(v);
          }
        }
      }
    }
    __syncthreads();

    // 2. sim = overlap / sqrt(mass) in fp64, in place
    const int64_t n_cand = WS ? static_cast<int64_t>(s_touched) : a.n_users;
    for (int64_t c = tid; c < n_cand; c += kBlock) {
      const int64_t v = WS ? touched[c] : c;
      const uint64_t ov = acc[v];
      if (ov != 0) acc[v] = dbits(static_cast<double>(ov) / sqrt(a.cu[v]));
    }
    __syncthreads();

    // 3. the k best by (sim, lower id): a round takes the best and marks it -1; when no positive sim is left the
    //    users with sim 0 follow in ascending id
    int n_pos = 0;
    for (; n_pos < k; ++n_pos) {
      SimKey best{kKnnNone, 0xffffffffu};
      for (int64_t c = tid; c < n_cand; c += kBlock) {
        const int64_t v = WS ? touched[c] : c;
        const uint64_t b = acc[v];
        if (bits_d(b) > 0.0) {
          const SimKey cand{~b, static_cast<uint32_t>(v)};
          if (sim_better(cand, best)) best = cand;
        }
      }
      best = block_best_sim(best, s_red, s_red_id);
      if (best.inv == kKnnNone) break;
      if (tid == 0) {
        s_nb_id[n_pos] = static_cast<int32_t>(best.id);
        s_nb_sim[n_pos] = bits_d(~best.inv);
        acc[best.id] = dbits(-1.0);
      }
      __syncthreads();
    }
    if (n_pos < k && tid == 0) {
      int f = n_pos;
      for (int64_t v = 0; v < a.n_users && f < k; ++v) {
        if (acc[v] == 0) s_nb_id[f] = static_cast<int32_t>(v), s_nb_sim[f] = 0.0, ++f;
      }
      for (; f < k; ++f) s_nb_id[f] = -1, s_nb_sim[f] = 0.0;  // (k <= n_users: not reached)
    }
    __syncthreads();
    if (a.out_nb_ids != nullptr) {
      for (int r = tid; r < k; r += kBlock) {
        a.out_nb_ids[q * k + r] = s_nb_id[r];
        a.out_nb_sims[q * k + r] = s_nb_sim[r];
      }
    }

    // 4. the accumulator back to zero: it becomes the score row
    for (int64_t c = tid; c < n_cand; c += kBlock) acc[WS ? touched[c] : c] = 0;
    __syncthreads();
    if (tid == 0) s_touched = 0;
    __syncthreads();

    // 5. scores: one neighbour at a time, best first; a neighbour's row has distinct items, so every entry has one
    //    writer between two barriers.  The product is rounded before it is added, as the reference's is.
    for (int r = 0; r < n_pos; ++r) {
      const int64_t v = s_nb_id[r];
      const double s = s_nb_sim[r];
      for (int64_t e = a.b_ptr[v] + tid; e < a.b_ptr[v + 1]; e += kBlock) {
        const int64_t j = a.b_idx[e];
        if (j < 0 || j >= a.n_items) continue;
        row.note(j);
        {
#pragma clang fp contract(off)
          const double p = s * static_cast<double>(a.b_val[e]);
          acc[j] = dbits(bits_d(acc[j]) + p);
        }
      }
      __syncthreads();
    }

    // 6. the user's own items
    for (int64_t e = r0 + tid; e < r1; e += kBlock) {
      const int64_t j = a.b_idx[e];
      if (j >= 0 && j < a.n_items) row.mask(j);
    }
    __syncthreads();

    knn_output_stage(row, a.out, q, user, a.n_items, s_red);
    __syncthreads();

    // 7. the row back to zero
    if constexpr (WS) {
      const unsigned n = s_touched;
      for (unsigned c = tid; c < n; c += kBlock) acc[touched[c]] = 0;
    } else {
      for (int64_t j = tid; j < a.n_items; j += kBlock) acc[j] = 0;
    }
    __syncthreads();
    if (tid == 0) s_touched = 0;
    __syncthreads();
  }
}

// ---------------------------------------------------------------- host side
constexpr int64_t kKnnMaxDim = 0x7fffffffll;

bool knn_sizes_ok(int32_t op, int64_t n_users, int64_t n_items, int64_t n_query, int32_t lds_cap) {
  return op >= HIPREC_KNN_OP_ITEM_SIMILARITY && op <= HIPREC_KNN_OP_USER_SCORES && n_users >= 1 && n_items >= 1 &&
         n_users < kKnnMaxDim && n_items < kKnnMaxDim && n_query >= 0 && lds_cap >= 0;
}

int64_t knn_acc_entries(int32_t op, int64_t n_users, int64_t n_items) {
  return op == HIPREC_KNN_OP_USER_SCORES ? (n_users > n_items ? n_users : n_items) : n_items;
}

bool knn_in_lds(int32_t op, int64_t n_users, int64_t n_items, int32_t lds_cap) {
  const int64_t cap = (lds_cap == 0 || lds_cap > HIPREC_KNN_LDS_CAP) ? HIPREC_KNN_LDS_CAP : lds_cap;
  return knn_acc_entries(op, n_users, n_items) <= cap;
}

int64_t knn_blocks(int32_t op, int64_t n_items, int64_t n_query) {
  const int64_t n = op == HIPREC_KNN_OP_ITEM_SIMILARITY ? n_items : n_query;
  return n < 1 ? 1 : (n > kKnnMaxBlocks ? kKnnMaxBlocks : n);
}

size_t knn_slice_bytes(int32_t op, int64_t n_users, int64_t n_items) {
  const size_t n = static_cast<size_t>(knn_acc_entries(op, n_users, n_items));
  if (op == HIPREC_KNN_OP_ITEM_SIMILARITY) return n * 8;                      // uint32 overlaps + int32 touched list
  if (op == HIPREC_KNN_OP_ITEM_SCORES) return n * 4;                          // the fp32 row
  return n * 8 + ((n * 4 + 7) / 8) * 8;                                       // 64-bit accumulator + int32 touched list
}

int knn_check_out(const char* what, int64_t n_query, const int64_t* pair_ptr, const int64_t* pair_items,
                  const void* out_pick, int32_t topk, const int64_t* seen_ptr, const int64_t* seen_idx,
                  const int64_t* out_items, const float* out_scores, const hiprec_stats* stats) {
  HIPREC_REQUIRE(topk >= 0 && topk <= HIPREC_KNN_MAX_K, "%s: topk=%d outside 0..%d", what, topk, HIPREC_KNN_MAX_K);
  if (n_query == 0) return 0;
  HIPREC_REQUIRE(stats != nullptr, "%s: NULL stats", what);
  HIPREC_REQUIRE(pair_ptr == nullptr || (pair_items != nullptr && out_pick != nullptr),
                 "%s: a pair list needs pair_ptr, pair_items and out_pick", what);
  HIPREC_REQUIRE(topk == 0 || (out_items != nullptr && out_scores != nullptr),
                 "%s: topk=%d needs out_items and out_scores", what, topk);
  HIPREC_REQUIRE((seen_ptr == nullptr) == (seen_idx == nullptr),
                 "%s: the seen-item CSR needs both seen_ptr and seen_idx (or neither)", what);
  return 0;
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_knn_workspace_bytes(int32_t op, int64_t n_users, int64_t n_items, int64_t n_query,
                                             int32_t lds_cap) {
  if (!knn_sizes_ok(op, n_users, n_items, n_query, lds_cap)) return static_cast<size_t>(-1);
  if (knn_in_lds(op, n_users, n_items, lds_cap)) return 0;
  return static_cast<size_t>(knn_blocks(op, n_items, n_query)) * knn_slice_bytes(op, n_users, n_items);
}

extern "C" int hiprec_knn_item_similarity(const int64_t* bt_ptr, const int64_t* bt_idx, const int64_t* b_ptr,
                                          const int64_t* b_idx, const float* b_val, const double* cnt, int64_t n_users,
                                          int64_t n_items, float* S, int64_t lds, int32_t lds_cap, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  const int32_t op = HIPREC_KNN_OP_ITEM_SIMILARITY;
  HIPREC_REQUIRE(knn_sizes_ok(op, n_users, n_items, 0, lds_cap),
                 "knn_item_similarity: bad sizes (n_users=%lld n_items=%lld lds_cap=%d)", (long long)n_users,
                 (long long)n_items, lds_cap);
  HIPREC_REQUIRE(lds >= n_items, "knn_item_similarity: leading dimension %lld < n_items=%lld", (long long)lds,
                 (long long)n_items);
  HIPREC_REQUIRE(bt_ptr && bt_idx && b_ptr && b_idx && b_val && cnt && S, "knn_item_similarity: NULL pointer");
  const size_t need = hiprec_knn_workspace_bytes(op, n_users, n_items, 0, lds_cap);
  HIPREC_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need),
                 "knn_item_similarity: workspace %zu B < %zu B", workspace_bytes, need);
  KnnSimArgs a{};
  a.bt_ptr = bt_ptr, a.bt_idx = bt_idx, a.b_ptr = b_ptr, a.b_idx = b_idx, a.b_val = b_val, a.cnt = cnt, a.S = S;
  a.ws = workspace, a.n_users = n_users, a.n_items = n_items, a.lds = lds;
  a.slice_bytes = static_cast<int64_t>(knn_slice_bytes(op, n_users, n_items));
  auto s = static_cast<hipStream_t>(stream);
  const unsigned grid = static_cast<unsigned>(knn_blocks(op, n_items, 0));
  if (need == 0) {
    knn_item_sim_kernel<false><<<grid, kBlock, sizeof(unsigned) * static_cast<size_t>(n_items), s>>>(a);
  } else {
    HIPREC_TRY(hipMemsetAsync(workspace, 0, need, s));
    knn_item_sim_kernel<true><<<grid, kBlock, 0, s>>>(a);
  }
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_knn_item_scores(const int64_t* b_ptr, const int64_t* b_idx, int64_t n_users, int64_t n_items,
                                      const float* S, int64_t lds, const int64_t* query_users, int64_t n_query,
                                      const int64_t* pair_ptr, const int64_t* pair_items, float* out_pick, int32_t topk,
                                      const int64_t* seen_ptr, const int64_t* seen_idx, int64_t* out_items,
                                      float* out_scores, int32_t lds_cap, void* workspace, size_t workspace_bytes,
                                      hiprec_stats* stats, void* stream) {
  const int32_t op = HIPREC_KNN_OP_ITEM_SCORES;
  HIPREC_REQUIRE(knn_sizes_ok(op, n_users, n_items, n_query, lds_cap),
                 "knn_item_scores: bad sizes (n_users=%lld n_items=%lld n_query=%lld lds_cap=%d)", (long long)n_users,
                 (long long)n_items, (long long)n_query, lds_cap);
  HIPREC_REQUIRE(lds >= n_items, "knn_item_scores: leading dimension %lld < n_items=%lld", (long long)lds,
                 (long long)n_items);
  if (int rc = knn_check_out("knn_item_scores", n_query, pair_ptr, pair_items, out_pick, topk, seen_ptr, seen_idx,
                             out_items, out_scores, stats))
    return rc;
  if (n_query == 0) return 0;
  HIPREC_REQUIRE(b_ptr && b_idx && S && query_users, "knn_item_scores: NULL pointer");
  const size_t need = hiprec_knn_workspace_bytes(op, n_users, n_items, n_query, lds_cap);
  HIPREC_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need),
                 "knn_item_scores: workspace %zu B < %zu B", workspace_bytes, need);
  KnnItemArgs a{};
  a.b_ptr = b_ptr, a.b_idx = b_idx, a.S = S, a.query = query_users, a.ws = workspace;
  a.out = KnnOut{pair_ptr, pair_items, out_pick, seen_ptr, seen_idx, out_items, out_scores, stats, topk};
  a.n_users = n_users, a.n_items = n_items, a.lds = lds, a.n_query = n_query;
  auto s = static_cast<hipStream_t>(stream);
  const unsigned grid = static_cast<unsigned>(knn_blocks(op, n_items, n_query));
  if (need == 0) knn_item_scores_kernel<false><<<grid, kBlock, sizeof(float) * static_cast<size_t>(n_items), s>>>(a);
  else knn_item_scores_kernel<true><<<grid, kBlock, 0, s>>>(a);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_knn_user_scores(const int64_t* b_ptr, const int64_t* b_idx, const float* b_val,
                                      const int64_t* bt_ptr, const int64_t* bt_idx, const float* bt_val,
                                      const double* cu, int64_t n_users, int64_t n_items, int32_t k,
                                      const int64_t* query_users, int64_t n_query, int64_t* out_nb_ids,
                                      double* out_nb_sims, const int64_t* pair_ptr, const int64_t* pair_items,
                                      double* out_pick, int32_t topk, const int64_t* seen_ptr, const int64_t* seen_idx,
                                      int64_t* out_items, float* out_scores, int32_t lds_cap, void* workspace,
                                      size_t workspace_bytes, hiprec_stats* stats, void* stream) {
  const int32_t op = HIPREC_KNN_OP_USER_SCORES;
  HIPREC_REQUIRE(k >= 1 && k <= HIPREC_KNN_MAX_K, "knn_user_scores: k=%d outside 1..%d", k, HIPREC_KNN_MAX_K);
  HIPREC_REQUIRE(knn_sizes_ok(op, n_users, n_items, n_query, lds_cap),
                 "knn_user_scores: bad sizes (n_users=%lld n_items=%lld n_query=%lld lds_cap=%d)", (long long)n_users,
                 (long long)n_items, (long long)n_query, lds_cap);
  HIPREC_REQUIRE(k <= n_users, "knn_user_scores: k=%d neighbours of n_users=%lld", k, (long long)n_users);
  if (int rc = knn_check_out("knn_user_scores", n_query, pair_ptr, pair_items, out_pick, topk, seen_ptr, seen_idx,
                             out_items, out_scores, stats))
    return rc;
  HIPREC_REQUIRE((out_nb_ids == nullptr) == (out_nb_sims == nullptr),
                 "knn_user_scores: the neighbour lists need both out_nb_ids and out_nb_sims (or neither)");
  if (n_query == 0) return 0;
  HIPREC_REQUIRE(b_ptr && b_idx && b_val && bt_ptr && bt_idx && bt_val && cu && query_users,
                 "knn_user_scores: NULL pointer");
  const size_t need = hiprec_knn_workspace_bytes(op, n_users, n_items, n_query, lds_cap);
  HIPREC_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need),
                 "knn_user_scores: workspace %zu B < %zu B", workspace_bytes, need);
  KnnUserArgs a{};
  a.b_ptr = b_ptr, a.b_idx = b_idx, a.b_val = b_val, a.bt_ptr = bt_ptr, a.bt_idx = bt_idx, a.bt_val = bt_val;
  a.cu = cu, a.query = query_users, a.out_nb_ids = out_nb_ids, a.out_nb_sims = out_nb_sims, a.ws = workspace;
  a.out = KnnOut{pair_ptr, pair_items, out_pick, seen_ptr, seen_idx, out_items, out_scores, stats, topk};
  a.n_users = n_users, a.n_items = n_items, a.n_acc = knn_acc_entries(op, n_users, n_items), a.n_query = n_query;
  a.slice_bytes = static_cast<int64_t>(knn_slice_bytes(op, n_users, n_items));
  a.k = k;
  auto s = static_cast<hipStream_t>(stream);
  const unsigned grid = static_cast<unsigned>(knn_blocks(op, n_items, n_query));
  if (need == 0) {
    knn_user_kernel<false><<<grid, kBlock, sizeof(uint64_t) * static_cast<size_t>(a.n_acc), s>>>(a);
  } else {
    HIPREC_TRY(hipMemsetAsync(workspace, 0, need, s));
    knn_user_kernel<true><<<grid, kBlock, 0, s>>>(a);
  }
  HIPREC_TRY(hipGetLastError());
  return 0;
}
