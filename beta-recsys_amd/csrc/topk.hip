// Top-K recommendation over the whole catalogue: score a tile of query users against every item, mask the items the
// user has already interacted with, keep a running top-K per user on the CU.  No score ever reaches HBM.
//
//   score(u, i) = alpha * dot(U[u, 0:D], I[i, 0:D]) + item_bias[i]                                      (fp32)
//
// topk_score_kernel: a block of 4 waves owns 64 query users (16 per wave) and one of `splits` contiguous item ranges.
// Every wave walks the range in tiles of 64 items: four 16 x 16 score tiles on the fp32 MFMA (v_mfma_f32_16x16x4_f32:
// items are the A rows, users the B columns, so a lane ends up with 16 scores of ONE user, lane & 15).  The user rows
// stay in registers for the whole range; the item rows come straight from L2 into registers with the k permutation of
// ncf.hip's FusedGemm (lane group kq = lane >> 4 feeds k = 32 c + 8 kq + j to MFMA j of chunk c: two 16-byte loads of
// the lane's own row per chunk).  The MFMA is bitwise an fmaf chain in that k order, so the bits of a score depend on
// the two rows and D only -- not on the tile, the split or the block that formed it.
//
// Running list: K sorted 64-bit keys per user in LDS (smaller key = better candidate: score bits made orderable and
// inverted in the high word, item id in the low word -- eval.hip's rank_key, so ties go to the lower id and -0 == +0).
// A lane keeps its user's current K-th key in a register; a candidate that does not beat it is dropped by one 64-bit
// compare and never touches the list.  After the first tiles almost every candidate ends there (the expected number
// that get through is K (1 + ln(N / K)) per user and range).  The rest are inserted one at a time by the whole wave:
// every lane holds two entries, a ballot counts the entries in front of the candidate, the tail moves down by one.
//
// Seen items: the user's CSR row is ascending, and so are the tiles, so each user keeps a cursor into its row (one
// binary search per user and range finds where to start).  The four lanes of a user hold the next eight seen ids; the
// ones that fall into the tile become a 64-bit tile mask and the cursor moves on -- no search per (user, item) pair.
//
// topk_merge_kernel: one wave per query user merges the `splits` partial lists (sorted, so a list is left at the first
// key that does not beat the merged K-th) with the same insertion and writes ids and scores.
#include "common.hpp"

namespace hiprec {
namespace {

using tk_f32x4 = float __attribute__((ext_vector_type(4)));

constexpr int kTkUsers = 64;                 // query users per block: 16 per wave
constexpr int kTkTile = 64;                  // items per wave iteration: 4 MFMA tiles of 16
constexpr int kTkSub = kTkTile / 16;
constexpr uint64_t kTkNone = ~0ull;          // empty list slot: worse than every candidate
constexpr int kTkTargetBlocks = 1024;        // library-chosen splits: about 4 blocks per CU ...
constexpr int kTkMinTilesPerSplit = 4;       // ... of at least 256 items each (every range warms its lists up again)

__device__ __forceinline__ uint64_t topk_key(float score, uint32_t item) {
  if (score == 0.0f) score = 0.0f;  // -0 ties with +0
  uint32_t u = __float_as_uint(score);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending-orderable
  return (static_cast<uint64_t>(~u) << 32) | item;  // smaller key == better candidate
}

__device__ __forceinline__ float topk_key_score(uint64_t key) {
  const uint32_t u = ~static_cast<uint32_t>(key >> 32);
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

// row[k .. k+8), zeros beyond dim (and for a row that does not exist); `vec`: 16-byte loads are aligned
__device__ __forceinline__ void load8(const float* row, int k, int dim, bool vec, float (&out)[8]) {
  if (row != nullptr && vec && k + 8 <= dim) {
    const float4 x = *reinterpret_cast<const float4*>(row + k);
    const float4 y = *reinterpret_cast<const float4*>(row + k + 4);
    out[0] = x.x, out[1] = x.y, out[2] = x.z, out[3] = x.w;
    out[4] = y.x, out[5] = y.y, out[6] = y.z, out[7] = y.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = (row != nullptr && k + j < dim) ? row[k + j] : 0.f;
  }
}

// The same for a row that exists and a chunk that lies inside dim, 16-byte aligned: no branch, so the loads of a tile
// are issued back to back (behind load8's per-lane branches every load waits for the one before it)
__device__ __forceinline__ void load8_full(const float* row, int k, float (&out)[8]) {
  const float4 x = *reinterpret_cast<const float4*>(row + k);
  const float4 y = *reinterpret_cast<const float4*>(row + k + 4);
  out[0] = x.x, out[1] = x.y, out[2] = x.z, out[3] = x.w;
  out[4] = y.x, out[5] = y.y, out[6] = y.z, out[7] = y.w;
}

// The whole wave inserts key c (wave-uniform) into the ascending list l[0..k): lane holds entries lane and lane + 64.
// The list belongs to this wave alone and a wave's LDS operations complete in order: no barrier.
// Returns false when c does not beat the list's last entry (nothing is written then).
__device__ __forceinline__ bool wave_insert(volatile uint64_t* l, int k, uint64_t c, int lane) {
  const uint64_t e0 = lane < k ? l[lane] : kTkNone;
  const uint64_t e1 = lane + 64 < k ? l[lane + 64] : kTkNone;
  const int pos = __popcll(__ballot(e0 < c)) + __popcll(__ballot(e1 < c));  // entries in front of c
  if (pos >= k) return false;
  if (lane >= pos && lane + 1 < k) l[lane + 1] = e0;
  if (lane + 64 >= pos && lane + 65 < k) l[lane + 65] = e1;
  if (lane == 0) l[pos] = c;
  return true;
}

// v of lane src (wave-uniform) through the scalar unit: no LDS round trip
__device__ __forceinline__ uint64_t read_lane_u64(uint64_t v, int src) {
  const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(v)), src));
  const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(v >> 32)), src));
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

struct TopkArgs {
  const float* U;
  const float* I;
  const float* bias;
  const int64_t* query;
  const int64_t* user_ptr;
  const int64_t* pos;
  uint64_t* partial;       // [n_query][splits][k]
  hiprec_stats* stats;
  int64_t ldu, ldi, n_users, n_items, n_query, n_tiles, tiles_per_split;
  float alpha;
  int32_t dim, k, splits, vec_u, vec_i;
};

// NCH 32-wide k chunks: dim <= 32 * NCH.  FULL: dim == 32 * NCH and both tables take 16-byte loads; a row that does not
// exist (tile tail, out-of-range user) is then read from a row that does and its scores are dropped below.
template <int NCH, bool FULL>
__global__ __launch_bounds__(kBlock) void topk_score_kernel(const TopkArgs a) {
  extern __shared__ uint64_t tk_lists[];  // [64 users][k]
  const int lane = lane_id(), wv = wave_in_block();
  const int u16 = lane & 15, g = lane >> 4;
  const int k = a.k;
  volatile uint64_t* wave_lists = tk_lists + static_cast<size_t>(wv) * 16 * k;
  for (int e = lane; e < 16 * k; e += kWave) wave_lists[e] = kTkNone;
  volatile uint64_t* my_list = wave_lists + u16 * k;

  const int64_t q = static_cast<int64_t>(blockIdx.x) * kTkUsers + wv * 16 + u16;
  const int64_t user = q < a.n_query ? a.query[q] : -1;
  const bool valid = q < a.n_query && user >= 0 && user < a.n_users;
  if (q < a.n_query && !valid && g == 0 && blockIdx.y == 0) atomicOr(&a.stats->status, HIPREC_STATUS_USER_OOB);

  float ub[NCH][8];
  {
    const float* urow = valid ? a.U + user * a.ldu : (FULL ? a.U : nullptr);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if constexpr (FULL) load8_full(urow, 32 * c + 8 * g, ub[c]);
      else load8(urow, 32 * c + 8 * g, a.dim, a.vec_u != 0, ub[c]);
    }
  }

  const int64_t tile_lo = static_cast<int64_t>(blockIdx.y) * a.tiles_per_split;
  const int64_t tile_end = tile_lo + a.tiles_per_split < a.n_tiles ? tile_lo + a.tiles_per_split : a.n_tiles;

  // cursor into the user's seen row: first entry >= the range's first item
  const bool masked = a.user_ptr != nullptr;
  int64_t cur = 0, row_end = 0;
  if (masked && valid) {
    int64_t lo = a.user_ptr[user];
    row_end = a.user_ptr[user + 1];
    int64_t hi = row_end;
    const int64_t first = tile_lo * kTkTile;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (a.pos[mid] < first) lo = mid + 1; else hi = mid;
    }
    cur = lo;
  }
  constexpr int64_t kNoSeen = INT64_MAX;
  // the user's next eight seen ids, two per lane of the user
  int64_t w0 = (masked && cur + g < row_end) ? a.pos[cur + g] : kNoSeen;
  int64_t w1 = (masked && cur + 4 + g < row_end) ? a.pos[cur + 4 + g] : kNoSeen;

  uint64_t thr = kTkNone;
  for (int64_t tile = tile_lo; tile < tile_end; ++tile) {
    const int64_t base = tile * kTkTile;

    uint64_t seen = 0;  // bit b: item base + b is in the user's row
    if (masked) {
      for (;;) {
        const bool in0 = w0 < base + kTkTile, in1 = w1 < base + kTkTile;
        uint64_t m = (in0 ? 1ull << ((w0 - base) & 63) : 0ull) | (in1 ? 1ull << ((w1 - base) & 63) : 0ull);
        int cnt = (in0 ? 1 : 0) + (in1 ? 1 : 0);
        m |= __shfl_xor(static_cast<unsigned long long>(m), 16, kWave);
        cnt += __shfl_xor(cnt, 16, kWave);
        m |= __shfl_xor(static_cast<unsigned long long>(m), 32, kWave);
        cnt += __shfl_xor(cnt, 32, kWave);
        seen |= m;
        if (cnt > 0) {
          cur += cnt;  // (the row is ascending: the ids inside the tile are the first cnt of the eight)
          w0 = cur + g < row_end ? a.pos[cur + g] : kNoSeen;
          w1 = cur + 4 + g < row_end ? a.pos[cur + 4 + g] : kNoSeen;
        }
        if (!__any(cnt == 8)) break;  // a user whose eight were all in the tile may have more there
      }
    }

    tk_f32x4 acc[kTkSub];
#pragma unroll
    for (int t = 0; t < kTkSub; ++t) acc[t] = tk_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      float ia[kTkSub][8];
#pragma unroll
      for (int t = 0; t < kTkSub; ++t) {
        const int64_t item = base + 16 * t + u16;
        if constexpr (FULL)
          load8_full(a.I + (item < a.n_items ? item : a.n_items - 1) * a.ldi, 32 * c + 8 * g, ia[t]);
        else
          load8(item < a.n_items ? a.I + item * a.ldi : nullptr, 32 * c + 8 * g, a.dim, a.vec_i != 0, ia[t]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int t = 0; t < kTkSub; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ia[t][j], ub[c][j], acc[t], 0, 0, 0);
    }

    // acc[t][r]: user u16 (this lane's), item base + 16 t + 4 g + r
    uint64_t key[kTkSub][4];
    uint32_t pass = 0;
#pragma unroll
    for (int t = 0; t < kTkSub; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int b = 16 * t + 4 * g + r;
        const int64_t item = base + b;
        const bool exists = item < a.n_items;
        float s;
        {
#pragma clang fp contract(off)
          s = a.alpha * acc[t][r];
          if (a.bias != nullptr) s = s + (exists ? a.bias[item] : 0.f);
        }
        key[t][r] = topk_key(s, static_cast<uint32_t>(item));
        if (valid && exists && !((seen >> b) & 1ull) && key[t][r] < thr) pass |= 1u << (4 * t + r);
      }
    }
    if (__any(pass != 0)) {
#pragma unroll
      for (int t = 0; t < kTkSub; ++t) {
        if (t > 0) thr = my_list[k - 1];  // what the tile has put in so far already shuts most of the rest out
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          unsigned long long todo = __ballot(((pass >> (4 * t + r)) & 1u) && key[t][r] < thr);
          while (todo) {
            const int src = __ffsll(todo) - 1;
            todo &= todo - 1;
            const uint64_t c = read_lane_u64(key[t][r], src);
            wave_insert(wave_lists + (src & 15) * k, k, c, lane);
          }
        }
      }
      thr = my_list[k - 1];
    }
  }

  for (int e = lane; e < 16 * k; e += kWave) {
    const int64_t qq = static_cast<int64_t>(blockIdx.x) * kTkUsers + wv * 16 + e / k;
    if (qq < a.n_query) a.partial[(qq * a.splits + blockIdx.y) * k + e % k] = wave_lists[e];
  }
}

__global__ __launch_bounds__(kBlock) void topk_merge_kernel(const uint64_t* __restrict__ partial, int64_t n_query,
                                                            int splits, int k, int64_t* __restrict__ out_items,
                                                            float* __restrict__ out_scores) {
  extern __shared__ uint64_t tk_lists[];  // [4 waves][k]
  const int lane = lane_id(), wv = wave_in_block();
  const int64_t q = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wv;
  if (q >= n_query) return;  // (no block-wide barrier below)
  volatile uint64_t* l = tk_lists + wv * k;
  if (lane < k) l[lane] = kTkNone;
  if (lane + 64 < k) l[lane + 64] = kTkNone;
  for (int s = 0; s < splits; ++s) {
    const uint64_t* src = partial + (q * splits + s) * k;
    const uint64_t p0 = lane < k ? src[lane] : kTkNone;
    const uint64_t p1 = lane + 64 < k ? src[lane + 64] : kTkNone;
    for (int e = 0; e < k; ++e) {
      const uint64_t c = read_lane_u64(e < 64 ? p0 : p1, e & 63);
      if (!wave_insert(l, k, c, lane)) break;  // the partial list is ascending: nothing behind c gets in either
    }
  }
  for (int e = lane; e < k; e += kWave) {
    const uint64_t key = l[e];
    const bool none = key == kTkNone;
    out_items[q * k + e] = none ? -1 : static_cast<int64_t>(key & 0xffffffffull);
    out_scores[q * k + e] = none ? -INFINITY : topk_key_score(key);
  }
}

int choose_splits(int64_t n_query, int64_t n_items, int requested) {
  const int64_t n_tiles = (n_items + kTkTile - 1) / kTkTile;
  const int64_t user_blocks = (n_query + kTkUsers - 1) / kTkUsers;
  int64_t s = requested;
  if (s <= 0) {
    s = (kTkTargetBlocks + user_blocks - 1) / (user_blocks > 0 ? user_blocks : 1);
    const int64_t cap = n_tiles / kTkMinTilesPerSplit;
    if (s > cap) s = cap;
  }
  if (s > n_tiles) s = n_tiles;
  if (s > HIPREC_TOPK_MAX_SPLITS) s = HIPREC_TOPK_MAX_SPLITS;
  if (s < 1) s = 1;
  const int64_t per = (n_tiles + s - 1) / s;
  return static_cast<int>((n_tiles + per - 1) / per);  // no empty range
}

bool topk_sizes_ok(int64_t n_query, int64_t n_items, int32_t k, int32_t item_splits) {
  return n_query >= 0 && n_items >= 1 && n_items < 0xffffffffll && k >= 1 && k <= HIPREC_TOPK_MAX_K && item_splits >= 0;
}

// ---- metrics of the lists against a truth CSR: eval.hip's definitions with "hit" = membership in the truth row ----
struct TkKList {
  int32_t n;
  int32_t k[HIPREC_RANK_MAX_K];
};

// per_user row layout: [is_common, then for each cut-off: precision, recall, ndcg, map]   (one thread per user)
__global__ __launch_bounds__(kBlock) void topk_metrics_kernel(const int64_t* __restrict__ items, int64_t n_query, int k,
                                                              const int64_t* __restrict__ truth_ptr,
                                                              const int64_t* __restrict__ truth, TkKList kl,
                                                              double* __restrict__ per_user) {
  const int stride = 1 + 4 * kl.n;
  int k_max = 0;
  for (int j = 0; j < kl.n; ++j)
    if (kl.k[j] > k_max) k_max = kl.k[j];
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; q < n_query;
       q += static_cast<int64_t>(gridDim.x) * kBlock) {
    double* row = per_user + q * stride;
    const int64_t t0 = truth_ptr[q], t1 = truth_ptr[q + 1];
    const int64_t actual = t1 - t0;
    if (actual <= 0) {  // not a common user: contributes to nothing
      for (int c = 0; c < stride; ++c) row[c] = 0.0;
      continue;
    }
    int hits[HIPREC_RANK_MAX_K];
    double dcg[HIPREC_RANK_MAX_K], ap[HIPREC_RANK_MAX_K];
#pragma unroll
    for (int j = 0; j < HIPREC_RANK_MAX_K; ++j) {
      hits[j] = 0;
      dcg[j] = 0.0;
      ap[j] = 0.0;
    }
    for (int r = 1; r <= k_max; ++r) {
      const int64_t item = items[q * k + r - 1];
      if (item < 0) break;  // padding: the list is over
      int64_t lo = t0, hi = t1;
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (truth[mid] < item) lo = mid + 1; else hi = mid;
      }
      if (lo < t1 && truth[lo] == item) {
        const double gain = 1.0 / log1p(static_cast<double>(r));
#pragma unroll
        for (int j = 0; j < HIPREC_RANK_MAX_K; ++j) {
          if (j < kl.n && r <= kl.k[j]) {
            hits[j] += 1;
            dcg[j] += gain;
            ap[j] += static_cast<double>(hits[j]) / static_cast<double>(r);
          }
        }
      }
    }
    row[0] = 1.0;
#pragma unroll
    for (int j = 0; j < HIPREC_RANK_MAX_K; ++j) {
      if (j >= kl.n) continue;
      const int kk = kl.k[j];
      const int64_t ideal = actual < kk ? actual : kk;
      double idcg = 0.0;
      for (int64_t t = 1; t <= ideal; ++t) idcg += 1.0 / log1p(static_cast<double>(t));
      double* m = row + 1 + 4 * j;
      m[0] = static_cast<double>(hits[j]) / static_cast<double>(kk);
      m[1] = static_cast<double>(hits[j]) / static_cast<double>(actual);
      m[2] = dcg[j] / idcg;
      m[3] = ap[j] / static_cast<double>(actual);
    }
  }
}

// One block per column, fixed summation order (eval.hip's rank_reduce_kernel restated).
__global__ __launch_bounds__(kBlock) void topk_metrics_reduce_kernel(const double* __restrict__ per_user, int64_t n,
                                                                     int stride, double* __restrict__ out) {
  __shared__ double part[kBlock];
  const int col = blockIdx.x;
  double acc = 0.0, cnt = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) {
    acc += per_user[i * stride + col];
    cnt += per_user[i * stride];
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int off = kBlock / 2; off > 0; off >>= 1) {
    if (static_cast<int>(threadIdx.x) < off) part[threadIdx.x] += part[threadIdx.x + off];
    __syncthreads();
  }
  const double total = part[0];
  __syncthreads();
  part[threadIdx.x] = cnt;
  __syncthreads();
  for (int off = kBlock / 2; off > 0; off >>= 1) {
    if (static_cast<int>(threadIdx.x) < off) part[threadIdx.x] += part[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double n_common = part[0];
    out[col] = col == 0 ? n_common : (n_common > 0.0 ? total / n_common : 0.0);
  }
}

template <int NCH>
int launch_score(const TopkArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  if (a.dim == 32 * NCH && a.vec_u && a.vec_i) topk_score_kernel<NCH, true><<<grid, kBlock, lds, s>>>(a);
  else topk_score_kernel<NCH, false><<<grid, kBlock, lds, s>>>(a);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_topk_workspace_bytes(int64_t n_query, int64_t n_items, int32_t k, int32_t item_splits) {
  if (!topk_sizes_ok(n_query, n_items, k, item_splits)) return 0;
  return sizeof(uint64_t) * static_cast<size_t>(n_query) * choose_splits(n_query, n_items, item_splits) * k;
}

extern "C" int hiprec_topk_recommend(const float* user_factors, int64_t ldu, int64_t n_users,
                                     const float* item_factors, int64_t ldi, int64_t n_items, int32_t dim, float alpha,
                                     const float* item_bias, const int64_t* query_users, int64_t n_query,
                                     const int64_t* user_ptr, const int64_t* pos_sorted, int32_t k, int32_t item_splits,
                                     void* workspace, size_t workspace_bytes, int64_t* out_items, float* out_scores,
                                     hiprec_stats* stats, void* stream) {
  HIPREC_REQUIRE(k >= 1 && k <= HIPREC_TOPK_MAX_K, "topk_recommend: k=%d outside 1..%d", k, HIPREC_TOPK_MAX_K);
  HIPREC_REQUIRE(dim >= 1 && dim <= HIPREC_TOPK_MAX_DIM, "topk_recommend: dim=%d outside 1..%d", dim,
                 HIPREC_TOPK_MAX_DIM);
  HIPREC_REQUIRE(n_users >= 1 && topk_sizes_ok(n_query, n_items, k, item_splits),
                 "topk_recommend: bad sizes (n_users=%lld n_items=%lld n_query=%lld item_splits=%d)", (long long)n_users,
                 (long long)n_items, (long long)n_query, item_splits);
  HIPREC_REQUIRE(ldu >= dim && ldi >= dim, "topk_recommend: leading dimensions (%lld, %lld) < dim=%d", (long long)ldu,
                 (long long)ldi, dim);
  if (n_query == 0) return 0;
  HIPREC_REQUIRE(user_factors && item_factors && query_users && out_items && out_scores && stats && workspace,
                 "topk_recommend: NULL pointer");
  HIPREC_REQUIRE((user_ptr == nullptr) == (pos_sorted == nullptr),
                 "topk_recommend: the seen-item CSR needs both user_ptr and pos_sorted (or neither)");
  const size_t need = hiprec_topk_workspace_bytes(n_query, n_items, k, item_splits);
  HIPREC_REQUIRE(workspace_bytes >= need, "topk_recommend: workspace %zu B < %zu B", workspace_bytes, need);

  TopkArgs a{};
  a.U = user_factors, a.I = item_factors, a.bias = item_bias, a.query = query_users;
  a.user_ptr = user_ptr, a.pos = pos_sorted, a.partial = static_cast<uint64_t*>(workspace), a.stats = stats;
  a.ldu = ldu, a.ldi = ldi, a.n_users = n_users, a.n_items = n_items, a.n_query = n_query;
  a.n_tiles = (n_items + kTkTile - 1) / kTkTile;
  a.splits = choose_splits(n_query, n_items, item_splits);
  a.tiles_per_split = (a.n_tiles + a.splits - 1) / a.splits;
  a.alpha = alpha, a.dim = dim, a.k = k;
  a.vec_u = (reinterpret_cast<uintptr_t>(user_factors) % 16 == 0 && ldu % 4 == 0) ? 1 : 0;
  a.vec_i = (reinterpret_cast<uintptr_t>(item_factors) % 16 == 0 && ldi % 4 == 0) ? 1 : 0;

  auto s = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>((n_query + kTkUsers - 1) / kTkUsers), static_cast<unsigned>(a.splits));
  const size_t lds = sizeof(uint64_t) * kTkUsers * k;  // <= 64 KB
  int rc;
  if (dim <= 32) rc = launch_score<1>(a, grid, lds, s);
  else if (dim <= 64) rc = launch_score<2>(a, grid, lds, s);
  else if (dim <= 128) rc = launch_score<4>(a, grid, lds, s);
  else if (dim <= 256) rc = launch_score<8>(a, grid, lds, s);
  else rc = launch_score<16>(a, grid, lds, s);
  if (rc != 0) return rc;
  topk_merge_kernel<<<static_cast<unsigned>((n_query + kWavesPerBlock - 1) / kWavesPerBlock), kBlock,
                      sizeof(uint64_t) * kWavesPerBlock * k, s>>>(a.partial, n_query, a.splits, k, out_items,
                                                                  out_scores);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_topk_metrics(const int64_t* items, int64_t n_query, int32_t k, const int64_t* truth_ptr,
                                   const int64_t* truth_sorted, const int32_t* k_list_host, int32_t n_k,
                                   double* workspace, size_t workspace_bytes, double* out, void* stream) {
  HIPREC_REQUIRE(n_k >= 1 && n_k <= HIPREC_RANK_MAX_K, "topk_metrics: n_k=%d outside 1..%d", n_k, HIPREC_RANK_MAX_K);
  HIPREC_REQUIRE(k_list_host != nullptr && out != nullptr, "topk_metrics: null k_list/out");
  HIPREC_REQUIRE(n_query >= 0 && k >= 1, "topk_metrics: n_query=%lld k=%d", (long long)n_query, k);
  TkKList kl{};
  kl.n = n_k;
  for (int j = 0; j < n_k; ++j) {
    HIPREC_REQUIRE(k_list_host[j] >= 1 && k_list_host[j] <= k, "topk_metrics: k[%d]=%d outside 1..%d", j,
                   k_list_host[j], k);
    kl.k[j] = k_list_host[j];
  }
  const int stride = 1 + 4 * n_k;
  auto s = static_cast<hipStream_t>(stream);
  if (n_query == 0) {
    HIPREC_TRY(hipMemsetAsync(out, 0, sizeof(double) * stride, s));
    return 0;
  }
  HIPREC_REQUIRE(items && truth_ptr && workspace, "topk_metrics: null pointer");
  const size_t need = sizeof(double) * static_cast<size_t>(n_query) * stride;
  HIPREC_REQUIRE(workspace_bytes >= need, "topk_metrics: workspace %zu B < %zu B", workspace_bytes, need);
  topk_metrics_kernel<<<grid_for_threads(n_query), kBlock, 0, s>>>(items, n_query, k, truth_ptr, truth_sorted, kl,
                                                                   workspace);
  HIPREC_TRY(hipGetLastError());
  topk_metrics_reduce_kernel<<<stride, kBlock, 0, s>>>(workspace, n_query, stride, out);
  HIPREC_TRY(hipGetLastError());
  return 0;
}
