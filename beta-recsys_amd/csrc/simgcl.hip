// SimGCL training step for gfx950.
//
// Replaces beta_rec/models/simgcl.py:25-47 (SimGCL.forward: L hops of norm_adj, each perturbed by sign(Y) * normalize(u) *
// eps when asked to, mean-pooled over hops 1 .. L), :49-70 (cal_cl_loss: InfoNCE among the batch's UNIQUE users and
// unique positive items at temperature 0.2), :101-133 and :153-163 (train_single_batch: BPR sum of -log(1e-7 +
// sigmoid(pos - neg)) + reg * the unsquared Frobenius norms of the three batch matrices + lambda * cl), autograd's
// backward through all of it, and :72-82 (predict on the raw tables).
//
// sign() has zero derivative, so a view's noise is an additive constant and the clean view, view 1 and view 2 share the
// map E_0 -> pool = (1 / L) sum_k A^k E_0 + const.  Their three gradients are accumulated into ONE [n, D] table G (the
// gradient with respect to the hop SUM: every scatter into it carries the 1 / L) and ONE backward chain runs: h = G;
// (L - 1) x: h = G + A^T h; dE_0 = A^T h -- L SpMMs where the reference runs 3 L.  The forward computes hop 1's A E_0 once for all three
// views: 1 + 3 (L - 1) SpMMs (three calls per later hop: launch_spmm is built for widths up to 256, so the views are
// not stacked into one 3 D wide pass).
//
// The noise is drawn in registers by the wave that owns the row (sim_uniform: a counter-based draw keyed by seed, step,
// view, hop, row, column) and never stored; the backward does not need it.  Tests pass the uniforms in instead: the same
// kernel, another template argument, the same arithmetic after u.
//
// The unique ids are found on the device: the batch's users and positive items stamp a table with the workspace's step
// clock (nothing is ever cleared), one block per side compacts the stamped ids by an ordered scan -- ascending, which is
// torch.unique's order -- and leaves the two counts in device memory.  Every later launch is sized by the batch bound
// and reads the count; there is no host sync before the loss is read back.
//
// InfoNCE runs among the unique rows only, on v_mfma_f32_16x16x4_f32 with the tiling of csrc/sgl.hip: the [n_uniq,
// n_uniq] scores exist as 16 x 16 tiles in registers, the forward keeps log sum_j exp((s_ij - 1) / temp) per row
// (cosines are <= 1, so the shift is exact), the backward recomputes the probabilities from it, once with a query tile
// resident (dQ) and once with a key tile resident (dK, the positive's one-hot subtracted before the product).  Each
// unique row has one owner, so the way back through the normalisation adds into G with plain stores.
#include <algorithm>

#include "common.hpp"
#include "seqrec.hpp"
#include "spmm.hpp"

namespace hiprec {

constexpr int kSimTB = HIPREC_SIMGCL_TILE_B;   // query rows per tile (2 MFMA row blocks)
constexpr int kSimTN = HIPREC_SIMGCL_TILE_N;   // key rows per tile (one 16-column block per wave)
constexpr int kSimPS = kSimTN + 4;             // row stride of the probability tile
static_assert(kSimTB == 32 && kSimTN == 16 * kWavesPerBlock, "tile geometry is wired into the kernels");
static_assert(HIPREC_SIMGCL_MAX_DIM == 4 * kWave, "a wave holds a row in four registers per lane");

__host__ __device__ inline int sim_dp(int dim) { return (dim + 15) & ~15; }
static size_t sim_lds_bytes(int dim, bool with_p) {
  return sizeof(float) * (static_cast<size_t>(kSimTB + kSimTN) * (sim_dp(dim) + 4) + (with_p ? kSimTB * kSimPS : 0));
}

// one side of the contrastive term: its unique ids, their count, and the compact buffers over them
struct SimSide {
  const int64_t* uniq;    // [batch] ascending ids, the first *count are valid
  const int32_t* count;
  int64_t off;            // first node row of the side
  const float* pool_q;    // sum of the perturbed hops of the query view, [n, D]
  const float* pool_k;    // ... of the key view (== pool_q when a view is contrasted with itself)
  float *Q, *K;           // [batch, D] normalised rows (K == Q when pool_k == pool_q)
  float *inv_q, *inv_k;   // [batch] 1 / max(|row|, 1e-12)
  float *dq, *dk;         // [batch, D]
  float *logsum, *row_loss;   // [batch]
};
struct SimSides {
  SimSide s[2];
};

// ---- the draw ----------------------------------------------------------------------------------------------------
// uniform of element e = row * D + col at (seed, step, view, hop): 24-bit fraction in [0, 1), in the style of keep_draw;
// restated bit for bit in tests/simgcl_numpy.py
__device__ __forceinline__ float sim_uniform(uint64_t seed, uint64_t step, int view, int hop, int64_t e) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (static_cast<uint64_t>(e) + 1) + 0xD1B54A32D192ED03ull * (step + 1) +
               0x8CB92BA72F3D8DD7ull * static_cast<uint64_t>(view * HIPREC_SIMGCL_MAX_LAYERS + hop + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return static_cast<float>(z >> 40) * (1.0f / 16777216.0f);
}

__global__ __launch_bounds__(kBlock) void sim_noise_kernel(uint64_t seed, uint64_t step, int L, int64_t n, int D,
                                                           float* __restrict__ out) {
  const int64_t per = n * D, total = 2 * L * per;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < total; i += stride) {
    const int64_t vh = i / per;
    out[i] = sim_uniform(seed, step, static_cast<int>(vh / L), static_cast<int>(vh % L), i - vh * per);
  }
}

// ---- perturb and pool: one wave per row --------------------------------------------------------------------------
// x[r] = y[r] + sign(y[r]) * u / max(|u|, 1e-12) * eps; pool[r] = x[r] (first) or pool[r] + x[r].  x may be y.
// DRAW: u from sim_uniform at the workspace's step clock; otherwise from noise[view][hop][r].
template <bool DRAW>
__global__ __launch_bounds__(kBlock) void sim_perturb_kernel(const float* y, float* x, float* __restrict__ pool,
                                                             bool first, int view, int hop, int L, int64_t n, int D,
                                                             float eps, const float* __restrict__ noise, uint64_t seed,
                                                             const int32_t* __restrict__ clock) {
  const int lane = lane_id();
  const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  const uint64_t step = DRAW ? static_cast<uint64_t>(static_cast<uint32_t>(clock[0])) : 0;
  const float* nz = DRAW ? nullptr : noise + (static_cast<int64_t>(view) * L + hop) * n * D;
  for (int64_t r = wave0; r < n; r += n_waves) {
    float yv[4], u[4], ss = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane + kWave * k;
      const bool ok = c < D;
      yv[k] = ok ? y[r * D + c] : 0.f;
      if constexpr (DRAW)
        u[k] = ok ? sim_uniform(seed, step, view, hop, r * D + c) : 0.f;
      else
        u[k] = ok ? nz[r * D + c] : 0.f;
      ss += u[k] * u[k];
    }
    const float nrm = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane + kWave * k;
      if (c < D) {
        const float sg = yv[k] > 0.f ? 1.f : (yv[k] < 0.f ? -1.f : 0.f);
        const float xv = yv[k] + sg * (u[k] / nrm) * eps;
        x[r * D + c] = xv;
        pool[r * D + c] = first ? xv : pool[r * D + c] + xv;
      }
    }
  }
}

// ---- unique ids --------------------------------------------------------------------------------------------------
// stamps[0] is the step clock; stamps[1 + node] = clock + 1 for every user and positive item of the batch (equal values
// from several threads: plain stores)
__global__ __launch_bounds__(kBlock) void sim_stamp_kernel(const int64_t* __restrict__ users,
                                                           const int64_t* __restrict__ pos, int64_t batch,
                                                           int64_t n_users, int64_t n_items, int32_t* stamps) {
  const int32_t mark = stamps[0] + 1;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; t < batch; t += stride) {
    const int64_t u = users[t], i = pos[t];
    if (static_cast<uint64_t>(u) < static_cast<uint64_t>(n_users)) stamps[1 + u] = mark;
    if (static_cast<uint64_t>(i) < static_cast<uint64_t>(n_items)) stamps[1 + n_users + i] = mark;
  }
}

// block `side` compacts its side's stamped ids in ascending order: every thread counts a contiguous chunk, the counts are
// scanned in LDS, every thread writes its chunk
__global__ __launch_bounds__(kBlock) void sim_compact_kernel(const int32_t* __restrict__ stamps, int64_t n_users,
                                                             int64_t n_items, int64_t batch, int64_t* __restrict__ uniq,
                                                             int32_t* __restrict__ counts) {
  __shared__ int s_scan[kBlock];
  const int side = blockIdx.x;
  const int64_t n = side ? n_items : n_users;
  const int32_t* st = stamps + 1 + (side ? n_users : 0);
  const int32_t mark = stamps[0] + 1;
  const int64_t chunk = (n + kBlock - 1) / kBlock;
  const int64_t lo = chunk * threadIdx.x < n ? chunk * threadIdx.x : n, hi = lo + chunk < n ? lo + chunk : n;
  int cnt = 0;
  for (int64_t i = lo; i < hi; ++i) cnt += st[i] == mark ? 1 : 0;
  s_scan[threadIdx.x] = cnt;
  __syncthreads();
  for (int o = 1; o < kBlock; o <<= 1) {   // inclusive scan
    const int v = static_cast<int>(threadIdx.x) >= o ? s_scan[threadIdx.x - o] : 0;
    __syncthreads();
    s_scan[threadIdx.x] += v;
    __syncthreads();
  }
  int64_t at = s_scan[threadIdx.x] - cnt;
  int64_t* out = uniq + side * batch;
  for (int64_t i = lo; i < hi; ++i)
    if (st[i] == mark) {
      if (at < batch) out[at] = i;   // at most `batch` ids carry this step's stamp
      ++at;
    }
  if (threadIdx.x == kBlock - 1) counts[side] = static_cast<int32_t>(s_scan[kBlock - 1] < batch ? s_scan[kBlock - 1] : batch);
}

// ---- gather + L2 normalise the unique rows: one wave per slot, blockIdx.y = side ---------------------------------
__device__ __forceinline__ void sim_gather_row(const float* __restrict__ pool, int64_t row, int D, float scale,
                                               float* __restrict__ dst, float* __restrict__ inv) {
  const int lane = lane_id();
  float v[4], ss = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane + kWave * k;
    v[k] = c < D ? pool[row * D + c] * scale : 0.f;
    ss += v[k] * v[k];
  }
  const float w = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);   // F.normalize's clamp
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane + kWave * k;
    if (c < D) dst[c] = v[k] * w;
  }
  if (lane == 0) *inv = w;
}

__global__ __launch_bounds__(kBlock) void sim_gather_kernel(SimSides sides, int D, float scale) {
  const SimSide sd = sides.s[blockIdx.y];
  const int64_t count = *sd.count;
  const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t s = wave0; s < count; s += n_waves) {
    const int64_t row = sd.off + sd.uniq[s];
    sim_gather_row(sd.pool_q, row, D, scale, sd.Q + s * D, sd.inv_q + s);
    if (sd.K != sd.Q) sim_gather_row(sd.pool_k, row, D, scale, sd.K + s * D, sd.inv_k + s);
  }
}

// ---- InfoNCE tiles (the tiling of csrc/sgl.hip over compact buffers) ----------------------------------------------
// rows [r0, r0 + rows) of the compact [count, D] buffer into dst[rows][stride], zero beyond count and beyond D up to DP
__device__ __forceinline__ void sim_load_rows(float* dst, int stride, int DP, const float* __restrict__ src, int D,
                                              int rows, int64_t r0, int64_t count) {
  for (int e = threadIdx.x; e < rows * DP; e += kBlock) {
    const int r = e / DP, c = e - r * DP;
    dst[r * stride + c] = (r0 + r < count && c < D) ? src[(r0 + r) * D + c] : 0.f;
  }
}

// S = Q K^T for this wave's 16 key columns and both 16-row blocks of the query tile: s[rb] holds
// (row = rb * 16 + 4 * (lane >> 4) + reg, col = wave * 16 + (lane & 15))
__device__ __forceinline__ void sim_scores(const float* Qs, const float* Ks, int stride, int DP, f32x4 (&s)[2]) {
  const float* kb = Ks + wave_in_block() * 16 * stride;
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) s[rb] = mma16(f32x4{0.f, 0.f, 0.f, 0.f}, Qs + rb * 16 * stride, stride, 1, kb, 1, stride, DP);
}

// logsum[i] = log sum_j exp((s_ij - 1) / temp); row_loss[i] = logsum[i] - (s_ii - 1) / temp.  A block owns kSimTB query
// rows and streams every key tile past them.
__global__ __launch_bounds__(kBlock) void sim_nce_fwd_kernel(SimSides sides, int D, float inv_temp) {
  extern __shared__ float smem[];
  __shared__ float s_red[2][kWavesPerBlock][kSimTB];
  const SimSide sd = sides.s[blockIdx.y];
  const int64_t count = *sd.count;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * kSimTB;
  if (b0 >= count) return;   // the whole block: no barrier has been reached
  const int DP = sim_dp(D), stride = DP + 4;
  float* Qs = smem;
  float* Ks = smem + kSimTB * stride;
  const int lane = lane_id(), w = wave_in_block();
  sim_load_rows(Qs, stride, DP, sd.Q, D, kSimTB, b0, count);
  float rs[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  float ps[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int64_t j0 = 0; j0 < count; j0 += kSimTN) {
    __syncthreads();   // the previous tile's MFMA reads of Ks are done (and Qs is written, first round)
    sim_load_rows(Ks, stride, DP, sd.K, D, kSimTN, j0, count);
    __syncthreads();
    f32x4 s[2];
    sim_scores(Qs, Ks, stride, DP, s);
    const int64_t jcol = j0 + w * 16 + (lane & 15);
    const bool live = jcol < count;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        rs[rb][q] += live ? expf((s[rb][q] - 1.f) * inv_temp) : 0.f;
        ps[rb][q] += (live && jcol == b0 + rb * 16 + 4 * (lane >> 4) + q) ? s[rb][q] : 0.f;
      }
  }
  // the 16 columns of a row sit in the 16 lanes of one DPP row; then the four waves in a fixed order
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = rs[rb][q], p = ps[rb][q];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        v += __shfl_xor(v, o, 64);
        p += __shfl_xor(p, o, 64);
      }
      if ((lane & 15) == 0) {
        s_red[0][w][rb * 16 + 4 * (lane >> 4) + q] = v;
        s_red[1][w][rb * 16 + 4 * (lane >> 4) + q] = p;
      }
    }
  __syncthreads();
  if (threadIdx.x < kSimTB && b0 + threadIdx.x < count) {
    const int r = threadIdx.x;
    const float z = (s_red[0][0][r] + s_red[0][1][r]) + (s_red[0][2][r] + s_red[0][3][r]);
    const float pos = (s_red[1][0][r] + s_red[1][1][r]) + (s_red[1][2][r] + s_red[1][3][r]);
    const float lz = logf(z);
    sd.logsum[b0 + r] = lz;
    sd.row_loss[b0 + r] = lz - (pos - 1.f) * inv_temp;
  }
}

// dq[i] = coef * (sum_j p_ij K_j - K_i): a block owns kSimTB query rows and streams every key tile past them.
// NCBW: 16-column blocks of the output per wave (DP <= 64 * NCBW)
template <int NCBW>
__global__ __launch_bounds__(kBlock) void sim_nce_dq_kernel(SimSides sides, int D, float inv_temp, float coef) {
  extern __shared__ float smem[];
  __shared__ float s_lse[kSimTB];
  const SimSide sd = sides.s[blockIdx.y];
  const int64_t count = *sd.count;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * kSimTB;
  if (b0 >= count) return;
  const int DP = sim_dp(D), stride = DP + 4;
  float* Qs = smem;
  float* Ks = smem + kSimTB * stride;
  float* Ps = Ks + kSimTN * stride;
  const int lane = lane_id(), w = wave_in_block();
  sim_load_rows(Qs, stride, DP, sd.Q, D, kSimTB, b0, count);
  if (threadIdx.x < kSimTB) s_lse[threadIdx.x] = b0 + threadIdx.x < count ? sd.logsum[b0 + threadIdx.x] : 0.f;
  f32x4 acc[2][NCBW];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int t = 0; t < NCBW; ++t) acc[rb][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t j0 = 0; j0 < count; j0 += kSimTN) {
    __syncthreads();   // the previous product's reads of Ks and Ps are done
    sim_load_rows(Ks, stride, DP, sd.K, D, kSimTN, j0, count);
    __syncthreads();
    f32x4 s[2];
    sim_scores(Qs, Ks, stride, DP, s);
    const bool live = j0 + w * 16 + (lane & 15) < count;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = rb * 16 + 4 * (lane >> 4) + q;
        Ps[row * kSimPS + w * 16 + (lane & 15)] = live ? expf((s[rb][q] - 1.f) * inv_temp - s_lse[row]) : 0.f;
      }
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < NCBW; ++tt) {
      const int cb = w + kWavesPerBlock * tt;
      if (cb * 16 < DP) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
          acc[rb][tt] = mma16(acc[rb][tt], Ps + rb * 16 * kSimPS, kSimPS, 1, Ks + cb * 16, stride, 1, kSimTN);
      }
    }
  }
#pragma unroll
  for (int tt = 0; tt < NCBW; ++tt) {
    const int d = (w + kWavesPerBlock * tt) * 16 + (lane & 15);
    if (d >= D) continue;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t i = b0 + rb * 16 + 4 * (lane >> 4) + q;
        if (i < count) sd.dq[i * D + d] = coef * (acc[rb][tt][q] - sd.K[i * D + d]);
      }
  }
}

// dk[j] = coef * sum_i (p_ij - [i == j]) Q_i: a block owns kSimTN key rows and streams every query tile past them; each
// of its rows is stored once
template <int NCBW>
__global__ __launch_bounds__(kBlock) void sim_nce_dk_kernel(SimSides sides, int D, float inv_temp, float coef) {
  extern __shared__ float smem[];
  __shared__ float s_lse[kSimTB];
  const SimSide sd = sides.s[blockIdx.y];
  const int64_t count = *sd.count;
  const int64_t j0 = static_cast<int64_t>(blockIdx.x) * kSimTN;
  if (j0 >= count) return;
  const int DP = sim_dp(D), stride = DP + 4;
  float* Qs = smem;
  float* Ks = smem + kSimTB * stride;
  float* Ps = Ks + kSimTN * stride;
  const int lane = lane_id(), w = wave_in_block();
  sim_load_rows(Ks, stride, DP, sd.K, D, kSimTN, j0, count);
  f32x4 acc[4][NCBW];
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int t = 0; t < NCBW; ++t) acc[jb][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t jcol = j0 + w * 16 + (lane & 15);
  for (int64_t b0 = 0; b0 < count; b0 += kSimTB) {
    __syncthreads();   // the previous product's reads of Qs and Ps are done
    if (threadIdx.x < kSimTB) s_lse[threadIdx.x] = b0 + threadIdx.x < count ? sd.logsum[b0 + threadIdx.x] : 0.f;
    sim_load_rows(Qs, stride, DP, sd.Q, D, kSimTB, b0, count);
    __syncthreads();
    f32x4 s[2];
    sim_scores(Qs, Ks, stride, DP, s);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = rb * 16 + 4 * (lane >> 4) + q;
        const int64_t i = b0 + row;
        float pv = (i < count && jcol < count) ? expf((s[rb][q] - 1.f) * inv_temp - s_lse[row]) : 0.f;
        if (i < count && i == jcol) pv -= 1.f;   // the positive, before the product
        Ps[row * kSimPS + w * 16 + (lane & 15)] = pv;
      }
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < NCBW; ++tt) {
      const int cb = w + kWavesPerBlock * tt;
      if (cb * 16 < DP) {
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)   // A = P^T: element (key, query row) at Ps[query row][key]
          acc[jb][tt] = mma16(acc[jb][tt], Ps + jb * 16, 1, kSimPS, Qs + cb * 16, stride, 1, kSimTB);
      }
    }
  }
#pragma unroll
  for (int tt = 0; tt < NCBW; ++tt) {
    const int d = (w + kWavesPerBlock * tt) * 16 + (lane & 15);
    if (d >= D) continue;
#pragma unroll
    for (int jb = 0; jb < 4; ++jb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t j = j0 + jb * 16 + 4 * (lane >> 4) + q;
        if (j < count) sd.dk[j * D + d] = coef * acc[jb][tt][q];
      }
  }
}

// back through both normalisations into the one gradient table: G[row] += scale * (inv_q (dq - Q <Q, dq>) + inv_k (dk - K
// <K, dk>)), scale = 1 / L taking the gradient from the mean-pooled row, which is what was normalised, to the hop sum.
// One wave owns a unique row, the sides own disjoint rows and the launch is alone on its stream: plain adds.
__global__ __launch_bounds__(kBlock) void sim_nce_scatter_kernel(SimSides sides, int D, float scale, float* __restrict__ G) {
  const SimSide sd = sides.s[blockIdx.y];
  const int64_t count = *sd.count;
  const int lane = lane_id();
  const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t s = wave0; s < count; s += n_waves) {
    const int64_t row = sd.off + sd.uniq[s];
    float gq[4], gk[4], xq[4], xk[4], dot_q = 0.f, dot_k = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane + kWave * k;
      const bool ok = c < D;
      gq[k] = ok ? sd.dq[s * D + c] : 0.f;
      gk[k] = ok ? sd.dk[s * D + c] : 0.f;
      xq[k] = ok ? sd.Q[s * D + c] : 0.f;
      xk[k] = ok ? sd.K[s * D + c] : 0.f;
      dot_q += gq[k] * xq[k];
      dot_k += gk[k] * xk[k];
    }
    dot_q = wave_sum(dot_q);
    dot_k = wave_sum(dot_k);
    const float wq = scale * sd.inv_q[s], wk = scale * sd.inv_k[s];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane + kWave * k;
      if (c < D) G[row * D + c] += (gq[k] - xq[k] * dot_q) * wq + (gk[k] - xk[k] * dot_k) * wk;
    }
  }
}

// ---- BPR stage: one wave per triple ------------------------------------------------------------------------------
// rows[0][t] = -log(1e-7 + sigmoid(x_t)); rows[1..3][t] = |u_t|^2, |p_t|^2, |n_t|^2 of the clean mean-pooled rows
__global__ __launch_bounds__(kBlock) void sim_bpr_partials_kernel(const float* __restrict__ pool, int64_t n_users,
                                                                  int64_t n_items, int D, float scale,
                                                                  const int64_t* __restrict__ users,
                                                                  const int64_t* __restrict__ pos,
                                                                  const int64_t* __restrict__ neg, int64_t batch,
                                                                  float* __restrict__ rows, hiprec_stats* stats) {
  const int lane = lane_id();
  const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t t = wave0; t < batch; t += n_waves) {
    const int64_t u = users[t], ip = pos[t], in = neg[t];
    const bool u_ok = static_cast<uint64_t>(u) < static_cast<uint64_t>(n_users);
    const bool i_ok = static_cast<uint64_t>(ip) < static_cast<uint64_t>(n_items) &&
                      static_cast<uint64_t>(in) < static_cast<uint64_t>(n_items);
    if (!(u_ok && i_ok)) {
      if (lane == 0) {
        atomicOr(&stats->status, (u_ok ? 0u : HIPREC_STATUS_USER_OOB) | (i_ok ? 0u : HIPREC_STATUS_ITEM_OOB));
        for (int a = 0; a < 4; ++a) rows[a * batch + t] = 0.f;
      }
      continue;
    }
    const int64_t ru = u * D, rp = (n_users + ip) * D, rn = (n_users + in) * D;
    float x = 0.f, su = 0.f, sp = 0.f, sn = 0.f;
    for (int c = lane; c < D; c += kWave) {
      const float ue = pool[ru + c] * scale, pe = pool[rp + c] * scale, ne = pool[rn + c] * scale;
      x += ue * (pe - ne);
      su += ue * ue;
      sp += pe * pe;
      sn += ne * ne;
    }
    x = wave_sum(x);
    su = wave_sum(su);
    sp = wave_sum(sp);
    sn = wave_sum(sn);
    if (lane == 0) {
      rows[t] = -logf(1e-7f + sigmoid_f32(x));
      rows[batch + t] = su;
      rows[2 * batch + t] = sp;
      rows[3 * batch + t] = sn;
    }
  }
}

// one block: every sum of the step in a fixed order.  parts = bpr, reg, cl_user, cl_item, loss, |U_b|, |P_b|, |N_b|; the
// loss for the optimizer sweep, the step counter, the workspace's step clock
__global__ __launch_bounds__(kBlock) void sim_finish_kernel(const float* __restrict__ rows, int64_t batch, SimSides sides,
                                                            float reg, float lambda, float* __restrict__ parts,
                                                            hiprec_stats* stats, Scratch* scratch, int32_t* clock) {
  __shared__ double s_sum[6][kBlock];
  for (int a = 0; a < 6; ++a) {
    double v = 0.0;
    if (a < 4) {
      for (int64_t i = threadIdx.x; i < batch; i += kBlock) v += rows[a * batch + i];
    } else {
      const SimSide sd = sides.s[a - 4];
      const int64_t count = *sd.count;
      for (int64_t i = threadIdx.x; i < count; i += kBlock) v += sd.row_loss[i];
    }
    s_sum[a][threadIdx.x] = v;
  }
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s)
      for (int a = 0; a < 6; ++a) s_sum[a][threadIdx.x] += s_sum[a][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double nu = sqrt(s_sum[1][0]), np = sqrt(s_sum[2][0]), nn = sqrt(s_sum[3][0]);
    const double r = static_cast<double>(reg) * (nu + np + nn);
    const double loss = s_sum[0][0] + r + static_cast<double>(lambda) * (s_sum[4][0] + s_sum[5][0]);
    parts[0] = static_cast<float>(s_sum[0][0]);
    parts[1] = static_cast<float>(r);
    parts[2] = static_cast<float>(s_sum[4][0]);
    parts[3] = static_cast<float>(s_sum[5][0]);
    parts[4] = static_cast<float>(loss);
    parts[5] = static_cast<float>(nu);
    parts[6] = static_cast<float>(np);
    parts[7] = static_cast<float>(nn);
    scratch->partials[0] = make_float4(parts[4], parts[1], 0.f, 0.f);
    scratch->n_partials = 1;
    advance_step(stats);
    clock[0] += 1;
  }
}

// G += scale * d loss / d (mean-pooled clean rows): -(sigma (1 - sigma)) / (1e-7 + sigma) through the score, reg * row /
// |.|_F of its batch matrix (0 for a matrix of norm 0); scale = 1 / L takes it to the hop sum.  Row atomics: a node may sit
// in several triples.
template <int NPL>
__global__ __launch_bounds__(kBlock) void sim_bpr_scatter_kernel(const float* __restrict__ pool, int64_t n_users,
                                                                 int64_t n_items, int D, float scale, float reg,
                                                                 const int64_t* __restrict__ users,
                                                                 const int64_t* __restrict__ pos,
                                                                 const int64_t* __restrict__ neg, int64_t batch,
                                                                 const float* __restrict__ parts, float* __restrict__ G) {
  const int lane = lane_id();
  const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  const float nu = parts[5], np = parts[6], nn = parts[7];
  const float cu = nu > 0.f ? scale * reg / nu : 0.f, cp = np > 0.f ? scale * reg / np : 0.f,
              cn = nn > 0.f ? scale * reg / nn : 0.f;
  for (int64_t t = wave0; t < batch; t += n_waves) {
    const int64_t u = users[t], ip = pos[t], in = neg[t];
    if (static_cast<uint64_t>(u) >= static_cast<uint64_t>(n_users) ||
        static_cast<uint64_t>(ip) >= static_cast<uint64_t>(n_items) ||
        static_cast<uint64_t>(in) >= static_cast<uint64_t>(n_items))
      continue;   // flagged by the partials pass
    const int64_t ru = u * D, rp = (n_users + ip) * D, rn = (n_users + in) * D;
    float ue[NPL], pe[NPL], ne[NPL], x = 0.f;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int c = lane + kWave * k;
      const bool ok = c < D;
      ue[k] = ok ? pool[ru + c] * scale : 0.f;
      pe[k] = ok ? pool[rp + c] * scale : 0.f;
      ne[k] = ok ? pool[rn + c] * scale : 0.f;
      x += ue[k] * (pe[k] - ne[k]);
    }
    x = wave_sum(x);
    const float sg = sigmoid_f32(x);
    const float gx = -scale * (sg * (1.f - sg)) / (1e-7f + sg);
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int c = lane + kWave * k;
      if (c < D) {
        atomic_add_f32(G + ru + c, gx * (pe[k] - ne[k]) + cu * ue[k]);
        atomic_add_f32(G + rp + c, gx * ue[k] + cp * pe[k]);
        atomic_add_f32(G + rn + c, -gx * ue[k] + cn * ne[k]);
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void sim_predict_kernel(const float* __restrict__ e0, int64_t n_users,
                                                             int64_t n_items, int D, const int64_t* __restrict__ users,
                                                             const int64_t* __restrict__ items, int64_t n,
                                                             float* __restrict__ scores, hiprec_stats* stats) {
  const int lane = lane_id();
  const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t t = wave0; t < n; t += n_waves) {
    const int64_t u = users[t], i = items[t];
    if (static_cast<uint64_t>(u) >= static_cast<uint64_t>(n_users) ||
        static_cast<uint64_t>(i) >= static_cast<uint64_t>(n_items)) {
      if (lane == 0) {
        atomicOr(&stats->status, HIPREC_STATUS_ROW_OOB);
        scores[t] = __builtin_nanf("");
      }
      continue;
    }
    float dot = 0.f;
    for (int c = lane; c < D; c += kWave) dot += e0[u * D + c] * e0[(n_users + i) * D + c];
    dot = wave_sum(dot);
    if (lane == 0) scores[t] = dot;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------
static int64_t sim_ws_floats(int64_t n_rows, int dim) { return 7 * n_rows * dim; }
static int64_t sim_stamp_ints(int64_t n_rows) { return 1 + n_rows; }
// unique ids (int64 [2][batch]) | counts (4 ints) | rows [4][batch] | per side: row_loss, logsum, inv_q, inv_k [batch] and
// Q, K, dq, dk [batch, dim]
static int64_t sim_batch_floats(int64_t batch, int dim) { return 4 * batch + 4 + 4 * batch + 2 * (4 * batch + 4 * batch * dim); }

struct SimWs {
  float *y1, *pool[3], *xa, *xb, *G;
};

static SimWs sim_ws(const hiprec_simgcl_plan* p) {
  const int64_t nd = p->a.n_rows * p->dim;
  float* w = p->ws;
  return SimWs{w, {w + nd, w + 2 * nd, w + 3 * nd}, w + 4 * nd, w + 5 * nd, w + 6 * nd};
}

static int check_sim_plan(const hiprec_simgcl_plan* p, bool train) {
  HIPREC_REQUIRE(p != nullptr, "NULL plan");
  HIPREC_REQUIRE(p->n_users > 0 && p->n_items > 0, "bad sizes");
  HIPREC_REQUIRE(p->n_layers >= 1 && p->n_layers <= HIPREC_SIMGCL_MAX_LAYERS, "SimGCL n_layer %d: 1 .. %d are supported",
                 p->n_layers, HIPREC_SIMGCL_MAX_LAYERS);
  HIPREC_REQUIRE(p->dim >= 1 && p->dim <= HIPREC_SIMGCL_MAX_DIM, "SimGCL emb_dim %d: 1 .. %d are supported", p->dim,
                 HIPREC_SIMGCL_MAX_DIM);
  HIPREC_REQUIRE(p->e0 != nullptr, "NULL e0");
  if (!train) return 0;
  HIPREC_REQUIRE(p->a.rowptr && p->a.n_rows > 0 && p->a.nnz >= 0 && (p->a.nnz == 0 || (p->a.col && p->a.val)),
                 "bad CSR a");
  HIPREC_REQUIRE(p->a.n_rows == p->n_users + p->n_items, "graph size != n_users + n_items");
  HIPREC_REQUIRE(p->a.n_rows < (1ll << 31) - 1, "more than 2^31 - 2 nodes");
  HIPREC_REQUIRE(p->at.rowptr && p->at.n_rows == p->a.n_rows && p->at.nnz == p->a.nnz &&
                     (p->a.nnz == 0 || (p->at.col && p->at.val)),
                 "bad CSR at / a and at differ");
  HIPREC_REQUIRE(p->g != nullptr && p->ws != nullptr && p->stamps != nullptr, "NULL g / ws / stamps");
  HIPREC_REQUIRE(p->ws_floats >= sim_ws_floats(p->a.n_rows, p->dim), "ws holds %lld floats, %lld are needed",
                 (long long)p->ws_floats, (long long)sim_ws_floats(p->a.n_rows, p->dim));
  HIPREC_REQUIRE(p->user_view == 1 || p->user_view == 2, "user_view %d: 1 or 2", p->user_view);
  HIPREC_REQUIRE(p->cl_temp > 0.f, "cl_temp must be positive");
  return 0;
}

static std::atomic<uint64_t> g_sim_lds_ok{0};

static int sim_allow_lds() {
  return allow_dynamic_lds({reinterpret_cast<const void*>(&sim_nce_fwd_kernel),
                            reinterpret_cast<const void*>(&sim_nce_dq_kernel<1>),
                            reinterpret_cast<const void*>(&sim_nce_dq_kernel<2>),
                            reinterpret_cast<const void*>(&sim_nce_dq_kernel<4>),
                            reinterpret_cast<const void*>(&sim_nce_dk_kernel<1>),
                            reinterpret_cast<const void*>(&sim_nce_dk_kernel<2>),
                            reinterpret_cast<const void*>(&sim_nce_dk_kernel<4>)},
                           sim_lds_bytes(HIPREC_SIMGCL_MAX_DIM, true), g_sim_lds_ok, "SimGCL's InfoNCE tiles");
}

// hops 2 .. L of one perturbed view from the shared hop 1; its pool is left as the SUM of its hops
static int sim_forward_view(const hiprec_simgcl_plan* p, const SimWs& w, int view, hipStream_t st) {
  const int64_t N = p->a.n_rows;
  const int D = p->dim, L = p->n_layers;
  const int grid = grid_for_waves(N);
  const int32_t* clock = p->stamps;
  float* cur = w.xa;
  const float* src = w.y1;
  for (int hop = 0; hop < L; ++hop) {
    if (hop > 0) {
      float* nxt = cur == w.xa ? w.xb : w.xa;
      if (int rc = launch_spmm(&p->a, nullptr, 1.f, cur, nxt, nullptr, D, st, false)) return rc;
      cur = nxt;
      src = nxt;
    }
    if (p->noise)
      sim_perturb_kernel<false><<<grid, kBlock, 0, st>>>(src, cur, w.pool[1 + view], hop == 0, view, hop, L, N, D, p->eps,
                                                         p->noise, p->noise_seed, clock);
    else
      sim_perturb_kernel<true><<<grid, kBlock, 0, st>>>(src, cur, w.pool[1 + view], hop == 0, view, hop, L, N, D, p->eps,
                                                        nullptr, p->noise_seed, clock);
    HIPREC_TRY(hipGetLastError());
  }
  return 0;
}

}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_simgcl_plan_bytes(void) { return sizeof(hiprec_simgcl_plan); }
extern "C" int32_t hiprec_simgcl_tile_b(void) { return kSimTB; }
extern "C" int32_t hiprec_simgcl_tile_n(void) { return kSimTN; }
extern "C" int32_t hiprec_simgcl_max_dim(void) { return HIPREC_SIMGCL_MAX_DIM; }
extern "C" int32_t hiprec_simgcl_max_layers(void) { return HIPREC_SIMGCL_MAX_LAYERS; }
extern "C" int64_t hiprec_simgcl_ws_floats(int64_t n_rows, int32_t dim) { return sim_ws_floats(n_rows, dim); }
extern "C" int64_t hiprec_simgcl_stamp_ints(int64_t n_rows) { return sim_stamp_ints(n_rows); }
extern "C" int64_t hiprec_simgcl_batch_ws_floats(int64_t batch, int32_t dim) { return sim_batch_floats(batch, dim); }

extern "C" int hiprec_simgcl_noise(uint64_t seed, uint64_t step, int32_t n_layers, int64_t n_rows, int32_t dim,
                                   float* out, void* stream) {
  HIPREC_REQUIRE(n_layers >= 1 && n_layers <= HIPREC_SIMGCL_MAX_LAYERS, "SimGCL n_layer %d: 1 .. %d are supported",
                 n_layers, HIPREC_SIMGCL_MAX_LAYERS);
  HIPREC_REQUIRE(dim >= 1 && dim <= HIPREC_SIMGCL_MAX_DIM, "SimGCL emb_dim %d: 1 .. %d are supported", dim,
                 HIPREC_SIMGCL_MAX_DIM);
  HIPREC_REQUIRE(n_rows > 0 && out != nullptr, "NULL out / no rows");
  sim_noise_kernel<<<grid_for_threads(2 * n_layers * n_rows * dim), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      seed, step, n_layers, n_rows, dim, out);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_simgcl_predict(const hiprec_simgcl_plan* plan, const int64_t* users, const int64_t* items,
                                     int64_t n, float* scores, hiprec_stats* stats, void* stream) {
  if (int rc = check_sim_plan(plan, false)) return rc;
  if (n == 0) return 0;
  HIPREC_REQUIRE(n > 0 && users && items && scores && stats, "NULL pointer");
  sim_predict_kernel<<<grid_for_waves(n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      plan->e0, plan->n_users, plan->n_items, plan->dim, users, items, n, scores, stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

extern "C" int hiprec_simgcl_grad(const hiprec_simgcl_plan* plan, const int64_t* users, const int64_t* pos,
                                  const int64_t* neg, int64_t batch, float* parts, hiprec_stats* stats, void* scratch,
                                  size_t scratch_bytes, void* stream) {
  if (int rc = check_sim_plan(plan, true)) return rc;
  const hiprec_simgcl_plan* p = plan;
  HIPREC_REQUIRE(batch > 0 && users && pos && neg && parts && stats && scratch, "NULL pointer / empty batch");
  HIPREC_REQUIRE(batch < (1ll << 31), "batch too large");
  HIPREC_REQUIRE(p->batch_ws && p->batch_ws_floats >= sim_batch_floats(batch, p->dim),
                 "batch_ws holds %lld floats, %lld are needed", (long long)p->batch_ws_floats,
                 (long long)sim_batch_floats(batch, p->dim));
  if (scratch_bytes < kScratchBytes) {
    set_error("scratch too small: %zu < %zu", scratch_bytes, kScratchBytes);
    return HIPREC_E_SCRATCH;
  }
  if (int rc = sim_allow_lds()) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const SimWs w = sim_ws(p);
  const int D = p->dim, L = p->n_layers;
  const int64_t N = p->a.n_rows, nd = N * D, B = batch;
  const float scale = 1.0f / static_cast<float>(L);

  int64_t* uniq = reinterpret_cast<int64_t*>(p->batch_ws);
  int32_t* counts = reinterpret_cast<int32_t*>(p->batch_ws + 4 * B);
  float* rows = p->batch_ws + 4 * B + 4;
  SimSides sides;
  float* f = rows + 4 * B;
  for (int s = 0; s < 2; ++s) {
    SimSide& sd = sides.s[s];
    const bool self = s == 0 && p->user_view == 1;
    sd.uniq = uniq + s * B;
    sd.count = counts + s;
    sd.off = s ? p->n_users : 0;
    sd.pool_q = w.pool[1];
    sd.pool_k = self ? w.pool[1] : w.pool[2];
    sd.row_loss = f;
    sd.logsum = f + B;
    sd.inv_q = f + 2 * B;
    sd.inv_k = self ? sd.inv_q : f + 3 * B;
    sd.Q = f + 4 * B;
    sd.K = self ? sd.Q : sd.Q + B * D;
    sd.dq = sd.Q + 2 * B * D;
    sd.dk = sd.Q + 3 * B * D;
    f += 4 * B + 4 * B * D;
  }

  // the unique ids of both sides, in device memory
  sim_stamp_kernel<<<grid_for_threads(B), kBlock, 0, st>>>(users, pos, B, p->n_users, p->n_items, p->stamps);
  sim_compact_kernel<<<2, kBlock, 0, st>>>(p->stamps, p->n_users, p->n_items, B, uniq, counts);
  HIPREC_TRY(hipGetLastError());

  // forward: hop 1 once, then the clean chain and the two perturbed ones
  HIPREC_TRY(hipMemsetAsync(w.G, 0, sizeof(float) * nd, st));
  if (int rc = launch_spmm(&p->a, nullptr, 1.f, p->e0, w.y1, nullptr, D, st, false)) return rc;
  HIPREC_TRY(hipMemcpyAsync(w.pool[0], w.y1, sizeof(float) * nd, hipMemcpyDeviceToDevice, st));
  {
    const float* cur = w.y1;
    for (int hop = 1; hop < L; ++hop) {
      float* nxt = (hop & 1) ? w.xa : w.xb;
      if (int rc = launch_spmm(&p->a, nullptr, 1.f, cur, nxt, w.pool[0], D, st, false)) return rc;
      cur = nxt;
    }
  }
  if (int rc = sim_forward_view(p, w, 0, st)) return rc;
  if (int rc = sim_forward_view(p, w, 1, st)) return rc;

  // the contrastive term among the unique rows
  const float inv_temp = 1.0f / p->cl_temp, coef = p->lambda / p->cl_temp;
  const unsigned b_tiles = static_cast<unsigned>((B + kSimTB - 1) / kSimTB), n_tiles = static_cast<unsigned>((B + kSimTN - 1) / kSimTN);
  const dim3 row_grid(grid_for_waves(B), 2);
  sim_gather_kernel<<<row_grid, kBlock, 0, st>>>(sides, D, scale);
  sim_nce_fwd_kernel<<<dim3(b_tiles, 2), kBlock, sim_lds_bytes(D, false), st>>>(sides, D, inv_temp);
  HIPREC_TRY(hipGetLastError());
  const size_t lds = sim_lds_bytes(D, true);
  if (D <= 64) {
    sim_nce_dq_kernel<1><<<dim3(b_tiles, 2), kBlock, lds, st>>>(sides, D, inv_temp, coef);
    sim_nce_dk_kernel<1><<<dim3(n_tiles, 2), kBlock, lds, st>>>(sides, D, inv_temp, coef);
  } else if (D <= 128) {
    sim_nce_dq_kernel<2><<<dim3(b_tiles, 2), kBlock, lds, st>>>(sides, D, inv_temp, coef);
    sim_nce_dk_kernel<2><<<dim3(n_tiles, 2), kBlock, lds, st>>>(sides, D, inv_temp, coef);
  } else {
    sim_nce_dq_kernel<4><<<dim3(b_tiles, 2), kBlock, lds, st>>>(sides, D, inv_temp, coef);
    sim_nce_dk_kernel<4><<<dim3(n_tiles, 2), kBlock, lds, st>>>(sides, D, inv_temp, coef);
  }
  HIPREC_TRY(hipGetLastError());
  sim_nce_scatter_kernel<<<row_grid, kBlock, 0, st>>>(sides, D, scale, w.G);

  // the BPR stage on the clean pool: the norms first, then the scatter
  const int grid = grid_for_waves(B);
  sim_bpr_partials_kernel<<<grid, kBlock, 0, st>>>(w.pool[0], p->n_users, p->n_items, D, scale, users, pos, neg, B, rows,
                                                   stats);
  sim_finish_kernel<<<1, kBlock, 0, st>>>(rows, B, sides, p->reg, p->lambda, parts, stats, static_cast<Scratch*>(scratch),
                                          p->stamps);
  if (D <= 64)
    sim_bpr_scatter_kernel<1><<<grid, kBlock, 0, st>>>(w.pool[0], p->n_users, p->n_items, D, scale, p->reg, users, pos, neg,
                                                       B, parts, w.G);
  else if (D <= 128)
    sim_bpr_scatter_kernel<2><<<grid, kBlock, 0, st>>>(w.pool[0], p->n_users, p->n_items, D, scale, p->reg, users, pos, neg,
                                                       B, parts, w.G);
  else
    sim_bpr_scatter_kernel<4><<<grid, kBlock, 0, st>>>(w.pool[0], p->n_users, p->n_items, D, scale, p->reg, users, pos, neg,
                                                       B, parts, w.G);
  HIPREC_TRY(hipGetLastError());

  // ONE backward chain for the three views (G already carries the 1 / L of the mean): h = G; (L - 1) x: h = G + A^T h;
  // g += A^T h
  const float* h = w.G;
  for (int k = 1; k < L; ++k) {
    float* nxt = (k & 1) ? w.xa : w.xb;
    HIPREC_TRY(hipMemcpyAsync(nxt, w.G, sizeof(float) * nd, hipMemcpyDeviceToDevice, st));
    // the SpMM only ever ADDS into its output, so with y_is_zero it accumulates onto what is there
    if (int rc = launch_spmm(&p->at, nullptr, 1.f, h, nxt, nullptr, D, st, true)) return rc;
    h = nxt;
  }
  return launch_spmm(&p->at, nullptr, 1.f, h, p->g, nullptr, D, st, true);
}
