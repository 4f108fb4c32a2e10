// SR-GNN (Wu et al., AAAI 2019): zero_grad + forward + loss + backward of one training step as a fixed sequence of
// launches (their number depends on `step` and `nonhybrid` alone), no host sync and no device-scope float atomic apart
// from the row atomics that fold the node gradients into embedding.weight.
//
//   graph       two launches: the distinct ids of every session are counted, then one workgroup per session builds in LDS
//               its nodes (ascending ids), alias, the deduplicated edge set and both orientations of it as ragged lists;
//               the batch-wide node offset is the ordered sum of the counts of the sessions in front.  The node total N is
//               known on the device only: everything over node rows is launched for R = sum(lens) >= N rows, and a row
//               that belongs to no session (node_sess < 0) is written as zeros everywhere, so it adds nothing to any sum.
//   cell        per repetition: ONE grouped launch h -> [W_in h + b_in | W_out h + b_out | w_hh h + b_hh] ([R, 5H]); one wave
//               per node: both neighbourhood means plus b_iah / b_oah ([R, 2H]); gi = [a_in | a_out] w_ih^T + b_ih; the gate
//   readout     h_T gathered, q1 = linear_one(h_T) and q2 = linear_two(h) PER NODE (x_t = h[alias[t]] makes linear_two(x_t) a
//               gather of it) in one grouped launch; one wave per session walks the session's nodes, each weighted by the
//               number of positions that name it: alpha, s_g; a = linear_transform([s_g | h_T])
//   scores      a E[1:]^T into the workspace, a block per row turns them into dscores in place; d a = dscores E[1:] as
//               kSrgnnKSlices K slices of the grouped GEMM added up in slice order; d E[1:] = dscores^T a is WRITTEN
//   backward    readout per session: the wave writes d x of its own node rows, the positions that name one node folded into
//               that node's count (nobody else touches those rows); per repetition in reverse: the gate, d [a_in |
//               a_out] and the w_hh term by GEMMs, the means' backward per node from the OTHER list -- the gradient of the
//               in-mean with respect to u's projection is the sum over u's out-list of d a_in[v] / indeg(v) -- and W_in,
//               W_out back to d h.  All weight and bias gradients of the cell come last, as products / column sums over
//               the rows of ALL repetitions at once (the saved activations of the repetitions are contiguous), without
//               split-K and with two-level fixed-order column sums.
#include <algorithm>

#include "gemm.hpp"
#include "srgnn.hpp"

namespace hiprec {
namespace {

static_assert(kSrgnnMaxLen <= kBlock, "one builder thread per position");
static_assert(kSrgnnWaves == kWavesPerBlock && kSrgnnKSlices <= kMaxGroup, "srgnn.hpp restates the launch constants");

__device__ __forceinline__ int sr_len(const int64_t* lens, int64_t b, int T) {
  const int64_t l = lens[b];
  return l < 0 ? 0 : (l > T ? T : static_cast<int>(l));
}

struct SrGraph {
  int *n_nodes, *node_off, *slot_off, *alias, *nodes, *node_sess, *node_cnt, *in_start, *indeg, *out_start, *outdeg,
      *in_idx, *out_idx;
  int64_t ints;
};

SrGraph sr_graph_carve(int* base, int64_t B, int T, int64_t R) {
  SrGraph g{};
  int* c = base;
  auto take = [&](int64_t n) { int* r = c; c += n; return r; };
  g.n_nodes = take(B);
  g.node_off = take(B + 1);
  g.slot_off = take(B + 1);
  g.alias = take(B * T);
  g.nodes = take(R);
  g.node_sess = take(R);
  g.node_cnt = take(R);
  g.in_start = take(R);
  g.indeg = take(R);
  g.out_start = take(R);
  g.outdeg = take(R);
  g.in_idx = take(R);
  g.out_idx = take(R);
  g.ints = c - base;
  return g;
}

// ---- graph builder ------------------------------------------------------------------------------------------------------
// the id of position t of session b, or -1 behind its length; an id outside [1, n_node) raises the status and counts as 1
__device__ __forceinline__ int sr_load_id(const int64_t* seq, int64_t B, int64_t b, int t, int len, int64_t n_node,
                                          hiprec_stats* stats) {
  if (t >= len) return -1;
  int64_t id = seq[static_cast<int64_t>(t) * B + b];
  if (id < 1 || id >= n_node) {
    atomicOr(&stats->status, HIPREC_STATUS_ITEM_OOB);
    id = 1;
  }
  return static_cast<int>(id);
}

// grid = B: n_nodes[b]; the blocks also fill the per-row lists with what a row of no session holds
__global__ __launch_bounds__(kBlock) void srgnn_count_kernel(const int64_t* __restrict__ seq,
                                                             const int64_t* __restrict__ lens, int64_t B, int T,
                                                             int64_t R, int64_t n_node, SrGraph g, hiprec_stats* stats) {
  __shared__ int s_id[kSrgnnMaxLen];
  const int64_t b = blockIdx.x;
  const int t = threadIdx.x, len = sr_len(lens, b, T);
  for (int64_t e = b * kBlock + t; e < R; e += B * kBlock) {
    g.nodes[e] = 0;
    g.node_sess[e] = -1;
    g.node_cnt[e] = 0;
    g.in_start[e] = 0;
    g.indeg[e] = 0;
    g.out_start[e] = 0;
    g.outdeg[e] = 0;
    g.in_idx[e] = -1;
    g.out_idx[e] = -1;
  }
  const int id = sr_load_id(seq, B, b, t, len, n_node, stats);
  s_id[t] = id;
  __syncthreads();
  bool first = id >= 0;
  for (int u = 0; u < t && first; ++u) first = s_id[u] != id;
  const int count = __syncthreads_count(first);
  if (t == 0) g.n_nodes[b] = count;
}

// grid = B.  A session whose slots would not fit n_rows (the caller's sum of lens was too small) raises ROW_OOB and
// writes nothing but its alias row of -1.
__global__ __launch_bounds__(kBlock) void srgnn_graph_kernel(const int64_t* __restrict__ seq,
                                                             const int64_t* __restrict__ lens, int64_t B, int T,
                                                             int64_t R, int64_t n_node, SrGraph g, hiprec_stats* stats) {
  __shared__ int s_id[kSrgnnMaxLen], s_al[kSrgnnMaxLen], s_key[kSrgnnMaxLen];
  __shared__ int s_base[2];
  const int64_t b = blockIdx.x;
  const int t = threadIdx.x, len = sr_len(lens, b, T);
  if (t < 2) s_base[t] = 0;
  __syncthreads();
  {
    int nodes_before = 0, slots_before = 0;      // integer sums: any order gives the same offsets
    for (int64_t p = t; p < b; p += kBlock) {
      nodes_before += g.n_nodes[p];
      slots_before += sr_len(lens, p, T);
    }
    if (nodes_before) atomicAdd(&s_base[0], nodes_before);
    if (slots_before) atomicAdd(&s_base[1], slots_before);
  }
  const int id = sr_load_id(seq, B, b, t, len, n_node, stats);
  s_id[t] = id;
  __syncthreads();
  const int node_base = s_base[0], slot_base = s_base[1], count = g.n_nodes[b];
  const bool fits = static_cast<int64_t>(slot_base) + len <= R;
  if (t == 0) {
    g.node_off[b] = node_base;
    g.slot_off[b] = slot_base;
    if (b == B - 1) {
      g.node_off[B] = node_base + count;
      g.slot_off[B] = slot_base + len;
    }
    if (!fits) atomicOr(&stats->status, HIPREC_STATUS_ROW_OOB);
  }
  if (!fits) {
    if (t < T) g.alias[static_cast<int64_t>(t) * B + b] = -1;
    return;
  }
  // a position is the first of its id; its node = the number of distinct smaller ids
  bool first = id >= 0;
  for (int u = 0; u < t && first; ++u) first = s_id[u] != id;
  s_key[t] = first ? id : -1;
  __syncthreads();
  int al = -1;
  if (id >= 0) {
    al = 0;
    for (int u = 0; u < len; ++u) al += (s_key[u] >= 0 && s_key[u] < id) ? 1 : 0;
  }
  s_al[t] = al;
  if (t < T) g.alias[static_cast<int64_t>(t) * B + b] = al >= 0 ? node_base + al : -1;
  if (first) {
    int cnt = 0;
    for (int u = 0; u < len; ++u) cnt += s_id[u] == id ? 1 : 0;
    g.nodes[node_base + al] = id;
    g.node_sess[node_base + al] = static_cast<int>(b);
    g.node_cnt[node_base + al] = cnt;
  }
  __syncthreads();
  // edges (alias[t], alias[t + 1]) as keys u * 256 + v; the first occurrence of a key is the edge
  const int n_tr = len - 1;
  int key = -1;
  if (t < n_tr) key = s_al[t] * kSrgnnMaxLen + s_al[t + 1];
  s_id[t] = key;
  __syncthreads();
  bool efirst = key >= 0;
  for (int u = 0; u < t && efirst; ++u) efirst = s_id[u] != key;
  s_key[t] = efirst ? key : -1;
  __syncthreads();
  if (efirst) {
    // its slot in the out-lists = its rank among the edges ordered by (u, v), in the in-lists by (v, u)
    const int eu = key / kSrgnnMaxLen, ev = key % kSrgnnMaxLen, key_in = ev * kSrgnnMaxLen + eu;
    int r_out = 0, r_in = 0;
    for (int u = 0; u < n_tr; ++u) {
      const int k = s_key[u];
      if (k < 0) continue;
      r_out += k < key ? 1 : 0;
      r_in += (k % kSrgnnMaxLen) * kSrgnnMaxLen + k / kSrgnnMaxLen < key_in ? 1 : 0;
    }
    g.out_idx[slot_base + r_out] = node_base + ev;
    g.in_idx[slot_base + r_in] = node_base + eu;
  }
  if (t < count) {
    int o_lt = 0, o_eq = 0, i_lt = 0, i_eq = 0;
    for (int u = 0; u < n_tr; ++u) {
      const int k = s_key[u];
      if (k < 0) continue;
      const int eu = k / kSrgnnMaxLen, ev = k % kSrgnnMaxLen;
      o_lt += eu < t ? 1 : 0;
      o_eq += eu == t ? 1 : 0;
      i_lt += ev < t ? 1 : 0;
      i_eq += ev == t ? 1 : 0;
    }
    g.out_start[node_base + t] = slot_base + o_lt;
    g.outdeg[node_base + t] = o_eq;
    g.in_start[node_base + t] = slot_base + i_lt;
    g.indeg[node_base + t] = i_eq;
  }
}

// ---- the cell -----------------------------------------------------------------------------------------------------------
// h0 [R, H] = embedding[nodes], 0 in a row of no session
__global__ __launch_bounds__(kBlock) void srgnn_embed_kernel(const float* __restrict__ emb, SrGraph g, int64_t R, int H,
                                                             float* __restrict__ h0) {
  const int64_t n = R * H, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
    const int64_t v = e / H;
    const int j = static_cast<int>(e - v * H);
    h0[e] = g.node_sess[v] >= 0 ? emb[static_cast<int64_t>(g.nodes[v]) * H + j] : 0.f;
  }
}

// one wave per node: A[v] = [b_iah + mean of P_in over v's in-list | b_oah + mean of P_out over its out-list]; an empty
// list leaves the bias alone.  P [R, 5H] = [P_in | P_out | gh].
__global__ __launch_bounds__(kBlock) void srgnn_mean_fwd_kernel(const float* __restrict__ P,
                                                                const float* __restrict__ b_iah,
                                                                const float* __restrict__ b_oah, SrGraph g, int64_t R,
                                                                int H, float* __restrict__ A) {
  const int lane = lane_id();
  const int64_t H5 = 5 * static_cast<int64_t>(H);
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); v < R;
       v += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const bool live = g.node_sess[v] >= 0;
    const int n_in = live ? g.indeg[v] : 0, n_out = live ? g.outdeg[v] : 0;
    const int* in_l = g.in_idx + g.in_start[v];
    const int* out_l = g.out_idx + g.out_start[v];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = lane + 64 * h;
      if (j >= H) continue;
      float a_in = 0.f, a_out = 0.f;
      if (live) {
        float s = 0.f;
        for (int k = 0; k < n_in; ++k) s += P[in_l[k] * H5 + j];
        a_in = b_iah[j] + (n_in ? s / static_cast<float>(n_in) : 0.f);
        s = 0.f;
        for (int k = 0; k < n_out; ++k) s += P[out_l[k] * H5 + H + j];
        a_out = b_oah[j] + (n_out ? s / static_cast<float>(n_out) : 0.f);
      }
      A[v * 2 * H + j] = a_in;
      A[v * 2 * H + H + j] = a_out;
    }
  }
}

// one wave per node: dP[u] = [sum over u's out-list of dA_in[v] / indeg(v) | sum over its in-list of dA_out[w] / outdeg(w)]
// dP has the leading dimension of P (it overwrites P's first 2H columns)
__global__ __launch_bounds__(kBlock) void srgnn_mean_bwd_kernel(const float* __restrict__ dA, SrGraph g, int64_t R, int H,
                                                                float* __restrict__ dP) {
  const int lane = lane_id();
  const int64_t H5 = 5 * static_cast<int64_t>(H), H2 = 2 * static_cast<int64_t>(H);
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); u < R;
       u += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const bool live = g.node_sess[u] >= 0;
    const int n_in = live ? g.indeg[u] : 0, n_out = live ? g.outdeg[u] : 0;
    const int* in_l = g.in_idx + g.in_start[u];
    const int* out_l = g.out_idx + g.out_start[u];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = lane + 64 * h;
      if (j >= H) continue;
      float d_in = 0.f, d_out = 0.f;
      for (int k = 0; k < n_out; ++k) {
        const int v = out_l[k];
        d_in += dA[v * H2 + j] / static_cast<float>(g.indeg[v]);
      }
      for (int k = 0; k < n_in; ++k) {
        const int w = in_l[k];
        d_out += dA[w * H2 + H + j] / static_cast<float>(g.outdeg[w]);
      }
      dP[u * H5 + j] = d_in;
      dP[u * H5 + H + j] = d_out;
    }
  }
}

// G [R, 3H] holds gi on entry and the gates r | z | n on exit; h_new = n + z (h - n), 0 in a row of no session
__global__ __launch_bounds__(kBlock) void srgnn_gate_fwd_kernel(const float* __restrict__ P, const float* __restrict__ h,
                                                                SrGraph g, int64_t R, int H, float* __restrict__ G,
                                                                float* __restrict__ h_new) {
  const int64_t n = R * H, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
    const int64_t v = e / H;
    const int j = static_cast<int>(e - v * H);
    float* gp = G + v * 3 * H + j;
    if (g.node_sess[v] < 0) {
      gp[0] = gp[H] = gp[2 * H] = 0.f;
      h_new[e] = 0.f;
      continue;
    }
    const float* gh = P + v * 5 * H + 2 * H + j;
    const float rr = sigmoid_f32(gp[0] + gh[0]);
    const float zz = sigmoid_f32(gp[H] + gh[H]);
    const float nn = tanhf(gp[2 * H] + rr * gh[2 * H]);
    gp[0] = rr;
    gp[H] = zz;
    gp[2 * H] = nn;
    h_new[e] = nn + zz * (h[e] - nn);
  }
}

// The gradient that reaches h' of one repetition is the sum of up to four [R, H] terms, in this order, plus, on the last
// node of a session, the two [B, H] terms of h_T.
struct SrGradIn {
  const float* src[4];
  const float *last_a, *last_b;
};

__device__ __forceinline__ float sr_grad_in(const SrGradIn& in, const SrGraph& g, const int64_t* lens, int64_t B, int T,
                                            int64_t v, int j, int H) {
  float d = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (in.src[i]) d += in.src[i][v * H + j];
  if (in.last_a) {
    const int64_t b = g.node_sess[v];
    const int len = sr_len(lens, b, T);
    if (len > 0 && g.alias[static_cast<int64_t>(len - 1) * B + b] == v) d += in.last_a[b * H + j] + in.last_b[b * H + j];
  }
  return d;
}

// G (the gates) becomes dGi in place, the gh columns of P become dGh in place, dhc = d h' z (the direct path to h)
__global__ __launch_bounds__(kBlock) void srgnn_gate_bwd_kernel(SrGradIn in, const float* __restrict__ h, SrGraph g,
                                                                const int64_t* __restrict__ lens, int64_t B, int T,
                                                                int64_t R, int H, float* __restrict__ G,
                                                                float* __restrict__ P, float* __restrict__ dhc) {
  const int64_t n = R * H, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
    const int64_t v = e / H;
    const int j = static_cast<int>(e - v * H);
    float* gp = G + v * 3 * H + j;
    float* gh = P + v * 5 * H + 2 * H + j;
    float d_r = 0.f, d_z = 0.f, d_n = 0.f, d_hn = 0.f, d_c = 0.f;
    if (g.node_sess[v] >= 0) {
      const float d = sr_grad_in(in, g, lens, B, T, v, j, H);
      const float rr = gp[0], zz = gp[H], nn = gp[2 * H];
      d_n = d * (1.f - zz) * (1.f - nn * nn);
      d_z = d * (h[e] - nn) * zz * (1.f - zz);
      d_r = d_n * gh[2 * H] * rr * (1.f - rr);
      d_hn = d_n * rr;
      d_c = d * zz;
    }
    gp[0] = d_r;
    gp[H] = d_z;
    gp[2 * H] = d_n;
    gh[0] = d_r;
    gh[H] = d_z;
    gh[2 * H] = d_hn;
    dhc[e] = d_c;
  }
}

// d embedding[nodes[v]] += the gradient of h0: the only device-scope float atomics of the step
__global__ __launch_bounds__(kBlock) void srgnn_embed_bwd_kernel(SrGradIn in, SrGraph g, int64_t R, int H,
                                                                 float* __restrict__ g_emb) {
  const int64_t n = R * H, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
    const int64_t v = e / H;
    const int j = static_cast<int>(e - v * H);
    if (g.node_sess[v] < 0) continue;
    const float d = sr_grad_in(in, g, nullptr, 0, 0, v, j, H);
    if (d != 0.f) atomic_add_f32(g_emb + static_cast<int64_t>(g.nodes[v]) * H + j, d);
  }
}

// ---- readout: one wave per session, H <= 128 = two values per lane -------------------------------------------------------
// a session the builder skipped has alias -1 everywhere: it counts as empty
__device__ __forceinline__ int sr_live_len(const SrGraph& g, const int64_t* lens, int64_t b, int64_t B, int T) {
  const int len = sr_len(lens, b, T);
  return (len > 0 && g.alias[b] >= 0) ? len : 0;
}

// cat [B, 2H]: the h_T half
__global__ __launch_bounds__(kBlock) void srgnn_last_kernel(const float* __restrict__ h, SrGraph g,
                                                            const int64_t* __restrict__ lens, int64_t B, int T, int H,
                                                            float* __restrict__ cat) {
  const int64_t n = B * H, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
    const int64_t b = e / H;
    const int j = static_cast<int>(e - b * H);
    const int len = sr_live_len(g, lens, b, B, T);
    cat[b * 2 * H + H + j] = len ? h[static_cast<int64_t>(g.alias[static_cast<int64_t>(len - 1) * B + b]) * H + j] : 0.f;
  }
}

// alpha_t depends on the position only through its node (q1 belongs to the session, q2 to the node), so the wave walks the
// session's NODES and weighs each by the number of positions that name it: s_g = sum_v cnt(v) alpha(v) h[v].  (Adding a
// revisited node's term once per position instead drifts: 256 equal addends lost 1.6e-5 of s_g in fp32.)
// alpha [R] per node row; cat's s_g half; sg_out (nonhybrid: the query itself) [B, H] or NULL
__global__ __launch_bounds__(kBlock) void srgnn_readout_fwd_kernel(const float* __restrict__ h,
                                                                   const float* __restrict__ q1,
                                                                   const float* __restrict__ q2,
                                                                   const float* __restrict__ w3, SrGraph g,
                                                                   const int64_t* __restrict__ lens, int64_t B, int T,
                                                                   int H, float* __restrict__ alpha,
                                                                   float* __restrict__ cat, float* __restrict__ sg_out) {
  const int lane = lane_id();
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); b < B;
       b += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const bool live = sr_live_len(g, lens, b, B, T) > 0;
    const int64_t v0 = g.node_off[b], v1 = live ? v0 + g.n_nodes[b] : v0;
    float q[2], w[2], c[2] = {0.f, 0.f};
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int j = lane + 64 * hh;
      q[hh] = j < H ? q1[b * H + j] : 0.f;
      w[hh] = j < H ? w3[j] : 0.f;
    }
    for (int64_t row = v0; row < v1; ++row) {
      float x[2] = {0.f, 0.f}, part = 0.f;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int j = lane + 64 * hh;
        if (j < H) {
          x[hh] = h[row * H + j];
          part += w[hh] * sigmoid_f32(q[hh] + q2[row * H + j]);
        }
      }
      const float a = wave_sum(part) * static_cast<float>(g.node_cnt[row]);
      if (lane == 0) alpha[row] = a;
      c[0] += a * x[0];
      c[1] += a * x[1];
    }
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int j = lane + 64 * hh;
      if (j < H) {
        cat[b * 2 * H + j] = c[hh];
        if (sg_out) sg_out[b * H + j] = c[hh];
      }
    }
  }
}

// dcat [B, ldd]: d s_g in its first H columns, d h_T behind them when has_ht.  The wave WRITES dq2 and dh of its own node
// rows (rows of no session are zero on entry and stay so).  dq1, vs (the rows whose column sum is d linear_three),
// dhT [B, H].  alpha holds cnt(v) alpha(v).
__global__ __launch_bounds__(kBlock) void srgnn_readout_bwd_kernel(
    const float* __restrict__ h, const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ w3,
    const float* __restrict__ alpha, const float* __restrict__ dcat, int ldd, int has_ht, SrGraph g,
    const int64_t* __restrict__ lens, int64_t B, int T, int H, float* __restrict__ dq2, float* __restrict__ dh,
    float* __restrict__ dq1, float* __restrict__ vs, float* __restrict__ dhT) {
  const int lane = lane_id();
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); b < B;
       b += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    const bool live = sr_live_len(g, lens, b, B, T) > 0;
    const int64_t v0 = g.node_off[b], v1 = live ? v0 + g.n_nodes[b] : v0;
    float q[2], w[2], ds[2], a1[2] = {0.f, 0.f}, av[2] = {0.f, 0.f};
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int j = lane + 64 * hh;
      q[hh] = j < H ? q1[b * H + j] : 0.f;
      w[hh] = j < H ? w3[j] : 0.f;
      ds[hh] = j < H ? dcat[b * ldd + j] : 0.f;
      if (j < H) dhT[b * H + j] = has_ht ? dcat[b * ldd + H + j] : 0.f;
    }
    for (int64_t row = v0; row < v1; ++row) {
      float s[2] = {0.f, 0.f}, part = 0.f;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int j = lane + 64 * hh;
        if (j < H) {
          part += ds[hh] * h[row * H + j];
          s[hh] = sigmoid_f32(q[hh] + q2[row * H + j]);
        }
      }
      const float da = wave_sum(part) * static_cast<float>(g.node_cnt[row]), a = alpha[row];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int j = lane + 64 * hh;
        if (j < H) {
          const float dpre = da * w[hh] * s[hh] * (1.f - s[hh]);
          av[hh] += da * s[hh];
          a1[hh] += dpre;
          dq2[row * H + j] = dpre;
          dh[row * H + j] = a * ds[hh];
        }
      }
    }
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int j = lane + 64 * hh;
      if (j < H) {
        dq1[b * H + j] = a1[hh];
        vs[b * H + j] = av[hh];
      }
    }
  }
}

// ---- cross-entropy over items 1 .. n_node - 1: a block per row, any I (NARM's form with the target shifted) ---------------
__device__ __forceinline__ float sr_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ float sr_block_reduce(float v, float* s_red, bool is_max) {
  v = is_max ? sr_wave_max(v) : wave_sum(v);
  __syncthreads();
  if (lane_id() == 0) s_red[wave_in_block()] = v;
  __syncthreads();
  float r = s_red[0];
#pragma unroll
  for (int i = 1; i < kWavesPerBlock; ++i) r = is_max ? fmaxf(r, s_red[i]) : r + s_red[i];
  return r;
}

// scores [B, I] (column i = item i + 1) -> dscores = (softmax - onehot) / B in place; the block's loss partial
__global__ __launch_bounds__(kBlock) void srgnn_ce_kernel(float* __restrict__ scores, const int64_t* __restrict__ target,
                                                          int64_t B, int64_t I, Scratch* scratch, hiprec_stats* stats) {
  __shared__ float s_red[kWavesPerBlock];
  const float inv_b = 1.0f / static_cast<float>(B);
  float loss = 0.f;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    float* row = scores + b * I;
    float mx = -INFINITY;
    for (int64_t i = threadIdx.x; i < I; i += kBlock) mx = fmaxf(mx, row[i]);
    mx = sr_block_reduce(mx, s_red, true);
    float sum = 0.f;
    for (int64_t i = threadIdx.x; i < I; i += kBlock) sum += expf(row[i] - mx);
    sum = sr_block_reduce(sum, s_red, false);
    const float lse = mx + logf(sum);
    const int64_t tg = target[b] - 1;
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

// out[e] = part[0][e] + part[1][e] + ... in slice order
__global__ __launch_bounds__(kBlock) void srgnn_slice_sum_kernel(const float* __restrict__ part, int n_slices, int64_t n,
                                                                 float* __restrict__ out) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
    float s = part[e];
    for (int z = 1; z < n_slices; ++z) s += part[z * n + e];
    out[e] = s;
  }
}

// Adam's weight decay: g += l2 * w over the whole flat buffer
__global__ __launch_bounds__(kBlock) void srgnn_l2_kernel(const float* __restrict__ w, float* __restrict__ g, int64_t n,
                                                          float l2) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) g[e] = fmaf(l2, w[e], g[e]);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
struct SrParams {      // pointers into a flat buffer laid out in state_dict() order
  float *emb, *w_ih, *w_hh, *b_ih, *b_hh, *b_iah, *b_oah, *w_in, *b_in, *w_out, *b_out, *w1, *b1, *w2, *b2, *w3, *wt, *bt;
};

int64_t sr_n_params(const hiprec_srgnn_shape& s) {
  const int64_t H = s.hidden;
  return s.n_node * H + 6 * H * H + 3 * H * H + 6 * H + 2 * H + 2 * (H * H + H) + 2 * (H * H + H) + H + 2 * H * H + H;
}

SrParams sr_params(float* base, const hiprec_srgnn_shape& s) {
  SrParams p{};
  const int64_t H = s.hidden;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += n; return r; };
  p.emb = take(s.n_node * H);
  p.w_ih = take(6 * H * H);
  p.w_hh = take(3 * H * H);
  p.b_ih = take(3 * H);
  p.b_hh = take(3 * H);
  p.b_iah = take(H);
  p.b_oah = take(H);
  p.w_in = take(H * H);
  p.b_in = take(H);
  p.w_out = take(H * H);
  p.b_out = take(H);
  p.w1 = take(H * H);
  p.b1 = take(H);
  p.w2 = take(H * H);
  p.b2 = take(H);
  p.w3 = take(H);
  p.wt = take(2 * H * H);
  p.bt = take(H);
  return p;
}

// the fixed K slices of d a = dscores E[1:]: kTK-aligned stretches, as many as hold anything
void sr_slices(int64_t K, int* n_slices, int* k_per) {
  int per = static_cast<int>((K + kSrgnnKSlices - 1) / kSrgnnKSlices);
  per = (per + 31) / 32 * 32;
  *k_per = per;
  *n_slices = static_cast<int>((K + per - 1) / per);
}

struct SrWorkspace {
  SrGraph graph;
  float *hs, *P, *A, *G, *dA, *q2, *alpha, *cat, *q1, *query;
  float *scores, *part, *da, *dcat, *dq1, *vs, *dhT, *dhT2, *dq2, *dhc, *dhg, *dpi, *dpo;
  float *cs_t, *cs_1, *cs_2, *cs_3, *cs_ih, *cs_hh, *cs_iah, *cs_oah, *cs_in, *cs_out;
  int64_t floats;
};

SrWorkspace sr_carve(float* base, const hiprec_srgnn_shape& s, int64_t B, int T, int64_t R, bool train) {
  SrWorkspace w{};
  const int64_t H = s.hidden, S = s.step, I = s.n_node - 1;
  float* c = base;
  auto take = [&](int64_t n) { float* r = c; c += (n + 3) / 4 * 4; return r; };
  w.graph = sr_graph_carve(reinterpret_cast<int*>(c), B, T, R);
  take(w.graph.ints);
  w.hs = take((S + 1) * R * H);
  w.P = take(S * R * 5 * H);
  w.A = take(S * R * 2 * H);
  w.G = take(S * R * 3 * H);
  w.q2 = take(R * H);
  w.alpha = take(R);
  w.cat = take(B * 2 * H);
  w.q1 = take(B * H);
  w.query = take(B * H);
  if (train) {
    const int SR = static_cast<int>(S * R), Bi = static_cast<int>(B), Hi = static_cast<int>(H);
    w.dA = take(S * R * 2 * H);
    w.scores = take(B * I);
    w.part = take(kSrgnnKSlices * B * H);
    w.da = take(B * H);
    w.dcat = take(B * 2 * H);
    w.dq1 = take(B * H);
    w.vs = take(B * H);
    w.dhT = take(B * H);
    w.dhT2 = take(B * H);
    w.dq2 = take(R * H);
    w.dhc = take(R * H);
    w.dhg = take(R * H);
    w.dpi = take(R * H);
    w.dpo = take(R * H);
    w.cs_t = take(colsum_ws_floats(Bi, Hi));
    w.cs_1 = take(colsum_ws_floats(Bi, Hi));
    w.cs_2 = take(colsum_ws_floats(static_cast<int>(R), Hi));
    w.cs_3 = take(colsum_ws_floats(Bi, Hi));
    w.cs_ih = take(colsum_ws_floats(SR, 3 * Hi));
    w.cs_hh = take(colsum_ws_floats(SR, 3 * Hi));
    w.cs_iah = take(colsum_ws_floats(SR, Hi));
    w.cs_oah = take(colsum_ws_floats(SR, Hi));
    w.cs_in = take(colsum_ws_floats(SR, Hi));
    w.cs_out = take(colsum_ws_floats(SR, Hi));
  }
  w.floats = c - base;
  return w;
}

int sr_check_shape(const hiprec_srgnn_shape* s) {
  HIPREC_REQUIRE(s, "NULL shape");
  HIPREC_REQUIRE(s->n_node >= 2 && s->n_node < (1ll << 31), "SR-GNN needs 2 <= n_node < 2^31 (the padding id is counted), got %lld",
                 static_cast<long long>(s->n_node));
  HIPREC_REQUIRE(s->hidden >= 1 && s->hidden <= kSrgnnMaxHidden, "SR-GNN needs 1 <= hidden_size <= %d (got %d)",
                 kSrgnnMaxHidden, s->hidden);
  HIPREC_REQUIRE(s->step >= 1 && s->step <= kSrgnnMaxStep, "SR-GNN needs 1 <= step <= %d (got %d)", kSrgnnMaxStep,
                 s->step);
  return 0;
}

bool sr_batch_ok(int64_t B, int T, int64_t R) {
  return B >= 1 && B <= kSrgnnMaxBatch && T >= 1 && T <= kSrgnnMaxLen && R >= 1 && R <= B * T;
}

int sr_build_graph(const hiprec_srgnn_shape& s, const int64_t* seq, const int64_t* lens, int64_t B, int T, int64_t R,
                   const SrGraph& g, hiprec_stats* stats, hipStream_t st) {
  srgnn_count_kernel<<<static_cast<int>(B), kBlock, 0, st>>>(seq, lens, B, T, R, s.n_node, g, stats);
  HIPREC_TRY(hipGetLastError());
  srgnn_graph_kernel<<<static_cast<int>(B), kBlock, 0, st>>>(seq, lens, B, T, R, s.n_node, g, stats);
  HIPREC_TRY(hipGetLastError());
  return 0;
}

GemmProblem sr_gemm(int mode, int64_t M, int N, int64_t K, const float* A, int lda, const float* Bm, int ldb, float* C,
                    int ldc, const float* bias) {
  return make_gemm(mode, static_cast<int>(M), N, static_cast<int>(K), A, lda, Bm, ldb, C, ldc, bias, 0, nullptr, 0, false);
}

// a column sum that always takes the two-level fixed-order form (make_colsum drops the workspace of a single slab: the
// number of launches would then depend on the batch)
GemmProblem sr_colsum(const float* X, int64_t M, int N, int ldx, float* out, float* ws) {
  GemmProblem q = make_colsum(X, static_cast<int>(M), N, ldx, out, ws);
  q.ws = ws;
  return q;
}

int sr_run(const hiprec_srgnn_shape& s, float* w_flat, float* g_flat, const int64_t* seq, const int64_t* lens,
           const int64_t* target, int64_t B, int T, int64_t R, float l2, float* query_out, hiprec_stats* stats,
           Scratch* scratch, float* ws_base, hipStream_t st) {
  const int H = s.hidden, S = s.step;
  const int64_t I = s.n_node - 1, RH = R * H;
  const int Ii = static_cast<int>(I);
  const bool train = g_flat != nullptr, hybrid = !s.nonhybrid;
  const SrParams w = sr_params(w_flat, s);
  const SrWorkspace a = sr_carve(ws_base, s, B, T, R, train);
  const SrGraph& gr = a.graph;
  const int node_waves = grid_for_waves(R), node_threads = grid_for_threads(RH);

  if (int rc = sr_build_graph(s, seq, lens, B, T, R, gr, stats, st)) return rc;
  srgnn_embed_kernel<<<node_threads, kBlock, 0, st>>>(w.emb, gr, R, H, a.hs);
  HIPREC_TRY(hipGetLastError());
  for (int k = 0; k < S; ++k) {
    const float* h = a.hs + k * RH;
    float* P = a.P + k * RH * 5;
    float* A = a.A + k * RH * 2;
    float* G = a.G + k * RH * 3;
    GemmGroup q{};
    q.n = 3;
    q.p[0] = sr_gemm(kNT, R, H, H, h, H, w.w_in, H, P, 5 * H, w.b_in);
    q.p[1] = sr_gemm(kNT, R, H, H, h, H, w.w_out, H, P + H, 5 * H, w.b_out);
    q.p[2] = sr_gemm(kNT, R, 3 * H, H, h, H, w.w_hh, H, P + 2 * H, 5 * H, w.b_hh);
    if (int rc = launch_group(q, st)) return rc;
    srgnn_mean_fwd_kernel<<<node_waves, kBlock, 0, st>>>(P, w.b_iah, w.b_oah, gr, R, H, A);
    HIPREC_TRY(hipGetLastError());
    GemmGroup q2{};
    q2.n = 1;
    q2.p[0] = sr_gemm(kNT, R, 3 * H, 2 * H, A, 2 * H, w.w_ih, 2 * H, G, 3 * H, w.b_ih);
    if (int rc = launch_group(q2, st)) return rc;
    srgnn_gate_fwd_kernel<<<node_threads, kBlock, 0, st>>>(P, h, gr, R, H, G, a.hs + (k + 1) * RH);
    HIPREC_TRY(hipGetLastError());
  }
  const float* hN = a.hs + S * RH;
  srgnn_last_kernel<<<grid_for_threads(B * H), kBlock, 0, st>>>(hN, gr, lens, B, T, H, a.cat);
  HIPREC_TRY(hipGetLastError());
  {
    GemmGroup q{};
    q.n = 2;
    q.p[0] = sr_gemm(kNT, B, H, H, a.cat + H, 2 * H, w.w1, H, a.q1, H, w.b1);
    q.p[1] = sr_gemm(kNT, R, H, H, hN, H, w.w2, H, a.q2, H, w.b2);
    if (int rc = launch_group(q, st)) return rc;
  }
  float* query = train ? a.query : query_out;
  srgnn_readout_fwd_kernel<<<grid_for_waves(B), kBlock, 0, st>>>(hN, a.q1, a.q2, w.w3, gr, lens, B, T, H, a.alpha, a.cat,
                                                                 hybrid ? nullptr : query);
  HIPREC_TRY(hipGetLastError());
  if (hybrid) {
    GemmGroup q{};
    q.n = 1;
    q.p[0] = sr_gemm(kNT, B, H, 2 * H, a.cat, 2 * H, w.wt, 2 * H, query, H, w.bt);
    if (int rc = launch_group(q, st)) return rc;
  }
  if (!train) return 0;

  const SrParams g = sr_params(g_flat, s);
  {
    GemmGroup q{};
    q.n = 1;
    q.p[0] = sr_gemm(kNT, B, Ii, H, query, H, w.emb + H, H, a.scores, Ii, nullptr);
    if (int rc = launch_group(q, st)) return rc;
  }
  srgnn_ce_kernel<<<static_cast<int>(std::min<int64_t>(B, kMaxBlocks)), kBlock, 0, st>>>(a.scores, target, B, I, scratch,
                                                                                         stats);
  HIPREC_TRY(hipGetLastError());
  {
    int n_slices, k_per;
    sr_slices(I, &n_slices, &k_per);
    GemmGroup q{};
    q.n = n_slices;
    for (int z = 0; z < n_slices; ++z) {
      const int64_t k0 = static_cast<int64_t>(z) * k_per;
      q.p[z] = sr_gemm(kNN, B, H, std::min<int64_t>(k_per, I - k0), a.scores + k0, Ii, w.emb + H + k0 * H, H,
                       a.part + z * B * H, H, nullptr);
    }
    if (int rc = launch_group(q, st)) return rc;
    srgnn_slice_sum_kernel<<<grid_for_threads(B * H), kBlock, 0, st>>>(a.part, n_slices, B * H, a.da);
    HIPREC_TRY(hipGetLastError());
  }
  {
    // d embedding[1:] is WRITTEN here (row 0 stays 0); the node rows' atomics come last
    GemmGroup q{};
    int n = 0;
    q.p[n++] = sr_gemm(kTNm, I, H, B, a.scores, Ii, query, H, g.emb + H, H, nullptr);
    if (hybrid) {
      q.p[n++] = sr_gemm(kNN, B, 2 * H, H, a.da, H, w.wt, 2 * H, a.dcat, 2 * H, nullptr);
      q.p[n++] = sr_gemm(kTNm, H, 2 * H, B, a.da, H, a.cat, 2 * H, g.wt, 2 * H, nullptr);
      q.p[n++] = sr_colsum(a.da, B, H, H, g.bt, a.cs_t);
    }
    q.n = n;
    if (int rc = launch_group(q, st)) return rc;
    if (int rc = launch_colsum_reduce(q, st)) return rc;
  }
  HIPREC_TRY(hipMemsetAsync(a.dq2, 0, sizeof(float) * RH, st));
  HIPREC_TRY(hipMemsetAsync(a.dpi, 0, sizeof(float) * RH, st));
  srgnn_readout_bwd_kernel<<<grid_for_waves(B), kBlock, 0, st>>>(hN, a.q1, a.q2, w.w3, a.alpha, hybrid ? a.dcat : a.da,
                                                                 hybrid ? 2 * H : H, hybrid ? 1 : 0, gr, lens, B, T, H,
                                                                 a.dq2, a.dpi, a.dq1, a.vs, a.dhT);
  HIPREC_TRY(hipGetLastError());
  {
    GemmGroup q{};
    q.n = 7;
    q.p[0] = sr_gemm(kNN, B, H, H, a.dq1, H, w.w1, H, a.dhT2, H, nullptr);
    q.p[1] = sr_gemm(kNN, R, H, H, a.dq2, H, w.w2, H, a.dpo, H, nullptr);
    q.p[2] = sr_gemm(kTNm, H, H, B, a.dq1, H, a.cat + H, 2 * H, g.w1, H, nullptr);
    q.p[3] = sr_gemm(kTNm, H, H, R, a.dq2, H, hN, H, g.w2, H, nullptr);
    q.p[4] = sr_colsum(a.dq1, B, H, H, g.b1, a.cs_1);
    q.p[5] = sr_colsum(a.dq2, R, H, H, g.b2, a.cs_2);
    q.p[6] = sr_colsum(a.vs, B, H, H, g.w3, a.cs_3);
    if (int rc = launch_group(q, st)) return rc;
    if (int rc = launch_colsum_reduce(q, st)) return rc;
  }
  // the last repetition receives the readout's terms, the others what the repetition behind them left
  SrGradIn in{{a.dpi, a.dpo, nullptr, nullptr}, a.dhT, a.dhT2};
  for (int k = S - 1; k >= 0; --k) {
    const float* h = a.hs + k * RH;
    float* P = a.P + k * RH * 5;
    float* G = a.G + k * RH * 3;
    float* dA = a.dA + k * RH * 2;
    srgnn_gate_bwd_kernel<<<node_threads, kBlock, 0, st>>>(in, h, gr, lens, B, T, R, H, G, P, a.dhc);
    HIPREC_TRY(hipGetLastError());
    GemmGroup q{};
    q.n = 2;
    q.p[0] = sr_gemm(kNN, R, 2 * H, 3 * H, G, 3 * H, w.w_ih, 2 * H, dA, 2 * H, nullptr);
    q.p[1] = sr_gemm(kNN, R, H, 3 * H, P + 2 * H, 5 * H, w.w_hh, H, a.dhg, H, nullptr);
    if (int rc = launch_group(q, st)) return rc;
    srgnn_mean_bwd_kernel<<<node_waves, kBlock, 0, st>>>(dA, gr, R, H, P);
    HIPREC_TRY(hipGetLastError());
    GemmGroup q2{};
    q2.n = 2;
    q2.p[0] = sr_gemm(kNN, R, H, H, P, 5 * H, w.w_in, H, a.dpi, H, nullptr);
    q2.p[1] = sr_gemm(kNN, R, H, H, P + H, 5 * H, w.w_out, H, a.dpo, H, nullptr);
    if (int rc = launch_group(q2, st)) return rc;
    in = SrGradIn{{a.dhc, a.dhg, a.dpi, a.dpo}, nullptr, nullptr};
  }
  {
    // every weight and bias gradient of the cell: the rows of all repetitions at once.  P now holds [dP_in | dP_out |
    // dGh], G holds dGi
    const int64_t SR = static_cast<int64_t>(S) * R;
    GemmGroup q{};
    q.n = 10;
    q.p[0] = sr_gemm(kTNm, 3 * H, 2 * H, SR, a.G, 3 * H, a.A, 2 * H, g.w_ih, 2 * H, nullptr);
    q.p[1] = sr_gemm(kTNm, 3 * H, H, SR, a.P + 2 * H, 5 * H, a.hs, H, g.w_hh, H, nullptr);
    q.p[2] = sr_gemm(kTNm, H, H, SR, a.P, 5 * H, a.hs, H, g.w_in, H, nullptr);
    q.p[3] = sr_gemm(kTNm, H, H, SR, a.P + H, 5 * H, a.hs, H, g.w_out, H, nullptr);
    q.p[4] = sr_colsum(a.G, SR, 3 * H, 3 * H, g.b_ih, a.cs_ih);
    q.p[5] = sr_colsum(a.P + 2 * H, SR, 3 * H, 5 * H, g.b_hh, a.cs_hh);
    q.p[6] = sr_colsum(a.dA, SR, H, 2 * H, g.b_iah, a.cs_iah);
    q.p[7] = sr_colsum(a.dA + H, SR, H, 2 * H, g.b_oah, a.cs_oah);
    q.p[8] = sr_colsum(a.P, SR, H, 5 * H, g.b_in, a.cs_in);
    q.p[9] = sr_colsum(a.P + H, SR, H, 5 * H, g.b_out, a.cs_out);
    if (int rc = launch_group(q, st)) return rc;
    if (int rc = launch_colsum_reduce(q, st)) return rc;
  }
  srgnn_embed_bwd_kernel<<<node_threads, kBlock, 0, st>>>(in, gr, R, H, g.emb);
  HIPREC_TRY(hipGetLastError());
  if (l2 != 0.f) {
    const int64_t n = sr_n_params(s);
    srgnn_l2_kernel<<<grid_for_threads(n), kBlock, 0, st>>>(w_flat, g_flat, n, l2);
    HIPREC_TRY(hipGetLastError());
  }
  return 0;
}

}  // namespace
}  // namespace hiprec

using namespace hiprec;

extern "C" size_t hiprec_srgnn_shape_bytes(void) { return sizeof(hiprec_srgnn_shape); }

extern "C" int64_t hiprec_srgnn_param_floats(const hiprec_srgnn_shape* shape) {
  if (sr_check_shape(shape)) return -1;
  return sr_n_params(*shape);
}

extern "C" size_t hiprec_srgnn_workspace_bytes(const hiprec_srgnn_shape* shape, int64_t batch, int32_t seq_len,
                                               int64_t n_rows) {
  if (sr_check_shape(shape)) return 0;
  if (n_rows == 0) n_rows = batch * seq_len;
  if (!sr_batch_ok(batch, seq_len, n_rows)) return 0;
  return sizeof(float) * static_cast<size_t>(sr_carve(nullptr, *shape, batch, seq_len, n_rows, true).floats);
}

extern "C" int64_t hiprec_srgnn_graph_ints(int64_t batch, int32_t seq_len, int64_t n_rows) {
  if (!sr_batch_ok(batch, seq_len, n_rows)) return 0;
  return sr_graph_carve(nullptr, batch, seq_len, n_rows).ints;
}

extern "C" int hiprec_srgnn_graph(const hiprec_srgnn_shape* shape, const int64_t* seq, const int64_t* lens,
                                  int64_t batch, int32_t seq_len, int64_t n_rows, int32_t* out, size_t out_bytes,
                                  hiprec_stats* stats, void* stream) {
  if (int rc = sr_check_shape(shape)) return rc;
  HIPREC_REQUIRE(seq && lens && out && stats, "NULL pointer");
  HIPREC_REQUIRE(sr_batch_ok(batch, seq_len, n_rows), "SR-GNN needs a batch in 1..%d, a length in 1..%d and 1 <= n_rows <= batch x length",
                 kSrgnnMaxBatch, kSrgnnMaxLen);
  const SrGraph g = sr_graph_carve(out, batch, seq_len, n_rows);
  HIPREC_REQUIRE(out_bytes >= sizeof(int32_t) * static_cast<size_t>(g.ints), "graph buffer %zu B < %zu B", out_bytes,
                 sizeof(int32_t) * static_cast<size_t>(g.ints));
  return sr_build_graph(*shape, seq, lens, batch, seq_len, n_rows, g, stats, static_cast<hipStream_t>(stream));
}

extern "C" int hiprec_srgnn_grad(const hiprec_srgnn_shape* shape, const float* w_flat, float* g_flat, const int64_t* seq,
                                 const int64_t* lens, const int64_t* target, int64_t batch, int32_t seq_len,
                                 int64_t n_rows, float l2, float* query_out, hiprec_stats* stats, void* scratch,
                                 size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = sr_check_shape(shape)) return rc;
  HIPREC_REQUIRE(w_flat && seq && lens && stats && workspace, "NULL pointer");
  if (n_rows == 0) n_rows = batch * seq_len;
  HIPREC_REQUIRE(sr_batch_ok(batch, seq_len, n_rows), "SR-GNN needs a batch in 1..%d, a length in 1..%d and 1 <= n_rows <= batch x length",
                 kSrgnnMaxBatch, kSrgnnMaxLen);
  if (g_flat) {
    HIPREC_REQUIRE(target && scratch, "training needs the targets and the scratch block");
    if (scratch_bytes < kScratchBytes) {
      set_error("scratch %zu B < %zu B", scratch_bytes, kScratchBytes);
      return HIPREC_E_SCRATCH;
    }
  } else {
    HIPREC_REQUIRE(query_out, "the forward alone needs a query buffer");
  }
  const size_t need = hiprec_srgnn_workspace_bytes(shape, batch, seq_len, n_rows);
  HIPREC_REQUIRE(workspace_bytes >= need, "workspace %zu B < %zu B", workspace_bytes, need);
  return sr_run(*shape, const_cast<float*>(w_flat), g_flat, seq, lens, target, batch, seq_len, n_rows, l2, query_out, stats,
                static_cast<Scratch*>(scratch), static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}
