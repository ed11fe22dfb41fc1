// K17: global pooling read-out.  Per graph g of a block-diagonal batch - rows [graph_ptr[g], graph_ptr[g + 1]) of y [rows, C] -
// the column sums, means, maxima and the row index of each maximum, and the backward that spreads the three gradients over
// the rows.  Permutation invariant, defined for every node count.
//
// Rules: an empty graph pools to +0.0 with argmax -1; ties of the maximum go to the LOWEST row (-0.0 == +0.0); a NaN makes its
// column's maximum NaN with argmax at the first NaN row, and its sum NaN by IEEE addition.  No atomics, no ticket counters.
//
// Summation order (fixed; a function of the graph's own rows and of C alone): the graph's rows are cut into chunks of
// R = kChunkRows rows counted from its own first row.  Inside a chunk, row-lane l of the workgroup (pool_index.h, Geometry)
// adds rows l, l + L, l + 2L, ... of the chunk in ascending order onto +0.0, and the L lane sums are folded by a halving tree
// (lane l += lane l + s for s = L/2, ..., 1).  The graph's sum is ((+0.0 + p_0) + p_1) + ... over its chunk sums in ascending
// order.  Both regimes compute exactly this, so they give the same bits, as does a graph pooled alone or inside any batch:
//   * many graphs: one workgroup per (graph, column tile) walks the graph's chunks itself;
//   * few large graphs (split): one workgroup per (chunk, column tile) writes (sum, max, argmax) partials to a workspace slot,
//     a merge launch folds each graph's slots in ascending order.
#include "gnc_common.h"
#include "pool_index.h"

#include <limits.h>

namespace {

using namespace gnc_pool;

constexpr int kT = kBlockThreads;

// (value, row) pairs under "larger value wins, NaN beats everything, the lower row wins a tie": commutative and associative, so
// the lane loop, the tree and the chunk merge may fold in any grouping.  (-inf, INT_MAX) is its identity.
__device__ __forceinline__ void fold_max(float& av, int& ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  bool take;
  if (an || bn) take = bn && (!an || bi < ai);
  else take = bv > av || (bv == av && bi < ai);
  if (take) av = bv, ai = bi;
}

struct PoolArgs {
  const float* y;
  const int64_t* graph_ptr;
  int64_t rows, C, G;
  float* psum;   // any of the four may be NULL
  float* pmean;
  float* pmax;
  int32_t* argmax;
  int64_t ld_out;
  float* ws_sum;  // split regime: [slots, C] each
  float* ws_max;
  int32_t* ws_idx;
  int64_t slots;
  int32_t col_lanes, row_lanes;  // Geometry of C
  int32_t y16;                   // y is 16-byte aligned (vec 4: one dwordx4 load per row and thread)
};

template <int VEC>
__device__ __forceinline__ void load_cols(const float* __restrict__ p, bool y16, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    if (y16) {
      const float4 q = *reinterpret_cast<const float4*>(p);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
      return;
    }
  }
#pragma unroll
  for (int u = 0; u < VEC; ++u) v[u] = p[u];
}

// Sum / max / argmax of rows [row0, row0 + nr) of the workgroup's column tile; the result is in the threads of row-lane 0.
// Every thread of the workgroup calls it (it synchronises); a thread whose columns lie behind C contributes identities.
template <int VEC>
__device__ __forceinline__ void chunk_reduce(const PoolArgs& a, int64_t row0, int nr, int64_t col0, bool active, int rl,
                                             float (&s_sum)[VEC][kT], float (&s_max)[VEC][kT], int (&s_idx)[VEC][kT],
                                             float (&sum)[VEC], float (&mx)[VEC], int (&ix)[VEC]) {
  const int t = threadIdx.x;
  const int L = a.row_lanes, CL = a.col_lanes;
#pragma unroll
  for (int u = 0; u < VEC; ++u) sum[u] = 0.f, mx[u] = -INFINITY, ix[u] = INT_MAX;
  if (active) {
    const float* __restrict__ base = a.y + row0 * a.C + col0;
#pragma unroll 4
    for (int r = rl; r < nr; r += L) {
      float v[VEC];
      load_cols<VEC>(base + (int64_t)r * a.C, a.y16 != 0, v);
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        sum[u] += v[u];
        fold_max(mx[u], ix[u], v[u], (int)(row0 + r));
      }
    }
  }
  __syncthreads();  // the previous chunk's tree has been read
#pragma unroll
  for (int u = 0; u < VEC; ++u) s_sum[u][t] = sum[u], s_max[u][t] = mx[u], s_idx[u][t] = ix[u];
  for (int s = L >> 1; s >= 1; s >>= 1) {
    __syncthreads();
    if (rl < s) {
      const int o = t + s * CL;  // row-lane rl + s, same columns
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        sum[u] += s_sum[u][o];
        fold_max(mx[u], ix[u], s_max[u][o], s_idx[u][o]);
        s_sum[u][t] = sum[u], s_max[u][t] = mx[u], s_idx[u][t] = ix[u];
      }
    }
  }
}

// the four outputs of (graph g, column c) from the folded chunk results
__device__ __forceinline__ void store_pooled(const PoolArgs& a, int64_t g, int64_t c, int64_t n, float sum, float mx, int ix) {
  const int64_t o = g * a.ld_out + c;
  if (a.psum) a.psum[o] = n > 0 ? sum : 0.f;
  if (a.pmean) a.pmean[o] = n > 0 ? sum / (float)n : 0.f;
  if (a.pmax) a.pmax[o] = n > 0 ? mx : 0.f;
  if (a.argmax) a.argmax[g * a.C + c] = n > 0 ? ix : -1;
}

// many graphs: workgroup (g, column tile)
template <int VEC>
__global__ __launch_bounds__(kT) void pool_graphs_kernel(const PoolArgs a) {
  __shared__ float s_sum[VEC][kT];
  __shared__ float s_max[VEC][kT];
  __shared__ int s_idx[VEC][kT];
  const int t = threadIdx.x, cl = t % a.col_lanes, rl = t / a.col_lanes;
  const int64_t g = blockIdx.x;
  const int64_t col0 = ((int64_t)blockIdx.y * a.col_lanes + cl) * VEC;
  const bool active = col0 < a.C;  // vec 4: C is a multiple of 4, so col0 + 3 < C as well
  int64_t ra, rb;
  graph_range(a.graph_ptr, g, a.rows, ra, rb);
  const int64_t n = rb - ra;
  float acc[VEC], amx[VEC];
  int aix[VEC];
#pragma unroll
  for (int u = 0; u < VEC; ++u) acc[u] = 0.f, amx[u] = -INFINITY, aix[u] = INT_MAX;
  for (int64_t k0 = 0; k0 < n; k0 += kChunkRows) {
    const int nr = (int)(n - k0 < kChunkRows ? n - k0 : kChunkRows);
    float sum[VEC], mx[VEC];
    int ix[VEC];
    chunk_reduce<VEC>(a, ra + k0, nr, col0, active, rl, s_sum, s_max, s_idx, sum, mx, ix);
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      acc[u] += sum[u];
      fold_max(amx[u], aix[u], mx[u], ix[u]);
    }
  }
  if (rl == 0 && active) {
#pragma unroll
    for (int u = 0; u < VEC; ++u) store_pooled(a, g, col0 + u, n, acc[u], amx[u], aix[u]);
  }
}

// split regime, first launch: workgroup (slot, column tile) -> the chunk's partials
template <int VEC>
__global__ __launch_bounds__(kT) void pool_chunks_kernel(const PoolArgs a) {
  __shared__ float s_sum[VEC][kT];
  __shared__ float s_max[VEC][kT];
  __shared__ int s_idx[VEC][kT];
  const int t = threadIdx.x, cl = t % a.col_lanes, rl = t / a.col_lanes;
  const int64_t slot = blockIdx.x;
  const int64_t col0 = ((int64_t)blockIdx.y * a.col_lanes + cl) * VEC;
  const bool active = col0 < a.C;
  int64_t g, row0;
  int nr;
  if (slot >= a.slots || !slot_chunk(a.graph_ptr, a.G, a.rows, slot, g, row0, nr)) return;  // uniform over the workgroup
  float sum[VEC], mx[VEC];
  int ix[VEC];
  chunk_reduce<VEC>(a, row0, nr, col0, active, rl, s_sum, s_max, s_idx, sum, mx, ix);
  if (rl == 0 && active) {
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      const int64_t o = slot * a.C + col0 + u;
      a.ws_sum[o] = sum[u], a.ws_max[o] = mx[u], a.ws_idx[o] = ix[u];
    }
  }
}

// split regime, second launch: thread (g, c) folds the graph's slots in ascending order
__global__ __launch_bounds__(kT) void pool_merge_kernel(const PoolArgs a) {
  const int64_t g = blockIdx.x;
  const int64_t c = (int64_t)blockIdx.y * kT + threadIdx.x;
  if (c >= a.C) return;
  int64_t ra, rb;
  graph_range(a.graph_ptr, g, a.rows, ra, rb);
  const int64_t n = rb - ra;
  const int64_t s0 = first_slot(a.graph_ptr, g, a.rows);
  int64_t s1 = s0 + chunks_of(n);
  if (s1 > a.slots) s1 = a.slots;  // offsets that overlap: only the slots that exist (and were written)
  float acc = 0.f, amx = -INFINITY;
  int aix = INT_MAX;
  for (int64_t s = s0; s < s1; ++s) {
    acc += a.ws_sum[s * a.C + c];
    fold_max(amx, aix, a.ws_max[s * a.C + c], a.ws_idx[s * a.C + c]);
  }
  store_pooled(a, g, c, n, acc, amx, aix);
}

struct PoolBwdArgs {
  const float* dsum;  // any may be NULL
  const float* dmean;
  const float* dmax;
  const int32_t* argmax;
  const int64_t* graph_ptr;
  int64_t rows, C, G, ld_grad;
  float* dy;
  int32_t dy16;
};

// backward: a streaming write of every row of dy; one item = VEC columns of one row
template <int VEC>
__global__ __launch_bounds__(kT) void pool_backward_kernel(const PoolBwdArgs a) {
  const int64_t per_row = a.C / VEC;
  const int64_t items = a.rows * per_row;
  for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < items; i += (int64_t)gridDim.x * kT) {
    const int64_t r = i / per_row, c0 = (i - r * per_row) * VEC;
    int64_t n = 0;
    const int64_t g = graph_of_row(a.graph_ptr, a.G, a.rows, r, n);
    float v[VEC];
#pragma unroll
    for (int u = 0; u < VEC; ++u) v[u] = 0.f;
    if (g >= 0) {
      const float fn = (float)n;
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        const int64_t o = g * a.ld_grad + c0 + u;
        // the first term present is taken as it is (a lone dsum reaches dy bit for bit), the others are added to it
        bool have = false;
        float x = 0.f;
        if (a.dsum) x = a.dsum[o], have = true;
        if (a.dmean) {
          const float m = a.dmean[o] / fn;
          x = have ? x + m : m, have = true;
        }
        if (a.dmax && a.argmax[g * a.C + c0 + u] == (int32_t)r) {
          const float m = a.dmax[o];
          x = have ? x + m : m;
        }
        v[u] = x;
      }
    }
    float* __restrict__ p = a.dy + r * a.C + c0;
    bool stored = false;
    if constexpr (VEC == 4) {
      if (a.dy16) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        stored = true;
      }
    }
    if (!stored) {
#pragma unroll
      for (int u = 0; u < VEC; ++u) p[u] = v[u];
    }
  }
}

bool plan_of(int64_t rows, int64_t C, int64_t G, gnc_graph_pool_plan_t* plan) {
  // row indices are int32 (argmax), the column tiles ride in gridDim.y, the graphs in gridDim.x
  if (rows < 0 || rows >= (1ll << 31) || C < 1 || C > (1ll << 20) || G < 1 || G >= (1ll << 31)) return false;
  const Geometry geo = geometry(C);
  if (geo.col_tiles > 65535) return false;
  const bool split = G * geo.col_tiles < kSplitBelowWorkgroups && rows > 2 * (int64_t)kChunkRows * G;
  if (plan) {
    plan->chunk_rows = kChunkRows;
    plan->split = split ? 1 : 0;
    plan->slots = split ? split_slots(rows, G) : 0;
    plan->vec = geo.vec, plan->col_lanes = geo.col_lanes, plan->row_lanes = geo.row_lanes, plan->col_tiles = geo.col_tiles;
    plan->workspace_floats = split ? 3 * split_slots(rows, G) * C : 0;
  }
  return true;
}

}  // namespace

extern "C" int32_t gnc_graph_pool_plan(int64_t rows, int64_t C, int64_t num_graphs, gnc_graph_pool_plan_t* plan) {
  return plan_of(rows, C, num_graphs, plan) ? 1 : 0;
}

extern "C" int gnc_graph_pool_forward_f32(const float* y, int64_t rows, int64_t C, const int64_t* graph_ptr, int64_t num_graphs,
                                          int32_t modes, float* psum, float* pmean, float* pmax, int32_t* argmax, int64_t ld_out,
                                          float* workspace, int64_t workspace_floats, void* stream) {
  gnc_graph_pool_plan_t plan;
  if (!plan_of(rows, C, num_graphs, &plan)) {
    gnc::set_error("gnc_graph_pool_forward_f32: rows %lld / C %lld / graphs %lld outside the supported set (rows < 2^31, "
                   "1 <= C <= 2^20, graphs >= 1)", (long long)rows, (long long)C, (long long)num_graphs);
    return GNC_ERR_UNSUPPORTED;
  }
  GNC_REQUIRE(modes != 0 && (modes & ~(GNC_POOL_SUM | GNC_POOL_MEAN | GNC_POOL_MAX)) == 0, "gnc_graph_pool_forward_f32: bad mode mask");
  GNC_REQUIRE(graph_ptr && (y || rows == 0), "gnc_graph_pool_forward_f32: null y / graph_ptr");
  GNC_REQUIRE(((modes & GNC_POOL_SUM) != 0) == (psum != nullptr) && ((modes & GNC_POOL_MEAN) != 0) == (pmean != nullptr) &&
                  ((modes & GNC_POOL_MAX) != 0) == (pmax != nullptr) && (pmax != nullptr) == (argmax != nullptr),
              "gnc_graph_pool_forward_f32: the outputs must be exactly those the mode mask names (argmax with max)");
  GNC_REQUIRE(ld_out >= C, "gnc_graph_pool_forward_f32: ld_out smaller than C");
  GNC_REQUIRE((reinterpret_cast<uintptr_t>(y) & 3u) == 0 && (reinterpret_cast<uintptr_t>(graph_ptr) & 7u) == 0,
              "gnc_graph_pool_forward_f32: a pointer is not aligned to its element size");
  PoolArgs a = {};
  a.y = y, a.graph_ptr = graph_ptr, a.rows = rows, a.C = C, a.G = num_graphs;
  a.psum = psum, a.pmean = pmean, a.pmax = pmax, a.argmax = argmax, a.ld_out = ld_out;
  a.col_lanes = (int32_t)plan.col_lanes, a.row_lanes = (int32_t)plan.row_lanes;
  a.y16 = gnc::aligned16(y) ? 1 : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 block(kT);
  if (!plan.split) {
    const dim3 grid((unsigned)num_graphs, (unsigned)plan.col_tiles);
    if (plan.vec == 4) pool_graphs_kernel<4><<<grid, block, 0, st>>>(a);
    else pool_graphs_kernel<1><<<grid, block, 0, st>>>(a);
    return gnc::check_launch("pool_graphs_kernel");
  }
  GNC_REQUIRE(workspace && workspace_floats >= plan.workspace_floats && (reinterpret_cast<uintptr_t>(workspace) & 3u) == 0,
              "gnc_graph_pool_forward_f32: the split regime needs a workspace of %lld floats", (long long)plan.workspace_floats);
  a.slots = plan.slots;
  a.ws_sum = workspace;
  a.ws_max = workspace + plan.slots * C;
  a.ws_idx = reinterpret_cast<int32_t*>(workspace + 2 * plan.slots * C);
  const dim3 grid((unsigned)plan.slots, (unsigned)plan.col_tiles);
  if (plan.vec == 4) pool_chunks_kernel<4><<<grid, block, 0, st>>>(a);
  else pool_chunks_kernel<1><<<grid, block, 0, st>>>(a);
  if (int rc = gnc::check_launch("pool_chunks_kernel")) return rc;
  pool_merge_kernel<<<dim3((unsigned)num_graphs, (unsigned)gnc::ceil_div(C, kT)), block, 0, st>>>(a);
  return gnc::check_launch("pool_merge_kernel");
}

extern "C" int gnc_graph_pool_backward_f32(const float* dsum, const float* dmean, const float* dmax, int64_t ld_grad,
                                           const int32_t* argmax, const int64_t* graph_ptr, int64_t num_graphs, int64_t rows, int64_t C,
                                           float* dy, void* stream) {
  if (!plan_of(rows, C, num_graphs, nullptr)) {
    gnc::set_error("gnc_graph_pool_backward_f32: rows %lld / C %lld / graphs %lld outside the supported set", (long long)rows,
                   (long long)C, (long long)num_graphs);
    return GNC_ERR_UNSUPPORTED;
  }
  GNC_REQUIRE(dsum || dmean || dmax, "gnc_graph_pool_backward_f32: no gradient given");
  GNC_REQUIRE(graph_ptr && (dy || rows == 0), "gnc_graph_pool_backward_f32: null graph_ptr / dy");
  GNC_REQUIRE(!dmax || argmax, "gnc_graph_pool_backward_f32: dmax needs argmax");
  GNC_REQUIRE(ld_grad >= C, "gnc_graph_pool_backward_f32: ld_grad smaller than C");
  GNC_REQUIRE((reinterpret_cast<uintptr_t>(dy) & 3u) == 0 && (reinterpret_cast<uintptr_t>(graph_ptr) & 7u) == 0,
              "gnc_graph_pool_backward_f32: a pointer is not aligned to its element size");
  if (rows == 0) return GNC_OK;
  PoolBwdArgs a = {};
  a.dsum = dsum, a.dmean = dmean, a.dmax = dmax, a.argmax = argmax, a.graph_ptr = graph_ptr;
  a.rows = rows, a.C = C, a.G = num_graphs, a.ld_grad = ld_grad, a.dy = dy;
  a.dy16 = gnc::aligned16(dy) ? 1 : 0;
  const int vec = C % 4 == 0 ? 4 : 1;
  int64_t blocks = gnc::ceil_div(rows * (C / vec), kT);
  const int64_t cap = 8ll * gnc::num_cu();
  blocks = blocks > cap ? cap : blocks;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec == 4) pool_backward_kernel<4><<<dim3((unsigned)blocks), dim3(kT), 0, st>>>(a);
  else pool_backward_kernel<1><<<dim3((unsigned)blocks), dim3(kT), 0, st>>>(a);
  return gnc::check_launch("pool_backward_kernel");
}
