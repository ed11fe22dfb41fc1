// K17: global pooling read-out.  Per graph g of a block-diagonal batch - rows [graph_ptr[g], graph_ptr[g + 1]) of y [rows, C] -
// the column sums, means, maxima and the row index of each maximum, and the backward that spreads the three gradients over
// the rows.  Permutation invariant, defined for every node count.
//
// Rules: an empty graph pools to +0.0 with argmax -1; ties of the maximum go to the LOWEST row (-0.0 == +0.0); a NaN makes its
// column's maximum NaN with argmax at the first NaN row, and its sum NaN by IEEE addition.  No atomics, no ticket counters.
//
// The forward is the chunked per-graph reduction of csrc/graph_reduce.h - the summation order is defined there, for both regimes -
// carrying (sum, max, argmax) per column: PoolOp below.  In the split regime the workspace holds the chunks' partials as three
// [slots, C] tables.
#include "graph_reduce.h"

#include <limits.h>

namespace {

using namespace gnc_reduce;

// (value, row) pairs under "larger value wins, NaN beats everything, the lower row wins a tie": commutative and associative, so
// the lane loop, the tree and the chunk merge may fold in any grouping.  (-inf, INT_MAX) is its identity.
__device__ __forceinline__ void fold_max(float& av, int& ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  bool take;
  if (an || bn) take = bn && (!an || bi < ai);
  else take = bv > av || (bv == av && bi < ai);
  if (take) av = bv, ai = bi;
}

struct PoolArgs : ReduceArgs {
  float* psum;  // any of the four may be NULL
  float* pmean;
  float* pmax;
  int32_t* argmax;
  int64_t ld_out;
  float* ws_sum;  // split regime: [slots, C] each
  float* ws_max;
  int32_t* ws_idx;
};

// K17's operation (graph_reduce.h): the sum and the fold_max pair of every column
template <int VEC>
struct PoolOp {
  const PoolArgs& a;
  struct Partial {
    float sum[VEC], mx[VEC];
    int ix[VEC];
  };
  struct Shared {
    float sum[VEC][kT], mx[VEC][kT];
    int ix[VEC][kT];
  };
  __device__ __forceinline__ Partial identity() const {
    Partial p;
#pragma unroll
    for (int u = 0; u < VEC; ++u) p.sum[u] = 0.f, p.mx[u] = -INFINITY, p.ix[u] = INT_MAX;
    return p;
  }
  __device__ __forceinline__ void graph_begin(int64_t, int64_t, int64_t, Shared&) {}
  __device__ __forceinline__ void slot_begin(int64_t) {}
  __device__ __forceinline__ void row(Partial& p, int64_t row, const float (&v)[VEC]) const {
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      p.sum[u] += v[u];
      fold_max(p.mx[u], p.ix[u], v[u], (int)row);
    }
  }
  __device__ __forceinline__ void fold(Partial& p, const Partial& q) const {
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      p.sum[u] += q.sum[u];
      fold_max(p.mx[u], p.ix[u], q.mx[u], q.ix[u]);
    }
  }
  __device__ __forceinline__ void park(Shared& sh, int t, const Partial& p) const {
#pragma unroll
    for (int u = 0; u < VEC; ++u) sh.sum[u][t] = p.sum[u], sh.mx[u][t] = p.mx[u], sh.ix[u][t] = p.ix[u];
  }
  __device__ __forceinline__ Partial parked(const Shared& sh, int t) const {
    Partial p;
#pragma unroll
    for (int u = 0; u < VEC; ++u) p.sum[u] = sh.sum[u][t], p.mx[u] = sh.mx[u][t], p.ix[u] = sh.ix[u][t];
    return p;
  }
  // the four outputs of (graph g, columns col0 ...) from the folded chunk results
  __device__ __forceinline__ void store(int64_t g, int64_t n, int64_t col0, const Partial& p) const {
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      const int64_t o = g * a.ld_out + col0 + u;
      if (a.psum) a.psum[o] = n > 0 ? p.sum[u] : 0.f;
      if (a.pmean) a.pmean[o] = n > 0 ? p.sum[u] / (float)n : 0.f;
      if (a.pmax) a.pmax[o] = n > 0 ? p.mx[u] : 0.f;
      if (a.argmax) a.argmax[g * a.C + col0 + u] = n > 0 ? p.ix[u] : -1;
    }
  }
  __device__ __forceinline__ void store_slot(int64_t slot, int64_t col0, const Partial& p) const {
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      const int64_t o = slot * a.C + col0 + u;
      a.ws_sum[o] = p.sum[u], a.ws_max[o] = p.mx[u], a.ws_idx[o] = p.ix[u];
    }
  }
  __device__ __forceinline__ Partial slot_partial(int64_t slot, int64_t c) const {
    const int64_t o = slot * a.C + c;
    return Partial{{a.ws_sum[o]}, {a.ws_max[o]}, {a.ws_idx[o]}};
  }
};

template <int VEC>
__global__ __launch_bounds__(kT) void pool_graphs_kernel(const PoolArgs a) {
  __shared__ typename PoolOp<VEC>::Shared sh;
  PoolOp<VEC> op{a};
  reduce_graph<VEC>(a, op, sh);
}

template <int VEC>
__global__ __launch_bounds__(kT) void pool_chunks_kernel(const PoolArgs a) {
  __shared__ typename PoolOp<VEC>::Shared sh;
  PoolOp<VEC> op{a};
  reduce_slot<VEC>(a, op, sh);
}

__global__ __launch_bounds__(kT) void pool_merge_kernel(const PoolArgs a) { merge_graph(a, PoolOp<1>{a}); }

const ReduceKernels<PoolArgs> kPoolKernels = {pool_graphs_kernel<1>, pool_graphs_kernel<4>, pool_chunks_kernel<1>, pool_chunks_kernel<4>,
                                              pool_merge_kernel,     "pool_graphs_kernel",  "pool_chunks_kernel",  "pool_merge_kernel"};

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
    int64_t r, c0;
    backward_item(i, per_row, VEC, r, c0);
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
  GNC_REQUIRE(gnc::aligned_to(y, 4) && gnc::aligned_to(graph_ptr, 8), "gnc_graph_pool_forward_f32: a pointer is not aligned to its element size");
  PoolArgs a = {};
  a.y = y, a.graph_ptr = graph_ptr, a.rows = rows, a.C = C, a.G = num_graphs;
  a.psum = psum, a.pmean = pmean, a.pmax = pmax, a.argmax = argmax, a.ld_out = ld_out;
  a.col_lanes = (int32_t)plan.col_lanes, a.row_lanes = (int32_t)plan.row_lanes;
  a.y16 = gnc::aligned16(y) ? 1 : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!plan.split) return launch_graph_owned(kPoolKernels, a, plan, st);
  GNC_REQUIRE(workspace && workspace_floats >= plan.workspace_floats && gnc::aligned_to(workspace, 4),
              "gnc_graph_pool_forward_f32: the split regime needs a workspace of %lld floats", (long long)plan.workspace_floats);
  a.slots = plan.slots;
  a.ws_sum = workspace;
  a.ws_max = workspace + plan.slots * C;
  a.ws_idx = reinterpret_cast<int32_t*>(workspace + 2 * plan.slots * C);
  return launch_split(kPoolKernels, a, plan, st);
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
  GNC_REQUIRE(gnc::aligned_to(dy, 4) && gnc::aligned_to(graph_ptr, 8), "gnc_graph_pool_backward_f32: a pointer is not aligned to its element size");
  if (rows == 0) return GNC_OK;
  PoolBwdArgs a = {};
  a.dsum = dsum, a.dmean = dmean, a.dmax = dmax, a.argmax = argmax, a.graph_ptr = graph_ptr;
  a.rows = rows, a.C = C, a.G = num_graphs, a.ld_grad = ld_grad, a.dy = dy;
  a.dy16 = gnc::aligned16(dy) ? 1 : 0;
  const int vec = C % 4 == 0 ? 4 : 1;
  const int64_t blocks = gnc::capped_blocks(rows * (C / vec), kT);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec == 4) pool_backward_kernel<4><<<dim3((unsigned)blocks), dim3(kT), 0, st>>>(a);
  else pool_backward_kernel<1><<<dim3((unsigned)blocks), dim3(kT), 0, st>>>(a);
  return gnc::check_launch("pool_backward_kernel");
}
