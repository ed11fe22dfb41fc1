// The chunked per-graph reduction that K17 (csrc/pool_readout.hip) and K19 (csrc/attention_pool.hip) share, and the vector row
// load / store that K20 (csrc/topk_pool.hip) uses with them.  Device code; the index arithmetic it calls is pool_index.h's.
//
// Summation order (fixed; a function of the graph's own rows and of C alone, and defined HERE, once): the graph's rows are cut
// into chunks of R = kChunkRows rows counted from its own first row.  Inside a chunk, row-lane l of the workgroup (pool_index.h,
// Geometry) enters rows l, l + L, l + 2L, ... of the chunk in ascending order into the operation's identity, and the L lane
// partials are folded by a halving tree (lane l takes lane l + s for s = L/2, ..., 1) - chunk_reduce.  The graph's result is
// ((identity + p_0) + p_1) + ... over its chunk partials in ascending order.  Both regimes compute exactly this, so they give the
// same bits, as does a graph reduced alone or inside any batch:
//   * many graphs: one workgroup per (graph, column tile) walks the graph's chunks itself - reduce_graph;
//   * few large graphs (split): one workgroup per (chunk, column tile) writes its partial to a workspace slot - reduce_slot -
//     and a merge launch folds each graph's slots in ascending order - merge_graph.
// No atomics, no ticket counters; the regime comes from gnc_graph_pool_plan (rows, C, G alone).
//
// What is reduced is an operation type Op<VEC> over the kernel's arguments:
//   Partial, identity()    what a thread carries for its VEC columns (K17: sum, max, argmax; K19: weighted sum and Z), and of no rows
//   Shared, park(sh, t, p), parked(sh, t)    the LDS the tree parks kBlockThreads partials in
//   graph_begin(g, a, b, sh), slot_begin(g)  what the operation needs of graph g before its first row in the graph-owned and the
//                          slot-owned body (K19: the score maximum); every thread of the workgroup calls it
//   row(p, row, v)         enter row `row`, whose VEC columns are v, into p
//   fold(p, q)             p = p (+) q, q being the LATER rows
//   store(g, n, col0, p)   the outputs of graph g (n rows) for the columns from col0, from the folded partial
//   store_slot(slot, col0, p), slot_partial(slot, c)   the workspace (the merge runs the VEC = 1 operation, one column per thread)
#pragma once
#include "gnc_common.h"
#include "pool_index.h"

namespace gnc_reduce {

using namespace gnc_pool;

constexpr int kT = kBlockThreads;

// VEC consecutive floats of a row: one 16-byte access when VEC is 4 and the caller vouches for the alignment, scalars otherwise.
template <int VEC>
__device__ __forceinline__ void load_vec(const float* __restrict__ p, bool p16, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    if (p16) {
      const float4 q = *reinterpret_cast<const float4*>(p);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
      return;
    }
  }
#pragma unroll
  for (int u = 0; u < VEC; ++u) v[u] = p[u];
}

template <int VEC>
__device__ __forceinline__ void store_vec(float* __restrict__ p, bool p16, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    if (p16) {
      *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
      return;
    }
  }
#pragma unroll
  for (int u = 0; u < VEC; ++u) p[u] = v[u];
}

// The arguments every reduction has; an operation's argument struct derives from it.
struct ReduceArgs {
  const float* y;  // [rows, C]
  const int64_t* graph_ptr;
  int64_t rows, C, G;
  int64_t slots;                 // split regime
  int32_t col_lanes, row_lanes;  // Geometry of C
  int32_t y16;                   // y is 16-byte aligned (vec 4: one dwordx4 load per row and thread)
  __host__ __device__ Geometry geometry(int vec) const { return Geometry{vec, col_lanes, row_lanes, 0}; }
};

// The partial of rows [row0, row0 + nr) of the workgroup's column tile; the result is in the threads of row-lane 0.  Every thread
// of the workgroup calls it (it synchronises); a thread whose columns lie behind C contributes the identity.
template <int VEC, class Op>
__device__ __forceinline__ typename Op::Partial chunk_reduce(const ReduceArgs& a, const Op& op, typename Op::Shared& sh, int64_t row0,
                                                             int nr, const Tile& x) {
  const int t = threadIdx.x;
  const Geometry geo = a.geometry(VEC);
  typename Op::Partial p = op.identity();
  if (x.col0 < a.C) {
    const float* __restrict__ base = a.y + row0 * a.C + x.col0;
#pragma unroll 4
    for (int r = x.rl; r < nr; r += geo.row_lanes) {
      float v[VEC];
      load_vec<VEC>(base + (int64_t)r * a.C, a.y16 != 0, v);
      op.row(p, row0 + r, v);
    }
  }
  __syncthreads();  // the previous chunk's tree has been read
  op.park(sh, t, p);
  for (int s = geo.row_lanes >> 1; s >= 1; s >>= 1) {
    __syncthreads();
    if (x.rl < s) {
      op.fold(p, op.parked(sh, tree_partner(t, s, geo)));
      op.park(sh, t, p);
    }
  }
  return p;
}

// many graphs: workgroup (g, column tile)
template <int VEC, class Op>
__device__ __forceinline__ void reduce_graph(const ReduceArgs& a, Op& op, typename Op::Shared& sh) {
  const Tile x = tile_of(threadIdx.x, blockIdx.y, a.geometry(VEC));
  const int64_t g = blockIdx.x;
  int64_t ra, rb;
  graph_range(a.graph_ptr, g, a.rows, ra, rb);
  const int64_t n = rb - ra;
  op.graph_begin(g, ra, rb, sh);
  typename Op::Partial acc = op.identity();
  for (int64_t k0 = 0; k0 < n; k0 += kChunkRows) op.fold(acc, chunk_reduce<VEC>(a, op, sh, ra + k0, chunk_len(n, k0), x));
  if (x.rl == 0 && x.col0 < a.C) op.store(g, n, x.col0, acc);
}

// split regime: workgroup (slot, column tile) -> the chunk's partial
template <int VEC, class Op>
__device__ __forceinline__ void reduce_slot(const ReduceArgs& a, Op& op, typename Op::Shared& sh) {
  const Tile x = tile_of(threadIdx.x, blockIdx.y, a.geometry(VEC));
  const int64_t slot = blockIdx.x;
  int64_t g, row0;
  int nr;
  if (slot >= a.slots || !slot_chunk(a.graph_ptr, a.G, a.rows, slot, g, row0, nr)) return;  // uniform over the workgroup
  op.slot_begin(g);
  const typename Op::Partial p = chunk_reduce<VEC>(a, op, sh, row0, nr, x);
  if (x.rl == 0 && x.col0 < a.C) op.store_slot(slot, x.col0, p);
}

// split regime, last launch: thread (g, c) folds the graph's slots in ascending order; Op is the VEC = 1 operation
template <class Op>
__device__ __forceinline__ void merge_graph(const ReduceArgs& a, const Op& op) {
  const int64_t g = blockIdx.x;
  const int64_t c = (int64_t)blockIdx.y * kT + threadIdx.x;
  if (c >= a.C) return;
  int64_t n, s0, s1;
  merge_slots(a.graph_ptr, g, a.rows, a.slots, n, s0, s1);
  typename Op::Partial acc = op.identity();
  for (int64_t s = s0; s < s1; ++s) op.fold(acc, op.slot_partial(s, c));
  op.store(g, n, c, acc);
}

// The five forward kernels of an operation and the two launch sequences; `Args` derives from ReduceArgs.
template <class Args>
struct ReduceKernels {
  void (*graphs1)(Args), (*graphs4)(Args), (*chunks1)(Args), (*chunks4)(Args), (*merge)(Args);
  const char *graphs_name, *chunks_name, *merge_name;
};

template <class Args>
int launch_graph_owned(const ReduceKernels<Args>& k, const Args& a, const gnc_graph_pool_plan_t& plan, hipStream_t st) {
  const dim3 grid((unsigned)a.G, (unsigned)plan.col_tiles);
  (plan.vec == 4 ? k.graphs4 : k.graphs1)<<<grid, dim3(kT), 0, st>>>(a);
  return gnc::check_launch(k.graphs_name);
}

// (a.slots and the operation's workspace pointers are set)
template <class Args>
int launch_split(const ReduceKernels<Args>& k, const Args& a, const gnc_graph_pool_plan_t& plan, hipStream_t st) {
  const dim3 grid((unsigned)plan.slots, (unsigned)plan.col_tiles);
  (plan.vec == 4 ? k.chunks4 : k.chunks1)<<<grid, dim3(kT), 0, st>>>(a);
  if (int rc = gnc::check_launch(k.chunks_name)) return rc;
  k.merge<<<dim3((unsigned)a.G, (unsigned)gnc::ceil_div(a.C, kT)), dim3(kT), 0, st>>>(a);
  return gnc::check_launch(k.merge_name);
}

}  // namespace gnc_reduce
