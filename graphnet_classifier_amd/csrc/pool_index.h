// Index arithmetic of the per-graph pooling kernels (K17 csrc/pool_readout.hip, K19 csrc/attention_pool.hip through
// csrc/graph_reduce.h, the row tiling of K20 csrc/topk_pool.hip), kept apart from the kernels so that the same functions compile
// for the host: the plan (gnc_graph_pool_plan) calls them there, and the host programs over tools/pool_walk.h walk every
// (workgroup, thread) of a launch through the very functions the kernels call and check each address against the buffers before
// a kernel ever runs on a device.  Nothing here touches memory except `graph_ptr`.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GNC_POOL_HD __host__ __device__ __forceinline__
#else
#define GNC_POOL_HD inline
#endif

namespace gnc_pool {

constexpr int kBlockThreads = 256;
// Rows per chunk.  A graph's sum is ((0 + p_0) + p_1) + ... over the partial sums p_k of its chunks [k R, (k + 1) R), counted
// from the graph's OWN first row; 128 rows give one 16,384-row graph 128 workgroups in the split regime, and a superpixel
// graph (~100-150 rows) one or two chunks.
constexpr int kChunkRows = 128;
// The split regime is taken when the graph-owned grid would leave CUs idle (fewer workgroups than an MI355X has CUs) and the
// graphs average more than two chunks each; both from host-known sizes only.
constexpr int kSplitBelowWorkgroups = 256;

// How the 256 threads of a workgroup tile [rows] x [columns]: `vec` consecutive columns per thread (4 = one 16-byte load, when C
// is a multiple of 4), `col_lanes` threads side by side along a row (a power of two), `row_lanes` = 256 / col_lanes rows in
// flight, `col_tiles` workgroups along C.  A function of C ALONE: it fixes the summation order.
struct Geometry {
  int vec, col_lanes, row_lanes, col_tiles;
};

GNC_POOL_HD Geometry geometry(int64_t C) {
  Geometry g;
  g.vec = (C % 4 == 0) ? 4 : 1;
  const int64_t per_row = (C + g.vec - 1) / g.vec;  // threads one row needs
  const int cap = g.vec == 4 ? 32 : 64;             // 512 B (vec 4) or 256 B (vec 1) of a row per workgroup
  int lanes = 1;
  while (lanes < cap && lanes < per_row) lanes <<= 1;
  g.col_lanes = lanes;
  g.row_lanes = kBlockThreads / lanes;
  g.col_tiles = (int)((per_row + lanes - 1) / lanes);
  return g;
}

// Thread t of the workgroup of column tile `tile`: its column lane, its row lane and the first of its `vec` columns (the thread
// takes part in the row loop only when col0 < C; vec 4: C is a multiple of 4, so col0 + 3 < C as well).
struct Tile {
  int cl, rl;
  int64_t col0;
};

GNC_POOL_HD Tile tile_of(int t, int64_t tile, const Geometry& geo) {
  Tile x;
  x.cl = t % geo.col_lanes;
  x.rl = t / geo.col_lanes;
  x.col0 = (tile * geo.col_lanes + x.cl) * geo.vec;
  return x;
}

// Halving tree over the row lanes: at step s (row_lanes / 2, ..., 1) thread t of a row lane < s adds the thread of row lane
// rl + s that owns the same columns.
GNC_POOL_HD int tree_partner(int t, int s, const Geometry& geo) { return t + s * geo.col_lanes; }

// Rows of the chunk that starts at row k0 (a multiple of kChunkRows, counted from the graph's first row) of an n-row graph.
GNC_POOL_HD int chunk_len(int64_t n, int64_t k0) { return (int)(n - k0 < kChunkRows ? n - k0 : kChunkRows); }

// Rows [a, b) of graph g, clamped into [0, rows]: offsets that point outside y read as shorter or empty graphs.
GNC_POOL_HD void graph_range(const int64_t* graph_ptr, int64_t g, int64_t rows, int64_t& a, int64_t& b) {
  a = graph_ptr[g];
  b = graph_ptr[g + 1];
  a = a < 0 ? 0 : (a > rows ? rows : a);
  b = b < a ? a : (b > rows ? rows : b);
}

GNC_POOL_HD int64_t chunks_of(int64_t n) { return (n + kChunkRows - 1) / kChunkRows; }

// Slots of the split regime's workspace: an upper bound of the chunks of G graphs that own at most `rows` rows in all
// (sum of ceil(n_g / R) <= floor(rows / R) + G).
GNC_POOL_HD int64_t split_slots(int64_t rows, int64_t G) { return rows / kChunkRows + G; }

// The slot of graph g's chunk 0: the chunks of the graphs in front of it.
GNC_POOL_HD int64_t first_slot(const int64_t* graph_ptr, int64_t g, int64_t rows) {
  int64_t cum = 0, a, b;
  for (int64_t h = 0; h < g; ++h) {
    graph_range(graph_ptr, h, rows, a, b);
    cum += chunks_of(b - a);
  }
  return cum;
}

// Split regime, merge: the rows n of graph g and the slots [s0, s1) of its chunks, in the order they are folded.  With offsets
// that overlap the chunks can outnumber the slots: only the slots that exist (and were written) are read.
GNC_POOL_HD void merge_slots(const int64_t* graph_ptr, int64_t g, int64_t rows, int64_t slots, int64_t& n, int64_t& s0, int64_t& s1) {
  int64_t a, b;
  graph_range(graph_ptr, g, rows, a, b);
  n = b - a;
  s0 = first_slot(graph_ptr, g, rows);
  s1 = s0 + chunks_of(n);
  if (s1 > slots) s1 = slots;
}

// Split regime: the chunk behind workspace slot `slot` - its graph, first row and row count (1 .. R).  false: no chunk (the
// slots behind the last graph's last chunk).
GNC_POOL_HD bool slot_chunk(const int64_t* graph_ptr, int64_t G, int64_t rows, int64_t slot, int64_t& g, int64_t& row0, int& nr) {
  int64_t cum = 0, a, b;
  for (g = 0; g < G; ++g) {
    graph_range(graph_ptr, g, rows, a, b);
    const int64_t nch = chunks_of(b - a);
    if (slot < cum + nch) {
      row0 = a + (slot - cum) * kChunkRows;
      nr = chunk_len(b - a, row0 - a);
      return true;
    }
    cum += nch;
  }
  return false;
}

// Backward: the graph that owns row r, or -1 (a row in front of graph_ptr[0], behind graph_ptr[G], or a slack row).  The
// number of graphs whose END is <= r is found by bisection (empty graphs are stepped over); the candidate is then checked
// against its clamped range, so offsets that are not sorted give some in-range answer or -1, never an index outside [0, G).
GNC_POOL_HD int64_t graph_of_row(const int64_t* graph_ptr, int64_t G, int64_t rows, int64_t r, int64_t& n) {
  int64_t lo = 0, hi = G;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (graph_ptr[mid + 1] <= r) lo = mid + 1;
    else hi = mid;
  }
  if (lo >= G) return -1;
  int64_t a, b;
  graph_range(graph_ptr, lo, rows, a, b);
  if (r < a || r >= b) return -1;
  n = b - a;
  return lo;
}

// K17's backward: item i of a [rows, C / vec] grid-stride walk is `vec` columns from c0 of row r.
GNC_POOL_HD void backward_item(int64_t i, int64_t per_row, int vec, int64_t& r, int64_t& c0) {
  r = i / per_row;
  c0 = (i - r * per_row) * vec;
}

// Row-wise launches (K19's backward, K20's row compaction): `lanes` threads side by side own ONE row (a power of two <= 64, so a
// row never straddles a wavefront), each `vec` consecutive columns at a time (4 when C is a multiple of 4); lane l takes the
// column groups l, l + lanes, ... in ascending order and the lanes' partial dot products are folded by a butterfly (lane l +=
// lane l ^ s for s = lanes / 2, ..., 1).  A function of C ALONE: it fixes the order of the dot over C.
struct RowGeometry {
  int vec, lanes, rows_per_block;
};

GNC_POOL_HD RowGeometry row_geometry(int64_t C) {
  RowGeometry g;
  g.vec = (C % 4 == 0) ? 4 : 1;
  const int64_t per_row = C / g.vec;  // column groups of a row (vec 1: C itself)
  int lanes = 1;
  while (lanes < 64 && lanes < per_row) lanes <<= 1;
  g.lanes = lanes;
  g.rows_per_block = kBlockThreads / lanes;
  return g;
}

// Thread t of such a workgroup: its lane inside the row and which of the workgroup's rows_per_block rows it works on.
struct RowLane {
  int lane, sub;
};

GNC_POOL_HD RowLane row_lane(unsigned t, int lanes) { return RowLane{(int)(t % lanes), (int)(t / lanes)}; }

}  // namespace gnc_pool
