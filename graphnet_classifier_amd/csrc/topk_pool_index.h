// Index arithmetic of K20 (csrc/topk_pool.hip): the order-preserving key of a score, the number of rows a graph keeps, the rows a
// select workgroup marks as dropped around its graph, the edge-scan tiling (the row tiling of the compaction launches is pool_index.h's).
// Host-compilable like pool_index.h, so that tools/topk_pool_index_check.cpp can walk every (workgroup, thread) of the launches
// and check each address before a kernel runs on a device.  Nothing here touches memory except `graph_ptr`.
#pragma once
#include "pool_index.h"

#include <math.h>

namespace gnc_topk {

constexpr int kT = gnc_pool::kBlockThreads;  // threads of every K20 workgroup
constexpr int kWaves = kT / 64;
// Edge scan: one workgroup owns kEdgeTile consecutive sorted-edge positions, walked as kEdgeSteps coalesced steps of kT edges
// (thread t takes positions tile * kEdgeTile + i * kT + t, i = 0 ... kEdgeSteps - 1).
constexpr int kEdgeSteps = 4;
constexpr int kEdgeTile = kEdgeSteps * kT;

// Order-preserving uint32 image of the fp32 bit pattern `u`: a < b as floats <=> key(a) < key(b); -0.0 and +0.0 share a key; every
// NaN (either sign, any payload) maps to 0, below -inf (0x007fffff).
GNC_POOL_HD uint32_t score_key(uint32_t u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;  // NaN
  if (u == 0x80000000u) u = 0u;                    // -0.0 -> +0.0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// k_g = min(n, max(1, ceil(ratio * n))) for n >= 1, 0 for n <= 0: product and ceiling in double (Python's math.ceil(ratio * n)).
GNC_POOL_HD int64_t keep_count(double ratio, int64_t n) {
  if (n <= 0) return 0;
  const double want = ceil(ratio * (double)n);
  if (!(want >= 1.0)) return 1;  // (a NaN product as well: nothing out of range is ever converted)
  if (want >= (double)n) return n;
  return (int64_t)want;
}

// The rows of NO graph that select workgroup g marks as dropped: those between the end of graph g - 1 (row 0 for g = 0) and the
// start of graph g, [lo, hi), and - the last graph alone - those behind its own end, [tail, rows).  With non-decreasing offsets the
// G workgroups cover every row outside the graphs exactly once.
GNC_POOL_HD void gap_rows(const int64_t* graph_ptr, int64_t g, int64_t G, int64_t rows, int64_t& lo, int64_t& hi, int64_t& tail) {
  int64_t a, b, pa, pb = 0;
  gnc_pool::graph_range(graph_ptr, g, rows, a, b);
  if (g > 0) gnc_pool::graph_range(graph_ptr, g - 1, rows, pa, pb);
  lo = pb < a ? pb : a;
  hi = a;
  tail = g == G - 1 ? b : rows;
}

GNC_POOL_HD int64_t edge_tiles(int64_t E) { return (E + kEdgeTile - 1) / kEdgeTile; }
GNC_POOL_HD int64_t edge_position(int64_t tile, int step, int t) { return tile * kEdgeTile + (int64_t)step * kT + t; }
// int32 workspace of the edge filter: the tiles' kept counts (turned into their exclusive scan in place) in front, the exclusive
// count of kept edges at EVERY sorted position behind.
GNC_POOL_HD int64_t edge_workspace_ints(int64_t E) { return edge_tiles(E) + E; }

// (the row tiling of the compaction launches is pool_index.h's row_geometry / row_lane)
using gnc_pool::RowGeometry;
using gnc_pool::row_geometry;

}  // namespace gnc_topk
