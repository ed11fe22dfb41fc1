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

// ---- the capacity-padded layout: a pooling layer's outputs keep the input's sizes, `rows` node rows and E edges.
// Behind the N' kept rows lie S_R = rows - N' SLACK rows (zero rows of no graph), behind the E' kept edges S_E = E - E' slack
// edges, each a self-loop of a slack row, spread evenly: slack edge t (position E' + t) belongs to slack row floor(t S_R / S_E), so
// the list stays destination-sorted, slack row u owns the edges [ceil(u S_E / S_R), ceil((u + 1) S_E / S_R)) and none owns more
// than ceil(S_E / S_R).  Products of two values below 2^31: 64 bits hold them.
struct Slack {
  int64_t n_out, e_out;  // N', E': the device counts, clamped into [0, rows] / [0, E]
  int64_t s_r, s_e;      // slack rows, slack edges
};

GNC_POOL_HD Slack slack_of(int64_t n_count, int64_t e_count, int64_t rows, int64_t E) {
  Slack s;
  s.n_out = n_count < 0 ? 0 : (n_count > rows ? rows : n_count);
  s.e_out = e_count < 0 ? 0 : (e_count > E ? E : e_count);
  s.s_r = rows - s.n_out;
  s.s_e = E - s.e_out;
  return s;
}

// Row of slack edge t, 0 <= t < S_E (rows >= 1).  S_R == 0 - every row was kept, so a dropped edge had an endpoint outside
// [0, rows) and the source topology's flags are set: the result is poisoned, and the loops go to the last row so that no index
// leaves the table.
GNC_POOL_HD int64_t slack_edge_row(const Slack& s, int64_t rows, int64_t t) {
  return s.s_r > 0 ? s.n_out + (int64_t)((uint64_t)t * (uint64_t)s.s_r / (uint64_t)s.s_e) : rows - 1;
}

// rowptr'[i] for N' < i <= rows: E' + ceil((i - N') S_E / S_R); rowptr'[rows] = E (also with S_R == 0, where the last row takes
// the poisoned result's slack loops).
GNC_POOL_HD int64_t slack_rowptr(const Slack& s, int64_t rows, int64_t E, int64_t i) {
  if (i >= rows) return E;
  const uint64_t u = (uint64_t)(i - s.n_out);
  return s.e_out + (int64_t)((u * (uint64_t)s.s_e + (uint64_t)s.s_r - 1) / (uint64_t)s.s_r);
}

// The tail kept[N', rows) = -1 is written by the select workgroups together: workgroup g, thread t takes N' + g kT + t, then
// strides by G kT.
GNC_POOL_HD int64_t kept_tail_first(int64_t n_out, int64_t g, int t) { return n_out + g * kT + t; }
GNC_POOL_HD int64_t kept_tail_stride(int64_t G) { return G * kT; }

// (the row tiling of the compaction launches is pool_index.h's row_geometry / row_lane)
using gnc_pool::RowGeometry;
using gnc_pool::row_geometry;

}  // namespace gnc_topk
