// Host walk of the capacity-padded layout of K20 (graphnet_classifier_amd/csrc/topk_pool_index.h: slack_of, slack_edge_row,
// slack_rowptr, kept_tail_first / kept_tail_stride).  For rows, E, N', E' drawn from the awkward sizes around the 256-thread chunk
// and the 1024-edge tile, every (workgroup, thread) of the three launches that write the tails is enumerated as the kernels of
// csrc/topk_pool.hip enumerate them: topk_edge_write_kernel's positions at and behind E' (the slack self-loops), topk_rowptr_kernel's
// entries behind N', and the select workgroups' share of kept[N', rows).  Checked: every slack position and every tail entry is
// written exactly once and nothing in front of them is touched; the loops' rows stay inside [N', rows); dst' is non-decreasing;
// rowptr' agrees with the edge list and ends at E; no slack row owns more than ceil(S_E / S_R) loops; with S_R == 0 the loops go to
// row rows - 1; with rows == 0 there is nothing to walk (the launcher launches nothing).  One case near 2^31 / 4 and one near 2^31
// exercise the 64-bit products at sampled positions.  Exit status 0 = every check held.
//   c++ -std=c++17 -O1 -fsanitize=address,undefined -I graphnet_classifier_amd/csrc -I tools tools/topk_pool_padded_index_check.cpp \
//       -o topk_pool_padded_index_check && ./topk_pool_padded_index_check
#include <algorithm>
#include <vector>

#include "pool_walk.h"
#include "topk_pool_index.h"

using namespace gnc_topk;

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the slack edges as topk_edge_write_kernel writes them: thread (tile, step, t) owns position p and, at p >= E', the loop at p
static void walk_slack_edges(const Slack& s, int64_t rows, int64_t E, std::vector<int32_t>& dst) {
  std::vector<int> writes(E + 1, 0);
  for (int64_t tile = 0; tile < edge_tiles(E); ++tile)
    for (int i = 0; i < kEdgeSteps; ++i)
      for (int t = 0; t < kT; ++t) {
        const int64_t p = edge_position(tile, i, t);
        if (p >= E || p < s.e_out) continue;
        const int64_t row = slack_edge_row(s, rows, p - s.e_out);
        CHECK(row >= 0 && row < rows, "slack edge %lld -> row %lld outside [0, %lld)", (long long)p, (long long)row, (long long)rows);
        if (s.s_r > 0) CHECK(row >= s.n_out, "slack edge %lld -> kept row %lld (N' %lld)", (long long)p, (long long)row, (long long)s.n_out);
        else CHECK(row == rows - 1, "S_R == 0: slack edge %lld -> row %lld, not the last row", (long long)p, (long long)row);
        ++writes[p];
        dst[p] = (int32_t)row;
      }
  for (int64_t p = 0; p < E; ++p) CHECK(writes[p] == (p >= s.e_out ? 1 : 0), "position %lld (E' %lld) written %d times", (long long)p, (long long)s.e_out, writes[p]);
  for (int64_t p = s.e_out; p + 1 < E; ++p) CHECK(dst[p] <= dst[p + 1], "dst' decreases at %lld", (long long)p);
}

// topk_rowptr_kernel with `blocks` workgroups: the first loop covers [0, N'], the padded loop (N', rows]
static void walk_rowptr(const Slack& s, int64_t rows, int64_t E, int64_t blocks, std::vector<int64_t>& rowptr) {
  std::vector<int> writes(rows + 2, 0);
  for (int64_t blk = 0; blk < blocks; ++blk)
    for (int t = 0; t < kT; ++t) {
      const int64_t first = blk * kT + t, stride = blocks * kT;
      for (int64_t i = first; i <= s.n_out; i += stride) {
        ++writes[i];
        if (i == s.n_out) rowptr[i] = i == rows ? E : s.e_out;  // (entries in front of N' come from the scan: not this walk's)
      }
      for (int64_t i = s.n_out + 1 + first; i <= rows; i += stride) {
        CHECK(i > s.n_out && i <= rows, "rowptr' entry %lld outside (N', rows]", (long long)i);
        ++writes[i];
        rowptr[i] = slack_rowptr(s, rows, E, i);
      }
    }
  for (int64_t i = 0; i <= rows; ++i) CHECK(writes[i] == 1, "rowptr'[%lld] written %d times (%lld blocks)", (long long)i, writes[i], (long long)blocks);
  CHECK(writes[rows + 1] == 0, "rowptr' written behind its end");
}

// the select workgroups' share of kept[N', rows)
static void walk_kept_tail(int64_t n_out, int64_t rows, int64_t G) {
  std::vector<int> writes(rows + 1, 0);
  for (int64_t g = 0; g < G; ++g)
    for (int t = 0; t < kT; ++t)
      for (int64_t r = kept_tail_first(n_out, g, t); r < rows; r += kept_tail_stride(G)) {
        CHECK(r >= n_out && r < rows, "kept tail entry %lld outside [%lld, %lld)", (long long)r, (long long)n_out, (long long)rows);
        if (r >= 0 && r < rows) ++writes[r];
      }
  for (int64_t r = 0; r < rows; ++r) CHECK(writes[r] == (r >= n_out ? 1 : 0), "kept[%lld] (N' %lld, %lld graphs) written %d times", (long long)r, (long long)n_out, (long long)G, writes[r]);
}

static void walk(int64_t rows, int64_t E, int64_t n_count, int64_t e_count) {
  const Slack s = slack_of(n_count, e_count, rows, E);
  CHECK(s.n_out == n_count && s.e_out == e_count && s.s_r == rows - n_count && s.s_e == E - e_count, "slack_of(%lld, %lld, %lld, %lld)",
        (long long)n_count, (long long)e_count, (long long)rows, (long long)E);
  if (rows == 0) return;  // the launcher launches nothing: no row a loop could sit on
  std::vector<int32_t> dst(E + 1, -1);
  std::vector<int64_t> rowptr(rows + 1, -1);
  walk_slack_edges(s, rows, E, dst);
  for (int64_t blocks : {(int64_t)1, (int64_t)7}) walk_rowptr(s, rows, E, blocks, rowptr);
  CHECK(rowptr[rows] == E, "rowptr'[rows] = %lld, not E = %lld", (long long)rowptr[rows], (long long)E);
  CHECK(rowptr[s.n_out] == (s.n_out == rows ? E : s.e_out), "rowptr'[N'] = %lld", (long long)rowptr[s.n_out]);
  // rowptr' agrees with the edge list: slack row i owns exactly the positions [rowptr'[i], rowptr'[i + 1])
  std::vector<int64_t> loops(rows + 1, 0);
  for (int64_t p = s.e_out; p < E; ++p) ++loops[dst[p]];
  const int64_t most = s.s_r > 0 ? ceil_div(s.s_e, s.s_r) : s.s_e;
  for (int64_t i = s.n_out; i < rows; ++i) {
    CHECK(rowptr[i + 1] - rowptr[i] == loops[i], "slack row %lld: rowptr' says %lld loops, the list holds %lld", (long long)i,
          (long long)(rowptr[i + 1] - rowptr[i]), (long long)loops[i]);
    CHECK(loops[i] <= most, "slack row %lld owns %lld loops, more than ceil(S_E / S_R) = %lld", (long long)i, (long long)loops[i], (long long)most);
    for (int64_t p = rowptr[i]; p < rowptr[i + 1] && p >= 0 && p < E; ++p) CHECK(dst[p] == i, "position %lld lies in row %lld's range but loops on %d", (long long)p, (long long)i, dst[p]);
  }
  if (s.s_r == 0) CHECK(loops[rows - 1] == s.s_e, "S_R == 0: the last row owns %lld of the %lld slack loops", (long long)loops[rows - 1], (long long)s.s_e);
}

// sizes too large to enumerate: the ends and a stride of sampled positions
static void walk_sampled(int64_t rows, int64_t E, int64_t n_count, int64_t e_count) {
  const Slack s = slack_of(n_count, e_count, rows, E);
  const int64_t step = s.s_e / 4099 + 1;
  int64_t before = -1;
  std::vector<int64_t> sampled;
  for (int64_t t = 0; t < s.s_e; t += step) sampled.push_back(t);
  for (int64_t t : {(int64_t)1, (int64_t)2, s.s_e - 3, s.s_e - 2, s.s_e - 1})
    if (t >= 0 && t < s.s_e) sampled.push_back(t);
  std::sort(sampled.begin(), sampled.end());
  for (int64_t t : sampled) {
    const int64_t row = slack_edge_row(s, rows, t);
    CHECK(row >= s.n_out && row < rows && row >= before, "sampled slack edge %lld -> row %lld (previous %lld)", (long long)t, (long long)row, (long long)before);
    before = row;
    // the row's range in rowptr' holds the position
    const int64_t lo = slack_rowptr(s, rows, E, row), hi = slack_rowptr(s, rows, E, row + 1);
    CHECK(lo <= s.e_out + t && s.e_out + t < hi && hi - lo <= ceil_div(s.s_e, s.s_r), "sampled slack edge %lld: row %lld owns [%lld, %lld)", (long long)t,
          (long long)row, (long long)lo, (long long)hi);
  }
  CHECK(slack_edge_row(s, rows, s.s_e - 1) == rows - 1 || s.s_e < s.s_r, "the last slack edge does not reach the last row");
  CHECK(slack_rowptr(s, rows, E, rows) == E && slack_rowptr(s, rows, E, s.n_out + 1) >= s.e_out, "ends of rowptr'");
  const int64_t rstep = s.s_r / 4099 + 1;
  for (int64_t i = s.n_out + 1; i < rows; i += rstep) {
    const int64_t a = slack_rowptr(s, rows, E, i), b = slack_rowptr(s, rows, E, i + 1);
    CHECK(a >= s.e_out && a <= b && b <= E, "sampled rowptr'[%lld] = %lld, next %lld", (long long)i, (long long)a, (long long)b);
    if (a < b) CHECK(slack_edge_row(s, rows, a - s.e_out) == i && slack_edge_row(s, rows, b - 1 - s.e_out) == i, "row %lld does not own its range's ends", (long long)i);
  }
}

int main() {
  const int64_t sizes[] = {0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 70001};
  for (int64_t rows : sizes)
    for (int64_t n_count : sizes) {
      if (n_count > rows) continue;
      for (int64_t G : {(int64_t)1, (int64_t)3, (int64_t)300}) walk_kept_tail(n_count, rows, G);
      for (int64_t E : sizes)
        for (int64_t e_count : sizes)
          if (e_count <= E) walk(rows, E, n_count, e_count);
    }
  // counts outside their range are clamped before anything is derived from them
  const Slack c = slack_of(-5, 1ll << 40, 10, 20);
  CHECK(c.n_out == 0 && c.e_out == 20 && c.s_r == 10 && c.s_e == 0, "clamping of the counts");
  const int64_t quarter = (1ll << 29) + 3, most = (1ll << 31) - 1;
  walk_sampled(quarter, quarter, 1, 2);
  walk_sampled(quarter, quarter - 7, quarter / 2 + 1, 1025);
  walk_sampled(most, most, 3, 0);
  walk_sampled(most, 1025, 1, 1);
  walk_sampled(1025, most, 1, 1);
  return pool_walk::finish("topk_pool_padded_index_check");
}
