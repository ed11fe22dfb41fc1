// Host walk of K17's index arithmetic (graphnet_classifier_amd/csrc/pool_index.h): for a set of batches - empty graphs, graphs
// whose row count is an exact multiple of the chunk length, slack rows, offsets that point outside the table - every
// (workgroup, thread) of the three forward launches and every item of the backward launch is enumerated through the functions
// the kernels call (tools/pool_walk.h), and every address they would form is checked against the buffers.  Exit status 0 = every
// check held.
//   c++ -std=c++17 -O1 -fsanitize=address,undefined -I graphnet_classifier_amd/csrc -I tools tools/pool_index_check.cpp \
//       -o pool_index_check && ./pool_index_check
#include "pool_walk.h"

using namespace pool_walk;

static void check_batch(int64_t rows, int64_t C, const Offsets& gp, bool sorted_in_range) {
  const Geometry geo = geometry(C);
  check_geometry(geo, C);
  const std::vector<int> expect = expected_reads(rows, C, gp);
  std::vector<int> seen(rows * C + 1, 0), seen2(rows * C + 1, 0);
  walk_graph_owned(geo, rows, C, gp, count_columns(seen, C, geo.vec), [](int64_t, int64_t, int64_t, int) {});
  CHECK(seen == expect, "many-graphs regime: an element of a graph is not read exactly once");
  walk_split(geo, rows, C, gp, sorted_in_range, count_columns(seen2, C, geo.vec), [](int64_t, int64_t) {}, [](int64_t, int64_t, int) {},
             [](int64_t, int64_t, int64_t, int64_t) {});
  if (sorted_in_range) CHECK(seen2 == expect, "split regime: an element of a graph is not read exactly once");
  // backward: the graph of every row, and every element of dy written exactly once by the grid-stride items
  for (int64_t r = 0; r < rows; ++r) check_graph_of_row(gp, rows, r, sorted_in_range);
  const int64_t per_row = C / geo.vec, items = rows * per_row;
  for (int64_t blocks : {(int64_t)1, (int64_t)3}) {
    std::vector<int> dy(rows * C + 1, 0);
    for (int64_t i0 = 0; i0 < blocks * kBlockThreads; ++i0)  // thread i0 of the grid
      for (int64_t i = i0; i < items; i += blocks * kBlockThreads) {
        int64_t r, c0;
        backward_item(i, per_row, geo.vec, r, c0);
        CHECK(r >= 0 && r < rows && c0 >= 0 && c0 + geo.vec <= C, "item %lld -> row %lld, columns from %lld", (long long)i, (long long)r, (long long)c0);
        if (r >= 0 && r < rows && c0 >= 0 && c0 + geo.vec <= C)
          for (int u = 0; u < geo.vec; ++u) ++dy[r * C + c0 + u];
      }
    bool once = true;
    for (int64_t i = 0; i < rows * C; ++i) once = once && dy[i] == 1;
    CHECK(once, "backward with %lld workgroups: an element of dy is not written exactly once", (long long)blocks);
  }
}

int main() {
  standard_batches({1, 2, 3, 4, 5, 8, 12, 63, 64, 65, 128, 130, 132, 256, 260, 1000}, 200, check_batch);
  return finish("pool_index_check");
}
