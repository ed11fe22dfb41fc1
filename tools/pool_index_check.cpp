// Host walk of K17's index arithmetic (graphnet_classifier_amd/csrc/pool_index.h): for a set of batches - empty graphs, graphs
// whose row count is an exact multiple of the chunk length, slack rows, offsets that point outside the table - every
// (workgroup, thread) of the three forward launches and every item of the backward launch is enumerated as the kernels
// enumerate them, and every address they would form is checked against the buffers.  Exit status 0 = every check held.
//   c++ -std=c++17 -O1 -I graphnet_classifier_amd/csrc tools/pool_index_check.cpp -o pool_index_check && ./pool_index_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pool_index.h"

using namespace gnc_pool;

static int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      if (++failures <= 20) {                  \
        std::printf("FAILED %s: ", #cond);     \
        std::printf(__VA_ARGS__);              \
        std::printf("\n");                     \
      }                                        \
    }                                          \
  } while (0)

// rows of y that the chunk (row0, nr) of graph g reads through column tile `tile`, as chunk_reduce walks them
static void walk_chunk(const Geometry& geo, int64_t rows, int64_t C, int64_t a, int64_t b, int64_t row0, int nr, int tile,
                       std::vector<int>& seen) {
  CHECK(nr >= 1 && nr <= kChunkRows && row0 >= a && row0 + nr <= b, "chunk [%lld, +%d) outside its graph [%lld, %lld)",
        (long long)row0, nr, (long long)a, (long long)b);
  for (int t = 0; t < kBlockThreads; ++t) {
    const int cl = t % geo.col_lanes, rl = t / geo.col_lanes;
    const int64_t col0 = ((int64_t)tile * geo.col_lanes + cl) * geo.vec;
    if (col0 >= C) continue;
    CHECK(col0 + geo.vec <= C, "columns [%lld, +%d) leave C = %lld", (long long)col0, geo.vec, (long long)C);
    for (int r = rl; r < nr; r += geo.row_lanes) {
      const int64_t row = row0 + r;
      CHECK(row >= 0 && row < rows, "row %lld outside [0, %lld)", (long long)row, (long long)rows);
      if (row < 0 || row >= rows) continue;
      for (int u = 0; u < geo.vec; ++u) ++seen[row * C + col0 + u];
    }
    for (int s = geo.row_lanes >> 1; s >= 1; s >>= 1)
      if (rl < s) CHECK(t + s * geo.col_lanes < kBlockThreads, "tree partner %d outside the workgroup", t + s * geo.col_lanes);
  }
}

static void check_batch(int64_t rows, int64_t C, const std::vector<int64_t>& gp, bool sorted_in_range) {
  const int64_t G = (int64_t)gp.size() - 1;
  const Geometry geo = geometry(C);
  CHECK(geo.col_lanes * geo.row_lanes == kBlockThreads && geo.row_lanes >= 4 && (geo.vec == 1 || C % 4 == 0) &&
            (int64_t)geo.col_tiles * geo.col_lanes * geo.vec >= C && (int64_t)(geo.col_tiles - 1) * geo.col_lanes * geo.vec < C,
        "geometry of C = %lld", (long long)C);
  // many-graphs regime
  std::vector<int> seen(rows * C + 1, 0);
  for (int64_t g = 0; g < G; ++g) {
    int64_t a, b;
    graph_range(gp.data(), g, rows, a, b);
    CHECK(0 <= a && a <= b && b <= rows, "range of graph %lld", (long long)g);
    for (int tile = 0; tile < geo.col_tiles; ++tile)
      for (int64_t k0 = 0; k0 < b - a; k0 += kChunkRows)
        walk_chunk(geo, rows, C, a, b, a + k0, (int)(b - a - k0 < kChunkRows ? b - a - k0 : kChunkRows), tile, seen);
  }
  std::vector<int> expect(rows * C + 1, 0);
  for (int64_t g = 0; g < G; ++g) {
    int64_t a, b;
    graph_range(gp.data(), g, rows, a, b);
    for (int64_t i = a * C; i < b * C; ++i) ++expect[i];
  }
  CHECK(seen == expect, "many-graphs regime: an element of a graph is not read exactly once");
  // split regime: slots -> chunks, then the merge's enumeration of the same slots
  const int64_t slots = split_slots(rows, G);
  std::vector<int> seen2(rows * C + 1, 0);
  std::vector<int64_t> slot_graph(slots, -1);
  int64_t used = 0;
  for (int64_t slot = 0; slot < slots; ++slot) {
    int64_t g, row0;
    int nr;
    if (!slot_chunk(gp.data(), G, rows, slot, g, row0, nr)) continue;
    CHECK(g >= 0 && g < G, "slot %lld names graph %lld", (long long)slot, (long long)g);
    int64_t a, b;
    graph_range(gp.data(), g, rows, a, b);
    CHECK((row0 - a) % kChunkRows == 0 && first_slot(gp.data(), g, rows) + (row0 - a) / kChunkRows == slot, "slot %lld is not its graph's chunk",
          (long long)slot);
    slot_graph[slot] = g;
    ++used;
    for (int tile = 0; tile < geo.col_tiles; ++tile) walk_chunk(geo, rows, C, a, b, row0, nr, tile, seen2);
  }
  int64_t chunks = 0;
  for (int64_t g = 0; g < G; ++g) {
    int64_t a, b;
    graph_range(gp.data(), g, rows, a, b);
    const int64_t s0 = first_slot(gp.data(), g, rows);
    int64_t s1 = s0 + chunks_of(b - a);
    chunks += chunks_of(b - a);
    if (s1 > slots) s1 = slots;
    for (int64_t s = s0; s < s1; ++s) CHECK(s >= 0 && s < slots && slot_graph[s] == g, "merge of graph %lld reads slot %lld", (long long)g, (long long)s);
  }
  if (sorted_in_range) {
    CHECK(chunks <= slots && used == chunks, "%lld chunks, %lld slots, %lld written", (long long)chunks, (long long)slots, (long long)used);
    CHECK(seen2 == expect, "split regime: an element of a graph is not read exactly once");
  }
  // backward: the graph of every row
  for (int64_t r = 0; r < rows; ++r) {
    int64_t n = -1;
    const int64_t g = graph_of_row(gp.data(), G, rows, r, n);
    CHECK(g >= -1 && g < G, "row %lld -> graph %lld", (long long)r, (long long)g);
    if (!sorted_in_range) continue;
    int64_t want = -1, wn = -1;
    for (int64_t h = 0; h < G; ++h)
      if (gp[h] <= r && r < gp[h + 1]) want = h, wn = gp[h + 1] - gp[h];
    CHECK(g == want && (g < 0 || n == wn), "row %lld -> graph %lld (n %lld), expected %lld (n %lld)", (long long)r, (long long)g,
          (long long)n, (long long)want, (long long)wn);
  }
}

static std::vector<int64_t> offsets(int64_t first, const std::vector<int64_t>& sizes) {
  std::vector<int64_t> gp{first};
  for (int64_t s : sizes) gp.push_back(gp.back() + s);
  return gp;
}

int main() {
  const int R = kChunkRows;
  const int64_t widths[] = {1, 2, 3, 4, 5, 8, 12, 63, 64, 65, 128, 130, 132, 256, 260, 1000};
  for (int64_t C : widths) {
    const std::vector<std::vector<int64_t>> batches = {
        {0, 1, 63, 64, 65, R, R + 1, 2 * R + 37, 5}, {0}, {0, 0, 0}, {R}, {2 * R}, {3 * R, 0, R}, {1}, {2 * R + 37}, {R - 1, R, R + 1, 0},
        {5 * R + 3}};
    for (const auto& sizes : batches)
      for (int64_t slack : {0, 40})
        for (int64_t first : {0, 7}) {
          const auto gp = offsets(first, sizes);
          check_batch(gp.back() + slack, C, gp, true);
        }
    // offsets that leave the table or are not sorted: nothing may be addressed outside the buffers
    check_batch(100, C, {0, 50, 400, 90}, false);
    check_batch(100, C, {-5, 300, 20, 1000}, false);
    check_batch(300, C, {0, 300, 0, 300, 0, 300}, false);
    check_batch(0, C, {0, 0}, true);
  }
  std::srand(12345);
  for (int it = 0; it < 200; ++it) {
    std::vector<int64_t> sizes(1 + std::rand() % 12);
    for (auto& s : sizes) s = (std::rand() % 4 == 0) ? (std::rand() % 4) * R : std::rand() % (3 * R);
    const auto gp = offsets(std::rand() % 3, sizes);
    check_batch(gp.back() + std::rand() % 50, 1 + std::rand() % 140, gp, true);
  }
  std::printf(failures ? "pool_index_check: %d FAILED\n" : "pool_index_check: ok\n", failures);
  return failures ? 1 : 0;
}
