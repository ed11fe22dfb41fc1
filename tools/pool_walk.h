// What the three host index checks (pool_index_check.cpp, attention_pool_index_check.cpp, topk_pool_index_check.cpp) share: the
// CHECK macro, the standard batches, and the walks of the chunked per-graph reduction and of the row-wise launches.  Every index
// a walk forms comes from the function of graphnet_classifier_amd/csrc/pool_index.h that the kernels call for it (tile_of,
// tree_partner, chunk_len, slot_chunk, merge_slots, backward_item, row_lane), so an edit there reaches the walk and the kernels alike.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pool_index.h"

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

namespace pool_walk {

using namespace gnc_pool;
using Offsets = std::vector<int64_t>;

inline int finish(const char* program) {
  if (failures) std::printf("%s: %d FAILED\n", program, failures);
  else std::printf("%s: ok\n", program);
  return failures ? 1 : 0;
}

inline Offsets offsets(int64_t first, const std::vector<int64_t>& sizes) {
  Offsets gp{first};
  for (int64_t s : sizes) gp.push_back(gp.back() + s);
  return gp;
}

// check(rows, C, graph_ptr, sorted_in_range) over the standard batches - empty graphs, exact multiples of the chunk length, slack
// rows, rows in front, offsets that leave the table or are not sorted - at every width, then over `random` seeded batches.
template <class Check>
void standard_batches(const std::vector<int64_t>& widths, int random, Check check) {
  const int R = kChunkRows;
  for (int64_t C : widths) {
    const std::vector<std::vector<int64_t>> batches = {
        {0, 1, 63, 64, 65, R, R + 1, 2 * R + 37, 5}, {0}, {0, 0, 0}, {R}, {2 * R}, {3 * R, 0, R}, {1}, {2 * R + 37}, {R - 1, R, R + 1, 0},
        {5 * R + 3}};
    for (const auto& sizes : batches)
      for (int64_t slack : {0, 40})
        for (int64_t first : {0, 7}) {
          const auto gp = offsets(first, sizes);
          check(gp.back() + slack, C, gp, true);
        }
    // offsets that leave the table or are not sorted: nothing may be addressed outside the buffers
    check(100, C, Offsets{0, 50, 400, 90}, false);
    check(100, C, Offsets{-5, 300, 20, 1000}, false);
    check(300, C, Offsets{0, 300, 0, 300, 0, 300}, false);
    check(0, C, Offsets{0, 0}, true);
  }
  std::srand(12345);
  for (int it = 0; it < random; ++it) {
    std::vector<int64_t> sizes(1 + std::rand() % 12);
    for (auto& s : sizes) s = (std::rand() % 4 == 0) ? (std::rand() % 4) * R : std::rand() % (3 * R);
    const auto gp = offsets(std::rand() % 3, sizes);
    check(gp.back() + std::rand() % 50, 1 + std::rand() % 140, gp, true);
  }
}

// how often each of the [rows, width] elements that belong to a graph must be read: once per graph that holds its row
inline std::vector<int> expected_reads(int64_t rows, int64_t width, const Offsets& gp) {
  std::vector<int> expect(rows * width + 1, 0);
  for (int64_t g = 0; g + 1 < (int64_t)gp.size(); ++g) {
    int64_t a, b;
    graph_range(gp.data(), g, rows, a, b);
    CHECK(0 <= a && a <= b && b <= rows, "range of graph %lld", (long long)g);
    for (int64_t i = a * width; i < b * width; ++i) ++expect[i];
  }
  return expect;
}

inline void check_geometry(const Geometry& geo, int64_t C) {
  CHECK(geo.col_lanes * geo.row_lanes == kBlockThreads && geo.row_lanes >= 4 && (geo.vec == 1 || C % 4 == 0) &&
            (int64_t)geo.col_tiles * geo.col_lanes * geo.vec >= C && (int64_t)(geo.col_tiles - 1) * geo.col_lanes * geo.vec < C,
        "geometry of C = %lld", (long long)C);
}

// chunk_reduce: visit(row, tile, x) for every row of chunk (row0, nr) of graph [a, b) that thread x of column tile `tile` reads
template <class Visit>
void walk_chunk(const Geometry& geo, int64_t rows, int64_t C, int64_t a, int64_t b, int64_t row0, int nr, int tile, Visit visit) {
  CHECK(nr >= 1 && nr <= kChunkRows && row0 >= a && row0 + nr <= b, "chunk [%lld, +%d) outside its graph [%lld, %lld)",
        (long long)row0, nr, (long long)a, (long long)b);
  for (int t = 0; t < kBlockThreads; ++t) {
    const Tile x = tile_of(t, tile, geo);
    CHECK(x.cl >= 0 && x.cl < geo.col_lanes && x.rl >= 0 && x.rl < geo.row_lanes, "thread %d -> lanes (%d, %d)", t, x.cl, x.rl);
    if (x.col0 >= C) continue;
    CHECK(x.col0 >= 0 && x.col0 + geo.vec <= C, "columns [%lld, +%d) leave C = %lld", (long long)x.col0, geo.vec, (long long)C);
    for (int r = x.rl; r < nr; r += geo.row_lanes) {
      const int64_t row = row0 + r;
      CHECK(row >= 0 && row < rows, "row %lld outside [0, %lld)", (long long)row, (long long)rows);
      if (row >= 0 && row < rows) visit(row, tile, x);
    }
    for (int s = geo.row_lanes >> 1; s >= 1; s >>= 1) {
      if (x.rl >= s) continue;
      const int o = tree_partner(t, s, geo);
      CHECK(o >= 0 && o < kBlockThreads, "tree partner %d outside the workgroup", o);
      if (o < 0 || o >= kBlockThreads) continue;
      const Tile y = tile_of(o, tile, geo);
      CHECK(y.rl == x.rl + s && y.col0 == x.col0, "tree partner %d of thread %d is not row-lane %d of its columns", o, t, x.rl + s);
    }
  }
}

// a visitor that counts the reads of y [rows, C]
inline auto count_columns(std::vector<int>& seen, int64_t C, int vec) {
  return [&seen, C, vec](int64_t row, int, const Tile& x) {
    for (int u = 0; u < vec; ++u) ++seen[row * C + x.col0 + u];
  };
}

// many-graphs regime: workgroup (g, tile) walks the graph's chunks; on_tile(g, a, b, tile) for what else the workgroup does
template <class Visit, class OnTile>
void walk_graph_owned(const Geometry& geo, int64_t rows, int64_t C, const Offsets& gp, Visit visit, OnTile on_tile) {
  for (int64_t g = 0; g + 1 < (int64_t)gp.size(); ++g) {
    int64_t a, b;
    graph_range(gp.data(), g, rows, a, b);
    for (int tile = 0; tile < geo.col_tiles; ++tile) {
      on_tile(g, a, b, tile);
      for (int64_t k0 = 0; k0 < b - a; k0 += kChunkRows) walk_chunk(geo, rows, C, a, b, a + k0, chunk_len(b - a, k0), tile, visit);
    }
  }
}

// split regime: workgroup (slot, tile) walks the slot's chunk - on_slot(slot, g) once, on_tile(slot, g, tile) per tile - then the
// merge of every graph, on_merge(g, n, s0, s1), reads only slots that its own graph's chunks wrote.
template <class Visit, class OnSlot, class OnTile, class OnMerge>
void walk_split(const Geometry& geo, int64_t rows, int64_t C, const Offsets& gp, bool sorted_in_range, Visit visit, OnSlot on_slot,
                OnTile on_tile, OnMerge on_merge) {
  const int64_t G = (int64_t)gp.size() - 1, slots = split_slots(rows, G);
  std::vector<int64_t> slot_graph(slots, -1);
  int64_t used = 0, chunks = 0;
  for (int64_t slot = 0; slot < slots; ++slot) {
    int64_t g, row0, a, b;
    int nr;
    if (!slot_chunk(gp.data(), G, rows, slot, g, row0, nr)) continue;
    CHECK(g >= 0 && g < G, "slot %lld names graph %lld", (long long)slot, (long long)g);
    if (g < 0 || g >= G) continue;
    graph_range(gp.data(), g, rows, a, b);
    CHECK((row0 - a) % kChunkRows == 0 && first_slot(gp.data(), g, rows) + (row0 - a) / kChunkRows == slot, "slot %lld is not its graph's chunk",
          (long long)slot);
    slot_graph[slot] = g;
    ++used;
    on_slot(slot, g);
    for (int tile = 0; tile < geo.col_tiles; ++tile) {
      walk_chunk(geo, rows, C, a, b, row0, nr, tile, visit);
      on_tile(slot, g, tile);
    }
  }
  for (int64_t g = 0; g < G; ++g) {
    int64_t a, b, n, s0, s1;
    graph_range(gp.data(), g, rows, a, b);
    merge_slots(gp.data(), g, rows, slots, n, s0, s1);
    CHECK(n == b - a && s0 >= 0 && s1 <= slots, "merge of graph %lld: %lld rows, slots [%lld, %lld) of %lld", (long long)g, (long long)n,
          (long long)s0, (long long)s1, (long long)slots);
    chunks += chunks_of(n);
    for (int64_t s = s0; s < s1 && s < slots; ++s) CHECK(s >= 0 && slot_graph[s] == g, "merge of graph %lld reads slot %lld", (long long)g, (long long)s);
    if (sorted_in_range) CHECK(s1 - s0 == chunks_of(n), "merge of graph %lld folds %lld of its %lld chunks", (long long)g, (long long)(s1 - s0), (long long)chunks_of(n));
    on_merge(g, n, s0, s1 < slots ? s1 : slots);
  }
  if (sorted_in_range) CHECK(chunks <= slots && used == chunks, "%lld chunks, %lld slots, %lld written", (long long)chunks, (long long)slots, (long long)used);
}

// graph_of_row: inside [-1, G), and for sorted in-range offsets the graph (and its row count) that holds the row
inline int64_t check_graph_of_row(const Offsets& gp, int64_t rows, int64_t r, bool sorted_in_range) {
  const int64_t G = (int64_t)gp.size() - 1;
  int64_t n = -1, want = -1, wn = -1;
  const int64_t g = graph_of_row(gp.data(), G, rows, r, n);
  CHECK(g >= -1 && g < G, "row %lld -> graph %lld", (long long)r, (long long)g);
  if (!sorted_in_range) return g;
  for (int64_t h = 0; h < G; ++h)
    if (gp[h] <= r && r < gp[h + 1]) want = h, wn = gp[h + 1] - gp[h];
  CHECK(g == want && (g < 0 || n == wn), "row %lld -> graph %lld (n %lld), expected %lld (n %lld)", (long long)r, (long long)g, (long long)n,
        (long long)want, (long long)wn);
  return g;
}

// Row-wise launches with `blocks` workgroups (K19's backward, K20's row kernels; K20's forward enumerates the same rows):
// cell(r, c) for every column a lane touches, row_done(r) for lane 0; the butterfly must stay inside the row's own lanes.
template <class Cell, class RowDone>
void walk_row_tiles(const RowGeometry& rg, int64_t rows, int64_t C, int64_t blocks, Cell cell, RowDone row_done) {
  CHECK(rg.lanes >= 1 && rg.lanes <= 64 && (rg.lanes & (rg.lanes - 1)) == 0 && rg.lanes * rg.rows_per_block == kBlockThreads &&
            (rg.vec == 1 || C % 4 == 0),
        "row geometry of C = %lld", (long long)C);
  const int W = rg.lanes, rpb = rg.rows_per_block;
  const int64_t per_row = C / rg.vec;
  for (int64_t blk = 0; blk < blocks; ++blk)
    for (int64_t base = blk * rpb; base < rows; base += blocks * rpb)
      for (int t = 0; t < kBlockThreads; ++t) {
        const RowLane x = row_lane(t, W);
        const int64_t r = base + x.sub;
        CHECK(x.lane >= 0 && x.lane < W && x.sub >= 0 && x.sub < rpb, "thread %d -> (lane %d, row %d)", t, x.lane, x.sub);
        for (int s = W >> 1; s >= 1; s >>= 1)
          CHECK(row_lane(t ^ s, W).sub == x.sub && (t ^ s) / 64 == t / 64, "butterfly partner %d of thread %d leaves its row", t ^ s, t);
        if (r >= rows) continue;
        for (int64_t q = x.lane; q < per_row; q += W)
          for (int u = 0; u < rg.vec; ++u) cell(r, q * rg.vec + u);
        if (x.lane == 0) row_done(r);
      }
}

}  // namespace pool_walk
