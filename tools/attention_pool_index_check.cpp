// Host walk of K19's index arithmetic (graphnet_classifier_amd/csrc/attention_pool_index.h over csrc/pool_index.h): for a set of
// batches - empty graphs, graphs whose row count is an exact multiple of the chunk length, slack rows, offsets that point outside
// the table - every (workgroup, thread) of the forward launches of both regimes, of the backward launch and of the weights launch
// is enumerated as csrc/attention_pool.hip enumerates them, every address they would form is checked against the buffers, and
// every workspace slot the merge reads is checked to have been written.  Exit status 0 = every check held.
//   c++ -std=c++17 -O1 -fsanitize=address,undefined -I graphnet_classifier_amd/csrc tools/attention_pool_index_check.cpp \
//       -o attention_pool_index_check && ./attention_pool_index_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "attention_pool_index.h"

using namespace gnc_pool;
using gnc_attn::RowGeometry;

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

struct Buffers {
  int64_t rows, C, G, ld_out;
  std::vector<int> y_reads, s_reads;  // [rows * C], [rows]: reads by the chunk walks
  std::vector<int> out_writes;        // [G * ld_out]
  std::vector<int> saved_m, saved_z;  // [G] each: writes
  Buffers(int64_t rows_, int64_t C_, int64_t G_)
      : rows(rows_), C(C_), G(G_), ld_out(C_ + 3), y_reads(rows_ * C_ + 1, 0), s_reads(rows_ + 1, 0), out_writes(G_ * (C_ + 3), 0),
        saved_m(G_, 0), saved_z(G_, 0) {}
};

// block_score_max: scores[a, b) strided over the workgroup, then the LDS tree
static void walk_score_max(int64_t rows, int64_t a, int64_t b, std::vector<int>& seen) {
  for (int t = 0; t < kBlockThreads; ++t) {
    for (int64_t r = a + t; r < b; r += kBlockThreads) {
      CHECK(r >= 0 && r < rows, "score %lld outside [0, %lld)", (long long)r, (long long)rows);
      if (r >= 0 && r < rows) ++seen[r];
    }
    for (int w = kBlockThreads >> 1; w >= 1; w >>= 1)
      if (t < w) CHECK(t + w < kBlockThreads, "tree partner %d outside the workgroup", t + w);
  }
}

// chunk_reduce: rows of y and scores that the chunk (row0, nr) reads through column tile `tile`
static void walk_chunk(const Geometry& geo, Buffers& B, int64_t a, int64_t b, int64_t row0, int nr, int tile) {
  CHECK(nr >= 1 && nr <= kChunkRows && row0 >= a && row0 + nr <= b, "chunk [%lld, +%d) outside its graph [%lld, %lld)",
        (long long)row0, nr, (long long)a, (long long)b);
  for (int t = 0; t < kBlockThreads; ++t) {
    const int cl = t % geo.col_lanes, rl = t / geo.col_lanes;
    const int64_t col0 = ((int64_t)tile * geo.col_lanes + cl) * geo.vec;
    if (col0 >= B.C) continue;
    CHECK(col0 + geo.vec <= B.C, "columns [%lld, +%d) leave C = %lld", (long long)col0, geo.vec, (long long)B.C);
    for (int r = rl; r < nr; r += geo.row_lanes) {
      const int64_t row = row0 + r;
      CHECK(row >= 0 && row < B.rows, "row %lld outside [0, %lld)", (long long)row, (long long)B.rows);
      if (row < 0 || row >= B.rows) continue;
      for (int u = 0; u < geo.vec; ++u) ++B.y_reads[row * B.C + col0 + u];
      if (tile == 0 && cl == 0) ++B.s_reads[row];  // (every column lane reads the same score; counted once)
    }
    for (int s = geo.row_lanes >> 1; s >= 1; s >>= 1)
      if (rl < s) CHECK(t + s * geo.col_lanes < kBlockThreads, "tree partner %d outside the workgroup", t + s * geo.col_lanes);
  }
}

// the stores of (graph g, column tile) by the threads of row-lane 0
static void walk_out_tile(const Geometry& geo, Buffers& B, int64_t g, int tile) {
  for (int t = 0; t < geo.col_lanes; ++t) {  // row-lane 0
    const int64_t col0 = ((int64_t)tile * geo.col_lanes + t) * geo.vec;
    if (col0 >= B.C) continue;
    for (int u = 0; u < geo.vec; ++u) {
      const int64_t o = g * B.ld_out + col0 + u;
      CHECK(o >= 0 && o < (int64_t)B.out_writes.size() && col0 + u < B.C, "out index %lld", (long long)o);
      if (o >= 0 && o < (int64_t)B.out_writes.size()) ++B.out_writes[o];
    }
  }
}

static void check_outputs(const Buffers& B, const char* regime) {
  for (int64_t g = 0; g < B.G; ++g) {
    for (int64_t c = 0; c < B.ld_out; ++c)
      CHECK(B.out_writes[g * B.ld_out + c] == (c < B.C ? 1 : 0), "%s: out[%lld, %lld] written %d times", regime, (long long)g,
            (long long)c, B.out_writes[g * B.ld_out + c]);
    CHECK(B.saved_m[g] == 1 && B.saved_z[g] == 1, "%s: saved[%lld] written (%d, %d) times", regime, (long long)g, B.saved_m[g],
          B.saved_z[g]);
  }
}

static void check_batch(int64_t rows, int64_t C, const std::vector<int64_t>& gp, bool sorted_in_range) {
  const int64_t G = (int64_t)gp.size() - 1;
  const Geometry geo = geometry(C);
  std::vector<int> expect_y(rows * C + 1, 0), expect_s(rows + 1, 0);
  for (int64_t g = 0; g < G; ++g) {
    int64_t a, b;
    graph_range(gp.data(), g, rows, a, b);
    CHECK(0 <= a && a <= b && b <= rows, "range of graph %lld", (long long)g);
    for (int64_t i = a * C; i < b * C; ++i) ++expect_y[i];
    for (int64_t i = a; i < b; ++i) ++expect_s[i];
  }
  {  // many-graphs regime: workgroup (g, tile)
    Buffers B(rows, C, G);
    std::vector<int> max_reads(rows + 1, 0);
    for (int64_t g = 0; g < G; ++g) {
      int64_t a, b;
      graph_range(gp.data(), g, rows, a, b);
      for (int tile = 0; tile < geo.col_tiles; ++tile) {
        if (tile == 0) walk_score_max(rows, a, b, max_reads);
        for (int64_t k0 = 0; k0 < b - a; k0 += kChunkRows)
          walk_chunk(geo, B, a, b, a + k0, (int)(b - a - k0 < kChunkRows ? b - a - k0 : kChunkRows), tile);
        walk_out_tile(geo, B, g, tile);
        if (tile == 0) ++B.saved_m[g], ++B.saved_z[g];
      }
    }
    CHECK(B.y_reads == expect_y && B.s_reads == expect_s && max_reads == expect_s,
          "many-graphs regime: a row of a graph is not read exactly once");
    check_outputs(B, "many graphs");
  }
  {  // split regime: the maxima, slots -> chunks, then the merge's enumeration of the same slots
    Buffers B(rows, C, G);
    const int64_t slots = split_slots(rows, G);
    const int64_t ws_floats = gnc_attn::workspace_floats(slots, C);
    std::vector<int> ws(ws_floats + 1, 0), max_reads(rows + 1, 0);
    for (int64_t g = 0; g < G; ++g) {
      int64_t a, b;
      graph_range(gp.data(), g, rows, a, b);
      walk_score_max(rows, a, b, max_reads);
      ++B.saved_m[g];
    }
    int64_t used = 0;
    for (int64_t slot = 0; slot < slots; ++slot) {
      int64_t g, row0;
      int nr;
      if (!slot_chunk(gp.data(), G, rows, slot, g, row0, nr)) continue;
      CHECK(g >= 0 && g < G, "slot %lld names graph %lld", (long long)slot, (long long)g);
      if (g < 0 || g >= G) continue;
      CHECK(B.saved_m[g] == 1, "slot %lld reads a maximum that was not written", (long long)slot);
      int64_t a, b;
      graph_range(gp.data(), g, rows, a, b);
      ++used;
      for (int tile = 0; tile < geo.col_tiles; ++tile) {
        walk_chunk(geo, B, a, b, row0, nr, tile);
        for (int t = 0; t < geo.col_lanes; ++t) {  // row-lane 0 stores the column partials
          const int64_t col0 = ((int64_t)tile * geo.col_lanes + t) * geo.vec;
          for (int u = 0; u < geo.vec && col0 < C; ++u) {
            const int64_t o = gnc_attn::ws_col_index(slot, C, col0 + u);
            CHECK(o >= 0 && o < slots * C, "column partial %lld outside its block", (long long)o);
            if (o >= 0 && o < ws_floats) ++ws[o];
          }
        }
        if (tile == 0) {
          const int64_t o = gnc_attn::ws_z_index(slots, C, slot);
          CHECK(o >= slots * C && o < ws_floats, "Z partial %lld outside its block", (long long)o);
          if (o >= 0 && o < ws_floats) ++ws[o];
        }
      }
    }
    int64_t chunks = 0;
    for (int64_t g = 0; g < G; ++g) {
      int64_t a, b;
      graph_range(gp.data(), g, rows, a, b);
      const int64_t s0 = first_slot(gp.data(), g, rows);
      int64_t s1 = s0 + chunks_of(b - a);
      chunks += chunks_of(b - a);
      if (s1 > slots) s1 = slots;
      for (int64_t c = 0; c < C; ++c) {  // thread (g, c) of the merge
        for (int64_t s = s0; s < s1; ++s) {
          const int64_t oc = gnc_attn::ws_col_index(s, C, c), oz = gnc_attn::ws_z_index(slots, C, s);
          CHECK(oc >= 0 && oc < ws_floats && oz >= 0 && oz < ws_floats && ws[oc] == 1 && ws[oz] == 1,
                "merge of graph %lld reads slot %lld that was not written once", (long long)g, (long long)s);
        }
        ++B.out_writes[g * B.ld_out + c];
      }
      ++B.saved_z[g];
    }
    check_outputs(B, "split");
    CHECK(max_reads == expect_s, "split regime: a score of a graph is not read exactly once by the maxima");
    if (sorted_in_range) {
      CHECK(chunks <= slots && used == chunks, "%lld chunks, %lld slots, %lld written", (long long)chunks, (long long)slots, (long long)used);
      CHECK(B.y_reads == expect_y && B.s_reads == expect_s, "split regime: a row of a graph is not read exactly once");
    }
  }
  {  // backward: `lanes` threads per row; dy written exactly once everywhere, y / dout / out read inside their buffers
    const RowGeometry rg = gnc_attn::row_geometry(C);
    CHECK(rg.lanes >= 1 && rg.lanes <= 64 && (rg.lanes & (rg.lanes - 1)) == 0 && rg.lanes * rg.rows_per_block == kBlockThreads &&
              (rg.vec == 1 || C % 4 == 0),
          "row geometry of C = %lld", (long long)C);
    const int W = rg.lanes, rpb = rg.rows_per_block;
    const int64_t per_row = C / rg.vec, ld = C + 3;
    std::vector<int> dy(rows * C + 1, 0), ds(rows + 1, 0);
    for (int64_t blocks : {(int64_t)1, (int64_t)3, (rows + rpb - 1) / rpb}) {
      if (blocks < 1) continue;
      std::fill(dy.begin(), dy.end(), 0);
      std::fill(ds.begin(), ds.end(), 0);
      for (int64_t blk = 0; blk < blocks; ++blk)
        for (int64_t base = blk * rpb; base < rows; base += blocks * rpb)
          for (int t = 0; t < kBlockThreads; ++t) {
            const int lane = t % W, sub = t / W;
            const int64_t r = base + sub;
            for (int s = W >> 1; s >= 1; s >>= 1)  // the butterfly stays inside the row's own lanes
              CHECK(((t ^ s) / W) == sub && (t ^ s) / 64 == t / 64, "butterfly partner %d of thread %d leaves its row", t ^ s, t);
            if (r >= rows) continue;
            int64_t n = -1;
            const int64_t g = graph_of_row(gp.data(), G, rows, r, n);
            CHECK(g >= -1 && g < G, "row %lld -> graph %lld", (long long)r, (long long)g);
            if (sorted_in_range && lane == 0) {
              int64_t want = -1;
              for (int64_t h = 0; h < G; ++h)
                if (gp[h] <= r && r < gp[h + 1]) want = h;
              CHECK(g == want, "row %lld -> graph %lld, expected %lld", (long long)r, (long long)g, (long long)want);
            }
            for (int64_t k = lane; k < per_row; k += W)
              for (int u = 0; u < rg.vec; ++u) {
                const int64_t c = k * rg.vec + u;
                CHECK(c < C, "column %lld of C = %lld", (long long)c, (long long)C);
                if (g >= 0 && g < G) CHECK(g * ld + c < G * ld, "dout / out index of graph %lld", (long long)g);
                if (c < C) ++dy[r * C + c];
              }
            if (lane == 0) ++ds[r];
          }
      bool once = true;
      for (int64_t i = 0; i < rows * C; ++i) once = once && dy[i] == 1;
      for (int64_t i = 0; i < rows; ++i) once = once && ds[i] == 1;
      CHECK(once, "backward with %lld workgroups: an element of dy or ds is not written exactly once", (long long)blocks);
    }
    // weights launch: one thread per row, grid-stride
    for (int64_t blocks : {(int64_t)1, (rows + kBlockThreads - 1) / kBlockThreads}) {
      if (blocks < 1) continue;
      std::fill(ds.begin(), ds.end(), 0);
      for (int64_t blk = 0; blk < blocks; ++blk)
        for (int t = 0; t < kBlockThreads; ++t)
          for (int64_t r = blk * kBlockThreads + t; r < rows; r += blocks * kBlockThreads) ++ds[r];
      bool once = true;
      for (int64_t i = 0; i < rows; ++i) once = once && ds[i] == 1;
      CHECK(once, "weights launch with %lld workgroups: a row is not written exactly once", (long long)blocks);
    }
  }
}

static std::vector<int64_t> offsets(int64_t first, const std::vector<int64_t>& sizes) {
  std::vector<int64_t> gp{first};
  for (int64_t s : sizes) gp.push_back(gp.back() + s);
  return gp;
}

int main() {
  const int R = kChunkRows;
  const int64_t widths[] = {1, 2, 3, 4, 5, 8, 12, 63, 64, 65, 128, 130, 132, 256, 260, 516};
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
  for (int it = 0; it < 60; ++it) {
    std::vector<int64_t> sizes(1 + std::rand() % 12);
    for (auto& s : sizes) s = (std::rand() % 4 == 0) ? (std::rand() % 4) * R : std::rand() % (3 * R);
    const auto gp = offsets(std::rand() % 3, sizes);
    check_batch(gp.back() + std::rand() % 50, 1 + std::rand() % 140, gp, true);
  }
  std::printf(failures ? "attention_pool_index_check: %d FAILED\n" : "attention_pool_index_check: ok\n", failures);
  return failures ? 1 : 0;
}
