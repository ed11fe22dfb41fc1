// Host walk of K19's index arithmetic (graphnet_classifier_amd/csrc/attention_pool_index.h over csrc/pool_index.h): for a set of
// batches - empty graphs, graphs whose row count is an exact multiple of the chunk length, slack rows, offsets that point outside
// the table - every (workgroup, thread) of the forward launches of both regimes, of the backward launch and of the weights launch
// is enumerated through the functions the kernels call (tools/pool_walk.h), every address they would form is checked against the
// buffers, and every workspace slot the merge reads is checked to have been written.  Exit status 0 = every check held.
//   c++ -std=c++17 -O1 -fsanitize=address,undefined -I graphnet_classifier_amd/csrc -I tools tools/attention_pool_index_check.cpp \
//       -o attention_pool_index_check && ./attention_pool_index_check
#include <algorithm>

#include "attention_pool_index.h"
#include "pool_walk.h"

using namespace pool_walk;

struct Buffers {
  int64_t rows, C, G, ld_out;
  std::vector<int> y_reads, s_reads, max_reads;  // [rows * C], [rows], [rows]: reads by the chunk walks and by the maxima
  std::vector<int> out_writes;                   // [G * ld_out]
  std::vector<int> saved_m, saved_z;             // [G] each: writes
  Buffers(int64_t rows_, int64_t C_, int64_t G_)
      : rows(rows_), C(C_), G(G_), ld_out(C_ + 3), y_reads(rows_ * C_ + 1, 0), s_reads(rows_ + 1, 0), max_reads(rows_ + 1, 0),
        out_writes(G_ * (C_ + 3), 0), saved_m(G_, 0), saved_z(G_, 0) {}
  // chunk_reduce's reads: VEC columns of y per thread, the row's score (every column lane reads the same one; counted once)
  auto visitor(int vec) {
    return [this, vec](int64_t row, int tile, const Tile& x) {
      for (int u = 0; u < vec; ++u) ++y_reads[row * C + x.col0 + u];
      if (tile == 0 && x.cl == 0) ++s_reads[row];
    };
  }
};

// block_score_max: scores[a, b) strided over the workgroup, then the LDS tree; the maximum is stored to saved[2 g]
static void walk_score_max(Buffers& B, int64_t g, int64_t a, int64_t b) {
  for (int t = 0; t < kBlockThreads; ++t) {
    for (int64_t r = a + t; r < b; r += kBlockThreads) {
      CHECK(r >= 0 && r < B.rows, "score %lld outside [0, %lld)", (long long)r, (long long)B.rows);
      if (r >= 0 && r < B.rows) ++B.max_reads[r];
    }
    for (int w = kBlockThreads >> 1; w >= 1; w >>= 1)
      if (t < w) CHECK(t + w < kBlockThreads, "tree partner %d outside the workgroup", t + w);
  }
  ++B.saved_m[g];
}

// the columns that the threads of row-lane 0 of column tile `tile` store: index(c) is where column c goes, into a table of `size`
template <class Index>
static void walk_tile_stores(const Geometry& geo, int64_t C, int tile, std::vector<int>& writes, int64_t size, Index index) {
  for (int t = 0; t < geo.col_lanes; ++t) {  // row-lane 0
    const Tile x = tile_of(t, tile, geo);
    CHECK(x.rl == 0, "thread %d is not of row-lane 0", t);
    for (int u = 0; u < geo.vec && x.col0 < C; ++u) {
      const int64_t o = index(x.col0 + u);
      CHECK(o >= 0 && o < size && x.col0 + u < C, "store index %lld", (long long)o);
      if (o >= 0 && o < size) ++writes[o];
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

static void check_batch(int64_t rows, int64_t C, const Offsets& gp, bool sorted_in_range) {
  const int64_t G = (int64_t)gp.size() - 1;
  const Geometry geo = geometry(C);
  const std::vector<int> expect_y = expected_reads(rows, C, gp), expect_s = expected_reads(rows, 1, gp);
  {  // many-graphs regime: workgroup (g, tile) forms the maximum (tile 0 stores it), walks the chunks, stores out (tile 0: Z too)
    Buffers B(rows, C, G);
    walk_graph_owned(geo, rows, C, gp, B.visitor(geo.vec), [&](int64_t g, int64_t a, int64_t b, int tile) {
      if (tile == 0) walk_score_max(B, g, a, b), ++B.saved_z[g];
      walk_tile_stores(geo, C, tile, B.out_writes, (int64_t)B.out_writes.size(), [&](int64_t c) { return g * B.ld_out + c; });
    });
    CHECK(B.y_reads == expect_y && B.s_reads == expect_s && B.max_reads == expect_s,
          "many-graphs regime: a row of a graph is not read exactly once");
    check_outputs(B, "many graphs");
  }
  {  // split regime: the maxima, slots -> chunks, then the merge's enumeration of the same slots
    Buffers B(rows, C, G);
    const int64_t slots = split_slots(rows, G), ws_floats = gnc_attn::workspace_floats(slots, C);
    std::vector<int> ws(ws_floats + 1, 0);
    for (int64_t g = 0; g < G; ++g) {
      int64_t a, b;
      graph_range(gp.data(), g, rows, a, b);
      walk_score_max(B, g, a, b);
    }
    walk_split(
        geo, rows, C, gp, sorted_in_range, B.visitor(geo.vec),
        [&](int64_t slot, int64_t g) { CHECK(B.saved_m[g] == 1, "slot %lld reads a maximum that was not written", (long long)slot); },
        [&](int64_t slot, int64_t, int tile) {
          walk_tile_stores(geo, C, tile, ws, slots * C, [&](int64_t c) { return gnc_attn::ws_col_index(slot, C, c); });
          if (tile != 0) return;
          const int64_t o = gnc_attn::ws_z_index(slots, C, slot);
          CHECK(o >= slots * C && o < ws_floats, "Z partial %lld outside its block", (long long)o);
          if (o >= 0 && o < ws_floats) ++ws[o];
        },
        [&](int64_t g, int64_t, int64_t s0, int64_t s1) {
          for (int64_t c = 0; c < C; ++c) {  // thread (g, c) of the merge
            for (int64_t s = s0; s < s1; ++s) {
              const int64_t oc = gnc_attn::ws_col_index(s, C, c), oz = gnc_attn::ws_z_index(slots, C, s);
              CHECK(oc >= 0 && oc < ws_floats && oz >= 0 && oz < ws_floats && ws[oc] == 1 && ws[oz] == 1,
                    "merge of graph %lld reads slot %lld that was not written once", (long long)g, (long long)s);
            }
            ++B.out_writes[g * B.ld_out + c];
          }
          ++B.saved_z[g];
        });
    check_outputs(B, "split");
    CHECK(B.max_reads == expect_s, "split regime: a score of a graph is not read exactly once by the maxima");
    if (sorted_in_range) CHECK(B.y_reads == expect_y && B.s_reads == expect_s, "split regime: a row of a graph is not read exactly once");
  }
  {  // backward: `lanes` threads per row; dy and ds written exactly once everywhere, y / dout / out read inside their buffers
    const RowGeometry rg = row_geometry(C);
    const int64_t ld = C + 3;
    std::vector<int> dy(rows * C + 1, 0), ds(rows + 1, 0);
    for (int64_t blocks : {(int64_t)1, (int64_t)3, (rows + rg.rows_per_block - 1) / rg.rows_per_block}) {
      if (blocks < 1) continue;
      std::fill(dy.begin(), dy.end(), 0);
      std::fill(ds.begin(), ds.end(), 0);
      walk_row_tiles(
          rg, rows, C, blocks,
          [&](int64_t r, int64_t c) {
            const int64_t g = check_graph_of_row(gp, rows, r, sorted_in_range && c == 0);
            CHECK(c < C, "column %lld of C = %lld", (long long)c, (long long)C);
            if (g >= 0 && g < G) CHECK(g * ld + c < G * ld, "dout / out index of graph %lld", (long long)g);
            if (c < C) ++dy[r * C + c];
          },
          [&](int64_t r) { ++ds[r]; });
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

int main() {
  standard_batches({1, 2, 3, 4, 5, 8, 12, 63, 64, 65, 128, 130, 132, 256, 260, 516}, 60, check_batch);
  return finish("attention_pool_index_check");
}
