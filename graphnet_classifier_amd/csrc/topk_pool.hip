// K20: top-K node pooling between the GN blocks.  Per graph g of a block-diagonal batch - rows [a, b) of
// graph_ptr, n = b - a - the k_g = min(n, max(1, ceil(ratio n))) rows with the best scores are kept, IN THEIR OLD ORDER, the others
// erased; the destination-sorted edge list is filtered to the edges between kept nodes and renumbered (it stays sorted: new ids
// are monotone in old ids), node rows are compacted through the gate tanh(s_v), edge rows without one.
//
// Order of the scores (total, a pure function of their fp32 bits): larger first, -0.0 == +0.0, NaN below -inf, ties by lower row.
// It is the order of (score_key descending, row ascending) - topk_pool_index.h.
//
// Launches, none with a global atomic, a ticket or a memset; every output element is written by exactly one thread:
//   select   topk_offsets_kernel   one workgroup: k_g from graph_ptr alone, their exclusive scan = graph_ptr', N' = counts[0]
//            topk_select_kernel    one workgroup per graph: radix select (4 passes of 8 bits, a 256-bin LDS histogram per pass) of
//                                  the k_g-th largest key T and of the number of rows with key == T still admitted, then one walk
//                                  over the graph's rows in chunks of 256 with a block scan that hands out new ids; the workgroup
//                                  also marks the rows of no graph around its graph as dropped
//   edges    topk_edge_count_kernel  workgroup = tile of kEdgeTile sorted positions: its number of kept edges
//            topk_tile_scan_kernel   one workgroup: exclusive scan of the tile counts in place, E' = counts[1]
//            topk_edge_write_kernel  the tile again: src', dst', kept_edges, edge_new_id and the exclusive count at every position
//            topk_rowptr_kernel      thread per kept node: rowptr'[v'] = exclusive count at rowptr[v]; rowptr'[N'] = E'
//   rows     topk_rows_forward_kernel / topk_rows_backward_kernel: one streaming pass each, 16-byte accesses at C % 4 == 0; the row
//            tiling is pool_index.h's (row_geometry, row_lane), load_vec / store_vec are graph_reduce.h's
//
// The capacity-padded form (gnc_topk_pool_select_padded_f32 / gnc_topk_pool_filter_edges_padded; the layout is topk_pool_index.h's)
// is the same launches with `padded` set, none added: every array is written over its whole length, so nothing behind N' / E' is
// left to a host read-back.  The select workgroups write kept[N', rows) = -1 between them; topk_edge_write_kernel writes, for each
// of its positions p >= E', the slack self-loop at p and kept_edges[p] = -1 (counts[1] is final before it starts);
// topk_rowptr_kernel covers all rows + 1 entries.  The row launches then run with n_out = rows / E: a -1 id gives a +0.0 row.
#include "graph_reduce.h"
#include "topk_pool_index.h"

#include <math.h>

namespace {

using namespace gnc_topk;
using gnc_pool::graph_range;
using gnc_pool::row_lane;
using gnc_reduce::load_vec;
using gnc_reduce::store_vec;
using gnc::aligned_to;

// Exclusive scan of `v` over the kT threads of the workgroup (thread order) and its total.  Every thread calls it (it synchronises).
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t (&s_wave)[kWaves], uint32_t& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  __syncthreads();  // the previous call's wave sums have been read
  if (lane == 63) s_wave[w] = inc;
  __syncthreads();
  uint32_t base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    const uint32_t x = s_wave[i];
    base += i < w ? x : 0u;
    total += x;
  }
  return base + inc - v;
}

// graph_ptr' [G + 1] and counts[0] = N' from the graphs' sizes alone
__global__ __launch_bounds__(kT) void topk_offsets_kernel(const int64_t* __restrict__ graph_ptr, int64_t G, int64_t rows, double ratio,
                                                          int64_t* __restrict__ new_ptr, int64_t* __restrict__ counts) {
  __shared__ uint32_t s_wave[kWaves];
  int64_t base = 0;
  for (int64_t g0 = 0; g0 < G; g0 += kT) {  // uniform over the workgroup
    const int64_t g = g0 + threadIdx.x;
    uint32_t k = 0;
    if (g < G) {
      int64_t a, b;
      graph_range(graph_ptr, g, rows, a, b);
      k = (uint32_t)keep_count(ratio, b - a);
    }
    uint32_t total;
    const uint32_t ex = block_exclusive_scan(k, s_wave, total);
    if (g < G) new_ptr[g] = base + ex;
    base += total;
  }
  if (threadIdx.x == 0) {
    new_ptr[G] = base;
    counts[0] = base;
  }
}

__device__ __forceinline__ uint32_t key_at(const float* __restrict__ scores, int64_t r) { return score_key(__float_as_uint(scores[r])); }

// workgroup g: the kept set of graph g
__global__ __launch_bounds__(kT) void topk_select_kernel(const float* __restrict__ scores, const int64_t* __restrict__ graph_ptr, int64_t G,
                                                         int64_t rows, double ratio, const int64_t* __restrict__ new_ptr,
                                                         int32_t* __restrict__ new_id, int32_t* __restrict__ kept, int padded) {
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_wave[kWaves];
  __shared__ uint32_t s_sel[2];
  static_assert(kT == 256, "one histogram bin per thread");
  const int t = threadIdx.x;
  const int64_t g = blockIdx.x;
  int64_t a, b, lo, hi, tail;
  graph_range(graph_ptr, g, rows, a, b);
  gap_rows(graph_ptr, g, G, rows, lo, hi, tail);
  for (int64_t r = lo + t; r < hi; r += kT) new_id[r] = -1;
  for (int64_t r = tail + t; r < rows; r += kT) new_id[r] = -1;
  if (padded) {  // uniform; new_ptr[G] = N' is the offsets launch's
    const int64_t n_out = slack_of(new_ptr[G], 0, rows, 0).n_out;
    for (int64_t r = kept_tail_first(n_out, g, t); r < rows; r += kept_tail_stride(G)) kept[r] = -1;
  }
  const int64_t n = b - a;
  if (n == 0) return;  // uniform
  const uint32_t k = (uint32_t)keep_count(ratio, n);
  // T: the k-th largest key; rem: how many of the rows with key == T are kept (the lowest rows first)
  uint32_t T = 0, rem = (uint32_t)n;  // k == n: everything is kept (key 0 = NaN is the smallest key there is)
  if (k < n) {
    uint32_t mask = 0;
    rem = k;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
      s_hist[t] = 0;
      __syncthreads();
      for (int64_t r = a + t; r < b; r += kT) {
        const uint32_t key = key_at(scores, r);
        if ((key & mask) == T) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);  // LDS, integer: the order does not matter
      }
      __syncthreads();
      const uint32_t h = s_hist[255 - t];  // thread t owns digit 255 - t: the scan counts the larger digits
      uint32_t total;
      const uint32_t above = block_exclusive_scan(h, s_wave, total);
      if (above < rem && rem <= above + h) {  // exactly one thread: the candidates number at least rem
        s_sel[0] = 255u - (uint32_t)t;
        s_sel[1] = rem - above;
      }
      __syncthreads();
      T |= s_sel[0] << shift;
      mask |= 255u << shift;
      rem = s_sel[1];
      __syncthreads();  // s_sel and s_hist are free again
    }
  }
  const int64_t out0 = new_ptr[g];
  uint32_t gt_base = 0, eq_base = 0;
  for (int64_t c0 = 0; c0 < n; c0 += kT) {  // uniform
    const bool valid = c0 + t < n;
    const int64_t r = a + c0 + t;
    const uint32_t key = valid ? key_at(scores, r) : 0u;
    const bool gt = valid && key > T, eq = valid && key == T;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan((gt ? 1u : 0u) | (eq ? 0x10000u : 0u), s_wave, total);  // two 16-bit counts <= 256
    const uint32_t gt_before = gt_base + (ex & 0xffffu), eq_before = eq_base + (ex >> 16);
    if (valid) {
      const bool keep = gt || (eq && eq_before < rem);
      const int64_t id = out0 + gt_before + (eq_before < rem ? eq_before : rem);
      new_id[r] = keep ? (int32_t)id : -1;
      if (keep && id < rows) kept[id] = (int32_t)r;  // (id < rows always, unless the offsets overlap)
    }
    gt_base += total & 0xffffu;
    eq_base += total >> 16;
  }
}

struct EdgeArgs {
  const int32_t* src;
  const int32_t* dst;
  const int32_t* new_id;
  int64_t E, rows;
  int32_t* tile;  // [tiles]: counts, then their exclusive scan
  int32_t* excl;  // [E]
  int32_t* src_out;
  int32_t* dst_out;
  int32_t* kept_edges;
  int32_t* edge_new_id;
  const int64_t* counts;  // padded form: [N', E'] (NULL: the sized form, nothing is written at or behind E')
};

// new endpoints of the edge at sorted position p; false: dropped (an endpoint erased, or outside [0, rows): never an index)
__device__ __forceinline__ bool edge_kept(const EdgeArgs& a, int64_t p, int32_t& s, int32_t& d) {
  const int32_t so = a.src[p], dq = a.dst[p];
  if ((uint64_t)(int64_t)so >= (uint64_t)a.rows || (uint64_t)(int64_t)dq >= (uint64_t)a.rows) return false;
  s = a.new_id[so];
  d = a.new_id[dq];
  return s >= 0 && d >= 0;
}

__global__ __launch_bounds__(kT) void topk_edge_count_kernel(const EdgeArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  uint32_t mine = 0;
#pragma unroll
  for (int i = 0; i < kEdgeSteps; ++i) {
    const int64_t p = edge_position(blockIdx.x, i, threadIdx.x);
    int32_t s, d;
    if (p < a.E && edge_kept(a, p, s, d)) ++mine;
  }
  uint32_t total;
  block_exclusive_scan(mine, s_wave, total);
  if (threadIdx.x == 0) a.tile[blockIdx.x] = (int32_t)total;
}

__global__ __launch_bounds__(kT) void topk_tile_scan_kernel(int32_t* __restrict__ tile, int64_t tiles, int64_t* __restrict__ counts) {
  __shared__ uint32_t s_wave[kWaves];
  uint32_t base = 0;
  for (int64_t i0 = 0; i0 < tiles; i0 += kT) {  // uniform
    const int64_t i = i0 + threadIdx.x;
    const uint32_t c = i < tiles ? (uint32_t)tile[i] : 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan(c, s_wave, total);
    if (i < tiles) tile[i] = (int32_t)(base + ex);
    base += total;
  }
  if (threadIdx.x == 0) counts[1] = base;
}

__global__ __launch_bounds__(kT) void topk_edge_write_kernel(const EdgeArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  uint32_t base = (uint32_t)a.tile[blockIdx.x];
  const bool padded = a.counts != nullptr;  // uniform
  const Slack slack = padded ? slack_of(a.counts[0], a.counts[1], a.rows, a.E) : Slack{};
#pragma unroll 1
  for (int i = 0; i < kEdgeSteps; ++i) {  // uniform: positions behind E take part in the scan with a zero
    const int64_t p = edge_position(blockIdx.x, i, threadIdx.x);
    int32_t s = -1, d = -1;
    const bool keep = p < a.E && edge_kept(a, p, s, d);
    uint32_t total;
    const uint32_t j = base + block_exclusive_scan(keep ? 1u : 0u, s_wave, total);
    if (p < a.E) {
      a.excl[p] = (int32_t)j;
      a.edge_new_id[p] = keep ? (int32_t)j : -1;
      if (keep) {  // j < E: at most p kept edges lie in front of position p
        a.src_out[j] = s;
        a.dst_out[j] = d;
        a.kept_edges[j] = (int32_t)p;
      }
      if (padded && p >= slack.e_out) {  // j <= E' - 1 for every kept edge: the slack positions are written here alone
        const int32_t row = (int32_t)slack_edge_row(slack, a.rows, p - slack.e_out);  // in [0, rows): the launcher requires rows >= 1
        a.src_out[p] = row;
        a.dst_out[p] = row;
        a.kept_edges[p] = -1;
      }
    }
    base += total;
  }
}

// thread i < N': rowptr'[i] = kept edges in front of rowptr[kept[i]]; thread N': E'; padded: threads N' < i <= rows, the slack rows' offsets
__global__ __launch_bounds__(kT) void topk_rowptr_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ kept,
                                                         const int32_t* __restrict__ excl, const int64_t* __restrict__ counts, int64_t E,
                                                         int64_t rows, int32_t* __restrict__ rowptr_out, int padded) {
  int64_t n_out = counts[0];
  n_out = n_out < 0 ? 0 : (n_out > rows ? rows : n_out);
  const int32_t e_out = (int32_t)counts[1];
  const int64_t first = (int64_t)blockIdx.x * kT + threadIdx.x, stride = (int64_t)gridDim.x * kT;
  for (int64_t i = first; i <= n_out; i += stride) {
    int32_t value = padded && i == rows ? (int32_t)E : e_out;  // (padded, every row kept: the list still ends at E)
    if (i < n_out) {
      const int32_t v = kept[i];
      const int64_t p = (uint64_t)(int64_t)v < (uint64_t)rows ? (int64_t)rowptr[v] : E;
      if (p >= 0 && p < E) value = excl[p];
      else if (p < 0) value = 0;
    }
    rowptr_out[i] = value;
  }
  if (!padded) return;  // uniform
  const Slack slack = slack_of(n_out, counts[1], rows, E);
  for (int64_t i = n_out + 1 + first; i <= rows; i += stride) rowptr_out[i] = (int32_t)slack_rowptr(slack, rows, E, i);  // arithmetic alone
}

struct RowsArgs {
  const float* x;       // [rows_in, C], pitch ld_x
  const float* scores;  // [rows_in] or NULL (no gate)
  const int32_t* index; // forward: kept [n_out]; backward: new_id [rows_in]
  const float* dout;    // backward: [n_out, C], pitch ld_dout
  float* out;           // forward: [n_out, C], pitch ld_out; backward: dx [rows_in, C], pitch ld_out (may be NULL)
  float* ds;            // backward: [rows_in] (may be NULL)
  int64_t rows_in, n_out, C, ld_x, ld_dout, ld_out;
  int32_t lanes, vec16;  // vec16: every row of every table starts on a 16-byte boundary
};

// out[i, :] = x[index[i], :] * tanh(scores[index[i]]) (no gate: the bits of x); `lanes` threads per row
template <int VEC>
__global__ __launch_bounds__(kT) void topk_rows_forward_kernel(const RowsArgs a) {
  const int W = a.lanes, rpb = kT / W;
  const gnc_pool::RowLane x = row_lane(threadIdx.x, W);
  const int lane = x.lane, sub = x.sub;
  const int64_t per_row = a.C / VEC;
  const bool v16 = a.vec16 != 0;
  for (int64_t i = (int64_t)blockIdx.x * rpb + sub; i < a.n_out; i += (int64_t)gridDim.x * rpb) {
    const int64_t v = a.index[i];
    const bool ok = (uint64_t)v < (uint64_t)a.rows_in;  // an id outside the table reads nothing and gives a zero row
    const float gate = ok && a.scores ? tanhf(a.scores[v]) : 1.f;
    for (int64_t q = lane; q < per_row; q += W) {
      float val[VEC];
#pragma unroll
      for (int u = 0; u < VEC; ++u) val[u] = 0.f;
      if (ok) {
        load_vec<VEC>(a.x + v * a.ld_x + q * VEC, v16, val);
        if (a.scores) {
#pragma unroll
          for (int u = 0; u < VEC; ++u) val[u] *= gate;
        }
      }
      store_vec<VEC>(a.out + i * a.ld_out + q * VEC, v16, val);
    }
  }
}

// dx[r, :] = tanh(s_r) dout[new_id[r], :],  ds[r] = (1 - tanh(s_r)^2) sum_c dout[new_id[r], c] x[r, c];  +0.0 for a dropped row
template <int VEC>
__global__ __launch_bounds__(kT) void topk_rows_backward_kernel(const RowsArgs a) {
  const int W = a.lanes, rpb = kT / W;
  const gnc_pool::RowLane x = row_lane(threadIdx.x, W);
  const int lane = x.lane, sub = x.sub;
  const int64_t per_row = a.C / VEC;
  const bool v16 = a.vec16 != 0;
  for (int64_t base = (int64_t)blockIdx.x * rpb; base < a.rows_in; base += (int64_t)gridDim.x * rpb) {  // uniform
    const int64_t r = base + sub;
    const bool valid = r < a.rows_in;
    const int64_t j = valid ? (int64_t)a.index[r] : -1;
    const bool keptrow = j >= 0 && j < a.n_out;
    const float gate = keptrow && a.scores ? tanhf(a.scores[r]) : 1.f;
    float dot = 0.f;
    if (valid) {
      for (int64_t q = lane; q < per_row; q += W) {
        float g[VEC];
#pragma unroll
        for (int u = 0; u < VEC; ++u) g[u] = 0.f;
        if (keptrow) {
          load_vec<VEC>(a.dout + j * a.ld_dout + q * VEC, v16, g);
          if (a.ds) {
            float xv[VEC];
            load_vec<VEC>(a.x + r * a.ld_x + q * VEC, v16, xv);
#pragma unroll
            for (int u = 0; u < VEC; ++u) dot = fmaf(g[u], xv[u], dot);
          }
          if (a.scores) {
#pragma unroll
            for (int u = 0; u < VEC; ++u) g[u] *= gate;
          }
        }
        if (a.out) store_vec<VEC>(a.out + r * a.ld_out + q * VEC, v16, g);
      }
    }
    if (a.ds) {  // uniform: every lane of the workgroup takes part in the butterfly
      for (int s = W >> 1; s >= 1; s >>= 1) dot += __shfl_xor(dot, s, W);
      if (valid && lane == 0) a.ds[r] = keptrow ? (1.f - gate * gate) * dot : 0.f;
    }
  }
}

constexpr int64_t kMaxRows = (1ll << 31) - 1;

}  // namespace

namespace {

int select_launch(const char* who, const float* scores, const int64_t* graph_ptr, int64_t num_graphs, int64_t rows, double ratio, int32_t* new_id,
                  int32_t* kept, int64_t* new_graph_ptr, int64_t* counts, void* stream, int padded) {
  GNC_REQUIRE(rows >= 0 && rows <= kMaxRows && num_graphs >= 1 && num_graphs <= kMaxRows,
              "%s: rows %lld / graphs %lld outside the supported set (0 <= rows < 2^31, 1 <= graphs < 2^31)", who,
              (long long)rows, (long long)num_graphs);
  GNC_REQUIRE(ratio > 0.0 && ratio <= 1.0, "%s: ratio %g is not in (0, 1]", who, ratio);
  GNC_REQUIRE(graph_ptr && new_graph_ptr && counts && ((scores && new_id && kept) || rows == 0),
              "%s: null scores / graph_ptr / new_id / kept / new_graph_ptr / counts", who);
  GNC_REQUIRE(aligned_to(scores, 4) && aligned_to(new_id, 4) && aligned_to(kept, 4) && aligned_to(graph_ptr, 8) &&
                  aligned_to(new_graph_ptr, 8) && aligned_to(counts, 8),
              "%s: a pointer is not aligned to its element size", who);
  hipStream_t st = static_cast<hipStream_t>(stream);
  topk_offsets_kernel<<<dim3(1), dim3(kT), 0, st>>>(graph_ptr, num_graphs, rows, ratio, new_graph_ptr, counts);
  if (int rc = gnc::check_launch("topk_offsets_kernel")) return rc;
  if (rows == 0) return GNC_OK;
  topk_select_kernel<<<dim3((unsigned)num_graphs), dim3(kT), 0, st>>>(scores, graph_ptr, num_graphs, rows, ratio, new_graph_ptr, new_id,
                                                                       kept, padded);
  return gnc::check_launch("topk_select_kernel");
}

}  // namespace

extern "C" int gnc_topk_pool_select_f32(const float* scores, const int64_t* graph_ptr, int64_t num_graphs, int64_t rows, double ratio,
                                        int32_t* new_id, int32_t* kept, int64_t* new_graph_ptr, int64_t* counts, void* stream) {
  return select_launch("gnc_topk_pool_select_f32", scores, graph_ptr, num_graphs, rows, ratio, new_id, kept, new_graph_ptr, counts, stream, 0);
}

// The padded form: the same two launches; kept[N', rows) = -1 as well, so all `rows` entries of `kept` are defined.
extern "C" int gnc_topk_pool_select_padded_f32(const float* scores, const int64_t* graph_ptr, int64_t num_graphs, int64_t rows,
                                               double ratio, int32_t* new_id, int32_t* kept, int64_t* new_graph_ptr, int64_t* counts,
                                               void* stream) {
  return select_launch("gnc_topk_pool_select_padded_f32", scores, graph_ptr, num_graphs, rows, ratio, new_id, kept, new_graph_ptr, counts, stream,
                       1);
}

extern "C" int64_t gnc_topk_pool_edge_workspace_ints(int64_t num_edges) {
  return num_edges < 0 || num_edges > kMaxRows ? -1 : edge_workspace_ints(num_edges);
}

namespace {

int filter_launch(const char* who, const int32_t* src_sorted, const int32_t* dst_sorted, const int32_t* rowptr, int64_t num_edges, int64_t rows,
                  const int32_t* new_id, const int32_t* kept, int64_t* counts, int32_t* src_out, int32_t* dst_out, int32_t* kept_edges,
                  int32_t* edge_new_id, int32_t* rowptr_out, int32_t* workspace, int64_t workspace_ints, void* stream, int padded) {
  GNC_REQUIRE(rows >= 0 && rows <= kMaxRows && num_edges >= 0 && num_edges <= kMaxRows,
              "%s: rows %lld / edges %lld outside the supported set (both in [0, 2^31))", who, (long long)rows,
              (long long)num_edges);
  GNC_REQUIRE(counts && rowptr_out && ((rowptr && new_id && kept) || rows == 0),
              "%s: null rowptr / new_id / kept / counts / rowptr_out", who);
  GNC_REQUIRE((src_sorted && dst_sorted && src_out && dst_out && kept_edges && edge_new_id) || num_edges == 0,
              "%s: null src_sorted / dst_sorted / src_out / dst_out / kept_edges / edge_new_id", who);
  const int64_t need = edge_workspace_ints(num_edges);
  GNC_REQUIRE(need == 0 || (workspace && workspace_ints >= need), "%s: the workspace needs %lld ints", who, (long long)need);
  GNC_REQUIRE(aligned_to(src_sorted, 4) && aligned_to(dst_sorted, 4) && aligned_to(rowptr, 4) && aligned_to(new_id, 4) && aligned_to(kept, 4) &&
                  aligned_to(src_out, 4) && aligned_to(dst_out, 4) && aligned_to(kept_edges, 4) && aligned_to(edge_new_id, 4) &&
                  aligned_to(rowptr_out, 4) && aligned_to(workspace, 4) && aligned_to(counts, 8),
              "%s: a pointer is not aligned to its element size", who);
  if (padded && rows == 0) return GNC_OK;  // no row a slack edge could loop on: nothing is launched
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t tiles = edge_tiles(num_edges);
  EdgeArgs a = {};
  a.src = src_sorted, a.dst = dst_sorted, a.new_id = new_id, a.E = num_edges, a.rows = rows;
  a.tile = workspace, a.excl = workspace ? workspace + tiles : nullptr;
  a.src_out = src_out, a.dst_out = dst_out, a.kept_edges = kept_edges, a.edge_new_id = edge_new_id;
  a.counts = padded ? counts : nullptr;
  if (tiles > 0) {
    topk_edge_count_kernel<<<dim3((unsigned)tiles), dim3(kT), 0, st>>>(a);
    if (int rc = gnc::check_launch("topk_edge_count_kernel")) return rc;
  }
  topk_tile_scan_kernel<<<dim3(1), dim3(kT), 0, st>>>(a.tile, tiles, counts);
  if (int rc = gnc::check_launch("topk_tile_scan_kernel")) return rc;
  if (tiles > 0) {
    topk_edge_write_kernel<<<dim3((unsigned)tiles), dim3(kT), 0, st>>>(a);
    if (int rc = gnc::check_launch("topk_edge_write_kernel")) return rc;
  }
  topk_rowptr_kernel<<<dim3((unsigned)gnc::capped_blocks(rows + 1, kT)), dim3(kT), 0, st>>>(rowptr, kept, a.excl, counts, num_edges, rows,
                                                                                     rowptr_out, padded);
  return gnc::check_launch("topk_rowptr_kernel");
}

}  // namespace

extern "C" int gnc_topk_pool_filter_edges(const int32_t* src_sorted, const int32_t* dst_sorted, const int32_t* rowptr, int64_t num_edges,
                                          int64_t rows, const int32_t* new_id, const int32_t* kept, int64_t* counts, int32_t* src_out,
                                          int32_t* dst_out, int32_t* kept_edges, int32_t* edge_new_id, int32_t* rowptr_out,
                                          int32_t* workspace, int64_t workspace_ints, void* stream) {
  return filter_launch("gnc_topk_pool_filter_edges", src_sorted, dst_sorted, rowptr, num_edges, rows, new_id, kept, counts, src_out, dst_out,
                       kept_edges, edge_new_id, rowptr_out, workspace, workspace_ints, stream, 0);
}

// The padded form: the same four launches; src_out / dst_out / kept_edges are written over all E entries (slack self-loops and -1
// at and behind E') and rowptr_out over all rows + 1, ending at E.  `kept` is gnc_topk_pool_select_padded_f32's.
extern "C" int gnc_topk_pool_filter_edges_padded(const int32_t* src_sorted, const int32_t* dst_sorted, const int32_t* rowptr,
                                                 int64_t num_edges, int64_t rows, const int32_t* new_id, const int32_t* kept,
                                                 int64_t* counts, int32_t* src_out, int32_t* dst_out, int32_t* kept_edges,
                                                 int32_t* edge_new_id, int32_t* rowptr_out, int32_t* workspace, int64_t workspace_ints,
                                                 void* stream) {
  return filter_launch("gnc_topk_pool_filter_edges_padded", src_sorted, dst_sorted, rowptr, num_edges, rows, new_id, kept, counts, src_out,
                       dst_out, kept_edges, edge_new_id, rowptr_out, workspace, workspace_ints, stream, 1);
}

namespace {

// the shared argument checks and geometry of the two row launches; GNC_OK + done = true: nothing to launch
int rows_args(const char* who, const float* x, int64_t ld_x, const float* scores, const int32_t* index, const float* dout, int64_t ld_dout,
              float* out, int64_t ld_out, float* ds, int64_t rows_in, int64_t n_out, int64_t C, RowsArgs& a, int& vec) {
  GNC_REQUIRE(rows_in >= 0 && rows_in <= kMaxRows && n_out >= 0 && n_out <= rows_in && C >= 1 && C <= (1 << 20),
              "%s: rows %lld / kept rows %lld / C %lld outside the supported set (0 <= kept <= rows < 2^31, 1 <= C <= 2^20)", who,
              (long long)rows_in, (long long)n_out, (long long)C);
  GNC_REQUIRE((!x || ld_x >= C) && (!dout || ld_dout >= C) && (!out || ld_out >= C), "%s: a leading dimension is smaller than C", who);
  GNC_REQUIRE(aligned_to(x, 4) && aligned_to(scores, 4) && aligned_to(index, 4) && aligned_to(dout, 4) && aligned_to(out, 4) && aligned_to(ds, 4),
              "%s: a pointer is not aligned to its element size", who);
  const RowGeometry geo = row_geometry(C);
  a = RowsArgs{};
  a.x = x, a.scores = scores, a.index = index, a.dout = dout, a.out = out, a.ds = ds;
  a.rows_in = rows_in, a.n_out = n_out, a.C = C, a.ld_x = ld_x, a.ld_dout = ld_dout, a.ld_out = ld_out;
  a.lanes = geo.lanes;
  a.vec16 = (!x || (gnc::aligned16(x) && ld_x % 4 == 0)) && (!dout || (gnc::aligned16(dout) && ld_dout % 4 == 0)) &&
                    (!out || (gnc::aligned16(out) && ld_out % 4 == 0))
                ? 1
                : 0;
  vec = geo.vec;
  return GNC_OK;
}

}  // namespace

extern "C" int gnc_topk_pool_rows_forward_f32(const float* x, int64_t ld_x, int64_t rows_in, int64_t C, const int32_t* kept, int64_t n_out,
                                              const float* scores, float* out, int64_t ld_out, void* stream) {
  RowsArgs a;
  int vec;
  if (int rc = rows_args("gnc_topk_pool_rows_forward_f32", x, ld_x, scores, kept, nullptr, 0, out, ld_out, nullptr, rows_in, n_out, C, a, vec))
    return rc;
  GNC_REQUIRE((x && kept && out) || n_out == 0, "gnc_topk_pool_rows_forward_f32: null x / kept / out");
  if (n_out == 0) return GNC_OK;
  const dim3 grid((unsigned)gnc::capped_blocks(n_out, kT / a.lanes)), block(kT);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec == 4) topk_rows_forward_kernel<4><<<grid, block, 0, st>>>(a);
  else topk_rows_forward_kernel<1><<<grid, block, 0, st>>>(a);
  return gnc::check_launch("topk_rows_forward_kernel");
}

extern "C" int gnc_topk_pool_rows_backward_f32(const float* dout, int64_t ld_dout, int64_t n_out, const float* x, int64_t ld_x,
                                               const float* scores, const int32_t* new_id, int64_t rows_in, int64_t C, float* dx,
                                               int64_t ld_dx, float* ds, void* stream) {
  RowsArgs a;
  int vec;
  if (int rc = rows_args("gnc_topk_pool_rows_backward_f32", ds ? x : nullptr, ld_x, scores, new_id, dout, ld_dout, dx, ld_dx, ds, rows_in, n_out,
                         C, a, vec))
    return rc;
  GNC_REQUIRE(dx || ds, "gnc_topk_pool_rows_backward_f32: no gradient wanted");
  GNC_REQUIRE(!ds || scores, "gnc_topk_pool_rows_backward_f32: ds belongs to the gated form (scores is null)");
  GNC_REQUIRE((new_id && (!ds || x)) || rows_in == 0, "gnc_topk_pool_rows_backward_f32: null new_id / x");
  GNC_REQUIRE(dout || n_out == 0, "gnc_topk_pool_rows_backward_f32: null dout");
  if (rows_in == 0) return GNC_OK;
  const dim3 grid((unsigned)gnc::capped_blocks(rows_in, kT / a.lanes)), block(kT);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec == 4) topk_rows_backward_kernel<4><<<grid, block, 0, st>>>(a);
  else topk_rows_backward_kernel<1><<<grid, block, 0, st>>>(a);
  return gnc::check_launch("topk_rows_backward_kernel");
}
