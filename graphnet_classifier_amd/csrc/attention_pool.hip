// K19: attention read-out.  Per graph g of a block-diagonal batch - rows [graph_ptr[g], graph_ptr[g + 1]) of y [rows, C] with one
// score per row - the softmax of the graph's scores and the column sums of y weighted by it:
//   m_g = max_v s_v,  e_v = expf(s_v - m_g),  Z_g = sum_v e_v,  out[g, c] = (sum_v e_v y[v, c]) / Z_g
// and the backward  dy[v, :] = alpha_v dout[g, :],  ds[v] = alpha_v sum_c dout[g, c] (y[v, c] - out[g, c]),  alpha_v = e_v / Z_g.
//
// Rules: an empty graph pools to +0.0 and nothing is divided; rows of no graph are never read and get +0.0 gradients.  The forward
// keeps (m_g, Z_g) per graph ([G, 2] floats); the backward recomputes alpha_v from them, no [rows] array is stored.  A non-finite
// score stays inside its graph: fmaxf drops a NaN from m_g, expf(NaN - m_g) makes Z_g and every column of that graph NaN.
//
// Summation order: K17's (csrc/pool_readout.hip), for Z_g and for the weighted column sums alike - chunks of kChunkRows rows
// counted from the graph's own first row; inside a chunk row-lane l adds rows l, l + L, ... in ascending order onto +0.0 (the
// product e_v y[v, c] enters by ONE fmaf, in chunk_reduce, which both regimes call), the L lane sums are folded by the halving
// tree, the chunk sums in ascending order onto +0.0.  The maximum is exact in any order.  Both regimes therefore give the same
// bits, as does a graph pooled alone or inside any batch:
//   * many graphs: one workgroup per (graph, column tile) forms the graph's maximum and walks its chunks itself;
//   * few large graphs (split): a launch of one workgroup per graph forms the maxima, one workgroup per (chunk, column tile) writes
//     its partial Z and column sums to a workspace slot, a merge launch folds each graph's slots in ascending order and divides.
// No atomics, no ticket counters; the regime comes from gnc_graph_pool_plan (rows, C, G alone).
#include "gnc_common.h"
#include "attention_pool_index.h"

#include <math.h>

namespace {

using namespace gnc_pool;

constexpr int kT = kBlockThreads;

struct AttnArgs {
  const float* y;
  const float* scores;
  const int64_t* graph_ptr;
  int64_t rows, C, G;
  float* out;
  int64_t ld_out;
  float* saved;   // [G, 2]: (m_g, Z_g); (0, 0) for an empty graph
  float* ws_col;  // split regime: [slots, C]
  float* ws_z;    // split regime: [slots]
  int64_t slots;
  int32_t col_lanes, row_lanes;  // Geometry of C
  int32_t y16;                   // y is 16-byte aligned (vec 4: one dwordx4 load per row and thread)
};

template <int VEC>
__device__ __forceinline__ void load_cols(const float* __restrict__ p, bool p16, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    if (p16) {
      const float4 q = *reinterpret_cast<const float4*>(p);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
      return;
    }
  }
#pragma unroll
  for (int u = 0; u < VEC; ++u) v[u] = p[u];
}

// alpha_v from the saved (m_g, Z_g): the backward and the weights launch share it
__device__ __forceinline__ float softmax_weight(float s, float m, float Z) { return expf(s - m) / Z; }

// Maximum of scores[a, b) (-inf for no rows), returned to every thread of the workgroup; every thread calls it (it synchronises).
__device__ __forceinline__ float block_score_max(const float* __restrict__ scores, int64_t a, int64_t b, float (&s_red)[kT]) {
  const int t = threadIdx.x;
  float m = -INFINITY;
  for (int64_t r = a + t; r < b; r += kT) m = fmaxf(m, scores[r]);
  s_red[t] = m;
  for (int w = kT >> 1; w >= 1; w >>= 1) {
    __syncthreads();
    if (t < w) s_red[t] = m = fmaxf(m, s_red[t + w]);
  }
  __syncthreads();
  m = s_red[0];
  __syncthreads();  // s_red is free again
  return m;
}

// Z and the weighted column sums of rows [row0, row0 + nr) of the workgroup's column tile; the result is in the threads of
// row-lane 0.  Every thread of the workgroup calls it (it synchronises); a thread whose columns lie behind C contributes nothing.
template <int VEC>
__device__ __forceinline__ void chunk_reduce(const AttnArgs& a, float m, int64_t row0, int nr, int64_t col0, bool active, int rl,
                                             float (&s_acc)[VEC][kT], float (&s_z)[kT], float (&acc)[VEC], float& z) {
  const int t = threadIdx.x;
  const int L = a.row_lanes, CL = a.col_lanes;
#pragma unroll
  for (int u = 0; u < VEC; ++u) acc[u] = 0.f;
  z = 0.f;
  if (active) {
    const float* __restrict__ base = a.y + row0 * a.C + col0;
    const float* __restrict__ sc = a.scores + row0;
#pragma unroll 4
    for (int r = rl; r < nr; r += L) {
      const float e = expf(sc[r] - m);
      float v[VEC];
      load_cols<VEC>(base + (int64_t)r * a.C, a.y16 != 0, v);
      z += e;
#pragma unroll
      for (int u = 0; u < VEC; ++u) acc[u] = fmaf(e, v[u], acc[u]);
    }
  }
  __syncthreads();  // the previous chunk's tree has been read
#pragma unroll
  for (int u = 0; u < VEC; ++u) s_acc[u][t] = acc[u];
  s_z[t] = z;
  for (int s = L >> 1; s >= 1; s >>= 1) {
    __syncthreads();
    if (rl < s) {
      const int o = t + s * CL;  // row-lane rl + s, same columns
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        acc[u] += s_acc[u][o];
        s_acc[u][t] = acc[u];
      }
      z += s_z[o];
      s_z[t] = z;
    }
  }
}

// many graphs: workgroup (g, column tile)
template <int VEC>
__global__ __launch_bounds__(kT) void attn_graphs_kernel(const AttnArgs a) {
  __shared__ float s_acc[VEC][kT];
  __shared__ float s_z[kT];
  const int t = threadIdx.x, cl = t % a.col_lanes, rl = t / a.col_lanes;
  const int64_t g = blockIdx.x;
  const int64_t col0 = ((int64_t)blockIdx.y * a.col_lanes + cl) * VEC;
  const bool active = col0 < a.C;  // vec 4: C is a multiple of 4, so col0 + 3 < C as well
  int64_t ra, rb;
  graph_range(a.graph_ptr, g, a.rows, ra, rb);
  const int64_t n = rb - ra;
  const float m = block_score_max(a.scores, ra, rb, s_z);
  float tot[VEC], Z = 0.f;
#pragma unroll
  for (int u = 0; u < VEC; ++u) tot[u] = 0.f;
  for (int64_t k0 = 0; k0 < n; k0 += kChunkRows) {
    const int nr = (int)(n - k0 < kChunkRows ? n - k0 : kChunkRows);
    float acc[VEC], z;
    chunk_reduce<VEC>(a, m, ra + k0, nr, col0, active, rl, s_acc, s_z, acc, z);
#pragma unroll
    for (int u = 0; u < VEC; ++u) tot[u] += acc[u];
    Z += z;
  }
  if (rl == 0 && active) {
#pragma unroll
    for (int u = 0; u < VEC; ++u) a.out[g * a.ld_out + col0 + u] = n > 0 ? tot[u] / Z : 0.f;
  }
  if (t == 0 && blockIdx.y == 0) {  // thread 0 is row-lane 0 of column 0: always active
    a.saved[2 * g] = n > 0 ? m : 0.f;
    a.saved[2 * g + 1] = n > 0 ? Z : 0.f;
  }
}

// split regime, first launch: workgroup g -> m_g
__global__ __launch_bounds__(kT) void attn_max_kernel(const AttnArgs a) {
  __shared__ float s_red[kT];
  const int64_t g = blockIdx.x;
  int64_t ra, rb;
  graph_range(a.graph_ptr, g, a.rows, ra, rb);
  const float m = block_score_max(a.scores, ra, rb, s_red);
  if (threadIdx.x == 0) a.saved[2 * g] = rb > ra ? m : 0.f;
}

// split regime, second launch: workgroup (slot, column tile) -> the chunk's partials
template <int VEC>
__global__ __launch_bounds__(kT) void attn_chunks_kernel(const AttnArgs a) {
  __shared__ float s_acc[VEC][kT];
  __shared__ float s_z[kT];
  const int t = threadIdx.x, cl = t % a.col_lanes, rl = t / a.col_lanes;
  const int64_t slot = blockIdx.x;
  const int64_t col0 = ((int64_t)blockIdx.y * a.col_lanes + cl) * VEC;
  const bool active = col0 < a.C;
  int64_t g, row0;
  int nr;
  if (slot >= a.slots || !slot_chunk(a.graph_ptr, a.G, a.rows, slot, g, row0, nr)) return;  // uniform over the workgroup
  const float m = a.saved[2 * g];
  float acc[VEC], z;
  chunk_reduce<VEC>(a, m, row0, nr, col0, active, rl, s_acc, s_z, acc, z);
  if (rl == 0 && active) {
#pragma unroll
    for (int u = 0; u < VEC; ++u) a.ws_col[gnc_attn::ws_col_index(slot, a.C, col0 + u)] = acc[u];
  }
  if (t == 0 && blockIdx.y == 0) a.ws_z[slot] = z;
}

// split regime, third launch: thread (g, c) folds the graph's slots in ascending order and divides
__global__ __launch_bounds__(kT) void attn_merge_kernel(const AttnArgs a) {
  const int64_t g = blockIdx.x;
  const int64_t c = (int64_t)blockIdx.y * kT + threadIdx.x;
  if (c >= a.C) return;
  int64_t ra, rb;
  graph_range(a.graph_ptr, g, a.rows, ra, rb);
  const int64_t n = rb - ra;
  const int64_t s0 = first_slot(a.graph_ptr, g, a.rows);
  int64_t s1 = s0 + chunks_of(n);
  if (s1 > a.slots) s1 = a.slots;  // offsets that overlap: only the slots that exist (and were written)
  float tot = 0.f, Z = 0.f;
  for (int64_t s = s0; s < s1; ++s) {
    tot += a.ws_col[gnc_attn::ws_col_index(s, a.C, c)];
    Z += a.ws_z[s];
  }
  a.out[g * a.ld_out + c] = n > 0 ? tot / Z : 0.f;
  if (c == 0) a.saved[2 * g + 1] = n > 0 ? Z : 0.f;
}

struct AttnBwdArgs {
  const float* dout;
  const float* y;  // NULL without ds
  const float* scores;
  const float* out;  // NULL without ds
  const float* saved;
  const int64_t* graph_ptr;
  int64_t rows, C, G, ld_dout, ld_out;
  float* dy;  // either may be NULL
  float* ds;
  int32_t lanes, y16, dy16;
};

// backward: `lanes` threads per row, kT / lanes rows per workgroup and pass; the row loop is uniform over the workgroup
template <int VEC>
__global__ __launch_bounds__(kT) void attn_backward_kernel(const AttnBwdArgs a) {
  const int W = a.lanes, rpb = kT / W;
  const int lane = threadIdx.x % W, sub = threadIdx.x / W;
  const int64_t per_row = a.C / VEC;
  for (int64_t base = (int64_t)blockIdx.x * rpb; base < a.rows; base += (int64_t)gridDim.x * rpb) {
    const int64_t r = base + sub;
    const bool valid = r < a.rows;
    int64_t n = 0;
    const int64_t g = valid ? graph_of_row(a.graph_ptr, a.G, a.rows, r, n) : -1;
    const float alpha = g >= 0 ? softmax_weight(a.scores[r], a.saved[2 * g], a.saved[2 * g + 1]) : 0.f;
    float dot = 0.f;
    if (valid) {
      for (int64_t k = lane; k < per_row; k += W) {
        const int64_t c0 = k * VEC;
        float dv[VEC];
#pragma unroll
        for (int u = 0; u < VEC; ++u) dv[u] = 0.f;
        if (g >= 0) {
          float go[VEC];
#pragma unroll
          for (int u = 0; u < VEC; ++u) go[u] = a.dout[g * a.ld_dout + c0 + u];
          if (a.ds) {
            float v[VEC];
            load_cols<VEC>(a.y + r * a.C + c0, a.y16 != 0, v);
#pragma unroll
            for (int u = 0; u < VEC; ++u) dot = fmaf(go[u], v[u] - a.out[g * a.ld_out + c0 + u], dot);
          }
#pragma unroll
          for (int u = 0; u < VEC; ++u) dv[u] = alpha * go[u];
        }
        if (a.dy) {
          float* __restrict__ p = a.dy + r * a.C + c0;
          bool stored = false;
          if constexpr (VEC == 4) {
            if (a.dy16) {
              *reinterpret_cast<float4*>(p) = make_float4(dv[0], dv[1], dv[2], dv[3]);
              stored = true;
            }
          }
          if (!stored) {
#pragma unroll
            for (int u = 0; u < VEC; ++u) p[u] = dv[u];
          }
        }
      }
    }
    if (a.ds) {  // uniform: every lane of the workgroup takes part in the butterfly
      for (int s = W >> 1; s >= 1; s >>= 1) dot += __shfl_xor(dot, s, W);
      if (valid && lane == 0) a.ds[r] = g >= 0 ? alpha * dot : 0.f;
    }
  }
}

// alpha [rows]: one thread per row, +0.0 for a row of no graph
__global__ __launch_bounds__(kT) void attn_weights_kernel(const float* __restrict__ scores, const float* __restrict__ saved,
                                                          const int64_t* __restrict__ graph_ptr, int64_t G, int64_t rows,
                                                          float* __restrict__ alpha) {
  for (int64_t r = (int64_t)blockIdx.x * kT + threadIdx.x; r < rows; r += (int64_t)gridDim.x * kT) {
    int64_t n = 0;
    const int64_t g = graph_of_row(graph_ptr, G, rows, r, n);
    alpha[r] = g >= 0 ? softmax_weight(scores[r], saved[2 * g], saved[2 * g + 1]) : 0.f;
  }
}

bool unsupported(const char* who, int64_t rows, int64_t C, int64_t G, gnc_graph_pool_plan_t* plan) {
  if (gnc_graph_pool_plan(rows, C, G, plan)) return false;
  gnc::set_error("%s: rows %lld / C %lld / graphs %lld outside the supported set (rows < 2^31, 1 <= C <= 2^20, graphs >= 1)", who,
                 (long long)rows, (long long)C, (long long)G);
  return true;
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" int64_t gnc_graph_attention_pool_workspace_floats(int64_t rows, int64_t C, int64_t num_graphs) {
  gnc_graph_pool_plan_t plan;
  if (!gnc_graph_pool_plan(rows, C, num_graphs, &plan)) return -1;
  return plan.split ? gnc_attn::workspace_floats(plan.slots, C) : 0;
}

extern "C" int gnc_graph_attention_pool_forward_f32(const float* y, const float* scores, int64_t rows, int64_t C,
                                                    const int64_t* graph_ptr, int64_t num_graphs, float* out, int64_t ld_out,
                                                    float* saved, float* workspace, int64_t workspace_floats, void* stream) {
  gnc_graph_pool_plan_t plan;
  if (unsupported("gnc_graph_attention_pool_forward_f32", rows, C, num_graphs, &plan)) return GNC_ERR_UNSUPPORTED;
  GNC_REQUIRE(graph_ptr && out && saved && ((y && scores) || rows == 0),
              "gnc_graph_attention_pool_forward_f32: null y / scores / graph_ptr / out / saved");
  GNC_REQUIRE(ld_out >= C, "gnc_graph_attention_pool_forward_f32: ld_out smaller than C");
  GNC_REQUIRE(aligned4(y) && aligned4(scores) && aligned4(out) && aligned4(saved) && (reinterpret_cast<uintptr_t>(graph_ptr) & 7u) == 0,
              "gnc_graph_attention_pool_forward_f32: a pointer is not aligned to its element size");
  AttnArgs a = {};
  a.y = y, a.scores = scores, a.graph_ptr = graph_ptr, a.rows = rows, a.C = C, a.G = num_graphs;
  a.out = out, a.ld_out = ld_out, a.saved = saved;
  a.col_lanes = (int32_t)plan.col_lanes, a.row_lanes = (int32_t)plan.row_lanes;
  a.y16 = gnc::aligned16(y) ? 1 : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 block(kT);
  if (!plan.split) {
    const dim3 grid((unsigned)num_graphs, (unsigned)plan.col_tiles);
    if (plan.vec == 4) attn_graphs_kernel<4><<<grid, block, 0, st>>>(a);
    else attn_graphs_kernel<1><<<grid, block, 0, st>>>(a);
    return gnc::check_launch("attn_graphs_kernel");
  }
  const int64_t need = gnc_attn::workspace_floats(plan.slots, C);
  GNC_REQUIRE(workspace && workspace_floats >= need && aligned4(workspace),
              "gnc_graph_attention_pool_forward_f32: the split regime needs a workspace of %lld floats", (long long)need);
  a.slots = plan.slots;
  a.ws_col = workspace;
  a.ws_z = workspace + gnc_attn::ws_z_index(plan.slots, C, 0);
  attn_max_kernel<<<dim3((unsigned)num_graphs), block, 0, st>>>(a);
  if (int rc = gnc::check_launch("attn_max_kernel")) return rc;
  const dim3 grid((unsigned)plan.slots, (unsigned)plan.col_tiles);
  if (plan.vec == 4) attn_chunks_kernel<4><<<grid, block, 0, st>>>(a);
  else attn_chunks_kernel<1><<<grid, block, 0, st>>>(a);
  if (int rc = gnc::check_launch("attn_chunks_kernel")) return rc;
  attn_merge_kernel<<<dim3((unsigned)num_graphs, (unsigned)gnc::ceil_div(C, kT)), block, 0, st>>>(a);
  return gnc::check_launch("attn_merge_kernel");
}

extern "C" int gnc_graph_attention_pool_backward_f32(const float* dout, int64_t ld_dout, const float* y, const float* scores,
                                                     const float* out, int64_t ld_out, const float* saved, const int64_t* graph_ptr,
                                                     int64_t num_graphs, int64_t rows, int64_t C, float* dy, float* ds, void* stream) {
  if (unsupported("gnc_graph_attention_pool_backward_f32", rows, C, num_graphs, nullptr)) return GNC_ERR_UNSUPPORTED;
  GNC_REQUIRE(dy || ds, "gnc_graph_attention_pool_backward_f32: no gradient wanted");
  GNC_REQUIRE(dout && saved && graph_ptr && (scores || rows == 0), "gnc_graph_attention_pool_backward_f32: null dout / saved / graph_ptr / scores");
  GNC_REQUIRE(!ds || (out && (y || rows == 0)), "gnc_graph_attention_pool_backward_f32: ds needs y and out");
  GNC_REQUIRE(ld_dout >= C && (!ds || ld_out >= C), "gnc_graph_attention_pool_backward_f32: ld_dout / ld_out smaller than C");
  GNC_REQUIRE(aligned4(dout) && aligned4(y) && aligned4(scores) && aligned4(out) && aligned4(saved) && aligned4(dy) && aligned4(ds) &&
                  (reinterpret_cast<uintptr_t>(graph_ptr) & 7u) == 0,
              "gnc_graph_attention_pool_backward_f32: a pointer is not aligned to its element size");
  if (rows == 0) return GNC_OK;
  const gnc_attn::RowGeometry geo = gnc_attn::row_geometry(C);
  AttnBwdArgs a = {};
  a.dout = dout, a.y = ds ? y : nullptr, a.scores = scores, a.out = ds ? out : nullptr, a.saved = saved, a.graph_ptr = graph_ptr;
  a.rows = rows, a.C = C, a.G = num_graphs, a.ld_dout = ld_dout, a.ld_out = ld_out, a.dy = dy, a.ds = ds;
  a.lanes = geo.lanes, a.y16 = gnc::aligned16(y) ? 1 : 0, a.dy16 = gnc::aligned16(dy) ? 1 : 0;
  int64_t blocks = gnc::ceil_div(rows, geo.rows_per_block);
  const int64_t cap = 8ll * gnc::num_cu();
  blocks = blocks > cap ? cap : blocks;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (geo.vec == 4) attn_backward_kernel<4><<<dim3((unsigned)blocks), dim3(kT), 0, st>>>(a);
  else attn_backward_kernel<1><<<dim3((unsigned)blocks), dim3(kT), 0, st>>>(a);
  return gnc::check_launch("attn_backward_kernel");
}

extern "C" int gnc_graph_attention_weights_f32(const float* scores, const float* saved, const int64_t* graph_ptr, int64_t num_graphs,
                                               int64_t rows, float* alpha, void* stream) {
  if (unsupported("gnc_graph_attention_weights_f32", rows, 1, num_graphs, nullptr)) return GNC_ERR_UNSUPPORTED;
  GNC_REQUIRE(saved && graph_ptr && ((scores && alpha) || rows == 0), "gnc_graph_attention_weights_f32: null scores / saved / graph_ptr / alpha");
  GNC_REQUIRE(aligned4(scores) && aligned4(saved) && aligned4(alpha) && (reinterpret_cast<uintptr_t>(graph_ptr) & 7u) == 0,
              "gnc_graph_attention_weights_f32: a pointer is not aligned to its element size");
  if (rows == 0) return GNC_OK;
  int64_t blocks = gnc::ceil_div(rows, kT);
  const int64_t cap = 8ll * gnc::num_cu();
  blocks = blocks > cap ? cap : blocks;
  attn_weights_kernel<<<dim3((unsigned)blocks), dim3(kT), 0, static_cast<hipStream_t>(stream)>>>(scores, saved, graph_ptr, num_graphs,
                                                                                               rows, alpha);
  return gnc::check_launch("attn_weights_kernel");
}
