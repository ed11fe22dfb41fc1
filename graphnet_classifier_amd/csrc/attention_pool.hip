// K19: attention read-out.  Per graph g of a block-diagonal batch - rows [graph_ptr[g], graph_ptr[g + 1]) of y [rows, C] with one
// score per row - the softmax of the graph's scores and the column sums of y weighted by it:
//   m_g = max_v s_v,  e_v = expf(s_v - m_g),  Z_g = sum_v e_v,  out[g, c] = (sum_v e_v y[v, c]) / Z_g
// and the backward  dy[v, :] = alpha_v dout[g, :],  ds[v] = alpha_v sum_c dout[g, c] (y[v, c] - out[g, c]),  alpha_v = e_v / Z_g.
//
// Rules: an empty graph pools to +0.0 and nothing is divided; rows of no graph are never read and get +0.0 gradients.  The forward
// keeps (m_g, Z_g) per graph ([G, 2] floats); the backward recomputes alpha_v from them, no [rows] array is stored.  A non-finite
// score stays inside its graph: fmaxf drops a NaN from m_g, expf(NaN - m_g) makes Z_g and every column of that graph NaN.
//
// The forward is the chunked per-graph reduction of csrc/graph_reduce.h - the summation order is defined there, for both regimes,
// and is the one K17 sums in because it is the same code - carrying the weighted column sums and Z: AttnOp below.  The product
// e_v y[v, c] enters by ONE fmaf.  The maximum, exact in any order, is K19's own step in front of the shared body: the graph-owned
// workgroup forms it itself, the split regime by a launch of one workgroup per graph (attn_max_kernel).  In the split regime the
// workspace layout is attention_pool_index.h's.
#include "graph_reduce.h"
#include "attention_pool_index.h"

#include <math.h>

namespace {

using namespace gnc_reduce;

struct AttnArgs : ReduceArgs {
  const float* scores;
  float* out;
  int64_t ld_out;
  float* saved;   // [G, 2]: (m_g, Z_g); (0, 0) for an empty graph
  float* ws_col;  // split regime: [slots, C]
  float* ws_z;    // split regime: [slots]
};

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

// K19's operation (graph_reduce.h): the e-weighted sum of every column and, per thread, Z; it carries the graph's maximum m
template <int VEC>
struct AttnOp {
  const AttnArgs& a;
  float m;
  struct Partial {
    float acc[VEC], z;
  };
  struct Shared {
    float acc[VEC][kT], z[kT];
  };
  __device__ __forceinline__ Partial identity() const {
    Partial p;
#pragma unroll
    for (int u = 0; u < VEC; ++u) p.acc[u] = 0.f;
    p.z = 0.f;
    return p;
  }
  // graph-owned: the workgroup forms m_g itself and keeps it, as attn_max_kernel does for the split regime
  __device__ __forceinline__ void graph_begin(int64_t g, int64_t ra, int64_t rb, Shared& sh) {
    m = block_score_max(a.scores, ra, rb, sh.z);
    if (threadIdx.x == 0 && blockIdx.y == 0) a.saved[2 * g] = rb > ra ? m : 0.f;
  }
  __device__ __forceinline__ void slot_begin(int64_t g) { m = a.saved[2 * g]; }
  __device__ __forceinline__ void row(Partial& p, int64_t row, const float (&v)[VEC]) const {
    const float e = expf(a.scores[row] - m);
    p.z += e;
#pragma unroll
    for (int u = 0; u < VEC; ++u) p.acc[u] = fmaf(e, v[u], p.acc[u]);
  }
  __device__ __forceinline__ void fold(Partial& p, const Partial& q) const {
#pragma unroll
    for (int u = 0; u < VEC; ++u) p.acc[u] += q.acc[u];
    p.z += q.z;
  }
  __device__ __forceinline__ void park(Shared& sh, int t, const Partial& p) const {
#pragma unroll
    for (int u = 0; u < VEC; ++u) sh.acc[u][t] = p.acc[u];
    sh.z[t] = p.z;
  }
  __device__ __forceinline__ Partial parked(const Shared& sh, int t) const {
    Partial p;
#pragma unroll
    for (int u = 0; u < VEC; ++u) p.acc[u] = sh.acc[u][t];
    p.z = sh.z[t];
    return p;
  }
  // out[g, col0 ...] and, from the thread of column 0, Z_g (every thread of a column holds the same Z)
  __device__ __forceinline__ void store(int64_t g, int64_t n, int64_t col0, const Partial& p) const {
#pragma unroll
    for (int u = 0; u < VEC; ++u) a.out[g * a.ld_out + col0 + u] = n > 0 ? p.acc[u] / p.z : 0.f;
    if (col0 == 0) a.saved[2 * g + 1] = n > 0 ? p.z : 0.f;
  }
  __device__ __forceinline__ void store_slot(int64_t slot, int64_t col0, const Partial& p) const {
#pragma unroll
    for (int u = 0; u < VEC; ++u) a.ws_col[gnc_attn::ws_col_index(slot, a.C, col0 + u)] = p.acc[u];
    if (col0 == 0) a.ws_z[slot] = p.z;
  }
  __device__ __forceinline__ Partial slot_partial(int64_t slot, int64_t c) const {
    return Partial{{a.ws_col[gnc_attn::ws_col_index(slot, a.C, c)]}, a.ws_z[slot]};
  }
};

template <int VEC>
__global__ __launch_bounds__(kT) void attn_graphs_kernel(const AttnArgs a) {
  __shared__ typename AttnOp<VEC>::Shared sh;
  AttnOp<VEC> op{a, 0.f};
  reduce_graph<VEC>(a, op, sh);
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

template <int VEC>
__global__ __launch_bounds__(kT) void attn_chunks_kernel(const AttnArgs a) {
  __shared__ typename AttnOp<VEC>::Shared sh;
  AttnOp<VEC> op{a, 0.f};
  reduce_slot<VEC>(a, op, sh);
}

__global__ __launch_bounds__(kT) void attn_merge_kernel(const AttnArgs a) { merge_graph(a, AttnOp<1>{a, 0.f}); }

const ReduceKernels<AttnArgs> kAttnKernels = {attn_graphs_kernel<1>, attn_graphs_kernel<4>, attn_chunks_kernel<1>, attn_chunks_kernel<4>,
                                              attn_merge_kernel,     "attn_graphs_kernel",  "attn_chunks_kernel",  "attn_merge_kernel"};

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
  const RowLane x = row_lane(threadIdx.x, W);
  const int lane = x.lane, sub = x.sub;
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
            load_vec<VEC>(a.y + r * a.C + c0, a.y16 != 0, v);
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

bool aligned4(const void* p) { return gnc::aligned_to(p, 4); }

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
  GNC_REQUIRE(aligned4(y) && aligned4(scores) && aligned4(out) && aligned4(saved) && gnc::aligned_to(graph_ptr, 8),
              "gnc_graph_attention_pool_forward_f32: a pointer is not aligned to its element size");
  AttnArgs a = {};
  a.y = y, a.scores = scores, a.graph_ptr = graph_ptr, a.rows = rows, a.C = C, a.G = num_graphs;
  a.out = out, a.ld_out = ld_out, a.saved = saved;
  a.col_lanes = (int32_t)plan.col_lanes, a.row_lanes = (int32_t)plan.row_lanes;
  a.y16 = gnc::aligned16(y) ? 1 : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!plan.split) return launch_graph_owned(kAttnKernels, a, plan, st);
  const int64_t need = gnc_attn::workspace_floats(plan.slots, C);
  GNC_REQUIRE(workspace && workspace_floats >= need && aligned4(workspace),
              "gnc_graph_attention_pool_forward_f32: the split regime needs a workspace of %lld floats", (long long)need);
  a.slots = plan.slots;
  a.ws_col = workspace;
  a.ws_z = workspace + gnc_attn::ws_z_index(plan.slots, C, 0);
  attn_max_kernel<<<dim3((unsigned)num_graphs), dim3(kT), 0, st>>>(a);
  if (int rc = gnc::check_launch("attn_max_kernel")) return rc;
  return launch_split(kAttnKernels, a, plan, st);
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
                  gnc::aligned_to(graph_ptr, 8),
              "gnc_graph_attention_pool_backward_f32: a pointer is not aligned to its element size");
  if (rows == 0) return GNC_OK;
  const RowGeometry geo = row_geometry(C);
  AttnBwdArgs a = {};
  a.dout = dout, a.y = ds ? y : nullptr, a.scores = scores, a.out = ds ? out : nullptr, a.saved = saved, a.graph_ptr = graph_ptr;
  a.rows = rows, a.C = C, a.G = num_graphs, a.ld_dout = ld_dout, a.ld_out = ld_out, a.dy = dy, a.ds = ds;
  a.lanes = geo.lanes, a.y16 = gnc::aligned16(y) ? 1 : 0, a.dy16 = gnc::aligned16(dy) ? 1 : 0;
  const int64_t blocks = gnc::capped_blocks(rows, geo.rows_per_block);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (geo.vec == 4) attn_backward_kernel<4><<<dim3((unsigned)blocks), dim3(kT), 0, st>>>(a);
  else attn_backward_kernel<1><<<dim3((unsigned)blocks), dim3(kT), 0, st>>>(a);
  return gnc::check_launch("attn_backward_kernel");
}

extern "C" int gnc_graph_attention_weights_f32(const float* scores, const float* saved, const int64_t* graph_ptr, int64_t num_graphs,
                                               int64_t rows, float* alpha, void* stream) {
  if (unsupported("gnc_graph_attention_weights_f32", rows, 1, num_graphs, nullptr)) return GNC_ERR_UNSUPPORTED;
  GNC_REQUIRE(saved && graph_ptr && ((scores && alpha) || rows == 0), "gnc_graph_attention_weights_f32: null scores / saved / graph_ptr / alpha");
  GNC_REQUIRE(aligned4(scores) && aligned4(saved) && aligned4(alpha) && gnc::aligned_to(graph_ptr, 8),
              "gnc_graph_attention_weights_f32: a pointer is not aligned to its element size");
  if (rows == 0) return GNC_OK;
  const int64_t blocks = gnc::capped_blocks(rows, kT);
  attn_weights_kernel<<<dim3((unsigned)blocks), dim3(kT), 0, static_cast<hipStream_t>(stream)>>>(scores, saved, graph_ptr, num_graphs,
                                                                                               rows, alpha);
  return gnc::check_launch("attn_weights_kernel");
}
