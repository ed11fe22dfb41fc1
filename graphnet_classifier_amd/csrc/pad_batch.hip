// Feed of a captured ragged mini-batch step: ONE launch writes every input buffer of the captured graph from a collated batch
// (image_to_graph.collate_graphs: x [N, Fx], pos [N, Fp], edge_index [2, E] with ids already shifted, host graph_ptr / edge_ptr).
// What the host knows - G, N, E, the two offset arrays, the G labels - travels BY VALUE in the kernel arguments (about 1.7 KB of
// the 4 KB argument segment, which is what bounds G at GNC_PAD_BATCH_MAX_GRAPHS): no host-to-device copy per step.
//
// Layout written, with M = node_capacity, C = edge_capacity, D = max(1, ceil(C / 8)) dummy nodes behind the M node slots:
//   x_buf[r]        = x[r] for r < N, 0 for N <= r < M (pos_buf likewise); rows [M, M + D) are the dummies: zero, never written;
//   ei_buf[:, k]    = edge_index[:, k] for k < E; both ends M + k % D for E <= k < C (a dummy self-loop, at most 8 per dummy);
//   graph_ptr_buf   = graph_ptr as int64 [G + 1] (slack rows [N, M) belong to no graph); labels_buf = labels as int64 [G].
// Both ends of edge k of graph g (found from edge_ptr) must lie in [graph_ptr[g], graph_ptr[g + 1]); otherwise 1 goes into the
// STICKY int32 flag, which this kernel never clears (the host does).  Ids are copied as given and never dereferenced here; one
// outside [0, M + D) is caught and sanitised by the topology build that follows.
//
// A grid-stride copy: 16-byte loads and stores where the pointers allow, element-wise otherwise (Fx = 3 makes N * Fx a
// non-multiple of 4; a source that is a view into a larger tensor may be only 4-byte aligned).  No atomics: racing stores of the
// same flag value are fine.
#include "gnc_common.h"

namespace {

constexpr int MAXG = GNC_PAD_BATCH_MAX_GRAPHS;

struct PadBatchArgs {
  const float* x;
  const float* pos;
  const int64_t* ei;
  int64_t ld_ei;
  float* x_buf;
  float* pos_buf;
  int64_t* ei_buf;
  int64_t* gp_buf;
  int64_t* labels_buf;  // NULL: no labels
  int32_t* flag;
  int64_t n_x, m_x;  // floats of x that hold nodes (N * Fx), floats of x_buf in front of the dummies (M * Fx)
  int64_t n_p, m_p;
  int64_t E, C, M, D;
  int32_t G;
  int64_t graph_ptr[MAXG + 1];
  int64_t edge_ptr[MAXG + 1];
  int64_t labels[MAXG];
};
static_assert(sizeof(PadBatchArgs) <= 4096, "kernel arguments must fit the 4 KB argument segment");

__device__ __forceinline__ bool is16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// floats [4 j, 4 j + 4) of dst [ndst]: src where it has them, zeros behind
__device__ __forceinline__ void copy_f32_chunk(const float* __restrict__ src, int64_t nsrc, bool src16, float* __restrict__ dst,
                                               int64_t ndst, bool dst16, int64_t j) {
  const int64_t i0 = 4 * j;
  float v[4];
  if (src16 && i0 + 4 <= nsrc) {
    const float4 q = *reinterpret_cast<const float4*>(src + i0);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = i0 + u < nsrc ? src[i0 + u] : 0.f;
  }
  if (dst16 && i0 + 4 <= ndst) {
    *reinterpret_cast<float4*>(dst + i0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i0 + u < ndst) dst[i0 + u] = v[u];
  }
}

// the graph that owns edge k < E: the number of entries of edge_ptr[1 .. G] that are <= k (graphs without edges are stepped over)
__device__ __forceinline__ int graph_of_edge(const PadBatchArgs& a, int64_t k) {
  int lo = 0, hi = a.G;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.edge_ptr[mid + 1] <= k) lo = mid + 1;
    else hi = mid;
  }
  return lo < a.G ? lo : a.G - 1;
}

__global__ __launch_bounds__(gnc::kBlock) void pad_graph_batch_kernel(const PadBatchArgs a) {
  const int64_t cx = (a.m_x + 3) >> 2, cp = (a.m_p + 3) >> 2, ce = (a.C + 1) >> 1;  // 16-byte chunks of x_buf, pos_buf, one ei_buf row
  const int64_t total = cx + cp + 2 * ce + (a.G + 1) + (a.labels_buf ? a.G : 0);
  const bool x_s16 = is16(a.x), x_d16 = is16(a.x_buf);
  const bool p_s16 = is16(a.pos), p_d16 = is16(a.pos_buf);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    int64_t i = t;
    if (i < cx) {
      copy_f32_chunk(a.x, a.n_x, x_s16, a.x_buf, a.m_x, x_d16, i);
      continue;
    }
    i -= cx;
    if (i < cp) {
      copy_f32_chunk(a.pos, a.n_p, p_s16, a.pos_buf, a.m_p, p_d16, i);
      continue;
    }
    i -= cp;
    if (i < 2 * ce) {
      const int row = i >= ce;
      const int64_t k0 = 2 * (i - (row ? ce : 0));
      const int64_t* __restrict__ src = a.ei + row * a.ld_ei;
      int64_t* __restrict__ dst = a.ei_buf + row * a.C;
      int64_t v[2];
      if (k0 + 2 <= a.E && is16(src)) {
        const longlong2 q = *reinterpret_cast<const longlong2*>(src + k0);
        v[0] = q.x, v[1] = q.y;
      } else {
#pragma unroll
        for (int u = 0; u < 2; ++u) v[u] = k0 + u < a.E ? src[k0 + u] : a.M + (k0 + u) % a.D;
      }
      bool bad = false;
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if (k0 + u < a.E) {
          const int g = graph_of_edge(a, k0 + u);
          bad |= v[u] < a.graph_ptr[g] || v[u] >= a.graph_ptr[g + 1];
        }
      if (bad) *a.flag = 1;
      if (k0 + 2 <= a.C && is16(dst)) {
        *reinterpret_cast<longlong2*>(dst + k0) = make_longlong2(v[0], v[1]);
      } else {
#pragma unroll
        for (int u = 0; u < 2; ++u)
          if (k0 + u < a.C) dst[k0 + u] = v[u];
      }
      continue;
    }
    i -= 2 * ce;
    if (i <= a.G) {
      a.gp_buf[i] = a.graph_ptr[i];
      continue;
    }
    i -= a.G + 1;
    a.labels_buf[i] = a.labels[i];
  }
}

bool supported(int64_t G, int64_t N, int64_t E, int64_t M, int64_t C, int64_t fx, int64_t fp) {
  if (G < 1 || G > MAXG || N < 0 || E < 0 || N > M || E > C || fx < 1 || fp < 1 || fx > 4096 || fp > 4096) return false;
  const int64_t D = C / 8 + 1;  // >= max(1, ceil(C / 8)), overflow-free
  return C <= (1ll << 31) && M <= (1ll << 30) && M + D < (1ll << 31);  // node ids are int32 inside the engine
}

}  // namespace

extern "C" int32_t gnc_pad_graph_batch_supported(int64_t num_graphs, int64_t num_nodes, int64_t num_edges, int64_t node_capacity,
                                                 int64_t edge_capacity, int32_t fx, int32_t fp) {
  return supported(num_graphs, num_nodes, num_edges, node_capacity, edge_capacity, fx, fp) ? 1 : 0;
}

extern "C" int gnc_pad_graph_batch(const float* x, int32_t fx, const float* pos, int32_t fp, const int64_t* edge_index,
                                   int64_t ld_edge_index, int64_t num_nodes, int64_t num_edges, int64_t num_graphs,
                                   const int64_t* graph_ptr, const int64_t* edge_ptr, const int64_t* labels, int64_t node_capacity,
                                   int64_t edge_capacity, float* x_buf, float* pos_buf, int64_t* ei_buf, int64_t* graph_ptr_buf,
                                   int64_t* labels_buf, int32_t* flag, void* stream) {
  if (!supported(num_graphs, num_nodes, num_edges, node_capacity, edge_capacity, fx, fp)) {
    gnc::set_error("gnc_pad_graph_batch: %lld graphs / %lld nodes / %lld edges into capacities %lld / %lld is outside the supported set "
                   "(at most %d graphs, sizes within the capacities)", (long long)num_graphs, (long long)num_nodes,
                   (long long)num_edges, (long long)node_capacity, (long long)edge_capacity, MAXG);
    return GNC_ERR_UNSUPPORTED;
  }
  GNC_REQUIRE(graph_ptr && edge_ptr, "gnc_pad_graph_batch: graph_ptr and edge_ptr (host arrays) are required");
  GNC_REQUIRE(x_buf && pos_buf && graph_ptr_buf && flag && (ei_buf || edge_capacity == 0), "gnc_pad_graph_batch: null output buffer");
  GNC_REQUIRE((x && pos) || num_nodes == 0, "gnc_pad_graph_batch: null x / pos");
  GNC_REQUIRE(edge_index || num_edges == 0, "gnc_pad_graph_batch: null edge_index");
  GNC_REQUIRE(num_edges == 0 || ld_edge_index >= num_edges, "gnc_pad_graph_batch: ld_edge_index smaller than the edge count");
  GNC_REQUIRE((labels == nullptr) == (labels_buf == nullptr), "gnc_pad_graph_batch: labels and labels_buf come together");
  GNC_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3u) == 0 && (reinterpret_cast<uintptr_t>(pos) & 3u) == 0 &&
                  (reinterpret_cast<uintptr_t>(x_buf) & 3u) == 0 && (reinterpret_cast<uintptr_t>(pos_buf) & 3u) == 0 &&
                  (reinterpret_cast<uintptr_t>(edge_index) & 7u) == 0 && (reinterpret_cast<uintptr_t>(ei_buf) & 7u) == 0 &&
                  (reinterpret_cast<uintptr_t>(graph_ptr_buf) & 7u) == 0 && (reinterpret_cast<uintptr_t>(labels_buf) & 7u) == 0 &&
                  (reinterpret_cast<uintptr_t>(flag) & 3u) == 0,
              "gnc_pad_graph_batch: a pointer is not aligned to its element size");
  const int G = (int)num_graphs;
  GNC_REQUIRE(graph_ptr[0] == 0 && graph_ptr[G] == num_nodes && edge_ptr[0] == 0 && edge_ptr[G] == num_edges,
              "gnc_pad_graph_batch: graph_ptr / edge_ptr must run from 0 to the node / edge count");
  for (int g = 0; g < G; ++g)
    GNC_REQUIRE(graph_ptr[g] <= graph_ptr[g + 1] && edge_ptr[g] <= edge_ptr[g + 1],
                "gnc_pad_graph_batch: graph_ptr / edge_ptr must not decrease");
  PadBatchArgs a = {};
  a.x = x, a.pos = pos, a.ei = edge_index, a.ld_ei = ld_edge_index;
  a.x_buf = x_buf, a.pos_buf = pos_buf, a.ei_buf = ei_buf, a.gp_buf = graph_ptr_buf, a.labels_buf = labels_buf, a.flag = flag;
  a.n_x = num_nodes * fx, a.m_x = node_capacity * fx, a.n_p = num_nodes * fp, a.m_p = node_capacity * fp;
  a.E = num_edges, a.C = edge_capacity, a.M = node_capacity;
  a.D = edge_capacity / 8 + (edge_capacity % 8 != 0);
  if (a.D < 1) a.D = 1;
  a.G = G;
  for (int g = 0; g <= G; ++g) a.graph_ptr[g] = graph_ptr[g], a.edge_ptr[g] = edge_ptr[g];
  for (int g = 0; g < G && labels; ++g) a.labels[g] = labels[g];
  const int64_t total = gnc::ceil_div(a.m_x, 4) + gnc::ceil_div(a.m_p, 4) + 2 * gnc::ceil_div(a.C, 2) + 2 * (int64_t)G + 1;
  const int64_t blocks = gnc::capped_blocks(total, gnc::kBlock, 4);
  pad_graph_batch_kernel<<<dim3((unsigned)blocks), dim3(gnc::kBlock), 0, static_cast<hipStream_t>(stream)>>>(a);
  return gnc::check_launch("pad_graph_batch_kernel");
}
