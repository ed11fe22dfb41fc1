// K24: k-nearest-neighbour edges inside every graph of a batch, ONE launch, no [n, n] matrix.
//
// Definition (what tests/knn_reference.py spells in NumPy): node v scans every candidate u of its OWN graph (u == v only with
// `loop`), d(v, u) = sum_c (f_v[c] - f_u[c])^2 in fp32 with c ascending from +0.0, subtract / multiply / add rounded once each
// (no fused multiply-add), candidates ordered by the 64-bit key (bits of d) << 32 | local index of u (a NaN distance takes the
// distance field 0xffffffff).  Edge slot v k + j is the j-th smallest key of v: sender u, receiver v.
//
// Shape: a workgroup is ONE wavefront that owns kQueryBlock = 64 consecutive query rows of one graph, a lane per query.  The
// lane keeps its feature row (DP floats, the columns behind `dim` are zeros: they add an exact +0.0) and a sorted list of KP keys
// in registers; the list is updated by a fully unrolled min / max chain, never indexed dynamically.  All lanes read the
// SAME candidate row, so its address is wave-uniform: the row comes through the scalar cache (scalar loads, the value is an SGPR
// operand of the subtraction), which is the broadcast an LDS tile would give a single-wave workgroup without the staging copy,
// its barriers and its drained vector-memory waits.  A lane compares against its worst key first and inserts
// only when the candidate beats it.  Work items are found from host sizes alone: item w of the `graph_ptr` form belongs to
// the last graph g with floor(graph_ptr[g] / 64) + g <= w (a bisection; the slots are an upper bound, an item behind its graph's
// last query block exits), the padded form is a plain [B, ceil(capacity / 64)] grid that reads its node count on the device.
// Every output element is written by exactly one lane with plain vector stores; the only atomic is an integer OR on `status`.
#include "gnc_common.h"

// The definition rounds the subtraction, the product and the sum once each.  hipcc contracts a * b + c into a fused multiply-add
// by default - through the __fmul_rn / __fadd_rn of the HIP headers as well, which are plain operators compiled under the
// headers' own setting - so the distance is written with plain operators and contraction is off for this whole file.
#pragma clang fp contract(off)

namespace {

constexpr int kQueryBlock = 64;   // query rows of a workgroup: one per lane of its single wavefront
constexpr int kCandidateUnroll = 4;  // unroll of the candidate loop (a remainder path is taken when n is no multiple of it)
constexpr int kMaxK = 16, kMaxDim = 16;
constexpr uint32_t kNanField = 0xffffffffu;        // distance field of a NaN distance
constexpr uint64_t kEmptyKey = ~uint64_t(0);        // "no candidate": behind every real key (a real index is < 2^31)

struct KnnArgs {
  int64_t ld_feat;
  int dim, k, loop;
  // graph_ptr form
  const int64_t* graph_ptr;
  int64_t num_graphs, num_nodes, ld_edges;
  int64_t total_rows;  // rows of feat, >= 1
  // padded form
  const int32_t* counts;
  int64_t counts_stride;
  int node_capacity, blocks_per_image;
  int64_t* edge_index;
  float* dist;
  int32_t* status;
};

// Slot of graph g's first query block: strictly increasing in g, and graph g's ceil(n / 64) blocks fit in front of the next.
__device__ __forceinline__ int64_t first_item(int64_t a, int64_t g) { return a / kQueryBlock + g; }

__device__ __forceinline__ int64_t clamp_row(int64_t r, int64_t rows) { return r < 0 ? 0 : (r > rows ? rows : r); }

template <int DP, int KP, bool PADDED>
__global__ __launch_bounds__(kQueryBlock) void knn_graph_kernel(const float* __restrict__ feat, const KnnArgs a) {
  const int lane = threadIdx.x;

  // ---- which graph, which query block
  int64_t row0;      // first row of the graph in feat
  int n;             // its candidates
  int q0;            // first local query row of this block
  int64_t* send;     // slot s of sender / receiver / dist: send[s], recv[s], dist[s]
  int64_t* recv;
  float* dist = nullptr;
  int64_t id_offset;  // added to a local id on output
  int64_t slot_base;  // slot of local query v: slot_base + v * k
  int q_end;          // local query rows in [q0, q_end) of this block get k slots written (padded: up to the capacity)
  if (PADDED) {
    const int64_t b = blockIdx.x / a.blocks_per_image;
    q0 = (int)(blockIdx.x % a.blocks_per_image) * kQueryBlock;
    const int32_t c = a.counts[b * a.counts_stride];
    n = c < 0 ? 0 : (c > a.node_capacity ? a.node_capacity : c);
    row0 = b * a.node_capacity;
    const int64_t cap_e = (int64_t)a.k * a.node_capacity;
    send = a.edge_index + b * 2 * cap_e;
    recv = send + cap_e;
    if (a.dist) dist = a.dist + b * cap_e;
    id_offset = 0;
    slot_base = 0;
    q_end = a.node_capacity;
  } else {
    const int64_t w = blockIdx.x, G = a.num_graphs;
    int64_t lo = 0, hi = G - 1;  // the last g with first_item(g) <= w; first_item(0) <= w as graph_ptr[0] is clamped to >= 0 ...
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (first_item(clamp_row(a.graph_ptr[mid], a.num_nodes), mid) <= w) lo = mid;
      else hi = mid - 1;
    }
    const int64_t ga = clamp_row(a.graph_ptr[lo], a.num_nodes);
    int64_t gb = clamp_row(a.graph_ptr[lo + 1], a.num_nodes);
    if (gb < ga) gb = ga;
    const int64_t qb = w - first_item(ga, lo);  // ... but a first graph that starts behind row 0 leaves negative blocks in front
    const bool item = qb >= 0 && qb * kQueryBlock < gb - ga;  // no item: no live lane and no slot below (not an early exit:
    n = item ? (int)(gb - ga) : 0;                              // the kernel keeps one straight path to its end)
    q0 = item ? (int)(qb * kQueryBlock) : 0;
    row0 = ga;
    send = a.edge_index;
    recv = a.edge_index + a.ld_edges;
    dist = a.dist;
    id_offset = ga;
    slot_base = ga * a.k;
    q_end = n;
  }

  const int v = q0 + lane;  // local query row
  const bool live = v < n;
  const int dim = a.dim;

  const int last = dim - 1;
  float fv[DP];
  {
    // a lane without a query reads the table's last row (total_rows >= 1) and drops it: no branch around the loads
    const int64_t qrow = row0 + v < a.total_rows ? row0 + v : a.total_rows - 1;
    const float* __restrict__ row = feat + qrow * a.ld_feat;
#pragma unroll
    for (int c = 0; c < DP; ++c) {
      const float f = row[c < dim ? c : last];  // columns behind dim: a valid address, the value is dropped
      fv[c] = c < dim ? f : 0.f;
    }
    // the query row has landed BEFORE the candidate loop: its vector-memory wait does not sit inside the loop
#pragma unroll
    for (int c = 0; c < DP; ++c) asm volatile("" : "+v"(fv[c]));
  }
  uint64_t best[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) best[j] = kEmptyKey;
  bool saw_nan = false;

  // Column offsets of a row, once: a column behind dim reads the last real one (a valid address) and its value is dropped.
  int off[DP];
#pragma unroll
  for (int c = 0; c < DP; ++c) off[c] = c < dim ? c : last;
  // d(v, u).  The address is the same in every lane: scalar loads, the values are SGPR operands of the subtraction.
  auto distance = [&](int u) -> float {
    const float* __restrict__ fu = feat + (row0 + u) * a.ld_feat;
    float d = 0.f;
#pragma unroll
    for (int c = 0; c < DP; ++c) {
      const float f = fu[off[c]];
      const float t = fv[c] - (c < dim ? f : 0.f);
      d = d + t * t;  // two roundings: contraction is off (above)
    }
    return d;
  };
  // Candidate u at distance d against the lane's list; the node itself is left out in the insert predicate.
  auto offer = [&](int u, float d) {
    const bool nan = d != d;
    const uint32_t field = nan ? kNanField : __float_as_uint(d);
    const uint64_t key = ((uint64_t)field << 32) | (uint32_t)u;
    const bool take = u != v || a.loop;
    saw_nan |= nan && take;
    if (take && key < best[KP - 1]) {  // the rare path: new[j] = max(old[j - 1], min(key, old[j]))
#pragma unroll
      for (int j = KP - 1; j > 0; --j) {
        const uint64_t m = key < best[j] ? key : best[j];
        best[j] = best[j - 1] > m ? best[j - 1] : m;
      }
      best[0] = key < best[0] ? key : best[0];
    }
  };
  if (live) {
#ifdef GNC_KNN_GROUPED_LOADS
    // Developer variant (make variant UNIT=knn_graph V=grouped EXTRA=-DGNC_KNN_GROUPED_LOADS): the distances of a group of
    // kCandidateUnroll rows first, so that all their scalar loads are issued ahead of ONE wait.  Measured slower at every shape
    // (DESIGN.md, K24), so it is not what ships.
    int u = 0;
    for (; u + kCandidateUnroll <= n; u += kCandidateUnroll) {
      float d[kCandidateUnroll];
#pragma unroll
      for (int i = 0; i < kCandidateUnroll; ++i) d[i] = distance(u + i);
#pragma unroll
      for (int i = 0; i < kCandidateUnroll; ++i) offer(u + i, d[i]);
    }
    for (; u < n; ++u) offer(u, distance(u));
#else
    // One candidate at a time, the loop body unrolled kCandidateUnroll times.  hipcc keeps each candidate's loads behind the
    // branch of the candidate in front and waits once per candidate: ONE row is in flight (see the variant above).
#pragma unroll 4
    for (int u = 0; u < n; ++u) {
      const float d = distance(u);
      if (u == v && !a.loop) continue;  // this skip is what keeps the next candidate's loads behind a branch
      offer(u, d);
    }
    static_assert(kCandidateUnroll == 4, "the unroll pragma above");
#endif
  }

  // ---- one lane, k slots
  const int k = a.k;
  bool short_of = false;
  if (v < q_end) {
    const int64_t s0 = slot_base + (int64_t)v * k;
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      if (j < k) {
        const uint32_t u = (uint32_t)best[j];
        const bool empty = !live || best[j] == kEmptyKey;
        short_of |= live && empty;
        send[s0 + j] = empty ? -1 : id_offset + (int64_t)u;
        recv[s0 + j] = empty ? -1 : id_offset + (int64_t)v;
        if (dist) dist[s0 + j] = empty ? __uint_as_float(0x7f800000u) : __uint_as_float((uint32_t)(best[j] >> 32));
      }
    }
  }
  const int flags = (short_of ? GNC_KNN_FEW_CANDIDATES : 0) | (saw_nan ? GNC_KNN_NAN_DISTANCE : 0);
  if (flags) atomicOr(a.status, flags);
}

template <int DP, int KP, bool PADDED>
void launch(const float* feat, const KnnArgs& a, int64_t blocks, hipStream_t stream) {
  knn_graph_kernel<DP, KP, PADDED><<<dim3((unsigned)blocks), dim3(kQueryBlock), 0, stream>>>(feat, a);
}

template <int DP, bool PADDED>
void launch_k(const float* feat, const KnnArgs& a, int64_t blocks, hipStream_t stream) {
  if (a.k <= 4) launch<DP, 4, PADDED>(feat, a, blocks, stream);
  else if (a.k <= 8) launch<DP, 8, PADDED>(feat, a, blocks, stream);
  else launch<DP, 16, PADDED>(feat, a, blocks, stream);
}

template <bool PADDED>
void launch_dim(const float* feat, const KnnArgs& a, int64_t blocks, hipStream_t stream) {
  if (a.dim <= 4) launch_k<4, PADDED>(feat, a, blocks, stream);
  else if (a.dim <= 8) launch_k<8, PADDED>(feat, a, blocks, stream);
  else launch_k<16, PADDED>(feat, a, blocks, stream);
}

int check_shape(const char* who, int64_t ld_feat, int32_t dim, int32_t k) {
  if (k < 1 || k > kMaxK || dim < 1 || dim > kMaxDim || ld_feat < dim) {
    gnc::set_error("%s: k = %d, dim = %d, ld_feat = %lld is outside the supported set (1 <= k <= %d, 1 <= dim <= %d, ld_feat >= dim)",
                   who, k, dim, (long long)ld_feat, kMaxK, kMaxDim);
    return GNC_ERR_UNSUPPORTED;
  }
  return GNC_OK;
}

}  // namespace

extern "C" int gnc_knn_graph_f32(const float* feat, int64_t ld_feat, int32_t dim, const int64_t* graph_ptr, int64_t num_graphs,
                                 int64_t num_nodes, int32_t k, int32_t loop, int64_t* edge_index, int64_t ld_edges, float* dist,
                                 int32_t* status, void* stream_) {
  if (const int rc = check_shape("gnc_knn_graph_f32", ld_feat, dim, k)) return rc;
  GNC_REQUIRE(num_graphs >= 0 && num_nodes >= 0 && num_nodes < (int64_t(1) << 31) && num_graphs < (int64_t(1) << 31),
              "gnc_knn_graph_f32: %lld graphs / %lld nodes", (long long)num_graphs, (long long)num_nodes);
  GNC_REQUIRE(ld_edges >= (int64_t)k * num_nodes, "gnc_knn_graph_f32: ld_edges %lld < k * num_nodes = %lld", (long long)ld_edges,
              (long long)k * num_nodes);
  GNC_REQUIRE(status, "gnc_knn_graph_f32: null status");
  hipStream_t stream = (hipStream_t)stream_;
  if (const int rc = gnc::check_hip(hipMemsetAsync(status, 0, sizeof(int32_t), stream), "gnc_knn_graph_f32: status")) return rc;
  if (num_nodes == 0 || num_graphs == 0) return GNC_OK;
  GNC_REQUIRE(feat && graph_ptr && edge_index, "gnc_knn_graph_f32: null pointer");
  KnnArgs a{};
  a.ld_feat = ld_feat; a.dim = dim; a.k = k; a.loop = loop != 0;
  a.graph_ptr = graph_ptr; a.num_graphs = num_graphs; a.num_nodes = num_nodes; a.ld_edges = ld_edges; a.total_rows = num_nodes;
  a.edge_index = edge_index; a.dist = dist; a.status = status;
  const int64_t blocks = num_nodes / kQueryBlock + num_graphs;  // >= first_item of a graph behind the last
  GNC_REQUIRE(blocks < (int64_t(1) << 31), "gnc_knn_graph_f32: %lld workgroups", (long long)blocks);
  launch_dim<false>(feat, a, blocks, stream);
  return gnc::check_launch("knn_graph_kernel");
}

extern "C" int gnc_knn_graph_padded_f32(const float* feat, int64_t ld_feat, int32_t dim, const int32_t* counts, int64_t counts_stride,
                                        int32_t B, int32_t node_capacity, int32_t k, int32_t loop, int64_t* edge_index, float* dist,
                                        int32_t* status, void* stream_) {
  if (const int rc = check_shape("gnc_knn_graph_padded_f32", ld_feat, dim, k)) return rc;
  GNC_REQUIRE(B >= 0 && B <= (1 << 20) && node_capacity >= 1 && node_capacity <= (1 << 20) && counts_stride >= 1,
              "gnc_knn_graph_padded_f32: %d images at %d nodes, counts stride %lld", B, node_capacity, (long long)counts_stride);
  GNC_REQUIRE(status, "gnc_knn_graph_padded_f32: null status");
  hipStream_t stream = (hipStream_t)stream_;
  if (const int rc = gnc::check_hip(hipMemsetAsync(status, 0, sizeof(int32_t), stream), "gnc_knn_graph_padded_f32: status")) return rc;
  if (B == 0) return GNC_OK;
  GNC_REQUIRE(feat && counts && edge_index, "gnc_knn_graph_padded_f32: null pointer");
  KnnArgs a{};
  a.ld_feat = ld_feat; a.dim = dim; a.k = k; a.loop = loop != 0;
  a.counts = counts; a.counts_stride = counts_stride; a.node_capacity = node_capacity; a.total_rows = (int64_t)B * node_capacity;
  a.blocks_per_image = (node_capacity + kQueryBlock - 1) / kQueryBlock;
  a.edge_index = edge_index; a.dist = dist; a.status = status;
  const int64_t blocks = (int64_t)B * a.blocks_per_image;
  GNC_REQUIRE(blocks < (int64_t(1) << 31), "gnc_knn_graph_padded_f32: %lld workgroups", (long long)blocks);
  launch_dim<true>(feat, a, blocks, stream);
  return gnc::check_launch("knn_graph_kernel");
}

extern "C" void gnc_knn_graph_constants(int32_t* query_block, int32_t* candidate_unroll) {
  if (query_block) *query_block = kQueryBlock;
  if (candidate_unroll) *candidate_unroll = kCandidateUnroll;
}
