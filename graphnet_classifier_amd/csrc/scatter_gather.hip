// K1 scatter-sum aggregation over a destination-sorted CSR, K2 row gather, K6 edge features.
// All three are HBM-bandwidth-bound row movers; the design rules are: 16 B per lane, whole
// rows per lane group, several independent loads in flight per lane, no atomics.
//
// K1's lane mapping, its regimes and the order in which a destination's rows are added are segment_csr.h's; what K1 adds to the
// skeleton is the plain sum from +0.0.  K2 is the skeleton's row pass.
#include <stdlib.h>

#include "gnc_common.h"
#include "segment_csr.h"

namespace {

using namespace gnc_csr;

__device__ __forceinline__ void acc4(f4& a, const f4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }

// rows [start, end) of one destination added from +0.0 in ascending k, columns [col, col + 4)
template <bool HAS_PERM, bool STREAM>
__device__ __forceinline__ f4 sum_rows(const float* __restrict__ src, int64_t ld_src, const int32_t* __restrict__ perm,
                                       int32_t start, int32_t end, int col) {
  f4 a = {0.f, 0.f, 0.f, 0.f};
  walk_rows<HAS_PERM, STREAM>(src, ld_src, perm, start, end, col, no_side{}, [&](int32_t, Nothing, const f4& x) { acc4(a, x); });
  return a;
}

// K1, chunk regime: feat_dim % 4 == 0, feat_dim <= 4*LPR, 16-B aligned rows.
template <int LPR, bool HAS_PERM>
__global__ __launch_bounds__(gnc::kBlock) void scatter_sum_csr_vec4(
    const float* __restrict__ src, int64_t ld_src, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ perm, int32_t num_nodes, int32_t feat_dim, float* __restrict__ out,
    int64_t ld_out) {
  for_chunk_destinations<LPR>(rowptr, num_nodes, feat_dim, [&](int64_t v, int32_t start, int32_t end, int col) {
    st4(out + v * ld_out + col, sum_rows<HAS_PERM, true>(src, ld_src, perm, start, end, col));
  });
}

// K1 for a small graph (the reference's one-graph-per-call regime; 1024 nodes at 128 features: 16 busy waves and 25..37 us in
// the chunk regime).  Same sums in the same order (bit-identical).
template <int LPR, bool HAS_PERM>
__global__ __launch_bounds__(gnc::kBlock) void scatter_sum_csr_small(
    const float* __restrict__ src, int64_t ld_src, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ perm, int32_t num_nodes, int32_t feat_dim, float* __restrict__ out,
    int64_t ld_out) {
  for_small_destinations<LPR>(rowptr, num_nodes, feat_dim, [&](int64_t v, int32_t start, int32_t end, int col) {
    st4(out + v * ld_out + col, sum_rows<HAS_PERM, false>(src, ld_src, perm, start, end, col));
  });
}

// Fix-up of the fused aggregation epilogue (mlp_resident.hip) in ONE launch: blocks [0, fix_blocks) sum the few
// destinations cut by a wave's row-range boundary from the stored rows, one 16-lane group (4 floats per lane and 64
// features) each; the blocks behind them give the destinations without any row their zeros (one thread per destination;
// far cheaper than a memset of the whole [N, D] aggregate in front of the edge kernel).
// VEC: whole 16-B pieces (feat_dim, ld_src % 4 == 0, aligned base); eight rows are requested before the first is added -
// a destination's rows are still ADDED in ascending order starting from 0.0, as K1 does, only their loads overlap
// (one dependent load per row made this 16 us for a dozen rows per destination).
template <bool VEC>
__global__ __launch_bounds__(gnc::kBlock) void agg_fixup_kernel(const float* __restrict__ src, int64_t ld_src,
                                                                const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ fix, int32_t n_fix, int32_t fix_blocks,
                                                                int32_t num_nodes, int32_t feat_dim,
                                                                float* __restrict__ out, int64_t ld_out) {
  if ((int)blockIdx.x >= fix_blocks) {
    const int64_t v = (int64_t)(blockIdx.x - fix_blocks) * blockDim.x + threadIdx.x;
    if (v >= num_nodes || rowptr[v] != rowptr[v + 1]) return;
    for (int c = 0; c < feat_dim; ++c) out[v * ld_out + c] = 0.f;
    return;
  }
  const int j = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 4);
  const int col = (threadIdx.x & 15) * 4;
  if (j >= n_fix) return;
  const int32_t v = fix[j];
  if (v < 0 || v >= num_nodes) return;
  const int32_t k0 = rowptr[v], k1 = rowptr[v + 1];
  if (k0 == k1) return;  // no rows: the zero blocks write it
  for (int c = col; c < feat_dim; c += 64) {
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (VEC) {
      int32_t k = k0;
      for (; k + 8 <= k1; k += 8) {
        float4 r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = *reinterpret_cast<const float4*>(src + (int64_t)(k + u) * ld_src + c);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          a[0] += r[u].x; a[1] += r[u].y; a[2] += r[u].z; a[3] += r[u].w;
        }
      }
      float4 r[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int32_t kk = k + u < k1 ? k + u : k1 - 1;  // clamped: every load is legal, the surplus is not added
        r[u] = *reinterpret_cast<const float4*>(src + (int64_t)kk * ld_src + c);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k + u < k1) {
          a[0] += r[u].x; a[1] += r[u].y; a[2] += r[u].z; a[3] += r[u].w;
        }
    } else {
      for (int32_t k = k0; k < k1; ++k)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (c + q < feat_dim) a[q] += src[(int64_t)k * ld_src + c + q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (c + q < feat_dim) out[(int64_t)v * ld_out + c + q] = a[q];
  }
}

// K1, generic: any feat_dim / alignment; one wave per destination, scalar columns.
template <bool HAS_PERM>
__global__ __launch_bounds__(gnc::kBlock) void scatter_sum_csr_scalar(
    const float* __restrict__ src, int64_t ld_src, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ perm, int32_t num_nodes, int32_t feat_dim, float* __restrict__ out,
    int64_t ld_out) {
  for_scalar_destinations(rowptr, num_nodes, feat_dim, no_side{}, [&](int64_t v, int32_t start, int32_t end, int c, Nothing) {
    float a = 0.f;
    walk_rows_scalar<HAS_PERM>(src, ld_src, perm, start, end, c, [&](int32_t, float x) { a += x; });
    out[v * ld_out + c] = a;
  });
}

// ---------------------------------------------------------------------------------------
// K2 row gather: out[r, :] = table[index[r], :]
// ---------------------------------------------------------------------------------------
template <int LPR, bool ADD = false>
__global__ __launch_bounds__(gnc::kBlock) void gather_rows_vec4(const float* __restrict__ table, int64_t ld_table,
                                                                const int32_t* __restrict__ index,
                                                                int64_t num_rows, int32_t feat_dim,
                                                                float* __restrict__ out, int64_t ld_out,
                                                                const float* __restrict__ addend = nullptr, int64_t ld_add = 0) {
  const int col = row_pass_col<LPR>();
  if (col >= feat_dim) return;
  for_rows_two_in_flight<LPR>(
      num_rows,
      [&](int64_t r) {
        f4 a = ld4(table + (int64_t)index[r] * ld_table + col);
        if (ADD) acc4(a, ld4_stream(addend + r * ld_add + col));
        return a;
      },
      [&](int64_t r, const f4& a) { st4(out + r * ld_out + col, a); });
}

template <bool ADD = false>
__global__ __launch_bounds__(gnc::kBlock) void gather_rows_scalar(const float* __restrict__ table, int64_t ld_table,
                                                                  const int32_t* __restrict__ index,
                                                                  int64_t num_rows, int32_t feat_dim,
                                                                  float* __restrict__ out, int64_t ld_out,
                                                                  const float* __restrict__ addend = nullptr, int64_t ld_add = 0) {
  const int64_t total = num_rows * feat_dim;
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; t < total; t += stride) {
    const int64_t r = t / feat_dim;
    const int c = (int)(t - r * feat_dim);
    float v = table[(int64_t)index[r] * ld_table + c];
    if (ADD) v += addend[r * ld_add + c];
    out[r * ld_out + c] = v;
  }
}

// ---------------------------------------------------------------------------------------
// K6 edge features: out[e] = [pos[dst]-pos[src], sum|pos[dst]-pos[src]|]
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(gnc::kBlock) void edge_features_kernel(const float* __restrict__ pos, int32_t space_dim,
                                                                    const int32_t* __restrict__ src,
                                                                    const int32_t* __restrict__ dst,
                                                                    int64_t num_edges, float* __restrict__ out,
                                                                    int64_t od) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; e < num_edges; e += stride) {
    const float* ps = pos + (int64_t)src[e] * space_dim;
    const float* pd = pos + (int64_t)dst[e] * space_dim;
    float dist = 0.f;
    for (int d = 0; d < space_dim; ++d) {
      const float rel = pd[d] - ps[d];
      out[e * od + d] = rel;
      dist += fabsf(rel);  // summed in dimension order like torch.sum(dim=1) on a short row
    }
    out[e * od + space_dim] = dist;
    for (int64_t d = space_dim + 1; d < od; ++d) out[e * od + d] = 0.f;
  }
}

template <bool HAS_PERM>
int launch_scatter(const float* src, int64_t ld_src, const int32_t* rowptr, const int32_t* perm, int32_t n,
                   int32_t d, float* out, int64_t ld_out, hipStream_t stream) {
  const dim3 block(gnc::kBlock);
  if (vec4_ok(src, ld_src, d) && vec4_ok(out, ld_out, d)) {
    // A/B switch of the small regime (profiles/README.md); K1 alone has it, so it stays here and not in forward_plan's rule
    static const bool no_small = getenv("GNC_NO_SMALL_K1") != nullptr;
    const ForwardPlan p = no_small ? forward_plan(n, d, false) : forward_plan(n, d);
    const int rc = dispatch_lanes(p.lpr, [&](auto lanes) {
      constexpr int L = decltype(lanes)::value;
      if (p.small) scatter_sum_csr_small<L, HAS_PERM><<<p.grid, block, 0, stream>>>(src, ld_src, rowptr, perm, n, d, out, ld_out);
      else scatter_sum_csr_vec4<L, HAS_PERM><<<p.grid, block, 0, stream>>>(src, ld_src, rowptr, perm, n, d, out, ld_out);
    });
    return rc ? rc : gnc::check_launch(p.small ? "scatter_sum_csr_small" : "scatter_sum_csr_vec4");
  }
  scatter_sum_csr_scalar<HAS_PERM><<<scalar_grid(n), block, 0, stream>>>(src, ld_src, rowptr, perm, n, d, out, ld_out);
  return gnc::check_launch("scatter_sum_csr_scalar");
}

}  // namespace

extern "C" int gnc_scatter_sum_csr_f32(const float* src, int64_t ld_src, const int32_t* rowptr, const int32_t* perm,
                                       int64_t num_nodes, int64_t num_edges, int32_t feat_dim, float* out,
                                       int64_t ld_out, void* stream_) {
  GNC_REQUIRE(num_nodes >= 0 && num_edges >= 0 && feat_dim >= 0, "gnc_scatter_sum_csr_f32: negative size");
  GNC_REQUIRE(num_nodes < INT32_MAX && num_edges < INT32_MAX, "gnc_scatter_sum_csr_f32: sizes exceed int32");
  if (num_nodes == 0 || feat_dim == 0) return GNC_OK;
  GNC_REQUIRE(rowptr && out, "gnc_scatter_sum_csr_f32: null rowptr/out");
  GNC_REQUIRE(num_edges == 0 || src, "gnc_scatter_sum_csr_f32: null src");
  GNC_REQUIRE(ld_src >= feat_dim && ld_out >= feat_dim, "gnc_scatter_sum_csr_f32: leading dimension < feat_dim");
  hipStream_t stream = (hipStream_t)stream_;
  if (perm)
    return launch_scatter<true>(src, ld_src, rowptr, perm, (int32_t)num_nodes, feat_dim, out, ld_out, stream);
  return launch_scatter<false>(src, ld_src, rowptr, nullptr, (int32_t)num_nodes, feat_dim, out, ld_out, stream);
}

extern "C" int gnc_agg_fixup_f32(const float* src, int64_t ld_src, const int32_t* rowptr, const int32_t* fix, int32_t n_fix,
                                 int64_t num_nodes, int32_t feat_dim, float* out, int64_t ld_out, void* stream_) {
  GNC_REQUIRE(n_fix >= 0 && num_nodes >= 0 && num_nodes < INT32_MAX && feat_dim >= 0, "gnc_agg_fixup_f32: bad sizes");
  if (feat_dim == 0 || num_nodes == 0) return GNC_OK;
  GNC_REQUIRE(rowptr && out && (n_fix == 0 || (src && fix)), "gnc_agg_fixup_f32: null pointer");
  GNC_REQUIRE(ld_src >= feat_dim && ld_out >= feat_dim, "gnc_agg_fixup_f32: leading dimension < feat_dim");
  const int64_t fix_blocks = n_fix > 0 ? gnc::ceil_div((int64_t)n_fix * 16, gnc::kBlock) : 0;
  const int64_t blocks = fix_blocks + gnc::ceil_div(num_nodes, gnc::kBlock);
  const bool vec = feat_dim % 4 == 0 && ld_src % 4 == 0 && gnc::aligned16(src);
  if (vec)
    agg_fixup_kernel<true><<<dim3((unsigned)blocks), dim3(gnc::kBlock), 0, (hipStream_t)stream_>>>(
        src, ld_src, rowptr, fix, n_fix, (int32_t)fix_blocks, (int32_t)num_nodes, feat_dim, out, ld_out);
  else
    agg_fixup_kernel<false><<<dim3((unsigned)blocks), dim3(gnc::kBlock), 0, (hipStream_t)stream_>>>(
        src, ld_src, rowptr, fix, n_fix, (int32_t)fix_blocks, (int32_t)num_nodes, feat_dim, out, ld_out);
  return gnc::check_launch("agg_fixup_kernel");
}

namespace {
template <bool ADD>
int launch_gather(const float* table, int64_t ld_table, const int32_t* index, const float* addend, int64_t ld_add,
                  int64_t num_rows, int32_t feat_dim, float* out, int64_t ld_out, hipStream_t stream) {
  const int64_t cap = gnc::num_cu() * 16;
  if (vec4_ok(table, ld_table, feat_dim) && vec4_ok(out, ld_out, feat_dim) && (!ADD || vec4_ok(addend, ld_add, feat_dim))) {
    const int lpr = pow2_lanes_for(feat_dim);
    const int rc = dispatch_lanes(lpr, [&](auto lanes) {
      gather_rows_vec4<decltype(lanes)::value, ADD><<<row_pass_grid(num_rows, lpr), dim3(gnc::kBlock), 0, stream>>>(
          table, ld_table, index, num_rows, feat_dim, out, ld_out, addend, ld_add);
    });
    if (rc) return rc;
    return gnc::check_launch("gather_rows_vec4");
  }
  int64_t blocks = gnc::ceil_div(num_rows * feat_dim, gnc::kBlock);
  if (blocks > cap) blocks = cap;
  gather_rows_scalar<ADD><<<dim3((unsigned)blocks), dim3(gnc::kBlock), 0, stream>>>(table, ld_table, index, num_rows, feat_dim,
                                                                                     out, ld_out, addend, ld_add);
  return gnc::check_launch("gather_rows_scalar");
}
}  // namespace

extern "C" int gnc_gather_rows_f32(const float* table, int64_t ld_table, const int32_t* index, int64_t num_rows,
                                   int32_t feat_dim, float* out, int64_t ld_out, void* stream_) {
  GNC_REQUIRE(num_rows >= 0 && feat_dim >= 0, "gnc_gather_rows_f32: negative size");
  if (num_rows == 0 || feat_dim == 0) return GNC_OK;
  GNC_REQUIRE(table && index && out, "gnc_gather_rows_f32: null pointer");
  GNC_REQUIRE(ld_table >= feat_dim && ld_out >= feat_dim, "gnc_gather_rows_f32: leading dimension < feat_dim");
  return launch_gather<false>(table, ld_table, index, nullptr, 0, num_rows, feat_dim, out, ld_out, (hipStream_t)stream_);
}

extern "C" int gnc_gather_rows_add_f32(const float* table, int64_t ld_table, const int32_t* index, const float* addend,
                                       int64_t ld_addend, int64_t num_rows, int32_t feat_dim, float* out, int64_t ld_out,
                                       void* stream_) {
  GNC_REQUIRE(num_rows >= 0 && feat_dim >= 0, "gnc_gather_rows_add_f32: negative size");
  if (num_rows == 0 || feat_dim == 0) return GNC_OK;
  GNC_REQUIRE(table && index && addend && out, "gnc_gather_rows_add_f32: null pointer");
  GNC_REQUIRE(ld_table >= feat_dim && ld_out >= feat_dim && ld_addend >= feat_dim,
              "gnc_gather_rows_add_f32: leading dimension < feat_dim");
  return launch_gather<true>(table, ld_table, index, addend, ld_addend, num_rows, feat_dim, out, ld_out, (hipStream_t)stream_);
}

// deferred validation (topology.py): a result computed from an edge_index with out-of-range ids must not look plausible.
// One launch that returns at once unless a flag is set (torch.where(flags.any(), nan, out) is three launches per forward).
__global__ __launch_bounds__(gnc::kBlock) void poison_if_flagged_kernel(float* __restrict__ out, int64_t count,
                                                                        const int32_t* __restrict__ flags, int nflags) {
  int any = 0;
  for (int k = 0; k < nflags; ++k) any |= flags[k];
  if (!any) return;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (int64_t)gridDim.x * blockDim.x)
    out[t] = __builtin_nanf("");
}

extern "C" int gnc_poison_if_flagged_f32(float* out, int64_t count, const int32_t* flags, int32_t nflags, void* stream_) {
  GNC_REQUIRE(count >= 0 && nflags >= 0 && nflags <= 16, "gnc_poison_if_flagged_f32: bad sizes");
  if (count == 0 || nflags == 0) return GNC_OK;
  GNC_REQUIRE(out && flags, "gnc_poison_if_flagged_f32: null pointer");
  int64_t blocks = gnc::ceil_div(count, gnc::kBlock);
  const int64_t cap = gnc::num_cu() * 4;
  if (blocks > cap) blocks = cap;
  poison_if_flagged_kernel<<<dim3((unsigned)blocks), dim3(gnc::kBlock), 0, (hipStream_t)stream_>>>(out, count, flags, nflags);
  return gnc::check_launch("poison_if_flagged_kernel");
}

extern "C" int gnc_edge_features_f32(const float* pos, int32_t space_dim, const int32_t* src, const int32_t* dst,
                                     int64_t num_edges, float* out, int64_t ld_out, void* stream_) {
  GNC_REQUIRE(num_edges >= 0 && space_dim >= 1 && space_dim <= 16 && ld_out >= space_dim + 1,
              "gnc_edge_features_f32: bad sizes");
  if (num_edges == 0) return GNC_OK;
  GNC_REQUIRE(pos && src && dst && out, "gnc_edge_features_f32: null pointer");
  int64_t blocks = gnc::ceil_div(num_edges, gnc::kBlock);
  const int64_t cap = gnc::num_cu() * 16;
  if (blocks > cap) blocks = cap;
  edge_features_kernel<<<dim3((unsigned)blocks), dim3(gnc::kBlock), 0, (hipStream_t)stream_>>>(pos, space_dim, src, dst,
                                                                                               num_edges, out, ld_out);
  return gnc::check_launch("edge_features_kernel");
}
