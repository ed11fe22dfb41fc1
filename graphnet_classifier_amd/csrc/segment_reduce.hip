// K18: mean and max neighbourhood aggregation over a destination-sorted CSR, their backward, and the division of an
// aggregate's rows by the in-degree.  Lane mapping, regimes and the order in which a destination's rows are folded
// are segment_csr.h's; this file holds the two folds, the division, and the backward's row.
//
// MEAN: the running sum exactly as K1 forms it (from +0.0, ascending k), then sum / (float)deg with a true fp32 division; a
//       destination without rows gives +0.0.  gnc_rows_div_degree_f32 applies the same division to an [N, D] table of K1 sums,
//       so "K1 (or the fused aggregation epilogue), then divide" gives the bits of the MEAN kernel.
// MAX:  the fold rule of K17 (pool_readout.hip, fold_max): the larger value wins, a NaN beats everything, a tie goes to the
//       lowest sorted position, -0.0 == +0.0.  A destination without rows gives +0.0 and argmax -1.  argmax holds the row of
//       `src` that won (perm[k], or k without a permutation) and is only written when the caller passes a pointer.
#include "gnc_common.h"
#include "segment_csr.h"

#include <math.h>

namespace {

using namespace gnc_csr;

constexpr int kMean = GNC_SEGMENT_MEAN;
constexpr int kMax = GNC_SEGMENT_MAX;

// One candidate folded into the running (value, row) pair; candidates arrive in ascending sorted position, so "keep on a tie"
// is "the lowest position wins".  The first candidate always enters (row < 0 marks "none yet"; without ARG the identity -inf
// does the same, since a first -inf leaves -inf).  Once the value is NaN nothing replaces it: argmax stays at the first NaN.
template <bool ARG>
__device__ __forceinline__ void fold1(float& av, int32_t& ai, float bv, int32_t bi) {
  // (bitwise, and selects instead of an `if`: the fold is four compares and two selects per value, no branch on the data)
  const bool take = (av == av) & ((bv != bv) | (bv > av) | (ARG & (ai < 0)));
  av = take ? bv : av;
  if (ARG) ai = take ? bi : ai;
}

template <int MODE, bool ARG>
__device__ __forceinline__ void fold4(f4& a, i4& ix, const f4& b, int32_t row) {
  if (MODE == kMean) {
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
  } else {
    fold1<ARG>(a.x, ix.x, b.x, row);
    fold1<ARG>(a.y, ix.y, b.y, row);
    fold1<ARG>(a.z, ix.z, b.z, row);
    fold1<ARG>(a.w, ix.w, b.w, row);
  }
}

__device__ __forceinline__ float mean_of(float sum, float deg) { return sum / deg; }  // THE division of K18 (no fast-math)

// Rows [start, end) of one destination, columns [col, col + 4), folded from the mode's identity.  Returns the finished output
// slice (and the winners' rows).
template <bool HAS_PERM, int MODE, bool ARG, bool STREAM>
__device__ __forceinline__ void reduce_rows(const float* __restrict__ src, int64_t ld_src, const int32_t* __restrict__ perm,
                                            int32_t start, int32_t end, int col, f4& a, i4& ix) {
  const float init = MODE == kMean ? 0.f : -INFINITY;
  a = f4{init, init, init, init};
  ix = i4{-1, -1, -1, -1};
  walk_rows<HAS_PERM, STREAM>(src, ld_src, perm, start, end, col, no_side{},
                              [&](int32_t row, Nothing, const f4& x) { fold4<MODE, ARG>(a, ix, x, row); });
  const int32_t deg = end - start;
  if (MODE == kMean) {
    if (deg > 0) {
      const float fd = (float)deg;
      a = f4{mean_of(a.x, fd), mean_of(a.y, fd), mean_of(a.z, fd), mean_of(a.w, fd)};
    }
  } else if (deg <= 0) {
    a = f4{0.f, 0.f, 0.f, 0.f};
  }
}

// the finished slice of destination v (and its winners) stored
template <bool HAS_PERM, int MODE, bool ARG, bool STREAM>
__device__ __forceinline__ void reduce_and_store(const float* __restrict__ src, int64_t ld_src, const int32_t* __restrict__ perm,
                                                 int64_t v, int32_t start, int32_t end, int col, int32_t feat_dim,
                                                 float* __restrict__ out, int64_t ld_out, int32_t* __restrict__ argmax) {
  f4 a;
  i4 ix;
  reduce_rows<HAS_PERM, MODE, ARG, STREAM>(src, ld_src, perm, start, end, col, a, ix);
  st4(out + v * ld_out + col, a);
  if (ARG) st4i(argmax + v * feat_dim + col, ix);
}

// chunk regime
template <int LPR, bool HAS_PERM, int MODE, bool ARG>
__global__ __launch_bounds__(gnc::kBlock) void segment_reduce_csr_vec4(
    const float* __restrict__ src, int64_t ld_src, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ perm,
    int32_t num_nodes, int32_t feat_dim, float* __restrict__ out, int64_t ld_out, int32_t* __restrict__ argmax) {
  for_chunk_destinations<LPR>(rowptr, num_nodes, feat_dim, [&](int64_t v, int32_t start, int32_t end, int col) {
    reduce_and_store<HAS_PERM, MODE, ARG, true>(src, ld_src, perm, v, start, end, col, feat_dim, out, ld_out, argmax);
  });
}

// small regime; same folds, same bits
template <int LPR, bool HAS_PERM, int MODE, bool ARG>
__global__ __launch_bounds__(gnc::kBlock) void segment_reduce_csr_small(
    const float* __restrict__ src, int64_t ld_src, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ perm,
    int32_t num_nodes, int32_t feat_dim, float* __restrict__ out, int64_t ld_out, int32_t* __restrict__ argmax) {
  for_small_destinations<LPR>(rowptr, num_nodes, feat_dim, [&](int64_t v, int32_t start, int32_t end, int col) {
    reduce_and_store<HAS_PERM, MODE, ARG, false>(src, ld_src, perm, v, start, end, col, feat_dim, out, ld_out, argmax);
  });
}

// scalar regime
template <bool HAS_PERM, int MODE>
__global__ __launch_bounds__(gnc::kBlock) void segment_reduce_csr_scalar(
    const float* __restrict__ src, int64_t ld_src, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ perm,
    int32_t num_nodes, int32_t feat_dim, float* __restrict__ out, int64_t ld_out, int32_t* __restrict__ argmax) {
  for_scalar_destinations(rowptr, num_nodes, feat_dim, no_side{}, [&](int64_t v, int32_t start, int32_t end, int c, Nothing) {
    const int32_t deg = end - start;
    float a = MODE == kMean ? 0.f : -INFINITY;
    int32_t ai = -1;
    walk_rows_scalar<HAS_PERM>(src, ld_src, perm, start, end, c, [&](int32_t i, float b) {
      if (MODE == kMean) a += b;
      else fold1<true>(a, ai, b, i);
    });
    if (MODE == kMean) {
      if (deg > 0) a = mean_of(a, (float)deg);
    } else if (deg <= 0) {
      a = 0.f;
    }
    out[v * ld_out + c] = a;
    if (MODE == kMax && argmax) argmax[v * feat_dim + c] = ai;
  });
}

// ---------------------------------------------------------------------------------------
// backward: one row pass over the E rows of grad_src
// ---------------------------------------------------------------------------------------
template <int MODE>
__device__ __forceinline__ f4 backward_row(const float* __restrict__ grad_out, int64_t ld_grad, const int32_t* __restrict__ rowptr,
                                           const int32_t* __restrict__ argmax, int32_t feat_dim, int32_t d, int32_t row, int col) {
  const f4 g = ld4(grad_out + (int64_t)d * ld_grad + col);
  if (MODE == kMean) {
    const float fd = (float)(rowptr[d + 1] - rowptr[d]);  // >= 1: row `row` is one of them
    return f4{mean_of(g.x, fd), mean_of(g.y, fd), mean_of(g.z, fd), mean_of(g.w, fd)};
  }
  const i4 am = *reinterpret_cast<const i4*>(argmax + (int64_t)d * feat_dim + col);
  return f4{am.x == row ? g.x : 0.f, am.y == row ? g.y : 0.f, am.z == row ? g.z : 0.f, am.w == row ? g.w : 0.f};
}

template <int LPR, int MODE>
__global__ __launch_bounds__(gnc::kBlock) void segment_reduce_backward_vec4(
    const float* __restrict__ grad_out, int64_t ld_grad, const int32_t* __restrict__ dst_of_row, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ argmax, int64_t num_rows, int32_t feat_dim, float* __restrict__ grad_src, int64_t ld_src) {
  const int col = row_pass_col<LPR>();
  if (col >= feat_dim) return;
  for_rows_two_in_flight<LPR>(
      num_rows,
      [&](int64_t r) { return backward_row<MODE>(grad_out, ld_grad, rowptr, argmax, feat_dim, dst_of_row[r], (int32_t)r, col); },
      [&](int64_t r, const f4& g) { st4(grad_src + r * ld_src + col, g); });
}

template <int MODE>
__global__ __launch_bounds__(gnc::kBlock) void segment_reduce_backward_scalar(
    const float* __restrict__ grad_out, int64_t ld_grad, const int32_t* __restrict__ dst_of_row, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ argmax, int64_t num_rows, int32_t feat_dim, float* __restrict__ grad_src, int64_t ld_src) {
  const int64_t total = num_rows * feat_dim;
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; t < total; t += stride) {
    const int64_t r = t / feat_dim;
    const int c = (int)(t - r * feat_dim);
    const int32_t d = dst_of_row[r];
    const float g = grad_out[(int64_t)d * ld_grad + c];
    float v;
    if (MODE == kMean) v = mean_of(g, (float)(rowptr[d + 1] - rowptr[d]));
    else v = argmax[(int64_t)d * feat_dim + c] == (int32_t)r ? g : 0.f;
    grad_src[r * ld_src + c] = v;
  }
}

// ---------------------------------------------------------------------------------------
// table[v, :] /= (float)deg(v) in place, rows of degree 0 untouched; one item = VEC columns of one row
// ---------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(gnc::kBlock) void rows_div_degree_kernel(float* __restrict__ table, int64_t ld,
                                                                      const int32_t* __restrict__ rowptr, int64_t num_nodes,
                                                                      int32_t feat_dim) {
  const int64_t per_row = feat_dim / VEC;
  const int64_t items = num_nodes * per_row;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = i / per_row;
    const int c = (int)(i - v * per_row) * VEC;
    const int32_t deg = rowptr[v + 1] - rowptr[v];
    if (deg <= 0) continue;
    const float fd = (float)deg;
    float* p = table + v * ld + c;
    if constexpr (VEC == 4) {
      const f4 a = ld4(p);
      st4(p, f4{mean_of(a.x, fd), mean_of(a.y, fd), mean_of(a.z, fd), mean_of(a.w, fd)});
    } else {
      p[0] = mean_of(p[0], fd);
    }
  }
}

struct FwdArgs {
  const float* src;
  int64_t ld_src;
  const int32_t* rowptr;
  const int32_t* perm;
  int32_t n, d;
  float* out;
  int64_t ld_out;
  int32_t* argmax;
};

template <bool HAS_PERM, int MODE, bool ARG>
int launch_vec(const FwdArgs& a, hipStream_t stream) {
  const ForwardPlan p = forward_plan(a.n, a.d);
  const dim3 block(gnc::kBlock);
  const int rc = dispatch_lanes(p.lpr, [&](auto lanes) {
    constexpr int L = decltype(lanes)::value;
    if (p.small)
      segment_reduce_csr_small<L, HAS_PERM, MODE, ARG><<<p.grid, block, 0, stream>>>(a.src, a.ld_src, a.rowptr, a.perm, a.n, a.d,
                                                                                      a.out, a.ld_out, a.argmax);
    else
      segment_reduce_csr_vec4<L, HAS_PERM, MODE, ARG><<<p.grid, block, 0, stream>>>(a.src, a.ld_src, a.rowptr, a.perm, a.n, a.d,
                                                                                     a.out, a.ld_out, a.argmax);
  });
  return rc ? rc : gnc::check_launch(p.small ? "segment_reduce_csr_small" : "segment_reduce_csr_vec4");
}

template <bool HAS_PERM>
int launch_forward(const FwdArgs& a, int mode, hipStream_t stream) {
  const bool vec = vec4_ok(a.src, a.ld_src, a.d) && vec4_ok(a.out, a.ld_out, a.d) && (!a.argmax || gnc::aligned16(a.argmax));
  if (vec) {
    if (mode == kMean) return launch_vec<HAS_PERM, kMean, false>(a, stream);
    if (a.argmax) return launch_vec<HAS_PERM, kMax, true>(a, stream);
    return launch_vec<HAS_PERM, kMax, false>(a, stream);
  }
  const dim3 grid = scalar_grid(a.n), block(gnc::kBlock);
  if (mode == kMean)
    segment_reduce_csr_scalar<HAS_PERM, kMean><<<grid, block, 0, stream>>>(a.src, a.ld_src, a.rowptr, a.perm, a.n, a.d, a.out,
                                                                          a.ld_out, nullptr);
  else
    segment_reduce_csr_scalar<HAS_PERM, kMax><<<grid, block, 0, stream>>>(a.src, a.ld_src, a.rowptr, a.perm, a.n, a.d, a.out,
                                                                         a.ld_out, a.argmax);
  return gnc::check_launch("segment_reduce_csr_scalar");
}

template <int MODE>
int launch_backward(const float* grad_out, int64_t ld_grad, const int32_t* dst_of_row, const int32_t* rowptr, const int32_t* argmax,
                    int64_t num_rows, int32_t d, float* grad_src, int64_t ld_src, hipStream_t stream) {
  if (vec4_ok(grad_out, ld_grad, d) && vec4_ok(grad_src, ld_src, d) && (MODE == kMean || gnc::aligned16(argmax))) {
    const int lpr = pow2_lanes_for(d);
    const int rc = dispatch_lanes(lpr, [&](auto lanes) {
      segment_reduce_backward_vec4<decltype(lanes)::value, MODE><<<row_pass_grid(num_rows, lpr), dim3(gnc::kBlock), 0, stream>>>(
          grad_out, ld_grad, dst_of_row, rowptr, argmax, num_rows, d, grad_src, ld_src);
    });
    if (rc) return rc;
    return gnc::check_launch("segment_reduce_backward_vec4");
  }
  const int64_t blocks = gnc::capped_blocks(num_rows * d, gnc::kBlock, 16);
  segment_reduce_backward_scalar<MODE><<<dim3((unsigned)blocks), dim3(gnc::kBlock), 0, stream>>>(
      grad_out, ld_grad, dst_of_row, rowptr, argmax, num_rows, d, grad_src, ld_src);
  return gnc::check_launch("segment_reduce_backward_scalar");
}

}  // namespace

extern "C" int gnc_segment_reduce_csr_f32(const float* src, int64_t ld_src, const int32_t* rowptr, const int32_t* perm,
                                          int64_t num_nodes, int64_t num_edges, int32_t feat_dim, int32_t mode, float* out,
                                          int64_t ld_out, int32_t* argmax, void* stream_) {
  GNC_REQUIRE(mode == GNC_SEGMENT_MEAN || mode == GNC_SEGMENT_MAX, "gnc_segment_reduce_csr_f32: mode %d is neither MEAN nor MAX",
              (int)mode);
  GNC_REQUIRE(num_nodes >= 0 && num_edges >= 0 && feat_dim >= 0, "gnc_segment_reduce_csr_f32: negative size");
  GNC_REQUIRE(num_nodes < INT32_MAX && num_edges < INT32_MAX, "gnc_segment_reduce_csr_f32: sizes exceed int32");
  GNC_REQUIRE(mode == GNC_SEGMENT_MAX || !argmax, "gnc_segment_reduce_csr_f32: argmax goes with MAX only");
  if (num_nodes == 0 || feat_dim == 0) return GNC_OK;
  GNC_REQUIRE(rowptr && out, "gnc_segment_reduce_csr_f32: null rowptr/out");
  GNC_REQUIRE(num_edges == 0 || src, "gnc_segment_reduce_csr_f32: null src");
  GNC_REQUIRE(ld_src >= feat_dim && ld_out >= feat_dim, "gnc_segment_reduce_csr_f32: leading dimension < feat_dim");
  GNC_REQUIRE((reinterpret_cast<uintptr_t>(src) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0 &&
                  (reinterpret_cast<uintptr_t>(argmax) & 3u) == 0,
              "gnc_segment_reduce_csr_f32: a pointer is not aligned to its element size");
  const FwdArgs a = {src, ld_src, rowptr, perm, (int32_t)num_nodes, feat_dim, out, ld_out, argmax};
  hipStream_t stream = (hipStream_t)stream_;
  return perm ? launch_forward<true>(a, mode, stream) : launch_forward<false>(a, mode, stream);
}

extern "C" int gnc_segment_reduce_backward_f32(const float* grad_out, int64_t ld_grad, const int32_t* dst_of_row,
                                               const int32_t* rowptr, const int32_t* argmax, int64_t num_nodes, int64_t num_rows,
                                               int32_t feat_dim, int32_t mode, float* grad_src, int64_t ld_src, void* stream_) {
  GNC_REQUIRE(mode == GNC_SEGMENT_MEAN || mode == GNC_SEGMENT_MAX, "gnc_segment_reduce_backward_f32: mode %d is neither MEAN nor MAX",
              (int)mode);
  GNC_REQUIRE(num_nodes >= 0 && num_rows >= 0 && feat_dim >= 0, "gnc_segment_reduce_backward_f32: negative size");
  GNC_REQUIRE(num_nodes < INT32_MAX && num_rows < INT32_MAX, "gnc_segment_reduce_backward_f32: sizes exceed int32");
  if (num_rows == 0 || feat_dim == 0) return GNC_OK;
  GNC_REQUIRE(num_nodes > 0, "gnc_segment_reduce_backward_f32: rows without a destination");
  GNC_REQUIRE(grad_out && dst_of_row && grad_src, "gnc_segment_reduce_backward_f32: null pointer");
  GNC_REQUIRE(mode == GNC_SEGMENT_MEAN ? rowptr != nullptr : argmax != nullptr,
              "gnc_segment_reduce_backward_f32: MEAN needs rowptr, MAX needs argmax");
  GNC_REQUIRE(ld_grad >= feat_dim && ld_src >= feat_dim, "gnc_segment_reduce_backward_f32: leading dimension < feat_dim");
  GNC_REQUIRE((reinterpret_cast<uintptr_t>(grad_out) & 3u) == 0 && (reinterpret_cast<uintptr_t>(grad_src) & 3u) == 0 &&
                  (reinterpret_cast<uintptr_t>(argmax) & 3u) == 0,
              "gnc_segment_reduce_backward_f32: a pointer is not aligned to its element size");
  hipStream_t stream = (hipStream_t)stream_;
  if (mode == GNC_SEGMENT_MEAN)
    return launch_backward<kMean>(grad_out, ld_grad, dst_of_row, rowptr, nullptr, num_rows, feat_dim, grad_src, ld_src, stream);
  return launch_backward<kMax>(grad_out, ld_grad, dst_of_row, rowptr, argmax, num_rows, feat_dim, grad_src, ld_src, stream);
}

extern "C" int gnc_rows_div_degree_f32(float* table, int64_t ld, const int32_t* rowptr, int64_t num_nodes, int32_t feat_dim,
                                       void* stream_) {
  GNC_REQUIRE(num_nodes >= 0 && feat_dim >= 0, "gnc_rows_div_degree_f32: negative size");
  GNC_REQUIRE(num_nodes < INT32_MAX, "gnc_rows_div_degree_f32: sizes exceed int32");
  if (num_nodes == 0 || feat_dim == 0) return GNC_OK;
  GNC_REQUIRE(table && rowptr, "gnc_rows_div_degree_f32: null pointer");
  GNC_REQUIRE(ld >= feat_dim, "gnc_rows_div_degree_f32: leading dimension < feat_dim");
  GNC_REQUIRE((reinterpret_cast<uintptr_t>(table) & 3u) == 0, "gnc_rows_div_degree_f32: table is not aligned to its element size");
  const bool vec = feat_dim % 4 == 0 && ld % 4 == 0 && gnc::aligned16(table);
  const int64_t blocks = gnc::capped_blocks(num_nodes * (feat_dim / (vec ? 4 : 1)), gnc::kBlock, 16);
  const dim3 grid((unsigned)blocks), block(gnc::kBlock);
  hipStream_t stream = (hipStream_t)stream_;
  if (vec) rows_div_degree_kernel<4><<<grid, block, 0, stream>>>(table, ld, rowptr, num_nodes, feat_dim);
  else rows_div_degree_kernel<1><<<grid, block, 0, stream>>>(table, ld, rowptr, num_nodes, feat_dim);
  return gnc::check_launch("rows_div_degree_kernel");
}
