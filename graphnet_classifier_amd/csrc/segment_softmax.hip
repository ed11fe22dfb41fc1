// K21: attention neighbourhood aggregation over a destination-sorted CSR - a softmax-weighted sum of a destination's incoming
// rows - its backward, and the weights themselves.  Lane mapping, regimes and the order in which a destination's
// rows are folded are segment_csr.h's; this file holds the softmax arithmetic.
//
// Per destination v with rows k, message rows x_k and one score s_k per row:
//   m = max_k s_k                    first pass over the scores (fmaxf from -inf: a NaN score does not enter m)
//   e_k = expf(s_k - m)              second pass over the scores, which is also the ONE pass over the rows:
//   acc[c] = fmaf(e_k, x_k[c], acc[c])  and  Z += e_k,  both from +0.0 in ascending k
//   out[v, c] = acc[c] / Z           a true fp32 division (no fast-math);  saved[v] = (m, Z)
// A destination without rows gives +0.0 and saved (0, 0); nothing is divided.  With all scores of a destination equal, s_k - m is
// +0.0, e_k is 1.0f, the fmaf is the plain add and Z is (float)deg: the bits of K18's MEAN kernel.  A NaN score makes Z and the
// row of ITS destination NaN and touches nothing else; a -inf score among finite ones has e_k = +0.0 and adds nothing.
// The lanes of a group read the same score (one address per group); every lane forms m, e_k and Z itself, so no lane waits for
// another and the three kernels give the same bits.
//
// Backward, one pass over the E rows, alpha_r = expf(s_r - m_d) / Z_d recomputed from `saved` (no [E] array is stored):
//   grad_src[r, :] = alpha_r grad_out[d, :]      grad_score[r] = alpha_r sum_c grad_out[d, c] (src[r, c] - out[d, c])
// Each lane sums its four columns in order, the row's lanes are then added by a fixed xor tree (no LDS).
#include "gnc_common.h"
#include "segment_csr.h"

#include <math.h>

namespace {

using namespace gnc_csr;

__device__ __forceinline__ float weight_of(float s, float m) { return expf(s - m); }  // e_k, unnormalised
__device__ __forceinline__ float over(float a, float z) { return a / z; }             // THE division of K21 (no fast-math)

// one row folded into the running numerator and into Z
__device__ __forceinline__ void fold_row(f4& a, float& z, float e, const f4& x) {
  a.x = fmaf(e, x.x, a.x);
  a.y = fmaf(e, x.y, a.y);
  a.z = fmaf(e, x.z, a.z);
  a.w = fmaf(e, x.w, a.w);
  z += e;
}

// first pass: the largest score of rows [start, end); -inf for none (and for NaN scores only)
template <bool HAS_PERM>
__device__ __forceinline__ float max_score(const float* __restrict__ scores, const int32_t* __restrict__ perm, int32_t start,
                                           int32_t end) {
  float m = -INFINITY;
  int32_t k = start;
  for (; k + 4 <= end; k += 4) {
    const float s0 = scores[HAS_PERM ? perm[k] : k], s1 = scores[HAS_PERM ? perm[k + 1] : k + 1];
    const float s2 = scores[HAS_PERM ? perm[k + 2] : k + 2], s3 = scores[HAS_PERM ? perm[k + 3] : k + 3];
    m = fmaxf(fmaxf(fmaxf(fmaxf(m, s0), s1), s2), s3);
  }
  for (; k < end; ++k) m = fmaxf(m, scores[HAS_PERM ? perm[k] : k]);
  return m;
}

// Rows [start, end) of one destination, columns [col, col + 4); a row's score is requested with the row.  Returns the finished
// output slice and (m, Z).
template <bool HAS_PERM, bool STREAM>
__device__ __forceinline__ void softmax_rows(const float* __restrict__ src, int64_t ld_src, const float* __restrict__ scores,
                                             const int32_t* __restrict__ perm, int32_t start, int32_t end, int col, f4& a,
                                             float& m, float& z) {
  m = max_score<HAS_PERM>(scores, perm, start, end);
  a = f4{0.f, 0.f, 0.f, 0.f};
  z = 0.f;
  walk_rows<HAS_PERM, STREAM>(
      src, ld_src, perm, start, end, col, [&](int32_t row) { return scores[row]; },
      [&](int32_t, float s, const f4& x) { fold_row(a, z, weight_of(s, m), x); });
  if (end > start) a = f4{over(a.x, z), over(a.y, z), over(a.z, z), over(a.w, z)};
  else m = 0.f;  // no rows: out +0.0, saved (0, 0)
}

__device__ __forceinline__ void store_saved(float* __restrict__ saved, int64_t v, float m, float z) {
  saved[2 * v] = m;
  saved[2 * v + 1] = z;
}

// the finished slice of destination v stored; the lane of column 0 stores (m, Z)
template <bool HAS_PERM, bool STREAM>
__device__ __forceinline__ void softmax_and_store(const float* __restrict__ src, int64_t ld_src, const float* __restrict__ scores,
                                                  const int32_t* __restrict__ perm, int64_t v, int32_t start, int32_t end, int col,
                                                  float* __restrict__ out, int64_t ld_out, float* __restrict__ saved) {
  f4 a;
  float m, z;
  softmax_rows<HAS_PERM, STREAM>(src, ld_src, scores, perm, start, end, col, a, m, z);
  st4(out + v * ld_out + col, a);
  if (col == 0) store_saved(saved, v, m, z);
}

// chunk regime
template <int LPR, bool HAS_PERM>
__global__ __launch_bounds__(gnc::kBlock) void segment_softmax_csr_vec4(
    const float* __restrict__ src, int64_t ld_src, const float* __restrict__ scores, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ perm, int32_t num_nodes, int32_t feat_dim, float* __restrict__ out, int64_t ld_out,
    float* __restrict__ saved) {
  for_chunk_destinations<LPR>(rowptr, num_nodes, feat_dim, [&](int64_t v, int32_t start, int32_t end, int col) {
    softmax_and_store<HAS_PERM, true>(src, ld_src, scores, perm, v, start, end, col, out, ld_out, saved);
  });
}

// small regime; same folds, same bits
template <int LPR, bool HAS_PERM>
__global__ __launch_bounds__(gnc::kBlock) void segment_softmax_csr_small(
    const float* __restrict__ src, int64_t ld_src, const float* __restrict__ scores, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ perm, int32_t num_nodes, int32_t feat_dim, float* __restrict__ out, int64_t ld_out,
    float* __restrict__ saved) {
  for_small_destinations<LPR>(rowptr, num_nodes, feat_dim, [&](int64_t v, int32_t start, int32_t end, int col) {
    softmax_and_store<HAS_PERM, false>(src, ld_src, scores, perm, v, start, end, col, out, ld_out, saved);
  });
}

// scalar regime
template <bool HAS_PERM>
__global__ __launch_bounds__(gnc::kBlock) void segment_softmax_csr_scalar(
    const float* __restrict__ src, int64_t ld_src, const float* __restrict__ scores, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ perm, int32_t num_nodes, int32_t feat_dim, float* __restrict__ out, int64_t ld_out,
    float* __restrict__ saved) {
  for_scalar_destinations(
      rowptr, num_nodes, feat_dim, [&](int64_t, int32_t start, int32_t end) { return max_score<HAS_PERM>(scores, perm, start, end); },
      [&](int64_t v, int32_t start, int32_t end, int c, float m) {
        float a = 0.f, z = 0.f;
        walk_rows_scalar<HAS_PERM>(src, ld_src, perm, start, end, c, [&](int32_t i, float x) {
          const float e = weight_of(scores[i], m);
          a = fmaf(e, x, a);
          z += e;
        });
        if (end > start) a = over(a, z);
        out[v * ld_out + c] = a;
        if (c == 0) store_saved(saved, v, end > start ? m : 0.f, z);
      });
}

// ---------------------------------------------------------------------------------------
// backward: one row pass over the E rows, plus the dot product over the row's lanes
// ---------------------------------------------------------------------------------------
struct BwdArgs {
  const float* grad_out;
  int64_t ld_grad;
  const float* src;
  int64_t ld_src;
  const float* scores;
  const float* out;
  int64_t ld_out;
  const float* saved;
  const int32_t* dst_of_row;
  int64_t num_rows;
  int32_t feat_dim;
  float* grad_src;
  int64_t ld_gsrc;
  float* grad_scores;
};

__device__ __forceinline__ float alpha_of(const float* __restrict__ scores, const float* __restrict__ saved, int64_t r, int32_t d) {
  return over(weight_of(scores[r], saved[2 * (int64_t)d]), saved[2 * (int64_t)d + 1]);
}

// the row's lanes added by a fixed xor tree: every lane of the group ends with the same sum
template <int LPR>
__device__ __forceinline__ float group_sum(float p) {
#pragma unroll
  for (int off = LPR / 2; off >= 1; off >>= 1) p += __shfl_xor(p, off, kWave);
  return p;
}

struct BwdRow {
  float alpha;
  f4 g, x, o;
};

__device__ __forceinline__ BwdRow load_row(const BwdArgs& a, int64_t r, int col, bool col_ok) {
  BwdRow w;
  const int32_t d = a.dst_of_row[r];
  w.alpha = alpha_of(a.scores, a.saved, r, d);
  const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
  w.g = col_ok ? ld4(a.grad_out + (int64_t)d * a.ld_grad + col) : zero;
  w.x = col_ok ? ld4(a.src + r * a.ld_src + col) : zero;
  w.o = col_ok ? ld4(a.out + (int64_t)d * a.ld_out + col) : zero;
  return w;
}

template <int LPR>
__device__ __forceinline__ void finish_row(const BwdArgs& a, const BwdRow& w, int64_t r, int col, bool col_ok) {
  if (col_ok) st4(a.grad_src + r * a.ld_gsrc + col, f4{w.alpha * w.g.x, w.alpha * w.g.y, w.alpha * w.g.z, w.alpha * w.g.w});
  float p = w.g.x * (w.x.x - w.o.x);  // the lane's four columns in order
  p = fmaf(w.g.y, w.x.y - w.o.y, p);
  p = fmaf(w.g.z, w.x.z - w.o.z, p);
  p = fmaf(w.g.w, w.x.w - w.o.w, p);
  p = group_sum<LPR>(p);
  if (col == 0) a.grad_scores[r] = w.alpha * p;
}

// (a lane whose columns lie beyond feat_dim stays in the loop with zeros: its group's tree reads it)
// The row pass written out, not for_rows_two_in_flight (segment_csr.h says why): through the helper this loop came out five
// scalar instructions longer and measured 0.9 % slower at c3 size.
template <int LPR>
__global__ __launch_bounds__(gnc::kBlock) void segment_softmax_backward_vec4(const BwdArgs a) {
  constexpr int RPB = gnc::kBlock / LPR;  // rows per block pass
  const int col = row_pass_col<LPR>();
  const bool col_ok = col < a.feat_dim;
  int64_t r = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const int64_t stride = (int64_t)gridDim.x * RPB;
  for (; r + stride < a.num_rows; r += 2 * stride) {
    const BwdRow w0 = load_row(a, r, col, col_ok);
    const BwdRow w1 = load_row(a, r + stride, col, col_ok);
    finish_row<LPR>(a, w0, r, col, col_ok);
    finish_row<LPR>(a, w1, r + stride, col, col_ok);
  }
  if (r < a.num_rows) finish_row<LPR>(a, load_row(a, r, col, col_ok), r, col, col_ok);
}

// generic: one wave per row, scalar columns; each lane sums its columns in ascending order, then the wave's xor tree
__global__ __launch_bounds__(gnc::kBlock) void segment_softmax_backward_scalar(const BwdArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t num_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t r = wave; r < a.num_rows; r += num_waves) {  // wave-uniform: all 64 lanes reach the tree
    const int32_t d = a.dst_of_row[r];
    const float alpha = alpha_of(a.scores, a.saved, r, d);
    float p = 0.f;
    for (int c = lane; c < a.feat_dim; c += kWave) {
      const float g = a.grad_out[(int64_t)d * a.ld_grad + c];
      a.grad_src[r * a.ld_gsrc + c] = alpha * g;
      p = fmaf(g, a.src[r * a.ld_src + c] - a.out[(int64_t)d * a.ld_out + c], p);
    }
    p = group_sum<kWave>(p);
    if (lane == 0) a.grad_scores[r] = alpha * p;
  }
}

__global__ __launch_bounds__(gnc::kBlock) void segment_softmax_weights_kernel(const float* __restrict__ scores,
                                                                              const float* __restrict__ saved,
                                                                              const int32_t* __restrict__ dst_of_row,
                                                                              int64_t num_rows, float* __restrict__ alpha) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < num_rows; r += (int64_t)gridDim.x * blockDim.x)
    alpha[r] = alpha_of(scores, saved, r, dst_of_row[r]);
}

bool aligned4(const void* p) { return gnc::aligned_to(p, 4); }

struct FwdArgs {
  const float* src;
  int64_t ld_src;
  const float* scores;
  const int32_t* rowptr;
  const int32_t* perm;
  int32_t n, d;
  float* out;
  int64_t ld_out;
  float* saved;
};

template <bool HAS_PERM>
int launch_forward(const FwdArgs& a, hipStream_t stream) {
  const dim3 block(gnc::kBlock);
  if (vec4_ok(a.src, a.ld_src, a.d) && vec4_ok(a.out, a.ld_out, a.d)) {
    const ForwardPlan p = forward_plan(a.n, a.d);
    const int rc = dispatch_lanes(p.lpr, [&](auto lanes) {
      constexpr int L = decltype(lanes)::value;
      if (p.small)
        segment_softmax_csr_small<L, HAS_PERM><<<p.grid, block, 0, stream>>>(a.src, a.ld_src, a.scores, a.rowptr, a.perm, a.n, a.d,
                                                                             a.out, a.ld_out, a.saved);
      else
        segment_softmax_csr_vec4<L, HAS_PERM><<<p.grid, block, 0, stream>>>(a.src, a.ld_src, a.scores, a.rowptr, a.perm, a.n, a.d,
                                                                            a.out, a.ld_out, a.saved);
    });
    return rc ? rc : gnc::check_launch(p.small ? "segment_softmax_csr_small" : "segment_softmax_csr_vec4");
  }
  segment_softmax_csr_scalar<HAS_PERM><<<scalar_grid(a.n), block, 0, stream>>>(
      a.src, a.ld_src, a.scores, a.rowptr, a.perm, a.n, a.d, a.out, a.ld_out, a.saved);
  return gnc::check_launch("segment_softmax_csr_scalar");
}

int launch_backward(const BwdArgs& a, hipStream_t stream) {
  const int d = a.feat_dim;
  if (vec4_ok(a.grad_out, a.ld_grad, d) && vec4_ok(a.src, a.ld_src, d) && vec4_ok(a.out, a.ld_out, d) &&
      vec4_ok(a.grad_src, a.ld_gsrc, d)) {
    const int lpr = pow2_lanes_for(d);
    const int rc = dispatch_lanes(lpr, [&](auto lanes) {
      segment_softmax_backward_vec4<decltype(lanes)::value><<<row_pass_grid(a.num_rows, lpr), dim3(gnc::kBlock), 0, stream>>>(a);
    });
    if (rc) return rc;
    return gnc::check_launch("segment_softmax_backward_vec4");
  }
  segment_softmax_backward_scalar<<<scalar_grid(a.num_rows), dim3(gnc::kBlock), 0, stream>>>(a);
  return gnc::check_launch("segment_softmax_backward_scalar");
}

}  // namespace

extern "C" int gnc_segment_softmax_csr_f32(const float* src, int64_t ld_src, const float* scores, const int32_t* rowptr,
                                           const int32_t* perm, int64_t num_nodes, int64_t num_edges, int32_t feat_dim, float* out,
                                           int64_t ld_out, float* saved, void* stream_) {
  GNC_REQUIRE(num_nodes >= 0 && num_edges >= 0 && feat_dim >= 0, "gnc_segment_softmax_csr_f32: negative size");
  GNC_REQUIRE(num_nodes < INT32_MAX && num_edges < INT32_MAX, "gnc_segment_softmax_csr_f32: sizes exceed int32");
  if (num_nodes == 0 || feat_dim == 0) return GNC_OK;
  GNC_REQUIRE(rowptr && out && saved, "gnc_segment_softmax_csr_f32: null rowptr/out/saved");
  GNC_REQUIRE(num_edges == 0 || (src && scores), "gnc_segment_softmax_csr_f32: null src/scores");
  GNC_REQUIRE(ld_src >= feat_dim && ld_out >= feat_dim, "gnc_segment_softmax_csr_f32: leading dimension < feat_dim");
  GNC_REQUIRE(aligned4(src) && aligned4(scores) && aligned4(out) && aligned4(saved),
              "gnc_segment_softmax_csr_f32: a pointer is not aligned to its element size");
  const FwdArgs a = {src, ld_src, scores, rowptr, perm, (int32_t)num_nodes, feat_dim, out, ld_out, saved};
  hipStream_t stream = (hipStream_t)stream_;
  return perm ? launch_forward<true>(a, stream) : launch_forward<false>(a, stream);
}

extern "C" int gnc_segment_softmax_backward_f32(const float* grad_out, int64_t ld_grad, const float* src, int64_t ld_src,
                                                const float* scores, const float* out, int64_t ld_out, const float* saved,
                                                const int32_t* dst_of_row, int64_t num_nodes, int64_t num_rows, int32_t feat_dim,
                                                float* grad_src, int64_t ld_gsrc, float* grad_scores, void* stream_) {
  GNC_REQUIRE(num_nodes >= 0 && num_rows >= 0 && feat_dim >= 0, "gnc_segment_softmax_backward_f32: negative size");
  GNC_REQUIRE(num_nodes < INT32_MAX && num_rows < INT32_MAX, "gnc_segment_softmax_backward_f32: sizes exceed int32");
  if (num_rows == 0 || feat_dim == 0) return GNC_OK;
  GNC_REQUIRE(num_nodes > 0, "gnc_segment_softmax_backward_f32: rows without a destination");
  GNC_REQUIRE(grad_out && src && scores && out && saved && dst_of_row && grad_src && grad_scores,
              "gnc_segment_softmax_backward_f32: null pointer");
  GNC_REQUIRE(ld_grad >= feat_dim && ld_src >= feat_dim && ld_out >= feat_dim && ld_gsrc >= feat_dim,
              "gnc_segment_softmax_backward_f32: leading dimension < feat_dim");
  GNC_REQUIRE(aligned4(grad_out) && aligned4(src) && aligned4(scores) && aligned4(out) && aligned4(saved) && aligned4(grad_src) &&
                  aligned4(grad_scores),
              "gnc_segment_softmax_backward_f32: a pointer is not aligned to its element size");
  const BwdArgs a = {grad_out, ld_grad, src, ld_src, scores, out, ld_out, saved, dst_of_row, num_rows, feat_dim, grad_src, ld_gsrc,
                     grad_scores};
  return launch_backward(a, (hipStream_t)stream_);
}

extern "C" int gnc_segment_softmax_weights_f32(const float* scores, const float* saved, const int32_t* dst_of_row, int64_t num_rows,
                                               float* alpha, void* stream_) {
  GNC_REQUIRE(num_rows >= 0, "gnc_segment_softmax_weights_f32: negative size");
  GNC_REQUIRE(num_rows < INT32_MAX, "gnc_segment_softmax_weights_f32: sizes exceed int32");
  if (num_rows == 0) return GNC_OK;
  GNC_REQUIRE(scores && saved && dst_of_row && alpha, "gnc_segment_softmax_weights_f32: null pointer");
  GNC_REQUIRE(aligned4(scores) && aligned4(saved) && aligned4(alpha),
              "gnc_segment_softmax_weights_f32: a pointer is not aligned to its element size");
  const int64_t blocks = gnc::capped_blocks(num_rows, gnc::kBlock, 16);
  segment_softmax_weights_kernel<<<dim3((unsigned)blocks), dim3(gnc::kBlock), 0, (hipStream_t)stream_>>>(scores, saved, dst_of_row,
                                                                                                         num_rows, alpha);
  return gnc::check_launch("segment_softmax_weights_kernel");
}
