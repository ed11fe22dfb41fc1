// K14: batch normalisation over the rows of a [rows, C] table (norm_type='BatchNorm1d', models/MLP.py:29-35), C <= 256.
//   gnc_bn_stats_f32 + gnc_bn_finalize_f32   per-column mean / biased variance of the training forward, running statistics
//   gnc_bn_apply_f32                         out = (z - mean) * invstd * gamma + beta (+ residual)
//   gnc_bn_backward_sums_f32                 partial rows [ colsum(G) | colsum(G * x_hat) ] (the layout of gnc_colsum_pair_f32,
//                                            summed by gnc_reduce_partials_f32), x_hat recomputed from z
//   gnc_bn_backward_dz_f32                   dz = gamma * invstd * (G - d beta / rows - x_hat * d gamma / rows)
//   gnc_bn_forward_small_f32 / gnc_bn_backward_small_f32   the same for rows <= gnc_bn_small_max_rows(): ONE launch each way
//   gnc_bn_fold_f32                          eval mode: the affine map of the running statistics folded into the last Linear
//
// One thread layout serves every streaming kernel here: a lane owns one group of 4 adjacent columns (one 16-B load per row),
// lanes-per-row = the power of two that covers ceil(C / 4) groups, so a wave covers 4 rows at C = 64 and 1 row at C = 256 and
// a 256-thread workgroup 256 / lanes-per-row rows per pass.  Tables whose rows are not 16-B pieces (C % 4 != 0, ld % 4 != 0,
// an unaligned base) run the same kernels with guarded scalar loads.
//
// Statistics: fp32 sum / sum-of-squares cancels catastrophically once |mean| >> std, so every thread forms the mean and the
// centred second moment M2 of 8 rows at a time from registers (two passes over the 8 values) and merges that chunk into its
// running (count, mean, M2) with Chan's formula (the mean as hi + lo); threads merge through an LDS tree, workgroups own CONTIGUOUS row ranges and
// write one partial row each, and the finalize kernel merges those in index order.  No atomics, no zero-initialised scratch:
// every partial row is fully written by the workgroup that owns it, results are bitwise equal from run to run.
#include "gnc_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kChunk = 8;        // rows a thread reduces from registers before one Chan merge
constexpr int kSmallRows = 4096; // up to here one launch per direction serves the table (a workgroup per 4 columns over all rows)
constexpr int kBlocksPerCU = 4;  // grid cap of the reducing kernels (= partial rows): 16 waves per CU, 8 loads in flight each

inline int lanes_log2(int width) {
  const int groups = (width + 3) / 4;
  int l = 0;
  while ((1 << l) < groups) ++l;
  return l;
}

// rows one workgroup consumes per chunk step; a workgroup's row range is a multiple of it
inline int64_t tile_rows(int width) { return (int64_t)(kThreads >> lanes_log2(width)) * kChunk; }

inline int64_t rows_per_partial(int64_t rows, int width) {
  const int64_t tile = tile_rows(width);
  const int64_t cap = (int64_t)gnc::num_cu() * kBlocksPerCU;
  const int64_t tiles = gnc::ceil_div(rows > 0 ? rows : 1, tile);
  return gnc::ceil_div(tiles, cap) * tile;
}

inline bool vec_ok(const void* p, int64_t ld, int width) { return width % 4 == 0 && ld % 4 == 0 && gnc::aligned16(p); }

template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* p, int valid) {
  if (VEC) return *reinterpret_cast<const f32x4*>(p);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (valid > 0) v.x = p[0];
  if (valid > 1) v.y = p[1];
  if (valid > 2) v.z = p[2];
  if (valid > 3) v.w = p[3];
  return v;
}

template <bool VEC>
__device__ __forceinline__ void store4(float* p, f32x4 v, int valid) {
  if (VEC) {
    *reinterpret_cast<f32x4*>(p) = v;
    return;
  }
  if (valid > 0) p[0] = v.x;
  if (valid > 1) p[1] = v.y;
  if (valid > 2) p[2] = v.z;
  if (valid > 3) p[3] = v.w;
}

// per-column vector of this lane's group: 4 guarded scalar loads (C floats in all, read once per thread)
__device__ __forceinline__ f32x4 load_cols(const float* p, int c0, int valid) { return load4<false>(p + c0, valid); }

// Chan et al.: (na, ma, M2a) <- merge with (nb, mb, M2b).  An empty side (count 0, mean 0, M2 0) is the identity.
// The mean is carried as hi + lo (la, lb: the part a float cannot hold at |mean| >> std): the difference of two means is then
// exact to their spread, not to ulp(mean), and the rounding of every update is kept (TwoSum) instead of lost.
template <typename T>
__device__ __forceinline__ void chan_merge(float& na, T& ma, T& la, T& m2a, float nb, T mb, T lb, T m2b) {
  const float n = na + nb;
  const float f = n > 0.f ? nb / n : 0.f;
  const T dh = mb - ma, dl = lb - la;  // kept apart: with an empty side dh is a whole mean and would swallow dl
  const T d = dh + dl;
  const T step = dh * f;
  const T hi = ma + step;
  const T bb = hi - ma;
  la += ((ma - (hi - bb)) + (step - bb)) + dl * f;
  ma = hi;
  m2a += m2b + d * d * (na * f);
  na = n;
}

// ---------------------------------------------------------------------------------------------------------------- statistics
// (count, mean hi + lo, M2) of the rows r_first, r_first + step, ... < r_end of one group of 4 columns (col = table + first column)
template <bool VEC>
__device__ __forceinline__ void accumulate_rows(const float* __restrict__ col, int64_t ld, int64_t r_first, int64_t r_end, int step,
                                                int valid, float& n, f32x4& mean, f32x4& mlo, f32x4& m2) {
  for (int64_t r0 = r_first; r0 < r_end; r0 += (int64_t)step * kChunk) {
    f32x4 v[kChunk];
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      const int64_t r = r0 + (int64_t)k * step;
      v[k] = load4<VEC>(col + (r < r_end ? r : r0) * ld, valid);  // past the range: a row of the range again, masked below
    }
    const int64_t left = (r_end - r0 + step - 1) / step;
    const int cnt = left < kChunk ? (int)left : kChunk;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < kChunk; ++k)
      if (k < cnt) s += v[k];
    const float fc = (float)cnt, inv = 1.f / fc;
    const f32x4 cm = s * inv;
    // second pass over the registers: the centred values are exact differences, their sum is what cm's rounding left over
    f32x4 q = {0.f, 0.f, 0.f, 0.f}, sd = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      const f32x4 d = v[k] - cm;
      if (k < cnt) { sd += d; q += d * d; }
    }
    const f32x4 clo = sd * inv;  // chunk mean = cm + clo; M2 about it = q - sd * clo
    chan_merge(n, mean, mlo, m2, fc, cm, clo, q - sd * clo);
  }
}

struct StatsShared {
  float n[kThreads];
  f32x4 m[kThreads], l[kThreads], q[kThreads];
};

// the `slots` row slots of a workgroup (a power of two; slot = t >> lpr_log2) hold the same columns: merge them pairwise
// through LDS (a fixed tree); afterwards slot 0's threads - and sh[...][t & (lanes - 1)] - hold the workgroup's result
__device__ __forceinline__ void tree_merge(StatsShared& sh, int t, int slot, int slots, int lpr_log2, float& n, f32x4& mean,
                                           f32x4& mlo, f32x4& m2) {
  sh.n[t] = n; sh.m[t] = mean; sh.l[t] = mlo; sh.q[t] = m2;
  __syncthreads();
  for (int s = slots >> 1; s >= 1; s >>= 1) {
    if (slot < s) {
      const int o = t + (s << lpr_log2);
      chan_merge(n, mean, mlo, m2, sh.n[o], sh.m[o], sh.l[o], sh.q[o]);
      sh.n[t] = n; sh.m[t] = mean; sh.l[t] = mlo; sh.q[t] = m2;
    }
    __syncthreads();
  }
}

// partial row b = [ count (C) | mean (C) | M2 (C) ] of the rows [b * chunk_rows, min(rows, (b + 1) * chunk_rows))
template <bool VEC>
__global__ __launch_bounds__(kThreads) void bn_stats_kernel(const float* __restrict__ z, int64_t ld, int64_t rows, int width,
                                                            int lpr_log2, int64_t chunk_rows, float* __restrict__ partial) {
  __shared__ StatsShared sh;
  const int t = (int)threadIdx.x;
  const int lpr = 1 << lpr_log2, rpb = kThreads >> lpr_log2;
  const int g = t & (lpr - 1), slot = t >> lpr_log2;
  const int c0 = 4 * g;
  const int valid = width - c0 < 0 ? 0 : (width - c0 > 4 ? 4 : width - c0);
  const int64_t r_begin = (int64_t)blockIdx.x * chunk_rows;
  const int64_t r_end = r_begin + chunk_rows < rows ? r_begin + chunk_rows : rows;
  float n = 0.f;
  f32x4 mean = {0.f, 0.f, 0.f, 0.f}, mlo = {0.f, 0.f, 0.f, 0.f}, m2 = {0.f, 0.f, 0.f, 0.f};
  if (valid > 0) accumulate_rows<VEC>(z + c0, ld, r_begin + slot, r_end, rpb, valid, n, mean, mlo, m2);
  tree_merge(sh, t, slot, rpb, lpr_log2, n, mean, mlo, m2);
  if (slot == 0 && valid > 0) {
    float* dst = partial + (int64_t)blockIdx.x * 3 * width + c0;
    const f32x4 nn = {n, n, n, n};
    store4<false>(dst, nn, valid);
    store4<false>(dst + width, mean + mlo, valid);
    store4<false>(dst + 2 * width, m2, valid);
  }
}

// 16 columns x 16 partial-lanes per workgroup: lane j merges the partial rows [j * q, (j + 1) * q) in index order, the 16
// lane results are merged pairwise, neighbours first (so the whole merge runs in index order)
__global__ __launch_bounds__(kThreads) void bn_finalize_kernel(const float* __restrict__ partial, int num_partials, int64_t rows,
                                                               int width, float eps, float momentum, float* __restrict__ mean_out,
                                                               float* __restrict__ invstd_out, float* __restrict__ running_mean,
                                                               float* __restrict__ running_var) {
  __shared__ float sh[4][kThreads];
  const int t = (int)threadIdx.x, tx = t & 15, ty = t >> 4;
  const int c = (int)blockIdx.x * 16 + tx;
  float n = 0.f, mean = 0.f, mlo = 0.f, m2 = 0.f;
  if (c < width) {
    const int q = (num_partials + 15) / 16;
    const int p1 = (ty + 1) * q < num_partials ? (ty + 1) * q : num_partials;
    for (int p = ty * q; p < p1; ++p) {
      const float* src = partial + (int64_t)p * 3 * width + c;
      chan_merge(n, mean, mlo, m2, src[0], src[width], 0.f, src[2 * width]);
    }
  }
  sh[0][t] = n; sh[1][t] = mean; sh[2][t] = mlo; sh[3][t] = m2;
  __syncthreads();
  for (int s = 1; s < 16; s <<= 1) {
    if ((ty & (2 * s - 1)) == 0) {
      const int o = t + 16 * s;
      chan_merge(n, mean, mlo, m2, sh[0][o], sh[1][o], sh[2][o], sh[3][o]);
      sh[0][t] = n; sh[1][t] = mean; sh[2][t] = mlo; sh[3][t] = m2;
    }
    __syncthreads();
  }
  mean += mlo;
  if (ty == 0 && c < width) {
    const float fn = (float)rows;
    const float var = m2 / fn;
    mean_out[c] = mean;
    invstd_out[c] = 1.f / sqrtf(var + eps);
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
    if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (var * (fn / (fn - 1.f)));
  }
}

// ------------------------------------------------------------------------------------------------------- elementwise passes
// MODE 0: out = (z - mean) * (invstd * gamma) + beta (+ res)           p0 = gamma, p1 = beta, b = residual or NULL
// MODE 1: out = gamma * invstd * (b - p0 / rows - x_hat * p1 / rows)   p0 = d beta, p1 = d gamma, b = grad_out
// `out` may be `z` itself (MODE 0): every element is read and then written by the same thread.
template <bool VEC, int MODE>
__global__ __launch_bounds__(kThreads) void bn_rows_kernel(const float* z, int64_t ldz, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ p0, const float* __restrict__ p1,
                                                           const float* b, int64_t ldb, int64_t rows, int width, int lpr_log2,
                                                           float* out, int64_t ldo) {
  constexpr int U = 4;
  const int t = (int)threadIdx.x;
  const int lpr = 1 << lpr_log2, rpb = kThreads >> lpr_log2;
  const int g = t & (lpr - 1), slot = t >> lpr_log2;
  const int c0 = 4 * g;
  const int valid = width - c0 < 0 ? 0 : (width - c0 > 4 ? 4 : width - c0);
  if (valid == 0) return;
  const f32x4 mu = load_cols(mean, c0, valid), is = load_cols(invstd, c0, valid);
  f32x4 scale, k0, k1;
  if (MODE == 0) {
    scale = is * load_cols(p0, c0, valid);
    k0 = load_cols(p1, c0, valid);
    k1 = k0;
  } else {
    const float inv_rows = 1.f / (float)rows;
    scale = is * load_cols(gamma, c0, valid);
    k0 = load_cols(p0, c0, valid) * inv_rows;
    k1 = load_cols(p1, c0, valid) * inv_rows;
  }
  const int64_t stride = (int64_t)gridDim.x * rpb;
  for (int64_t r0 = (int64_t)blockIdx.x * rpb + slot; r0 < rows; r0 += stride * U) {
    f32x4 zv[U], bv[U] = {};
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t r = r0 + k * stride;
      const int64_t rc = r < rows ? r : r0;
      zv[k] = load4<VEC>(z + rc * ldz + c0, valid);
      if (MODE == 1 || b) bv[k] = load4<VEC>(b + rc * ldb + c0, valid);
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t r = r0 + k * stride;
      if (r >= rows) break;
      f32x4 o;
      if (MODE == 0) {
        o = (zv[k] - mu) * scale + k0;
        if (b) o += bv[k];
      } else {
        const f32x4 xh = (zv[k] - mu) * is;
        o = scale * (bv[k] - k0 - xh * k1);
      }
      store4<VEC>(out + r * ldo + c0, o, valid);
    }
  }
}

// partial row b = [ colsum(G) (C) | colsum(G * x_hat) (C) ] over the workgroup's contiguous rows (gnc_colsum_pair_f32's layout)
template <bool VEC>
__global__ __launch_bounds__(kThreads) void bn_backward_sums_kernel(const float* __restrict__ G, int64_t ldg,
                                                                    const float* __restrict__ z, int64_t ldz,
                                                                    const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                    int64_t rows, int width, int lpr_log2, int64_t chunk_rows,
                                                                    float* __restrict__ partial) {
  constexpr int U = 4;
  __shared__ f32x4 sh_g[kThreads], sh_gx[kThreads];
  const int t = (int)threadIdx.x;
  const int lpr = 1 << lpr_log2, rpb = kThreads >> lpr_log2;
  const int g = t & (lpr - 1), slot = t >> lpr_log2;
  const int c0 = 4 * g;
  const int valid = width - c0 < 0 ? 0 : (width - c0 > 4 ? 4 : width - c0);
  const int64_t r_begin = (int64_t)blockIdx.x * chunk_rows;
  const int64_t r_end = r_begin + chunk_rows < rows ? r_begin + chunk_rows : rows;
  f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sgx = {0.f, 0.f, 0.f, 0.f};
  if (valid > 0) {
    const f32x4 mu = load_cols(mean, c0, valid), is = load_cols(invstd, c0, valid);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int64_t r0 = r_begin + slot; r0 < r_end; r0 += (int64_t)rpb * U) {
      f32x4 gv[U], zv[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int64_t r = r0 + (int64_t)k * rpb;
        const int64_t rc = r < r_end ? r : r0;
        gv[k] = load4<VEC>(G + rc * ldg + c0, valid);
        zv[k] = load4<VEC>(z + rc * ldz + c0, valid);
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const f32x4 gm = r0 + (int64_t)k * rpb < r_end ? gv[k] : zero;
        sg += gm;
        sgx += gm * ((zv[k] - mu) * is);
      }
    }
  }
  sh_g[t] = sg; sh_gx[t] = sgx;
  __syncthreads();
  for (int s = rpb >> 1; s >= 1; s >>= 1) {
    if (slot < s) {
      const int o = t + (s << lpr_log2);
      sg += sh_g[o]; sgx += sh_gx[o];
      sh_g[t] = sg; sh_gx[t] = sgx;
    }
    __syncthreads();
  }
  if (slot == 0 && valid > 0) {
    float* dst = partial + (int64_t)blockIdx.x * 2 * width + c0;
    store4<false>(dst, sg, valid);
    store4<false>(dst + width, sgx, valid);
  }
}

// ------------------------------------------------------------------------------------------- small tables: one launch each way
// rows <= kSmallRows (the per-sample regime: ~2000 rows): three launches and two scratch buffers cost more than the work.  A
// workgroup owns ONE group of 4 columns over ALL rows - statistics (the same chunked accumulation, 256 row slots), then the
// normalisation of those columns from the rows it has just read (L2-resident) - so nothing is exchanged between workgroups.
// `out` may be `z`: a workgroup reads all of its columns before it writes any, and no other workgroup touches them.
__device__ __forceinline__ f32x4 inv_sqrt4(f32x4 v) {
  const f32x4 r = {1.f / sqrtf(v.x), 1.f / sqrtf(v.y), 1.f / sqrtf(v.z), 1.f / sqrtf(v.w)};
  return r;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void bn_small_forward_kernel(const float* z, int64_t ldz, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, const float* res, int64_t ldr,
                                                                    int rows, int width, float eps, float momentum, float* out,
                                                                    int64_t ldo, float* __restrict__ mean_out,
                                                                    float* __restrict__ invstd_out, float* __restrict__ running_mean,
                                                                    float* __restrict__ running_var) {
  __shared__ StatsShared sh;
  const int t = (int)threadIdx.x;
  const int c0 = 4 * (int)blockIdx.x;
  const int valid = width - c0 > 4 ? 4 : width - c0;
  float n = 0.f;
  f32x4 mean = {0.f, 0.f, 0.f, 0.f}, mlo = {0.f, 0.f, 0.f, 0.f}, m2 = {0.f, 0.f, 0.f, 0.f};
  accumulate_rows<VEC>(z + c0, ldz, t, rows, kThreads, valid, n, mean, mlo, m2);
  tree_merge(sh, t, t, kThreads, 0, n, mean, mlo, m2);
  const float fn = (float)rows;
  const f32x4 mu = sh.m[0] + sh.l[0];
  const f32x4 var = sh.q[0] * (1.f / fn);
  const f32x4 is = inv_sqrt4(var + eps);
  if (t == 0) {
    store4<false>(mean_out + c0, mu, valid);
    store4<false>(invstd_out + c0, is, valid);
    if (running_mean) store4<false>(running_mean + c0, (1.f - momentum) * load_cols(running_mean, c0, valid) + momentum * mu, valid);
    if (running_var)
      store4<false>(running_var + c0, (1.f - momentum) * load_cols(running_var, c0, valid) + momentum * (var * (fn / (fn - 1.f))), valid);
  }
  const f32x4 scale = is * load_cols(gamma, c0, valid), shift = load_cols(beta, c0, valid);
  for (int r0 = t; r0 < rows; r0 += kThreads * 4) {
    f32x4 zv[4], rv[4] = {};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = r0 + k * kThreads;
      const int64_t rc = r < rows ? r : r0;
      zv[k] = load4<VEC>(z + rc * ldz + c0, valid);
      if (res) rv[k] = load4<VEC>(res + rc * ldr + c0, valid);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = r0 + k * kThreads;
      if (r >= rows) break;
      f32x4 o = (zv[k] - mu) * scale + shift;
      if (res) o += rv[k];
      store4<VEC>(out + (int64_t)r * ldo + c0, o, valid);
    }
  }
}

// the backward of a small table in one launch: the workgroup's column sums (a fixed tree), d beta / d gamma, then dz (NULL: skipped)
template <bool VEC>
__global__ __launch_bounds__(kThreads) void bn_small_backward_kernel(const float* __restrict__ G, int64_t ldg,
                                                                     const float* __restrict__ z, int64_t ldz,
                                                                     const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                     const float* __restrict__ gamma, int rows, int width,
                                                                     float* __restrict__ dz, int64_t ldd, float* __restrict__ dbeta,
                                                                     float* __restrict__ dgamma) {
  __shared__ f32x4 sh_g[kThreads], sh_gx[kThreads];
  const int t = (int)threadIdx.x;
  const int c0 = 4 * (int)blockIdx.x;
  const int valid = width - c0 > 4 ? 4 : width - c0;
  const f32x4 mu = load_cols(mean, c0, valid), is = load_cols(invstd, c0, valid);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 sg = zero, sgx = zero;
  for (int r0 = t; r0 < rows; r0 += kThreads * 4) {
    f32x4 gv[4], zv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = r0 + k * kThreads;
      const int64_t rc = r < rows ? r : r0;
      gv[k] = load4<VEC>(G + rc * ldg + c0, valid);
      zv[k] = load4<VEC>(z + rc * ldz + c0, valid);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const f32x4 gm = r0 + k * kThreads < rows ? gv[k] : zero;
      sg += gm;
      sgx += gm * ((zv[k] - mu) * is);
    }
  }
  sh_g[t] = sg; sh_gx[t] = sgx;
  __syncthreads();
  for (int s = kThreads >> 1; s >= 1; s >>= 1) {
    if (t < s) {
      sg += sh_g[t + s]; sgx += sh_gx[t + s];
      sh_g[t] = sg; sh_gx[t] = sgx;
    }
    __syncthreads();
  }
  const f32x4 db = sh_g[0], dg = sh_gx[0];
  if (t == 0) {
    store4<false>(dbeta + c0, db, valid);
    store4<false>(dgamma + c0, dg, valid);
  }
  if (!dz) return;
  const float inv_rows = 1.f / (float)rows;
  const f32x4 scale = is * load_cols(gamma, c0, valid), k0 = db * inv_rows, k1 = dg * inv_rows;
  for (int r0 = t; r0 < rows; r0 += kThreads * 4) {
    f32x4 gv[4], zv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = r0 + k * kThreads;
      const int64_t rc = r < rows ? r : r0;
      gv[k] = load4<VEC>(G + rc * ldg + c0, valid);
      zv[k] = load4<VEC>(z + rc * ldz + c0, valid);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = r0 + k * kThreads;
      if (r >= rows) break;
      store4<VEC>(dz + (int64_t)r * ldd + c0, scale * (gv[k] - k0 - ((zv[k] - mu) * is) * k1), valid);
    }
  }
}

// W'[m, k] = s[m] W[m, k], b'[m] = s[m] b[m] + beta[m] - running_mean[m] s[m], s = gamma / sqrt(running_var + eps)
__global__ __launch_bounds__(kThreads) void bn_fold_kernel(const float* __restrict__ w, int64_t ldw, const float* __restrict__ b,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ rmean, const float* __restrict__ rvar, float eps,
                                                           int M, int K, float* __restrict__ w_out, int64_t ldo,
                                                           float* __restrict__ b_out) {
  const int total = M * K + M;
  for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < total; i += (int)(gridDim.x * blockDim.x)) {
    const int m = i < M * K ? i / K : i - M * K;
    const float s = gamma[m] / sqrtf(rvar[m] + eps);
    if (i < M * K) {
      const int k = i - m * K;
      w_out[(int64_t)m * ldo + k] = s * w[(int64_t)m * ldw + k];
    } else {
      b_out[m] = s * (b ? b[m] : 0.f) + (beta[m] - rmean[m] * s);
    }
  }
}

int rows_grid(int64_t rows, int width) {
  const int64_t rpb = kThreads >> lanes_log2(width);
  const int64_t want = gnc::ceil_div(rows, rpb * 4);
  const int64_t cap = (int64_t)gnc::num_cu() * 8;
  return (int)(want < cap ? (want > 0 ? want : 1) : cap);
}

}  // namespace

extern "C" int gnc_bn_partials(int64_t rows, int32_t width) {
  if (rows < 1 || width < 1 || width > 256) return 0;
  return (int)gnc::ceil_div(rows, rows_per_partial(rows, width));
}

extern "C" int gnc_bn_stats_f32(const float* z, int64_t ld_z, int64_t rows, int32_t width, float* partial, int32_t num_partials,
                                void* stream) {
  GNC_REQUIRE(rows >= 1 && width >= 1 && width <= 256 && ld_z >= width, "gnc_bn_stats_f32: need rows >= 1, 1 <= width <= 256 <= ld");
  GNC_REQUIRE(z && partial, "gnc_bn_stats_f32: null pointer");
  const int parts = gnc_bn_partials(rows, width);
  GNC_REQUIRE(num_partials >= parts, "gnc_bn_stats_f32: partial buffer smaller than gnc_bn_partials()");
  const int64_t chunk = rows_per_partial(rows, width);
  const int l2 = lanes_log2(width);
  if (vec_ok(z, ld_z, width))
    bn_stats_kernel<true><<<dim3((unsigned)parts), dim3(kThreads), 0, (hipStream_t)stream>>>(z, ld_z, rows, width, l2, chunk, partial);
  else
    bn_stats_kernel<false><<<dim3((unsigned)parts), dim3(kThreads), 0, (hipStream_t)stream>>>(z, ld_z, rows, width, l2, chunk, partial);
  return gnc::check_launch("bn_stats_kernel");
}

extern "C" int gnc_bn_finalize_f32(const float* partial, int32_t num_partials, int64_t rows, int32_t width, float eps, float momentum,
                                   float* mean, float* invstd, float* running_mean, float* running_var, void* stream) {
  GNC_REQUIRE(rows >= 1 && width >= 1 && width <= 256 && num_partials >= 1, "gnc_bn_finalize_f32: bad sizes");
  GNC_REQUIRE(num_partials == gnc_bn_partials(rows, width), "gnc_bn_finalize_f32: num_partials is not gnc_bn_partials(rows, width)");
  GNC_REQUIRE(partial && mean && invstd, "gnc_bn_finalize_f32: null pointer");
  GNC_REQUIRE(rows >= 2 || !running_var, "gnc_bn_finalize_f32: the unbiased running variance needs rows >= 2");
  bn_finalize_kernel<<<dim3((unsigned)((width + 15) / 16)), dim3(kThreads), 0, (hipStream_t)stream>>>(
      partial, num_partials, rows, width, eps, momentum, mean, invstd, running_mean, running_var);
  return gnc::check_launch("bn_finalize_kernel");
}

extern "C" int gnc_bn_apply_f32(const float* z, int64_t ld_z, const float* mean, const float* invstd, const float* gamma,
                                const float* beta, const float* residual, int64_t ld_res, int64_t rows, int32_t width, float* out,
                                int64_t ld_out, void* stream) {
  GNC_REQUIRE(rows >= 0 && width >= 1 && width <= 256 && ld_z >= width && ld_out >= width && (!residual || ld_res >= width),
              "gnc_bn_apply_f32: bad sizes");
  if (rows == 0) return GNC_OK;
  GNC_REQUIRE(z && mean && invstd && gamma && beta && out, "gnc_bn_apply_f32: null pointer");
  const int l2 = lanes_log2(width);
  const bool vec = vec_ok(z, ld_z, width) && vec_ok(out, ld_out, width) && (!residual || vec_ok(residual, ld_res, width));
  const dim3 grid((unsigned)rows_grid(rows, width)), block(kThreads);
  if (vec)
    bn_rows_kernel<true, 0><<<grid, block, 0, (hipStream_t)stream>>>(z, ld_z, mean, invstd, nullptr, gamma, beta, residual, ld_res, rows,
                                                                      width, l2, out, ld_out);
  else
    bn_rows_kernel<false, 0><<<grid, block, 0, (hipStream_t)stream>>>(z, ld_z, mean, invstd, nullptr, gamma, beta, residual, ld_res, rows,
                                                                       width, l2, out, ld_out);
  return gnc::check_launch("bn_rows_kernel");
}

extern "C" int gnc_bn_backward_sums_f32(const float* grad_out, int64_t ld_grad, const float* z, int64_t ld_z, const float* mean,
                                        const float* invstd, int64_t rows, int32_t width, float* partial, int32_t num_partials,
                                        void* stream) {
  GNC_REQUIRE(rows >= 1 && width >= 1 && width <= 256 && ld_grad >= width && ld_z >= width, "gnc_bn_backward_sums_f32: bad sizes");
  GNC_REQUIRE(grad_out && z && mean && invstd && partial, "gnc_bn_backward_sums_f32: null pointer");
  const int parts = gnc_bn_partials(rows, width);
  GNC_REQUIRE(num_partials >= parts, "gnc_bn_backward_sums_f32: partial buffer smaller than gnc_bn_partials()");
  const int64_t chunk = rows_per_partial(rows, width);
  const int l2 = lanes_log2(width);
  if (vec_ok(grad_out, ld_grad, width) && vec_ok(z, ld_z, width))
    bn_backward_sums_kernel<true><<<dim3((unsigned)parts), dim3(kThreads), 0, (hipStream_t)stream>>>(grad_out, ld_grad, z, ld_z, mean,
                                                                                                    invstd, rows, width, l2, chunk, partial);
  else
    bn_backward_sums_kernel<false><<<dim3((unsigned)parts), dim3(kThreads), 0, (hipStream_t)stream>>>(grad_out, ld_grad, z, ld_z, mean,
                                                                                                     invstd, rows, width, l2, chunk, partial);
  return gnc::check_launch("bn_backward_sums_kernel");
}

extern "C" int gnc_bn_backward_dz_f32(const float* grad_out, int64_t ld_grad, const float* z, int64_t ld_z, const float* mean,
                                      const float* invstd, const float* gamma, const float* dbeta, const float* dgamma, int64_t rows,
                                      int32_t width, float* grad_z, int64_t ld_gz, void* stream) {
  GNC_REQUIRE(rows >= 0 && width >= 1 && width <= 256 && ld_grad >= width && ld_z >= width && ld_gz >= width,
              "gnc_bn_backward_dz_f32: bad sizes");
  if (rows == 0) return GNC_OK;
  GNC_REQUIRE(grad_out && z && mean && invstd && gamma && dbeta && dgamma && grad_z, "gnc_bn_backward_dz_f32: null pointer");
  const int l2 = lanes_log2(width);
  const bool vec = vec_ok(grad_out, ld_grad, width) && vec_ok(z, ld_z, width) && vec_ok(grad_z, ld_gz, width);
  const dim3 grid((unsigned)rows_grid(rows, width)), block(kThreads);
  if (vec)
    bn_rows_kernel<true, 1><<<grid, block, 0, (hipStream_t)stream>>>(z, ld_z, mean, invstd, gamma, dbeta, dgamma, grad_out, ld_grad, rows,
                                                                      width, l2, grad_z, ld_gz);
  else
    bn_rows_kernel<false, 1><<<grid, block, 0, (hipStream_t)stream>>>(z, ld_z, mean, invstd, gamma, dbeta, dgamma, grad_out, ld_grad, rows,
                                                                       width, l2, grad_z, ld_gz);
  return gnc::check_launch("bn_rows_kernel");
}

extern "C" int gnc_bn_small_max_rows(void) { return kSmallRows; }

extern "C" int gnc_bn_forward_small_f32(const float* z, int64_t ld_z, const float* gamma, const float* beta, const float* residual,
                                        int64_t ld_res, int64_t rows, int32_t width, float eps, float momentum, float* out,
                                        int64_t ld_out, float* mean, float* invstd, float* running_mean, float* running_var,
                                        void* stream) {
  GNC_REQUIRE(rows >= 1 && rows <= kSmallRows && width >= 1 && width <= 256 && ld_z >= width && ld_out >= width &&
                  (!residual || ld_res >= width),
              "gnc_bn_forward_small_f32: need 1 <= rows <= gnc_bn_small_max_rows(), 1 <= width <= 256 <= ld");
  GNC_REQUIRE(z && gamma && beta && out && mean && invstd, "gnc_bn_forward_small_f32: null pointer");
  GNC_REQUIRE(rows >= 2 || !running_var, "gnc_bn_forward_small_f32: the unbiased running variance needs rows >= 2");
  const bool vec = vec_ok(z, ld_z, width) && vec_ok(out, ld_out, width) && (!residual || vec_ok(residual, ld_res, width));
  const dim3 grid((unsigned)((width + 3) / 4)), block(kThreads);
  if (vec)
    bn_small_forward_kernel<true><<<grid, block, 0, (hipStream_t)stream>>>(z, ld_z, gamma, beta, residual, ld_res, (int)rows, width, eps,
                                                                            momentum, out, ld_out, mean, invstd, running_mean, running_var);
  else
    bn_small_forward_kernel<false><<<grid, block, 0, (hipStream_t)stream>>>(z, ld_z, gamma, beta, residual, ld_res, (int)rows, width, eps,
                                                                             momentum, out, ld_out, mean, invstd, running_mean, running_var);
  return gnc::check_launch("bn_small_forward_kernel");
}

extern "C" int gnc_bn_backward_small_f32(const float* grad_out, int64_t ld_grad, const float* z, int64_t ld_z, const float* mean,
                                         const float* invstd, const float* gamma, int64_t rows, int32_t width, float* grad_z,
                                         int64_t ld_gz, float* dbeta, float* dgamma, void* stream) {
  GNC_REQUIRE(rows >= 1 && rows <= kSmallRows && width >= 1 && width <= 256 && ld_grad >= width && ld_z >= width &&
                  (!grad_z || ld_gz >= width),
              "gnc_bn_backward_small_f32: need 1 <= rows <= gnc_bn_small_max_rows(), 1 <= width <= 256 <= ld");
  GNC_REQUIRE(grad_out && z && mean && invstd && gamma && dbeta && dgamma, "gnc_bn_backward_small_f32: null pointer");
  const bool vec = vec_ok(grad_out, ld_grad, width) && vec_ok(z, ld_z, width) && (!grad_z || vec_ok(grad_z, ld_gz, width));
  const dim3 grid((unsigned)((width + 3) / 4)), block(kThreads);
  if (vec)
    bn_small_backward_kernel<true><<<grid, block, 0, (hipStream_t)stream>>>(grad_out, ld_grad, z, ld_z, mean, invstd, gamma, (int)rows,
                                                                             width, grad_z, ld_gz, dbeta, dgamma);
  else
    bn_small_backward_kernel<false><<<grid, block, 0, (hipStream_t)stream>>>(grad_out, ld_grad, z, ld_z, mean, invstd, gamma, (int)rows,
                                                                              width, grad_z, ld_gz, dbeta, dgamma);
  return gnc::check_launch("bn_small_backward_kernel");
}

extern "C" int gnc_bn_fold_f32(const float* weight, int64_t ld_w, const float* bias, const float* gamma, const float* beta,
                               const float* running_mean, const float* running_var, float eps, int32_t out_dim, int32_t in_dim,
                               float* weight_out, int64_t ld_wo, float* bias_out, void* stream) {
  GNC_REQUIRE(out_dim >= 1 && out_dim <= 256 && in_dim >= 1 && in_dim <= 65536 && ld_w >= in_dim && ld_wo >= in_dim,
              "gnc_bn_fold_f32: bad sizes");
  GNC_REQUIRE(weight && gamma && beta && running_mean && running_var && weight_out && bias_out, "gnc_bn_fold_f32: null pointer");
  const int total = out_dim * in_dim + out_dim;
  const int blocks = (total + kThreads - 1) / kThreads;
  bn_fold_kernel<<<dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(kThreads), 0, (hipStream_t)stream>>>(
      weight, ld_w, bias, gamma, beta, running_mean, running_var, eps, out_dim, in_dim, weight_out, ld_wo, bias_out);
  return gnc::check_launch("bn_fold_kernel");
}
