// The destination-sorted CSR segment skeleton that K1 (csrc/scatter_gather.hip, sum), K18 (csrc/segment_reduce.hip, mean / max)
// and K21 (csrc/segment_softmax.hip, attention) share, the one-pass-over-the-rows skeleton of their backwards and of K2, and the
// host helpers of their launchers.  Lane mapping, regimes and fold order are defined HERE, once; an operation's file holds its
// arithmetic (what a fold is, what is divided by what) and nothing of the walk.
//
// Lane mapping (D = feature width): LPR = pow2_lanes_for(D) lanes own one destination row, 16 B (one float4 column slice, columns
// [col, col + 4)) per lane; a lane whose slice lies beyond D is idle.  No atomics: every output row is written exactly once, by
// the lanes that folded it.
//
// Fold order (fixed; a function of the destination's own rows alone): a destination's rows [rowptr[v], rowptr[v + 1]) enter the
// operation's fold one at a time in ascending sorted position k (= original edge order, the CSR sort is stable), starting from
// the operation's identity - walk_rows.  Four rows are REQUESTED before the first is folded; that overlaps the loads and changes
// nothing of the order.  Row k is row perm[k] of `src`, or row k itself without a permutation (rows already sorted).  All three
// regimes run this walk per (destination, column), so they give the same bits:
//   * chunk (N > 64 x CUs) - for_chunk_destinations: a wave owns chunks of 64 consecutive destinations; its lanes fetch the
//     chunk's row pointers with one coalesced load and hand them to the lane groups by cross-lane reads; the 64 / LPR groups of
//     the wave take the chunk's destinations in 64 / (64 / LPR) rounds.  Rows are streamed (nontemporal loads);
//   * small (N <= 64 x CUs) - for_small_destinations: every lane group takes ONE destination, so a launch is one chain of
//     row pointers -> ids -> rows per group instead of up to 64 dependent rounds on a mostly idle chip;
//   * scalar (any D, stride or alignment) - for_scalar_destinations: one wave per destination, lane l takes columns l, l + 64, ...
//     and walks the rows once per column (walk_rows_scalar).
// forward_plan gives the regime and the grid of the two vector regimes from (N, D) alone.
//
// Row passes (K2 and K18's backward) - for_rows_two_in_flight: LPR lanes per row, two rows loaded per lane before the first is
// finished, then the tail row.  A caller whose idle lanes may leave returns before it calls.  K21's backward
// (segment_softmax_backward_vec4) has the same shape but keeps its loop written out: it keeps its idle lanes, because its xor
// tree reads them, and through this helper the compiler advanced its three [E] pointers with scalar add pairs inside the loop
// (five instructions more than the hand-written loop, 0.9 % slower at c3 size); it uses row_pass_col and the vector helpers.
//
// Left in their files: the fused aggregation epilogue (mlp_resident.hip) and agg_fixup_kernel walk row RANGES of a tile, not a
// destination's segment through this mapping, and keep their own loops.
#pragma once
#include <type_traits>

#include "gnc_common.h"

namespace gnc_csr {

using gnc::kWave;

struct alignas(16) f4 { float x, y, z, w; };
struct alignas(16) i4 { int32_t x, y, z, w; };

__device__ __forceinline__ f4 ld4(const float* p) { return *reinterpret_cast<const f4*>(p); }
// Streamed-once rows (the messages of the chunk regime): nontemporal 16-B load, so the 2.5 GB stream does not push the
// row pointers / output lines out of L2 and MALL.  Measured on K1 at c3 size: 0.592 -> 0.529 ms per launch.
__device__ __forceinline__ f4 ld4_stream(const float* p) {
  typedef float v4 __attribute__((ext_vector_type(4)));
  const v4 v = __builtin_nontemporal_load(reinterpret_cast<const v4*>(p));
  return f4{v.x, v.y, v.z, v.w};
}
template <bool STREAM>
__device__ __forceinline__ f4 ld4_row(const float* p) { return STREAM ? ld4_stream(p) : ld4(p); }
__device__ __forceinline__ void st4(float* p, f4 v) { *reinterpret_cast<f4*>(p) = v; }
__device__ __forceinline__ void st4i(int32_t* p, i4 v) { *reinterpret_cast<i4*>(p) = v; }

constexpr int kChunk = 64;  // destinations per wave iteration of the chunk regime

// what an operation without a per-row / per-destination side value hands to walk_rows / for_scalar_destinations
struct Nothing {};
struct no_side {
  template <class... A>
  __device__ __forceinline__ Nothing operator()(A...) const { return Nothing{}; }
};

// ---------------------------------------------------------------------------------------
// the row walk
// ---------------------------------------------------------------------------------------
// Rows [start, end) of one destination, columns [col, col + 4): fold(row, side(row), slice) in ascending k.  side(row) is
// evaluated where the row's load is issued (K21: the row's score), so what it fetches travels with the row, not behind it.
template <bool HAS_PERM, bool STREAM, class Side, class Fold>
__device__ __forceinline__ void walk_rows(const float* __restrict__ src, int64_t ld_src, const int32_t* __restrict__ perm,
                                          int32_t start, int32_t end, int col, Side side, Fold fold) {
  int32_t k = start;
  for (; k + 4 <= end; k += 4) {
    int32_t i0 = k, i1 = k + 1, i2 = k + 2, i3 = k + 3;
    if (HAS_PERM) { i0 = perm[k]; i1 = perm[k + 1]; i2 = perm[k + 2]; i3 = perm[k + 3]; }
    const auto s0 = side(i0), s1 = side(i1), s2 = side(i2), s3 = side(i3);
    const f4 r0 = ld4_row<STREAM>(src + (int64_t)i0 * ld_src + col);
    const f4 r1 = ld4_row<STREAM>(src + (int64_t)i1 * ld_src + col);
    const f4 r2 = ld4_row<STREAM>(src + (int64_t)i2 * ld_src + col);
    const f4 r3 = ld4_row<STREAM>(src + (int64_t)i3 * ld_src + col);
    fold(i0, s0, r0); fold(i1, s1, r1); fold(i2, s2, r2); fold(i3, s3, r3);  // ascending k: reference edge order
  }
  for (; k < end; ++k) {
    const int32_t i0 = HAS_PERM ? perm[k] : k;
    const auto s0 = side(i0);
    fold(i0, s0, ld4_row<STREAM>(src + (int64_t)i0 * ld_src + col));
  }
}

// the same walk for ONE column c: fold(row, value) in ascending k
template <bool HAS_PERM, class Fold>
__device__ __forceinline__ void walk_rows_scalar(const float* __restrict__ src, int64_t ld_src, const int32_t* __restrict__ perm,
                                                 int32_t start, int32_t end, int c, Fold fold) {
  for (int32_t k = start; k < end; ++k) {
    const int32_t i = HAS_PERM ? perm[k] : k;
    fold(i, src[(int64_t)i * ld_src + c]);
  }
}

// ---------------------------------------------------------------------------------------
// who takes which destination: body(v, start, end, col) for every (destination, live column slice)
// ---------------------------------------------------------------------------------------
template <int LPR, class Body>
__device__ __forceinline__ void for_chunk_destinations(const int32_t* __restrict__ rowptr, int32_t num_nodes, int32_t feat_dim,
                                                       Body body) {
  constexpr int GPW = kWave / LPR;      // lane groups (destinations) per wave
  constexpr int ROUNDS = kChunk / GPW;  // rounds to cover the 64-destination chunk
  const int lane = threadIdx.x & (kWave - 1);
  const int grp = lane / LPR;
  const int col = (lane % LPR) * 4;
  const bool col_ok = col < feat_dim;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t num_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int64_t num_chunks = ((int64_t)num_nodes + kChunk - 1) / kChunk;

  for (int64_t chunk = wave; chunk < num_chunks; chunk += num_waves) {
    const int64_t base = chunk * kChunk;
    // lane l holds rowptr[base + l] (clamped), lane 63's upper bound is fetched separately
    const int64_t vl = base + lane;
    const int32_t rp = rowptr[vl < num_nodes ? vl : num_nodes];
    const int64_t vlast = base + kChunk;
    const int32_t rp_last = rowptr[vlast < num_nodes ? vlast : num_nodes];

#pragma unroll 1
    for (int r = 0; r < ROUNDS; ++r) {
      const int slot = r * GPW + grp;  // destination inside the chunk
      const int64_t v = base + slot;
      const int32_t start = __shfl(rp, slot, kWave);
      const int32_t hi = __shfl(rp, (slot + 1) & (kWave - 1), kWave);
      const int32_t end = (slot + 1 < kWave) ? hi : rp_last;
      if (base + r * GPW >= num_nodes) break;  // wave-uniform: nothing left in this chunk
      if ((v < num_nodes) & col_ok) body(v, start, end, col);
    }
  }
}

template <int LPR, class Body>
__device__ __forceinline__ void for_small_destinations(const int32_t* __restrict__ rowptr, int32_t num_nodes, int32_t feat_dim,
                                                       Body body) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t v = tid / LPR;
  const int col = (int)(tid % LPR) * 4;
  if (v >= num_nodes || col >= feat_dim) return;
  body(v, rowptr[v], rowptr[v + 1], col);
}

// head(v, start, end) once per destination (K21: the score maximum), then column(v, start, end, c, head's value) per column
template <class Head, class Column>
__device__ __forceinline__ void for_scalar_destinations(const int32_t* __restrict__ rowptr, int32_t num_nodes, int32_t feat_dim,
                                                        Head head, Column column) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t num_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t v = wave; v < num_nodes; v += num_waves) {
    const int32_t start = rowptr[v], end = rowptr[v + 1];
    const auto h = head(v, start, end);
    for (int c = lane; c < feat_dim; c += kWave) column(v, start, end, c, h);
  }
}

// ---------------------------------------------------------------------------------------
// one pass over num_rows rows, LPR lanes per row: finish(r, load(r)), two rows in flight per lane
// ---------------------------------------------------------------------------------------
template <int LPR>
__device__ __forceinline__ int row_pass_col() { return (threadIdx.x % LPR) * 4; }  // the lane's column slice in a row pass

template <int LPR, class Load, class Finish>
__device__ __forceinline__ void for_rows_two_in_flight(int64_t num_rows, Load load, Finish finish) {
  constexpr int RPB = gnc::kBlock / LPR;  // rows per block pass
  int64_t r = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const int64_t stride = (int64_t)gridDim.x * RPB;
  for (; r + stride < num_rows; r += 2 * stride) {
    const auto w0 = load(r);
    const auto w1 = load(r + stride);
    finish(r, w0);
    finish(r + stride, w1);
  }
  if (r < num_rows) finish(r, load(r));
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
inline int pow2_lanes_for(int feat_dim) {  // smallest power-of-two lane count whose float4 slices cover a row
  int lanes = 1;
  while (lanes * 4 < feat_dim) lanes *= 2;
  return lanes;
}

inline bool vec4_ok(const void* p, int64_t ld, int feat_dim) {
  return feat_dim % 4 == 0 && feat_dim <= 256 && ld % 4 == 0 && gnc::aligned16(p);
}

// Regime and grid of a vector forward launch over n destinations of width d (vec4_ok).  The three-argument form exists for
// K1's A/B switch GNC_NO_SMALL_K1, which forces the chunk regime from K1's launcher; nothing else names a regime itself.
struct ForwardPlan {
  bool small;
  int lpr;
  dim3 grid;
};

inline ForwardPlan forward_plan(int32_t n, int32_t d, bool small) {
  const int lpr = pow2_lanes_for(d);
  const int64_t blocks = small ? gnc::ceil_div((int64_t)n * lpr, (int64_t)gnc::kBlock)
                               : gnc::capped_blocks(gnc::ceil_div(n, kChunk), gnc::kBlock / kWave, 16);
  return ForwardPlan{small, lpr, dim3((unsigned)blocks)};
}
// THE regime rule: a graph of at most 64 destinations per compute unit gets one lane group per destination
inline ForwardPlan forward_plan(int32_t n, int32_t d) { return forward_plan(n, d, n <= 64 * gnc::num_cu()); }

inline dim3 scalar_grid(int64_t n) { return dim3((unsigned)gnc::capped_blocks(n, gnc::kBlock / kWave, 16)); }
inline dim3 row_pass_grid(int64_t num_rows, int lpr) {
  return dim3((unsigned)gnc::capped_blocks(num_rows, 2 * (gnc::kBlock / lpr), 16));
}

// f(std::integral_constant<int, LPR>) for the lane count of a row; GNC_OK, or the error of a count no kernel is built for
template <class F>
int dispatch_lanes(int lpr, F f) {
  switch (lpr) {
    case 1: f(std::integral_constant<int, 1>{}); return GNC_OK;
    case 2: f(std::integral_constant<int, 2>{}); return GNC_OK;
    case 4: f(std::integral_constant<int, 4>{}); return GNC_OK;
    case 8: f(std::integral_constant<int, 8>{}); return GNC_OK;
    case 16: f(std::integral_constant<int, 16>{}); return GNC_OK;
    case 32: f(std::integral_constant<int, 32>{}); return GNC_OK;
    case 64: f(std::integral_constant<int, 64>{}); return GNC_OK;
    default:
      gnc::set_error("internal lane mapping error: no kernel for %d lanes per row", lpr);
      return GNC_ERR_UNSUPPORTED;
  }
}

}  // namespace gnc_csr
