// Read-out classifier of G graphs (models/GNN.py:312-325 over a block-diagonal batch): logits [G, C] = fc3(relu(fc2(relu(fc1(feats))))),
// where feature k * out_dim + j of graph g is y[start_g + k, j] for k < min(size_g, num_nodes) and 0 otherwise - the gather rule of
// CombinedModel.forward_batched / ragged_readout_rows, applied where fc1's operand is loaded: no [G, F] feature matrix is ever stored.
// Since y is row-major, the features of graph g are the contiguous run y_flat[start_g * out_dim ...] cut at lim_g = valid rows * out_dim.
//
// Forward, two launches.  rb_fc1_kernel: a workgroup owns 16 graphs x all 128 fc1 outputs x one slice of F; W1 and the feature tile go
// through LDS in 32-wide steps, the products run on v_mfma_f32_16x16x4_f32 (wave w owns outputs [32 w, 32 w + 32)), and the workgroup
// writes its [16, 128] partial into the caller's workspace.  rb_tail_kernel: sums the slices in ascending order, adds b1, ReLU (h1 kept),
// then fc2 and fc3 from LDS (h2 kept).  The split of F comes from decide(): G in the thousands -> one slice, the graph tiles are the
// parallelism; a handful of graphs at F = 16384 -> up to 128 slices, so that fc1's 8 MB weight stream is spread over the device.
//
// Backward.  rb_upper_kernel: dz2, dz1 per graph (dz1 stored) and, per chunk of 32 graphs, partial dW2 / db2 / dW3 / db3 / db1.
// rb_dw1_kernel: dW1 [128, F] = dz1^T feats on MFMA, a workgroup owns 128 x 64 of it over one range of graphs.  rb_dy_kernel:
// dy = dz1 W1 on MFMA, a [128, 64] tile of W1 resident in LDS while the workgroup walks its graph tiles; in graph_ptr mode dy is
// cleared by a kernel first (rows behind num_nodes, rows outside every graph).  Partials over graph chunks / ranges are summed by
// rb_reduce_kernel in ascending order.  No atomics, no ticket, no memset: the workspace belongs to the call, every sum has a fixed order.
#include <stdlib.h>

#include "gnc_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }  // nn.ReLU keeps a NaN (fmaxf would not)
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int BT = 256;     // threads per workgroup (4 waves)
constexpr int BH1 = 128;    // fc1 width the kernels are written for
constexpr int BMAXH2 = 32;  // fc2 width, at most
constexpr int BMAXC = 64;   // classes, at most
constexpr int KT = 32;      // fc1: k step staged in LDS
constexpr int KP = 36;      // ... and its row pitch: 16-B aligned rows, and (36 r + k) mod 64 is distinct over 16 rows x 4 k
constexpr int FT = 64;      // backward: F tile of a workgroup
constexpr int FP = 80;      // pitch of a [k][64] operand tile (80 = 16 mod 64: 4 k x 16 columns hit 64 banks)
constexpr int DP = 144;     // pitch of dz1 rows read as A^T (k = graph): 144 = 16 mod 64
constexpr int AP = 132;     // pitch of dz1 rows read as A (k = fc1 unit): 132 = 4 mod 64
constexpr int GC = 32;      // graphs per chunk of the small-gradient partials
constexpr int MIN_SLICE = 64, MAX_SLICES = 128, WG_TARGET = 512;

struct Plan {
  bool ok;
  int64_t slices, slice_len, tail_rows, small_parts, dw1_parts, dw1_range, dy_groups, dy_tiles, fwd_ws, bwd_ws, small_len;
};

// The ONE decision about a shape: the launchers and gnc_readout_batched_supported both read it.
Plan decide(int64_t G, int64_t F, int32_t H1, int32_t H2, int32_t C) {
  Plan p = {};
  if (G < 1 || G > (1ll << 22) || F < 1 || F > (1ll << 26) || H1 != BH1 || H2 < 1 || H2 > BMAXH2 || C < 1 || C > BMAXC) return p;
  p.ok = true;
  const int64_t tiles = gnc::ceil_div(G, 16);
  int64_t want = WG_TARGET / tiles;  // slices that bring the grid to about two workgroups per CU
  want = want < 1 ? 1 : (want > MAX_SLICES ? MAX_SLICES : want);
  int64_t len = gnc::ceil_div(gnc::ceil_div(F, want), KT) * KT;
  p.slice_len = len < MIN_SLICE ? MIN_SLICE : len;
  p.slices = gnc::ceil_div(F, p.slice_len);
  p.tail_rows = G >= 256 ? 16 : 1;
  p.small_parts = gnc::ceil_div(G, GC);
  p.small_len = (int64_t)H2 * BH1 + H2 + (int64_t)C * H2 + C + BH1;
  const int64_t ftiles = gnc::ceil_div(F, FT);
  int64_t parts = gnc::ceil_div(WG_TARGET / 2, ftiles);
  parts = parts > tiles ? tiles : parts;
  p.dw1_range = gnc::ceil_div(gnc::ceil_div(G, parts), 16) * 16;
  p.dw1_parts = gnc::ceil_div(G, p.dw1_range);
  int64_t groups = WG_TARGET / ftiles;
  groups = groups < 1 ? 1 : (groups > tiles ? tiles : groups);
  p.dy_tiles = gnc::ceil_div(tiles, groups);
  p.dy_groups = gnc::ceil_div(tiles, p.dy_tiles);
  p.fwd_ws = p.slices * G * BH1;
  p.bwd_ws = G * BH1 + (p.small_parts > 1 ? p.small_parts * p.small_len : 0) + (p.dw1_parts > 1 ? p.dw1_parts * BH1 * F : 0);
  if (ftiles > 0x7fffffffll || p.fwd_ws > (1ll << 40) || p.bwd_ws > (1ll << 40)) p.ok = false;
  return p;
}

// rows of y behind graph g that feed fc1: y_flat[base, base + lim), clamped to the table (a graph_ptr with values outside it reads
// as shorter or empty graphs, never outside y)
__device__ __forceinline__ void graph_extent(const int64_t* __restrict__ gp, int64_t g, int64_t num_nodes, int od, int64_t n_total,
                                             int64_t& base, int64_t& lim) {
  int64_t start = g * num_nodes, size = num_nodes;
  if (gp) {
    start = gp[g];
    size = gp[g + 1] - start;
  }
  int64_t rows = size < num_nodes ? size : num_nodes;
  if (start < 0 || start > n_total) rows = 0;
  else if (rows > n_total - start) rows = n_total - start;
  if (rows < 0) rows = 0;
  base = start * od;
  lim = rows * od;
}

__global__ __launch_bounds__(BT) void rb_fc1_kernel(const float* __restrict__ y, const int64_t* __restrict__ gp, int64_t G, int64_t num_nodes,
                                                    int od, int64_t n_total, int64_t F, const float* __restrict__ w1, int64_t ld1,
                                                    int64_t slice_len, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float As[16 * KP];
  __shared__ __attribute__((aligned(16))) float Ws[BH1 * KP];
  __shared__ int64_t sbase[16], slim[16];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int64_t tile = blockIdx.x, slice = blockIdx.y;
  if (tid < 16) {
    const int64_t g = tile * 16 + tid;
    int64_t b = 0, l = 0;
    if (g < G) graph_extent(gp, g, num_nodes, od, n_total, b, l);
    sbase[tid] = b;
    slim[tid] = l;
  }
  __syncthreads();
  const int64_t k_begin = slice * slice_len;
  const int64_t k_end = k_begin + slice_len < F ? k_begin + slice_len : F;
  const bool vec = ld1 % 4 == 0 && (reinterpret_cast<uintptr_t>(w1) & 15u) == 0;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int64_t k0 = k_begin; k0 < k_end; k0 += KT) {
#pragma unroll
    for (int j = 0; j < 16 * KT / BT; ++j) {  // feature tile: the gather rule
      const int e = tid + j * BT, r = e / KT, kk = e % KT;
      const int64_t k = k0 + kk;
      As[r * KP + kk] = k < slim[r] ? y[sbase[r] + k] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < BH1 * KT / 4 / BT; ++j) {  // W1 tile, columns at or behind F read as zeros
      const int e = tid + j * BT, h = e / (KT / 4), kk = (e % (KT / 4)) * 4;
      const int64_t k = k0 + kk;
      const float* src = w1 + (int64_t)h * ld1 + k;
      float4 v;
      if (vec && k + 3 < F) {
        v = *reinterpret_cast<const float4*>(src);
      } else {
        v.x = k < F ? src[0] : 0.f;
        v.y = k + 1 < F ? src[1] : 0.f;
        v.z = k + 2 < F ? src[2] : 0.f;
        v.w = k + 3 < F ? src[3] : 0.f;
      }
      *reinterpret_cast<float4*>(&Ws[h * KP + kk]) = v;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < KT; kk += 4) {
      const float a = As[lr * KP + kk + lk];
      acc0 = mfma16(a, Ws[(wave * 32 + lr) * KP + kk + lk], acc0);
      acc1 = mfma16(a, Ws[(wave * 32 + 16 + lr) * KP + kk + lk], acc1);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // D: column = lane & 15, row = 4 (lane >> 4) + i
    const int64_t g = tile * 16 + lk * 4 + i;
    if (g < G) {
      float* dst = part + (slice * G + g) * BH1 + wave * 32 + lr;
      dst[0] = acc0[i];
      dst[16] = acc1[i];
    }
  }
}

__global__ __launch_bounds__(BT) void rb_tail_kernel(const float* __restrict__ part, int64_t slices, int64_t G, int rows,
                                                     const float* __restrict__ b1, const float* __restrict__ w2, int64_t ld2,
                                                     const float* __restrict__ b2, int H2, const float* __restrict__ w3, int64_t ld3,
                                                     const float* __restrict__ b3, int C, float* __restrict__ h1, float* __restrict__ h2,
                                                     float* __restrict__ logits) {
  __shared__ float sw2[BMAXH2 * (BH1 + 1)], sw3[BMAXC * (BMAXH2 + 1)], sh1[16 * BH1], sh2[16 * (BMAXH2 + 1)];
  const int tid = threadIdx.x;
  const int64_t g0 = (int64_t)blockIdx.x * rows;
  for (int e = tid; e < H2 * BH1; e += BT) sw2[(e / BH1) * (BH1 + 1) + e % BH1] = w2[(int64_t)(e / BH1) * ld2 + e % BH1];
  for (int e = tid; e < C * H2; e += BT) sw3[(e / H2) * (BMAXH2 + 1) + e % H2] = w3[(int64_t)(e / H2) * ld3 + e % H2];
  for (int e = tid; e < rows * BH1; e += BT) {
    const int64_t g = g0 + e / BH1;
    const int h = e % BH1;
    float v = 0.f;
    if (g < G) {
      const float* p = part + g * BH1 + h;
      float a = p[0];
#pragma unroll 8
      for (int64_t s = 1; s < slices; ++s) a += p[s * G * BH1];  // ascending slice order
      v = relu_keep_nan(a + (b1 ? b1[h] : 0.f));
      h1[g * BH1 + h] = v;
    }
    sh1[e] = v;
  }
  __syncthreads();
  for (int e = tid; e < rows * H2; e += BT) {
    const int r = e / H2, o = e % H2;
    float a = 0.f;
#pragma unroll 8
    for (int k = 0; k < BH1; ++k) a += sw2[o * (BH1 + 1) + k] * sh1[r * BH1 + k];
    const float v = relu_keep_nan(a + (b2 ? b2[o] : 0.f));
    sh2[r * (BMAXH2 + 1) + o] = v;
    if (g0 + r < G) h2[(g0 + r) * H2 + o] = v;
  }
  __syncthreads();
  for (int e = tid; e < rows * C; e += BT) {
    const int r = e / C, c = e % C;
    float a = 0.f;
#pragma unroll 4
    for (int k = 0; k < H2; ++k) a += sw3[c * (BMAXH2 + 1) + k] * sh2[r * (BMAXH2 + 1) + k];
    if (g0 + r < G) logits[(g0 + r) * C + c] = a + (b3 ? b3[c] : 0.f);
  }
}

// dz2, dz1 of a chunk of GC graphs, and the chunk's part of the small gradients: out = [dW2 H2 x 128 | db2 | dW3 C x H2 | db3 | db1]
__global__ __launch_bounds__(BT) void rb_upper_kernel(const float* __restrict__ grad, const float* __restrict__ h1, const float* __restrict__ h2,
                                                      int64_t G, const float* __restrict__ w2, int64_t ld2, int H2,
                                                      const float* __restrict__ w3, int64_t ld3, int C, float* __restrict__ dz1,
                                                      float* __restrict__ out, int64_t out_stride) {
  __shared__ float sg[GC * BMAXC], sh2[GC * (BMAXH2 + 1)], sdz2[GC * (BMAXH2 + 1)], sh1[GC * BH1], sdz1[GC * BH1];
  const int tid = threadIdx.x;
  const int64_t g0 = (int64_t)blockIdx.x * GC;
  const int n = G - g0 < GC ? (int)(G - g0) : GC;
  for (int e = tid; e < GC * C; e += BT) sg[e] = e / C < n ? grad[g0 * C + e] : 0.f;
  for (int e = tid; e < GC * (BMAXH2 + 1); e += BT) {
    const int r = e / (BMAXH2 + 1), k = e % (BMAXH2 + 1);
    sh2[e] = (r < n && k < H2) ? h2[(g0 + r) * H2 + k] : 0.f;
    sdz2[e] = 0.f;
  }
  for (int e = tid; e < GC * BH1; e += BT) sh1[e] = e / BH1 < n ? h1[g0 * BH1 + e] : 0.f;
  __syncthreads();
  for (int e = tid; e < GC * H2; e += BT) {  // dz2[k] = (sum_c w3[c][k] g[c]) [h2[k] > 0], ascending c
    const int r = e / H2, k = e % H2;
    float a = 0.f;
#pragma unroll 4
    for (int c = 0; c < C; ++c) a += w3[(int64_t)c * ld3 + k] * sg[r * C + c];
    sdz2[r * (BMAXH2 + 1) + k] = sh2[r * (BMAXH2 + 1) + k] > 0.f ? a : 0.f;
  }
  __syncthreads();
  {  // dz1[h] = (sum_o w2[o][h] dz2[o]) [h1[h] > 0], ascending o; a thread keeps its column of w2
    const int h = tid % BH1;
    float wc[BMAXH2];
#pragma unroll
    for (int o = 0; o < BMAXH2; ++o) wc[o] = o < H2 ? w2[(int64_t)o * ld2 + h] : 0.f;
    for (int r = tid / BH1; r < GC; r += BT / BH1) {
      float a = 0.f;
#pragma unroll
      for (int o = 0; o < BMAXH2; ++o) a += wc[o] * sdz2[r * (BMAXH2 + 1) + o];
      const float v = sh1[r * BH1 + h] > 0.f ? a : 0.f;
      sdz1[r * BH1 + h] = v;
      if (r < n) dz1[(g0 + r) * BH1 + h] = v;
    }
  }
  __syncthreads();
  float* dst = out + (int64_t)blockIdx.x * out_stride;
  {  // dW2[o][h] = sum_r dz2[r][o] h1[r][h], ascending r
    const int h = tid % BH1, o0 = (tid / BH1) * (BMAXH2 / 2);
    float acc[BMAXH2 / 2];
#pragma unroll
    for (int j = 0; j < BMAXH2 / 2; ++j) acc[j] = 0.f;
#pragma unroll 2
    for (int r = 0; r < GC; ++r) {
      const float hv = sh1[r * BH1 + h];
#pragma unroll
      for (int j = 0; j < BMAXH2 / 2; ++j) acc[j] += sdz2[r * (BMAXH2 + 1) + o0 + j] * hv;
    }
#pragma unroll
    for (int j = 0; j < BMAXH2 / 2; ++j)
      if (o0 + j < H2) dst[(o0 + j) * BH1 + h] = acc[j];
  }
  dst += H2 * BH1;
  for (int o = tid; o < H2; o += BT) {
    float a = 0.f;
#pragma unroll 4
    for (int r = 0; r < GC; ++r) a += sdz2[r * (BMAXH2 + 1) + o];
    dst[o] = a;
  }
  dst += H2;
  for (int e = tid; e < C * H2; e += BT) {
    const int c = e / H2, k = e % H2;
    float a = 0.f;
#pragma unroll 4
    for (int r = 0; r < GC; ++r) a += sg[r * C + c] * sh2[r * (BMAXH2 + 1) + k];
    dst[e] = a;
  }
  dst += C * H2;
  for (int c = tid; c < C; c += BT) {
    float a = 0.f;
#pragma unroll 4
    for (int r = 0; r < GC; ++r) a += sg[r * C + c];
    dst[c] = a;
  }
  dst += C;
  for (int h = tid; h < BH1; h += BT) {
    float a = 0.f;
#pragma unroll 4
    for (int r = 0; r < GC; ++r) a += sdz1[r * BH1 + h];
    dst[h] = a;
  }
}

__global__ __launch_bounds__(BT) void rb_reduce_kernel(const float* __restrict__ part, int64_t parts, int64_t n, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * BT + threadIdx.x;
  if (e >= n) return;
  float a = part[e];
#pragma unroll 8
  for (int64_t p = 1; p < parts; ++p) a += part[p * n + e];  // ascending part order (the loads of a group are independent)
  out[e] = a;
}

__global__ __launch_bounds__(BT) void rb_dw1_kernel(const float* __restrict__ y, const int64_t* __restrict__ gp, int64_t G, int64_t num_nodes,
                                                    int od, int64_t n_total, int64_t F, const float* __restrict__ dz1, int64_t range,
                                                    float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float Ds[16 * DP];
  __shared__ float Fs[16 * FP];
  __shared__ int64_t sbase[16], slim[16];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int64_t f0 = (int64_t)blockIdx.x * FT, part = blockIdx.y;
  const int64_t g_begin = part * range, g_end = g_begin + range < G ? g_begin + range : G;
  f32x4 acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[a][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t gc = g_begin; gc < g_end; gc += 16) {
    if (tid < 16) {
      int64_t b = 0, l = 0;
      if (gc + tid < g_end) graph_extent(gp, gc + tid, num_nodes, od, n_total, b, l);
      sbase[tid] = b;
      slim[tid] = l;
    }
#pragma unroll
    for (int j = 0; j < 16 * BH1 / 4 / BT; ++j) {  // dz1 rows of the 16 graphs (the workspace is 16-B aligned)
      const int e = tid + j * BT, r = e / (BH1 / 4), h = (e % (BH1 / 4)) * 4;
      float4 v = {0.f, 0.f, 0.f, 0.f};
      if (gc + r < g_end) v = *reinterpret_cast<const float4*>(dz1 + (gc + r) * BH1 + h);
      *reinterpret_cast<float4*>(&Ds[r * DP + h]) = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16 * FT / BT; ++j) {  // their features of this F tile: the gather rule
      const int e = tid + j * BT, r = e / FT, ff = e % FT;
      const int64_t f = f0 + ff;
      Fs[r * FP + ff] = f < slim[r] ? y[sbase[r] + f] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; kk += 4) {  // A[h][g] = dz1[g][h], B[g][f] = feats[g][f]
      const float a0 = Ds[(kk + lk) * DP + wave * 32 + lr], a1 = Ds[(kk + lk) * DP + wave * 32 + 16 + lr];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float b = Fs[(kk + lk) * FP + j * 16 + lr];
        acc[0][j] = mfma16(a0, b, acc[0][j]);
        acc[1][j] = mfma16(a1, b, acc[1][j]);
      }
    }
    __syncthreads();
  }
  float* dst = out + part * BH1 * F;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t f = f0 + j * 16 + lr;
      if (f < F) {
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[(int64_t)(wave * 32 + a * 16 + lk * 4 + i) * F + f] = acc[a][j][i];
      }
    }
}

__global__ __launch_bounds__(BT) void rb_fill_zero_kernel(float* __restrict__ p, int64_t n) {
  for (int64_t e = (int64_t)blockIdx.x * BT + threadIdx.x; e < n; e += (int64_t)gridDim.x * BT) p[e] = 0.f;
}

__global__ __launch_bounds__(BT) void rb_dy_kernel(const int64_t* __restrict__ gp, int64_t G, int64_t num_nodes, int od, int64_t n_total,
                                                   int64_t F, const float* __restrict__ w1, int64_t ld1, const float* __restrict__ dz1,
                                                   int64_t tiles_per_group, float* __restrict__ dy) {
  __shared__ __attribute__((aligned(16))) float Wt[BH1 * FP];
  __shared__ __attribute__((aligned(16))) float Ds[16 * AP];
  __shared__ int64_t sbase[16], slim[16];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int64_t f0 = (int64_t)blockIdx.x * FT;
  const bool vec = ld1 % 4 == 0 && (reinterpret_cast<uintptr_t>(w1) & 15u) == 0;
#pragma unroll
  for (int j = 0; j < BH1 * FT / 4 / BT; ++j) {  // W1[:, f0 : f0 + 64], resident for all graph tiles of this workgroup
    const int e = tid + j * BT, h = e / (FT / 4), ff = (e % (FT / 4)) * 4;
    const int64_t f = f0 + ff;
    const float* src = w1 + (int64_t)h * ld1 + f;
    float4 v;
    if (vec && f + 3 < F) {
      v = *reinterpret_cast<const float4*>(src);
    } else {
      v.x = f < F ? src[0] : 0.f;
      v.y = f + 1 < F ? src[1] : 0.f;
      v.z = f + 2 < F ? src[2] : 0.f;
      v.w = f + 3 < F ? src[3] : 0.f;
    }
    *reinterpret_cast<float4*>(&Wt[h * FP + ff]) = v;
  }
  const int64_t tiles = (G + 15) / 16;
  const int64_t t_begin = (int64_t)blockIdx.y * tiles_per_group;
  const int64_t t_end = t_begin + tiles_per_group < tiles ? t_begin + tiles_per_group : tiles;
  for (int64_t t = t_begin; t < t_end; ++t) {
    const int64_t gc = t * 16;
    if (tid < 16) {
      int64_t b = 0, l = 0;
      if (gc + tid < G) graph_extent(gp, gc + tid, num_nodes, od, n_total, b, l);
      sbase[tid] = b;
      slim[tid] = l;
    }
#pragma unroll
    for (int j = 0; j < 16 * BH1 / 4 / BT; ++j) {
      const int e = tid + j * BT, r = e / (BH1 / 4), h = (e % (BH1 / 4)) * 4;
      float4 v = {0.f, 0.f, 0.f, 0.f};
      if (gc + r < G) v = *reinterpret_cast<const float4*>(dz1 + (gc + r) * BH1 + h);
      *reinterpret_cast<float4*>(&Ds[r * AP + h]) = v;
    }
    __syncthreads();
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};  // two chains over alternating k steps, added at the end
#pragma unroll
    for (int kk = 0; kk < BH1; kk += 8) {  // A[g][h] = dz1[g][h], B[h][f] = W1[h][f]
      acc0 = mfma16(Ds[lr * AP + kk + lk], Wt[(kk + lk) * FP + wave * 16 + lr], acc0);
      acc1 = mfma16(Ds[lr * AP + kk + 4 + lk], Wt[(kk + 4 + lk) * FP + wave * 16 + lr], acc1);
    }
    const int64_t f = f0 + wave * 16 + lr;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = lk * 4 + i;
      if (f < slim[r]) dy[sbase[r] + f] = acc0[i] + acc1[i];
    }
    __syncthreads();
  }
}

int check_widths(const char* who, int64_t G, int64_t num_nodes, int32_t od, int64_t n_total, int64_t ld1, int64_t ld2, int64_t ld3,
                 int32_t H1, int32_t H2, const int64_t* gp) {
  GNC_REQUIRE(num_nodes >= 1 && od >= 1 && n_total >= 0, "%s: num_nodes, out_dim >= 1 expected", who);
  GNC_REQUIRE(ld1 >= num_nodes * od && ld2 >= H1 && ld3 >= H2, "%s: leading dimension below the row width", who);
  GNC_REQUIRE(gp || n_total == G * num_nodes, "%s: without graph_ptr, y holds num_graphs x num_nodes rows", who);
  return GNC_OK;
}

}  // namespace

extern "C" int32_t gnc_readout_batched_supported(int64_t num_graphs, int64_t F, int32_t H1, int32_t H2, int32_t C,
                                                 gnc_readout_batched_plan_t* plan) {
  const Plan p = decide(num_graphs, F, H1, H2, C);
  if (plan) {
    plan->f_slices = p.slices;
    plan->f_slice_len = p.slice_len;
    plan->tail_rows = p.tail_rows;
    plan->small_parts = p.small_parts;
    plan->dw1_parts = p.dw1_parts;
    plan->dw1_graph_range = p.dw1_range;
    plan->dy_groups = p.dy_groups;
    plan->forward_workspace_floats = p.fwd_ws;
    plan->backward_workspace_floats = p.bwd_ws;
  }
  return p.ok ? 1 : 0;
}

extern "C" int gnc_readout_batched_forward_f32(const float* y, const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes, int32_t out_dim,
                                               int64_t n_total, const float* w1, int64_t ld1, const float* b1, int32_t H1, const float* w2,
                                               int64_t ld2, const float* b2, int32_t H2, const float* w3, int64_t ld3, const float* b3,
                                               int32_t C, float* h1, float* h2, float* logits, float* workspace, int64_t workspace_floats,
                                               void* stream) {
  GNC_REQUIRE(y && w1 && w2 && w3 && h1 && h2 && logits && workspace, "gnc_readout_batched_forward_f32: null pointer");
  const int64_t F = num_nodes * out_dim;
  const Plan p = decide(num_graphs, num_nodes >= 1 && out_dim >= 1 ? F : 0, H1, H2, C);
  if (!p.ok) {
    gnc::set_error("gnc_readout_batched_forward_f32: shape outside the supported set (fc1 width %d, fc2 width <= %d, classes <= %d)", BH1,
                   BMAXH2, BMAXC);
    return GNC_ERR_UNSUPPORTED;
  }
  if (int rc = check_widths("gnc_readout_batched_forward_f32", num_graphs, num_nodes, out_dim, n_total, ld1, ld2, ld3, H1, H2, graph_ptr)) return rc;
  if (workspace_floats < p.fwd_ws) {
    gnc::set_error("gnc_readout_batched_forward_f32: workspace of %lld floats, %lld needed", (long long)workspace_floats, (long long)p.fwd_ws);
    return GNC_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  rb_fc1_kernel<<<dim3((unsigned)gnc::ceil_div(num_graphs, 16), (unsigned)p.slices), dim3(BT), 0, s>>>(
      y, graph_ptr, num_graphs, num_nodes, out_dim, n_total, F, w1, ld1, p.slice_len, workspace);
  if (int rc = gnc::check_launch("rb_fc1_kernel")) return rc;
  rb_tail_kernel<<<dim3((unsigned)gnc::ceil_div(num_graphs, p.tail_rows)), dim3(BT), 0, s>>>(
      workspace, p.slices, num_graphs, (int)p.tail_rows, b1, w2, ld2, b2, H2, w3, ld3, b3, C, h1, h2, logits);
  return gnc::check_launch("rb_tail_kernel");
}

extern "C" int gnc_readout_batched_backward_f32(const float* grad_logits, const float* y, const int64_t* graph_ptr, int64_t num_graphs,
                                                int64_t num_nodes, int32_t out_dim, int64_t n_total, const float* w1, int64_t ld1, int32_t H1,
                                                const float* w2, int64_t ld2, int32_t H2, const float* w3, int64_t ld3, int32_t C,
                                                const float* h1, const float* h2, float* dw1, float* small_grads, float* dy, float* workspace,
                                                int64_t workspace_floats, void* stream) {
  GNC_REQUIRE(grad_logits && y && w1 && w2 && w3 && h1 && h2 && dw1 && small_grads && workspace,
              "gnc_readout_batched_backward_f32: null pointer");
  const int64_t F = num_nodes * out_dim, G = num_graphs;
  const Plan p = decide(G, num_nodes >= 1 && out_dim >= 1 ? F : 0, H1, H2, C);
  if (!p.ok) {
    gnc::set_error("gnc_readout_batched_backward_f32: shape outside the supported set (fc1 width %d, fc2 width <= %d, classes <= %d)", BH1,
                   BMAXH2, BMAXC);
    return GNC_ERR_UNSUPPORTED;
  }
  if (int rc = check_widths("gnc_readout_batched_backward_f32", G, num_nodes, out_dim, n_total, ld1, ld2, ld3, H1, H2, graph_ptr)) return rc;
  GNC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15u) == 0, "gnc_readout_batched_backward_f32: workspace not 16-B aligned");
  if (workspace_floats < p.bwd_ws) {
    gnc::set_error("gnc_readout_batched_backward_f32: workspace of %lld floats, %lld needed", (long long)workspace_floats, (long long)p.bwd_ws);
    return GNC_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  float* dz1 = workspace;
  float* small_part = dz1 + G * BH1;
  float* dw1_part = small_part + (p.small_parts > 1 ? p.small_parts * p.small_len : 0);
  rb_upper_kernel<<<dim3((unsigned)p.small_parts), dim3(BT), 0, s>>>(grad_logits, h1, h2, G, w2, ld2, H2, w3, ld3, C, dz1,
                                                                     p.small_parts > 1 ? small_part : small_grads, p.small_len);
  if (int rc = gnc::check_launch("rb_upper_kernel")) return rc;
  if (p.small_parts > 1) {
    rb_reduce_kernel<<<dim3((unsigned)gnc::ceil_div(p.small_len, BT)), dim3(BT), 0, s>>>(small_part, p.small_parts, p.small_len, small_grads);
    if (int rc = gnc::check_launch("rb_reduce_kernel")) return rc;
  }
  rb_dw1_kernel<<<dim3((unsigned)gnc::ceil_div(F, FT), (unsigned)p.dw1_parts), dim3(BT), 0, s>>>(
      y, graph_ptr, G, num_nodes, out_dim, n_total, F, dz1, p.dw1_range, p.dw1_parts > 1 ? dw1_part : dw1);
  if (int rc = gnc::check_launch("rb_dw1_kernel")) return rc;
  if (p.dw1_parts > 1) {
    rb_reduce_kernel<<<dim3((unsigned)gnc::ceil_div(BH1 * F, BT)), dim3(BT), 0, s>>>(dw1_part, p.dw1_parts, BH1 * F, dw1);
    if (int rc = gnc::check_launch("rb_reduce_kernel")) return rc;
  }
  if (dy) {
    if (graph_ptr) {  // rows behind num_nodes of a larger graph, rows outside every graph: cleared by a kernel (no memset node)
      const int64_t n = n_total * out_dim;
      if (n > 0) {
        const int64_t blocks = gnc::ceil_div(n, BT);
        rb_fill_zero_kernel<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(BT), 0, s>>>(dy, n);
        if (int rc = gnc::check_launch("rb_fill_zero_kernel")) return rc;
      }
    }
    rb_dy_kernel<<<dim3((unsigned)gnc::ceil_div(F, FT), (unsigned)p.dy_groups), dim3(BT), 0, s>>>(graph_ptr, G, num_nodes, out_dim, n_total, F,
                                                                                              w1, ld1, dz1, p.dy_tiles, dy);
    if (int rc = gnc::check_launch("rb_dy_kernel")) return rc;
  }
  return GNC_OK;
}
