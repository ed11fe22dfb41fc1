// K16: the first Linear of an MLP whose input is wide and whose batch is small (the image-MLP baseline, main.py:21-29:
// [8, 3 * 128 * 128] x [128, 49152]^T).  Every fused-MLP kernel tiles over rows only, so such a call is ONE workgroup walking a 25 MB
// weight matrix; here the K dimension is split instead, as fc1 of the batched read-out is (K13, readout_batched.hip).
//
// Forward, two launches.  wl_partial_kernel: a workgroup owns 16 rows x all H outputs (padded to a multiple of 16) x one slice of K;
// x and W0 tiles go through LDS in 32-wide steps (the next step's tile is already on its way in registers), the products run on
// v_mfma_f32_16x16x4_f32 (wave w owns the 16-output tiles w, w + 4, ...), and the workgroup writes its [16, HP] partial into the
// caller's workspace.  wl_tail_kernel: sums the slices in ascending order, adds b0, stores the pre-activation when asked (the backward
// of an activation other than ReLU reads it) and the activation (gnc_mlp::activate: the ids and formulas of every fused-MLP kernel).
//
// Backward.  wl_dw_kernel: dz0 = da0 * act' is formed where the operand is staged (ReLU: from a0 > 0; otherwise from z0), dW0 [H, K] =
// dz0^T x on MFMA with K as the M dimension, so that a lane ends up with four consecutive columns of one row of dW0 and stores them as
// one 16-B piece where the pitch allows; a workgroup owns all H rows x 64 columns of dW0 over one range of rows, and the workgroups of
// the first column tile also form db0 (column sums of dz0, ascending rows).  Range partials are summed by wl_reduce_kernel in ascending
// order.  dx is not formed: the input of this Linear is data.  No atomics, no ticket, no memset: the workspace belongs to the call and
// every sum has one order, so both directions are bitwise reproducible and every launch is a kernel node under stream capture.
#include "mlp_device.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool dev_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// d act(x) / dx as torch.autograd has it (the formulas of csrc/elementwise.hip)
__device__ __forceinline__ float act_grad(float x, int act, float p) {
  switch (act) {
    case GNC_ACT_RELU: return x > 0.f ? 1.f : 0.f;  // also right on the post-activation: relu(z) > 0 <=> z > 0
    case GNC_ACT_IDENTITY: return 1.f;
    case GNC_ACT_TANH: { const float t = tanhf(x); return 1.f - t * t; }
    case GNC_ACT_SIGMOID: { const float s = 1.f / (1.f + expf(-x)); return s * (1.f - s); }
    case GNC_ACT_SILU: { const float s = 1.f / (1.f + expf(-x)); return s * (1.f + x * (1.f - s)); }
    case GNC_ACT_GELU: {
      const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752440f));
      const float pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
      return cdf + x * pdf;
    }
    case GNC_ACT_LEAKY_RELU: return x > 0.f ? 1.f : p;
    case GNC_ACT_ELU: return x > 0.f ? 1.f : p * expf(x);
    default: return 1.f;
  }
}

constexpr int BT = 256;    // threads per workgroup (4 waves)
constexpr int MAXH = 256;  // widest first Linear served
constexpr int KT = 32;     // forward: k step staged in LDS
constexpr int KP = 36;     // ... and its row pitch: 16-B aligned rows, and (36 r + k) mod 64 is distinct over 16 rows x 4 k
constexpr int FT = 64;     // backward: columns of dW0 a workgroup owns
constexpr int FP = 80;     // pitch of a [row][64] operand tile (80 = 16 mod 64: 4 k x 16 columns hit 64 banks)
constexpr int WPT = MAXH * (KT / 4) / BT;  // 16-B pieces of a W0 tile per thread, at most
constexpr int MIN_K = 1024;                // narrower first Linears stay with the row-tiled kernels
constexpr int MIN_SLICE = 64, MAX_SLICES = 256, WG_TARGET = 512;
constexpr int64_t MAX_ROWS = 512;  // the largest batch timed against the row-tiled kernels (DESIGN K16): larger ones stay with them
constexpr int64_t MAX_K = 1ll << 26;

struct Plan {
  bool ok;
  int32_t hp;  // H padded to a multiple of 16
  int64_t slices, slice_len, dw_parts, dw_range, fwd_ws, bwd_ws;
};

// The ONE decision about a shape: the launchers, gnc_wide_linear_supported and gnc_wide_linear_workspace_floats all read it.
Plan decide(int64_t rows, int64_t K, int32_t H) {
  Plan p = {};
  if (rows < 1 || rows > MAX_ROWS || K < MIN_K || K > MAX_K || H < 1 || H > MAXH) return p;
  p.ok = true;
  p.hp = (H + 15) / 16 * 16;
  const int64_t tiles = gnc::ceil_div(rows, 16);
  int64_t want = WG_TARGET / tiles;  // slices that bring the grid to about two workgroups per CU
  want = want < 1 ? 1 : (want > MAX_SLICES ? MAX_SLICES : want);
  const int64_t len = gnc::ceil_div(gnc::ceil_div(K, want), KT) * KT;
  p.slice_len = len < MIN_SLICE ? MIN_SLICE : len;
  p.slices = gnc::ceil_div(K, p.slice_len);
  const int64_t ftiles = gnc::ceil_div(K, FT);
  int64_t parts = gnc::ceil_div(WG_TARGET / 2, ftiles);
  parts = parts > tiles ? tiles : parts;
  p.dw_range = gnc::ceil_div(gnc::ceil_div(rows, parts), 16) * 16;
  p.dw_parts = gnc::ceil_div(rows, p.dw_range);
  p.fwd_ws = p.slices * rows * p.hp;
  p.bwd_ws = p.dw_parts > 1 ? p.dw_parts * ((int64_t)H * K + p.hp) : 0;
  if (tiles > 0x7fffffffll || p.fwd_ws > (1ll << 40) || p.bwd_ws > (1ll << 40)) p.ok = false;
  return p;
}

// ... and about a fused-MLP description: ONE plain row-ordered segment in front of at least two Linears, nothing fused around it
Plan decide(const gnc_mlp_desc_t* d) {
  Plan none = {};
  if (!d || d->num_segments != 1 || d->num_linear < 2 || d->num_linear > GNC_MAX_LINEAR) return none;
  const gnc_mlp_segment_t& s = d->seg[0];
  if (s.index || s.mode != GNC_SEG_MATMUL || s.wcol != 0 || s.width != d->in_dim[0] || s.ld < s.width) return none;
  if (d->residual || d->agg_out || d->ef_pos || d->save_act[0]) return none;
  if (d->activation < GNC_ACT_RELU || d->activation > GNC_ACT_ELU || d->ld_weight[0] < d->in_dim[0]) return none;
  return decide(d->rows, d->in_dim[0], d->out_dim[0]);
}

// 4 floats at p[0 .. 3] of a row that ends at column `limit` (col = column of p[0]); 16-B load when the row allows it
__device__ __forceinline__ float4 load4(const float* __restrict__ p, int64_t col, int64_t limit, bool vec, bool row_ok) {
  float4 v = {0.f, 0.f, 0.f, 0.f};
  if (!row_ok) return v;
  if (vec && col + 3 < limit) return *reinterpret_cast<const float4*>(p);
  if (col < limit) v.x = p[0];
  if (col + 1 < limit) v.y = p[1];
  if (col + 2 < limit) v.z = p[2];
  if (col + 3 < limit) v.w = p[3];
  return v;
}

__global__ __launch_bounds__(BT) void wl_partial_kernel(const float* __restrict__ x, int64_t ldx, int64_t rows, int64_t K,
                                                        const float* __restrict__ w, int64_t ldw, int H, int HP, int64_t slice_len,
                                                        float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float As[16 * KP];
  __shared__ __attribute__((aligned(16))) float Ws[MAXH * KP];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int64_t tile = blockIdx.x, slice = blockIdx.y;
  const int64_t k_begin = slice * slice_len;
  const int64_t k_end = k_begin + slice_len < K ? k_begin + slice_len : K;
  const bool vecw = ldw % 4 == 0 && dev_aligned16(w), vecx = ldx % 4 == 0 && dev_aligned16(x);
  const int ntiles = HP / 16, pieces = HP * (KT / 4);
  const int xr = tid / (KT / 4), xk = (tid % (KT / 4)) * 4;  // threads below 128 carry the x tile, one 16-B piece each
  const int64_t xrow = tile * 16 + xr;
  float4 xreg = {0.f, 0.f, 0.f, 0.f}, wreg[WPT];
  auto fetch = [&](int64_t k0) {  // global -> registers; columns at or behind K and rows outside the operands read as zeros
    if (tid < 16 * (KT / 4)) xreg = load4(x + xrow * ldx + k0 + xk, k0 + xk, K, vecx, xrow < rows);
#pragma unroll
    for (int j = 0; j < WPT; ++j) {
      const int e = tid + j * BT, h = e / (KT / 4), kk = (e % (KT / 4)) * 4;
      if (e < pieces) wreg[j] = load4(w + (int64_t)h * ldw + k0 + kk, k0 + kk, K, vecw, h < H);
    }
  };
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  fetch(k_begin);
  for (int64_t k0 = k_begin; k0 < k_end; k0 += KT) {
    if (tid < 16 * (KT / 4)) *reinterpret_cast<float4*>(&As[xr * KP + xk]) = xreg;
#pragma unroll
    for (int j = 0; j < WPT; ++j) {
      const int e = tid + j * BT;
      if (e < pieces) *reinterpret_cast<float4*>(&Ws[(e / (KT / 4)) * KP + (e % (KT / 4)) * 4]) = wreg[j];
    }
    __syncthreads();
    if (k0 + KT < k_end) fetch(k0 + KT);
#pragma unroll
    for (int kk = 0; kk < KT; kk += 4) {  // A[row][k] = x, B[k][h] = W0[h][k]
      const float a = As[lr * KP + kk + lk];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (wave + 4 * j < ntiles) acc[j] = mfma16(a, Ws[((wave + 4 * j) * 16 + lr) * KP + kk + lk], acc[j]);  // wave-uniform
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (wave + 4 * j >= ntiles) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // D: column = lane & 15, row = 4 (lane >> 4) + i
      const int64_t r = tile * 16 + lk * 4 + i;
      if (r < rows) part[(slice * rows + r) * HP + (wave + 4 * j) * 16 + lr] = acc[j][i];
    }
  }
}

__global__ __launch_bounds__(BT) void wl_tail_kernel(const float* __restrict__ part, int64_t slices, int64_t rows, int H, int HP,
                                                     const float* __restrict__ bias, int act, float act_param, float* __restrict__ a0,
                                                     int64_t lda, float* __restrict__ z0, int64_t ldz) {
  const int64_t e = (int64_t)blockIdx.x * BT + threadIdx.x;
  if (e >= rows * H) return;
  const int64_t r = e / H;
  const int h = (int)(e - r * H);
  const float* p = part + r * HP + h;
  float a = p[0];
#pragma unroll 8
  for (int64_t s = 1; s < slices; ++s) a += p[s * rows * HP];  // ascending slice order
  const float z = a + (bias ? bias[h] : 0.f);
  if (z0) z0[r * ldz + h] = z;
  a0[r * lda + h] = gnc_mlp::activate(z, act, act_param);
}

__global__ __launch_bounds__(BT) void wl_reduce_kernel(const float* __restrict__ part, int64_t parts, int64_t n, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * BT + threadIdx.x;
  if (e >= n) return;
  float a = part[e];
#pragma unroll 8
  for (int64_t p = 1; p < parts; ++p) a += part[p * n + e];  // ascending part order
  out[e] = a;
}

// AT: 16-row tiles of dW0 per wave; the workgroup owns rows [0, 64 AT) of dW0 (those at or behind H are zeros and not stored)
template <int AT>
__global__ __launch_bounds__(BT) void wl_dw_kernel(const float* __restrict__ da, int64_t ldd, const float* __restrict__ az, int64_t ldaz,
                                                   const float* __restrict__ x, int64_t ldx, int64_t rows, int64_t K, int H, int act,
                                                   float act_param, int64_t range, float* __restrict__ dw, int64_t ld_dw,
                                                   int64_t dw_part_stride, float* __restrict__ db, int64_t db_part_stride) {
  constexpr int HW = 64 * AT, DP = HW + 16;  // pitch of dz0 rows read with k = row: 16 mod 64
  __shared__ float Ds[16 * DP];
  __shared__ float Fs[16 * FP];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int64_t f0 = (int64_t)blockIdx.x * FT, part = blockIdx.y;
  const int64_t g_begin = part * range, g_end = g_begin + range < rows ? g_begin + range : rows;
  const bool sums = blockIdx.x == 0 && tid < HW;
  float colsum = 0.f;
  f32x4 acc[AT][4];
#pragma unroll
  for (int a = 0; a < AT; ++a)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[a][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t gc = g_begin; gc < g_end; gc += 16) {
    // every load of the tile is issued before the first is used (addresses clamped into the operands, values outside them dropped)
    float dv[16 * HW / BT], zv[16 * HW / BT], xv[16 * FT / BT];
#pragma unroll
    for (int j = 0; j < 16 * HW / BT; ++j) {  // dz0 of 16 rows
      const int e = tid + j * BT, r = e / HW, h = e % HW;
      const int64_t row = gc + r < g_end ? gc + r : g_end - 1;
      const int hc = h < H ? h : H - 1;
      dv[j] = da[row * ldd + hc];
      zv[j] = az[row * ldaz + hc];
    }
#pragma unroll
    for (int j = 0; j < 16 * FT / BT; ++j) {  // their inputs of this column tile
      const int e = tid + j * BT, r = e / FT;
      const int64_t row = gc + r < g_end ? gc + r : g_end - 1, f = f0 + e % FT;
      xv[j] = x[row * ldx + (f < K ? f : K - 1)];
    }
#pragma unroll
    for (int j = 0; j < 16 * HW / BT; ++j) {
      const int e = tid + j * BT, r = e / HW, h = e % HW;
      Ds[r * DP + h] = (gc + r < g_end && h < H) ? dv[j] * act_grad(zv[j], act, act_param) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 16 * FT / BT; ++j) {
      const int e = tid + j * BT, r = e / FT, ff = e % FT;
      Fs[r * FP + ff] = (gc + r < g_end && f0 + ff < K) ? xv[j] : 0.f;
    }
    __syncthreads();
    if (sums) {
#pragma unroll
      for (int r = 0; r < 16; ++r) colsum += Ds[r * DP + tid];  // ascending rows
    }
#pragma unroll
    for (int kk = 0; kk < 16; kk += 4) {  // A[f][row] = x[row][f], B[row][h] = dz0[row][h]
      float b[AT];
#pragma unroll
      for (int a = 0; a < AT; ++a) b[a] = Ds[(kk + lk) * DP + (wave * AT + a) * 16 + lr];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float xa = Fs[(kk + lk) * FP + j * 16 + lr];
#pragma unroll
        for (int a = 0; a < AT; ++a) acc[a][j] = mfma16(xa, b[a], acc[a][j]);
      }
    }
    __syncthreads();
  }
  float* dst = dw + part * dw_part_stride;
  const bool vec = ld_dw % 4 == 0 && dev_aligned16(dst);
#pragma unroll
  for (int a = 0; a < AT; ++a) {
    const int h = (wave * AT + a) * 16 + lr;  // D: column = lane & 15 = h, row = 4 (lane >> 4) + i = f
    if (h >= H) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t f = f0 + j * 16 + lk * 4;
      float* q = dst + (int64_t)h * ld_dw + f;
      if (vec && f + 3 < K) {
        *reinterpret_cast<float4*>(q) = float4{acc[a][j][0], acc[a][j][1], acc[a][j][2], acc[a][j][3]};
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (f + i < K) q[i] = acc[a][j][i];
      }
    }
  }
  if (sums && tid < H) db[part * db_part_stride + tid] = colsum;
}

int check_act(const char* who, int32_t activation) {
  GNC_REQUIRE(activation >= GNC_ACT_RELU && activation <= GNC_ACT_ELU, "%s: unknown activation %d", who, activation);
  return GNC_OK;
}

int unsupported(const char* who) {
  gnc::set_error("%s: shape outside the supported set (1 <= rows <= %lld, %d <= K <= 2^26, 1 <= H <= %d)", who, (long long)MAX_ROWS, MIN_K, MAXH);
  return GNC_ERR_UNSUPPORTED;
}

}  // namespace

extern "C" int32_t gnc_wide_linear_supported(const gnc_mlp_desc_t* desc, gnc_wide_linear_plan_t* plan) {
  const Plan p = decide(desc);
  if (plan) {
    plan->k_slices = p.slices;
    plan->k_slice_len = p.slice_len;
    plan->dw_parts = p.dw_parts;
    plan->dw_row_range = p.dw_range;
    plan->forward_workspace_floats = p.fwd_ws;
    plan->backward_workspace_floats = p.bwd_ws;
  }
  return p.ok ? 1 : 0;
}

extern "C" int64_t gnc_wide_linear_workspace_floats(int64_t rows, int64_t K, int32_t H, int32_t backward) {
  const Plan p = decide(rows, K, H);
  if (!p.ok) return -1;
  return backward ? p.bwd_ws : p.fwd_ws;
}

extern "C" int gnc_wide_linear_forward_f32(const float* x, int64_t ld_x, int64_t rows, int64_t K, const float* w, int64_t ld_w,
                                           const float* bias, int32_t H, int32_t activation, float act_param, float* a0, int64_t ld_a,
                                           float* z0, int64_t ld_z, float* workspace, int64_t workspace_floats, void* stream) {
  const char* who = "gnc_wide_linear_forward_f32";
  GNC_REQUIRE(x && w && a0 && workspace, "%s: null pointer", who);
  const Plan p = decide(rows, K, H);
  if (!p.ok) return unsupported(who);
  if (int rc = check_act(who, activation)) return rc;
  GNC_REQUIRE(ld_x >= K && ld_w >= K && ld_a >= H && (!z0 || ld_z >= H), "%s: leading dimension below the row width", who);
  if (workspace_floats < p.fwd_ws) {
    gnc::set_error("%s: workspace of %lld floats, %lld needed", who, (long long)workspace_floats, (long long)p.fwd_ws);
    return GNC_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  wl_partial_kernel<<<dim3((unsigned)gnc::ceil_div(rows, 16), (unsigned)p.slices), dim3(BT), 0, s>>>(x, ld_x, rows, K, w, ld_w, H, p.hp,
                                                                                                   p.slice_len, workspace);
  if (int rc = gnc::check_launch("wl_partial_kernel")) return rc;
  wl_tail_kernel<<<dim3((unsigned)gnc::ceil_div(rows * H, BT)), dim3(BT), 0, s>>>(workspace, p.slices, rows, H, p.hp, bias, activation,
                                                                                 act_param, a0, ld_a, z0, ld_z);
  return gnc::check_launch("wl_tail_kernel");
}

extern "C" int gnc_wide_linear_backward_f32(const float* grad_a0, int64_t ld_grad, const float* az, int64_t ld_az, const float* x,
                                            int64_t ld_x, int64_t rows, int64_t K, int32_t H, int32_t activation, float act_param,
                                            float* dw, float* db, float* workspace, int64_t workspace_floats, void* stream) {
  const char* who = "gnc_wide_linear_backward_f32";
  GNC_REQUIRE(grad_a0 && az && x && dw && db, "%s: null pointer", who);
  const Plan p = decide(rows, K, H);
  if (!p.ok) return unsupported(who);
  if (int rc = check_act(who, activation)) return rc;
  GNC_REQUIRE(ld_grad >= H && ld_az >= H && ld_x >= K, "%s: leading dimension below the row width", who);
  const bool parts = p.dw_parts > 1;
  if (parts) {
    GNC_REQUIRE(workspace && gnc::aligned16(workspace), "%s: workspace missing or not 16-B aligned", who);
    if (workspace_floats < p.bwd_ws) {
      gnc::set_error("%s: workspace of %lld floats, %lld needed", who, (long long)workspace_floats, (long long)p.bwd_ws);
      return GNC_ERR_WORKSPACE;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)H * K;
  float* dw_dst = parts ? workspace : dw;
  float* db_dst = parts ? workspace + p.dw_parts * n : db;
  const dim3 grid((unsigned)gnc::ceil_div(K, FT), (unsigned)p.dw_parts);
#define GNC_WL_DW(AT)                                                                                                                 \
  wl_dw_kernel<AT><<<grid, dim3(BT), 0, s>>>(grad_a0, ld_grad, az, ld_az, x, ld_x, rows, K, H, activation, act_param, p.dw_range, dw_dst, \
                                             K, n, db_dst, H)
  switch ((p.hp + 63) / 64) {
    case 1: GNC_WL_DW(1); break;
    case 2: GNC_WL_DW(2); break;
    case 3: GNC_WL_DW(3); break;
    default: GNC_WL_DW(4); break;
  }
#undef GNC_WL_DW
  if (int rc = gnc::check_launch("wl_dw_kernel")) return rc;
  if (parts) {
    wl_reduce_kernel<<<dim3((unsigned)gnc::ceil_div(n, BT)), dim3(BT), 0, s>>>(workspace, p.dw_parts, n, dw);
    if (int rc = gnc::check_launch("wl_reduce_kernel")) return rc;
    wl_reduce_kernel<<<dim3((unsigned)gnc::ceil_div(H, BT)), dim3(BT), 0, s>>>(db_dst, p.dw_parts, H, db);
    return gnc::check_launch("wl_reduce_kernel");
  }
  return GNC_OK;
}
