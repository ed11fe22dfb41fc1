// Classification loss head (DESIGN K23): weighted cross-entropy with label smoothing, or the write-up's binary cross-entropy on one
// logit - loss, d loss / d logits, the trainer's float64 loss accumulator, the confusion counts and a label check.
//
// Launches of one call:
//   G <= GNC_CLASS_LOSS_ONE_LAUNCH_ROWS (the captured regime)   class_loss_one_kernel: ONE workgroup does all of it.
//   above                        class_loss_rows_kernel   per-row loss and weight, summed in double into one partial per workgroup of a
//                                                         grid that (G, C) alone decide; counts and the label flag
//                                class_loss_tick_kernel   one workgroup: the partials in fixed order (an LDS tree), den, the loss,
//                                                         the accumulator, and k = scale / den for the gradient
//                                class_loss_grad_kernel   (not in scoring mode) dlogits = k * g, the row statistics taken again
// No floating-point atomics and no grid sized from the compute-unit count: the bits depend on the values and on (G, C) alone.
// The counts and the flag are integer atomics (exact, order-independent).
//
// Lane mapping, chosen by C alone, so a row has the same bits alone and inside any batch:
//   C <= kLaneRowMaxC, and BCE    a lane per row, the classes walked serially
//   above                         a wave per row, lane l takes classes l, l + 64, ...; xor trees across the wave (a commutative
//                                 butterfly: every lane ends with the same bits)
//
// Per row, fp32, one rounding per operation (contraction off), accurate expf / logf / log1pf:
//   CE    m = max_c z_c (lowest index on ties: the predicted class);  S = sum_c expf(z_c - m);  lse = m + logf(S)
//         W = sum_c w_c;  T = sum_c w_c * (z_c - lse);  A = (1 - s) * w[y];  B = s / C
//         row = -(A * (z_y - lse)) - B * T
//         g_c = A * (p_c - [c == y]) + B * (W * p_c - w_c),  p_c = expf(z_c - m) / S
//   BCE   t = y * (1 - s) + s / 2;  e = expf(-|z|);  l = log1pf(e);  softplus(+-z) = max(+-z, 0) + l
//         row = pw * t * softplus(-z) + (1 - t) * softplus(z);  g = (1 - t) * sigmoid(z) - pw * t * sigmoid(-z)
//         sigmoid(|z|) = 1 / (1 + e), sigmoid(-|z|) = e / (1 + e);  predicted class: z > 0
// Across rows, double: sum = sum_i row_i, den = sum_i w[y_i] (MEAN; BCE: the number of rows) or 1 (SUM);
//   loss = fl32(scale * sum / den);  k = fl32(scale / den);  dlogits = k * g;  den == 0: loss = 0, k = 0.
// A row whose label lies outside the classes sets the flag and is otherwise absent: nothing is indexed with its label, its loss
// and weight are 0, its dlogits row is zeros, it is not counted.
#include <math.h>

#include "gnc_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / gnc::kWave;
constexpr int kBlocks = GNC_CLASS_LOSS_BLOCKS;  // == the tick kernel's workgroup size: one thread per partial
constexpr int kOneRows = GNC_CLASS_LOSS_ONE_LAUNCH_ROWS;
constexpr int kLaneRowMaxC = 8;
static_assert(kBlocks == 256 && kThreads == 256 && kOneRows == 64, "the LDS trees below halve from 128 and from 32");
static_assert(GNC_CLASS_LOSS_WORKSPACE_DOUBLES == 2 * kBlocks + 1, "two partials per workgroup and k");

enum { MODE_CE_LANE = 0, MODE_CE_WAVE = 1, MODE_BCE = 2 };

struct Head {
  const float* logits;
  int64_t ld;
  const int64_t* labels;
  const float* weight;  // [C] or null (CE)
  int64_t G;
  int C, K;      // K: classes of the labels and the counts (C, or 2 for BCE)
  int mean;
  float oms;     // 1 - s
  float B;       // CE: s / C;  BCE: s / 2
  float pw;      // BCE
  double scale;
};

struct Out {
  float* loss;
  float* dlogits;  // null: scoring only
  int64_t ld_d;
  double* loss_sum;
  int64_t* confusion;
  int32_t* status;
};

struct Row {
  float loss, wy;  // 0 for a row with a bad label
  float m, S, W;   // CE statistics
  int y, pred;     // y == -1: the label lies outside the classes
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int MODE>
__device__ __forceinline__ Row row_stats(const Head& h, int64_t i, int lane) {
#pragma clang fp contract(off)
  const float* __restrict__ z = h.logits + i * h.ld;
  const int64_t y64 = h.labels[i];
  Row r;
  r.y = (y64 >= 0 && y64 < (int64_t)h.K) ? (int)y64 : -1;  // the only use of the label as it came
  r.loss = r.wy = 0.f;
  r.m = r.S = r.W = 0.f;
  if (MODE == MODE_BCE) {
    const float x = z[0];
    r.pred = x > 0.f ? 1 : 0;
    if (r.y < 0) return r;
    const float t = r.y ? h.oms + h.B : h.B;
    const float l = log1pf(expf(-fabsf(x)));
    const float sp_pos = fmaxf(x, 0.f) + l, sp_neg = fmaxf(-x, 0.f) + l;
    const float a = (h.pw * t) * sp_neg, b = (1.f - t) * sp_pos;
    r.loss = a + b;
    r.wy = 1.f;
    return r;
  }
  const int C = h.C;
  const float* __restrict__ w = h.weight;
  float m, S = 0.f, T = 0.f, W = 0.f, lse;
  int best = 0;
  if (MODE == MODE_CE_LANE) {
    m = z[0];
    for (int c = 1; c < C; ++c) {
      const float v = z[c];
      if (v > m) m = v, best = c;
    }
    for (int c = 0; c < C; ++c) S += expf(z[c] - m);
    lse = m + logf(S);
    if (h.B != 0.f) {  // uniform; without smoothing neither W nor T is read (a class masked with -inf then stays harmless)
      for (int c = 0; c < C; ++c) {
        const float wc = w ? w[c] : 1.f;
        W += wc;
        T += wc * (z[c] - lse);
      }
    }
  } else {
    m = -INFINITY;  // a lane without a class: (-inf, 0) loses every comparison but a tie with class 0
    for (int c = lane; c < C; c += gnc::kWave) {
      const float v = z[c];
      if (v > m) m = v, best = c;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float om = __shfl_xor(m, off, 64);
      const int ob = __shfl_xor(best, off, 64);
      if (om > m || (om == m && ob < best)) m = om, best = ob;
    }
    for (int c = lane; c < C; c += gnc::kWave) S += expf(z[c] - m);
    S = wave_sum(S);
    lse = m + logf(S);
    if (h.B != 0.f) {
      for (int c = lane; c < C; c += gnc::kWave) {
        const float wc = w ? w[c] : 1.f;
        W += wc;
        T += wc * (z[c] - lse);
      }
      W = wave_sum(W);
      T = wave_sum(T);
    }
  }
  // whatever the logits hold (a NaN fails every comparison above), 0 <= best < C
  r.pred = best, r.m = m, r.S = S, r.W = W;
  if (r.y < 0) return r;
  r.wy = w ? w[r.y] : 1.f;
  const float A = h.oms * r.wy;
  const float a = A * (z[r.y] - lse), b = h.B != 0.f ? h.B * T : 0.f;
  r.loss = -a - b;
  return r;
}

// dlogits row i = k * g; a wave-per-row caller passes its lane, a lane-per-row caller 0
template <int MODE>
__device__ __forceinline__ void row_grad(const Head& h, const Out& o, int64_t i, const Row& r, float k, int lane) {
#pragma clang fp contract(off)
  const float* __restrict__ z = h.logits + i * h.ld;
  float* __restrict__ d = o.dlogits + i * o.ld_d;
  if (MODE == MODE_BCE) {
    float g = 0.f;
    if (r.y >= 0) {
      const float x = z[0];
      const float t = r.y ? h.oms + h.B : h.B;
      const float e = expf(-fabsf(x));
      const float big = 1.f / (1.f + e), small = e / (1.f + e);  // sigmoid(|x|), sigmoid(-|x|)
      const float sig_pos = x >= 0.f ? big : small, sig_neg = x >= 0.f ? small : big;
      const float a = (1.f - t) * sig_pos, b = (h.pw * t) * sig_neg;
      g = k * (a - b);
    }
    d[0] = g;
    return;
  }
  const int C = h.C;
  const int first = MODE == MODE_CE_LANE ? 0 : lane, step = MODE == MODE_CE_LANE ? 1 : gnc::kWave;
  if (r.y < 0) {
    for (int c = first; c < C; c += step) d[c] = 0.f;
    return;
  }
  const float* __restrict__ w = h.weight;
  const float A = h.oms * r.wy;
  for (int c = first; c < C; c += step) {
    const float p = expf(z[c] - r.m) / r.S;
    const float wc = w ? w[c] : 1.f;
    const float a = A * (p - (c == r.y ? 1.f : 0.f)), b = h.B != 0.f ? h.B * (r.W * p - wc) : 0.f;
    d[c] = k * (a + b);
  }
}

__device__ __forceinline__ void tally(const Head& h, const Out& o, const Row& r) {
  if (r.y < 0) {
    atomicOr(o.status, 1);
    return;
  }
  if (o.confusion) atomicAdd(reinterpret_cast<unsigned long long*>(o.confusion + (int64_t)r.y * h.K + r.pred), 1ull);
}

// One thread, after the rows are summed: the loss, the accumulator, and the gradient's factor k.
__device__ float finish(const Head& h, const Out& o, double sum, double wsum) {
#pragma clang fp contract(off)
  const double den = h.mean ? wsum : 1.0;
  double loss = 0.0, k = 0.0;
  if (den > 0.0) {
    loss = h.scale * sum / den;
    k = h.scale / den;
  }
  const float lf = (float)loss;
  o.loss[0] = lf;
  if (o.loss_sum) o.loss_sum[0] += (double)lf;
  return (float)k;
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void class_loss_one_kernel(Head h, Out o) {
  __shared__ Row rec[kOneRows];
  __shared__ double sh_loss[kOneRows], sh_w[kOneRows];
  __shared__ float sh_k;
  const int tid = threadIdx.x, lane = tid & (gnc::kWave - 1), wave = tid >> 6;
  const int G = (int)h.G;  // <= kOneRows
  if (tid < kOneRows) sh_loss[tid] = 0.0, sh_w[tid] = 0.0;
  __syncthreads();
  if (MODE == MODE_CE_WAVE) {
    for (int i = wave; i < G; i += kWaves) {
      const Row r = row_stats<MODE>(h, i, lane);
      if (lane == 0) {
        rec[i] = r, sh_loss[i] = (double)r.loss, sh_w[i] = (double)r.wy;
        tally(h, o, r);
      }
    }
  } else if (tid < G) {
    const Row r = row_stats<MODE>(h, tid, 0);
    rec[tid] = r, sh_loss[tid] = (double)r.loss, sh_w[tid] = (double)r.wy;
    tally(h, o, r);
  }
  __syncthreads();
#pragma unroll
  for (int s = kOneRows / 2; s > 0; s >>= 1) {  // the same order for every G: absent rows are zeros
    if (tid < s) sh_loss[tid] += sh_loss[tid + s], sh_w[tid] += sh_w[tid + s];
    __syncthreads();
  }
  if (tid == 0) sh_k = finish(h, o, sh_loss[0], sh_w[0]);
  if (!o.dlogits) return;  // uniform
  __syncthreads();
  const float k = sh_k;
  if (MODE == MODE_CE_WAVE) {
    for (int i = wave; i < G; i += kWaves) row_grad<MODE>(h, o, i, rec[i], k, lane);
  } else if (tid < G) {
    row_grad<MODE>(h, o, tid, rec[tid], k, 0);
  }
}

// sum over the workgroup in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double block_tree_sum(double v, double* sh) {
  const int tid = threadIdx.x;
  __syncthreads();  // the caller's last use of sh is over
  sh[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  return sh[0];
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void class_loss_rows_kernel(Head h, Out o, double* __restrict__ partials) {
  __shared__ double sh[kThreads];
  const int tid = threadIdx.x, lane = tid & (gnc::kWave - 1), wave = tid >> 6;
  double a = 0.0, w = 0.0;
  if (MODE == MODE_CE_WAVE) {
    for (int64_t i = (int64_t)blockIdx.x * kWaves + wave; i < h.G; i += (int64_t)gridDim.x * kWaves) {
      const Row r = row_stats<MODE>(h, i, lane);
      if (lane == 0) {
        a += (double)r.loss, w += (double)r.wy;
        tally(h, o, r);
      }
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + tid; i < h.G; i += (int64_t)gridDim.x * kThreads) {
      const Row r = row_stats<MODE>(h, i, 0);
      a += (double)r.loss, w += (double)r.wy;
      tally(h, o, r);
    }
  }
  const double ta = block_tree_sum(a, sh);
  const double tw = block_tree_sum(w, sh);
  if (tid == 0) partials[blockIdx.x] = ta, partials[kBlocks + blockIdx.x] = tw;
}

__global__ __launch_bounds__(kBlocks) void class_loss_tick_kernel(Head h, Out o, double* __restrict__ workspace, int blocks) {
  __shared__ double sh[kBlocks];
  const int tid = threadIdx.x;
  const bool live = tid < blocks;  // the rows grid wrote this many partials
  const double ta = block_tree_sum(live ? workspace[tid] : 0.0, sh);
  const double tw = block_tree_sum(live ? workspace[kBlocks + tid] : 0.0, sh);
  if (tid == 0) workspace[2 * kBlocks] = (double)finish(h, o, ta, tw);
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void class_loss_grad_kernel(Head h, Out o, const double* __restrict__ workspace) {
  const int tid = threadIdx.x, lane = tid & (gnc::kWave - 1), wave = tid >> 6;
  const float k = (float)workspace[2 * kBlocks];  // exact: the tick stored an fp32 value
  if (MODE == MODE_CE_WAVE) {
    for (int64_t i = (int64_t)blockIdx.x * kWaves + wave; i < h.G; i += (int64_t)gridDim.x * kWaves)
      row_grad<MODE>(h, o, i, row_stats<MODE>(h, i, lane), k, lane);
  } else {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + tid; i < h.G; i += (int64_t)gridDim.x * kThreads)
      row_grad<MODE>(h, o, i, row_stats<MODE>(h, i, 0), k, 0);
  }
}

template <int MODE>
int launch(const Head& h, const Out& o, double* workspace, hipStream_t stream) {
  if (h.G <= kOneRows) {
    class_loss_one_kernel<MODE><<<1, kThreads, 0, stream>>>(h, o);
    return gnc::check_launch("class_loss_one_kernel");
  }
  const int64_t rows_per_block = MODE == MODE_CE_WAVE ? kWaves : kThreads;
  const int64_t need = gnc::ceil_div(h.G, rows_per_block);
  const int blocks = (int)(need < kBlocks ? need : kBlocks);  // of (G, C) alone
  int rc;
  class_loss_rows_kernel<MODE><<<blocks, kThreads, 0, stream>>>(h, o, workspace);
  if ((rc = gnc::check_launch("class_loss_rows_kernel"))) return rc;
  class_loss_tick_kernel<<<1, kBlocks, 0, stream>>>(h, o, workspace, blocks);
  if ((rc = gnc::check_launch("class_loss_tick_kernel"))) return rc;
  if (!o.dlogits) return GNC_OK;
  class_loss_grad_kernel<MODE><<<blocks, kThreads, 0, stream>>>(h, o, workspace);
  return gnc::check_launch("class_loss_grad_kernel");
}

}  // namespace

extern "C" int32_t gnc_class_loss_workspace_doubles(void) { return GNC_CLASS_LOSS_WORKSPACE_DOUBLES; }

extern "C" int32_t gnc_class_loss_launches(int64_t G, int32_t with_gradient) {
  return G <= kOneRows ? 1 : 2 + (with_gradient ? 1 : 0);
}

extern "C" int gnc_class_loss_f32(const float* logits, int64_t ld_logits, const int64_t* labels, const float* class_weight, int64_t G,
                                  int64_t C, int32_t kind, double label_smoothing, double pos_weight, int32_t reduction, double scale,
                                  float* loss, float* dlogits, int64_t ld_dlogits, double* loss_sum, int64_t* confusion,
                                  int32_t* status, double* workspace, void* stream_) {
  const char* who = "gnc_class_loss_f32";
  GNC_REQUIRE(G >= 0 && C >= 1 && C <= (1 << 24), "%s: G >= 0 and 1 <= C <= 2^24 expected", who);
  GNC_REQUIRE(kind == GNC_LOSS_CE || kind == GNC_LOSS_BCE, "%s: unknown kind", who);
  GNC_REQUIRE(reduction == GNC_LOSS_MEAN || reduction == GNC_LOSS_SUM, "%s: unknown reduction", who);
  // every comparison is written so that a NaN fails it
  GNC_REQUIRE(label_smoothing >= 0.0 && label_smoothing < 1.0, "%s: label_smoothing must lie in [0, 1)", who);
  GNC_REQUIRE(scale >= -3.0e38 && scale <= 3.0e38, "%s: scale must be finite", who);
  if (kind == GNC_LOSS_BCE) {
    GNC_REQUIRE(C == 1, "%s: the binary loss takes ONE logit per row, not %lld", who, (long long)C);
    GNC_REQUIRE(!class_weight, "%s: class_weight belongs to the cross-entropy", who);
    GNC_REQUIRE(pos_weight >= 0.0 && pos_weight <= 3.0e38, "%s: pos_weight must be finite and >= 0", who);
  }
  GNC_REQUIRE(loss && status && (G == 0 || (logits && labels)), "%s: null pointer", who);
  GNC_REQUIRE(G <= 1 || ld_logits >= C, "%s: the logits' row stride is below C", who);
  GNC_REQUIRE(!dlogits || G <= 1 || ld_dlogits >= C, "%s: dlogits' row stride is below C", who);
  GNC_REQUIRE(G <= kOneRows || workspace, "%s: more than %d rows need the workspace", who, kOneRows);
  GNC_REQUIRE(gnc::aligned_to(logits, 4) && gnc::aligned_to(dlogits, 4) && gnc::aligned_to(class_weight, 4) && gnc::aligned_to(loss, 4) &&
                  gnc::aligned_to(status, 4) && gnc::aligned_to(labels, 8) && gnc::aligned_to(loss_sum, 8) &&
                  gnc::aligned_to(confusion, 8) && gnc::aligned_to(workspace, 8),
              "%s: misaligned buffer", who);
  Head h;
  h.logits = logits, h.ld = ld_logits, h.labels = labels, h.weight = class_weight;
  h.G = G, h.C = (int)C, h.K = kind == GNC_LOSS_BCE ? 2 : (int)C;
  h.mean = reduction == GNC_LOSS_MEAN;
  h.oms = (float)(1.0 - label_smoothing);
  h.B = (float)(kind == GNC_LOSS_BCE ? label_smoothing / 2.0 : label_smoothing / (double)C);
  h.pw = (float)pos_weight;
  h.scale = scale;
  const Out o = {loss, dlogits, ld_dlogits, loss_sum, confusion, status};
  hipStream_t stream = (hipStream_t)stream_;
  if (kind == GNC_LOSS_BCE) return launch<MODE_BCE>(h, o, workspace, stream);
  if (C <= kLaneRowMaxC) return launch<MODE_CE_LANE>(h, o, workspace, stream);
  return launch<MODE_CE_WAVE>(h, o, workspace, stream);
}
