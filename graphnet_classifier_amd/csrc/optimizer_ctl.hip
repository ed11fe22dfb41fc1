// Controlled optimizer step over the flat buffers (DESIGN K22): gradient clipping by the global norm, Adam + L2 / AdamW / SGD,
// learning-rate schedules and a skip on non-finite gradients - with every scalar that steers the update ON THE DEVICE, so that
// one captured step replays all of it.  optimizer.hip (K10) stays the default path: Adam at a fixed lr, two launches.
//
// Launches of one step:
//   grad_sumsq_kernel   (only with clipping or the non-finite check)  sum of g * g into kSumBlocks partials in double.  The grid
//                       is a compile-time constant and every thread walks a fixed stride, so the summation order - and the bits
//                       of the norm - depend on n alone (not on the compute-unit count, as the element grids do); no atomics.
//                       fp32 x fp32 is exact in double, and finite fp32 squares cannot overflow a double sum at any n, so a
//                       non-finite sum means a non-finite gradient.
//   ctl_tick_kernel     one workgroup: sums the partials in fixed order (an LDS tree), advances the step counter and derives the
//                       step's scalars in double, each rounded to fp32 once (see gnc_hip.h for the layout):
//                         t = step + 1;  lr = lr_at(t);  norm = sqrt(sum);  clip_coef = min(1, max_norm / (norm + 1e-6))
//                         Adam, AdamW: step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t);  AdamW: decay = 1 - lr * wd
//                         SGD: step_size = lr
//                       Non-finite sum: the skip flag is set, the skipped-steps counter advanced, the step counter and the other
//                       scalars left alone.  (torch.nn.utils.clip_grad_norm_ would multiply every gradient by a NaN coefficient
//                       and poison every parameter; here the step is dropped and counted.)
//   ctl_flat_kernel<rule>  one pass over the flat buffers; returns before touching anything when the skip flag is set.
//
// fp32 operation order per element, one rounding per line (ATen's foreach kernels: a multiply-add inside one kernel is fused):
//   every rule   g = clip_coef * g                       the gradient buffer itself is not rewritten
//   Adam + L2    adam_one (optimizer.hip)                g = fma(wd, p, g); m; v; den; p
//   AdamW        p = p * decay                           param.mul_(1 - lr * weight_decay)
//                adam_one with wd = 0
//   SGD          g = fma(wd, p, g)                       grad.add(param, alpha=weight_decay)       (wd != 0)
//                buf = buf * mu                          buf.mul_(momentum)                        (mu != 0; buf starts at 0, which
//                buf = buf + g                           buf.add_(grad)                             is torch's first-step buf = g)
//                d = fma(mu, buf, g)  |  d = buf         grad.add(buf, alpha=momentum) with nesterov
//                p = fma(-lr, d, p)                      param.add_(d, alpha=-lr)
// An element with zero gradient, zero state and zero value stays bit-unchanged under every rule (FlatParameters' padding).
#include <math.h>

#include "gnc_common.h"
#include "optimizer_rules.h"

namespace {

using gnc::f4;

constexpr int kSumBlocks = GNC_GRAD_NORM_BLOCKS;  // == the tick kernel's workgroup size: one thread per partial
constexpr int kSumThreads = 256;
static_assert((int64_t)kSumBlocks * kSumThreads * 4 == GNC_GRAD_NORM_PASS, "GNC_GRAD_NORM_PASS is one grid pass of float4 loads");
static_assert(kSumBlocks == 256 && kSumThreads == 256, "the LDS trees below halve from 128");

// sum over the workgroup in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double block_tree_sum(double v, double* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(kSumThreads) void grad_sumsq_kernel(const float* __restrict__ grad, int64_t n,
                                                                 double* __restrict__ partials) {
  __shared__ double sh[kSumThreads];
  const int64_t n4 = n >> 2;
  const int64_t first = (int64_t)blockIdx.x * kSumThreads + threadIdx.x;
  double acc = 0.0;
  for (int64_t i = first; i < n4; i += (int64_t)kSumBlocks * kSumThreads) {
    const f4 g = reinterpret_cast<const f4*>(grad)[i];
    const double x = g.x, y = g.y, z = g.z, w = g.w;
    acc += (x * x + y * y) + (z * z + w * w);
  }
  const int64_t i = (n4 << 2) + first;  // tail (n % 4 elements)
  if (i < n) {
    const double x = grad[i];
    acc += x * x;
  }
  const double total = block_tree_sum(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;  // every workgroup writes, also one with no element: nothing stale is summed
}

__device__ double lr_at(const gnc_opt_ctl_t& c, int64_t t) {
#pragma clang fp contract(off)
  if (t <= c.warmup_steps) return c.lr * ((double)t / (double)c.warmup_steps);  // exactly lr at t == warmup_steps
  if (c.schedule == GNC_LR_COSINE) {
    if (t >= c.total_steps) return c.min_lr;
    const double progress = (double)(t - c.warmup_steps) / (double)(c.total_steps - c.warmup_steps);
    return c.min_lr + 0.5 * (c.lr - c.min_lr) * (1.0 + cos(M_PI * progress));
  }
  if (c.schedule == GNC_LR_STEP) return c.lr * pow(c.gamma, (double)((t - c.warmup_steps) / c.every));
  return c.lr;
}

// Thread 0 of the tick, after the partials are summed: everything in double, every scalar rounded to fp32 once.
__device__ void tick_scalars(int64_t* __restrict__ step, float* __restrict__ scal, int64_t* __restrict__ skipped,
                             const gnc_opt_ctl_t& c, bool use_norm, double sum) {
#pragma clang fp contract(off)
  const double norm = sqrt(sum);
  scal[5] = use_norm ? (float)norm : __builtin_nanf("");
  const bool bad = use_norm && !(sum <= 1.7976931348623157e308);  // NaN or +inf (a sum of squares is never negative)
  skipped[1] = bad ? 1 : 0;
  if (bad) {
    skipped[0] += 1;
    return;
  }
  const int64_t t = *step + 1;
  *step = t;
  const double lr = lr_at(c, t);
  double coef = 1.0;
  if (c.clip) coef = fmin(1.0, c.max_grad_norm / (norm + 1e-6));
  double step_size = lr, bc2_sqrt = 1.0, decay = 1.0;
  if (c.rule != GNC_OPT_SGD) {
    step_size = lr / (1.0 - pow(c.beta1, (double)t));
    bc2_sqrt = sqrt(1.0 - pow(c.beta2, (double)t));
    if (c.rule == GNC_OPT_ADAMW) decay = 1.0 - lr * c.weight_decay;
  }
  scal[0] = (float)step_size;
  scal[1] = (float)bc2_sqrt;
  scal[2] = (float)decay;
  scal[3] = (float)coef;
  scal[4] = (float)lr;
}

// The hyper-parameters are constants of a run: passed by value, a capture bakes them in.  What changes from step to step is
// read from device memory (the counter, the partials).
__global__ __launch_bounds__(kSumBlocks) void ctl_tick_kernel(int64_t* __restrict__ step, const double* __restrict__ partials,
                                                              float* __restrict__ scal, int64_t* __restrict__ skipped,
                                                              gnc_opt_ctl_t c, int use_norm) {
  __shared__ double sh[kSumBlocks];
  double sum = 0.0;
  if (use_norm) sum = block_tree_sum(partials[threadIdx.x], sh);  // use_norm is uniform: every thread reaches the barriers
  if (threadIdx.x == 0) tick_scalars(step, scal, skipped, c, use_norm != 0, sum);
}

struct RuleConsts {
  float omb1, beta2, omb2, eps, wd, mu;
};

template <int RULE, bool NESTEROV>
__device__ __forceinline__ void rule_one(float& p, float g, float& a, float& b, float step_size, float bc2_sqrt, float decay,
                                         float coef, const RuleConsts& k) {
#pragma clang fp contract(off)  // the product is rounded on its own, never fused into the rule's first subtraction or sum
  g = coef * g;                // exact when the clip does not bite (coef == 1)
  if (RULE == GNC_OPT_ADAM) gnc::adam_one(p, g, a, b, step_size, bc2_sqrt, k.omb1, k.beta2, k.omb2, k.eps, k.wd);
  if (RULE == GNC_OPT_ADAMW) gnc::adamw_one(p, g, a, b, step_size, bc2_sqrt, k.omb1, k.beta2, k.omb2, k.eps, decay);
  if (RULE == GNC_OPT_SGD) gnc::sgd_one<NESTEROV>(p, g, a, step_size, k.mu, k.wd);
}

// state1: exp_avg (Adam, AdamW) or the momentum buffer (SGD; untouched, and may be null, when mu == 0); state2: exp_avg_sq (Adam, AdamW)
template <int RULE, bool NESTEROV>
__global__ __launch_bounds__(256) void ctl_flat_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                       float* __restrict__ state1, float* __restrict__ state2, int64_t n,
                                                       const float* __restrict__ scal, const int64_t* __restrict__ skipped,
                                                       RuleConsts k) {
  if (skipped[1] != 0) return;  // the tick found a non-finite gradient: nothing is touched
  constexpr bool kTwo = RULE != GNC_OPT_SGD;
  const bool one = kTwo || k.mu != 0.f;  // uniform
  const float step_size = scal[0], bc2_sqrt = scal[1], decay = scal[2], coef = scal[3];
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const f4 pv = reinterpret_cast<f4*>(param)[i], gv = reinterpret_cast<const f4*>(grad)[i];
    const f4 av = one ? reinterpret_cast<f4*>(state1)[i] : zero;
    f4 bv = zero;
    if (kTwo) bv = reinterpret_cast<f4*>(state2)[i];
    float pe[4] = {pv.x, pv.y, pv.z, pv.w}, ae[4] = {av.x, av.y, av.z, av.w}, be[4] = {bv.x, bv.y, bv.z, bv.w};
    const float ge[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) rule_one<RULE, NESTEROV>(pe[j], ge[j], ae[j], be[j], step_size, bc2_sqrt, decay, coef, k);
    const f4 p = {pe[0], pe[1], pe[2], pe[3]}, a = {ae[0], ae[1], ae[2], ae[3]}, b = {be[0], be[1], be[2], be[3]};
    reinterpret_cast<f4*>(param)[i] = p;
    if (one) reinterpret_cast<f4*>(state1)[i] = a;
    if (kTwo) reinterpret_cast<f4*>(state2)[i] = b;
  }
  // tail (n % 4 elements)
  const int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    float a = one ? state1[i] : 0.f, b = 0.f;
    if (kTwo) b = state2[i];
    rule_one<RULE, NESTEROV>(param[i], grad[i], a, b, step_size, bc2_sqrt, decay, coef, k);
    if (one) state1[i] = a;
    if (kTwo) state2[i] = b;
  }
}

int launch_sumsq(const float* grad, int64_t n, double* partials, hipStream_t stream) {
  grad_sumsq_kernel<<<dim3(kSumBlocks), kSumThreads, 0, stream>>>(grad, n, partials);
  return gnc::check_launch("grad_sumsq_kernel");
}

}  // namespace

extern "C" int32_t gnc_sizeof_opt_ctl(void) { return (int32_t)sizeof(gnc_opt_ctl_t); }
extern "C" int64_t gnc_grad_norm_pass(void) { return GNC_GRAD_NORM_PASS; }
extern "C" int32_t gnc_grad_norm_blocks(void) { return kSumBlocks; }

extern "C" int gnc_grad_sumsq_f32(const float* grad, int64_t n, double* partials, void* stream_) {
  GNC_REQUIRE(n >= 0, "gnc_grad_sumsq_f32: negative size");
  GNC_REQUIRE(partials && (grad || n == 0), "gnc_grad_sumsq_f32: null pointer");
  GNC_REQUIRE(gnc::aligned16(grad) && gnc::aligned_to(partials, 8), "gnc_grad_sumsq_f32: grad must be 16-B aligned, partials 8-B");
  return launch_sumsq(grad, n, partials, (hipStream_t)stream_);
}

extern "C" int gnc_optimizer_ctl_step_f32(float* param, const float* grad, float* state1, float* state2, int64_t n,
                                          const gnc_opt_ctl_t* ctl, int64_t* step, float* scalars, int64_t* skipped,
                                          double* partials, void* stream_) {
  const char* who = "gnc_optimizer_ctl_step_f32";
  GNC_REQUIRE(n >= 0, "%s: negative size", who);
  GNC_REQUIRE(ctl, "%s: null pointer", who);
  const gnc_opt_ctl_t c = *ctl;
  GNC_REQUIRE(c.rule >= GNC_OPT_ADAM && c.rule <= GNC_OPT_SGD && c.schedule >= GNC_LR_CONSTANT && c.schedule <= GNC_LR_STEP,
              "%s: unknown rule or schedule", who);
  const bool adam = c.rule != GNC_OPT_SGD;
  const bool use_norm = c.clip != 0 || c.check_nonfinite != 0;
  const bool need1 = adam || c.momentum != 0.0;
  // every comparison is written so that a NaN fails it
  bool ok = c.lr >= 0.0 && c.lr <= 3.0e38 && c.weight_decay >= 0.0 && c.weight_decay <= 3.0e38 && c.warmup_steps >= 0;
  if (c.clip) ok = ok && c.max_grad_norm > 0.0;
  if (c.schedule == GNC_LR_COSINE) ok = ok && c.total_steps > c.warmup_steps && c.min_lr >= 0.0 && c.min_lr <= c.lr;
  if (c.schedule == GNC_LR_STEP) ok = ok && c.every >= 1 && c.gamma > 0.0 && c.gamma <= 3.0e38;
  if (adam) {
    const float b1 = (float)c.beta1, b2 = (float)c.beta2;  // as gnc_adam_step_f32: the guards hold for the fp32 values too
    ok = ok && c.beta1 >= 0.0 && c.beta2 >= 0.0 && b1 >= 0.f && b1 < 1.f && b2 >= 0.f && b2 < 1.f && c.eps >= 0.0 && c.eps <= 3.0e38;
    if (c.rule == GNC_OPT_ADAMW) ok = ok && c.lr * c.weight_decay < 1.0;  // decay > 0: a padding zero keeps its sign
  } else {
    ok = ok && c.momentum >= 0.0 && c.momentum <= 3.0e38 && (!c.nesterov || c.momentum > 0.0);
  }
  GNC_REQUIRE(ok, "%s: hyper-parameters out of range", who);
  if (n == 0) return GNC_OK;
  GNC_REQUIRE(param && grad && step && scalars && skipped && (!need1 || state1) && (!adam || state2) && (!use_norm || partials),
              "%s: null pointer", who);
  GNC_REQUIRE(gnc::aligned16(param) && gnc::aligned16(grad) && (!need1 || gnc::aligned16(state1)) && (!adam || gnc::aligned16(state2)),
              "%s: flat buffers must be 16-B aligned", who);
  GNC_REQUIRE(gnc::aligned_to(step, 8) && gnc::aligned_to(skipped, 8) && gnc::aligned_to(partials, 8) && gnc::aligned_to(scalars, 4),
              "%s: misaligned control buffers", who);
  hipStream_t stream = (hipStream_t)stream_;
  int rc;
  if (use_norm && (rc = launch_sumsq(grad, n, partials, stream))) return rc;
  ctl_tick_kernel<<<1, kSumBlocks, 0, stream>>>(step, partials, scalars, skipped, c, use_norm ? 1 : 0);
  if ((rc = gnc::check_launch("ctl_tick_kernel"))) return rc;
  const RuleConsts k = {(float)(1.0 - c.beta1), (float)c.beta2, (float)(1.0 - c.beta2), (float)c.eps, (float)c.weight_decay,
                        (float)c.momentum};
  const dim3 grid((unsigned)gnc::capped_blocks(gnc::ceil_div(n, 4), 256));
  float* s1 = need1 ? state1 : nullptr;
  float* s2 = adam ? state2 : nullptr;
  if (c.rule == GNC_OPT_ADAM)
    ctl_flat_kernel<GNC_OPT_ADAM, false><<<grid, 256, 0, stream>>>(param, grad, s1, s2, n, scalars, skipped, k);
  else if (c.rule == GNC_OPT_ADAMW)
    ctl_flat_kernel<GNC_OPT_ADAMW, false><<<grid, 256, 0, stream>>>(param, grad, s1, s2, n, scalars, skipped, k);
  else if (c.nesterov)
    ctl_flat_kernel<GNC_OPT_SGD, true><<<grid, 256, 0, stream>>>(param, grad, s1, s2, n, scalars, skipped, k);
  else
    ctl_flat_kernel<GNC_OPT_SGD, false><<<grid, 256, 0, stream>>>(param, grad, s1, s2, n, scalars, skipped, k);
  return gnc::check_launch("ctl_flat_kernel");
}
