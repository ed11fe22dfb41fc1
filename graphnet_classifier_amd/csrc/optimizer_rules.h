// Per-element update rules of the flat optimizers, shared by optimizer.hip (Adam, K10) and optimizer_ctl.hip (K22).
// Every line of a rule is one fp32 rounding; the orders are written out in the headers of those two files.
#pragma once
#include <math.h>

#include "gnc_common.h"

namespace gnc {

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float step_size, float bc2_sqrt, float omb1,
                                         float beta2, float omb2, float eps, float wd) {
  // one rounding per ATen kernel of the foreach path (lerp_, mul_, addcmul_, sqrt, div_, add_, addcdiv_); the
  // multiply-adds inside one of those kernels are fused there too
  if (wd != 0.f) g = fmaf(wd, p, g);
  m = fmaf(omb1, g - m, m);
  v = fmaf(__fmul_rn(omb2, g), g, __fmul_rn(v, beta2));
  // sqrtf, not __fsqrt_rn: despite its name that one is the native v_sqrt_f32 (1 ulp) here, sqrtf is correctly rounded as ATen's is
  const float den = __fadd_rn(__fdiv_rn(sqrtf(v), bc2_sqrt), eps);
  p = fmaf(-step_size, __fdiv_rn(m, den), p);
}

// torch.optim.AdamW: param.mul_(1 - lr * weight_decay) with the factor formed in double and rounded once, then Adam without L2
__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, float step_size, float bc2_sqrt, float omb1,
                                          float beta2, float omb2, float eps, float decay) {
#pragma clang fp contract(off)
  p = p * decay;
  adam_one(p, g, m, v, step_size, bc2_sqrt, omb1, beta2, omb2, eps, 0.f);
}

// torch.optim.SGD (foreach, dampening 0, maximize off): add(param, alpha=wd) is one fused kernel, mul_(momentum) and add_(grad)
// are two, add(buf, alpha=momentum) and add_(d, alpha=-lr) one each.  `buf` is read and written only when mu != 0.
template <bool NESTEROV>
__device__ __forceinline__ void sgd_one(float& p, float g, float& buf, float lr, float mu, float wd) {
#pragma clang fp contract(off)
  if (wd != 0.f) g = fmaf(wd, p, g);
  float d = g;
  if (mu != 0.f) {
    const float scaled = buf * mu;
    buf = scaled + g;
    d = NESTEROV ? fmaf(mu, buf, g) : buf;
  }
  p = fmaf(-lr, d, p);
}

}  // namespace gnc
