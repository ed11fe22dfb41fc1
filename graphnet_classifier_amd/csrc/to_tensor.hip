// torchvision's ToTensor for a batch of uint8 images already on the device (main.py:13-18 of the reference, after the resize of
// csrc/resize.hip): out[b, c, y, x] = float(img[b, y, x, c]) / 255, a correctly rounded division, so that the result equals
// `t.permute(2, 0, 1).float().div(255)` bit for bit (a multiplication by 1 / 255 does not).  One pass, a thread per output element:
// the writes are contiguous, the byte reads of a wave stay within 64 * C bytes.
#include "gnc_common.h"

namespace {

__global__ __launch_bounds__(gnc::kBlock) void u8_hwc_to_f32_chw_kernel(const uint8_t* __restrict__ img, int64_t hw, int C,
                                                                        float* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * gnc::kBlock + threadIdx.x;  // pixel of the image
  const int c = blockIdx.y;
  const int64_t b = blockIdx.z;
  if (p >= hw) return;
  out[(b * C + c) * hw + p] = __fdiv_rn((float)img[(b * hw + p) * C + c], 255.f);
}

}  // namespace

extern "C" int gnc_u8_hwc_to_f32_chw(const uint8_t* img, int32_t B, int32_t H, int32_t W, int32_t C, float* out, void* stream) {
  GNC_REQUIRE(B >= 0 && H >= 0 && W >= 0 && C >= 0, "gnc_u8_hwc_to_f32_chw: negative size");
  if (B == 0 || H == 0 || W == 0 || C == 0) return GNC_OK;
  GNC_REQUIRE(img && out, "gnc_u8_hwc_to_f32_chw: null pointer");
  if (B > 65535 || C > 65535) {
    gnc::set_error("gnc_u8_hwc_to_f32_chw: batch or channel count above 65535");
    return GNC_ERR_UNSUPPORTED;
  }
  const int64_t hw = (int64_t)H * W;
  const dim3 grid((unsigned)gnc::ceil_div(hw, gnc::kBlock), (unsigned)C, (unsigned)B);
  u8_hwc_to_f32_chw_kernel<<<grid, gnc::kBlock, 0, (hipStream_t)stream>>>(img, hw, C, out);
  return gnc::check_launch("u8_hwc_to_f32_chw_kernel");
}
