// Batched RGB resize on the device: Pillow's `Image.resize((out_w, out_h), resample)` (libImaging/Resample.c) bit
// for bit, for BICUBIC, BILINEAR and BOX, over B uint8 [h_b, w_b, 3] images of any sizes to one output size.
// The rules and the three stages live in resize_device.h, which augment.hip shares for its crop boxes; this file is
// the whole-image entry point.
#include "resize_device.h"

extern "C" size_t gnc_resize_workspace_bytes(int32_t B, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                                             int32_t filter) {
  return gnc_resize::workspace_bytes(B, in_h, in_w, out_h, out_w, filter);
}

extern "C" int gnc_resize_rgb_u8(const uint8_t* src, const int64_t* table, int32_t B, int32_t in_h, int32_t in_w,
                                 int32_t out_h, int32_t out_w, int32_t filter, uint8_t* out, void* workspace,
                                 size_t workspace_bytes, void* stream_) {
  return gnc_resize::run<false>("gnc_resize_rgb_u8", src, table, nullptr, B, in_h, in_w, out_h, out_w, filter, out,
                                workspace, workspace_bytes, stream_);
}
