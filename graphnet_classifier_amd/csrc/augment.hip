// Train-time image augmentation on the device (K25), pinned to Pillow byte for byte.
//
// gnc_crop_resize_rgb_u8   `Image.crop(box).resize((out_w, out_h), filter)` and an optional FLIP_LEFT_RIGHT per image: the three
//                          stages of resize_device.h run over each image's box (filter windows clamp at the box, as a crop
//                          followed by a resize does - not `Image.resize(box=...)`, which reads outside it); the flip is folded
//                          into the store of the pass that writes the output.
// gnc_color_jitter_rgb_u8  up to three `ImageEnhance` operations per image, in the image's own order, in place on a dense
//                          [B, H, W, 3] batch.  Every operation is Pillow's `Image.blend(degenerate, image, f)`:
//                            v = (float)d + f * (float)(p - d) in float32 with the multiply and the add rounded separately
//                            (Blend.c is compiled without FMA contraction; nor may this file be), byte = v <= 0 ? 0 : v >= 255 ? 255 : (uint8)v
//                            (for f in [0, 1] v never leaves [0, 255], so Pillow's unclamped branch is the same function);
//                            Brightness: d = 0.  Color: d = L of the pixel, L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16.
//                            Contrast: d = int(mean(L) + 0.5) over the image as it is when contrast is applied
//                            = (2 sum(L) + n) / (2 n) in integers, the sum exact in 64 bits.
//                          Only contrast needs the whole image, and at most once per chain.  So one workgroup of 1024 lanes takes
//                          one image: it applies the operations in front of the contrast per pixel while it sums L, reduces the
//                          sum (wave shuffles, then one LDS slot per wave - no atomics), and applies the contrast and what follows
//                          it.  An image of up to kResident pixels (128 x 128: 48 KB) waits in the LDS between the two halves; a
//                          larger one is read a second time from memory (the first half writes nothing, so the second half sees
//                          the input).  A chain without contrast is one pass without a barrier.
//                          A factor of exactly 1 is the identity of blend and is skipped like a missing operation.
#include "resize_device.h"

namespace {

constexpr int kJitterBlock = 1024;    // 16 waves: one workgroup per image
constexpr int kResident = 128 * 128;  // pixels of an image that is staged in the LDS (48 KB)

enum { kBrightness = 0, kContrast = 1, kColor = 2 };

__device__ inline int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__device__ inline int blend(int d, int p, float f) {
  // plain operators under this file's `fp contract(off)` (resize_device.h): two roundings.  HIP's __fmul_rn / __fadd_rn are
  // `x * y` and `x + y` compiled where contraction is on, and fuse into one FMA once inlined - not Pillow's result.
  const float prod = f * (float)(p - d);
  const float v = (float)d + prod;
  return v <= 0.0f ? 0 : v >= 255.0f ? 255 : (int)v;
}

// operation `op` with factor f on one pixel; `mean` is the contrast's degenerate value
__device__ inline void apply(int op, float f, int mean, int& r, int& g, int& b) {
  const int d = op == kBrightness ? 0 : op == kContrast ? mean : luma(r, g, b);
  r = blend(d, r, f);
  g = blend(d, g, f);
  b = blend(d, b, f);
}

// The image's chain in three slots, in the order they run; a slot whose op is -1 does nothing.  Plain scalars, uniform over the
// workgroup, so that the chain lives in SGPRs and every test on it is a scalar branch.
struct Chain {
  int op0, op1, op2;
  float f0, f1, f2;
  int pivot;  // slot of the contrast, or 3 when there is none
  bool any;
};

// order [B, 3]: operation codes in the order they run; an entry outside 0..2, or a second occurrence, is no operation.
__device__ inline void slot_of(const int32_t* order, const float* factor, int b, int s, unsigned& seen, int& op, float& f) {
  op = order[3 * b + s];
  f = 1.0f;
  if (op < 0 || op > 2 || (seen >> op & 1)) {
    op = -1;
    return;
  }
  seen |= 1u << op;
  f = factor[3 * b + op];
  if (f == 1.0f) op = -1;  // blend(d, p, 1) = p
}

__device__ inline Chain chain_of(const int32_t* order, const float* factor, int b) {
  Chain c;
  unsigned seen = 0;
  slot_of(order, factor, b, 0, seen, c.op0, c.f0);
  slot_of(order, factor, b, 1, seen, c.op1, c.f1);
  slot_of(order, factor, b, 2, seen, c.op2, c.f2);
  c.pivot = c.op0 == kContrast ? 0 : c.op1 == kContrast ? 1 : c.op2 == kContrast ? 2 : 3;
  c.any = (c.op0 & c.op1 & c.op2) >= 0;  // not all three are -1
  return c;
}

// slots [from, to) of the chain on one pixel
__device__ inline void run_chain(const Chain& c, int from, int to, int mean, int& r, int& g, int& b) {
  if (c.op0 >= 0 && from <= 0 && 0 < to) apply(c.op0, c.f0, mean, r, g, b);
  if (c.op1 >= 0 && from <= 1 && 1 < to) apply(c.op1, c.f1, mean, r, g, b);
  if (c.op2 >= 0 && from <= 2 && 2 < to) apply(c.op2, c.f2, mean, r, g, b);
}

__device__ inline void load_px(const uint8_t* p, int& r, int& g, int& b) { r = p[0], g = p[1], b = p[2]; }
__device__ inline void store_px(uint8_t* p, int r, int g, int b) {
  p[0] = (uint8_t)r, p[1] = (uint8_t)g, p[2] = (uint8_t)b;
}

// sum over the workgroup, returned to every lane
__device__ inline unsigned long long block_sum(unsigned long long v) {
  __shared__ unsigned long long part[kJitterBlock / gnc::kWave];
  for (int o = gnc::kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, gnc::kWave);
  if ((threadIdx.x & (gnc::kWave - 1)) == 0) part[threadIdx.x / gnc::kWave] = v;
  __syncthreads();
  unsigned long long s = 0;
  for (int w = 0; w < kJitterBlock / gnc::kWave; ++w) s += part[w];
  return s;
}

template <bool kStaged>
__global__ void __launch_bounds__(kJitterBlock) color_jitter(uint8_t* __restrict__ img, int64_t npix,
                                                             const int32_t* __restrict__ order,
                                                             const float* __restrict__ factor) {
  const int b = blockIdx.x;
  const Chain c = chain_of(order, factor, b);  // uniform over the workgroup
  if (!c.any) return;
  uint8_t* base = img + (int64_t)b * npix * 3;
  const bool contrast = c.pivot < 3;
  int mean = 0;
  if (kStaged) {
    __shared__ uint8_t px[kResident * 3];
    unsigned long long sum = 0;
    for (int i = threadIdx.x; i < (int)npix; i += kJitterBlock) {
      int r, g, bl;
      load_px(base + 3 * i, r, g, bl);
      run_chain(c, 0, c.pivot, 0, r, g, bl);
      if (contrast) sum += (unsigned)luma(r, g, bl);
      store_px(px + 3 * i, r, g, bl);
    }
    if (contrast) {
      const unsigned long long total = block_sum(sum);
      mean = (int)((2 * total + (unsigned long long)npix) / (2 * (unsigned long long)npix));
    }
    // every lane reads back the pixels it wrote itself, so the staging needs no barrier of its own
    for (int i = threadIdx.x; i < (int)npix; i += kJitterBlock) {
      int r, g, bl;
      load_px(px + 3 * i, r, g, bl);
      run_chain(c, c.pivot, 3, mean, r, g, bl);
      store_px(base + 3 * i, r, g, bl);
    }
    return;
  }
  if (contrast) {  // first half: nothing is written, so the second half reads the input again
    unsigned long long sum = 0;
    for (int64_t i = threadIdx.x; i < npix; i += kJitterBlock) {
      int r, g, bl;
      load_px(base + 3 * i, r, g, bl);
      run_chain(c, 0, c.pivot, 0, r, g, bl);
      sum += (unsigned)luma(r, g, bl);
    }
    const unsigned long long total = block_sum(sum);  // its barrier also orders every read above before the writes below
    mean = (int)((2 * total + (unsigned long long)npix) / (2 * (unsigned long long)npix));
  }
  for (int64_t i = threadIdx.x; i < npix; i += kJitterBlock) {
    int r, g, bl;
    load_px(base + 3 * i, r, g, bl);
    run_chain(c, 0, 3, mean, r, g, bl);
    store_px(base + 3 * i, r, g, bl);
  }
}

}  // namespace

extern "C" size_t gnc_crop_resize_workspace_bytes(int32_t B, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                                                  int32_t filter) {
  return gnc_resize::workspace_bytes(B, in_h, in_w, out_h, out_w, filter);
}

extern "C" int gnc_crop_resize_rgb_u8(const uint8_t* src, const int64_t* table, const int64_t* boxes, int32_t B, int32_t in_h,
                                      int32_t in_w, int32_t out_h, int32_t out_w, int32_t filter, uint8_t* out, void* workspace,
                                      size_t workspace_bytes, void* stream_) {
  return gnc_resize::run<true>("gnc_crop_resize_rgb_u8", src, table, boxes, B, in_h, in_w, out_h, out_w, filter, out, workspace,
                               workspace_bytes, stream_);
}

extern "C" int64_t gnc_color_jitter_resident_pixels(void) { return kResident; }

extern "C" int gnc_color_jitter_rgb_u8(uint8_t* img, int32_t B, int32_t H, int32_t W, const int32_t* order, const float* factor,
                                       void* stream_) {
  GNC_REQUIRE(img && order && factor, "gnc_color_jitter_rgb_u8: null pointer");
  GNC_REQUIRE(B >= 1 && H >= 1 && W >= 1, "gnc_color_jitter_rgb_u8: empty batch or image (B %d, %d x %d)", B, H, W);
  if (H > gnc_resize::kMaxSide || W > gnc_resize::kMaxSide) {
    gnc::set_error("gnc_color_jitter_rgb_u8: a side outside the supported set (sides <= %d)", gnc_resize::kMaxSide);
    return GNC_ERR_UNSUPPORTED;
  }
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t npix = (int64_t)H * W;
  if (npix <= kResident)
    color_jitter<true><<<(unsigned)B, kJitterBlock, 0, stream>>>(img, npix, order, factor);
  else
    color_jitter<false><<<(unsigned)B, kJitterBlock, 0, stream>>>(img, npix, order, factor);
  return gnc::check_launch("color_jitter");
}
