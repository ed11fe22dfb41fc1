// The three stages of the Pillow-exact batched RGB resize, shared by resize.hip (whole images) and augment.hip (a crop box and
// a horizontal flip per image).  Pillow's `Image.resize((out_w, out_h), resample)` (libImaging/Resample.c) bit for bit, for
// BICUBIC, BILINEAR and BOX, over B uint8 RGB images of any sizes to one output size.
//
// Pillow's rules, per axis (in = input length, out = output length):
//   scale = in / out, fs = max(scale, 1), support = filter_support * fs, ksize = ceil(support) * 2 + 1
//   output index xx: center = (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0),
//   n = min((int)(center + support + 0.5), in) - xmin, w_x = filter((x + xmin - center + 0.5) * (1 / fs)),
//   each w_x divided by their running double sum when it is not 0, then rounded half away from zero to int32 at
//   22 fraction bits.  A pass is acc = 2^21 + sum(pixel * k) in int32 and clamp(acc >> 22, 0, 255).
//   The horizontal pass runs only if the width changes and stores its result as uint8; the vertical pass runs over
//   that uint8 intermediate only if the height changes; with neither the output is a copy.
// Integer accumulation is exact (no partial sum leaves int32 for pixels <= 255 and these filters), so only the
// coefficients need Pillow's exact operation order: they are computed here in fp64 with FP contraction off.
//
// Stages (one launch each for the whole batch; stream-ordered, no host synchronisation, capture-safe):
//   resize_coeffs      one lane per (image, axis, output index): bounds and int32 coefficients into the workspace.
//   resize_horizontal  one workgroup per (image, band of kRows input rows): each row is staged into LDS with dword
//                      loads (rows up to kRowBytes; wider rows are read where they lie), then every lane produces
//                      output columns from LDS.  Writes the intermediate, or the output when the height is unchanged.
//   resize_vertical    one lane per output byte: the rows of a window are read with coalesced byte loads and every
//                      lane of a row shares one coefficient.  Also the plain copy when neither side changes.
//
// kBoxed = true is `Image.crop(box).resize(...)`: the "image" every stage sees is the box - its rows start 3 left bytes into
// the image's rows, top rows down, and keep the image's row pitch - so filter windows are clamped at the box.  A row of the
// box may start on any byte: the staging loop reads the aligned dwords that cover it (as it does for a mixed-size batch).
// A set flip flag mirrors the columns in the store of whichever pass writes the output, so a flip is no further launch.
#pragma once
#pragma clang fp contract(off)  // Pillow's coefficients are separate multiplies and adds: no FMA contraction

#include "gnc_common.h"

namespace gnc_resize {

constexpr size_t kAlign = 256;
inline size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

constexpr int kMaxSide = 65535;   // per input side; keeps every per-row index in int32
constexpr int kMaxBatch = 65535;  // grid.y
constexpr int kRows = 4;          // input rows per workgroup of the horizontal pass
constexpr int kRowBytes = 32768;  // LDS staging limit of one input row (10922 RGB pixels)

enum { kBilinear = 2, kBicubic = 3, kBox = 4 };  // PIL.Image.Resampling values

__host__ __device__ inline double support_of(int filter) {
  return filter == kBicubic ? 2.0 : filter == kBilinear ? 1.0 : 0.5;
}

// Pillow's ksize for one axis; also the row stride of that axis' coefficient table.  Monotone in `in`, so the
// stride computed from the batch's largest side holds every image's window (and every box's: a box lies in its image).
inline int64_t ksize_of(int in, int out, int filter) {
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  return (int64_t)ceil(support_of(filter) * fs) * 2 + 1;
}

struct Layout {
  int64_t kx, ky;            // coefficient row strides (ints)
  int64_t coef_stride;       // ints per image: [out_w][2] bounds, [out_w][kx], [out_h][2] bounds, [out_h][ky]
  int64_t inter_stride;      // bytes per image of the horizontal pass output (max_h rows of out_w pixels)
  size_t coef_bytes, total;  // workspace: B coefficient blocks, then B intermediates
};

inline Layout layout_of(int B, int in_h, int in_w, int out_h, int out_w, int filter) {
  Layout l;
  l.kx = ksize_of(in_w, out_w, filter);
  l.ky = ksize_of(in_h, out_h, filter);
  l.coef_stride = (int64_t)align_up((size_t)(out_w * (2 + l.kx) + out_h * (2 + l.ky)) * 4) / 4;
  l.inter_stride = (int64_t)align_up((size_t)in_h * out_w * 3);
  l.coef_bytes = (size_t)B * l.coef_stride * 4;
  l.total = l.coef_bytes + (size_t)B * l.inter_stride;
  return l;
}

struct Img {
  int64_t off;    // byte offset in src of the first pixel the stages read (the image's, or its box's)
  int h, w;       // rows and columns the stages resize
  int64_t pitch;  // bytes from one row to the next (3 x the IMAGE's width)
  bool flip;      // mirror the output's columns
};

// table == nullptr: a dense [B, in_h, in_w, 3] batch.  Otherwise int64 rows (offset, h, w) with h <= in_h, w <= in_w;
// an entry outside that is skipped (its output left as it was) rather than read or written out of bounds.
// kBoxed: `boxes` holds int64 rows (left, top, right, bottom, flip); a box that is empty or leaves its image is skipped too.
template <bool kBoxed>
__device__ inline bool image_of(const int64_t* table, const int64_t* boxes, int b, int in_h, int in_w, Img& m) {
  if (!table) {
    m = {(int64_t)b * in_h * in_w * 3, in_h, in_w, (int64_t)in_w * 3, false};
  } else {
    const int64_t off = table[3 * b], h = table[3 * b + 1], w = table[3 * b + 2];
    m = {off, (int)h, (int)w, w * 3, false};
    if (!(off >= 0 && h >= 1 && w >= 1 && h <= in_h && w <= in_w)) return false;
  }
  if (kBoxed) {
    const int64_t left = boxes[5 * b], top = boxes[5 * b + 1], right = boxes[5 * b + 2], bottom = boxes[5 * b + 3];
    if (!(left >= 0 && top >= 0 && left < right && top < bottom && right <= m.w && bottom <= m.h)) return false;
    m.off += top * m.pitch + left * 3;
    m.h = (int)(bottom - top);
    m.w = (int)(right - left);
    m.flip = boxes[5 * b + 4] != 0;
  }
  return true;
}

__device__ inline double filter_at(int filter, double x) {
  if (filter == kBicubic) {  // Resample.c bicubic_filter, a = -0.5
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
  }
  if (filter == kBilinear) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
  }
  return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;  // box
}

__device__ inline uint8_t clip8(int acc) {
  const int v = acc >> 22;  // arithmetic shift, as Pillow's clip8
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

template <bool kBoxed>
__global__ void resize_coeffs(const int64_t* __restrict__ table, const int64_t* __restrict__ boxes, int in_h, int in_w,
                              int out_h, int out_w, int filter, int64_t kx, int64_t ky, int64_t coef_stride,
                              int32_t* __restrict__ coef) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  Img m;
  if (i >= out_w + out_h || !image_of<kBoxed>(table, boxes, b, in_h, in_w, m)) return;
  const bool horiz = i < out_w;
  const int in = horiz ? m.w : m.h, out = horiz ? out_w : out_h, xx = horiz ? i : i - out_w;
  if (in == out) return;  // that pass does not run
  int32_t* base = coef + (int64_t)b * coef_stride + (horiz ? 0 : out_w * (2 + kx));
  int32_t* bounds = base + 2 * xx;
  int32_t* k = base + 2 * (int64_t)out + xx * (horiz ? kx : ky);
  const int64_t kcap = horiz ? kx : ky;

  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = support_of(filter) * fs;
  const double center = (xx + 0.5) * scale;
  const double ss = 1.0 / fs;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int n = (int)(center + support + 0.5);
  if (n > in) n = in;
  n -= xmin;
  if (n > kcap) n = (int)kcap;  // cannot happen (ksize bounds the window); keeps the writes inside the row
  double ww = 0.0;
  for (int x = 0; x < n; ++x) ww += filter_at(filter, (x + xmin - center + 0.5) * ss);
  for (int x = 0; x < n; ++x) {
    double w = filter_at(filter, (x + xmin - center + 0.5) * ss);
    if (ww != 0.0) w /= ww;
    k[x] = w < 0 ? (int)(-0.5 + w * (1 << 22)) : (int)(0.5 + w * (1 << 22));
  }
  bounds[0] = xmin;
  bounds[1] = n;
}

template <bool kBoxed>
__global__ void __launch_bounds__(256) resize_horizontal(const uint8_t* __restrict__ src, const int64_t* __restrict__ table,
                                                         const int64_t* __restrict__ boxes, int in_h, int in_w, int out_h,
                                                         int out_w, int64_t kx, int64_t coef_stride,
                                                         const int32_t* __restrict__ coef, int64_t inter_stride,
                                                         uint8_t* __restrict__ inter, uint8_t* __restrict__ out) {
  __shared__ uint32_t stage[kRowBytes / 4 + 1];
  const int b = blockIdx.y;
  Img m;
  if (!image_of<kBoxed>(table, boxes, b, in_h, in_w, m) || m.w == out_w) return;
  const int y0 = blockIdx.x * kRows;
  if (y0 >= m.h) return;
  const int32_t* bounds = coef + (int64_t)b * coef_stride;
  const int32_t* kk = bounds + 2 * out_w;
  const bool last = m.h == out_h;  // no vertical pass follows: this one writes the output
  uint8_t* dst = last ? out + (int64_t)b * out_h * out_w * 3 : inter + (int64_t)b * inter_stride;
  const bool mirror = kBoxed && last && m.flip;
  const int row_bytes = m.w * 3;
  const bool staged = row_bytes <= kRowBytes;
  for (int y = y0; y < y0 + kRows && y < m.h; ++y) {
    const uint8_t* grow = src + m.off + (int64_t)y * m.pitch;
    const uint8_t* row = grow;
    if (staged) {
      // aligned dwords covering the row: the first and last may hold bytes of the neighbours, never bytes past the
      // dword that holds the row's last byte
      const uintptr_t a0 = reinterpret_cast<uintptr_t>(grow) & ~uintptr_t(3);
      const int head = (int)(reinterpret_cast<uintptr_t>(grow) - a0);
      const int words = (head + row_bytes + 3) / 4;
      const uint32_t* gw = reinterpret_cast<const uint32_t*>(a0);
      __syncthreads();  // the previous row's readers are done
      for (int i = threadIdx.x; i < words; i += blockDim.x) stage[i] = gw[i];
      __syncthreads();
      row = reinterpret_cast<const uint8_t*>(stage) + head;
    }
    uint8_t* drow = dst + (int64_t)y * out_w * 3;
    for (int xx = threadIdx.x; xx < out_w; xx += blockDim.x) {
      const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
      const int32_t* k = kk + xx * kx;
      const uint8_t* p = row + xmin * 3;
      int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
      for (int x = 0; x < n; ++x) {
        const int c = k[x];
        s0 += p[3 * x] * c;
        s1 += p[3 * x + 1] * c;
        s2 += p[3 * x + 2] * c;
      }
      uint8_t* d = drow + 3 * (mirror ? out_w - 1 - xx : xx);
      d[0] = clip8(s0);
      d[1] = clip8(s1);
      d[2] = clip8(s2);
    }
  }
}

template <bool kBoxed>
__global__ void __launch_bounds__(256) resize_vertical(const uint8_t* __restrict__ src, const int64_t* __restrict__ table,
                                                       const int64_t* __restrict__ boxes, int in_h, int in_w, int out_h,
                                                       int out_w, int64_t kx, int64_t ky, int64_t coef_stride,
                                                       const int32_t* __restrict__ coef, int64_t inter_stride,
                                                       const uint8_t* __restrict__ inter, uint8_t* __restrict__ out) {
  const int b = blockIdx.y;
  const int64_t row_bytes = (int64_t)out_w * 3;
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  Img m;
  if (j >= out_h * row_bytes || !image_of<kBoxed>(table, boxes, b, in_h, in_w, m)) return;
  if (m.h == out_h && m.w != out_w) return;  // the horizontal pass wrote the output
  const int yy = (int)(j / row_bytes);
  const int64_t col = j - (int64_t)yy * row_bytes;
  // lane j produces the byte that belongs at column `col` of row yy, and stores it at the mirrored pixel under a flip
  int64_t at = j;
  if (kBoxed && m.flip) {
    const int64_t px = col / 3;
    at = (int64_t)yy * row_bytes + (out_w - 1 - px) * 3 + (col - px * 3);
  }
  uint8_t* o = out + (int64_t)b * out_h * row_bytes + at;
  if (m.h == out_h) {  // neither side changes: a copy
    *o = src[m.off + (int64_t)yy * m.pitch + col];
    return;
  }
  // the vertical pass reads the intermediate, or the source itself when the width is unchanged
  const bool from_src = m.w == out_w;
  const uint8_t* base = from_src ? src + m.off : inter + (int64_t)b * inter_stride;
  const int64_t pitch = from_src ? m.pitch : row_bytes;
  const int32_t* bounds = coef + (int64_t)b * coef_stride + out_w * (2 + kx);
  const int ymin = bounds[2 * yy], n = bounds[2 * yy + 1];
  const int32_t* k = bounds + 2 * out_h + yy * ky;
  const uint8_t* p = base + (int64_t)ymin * pitch + col;
  int s = 1 << 21;
  for (int y = 0; y < n; ++y) s += p[y * pitch] * k[y];
  *o = clip8(s);
}

inline bool supported_filter(int f) { return f == kBilinear || f == kBicubic || f == kBox; }

inline size_t workspace_bytes(int32_t B, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w, int32_t filter) {
  if (B < 1 || B > kMaxBatch || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1 || in_h > kMaxSide ||
      in_w > kMaxSide || out_h > kMaxSide || out_w > kMaxSide || !supported_filter(filter))
    return 0;
  return layout_of(B, in_h, in_w, out_h, out_w, filter).total;
}

// The argument checks and the three launches of gnc_resize_rgb_u8 (kBoxed = false, boxes unused) and of
// gnc_crop_resize_rgb_u8 (kBoxed = true); `who` names the entry point in error messages.
template <bool kBoxed>
inline int run(const char* who, const uint8_t* src, const int64_t* table, const int64_t* boxes, int32_t B, int32_t in_h,
               int32_t in_w, int32_t out_h, int32_t out_w, int32_t filter, uint8_t* out, void* workspace,
               size_t workspace_bytes, void* stream_) {
  GNC_REQUIRE(src && out && workspace && (!kBoxed || boxes), "%s: null pointer", who);
  GNC_REQUIRE(B >= 1 && in_h >= 1 && in_w >= 1 && out_h >= 1 && out_w >= 1,
              "%s: empty batch or image (B %d, %d x %d -> %d x %d)", who, B, in_h, in_w, out_h, out_w);
  if (!supported_filter(filter)) {
    gnc::set_error("%s: filter %d not supported (BILINEAR 2, BICUBIC 3, BOX 4)", who, filter);
    return GNC_ERR_UNSUPPORTED;
  }
  if (B > kMaxBatch || in_h > kMaxSide || in_w > kMaxSide || out_h > kMaxSide || out_w > kMaxSide) {
    gnc::set_error("%s: B or a side outside the supported set (B <= %d, sides <= %d)", who, kMaxBatch, kMaxSide);
    return GNC_ERR_UNSUPPORTED;
  }
  const Layout l = layout_of(B, in_h, in_w, out_h, out_w, filter);
  if (l.total > workspace_bytes) {
    gnc::set_error("%s: workspace too small", who);
    return GNC_ERR_WORKSPACE;
  }
  if ((int64_t)out_h * out_w * 3 > INT32_MAX) {
    gnc::set_error("%s: output image of %d x %d is too large", who, out_h, out_w);
    return GNC_ERR_UNSUPPORTED;
  }
  hipStream_t stream = (hipStream_t)stream_;
  int32_t* coef = static_cast<int32_t*>(workspace);
  uint8_t* inter = static_cast<uint8_t*>(workspace) + l.coef_bytes;
  int rc;
  const dim3 cgrid((unsigned)gnc::ceil_div(out_w + out_h, gnc::kBlock), (unsigned)B);
  resize_coeffs<kBoxed><<<cgrid, gnc::kBlock, 0, stream>>>(table, boxes, in_h, in_w, out_h, out_w, filter, l.kx, l.ky,
                                                           l.coef_stride, coef);
  if ((rc = gnc::check_launch("resize_coeffs"))) return rc;
  const dim3 hgrid((unsigned)gnc::ceil_div(in_h, kRows), (unsigned)B);
  resize_horizontal<kBoxed><<<hgrid, gnc::kBlock, 0, stream>>>(src, table, boxes, in_h, in_w, out_h, out_w, l.kx,
                                                               l.coef_stride, coef, l.inter_stride, inter, out);
  if ((rc = gnc::check_launch("resize_horizontal"))) return rc;
  const dim3 vgrid((unsigned)gnc::ceil_div((int64_t)out_h * out_w * 3, gnc::kBlock), (unsigned)B);
  resize_vertical<kBoxed><<<vgrid, gnc::kBlock, 0, stream>>>(src, table, boxes, in_h, in_w, out_h, out_w, l.kx, l.ky,
                                                             l.coef_stride, coef, l.inter_stride, inter, out);
  return gnc::check_launch("resize_vertical");
}

}  // namespace gnc_resize
