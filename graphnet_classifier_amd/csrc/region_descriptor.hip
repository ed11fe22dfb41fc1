// Region descriptors: B label images of one size -> GNC_REGION_DESCRIPTOR_DIM float32 columns per region, ONE launch (K26).
//
// The kernel has the shape of rag_batched.hip and numbers the regions as it does, so row i here is node i there:
//
//   1. presence bitmap over the labels [0, H*W) and a popcount prefix per word: the dense index of label l is
//      prefix[l / 32] + popc(bitmap[l / 32] below bit l % 32) (labels may have gaps);
//   2. every thread walks a run of consecutive pixels and keeps the current label's partial sums in registers - pixel
//      count, colour sums and sums of squares, first and second moments of the row / column index, bounding box,
//      boundary pixels, inner pixel pairs and their absolute colour differences - flushed with integer LDS atomics
//      (add, min, max; 64-bit add for the two second moments) when the label changes;
//   3. a thread per region turns the integers into the 16 columns in double precision, every expression written as
//      the reference of the tests writes it (tests/region_descriptor_reference.py), and stores the row as four 16-byte
//      stores.
//
// Widths for H*W <= 65536: every 32-bit sum stays below 2^32 (sum of squares of one channel <= 65025 * 65536, a moment
// sum <= 65535 * 65536 / 2, absolute differences <= 255 * 2 * 65536); the sums of y^2 and x^2 pass 2^32 (a 1 x 2400 row
// does) and are 64 bits wide, n * Syy < 65536 * 65536 * 65535^2 / 3 < 2^64.  Only integer atomics: the result does not
// depend on the order in which threads run, and an image has the same bits alone and inside a batch.  Rows behind the
// region count are zeros; an image with a label outside [0, H*W) or with more regions than node_capacity sets its own
// flag and leaves its slice all zeros.
#include "gnc_common.h"

namespace {

constexpr int kThreads = 1024;                 // one workgroup per image, 16 waves
constexpr int kWaves = kThreads / gnc::kWave;
constexpr int kMaxPixels = 256 * 256;          // labels lie in [0, H*W): the presence bitmap has one bit per label
constexpr int kBitmapWords = kMaxPixels / 32;  // 2048
constexpr int kMaxNodes = 512;
constexpr int kDim = GNC_REGION_DESCRIPTOR_DIM;
constexpr size_t kWorkspaceBytes = 256;        // nothing is staged in HBM; the query doubles as the supported-set check
static_assert(kDim == 16, "a row leaves as four 16-byte stores");

// 32-bit accumulators of a region, field-major in LDS (neighbouring regions in neighbouring banks)
enum Field : int {
  kN = 0, kSr, kSg, kSb, kQr, kQg, kQb, kSy, kSx, kYmin, kYmax, kXmin, kXmax, kNb, kM, kTr, kTg, kTb, kFields
};

// Exclusive prefix of one value per thread over the workgroup; *total receives the sum.  `scratch` holds kWaves words.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* scratch, uint32_t* total) {
  const int lane = threadIdx.x & (gnc::kWave - 1), wave = threadIdx.x / gnc::kWave;
  uint32_t inc = v;
  for (int d = 1; d < gnc::kWave; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d, gnc::kWave);
    if (lane >= d) inc += up;
  }
  __syncthreads();  // the previous use of scratch has been read
  if (lane == gnc::kWave - 1) scratch[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int w = 0; w < kWaves; ++w) {
    const uint32_t t = scratch[w];
    if (w < wave) before += t;
    all += t;
  }
  *total = all;
  return before + inc - v;
}

__device__ __forceinline__ uint32_t absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

__global__ __launch_bounds__(kThreads) void region_descriptor_kernel(
    const int32_t* __restrict__ labels_all, const uint8_t* __restrict__ img_all, int H, int W, int node_capacity,
    float* __restrict__ out_all, int32_t* __restrict__ counts_all) {
  __shared__ uint32_t bitmap[kBitmapWords];               // 8 KB  label l occurs
  __shared__ uint32_t prefix[kBitmapWords];               // 8 KB  labels present below word w
  __shared__ uint32_t acc[kFields * kMaxNodes];           // 36 KB
  __shared__ unsigned long long acc64[2 * kMaxNodes];     // 8 KB  sum of y^2, sum of x^2
  __shared__ uint32_t scratch[kWaves];
  __shared__ uint32_t bad_flag;

  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = H * W;
  const int32_t* __restrict__ labels = labels_all + (size_t)b * n;
  const uint8_t* __restrict__ img = img_all + (size_t)b * n * 3;
  float* __restrict__ out = out_all + (size_t)b * node_capacity * kDim;
  int32_t* __restrict__ counts = counts_all + 3 * b;

  const int words = (n + 31) / 32;
  for (int i = tid; i < words; i += kThreads) bitmap[i] = 0;
  for (int i = tid; i < kFields * kMaxNodes; i += kThreads) {
    const int f = i / kMaxNodes;
    acc[i] = (f == kYmin || f == kXmin) ? 0xffffffffu : 0u;
  }
  for (int i = tid; i < 2 * kMaxNodes; i += kThreads) acc64[i] = 0;
  if (tid == 0) bad_flag = 0;
  __syncthreads();

  // ---- 1. which labels occur
  const int chunk = (n + kThreads - 1) / kThreads;  // consecutive pixels per thread
  const int p0 = min(tid * chunk, n), p1 = min(p0 + chunk, n);
  {
    bool bad = false;
    int32_t last = -1;
    for (int p = p0; p < p1; ++p) {
      const int32_t l = labels[p];
      if (l < 0 || l >= n) { bad = true; continue; }
      if (l == last) continue;
      last = l;
      const uint32_t bit = 1u << (l & 31);
      if (!(bitmap[l >> 5] & bit)) atomicOr(&bitmap[l >> 5], bit);
    }
    if (bad) bad_flag = 1;  // every writer stores the same value
  }
  __syncthreads();
  uint32_t S;
  {
    const int w0 = 2 * tid, w1 = 2 * tid + 1;  // 2 * kThreads == kBitmapWords
    const uint32_t c0 = w0 < words ? __popc(bitmap[w0]) : 0, c1 = w1 < words ? __popc(bitmap[w1]) : 0;
    const uint32_t ex = block_exclusive_scan(c0 + c1, scratch, &S);
    if (w0 < words) prefix[w0] = ex;
    if (w1 < words) prefix[w1] = ex + c0;
  }
  __syncthreads();
  auto rank_of = [&](int32_t l) -> uint32_t { return prefix[l >> 5] + __popc(bitmap[l >> 5] & ((1u << (l & 31)) - 1u)); };

  const bool bad_image = bad_flag != 0;
  const bool overflow = S > (uint32_t)node_capacity;  // node_capacity <= kMaxNodes: what is accumulated fits the LDS arrays
  const bool active = !bad_image && !overflow;        // every label is in range from here on
  if (active) {
    // ---- 2. the sums of the current label in registers, flushed when the label changes
    int32_t cur = -1;
    uint32_t s = 0, cnt = 0, sr = 0, sg = 0, sb = 0, qr = 0, qg = 0, qb = 0, ys = 0, xs = 0;
    uint32_t ymin = 0xffffffffu, ymax = 0, xmin = 0xffffffffu, xmax = 0, nb = 0, m = 0, tr = 0, tg = 0, tb = 0;
    unsigned long long yy = 0, xx = 0;
    auto flush = [&]() {
      if (cnt) {
        uint32_t* a = acc + s;
        atomicAdd(a + kN * kMaxNodes, cnt);
        atomicAdd(a + kSr * kMaxNodes, sr); atomicAdd(a + kSg * kMaxNodes, sg); atomicAdd(a + kSb * kMaxNodes, sb);
        atomicAdd(a + kQr * kMaxNodes, qr); atomicAdd(a + kQg * kMaxNodes, qg); atomicAdd(a + kQb * kMaxNodes, qb);
        atomicAdd(a + kSy * kMaxNodes, ys); atomicAdd(a + kSx * kMaxNodes, xs);
        atomicMin(a + kYmin * kMaxNodes, ymin); atomicMax(a + kYmax * kMaxNodes, ymax);
        atomicMin(a + kXmin * kMaxNodes, xmin); atomicMax(a + kXmax * kMaxNodes, xmax);
        if (nb) atomicAdd(a + kNb * kMaxNodes, nb);
        if (m) {
          atomicAdd(a + kM * kMaxNodes, m);
          atomicAdd(a + kTr * kMaxNodes, tr); atomicAdd(a + kTg * kMaxNodes, tg); atomicAdd(a + kTb * kMaxNodes, tb);
        }
        atomicAdd(&acc64[s], yy); atomicAdd(&acc64[kMaxNodes + s], xx);
      }
      cnt = sr = sg = sb = qr = qg = qb = ys = xs = 0;
      ymin = xmin = 0xffffffffu; ymax = xmax = 0;
      nb = m = tr = tg = tb = 0;
      yy = xx = 0;
    };
    int row = p0 / W, col = p0 - row * W;
    // the label and colour of pixel p and the label of pixel p - 1 travel from one iteration to the next
    int32_t l = 0, lprev = -1;
    uint32_t r_ = 0, g_ = 0, b_ = 0;
    if (p0 < p1) {
      l = labels[p0];
      r_ = img[3 * p0]; g_ = img[3 * p0 + 1]; b_ = img[3 * p0 + 2];
      if (p0 > 0) lprev = labels[p0 - 1];
    }
    for (int p = p0; p < p1; ++p) {
      int32_t lnext = -1;
      uint32_t rn = 0, gn = 0, bn = 0;
      if (p + 1 < n) {
        lnext = labels[p + 1];
        rn = img[3 * p + 3]; gn = img[3 * p + 4]; bn = img[3 * p + 5];
      }
      if (l != cur) { flush(); cur = l; s = rank_of(l); }
      const uint32_t y = (uint32_t)row, x = (uint32_t)col;
      ++cnt;
      sr += r_; sg += g_; sb += b_;
      qr += r_ * r_; qg += g_ * g_; qb += b_ * b_;
      ys += y; xs += x;
      yy += (unsigned long long)(y * y);  // y, x < 65536: the squares fit 32 bits
      xx += (unsigned long long)(x * x);
      ymin = min(ymin, y); ymax = max(ymax, y); xmin = min(xmin, x); xmax = max(xmax, x);
      bool edge = col > 0 && lprev != l;
      if (col + 1 < W) {
        if (lnext == l) { ++m; tr += absdiff(r_, rn); tg += absdiff(g_, gn); tb += absdiff(b_, bn); }
        else edge = true;
      }
      if (row > 0 && labels[p - W] != l) edge = true;
      if (row + 1 < H) {
        const int q = p + W;
        if (labels[q] == l) { ++m; tr += absdiff(r_, img[3 * q]); tg += absdiff(g_, img[3 * q + 1]); tb += absdiff(b_, img[3 * q + 2]); }
        else edge = true;
      }
      nb += edge ? 1u : 0u;
      lprev = l; l = lnext; r_ = rn; g_ = gn; b_ = bn;
      if (++col == W) { col = 0; ++row; }
    }
    flush();
  }
  __syncthreads();

  if (tid == 0) {
    counts[0] = (int32_t)S;
    counts[1] = bad_image ? 1 : 0;
    counts[2] = overflow ? 1 : 0;
  }
  // ---- 3. the rows; every operand is converted to double, every result cast to float
  const uint32_t regions = active ? S : 0;
  for (int i = tid; i < node_capacity; i += kThreads) {
    float v[kDim];
    for (int k = 0; k < kDim; ++k) v[k] = 0.f;
    if ((uint32_t)i < regions) {
      const uint32_t* a = acc + i;
      const unsigned long long cnt = a[kN * kMaxNodes];
      const double c = (double)cnt;
      const double hgt = (double)(a[kYmax * kMaxNodes] - a[kYmin * kMaxNodes] + 1u);
      const double wid = (double)(a[kXmax * kMaxNodes] - a[kXmin * kMaxNodes] + 1u);
      const unsigned long long pairs = a[kM * kMaxNodes];
      for (int k = 0; k < 3; ++k) {
        const unsigned long long sum = a[(kSr + k) * kMaxNodes], sq = a[(kQr + k) * kMaxNodes];
        v[k] = (float)(((double)sum / 255.0) / c);                                   // rag_nodes' mean colour
        v[3 + k] = (float)(sqrt((double)(cnt * sq - sum * sum)) / (255.0 * c));      // colour std
        v[13 + k] = pairs ? (float)(((double)a[(kTr + k) * kMaxNodes] / 255.0) / (double)pairs) : 0.f;  // texture
      }
      const unsigned long long sy = a[kSy * kMaxNodes], sx = a[kSx * kMaxNodes];
      v[6] = (float)(c / (double)n);                                                 // area share
      v[7] = (float)(hgt / (double)H);                                               // bounding-box extent
      v[8] = (float)(wid / (double)W);
      v[9] = (float)(sqrt((double)(cnt * acc64[i] - sy * sy)) / (c * (double)H));    // spatial spread
      v[10] = (float)(sqrt((double)(cnt * acc64[kMaxNodes + i] - sx * sx)) / (c * (double)W));
      v[11] = (float)(c / (hgt * wid));                                              // box fill
      v[12] = (float)((double)a[kNb * kMaxNodes] / c);                               // boundary share
    }
    float4* dst = reinterpret_cast<float4*>(out + (size_t)i * kDim);
    for (int k = 0; k < kDim / 4; ++k) dst[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
  }
}

bool supported(int32_t B, int32_t H, int32_t W, int32_t node_capacity) {
  return B >= 1 && B <= (1 << 20) && H >= 1 && W >= 1 && (int64_t)H * W <= kMaxPixels && node_capacity >= 1 &&
         node_capacity <= kMaxNodes;
}

}  // namespace

extern "C" size_t gnc_region_descriptors_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t node_capacity) {
  if (!supported(B, H, W, node_capacity)) {
    gnc::set_error("gnc_region_descriptors_workspace_bytes: %d images of %d x %d at %d nodes is outside the supported set "
                   "(H*W <= %d, node_capacity <= %d)", B, H, W, node_capacity, kMaxPixels, kMaxNodes);
    return 0;
  }
  return kWorkspaceBytes;
}

extern "C" int gnc_region_descriptors_rgb_u8(const int32_t* labels, const uint8_t* img, int32_t B, int32_t H, int32_t W,
                                             int32_t node_capacity, float* out, int32_t* counts, void* workspace,
                                             size_t workspace_bytes, void* stream_) {
  GNC_REQUIRE(supported(B, H, W, node_capacity),
              "gnc_region_descriptors_rgb_u8: %d images of %d x %d at %d nodes is outside the supported set", B, H, W,
              node_capacity);
  GNC_REQUIRE(labels && img && out && counts, "gnc_region_descriptors_rgb_u8: null pointer");
  GNC_REQUIRE(gnc::aligned16(out), "gnc_region_descriptors_rgb_u8: out must be 16-byte aligned");
  if (!workspace || workspace_bytes < kWorkspaceBytes) {
    gnc::set_error("gnc_region_descriptors_rgb_u8: workspace too small");
    return GNC_ERR_WORKSPACE;
  }
  region_descriptor_kernel<<<B, kThreads, 0, (hipStream_t)stream_>>>(labels, img, H, W, node_capacity, out, counts);
  return gnc::check_launch("region_descriptor_kernel");
}
