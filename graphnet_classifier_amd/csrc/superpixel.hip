// Device-side SLIC superpixels: scikit-image 0.18.3 `slic()` for a 2-D uint8 RGB image with the options the
// reference passes (utils/image_to_graph/image_to_graph_superpixel.py:31): Lab conversion, sigma = 0, no mask,
// unit spacing, slic_zero off, enforce_connectivity with min/max size factors, start_label 0 or 1.
//
// Stages (one launch each, many images per launch; no host synchronisation anywhere):
//   slic_lab       uint8 -> img_as_float -> rgb2lab (skimage/color/colorconv.py) -> * 1/compactness, in fp64.
//   slic_seed      centres on skimage's regular_grid (z, y, x, L, a, b) = (0, y, x, 0, 0, 0); the grid itself is
//                  a function of (H, W, n_segments) only and is worked out on the host.
//   slic_assign    every pixel takes the nearest centre whose window covers it; ties go to the lowest centre
//                  index, exactly as the sequential centre loop with its strict `>` would; a pixel no window covers
//                  keeps its previous centre (the sequential code never resets that array).
//   slic_update    each centre moves to the mean (z, y, x, L, a, b) of its pixels.  Coordinate sums are integers
//                  (exact); colour sums are accumulated in raster order, the order of the sequential loop, so
//                  every bit matches.  A centre left without pixels becomes NaN there and never wins again: here
//                  it is marked dead.
//   slic_connect   _enforce_label_connectivity_cython verbatim: one workgroup per image, one lane running the
//                  raster scan with its breadth-first flood fill (capped at max_size, which splits a large
//                  component into pieces that start new labels), small components relabelled to the last
//                  already-labelled neighbour met by the fill (0 if none).
//
// The tile search in slic_assign makes the result independent of how far centres drift: a workgroup of 16 x 16
// pixels scans every centre once per iteration and keeps (in centre order) those whose window meets its tile.
#pragma clang fp contract(off)  // the reference's arithmetic is separate multiplies and adds: no FMA contraction

#include <math.h>

#include <algorithm>

#include "gnc_common.h"

namespace {

constexpr size_t kAlign = 256;
inline size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

// sRGB gamma of the 256 values u * (1/255) (img_as_float), as rgb2xyz computes them:
// v > 0.04045 ? ((v + 0.055) / 1.055) ** 2.4 : v / 12.92.  Tabulated bit for bit from NumPy's float64 `power`,
// whose last bit a device `pow` does not always reproduce.
__constant__ double kGamma[256] = {
    0x0.0p+0, 0x1.3e45677c176f7p-12, 0x1.3e45677c176f7p-11, 0x1.dd681b3a23272p-11,
    0x1.3e45677c176f7p-10, 0x1.8dd6c15b1d4b4p-10, 0x1.dd681b3a23272p-10, 0x1.167cba8c94818p-9,
    0x1.3e45677c176f7p-9, 0x1.660e146b9a5d5p-9, 0x1.8dd6c15b1d4b4p-9, 0x1.b6a31b5259c98p-9,
    0x1.e1e31d70c99ddp-9, 0x1.07c38bf8583a9p-8, 0x1.1fcc2beed6421p-8, 0x1.390ffaf95e279p-8,
    0x1.53936cc7bc927p-8, 0x1.6f5addb50c915p-8, 0x1.8c6a94031b561p-8, 0x1.aac6c0fb97350p-8,
    0x1.ca7381f9f602bp-8, 0x1.eb74e160978d0p-8, 0x1.06e76bbda92b8p-7, 0x1.18c2a5a8a8044p-7,
    0x1.2b4e09b3f0ae2p-7, 0x1.3e8b7b3bde964p-7, 0x1.527cd60af8b85p-7, 0x1.6723eea8d3708p-7,
    0x1.7c8292a3db6b4p-7, 0x1.929a88d67b520p-7, 0x1.a96d91a8016bdp-7, 0x1.c0fd67499fab6p-7,
    0x1.d94bbdefd740ep-7, 0x1.f25a44089883cp-7, 0x1.061551372c694p-6, 0x1.135f3e4c2cce2p-6,
    0x1.210bb8642b173p-6, 0x1.2f1b8c1ae46bbp-6, 0x1.3d8f839b79c0bp-6, 0x1.4c6866b3e9fa3p-6,
    0x1.5ba6fae794313p-6, 0x1.6b4c0380d2dedp-6, 0x1.7b5841a1bf3adp-6, 0x1.8bcc74542addap-6,
    0x1.9ca95898dc8b4p-6, 0x1.adefa9761c01dp-6, 0x1.bfa0200597bd9p-6, 0x1.d1bb7381aec1fp-6,
    0x1.e442595227bcap-6, 0x1.f73585185e1b3p-6, 0x1.054ad45d76878p-5, 0x1.0f31ba386ff26p-5,
    0x1.194fcb663747bp-5, 0x1.23a55e62a6627p-5, 0x1.2e32c8e148d10p-5, 0x1.38f85fd21eacfp-5,
    0x1.43f67766310fep-5, 0x1.4f2d6313fa8cdp-5, 0x1.5a9d759ba5ed0p-5, 0x1.6647010b254eep-5,
    0x1.722a56c2239eep-5, 0x1.7e47c775d2424p-5, 0x1.8a9fa33494b08p-5, 0x1.973239698b9ccp-5,
    0x1.a3ffd8e001389p-5, 0x1.b108cfc6b7fbcp-5, 0x1.be4d6bb31d51ep-5, 0x1.cbcdf9a4616f2p-5,
    0x1.d98ac60675832p-5, 0x1.e7841cb4f16dfp-5, 0x1.f5ba48fde2048p-5, 0x1.0216cad240765p-4,
    0x1.096f2671eb815p-4, 0x1.10e65c38a5191p-4, 0x1.187c90bf8bce2p-4, 0x1.2031e85f5d6dbp-4,
    0x1.28068731a1952p-4, 0x1.2ffa9111cb94bp-4, 0x1.380e299e53f91p-4, 0x1.40417439ca10fp-4,
    0x1.4894940bddbfap-4, 0x1.5107ac0261e59p-4, 0x1.599aded247aa9p-4, 0x1.624e4ef892ed4p-4,
    0x1.6b221ebb4817ep-4, 0x1.7416702a539d1p-4, 0x1.7d2b65206b528p-4, 0x1.86611f43e9e6ap-4,
    0x1.8fb7c007a4a6fp-4, 0x1.992f68abbbc89p-4, 0x1.a2c83a3e6566ap-4, 0x1.ac82559cb3644p-4,
    0x1.b65ddb7354604p-4, 0x1.c05aec3f4fe5dp-4, 0x1.ca79a84ebe030p-4, 0x1.d4ba2fc17a6a5p-4,
    0x1.df1ca289d34b8p-4, 0x1.e9a1206d34003p-4, 0x1.f447c904cbb4bp-4, 0x1.ff10bbbe302c3p-4,
    0x1.04fe0bedfe5f1p-3, 0x1.0a84fe3b36d8fp-3, 0x1.101d443dfc06ep-3, 0x1.15c6ed58eefdfp-3,
    0x1.1b8208da5fef1p-3, 0x1.214ea5fc9514ap-3, 0x1.272cd3e610121p-3, 0x1.2d1ca1a9d1cfbp-3,
    0x1.331e1e479cdf5p-3, 0x1.393158ac3674ep-3, 0x1.3f565fb1a5fd5p-3, 0x1.458d421f735dfp-3,
    0x1.4bd60eaae3e72p-3, 0x1.5230d3f736034p-3, 0x1.589da095dbaa1p-3, 0x1.5f1c8306b3a3bp-3,
    0x1.65ad89b841a2bp-3, 0x1.6c50c307e53c0p-3, 0x1.73063d420fc80p-3, 0x1.79ce06a279303p-3,
    0x1.80a82d5453b5dp-3, 0x1.8794bf727eb40p-3, 0x1.8e93cb07b8679p-3, 0x1.95a55e0ecec0ap-3,
    0x1.9cc98672cf47ep-3, 0x1.a400520f3619cp-3, 0x1.ab49ceb01c003p-3, 0x1.b2a60a1263b0ap-3,
    0x1.ba1511e3e632cp-3, 0x1.c196f3c39e76fp-3, 0x1.c92bbd41d41fep-3, 0x1.d0d37be045851p-3,
    0x1.d88e3d1250f63p-3, 0x1.e05c0e3d1d3e0p-3, 0x1.e83cfcb7c16f0p-3, 0x1.f03115cb6bfd4p-3,
    0x1.f83866b38924dp-3, 0x1.00297e4ef4553p-2, 0x1.044072557177ap-2, 0x1.086115f6beb39p-2,
    0x1.0c8b6fb5c735dp-2, 0x1.10bf860ef0399p-2, 0x1.14fd5f782a5a6p-2, 0x1.1945026102997p-2,
    0x1.1d967532b31b1p-2, 0x1.21f1be50339e7p-2, 0x1.2656e41649ae3p-2, 0x1.2ac5ecdb988f8p-2,
    0x1.2f3edef0b0ed5p-2, 0x1.33c1c0a020438p-2, 0x1.384e982e800b1p-2, 0x1.3ce56bda84a80p-2,
    0x1.418641dd0c1bcp-2, 0x1.463120692c7afp-2, 0x1.4ae60dac4229dp-2, 0x1.4fa50fcdfde15p-2,
    0x1.546e2cf0727a9p-2, 0x1.59416b3022857p-2, 0x1.5e1ed0a40daabp-2, 0x1.6306635dbdd7ap-2,
    0x1.67f82969543a2p-2, 0x1.6cf428cd9607ap-2, 0x1.71fa678bf915dp-2, 0x1.770aeba0b042ap-2,
    0x1.7c25bb02b7ac2p-2, 0x1.814adba3e0bd9p-2, 0x1.867a5370de0b1p-2, 0x1.8bb428514f066p-2,
    0x1.90f86027cb84dp-2, 0x1.964700d1ef1b1p-2, 0x1.9ba0102864520p-2, 0x1.a10393feefafdp-2,
    0x1.a67192247a9bep-2, 0x1.abea10631e195p-2, 0x1.b16d14802d5cap-2, 0x1.b6faa43c403bbp-2,
    0x1.bc92c5533d784p-2, 0x1.c2357d7c64e5dp-2, 0x1.c7e2d26a596dep-2, 0x1.cd9ac9cb2aef1p-2,
    0x1.d35d69485ffc2p-2, 0x1.d92ab686ff782p-2, 0x1.df02b7279a10cp-2, 0x1.e4e570c6539c5p-2,
    0x1.ead2e8faec526p-2, 0x1.f0cb2558c9ea5p-2, 0x1.f6ce2b6f00983p-2, 0x1.fcdc00c85bec2p-2,
    0x1.017a5575b3cb2p-1, 0x1.048c17ad3c04bp-1, 0x1.07a349c9d9837p-1, 0x1.0abfee888c050p-1,
    0x1.0de208a4444c8p-1, 0x1.11099ad5e83eap-1, 0x1.1436a7d456eeep-1, 0x1.176932546ca12p-1,
    0x1.1aa13d0906bd9p-1, 0x1.1ddecaa307b85p-1, 0x1.2121ddd15aecep-1, 0x1.246a7940f86d1p-1,
    0x1.27b89f9ce8c4ap-1, 0x1.2b0c538e48b07p-1, 0x1.2e6597bc4cc9fp-1, 0x1.31c46ecc4528dp-1,
    0x1.3528db61a0f72p-1, 0x1.3892e01df1fccp-1, 0x1.3c027fa0f01ebp-1, 0x1.3f77bc887cd3bp-1,
    0x1.42f29970a68f7p-1, 0x1.467318f3ac22cp-1, 0x1.49f93daa00113p-1, 0x1.4d850a2a4bde1p-1,
    0x1.51168109734e3p-1, 0x1.54ada4da97a1bp-1, 0x1.584a782f1ac23p-1, 0x1.5becfd96a2698p-1,
    0x1.5f95379f1b3ecp-1, 0x1.634328d4bbe97p-1, 0x1.66f6d3c2081cfp-1, 0x1.6ab03aefd39abp-1,
    0x1.6e6f60e5452b2p-1, 0x1.72344827d98f6p-1, 0x1.75fef33b6669bp-1, 0x1.79cf64a21d1e3p-1,
    0x1.7da59edc8dab0p-1, 0x1.8181a469a9787p-1, 0x1.856377c6c6224p-1, 0x1.894b1b6fa0378p-1,
    0x1.8d3891de5df47p-1, 0x1.912bdd8b91f44p-1, 0x1.952500ee3dda5p-1, 0x1.9923fe7bd4f67p-1,
    0x1.9d28d8a83edfcp-1, 0x1.a13391e5da09fp-1, 0x1.a5442ca57e52ep-1, 0x1.a95aab567f88fp-1,
    0x1.ad771066afec2p-1, 0x1.b1995e4262a68p-1, 0x1.b5c197546e3f7p-1, 0x1.b9efbe062f086p-1,
    0x1.be23d4bf8981bp-1, 0x1.c25ddde6ecbbbp-1, 0x1.c69ddbe154af1p-1, 0x1.cae3d1124c90bp-1,
    0x1.cf2fbfdbf11ecp-1, 0x1.d381aa9ef2e82p-1, 0x1.d7d993ba988d4p-1, 0x1.dc377d8cc0fd5p-1,
    0x1.e09b6a71e5aa6p-1, 0x1.e5055cc51cbb4p-1, 0x1.e97556e01b351p-1, 0x1.edeb5b1b37216p-1,
    0x1.f2676bcd69adep-1, 0x1.f6e98b4c51466p-1, 0x1.fb71bbec33ab3p-1, 0x1.0000000000000p+0,
};

// skimage.color.colorconv.xyz_from_rgb and the D65 / 2-degree white point
constexpr double kM[3][3] = {{0.412453, 0.357580, 0.180423}, {0.212671, 0.715160, 0.072169}, {0.019334, 0.119193, 0.950227}};
constexpr double kWhite[3] = {0.95047, 1.0, 1.08883};

struct Centre {
  double y, x, l, a, b;
  int32_t alive;
  int32_t pad;
};
struct Box {
  int32_t y0, y1, x0, x1;  // inclusive pixel bounds of the centre's pixels; y1 < 0 when it has none
};

struct Geometry {
  int H, W, K, ny, nx, y0, x0, sy, sx;  // seeds at (y0 + i*sy, x0 + j*sx), K = ny*nx
  int wy, wx;                           // window half-widths / 2 of _slic_cython (its own grid of K points)
  double step;                          // max of the seed grid's steps: spatial weight 1 / step^2
};

// skimage.util.regular_grid((1, H, W), n): (start, step) of the y and x slices; steps 1 and starts 0 when the
// image has no more than n pixels (slice(None)).
void regular_grid_2d(int H, int W, int64_t n, int* y0, int* sy, int* x0, int* sx) {
  const double space = (double)H * (double)W;
  if (space <= (double)n) {
    *y0 = *x0 = 0;
    *sy = *sx = 1;
    return;
  }
  // (space / n) ** (1/3) > 1 always here, so the loop over sorted dims (1, min, max) runs: dim 0 fixes the unit
  // depth; it ends there unless the short side is below the square step, when dim 1 fixes the short side.
  const double d1 = (double)std::min(H, W), d2 = (double)std::max(H, W);
  double s1 = pow(space / (double)n, 1.0 / 2.0), s2 = s1;
  if (!(d1 >= s1 && d2 >= s2)) {
    s1 = d1;
    s2 = pow(d2 / (double)n, 1.0 / 1.0);
  }
  const int st1 = (int)floor(s1 / 2.0), st2 = (int)floor(s2 / 2.0);  // (stepsizes // 2).astype(int)
  const int r1 = (int)rint(s1), r2 = (int)rint(s2);                  // np.round: half to even
  if (H <= W) {
    *y0 = st1; *sy = r1; *x0 = st2; *sx = r2;
  } else {
    *y0 = st2; *sy = r2; *x0 = st1; *sx = r1;
  }
}

Geometry geometry(int H, int W, int64_t n_segments) {
  Geometry g;
  g.H = H;
  g.W = W;
  regular_grid_2d(H, W, n_segments, &g.y0, &g.sy, &g.x0, &g.sx);
  g.ny = (H - g.y0 + g.sy - 1) / g.sy;
  g.nx = (W - g.x0 + g.sx - 1) / g.sx;
  g.K = g.ny * g.nx;
  g.step = std::max(1.0, (double)std::max(g.sy, g.sx));  // max(steps), steps = (1.0, sy, sx)
  int wy0, wx0;
  regular_grid_2d(H, W, g.K, &wy0, &g.wy, &wx0, &g.wx);  // _slic_cython: regular_grid(shape, n_centroids)
  return g;
}

struct SlicWs {
  double* lab;      // [B][HW][3] scaled Lab
  int32_t* near;    // [B][HW] nearest centre
  int32_t* queue;   // [B][HW] flood-fill coordinate list
  Centre* centres;  // [B][K]
  Box* boxes;       // [B][K]
};

size_t carve_bytes(int64_t B, int64_t HW, int64_t K, SlicWs* w, void* base) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? (char*)base + off : nullptr;
    off += align_up(bytes);
    return p;
  };
  char* lab = take((size_t)B * HW * 3 * sizeof(double));
  char* near = take((size_t)B * HW * sizeof(int32_t));
  char* queue = take((size_t)B * HW * sizeof(int32_t));
  char* centres = take((size_t)B * K * sizeof(Centre));
  char* boxes = take((size_t)B * K * sizeof(Box));
  if (w) {
    w->lab = (double*)lab;
    w->near = (int32_t*)near;
    w->queue = (int32_t*)queue;
    w->centres = (Centre*)centres;
    w->boxes = (Box*)boxes;
  }
  return off;
}

__global__ void slic_lab(const uint8_t* __restrict__ img, int64_t total, double ratio, double* __restrict__ lab,
                         int32_t* __restrict__ near) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; p < total; p += stride) {
    const double r = kGamma[img[3 * p]], g = kGamma[img[3 * p + 1]], b = kGamma[img[3 * p + 2]];
    double t[3];
    for (int j = 0; j < 3; ++j) {
      const double xyz = r * kM[j][0] + g * kM[j][1] + b * kM[j][2];  // arr @ xyz_from_rgb.T
      const double v = xyz / kWhite[j];
      t[j] = v > 0.008856 ? cbrt(v) : 7.787 * v + 16. / 116.;
    }
    lab[3 * p + 0] = ((116. * t[1]) - 16.) * ratio;
    lab[3 * p + 1] = (500.0 * (t[0] - t[1])) * ratio;
    lab[3 * p + 2] = (200.0 * (t[1] - t[2])) * ratio;
    near[p] = -1;  // np.full(..., -1): a pixel no first-round window covers stays -1
  }
}

__global__ void slic_seed(Geometry g, int64_t total, Centre* __restrict__ centres, Box* __restrict__ boxes) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; t < total; t += stride) {
    const int k = (int)(t % g.K);
    Centre c;
    c.y = (double)(g.y0 + (k / g.nx) * g.sy);
    c.x = (double)(g.x0 + (k % g.nx) * g.sx);
    c.l = c.a = c.b = 0.0;
    c.alive = 1;
    c.pad = 0;
    centres[t] = c;
    boxes[t] = Box{INT32_MAX, -1, INT32_MAX, -1};
  }
}

constexpr int kTile = 16;  // slic_assign: 16 x 16 pixels, one per lane of a 256-lane workgroup

struct Cand {
  double y, x, l, a, b;
  int32_t k, y0, y1, x0, x1, pad;
};

__global__ __launch_bounds__(256) void slic_assign(Geometry g, const double* __restrict__ lab,
                                                   const Centre* __restrict__ centres, int32_t* __restrict__ near,
                                                   Box* __restrict__ boxes) {
  __shared__ Cand cand[256];
  __shared__ int wave_count[4];
  const int b = blockIdx.z;
  const int ty0 = blockIdx.y * kTile, tx0 = blockIdx.x * kTile;
  const int ty1 = std::min(ty0 + kTile, g.H), tx1 = std::min(tx0 + kTile, g.W);
  const int tid = threadIdx.x, lane = tid % gnc::kWave, wave = tid / gnc::kWave;
  const int py = ty0 + tid / kTile, px = tx0 + tid % kTile;
  const bool mine = py < g.H && px < g.W;
  const int64_t HW = (int64_t)g.H * g.W;
  const int64_t p = (int64_t)b * HW + (int64_t)py * g.W + px;
  double pl = 0, pa = 0, pb = 0;
  int32_t best_k = -1;
  if (mine) {
    pl = lab[3 * p];
    pa = lab[3 * p + 1];
    pb = lab[3 * p + 2];
    best_k = near[p];
  }
  double best = 1.7976931348623157e308;  // DBL_MAX
  const double sw = 1.0 / (g.step * g.step);
  const Centre* cb = centres + (int64_t)b * g.K;
  for (int base = 0; base < g.K; base += 256) {  // bounded by K <= H*W
    const int k = base + tid;
    bool hit = false;
    Cand c;
    if (k < g.K) {
      const Centre cc = cb[k];
      if (cc.alive) {
        // <Py_ssize_t>max(c - 2*step, 0) and <Py_ssize_t>min(c + 2*step + 1, size): truncation toward zero
        c.y0 = (int)fmax(cc.y - 2.0 * g.wy, 0.0);
        c.y1 = (int)fmin(cc.y + 2.0 * g.wy + 1.0, (double)g.H);
        c.x0 = (int)fmax(cc.x - 2.0 * g.wx, 0.0);
        c.x1 = (int)fmin(cc.x + 2.0 * g.wx + 1.0, (double)g.W);
        hit = c.y0 < ty1 && c.y1 > ty0 && c.x0 < tx1 && c.x1 > tx0;
        c.y = cc.y; c.x = cc.x; c.l = cc.l; c.a = cc.a; c.b = cc.b; c.k = k;
      }
    }
    // ordered compaction: candidates keep ascending centre order
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wave_count[wave] = __popcll(m);
    __syncthreads();
    int off = 0, n = 0;
    for (int w = 0; w < 4; ++w) {
      off += w < wave ? wave_count[w] : 0;
      n += wave_count[w];
    }
    if (hit) cand[off + __popcll(m & ((1ull << lane) - 1ull))] = c;
    __syncthreads();
    if (mine) {
      for (int i = 0; i < n; ++i) {
        const Cand& q = cand[i];
        if (py < q.y0 || py >= q.y1 || px < q.x0 || px >= q.x1) continue;
        const double dy = (q.y - py) * (q.y - py), dx = (q.x - px) * (q.x - px);
        double d = (dy + dx) * sw;  // (dz + dy + dx) * spatial_weight with dz = 0
        double col = 0;
        col += (pl - q.l) * (pl - q.l);
        col += (pa - q.a) * (pa - q.a);
        col += (pb - q.b) * (pb - q.b);
        d += col;
        if (best > d) {
          best = d;
          best_k = q.k;
        }
      }
    }
    __syncthreads();
  }
  if (mine && best_k >= 0) {
    near[p] = best_k;
    Box* bx = boxes + (int64_t)b * g.K + best_k;
    atomicMin(&bx->y0, py);
    atomicMax(&bx->y1, py);
    atomicMin(&bx->x0, px);
    atomicMax(&bx->x1, px);
  }
}

// One wave per centre: the centre's pixels are those inside its box with its label, summed in raster order.
__global__ __launch_bounds__(256) void slic_update(Geometry g, int64_t total, const double* __restrict__ lab,
                                                   const int32_t* __restrict__ near, Centre* __restrict__ centres,
                                                   Box* __restrict__ boxes) {
  const int lane = threadIdx.x % gnc::kWave;
  const int64_t t = (int64_t)blockIdx.x * (blockDim.x / gnc::kWave) + threadIdx.x / gnc::kWave;
  if (t >= total) return;
  const int b = (int)(t / g.K), k = (int)(t % g.K);
  const int64_t HW = (int64_t)g.H * g.W;
  const Box box = boxes[t];
  Centre c = centres[t];  // a dead centre still owns the pixels no window reached since: it comes back
  int64_t cnt = 0, sy = 0, sx = 0;
  double sl = 0, sa = 0, sb = 0;
  for (int y = box.y0; y <= box.y1; ++y) {  // empty when the centre has no pixels (y1 = -1)
    for (int x0 = box.x0; x0 <= box.x1; x0 += gnc::kWave) {
      const int x = x0 + lane;
      const int64_t p = (int64_t)b * HW + (int64_t)y * g.W + x;
      const bool own = x <= box.x1 && near[p] == k;
      double vl = 0, va = 0, vb = 0;
      if (own) {
        vl = lab[3 * p];
        va = lab[3 * p + 1];
        vb = lab[3 * p + 2];
        sx += x;
      }
      unsigned long long m = __ballot(own);
      const int n = __popcll(m);
      cnt += n;
      sy += (int64_t)y * n;
      while (m) {  // ascending x: the sequential summation order
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        sl += __shfl(vl, src);
        sa += __shfl(va, src);
        sb += __shfl(vb, src);
      }
    }
  }
  for (int o = gnc::kWave / 2; o > 0; o /= 2) sx += __shfl_xor(sx, o);
  if (lane == 0) {
    if (cnt == 0) {
      c.alive = 0;  // 0 / 0: NaN centre, outside every later window comparison
    } else {
      c.alive = 1;
      const double n = (double)cnt;
      c.y = (double)sy / n;
      c.x = (double)sx / n;
      c.l = sl / n;
      c.a = sa / n;
      c.b = sb / n;
    }
    centres[t] = c;
    boxes[t] = Box{INT32_MAX, -1, INT32_MAX, -1};
  }
}

__global__ void slic_plain_labels(const int32_t* __restrict__ near, int64_t total, int start_label, int B, int K,
                                  int32_t* __restrict__ labels, int32_t* __restrict__ counts) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = p; i < B; i += stride) counts[i] = K;
  for (; p < total; p += stride) labels[p] = near[p] + start_label;
}

// _enforce_label_connectivity_cython on one image per workgroup.  `near` + start_label are the segments; a pixel
// whose segment equals start_label - 1 is never a seed (the scan skips such values), and `out` holds
// start_label - 1 for "not yet reached".
__global__ __launch_bounds__(64) void slic_connect(const int32_t* __restrict__ near, int H, int W, int start_label,
                                                   int min_size, int max_size, int32_t* __restrict__ queue_all,
                                                   int32_t* __restrict__ labels, int32_t* __restrict__ counts) {
  const int b = blockIdx.x;
  const int64_t HW = (int64_t)H * W;
  const int32_t* seg = near + (int64_t)b * HW;
  int32_t* out = labels + (int64_t)b * HW;
  int32_t* queue = queue_all + (int64_t)b * HW;
  const int unset = start_label - 1;
  for (int64_t p = threadIdx.x; p < HW; p += blockDim.x) out[p] = unset;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int dx[4] = {1, -1, 0, 0}, dy[4] = {0, 0, 1, -1};
  int cur = start_label;
  for (int y = 0; y < H; ++y) {
    for (int x = 0; x < W; ++x) {
      const int p0 = y * W + x;
      const int label = seg[p0] + start_label;
      if (label == unset || out[p0] >= start_label) continue;
      int adjacent = 0;
      out[p0] = cur;
      int size = 1, visited = 0;
      queue[0] = p0;
      while (visited < size && size < max_size) {  // bounded: size <= H*W
        const int q = queue[visited];
        const int qy = q / W, qx = q % W;
        for (int i = 0; i < 4; ++i) {
          const int yy = qy + dy[i], xx = qx + dx[i];
          if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
          const int r = yy * W + xx;
          const int o = out[r];
          if (seg[r] + start_label == label && o == unset) {
            out[r] = cur;
            queue[size++] = r;
            if (size >= max_size) break;
          } else if (o >= start_label && o != cur) {
            adjacent = o;
          }
        }
        ++visited;
      }
      if (size < min_size) {
        for (int i = 0; i < size; ++i) out[queue[i]] = adjacent;
      } else {
        ++cur;
      }
    }
  }
  counts[b] = cur - start_label;
}

int grid_for(int64_t n) {
  int64_t g = gnc::ceil_div(n > 0 ? n : 1, gnc::kBlock);
  const int64_t cap = (int64_t)gnc::num_cu() * 8;
  return (int)(g < cap ? g : cap);
}

constexpr int kMaxSide = 4096;

}  // namespace

extern "C" size_t gnc_slic_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t n_segments) {
  if (B < 1 || H < 1 || W < 1 || H > kMaxSide || W > kMaxSide || n_segments < 1) return 0;
  const Geometry g = geometry(H, W, n_segments);
  return carve_bytes(B, (int64_t)H * W, g.K, nullptr, nullptr);
}

extern "C" int gnc_slic_rgb_u8(const uint8_t* img, int32_t B, int32_t H, int32_t W, int32_t n_segments,
                               double compactness, int32_t max_iter, int32_t enforce_connectivity,
                               double min_size_factor, double max_size_factor, int32_t start_label, int32_t* labels,
                               int32_t* counts, void* workspace, size_t workspace_bytes, void* stream_) {
  GNC_REQUIRE(img && labels && counts && workspace, "gnc_slic_rgb_u8: null pointer");
  GNC_REQUIRE(B >= 1 && H >= 1 && W >= 1, "gnc_slic_rgb_u8: empty batch or image (%d x %d x %d)", B, H, W);
  if (H > kMaxSide || W > kMaxSide || n_segments < 1 || !(compactness > 0) || max_iter < 1 || max_iter > 1000 ||
      (start_label != 0 && start_label != 1) || !(min_size_factor >= 0) || !(max_size_factor > 0)) {
    gnc::set_error("gnc_slic_rgb_u8: options outside the supported set (H, W <= %d, n_segments >= 1, compactness > 0, "
                   "1 <= max_iter <= 1000, start_label 0 or 1, size factors >= 0)", kMaxSide);
    return GNC_ERR_UNSUPPORTED;
  }
  const Geometry g = geometry(H, W, n_segments);
  const int64_t HW = (int64_t)H * W;
  SlicWs w;
  if (carve_bytes(B, HW, g.K, &w, workspace) > workspace_bytes) {
    gnc::set_error("gnc_slic_rgb_u8: workspace too small");
    return GNC_ERR_WORKSPACE;
  }
  hipStream_t stream = (hipStream_t)stream_;
  int rc;
  slic_lab<<<grid_for(B * HW), gnc::kBlock, 0, stream>>>(img, B * HW, 1.0 / compactness, w.lab, w.near);
  if ((rc = gnc::check_launch("slic_lab"))) return rc;
  const int64_t nc = (int64_t)B * g.K;
  slic_seed<<<grid_for(nc), gnc::kBlock, 0, stream>>>(g, nc, w.centres, w.boxes);
  if ((rc = gnc::check_launch("slic_seed"))) return rc;
  const dim3 tiles((unsigned)gnc::ceil_div(W, kTile), (unsigned)gnc::ceil_div(H, kTile), (unsigned)B);
  const unsigned update_blocks = (unsigned)gnc::ceil_div(nc, gnc::kBlock / gnc::kWave);
  for (int it = 0; it < max_iter; ++it) {
    slic_assign<<<tiles, 256, 0, stream>>>(g, w.lab, w.centres, w.near, w.boxes);
    if ((rc = gnc::check_launch("slic_assign"))) return rc;
    if (it + 1 == max_iter) break;  // the last update moves centres nobody reads
    slic_update<<<update_blocks, gnc::kBlock, 0, stream>>>(g, nc, w.lab, w.near, w.centres, w.boxes);
    if ((rc = gnc::check_launch("slic_update"))) return rc;
  }
  if (!enforce_connectivity) {
    slic_plain_labels<<<grid_for(B * HW), gnc::kBlock, 0, stream>>>(w.near, B * HW, start_label, B, g.K, labels, counts);
    return gnc::check_launch("slic_plain_labels");
  }
  const double segment_size = (double)HW / (double)g.K;
  const int min_size = (int)(min_size_factor * segment_size), max_size = (int)(max_size_factor * segment_size);
  slic_connect<<<B, gnc::kWave, 0, stream>>>(w.near, H, W, start_label, min_size, max_size, w.queue, labels, counts);
  return gnc::check_launch("slic_connect");
}
