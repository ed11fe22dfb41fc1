// Batched region-adjacency build: B label images of one size -> B graphs at fixed capacities, ONE launch.
//
// Same result per image as gnc_rag_build (graph_build.hip: utils/image_to_graph/image_to_graph_superpixel.py:36-71
// after the SLIC call), bit for bit, without its 5 memsets, 4 kernels, scan, 64-bit radix sort, unique and the host
// read of the sizes: a workgroup owns one image and keeps everything in LDS.
//
//   1. presence bitmap over the labels [0, H*W) (2048 words), popcount prefix per word: the dense index of label l
//      is prefix[l / 32] + popc(bitmap[l / 32] below bit l % 32) - labels may have gaps, as in gnc_rag_build;
//   2. every thread walks a run of consecutive pixels and keeps count / R / G / B / y / x sums of the current label in
//      registers, flushed with integer LDS atomics when the label changes (~1-2 flushes per 16 pixels); a pixel whose
//      right or lower neighbour has another label sets bit (lo, hi) of a 512 x 512 adjacency bit matrix;
//   3. node rows from the sums with gnc_rag_build's double-precision expression; popcounts of the matrix rows and a
//      scan give every row's first pair slot, and a thread per row writes its set bits in ascending order as
//      [i,j],[j,i] - the lexicographic order of the sorted unique pairs.
//
// Only integer atomics (add, or) are used, so the result does not depend on the order in which threads run.
// Rows behind the node count are zeros and edge slots behind the edge count are -1: whole buffers are reproducible.
// A graph that does not fit the capacities sets its overflow flag and leaves its slices all padding.
#include "gnc_common.h"

namespace {

constexpr int kThreads = 1024;                 // one workgroup per image, 16 waves
constexpr int kWaves = kThreads / gnc::kWave;
constexpr int kMaxPixels = 256 * 256;          // labels lie in [0, H*W): the presence bitmap has one bit per label
constexpr int kBitmapWords = kMaxPixels / 32;  // 2048
constexpr int kMaxNodes = 512;                 // adjacency bit matrix 512 x 512 = 32 KB
constexpr int kRowWords = kMaxNodes / 32;      // 16
constexpr int kMaxEdges = 4096;
constexpr size_t kWorkspaceBytes = 256;        // nothing is staged in HBM; the query doubles as the supported-set check

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

__global__ __launch_bounds__(kThreads) void rag_batched_kernel(
    const int32_t* __restrict__ labels_all, const uint8_t* __restrict__ img_all, int H, int W, int node_capacity,
    int edge_capacity, float* __restrict__ x_all, float* __restrict__ pos_all, int64_t* __restrict__ ei_all,
    int32_t* __restrict__ counts_all) {
  __shared__ uint32_t bitmap[kBitmapWords];       // 8 KB  label l occurs
  __shared__ uint32_t prefix[kBitmapWords];       // 8 KB  labels present below word w
  __shared__ uint32_t sums[6 * kMaxNodes];        // 12 KB count, R, G, B, y, x per segment (all below 2^32 for H*W <= 65536)
  __shared__ uint32_t adj[kMaxNodes * kRowWords];  // 32 KB bit (i, j), i < j: segments i and j touch
  __shared__ uint32_t row_first[kMaxNodes];       // 2 KB  first pair slot of row i
  __shared__ uint32_t scratch[kWaves];
  __shared__ uint32_t bad_flag;

  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = H * W;
  const int32_t* __restrict__ labels = labels_all + (size_t)b * n;
  const uint8_t* __restrict__ img = img_all + (size_t)b * n * 3;
  float* __restrict__ x = x_all + (size_t)b * node_capacity * 3;
  float* __restrict__ pos = pos_all + (size_t)b * node_capacity * 2;
  int64_t* __restrict__ ei = ei_all + (size_t)b * 2 * edge_capacity;
  int32_t* __restrict__ counts = counts_all + 4 * b;

  const int words = (n + 31) / 32;
  for (int i = tid; i < words; i += kThreads) bitmap[i] = 0;
  for (int i = tid; i < 6 * kMaxNodes; i += kThreads) sums[i] = 0;
  for (int i = tid; i < kMaxNodes * kRowWords; i += kThreads) adj[i] = 0;
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

  const bool matrix_fits = S <= (uint32_t)kMaxNodes;
  uint32_t pairs = 0;
  if (matrix_fits) {
    // ---- 2. sums per segment and the adjacency bits
    int32_t cur = -1;
    uint32_t s = 0, cnt = 0, r_ = 0, g_ = 0, b_ = 0, ys = 0, xs = 0;
    auto flush = [&]() {
      if (cnt) {
        atomicAdd(&sums[6 * s + 0], cnt); atomicAdd(&sums[6 * s + 1], r_); atomicAdd(&sums[6 * s + 2], g_);
        atomicAdd(&sums[6 * s + 3], b_);  atomicAdd(&sums[6 * s + 4], ys); atomicAdd(&sums[6 * s + 5], xs);
      }
      cnt = r_ = g_ = b_ = ys = xs = 0;
    };
    auto touch = [&](uint32_t a, int32_t l2) {
      const uint32_t c = rank_of(l2);
      const uint32_t lo = a < c ? a : c, hi = a < c ? c : a;
      const uint32_t bit = 1u << (hi & 31);
      uint32_t* word = &adj[lo * kRowWords + (hi >> 5)];
      if (!(*word & bit)) atomicOr(word, bit);
    };
    int row = p0 / W, col = p0 - row * W;
    for (int p = p0; p < p1; ++p) {
      const int32_t l = labels[p];
      if (l >= 0 && l < n) {
        if (l != cur) { flush(); cur = l; s = rank_of(l); }
        ++cnt; r_ += img[3 * p]; g_ += img[3 * p + 1]; b_ += img[3 * p + 2]; ys += (uint32_t)row; xs += (uint32_t)col;
        if (col + 1 < W) {
          const int32_t l2 = labels[p + 1];
          if (l2 != l && l2 >= 0 && l2 < n) touch(s, l2);
        }
        if (row + 1 < H) {
          const int32_t l2 = labels[p + W];
          if (l2 != l && l2 >= 0 && l2 < n) touch(s, l2);
        }
      }
      if (++col == W) { col = 0; ++row; }
    }
    flush();
    __syncthreads();
    // ---- 3a. pair slots: popcount per matrix row, exclusive scan (kMaxNodes <= kThreads)
    uint32_t deg = 0;
    if (tid < (int)S)
      for (int w = 0; w < kRowWords; ++w) deg += __popc(adj[tid * kRowWords + w]);
    const uint32_t first = block_exclusive_scan(deg, scratch, &pairs);
    if (tid < kMaxNodes) row_first[tid] = first;
    __syncthreads();
  }

  const bool fits = matrix_fits && S <= (uint32_t)node_capacity && 2 * pairs <= (uint32_t)edge_capacity;
  if (tid == 0) {
    counts[0] = (int32_t)S;
    counts[1] = matrix_fits ? (int32_t)(2 * pairs) : -1;  // beyond the matrix the adjacency is not formed: unknown
    counts[2] = (int32_t)bad_flag;
    counts[3] = fits ? 0 : 1;
  }
  const uint32_t nodes = fits ? S : 0, edges = fits ? 2 * pairs : 0;
  // ---- 3b. node rows (gnc_rag_build's rag_nodes, same expressions), zeros behind them
  for (int i = tid; i < node_capacity; i += kThreads) {
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if ((uint32_t)i < nodes) {
      const double c = (double)sums[6 * i];
      for (int k = 0; k < 3; ++k) v[k] = (float)(((double)sums[6 * i + 1 + k] / 255.0) / c);  // img_as_float mean
      v[3] = (float)((double)sums[6 * i + 4] / c);                                            // centroid y, x
      v[4] = (float)((double)sums[6 * i + 5] / c);
    }
    x[3 * i] = v[0]; x[3 * i + 1] = v[1]; x[3 * i + 2] = v[2];
    pos[2 * i] = v[3]; pos[2 * i + 1] = v[4];
  }
  // ---- 3c. edges [i,j],[j,i] in the order of the sorted pairs, -1 behind them
  for (int k = edges + tid; k < edge_capacity; k += kThreads) { ei[k] = -1; ei[edge_capacity + k] = -1; }
  if (fits && tid < (int)S) {
    uint32_t k = 2 * row_first[tid];  // < edges <= edge_capacity for every set bit of this row
    for (int w = 0; w < kRowWords; ++w) {
      uint32_t bits = adj[tid * kRowWords + w];
      while (bits) {
        const int j = w * 32 + __ffs(bits) - 1;
        bits &= bits - 1;
        ei[k] = tid;     ei[edge_capacity + k] = j;        // [i, j]
        ei[k + 1] = j;   ei[edge_capacity + k + 1] = tid;  // [j, i]   (superpixel.py:65-66)
        k += 2;
      }
    }
  }
}

bool supported(int32_t B, int32_t H, int32_t W, int32_t node_capacity, int32_t edge_capacity) {
  return B >= 1 && B <= (1 << 20) && H >= 1 && W >= 1 && (int64_t)H * W <= kMaxPixels && node_capacity >= 1 &&
         node_capacity <= kMaxNodes && edge_capacity >= 1 && edge_capacity <= kMaxEdges;
}

}  // namespace

extern "C" size_t gnc_rag_batched_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t node_capacity,
                                                  int32_t edge_capacity) {
  if (!supported(B, H, W, node_capacity, edge_capacity)) {
    gnc::set_error("gnc_rag_batched_workspace_bytes: %d images of %d x %d at %d nodes / %d edges is outside the supported set "
                   "(H*W <= %d, node_capacity <= %d, edge_capacity <= %d)",
                   B, H, W, node_capacity, edge_capacity, kMaxPixels, kMaxNodes, kMaxEdges);
    return 0;
  }
  return kWorkspaceBytes;
}

extern "C" int gnc_rag_build_batched(const int32_t* labels, const uint8_t* img, int32_t B, int32_t H, int32_t W,
                                     int32_t node_capacity, int32_t edge_capacity, float* x, float* pos,
                                     int64_t* edge_index, int32_t* counts, void* workspace, size_t workspace_bytes,
                                     void* stream_) {
  GNC_REQUIRE(supported(B, H, W, node_capacity, edge_capacity),
              "gnc_rag_build_batched: %d images of %d x %d at %d nodes / %d edges is outside the supported set", B, H, W,
              node_capacity, edge_capacity);
  GNC_REQUIRE(labels && img && x && pos && edge_index && counts, "gnc_rag_build_batched: null pointer");
  if (!workspace || workspace_bytes < kWorkspaceBytes) {
    gnc::set_error("gnc_rag_build_batched: workspace too small");
    return GNC_ERR_WORKSPACE;
  }
  rag_batched_kernel<<<B, kThreads, 0, (hipStream_t)stream_>>>(labels, img, H, W, node_capacity, edge_capacity, x, pos,
                                                               edge_index, counts);
  return gnc::check_launch("rag_batched_kernel");
}
