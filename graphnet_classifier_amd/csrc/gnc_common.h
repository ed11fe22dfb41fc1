// Internal helpers shared by the HIP translation units of libgnc_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gnc_hip.h"

namespace gnc {

void set_error(const char* fmt, ...);  // thread-local message behind gnc_last_error_string()

inline int check_hip(hipError_t e, const char* what) {
  if (e == hipSuccess) return GNC_OK;
  set_error("%s: %s", what, hipGetErrorString(e));
  return GNC_ERR_HIP;
}

// Launch check: kernels are enqueued asynchronously, so this only catches launch-time
// failures (bad configuration, missing code object), never synchronises.
inline int check_launch(const char* kernel) { return check_hip(hipGetLastError(), kernel); }

constexpr int kWave = 64;        // gfx950 wavefront
constexpr int kNumCUMax = 256;   // MI355X in SPX mode; a partitioned device (CPX/DPX) shows fewer
// Compute units of the CURRENT device, queried once per device (persistent grids are sized from it).
int num_cu();
constexpr int kBlock = 256;      // default workgroup: 4 waves, one per SIMD

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// `bytes` is a power of two; a null pointer is aligned to everything
inline bool aligned_to(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }
inline bool aligned16(const void* p) { return aligned_to(p, 16); }
// Grid of a grid-stride launch: ceil(work / per_block) workgroups, at most `per_cu` for each compute unit and at least one
// (callers with no work at all return before they launch).
inline int64_t capped_blocks(int64_t work, int64_t per_block, int per_cu = 8) {
  const int64_t blocks = ceil_div(work, per_block), cap = (int64_t)per_cu * num_cu();
  return blocks > cap ? cap : (blocks < 1 ? 1 : blocks);
}

}  // namespace gnc

#define GNC_REQUIRE(cond, ...)                 \
  do {                                         \
    if (!(cond)) {                             \
      gnc::set_error(__VA_ARGS__);             \
      return GNC_ERR_INVALID_ARGUMENT;         \
    }                                          \
  } while (0)
