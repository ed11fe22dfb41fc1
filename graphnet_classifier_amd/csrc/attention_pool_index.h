// Index arithmetic of K19 (csrc/attention_pool.hip) that K17's pool_index.h does not have: the workspace layout of the split
// regime and the tiling of the backward launch.  Host-compilable like pool_index.h, so that tools/attention_pool_index_check.cpp
// can walk every (workgroup, thread) of the launches and check each address before a kernel runs on a device.
#pragma once
#include "pool_index.h"

namespace gnc_attn {

// Split regime: the workspace holds the chunks' weighted column sums [slots, C] in front and their partial Z [slots] behind.
GNC_POOL_HD int64_t workspace_floats(int64_t slots, int64_t C) { return slots * (C + 1); }
GNC_POOL_HD int64_t ws_col_index(int64_t slot, int64_t C, int64_t c) { return slot * C + c; }
GNC_POOL_HD int64_t ws_z_index(int64_t slots, int64_t C, int64_t slot) { return slots * C + slot; }

// Backward: `lanes` threads side by side own ONE row (a power of two <= 64, so a row never straddles a wavefront), each `vec`
// consecutive columns at a time (4 when C is a multiple of 4); lane l takes the column groups l, l + lanes, ... in ascending order
// and the lanes' partial dot products are folded by a butterfly (lane l += lane l ^ s for s = lanes / 2, ..., 1).  A function of
// C ALONE: it fixes the order of the dot over C.
struct RowGeometry {
  int vec, lanes, rows_per_block;
};

GNC_POOL_HD RowGeometry row_geometry(int64_t C) {
  RowGeometry g;
  g.vec = (C % 4 == 0) ? 4 : 1;
  const int64_t per_row = C / g.vec;  // column groups of a row (vec 1: C itself)
  int lanes = 1;
  while (lanes < 64 && lanes < per_row) lanes <<= 1;
  g.lanes = lanes;
  g.rows_per_block = gnc_pool::kBlockThreads / lanes;
  return g;
}

}  // namespace gnc_attn
