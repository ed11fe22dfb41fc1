// Index arithmetic of K19 (csrc/attention_pool.hip) that pool_index.h does not have: the workspace layout of the split regime.
// Host-compilable like pool_index.h, so that tools/attention_pool_index_check.cpp can check every workspace address before a
// kernel runs on a device.
#pragma once
#include "pool_index.h"

namespace gnc_attn {

// Split regime: the workspace holds the chunks' weighted column sums [slots, C] in front and their partial Z [slots] behind.
GNC_POOL_HD int64_t workspace_floats(int64_t slots, int64_t C) { return slots * (C + 1); }
GNC_POOL_HD int64_t ws_col_index(int64_t slot, int64_t C, int64_t c) { return slot * C + c; }
GNC_POOL_HD int64_t ws_z_index(int64_t slots, int64_t C, int64_t slot) { return slots * C + slot; }

}  // namespace gnc_attn
