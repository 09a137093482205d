// fa_bwd_internal.h — host helpers of fa_bwd_api.hip that fa_bwd_bs_api.hip calls (not part of the C-ABI).  They keep the one
// instantiation of bwd_dot_kernel, the params filler and the last-plan text of fa_bwd_last_plan_name() in fa_bwd_api.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fa_bwd.h"

namespace fa {

struct BParams;

// fa_bwd_params (validated) -> kernel params: pointers, strides, sizes, the window normalisation, scales.  The launch fields
// (num_blocks, num_tiles, whole_slots, grid) are left to the caller.
void bwd_fill_params(const fa_bwd_params *p, BParams &bp);

// D = rowsum(dO * O) for all rows: bwd_dot_kernel<T, LPR> of head-dim tile `tile` (LPR = min(tile / 8, 32)).  FA_OK / FA_ERR_LAUNCH.
int bwd_launch_dot(const BParams &bp, int32_t dtype, int tile, hipStream_t stream);

// The launch fields of decode_block()'s grid, one work item per (batch, head, block): num_blocks = blocks, num_tiles =
// blocks * heads * b, whole_slots and grid.  FA_OK, or FA_ERR_BAD_SHAPE when a count does not fit 31 bits.
int bwd_set_grid(BParams &bp, int64_t blocks, int64_t heads);

// What fa_bwd_last_plan_name() answers for the calling thread until its next fa_bwd / fa_bwd_block_sparse; NULL or "" = nothing.
void bwd_set_last_plan_text(const char *text);

}  // namespace fa
