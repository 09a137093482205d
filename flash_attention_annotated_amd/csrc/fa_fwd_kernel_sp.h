// fa_fwd_kernel_sp.h — gfx950 block-sparse forward over a KV cache (fa_fwd_sparse_kv, include/fa_fwd.h): a decode / verify /
// ragged serving step that reads only the key blocks a selection step listed per kv head (Quest-style page selection, NSA-style
// selected blocks shared by a GQA group).
//
// sp_fwd_kernel is packed_rows_fwd (fa_fwd_kernel_pk.h) with the walk policy ListWalk in place of RangeWalk: the work shape
// (a block of (query row, head of the GQA group) pairs of ONE kv head per workgroup), the dense / paged staging, the tile step
// (fa_fwd_tile_step.h), the masks and the epilogue are pk_fwd_kernel's / kv8_fwd_kernel's code, not a copy of it, and the tile
// policy KV is theirs: Kv16<T, D> for a 16-bit cache, Kv8<T, D> for an e4m3 cache (descales as fa_fwd_kv8).  What ListWalk
// changes is said at its definition and at every `WALK::SPARSE` in packed_rows_fwd:
//   * the tiles come from the list (entry t / sub, sub-tile t % sub), in list order, one entry prefetched ahead;
//   * an entry outside [0, ceil(sk / block_size)) or a tile outside the block's key range is passed over before any load;
//   * split-KV partitions list positions; an empty part writes LSE = -inf when another part may hold a listed key of the row,
//     +inf when no listed key is visible to the row at all (fa_fwd_combine's convention, for both cache types);
//   * seqused_k is clamped to the capacity for both cache types; no cu_seqlens_k and no sink (fa_fwd_sparse_kv_validate).
// The element masks stay the lane's [lim_lo, lim_hi) by logical key position, so a listed block that straddles sk, the diagonal
// or a window edge is masked like any boundary tile.
#pragma once

#include "fa_fwd_kernel_kv8.h"

namespace fa {

struct SpParams {
    PkParams pk;
    ListWalk walk;
};

template <typename T, int D, bool SOFTCAP, typename KV>
__global__ __launch_bounds__(PK_NWAVES * 64, 2) void sp_fwd_kernel(const SpParams sa) {
    packed_rows_fwd<T, D, SOFTCAP, KV, ListWalk>(sa.pk, sa.walk);
}

}  // namespace fa
