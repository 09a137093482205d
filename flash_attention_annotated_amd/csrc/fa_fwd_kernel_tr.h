// fa_fwd_kernel_tr.h — gfx950 tree attention over a KV cache (fa_fwd_tree, include/fa_fwd.h): the verify step of speculative
// decoding with a token TREE as the draft (Medusa, EAGLE-2, SpecInfer, sequoia).  The caller has appended the sq nodes of the tree
// at the end of the cache; every node attends to the whole committed prefix and, among the draft keys, to the ones a 64-bit word
// per node names (its ancestors and itself).  A chain -- row i's word = bits 0 .. i -- is the bottom-right aligned causal mask.
//
// tr_fwd_kernel is packed_rows_fwd (fa_fwd_kernel_pk.h) with the mask policy TreeMask in place of RangeMask: the work shape (a
// block of (query row, head of the GQA group) pairs of ONE kv head per workgroup, so a 16-to-64-node tree fills its tiles g times
// over), the dense / paged staging, the range walk with its split-KV, the tile step (fa_fwd_tile_step.h) and the epilogue are
// pk_fwd_kernel's / kv8_fwd_kernel's code, not a copy of it, and the tile policy KV is theirs: Kv16<T, D> for a 16-bit cache,
// Kv8<T, D> for an e4m3 cache (descales as fa_fwd_kv8).  What TreeMask changes is said at its definition and at every
// `MASK::TREE` in packed_rows_fwd:
//   * each lane loads the word of its own QUERY row once, in front of the loop, and cuts it to the bits that name a key below sk;
//   * the key range of a block is all of [0, sk): no causal edge, no window (fa_fwd_tree_validate refuses both);
//   * a tile takes the element mask when it reaches past shift = sk - sq, i.e. holds a draft key or the end of the cache: at most
//     two tiles of the walk (sq <= 64); every tile in front of them runs the unmasked interior step;
//   * split-KV: an empty part writes LSE = -inf when the row sees a key anywhere (a non-empty prefix or a set bit), +inf when it
//     sees none at all (fa_fwd_combine's convention, for both cache types);
//   * seqused_k is clamped to the capacity for both cache types; no cu_seqlens_k and no sink.
#pragma once

#include "fa_fwd_kernel_kv8.h"

namespace fa {

struct TrParams {
    PkParams pk;
    TreeMask mask;
};

template <typename T, int D, bool SOFTCAP, typename KV>
__global__ __launch_bounds__(PK_NWAVES * 64, 2) void tr_fwd_kernel(const TrParams ta) {
    packed_rows_fwd<T, D, SOFTCAP, KV, RangeWalk, TreeMask>(ta.pk, RangeWalk(), ta.mask);
}

}  // namespace fa
