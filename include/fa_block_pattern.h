/*
 * fa_block_pattern.h -- C ABI of the producer of block-sparse prefill / training patterns (csrc/fa_block_pattern.hip): from q and
 * k, the lists full_block_cnt / full_block_idx / mask_block_cnt / mask_block_idx that fa_fwd_block_sparse (fa_fwd.h) reads, and
 * the key-major lists q_block_cnt / q_block_idx that fa_bwd_block_sparse (fa_bwd.h) reads: mean-pooled block scores, a top-k
 * per query block with forced sink and local blocks (the block top-k of MInference's block-sparse heads, Jiang et al., arXiv
 * 2407.02490, and of SeerAttention, Gao et al., arXiv 2410.13276).  Not in the reference.  A unit of its own: every header of
 * include/ declares one unit, and the symbol set of each is what it was.  Status codes, dtype codes and fa_strerror are those of
 * fa_fwd.h.
 *
 * B = 128, the block size of the lists.  q (b, sq, h, d), k (b, sk, h_k, d), fp16 / bf16, any strides with a unit last one; d a
 * multiple of 16, at most 128.  nm = ceil(sq / B), nk = ceil(sk / B) <= FA_BLOCK_PATTERN_MAX_BLOCKS, g = h / h_k.  Query block m
 * holds the rows [m B, min(sq, (m + 1) B)), key block n the keys [n B, min(sk, (n + 1) B)): the rows and keys "that exist".
 *
 * ---- the rule --------------------------------------------------------------------------------------------------------------------
 * 1. pooling     qs[b, h, m, c]  = the fp32 sum of channel c over the rows of query block m that exist.
 *                km[b, hk, n, c] = the fp32 sum of channel c over the keys of key block n that exist, times the fp32 value
 *                1 / count: a mean, so that a ragged last key block does not rank lower for being short.  Every addend is a
 *                16-bit value, exact in fp32.  The order of the sums is fixed by the call's form: 256 / L row groups (L = 16
 *                lanes where d > 64, else 8) each add the rows r, r + 256 / L, ... in ascending order, then the groups are added
 *                in ascending order.
 * 2. score       u[b, h, m, n] = sum_c qs[b, h, m, c] * km[b, h / g, n, c] in fp32: each lane adds its 8 channels in ascending
 *                order (fused multiply-adds), then a butterfly over the L lanes (distances L / 2, ..., 1).  No softmax scale: a
 *                monotone rescale can only create ties.  u + 0 is what counts: -0 equals +0.
 * 3. visibility  the call's own mask, bottom-right aligned as everywhere in this project: row i sees key j iff
 *                i + sk - sq - left <= j <= i + sk - sq + right; is_causal means right = 0; a negative window side means
 *                unbounded.  Block (m, n) is VISIBLE iff some pair (row of m that exists, key of n that exists) is visible.
 *                The visible blocks of a query block are consecutive.  Block (m, n) is FULL iff every such pair is visible AND
 *                all B keys of block n exist.  The second condition is what fa_fwd_block_sparse says of its full list: a full
 *                block is one that needs no element-wise mask, and the seqlen_k bound is part of that mask, so a ragged last
 *                key block never goes to the full list (a ragged last query block may: rows that do not exist are not written).
 * 4. choice      per (b, h, m): V = the visible blocks, ascending; K = min(num_blocks, |V|).  The first min(sink_blocks, |V|)
 *                and the last min(local_blocks, |V|) blocks of V are forced.  The other K - |forced| places go to the unforced
 *                blocks of V of the highest u; of equal ones the lower index wins.  num_blocks >= sink_blocks + local_blocks,
 *                both non-negative (FA_ERR_BAD_SHAPE).  |V| = 0 (the rows above the diagonal band when sq > sk): counts of 0.
 * 5. lists       the chosen full blocks go to full_block_idx[b, h, m, :full_block_cnt[b, h, m]], the other chosen blocks to
 *                mask_block_idx[b, h, m, :mask_block_cnt[b, h, m]]: indices ascending, tails [cnt, nk) zero -- the conventions
 *                of block_sparse_from_mask (cute_interface.py).  scores (b, h, nm, nk) fp32, optional, holds u + 0, and -inf at
 *                invisible blocks.  With finite inputs the result is a function of the arguments alone (no atomics on a
 *                result, no sort).  With NaN inputs the choice is unspecified, but every index written is in [0, nk) or a zero
 *                tail, and nothing outside the tensors is read.
 * 6. key-major   with q_block_cnt / q_block_idx: for every (b, h, n), q_block_idx[b, h, n, :q_block_cnt[b, h, n]] is the
 *                ascending list of the query blocks m whose chosen set holds n, full and mask blocks merged, tails [cnt, nm)
 *                zero: what block_sparse_bwd_lists (cute_interface.py) returns for the four lists above.
 *
 * ---- the launches ----------------------------------------------------------------------------------------------------------------
 * Two or three launches, ordered by the stream; nothing is read on the host, nothing is allocated: HIP-graph capturable.
 *   pool_kernel<VEC>    one workgroup of 256 threads per (b, head, block) of q and of k, grid (b h nm + b h_k nk): reads q and
 *                       k once and writes qs / km to the workspace.  VEC: 16-byte loads, where both bases are 16-byte aligned
 *                       and all strides are multiples of 8 elements; else 2-byte element loads.  No atomics.
 *   pattern_kernel      one workgroup per (m, h, b), 256 threads up to 1024 key blocks and 1024 above: qs[m] in registers
 *                       against km streamed by 16-byte loads gives the visible scores, whose order-preserving keys lie in LDS;
 *                       the cut by a radix descent (4 passes of 8 bits, histograms in LDS), the ties by index, both lists
 *                       compacted in ascending order by one workgroup scan.  With the key-major lists it also writes the
 *                       membership of row m as a bitmap of nk bits to the workspace.
 *   transpose_kernel    only with the key-major lists: one workgroup of 256 threads per (n, h, b) scans bit n of the nm rows
 *                       and compacts the set ones in ascending order.
 * workspace: fp32 qs (b, h, nm, d), fp32 km (b, h_k, nk, d), and with the key-major lists uint32 (b, h, nm, ceil(nk / 32)), each
 * part rounded up to 16 bytes; fa_block_pattern_workspace_size gives the bytes.  The caller allocates it, 16-byte aligned.
 *
 * The seven outputs are contiguous.  Alignment (FA_ERR_BAD_STRIDE): q and k keep 2 bytes, int32 / fp32 tensors 4, the workspace
 * 16.  b, h <= 65535; sq, sk >= 1.
 */
#ifndef FA_BLOCK_PATTERN_H_
#define FA_BLOCK_PATTERN_H_

#include "fa_fwd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_BLOCK_PATTERN_BLOCK 128
#define FA_BLOCK_PATTERN_MAX_BLOCKS 8192 /* nk */

typedef struct fa_block_pattern_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *q;           /* (b, sq, h, d) of dtype */
    const void *k;           /* (b, sk, h_k, d) of dtype */
    int32_t *full_block_cnt; /* (b, h, nm) */
    int32_t *full_block_idx; /* (b, h, nm, nk) */
    int32_t *mask_block_cnt; /* (b, h, nm) */
    int32_t *mask_block_idx; /* (b, h, nm, nk) */
    int32_t *q_block_cnt;    /* (b, h, nk), or NULL together with q_block_idx: no key-major lists */
    int32_t *q_block_idx;    /* (b, h, nk, nm) */
    float *scores;           /* (b, h, nm, nk), or NULL */
    void *workspace;
    uint64_t workspace_bytes;
    int64_t q_batch_stride, q_row_stride, q_head_stride; /* in elements */
    int64_t k_batch_stride, k_row_stride, k_head_stride;
    int32_t b, sq, sk, h, h_k, d;
    int32_t num_blocks, sink_blocks, local_blocks;
    int32_t is_causal;
    int32_t window_size_left, window_size_right; /* negative: unbounded */
    int32_t dtype;                               /* FA_DTYPE_FP16 / FA_DTYPE_BF16 */
    int32_t reserved;
} fa_block_pattern_params;

/* the checks of the launch entry without a device: FA_OK or the status the entry would return before it launches */
int fa_block_pattern_validate(const fa_block_pattern_params *params);
/* asynchronous on `stream` (a hipStream_t; NULL: the default stream); no host synchronisation, no allocation */
int fa_block_pattern(const fa_block_pattern_params *params, void *stream);
/* the bytes of the workspace the call needs; `workspace` and `workspace_bytes` are not looked at.  A negative status where the
 * params are refused */
int64_t fa_block_pattern_workspace_size(const fa_block_pattern_params *params);
/* the form the call takes, as text: the pooling form (16-byte or element loads), the selection's form (query blocks per
 * workgroup, the nk class as the workgroup's threads), whether the transpose runs, and the three grids; NULL where the params
 * are refused.  No device access.  The buffer is the calling thread's and is overwritten by its next call */
const char *fa_block_pattern_plan_name(const fa_block_pattern_params *params);
uint32_t fa_block_pattern_params_size(void);

#ifdef __cplusplus
}
#endif
#endif /* FA_BLOCK_PATTERN_H_ */
