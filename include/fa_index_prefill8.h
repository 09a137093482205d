/*
 * fa_index_prefill8.h -- C ABI of the prefill-sized lightning indexer over an fp8 (OCP e4m3fn) index-key cache with one fp32 scale
 * per token (csrc/fa_index_prefill8.hip): the index logits of a prompt, or of a chunk of a chunked prefill, against the cache
 * fa_index_append8 fills, and the top-k of them per query token.  The unit beside fa_index_prefill.h (16-bit caches) and
 * fa_index_topk8.h (steps of at most 16 query tokens over this cache), both what they were.  Not in the reference.  A unit of its
 * own.  Status codes, dtype codes and fa_strerror are those of fa_fwd.h.
 *
 * The cache format -- k_index_cache, k_index_scale, the key at a position -- is the one fa_index_topk8.h defines, and so is the
 * rule, word for word: fill, logit (with its summation order: step 2 m + e takes the channels 32 m + 8 e + [0, 8) and 32 m + 16 +
 * 8 e + [0, 8) on the 32x32x16 matrix instruction, the head sum in the pinned in-lane order, the scale multiplying that sum once
 * in fp32, -0 stored as +0), visible, choice, lists.  A token's logits are bit-equal to what fa_index_topk8 computes for it, and a
 * position's list does not depend on which call produced it.
 *
 * The call is fa_index_prefill's: q_index (b, s_q, h_i, d_i) fp16 / bf16, NOT quantised, d_i 64 or 128, h_i a multiple of 16 at
 * most FA_INDEX_MAX_HEADS, any s_q >= 1 with b * s_q < 2^31; weights (b, s_q, h_i) fp32; indices (b, s_q, 1, list_width >= topk)
 * int32; the logits a WORKSPACE (workspace_rows >= FA_INDEX_PREFILL_BLOCK, workspace_width >= capacity) fp32 the call walks in
 * rounds of floor(workspace_rows / FA_INDEX_PREFILL_BLOCK) token blocks, row (block - first block of the round) *
 * FA_INDEX_PREFILL_BLOCK + (token - first token of the block), of which only [0, n(b, i)) is written and read.  The result does
 * not depend on workspace_rows; with one round the workspace holds every row of the call when it returns.
 *
 * The differences from fa_index_prefill_validate are fa_index_topk8_validate's: cache_dtype must be FA_DTYPE_FP8_E4M3 (a 16-bit
 * cache is fa_index_prefill's: FA_ERR_UNSUPPORTED; anything else FA_ERR_BAD_DTYPE); k_index_scale must not be NULL
 * (FA_ERR_NULL_POINTER) and keeps 4 bytes, scale_batch_stride >= 0, and the cache is 16-byte aligned with row and batch strides
 * that are multiples of 16 bytes (FA_ERR_BAD_STRIDE).
 *
 * Rows of the cache and of the scales at or behind sk(b), and the page-table entries of pages wholly behind it, are never read; a
 * key tile at or behind the largest n of a token block is skipped without a load.  With finite inputs the result is a function of
 * the arguments alone.  Nothing is read on the host; no allocation; HIP-graph capturable, and a replay sees changed fill levels.
 *
 * Two launches a round.  index_logits_prefill8_kernel: one workgroup of 4 waves per (token block, chunk of keys), the heaviest
 * blocks of the round first; the block's query fragments live in registers in the permuted channel order, the key tiles of
 * FA_INDEX_PREFILL8_TILE rows stream through LDS as BYTES with their scales and are expanded to 16 bits at the matrix operand.
 * index_select_prefill_kernel: one workgroup per token, the selection of fa_index_topk over the token's workspace row.
 */
#ifndef FA_INDEX_PREFILL8_H_
#define FA_INDEX_PREFILL8_H_

#include "fa_index_prefill.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_INDEX_PREFILL8_TILE 128 /* the key rows of one tile in LDS */

/* fa_index_prefill_params' fields, and the scales with their batch stride */
typedef struct fa_index_prefill8_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *q_index;            /* (b, s_q, h_i, d_i) of dtype */
    const void *k_index_cache;      /* (slots, capacity, d_i), or pages (num_pages, page_size, d_i), e4m3 bytes */
    const float *weights;           /* (b, s_q, h_i), last dimension contiguous */
    const int32_t *cache_seqlens;   /* (b) */
    const int32_t *cache_batch_idx; /* (b), or NULL; dense caches only */
    const int32_t *page_table;      /* (b, capacity / page_size), or NULL */
    const int32_t *cu_seqlens_q;    /* must be NULL */
    const int32_t *cache_leftpad;   /* must be NULL */
    float *workspace;               /* (workspace_rows, workspace_width), last dimension contiguous */
    int32_t *indices;               /* (b, s_q, 1, list_width), last dimension contiguous */
    const float *k_index_scale;     /* (slots, capacity) or (num_pages, page_size), last dimension contiguous */
    int64_t q_batch_stride, q_row_stride, q_head_stride; /* in elements */
    int64_t cache_batch_stride, cache_row_stride;        /* in bytes; batch: of a slot, or of a page */
    int64_t w_batch_stride, w_row_stride;
    int64_t page_table_batch_stride;
    int64_t workspace_row_stride;
    int64_t idx_batch_stride, idx_row_stride;
    int64_t workspace_rows;
    int64_t scale_batch_stride; /* in elements; of a slot, or of a page */
    int32_t b, s_q, h_i, d_i;
    int32_t capacity; /* rows a batch entry can hold: the dense cache's length, or pages per entry * page_size */
    int32_t page_size; /* with page_table */
    int32_t topk;
    int32_t list_width;
    int32_t workspace_width;
    int32_t is_causal;
    int32_t dtype;       /* of q_index: FA_DTYPE_FP16 / FA_DTYPE_BF16 */
    int32_t cache_dtype; /* FA_DTYPE_FP8_E4M3 */
} fa_index_prefill8_params;

/* the checks of the launch entry without a device: FA_OK or the status the entry would return before it launches */
int fa_index_prefill8_validate(const fa_index_prefill8_params *params);
/* asynchronous on `stream` (a hipStream_t; NULL: the default stream); no host synchronisation, no allocation */
int fa_index_prefill8(const fa_index_prefill8_params *params, void *stream);
/* the bytes of a contiguous workspace at its least width, as fa_index_prefill_workspace_size: one_round = 0 the least the entry
 * takes, otherwise what holds the call in one round; a negative status where the rest of the params is refused */
int64_t fa_index_prefill8_workspace_size(const fa_index_prefill8_params *params, int32_t one_round);
/* the form the call takes, as text: both kernels, the token block, the key tile and chunk, the grids of the first round and the
 * number of rounds; NULL where the params are refused.  The buffer is the calling thread's and is overwritten by its next call */
const char *fa_index_prefill8_plan_name(const fa_index_prefill8_params *params);
uint32_t fa_index_prefill8_params_size(void);

#ifdef __cplusplus
}
#endif
#endif /* FA_INDEX_PREFILL8_H_ */
