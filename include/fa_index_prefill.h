/*
 * fa_index_prefill.h -- C ABI of the prefill-sized lightning indexer (csrc/fa_index_prefill.hip): the index logits of a prompt, or
 * of a chunk of a chunked prefill, against the indexer's single-head key cache, and the top-k of them per query token as the int32
 * list the token-sparse MLA decode takes.  The unit beside fa_index_topk.h, which serves steps of at most 16 query tokens and is
 * what it was; s_q <= 16 is accepted here as well and gives that entry's result.  Not in the reference.  A unit of its own.  Status
 * codes, dtype codes and fa_strerror are those of fa_fwd.h.
 *
 * The rule is the one fa_index_topk.h states, word for word -- fill, logit (with its summation order: 16 channels a step ascending
 * on the 32x32x16 matrix instruction, the head sum in the pinned in-lane order), visible, choice, lists -- so a token's logits are
 * bit-equal to what fa_index_topk computes for it, and a position's list does not depend on which call produced it.
 *
 * q_index (b, s_q, h_i, d_i), fp16 / bf16; d_i 64 or 128 (FA_ERR_BAD_HEAD_DIM); h_i a multiple of 16, at most FA_INDEX_MAX_HEADS
 * (FA_ERR_BAD_HEADS); s_q >= 1 with b * s_q < 2^31 (FA_ERR_BAD_SHAPE).  weights (b, s_q, h_i) fp32, last dimension contiguous.
 * k_index_cache: one head, of q_index's dtype (e4m3: FA_ERR_UNSUPPORTED; anything else: FA_ERR_BAD_DTYPE) -- dense (slots,
 * capacity, d_i), entry b on slot cache_batch_idx[b] (b without it), or pages (num_pages, page_size, d_i) behind page_table
 * (b, capacity / page_size) with ANY page size.  capacity <= FA_INDEX_MAX_KEYS.  indices (b, s_q, 1, list_width >= topk) int32, last
 * dimension contiguous: [b, i, 0, :K] the chosen logical positions ascending, [K:topk) = -1, [topk:list_width) untouched.
 *
 * Logits are a WORKSPACE here, not an output: workspace (workspace_rows, workspace_width >= capacity) fp32, last dimension
 * contiguous, workspace_rows >= FA_INDEX_PREFILL_BLOCK.  The tokens of a batch entry form ceil(s_q / FA_INDEX_PREFILL_BLOCK) token
 * blocks (the last one may be short); the blocks of the call are numbered (b, block) ascending.  The call runs in rounds of
 * floor(workspace_rows / FA_INDEX_PREFILL_BLOCK) blocks: the logits launch of a round writes row (block - first block of the round)
 * * FA_INDEX_PREFILL_BLOCK + (token - first token of the block), its selection launch reads it, the next round reuses the rows,
 * ordered by the stream.  Of a row only [0, n(b, i)) is defined: nothing is written at or behind n(b, i), and the selection reads
 * nothing there.  The result does not depend on workspace_rows.  With one round (fa_index_prefill_workspace_size, one_round) the
 * workspace holds every row of the call when it returns.
 *
 * Rows of the cache at or behind sk(b), and the page-table entries of pages wholly behind it, are never read; a key tile at or
 * behind the largest n of a token block is skipped without a load.  With finite inputs the result is a function of the arguments
 * alone (no atomics on results, no sort).  With NaN the choice is unspecified, but every index written is in [0, n) or -1.  Nothing
 * is read on the host; no allocation; HIP-graph capturable, and a replay sees changed fill levels.  cu_seqlens_q and cache_leftpad
 * must be NULL (FA_ERR_UNSUPPORTED).  topk >= 1, list_width >= topk, workspace_width >= capacity, capacity a multiple of page_size,
 * no cache_batch_idx with pages (FA_ERR_BAD_SHAPE).
 *
 * Two launches a round.  index_logits_prefill_kernel: one workgroup of 4 waves per (token block, chunk of keys), the heaviest
 * blocks of the round first; the block's query fragments live in registers, the key tiles stream through LDS.
 * index_select_prefill_kernel: one workgroup per token, the selection of fa_index_topk over the token's workspace row.
 *
 * Alignment (FA_ERR_BAD_STRIDE): q_index and the cache are 16-byte aligned with strides that are multiples of 8 elements;
 * int32 / fp32 tensors keep 4 bytes.
 */
#ifndef FA_INDEX_PREFILL_H_
#define FA_INDEX_PREFILL_H_

#include "fa_index_topk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_INDEX_PREFILL_BLOCK 8 /* the tokens of one workgroup's block */

typedef struct fa_index_prefill_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *q_index;            /* (b, s_q, h_i, d_i) of dtype */
    const void *k_index_cache;      /* (slots, capacity, d_i), or pages (num_pages, page_size, d_i), of cache_dtype */
    const float *weights;           /* (b, s_q, h_i), last dimension contiguous */
    const int32_t *cache_seqlens;   /* (b) */
    const int32_t *cache_batch_idx; /* (b), or NULL; dense caches only */
    const int32_t *page_table;      /* (b, capacity / page_size), or NULL */
    const int32_t *cu_seqlens_q;    /* must be NULL */
    const int32_t *cache_leftpad;   /* must be NULL */
    float *workspace;               /* (workspace_rows, workspace_width), last dimension contiguous */
    int32_t *indices;               /* (b, s_q, 1, list_width), last dimension contiguous */
    int64_t q_batch_stride, q_row_stride, q_head_stride; /* in elements */
    int64_t cache_batch_stride, cache_row_stride;        /* in elements; batch: of a slot, or of a page */
    int64_t w_batch_stride, w_row_stride;
    int64_t page_table_batch_stride;
    int64_t workspace_row_stride;
    int64_t idx_batch_stride, idx_row_stride;
    int64_t workspace_rows;
    int32_t b, s_q, h_i, d_i;
    int32_t capacity; /* rows a batch entry can hold: the dense cache's length, or pages per entry * page_size */
    int32_t page_size; /* with page_table */
    int32_t topk;
    int32_t list_width;
    int32_t workspace_width;
    int32_t is_causal;
    int32_t dtype;       /* FA_DTYPE_FP16 / FA_DTYPE_BF16 */
    int32_t cache_dtype; /* dtype */
} fa_index_prefill_params;

/* the checks of the launch entry without a device: FA_OK or the status the entry would return before it launches */
int fa_index_prefill_validate(const fa_index_prefill_params *params);
/* asynchronous on `stream` (a hipStream_t; NULL: the default stream); no host synchronisation, no allocation */
int fa_index_prefill(const fa_index_prefill_params *params, void *stream);
/* the bytes of a contiguous workspace at its least width: one_round = 0 the least the entry takes, FA_INDEX_PREFILL_BLOCK *
 * capacity * 4; otherwise what holds the call in one round, b * ceil(s_q / FA_INDEX_PREFILL_BLOCK) * FA_INDEX_PREFILL_BLOCK *
 * capacity * 4.  workspace, workspace_rows and workspace_width of the params are not looked at; a negative status where the rest
 * is refused */
int64_t fa_index_prefill_workspace_size(const fa_index_prefill_params *params, int32_t one_round);
/* the form the call takes, as text: both kernels, the token block, the key chunk, the grids of the first round and the number of
 * rounds; NULL where the params are refused.  The buffer is the calling thread's and is overwritten by its next call */
const char *fa_index_prefill_plan_name(const fa_index_prefill_params *params);
uint32_t fa_index_prefill_params_size(void);

#ifdef __cplusplus
}
#endif
#endif /* FA_INDEX_PREFILL_H_ */
