/*
 * fa_index_topk.h -- C ABI of the lightning indexer of DeepSeek-V3.2-style sparse attention (csrc/fa_index_topk.hip): the index
 * logits of a decode or verify step against the indexer's own single-head key cache, and the top-k of them per query token as
 * the int32 list the token-sparse MLA decode (fa_fwd_topk_kv of fa_fwd.h) takes.  Not in the reference.  A unit of its own: every
 * header of include/ declares one unit, and the symbol set of each is what it was.  Status codes, dtype codes and fa_strerror
 * are those of fa_fwd.h.
 *
 * q_index (b, s_q, h_i, d_i), fp16 / bf16; d_i 64 or 128 (FA_ERR_BAD_HEAD_DIM); h_i a multiple of 16, at most FA_INDEX_MAX_HEADS
 * (FA_ERR_BAD_HEADS); 1 <= s_q <= FA_INDEX_MAX_ROWS (FA_ERR_BAD_SHAPE): a decode, MTP or verify step.  weights (b, s_q, h_i) fp32,
 * last dimension contiguous: the caller folds the softmax scale and any h_i^-0.5 into it.  k_index_cache: one head, of q_index's
 * dtype (e4m3: FA_ERR_UNSUPPORTED; anything else: FA_ERR_BAD_DTYPE) -- dense (slots, capacity, d_i), entry b on slot
 * cache_batch_idx[b] (b without it), or pages (num_pages, page_size, d_i) behind page_table (b, capacity / page_size) with ANY page
 * size.  The last dimension is contiguous, the others go by stride.  capacity <= FA_INDEX_MAX_KEYS.
 *
 *   fill      sk(b) = cache_seqlens[b], clamped to [0, capacity].
 *   logit     L[b, i, s] = sum_j weights[b, i, j] * max(0, q_index[b, i, j, :] . k_index[b, s, :]).  The dot product accumulates
 *             in fp32 on the matrix pipe, 16 channels a step in ascending order.  The head sum is in fp32, in this order: a lane
 *             adds the terms of the heads 32 m + 8 e + 4 f + r for m, then e = 0..3, then r = 0..3 ascending, f = 0 or 1 fixed;
 *             then the sums of f = 0 and f = 1 are added.  (Heads behind h_i count as +0.)  -0 is stored as +0.
 *   visible   n(b, i) = sk(b) without is_causal; with it clamp(sk(b) - (s_q - 1 - i), 0, sk(b)): bottom-right aligned.  Key s is a
 *             candidate of token i iff s < n(b, i).
 *   choice    K = min(topk, n(b, i)) candidates of the highest L; of equal logits the lower position wins; -0 equals +0.
 *   lists     indices (b, s_q, 1, list_width >= topk) int32, last dimension contiguous: [b, i, 0, :K] the chosen LOGICAL positions
 *             ascending, [K:topk) = -1, [topk:list_width) untouched.  Ascending order is part of the contract: it makes "all
 *             listed" the dense walk.
 *   logits    (b, s_q, logits_width >= capacity) fp32, last dimension contiguous: [b, i, :capacity] holds L, and -inf at and behind
 *             n(b, i); [capacity:logits_width) untouched.  An output, and the workspace that orders the two launches: the caller's
 *             to allocate (fa_index_topk_workspace_size).
 * Rows of the cache at or behind sk(b), and the page-table entries of pages wholly behind it, are never read.  With finite inputs
 * the result is a function of the arguments alone (no atomics on results, no sort).  With NaN the choice is unspecified, but
 * every index written is in [0, n) or -1, and nothing outside the tensors is read.  Nothing is read on the host; no allocation;
 * HIP-graph capturable, and a replay sees changed fill levels.  cu_seqlens_q and cache_leftpad must be NULL (FA_ERR_UNSUPPORTED).
 * topk >= 1, list_width >= topk, logits_width >= capacity, capacity a multiple of page_size, no cache_batch_idx with pages
 * (FA_ERR_BAD_SHAPE).
 *
 * Two launches, ordered by the stream.  index_logits_kernel: grid (ceil(capacity / chunk), b) -- one batch entry is spread over
 * as many workgroups as its capacity has chunks, so batch 1 fills the chip; a workgroup whose chunk starts at or behind sk(b)
 * writes its -inf and loads no key.  index_select_kernel: one workgroup per (b, i) finds the cut by a radix descent over the
 * order-preserving keys of the logits (4 passes of 8 bits, histograms in LDS, the row re-read from L2), then the ties by index,
 * and compacts the chosen positions in ascending order.
 *
 * Alignment (FA_ERR_BAD_STRIDE): q_index and the cache are 16-byte aligned with strides that are multiples of 8 elements;
 * int32 / fp32 tensors keep 4 bytes.
 */
#ifndef FA_INDEX_TOPK_H_
#define FA_INDEX_TOPK_H_

#include "fa_fwd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_INDEX_MAX_KEYS 131072
#define FA_INDEX_MAX_HEADS 64
#define FA_INDEX_MAX_ROWS 16 /* s_q */

typedef struct fa_index_topk_params {
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
    float *logits;                  /* (b, s_q, logits_width), last dimension contiguous */
    int32_t *indices;               /* (b, s_q, 1, list_width), last dimension contiguous */
    int64_t q_batch_stride, q_row_stride, q_head_stride; /* in elements */
    int64_t cache_batch_stride, cache_row_stride;        /* in elements; batch: of a slot, or of a page */
    int64_t w_batch_stride, w_row_stride;
    int64_t page_table_batch_stride;
    int64_t logits_batch_stride, logits_row_stride;
    int64_t idx_batch_stride, idx_row_stride;
    int32_t b, s_q, h_i, d_i;
    int32_t capacity; /* rows a batch entry can hold: the dense cache's length, or pages per entry * page_size */
    int32_t page_size; /* with page_table */
    int32_t topk;
    int32_t list_width;
    int32_t logits_width;
    int32_t is_causal;
    int32_t dtype;       /* FA_DTYPE_FP16 / FA_DTYPE_BF16 */
    int32_t cache_dtype; /* dtype */
} fa_index_topk_params;

/* the checks of the launch entry without a device: FA_OK or the status the entry would return before it launches */
int fa_index_topk_validate(const fa_index_topk_params *params);
/* asynchronous on `stream` (a hipStream_t; NULL: the default stream); no host synchronisation, no allocation */
int fa_index_topk(const fa_index_topk_params *params, void *stream);
/* the bytes `logits` spans when contiguous at its least width, b * s_q * capacity * 4: the workspace between the two launches
 * and the caller's to allocate; a negative status where the params are refused */
int64_t fa_index_topk_workspace_size(const fa_index_topk_params *params);
/* the form the call takes, as text: both kernels, the chunk and the grid; NULL where the params are refused.  The buffer is the
 * calling thread's and is overwritten by its next call */
const char *fa_index_topk_plan_name(const fa_index_topk_params *params);
uint32_t fa_index_topk_params_size(void);

#ifdef __cplusplus
}
#endif
#endif /* FA_INDEX_TOPK_H_ */
