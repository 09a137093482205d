/*
 * fa_block_select.h -- C ABI of the producer half of block-sparse decode over a KV cache (csrc/fa_block_select.hip): the per-block
 * summaries of the keys, kept up to date on append, and the Quest selection (Tang et al., "Quest: Query-Aware Sparsity for
 * Efficient Long-Context LLM Inference", arXiv 2406.10774) that turns them and a step's queries into the lists kv_block_cnt /
 * kv_block_idx the sparse read (fa_fwd_sparse_kv of fa_fwd.h) takes.  Not in the reference.  A unit of its own: every header of
 * include/ declares one unit, and the symbol set of each is what it was.  Status codes, dtype codes and fa_strerror are those of
 * fa_fwd.h.
 *
 * B = block_size, a multiple of 64.  g = h / h_k.  Every fill level is clamped: below 0 counts as 0, above the capacity as the
 * capacity.  n(b) = ceil(sk(b) / B).
 *
 * ---- 1. summaries ----------------------------------------------------------------------------------------------------------------
 * k_summary (slots, max_blocks, 2, h_k, d), of the 16-bit dtype of the queries, last dimension contiguous, the others by stride:
 * [s, j, 0, hk, c] is the minimum and [s, j, 1, hk, c] the maximum of channel c of KV head hk over the filled rows of block j of
 * slot s.  Dense cache (slots_cache, capacity, h_k, d): batch entry b uses slot cache_batch_idx[b] (b without it) of the cache and
 * of the summary.  Paged cache (pages, page_size, h_k, d) behind page_table (b, capacity / page_size): the summary slot is b and
 * blocks are logical, so any page size serves and a block may span pages.  max_blocks * B >= capacity (FA_ERR_BAD_SHAPE).
 * The cache is of the summary's dtype, or e4m3: then the stored byte's value, converted exactly, without a descale (a positive
 * factor per (b, hk) changes no ranking).  Minimum and maximum are exact.  NaN keys are not legal.
 *
 * fa_block_summary_update: one launch, in place.  Rows [old(b), new(b)) were just written (seqlens_old NULL: 0, a rebuild;
 * old > new counts as an empty range, which touches nothing).  For every block j that meets the range: where old <= j * B the
 * summary is SET from rows [j * B, min(new, (j + 1) * B)); else the stored summary is MERGED with rows [old, min(new, (j + 1) * B)).
 * Blocks outside the range are not written.  max_seqlen_new bounds new - old and sizes the grid (ceil(max_seqlen_new / B) + 1
 * blocks per entry, max_blocks at the most); rows beyond it are the caller's duty.  One workgroup writes one (slot, block, head):
 * no atomics, the same bits every time.  Two batch entries on one slot are the caller's duty.  Nothing is read on the host.
 * cache_leftpad and cu_seqlens_k_new must be NULL (FA_ERR_UNSUPPORTED): the two fill-level tensors already describe a ragged step.
 *
 * ---- 2. selection ----------------------------------------------------------------------------------------------------------------
 * q (b, s_q, h, d), fp16 / bf16 like k_summary; d a multiple of 16, at most 128; 1 <= s_q * g <= 128.  sk(b) = cache_seqlens[b],
 * clamped to max_blocks * B.  The summary slot of b is cache_batch_idx[b], or b.
 *   score    row i, head hd of the group of hk:  U = sum_c max(q_c * min_c, q_c * max_c), every product exact in fp32, the sum in
 *            fp32 in an order that the call's form fixes.  u[b, hk, j] reduces U over the s_q * g rows: the maximum
 *            (FA_BLOCK_REDUCE_MAX) or the fp32 sum (FA_BLOCK_REDUCE_SUM).  No softmax scale and no descale: a monotone rescale
 *            can turn distinct scores into ties.
 *   choice   K = min(num_blocks, n).  Blocks j < min(sink_blocks, n) and j >= n - local_blocks are forced.  The other
 *            K - |forced| places go to the unforced blocks of the highest u; of equal ones the lower index wins; -0 equals +0.
 *   lists    block_cnt[b, hk] = K; block_idx[b, hk, :K] the chosen blocks ascending, [K:list_width) = -1.  n = 0: a count of 0.
 *   scores   (b, h_k, max_blocks) fp32 holds u, and -inf at and behind n(b): an output, and what orders the two launches.
 * num_blocks >= sink_blocks + local_blocks and list_width >= num_blocks (FA_ERR_BAD_SHAPE).  max_blocks <= FA_BLOCK_SELECT_MAX_BLOCKS.
 * Summaries of blocks >= n(b) are never read.  With finite inputs the result is a function of the arguments alone (no atomics on
 * the result, no sort).  With NaN the choice is unspecified, but every index written is in [0, n) or -1, and nothing outside the
 * tensors is read.  cu_seqlens_q and cache_leftpad must be NULL (FA_ERR_UNSUPPORTED).
 *
 * Two launches, ordered by the stream.  block_score_kernel: grid (ceil(max_blocks / chunk), h_k, b) -- one (b, hk) is spread over
 * as many workgroups as its summaries have chunks, so batch 1 fills the chip -- streams the summaries by 16-byte loads and
 * writes `scores`.  block_select_kernel: one workgroup per (b, hk) finds the cut by a radix descent over the order-preserving
 * keys of the scores (4 passes of 8 bits, histograms in LDS), then the ties by index, and compacts the chosen blocks in
 * ascending order by a workgroup scan.  Nothing is read on the host; no allocation; HIP-graph capturable.
 *
 * Alignment (FA_ERR_BAD_STRIDE): q, k_summary and a 16-bit cache are 16-byte aligned with strides that are multiples of 8
 * elements; an e4m3 cache is 8-byte aligned with strides that are multiples of 8; int32 / fp32 tensors keep 4 bytes.
 */
#ifndef FA_BLOCK_SELECT_H_
#define FA_BLOCK_SELECT_H_

#include "fa_fwd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_BLOCK_REDUCE_MAX 0
#define FA_BLOCK_REDUCE_SUM 1
#define FA_BLOCK_SELECT_MAX_BLOCKS 8192
#define FA_BLOCK_SELECT_MAX_ROWS 128 /* s_q * g */

typedef struct fa_block_summary_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    void *k_summary;                 /* (slots, max_blocks, 2, h_k, d) of summary_dtype */
    const void *k_cache;             /* (slots, capacity, h_k, d), or pages (num_pages, page_size, h_k, d) */
    const int32_t *seqlens_old;      /* (b), or NULL: 0 */
    const int32_t *seqlens_new;      /* (b) */
    const int32_t *cache_batch_idx;  /* (b), or NULL; dense caches only */
    const int32_t *page_table;       /* (b, capacity / page_size), or NULL */
    const int32_t *cache_leftpad;    /* must be NULL */
    const int32_t *cu_seqlens_k_new; /* must be NULL */
    int64_t sum_slot_stride, sum_block_stride, sum_side_stride, sum_head_stride; /* in elements */
    int64_t cache_batch_stride, cache_row_stride, cache_head_stride;             /* in elements (e4m3: bytes) */
    int64_t page_table_batch_stride;
    int32_t b;
    int32_t capacity; /* rows a batch entry can hold: the dense cache's length, or pages per entry * page_size */
    int32_t h_k, d;
    int32_t max_blocks;
    int32_t block_size;
    int32_t page_size; /* with page_table */
    int32_t max_seqlen_new;
    int32_t summary_dtype; /* FA_DTYPE_FP16 / FA_DTYPE_BF16 */
    int32_t cache_dtype;   /* summary_dtype, or FA_DTYPE_FP8_E4M3 */
} fa_block_summary_params;

typedef struct fa_block_select_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *q;                  /* (b, s_q, h, d) of dtype */
    const void *k_summary;          /* (slots, max_blocks, 2, h_k, d) of dtype */
    const int32_t *cache_seqlens;   /* (b) */
    const int32_t *cache_batch_idx; /* (b), or NULL */
    const int32_t *cu_seqlens_q;    /* must be NULL */
    const int32_t *cache_leftpad;   /* must be NULL */
    float *scores;                  /* (b, h_k, max_blocks), last dimension contiguous */
    int32_t *block_cnt;             /* (b, h_k) */
    int32_t *block_idx;             /* (b, h_k, list_width), last dimension contiguous */
    int64_t q_batch_stride, q_row_stride, q_head_stride;                         /* in elements */
    int64_t sum_slot_stride, sum_block_stride, sum_side_stride, sum_head_stride; /* in elements */
    int64_t scores_batch_stride, scores_head_stride;
    int64_t cnt_batch_stride, cnt_head_stride;
    int64_t idx_batch_stride, idx_head_stride;
    int32_t b, s_q, h, h_k, d;
    int32_t max_blocks;
    int32_t list_width;
    int32_t block_size;
    int32_t num_blocks, sink_blocks, local_blocks;
    int32_t group_reduce; /* FA_BLOCK_REDUCE_* */
    int32_t dtype;        /* FA_DTYPE_FP16 / FA_DTYPE_BF16 */
    int32_t reserved;
} fa_block_select_params;

/* the checks of the launch entry without a device: FA_OK or the status the entry would return before it launches */
int fa_block_summary_update_validate(const fa_block_summary_params *params);
/* asynchronous on `stream` (a hipStream_t; NULL: the default stream); no host synchronisation, no allocation */
int fa_block_summary_update(const fa_block_summary_params *params, void *stream);
/* 0: the update needs no workspace; a negative status where the params are refused */
int64_t fa_block_summary_update_workspace_size(const fa_block_summary_params *params);
/* the form the call takes, as text: the kernel, the cache side and the grid; NULL where the params are refused.  The buffer is
 * the calling thread's and is overwritten by its next call */
const char *fa_block_summary_update_plan_name(const fa_block_summary_params *params);
uint32_t fa_block_summary_params_size(void);

int fa_block_select_validate(const fa_block_select_params *params);
int fa_block_select(const fa_block_select_params *params, void *stream);
/* the bytes `scores` spans, b * scores_batch_stride * 4 with contiguous scores: it is the workspace between the two launches and
 * the caller's to allocate; a negative status where the params are refused */
int64_t fa_block_select_workspace_size(const fa_block_select_params *params);
const char *fa_block_select_plan_name(const fa_block_select_params *params);
uint32_t fa_block_select_params_size(void);

#ifdef __cplusplus
}
#endif
#endif /* FA_BLOCK_SELECT_H_ */
