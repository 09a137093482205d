/*
 * fa_index_topk8.h -- C ABI of the lightning indexer over an fp8 (OCP e4m3fn) index-key cache, and of the quantising append
 * that fills that cache (csrc/fa_index_topk8.hip).  Not in the reference.  A unit of its own: every header of include/ declares
 * one unit, and the symbol set of each is what it was.  Status codes, dtype codes and fa_strerror are those of fa_fwd.h; the
 * limits FA_INDEX_MAX_KEYS / _HEADS / _ROWS are those of fa_index_topk.h.
 *
 * The cache format, one definition for both entries:
 *   k_index_cache  e4m3 bytes, one head: dense (slots, capacity, d_i), entry b on slot cache_batch_idx[b] (b without it), or
 *                  pages (num_pages, page_size, d_i) behind page_table (b, capacity / page_size) with ANY page size.  d_i is 64 or
 *                  128; the last dimension is contiguous; the pointer is 16-byte aligned and the row and batch strides are
 *                  multiples of 16 bytes (an element is a byte: strides in elements are strides in bytes).
 *   k_index_scale  fp32, (slots, capacity) or (num_pages, page_size): the leading index of the cache, last dimension contiguous,
 *                  the other by scale_batch_stride.
 *   the key        at a position is k_index_scale[..] * float(k_index_cache[..]): one scale per token.  Scales are positive and
 *                  finite (the append writes powers of two).
 *
 * fa_index_topk8 -- the read.  q_index (b, s_q, h_i, d_i), fp16 / bf16, NOT quantised; h_i a multiple of 16, at most
 * FA_INDEX_MAX_HEADS (FA_ERR_BAD_HEADS); 1 <= s_q <= FA_INDEX_MAX_ROWS (FA_ERR_BAD_SHAPE).  weights (b, s_q, h_i) fp32, last
 * dimension contiguous.  cache_dtype must be FA_DTYPE_FP8_E4M3: a 16-bit cache is fa_index_topk's (FA_ERR_UNSUPPORTED here);
 * anything else FA_ERR_BAD_DTYPE.  capacity <= FA_INDEX_MAX_KEYS.
 *
 *   fill      sk(b) = cache_seqlens[b], clamped to [0, capacity].
 *   logit     L[b, i, s] = scale[b, s] * sum_j weights[b, i, j] * max(0, q_index[b, i, j, :] . k8[b, s, :]), k8 the bytes' values.
 *             e4m3 -> fp16 / bf16 is exact for every finite e4m3 value, so the dot product is formed on the 16-bit matrix pipe
 *             with fp32 accumulation, 16 channels a step: step 2 m + e takes the channels 32 m + 8 e + [0, 8) and 32 m + 16 + 8 e
 *             + [0, 8), m then e ascending.  The head sum is in fp32, in this order: a lane adds the terms of the heads 32 m +
 *             8 e + 4 f + r for m, then e = 0..3, then r = 0..3 ascending, f = 0 or 1 fixed; then the sums of f = 0 and f = 1 are
 *             added.  (Heads behind h_i count as +0.)  The scale multiplies that sum once, in fp32.  -0 is stored as +0.
 *   visible   n(b, i) = sk(b) without is_causal; with it clamp(sk(b) - (s_q - 1 - i), 0, sk(b)): bottom-right aligned.  Key s is a
 *             candidate of token i iff s < n(b, i).
 *   choice    K = min(topk, n(b, i)) candidates of the highest L; of equal logits the lower position wins; -0 equals +0.
 *   lists     indices (b, s_q, 1, list_width >= topk) int32, last dimension contiguous: [b, i, 0, :K] the chosen LOGICAL positions
 *             ascending, [K:topk) = -1, [topk:list_width) untouched.
 *   logits    (b, s_q, logits_width >= capacity) fp32, last dimension contiguous: [b, i, :capacity] holds L, and -inf at and behind
 *             n(b, i); [capacity:logits_width) untouched.  An output, and the workspace that orders the two launches: the caller's
 *             to allocate (fa_index_topk8_workspace_size).
 * Rows of the cache and of the scales at or behind sk(b), and the page-table entries of pages wholly behind it, are never read.
 * With finite inputs the result is a function of the arguments alone.  With a NaN byte or query, or a scale that is not positive
 * and finite, the choice is unspecified, but every index written is in [0, n) or -1, and nothing outside the tensors is touched.
 * Nothing is read on the host; no allocation; HIP-graph capturable, and a replay sees changed fill levels.  cu_seqlens_q and
 * cache_leftpad must be NULL (FA_ERR_UNSUPPORTED).  topk >= 1, list_width >= topk, logits_width >= capacity, capacity a multiple
 * of page_size, no cache_batch_idx with pages (FA_ERR_BAD_SHAPE).  Alignment (FA_ERR_BAD_STRIDE): q_index is 16-byte aligned with
 * strides that are multiples of 8 elements; the cache as above; int32 / fp32 tensors keep 4 bytes; scale_batch_stride >= 0.
 *
 * Two launches, ordered by the stream.  index_logits8_kernel: grid (ceil(capacity / chunk), b), chunk 256 keys doubled up to 1024
 * while the grid would exceed 1024 workgroups; a wave owns tiles of 64 key rows it loads as bytes, 32 contiguous bytes per row and
 * load instruction, and expands in registers once per tile.  index_select_kernel: one workgroup per (b, i), the radix descent of
 * fa_index_topk.h over the row of logits.
 *
 * fa_index_append8 -- the write.  New rows k_index_new, fp16 / bf16: (b, s_new, d_i) by new_batch_stride / new_row_stride, or
 * (total_new, d_i) with cu_seqlens_k_new (b + 1), entry b's rows [cu[b], cu[b + 1]).  Row i of entry b lands at position
 * cache_seqlens[b] + i, through cache_batch_idx or page_table; a position outside [0, capacity) is dropped.  Per row:
 *   scale     amax = max |x|;  scale = 2^e, e the smallest integer with amax * 2^-e <= 448, clamped to [-126, 127]; amax = 0
 *             gives scale = 1.  e comes from the exponent and mantissa bits of amax by integer logic.
 *   bytes     e4m3fn_rne(x / scale): the scaling is exact and the quotient always in range.
 * A non-finite x leaves its row's bytes and scale unspecified; nothing else is written.  seqused_out (b) int32 receives
 * min(cache_seqlens[b] + new rows of b, capacity); cache_seqlens is not modified and must not be seqused_out.  One launch, no
 * host synchronisation, no allocation, no atomics; HIP-graph capturable.  The new rows are 16-byte aligned with strides that are
 * multiples of 8 elements; the cache is 8-byte aligned with strides that are multiples of 8 bytes (FA_ERR_BAD_STRIDE).  Any
 * rotary embedding is applied by the caller beforehand.
 */
#ifndef FA_INDEX_TOPK8_H_
#define FA_INDEX_TOPK8_H_

#include "fa_index_topk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fa_index_topk_params' fields, and the scales with their batch stride */
typedef struct fa_index_topk8_params {
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
    float *logits;                  /* (b, s_q, logits_width), last dimension contiguous */
    int32_t *indices;               /* (b, s_q, 1, list_width), last dimension contiguous */
    const float *k_index_scale;     /* (slots, capacity) or (num_pages, page_size), last dimension contiguous */
    int64_t q_batch_stride, q_row_stride, q_head_stride; /* in elements */
    int64_t cache_batch_stride, cache_row_stride;        /* in bytes; batch: of a slot, or of a page */
    int64_t w_batch_stride, w_row_stride;
    int64_t page_table_batch_stride;
    int64_t logits_batch_stride, logits_row_stride;
    int64_t idx_batch_stride, idx_row_stride;
    int64_t scale_batch_stride; /* in elements; of a slot, or of a page */
    int32_t b, s_q, h_i, d_i;
    int32_t capacity; /* rows a batch entry can hold: the dense cache's length, or pages per entry * page_size */
    int32_t page_size; /* with page_table */
    int32_t topk;
    int32_t list_width;
    int32_t logits_width;
    int32_t is_causal;
    int32_t dtype;       /* of q_index: FA_DTYPE_FP16 / FA_DTYPE_BF16 */
    int32_t cache_dtype; /* FA_DTYPE_FP8_E4M3 */
} fa_index_topk8_params;

typedef struct fa_index_append8_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *k_index_new;         /* (b, s_new, d_i), or (total_new, d_i) with cu_seqlens_k_new, of dtype */
    void *k_index_cache;             /* as fa_index_topk8_params' */
    float *k_index_scale;            /* as fa_index_topk8_params' */
    const int32_t *cache_seqlens;    /* (b) */
    const int32_t *cache_batch_idx;  /* (b), or NULL; dense caches only */
    const int32_t *page_table;       /* (b, capacity / page_size), or NULL */
    const int32_t *cu_seqlens_k_new; /* (b + 1), or NULL */
    int32_t *seqused_out;            /* (b) */
    int64_t new_batch_stride, new_row_stride;     /* in elements; the batch stride is read without cu_seqlens_k_new only */
    int64_t cache_batch_stride, cache_row_stride; /* in bytes */
    int64_t scale_batch_stride;
    int64_t page_table_batch_stride;
    int32_t b;
    int32_t s_new;     /* without cu_seqlens_k_new */
    int32_t total_new; /* with cu_seqlens_k_new */
    int32_t d_i;
    int32_t capacity;
    int32_t page_size; /* with page_table */
    int32_t dtype;     /* of k_index_new: FA_DTYPE_FP16 / FA_DTYPE_BF16 */
    int32_t reserved;
} fa_index_append8_params;

/* the checks of the launch entry without a device: FA_OK or the status the entry would return before it launches */
int fa_index_topk8_validate(const fa_index_topk8_params *params);
/* asynchronous on `stream` (a hipStream_t; NULL: the default stream); no host synchronisation, no allocation */
int fa_index_topk8(const fa_index_topk8_params *params, void *stream);
/* the bytes `logits` spans when contiguous at its least width, b * s_q * capacity * 4; a negative status where the params are
 * refused */
int64_t fa_index_topk8_workspace_size(const fa_index_topk8_params *params);
/* the form the call takes, as text: both kernels, the chunk and the grid; NULL where the params are refused.  The buffer is the
 * calling thread's and is overwritten by its next call */
const char *fa_index_topk8_plan_name(const fa_index_topk8_params *params);
uint32_t fa_index_topk8_params_size(void);

int fa_index_append8_validate(const fa_index_append8_params *params);
/* asynchronous on `stream`; one launch */
int fa_index_append8(const fa_index_append8_params *params, void *stream);
/* the kernel, the rows a wave takes per pass and the grid; NULL where the params are refused.  The calling thread's buffer */
const char *fa_index_append8_plan_name(const fa_index_append8_params *params);
uint32_t fa_index_append8_params_size(void);

#ifdef __cplusplus
}
#endif
#endif /* FA_INDEX_TOPK8_H_ */
