/*
 * fa_rotary.h -- C ABI of the rotary embedding layer (csrc/fa_rotary_emb.hip): what the reference's
 * flash_attn.layers.rotary reaches through apply_rotary (flash_attn/ops/triton/rotary.py:102-185), forward and -- with
 * `conjugate` -- backward.  A header of its own: fa_fwd.h, its ABI version and the kernel set of fa_fwd_api.hip are what
 * they were.  Status codes, dtype codes and fa_strerror are those of fa_fwd.h.
 *
 *   out = rotate(x)       x, out: (b, seqlen, h, d), or (total, h, d) with cu_seqlens (b + 1 entries) and max_seqlen;
 *                         out may be x itself.  All four strides of both are in elements.
 *   cos, sin              (seqlen_ro, rotary_dim / 2), contiguous, of x's dtype or fp32 (both the same)
 *   rotary_dim            even, <= d <= 256.  interleaved: pairs (2j, 2j + 1); otherwise (j, j + rotary_dim / 2)
 *   conjugate             rotate by -sin: the gradient of the forward rotation
 *   position of row i of sequence s: off(s) + i, off = seqlen_offset, or seqlen_offsets[s] (a device tensor of b int32 or
 *                         int64 entries, read on the device only)
 *
 * A row whose position is outside [0, seqlen_ro) passes through unchanged (cos = 1, sin = 0: the reference's masked loads);
 * nothing outside the tables is read.  Rows at or past a sequence's length under cu_seqlens are not touched.  Columns at or past
 * rotary_dim are copied where out != x and left alone in place.  fp32 arithmetic, one rounding to the storage type.
 *
 * 16-bit x with tables of the same type, unit last strides, 16-byte aligned rows, d % 8 == 0 and rotary_dim % 16 == 0 take
 * 16-byte accesses (the rotation of csrc/fa_rotary.h, which the KV-cache append shares); anything else valid takes scalar
 * accesses.
 */
#ifndef FA_ROTARY_H_
#define FA_ROTARY_H_

#include "fa_fwd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fa_rotary_emb_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *x;
    void *out;
    int64_t x_batch_stride, x_row_stride, x_head_stride, x_dim_stride;         /* batch stride unread with cu_seqlens */
    int64_t out_batch_stride, out_row_stride, out_head_stride, out_dim_stride;
    const void *cos;
    const void *sin;
    const int32_t *cu_seqlens;  /* NULL: dense */
    const void *seqlen_offsets; /* NULL: every sequence at seqlen_offset */
    int64_t seqlen_offset;
    int32_t b;
    int32_t seqlen;     /* dense: rows per sequence */
    int32_t total;      /* with cu_seqlens: rows of x */
    int32_t max_seqlen; /* with cu_seqlens: > 0, no sequence is longer */
    int32_t h, d;
    int32_t rotary_dim;
    int32_t seqlen_ro;
    int32_t dtype;                /* FA_DTYPE_FP16 / FA_DTYPE_BF16 / FA_DTYPE_FP32 */
    int32_t cos_dtype, sin_dtype; /* dtype or FA_DTYPE_FP32 */
    int32_t offsets_int64;        /* seqlen_offsets holds int64 (else int32) */
    int32_t interleaved;
    int32_t conjugate;
} fa_rotary_emb_params;

/* the checks of fa_rotary_emb without a device: FA_OK or the status fa_rotary_emb would return before it launches */
int fa_rotary_emb_validate(const fa_rotary_emb_params *params);
/* asynchronous on `stream` (a hipStream_t; NULL: the default stream); no host synchronisation, no allocation */
int fa_rotary_emb(const fa_rotary_emb_params *params, void *stream);
uint32_t fa_rotary_emb_params_size(void);

#ifdef __cplusplus
}
#endif
#endif /* FA_ROTARY_H_ */
