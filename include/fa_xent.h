/*
 * fa_xent.h -- C ABI of the fused cross-entropy loss (csrc/fa_xent.hip): what the reference's
 * flash_attn.ops.triton.cross_entropy computes in cross_entropy_fwd_kernel / cross_entropy_bwd_kernel
 * (flash_attn/ops/triton/cross_entropy.py:25-146), with logit_scale, label smoothing, z-loss, a precomputed LSE and a
 * vocabulary split over ranks.  A header of its own: fa_fwd.h, its ABI version and the kernel sets of the other units are what
 * they were.  Status codes, dtype codes and fa_strerror are those of fa_fwd.h.
 *
 * Forward, per row r of N columns, all arithmetic in fp32, x = logits[r, :] * logit_scale:
 *   lse   = log(sum(exp(x))), by an online max / sum in one read of the row; written to lse[r].  With
 *           FA_XENT_PRECOMPUTED_LSE it is read from lse[r] instead, and of the row only the label's logit is read
 *           (valid only with smoothing == 0 and logit_scale == 1: FA_ERR_BAD_SHAPE otherwise)
 *   sum_x = sum(x), taken only when smoothing > 0
 *   lab   = labels[r] - class_start_idx
 *   labels[r] == ignore_index:  loss = z_loss = 0
 *   else, base = lse (0 with FA_XENT_SPLIT):
 *     lab in [0, N):      loss = base - smoothing * sum_x / total_classes - (1 - smoothing) * x[lab]
 *     lab outside [0, N): loss = smoothing * (base - sum_x / total_classes) (0 when smoothing == 0); logits[r, lab] is not read
 *     not split:          z_loss = lse_square_scale * lse^2, loss += z_loss
 *     split:              z_losses is not written (and may be NULL); the host adds the global lse and its z-loss
 * Backward, per element, with lse[r] as saved (under a split: the global one, which the host wrote back):
 *   d       = labels[r] == ignore_index ? 0 : dloss[r * dloss_stride]     (dloss_stride may be 0: an expanded scalar)
 *   p       = exp(x - lse) * (1 + 2 * lse_square_scale * lse);  p -= (1 - smoothing) at column lab;  p -= smoothing / total_classes
 *   dlogits = d * logit_scale * p, rounded once to the dtype of logits
 * A row with the ignore label is written as zeros WITHOUT its logits being read: padding rows may hold anything, NaN included,
 * and 0 * NaN does not leak into the gradient.  This departs from the reference, which multiplies by zero.
 * dlogits may be logits itself (the in-place backward).
 *
 * logits / dlogits: M rows of N elements of fp16, bf16 or fp32 (one dtype for both), unit column stride, a row stride in
 * elements each; dlogits rows do not overlap (row stride >= N where M > 1).  labels: int64 or int32 (labels_dtype).  losses,
 * lse, z_losses, dloss: fp32.  1 <= N < 2^31; M * N may pass 2^31: rows are addressed in 64 bits.  M == 0 is FA_OK and launches
 * nothing.  logit_scale > 0, 0 <= smoothing <= 1, total_classes >= N: FA_ERR_BAD_SHAPE otherwise.  Pointers keep the natural
 * alignment of their element (FA_ERR_BAD_STRIDE); nothing more is asked: every row is taken as an element head up to the first
 * 16-byte boundary, a body of 16-byte accesses and an element tail, so rows of any pitch and base use 16-byte accesses.  The
 * backward does so where a row of logits and the same row of dlogits have the same phase within 16 bytes (always so in place
 * and for a tensor allocated like logits); otherwise it takes element accesses.
 * No atomics: the same call gives the same bits every time.
 */
#ifndef FA_XENT_H_
#define FA_XENT_H_

#include "fa_fwd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_XENT_PRECOMPUTED_LSE 1 /* forward: lse is an input */
#define FA_XENT_SPLIT 2           /* the N columns are one rank's part of total_classes */
#define FA_XENT_LABELS_INT64 0
#define FA_XENT_LABELS_INT32 1

typedef struct fa_xent_fwd_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *logits;
    const void *labels; /* (M) */
    float *losses;      /* (M) */
    float *lse;         /* (M); read, not written, with FA_XENT_PRECOMPUTED_LSE */
    float *z_losses;    /* (M); not written and may be NULL with FA_XENT_SPLIT */
    int64_t logits_row_stride; /* in elements */
    int64_t M;
    int64_t ignore_index;
    int64_t class_start_idx; /* the vocabulary index of column 0 */
    int64_t total_classes;   /* >= N; the divisor of the smoothing term */
    int32_t N;
    int32_t logits_dtype; /* FA_DTYPE_FP16 / FA_DTYPE_BF16 / FA_DTYPE_FP32 */
    int32_t labels_dtype; /* FA_XENT_LABELS_* */
    int32_t flags;        /* FA_XENT_* */
    float smoothing;
    float logit_scale;
    float lse_square_scale;
    int32_t reserved;
} fa_xent_fwd_params;

typedef struct fa_xent_bwd_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *logits;
    const void *labels; /* (M) */
    const float *lse;   /* (M) */
    const float *dloss; /* element r at dloss[r * dloss_stride] */
    void *dlogits;      /* may be logits */
    int64_t logits_row_stride, dlogits_row_stride; /* in elements */
    int64_t dloss_stride;                          /* in elements; may be 0 */
    int64_t M;
    int64_t ignore_index;
    int64_t class_start_idx;
    int64_t total_classes;
    int32_t N;
    int32_t logits_dtype; /* of logits and dlogits */
    int32_t labels_dtype;
    int32_t flags; /* FA_XENT_SPLIT is accepted and changes nothing: lse is the global one */
    float smoothing;
    float logit_scale;
    float lse_square_scale;
    int32_t reserved;
} fa_xent_bwd_params;

/* the checks of the launch entries without a device: FA_OK or the status the entry would return before it launches */
int fa_xent_fwd_validate(const fa_xent_fwd_params *params);
int fa_xent_bwd_validate(const fa_xent_bwd_params *params);
/* asynchronous on `stream` (a hipStream_t; NULL: the default stream); no host synchronisation, no allocation */
int fa_xent_fwd(const fa_xent_fwd_params *params, void *stream);
int fa_xent_bwd(const fa_xent_bwd_params *params, void *stream);
uint32_t fa_xent_fwd_params_size(void);
uint32_t fa_xent_bwd_params_size(void);

/* The form a call takes, filled by the host function the launch itself consumes; no device.  cw: elements per body chunk (8 / 4:
 * 16-byte accesses with an element head and tail; 1: element accesses, and the one load of the lse_given kernel).  Forward:
 * grid_x workgroups walk the rows, grid_y = 1.  Backward: grid_x slabs of 1024 chunks, grid_y rows; what is beyond is walked. */
typedef struct fa_xent_plan {
    int32_t cw, grid_x, grid_y;
    int32_t lse_given; /* forward with FA_XENT_PRECOMPUTED_LSE: a thread per row */
} fa_xent_plan;
/* validate first: its status on failure, and *plan untouched.  M = 0 is valid and launches nothing: the plan then has no rows,
 * grid_x = 0 forward and grid_y = 0 backward */
int fa_xent_fwd_plan(const fa_xent_fwd_params *params, fa_xent_plan *plan);
int fa_xent_bwd_plan(const fa_xent_bwd_params *params, fa_xent_plan *plan);

#ifdef __cplusplus
}
#endif
#endif /* FA_XENT_H_ */
