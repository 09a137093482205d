/*
 * fa_dropout_norm.h -- C ABI of the fused dropout + residual-add + LayerNorm / RMSNorm (csrc/fa_dropout_norm.hip): what the
 * reference's flash_attn.ops.layer_norm reaches through dropout_layer_norm.dropout_add_ln_fwd / _bwd and their
 * parallel_residual forms (flash_attn/ops/layer_norm.py:16-108, 212-308), without the subset form.  A header of its own:
 * fa_fwd.h, its ABI version, fa_norm.h and the kernel sets of the other units are what they were.  Status codes, dtype codes
 * and fa_strerror are those of fa_fwd.h.
 *
 * Forward, per row r of N columns c, all arithmetic in fp32:
 *   h0 = x0 * rowscale[r] * colscale[c]                              (each factor optional)
 *   x  = keep0 ? h0 / (1 - p) : 0  [+ keep1 ? x1 / (1 - p) : 0]  [+ residual],  rounded once to the stream dtype
 *   mu = sum(x) / N, var = sum((x - mu)^2) / N  (RMS: no mu, var = sum(x^2) / N), of the rounded x;  rsigma = 1 / sqrt(var + eps)
 *   z0 = (x - mu) * rsigma * weight0 + bias0,  z1 = (x - mu) * rsigma * weight1 + bias1   (z1 with weight1), rounded once
 * Dropout decisions: one 32-bit avalanche (lowbias32) per group of 4 consecutive columns of a row gives the four bytes of
 * the group; an element is kept iff its byte <= floor(255 (1 - p)).  The counter of the avalanche is formed from the 64-bit
 * row, the group, the stream (0: x0, 1: x1) and a mix of rng_state = {seed, offset}; the row enters through an avalanche of
 * its own, its upper half beside the seed, so no two elements of a call share a counter by truncation.  dmask0 / dmask1
 * (1 = kept) are written only where given; the backward forms the decisions again from rng_state.
 * Backward, x being the stream the forward wrote (or its x0 where it wrote none):
 *   xhat = (x - mu) * rsigma, wdz = weight0 * dz0 [+ weight1 * dz1], c1 = sum(xhat * wdz) / N, c2 = sum(wdz) / N (RMS: no c2)
 *   dxs  = (wdz - (xhat * c1 + c2)) * rsigma [+ dx];  dresidual = dxs
 *   dx0  = keep0 ? dxs * rowscale * colscale / (1 - p) : 0,  dx1 = keep1 ? dxs / (1 - p) : 0
 *   dw0 = sum over rows of dz0 * xhat, db0 = sum of dz0 (dw1, db1 of dz1); dcolscale = sum of keep0 ? dxs * x0 * rowscale / (1 - p) : 0
 * Column sums: every workgroup owns a contiguous block of rows and writes one fp32 partial row per sum into `workspace`; a
 * second kernel adds the partial rows in a fixed order and casts.  No atomics, and the partial count is a function of M alone:
 * the same call gives the same bits every time.
 *
 * x0 / x1 / residual / z0 ...: M rows of N elements with unit column stride and a row stride in elements; dmask0 / dmask1 are
 * dense (M, N) bytes.  x1 is of x0's dtype, the residual and the stream of x0's dtype or fp32, the four weights and biases of
 * one dtype; fp16, bf16 or fp32 each.  A row of x0 and of the stream is at most FA_NORM_MAX_ROW_BYTES.  16-byte accesses where
 * N times the element size of every operand present (a mask: one byte) is a multiple of 16 and every base and row pitch is
 * 16-byte aligned; anything else valid takes element accesses.  M * N may pass 2^31: rows are addressed in 64 bits.  Rows wider
 * than 16384 columns (forward) or 8192 (backward) take one workgroup per row: M < 2^31 there (FA_ERR_BAD_SHAPE).
 * rowscale / colscale are of the one-weight form: with x1 or weight1 they are refused (FA_ERR_UNSUPPORTED).
 */
#ifndef FA_DROPOUT_NORM_H_
#define FA_DROPOUT_NORM_H_

#include "fa_norm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_DROPOUT_NORM_RMS 1 /* RMSNorm: no mu */

typedef struct fa_dropout_norm_fwd_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *x0;
    const void *x1;       /* NULL: none */
    const void *residual; /* NULL: none */
    const void *weight0;  /* (N) */
    const void *bias0;    /* (N); NULL: none */
    const void *weight1;  /* (N); NULL: no z1 */
    const void *bias1;    /* (N); NULL: none */
    const void *rowscale; /* (M); NULL: none */
    const void *colscale; /* (N); NULL: none */
    const uint64_t *rng_state; /* device {seed, offset}; read with p_dropout > 0 */
    void *z0;
    void *z1;        /* with weight1 */
    void *x;         /* the stream; NULL: not written */
    uint8_t *dmask0; /* (M, N) dense; NULL: not written; p_dropout > 0 only */
    uint8_t *dmask1; /* ... of x1 */
    float *mu;       /* (M); unread and may be NULL with FA_DROPOUT_NORM_RMS */
    float *rsigma;   /* (M) */
    int64_t x0_row_stride, x1_row_stride, residual_row_stride, z0_row_stride, z1_row_stride, x_row_stride; /* in elements */
    int64_t M;
    int32_t N;
    int32_t x0_dtype;                /* of x0 and x1 */
    int32_t residual_dtype, x_dtype; /* x0_dtype or FA_DTYPE_FP32; x_dtype is the stream's also where x is NULL */
    int32_t weight_dtype;            /* of weight0, bias0, weight1, bias1 */
    int32_t z_dtype;                 /* of z0 and z1 */
    int32_t rowscale_dtype, colscale_dtype;
    float eps;
    float p_dropout; /* 0 <= p < 1 */
    int32_t flags;   /* FA_DROPOUT_NORM_* */
    int32_t reserved;
} fa_dropout_norm_fwd_params;

typedef struct fa_dropout_norm_bwd_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *dz0;
    const void *dz1;      /* with weight1 */
    const void *dx;       /* the gradient of the stream (prenorm); NULL: none */
    const void *x;        /* the stream */
    const void *x0;       /* read with colscale */
    const void *weight0;
    const void *weight1;  /* NULL: one weight */
    const void *rowscale; /* NULL: none */
    const void *colscale; /* NULL: none */
    const uint64_t *rng_state; /* the pair the forward used; read with p_dropout > 0 */
    const float *mu;      /* unread with FA_DROPOUT_NORM_RMS */
    const float *rsigma;
    void *dx0;
    void *dx1;       /* NULL: not written */
    void *dresidual; /* NULL: not written */
    void *dw0;       /* (N), weight_dtype */
    void *db0;       /* (N); NULL: not computed */
    void *dw1;       /* (N); with weight1 */
    void *db1;       /* (N); NULL: not computed */
    void *dcolscale; /* (N), colscale_dtype; with colscale */
    void *workspace; /* fa_dropout_norm_bwd_workspace_bytes() bytes, 16-byte aligned */
    uint64_t workspace_bytes;
    int64_t dz0_row_stride, dz1_row_stride, dx_row_stride, x_row_stride, x0_row_stride, dx0_row_stride, dx1_row_stride,
        dresidual_row_stride;
    int64_t M;
    int32_t N;
    int32_t dz_dtype;     /* of dz0 and dz1 */
    int32_t x_dtype;      /* of x, dx and dresidual: x0_dtype or FA_DTYPE_FP32 */
    int32_t x0_dtype;     /* of x0, dx0 and dx1 */
    int32_t weight_dtype; /* of the weights and their gradients */
    int32_t rowscale_dtype, colscale_dtype;
    float p_dropout;
    int32_t flags; /* FA_DROPOUT_NORM_* */
} fa_dropout_norm_bwd_params;

/* the checks of the launch entries without a device: FA_OK or the status the entry would return before it launches */
int fa_dropout_norm_fwd_validate(const fa_dropout_norm_fwd_params *params);
int fa_dropout_norm_bwd_validate(const fa_dropout_norm_bwd_params *params);
/* asynchronous on `stream` (a hipStream_t; NULL: the default stream); no host synchronisation, no allocation */
int fa_dropout_norm_fwd(const fa_dropout_norm_fwd_params *params, void *stream);
int fa_dropout_norm_bwd(const fa_dropout_norm_bwd_params *params, void *stream);
/* bytes of workspace fa_dropout_norm_bwd needs: a function of M, N and of which column sums there are (weight1, colscale) */
uint64_t fa_dropout_norm_bwd_workspace_bytes(const fa_dropout_norm_bwd_params *params);
uint32_t fa_dropout_norm_fwd_params_size(void);
uint32_t fa_dropout_norm_bwd_params_size(void);

/* The form a call takes, filled by the host function the launch itself consumes; no device.  cw: 8 / 4 (16-byte accesses of a
 * 16-bit / fp32 x0) or 1 (element accesses).  threads: of a workgroup, which takes one row at a time.  wide: rows beyond the
 * registers of 1024 threads (three walks over the row in the forward; row sums in a launch of their own and column slabs in
 * the backward).  dropout: the instantiation that draws decisions (p > 0).  two_weights: weight1 is there.  sums: the column
 * sums of the backward (2: dw0, db0; 3: and dcolscale; 4: dw0, db0, dw1, db1), 0 in the forward.  grid_x workgroups of
 * rows_per_wg rows; grid_y: column slabs, 1 unless wide backward. */
typedef struct fa_dropout_norm_plan {
    int32_t cw, threads, wide, dropout, two_weights, sums, rows_per_wg, grid_x, grid_y;
} fa_dropout_norm_plan;
/* validate first: its status on failure, and *plan untouched.  M = 0 is valid and launches nothing of the rows: the plan then
 * has grid_x = 0 */
int fa_dropout_norm_fwd_plan(const fa_dropout_norm_fwd_params *params, fa_dropout_norm_plan *plan);
int fa_dropout_norm_bwd_plan(const fa_dropout_norm_bwd_params *params, fa_dropout_norm_plan *plan);

#ifdef __cplusplus
}
#endif
#endif /* FA_DROPOUT_NORM_H_ */
