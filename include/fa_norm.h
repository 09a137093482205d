/*
 * fa_norm.h -- C ABI of the fused residual-add + LayerNorm / RMSNorm (csrc/fa_norm.hip): what the reference's
 * flash_attn.ops.triton.layer_norm reaches through _layer_norm_fwd / _layer_norm_bwd (flash_attn/ops/triton/layer_norm.py:
 * 214-288, 531-640), without dropout and without the parallel (x1 / weight1) form.  A header of its own: fa_fwd.h, its ABI
 * version and the kernel sets of the other units are what they were.  Status codes, dtype codes and fa_strerror are those of
 * fa_fwd.h.
 *
 * Forward, per row of N columns, all arithmetic in fp32:
 *   z            = x * rowscale[row] + residual            (rowscale, residual optional)
 *   residual_out = z rounded once to its dtype             (optional)
 *   mean         = sum(z) / N, var = sum((z - mean)^2) / N (RMS: no mean, var = sum(z^2) / N); from the unrounded z
 *   rstd         = 1 / sqrt(var + eps)
 *   y            = (z - mean) * rstd * w + b               (w + 1 with FA_NORM_ZERO_CENTERED; bias optional), rounded once
 * Backward, x being what the forward wrote as residual_out (or its x where it wrote none):
 *   xhat = (x - mean) * rstd, wdy = w * dy, c1 = sum(xhat * wdy) / N, c2 = sum(wdy) / N (RMS: no c2)
 *   dx   = (wdy - (xhat * c1 + c2)) * rstd + dresidual;  dresidual_in = dx;  dx *= rowscale[row]
 *   dw   = sum over rows of dy * xhat,  db = sum over rows of dy;  y (optional) = xhat * w + b, recomputed in the same pass
 * dw / db: every workgroup owns a contiguous block of rows and writes one fp32 partial row into `workspace`; a second kernel
 * adds the partials in a fixed order and casts.  No atomics, and the partial count is a function of M alone: the same call
 * gives the same bits every time.  What the operands' alignment changes is the access shape (16-byte or element accesses), and
 * with it the order in which a row's sums are added: mean / rstd in the forward and c1 / c2 -- hence dx -- in the backward may
 * differ in the last bits between an aligned and a misaligned view of the same values; which rows a dw / db partial holds does not.
 *
 * x / residual / y / dy / dx ...: M rows of N elements with unit column stride and a row stride in elements.  Every tensor
 * carries a dtype code of its own (FA_DTYPE_FP16 / FA_DTYPE_BF16 / FA_DTYPE_FP32).  A row of x is at most 64 KiB.  16-byte
 * accesses (8 x 16-bit or 4 x fp32 of x per lane) where N is a multiple of that width and every base pointer and row pitch is
 * 16-byte aligned; anything else valid takes element accesses.  M * N may pass 2^31: rows are addressed in 64 bits.  Rows wider
 * than 16384 columns (forward) or 8192 (backward) take one workgroup per row: M < 2^31 there (FA_ERR_BAD_SHAPE).
 */
#ifndef FA_NORM_H_
#define FA_NORM_H_

#include "fa_fwd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_NORM_RMS 1           /* RMSNorm: no mean */
#define FA_NORM_ZERO_CENTERED 2 /* the weight is stored minus one */
#define FA_NORM_MAX_ROW_BYTES 65536

typedef struct fa_norm_fwd_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *x;
    const void *residual; /* NULL: none */
    const void *weight;   /* (N) */
    const void *bias;     /* (N); NULL: none */
    const void *rowscale; /* (M); NULL: none */
    void *y;
    void *residual_out; /* NULL: not written */
    float *mean;        /* (M); unread and may be NULL with FA_NORM_RMS */
    float *rstd;        /* (M) */
    int64_t x_row_stride, residual_row_stride, y_row_stride, residual_out_row_stride; /* in elements */
    int64_t M;
    int32_t N;
    int32_t x_dtype;
    int32_t residual_dtype, residual_out_dtype; /* x_dtype or FA_DTYPE_FP32 */
    int32_t weight_dtype, bias_dtype, y_dtype, rowscale_dtype;
    float eps;
    int32_t flags; /* FA_NORM_* */
} fa_norm_fwd_params;

typedef struct fa_norm_bwd_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *x; /* the forward's residual_out, or its x */
    const void *dy;
    const void *weight;
    const void *bias;      /* read for y only; NULL: none */
    const void *dresidual; /* NULL: none */
    const void *rowscale;  /* NULL: none */
    const float *mean;     /* unread with FA_NORM_RMS */
    const float *rstd;
    void *dx;
    void *dresidual_in; /* NULL: not written */
    void *dw;           /* (N), weight_dtype */
    void *db;           /* (N), bias_dtype; NULL: not computed */
    void *y;            /* NULL: not recomputed */
    void *workspace;    /* fa_norm_bwd_workspace_bytes() bytes, 16-byte aligned */
    uint64_t workspace_bytes;
    int64_t x_row_stride, dy_row_stride, dresidual_row_stride, dx_row_stride, dresidual_in_row_stride, y_row_stride;
    int64_t M;
    int32_t N;
    int32_t x_dtype; /* dx_dtype or FA_DTYPE_FP32 */
    int32_t dy_dtype, weight_dtype, bias_dtype;
    int32_t dresidual_dtype, dresidual_in_dtype; /* x_dtype */
    int32_t dx_dtype, y_dtype, rowscale_dtype;
    float eps;
    int32_t flags; /* FA_NORM_* */
} fa_norm_bwd_params;

/* the checks of the launch entries without a device: FA_OK or the status the entry would return before it launches */
int fa_norm_fwd_validate(const fa_norm_fwd_params *params);
int fa_norm_bwd_validate(const fa_norm_bwd_params *params);
/* asynchronous on `stream` (a hipStream_t; NULL: the default stream); no host synchronisation, no allocation */
int fa_norm_fwd(const fa_norm_fwd_params *params, void *stream);
int fa_norm_bwd(const fa_norm_bwd_params *params, void *stream);
/* bytes of workspace fa_norm_bwd needs for these M and N (the workspace fields themselves are not read) */
uint64_t fa_norm_bwd_workspace_bytes(const fa_norm_bwd_params *params);
uint32_t fa_norm_fwd_params_size(void);
uint32_t fa_norm_bwd_params_size(void);

/* The form a call takes, filled by the host function the launch itself consumes; no device.  cw: 8 / 4 (16-byte accesses of a
 * 16-bit / fp32 x) or 1 (element accesses).  threads: of a workgroup; team_wave: a row is the work of one wavefront of it, else
 * of all of it.  wide: rows beyond the registers of 1024 threads (one row per workgroup in the forward; row sums in a launch of
 * their own and column slabs in the backward).  grid_x workgroups of rows_per_wg rows; grid_y: column slabs, 1 unless wide
 * backward. */
typedef struct fa_norm_plan {
    int32_t cw, threads, team_wave, wide, rows_per_wg, grid_x, grid_y;
} fa_norm_plan;
/* validate first: its status on failure, and *plan untouched.  M = 0 is valid and launches nothing of the rows: the plan then
 * has grid_x = 0 */
int fa_norm_fwd_plan(const fa_norm_fwd_params *params, fa_norm_plan *plan);
int fa_norm_bwd_plan(const fa_norm_bwd_params *params, fa_norm_plan *plan);

#ifdef __cplusplus
}
#endif
#endif /* FA_NORM_H_ */
