/*
 * fa_gemm_act.h -- C ABI of the GEMM with a fused bias + activation epilogue (csrc/fa_gemm_act.hip): what the reference
 * computes with its Triton GEMM in flash_attn/ops/triton/linear.py (triton_linear_act, triton_dgrad_act), the fc1 of
 * flash_attn/ops/triton/mlp.py.  A header of its own: fa_fwd.h, its ABI version and the kernel sets of the other units are
 * what they were.  Status codes, dtype codes and fa_strerror are those of fa_fwd.h; the activation codes are those of the
 * fused activations' header (FA_ACT_GELU_TANH ... FA_ACT_IDENTITY = 0 ... 6), and the activations are the same fp32
 * expressions.
 *
 * Forward:  s[m, n] = sum_k x[m, k] * weight[n, k] + bias[n]      (fp32 on MFMA, bias added in fp32; bias optional)
 *           act_input[m, n] = s rounded once                      (optional)
 *           out[m, n]       = act(s) rounded once                 (act of the UNROUNDED fp32 value)
 *   This is the order of the reference's kernel.  It has one rounding fewer than a GEMM that writes s in 16 bits followed by
 *   an activation pass that reads it back: there out = act(round(s)), here out = act(s).
 * Dgrad:    g[m, n] = sum_k grad_out[m, k] * weight[k, n]         (fp32 on MFMA; weight is row-major (K, N), not transposed)
 *           grad_in[m, n] = act'(act_input[m, n]) * g rounded once (act' in fp32 on the stored act_input; identity: g)
 *           dbias[n] = sum_m of the unrounded products            (optional, fp32 sums, no atomics)
 *
 * x / grad_out (M, K), weight (N, K) forward and (K, N) dgrad, out / act_input / grad_in (M, N), bias / dbias (N): fp16 or
 * bf16, and every tensor of a call has the same dtype (each carries its code; fp32 or a code that differs is
 * FA_ERR_BAD_DTYPE).  Any M >= 0 (M == 0 is FA_OK and launches nothing; dbias is then not written).  N and K are positive
 * multiples of 8 (FA_ERR_BAD_SHAPE otherwise), every base is 16-byte aligned and every row stride is a multiple of 8 elements
 * and at least the row's length (FA_ERR_BAD_STRIDE otherwise): every global access is 16 bytes.  Strides are in elements, the
 * last stride is 1.  M is 64 bits and so are the row bases: M * N, M * K and an operand's size in bytes may pass 2^31 and
 * 4 GiB.  Tiles may be ragged in M, N and K (K may be shorter than one K-step): a load past an edge is issued at a clamped,
 * in-bounds address and its value replaced by zero.
 *
 * dbias without atomics: the workgroup of output tile (i, j) writes the column sums of its rows as fp32 into partial row i of
 * the workspace (tiles_m rows of N floats); a reduce kernel adds the partial rows in their order and casts.  The same call
 * gives the same bits every time.
 */
#ifndef FA_GEMM_ACT_H_
#define FA_GEMM_ACT_H_

#include "fa_fwd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fa_gemm_act_fwd_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *x;      /* (M, K) */
    const void *weight; /* (N, K) */
    const void *bias;   /* (N) or NULL */
    void *out;          /* (M, N) */
    void *act_input;    /* (M, N) or NULL */
    int64_t x_row_stride, weight_row_stride, out_row_stride, act_input_row_stride; /* in elements */
    int64_t M;
    int32_t N, K;
    int32_t activation; /* a FA_ACT_* code; the plain forms only (no gating) */
    int32_t x_dtype, weight_dtype, bias_dtype, out_dtype, act_input_dtype;
} fa_gemm_act_fwd_params;

typedef struct fa_gemm_act_dgrad_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *grad_out;  /* (M, K) */
    const void *weight;    /* (K, N), row-major */
    const void *act_input; /* (M, N); may be NULL with FA_ACT_IDENTITY only */
    void *grad_in;         /* (M, N) */
    void *dbias;           /* (N) or NULL */
    void *workspace;       /* fa_gemm_act_dgrad_workspace_bytes(), 16-byte aligned; read and written only with dbias */
    uint64_t workspace_bytes;
    int64_t grad_out_row_stride, weight_row_stride, act_input_row_stride, grad_in_row_stride; /* in elements */
    int64_t M;
    int32_t N, K;
    int32_t activation;
    int32_t grad_out_dtype, weight_dtype, act_input_dtype, grad_in_dtype, dbias_dtype;
} fa_gemm_act_dgrad_params;

/* the checks of the launch entries without a device: FA_OK or the status the entry would return before it launches */
int fa_gemm_act_fwd_validate(const fa_gemm_act_fwd_params *params);
int fa_gemm_act_dgrad_validate(const fa_gemm_act_dgrad_params *params);
/* asynchronous on `stream` (a hipStream_t; NULL: the default stream); no host synchronisation, no allocation */
int fa_gemm_act_fwd(const fa_gemm_act_fwd_params *params, void *stream);
int fa_gemm_act_dgrad(const fa_gemm_act_dgrad_params *params, void *stream);
uint32_t fa_gemm_act_fwd_params_size(void);
uint32_t fa_gemm_act_dgrad_params_size(void);
/* bytes of fp32 partial rows a dgrad with dbias needs (0 without dbias or rows); M, N and dbias are read, nothing else */
uint64_t fa_gemm_act_dgrad_workspace_bytes(const fa_gemm_act_dgrad_params *params);

/* The form a call takes, filled by the host function the launch itself consumes; no device.  A workgroup of `threads` threads
 * owns one tile_m x tile_n tile of the output and walks k_steps steps of tile_k; tile_m is 64 where M <= 64 and 128 above.
 * The grid is one-dimensional, grid_x = tiles_m * tiles_n workgroups: a workgroup's index is first made contiguous per XCD
 * (the indices that share an XCD, every 8th, take consecutive tiles) and then mapped so that group_m row tiles share their
 * column tiles while they are resident (the reference's GROUP_M).  ragged_*: the last tile of that dimension is partial.
 * partial_rows / reduce_grid_x: the partial rows of dbias and the grid of the reduce kernel; 0 without dbias. */
typedef struct fa_gemm_act_plan {
    int32_t tile_m, tile_n, tile_k, threads;
    int32_t tiles_m, tiles_n, grid_x, k_steps;
    int32_t ragged_m, ragged_n, ragged_k, group_m;
    int32_t partial_rows, reduce_grid_x, dtype, dgrad;
} fa_gemm_act_plan;
/* validate first: its status on failure, and *plan untouched.  M = 0 is valid and launches nothing: grid_x = 0 */
int fa_gemm_act_fwd_plan(const fa_gemm_act_fwd_params *params, fa_gemm_act_plan *plan);
int fa_gemm_act_dgrad_plan(const fa_gemm_act_dgrad_params *params, fa_gemm_act_plan *plan);

#ifdef __cplusplus
}
#endif
#endif /* FA_GEMM_ACT_H_ */
