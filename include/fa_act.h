/*
 * fa_act.h -- C ABI of the fused MLP activations (csrc/fa_act.hip): the pass between the two GEMMs of an MLP, what the
 * reference computes in flash_attn/ops/activations.py (bias_gelu, gelu_fwd / gelu_bwd, relu_bwd, sqrelu_fwd / sqrelu_bwd,
 * swiglu_fwd / swiglu_bwd) and in the epilogues of flash_attn/ops/fused_dense.py.  A header of its own: fa_fwd.h, its ABI
 * version and the kernel sets of the other units are what they were.  Status codes, dtype codes and fa_strerror are those of
 * fa_fwd.h.
 *
 * Plain form, x = pre[r, c] + bias[c] (bias optional), all arithmetic in fp32, every result rounded once:
 *   forward   out[r, c]  = act(x)
 *   backward  dpre[r, c] = act'(x) * dout[r, c];  dbias[c] = sum_r of the unrounded products (optional, fp32 sums)
 * Gated form (FA_ACT_GATED), g = gate[r, c], u = up[r, c]; gate and up are two base pointers with one row pitch, so the two
 * halves of one (M, 2H) tensor are passed without a copy, and so are two tensors of the same pitch:
 *   forward   out[r, c]   = act(g) * u
 *   backward  dgate[r, c] = (act'(g) * u) * dout[r, c];  dup[r, c] = act(g) * dout[r, c]
 *             dgate and dup are two base pointers with one row pitch: the two halves of one (M, 2H) gradient.
 *   FA_ACT_SIGMOID gives GLU, FA_ACT_SILU SwiGLU, FA_ACT_GELU_TANH GEGLU, FA_ACT_RELU ReGLU.
 * Backward, both forms: with recompute_out the same pass writes the forward's out, bit-equal to what fa_act_fwd writes.
 *
 * The activations, written so that saturation selects the limit and no finite input gives NaN (s(z) = 1 / (1 + exp(-z)) is
 * formed from exp(-|z|), together with 1 - s(z)):
 *   GELU_TANH  x * s(z), z = 2 * 0.79788456 * x * (1 + 0.044715 x^2)  (= 0.5 x (1 + tanh(z / 2)), the reference's form);
 *              act' = s + x * s (1 - s) * dz/dx, the second term 0 once s (1 - s) is 0
 *   GELU_ERF   x * Phi(x), Phi from erf (x >= 0) or erfc (x < 0);  act' = Phi + x * exp(-x^2 / 2) / sqrt(2 pi)
 *   RELU       x > 0 ? x : 0;  act' = x > 0 ? 1 : 0 (0 at x = 0, as autograd has it)
 *   SQRELU     relu(x)^2;  act' = 2 relu(x), its product with a factor g formed as (relu(x) * g) * 2
 *   SILU       x * s(x);  act' = s + x * s (1 - s)
 *   SIGMOID    s(x);  act' = s (1 - s)
 *   IDENTITY   x;  act' = 1
 * A product that overflows fp32 is inf (sqrelu of a large value), as the fp64 result rounded to the tensor's dtype is.
 * Non-finite inputs propagate as IEEE arithmetic does.
 *
 * pre / gate / up / out / dout / dpre / dgate / dup / recompute_out: M rows of H elements, unit column stride, one dtype for
 * all of them (fp16, bf16 or fp32; every tensor carries its code, and a code that differs is FA_ERR_BAD_DTYPE); bias and dbias
 * (H) are of that dtype or fp32.  H >= 1, row pitches >= H in elements (where M > 1), pointers aligned to their element.
 * M is 64 bits and so are the row bases: M * pitch may pass 2^31.  M == 0 is FA_OK and launches nothing (dbias is then not
 * written: the caller zeroes it).
 * Access forms: where every tensor of the call has a 16-byte aligned base and (M > 1) a row pitch that is a multiple of 16
 * bytes, a row is H / cw chunks of 16 bytes (cw = 8 elements of a 16-bit dtype, 4 of fp32; an fp32 bias beside 16-bit data is
 * two 16-byte accesses per chunk) and an element tail of H % cw columns; everywhere else every column is an element access
 * (cw = 1).  fa_act_*_plan says which.
 * dbias without atomics: a workgroup owns rows_per_wg rows times a slab of columns, keeps the column sums of all its row
 * blocks in registers and writes one fp32 partial row; a reduce kernel adds the partial rows in their order.  Their number is
 * the backward's grid_y, a function of M alone.  The same call gives the same bits every time.
 */
#ifndef FA_ACT_H_
#define FA_ACT_H_

#include "fa_fwd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_ACT_GELU_TANH 0
#define FA_ACT_GELU_ERF 1
#define FA_ACT_RELU 2
#define FA_ACT_SQRELU 3
#define FA_ACT_SILU 4
#define FA_ACT_SIGMOID 5
#define FA_ACT_IDENTITY 6

#define FA_ACT_GATED 1 /* flags: pre is the gate and up is read */

typedef struct fa_act_fwd_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *pre;  /* (M, H); the gate with FA_ACT_GATED */
    const void *up;   /* (M, H), FA_ACT_GATED only; the pitch of pre */
    const void *bias; /* (H) or NULL; plain form only */
    void *out;        /* (M, H) */
    int64_t pre_row_stride, out_row_stride; /* in elements */
    int64_t M;
    int32_t H;
    int32_t activation; /* FA_ACT_* */
    int32_t flags;      /* FA_ACT_GATED */
    int32_t pre_dtype, up_dtype, bias_dtype, out_dtype;
    int32_t reserved;
} fa_act_fwd_params;

typedef struct fa_act_bwd_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *pre;     /* (M, H); the gate with FA_ACT_GATED */
    const void *up;      /* FA_ACT_GATED only; the pitch of pre */
    const void *bias;    /* (H) or NULL; plain form only */
    const void *dout;    /* (M, H) */
    void *dpre;          /* (M, H); dgate with FA_ACT_GATED */
    void *dup;           /* FA_ACT_GATED only; the pitch of dpre */
    void *dbias;         /* (H) or NULL; plain form only */
    void *recompute_out; /* (M, H) or NULL */
    void *workspace;     /* fa_act_bwd_workspace_bytes(), 16-byte aligned; read and written only with dbias */
    uint64_t workspace_bytes;
    int64_t pre_row_stride, dout_row_stride, dpre_row_stride, out_row_stride; /* in elements */
    int64_t M;
    int32_t H;
    int32_t activation;
    int32_t flags;
    int32_t pre_dtype, up_dtype, bias_dtype, dout_dtype, dpre_dtype, dup_dtype, dbias_dtype, out_dtype;
    int32_t reserved;
} fa_act_bwd_params;

/* the checks of the launch entries without a device: FA_OK or the status the entry would return before it launches */
int fa_act_fwd_validate(const fa_act_fwd_params *params);
int fa_act_bwd_validate(const fa_act_bwd_params *params);
/* asynchronous on `stream` (a hipStream_t; NULL: the default stream); no host synchronisation, no allocation */
int fa_act_fwd(const fa_act_fwd_params *params, void *stream);
int fa_act_bwd(const fa_act_bwd_params *params, void *stream);
uint32_t fa_act_fwd_params_size(void);
uint32_t fa_act_bwd_params_size(void);
/* bytes of fp32 partial rows a backward with dbias needs (0 without dbias or rows); M, H and dbias are read, nothing else */
uint64_t fa_act_bwd_workspace_bytes(const fa_act_bwd_params *params);

/* The form a call takes, filled by the host function the launch itself consumes; no device.  cw: elements per access (8 / 4:
 * 16-byte chunks and an element tail; 1: elements).  grid_x slabs of `threads` chunks, grid_y blocks of rows_per_wg rows; what
 * is beyond either is walked.  The backward writes grid_y partial rows of dbias. */
typedef struct fa_act_plan {
    int32_t cw, threads, grid_x, grid_y, rows_per_wg;
} fa_act_plan;
/* validate first: its status on failure, and *plan untouched.  M = 0 is valid and launches nothing: grid_y = 0 */
int fa_act_fwd_plan(const fa_act_fwd_params *params, fa_act_plan *plan);
int fa_act_bwd_plan(const fa_act_bwd_params *params, fa_act_plan *plan);

#ifdef __cplusplus
}
#endif
#endif /* FA_ACT_H_ */
