/*
 * fa_bwd.h — C-ABI of the MI355X (gfx950) FlashAttention backward.
 *
 *   reference interface replaced                                  entry point here
 *   ------------------------------------------------------------  -----------------
 *   mha_bwd          csrc/flash_attn/flash_api.cpp:767-971        fa_bwd (dense)
 *   mha_varlen_bwd   csrc/flash_attn/flash_api.cpp:973-1200       fa_bwd (cu_seqlens_* set)
 *   set_params_dgrad csrc/flash_attn/flash_api.cpp:161-221        fa_bwd_params
 *   Flash_bwd_params csrc/flash_attn/src/flash.h:147-191          fa_bwd_params
 *
 * Same conventions as fa_fwd.h: raw device pointers, ELEMENT strides, head-dim stride 1, the callee never
 * allocates or synchronises and launches on `stream`.  Three launches: D = rowsum(dO * O) (role of
 * compute_dot_do_o, csrc/flash_attn/src/flash_bwd_preprocess_kernel.h:60-127), then dK/dV (one workgroup per
 * 128-key block of a kv head, looping over the query tiles of every query head of its GQA group) and dQ (one
 * workgroup per 128-row query block, looping over the key tiles).  Each output element is produced by exactly
 * one workgroup in a fixed order: no atomics, bit-reproducible ("deterministic" is always on); the price is
 * that S and dP are recomputed by the dQ pass (7 matrix products instead of the reference's 5).
 */
#ifndef FA_BWD_H_
#define FA_BWD_H_

#include <stdint.h>

#include "fa_fwd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fa_bwd_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size; /* sizeof(fa_bwd_params) */

    /* inputs (device pointers): the forward's operands and results, and the incoming gradient */
    const void *q;
    const void *k;
    const void *v;
    const void *o;
    const void *dout;
    const float *softmax_lse; /* as written by fa_fwd: (b, h, seqlen_q) or varlen (h, total_q) */
    /* outputs */
    void *dq; /* like q */
    void *dk; /* like k: (b, seqlen_k, h_k, d) -- already summed over the query heads of each GQA group */
    void *dv; /* like v */
    float *softmax_d; /* D = rowsum(dO * O): dense (b, h, softmax_d_row_len), varlen (h, softmax_d_row_len) */

    /* element strides; head_dim stride is 1 */
    int64_t q_batch_stride, q_row_stride, q_head_stride;
    int64_t k_batch_stride, k_row_stride, k_head_stride;
    int64_t v_batch_stride, v_row_stride, v_head_stride;
    int64_t o_batch_stride, o_row_stride, o_head_stride;
    int64_t do_batch_stride, do_row_stride, do_head_stride;
    int64_t dq_batch_stride, dq_row_stride, dq_head_stride;
    int64_t dk_batch_stride, dk_row_stride, dk_head_stride;
    int64_t dv_batch_stride, dv_row_stride, dv_head_stride;
    int64_t softmax_d_row_len; /* >= seqlen_q (dense; the reference rounds to 128) / >= total_q (varlen) */

    /* sizes: as fa_fwd_params */
    int32_t b, seqlen_q, seqlen_k, h, h_k, d, total_q, total_k;
    int32_t dtype; /* FA_DTYPE_FP16 / FA_DTYPE_BF16 */

    const int32_t *cu_seqlens_q; /* (b+1) or NULL = dense */
    const int32_t *cu_seqlens_k;

    float softmax_scale;
    float softcap;
    int32_t is_causal;
    int32_t window_size_left;
    int32_t window_size_right;

    const float *alibi_slopes; /* as fa_fwd_params */
    int64_t alibi_slopes_batch_stride;

    int32_t deterministic; /* accepted; results are always bit-reproducible */
    float p_dropout;       /* as fa_fwd_params; rng_state must be the pair the forward used */
    const uint64_t *rng_state;
    int32_t flags;         /* FA_FLAG_* as fa_fwd_params (FA_FLAG_FA3_WINDOW) */
    /* ABI v12 -- head dim of v / o / dout / dv when it differs from d (FA3 headdim_v, hopper/flash_api.cpp:1345-1369:
     * the reference's backward rounds both to the larger): 0 = d.  Built for the wide head-dim tile only (max(d, d_v) in
     * (128, 256], e.g. 192 / 128); other pairs return FA_ERR_UNSUPPORTED. */
    int32_t d_v;
} fa_bwd_params;

/* Validate and enqueue the backward on `stream`.  Returns FA_OK or a negative fa_status; asynchronous. */
int fa_bwd(const fa_bwd_params *params, void *stream);

/* Validation only (what mha_bwd's TORCH_CHECKs do); no device access. */
int fa_bwd_validate(const fa_bwd_params *params);

/* sizeof(fa_bwd_params) as compiled, for binding self-checks. */
uint32_t fa_bwd_params_size(void);

/* Test hook: the kernels fa_bwd would launch for `params`, without launching (no device access; NULL when fa_bwd_validate
 * refuses them).  One segment per launched kernel, in launch order, e.g.
 *     "bwd_dot LPR=16 | bwd_dkdv D=128 NB=1 DEFF=96 | bwd_dq D=128 NB=2 DEFF=96"
 * D = head-dim tile, NB = 32-wide blocks per wave, DEFF = columns of the tile the products cover; flags SOFTCAP / DROPOUT; the
 * 256 tile shows its two dK/dV launches as PART=1 and PART=2.  A launch without work items (no query rows: bwd_dot, bwd_dq; no
 * keys: bwd_dkdv) has no segment.  The string lives in thread-local storage until the thread's next call. */
const char *fa_bwd_plan_name(const fa_bwd_params *params);

/* Test hook: the plan of the calling thread's most recent fa_bwd() (same text; NULL before the first call and after a call
 * that failed validation).  Tests read it to tie a gradient to the kernels that produced it. */
const char *fa_bwd_last_plan_name(void);

/*
 * Gradient of a learnable attention sink (fa_fwd_sink, include/fa_fwd.h).  With the sink inside the stored LSE,
 * P = exp(S - LSE) and D_i = sum_d dO.O = sum_j P_ij dP_ij (the sink's column has no value: it adds nothing to D), so
 * fa_bwd gives dq, dk, dv of a call with a sink as it stands; the sink's own gradient is
 *     dsink[h] = - sum_{b, i} exp(z_h - LSE[b, h, i]) * D[b, h, i]
 * over the valid rows of the softmax_d fa_bwd has written (run this behind it, on the same stream).  One workgroup per
 * head, every partial sum in a fixed order, no atomics: bit-reproducible like the rest of the backward.  No workspace.
 */
typedef struct fa_sink_grad_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size; /* sizeof(fa_sink_grad_params) */
    const float *softmax_lse;   /* as fa_fwd_sink wrote it: (b, h, seqlen_q) or varlen (h, total_q) */
    const float *softmax_d;     /* as fa_bwd wrote it: (b, h, softmax_d_row_len) or varlen (h, softmax_d_row_len) */
    const void *learnable_sink; /* (h), contiguous */
    float *dsink;               /* (h) fp32, written (not accumulated) */
    const int32_t *cu_seqlens_q; /* (b + 1) or NULL = dense */
    const int32_t *seqused_q;    /* (b) or NULL: rows of each sequence that count */
    int64_t softmax_d_row_len;
    int32_t b, seqlen_q, h, total_q;
    int32_t sink_dtype; /* FA_DTYPE_BF16 / FA_DTYPE_FP32 */
    int32_t reserved;
} fa_sink_grad_params;

int fa_sink_grad(const fa_sink_grad_params *params, void *stream);
int fa_sink_grad_validate(const fa_sink_grad_params *params);
uint32_t fa_sink_grad_params_size(void);

/*
 * Block-sparse backward: the gradient of fa_fwd_block_sparse (include/fa_fwd.h).  The function differentiated is the
 * forward's: dense attention restricted to the visited 128 x 128 blocks and, inside them, to what is_causal /
 * window_size_left / right (bottom-right aligned) and the sequence ends allow.  (The reference has no such backward: its
 * cute surface returns the dense gradient for a block-sparse forward, flash_attn/cute/interface.py:1055-1069.)
 * Three launches like fa_bwd, one producer per output element, no atomics, no workspace, bit-reproducible:
 *   D      bwd_dot_kernel over all rows (softmax_d is written for every row: fa_sink_grad reads it);
 *   dK/dV  one workgroup per 128-key block of a (batch, kv head).  It owns a key block and needs the query blocks that visit
 *          it -- the transpose of the forward's lists, which the CALLER passes as key-major lists (a sparsity pattern is
 *          normally fixed across layers and steps: built once, not in every call):
 *            q_block_cnt  int32, logical shape (b, h, nk)        h = QUERY heads, as the forward's lists
 *            q_block_idx  int32, logical shape (b, h, nk, nm)
 *          read through element strides, stride 0 for a broadcast dimension.  Key block n of query head h is visited by the
 *          first q_block_cnt[.., n] query blocks of q_block_idx[.., n, :].  One merged list: the full / mask split is a hint
 *          the kernels ignore.  For every query head of the GQA group in ascending order the workgroup walks that list;
 *   dQ     one workgroup per 128-row query block; it walks `fwd_lists` (the full list first) exactly as the forward does.
 * That the key-major lists and the forward's lists describe the same set of (query block, key block) pairs is the caller's
 * duty, as are distinct indices inside [0, nm) / [0, nk); the result of anything else is undefined, but no list content makes
 * a kernel read or write out of bounds: counts are clamped to [0, nm] / [0, nk], and a listed pair that cannot hold a visible
 * (row, key) -- an index outside the range, a tile past seqlen_q / seqlen_k or outside the causal / window range of the
 * block -- is neither loaded nor computed.  The host never reads the lists.  The accumulation order is the list order, so
 * equal lists give bit-equal gradients.
 * Rows with LSE = +inf (no visible key, no sink) have P = 0: dq = 0 there, never NaN.  A key block nobody visits gets
 * dk = dv = 0 written, a query block with both counts 0 gets dq = 0 written.  With a learnable sink nothing changes here (the
 * LSE holds it); fa_sink_grad behind this call gives the sink's gradient.
 * Accepted: fp16 / bf16, d <= 128 with d_v = d (0 or d), MHA / GQA / MQA, is_causal, both window sides, softcap, arbitrary
 * strides.  FA_ERR_UNSUPPORTED, checked before anything the params may lack: cu_seqlens_*, ALiBi, dropout, d > 128, d_v set and
 * != d, block_m / block_n other than 128 (in either list struct).  NULL or misaligned list pointers and negative strides
 * return fa_fwd_block_sparse_validate's codes.
 * fa_bwd_params is untouched (its size is pinned).  fa_bwd_plan_name of plain params means what it meant;
 * fa_bwd_last_plan_name() answers for this call e.g. "bwd_dot LPR=16 | bs_bwd_dkdv D=128 | bs_bwd_dq D=128 SOFTCAP"
 * (D = head-dim tile 64 / 128; a launch without work items has no segment).
 */
typedef struct fa_block_sparse_bwd_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size; /* sizeof(fa_block_sparse_bwd_params) */
    const int32_t *q_block_cnt; /* device pointers, both required */
    const int32_t *q_block_idx;
    /* element strides, >= 0: cnt (batch, head, n, unused = 0), idx (batch, head, n, m) */
    int64_t q_cnt_stride[4], q_idx_stride[4];
    int32_t block_m, block_n; /* 128, 128 */
} fa_block_sparse_bwd_params;

int fa_bwd_block_sparse(const fa_bwd_params *params, const fa_block_sparse_params *fwd_lists,
                        const fa_block_sparse_bwd_params *key_lists, void *stream);
/* Validation only; no device access. */
int fa_bwd_block_sparse_validate(const fa_bwd_params *params, const fa_block_sparse_params *fwd_lists,
                                 const fa_block_sparse_bwd_params *key_lists);
uint32_t fa_block_sparse_bwd_params_size(void);

#ifdef __cplusplus
}
#endif
#endif /* FA_BWD_H_ */
