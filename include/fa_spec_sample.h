/*
 * fa_spec_sample.h -- C ABI of the fused verification step of speculative sampling (csrc/fa_spec_sample.hip): Algorithm 1 of
 * Leviathan, Kalman, Matias, "Fast Inference from Transformers via Speculative Decoding" (arXiv 2211.17192), which the reference
 * builds from torch calls in flash_attn.utils.generation.sample_speculative (flash_attn/utils/generation.py:209-265).  Two
 * launches behind one entry, no sort, no host synchronisation.  A header of its own beside that of the token sampling unit
 * (DESIGN 4.27), whose FILTER rule, arithmetic and uniforms it takes over: every header of include/ declares one unit, and the
 * symbol set of each is what it was.  Status codes, dtype codes and fa_strerror are those of fa_fwd.h.
 *
 * Per sequence b, with logits (B, S + 1, V) of the target model, logits_draft (B, S, V) and tokens_draft (B, S), S >= 0:
 *   kept sets    every target row (b, t), t <= S, and every draft row (b, t), t < S, is s = logits / temperature (one correctly
 *                rounded fp32 division, -0 counts as +0), and its kept set is exactly what the sampling unit's FILTER mode leaves
 *                of s with the same top_k / top_p: with top_k >= 1 the entries below the min(top_k, V)-th largest value leave and
 *                ALL entries equal to it stay (not the exactly-k rule of the draw); then with 0 < top_p < 1 the top-p rule.
 *                top_k == 1 takes no shortcut.  A row of nothing but -inf keeps nothing.
 *   P, Q         the probabilities of the target and of the draft row over their kept sets: with e_i = exp2((s_i - m) * log2 e)
 *                in fp32, w_i = trunc(e_i * 2^F) the fixed-point weight of a kept entry (F as below) and Z_kept the 64-bit sum
 *                of the w_i, P_i = fp32((double)(e_i * 2^F) / (double)Z_kept); 0 outside the kept set and in a row that keeps
 *                nothing.  (e_i and not w_i above the line: a probability below 2^-F keeps its digits.)
 *   acceptance   with x = tokens_draft[b, t]: position t is accepted iff (double)u_acc[b, t] * (double)Q_t(x) <= (double)P_t(x).
 *                A token outside the draft's kept set has Q = 0 and is accepted, as in the reference.  A token outside [0, V)
 *                is rejected, and nothing is read for it; its P and Q read 0.
 *   n_b          the first rejected position, S if there is none.
 *   resample     n_b < S: weights r_i = trunc((P_i - Q_i) * 2^F) where the fp32 difference P_i - Q_i is positive, else 0, of
 *                the rows (b, n_b); R their 64-bit sum.  R == 0 (no residual weight), or n_b == S: weights w_i of the target
 *                row (b, n_b), R = Z_kept.  Walked in ascending index order, the token is the first index whose inclusive
 *                cumulative weight exceeds floor(u_res[b] * R) (fp64 product of the fp32 u and R); where u >= 1 leaves none,
 *                the last index of positive weight.  A target row that keeps nothing gives token 0.
 *   outputs      tokens (B, S + 1) of the dtype of tokens_draft: tokens_draft[b, t] at t < S (out-of-range ones as they are), 0
 *                in column S, and then the resampled token in column n_b.  num_generated (B) int64 = n_b + 1.
 * The reference writes `tokens[:, first_rejected_idx] = resample`, which for B > 1 sets whole columns: every sequence gets the
 * resampled tokens of the others at their rejection columns.  That is not reproduced: the write is per row, as the algorithm means.
 *
 * The result is a function of the arguments alone: all sums are 64-bit integers (F = min(40, 62 - ceil(log2 V)) fraction bits),
 * so no result depends on the order in which threads arrive, and the same call gives the same bits.  NaN logits are not legal;
 * nothing is read or written out of bounds because of one.
 *
 * Uniforms: u_acc (B, S) and u_res (B) fp32 in [0, 1), or rng_state = {seed, offset} on the device and the counter hash of the
 * sampling unit, with row index b * S + t for the acceptance of (b, t) and B * S + b for the resample of b.
 *
 * Two launches, ordered by the stream.  Phase A: one workgroup per (b, t), t <= S, selects the kept set of the target row and,
 * where t < S, of the draft row, and writes a record of 24 bytes per row into `workspace`:
 *     float m (the maximum of s; -inf: nothing kept) | uint32 K | int32 J | int32 accept | uint64 Z_kept
 * (K, J): kept are the entries whose cut key is above K, and those with key K and index below J.  accept: of the target record
 * of (b, t), t < S, the acceptance.  Target records first, (b, t) at b * (S + 1) + t; then the draft records, at
 * B * (S + 1) + b * S + t.  Phase B: one workgroup per b finds n_b from the flags and walks the one or two rows at n_b with
 * their records, selecting nothing again.  No workgroup waits for another inside a launch.
 *
 * logits and logits_draft have one dtype (fp16, bf16, fp32), a unit column stride, and batch and position strides in elements;
 * rows are addressed in 64 bits.  tokens_draft is int32 or int64 with a batch stride in elements and a unit position stride;
 * tokens and the optional outputs are contiguous.  1 <= V < 2^31, 0 <= S, 0 <= B, B * (2 S + 1) < 2^31 (FA_ERR_BAD_SHAPE); B == 0
 * is FA_OK and launches nothing.  S == 0 is a pure draw from P_0; logits_draft, tokens_draft and u_acc are then not used.
 * temperature > 0, 0 <= top_p <= 1, top_k >= 0 (FA_ERR_BAD_SHAPE; NaN fails).  Exactly one source of uniforms: u_res (with u_acc
 * where S > 0), or rng_state (FA_ERR_NULL_POINTER: neither, or u_res without u_acc; FA_ERR_BAD_SHAPE: both).  workspace holds
 * fa_spec_sample_workspace_size(B, S) bytes, 8-byte aligned (FA_ERR_WORKSPACE: NULL or workspace_bytes too small).  Pointers keep
 * the natural alignment of their element (FA_ERR_BAD_STRIDE).
 * Rows are taken by 16-byte accesses where both tensors qualify: the bases, every pitch in bytes that is used (batch with B > 1,
 * position with more than one row per sequence) and V * element size are multiples of 16; by element accesses otherwise.
 *
 * Optional outputs: p_tok, q_tok (B, S) fp32, P_t(x) and Q_t(x) of every draft token; accepted (B, S) int32, the flags.
 *
 * Known limit: one workgroup per row.  A form that splits a row over workgroups is not part of this unit.
 */
#ifndef FA_SPEC_SAMPLE_H_
#define FA_SPEC_SAMPLE_H_

#include "fa_fwd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_SPEC_TOKENS_INT32 0
#define FA_SPEC_TOKENS_INT64 1
#define FA_SPEC_RECORD_BYTES 24

typedef struct fa_spec_sample_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *logits;        /* (B, S + 1, V) */
    const void *logits_draft;  /* (B, S, V); not used with S == 0 */
    const void *tokens_draft;  /* (B, S); not used with S == 0 */
    const float *u_acc;        /* (B, S) uniforms in [0, 1), or NULL */
    const float *u_res;        /* (B) uniforms in [0, 1), or NULL */
    const uint64_t *rng_state; /* device {seed, offset}, or NULL */
    void *workspace;           /* fa_spec_sample_workspace_size(B, S) bytes */
    void *tokens;              /* (B, S + 1) of tokens_dtype */
    int64_t *num_generated;    /* (B) */
    float *p_tok;              /* (B, S) or NULL */
    float *q_tok;              /* (B, S) or NULL */
    int32_t *accepted;         /* (B, S) or NULL */
    int64_t logits_batch_stride, logits_pos_stride; /* in elements */
    int64_t draft_batch_stride, draft_pos_stride;
    int64_t tokens_draft_batch_stride;
    int64_t workspace_bytes;
    int64_t B;
    int32_t S;
    int32_t V;
    int32_t logits_dtype; /* FA_DTYPE_FP16 / FA_DTYPE_BF16 / FA_DTYPE_FP32, of both logits tensors */
    int32_t tokens_dtype; /* FA_SPEC_TOKENS_* */
    int32_t top_k;
    float top_p;
    float temperature;
    int32_t reserved;
} fa_spec_sample_params;

/* the checks of the launch entry without a device: FA_OK or the status the entry would return before it launches */
int fa_spec_sample_validate(const fa_spec_sample_params *params);
/* asynchronous on `stream` (a hipStream_t; NULL: the default stream); no host synchronisation, no allocation */
int fa_spec_sample(const fa_spec_sample_params *params, void *stream);
uint32_t fa_spec_sample_params_size(void);
/* bytes of the records of a call; 0 where B or S is negative */
int64_t fa_spec_sample_workspace_size(int64_t B, int32_t S);

/* The form a call takes, filled by the host function the launch itself consumes (the kernels get this struct); no device.
 * cw: elements per access (8 / 4: 16 bytes; 1: elements).  threads: of the one workgroup a row has, 256 up to 1024 accesses per
 * row and 1024 above, in both phases.  topk / topp: the selections that run in phase A; k = min(top_k, V) where topk.  key_bits,
 * key_passes, index_bits, index_passes, frac_bits: as in the sampling unit's form.  grid_a workgroups walk the B * (S + 1)
 * positions of phase A, grid_b the B sequences of phase B; 0 with B == 0. */
typedef struct fa_spec_sample_form {
    int32_t cw, threads, topk, topp, k;
    int32_t key_bits, key_passes, index_bits, index_passes;
    int32_t frac_bits, grid_a, grid_b;
} fa_spec_sample_form;
/* validate first: its status on failure, and *plan untouched */
int fa_spec_sample_plan(const fa_spec_sample_params *params, fa_spec_sample_form *plan);

#ifdef __cplusplus
}
#endif
#endif /* FA_SPEC_SAMPLE_H_ */
