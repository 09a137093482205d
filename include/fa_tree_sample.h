/*
 * fa_tree_sample.h -- C ABI of the fused acceptance walk over a draft token TREE (csrc/fa_tree_sample.hip): the sampling step of
 * a tree-shaped verify step of speculative decoding (SpecInfer, arXiv 2305.09781, multi-round rejection; Medusa / EAGLE with top-m
 * children).  Not in the reference, which verifies chains only.  Two launches behind one entry, no sort, no host synchronisation.
 * A header of its own: every header of include/ declares one unit.  The kept sets, the arithmetic and the uniforms are those of
 * the chain verification, which takes them from the token sampling unit; a chain-shaped tree gives
 * the chain verification's tokens bit for bit.  Status codes, dtype codes and fa_strerror are those of fa_fwd.h.
 *
 * Per sequence b, with T nodes, 1 <= T <= 64 (the limit of the tree attention):
 *   parents       int32 (B, T).  Node 0 is the root: the last committed token, always on the path, never tested; parents[b, 0] is
 *                 not read.  Node i > 0 has its parent parents[b, i] in [0, i); any other value (negative: the padding of ragged
 *                 trees, as tree_mask_from_parents has it) makes i an absent node, which is never visited.  The children of n are
 *                 the nodes i with parents[b, i] == n, in ascending i.
 *   tokens_draft  int32 / int64 (B, T): the token of node i.  Entry 0 is not read.
 *   logits        (B, T, V): row n is the target model's distribution of the token that follows node n.
 *   logits_draft  (B, T, V) or NULL: row n is the distribution the children of node n were drawn from, independently (duplicates
 *                 allowed).  NULL: a deterministic drafter, the one-hot rule below.
 *   kept sets     of every target row and every draft row as in DESIGN 4.28: s = logits / temperature (one fp32 division, -0 counts
 *                 as +0), top-k with all ties of the k-th value staying, then top-p.  e_i = exp2((s_i - m) log2 e) in fp32,
 *                 w_i = trunc(e_i 2^F), Z_kept the 64-bit sum of the w_i, P_i = fp32((double)(e_i 2^F) / (double)Z_kept) of a
 *                 target row, Q_i of a draft row; 0 outside the kept set and in a row that keeps nothing.
 *                 F = min(40, 62 - ceil(log2 V)).
 *   walk          n = 0.  The children of n are tried in ascending order as rounds r = 0, 1, ..., child i with the uniform
 *                 u_acc[b, i] and its token x.  A token outside [0, V) is rejected, and nothing is read for it.
 *     draft rows  c_0 = 0, c_1 = 1.  For c > 0, r_i(c) = trunc(fmaf(-c, Q_i, P_i) 2^F) where that fp32 value is positive, else 0,
 *                 over the rows (b, n); R(c) their 64-bit sum.  Round 0 accepts iff (double)u (double)Q(x) <= (double)P(x): the
 *                 chain's test.  Round r >= 1 accepts iff (double)u (double)Q(x) (double)R(c_r) <= (double)r_x(c_r).  After the
 *                 rejection of round r >= 1, c_{r+1} = fp32((double)c_r + (double)R(c_r) 2^-F).  (SpecInfer renormalises the
 *                 residual max(P - Q, 0) after every rejection and subtracts Q again.  max(max(P - c Q, 0) - s Q, 0) =
 *                 max(P - (c + s) Q, 0): the residual after r rejections is max(P - c_r Q, 0) up to its norm R(c_r), so one
 *                 scalar stands for the row and no row is rewritten.)  R(c) == 0 after a rejection: the siblings left are not
 *                 tried.
 *     one-hot     (no draft rows) the weights at n are the w_i of the target row with the tokens rejected at n so far set to 0;
 *                 Z_r is Z_kept minus the weights of the distinct rejected tokens.  A child is accepted iff its w_x (after the
 *                 zeroing: 0 for a token rejected before at n, and outside the kept set) is positive and
 *                 (double)u (double)Z_r <= (double)w_x.  Z_r == 0 after a rejection: the siblings left are not tried.
 *                 Accepting child i sets n = i, and the walk goes on with the children of i; the rounds begin again.
 *   the draw      at the last n.  Draft rows: after m >= 1 rejections at n with R(c_m) > 0 the weights are r_i(c_m), R = R(c_m);
 *                 with no child at n, or R(c_m) == 0, the w_i of the target row, R = Z_kept.  One-hot: the w_i of the target row
 *                 without the rejected tokens, R = Z_r.  Walked in ascending index order, the token is the first index whose
 *                 inclusive cumulative weight exceeds floor(u_res[b] R) (fp64 product); where u >= 1 leaves none, the last index
 *                 of positive weight.  R == 0 (a target row that keeps nothing; one-hot: nothing left) gives token 0.
 *   outputs       path int32 (B, T): the nodes of the accepted path in ascending order, path[b, 0] = 0, 0 behind path_len;
 *                 path_len int32 (B): their number, the root included: what kvcache_keep_tree_path_ takes.  tokens (B, T) of the
 *                 dtype of tokens_draft: the tokens of the accepted nodes in path order without the root's, the drawn token in
 *                 column path_len - 1, 0 behind it.  num_generated int64 (B) = path_len: path_len - 1 accepted drafts and the
 *                 drawn token.
 *   stats         optional, (B, T) per node: p_tok, q_tok fp32, the round-0 P(x) and Q(x) of node i > 0 with a parent in [0, i)
 *                 from the rows of that parent (one-hot: Q = 1) and 0 for a token outside [0, V), an absent node and the root;
 *                 visited int32, 1 where the node's test ran; accepted int32.
 * The result is a function of the arguments alone: all sums are 64-bit integers, so no result depends on the order in which
 * threads arrive, and the same call gives the same bits.  NaN logits are not legal; nothing is read or written out of bounds
 * because of one, nor because of any value in parents or tokens_draft.
 *
 * Uniforms: u_acc (B, T) (entry 0 unused) and u_res (B) fp32 in [0, 1), or rng_state = {seed, offset} on the device and the
 * counter hash of the sampling unit, with row index b * T + i for node i and B * T + b for the draw of b.
 *
 * Two launches, ordered by the stream.  Phase A: one workgroup per row (b, n) selects the kept set of the target row and, with
 * draft rows, of the draft row of every node that has a child, and writes a record of 24 bytes per row into `workspace`:
 *     float m (the maximum of s; -inf: nothing kept) | uint32 K | int32 J | int32 flags (0) | uint64 Z_kept
 * (K, J): kept are the entries whose cut key is above K, and those with key K and index below J.  Target records at b * T + n,
 * draft records at B * T + b * T + n (not written for a node without children, and never read).  Phase B: one workgroup per b
 * holds parents, tokens and uniforms in LDS, walks down from the root with the records, selecting nothing again, draws and
 * writes the outputs.  No workgroup waits for another inside a launch.
 *
 * logits and logits_draft have one dtype (fp16, bf16, fp32), a unit column stride, and batch and node strides in elements; rows
 * are addressed in 64 bits.  tokens_draft and parents have a batch stride in elements and a unit node stride; the outputs and the
 * uniforms are contiguous.  1 <= V < 2^31, 1 <= T <= 64, 0 <= B, B * 2 T < 2^31 (FA_ERR_BAD_SHAPE); B == 0 is FA_OK and launches
 * nothing.  temperature > 0, 0 <= top_p <= 1, top_k >= 0 (FA_ERR_BAD_SHAPE; NaN fails).  Exactly one source of uniforms: u_res
 * (with u_acc where T > 1), or rng_state (FA_ERR_NULL_POINTER: neither, or one of u_res / u_acc without the other where T > 1;
 * FA_ERR_BAD_SHAPE: both).  workspace holds fa_tree_sample_workspace_size(B, T) bytes, 8-byte aligned (FA_ERR_WORKSPACE: NULL or
 * workspace_bytes too small).  Pointers keep the natural alignment of their element (FA_ERR_BAD_STRIDE).
 * Rows are taken by 16-byte accesses where every logits tensor given qualifies: the bases, every pitch in bytes that is used
 * (batch with B > 1, node with T > 1) and V * element size are multiples of 16; by element accesses otherwise.
 *
 * Known limit: phase B is sequential per sequence, (rejections + 1) walks of the one or two rows of a node; one workgroup per
 * row.  A form that splits a row over workgroups is not part of this unit.  Sampling the children without replacement (a Q
 * renormalised per sibling) is not expressible by one scalar c and is not part of it either.
 */
#ifndef FA_TREE_SAMPLE_H_
#define FA_TREE_SAMPLE_H_

#include "fa_fwd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_TREE_TOKENS_INT32 0
#define FA_TREE_TOKENS_INT64 1
#define FA_TREE_RECORD_BYTES 24
#define FA_TREE_SAMPLE_MAX_NODES 64

typedef struct fa_tree_sample_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    const void *logits;        /* (B, T, V) */
    const void *logits_draft;  /* (B, T, V), or NULL: the one-hot rule */
    const void *tokens_draft;  /* (B, T) */
    const int32_t *parents;    /* (B, T) */
    const float *u_acc;        /* (B, T) uniforms in [0, 1), or NULL */
    const float *u_res;        /* (B) uniforms in [0, 1), or NULL */
    const uint64_t *rng_state; /* device {seed, offset}, or NULL */
    void *workspace;           /* fa_tree_sample_workspace_size(B, T) bytes */
    int32_t *path;             /* (B, T) */
    int32_t *path_len;         /* (B) */
    void *tokens;              /* (B, T) of tokens_dtype */
    int64_t *num_generated;    /* (B) */
    float *p_tok;              /* (B, T) or NULL */
    float *q_tok;              /* (B, T) or NULL */
    int32_t *visited;          /* (B, T) or NULL */
    int32_t *accepted;         /* (B, T) or NULL */
    int64_t logits_batch_stride, logits_node_stride; /* in elements */
    int64_t draft_batch_stride, draft_node_stride;
    int64_t tokens_draft_batch_stride, parents_batch_stride;
    int64_t workspace_bytes;
    int64_t B;
    int32_t T;
    int32_t V;
    int32_t logits_dtype; /* FA_DTYPE_FP16 / FA_DTYPE_BF16 / FA_DTYPE_FP32, of both logits tensors */
    int32_t tokens_dtype; /* FA_TREE_TOKENS_* */
    int32_t top_k;
    float top_p;
    float temperature;
    int32_t reserved;
} fa_tree_sample_params;

/* the checks of the launch entry without a device: FA_OK or the status the entry would return before it launches */
int fa_tree_sample_validate(const fa_tree_sample_params *params);
/* asynchronous on `stream` (a hipStream_t; NULL: the default stream); no host synchronisation, no allocation */
int fa_tree_sample(const fa_tree_sample_params *params, void *stream);
uint32_t fa_tree_sample_params_size(void);
/* bytes of the records of a call, a target and a draft record per node; 0 where B is negative or T < 1 */
int64_t fa_tree_sample_workspace_size(int64_t B, int32_t T);

/* The form a call takes, filled by the host function the launch itself consumes (the kernels get this struct); no device.
 * cw: elements per access (8 / 4: 16 bytes; 1: elements).  threads: of the one workgroup a row has, 256 up to 1024 accesses per
 * row and 1024 above, in both phases.  drafts: 1 with draft rows, 0 under the one-hot rule.  topk / topp: the selections that
 * run in phase A; k = min(top_k, V) where topk.  key_bits, key_passes, index_bits, index_passes, frac_bits: as in the sampling
 * unit's form.  grid_a workgroups walk the B * T rows of phase A, grid_b the B sequences of phase B; 0 with B == 0. */
typedef struct fa_tree_sample_form {
    int32_t cw, threads, drafts, topk, topp, k;
    int32_t key_bits, key_passes, index_bits, index_passes;
    int32_t frac_bits, grid_a, grid_b;
} fa_tree_sample_form;
/* validate first: its status on failure, and *plan untouched */
int fa_tree_sample_plan(const fa_tree_sample_params *params, fa_tree_sample_form *plan);

#ifdef __cplusplus
}
#endif
#endif /* FA_TREE_SAMPLE_H_ */
