/*
 * fa_sample.h -- C ABI of the fused top-k / top-p token sampling (csrc/fa_sample.hip): the step between (B, V) logits and the
 * next token that the reference builds from torch calls in flash_attn.utils.generation (sample, modify_logits_for_top_k_filtering,
 * modify_logits_for_top_p_filtering; flash_attn/utils/generation.py:45-95).  One launch, one workgroup per row, no sort.  A header
 * of its own: fa_fwd.h, its ABI version and the kernel sets of the other units are what they were.  Status codes, dtype codes and
 * fa_strerror are those of fa_fwd.h.
 *
 * The result is a function of (logits, top_k, top_p, temperature, u): no tie is left to the order in which threads arrive.
 * Per row, s_i = logits_i / temperature, one correctly rounded fp32 division (-0 counts as +0):
 *   top-k   top_k == 1: token = argmax s, the lowest index among equal maxima; nothing else is computed (FA_SAMPLE_DRAW only).
 *           top_k >= 2: the candidate set C is exactly min(top_k, V) entries with the largest s; among equal s the lower index
 *           is taken.  top_k == 0 or top_k >= V: C is the row.
 *   top-p   with 0 < top_p < 1: p_i = softmax of s over C.  C in ascending order of (p_i, -index): among equals the higher
 *           index comes first.  Every entry whose inclusive cumulative probability in that order is <= 1 - top_p leaves C; the
 *           largest entry never does.
 *   draw    p renormalised over what is left, walked in ascending index order: token = the first index whose inclusive
 *           cumulative probability exceeds u; the last kept index if rounding leaves the total at or below u.
 * -inf logits are legal and are never chosen while a finite one exists; a row of nothing but -inf gives token 0, kept 0, mass 0
 * (and is left as it is by FA_SAMPLE_FILTER).  NaN logits are not legal; nothing on the device checks for them, and nothing
 * is read or written out of bounds because of one.
 *
 * The arithmetic: s, the maximum m and e_i = exp2((s_i - m) * log2 e) are fp32.  Sums of e are taken in fixed point, e_i * 2^F
 * truncated to an integer with F = min(40, 62 - ceil(log2 V)) (F = 40 up to V = 2^22), in 64 bits: a sum does not depend on the
 * order of its terms, so LDS atomics make the histograms and the call still gives the same bits every time.  The comparison
 * values are floor((1 - top_p) * Z) and floor(u * Z_kept), formed once per row in fp64 from the fp32 scalars.
 *
 * u: B fp32 uniforms in [0, 1).  Or rng_state = {seed, offset} on the device, from which the kernel forms the uniform of row r:
 *   x = (uint32)seed ^ (uint32)(seed >> 32) * 0x27D4EB2F ^ (uint32)offset * 0xC2B2AE3D ^ (uint32)(offset >> 32)
 *   x ^= x >> 15;  x *= 0x2C1B3C6D;  x ^= x >> 12                                  (the seed mix of DESIGN 4.26)
 *   h = lowbias32((x ^ (uint32)(r >> 32) * 0x2545F491) ^ (uint32)r * 0x9E3779B1)
 *   lowbias32(y): y ^= y >> 16; y *= 0x7FEB352D; y ^= y >> 15; y *= 0x846CA68B; y ^= y >> 16
 *   u_r = (h >> 8) * 2^-24
 * (all products modulo 2^32).  utils.generation.uniform_ref restates it in torch.
 *
 * FA_SAMPLE_FILTER writes -inf over the entries that leave, in place, and draws nothing:
 *   top-k   with top_k >= 1: entries below the min(top_k, V)-th largest value leave; ALL entries equal to it stay
 *           (logits < kth, reference :45-48), which differs from the exactly-k rule of the draw on purpose
 *   top-p   with 0 < top_p < 1: the rule above on what is left
 * kept and mass are written as in a draw.
 *
 * logits: B rows of V elements of fp16, bf16 or fp32, unit column stride, a row stride in elements; rows are addressed in 64
 * bits (B * stride may pass 2^31).  1 <= V < 2^31 and B >= 0 (FA_ERR_BAD_SHAPE); B == 0 is FA_OK and launches nothing.
 * temperature > 0, 0 <= top_p <= 1, top_k >= 0: FA_ERR_BAD_SHAPE otherwise (NaN fails).  token (B) int64; kept (B) int32 and
 * mass (B) fp32 are optional, and must be NULL with top_k == 1 in a draw, which computes neither (FA_ERR_BAD_SHAPE).  A draw with
 * top_k != 1 takes exactly one of u and rng_state (FA_ERR_NULL_POINTER: neither; FA_ERR_BAD_SHAPE: both).  Pointers keep the
 * natural alignment of their element, rng_state 8 bytes (FA_ERR_BAD_STRIDE).  In FA_SAMPLE_FILTER rows do not overlap (row
 * stride >= V where B > 1: FA_ERR_BAD_STRIDE) and token is not used.
 * Rows are taken by 16-byte accesses where the base, the pitch in bytes (with B > 1) and V * element size are multiples of 16;
 * by element accesses otherwise.
 *
 * Known limit: one workgroup per row.  With B below the number of compute units most of the device idles, and a row of 150k
 * bf16 entries is 300 KB per walk out of L2; a form that splits a row over workgroups is not part of this unit.
 */
#ifndef FA_SAMPLE_H_
#define FA_SAMPLE_H_

#include "fa_fwd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_SAMPLE_DRAW 0   /* write token (and kept, mass) */
#define FA_SAMPLE_FILTER 1 /* write -inf over the removed entries of logits */

typedef struct fa_sample_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size;
    void *logits;              /* (B, V); written only with FA_SAMPLE_FILTER */
    const float *u;            /* (B) uniforms in [0, 1), or NULL */
    const uint64_t *rng_state; /* device {seed, offset}, or NULL */
    int64_t *token;            /* (B) */
    int32_t *kept;             /* (B) or NULL: the size of the final candidate set */
    float *mass;               /* (B) or NULL: its probability before renormalising (within C where top-k ran) */
    int64_t logits_row_stride; /* in elements */
    int64_t B;
    int32_t V;
    int32_t logits_dtype; /* FA_DTYPE_FP16 / FA_DTYPE_BF16 / FA_DTYPE_FP32 */
    int32_t mode;         /* FA_SAMPLE_* */
    int32_t top_k;
    float top_p;
    float temperature;
} fa_sample_params;

/* the checks of the launch entry without a device: FA_OK or the status the entry would return before it launches */
int fa_sample_validate(const fa_sample_params *params);
/* asynchronous on `stream` (a hipStream_t; NULL: the default stream); no host synchronisation, no allocation */
int fa_sample(const fa_sample_params *params, void *stream);
uint32_t fa_sample_params_size(void);

/* The form a call takes, filled by the host function the launch itself consumes (the kernel gets this struct); no device.
 * cw: elements per access (8 / 4: 16 bytes; 1: elements).  threads: of the one workgroup a row has, 256 up to 1024 accesses per
 * row and 1024 above.  greedy: the argmax kernel.  topk / topp / draw: the phases that run; k = min(top_k, V) where topk.
 * A phase selects by radix descent over histograms of 2048 bins in LDS: over the key_bits significant bits of the order-preserving
 * key of s in key_passes walks of the row (16 / 19 bits of a bf16 / fp16 row at temperature 1, else 32), or over the index_bits
 * bits of a column index in index_passes walks.  frac_bits: F above.  grid_x workgroups walk the rows; 0 with B == 0. */
typedef struct fa_sample_form {
    int32_t cw, threads, mode, greedy;
    int32_t topk, topp, draw, k;
    int32_t key_bits, key_passes, index_bits, index_passes;
    int32_t frac_bits, grid_x;
} fa_sample_form;
/* validate first: its status on failure, and *plan untouched */
int fa_sample_plan(const fa_sample_params *params, fa_sample_form *plan);

#ifdef __cplusplus
}
#endif
#endif /* FA_SAMPLE_H_ */
