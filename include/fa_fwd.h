/*
 * fa_fwd.h — C-ABI of the MI355X (gfx950) FlashAttention forward.
 *
 * This is the drop-in boundary of the hot path.  Plain C, raw
 * device pointers, element strides, int status codes; no torch types.  It is
 * what a binding for the reference's forward entry points would call:
 *
 *   reference interface replaced                                  entry point here
 *   ------------------------------------------------------------  -----------------
 *   mha_fwd          csrc/flash_attn/flash_api.cpp:350-512        fa_fwd (dense)
 *   mha_varlen_fwd   csrc/flash_attn/flash_api.cpp:514-755        fa_fwd (cu_seqlens_* set)
 *   mha_fwd (FA3)    hopper/flash_api.cpp:672-1198                fa_fwd (+ seqused_*, fp8 e4m3 + descale)
 *   set_params_fprop csrc/flash_attn/flash_api.cpp:26-159         fa_fwd_params (field for field)
 *   Flash_fwd_params csrc/flash_attn/src/flash.h:48-143,
 *                    hopper/flash.h:37-168                        fa_fwd_params
 *   flash_attention_forward(FlashAttentionParams&, cudaStream_t)
 *                    standalone/include/flash_api.h:222-225       fa_fwd(const fa_fwd_params*, void*)
 *   mha_fwd_kvcache  csrc/flash_attn/flash_api.cpp:1202-1476      fa_kvcache_append + fa_fwd (seqused_k, kv_batch_idx)
 *   mha_fwd (FA3) over an fp8 KV cache, 16-bit q
 *                    hopper/flash_api.cpp:714-760, 1115-1146      fa_fwd_kv8 (k / v e4m3 bytes + k / v descale)
 *   ... with k_new / v_new, rotary (the append into that cache)   fa_kvcache_append_kv8 (16-bit rows -> e4m3 bytes)
 *   ... the append into a cache of the MLA shape                   fa_kvcache_append_qv8
 *   error codes      standalone/src/flash_api.cu:403-426          FA_ERR_* / fa_strerror
 *
 * Conventions (same as the reference's params struct):
 *   - strides are in ELEMENTS, not bytes (csrc/flash_attn/flash_api.cpp:64-73);
 *     the last (head_dim) stride of q/k/v/o must be 1;
 *   - dense layout  q:(b, seqlen_q, h, d)  k,v:(b, seqlen_k, h_k, d)  o like q,
 *     softmax_lse:(b, h, seqlen_q) fp32;
 *   - varlen layout q:(total_q, h, d) k,v:(total_k, h_k, d), cu_seqlens_{q,k}
 *     int32 (b+1) device arrays, softmax_lse:(h, total_q) fp32
 *     (csrc/flash_attn/flash_api.cpp:652); *_batch_stride is ignored;
 *   - ragged queries over a batched cache (flash_attn_with_kvcache(..., cu_seqlens_q=), hopper/flash_api.cpp:736-760):
 *     cu_seqlens_q set, cu_seqlens_k NULL, seqused_k set.  q / o / qv and softmax_lse are varlen ((total_q, h, .),
 *     (h, total_q)); k / v are the dense cache (b_cache, seqlen_k, h_k, .) addressed by *_batch_stride and kv_batch_idx,
 *     or pages behind block_table; seqlen_k is the cache capacity, seqused_k the fill levels (see fa_fwd_params);
 *   - the callee never allocates, never synchronises and launches on `stream`;
 *   - outputs are written in place; inputs are borrowed.
 */
#ifndef FA_FWD_H_
#define FA_FWD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FA_ABI_VERSION 13

#define FA_FLAG_FA3_WINDOW 1
#define FA_FLAG_SDMASK_SIGNED 2   /* s_dmask is the reference's sign-encoded probability tensor (below), not random bytes */
#define FA_FLAG_PACK_GQA 4        /* hint (FA3 pack_gqa = True): pack the h / h_k query heads of a kv head into the rows of a tile */

/* element types of q/k/v (o has the same type; fp8 inputs produce bf16 o) */
enum fa_dtype {
    FA_DTYPE_FP16 = 0,
    FA_DTYPE_BF16 = 1,
    FA_DTYPE_FP8_E4M3 = 2, /* OCP e4m3fn; hopper/flash_api.cpp:714-722 */
    FA_DTYPE_FP32 = 3      /* output type of fa_fwd_combine only */
};

/* status codes: 0 ok, negative = rejected before launch, nothing was written */
enum fa_status {
    FA_OK = 0,
    FA_ERR_NULL_POINTER = -1,      /* a required pointer is NULL */
    FA_ERR_BAD_DTYPE = -2,         /* "FlashAttention only support fp16 and bf16 data type" */
    FA_ERR_BAD_HEAD_DIM = -3,      /* d > 256 or d % 8 != 0 */
    FA_ERR_BAD_HEADS = -4,         /* h % h_k != 0 */
    FA_ERR_BAD_SHAPE = -5,         /* b <= 0, negative lengths, ... */
    FA_ERR_BAD_STRIDE = -6,        /* misaligned rows: strides must keep 16-byte row alignment */
    FA_ERR_UNSUPPORTED = -7,       /* feature accepted by the ABI but not built for this combination */
    FA_ERR_LAUNCH = -8,            /* hipLaunchKernel failed */
    FA_ERR_BAD_ABI = -9,           /* params->abi_version / struct size mismatch */
    FA_ERR_NO_DEVICE = -10,        /* not a gfx950 device */
    FA_ERR_WORKSPACE = -11         /* fp8 inputs / split-KV need params->workspace of fa_fwd_workspace_size() bytes */
};

/*
 * Mirrors Flash_fwd_params (csrc/flash_attn/src/flash.h:48-143) restricted to
 * the forward hot path, plus the FA3 additions used by BASELINE config 5
 * (hopper/flash.h:37-168: seqused_q/k, q/k/v descale).
 */
typedef struct fa_fwd_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size; /* sizeof(fa_fwd_params) */

    /* tensors (device pointers) */
    const void *q;
    const void *k;
    const void *v;
    void *o;
    float *softmax_lse;

    /* element strides; head_dim stride is 1 */
    int64_t q_batch_stride, q_row_stride, q_head_stride;
    int64_t k_batch_stride, k_row_stride, k_head_stride;
    int64_t v_batch_stride, v_row_stride, v_head_stride;
    int64_t o_batch_stride, o_row_stride, o_head_stride;

    /* sizes */
    int32_t b;        /* batch (varlen: number of sequences) */
    int32_t seqlen_q; /* dense: seqlen_q; varlen: max_seqlen_q */
    int32_t seqlen_k; /* dense: seqlen_k; varlen: max_seqlen_k */
    int32_t h;        /* query heads */
    int32_t h_k;      /* key/value heads; h % h_k == 0; q head i reads kv head i / (h/h_k) */
    int32_t d;        /* head dim, multiple of 8, <= 256 */
    int32_t total_q;  /* varlen: rows of q (lse row length); dense: ignored */
    int32_t dtype;    /* enum fa_dtype */

    /* varlen bookkeeping (NULL => dense); BlockInfo csrc/flash_attn/src/block_info.h:12-45 */
    const int32_t *cu_seqlens_q; /* (b+1) */
    const int32_t *cu_seqlens_k; /* (b+1); NULL beside cu_seqlens_q = ragged queries over a batched cache (below) */
    const int32_t *seqused_q;    /* (b) optional: rows actually used (FA3 hopper/seqlen.h:32-93) */
    const int32_t *seqused_k;    /* (b) optional: keys actually used */

    /* softmax */
    float softmax_scale; /* scores = q.k * softmax_scale */
    float softcap;       /* >0: scores = softcap * tanh(scores / softcap) */

    /* masking: bottom-right aligned (flash_attn/flash_attn_interface.py:1164-1174) */
    int32_t is_causal;         /* != 0 => window_size_right = 0 */
    int32_t window_size_left;  /* <0: unbounded */
    int32_t window_size_right; /* <0: unbounded */

    /* fp8 only: per-(batch, kv head) fp32 descales (hopper/flash_api.cpp:1115-1146); NULL = 1.0 */
    const float *q_descale, *k_descale, *v_descale;
    int64_t q_descale_batch_stride, q_descale_head_stride;
    int64_t k_descale_batch_stride, k_descale_head_stride;
    int64_t v_descale_batch_stride, v_descale_head_stride;

    /* performance hint, never changes results: 0 = library default */
    int32_t kernel_variant;
    int32_t total_k;      /* varlen: rows of k/v (only needed for fp8 inputs: size of the expansion workspace) */

    /* caller-provided scratch (the callee never allocates), 256-byte aligned, fa_fwd_workspace_size() bytes.
     * fp8: head dim 128 (dense / varlen / causal / right window) runs natively -- e4m3 operands straight into the block-scaled
     * MFMA, no workspace (fa_fwd_workspace_size() returns 0).  The other fp8 shapes (other head dims, softcap, left windows,
     * K or V of 2 GiB or more per batch entry) expand q/k/v to bf16 here (exact: every e4m3 value is a bf16 value) and run the
     * 16-bit mainloop; either way the descales are folded into the softmax scale and the final normalisation.
     * 16-bit dense problems that split the key range (num_splits) keep their fp32 partial O / LSE here. */
    void *workspace;
    uint64_t workspace_bytes;

    /* ALiBi (csrc/flash_attn/src/alibi.h:18-71, set_params_alibi csrc/flash_attn/flash_api.cpp:331-349): fp32 slopes,
     * (h) [batch stride 0] or (b, h); NULL = off.  The bias added to the scaled (and soft-capped) score of query i,
     * key j is  -slope * |i + seqlen_k - seqlen_q - j|  (tests/test_flash_attn.py:29-56); under a causal mask this
     * differs from the reference kernel's  +slope * j  only by a per-row constant (same O; LSE includes the bias). */
    const float *alibi_slopes;
    int64_t alibi_slopes_batch_stride;

    /* KV-cache decode (mha_fwd_kvcache csrc/flash_attn/flash_api.cpp:1202-1476; FA3 kv_batch_idx
     * hopper/flash_api.cpp:686): dense K/V layout only; batch i reads k/v rows of cache entry kv_batch_idx[i]
     * (NULL = i).  The valid length of each cache entry is given through seqused_k.
     * Ragged queries over the cache -- one serving step that mixes prefill chunks with single-token decodes: cu_seqlens_q
     * set, cu_seqlens_k NULL, seqused_k set (required).  q, o, qv: (total_q, h, .) with q/o/qv_batch_stride ignored,
     * softmax_lse (h, total_q); k, v: the cache, (b_cache, seqlen_k, h_k, .) through k/v_batch_stride and kv_batch_idx, or
     * paged through block_table; seqlen_k = the cache capacity (it bounds the key tiles), seqlen_q = max_seqlen_q;
     * leftpad_k as on the dense route.  Every 16-bit mask (causal, windows, softcap), seqused_q, qv (on the qv kernel) and
     * split-KV.  FA_ERR_UNSUPPORTED with fp8, dropout or ALiBi.  cu_seqlens_k without cu_seqlens_q: FA_ERR_BAD_SHAPE. */
    const int32_t *kv_batch_idx;

    /* Paged KV cache (csrc/flash_attn/flash_api.cpp:1245-1266, 538-560; src/flash_fwd_kernel.h:560-576): k and v are
     * (num_blocks, page_block_size, h_k, d) -- k/v_batch_stride is the page stride -- and key row j of batch i lives in
     * page block_table[i * block_table_batch_stride + j / page_block_size], row j % page_block_size.
     * Any page_block_size >= 1 (multiples of 64 take the tile-granular lookup, others a per-row one).  NULL = contiguous. */
    const int32_t *block_table;
    int64_t block_table_batch_stride;
    int32_t page_block_size;
    /* Split-KV (set_params_splitkv / num_splits_heuristic csrc/flash_attn/flash_api.cpp:257-329, combine kernel
     * src/flash_fwd_kernel.h:1108-1290): 1 = off, N > 1 = the key range of every tile is cut into N parts computed by
     * N workgroups and merged by a second launch, 0 = library heuristic (splits only dense problems and ragged queries
     * over a cache with few tiles, i.e. decode; the tiles of a ragged batch are counted from total_q and seqlen_q, never from
     * device data).  cu_seqlens_q + cu_seqlens_k problems never split, nor do dropout, fp8 and attention_chunk problems
     * (any num_splits is planned as 1 there).  Ragged queries over a cache keep partials of
     * (splits, total_q, h, d_v) + (splits, h, total_q) fp32.  Needs params->workspace of fa_fwd_workspace_size() bytes when the effective value is > 1 (the partial
     * outputs and LSEs of the parts, both fp32 like the reference's out_accum / softmax_lse_accum).
     * The default-initialised struct (0) therefore may split: callers without a workspace must pass 1. */
    int32_t num_splits;

    /* Left-padded keys (leftpad_k of mha_varlen_fwd / mha_fwd_kvcache, csrc/flash_attn/src/block_info.h:22-35): the first
     * leftpad_k[i] key rows of batch i are padding -- the kernel starts reading at row leftpad_k[i] and the valid length
     * becomes (seqused_k or the sequence length) - leftpad_k[i].  (b) int32 or NULL.  Not with block_table. */
    const int32_t *leftpad_k;

    /* Attention dropout (csrc/flash_attn/flash_api.cpp:486-493, src/dropout.h).  p_dropout in [0, 1): every probability
     * is kept with probability ~(1 - p) and the kept ones scaled by 1 / (1 - p).  The decision for (batch, head, query i,
     * key j) is an 8-bit counter-based random value r = fa_rand8(seed, offset, batch * h + head, i, j) compared with
     * floor(255 (1 - p)): kept iff r <= floor(255 (1 - p)) -- the "randval" convention of the reference's ROCm tests
     * (tests/test_flash_attn_ck.py:34-38).  rng_state: device pointer to {seed, offset} (2 x uint64), read by the
     * kernel (no host sync), the same pair must be given to fa_bwd.  s_dmask (optional, testing): receives r as uint8,
     * dense (b, h, seqlen_q, seqlen_k), varlen (h, total_q, seqlen_k [= max_seqlen_k]).  Dropout runs on the
     * compiler-scheduled kernel shape (no split-KV). */
    float p_dropout;
    /* FA_FLAG_* bits.  FA_FLAG_FA3_WINDOW: window sides follow the FA3 rule (hopper/flash_api.cpp:152-153, 589-590): a
     * negative side is UNBOUNDED and stays so; without the flag a one-sided window gets seqlen_k on the other side as
     * set_params_fprop does (csrc/flash_attn/flash_api.cpp:141-142), which masks rows when seqlen_q > seqlen_k.
     * FA_FLAG_PACK_GQA (hopper/pack_gqa.h; no ABI change: a bit of this field): a performance hint that never changes what is
     * computed.  Honoured -- one workgroup per block of (query row, head of the GQA group) pairs of one kv head, pk_fwd_kernel
     * in fa_fwd_plan_name -- exactly when h > h_k, the type is 16-bit, d <= 128, and the call has no ALiBi, dropout,
     * attention_chunk, V head dim of its own or qv; every other call runs as without the bit.  Dense, varlen, seqused_*, caches
     * (kv_batch_idx, leftpad_k, paged), ragged queries over a cache, split-KV, softcap and fa_fwd_sink are all served.
     * fa_fwd_block_sparse ignores it. */
    int32_t flags;
    const uint64_t *rng_state;
    uint8_t *s_dmask;
    /* ABI v11 -- FA_FLAG_SDMASK_SIGNED: s_dmask is what the reference's CUDA forward returns for return_softmax
     * (csrc/flash_attn/src/flash_fwd_kernel.h:350-360, src/dropout.h:26-33; decoded by tests/test_flash_attn.py:411-526):
     * (b, h, s_dmask_rows, s_dmask_cols) elements of the INPUT dtype, row-major, rows / cols = seqlen_q / seqlen_k rounded up
     * to 128 (varlen: the max_seqlen's; batch entry i's block at [i, :, 0:seqlen_q_i, 0:seqlen_k_i]).  Element (row, key) =
     * exp(score - m) with m the maximum of the row's scores over key blocks [key / s_dmask_block_n, last] -- the running
     * maximum of a sweep that walks the key blocks from the last to the first, as the reference's kernel does -- and a
     * NEGATIVE sign where dropout discards the element.  s_dmask_block_n = the reference's kBlockN for this head dim
     * (flash_attn/flash_attn_interface.py:23-46).  Testing aid like the reference's: written by a pass of its own behind the
     * forward (fa_sdmask in fa_fwd_api.hip), seqlen_k <= 32768. */
    int32_t s_dmask_rows, s_dmask_cols, s_dmask_block_n;
    /* ABI v12 -- attention_chunk (FA3, hopper/flash_api.cpp:148-160, hopper/mask.h:116-119, hopper/block.h:30-42; oracle
     * construct_chunk_mask hopper/test_util.py:193-223): C > 0 = query i only sees the keys of its own chunk,
     * [floor((i + seqlen_k - seqlen_q) / C) * C, ... + C), intersected with the causal / window mask.  0 = off.  Forward only
     * (the reference's backward has no such argument, hopper/flash_api.cpp:1523), 16-bit and expanded-fp8 kernels. */
    int32_t attention_chunk;
    /* ABI v12 -- head dim of V and O when it differs from d (FA3 "headdim_v", hopper/flash_api.cpp:764,782-792: q/k in
     * (128, 192] with v in (96, 128], or q/k <= 64 with v <= 512): v is (.., h_k, d_v), o (.., h, d_v).  0 = d.  Multiple of 8,
     * <= 512; above 256 the library runs one launch per 256 columns of V.  16-bit types; not with split-KV, paged or fp8 --
     * except d <= 64 beside d_v in [256, 512], which runs the qv kernel below on paged caches and with split-KV too. */
    int32_t d_v;
    int32_t reserved_v12;
    /* ABI v13 -- FA3 `qv` (hopper/flash_api.cpp:1028-1048; oracle hopper/test_util.py:287-292): the score gets a second
     * product, scores = (q.k + qv.v) * softmax_scale, with qv of V's head dim: dense (b, seqlen_q, h, d_v), varlen
     * (total_q, h, d_v) (qv_batch_stride ignored).  NULL = off.  16-bit types, d <= 64, 256 <= d_v <= 512, 16-byte aligned
     * rows; every mask, softcap, seqused_*, varlen, leftpad_k, kv_batch_idx, paged K/V and split-KV (its partials are
     * (splits, b, seqlen_q, h, d_v) + (splits, b, h, seqlen_q) fp32 in the workspace).  Not with fp8, ALiBi or dropout
     * (FA3 has neither).  The query heads of one kv head are packed into the kernel's rows: one pass over K/V serves them. */
    const void *qv;
    int64_t qv_batch_stride, qv_row_stride, qv_head_stride;
} fa_fwd_params;

/* Validate and enqueue the forward on `stream` (a hipStream_t; NULL = default
 * stream).  Returns FA_OK or a negative fa_status; asynchronous. */
int fa_fwd(const fa_fwd_params *params, void *stream);

/* Scratch bytes fa_fwd needs in params->workspace for these params (0 for fp16/bf16 inputs; <0 = fa_status). */
int64_t fa_fwd_workspace_size(const fa_fwd_params *params);

/* Validation only (what mha_fwd's TORCH_CHECKs do); no device access. */
int fa_fwd_validate(const fa_fwd_params *params);

/* Test hook: a short, stable text naming the forward plan of these params on a device of num_cus compute units -- the kernel,
 * its template shape and forms, block_m, the split-KV count, the fp8 expansion and the 256-column calls of a wide V (e.g.
 * "fwd_kernel_w64 D=128 DEFF=128 waves=4 PERSIST block_m=256 splits=1").  NULL when fa_fwd would reject the params.  No
 * device access; the text lives in thread-local storage until the next call on the same thread. */
const char *fa_fwd_plan_name(const fa_fwd_params *params, int32_t num_cus);

/* Test hook: the name of the plan the calling thread's most recent fa_fwd() (or fa_fwd_sink, fa_fwd_block_sparse, fa_fwd_kv8, fa_fwd_qv8, fa_fwd_sparse_kv, fa_fwd_tree) launched (same text as fa_fwd_plan_name on that
 * call's params and the device's CU count; for a wide V run as several 256-column calls, the outer "... cols=N" plan).  NULL
 * before the first call or when that call failed validation; unspecified after a call that returned any other error (a failed
 * 256-column part leaves that part's plan).  fa_fwd keeps a struct copy; the text is made here, in
 * thread-local storage of its own, valid until the next call on the same thread. */
const char *fa_fwd_last_plan_name(void);

/*
 * Learnable attention sink -- `learnable_sink=` of flash_attn.cute.interface.flash_attn_func / flash_attn_varlen_func
 * (flash_attn/cute/interface.py:1141-1210; kernel side flash_attn/cute/softmax.py:111-141; oracle
 * flash_attn/cute/testing.py:376-387): one logit z per query head, in natural-log units (neither scaled by softmax_scale nor
 * soft-capped), that joins the softmax denominator and carries no value.  For query row i with final scores s_ij:
 *     m' = max(max_j s_ij, z)     l' = sum_j exp(s_ij - m') + exp(z - m')
 *     P_ij = exp(s_ij - m') / l'  O_i = sum_j P_ij v_j      LSE_i = m' + log l'   (the sink included)
 * The pair is rebased on the larger of the row maximum and the sink, so a sink far above every score gives LSE ~ z, never
 * inf.  A row without a visible key gives O = 0 and LSE = z (without a sink such rows keep +inf).  z = -inf is the call
 * without a sink, bit for bit in O and LSE.
 * fa_fwd_params has no room for a pointer (its size is pinned), so the sink travels in a struct of its own.  A sink never
 * changes the plan: fa_fwd_workspace_size, fa_fwd_plan_name and fa_fwd_last_plan_name read fa_fwd_params alone and mean
 * the same with and without one -- the sink is a run-time term of the kernels' epilogues (fwd_kernel, fwd_kernel_w64,
 * fwd_kernel_d256) and, under split-KV, of the merge (the parts write sink-free partials; fa_fwd_combine over caller-held
 * partials knows no sink).
 * Accepted: everything the 16-bit kernels take -- causal, both window sides, softcap, attention_chunk, d_v != d, varlen,
 * seqused_q/k, leftpad_k, kv_batch_idx, paged K/V, split-KV, ragged queries over a cache.  FA_ERR_UNSUPPORTED: fp8 inputs,
 * qv (and the other calls the qv kernel runs), dropout, ALiBi, s_dmask.
 */
typedef struct fa_sink_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size; /* sizeof(fa_sink_params) */
    const void *learnable_sink; /* device pointer, (h) logits through the strides below */
    int32_t sink_dtype;         /* FA_DTYPE_BF16 (the reference's) or FA_DTYPE_FP32 */
    /* row r of head g (as fa_fwd_params counts heads and rows) reads learnable_sink[g * sink_head_stride + r * sink_row_stride]:
     * (1, 0) normally; (h / h_k, 1) when the caller has folded the GQA group of a one-row decode step into the rows
     * ((b, 1, h, d) viewed as (b, h / h_k, h_k, d)).  sink_row_stride must be 0 with cu_seqlens_q.  Both >= 0. */
    int32_t sink_head_stride, sink_row_stride;
    int32_t reserved;
} fa_sink_params;

/* fa_fwd with a sink: same params, same plan, same workspace.  `sink` must not be NULL (use fa_fwd). */
int fa_fwd_sink(const fa_fwd_params *params, const fa_sink_params *sink, void *stream);
/* Validation only; the sink's own refusals are looked at before fa_fwd_validate's. */
int fa_fwd_sink_validate(const fa_fwd_params *params, const fa_sink_params *sink);
uint32_t fa_sink_params_size(void);

/*
 * Block-sparse forward -- `full_block_cnt / full_block_idx / mask_block_cnt / mask_block_idx` of
 * flash_attn.cute.interface.flash_attn_func (flash_attn/cute/interface.py:262-273, 377-385, 1004-1053; the list format
 * flash_attn/cute/block_sparsity.py:33-115; the kernel side flash_attn/cute/block_sparse_utils.py:265-419): the caller says
 * which key blocks each query block attends to.
 * Blocks are 128 query rows x 128 keys (the reference's m_block_size / n_block_size under block sparsity), whatever tile the
 * kernel uses inside.  nm = ceil(seqlen_q / 128), nk = ceil(seqlen_k / 128).
 *   *_block_cnt  int32, logical shape (b, h, nm)       h = QUERY heads
 *   *_block_idx  int32, logical shape (b, h, nm, nk)
 * read through the element strides below; a batch or head dimension of size 1 is given stride 0 (no expanded copy).
 * Query block m of (batch, head) visits the first mask_block_cnt[.., m] entries of mask_block_idx[.., m, :] and the first
 * full_block_cnt[.., m] entries of full_block_idx[.., m, :].  Entries past the count are never read for their meaning.  The
 * visited indices of one query block must be distinct and inside [0, nk): a duplicate, an index in both lists or one outside
 * the range is the caller's error with an undefined result (the kernel does not read K / V outside seqlen_k for any list
 * content; counts are clamped to [0, nk]).  The host never reads the lists.  The order of a list does not matter beyond rounding.
 * The output is dense attention restricted to the visited blocks: the pair (i, j) counts iff key block j / 128 is visited
 * for query block i / 128 AND the call's own mask allows it -- the seqlen_k bound, is_causal and window_size_left / right,
 * bottom-right aligned as everywhere here.  The call's mask applies inside "full" blocks as well (the reference's does,
 * flash_attn/cute/flash_fwd.py:1985-1994), so the two lists differ as a hint only: a full block is one the caller promises
 * needs no element-wise mask.  This kernel decides per 64-key tile from the call's mask alone and ignores the hint; a causal
 * diagonal block in the full list is therefore handled correctly.
 * A row without a visible key -- a query block whose two counts are 0 included -- gives O = 0 and LSE = +inf, or, with a
 * learnable sink z, O = 0 and LSE = z (fa_sink_params above).
 * Accepted: fp16 / bf16, d <= 256, d_v != d up to 256, MHA / GQA / MQA, is_causal, both window sides, softcap, a learnable
 * sink, arbitrary q / k / v / o strides.  num_splits 0 and 1 both mean no split.  FA_ERR_UNSUPPORTED: cu_seqlens_*, seqused_*,
 * block_table (the reference refuses block sparsity with varlen too), kv_batch_idx, leftpad_k, fp8, qv, dropout, s_dmask,
 * ALiBi, attention_chunk, num_splits > 1, d_v > 256, block_m / block_n other than 128.  These are checked before anything the
 * params may lack.  fa_fwd_params is untouched (its size is pinned): the lists travel in a struct of their own.
 * fa_fwd_plan_name and fa_fwd_workspace_size keep their meaning for plain params; fa_fwd_last_plan_name() names such a call
 * "bs_fwd_kernel D=<head-dim tile> waves=4[ SOFTCAP] block_m=128 splits=1".  No workspace.
 */
typedef struct fa_block_sparse_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size; /* sizeof(fa_block_sparse_params) */
    const int32_t *full_block_cnt; /* device pointers; full_* NULL together = no full list */
    const int32_t *full_block_idx;
    const int32_t *mask_block_cnt; /* required */
    const int32_t *mask_block_idx;
    /* element strides, >= 0: cnt (batch, head, m, unused = 0), idx (batch, head, m, n) */
    int64_t full_cnt_stride[4], full_idx_stride[4];
    int64_t mask_cnt_stride[4], mask_idx_stride[4];
    int32_t block_m, block_n; /* 128, 128 */
} fa_block_sparse_params;

/* fa_fwd restricted to the listed blocks; `sink` may be NULL. */
int fa_fwd_block_sparse(const fa_fwd_params *params, const fa_block_sparse_params *sparse, const fa_sink_params *sink, void *stream);
/* Validation only; no device access. */
int fa_fwd_block_sparse_validate(const fa_fwd_params *params, const fa_block_sparse_params *sparse, const fa_sink_params *sink);
uint32_t fa_block_sparse_params_size(void);

/*
 * 16-bit queries over an fp8 (OCP e4m3fn) KV cache -- what a serving stack runs with kv_cache_dtype = fp8: q and o are fp16 /
 * bf16 (params->dtype), k and v point at e4m3 BYTES, k / v_*_stride are in elements = bytes, and k_descale / v_descale are
 * the fp32 dequantisation factors per (batch, kv head) through their strides (NULL = 1.0).  The result is attention over the
 * dequantised cache: k_descale multiplies the score scale -- under softcap it acts BEFORE the tanh -- and v_descale the final
 * normalisation; q_descale is ignored (q is not quantised).  The bytes are converted to q's type on the way to the MFMA
 * (exact: every finite e4m3 value is a bf16 and an fp16 value), both products are the 16-bit MFMAs with fp32 accumulation.
 * The NaN bytes 0x7f / 0xff are unspecified.  fa_fwd_params is untouched (its size is pinned): the entry point is its own,
 * and fa_fwd / fa_fwd_validate keep refusing the all-fp8 call (dtype = FA_DTYPE_FP8_E4M3) beside KV-cache arguments.
 * One kernel, kv8_fwd_kernel (csrc/fa_fwd_kernel_kv8.h), in the work shape of pk_fwd_kernel: a workgroup owns a block of 128
 * (query row, head of the GQA group) pairs of one kv head, so K / V stream once per kv head for any h / h_k
 * (FA_FLAG_PACK_GQA is meaningless here: the kernel always packs).
 * Served: a dense cache (b_cache, seqlen_k, h_k, d) with seqused_k, kv_batch_idx and leftpad_k; a paged cache through
 * block_table with any page_block_size >= 1; dense queries of any seqlen_q and ragged queries over the cache (cu_seqlens_q
 * without cu_seqlens_k, seqused_k required, seqused_q); is_causal, both window sides (FA_FLAG_FA3_WINDOW as in fa_fwd),
 * softcap; head dims <= 128 that are multiples of 16 (an e4m3 row keeps 16-byte alignment); split-KV.
 * num_splits: 1 = off, N > 1 = N parts, 0 = fa_fwd's heuristic for the pk shape, counted from shapes only.  The parts write
 * fp32 partial O (splits, b, seqlen_q, h, d) and LSE (splits, b, h, seqlen_q) -- ragged queries (splits, total_q, h, d) and
 * (splits, h, total_q) -- into params->workspace (fa_fwd_kv8_workspace_size() bytes, 256-byte aligned; 0 unsplit), and the
 * merge is one fa_fwd_combine launch over them.  A row without a visible key gives O = 0, LSE = +inf, split or not.
 * FA_ERR_UNSUPPORTED, checked before anything the params may lack and before anything is launched: dtype fp8, d > 128 or
 * d % 16 != 0, d_v set and != d, qv, ALiBi, dropout, attention_chunk, s_dmask, cu_seqlens_k (and, as in fa_fwd, block_table
 * beside kv_batch_idx or leftpad_k).  k / v strides must be multiples of 16 bytes, the row strides below 2^24 bytes; the
 * kernel rebuilds a 64-bit base per 64-key tile, so a cache entry of 2 GiB or more is served, not refused.
 * The callee never allocates and never synchronises: the call can be captured into a HIP graph.
 * fa_fwd_last_plan_name() names such a call "kv8_fwd_kernel D=<64|128> waves=4[ SOFTCAP] block_m=128 splits=<N>" (splits=1:
 * the kernel stores O itself; N > 1: N parts and the merge); fa_fwd_kv8_plan_name gives the same text from params alone
 * (num_cus is accepted for symmetry with fa_fwd_plan_name and decides nothing), NULL when fa_fwd_kv8 would reject them.
 */
int fa_fwd_kv8(const fa_fwd_params *params, void *stream);
int fa_fwd_kv8_validate(const fa_fwd_params *params);
int64_t fa_fwd_kv8_workspace_size(const fa_fwd_params *params);
const char *fa_fwd_kv8_plan_name(const fa_fwd_params *params, int32_t num_cus);

/*
 * The MLA decode shape over an fp8 (OCP e4m3fn) KV cache: fa_fwd_kv8's contract for a q/k head dim d <= 64 beside a V / latent
 * head dim d_v in [256, 512] (required), with the optional second score term params->qv (16-bit (.., h, d_v) rows beside q,
 * qv_*_stride in elements; NULL = the same shape without it).  q, qv and o are fp16 / bf16 (params->dtype), k and v point at
 * e4m3 BYTES with strides in bytes.  Descales act in fp32 on the products, never on a 16-bit operand:
 *     S = (k_descale . Q.K8^T + v_descale . Qv.V8^T) . softmax_scale        O = v_descale . P.V8 / l
 * with k_descale / v_descale per (batch, kv head), NULL = 1.0; under softcap both factors act in front of the tanh; q_descale is
 * ignored.  One kernel, qv8_fwd_kernel (csrc/fa_fwd_kernel_qv8.h), in the work shape of fwd_kernel_qv: 32 (query row, head of
 * the GQA group) pairs of one kv head per workgroup.
 * Served: what fa_fwd_kv8 serves (dense cache with seqused_k -- clamped to the capacity --, kv_batch_idx, leftpad_k; paged cache
 * with any page_block_size >= 1; dense and ragged queries; is_causal, both window sides, softcap; split-KV), for d % 16 == 0,
 * d_v % 16 == 0.  num_splits: 1 = off, N > 1 = N parts, 0 = what fa_fwd's qv kernel splits the 16-bit call of the same shape
 * into.  The parts write fp32 partial O (splits, b, seqlen_q, h, d_v) and LSE (splits, b, h, seqlen_q) -- ragged queries
 * (splits, total_q, h, d_v) and (splits, h, total_q) -- into params->workspace (fa_fwd_qv8_workspace_size() bytes, 256-byte
 * aligned), merged by one fa_fwd_combine launch with d = d_v.  A row without a visible key gives O = 0, LSE = +inf, split or not.
 * FA_ERR_UNSUPPORTED, checked first: dtype fp8, d > 64, d % 16 != 0, d_v outside [256, 512] or d_v % 16 != 0, ALiBi, dropout,
 * attention_chunk, s_dmask, cu_seqlens_k (and block_table beside kv_batch_idx or leftpad_k).  There is no sink argument.  q / o /
 * qv strides are multiples of 8 elements, k / v strides multiples of 16 bytes with the row strides in [0, 2^24); pointers are
 * 16-byte aligned.  A cache entry of 2 GiB or more is served (64-bit base per 64-key tile).  FA_ERR_WORKSPACE when a split call
 * lacks its workspace.  The callee never allocates and never synchronises.  fa_fwd_kv8_validate keeps refusing qv and a wide V.
 * fa_fwd_last_plan_name() names such a call "qv8_fwd_kernel DVT=<256|512> waves=4[ SOFTCAP] block_m=32 splits=<N>";
 * fa_fwd_qv8_plan_name gives the same text from params alone (num_cus decides nothing), NULL when fa_fwd_qv8 would reject them.
 */
int fa_fwd_qv8(const fa_fwd_params *params, void *stream);
int fa_fwd_qv8_validate(const fa_fwd_params *params);
int64_t fa_fwd_qv8_workspace_size(const fa_fwd_params *params);
const char *fa_fwd_qv8_plan_name(const fa_fwd_params *params, int32_t num_cus);

/*
 * Block-sparse forward over a KV cache: a decode, verify or ragged serving step that reads only the key blocks a selection step
 * listed (Quest-style page selection, NSA-style selected blocks shared by a GQA group).  B = block_size keys per block, a
 * positive multiple of 64; g = h / h_k; sk(b) = the fill level of batch entry b as the non-sparse routes compute it (seqused_k,
 * clamped to the capacity, minus leftpad_k).
 *   block_cnt  int32, logical shape (b | 1, h_k | 1)
 *   block_idx  int32, logical shape (b | 1, h_k | 1, max_blocks), innermost stride 1
 * on the device, read through the element strides below; a broadcast dimension is given stride 0.
 * Key j of batch b is visible to query row i of head hd iff  j < sk(b)  AND  is_causal / window / softcap allow (i, j) exactly as
 * on the non-sparse routes (bottom-right aligned on sk(b), FA_FLAG_FA3_WINDOW)  AND  j / B is among the first
 * min(block_cnt[b, hd / g], max_blocks) entries of block_idx[b, hd / g, :].
 * Lists are per KV head, shared by every query row of the call and every head of the GQA group (which is what lets the group
 * share one pass over the cache).  Entries may come in any order (results differ by rounding only).  An entry outside
 * [0, ceil(sk(b) / B)) is skipped without touching memory; entries at or behind the count are never used as addresses.  Distinct
 * entries are the caller's duty: a duplicate counts twice.  A row with no visible key gives O = 0, LSE = +inf, split or not.
 * The host never reads the lists: the call can be captured into a HIP graph, and a replay after the lists changed computes the
 * new selection.  The callee never allocates and never synchronises.
 * params->dtype names q / o (fp16 / bf16).  fp8_cache = 0: k / v are 16-bit elements of that type, strides in elements, descales
 * ignored.  fp8_cache != 0: k / v point at e4m3 BYTES with byte strides, and k_descale / v_descale (fa_fwd_kv8's meaning) are
 * both required.
 * One kernel, sp_fwd_kernel (csrc/fa_fwd_kernel_sp.h): the packed-row body of pk_fwd_kernel / kv8_fwd_kernel walking the list in
 * place of the key range.  List position t in [0, cnt * B / 64) is entry t / (B / 64), sub-tile t % (B / 64); the next entry is
 * fetched one step ahead.  Served: a dense cache with seqused_k, kv_batch_idx and leftpad_k; a paged cache with any
 * page_block_size >= 1; dense and ragged queries (cu_seqlens_q without cu_seqlens_k, seqused_k required); is_causal, both window
 * sides, softcap; head dims <= 128 that are multiples of 16; split-KV.
 * num_splits: 1 = off, N > 1 = N parts, 0 = what fa_fwd's heuristic gives the pk shape for a key length of max_blocks * B
 * (shapes only).  The parts are ranges of LIST POSITIONS, not of key tiles; partials, workspace layout and the merge (one
 * fa_fwd_combine launch) are fa_fwd_kv8's, for both cache types.
 * FA_ERR_UNSUPPORTED, checked before anything the params may lack: dtype fp8 (the all-fp8 call), d > 128 or d % 16 != 0, d_v
 * set and != d, qv, ALiBi, dropout, attention_chunk, s_dmask, cu_seqlens_k (and block_table beside kv_batch_idx or leftpad_k).
 * There is no sink argument.  FA_ERR_BAD_SHAPE: block_size not a positive multiple of 64, max_blocks < 0, max_blocks *
 * block_size >= 2^31.  FA_ERR_NULL_POINTER: a NULL list, a missing descale with fp8_cache.  FA_ERR_WORKSPACE when a split call
 * lacks its workspace (fa_fwd_sparse_kv_workspace_size() bytes, 256-byte aligned; 0 unsplit).
 * fa_fwd_last_plan_name() names such a call
 *   "sp_fwd_kernel D=<64|128> waves=4[ SOFTCAP] KV=<16|e4m3> B=<block_size> block_m=128 splits=<N>";
 * fa_fwd_sparse_kv_plan_name gives the same text from the two structs alone (num_cus decides nothing), NULL when
 * fa_fwd_sparse_kv would reject them.
 */
typedef struct fa_sparse_kv_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size; /* sizeof(fa_sparse_kv_params) */
    const int32_t *block_cnt; /* device pointers, both required */
    const int32_t *block_idx;
    int64_t cnt_batch_stride, cnt_head_stride; /* element strides, >= 0, 0 = broadcast */
    int64_t idx_batch_stride, idx_head_stride;
    int32_t max_blocks; /* entries per list, >= 0 */
    int32_t block_size; /* B: keys per block, a positive multiple of 64 */
    int32_t fp8_cache;  /* 0: 16-bit k / v; != 0: e4m3 bytes + descales */
    int32_t reserved;
} fa_sparse_kv_params;

int fa_fwd_sparse_kv(const fa_fwd_params *params, const fa_sparse_kv_params *sparse, void *stream);
/* Validation only; no device access. */
int fa_fwd_sparse_kv_validate(const fa_fwd_params *params, const fa_sparse_kv_params *sparse);
int64_t fa_fwd_sparse_kv_workspace_size(const fa_fwd_params *params, const fa_sparse_kv_params *sparse);
const char *fa_fwd_sparse_kv_plan_name(const fa_fwd_params *params, const fa_sparse_kv_params *sparse, int32_t num_cus);
uint32_t fa_sparse_kv_params_size(void);

/*
 * Tree attention over a KV cache: the verify step of speculative decoding whose draft is a token TREE (Medusa, EAGLE-2,
 * SpecInfer, sequoia) of up to 64 nodes.  The query rows of batch entry b are the sq(b) nodes of its tree (seqlen_q, or
 * cu_seqlens_q[b + 1] - cu_seqlens_q[b] for ragged queries); the caller has appended their keys / values at positions
 * [sk(b) - sq(b), sk(b)) of the cache, sk(b) = the fill level as the other cache routes compute it (seqused_k, clamped to the
 * capacity, minus leftpad_k) INCLUDING the draft.
 *   tree_mask  int64 on the device, logical shape (b, seqlen_q) behind the two element strides below; ragged queries: (total_q,),
 *              row_stride alone (batch_stride is not read)
 * With shift = sk(b) - sq(b) and t = j - shift, key j of batch b is visible to query row i of any head iff
 *   j < sk(b)  AND  ( t < 0  OR  ( t < 64  AND  bit t of tree_mask[b, i] is set ) ),
 * so the committed prefix is seen by every node; softcap applies as elsewhere.  Bits at or above sq(b) are ignored.  A tree key
 * with t >= 64 is invisible: seqlen_q (the bound of every sq(b)) above 64 is refused, and a ragged entry that is longer at run
 * time falls under this rule, without a fault.  No structure is assumed of the words: they need not be lower-triangular, and the
 * diagonal bit is the caller's duty.  A chain is row i = bits 0 .. i, which is is_causal of the other routes.  A row with no
 * visible key gives O = 0, LSE = +inf, split or not.  Positions in a tree are depths, not indices: there is no rotary here, the
 * caller rotates q / k before the append.  Read-only.
 * The host never reads the words or the fill levels: the call can be captured into a HIP graph, and a replay after both were
 * overwritten in place computes the new tree.  The callee never allocates and never synchronises.
 * params->dtype names q / o (fp16 / bf16).  fp8_cache = 0: k / v are 16-bit elements of that type, strides in elements, descales
 * ignored.  fp8_cache != 0: k / v point at e4m3 BYTES with byte strides, and k_descale / v_descale (fa_fwd_kv8's meaning) are
 * both required.
 * One kernel, tr_fwd_kernel (csrc/fa_fwd_kernel_tr.h): the packed-row body of pk_fwd_kernel / kv8_fwd_kernel with the per-row
 * word in place of the lane's key range; only the (at most two) 64-key tiles that reach past shift take the element mask.
 * Served: a dense cache with seqused_k, kv_batch_idx and leftpad_k; a paged cache with any page_block_size >= 1; dense and ragged
 * queries (cu_seqlens_q without cu_seqlens_k, seqused_k required); softcap; head dims <= 128 that are multiples of 16; split-KV
 * over the key range.  num_splits: 1 = off, N > 1 = N parts (clamped to the key tiles), 0 = what fa_fwd's heuristic gives the pk
 * shape (shapes only); partials, workspace layout and the merge (one fa_fwd_combine launch) are fa_fwd_kv8's, for both cache types.
 * FA_ERR_UNSUPPORTED, checked before anything the params may lack: dtype fp8 (the all-fp8 call), d > 128 or d % 16 != 0, d_v
 * set and != d, seqlen_q > 64, is_causal, a window side >= 0, attention_chunk, qv, ALiBi, dropout, s_dmask, cu_seqlens_k (and
 * block_table beside kv_batch_idx or leftpad_k).  There is no sink argument and no rotary argument.  FA_ERR_NULL_POINTER: a NULL
 * tree_mask, a missing descale with fp8_cache.  FA_ERR_BAD_STRIDE: tree_mask not 8-byte aligned, a negative stride.
 * FA_ERR_WORKSPACE when a split call lacks its workspace (fa_fwd_tree_workspace_size() bytes, 256-byte aligned; 0 unsplit).
 * fa_fwd_last_plan_name() names such a call
 *   "tr_fwd_kernel D=<64|128> waves=4[ SOFTCAP] KV=<16|e4m3> block_m=128 splits=<N>";
 * fa_fwd_tree_plan_name gives the same text from the two structs alone (num_cus decides nothing), NULL when fa_fwd_tree would
 * reject them.
 */
typedef struct fa_tree_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size; /* sizeof(fa_tree_params) */
    const int64_t *tree_mask; /* device pointer, required */
    int64_t batch_stride, row_stride; /* element strides, >= 0 */
    int32_t fp8_cache; /* 0: 16-bit k / v; != 0: e4m3 bytes + descales */
    int32_t reserved;
} fa_tree_params;

int fa_fwd_tree(const fa_fwd_params *params, const fa_tree_params *tree, void *stream);
/* Validation only; no device access. */
int fa_fwd_tree_validate(const fa_fwd_params *params, const fa_tree_params *tree);
int64_t fa_fwd_tree_workspace_size(const fa_fwd_params *params, const fa_tree_params *tree);
const char *fa_fwd_tree_plan_name(const fa_fwd_params *params, const fa_tree_params *tree, int32_t num_cus);
uint32_t fa_tree_params_size(void);

/* Human-readable text for a status code (static storage). */
const char *fa_strerror(int status);

/* sizeof(fa_fwd_params) as compiled, for binding self-checks. */
uint32_t fa_fwd_params_size(void);

/* FA_ABI_VERSION as compiled. */
uint32_t fa_abi_version(void);

/* Tile geometry chosen for (d, dtype, causal): writes block_m / block_n.
 * Role of tile_size_fwd_sm90 (hopper/tile_size.h:10-54). */
int fa_fwd_tile_shape(int32_t d, int32_t dtype, int32_t is_causal, int32_t *block_m, int32_t *block_n);

/*
 * In-place append of new keys/values to a KV cache -- the "Append_KV" step of mha_fwd_kvcache
 * (csrc/flash_attn/flash_api.cpp:1354-1382, src/flash_fwd_kernel.h:651-735), as its own HBM-bound launch:
 * rows k_new[i, 0:seqlen_new) go to k_cache[idx(i), cache_seqlens[i] + 0:seqlen_new) (idx = cache_batch_idx or
 * identity); rows that would fall past seqlen_cache are dropped.  16-bit elements, head_dim stride 1, d % 8 == 0.
 */
typedef struct fa_kvcache_append_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size; /* sizeof(fa_kvcache_append_params) */
    const void *k_new; /* (b, seqlen_new, h_k, d) */
    const void *v_new;
    void *k_cache;     /* (b_cache, seqlen_cache, h_k, d) */
    void *v_cache;
    int64_t knew_batch_stride, knew_row_stride, knew_head_stride;
    int64_t vnew_batch_stride, vnew_row_stride, vnew_head_stride;
    int64_t kcache_batch_stride, kcache_row_stride, kcache_head_stride;
    int64_t vcache_batch_stride, vcache_row_stride, vcache_head_stride;
    int32_t b, seqlen_new, seqlen_cache, h_k, d;
    int32_t reserved;
    const int32_t *cache_seqlens;   /* (b) int32, rows already valid in each cache entry */
    const int32_t *cache_batch_idx; /* (b) int32 or NULL */
    const int32_t *block_table;     /* paged cache (see fa_fwd_params) or NULL; then seqlen_cache = pages per sequence
                                       x page_block_size and k/vcache_batch_stride is the page stride */
    int64_t block_table_batch_stride;
    int32_t page_block_size;
    int32_t dtype; /* enum fa_dtype (16-bit types); only read when rotary_cos is set */
    /* Rotary embedding of the appended KEYS (csrc/flash_attn/flash_api.cpp:1404-1428, src/flash_fwd_kernel.h:679-735):
     * row i of k_new is rotated by position cache_seqlens[b] + i before it is stored; values are copied unchanged.
     * rotary_cos / rotary_sin: (seqlen_ro, rotary_dim / 2), contiguous, same 16-bit dtype as k; rotary_dim % 16 == 0,
     * <= d; interleaved: pairs (2j, 2j+1) (GPT-J), otherwise (j, j + rotary_dim/2) (GPT-NeoX).  NULL = no rotary. */
    const void *rotary_cos;
    const void *rotary_sin;
    int32_t rotary_dim;
    int32_t rotary_interleaved;
    /* ABI v12 -- FA3 `seqlens_rotary` (hopper/flash_api.cpp:1074-1079, hopper/seqlen.h:89): (b) int32 rotary position of the
     * first appended row of each batch entry when it is not the cache fill level; NULL = cache_seqlens. */
    const int32_t *rotary_seqlens;
    /* ABI v13 -- head dim of v_new / v_cache when it differs from d (MLA: 512-wide V rows beside 64-wide K rows); 0 = d.
     * Multiple of 8, <= 512.  Rotary still touches the keys only. */
    int32_t d_v;
    int32_t reserved_v13;
} fa_kvcache_append_params;

int fa_kvcache_append(const fa_kvcache_append_params *params, void *stream);
uint32_t fa_kvcache_append_params_size(void);

/*
 * Rotary embedding of a (b, s, h, d) tensor into `dst` (same shape; dst may alias src): row i of batch b is rotated by
 * position seqlen_offsets[b] + (per_row_positions ? i : 0) -- the query side of mha_fwd_kvcache (causal / local: one
 * position per query row; otherwise every row at cache_seqlens, flash_attn/flash_attn_interface.py:1516-1524).
 */
typedef struct fa_rotary_params {
    uint32_t abi_version;
    uint32_t struct_size;
    const void *src;
    void *dst;
    int64_t src_batch_stride, src_row_stride, src_head_stride;
    int64_t dst_batch_stride, dst_row_stride, dst_head_stride;
    int32_t b, s, h, d;
    int32_t dtype; /* FA_DTYPE_FP16 / FA_DTYPE_BF16 */
    int32_t rotary_dim;
    int32_t rotary_interleaved;
    int32_t per_row_positions;
    const void *rotary_cos; /* (seqlen_ro, rotary_dim / 2) */
    const void *rotary_sin;
    const int32_t *seqlen_offsets; /* (b) */
} fa_rotary_params;

int fa_rotary_apply(const fa_rotary_params *params, void *stream);
uint32_t fa_rotary_params_size(void);

/*
 * Ragged in-place append: one serving step's new keys / values, packed (total_k_new, h_k, .) with cu_seqlens_k_new like a
 * varlen tensor (flash_attn_with_kvcache(..., cu_seqlens_k_new=), hopper/flash_api.cpp:935-975), into a batched or paged
 * cache.  Row i of sequence s goes to cache row cache_seqlens[s] + i of entry cache_batch_idx[s] (NULL = s) or of its page;
 * rows that would fall past seqlen_cache are dropped.  Keys are rotated at position
 * (rotary_seqlens ? rotary_seqlens[s] : cache_seqlens[s]) + i by the rules of fa_kvcache_append; values are copied.  The same
 * launch writes seqused_out[s] = min(cache_seqlens[s] + (cu_seqlens_k_new[s+1] - cu_seqlens_k_new[s]), seqlen_cache) -- the
 * fill levels the attention launch reads as seqused_k (never past the capacity: the dropped rows are not there).
 * seqused_out must not alias cache_seqlens.  One HBM-bound launch, one wavefront per new row: with max_seqlen_k_new > 0
 * (an upper bound of the lengths) the grid is (row blocks of the longest sequence) x b; with 0 the rows are dealt flat and
 * every wavefront finds its sequence by a binary search in cu_seqlens_k_new (held in LDS up to 16383 sequences).
 * 16-bit elements, head_dim stride 1, d % 8 == 0, d_v <= 512, 16-byte aligned rows; block_table not with cache_batch_idx.
 */
typedef struct fa_kvcache_append_varlen_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size; /* sizeof(fa_kvcache_append_varlen_params) */
    const void *k_new; /* (total_k_new, h_k, d) */
    const void *v_new; /* (total_k_new, h_k, d_v) */
    void *k_cache;     /* (b_cache, seqlen_cache, h_k, d) or pages (num_pages, page_block_size, h_k, d) */
    void *v_cache;
    int64_t knew_row_stride, knew_head_stride;
    int64_t vnew_row_stride, vnew_head_stride;
    int64_t kcache_batch_stride, kcache_row_stride, kcache_head_stride;
    int64_t vcache_batch_stride, vcache_row_stride, vcache_head_stride;
    int32_t b;                /* sequences */
    int32_t total_k_new;      /* rows of k_new / v_new (>= cu_seqlens_k_new[b]; rows behind it are ignored) */
    int32_t max_seqlen_k_new; /* upper bound of the new lengths, or 0 = not known (search in cu_seqlens_k_new) */
    int32_t seqlen_cache;     /* capacity; paged: pages per sequence x page_block_size */
    int32_t h_k, d;
    int32_t d_v;   /* head dim of v_new / v_cache; 0 = d */
    int32_t dtype; /* enum fa_dtype (16-bit types) */
    const int32_t *cu_seqlens_k_new; /* (b + 1) */
    const int32_t *cache_seqlens;    /* (b) rows already valid in each sequence's cache */
    const int32_t *cache_batch_idx;  /* (b) or NULL */
    int32_t *seqused_out;            /* (b) written by the launch */
    const int32_t *block_table;      /* paged cache (see fa_fwd_params) or NULL */
    int64_t block_table_batch_stride;
    int32_t page_block_size;
    int32_t rotary_dim;         /* % 16 == 0, <= d; only read when rotary_cos is set */
    const void *rotary_cos;     /* (seqlen_ro, rotary_dim / 2), the dtype of k; NULL = no rotary */
    const void *rotary_sin;
    const int32_t *rotary_seqlens; /* (b) or NULL = cache_seqlens */
    int32_t rotary_interleaved;
    int32_t reserved;
} fa_kvcache_append_varlen_params;

int fa_kvcache_append_varlen(const fa_kvcache_append_varlen_params *params, void *stream);
uint32_t fa_kvcache_append_varlen_params_size(void);

/*
 * Rotary embedding of a ragged (total_q, h, d) tensor into `dst` (same shape; dst may alias src): row i of sequence s is
 * rotated at position offsets[s] + (per_row_positions ? i : 0) -- the query side of a ragged KV-cache step.  Same launch
 * shape and sequence lookup as fa_kvcache_append_varlen (max_seqlen_q > 0: a 2-D grid, 0: a search in cu_seqlens_q).
 */
typedef struct fa_rotary_varlen_params {
    uint32_t abi_version;
    uint32_t struct_size;
    const void *src;
    void *dst;
    int64_t src_row_stride, src_head_stride;
    int64_t dst_row_stride, dst_head_stride;
    int32_t b, total_q, max_seqlen_q, h, d;
    int32_t dtype; /* FA_DTYPE_FP16 / FA_DTYPE_BF16 */
    int32_t rotary_dim;
    int32_t rotary_interleaved;
    int32_t per_row_positions;
    int32_t reserved;
    const void *rotary_cos; /* (seqlen_ro, rotary_dim / 2) */
    const void *rotary_sin;
    const int32_t *cu_seqlens_q; /* (b + 1) */
    const int32_t *offsets;      /* (b) */
} fa_rotary_varlen_params;

int fa_rotary_apply_varlen(const fa_rotary_varlen_params *params, void *stream);
uint32_t fa_rotary_varlen_params_size(void);

/*
 * Quantising in-place append to an fp8 (OCP e4m3fn) KV cache -- the write half of what fa_fwd_kv8 reads: new 16-bit keys /
 * values go into a cache of e4m3 BYTES at the rows fa_kvcache_append / fa_kvcache_append_varlen would have written in a 16-bit
 * cache.  One struct, both forms: cu_seqlens_k_new == NULL is the dense form, new rows (b, seqlen_new, h_k, d) through the
 * batch strides; otherwise the rows are ragged, (total_k_new, h_k, d) with cu_seqlens_k_new and max_seqlen_k_new (0 = a search
 * in cu_seqlens_k_new), as in fa_kvcache_append_varlen.
 * An element x of sequence s (the index of the call, the one fa_fwd_kv8 reads descales by -- not the cache entry) and kv head g:
 *     inv  = 1.0f / ds           ds = k_descale[s, g] for keys, v_descale[s, g] for values (NULL = 1.0); IEEE fp32, once
 *     y    = float(x) * inv      one fp32 multiply
 *     byte = e4m3fn_rne(min(max(y, -448), 448))      round to nearest even, saturating; +-inf -> +-448; -0 keeps its sign
 * Keys are rotated first, by the code of the 16-bit appends (fp32 arithmetic, position (rotary_seqlens ? rotary_seqlens[s] :
 * cache_seqlens[s]) + i, interleaved or not, columns >= rotary_dim passed through), the result rounded to the 16-bit type and
 * then quantised: the bytes are the quantisation of what the 16-bit appends write.  Values are never rotated.  NaN inputs are
 * unspecified.  Row i of sequence s goes to cache row cache_seqlens[s] + i of entry cache_batch_idx[s] (NULL = s) or of its
 * page (any page size); rows at or past seqlen_cache are dropped; nothing but the d bytes per head of the appended rows is
 * written.  seqused_out[s] = min(cache_seqlens[s] + new rows of s, seqlen_cache) is written by the same launch: required in
 * the ragged form, optional (NULL) in the dense one; it must not alias cache_seqlens.
 * One kernel, kvcache_append_kv8_kernel (csrc/fa_kvcache_append_kv8.hip): a wavefront per new row, 16-byte loads, 8-byte
 * stores, 64-bit addresses from a per-row base (a cache entry of 2 GiB and more is served), no atomics, no allocation, no
 * synchronisation: the call can be captured into a HIP graph.
 * d % 16 == 0 and d <= 128 (what fa_fwd_kv8 serves), d_v 0 or d; new rows 16-byte aligned (pointers, strides % 8 elements);
 * the cache 8-byte aligned (pointers, strides % 8 bytes); rotary_dim % 16 == 0, <= d, cos and sin together, 16-byte aligned;
 * block_table not with cache_batch_idx.  The status codes are those of the 16-bit appends for the same faults
 * (FA_ERR_BAD_SHAPE for seqused_out == cache_seqlens).
 */
typedef struct fa_kvcache_append_kv8_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size; /* sizeof(fa_kvcache_append_kv8_params) */
    const void *k_new; /* 16-bit: (b, seqlen_new, h_k, d) or (total_k_new, h_k, d) */
    const void *v_new;
    void *k_cache;     /* e4m3 bytes: (b_cache, seqlen_cache, h_k, d) or pages (num_pages, page_block_size, h_k, d) */
    void *v_cache;
    int64_t knew_batch_stride, knew_row_stride, knew_head_stride; /* elements; the batch stride is read in the dense form only */
    int64_t vnew_batch_stride, vnew_row_stride, vnew_head_stride;
    int64_t kcache_batch_stride, kcache_row_stride, kcache_head_stride; /* bytes; paged: the batch stride is the page stride */
    int64_t vcache_batch_stride, vcache_row_stride, vcache_head_stride;
    int32_t b;                /* sequences */
    int32_t seqlen_new;       /* dense form: new rows per sequence */
    int32_t total_k_new;      /* ragged form: rows of k_new / v_new (>= cu_seqlens_k_new[b]) */
    int32_t max_seqlen_k_new; /* ragged form: upper bound of the new lengths, or 0 = not known */
    int32_t seqlen_cache;     /* capacity; paged: pages per sequence x page_block_size */
    int32_t h_k, d;
    int32_t d_v;              /* 0 or d; fa_kvcache_append_qv8: the latent / V head dim, in [256, 512] */
    int32_t dtype;            /* of the new rows and of rotary_cos / rotary_sin: FA_DTYPE_FP16 / FA_DTYPE_BF16 */
    int32_t page_block_size;
    int32_t rotary_dim;       /* only read when rotary_cos is set */
    int32_t rotary_interleaved;
    const int32_t *cu_seqlens_k_new; /* (b + 1), or NULL = the dense form */
    const int32_t *cache_seqlens;    /* (b) rows already valid in each sequence's cache */
    const int32_t *cache_batch_idx;  /* (b) or NULL */
    int32_t *seqused_out;            /* (b) written by the launch; may be NULL in the dense form */
    const int32_t *block_table;      /* paged cache (see fa_fwd_params) or NULL */
    int64_t block_table_batch_stride;
    const void *rotary_cos;          /* (seqlen_ro, rotary_dim / 2), contiguous, `dtype`; NULL = no rotary */
    const void *rotary_sin;
    const int32_t *rotary_seqlens;   /* (b) or NULL = cache_seqlens */
    const float *k_descale;          /* fp32 per (sequence, kv head) through the strides below; NULL = 1.0 */
    const float *v_descale;
    int64_t k_descale_batch_stride, k_descale_head_stride;
    int64_t v_descale_batch_stride, v_descale_head_stride;
} fa_kvcache_append_kv8_params;

int fa_kvcache_append_kv8(const fa_kvcache_append_kv8_params *params, void *stream);
/* Validation only; no device access. */
int fa_kvcache_append_kv8_validate(const fa_kvcache_append_kv8_params *params);
uint32_t fa_kvcache_append_kv8_params_size(void);

/*
 * The same append for the MLA shape of the fp8 KV cache -- the write half of what fa_fwd_qv8 reads: a rotated k_pe row (head dim
 * d <= 64, d % 16 == 0) into k_cache and the latent row (d_v in [256, 512], d_v % 16 == 0, required here) into v_cache, as e4m3
 * bytes, in place.  The struct, the quantisation (keys by k_descale, the latent by v_descale), the rotation of the keys, the
 * placement, seqused_out, the alignment rules and the status codes are those of fa_kvcache_append_kv8, rule for rule
 * (FA_ERR_BAD_HEAD_DIM for any d / d_v outside the shape above); per appended row and head d bytes of K and d_v bytes of V are
 * written and nothing else.  One kernel, kvcache_append_qv8_kernel (csrc/fa_kvcache_append_qv8.hip): a wavefront per new row,
 * its lanes on 64 consecutive 16-byte chunks of V per pass, the few K chunks on the lanes at the other end of the same pass.
 */
int fa_kvcache_append_qv8(const fa_kvcache_append_kv8_params *params, void *stream);
/* Validation only; no device access. */
int fa_kvcache_append_qv8_validate(const fa_kvcache_append_kv8_params *params);

/* Merge of split-KV partial results given by the caller: mha_combine / flash_attn_3::fwd_combine
 * (hopper/flash_api.cpp:1569-1670, hopper/flash_fwd_combine_kernel.h).
 *   lse[b, i, h] = log sum_s exp(lse_partial[s, b, i, h]);   out[b, i, h, :] = sum_s exp(lse_partial[s] - lse) out_partial[s]
 * A split with lse_partial = -inf carries no weight; rows where every split is -inf give out = 0, lse = -inf
 * (attention_combine_ref, hopper/test_flash_attn.py:1105-1114).  Partials are fp32 with arbitrary element strides
 * (head-dim stride 1); out is fp32 / fp16 / bf16.  num_splits <= 256 like the reference. */
typedef struct fa_combine_params {
    uint32_t abi_version; /* FA_ABI_VERSION */
    uint32_t struct_size; /* sizeof(fa_combine_params) */
    const float *out_partial; /* (num_splits, b, seqlen, h, d) */
    const float *lse_partial; /* (num_splits, b, seqlen, h) */
    void *out;                /* (b, seqlen, h, d) of out_dtype */
    float *softmax_lse;       /* (b, seqlen, h) through the strides below */
    int64_t op_split_stride, op_batch_stride, op_row_stride, op_head_stride;
    int64_t lp_split_stride, lp_batch_stride, lp_row_stride, lp_head_stride;
    int64_t o_batch_stride, o_row_stride, o_head_stride;
    int64_t lse_batch_stride, lse_row_stride, lse_head_stride;
    int32_t num_splits, b, seqlen, h, d;
    int32_t out_dtype; /* FA_DTYPE_FP32 / FA_DTYPE_FP16 / FA_DTYPE_BF16 */
} fa_combine_params;

int fa_fwd_combine(const fa_combine_params *params, void *stream);
uint32_t fa_combine_params_size(void);

/* Test hook: overrides the default kernel variant process-wide (0 = default). */
void fa_set_default_variant(int32_t variant);
/* Test hook: the persistent form of the 256-row kernel (one workgroup per CU walking a chain of work items):
 * 0 = the library's choice, -1 = never, 1 = for every problem it can run (also chains of a single item). */
void fa_set_persist_mode(int32_t mode);

#ifdef __cplusplus
}
#endif
#endif /* FA_FWD_H_ */
