// fa_fwd_internal.h — host helpers of the forward C-ABI layer (not part of the C-ABI), shared by fa_fwd_api.hip,
// fa_fwd_kv8_api.hip and fa_fwd_qv8_api.hip: the one window rule and softmax scales (fa_bwd_api.hip uses these two as well), the
// one fill of KParams from fa_fwd_params, the one split-KV workspace layout, the one packed-row grid, and what the two fp8-cache
// routes have in common.  The split-KV heuristic and the last-plan text of fa_fwd_last_plan_name() stay in fa_fwd_api.hip.
#pragma once

#include "fa_fwd.h"
#include "fa_fwd_kernel.h"

#include <cmath>

namespace fa {

// Parts of the key range for the pk work shape (blocks of 128 packed rows per kv head, 4 waves; split_plan of fa_fwd_api.hip):
// num_splits 1 = off, N > 1 = N (clamped to the key blocks), 0 = the heuristic.  Counted from shapes only.  `p` is 16-bit.
int fwd_pk_split_count(const fa_fwd_params *p);

// The same for the qv work shape (blocks of 32 packed rows per kv head, one workgroup per CU; split_plan_qv of fa_fwd_api.hip):
// what the 16-bit qv call of the same shape is split into.  Reads the shape fields and num_splits only.
int fwd_qv_split_count(const fa_fwd_params *p);

// What fa_fwd_last_plan_name() answers for the calling thread until its next fa_fwd / fa_fwd_sink / fa_fwd_block_sparse;
// NULL or "" = nothing.
void fwd_set_last_plan_text(const char *text);

// compute units of the current device (cached per device ordinal)
int fwd_device_cus();

// ---- window normalisation (csrc/flash_attn/flash_api.cpp:396-402), forward and backward --------------------------------
// In: the caller's window_size_left / window_size_right; out: the kernels' window_left / window_right (< 0 = unbounded).
inline void normalise_window(bool is_causal, int32_t flags, int32_t seqlen_k, int32_t &wl, int32_t &wr) {
    if (is_causal) wr = 0;
    // FA3 rule, FA_FLAG_FA3_WINDOW (hopper/flash_api.cpp:152-153, 589-590): a missing side becomes seqlen_k - 1 / seqlen_q - 1,
    // which never masks anything = unbounded here; sides are taken as given otherwise
    if (flags & FA_FLAG_FA3_WINDOW) return;
    if (wl >= seqlen_k) wl = -1;
    if (wr >= seqlen_k) wr = -1;
    if (is_causal) wr = 0;
    // set_params_fprop csrc/flash_attn/flash_api.cpp:141-142: a one-sided window gets seqlen_k on the other side.
    // For a left-only window that is NOT the same as unbounded when seqlen_q > seqlen_k (the bottom-right aligned
    // diagonal starts left of key 0), so it is mirrored.  The symmetric rule (right-only -> left = seqlen_k) never
    // masks anything (row + sk - sq - seqlen_k < 0 for every row) and is left as "unbounded".
    if (wl >= 0 && wr < 0) wr = seqlen_k;
}

// ---- softmax scales (set_params_fprop csrc/flash_attn/flash_api.cpp:103-117): under softcap the scores are
// tanh(s * softmax_scale / softcap) and the softmax multiplies them by softcap
struct SoftmaxScales {
    float softcap_pre, scale, scale_log2;
};
inline SoftmaxScales softmax_scales(float softmax_scale, float softcap) {
    constexpr float kLog2e = 1.4426950408889634f;
    if (softcap > 0.f) return {softmax_scale / softcap, softcap, softcap * kLog2e};
    return {0.f, softmax_scale, softmax_scale * kLog2e};
}

// ---- fa_fwd_params -> KParams: what every forward route hands its kernel.  `dv` is the route's head dim of V / O.  Left to
// the route: the descales (fwd_fill_kv_descales), the work list (num_m_blocks ... num_cus), num_splits and the split strides,
// ALiBi, dropout, chunk, the sink.
inline void fwd_fill_params(const fa_fwd_params *p, int32_t dv, KParams &kp) {
    kp.q = p->q; kp.k = p->k; kp.v = p->v; kp.o = p->o; kp.lse = p->softmax_lse;
    kp.cu_seqlens_q = p->cu_seqlens_q; kp.cu_seqlens_k = p->cu_seqlens_k;
    kp.seqused_q = p->seqused_q; kp.seqused_k = p->seqused_k;
    kp.q_batch_stride = p->q_batch_stride; kp.q_row_stride = p->q_row_stride; kp.q_head_stride = p->q_head_stride;
    kp.k_batch_stride = p->k_batch_stride; kp.k_row_stride = p->k_row_stride; kp.k_head_stride = p->k_head_stride;
    kp.v_batch_stride = p->v_batch_stride; kp.v_row_stride = p->v_row_stride; kp.v_head_stride = p->v_head_stride;
    kp.o_batch_stride = p->o_batch_stride; kp.o_row_stride = p->o_row_stride; kp.o_head_stride = p->o_head_stride;
    kp.b = p->b; kp.seqlen_q = p->seqlen_q; kp.seqlen_k = p->seqlen_k; kp.h = p->h; kp.h_k = p->h_k; kp.d = p->d;
    kp.total_q = p->total_q;
    kp.dv = dv;
    kp.h_ratio = p->h / p->h_k;
    kp.window_left = p->window_size_left;
    kp.window_right = p->window_size_right;
    normalise_window(p->is_causal, p->flags, p->seqlen_k, kp.window_left, kp.window_right);
    const SoftmaxScales sc = softmax_scales(p->softmax_scale, p->softcap);
    kp.softcap_pre = sc.softcap_pre; kp.scale = sc.scale; kp.scale_log2 = sc.scale_log2;
    kp.leftpad_k = p->leftpad_k;
    kp.kv_batch_idx = p->kv_batch_idx;
    kp.block_table = p->block_table;
    kp.bt_bs = (int32_t)p->block_table_batch_stride;
    kp.page_size = p->page_block_size;
    kp.drop_thr = 255;  // dropout off
    kp.rp_dropout = 1.f;
}
// The k / v descales, for the routes that read an fp8 K / V.  Not part of the fill: a 16-bit fa_fwd call hands its kernel NULL
// whatever the caller's descale fields hold, and q_descale is fa_fwd's alone (the fp8-cache routes do not quantise q).
inline void fwd_fill_kv_descales(const fa_fwd_params *p, KParams &kp) {
    kp.k_descale = p->k_descale; kp.v_descale = p->v_descale;
    kp.kd_bs = (int32_t)p->k_descale_batch_stride; kp.kd_hs = (int32_t)p->k_descale_head_stride;
    kp.vd_bs = (int32_t)p->v_descale_batch_stride; kp.vd_hs = (int32_t)p->v_descale_head_stride;
}

// ---- split-KV workspace: fp32 partials, O (splits, b, sq, h, dv) then LSE (splits, b, h, sq), each rounded up to 256 bytes;
// ragged queries (splits, total_q, h, dv) and (splits, h, total_q)
inline int64_t align256(int64_t x) { return (x + 255) & ~int64_t(255); }
inline int64_t query_rows(const fa_fwd_params *p) { return p->cu_seqlens_q ? p->total_q : (int64_t)p->b * p->seqlen_q; }
struct SplitPlan {
    int splits;
    int64_t o_bytes, lse_bytes, total;
};
inline SplitPlan split_layout(const fa_fwd_params *p, int splits, int dv) {
    if (splits <= 1) return SplitPlan{1, 0, 0, 0};
    SplitPlan sp{splits, 0, 0, 0};
    const int64_t rows = query_rows(p);
    sp.o_bytes = align256(splits * rows * p->h * dv * 4);
    sp.lse_bytes = align256(splits * rows * p->h * 4);
    sp.total = sp.o_bytes + sp.lse_bytes;
    return sp;
}
inline bool workspace_short(const fa_fwd_params *p, int64_t bytes) {
    return !p->workspace || reinterpret_cast<uintptr_t>(p->workspace) % 256 != 0 || (int64_t)p->workspace_bytes < bytes;
}
// a split launch writes its partials into the workspace (kp.dv columns) in place of the caller's o / softmax_lse
inline void split_redirect(const fa_fwd_params *p, const SplitPlan &sp, KParams &kp) {
    char *ws = static_cast<char *>(p->workspace);
    kp.o = ws;
    kp.lse = reinterpret_cast<float *>(ws + sp.o_bytes);
    kp.o_row_stride = (int64_t)p->h * kp.dv; kp.o_head_stride = kp.dv; kp.o_batch_stride = kp.o_row_stride * p->seqlen_q;
    kp.o_split_stride = kp.o_batch_stride * p->b;
    kp.lse_split_stride = (int64_t)p->b * p->h * p->seqlen_q;
    if (p->cu_seqlens_q) {
        kp.o_split_stride = kp.o_row_stride * p->total_q;
        kp.lse_split_stride = (int64_t)p->h * p->total_q;
    }
}
// ... and the public fa_fwd_combine merges them into the caller's.  Ragged queries are one "batch" of total_q rows to it.
inline fa_combine_params split_combine_params(const fa_fwd_params *p, const KParams &kp) {
    fa_combine_params c{};
    c.abi_version = FA_ABI_VERSION;
    c.struct_size = sizeof(fa_combine_params);
    c.out_partial = static_cast<const float *>(kp.o);
    c.lse_partial = kp.lse;
    c.out = p->o;
    c.softmax_lse = p->softmax_lse;
    const bool ragged = p->cu_seqlens_q != nullptr;
    const int64_t rows = ragged ? p->total_q : p->seqlen_q;
    c.b = ragged ? 1 : p->b; c.seqlen = (int32_t)rows; c.h = p->h; c.d = kp.dv; c.num_splits = kp.num_splits;
    c.op_split_stride = kp.o_split_stride; c.op_batch_stride = kp.o_row_stride * rows; c.op_row_stride = kp.o_row_stride; c.op_head_stride = kp.dv;
    c.lp_split_stride = kp.lse_split_stride; c.lp_batch_stride = (int64_t)p->h * rows; c.lp_head_stride = rows; c.lp_row_stride = 1;
    c.o_batch_stride = ragged ? 0 : p->o_batch_stride; c.o_row_stride = p->o_row_stride; c.o_head_stride = p->o_head_stride;
    c.lse_batch_stride = (int64_t)p->h * rows; c.lse_head_stride = rows; c.lse_row_stride = 1;
    c.out_dtype = p->dtype;
    return c;
}

// ---- the packed-row work shape (pk_fwd_kernel, fwd_kernel_qv, kv8_fwd_kernel, qv8_fwd_kernel): blocks of `block_m` packed rows
// (query row x head of the GQA group) per (batch, kv head, split) group; the groups are dealt over the 8 XCDs, the blocks of a
// group stay on one.  The kernels count all three in 32 bits.
struct PackedGrid {
    int64_t pblocks, groups, grid;
    int status;  // FA_ERR_BAD_SHAPE when one of them does not fit 31 bits
};
inline PackedGrid packed_grid(const fa_fwd_params *p, int block_m, int splits) {
    PackedGrid g{};
    g.pblocks = ((int64_t)p->seqlen_q * (p->h / p->h_k) + block_m - 1) / block_m;
    g.groups = (int64_t)p->b * p->h_k * splits;
    g.grid = (g.groups + 7) / 8 * 8 * g.pblocks;
    g.status = (g.pblocks > 0x7fffffff || g.groups > 0x7fffffff || g.grid > 0x7fffffff) ? FA_ERR_BAD_SHAPE : FA_OK;
    return g;
}

// ---- the routes over an fp8 (e4m3) KV cache, fa_fwd_kv8 and fa_fwd_qv8: one plan struct, one validate body, one fill, one merge
struct Fp8CachePlan {
    int tile;      // kv8_fwd_kernel: the head-dim tile D; qv8_fwd_kernel: the V tile DVT
    bool softcap;
    bool nothing;  // no query or no key: nothing is launched
    SplitPlan split;
    PackedGrid grid;
};
// Reads `p` alone (shapes, never device data).
inline Fp8CachePlan plan_fp8_cache(const fa_fwd_params *p, int tile, int block_m, int dv, int (*split_count)(const fa_fwd_params *)) {
    Fp8CachePlan pl{};
    pl.tile = tile;
    pl.softcap = p->softcap > 0.f;
    pl.nothing = p->seqlen_q == 0 || p->seqlen_k == 0 || (p->cu_seqlens_q && p->total_q == 0);
    pl.split = split_layout(p, pl.nothing ? 1 : split_count(p), dv);
    pl.grid = packed_grid(p, block_m, pl.split.splits);
    return pl;
}

// What fa_fwd_kv8_validate and fa_fwd_qv8_validate check behind their own shape rules (which have seen to b, h, h_k and the
// sequence lengths), in this order.  fa_fwd_kv8 has refused qv by then, so the qv terms are zeros there.
inline int validate_fp8_cache(const fa_fwd_params *p, Fp8CachePlan (*plan)(const fa_fwd_params *)) {
    const bool ragged = p->cu_seqlens_q != nullptr;
    if (ragged && (!p->seqused_k || p->total_q < 0)) return FA_ERR_BAD_SHAPE;
    const bool empty = p->seqlen_q == 0 || (ragged && p->total_q == 0);
    if (!empty) {
        if (!p->q || !p->o || !p->softmax_lse) return FA_ERR_NULL_POINTER;
        if (p->seqlen_k > 0 && (!p->k || !p->v)) return FA_ERR_NULL_POINTER;
    }
    // 16-byte vector loads / stores: q / o / qv strides are in 16-bit elements, k / v strides in bytes (their elements)
    const int64_t qo[] = {p->q_row_stride, p->q_head_stride, p->o_row_stride, p->o_head_stride,
                          ragged ? 0 : p->q_batch_stride, ragged ? 0 : p->o_batch_stride,
                          p->qv ? p->qv_row_stride : 0, p->qv ? p->qv_head_stride : 0, p->qv && !ragged ? p->qv_batch_stride : 0};
    for (int64_t s : qo)
        if (s % 8 != 0) return FA_ERR_BAD_STRIDE;
    const int64_t kv[] = {p->k_row_stride, p->k_head_stride, p->k_batch_stride, p->v_row_stride, p->v_head_stride, p->v_batch_stride};
    for (int64_t s : kv)
        if (s % 16 != 0) return FA_ERR_BAD_STRIDE;
    // The kernel addresses a tile as 64-bit base + 32-bit (row * stride) lane offset, row < 64: the row stride stays below 2^24
    // bytes.  The base is rebuilt per tile, so the extent of a cache entry is not bounded (2 GiB and more are fine).
    if (p->k_row_stride < 0 || p->v_row_stride < 0 || p->k_row_stride >= (1 << 24) || p->v_row_stride >= (1 << 24))
        return FA_ERR_BAD_STRIDE;
    const void *ptrs[] = {p->q, p->k, p->v, p->o, p->qv};
    for (const void *ptr : ptrs)
        if (reinterpret_cast<uintptr_t>(ptr) % 16 != 0) return FA_ERR_BAD_STRIDE;
    const int64_t ds[] = {p->k_descale_batch_stride, p->k_descale_head_stride, p->v_descale_batch_stride, p->v_descale_head_stride};
    for (int64_t s : ds)
        if (s < 0 || s > 0x7fffffff) return FA_ERR_BAD_STRIDE;
    if ((p->k_descale && reinterpret_cast<uintptr_t>(p->k_descale) % 4 != 0) || (p->v_descale && reinterpret_cast<uintptr_t>(p->v_descale) % 4 != 0))
        return FA_ERR_BAD_STRIDE;
    if (p->num_splits < 0) return FA_ERR_BAD_SHAPE;
    if (p->softcap < 0.f || std::isnan(p->softcap) || std::isnan(p->softmax_scale)) return FA_ERR_BAD_SHAPE;
    if (p->leftpad_k && p->block_table) return FA_ERR_UNSUPPORTED;  // as fa_fwd
    if (p->block_table) {
        if (p->kv_batch_idx) return FA_ERR_UNSUPPORTED;  // as fa_fwd
        if (p->page_block_size <= 0) return FA_ERR_BAD_SHAPE;  // any size
        if (p->block_table_batch_stride < 0 || p->block_table_batch_stride > 0x7fffffff) return FA_ERR_BAD_STRIDE;
    }
    const SplitPlan sp = plan(p).split;
    return sp.splits > 1 && workspace_short(p, sp.total) ? FA_ERR_WORKSPACE : FA_OK;
}

// The same for the routes that also read a 16-bit cache through the packed-row body (fa_fwd_sparse_kv, fa_fwd_tree):
// validate_fp8_cache's rules with k / v strides in 16-bit elements and no descales; the workspace check is the route's
inline int validate_16bit_cache(const fa_fwd_params *p) {
    const bool ragged = p->cu_seqlens_q != nullptr;
    if (ragged && (!p->seqused_k || p->total_q < 0)) return FA_ERR_BAD_SHAPE;
    const bool empty = p->seqlen_q == 0 || (ragged && p->total_q == 0);
    if (!empty) {
        if (!p->q || !p->o || !p->softmax_lse) return FA_ERR_NULL_POINTER;
        if (p->seqlen_k > 0 && (!p->k || !p->v)) return FA_ERR_NULL_POINTER;
    }
    const int64_t strides[] = {p->q_row_stride, p->q_head_stride, p->o_row_stride, p->o_head_stride,
                               ragged ? 0 : p->q_batch_stride, ragged ? 0 : p->o_batch_stride,
                               p->k_row_stride, p->k_head_stride, p->k_batch_stride, p->v_row_stride, p->v_head_stride, p->v_batch_stride};
    for (int64_t s : strides)
        if (s % 8 != 0) return FA_ERR_BAD_STRIDE;
    // 64-bit base per tile + 32-bit (row * stride) lane offset, row < 64
    if (p->k_row_stride < 0 || p->v_row_stride < 0 || p->k_row_stride >= (1 << 24) || p->v_row_stride >= (1 << 24))
        return FA_ERR_BAD_STRIDE;
    const void *ptrs[] = {p->q, p->k, p->v, p->o};
    for (const void *ptr : ptrs)
        if (reinterpret_cast<uintptr_t>(ptr) % 16 != 0) return FA_ERR_BAD_STRIDE;
    if (p->num_splits < 0) return FA_ERR_BAD_SHAPE;
    if (p->softcap < 0.f || std::isnan(p->softcap) || std::isnan(p->softmax_scale)) return FA_ERR_BAD_SHAPE;
    if (p->leftpad_k && p->block_table) return FA_ERR_UNSUPPORTED;  // as fa_fwd
    if (p->block_table) {
        if (p->kv_batch_idx) return FA_ERR_UNSUPPORTED;  // as fa_fwd
        if (p->page_block_size <= 0) return FA_ERR_BAD_SHAPE;  // any size
        if (p->block_table_batch_stride < 0 || p->block_table_batch_stride > 0x7fffffff) return FA_ERR_BAD_STRIDE;
    }
    return FA_OK;
}

// the kernel params of a launch that validate and the plan have accepted (the route adds what its kernel has beside KParams)
inline void fill_fp8_cache(const fa_fwd_params *p, const Fp8CachePlan &pl, int32_t dv, KParams &kp) {
    fwd_fill_params(p, dv, kp);
    fwd_fill_kv_descales(p, kp);  // (the kernel applies them itself; q_descale stays NULL: q is not quantised)
    kp.num_cus = fwd_device_cus();
    kp.num_splits = pl.split.splits;
    if (pl.split.splits > 1) split_redirect(p, pl.split, kp);
}
// behind the launch (its status): the merge of a split call
inline int merge_fp8_cache(const fa_fwd_params *p, const KParams &kp, int st_main, void *stream) {
    if (st_main != FA_OK || kp.num_splits <= 1) return st_main;
    const fa_combine_params c = split_combine_params(p, kp);
    return fa_fwd_combine(&c, stream);
}

}  // namespace fa
