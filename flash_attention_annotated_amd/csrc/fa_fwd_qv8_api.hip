// fa_fwd_qv8_api.hip — C-ABI of the MLA decode shape over an fp8 (e4m3) KV cache with 16-bit q / qv / o (include/fa_fwd.h:
// fa_fwd_qv8, fa_fwd_qv8_validate, fa_fwd_qv8_workspace_size, fa_fwd_qv8_plan_name).  A translation unit of its own: the
// kernels of fa_fwd_api.hip and fa_fwd_kv8_api.hip are pinned sets.  The split-KV count (the 16-bit qv kernel's) and the
// last-plan text live in fa_fwd_api.hip (fa_fwd_internal.h); the merge of the split partials is the public fa_fwd_combine.
#include "fa_fwd.h"
#include "fa_fwd_internal.h"
#include "fa_fwd_kernel_qv8.h"
#include "fa_launch.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace {

struct Qv8Plan {
    int tile;      // V tile DVT of qv8_fwd_kernel: 256 (d_v = 256) or 512 (d_v in (256, 512])
    bool softcap;
    bool nothing;  // no query or no key: nothing is launched
    int splits;
    int64_t pblocks, groups, grid;
    int64_t o_bytes, lse_bytes, workspace;  // fp32 partials: O (splits, b, sq, h, d_v) / (splits, total_q, h, d_v), LSE (splits, b, h, sq) / (splits, h, total_q)
    int status;
};

inline int64_t query_rows(const fa_fwd_params *p) { return p->cu_seqlens_q ? p->total_q : (int64_t)p->b * p->seqlen_q; }

// The plan of one fa_fwd_qv8 call.  Reads `p` alone (shapes, never device data).
Qv8Plan plan_qv8(const fa_fwd_params *p) {
    Qv8Plan pl{};
    pl.status = FA_OK;
    pl.tile = p->d_v <= 256 ? 256 : 512;
    pl.softcap = p->softcap > 0.f;
    pl.nothing = p->seqlen_q == 0 || p->seqlen_k == 0 || (p->cu_seqlens_q && p->total_q == 0);
    pl.splits = pl.nothing ? 1 : fa::fwd_qv_split_count(p);
    if (pl.splits > 1) {
        const int64_t rows = query_rows(p);
        pl.o_bytes = (pl.splits * rows * p->h * p->d_v * 4 + 255) & ~int64_t(255);
        pl.lse_bytes = (pl.splits * rows * p->h * 4 + 255) & ~int64_t(255);
        pl.workspace = pl.o_bytes + pl.lse_bytes;
    }
    pl.pblocks = ((int64_t)p->seqlen_q * (p->h / p->h_k) + 31) / 32;
    pl.groups = (int64_t)p->b * p->h_k * pl.splits;
    pl.grid = (pl.groups + 7) / 8 * 8 * pl.pblocks;
    if (pl.pblocks > 0x7fffffff || pl.groups > 0x7fffffff || pl.grid > 0x7fffffff) pl.status = FA_ERR_BAD_SHAPE;
    return pl;
}

const char *plan_text(const Qv8Plan &pl, char (&name)[160]) {
    if (pl.status != FA_OK) return nullptr;
    snprintf(name, sizeof(name), "qv8_fwd_kernel DVT=%d waves=%d%s block_m=32 splits=%d", pl.tile, fa::QV_NWAVES,
             pl.softcap ? " SOFTCAP" : "", pl.splits);
    return name;
}

template <typename T, int DVT>
int launch_form(const Qv8Plan &pl, const fa::QvParams &qa, hipStream_t stream) {
    constexpr int smem = fa::smem_bytes_qv8<DVT>(), NT = fa::QV_NWAVES * 64;
    return pl.softcap ? fa::launch_kernel<fa::qv8_fwd_kernel<T, DVT, true>>(smem, pl.grid, NT, stream, qa)
                      : fa::launch_kernel<fa::qv8_fwd_kernel<T, DVT, false>>(smem, pl.grid, NT, stream, qa);
}
template <typename T>
int launch(const Qv8Plan &pl, const fa::QvParams &qa, hipStream_t stream) {
    return pl.tile == 256 ? launch_form<T, 256>(pl, qa, stream) : launch_form<T, 512>(pl, qa, stream);
}

// the shape rules both fa_fwd_qv8_validate and fa_fwd_qv8_workspace_size apply before anything is planned
int check_shape(const fa_fwd_params *p) {
    if (p->dtype == FA_DTYPE_FP8_E4M3) return FA_ERR_UNSUPPORTED;  // (q is 16-bit here; the all-fp8 call is fa_fwd's to refuse)
    if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16) return FA_ERR_BAD_DTYPE;
    if (p->d <= 0 || p->d_v <= 0) return FA_ERR_BAD_HEAD_DIM;  // (d_v is required)
    if (p->d > 64 || p->d % 16 != 0 || p->d_v < 256 || p->d_v > 512 || p->d_v % 16 != 0) return FA_ERR_UNSUPPORTED;  // (e4m3 rows keep 16-byte alignment)
    if (p->alibi_slopes || p->p_dropout > 0.f || p->attention_chunk > 0 || p->s_dmask || p->cu_seqlens_k) return FA_ERR_UNSUPPORTED;
    if (!(p->p_dropout >= 0.f) || p->attention_chunk < 0) return FA_ERR_BAD_SHAPE;
    if (p->b <= 0 || p->h <= 0 || p->h_k <= 0 || p->seqlen_q < 0 || p->seqlen_k < 0) return FA_ERR_BAD_SHAPE;
    if (p->h % p->h_k != 0) return FA_ERR_BAD_HEADS;
    if ((int64_t)p->seqlen_q * (p->h / p->h_k) > 0x7fffffff) return FA_ERR_BAD_SHAPE;  // (the kernel counts packed rows in 32 bits)
    if (p->cu_seqlens_q && p->total_q < 0) return FA_ERR_BAD_SHAPE;
    return FA_OK;
}

}  // namespace

extern "C" {

int fa_fwd_qv8_validate(const fa_fwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_fwd_params)) return FA_ERR_BAD_ABI;
    // what this route does not serve comes first, whatever else the params may lack
    const int shape = check_shape(p);
    if (shape != FA_OK) return shape;
    const bool ragged = p->cu_seqlens_q != nullptr;
    if (ragged && !p->seqused_k) return FA_ERR_BAD_SHAPE;
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
    const Qv8Plan pl = plan_qv8(p);
    if (pl.splits > 1 &&
        (!p->workspace || reinterpret_cast<uintptr_t>(p->workspace) % 256 != 0 || (int64_t)p->workspace_bytes < pl.workspace))
        return FA_ERR_WORKSPACE;
    return FA_OK;
}

int64_t fa_fwd_qv8_workspace_size(const fa_fwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_fwd_params)) return FA_ERR_BAD_ABI;
    const int shape = check_shape(p);
    if (shape != FA_OK) return shape;
    return plan_qv8(p).workspace;
}

const char *fa_fwd_qv8_plan_name(const fa_fwd_params *p, int32_t /*num_cus*/) {
    if (fa_fwd_qv8_validate(p) != FA_OK) return nullptr;
    thread_local char name[160];
    return plan_text(plan_qv8(p), name);
}

int fa_fwd_qv8(const fa_fwd_params *p, void *stream_) {
    const int st = fa_fwd_qv8_validate(p);
    fa::fwd_set_last_plan_text(nullptr);
    if (st != FA_OK) return st;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const Qv8Plan pl = plan_qv8(p);
    if (pl.status != FA_OK) return pl.status;
    char name[160];
    fa::fwd_set_last_plan_text(plan_text(pl, name));
    if (pl.nothing || pl.pblocks == 0) return FA_OK;  // nothing to compute: the caller owns the outputs of an empty problem

    fa::QvParams qa{};
    fa::KParams &kp = qa.p;
    kp.q = p->q; kp.k = p->k; kp.v = p->v; kp.o = p->o; kp.lse = p->softmax_lse;
    kp.cu_seqlens_q = p->cu_seqlens_q; kp.seqused_q = p->seqused_q; kp.seqused_k = p->seqused_k;
    kp.q_batch_stride = p->q_batch_stride; kp.q_row_stride = p->q_row_stride; kp.q_head_stride = p->q_head_stride;
    kp.k_batch_stride = p->k_batch_stride; kp.k_row_stride = p->k_row_stride; kp.k_head_stride = p->k_head_stride;
    kp.v_batch_stride = p->v_batch_stride; kp.v_row_stride = p->v_row_stride; kp.v_head_stride = p->v_head_stride;
    kp.o_batch_stride = p->o_batch_stride; kp.o_row_stride = p->o_row_stride; kp.o_head_stride = p->o_head_stride;
    kp.b = p->b; kp.seqlen_q = p->seqlen_q; kp.seqlen_k = p->seqlen_k; kp.h = p->h; kp.h_k = p->h_k; kp.d = p->d;
    kp.total_q = p->total_q;
    kp.dv = p->d_v;
    kp.h_ratio = p->h / p->h_k;
    kp.num_cus = fa::fwd_device_cus();
    kp.k_descale = p->k_descale; kp.v_descale = p->v_descale;  // (the kernel applies them itself; q_descale stays NULL)
    kp.kd_bs = (int32_t)p->k_descale_batch_stride; kp.kd_hs = (int32_t)p->k_descale_head_stride;
    kp.vd_bs = (int32_t)p->v_descale_batch_stride; kp.vd_hs = (int32_t)p->v_descale_head_stride;
    kp.num_splits = pl.splits;
    if (pl.splits > 1) {
        char *ws = static_cast<char *>(p->workspace);
        kp.o = ws;
        kp.lse = reinterpret_cast<float *>(ws + pl.o_bytes);
        kp.o_row_stride = (int64_t)p->h * p->d_v; kp.o_head_stride = p->d_v; kp.o_batch_stride = kp.o_row_stride * p->seqlen_q;
        kp.o_split_stride = kp.o_batch_stride * p->b;
        kp.lse_split_stride = (int64_t)p->b * p->h * p->seqlen_q;
        if (p->cu_seqlens_q) {  // ragged queries: (splits, total_q, h, d_v) and (splits, h, total_q)
            kp.o_split_stride = kp.o_row_stride * p->total_q;
            kp.lse_split_stride = (int64_t)p->h * p->total_q;
        }
    }
    // windows: the FA3 rule with FA_FLAG_FA3_WINDOW (a negative side is unbounded), fa_fwd's FA2 normalisation without it
    int wl = p->window_size_left, wr = p->window_size_right;
    if (p->is_causal) wr = 0;
    if (!(p->flags & FA_FLAG_FA3_WINDOW)) {
        if (wl >= p->seqlen_k) wl = -1;
        if (wr >= p->seqlen_k) wr = -1;
        if (p->is_causal) wr = 0;
        if (wl >= 0 && wr < 0) wr = p->seqlen_k;
    }
    kp.window_left = wl;
    kp.window_right = wr;
    kp.leftpad_k = p->leftpad_k;
    kp.kv_batch_idx = p->kv_batch_idx;
    kp.block_table = p->block_table;
    kp.bt_bs = (int32_t)p->block_table_batch_stride;
    kp.page_size = p->page_block_size;
    kp.drop_thr = 255;
    kp.rp_dropout = 1.f;
    constexpr float kLog2e = 1.4426950408889634f;
    if (pl.softcap) {
        kp.softcap_pre = p->softmax_scale / p->softcap;
        kp.scale = p->softcap;
        kp.scale_log2 = p->softcap * kLog2e;
    } else {
        kp.softcap_pre = 0.f;
        kp.scale = p->softmax_scale;
        kp.scale_log2 = p->softmax_scale * kLog2e;
    }
    qa.qv = p->qv;
    qa.qv_batch_stride = p->qv_batch_stride; qa.qv_row_stride = p->qv_row_stride; qa.qv_head_stride = p->qv_head_stride;
    qa.num_pblocks = (int32_t)pl.pblocks;
    qa.num_groups = (int32_t)pl.groups;

    const int st_main = p->dtype == FA_DTYPE_BF16 ? launch<__bf16>(pl, qa, stream) : launch<_Float16>(pl, qa, stream);
    if (st_main != FA_OK || pl.splits <= 1) return st_main;

    // merge: the public combine over the partials, d = d_v.  Ragged queries are one "batch" of total_q rows to it.
    fa_combine_params c{};
    c.abi_version = FA_ABI_VERSION;
    c.struct_size = sizeof(fa_combine_params);
    c.out_partial = static_cast<const float *>(kp.o);
    c.lse_partial = kp.lse;
    c.out = p->o;
    c.softmax_lse = p->softmax_lse;
    const bool ragged = p->cu_seqlens_q != nullptr;
    const int64_t rows = ragged ? p->total_q : p->seqlen_q;
    c.b = ragged ? 1 : p->b; c.seqlen = (int32_t)rows; c.h = p->h; c.d = p->d_v; c.num_splits = pl.splits;
    c.op_split_stride = kp.o_split_stride; c.op_batch_stride = kp.o_row_stride * rows; c.op_row_stride = kp.o_row_stride; c.op_head_stride = p->d_v;
    c.lp_split_stride = kp.lse_split_stride; c.lp_batch_stride = (int64_t)p->h * rows; c.lp_head_stride = rows; c.lp_row_stride = 1;
    c.o_batch_stride = ragged ? 0 : p->o_batch_stride; c.o_row_stride = p->o_row_stride; c.o_head_stride = p->o_head_stride;
    c.lse_batch_stride = (int64_t)p->h * rows; c.lse_head_stride = rows; c.lse_row_stride = 1;
    c.out_dtype = p->dtype;
    return fa_fwd_combine(&c, stream_);
}

}  // extern "C"
