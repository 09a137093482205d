// fa_fwd_topk_kv8_api.hip — C-ABI of the top-k token-sparse MLA decode over the fp8 (e4m3) latent KV cache (include/fa_fwd.h:
// fa_fwd_topk_kv8, fa_fwd_topk_kv8_validate, fa_fwd_topk_kv8_workspace_size, fa_fwd_topk_kv8_plan_name).  A translation unit of
// its own: the kernel sets of the other forward units are pinned.  Here: the route's shape rules, plan text and launch ladder
// over tk8_fwd_kernel (fa_fwd_kernel_tk8.h).  The list rules and the plan are fa_fwd_topk_kv's, the cache rules fa_fwd_qv8's;
// the params fill, the split layout, the packed-row grid, the cache half of the validation and the merge (the public
// fa_fwd_combine) are the shared host path of fa_fwd_internal.h.
#include "fa_fwd.h"
#include "fa_fwd_internal.h"
#include "fa_fwd_kernel_tk8.h"
#include "fa_launch.h"

#include <algorithm>
#include <cstdio>

namespace {

bool abi_ok(const fa_fwd_params *p, const fa_topk_kv_params *s) {
    return p->abi_version == FA_ABI_VERSION && p->struct_size == sizeof(fa_fwd_params) && s->abi_version == FA_ABI_VERSION &&
           s->struct_size == sizeof(fa_topk_kv_params);
}

// The call as the work shape sees it (fa_fwd_topk_kv's): every (batch, token) is a single-token query of its own over a key
// range of topk positions.
fa_fwd_params per_token(const fa_fwd_params *p, const fa_topk_kv_params *s) {
    fa_fwd_params t = *p;
    t.b = (int32_t)std::min<int64_t>((int64_t)p->b * p->seqlen_q, 0x7fffffff);
    t.seqlen_q = p->seqlen_q > 0 ? 1 : 0;
    t.seqlen_k = s->topk;
    t.block_table = nullptr;  // (the split heuristic reads shapes only)
    return t;
}

struct TopkPlan {
    int tile;      // the V tile DVT
    bool nothing;  // no query token: nothing is launched (an empty cache still is: its rows get O = 0, LSE = +inf)
    fa::SplitPlan split;
    fa::PackedGrid grid;
};
// Shapes only: the list and the fill levels are never read here.  The parts are the 16-bit call's for the same shapes.
TopkPlan plan_topk(const fa_fwd_params *p, const fa_topk_kv_params *s) {
    TopkPlan pl{};
    pl.tile = p->d_v <= 256 ? 256 : 512;
    pl.nothing = p->seqlen_q == 0;
    const fa_fwd_params t = per_token(p, s);
    const int parts = pl.nothing ? 1 : p->num_splits > 0 ? std::min(p->num_splits, 128) : fa::fwd_qv_split_count(&t);
    pl.split = fa::split_layout(p, parts, p->d_v);
    pl.grid = fa::packed_grid(&t, 32, pl.split.splits);
    if ((int64_t)p->b * p->seqlen_q > 0x7fffffff) pl.grid.status = FA_ERR_BAD_SHAPE;
    return pl;
}

const char *plan_text(const TopkPlan &pl, const fa_topk_kv_params *s, char (&name)[160]) {
    if (pl.grid.status != FA_OK) return nullptr;
    snprintf(name, sizeof(name), "tk8_fwd_kernel DVT=%d waves=%d topk=%d splits=%d", pl.tile, fa::QV_NWAVES, s->topk, pl.split.splits);
    return name;
}

template <typename T, int DVT>
int launch_form(const TopkPlan &pl, const fa::TkParams &ta, hipStream_t stream) {
    return fa::launch_kernel<fa::tk8_fwd_kernel<T, DVT>>(fa::smem_bytes_tk8<DVT>(), pl.grid.grid, fa::QV_NWAVES * 64, stream, ta);
}
template <typename T>
int launch(const TopkPlan &pl, const fa::TkParams &ta, hipStream_t stream) {
    return pl.tile == 256 ? launch_form<T, 256>(pl, ta, stream) : launch_form<T, 512>(pl, ta, stream);
}

// what this route does not serve, and the list: before anything is planned and before anything else the params may lack
int check_shape(const fa_fwd_params *p, const fa_topk_kv_params *s) {
    if (p->dtype == FA_DTYPE_FP8_E4M3) return FA_ERR_UNSUPPORTED;  // (q is 16-bit here)
    if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16) return FA_ERR_BAD_DTYPE;
    if (p->d <= 0 || p->d_v <= 0) return FA_ERR_BAD_HEAD_DIM;  // (d_v is required)
    if (p->d > 64 || p->d % 16 != 0 || p->d_v < 256 || p->d_v > 512 || p->d_v % 16 != 0) return FA_ERR_UNSUPPORTED;  // (e4m3 rows keep 16-byte alignment)
    if (p->is_causal || p->window_size_left >= 0 || p->window_size_right >= 0 || p->attention_chunk > 0 || p->softcap > 0.f ||
        p->alibi_slopes || p->p_dropout > 0.f || p->s_dmask || p->leftpad_k || p->cu_seqlens_q || p->cu_seqlens_k)
        return FA_ERR_UNSUPPORTED;
    if (p->block_table && p->kv_batch_idx) return FA_ERR_UNSUPPORTED;
    if (!(p->p_dropout >= 0.f) || p->attention_chunk < 0) return FA_ERR_BAD_SHAPE;
    if (!s->indices) return FA_ERR_NULL_POINTER;
    if (s->topk < 1) return FA_ERR_BAD_SHAPE;
    if (s->batch_stride < 0 || s->row_stride < 0 || s->head_stride < 0 || reinterpret_cast<uintptr_t>(s->indices) % 4 != 0)
        return FA_ERR_BAD_STRIDE;
    if (p->b <= 0 || p->h <= 0 || p->h_k <= 0 || p->seqlen_q < 0 || p->seqlen_k < 0) return FA_ERR_BAD_SHAPE;
    if (p->h % p->h_k != 0) return FA_ERR_BAD_HEADS;
    return FA_OK;
}

}  // namespace

extern "C" {

int fa_fwd_topk_kv8_validate(const fa_fwd_params *p, const fa_topk_kv_params *s) {
    if (!p || !s) return FA_ERR_NULL_POINTER;
    if (!abi_ok(p, s)) return FA_ERR_BAD_ABI;
    int st = check_shape(p, s);
    if (st != FA_OK) return st;
    // fa_fwd_qv8's cache rules: byte strides, 16-byte alignment, row stride below 2^24 bytes, descale strides.  The workspace
    // is this route's to check (its parts come from the list), so the shared body sees an unsplit plan.
    st = fa::validate_fp8_cache(p, [](const fa_fwd_params *) { return fa::Fp8CachePlan{}; });
    if (st != FA_OK) return st;
    const TopkPlan pl = plan_topk(p, s);
    if (pl.grid.status != FA_OK) return pl.grid.status;
    return pl.split.splits > 1 && fa::workspace_short(p, pl.split.total) ? FA_ERR_WORKSPACE : FA_OK;
}

int64_t fa_fwd_topk_kv8_workspace_size(const fa_fwd_params *p, const fa_topk_kv_params *s) {
    if (!p || !s) return FA_ERR_NULL_POINTER;
    if (!abi_ok(p, s)) return FA_ERR_BAD_ABI;
    const int st = check_shape(p, s);
    return st != FA_OK ? st : plan_topk(p, s).split.total;
}

const char *fa_fwd_topk_kv8_plan_name(const fa_fwd_params *p, const fa_topk_kv_params *s, int32_t /*num_cus*/) {
    if (fa_fwd_topk_kv8_validate(p, s) != FA_OK) return nullptr;
    thread_local char name[160];
    return plan_text(plan_topk(p, s), s, name);
}

int fa_fwd_topk_kv8(const fa_fwd_params *p, const fa_topk_kv_params *s, void *stream_) {
    const int st = fa_fwd_topk_kv8_validate(p, s);
    fa::fwd_set_last_plan_text(nullptr);
    if (st != FA_OK) return st;
    const TopkPlan pl = plan_topk(p, s);
    char name[160];
    fa::fwd_set_last_plan_text(plan_text(pl, s, name));
    if (pl.nothing) return FA_OK;  // no query token: the caller owns the outputs of an empty problem

    fa::TkParams ta{};
    fa::KParams &kp = ta.qa.p;
    fa::fwd_fill_params(p, p->d_v, kp);
    fa::fwd_fill_kv_descales(p, kp);  // (NULL = 1; the kernel applies them itself)
    kp.num_cus = fa::fwd_device_cus();
    kp.num_splits = pl.split.splits;
    if (pl.split.splits > 1) fa::split_redirect(p, pl.split, kp);
    ta.qa.qv = p->qv;
    ta.qa.qv_batch_stride = p->qv_batch_stride; ta.qa.qv_row_stride = p->qv_row_stride; ta.qa.qv_head_stride = p->qv_head_stride;
    ta.qa.num_pblocks = (int32_t)pl.grid.pblocks;
    ta.qa.num_groups = (int32_t)pl.grid.groups;
    ta.indices = s->indices;
    ta.idx_batch_stride = s->batch_stride; ta.idx_row_stride = s->row_stride; ta.idx_head_stride = s->head_stride;
    ta.topk = s->topk;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int st_main = p->dtype == FA_DTYPE_BF16 ? launch<__bf16>(pl, ta, stream) : launch<_Float16>(pl, ta, stream);
    return fa::merge_fp8_cache(p, kp, st_main, stream_);
}

}  // extern "C"
