// fa_fwd_tree_api.hip — C-ABI of tree attention over a KV cache (include/fa_fwd.h: fa_fwd_tree, fa_fwd_tree_validate,
// fa_fwd_tree_workspace_size, fa_fwd_tree_plan_name).  A translation unit of its own: the kernel sets of fa_fwd_api.hip,
// fa_fwd_kv8_api.hip, fa_fwd_qv8_api.hip and fa_fwd_sparse_kv_api.hip are pinned.  Here: the route's shape rules, plan text and
// launch ladder over tr_fwd_kernel (fa_fwd_kernel_tr.h).  The params fill, the split layout, the packed-row grid, both halves of
// the validation and the merge (the public fa_fwd_combine) are the shared host path of fa_fwd_internal.h.
#include "fa_fwd.h"
#include "fa_fwd_internal.h"
#include "fa_fwd_kernel_tr.h"
#include "fa_launch.h"

#include <cstdio>

namespace {

using fa::Fp8CachePlan;

constexpr int MAX_NODES = 64;  // bits of a word

bool abi_ok(const fa_fwd_params *p, const fa_tree_params *t) {
    return p->abi_version == FA_ABI_VERSION && p->struct_size == sizeof(fa_fwd_params) && t->abi_version == FA_ABI_VERSION &&
           t->struct_size == sizeof(fa_tree_params);
}

// what the route does not serve, by the params alone (both the validation and the workspace size say it first)
bool unsupported(const fa_fwd_params *p) {
    if (p->d > 128 || p->d % 16 != 0 || (p->d_v != 0 && p->d_v != p->d) || p->seqlen_q > MAX_NODES) return true;
    if (p->is_causal || p->window_size_left >= 0 || p->window_size_right >= 0 || p->attention_chunk > 0) return true;
    return p->qv || p->alibi_slopes || p->p_dropout > 0.f || p->s_dmask || p->cu_seqlens_k;
}

// pk_fwd_kernel's work shape and its parts of the key range, head-dim tile D = 64 or 128, V as wide as K.  Unlike the dense
// routes an empty cache is no "nothing": the rows of such a call still get O = 0, LSE = +inf from the kernel
Fp8CachePlan plan_tree(const fa_fwd_params *p) {
    Fp8CachePlan pl{};
    pl.tile = p->d <= 64 ? 64 : 128;
    pl.softcap = p->softcap > 0.f;
    pl.nothing = p->seqlen_q == 0 || (p->cu_seqlens_q && p->total_q == 0);
    pl.split = fa::split_layout(p, pl.nothing ? 1 : fa::fwd_pk_split_count(p), p->d);
    pl.grid = fa::packed_grid(p, fa::PK_BLOCK_M, pl.split.splits);
    return pl;
}
// (validate_fp8_cache's workspace check reads a plan of the params alone; this route makes that check itself)
Fp8CachePlan plan_unsplit(const fa_fwd_params *p) {
    Fp8CachePlan pl{};
    pl.split = fa::split_layout(p, 1, p->d);
    return pl;
}

const char *plan_text(const Fp8CachePlan &pl, const fa_tree_params *t, char (&name)[160]) {
    if (pl.grid.status != FA_OK) return nullptr;
    snprintf(name, sizeof(name), "tr_fwd_kernel D=%d waves=%d%s KV=%s block_m=%d splits=%d", pl.tile, fa::PK_NWAVES,
             pl.softcap ? " SOFTCAP" : "", t->fp8_cache ? "e4m3" : "16", fa::PK_BLOCK_M, pl.split.splits);
    return name;
}

template <typename T, int D, typename KV>
int launch_form(const Fp8CachePlan &pl, const fa::TrParams &ta, hipStream_t stream) {
    constexpr int smem = KV::FP8_CACHE ? fa::smem_bytes_kv8<D>() : fa::smem_bytes<D, fa::PK_NWAVES>(), NT = fa::PK_NWAVES * 64;
    return pl.softcap ? fa::launch_kernel<fa::tr_fwd_kernel<T, D, true, KV>>(smem, pl.grid.grid, NT, stream, ta)
                      : fa::launch_kernel<fa::tr_fwd_kernel<T, D, false, KV>>(smem, pl.grid.grid, NT, stream, ta);
}
template <typename T, int D>
int launch_tile(const Fp8CachePlan &pl, bool fp8, const fa::TrParams &ta, hipStream_t stream) {
    return fp8 ? launch_form<T, D, fa::Kv8<T, D>>(pl, ta, stream) : launch_form<T, D, fa::Kv16<T, D>>(pl, ta, stream);
}
template <typename T>
int launch(const Fp8CachePlan &pl, bool fp8, const fa::TrParams &ta, hipStream_t stream) {
    return pl.tile == 64 ? launch_tile<T, 64>(pl, fp8, ta, stream) : launch_tile<T, 128>(pl, fp8, ta, stream);
}

}  // namespace

extern "C" {

uint32_t fa_tree_params_size(void) { return (uint32_t)sizeof(fa_tree_params); }

int fa_fwd_tree_validate(const fa_fwd_params *p, const fa_tree_params *t) {
    if (!p || !t) return FA_ERR_NULL_POINTER;
    if (!abi_ok(p, t)) return FA_ERR_BAD_ABI;
    // what this route does not serve comes first, whatever else the params may lack
    if (p->dtype == FA_DTYPE_FP8_E4M3) return FA_ERR_UNSUPPORTED;  // (q is 16-bit here, over either cache type)
    if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16) return FA_ERR_BAD_DTYPE;
    if (p->d <= 0) return FA_ERR_BAD_HEAD_DIM;
    if (unsupported(p)) return FA_ERR_UNSUPPORTED;
    if (!(p->p_dropout >= 0.f) || p->attention_chunk < 0) return FA_ERR_BAD_SHAPE;
    // the words
    if (!t->tree_mask) return FA_ERR_NULL_POINTER;
    if (reinterpret_cast<uintptr_t>(t->tree_mask) % 8 != 0 || t->batch_stride < 0 || t->row_stride < 0) return FA_ERR_BAD_STRIDE;
    if (p->b <= 0 || p->h <= 0 || p->h_k <= 0 || p->seqlen_q < 0 || p->seqlen_k < 0) return FA_ERR_BAD_SHAPE;
    if (p->h % p->h_k != 0) return FA_ERR_BAD_HEADS;
    if (t->fp8_cache && (!p->k_descale || !p->v_descale)) return FA_ERR_NULL_POINTER;  // (both descales are required)
    const int st = t->fp8_cache ? fa::validate_fp8_cache(p, plan_unsplit) : fa::validate_16bit_cache(p);
    if (st != FA_OK) return st;
    const fa::SplitPlan sp = plan_tree(p).split;
    return sp.splits > 1 && fa::workspace_short(p, sp.total) ? FA_ERR_WORKSPACE : FA_OK;
}

int64_t fa_fwd_tree_workspace_size(const fa_fwd_params *p, const fa_tree_params *t) {
    if (!p || !t) return FA_ERR_NULL_POINTER;
    if (!abi_ok(p, t)) return FA_ERR_BAD_ABI;
    if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16) return p->dtype == FA_DTYPE_FP8_E4M3 ? FA_ERR_UNSUPPORTED : FA_ERR_BAD_DTYPE;
    if (p->b <= 0 || p->h <= 0 || p->h_k <= 0 || p->d <= 0 || p->seqlen_q < 0 || p->seqlen_k < 0 || p->h % p->h_k != 0) return FA_ERR_BAD_SHAPE;
    if (p->cu_seqlens_q && p->total_q < 0) return FA_ERR_BAD_SHAPE;
    if (unsupported(p)) return FA_ERR_UNSUPPORTED;
    return plan_tree(p).split.total;
}

const char *fa_fwd_tree_plan_name(const fa_fwd_params *p, const fa_tree_params *t, int32_t /*num_cus*/) {
    if (fa_fwd_tree_validate(p, t) != FA_OK) return nullptr;
    thread_local char name[160];
    return plan_text(plan_tree(p), t, name);
}

int fa_fwd_tree(const fa_fwd_params *p, const fa_tree_params *t, void *stream_) {
    const int st = fa_fwd_tree_validate(p, t);
    fa::fwd_set_last_plan_text(nullptr);
    if (st != FA_OK) return st;
    const Fp8CachePlan pl = plan_tree(p);
    if (pl.grid.status != FA_OK) return pl.grid.status;
    char name[160];
    fa::fwd_set_last_plan_text(plan_text(pl, t, name));
    if (pl.nothing || pl.grid.pblocks == 0) return FA_OK;  // no query row: the caller owns the outputs of an empty problem

    fa::TrParams ta{};
    fa::fwd_fill_params(p, p->d, ta.pk.p);
    if (t->fp8_cache) fa::fwd_fill_kv_descales(p, ta.pk.p);  // (a 16-bit cache hands its kernel NULL: no descale is read)
    ta.pk.p.num_cus = fa::fwd_device_cus();
    ta.pk.p.num_splits = pl.split.splits;
    if (pl.split.splits > 1) fa::split_redirect(p, pl.split, ta.pk.p);
    ta.pk.num_pblocks = (int32_t)pl.grid.pblocks;
    ta.pk.num_groups = (int32_t)pl.grid.groups;
    ta.mask.words = t->tree_mask;
    ta.mask.batch_stride = p->cu_seqlens_q ? 0 : t->batch_stride;
    ta.mask.row_stride = t->row_stride;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int st_main = p->dtype == FA_DTYPE_BF16 ? launch<__bf16>(pl, t->fp8_cache != 0, ta, stream) : launch<_Float16>(pl, t->fp8_cache != 0, ta, stream);
    return fa::merge_fp8_cache(p, ta.pk.p, st_main, stream_);
}

}  // extern "C"
