// fa_fwd_sparse_kv_api.hip — C-ABI of the block-sparse forward over a KV cache (include/fa_fwd.h: fa_fwd_sparse_kv,
// fa_fwd_sparse_kv_validate, fa_fwd_sparse_kv_workspace_size, fa_fwd_sparse_kv_plan_name).  A translation unit of its own: the
// kernel sets of fa_fwd_api.hip, fa_fwd_kv8_api.hip and fa_fwd_qv8_api.hip are pinned.  Here: the route's shape rules, plan text
// and launch ladder over sp_fwd_kernel (fa_fwd_kernel_sp.h).  The params fill, the split layout, the packed-row grid, the fp8
// half of the validation and the merge (the public fa_fwd_combine) are the shared host path of fa_fwd_internal.h.
#include "fa_fwd.h"
#include "fa_fwd_internal.h"
#include "fa_fwd_kernel_sp.h"
#include "fa_launch.h"

#include <cstdio>

namespace {

using fa::Fp8CachePlan;

bool abi_ok(const fa_fwd_params *p, const fa_sparse_kv_params *s) {
    return p->abi_version == FA_ABI_VERSION && p->struct_size == sizeof(fa_fwd_params) && s->abi_version == FA_ABI_VERSION &&
           s->struct_size == sizeof(fa_sparse_kv_params);
}

// Parts of the list positions: num_splits 1 = off, N > 1 = N (clamped to the 64-key tiles of max_blocks blocks), 0 = what
// split_plan gives the pk shape for a key length of max_blocks * block_size.  Shapes only: the lists are never read here.
int split_count(const fa_fwd_params *p, const fa_sparse_kv_params *s) {
    fa_fwd_params as_long = *p;
    as_long.seqlen_k = (int32_t)((int64_t)s->max_blocks * s->block_size);
    return fa::fwd_pk_split_count(&as_long);
}

// pk_fwd_kernel's work shape, head-dim tile D = 64 or 128, V as wide as K.  Unlike the dense routes an empty cache or an empty
// list is no "nothing": the rows of such a call still get O = 0, LSE = +inf from the kernel
Fp8CachePlan plan_sparse(const fa_fwd_params *p, const fa_sparse_kv_params *s) {
    Fp8CachePlan pl{};
    pl.tile = p->d <= 64 ? 64 : 128;
    pl.softcap = p->softcap > 0.f;
    pl.nothing = p->seqlen_q == 0 || (p->cu_seqlens_q && p->total_q == 0);
    pl.split = fa::split_layout(p, pl.nothing ? 1 : split_count(p, s), p->d);
    pl.grid = fa::packed_grid(p, fa::PK_BLOCK_M, pl.split.splits);
    return pl;
}
// (validate_fp8_cache's workspace check reads a plan of the params alone; this route makes that check itself)
Fp8CachePlan plan_unsplit(const fa_fwd_params *p) {
    Fp8CachePlan pl{};
    pl.split = fa::split_layout(p, 1, p->d);
    return pl;
}

const char *plan_text(const Fp8CachePlan &pl, const fa_sparse_kv_params *s, char (&name)[160]) {
    if (pl.grid.status != FA_OK) return nullptr;
    snprintf(name, sizeof(name), "sp_fwd_kernel D=%d waves=%d%s KV=%s B=%d block_m=%d splits=%d", pl.tile, fa::PK_NWAVES,
             pl.softcap ? " SOFTCAP" : "", s->fp8_cache ? "e4m3" : "16", s->block_size, fa::PK_BLOCK_M, pl.split.splits);
    return name;
}

template <typename T, int D, typename KV>
int launch_form(const Fp8CachePlan &pl, const fa::SpParams &sa, hipStream_t stream) {
    constexpr int smem = KV::FP8_CACHE ? fa::smem_bytes_kv8<D>() : fa::smem_bytes<D, fa::PK_NWAVES>(), NT = fa::PK_NWAVES * 64;
    return pl.softcap ? fa::launch_kernel<fa::sp_fwd_kernel<T, D, true, KV>>(smem, pl.grid.grid, NT, stream, sa)
                      : fa::launch_kernel<fa::sp_fwd_kernel<T, D, false, KV>>(smem, pl.grid.grid, NT, stream, sa);
}
template <typename T, int D>
int launch_tile(const Fp8CachePlan &pl, bool fp8, const fa::SpParams &sa, hipStream_t stream) {
    return fp8 ? launch_form<T, D, fa::Kv8<T, D>>(pl, sa, stream) : launch_form<T, D, fa::Kv16<T, D>>(pl, sa, stream);
}
template <typename T>
int launch(const Fp8CachePlan &pl, bool fp8, const fa::SpParams &sa, hipStream_t stream) {
    return pl.tile == 64 ? launch_tile<T, 64>(pl, fp8, sa, stream) : launch_tile<T, 128>(pl, fp8, sa, stream);
}

}  // namespace

extern "C" {

uint32_t fa_sparse_kv_params_size(void) { return (uint32_t)sizeof(fa_sparse_kv_params); }

int fa_fwd_sparse_kv_validate(const fa_fwd_params *p, const fa_sparse_kv_params *s) {
    if (!p || !s) return FA_ERR_NULL_POINTER;
    if (!abi_ok(p, s)) return FA_ERR_BAD_ABI;
    // what this route does not serve comes first, whatever else the params may lack
    if (p->dtype == FA_DTYPE_FP8_E4M3) return FA_ERR_UNSUPPORTED;  // (q is 16-bit here, over either cache type)
    if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16) return FA_ERR_BAD_DTYPE;
    if (p->d <= 0) return FA_ERR_BAD_HEAD_DIM;
    if (p->d > 128 || p->d % 16 != 0) return FA_ERR_UNSUPPORTED;
    if (p->d_v != 0 && p->d_v != p->d) return FA_ERR_UNSUPPORTED;
    if (p->qv || p->alibi_slopes || p->p_dropout > 0.f || p->attention_chunk > 0 || p->s_dmask || p->cu_seqlens_k) return FA_ERR_UNSUPPORTED;
    if (!(p->p_dropout >= 0.f) || p->attention_chunk < 0) return FA_ERR_BAD_SHAPE;
    // the lists
    if (s->block_size <= 0 || s->block_size % fa::BLOCK_N != 0 || s->max_blocks < 0) return FA_ERR_BAD_SHAPE;
    if ((int64_t)s->max_blocks * s->block_size > 0x7fffffff) return FA_ERR_BAD_SHAPE;  // (the kernel counts list positions in 32 bits)
    if (!s->block_cnt || !s->block_idx) return FA_ERR_NULL_POINTER;
    if (reinterpret_cast<uintptr_t>(s->block_cnt) % 4 != 0 || reinterpret_cast<uintptr_t>(s->block_idx) % 4 != 0) return FA_ERR_BAD_STRIDE;
    if (s->cnt_batch_stride < 0 || s->cnt_head_stride < 0 || s->idx_batch_stride < 0 || s->idx_head_stride < 0) return FA_ERR_BAD_STRIDE;
    if (p->b <= 0 || p->h <= 0 || p->h_k <= 0 || p->seqlen_q < 0 || p->seqlen_k < 0) return FA_ERR_BAD_SHAPE;
    if (p->h % p->h_k != 0) return FA_ERR_BAD_HEADS;
    if ((int64_t)p->seqlen_q * (p->h / p->h_k) > 0x7fffffff) return FA_ERR_BAD_SHAPE;  // (the kernel counts packed rows in 32 bits)
    if (s->fp8_cache && (!p->k_descale || !p->v_descale)) return FA_ERR_NULL_POINTER;  // (both descales are required)
    const int st = s->fp8_cache ? fa::validate_fp8_cache(p, plan_unsplit) : fa::validate_16bit_cache(p);
    if (st != FA_OK) return st;
    const fa::SplitPlan sp = plan_sparse(p, s).split;
    return sp.splits > 1 && fa::workspace_short(p, sp.total) ? FA_ERR_WORKSPACE : FA_OK;
}

int64_t fa_fwd_sparse_kv_workspace_size(const fa_fwd_params *p, const fa_sparse_kv_params *s) {
    if (!p || !s) return FA_ERR_NULL_POINTER;
    if (!abi_ok(p, s)) return FA_ERR_BAD_ABI;
    if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16) return p->dtype == FA_DTYPE_FP8_E4M3 ? FA_ERR_UNSUPPORTED : FA_ERR_BAD_DTYPE;
    if (p->b <= 0 || p->h <= 0 || p->h_k <= 0 || p->d <= 0 || p->seqlen_q < 0 || p->seqlen_k < 0 || p->h % p->h_k != 0) return FA_ERR_BAD_SHAPE;
    if (p->cu_seqlens_q && p->total_q < 0) return FA_ERR_BAD_SHAPE;
    if (s->block_size <= 0 || s->block_size % fa::BLOCK_N != 0 || s->max_blocks < 0 || (int64_t)s->max_blocks * s->block_size > 0x7fffffff)
        return FA_ERR_BAD_SHAPE;
    if (p->cu_seqlens_k || p->p_dropout > 0.f || p->attention_chunk > 0 || (p->d_v != 0 && p->d_v != p->d)) return FA_ERR_UNSUPPORTED;
    return plan_sparse(p, s).split.total;
}

const char *fa_fwd_sparse_kv_plan_name(const fa_fwd_params *p, const fa_sparse_kv_params *s, int32_t /*num_cus*/) {
    if (fa_fwd_sparse_kv_validate(p, s) != FA_OK) return nullptr;
    thread_local char name[160];
    return plan_text(plan_sparse(p, s), s, name);
}

int fa_fwd_sparse_kv(const fa_fwd_params *p, const fa_sparse_kv_params *s, void *stream_) {
    const int st = fa_fwd_sparse_kv_validate(p, s);
    fa::fwd_set_last_plan_text(nullptr);
    if (st != FA_OK) return st;
    const Fp8CachePlan pl = plan_sparse(p, s);
    if (pl.grid.status != FA_OK) return pl.grid.status;
    char name[160];
    fa::fwd_set_last_plan_text(plan_text(pl, s, name));
    if (pl.nothing || pl.grid.pblocks == 0) return FA_OK;  // no query row: the caller owns the outputs of an empty problem

    fa::SpParams sa{};
    fa::fwd_fill_params(p, p->d, sa.pk.p);
    if (s->fp8_cache) fa::fwd_fill_kv_descales(p, sa.pk.p);  // (a 16-bit cache hands its kernel NULL: no descale is read)
    sa.pk.p.num_cus = fa::fwd_device_cus();
    sa.pk.p.num_splits = pl.split.splits;
    if (pl.split.splits > 1) fa::split_redirect(p, pl.split, sa.pk.p);
    sa.pk.num_pblocks = (int32_t)pl.grid.pblocks;
    sa.pk.num_groups = (int32_t)pl.grid.groups;
    sa.walk.block_cnt = s->block_cnt; sa.walk.block_idx = s->block_idx;
    sa.walk.cnt_batch_stride = s->cnt_batch_stride; sa.walk.cnt_head_stride = s->cnt_head_stride;
    sa.walk.idx_batch_stride = s->idx_batch_stride; sa.walk.idx_head_stride = s->idx_head_stride;
    sa.walk.max_blocks = s->max_blocks; sa.walk.block_size = s->block_size;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int st_main = p->dtype == FA_DTYPE_BF16 ? launch<__bf16>(pl, s->fp8_cache != 0, sa, stream) : launch<_Float16>(pl, s->fp8_cache != 0, sa, stream);
    return fa::merge_fp8_cache(p, sa.pk.p, st_main, stream_);
}

}  // extern "C"
