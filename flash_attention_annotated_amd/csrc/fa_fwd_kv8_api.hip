// fa_fwd_kv8_api.hip — C-ABI of the forward over an fp8 (e4m3) KV cache with 16-bit queries (include/fa_fwd.h: fa_fwd_kv8,
// fa_fwd_kv8_validate, fa_fwd_kv8_workspace_size, fa_fwd_kv8_plan_name).  A translation unit of its own: the kernels of
// fa_fwd_api.hip are a pinned set.  Here: the route's shape rules, plan text and launch ladder.  The plan, the rest of the
// validation, the params fill and the merge (the public fa_fwd_combine) are fa_fwd_qv8's too: fa_fwd_internal.h.
#include "fa_fwd.h"
#include "fa_fwd_internal.h"
#include "fa_fwd_kernel_kv8.h"
#include "fa_launch.h"

#include <cstdio>

namespace {

using fa::Fp8CachePlan;

// pk_fwd_kernel's work shape and split count, head-dim tile D = 64 or 128, V as wide as K
Fp8CachePlan plan_kv8(const fa_fwd_params *p) {
    return fa::plan_fp8_cache(p, p->d <= 64 ? 64 : 128, fa::PK_BLOCK_M, p->d, fa::fwd_pk_split_count);
}

const char *plan_text(const Fp8CachePlan &pl, char (&name)[160]) {
    if (pl.grid.status != FA_OK) return nullptr;
    snprintf(name, sizeof(name), "kv8_fwd_kernel D=%d waves=%d%s block_m=%d splits=%d", pl.tile, fa::PK_NWAVES,
             pl.softcap ? " SOFTCAP" : "", fa::PK_BLOCK_M, pl.split.splits);
    return name;
}

template <typename T, int D>
int launch_form(const Fp8CachePlan &pl, const fa::PkParams &pa, hipStream_t stream) {
    constexpr int smem = fa::smem_bytes_kv8<D>(), NT = fa::PK_NWAVES * 64;
    return pl.softcap ? fa::launch_kernel<fa::kv8_fwd_kernel<T, D, true>>(smem, pl.grid.grid, NT, stream, pa)
                      : fa::launch_kernel<fa::kv8_fwd_kernel<T, D, false>>(smem, pl.grid.grid, NT, stream, pa);
}
template <typename T>
int launch(const Fp8CachePlan &pl, const fa::PkParams &pa, hipStream_t stream) {
    return pl.tile == 64 ? launch_form<T, 64>(pl, pa, stream) : launch_form<T, 128>(pl, pa, stream);
}

}  // namespace

extern "C" {

int fa_fwd_kv8_validate(const fa_fwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_fwd_params)) return FA_ERR_BAD_ABI;
    // what this route does not serve comes first, whatever else the params may lack
    if (p->dtype == FA_DTYPE_FP8_E4M3) return FA_ERR_UNSUPPORTED;  // (q is 16-bit here; the all-fp8 call is fa_fwd's to refuse)
    if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16) return FA_ERR_BAD_DTYPE;
    if (p->d <= 0) return FA_ERR_BAD_HEAD_DIM;
    if (p->d > 128 || p->d % 16 != 0) return FA_ERR_UNSUPPORTED;  // (an e4m3 row keeps 16-byte alignment)
    if (p->d_v != 0 && p->d_v != p->d) return FA_ERR_UNSUPPORTED;
    if (p->qv || p->alibi_slopes || p->p_dropout > 0.f || p->attention_chunk > 0 || p->s_dmask || p->cu_seqlens_k) return FA_ERR_UNSUPPORTED;
    if (!(p->p_dropout >= 0.f) || p->attention_chunk < 0) return FA_ERR_BAD_SHAPE;
    if (p->b <= 0 || p->h <= 0 || p->h_k <= 0 || p->seqlen_q < 0 || p->seqlen_k < 0) return FA_ERR_BAD_SHAPE;
    if (p->h % p->h_k != 0) return FA_ERR_BAD_HEADS;
    if ((int64_t)p->seqlen_q * (p->h / p->h_k) > 0x7fffffff) return FA_ERR_BAD_SHAPE;  // (the kernel counts packed rows in 32 bits)
    return fa::validate_fp8_cache(p, plan_kv8);
}

int64_t fa_fwd_kv8_workspace_size(const fa_fwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_fwd_params)) return FA_ERR_BAD_ABI;
    if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16) return p->dtype == FA_DTYPE_FP8_E4M3 ? FA_ERR_UNSUPPORTED : FA_ERR_BAD_DTYPE;
    if (p->b <= 0 || p->h <= 0 || p->h_k <= 0 || p->d <= 0 || p->seqlen_q < 0 || p->seqlen_k < 0 || p->h % p->h_k != 0) return FA_ERR_BAD_SHAPE;
    if (p->cu_seqlens_q && p->total_q < 0) return FA_ERR_BAD_SHAPE;
    if (p->cu_seqlens_k || p->p_dropout > 0.f || p->attention_chunk > 0 || (p->d_v != 0 && p->d_v != p->d)) return FA_ERR_UNSUPPORTED;
    return plan_kv8(p).split.total;
}

const char *fa_fwd_kv8_plan_name(const fa_fwd_params *p, int32_t /*num_cus*/) {
    if (fa_fwd_kv8_validate(p) != FA_OK) return nullptr;
    thread_local char name[160];
    return plan_text(plan_kv8(p), name);
}

int fa_fwd_kv8(const fa_fwd_params *p, void *stream_) {
    const int st = fa_fwd_kv8_validate(p);
    fa::fwd_set_last_plan_text(nullptr);
    if (st != FA_OK) return st;
    const Fp8CachePlan pl = plan_kv8(p);
    if (pl.grid.status != FA_OK) return pl.grid.status;
    char name[160];
    fa::fwd_set_last_plan_text(plan_text(pl, name));
    if (pl.nothing || pl.grid.pblocks == 0) return FA_OK;  // nothing to compute: the caller owns the outputs of an empty problem

    fa::PkParams pa{};
    fa::fill_fp8_cache(p, pl, p->d, pa.p);
    pa.num_pblocks = (int32_t)pl.grid.pblocks;
    pa.num_groups = (int32_t)pl.grid.groups;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int st_main = p->dtype == FA_DTYPE_BF16 ? launch<__bf16>(pl, pa, stream) : launch<_Float16>(pl, pa, stream);
    return fa::merge_fp8_cache(p, pa.p, st_main, stream_);
}

}  // extern "C"
