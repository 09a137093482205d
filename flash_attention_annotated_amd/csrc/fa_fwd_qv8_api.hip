// fa_fwd_qv8_api.hip — C-ABI of the MLA decode shape over an fp8 (e4m3) KV cache with 16-bit q / qv / o (include/fa_fwd.h:
// fa_fwd_qv8, fa_fwd_qv8_validate, fa_fwd_qv8_workspace_size, fa_fwd_qv8_plan_name).  A translation unit of its own: the
// kernels of fa_fwd_api.hip and fa_fwd_kv8_api.hip are pinned sets.  Here: the route's shape rules, plan text and launch
// ladder.  The plan, the rest of the validation, the params fill and the merge (the public fa_fwd_combine) are fa_fwd_kv8's
// too: fa_fwd_internal.h.
#include "fa_fwd.h"
#include "fa_fwd_internal.h"
#include "fa_fwd_kernel_qv8.h"
#include "fa_launch.h"

#include <cstdio>

namespace {

using fa::Fp8CachePlan;

// fwd_kernel_qv's work shape (blocks of 32 packed rows) and split count, V tile DVT = 256 (d_v = 256) or 512 (d_v in (256, 512])
Fp8CachePlan plan_qv8(const fa_fwd_params *p) {
    return fa::plan_fp8_cache(p, p->d_v <= 256 ? 256 : 512, 32, p->d_v, fa::fwd_qv_split_count);
}

const char *plan_text(const Fp8CachePlan &pl, char (&name)[160]) {
    if (pl.grid.status != FA_OK) return nullptr;
    snprintf(name, sizeof(name), "qv8_fwd_kernel DVT=%d waves=%d%s block_m=32 splits=%d", pl.tile, fa::QV_NWAVES,
             pl.softcap ? " SOFTCAP" : "", pl.split.splits);
    return name;
}

template <typename T, int DVT>
int launch_form(const Fp8CachePlan &pl, const fa::QvParams &qa, hipStream_t stream) {
    constexpr int smem = fa::smem_bytes_qv8<DVT>(), NT = fa::QV_NWAVES * 64;
    return pl.softcap ? fa::launch_kernel<fa::qv8_fwd_kernel<T, DVT, true>>(smem, pl.grid.grid, NT, stream, qa)
                      : fa::launch_kernel<fa::qv8_fwd_kernel<T, DVT, false>>(smem, pl.grid.grid, NT, stream, qa);
}
template <typename T>
int launch(const Fp8CachePlan &pl, const fa::QvParams &qa, hipStream_t stream) {
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
    return shape != FA_OK ? shape : fa::validate_fp8_cache(p, plan_qv8);
}

int64_t fa_fwd_qv8_workspace_size(const fa_fwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_fwd_params)) return FA_ERR_BAD_ABI;
    const int shape = check_shape(p);
    return shape != FA_OK ? shape : plan_qv8(p).split.total;
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
    const Fp8CachePlan pl = plan_qv8(p);
    if (pl.grid.status != FA_OK) return pl.grid.status;
    char name[160];
    fa::fwd_set_last_plan_text(plan_text(pl, name));
    if (pl.nothing || pl.grid.pblocks == 0) return FA_OK;  // nothing to compute: the caller owns the outputs of an empty problem

    fa::QvParams qa{};
    fa::fill_fp8_cache(p, pl, p->d_v, qa.p);
    qa.qv = p->qv;
    qa.qv_batch_stride = p->qv_batch_stride; qa.qv_row_stride = p->qv_row_stride; qa.qv_head_stride = p->qv_head_stride;
    qa.num_pblocks = (int32_t)pl.grid.pblocks;
    qa.num_groups = (int32_t)pl.grid.groups;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int st_main = p->dtype == FA_DTYPE_BF16 ? launch<__bf16>(pl, qa, stream) : launch<_Float16>(pl, qa, stream);
    return fa::merge_fp8_cache(p, qa.p, st_main, stream_);
}

}  // extern "C"
