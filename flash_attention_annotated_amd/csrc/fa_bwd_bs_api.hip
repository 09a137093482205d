// fa_bwd_bs_api.hip — fa_bwd_block_sparse (include/fa_bwd.h): validation, the D pass through fa_bwd_api.hip's bwd_dot_kernel
// (fa_bwd_internal.h), and the two list-driven kernels of fa_bwd_kernel_bs.h.  A translation unit of its own: the device code
// of fa_bwd_api.hip stays exactly the kernels tests/test_bwd_plan.py counts.  No allocation, no synchronisation, nothing of
// the lists is read on the host.
#include "fa_bwd.h"
#include "fa_bwd_internal.h"
#include "fa_bwd_kernel_bs.h"
#include "fa_launch.h"

#include <cstdio>

namespace {

template <typename T, int D>
int launch_bs_bwd(bool softcap, bool dkdv, const fa::BsBwdParams &bp, hipStream_t stream) {
    if (dkdv)
        return softcap ? fa::launch_kernel<fa::bs_bwd_dkdv_kernel<T, D, true>>(fa::smem_bytes_bs_dkdv<D>(), bp.p.grid, 256, stream, bp)
                       : fa::launch_kernel<fa::bs_bwd_dkdv_kernel<T, D, false>>(fa::smem_bytes_bs_dkdv<D>(), bp.p.grid, 256, stream, bp);
    return softcap ? fa::launch_kernel<fa::bs_bwd_dq_kernel<T, D, true>>(fa::smem_bytes_bs_dq<D>(), bp.p.grid, 256, stream, bp)
                   : fa::launch_kernel<fa::bs_bwd_dq_kernel<T, D, false>>(fa::smem_bytes_bs_dq<D>(), bp.p.grid, 256, stream, bp);
}

}  // namespace

extern "C" {

uint32_t fa_block_sparse_bwd_params_size(void) { return (uint32_t)sizeof(fa_block_sparse_bwd_params); }

// The refusals come first: what the block-sparse backward cannot go with is refused as such, whatever else the params lack.
int fa_bwd_block_sparse_validate(const fa_bwd_params *p, const fa_block_sparse_params *s, const fa_block_sparse_bwd_params *kl) {
    if (!p || !s || !kl) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_bwd_params)) return FA_ERR_BAD_ABI;
    if (s->abi_version != FA_ABI_VERSION || s->struct_size != sizeof(fa_block_sparse_params)) return FA_ERR_BAD_ABI;
    if (kl->abi_version != FA_ABI_VERSION || kl->struct_size != sizeof(fa_block_sparse_bwd_params)) return FA_ERR_BAD_ABI;
    if (s->block_m != fa::BS_BLOCK || s->block_n != fa::BS_BLOCK || kl->block_m != fa::BS_BLOCK || kl->block_n != fa::BS_BLOCK)
        return FA_ERR_UNSUPPORTED;
    if (p->cu_seqlens_q || p->cu_seqlens_k || p->alibi_slopes || p->p_dropout > 0.f || p->d > 128 || (p->d_v > 0 && p->d_v != p->d))
        return FA_ERR_UNSUPPORTED;
    if (!s->mask_block_cnt || !s->mask_block_idx || !kl->q_block_cnt || !kl->q_block_idx) return FA_ERR_NULL_POINTER;
    if ((s->full_block_cnt == nullptr) != (s->full_block_idx == nullptr)) return FA_ERR_NULL_POINTER;
    const void *lists[] = {s->full_block_cnt, s->full_block_idx, s->mask_block_cnt, s->mask_block_idx, kl->q_block_cnt, kl->q_block_idx};
    for (const void *l : lists)
        if (reinterpret_cast<uintptr_t>(l) % 4 != 0) return FA_ERR_BAD_STRIDE;
    const int64_t *strides[] = {s->full_cnt_stride, s->full_idx_stride, s->mask_cnt_stride, s->mask_idx_stride, kl->q_cnt_stride,
                                kl->q_idx_stride};
    for (const int64_t *st : strides)
        for (int i = 0; i < 4; ++i)
            if (st[i] < 0) return FA_ERR_BAD_STRIDE;
    return fa_bwd_validate(p);
}

int fa_bwd_block_sparse(const fa_bwd_params *p, const fa_block_sparse_params *s, const fa_block_sparse_bwd_params *kl, void *stream_) {
    const int st = fa_bwd_block_sparse_validate(p, s, kl);
    fa::bwd_set_last_plan_text(nullptr);
    if (st != FA_OK) return st;
    hipStream_t stream = static_cast<hipStream_t>(stream_);

    fa::BsBwdParams bp{};
    fa::bwd_fill_params(p, bp.p);
    auto list = [](const int32_t *cnt, const int32_t *idx, const int64_t *cs, const int64_t *is) {
        return fa::BsList{cnt, idx, cs[0], cs[1], cs[2], is[0], is[1], is[2], is[3]};
    };
    bp.full = list(s->full_block_cnt, s->full_block_idx, s->full_cnt_stride, s->full_idx_stride);
    bp.mask = list(s->mask_block_cnt, s->mask_block_idx, s->mask_cnt_stride, s->mask_idx_stride);
    bp.keyq = list(kl->q_block_cnt, kl->q_block_idx, kl->q_cnt_stride, kl->q_idx_stride);
    const int64_t nm = ((int64_t)p->seqlen_q + fa::BS_BLOCK - 1) / fa::BS_BLOCK, nk = ((int64_t)p->seqlen_k + fa::BS_BLOCK - 1) / fa::BS_BLOCK;
    bp.nm = (int32_t)nm;
    bp.nk = (int32_t)nk;

    const int tile = p->d <= 64 ? 64 : 128;
    const bool softcap = p->softcap > 0.f;
    // a launch without work items is left out: no query rows -- D and dQ; no keys -- dK / dV (seqlen_q == 0 with keys: the
    // dK / dV pass writes zeros, every count clamps to nm = 0)
    const bool run_dot = nm > 0, run_dkdv = nk > 0, run_dq = nm > 0;
    char text[320];
    int n = 0;
    text[0] = 0;
    if (run_dot) n += snprintf(text + n, sizeof(text) - n, "bwd_dot LPR=%d", tile / 8);
    if (run_dkdv) n += snprintf(text + n, sizeof(text) - n, "%sbs_bwd_dkdv D=%d%s", n ? " | " : "", tile, softcap ? " SOFTCAP" : "");
    if (run_dq) n += snprintf(text + n, sizeof(text) - n, "%sbs_bwd_dq D=%d%s", n ? " | " : "", tile, softcap ? " SOFTCAP" : "");
    fa::bwd_set_last_plan_text(text);

    const bool bf16 = p->dtype == FA_DTYPE_BF16;
    auto launch = [&](bool dkdv) {
        if (tile == 64) return bf16 ? launch_bs_bwd<__bf16, 64>(softcap, dkdv, bp, stream) : launch_bs_bwd<_Float16, 64>(softcap, dkdv, bp, stream);
        return bf16 ? launch_bs_bwd<__bf16, 128>(softcap, dkdv, bp, stream) : launch_bs_bwd<_Float16, 128>(softcap, dkdv, bp, stream);
    };
    int rc;
    if (run_dot && (rc = fa::bwd_launch_dot(bp.p, p->dtype, tile, stream)) != FA_OK) return rc;
    if (run_dkdv) {
        if ((rc = fa::bwd_set_grid(bp.p, nk, p->h_k)) != FA_OK || (rc = launch(true)) != FA_OK) return rc;
    }
    if (run_dq) {
        if ((rc = fa::bwd_set_grid(bp.p, nm, p->h)) != FA_OK || (rc = launch(false)) != FA_OK) return rc;
    }
    return FA_OK;
}

}  // extern "C"
