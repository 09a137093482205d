// fa_bwd_api.hip — C-ABI entry points declared in include/fa_bwd.h.
//
// Host-side role of mha_bwd / mha_varlen_bwd (csrc/flash_attn/flash_api.cpp:767-971, 973-1200),
// set_params_dgrad (:161-221) and run_mha_bwd (:757-765): validate, fill the kernel params, launch the three
// kernels on the caller's stream.  No allocation, no synchronisation.
#include "fa_bwd.h"
#include "fa_bwd_internal.h"
#include "fa_bwd_kernel.h"
#include "fa_fwd_internal.h"
#include "fa_launch.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace fa {

// ---- dsink[h] = - sum over the valid rows of exp(z_h - LSE) * D (include/fa_bwd.h).  One workgroup per head.  Memory-bound:
// two fp32 streams, read once; the threads of a workgroup walk one sequence's rows side by side (consecutive lanes,
// consecutive addresses: whole cache lines per wavefront), sequence after sequence.  Every thread adds its rows in a fixed
// order, then a butterfly inside each wavefront and a serial sum of the four wavefront totals: no atomics, the same bits on
// every run.
__global__ __launch_bounds__(256) void sink_grad_kernel(const fa_sink_grad_params p) {
    __shared__ float wave_sum[4];
    const int head = blockIdx.x, tid = threadIdx.x;
    const float z = p.sink_dtype == FA_DTYPE_FP32
                        ? ((const float *)p.learnable_sink)[head]
                        : __uint_as_float((uint32_t)((const uint16_t *)p.learnable_sink)[head] << 16);
    float acc = 0.f;
    if (z != -INFINITY) {  // (no sink: its weight is 0 everywhere)
        for (int bb = 0; bb < p.b; ++bb) {
            int len;
            int64_t lse_off, d_off;
            if (p.cu_seqlens_q) {
                const int q0 = p.cu_seqlens_q[bb];
                len = min(p.cu_seqlens_q[bb + 1], p.total_q) - q0;
                lse_off = (int64_t)head * p.total_q + q0;
                d_off = (int64_t)head * p.softmax_d_row_len + q0;
            } else {
                len = p.seqlen_q;
                lse_off = ((int64_t)bb * p.h + head) * p.seqlen_q;
                d_off = ((int64_t)bb * p.h + head) * p.softmax_d_row_len;
            }
            if (p.seqused_q) len = min(len, p.seqused_q[bb]);
            for (int r = tid; r < len; r += 256) acc += __expf(z - p.softmax_lse[lse_off + r]) * p.softmax_d[d_off + r];
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) p.dsink[head] = -(((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3]);
}

}  // namespace fa

namespace {

int head_dim_tile_b(int d) {
    if (d <= 64) return 64;
    if (d <= 128) return 128;
    return 256;
}

// ---- backward routing ---------------------------------------------------------------------------------------------------
// plan_bwd() is the one place that decides which instantiation of each of the three kernels a problem runs.  Host code without
// HIP calls: fa_bwd launches from the plan, fa_bwd_plan_name / fa_bwd_last_plan_name (the test hooks, tests/test_bwd_plan.py)
// print the same plan.
//
// 32-wide blocks per wave (NB; every LDS fragment feeds NB MFMAs): two wherever accumulators + resident operands fit
// the 512-register budget of a lone wave.  dQ: 2 for D <= 128; dK/dV (two accumulator sets + K and V): 2 for D = 64
// (at D = 128 two blocks would fill all 256 AGPRs with accumulators; hipcc then rotates the whole AGPR file
//  through v_accvgpr_mov to find temporaries -- measured 3x slower and not worth fighting).
//  At D = 64 the plain problem -- no softcap / dropout / ALiBi -- takes the one-block form as well: that is the shape of the
//  generated tile loop, tools/gen_bwd_loop.py.
// DEFF (plain problems only): head dims <= 96 on the 128-wide tiles and <= 160 / <= 192 on the 256-wide ones run the
// instantiations that skip the zero padding.  Head-dim tile 256: dV and dK by a launch each (PART 1 / 2, fa_bwd_kernel.h) -- one
// accumulator set per sweep.
struct BwdPlan {
    int32_t dtype;          // FA_DTYPE_FP16 / FA_DTYPE_BF16
    int tile;               // head-dim tile D: 64 / 128 / 256
    bool softcap, dropout;
    int lpr;                // bwd_dot_kernel: lanes per (row, head)
    int nbk, deffk;         // bwd_dkdv_kernel
    bool two_parts;         //   PART 1 (dV) then PART 2 (dK) instead of one sweep
    int nbq, deffq;         // bwd_dq_kernel
    bool run_dot, run_dkdv, run_dq;  // a launch without work items is left out
};

BwdPlan plan_bwd(const fa_bwd_params *p) {
    BwdPlan pl{};
    const int d_v = p->d_v > 0 ? p->d_v : p->d, w = std::max(p->d, d_v);
    pl.dtype = p->dtype;
    pl.tile = head_dim_tile_b(w);
    pl.softcap = p->softcap > 0.f;
    pl.dropout = p->p_dropout > 0.f;  // (never together with softcap: fa_bwd_validate)
    const bool plain = !pl.softcap && !pl.dropout;
    pl.lpr = std::min(pl.tile / 8, 32);
    pl.nbk = pl.tile == 64 && !(plain && !p->alibi_slopes) ? 2 : 1;
    pl.nbq = pl.tile <= 128 ? 2 : 1;
    int deff = pl.tile;
    if (plain && pl.tile == 128 && p->d <= 96) deff = 96;
    if (plain && pl.tile == 256) deff = w <= 160 ? 160 : w <= 192 ? 192 : 256;
    pl.deffk = pl.deffq = deff;
    pl.two_parts = pl.tile == 256;
    const int64_t rows_q = p->cu_seqlens_q ? (int64_t)p->total_q : (int64_t)p->b * p->seqlen_q;
    const bool no_q = (p->seqlen_q == 0) || (p->cu_seqlens_q && p->total_q == 0);
    const bool no_k = (p->seqlen_k == 0) || (p->cu_seqlens_q && p->total_k == 0);
    const bool any = !(no_q && no_k);   // (nothing to do: fa_bwd returns before the first launch)
    pl.run_dot = any && rows_q > 0;
    pl.run_dkdv = any && p->seqlen_k > 0;  // seqlen_q == 0: dK = dV = 0 is written by the dK/dV pass
    pl.run_dq = any && p->seqlen_q > 0;    // seqlen_k == 0: dQ = 0 likewise
    return pl;
}

// the text of a plan: one segment per launched kernel, in launch order
const char *plan_text(const BwdPlan &pl, char (&name)[320]) {
    int n = 0;
    name[0] = 0;
    auto seg = [&](const char *kernel, int nb, int deff, int part) {
        n += snprintf(name + n, sizeof(name) - n, "%s%s D=%d NB=%d DEFF=%d", n ? " | " : "", kernel, pl.tile, nb, deff);
        if (part) n += snprintf(name + n, sizeof(name) - n, " PART=%d", part);
        n += snprintf(name + n, sizeof(name) - n, "%s%s", pl.softcap ? " SOFTCAP" : "", pl.dropout ? " DROPOUT" : "");
    };
    if (pl.run_dot) n += snprintf(name + n, sizeof(name) - n, "bwd_dot LPR=%d", pl.lpr);
    if (pl.run_dkdv) {
        seg("bwd_dkdv", pl.nbk, pl.deffk, pl.two_parts ? 1 : 0);
        if (pl.two_parts) seg("bwd_dkdv", pl.nbk, pl.deffk, 2);
    }
    if (pl.run_dq) seg("bwd_dq", pl.nbq, pl.deffq, 0);
    return name;
}

// the plan the calling thread's most recent fa_bwd launched (fa_bwd_last_plan_name) ...
thread_local BwdPlan t_last_plan;
thread_local bool t_last_plan_set = false;
// ... or, when that call was fa_bwd_block_sparse, the text it left (fa::bwd_set_last_plan_text; empty = it was not)
thread_local char t_last_text[320] = "";

template <typename T, int D, bool SOFTCAP, bool DROPOUT = false>
int run_bwd(const BwdPlan &pl, fa::BParams bp, int rows_q_max, int rows_k_max, hipStream_t stream) {
    constexpr int NBQ = D <= 128 ? 2 : 1;
    constexpr int NBK2 = D <= 64 ? 2 : 1;
    constexpr int LPR = D / 8 > 32 ? 32 : D / 8;
    // what this instantiation can launch; a plan outside it is a routing bug, never another kernel
    if (pl.tile != D || pl.softcap != SOFTCAP || pl.dropout != DROPOUT || pl.lpr != LPR || pl.nbq != NBQ ||
        (pl.nbk != 1 && pl.nbk != NBK2) || pl.two_parts != (D == 256))
        return FA_ERR_UNSUPPORTED;
    int st;
    // 1. D = rowsum(dO * O)
    if (pl.run_dot && (st = fa::bwd_launch_dot(bp, pl.dtype, D, stream)) != FA_OK) return st;
    // 2. dK, dV
    if (pl.run_dkdv) {
        if ((st = fa::bwd_set_grid(bp, (rows_k_max + 128 * pl.nbk - 1) / (128 * pl.nbk), bp.h_k)) != FA_OK) return st;
        if constexpr (D == 128 && !SOFTCAP && !DROPOUT) {
            st = pl.deffk == 96 ? fa::launch_kernel<fa::bwd_dkdv_kernel<T, D, 1, false, false, 96>>(fa::smem_bytes_dkdv<D>(), bp.grid, 256, stream, bp)
               : pl.deffk == D  ? fa::launch_kernel<fa::bwd_dkdv_kernel<T, D, 1, false, false>>(fa::smem_bytes_dkdv<D>(), bp.grid, 256, stream, bp)
                                : FA_ERR_UNSUPPORTED;
        } else if constexpr (D == 256) {
            auto two = [&](auto deff_c) {
                constexpr int DEFF = decltype(deff_c)::value;
                int s2 = fa::launch_kernel<fa::bwd_dkdv_kernel<T, D, 1, SOFTCAP, DROPOUT, DEFF, 1>>(fa::smem_bytes_dkdv<D>(), bp.grid, 256, stream, bp);
                if (s2 == FA_OK)
                    s2 = fa::launch_kernel<fa::bwd_dkdv_kernel<T, D, 1, SOFTCAP, DROPOUT, DEFF, 2>>(fa::smem_bytes_dkdv<D>(), bp.grid, 256, stream, bp);
                return s2;
            };
            if constexpr (!SOFTCAP && !DROPOUT) {
                st = pl.deffk == 160 ? two(std::integral_constant<int, 160>{})
                   : pl.deffk == 192 ? two(std::integral_constant<int, 192>{})
                   : pl.deffk == D   ? two(std::integral_constant<int, 256>{})
                                     : FA_ERR_UNSUPPORTED;
            } else {
                st = pl.deffk == D ? two(std::integral_constant<int, 256>{}) : FA_ERR_UNSUPPORTED;
            }
        } else {
            st = pl.deffk != D ? FA_ERR_UNSUPPORTED
               : pl.nbk == 1   ? fa::launch_kernel<fa::bwd_dkdv_kernel<T, D, 1, SOFTCAP, DROPOUT>>(fa::smem_bytes_dkdv<D>(), bp.grid, 256, stream, bp)
                               : fa::launch_kernel<fa::bwd_dkdv_kernel<T, D, NBK2, SOFTCAP, DROPOUT>>(fa::smem_bytes_dkdv<D>(), bp.grid, 256, stream, bp);
        }
        if (st != FA_OK) return st;
    }
    // 3. dQ
    if (pl.run_dq) {
        if ((st = fa::bwd_set_grid(bp, (rows_q_max + 128 * NBQ - 1) / (128 * NBQ), bp.h)) != FA_OK) return st;
        if constexpr (D == 128 && !SOFTCAP && !DROPOUT) {
            st = pl.deffq == 96 ? fa::launch_kernel<fa::bwd_dq_kernel<T, D, NBQ, false, false, 96>>(fa::smem_bytes_dq<D>(), bp.grid, 256, stream, bp)
               : pl.deffq == D  ? fa::launch_kernel<fa::bwd_dq_kernel<T, D, NBQ, false, false>>(fa::smem_bytes_dq<D>(), bp.grid, 256, stream, bp)
                                : FA_ERR_UNSUPPORTED;
        } else if constexpr (D == 256 && !SOFTCAP && !DROPOUT) {
            st = pl.deffq == 160 ? fa::launch_kernel<fa::bwd_dq_kernel<T, D, NBQ, false, false, 160>>(fa::smem_bytes_dq<D>(), bp.grid, 256, stream, bp)
               : pl.deffq == 192 ? fa::launch_kernel<fa::bwd_dq_kernel<T, D, NBQ, false, false, 192>>(fa::smem_bytes_dq<D>(), bp.grid, 256, stream, bp)
               : pl.deffq == D   ? fa::launch_kernel<fa::bwd_dq_kernel<T, D, NBQ, false, false>>(fa::smem_bytes_dq<D>(), bp.grid, 256, stream, bp)
                                 : FA_ERR_UNSUPPORTED;
        } else {
            st = pl.deffq == D ? fa::launch_kernel<fa::bwd_dq_kernel<T, D, NBQ, SOFTCAP, DROPOUT>>(fa::smem_bytes_dq<D>(), bp.grid, 256, stream, bp)
                               : FA_ERR_UNSUPPORTED;
        }
        if (st != FA_OK) return st;
    }
    return FA_OK;
}

template <typename T>
int dispatch_bwd(const BwdPlan &pl, const fa::BParams &bp, int sq, int sk, hipStream_t stream) {
    switch (pl.tile) {
        case 64:
            if (pl.dropout) return run_bwd<T, 64, false, true>(pl, bp, sq, sk, stream);
            return pl.softcap ? run_bwd<T, 64, true>(pl, bp, sq, sk, stream) : run_bwd<T, 64, false>(pl, bp, sq, sk, stream);
        case 128:
            if (pl.dropout) return run_bwd<T, 128, false, true>(pl, bp, sq, sk, stream);
            return pl.softcap ? run_bwd<T, 128, true>(pl, bp, sq, sk, stream) : run_bwd<T, 128, false>(pl, bp, sq, sk, stream);
        default:
            if (pl.dropout) return run_bwd<T, 256, false, true>(pl, bp, sq, sk, stream);
            return pl.softcap ? run_bwd<T, 256, true>(pl, bp, sq, sk, stream) : run_bwd<T, 256, false>(pl, bp, sq, sk, stream);
    }
}

}  // namespace

// ---- what fa_bwd_block_sparse (fa_bwd_bs_api.hip) shares with fa_bwd: fa_bwd_internal.h -----------------------------------
namespace fa {

void bwd_fill_params(const fa_bwd_params *p, BParams &bp) {
    bp.q = p->q; bp.k = p->k; bp.v = p->v; bp.o = p->o; bp.dout = p->dout; bp.lse = p->softmax_lse;
    bp.dq = p->dq; bp.dk = p->dk; bp.dv = p->dv; bp.dsum = p->softmax_d;
    bp.cu_seqlens_q = p->cu_seqlens_q; bp.cu_seqlens_k = p->cu_seqlens_k;
    bp.q_batch_stride = p->q_batch_stride; bp.q_row_stride = p->q_row_stride; bp.q_head_stride = p->q_head_stride;
    bp.k_batch_stride = p->k_batch_stride; bp.k_row_stride = p->k_row_stride; bp.k_head_stride = p->k_head_stride;
    bp.v_batch_stride = p->v_batch_stride; bp.v_row_stride = p->v_row_stride; bp.v_head_stride = p->v_head_stride;
    bp.o_batch_stride = p->o_batch_stride; bp.o_row_stride = p->o_row_stride; bp.o_head_stride = p->o_head_stride;
    bp.do_batch_stride = p->do_batch_stride; bp.do_row_stride = p->do_row_stride; bp.do_head_stride = p->do_head_stride;
    bp.dq_batch_stride = p->dq_batch_stride; bp.dq_row_stride = p->dq_row_stride; bp.dq_head_stride = p->dq_head_stride;
    bp.dk_batch_stride = p->dk_batch_stride; bp.dk_row_stride = p->dk_row_stride; bp.dk_head_stride = p->dk_head_stride;
    bp.dv_batch_stride = p->dv_batch_stride; bp.dv_row_stride = p->dv_row_stride; bp.dv_head_stride = p->dv_head_stride;
    bp.dsum_row_len = p->softmax_d_row_len;
    bp.b = p->b; bp.seqlen_q = p->seqlen_q; bp.seqlen_k = p->seqlen_k; bp.h = p->h; bp.h_k = p->h_k; bp.d = p->d;
    bp.d_v = (p->d_v > 0) ? p->d_v : p->d;
    bp.total_q = p->total_q;
    bp.h_ratio = p->h / p->h_k;

    // the forward's window rule and softmax scales (fa_fwd_internal.h; csrc/flash_attn/flash_api.cpp:790,836-837)
    bp.window_left = p->window_size_left;
    bp.window_right = p->window_size_right;
    normalise_window(p->is_causal, p->flags, p->seqlen_k, bp.window_left, bp.window_right);
    const SoftmaxScales sc = softmax_scales(p->softmax_scale, p->softcap);
    bp.softcap_pre = sc.softcap_pre;
    bp.scale_log2 = sc.scale_log2;
    bp.out_scale = p->softmax_scale;
    bp.alibi = p->alibi_slopes;
    bp.alibi_bs = (int32_t)p->alibi_slopes_batch_stride;
    bp.drop_thr = p->p_dropout > 0.f ? (int)std::floor(255.0 * (1.0 - (double)p->p_dropout)) : 255;  // as fa_fwd
    bp.rp_dropout = p->p_dropout > 0.f ? 1.f / (1.f - p->p_dropout) : 1.f;
    bp.rng_state = p->rng_state;
}

int bwd_launch_dot(const BParams &bp, int32_t dtype, int tile, hipStream_t stream) {
    const int64_t rows = bp.cu_seqlens_q ? (int64_t)bp.total_q : (int64_t)bp.b * bp.seqlen_q;
    const int64_t items = rows * bp.h;
    const int lpr = std::min(tile / 8, 32), per_block = 256 / lpr;
    const int grid = (int)std::min<int64_t>((items + per_block - 1) / per_block, 256 * 16);
    const bool bf16 = dtype == FA_DTYPE_BF16;
    if (lpr == 8) {
        if (bf16) hipLaunchKernelGGL((bwd_dot_kernel<__bf16, 8>), dim3(grid), dim3(256), 0, stream, bp);
        else hipLaunchKernelGGL((bwd_dot_kernel<_Float16, 8>), dim3(grid), dim3(256), 0, stream, bp);
    } else if (lpr == 16) {
        if (bf16) hipLaunchKernelGGL((bwd_dot_kernel<__bf16, 16>), dim3(grid), dim3(256), 0, stream, bp);
        else hipLaunchKernelGGL((bwd_dot_kernel<_Float16, 16>), dim3(grid), dim3(256), 0, stream, bp);
    } else {
        if (bf16) hipLaunchKernelGGL((bwd_dot_kernel<__bf16, 32>), dim3(grid), dim3(256), 0, stream, bp);
        else hipLaunchKernelGGL((bwd_dot_kernel<_Float16, 32>), dim3(grid), dim3(256), 0, stream, bp);
    }
    return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

// grid of decode_block(): whole units of `blocks` workgroups for as many (batch, head) units as deal evenly over the 8 XCDs,
// the remaining heads block by block (any head count loads the XCDs equally; fewer than 16 units: everything block by block)
int bwd_set_grid(BParams &bp, int64_t blocks, int64_t heads) {
    const int64_t tiles = blocks * heads * bp.b;
    if (tiles > 0x7fffffff) return FA_ERR_BAD_SHAPE;
    bp.num_blocks = (int32_t)blocks;
    bp.num_tiles = (int32_t)tiles;
    const int64_t units = tiles / blocks;
    const int64_t ws = units >= 16 ? units / 8 * blocks : 0;
    const int64_t grid = 8 * (ws + (tiles - ws * 8 + 7) / 8);
    if (grid > 0x7fffffff) return FA_ERR_BAD_SHAPE;
    bp.whole_slots = (int32_t)ws;
    bp.grid = (int32_t)grid;
    return FA_OK;
}

void bwd_set_last_plan_text(const char *text) {
    t_last_plan_set = false;
    snprintf(t_last_text, sizeof(t_last_text), "%s", text ? text : "");
}

}  // namespace fa

extern "C" {

uint32_t fa_bwd_params_size(void) { return (uint32_t)sizeof(fa_bwd_params); }

int fa_bwd_validate(const fa_bwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_bwd_params)) return FA_ERR_BAD_ABI;
    if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16) return FA_ERR_BAD_DTYPE;
    if (!(p->p_dropout >= 0.f && p->p_dropout < 1.f)) return FA_ERR_BAD_SHAPE;
    if (p->p_dropout > 0.f && (!p->rng_state || reinterpret_cast<uintptr_t>(p->rng_state) % 8 != 0)) return FA_ERR_NULL_POINTER;
    if (p->p_dropout > 0.f && p->softcap > 0.f) return FA_ERR_UNSUPPORTED;  // "Softcapping does not support dropout for now"
    if (p->b <= 0 || p->h <= 0 || p->h_k <= 0 || p->seqlen_q < 0 || p->seqlen_k < 0) return FA_ERR_BAD_SHAPE;
    if (p->d <= 0 || p->d > 256 || p->d % 8 != 0) return FA_ERR_BAD_HEAD_DIM;
    if (p->d_v < 0 || p->d_v % 8 != 0) return FA_ERR_BAD_HEAD_DIM;
    if (p->d_v > 0 && p->d_v != p->d && (p->d_v > 256 || std::max(p->d, p->d_v) <= 128)) return FA_ERR_UNSUPPORTED;  // wide tile only
    if (p->h % p->h_k != 0) return FA_ERR_BAD_HEADS;
    if ((p->cu_seqlens_q == nullptr) != (p->cu_seqlens_k == nullptr)) return FA_ERR_BAD_SHAPE;
    if (p->cu_seqlens_q && (p->total_q < 0 || p->total_k < 0)) return FA_ERR_BAD_SHAPE;
    const bool no_q = (p->seqlen_q == 0) || (p->cu_seqlens_q && p->total_q == 0);
    const bool no_k = (p->seqlen_k == 0) || (p->cu_seqlens_q && p->total_k == 0);
    if (!no_q && (!p->q || !p->o || !p->dout || !p->softmax_lse || !p->dq || !p->softmax_d)) return FA_ERR_NULL_POINTER;
    if (!no_k && (!p->k || !p->v || !p->dk || !p->dv)) return FA_ERR_NULL_POINTER;
    const int64_t strides[] = {p->q_row_stride, p->q_head_stride, p->k_row_stride, p->k_head_stride, p->v_row_stride,
                               p->v_head_stride, p->o_row_stride, p->o_head_stride, p->do_row_stride, p->do_head_stride,
                               p->dq_row_stride, p->dq_head_stride, p->dk_row_stride, p->dk_head_stride,
                               p->dv_row_stride, p->dv_head_stride};
    for (int64_t s : strides)
        if (s % 8 != 0) return FA_ERR_BAD_STRIDE;
    if (!p->cu_seqlens_q) {
        const int64_t bs[] = {p->q_batch_stride, p->k_batch_stride, p->v_batch_stride, p->o_batch_stride,
                              p->do_batch_stride, p->dq_batch_stride, p->dk_batch_stride, p->dv_batch_stride};
        for (int64_t s : bs)
            if (s % 8 != 0) return FA_ERR_BAD_STRIDE;
    }
    // tiles are addressed as 64-bit tile base + 32-bit (row * stride) lane offset
    if (p->q_row_stride < 0 || p->do_row_stride < 0 || p->q_row_stride >= (1 << 24) || p->do_row_stride >= (1 << 24) ||
        p->k_row_stride < 0 || p->v_row_stride < 0 || p->k_row_stride >= (1 << 24) || p->v_row_stride >= (1 << 24))
        return FA_ERR_BAD_STRIDE;
    const void *ptrs[] = {p->q, p->k, p->v, p->o, p->dout, p->dq, p->dk, p->dv};
    for (const void *ptr : ptrs)
        if (reinterpret_cast<uintptr_t>(ptr) % 16 != 0) return FA_ERR_BAD_STRIDE;
    const int64_t need = p->cu_seqlens_q ? (int64_t)p->total_q : (int64_t)p->seqlen_q;
    if (p->softmax_d_row_len < need) return FA_ERR_BAD_SHAPE;
    if (p->softcap < 0.f || std::isnan(p->softcap) || std::isnan(p->softmax_scale)) return FA_ERR_BAD_SHAPE;
    if (p->alibi_slopes && (reinterpret_cast<uintptr_t>(p->alibi_slopes) % 4 != 0 || p->alibi_slopes_batch_stride < 0 ||
                            p->alibi_slopes_batch_stride > 0x7fffffff))
        return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

const char *fa_bwd_plan_name(const fa_bwd_params *p) {
    if (fa_bwd_validate(p) != FA_OK) return nullptr;
    thread_local char name[320];
    return plan_text(plan_bwd(p), name);
}

const char *fa_bwd_last_plan_name(void) {
    thread_local char name[320];
    if (t_last_text[0]) return t_last_text;
    return t_last_plan_set ? plan_text(t_last_plan, name) : nullptr;
}

int fa_bwd(const fa_bwd_params *p, void *stream_) {
    const int st = fa_bwd_validate(p);
    t_last_plan_set = false;
    t_last_text[0] = 0;
    if (st != FA_OK) return st;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const BwdPlan pl = plan_bwd(p);
    t_last_plan = pl;
    t_last_plan_set = true;
    if (!pl.run_dot && !pl.run_dkdv && !pl.run_dq) return FA_OK;  // no queries and no keys

    fa::BParams bp{};
    fa::bwd_fill_params(p, bp);

    // seqlen_q == 0: dK = dV = 0 is written by the dK/dV pass (no query tile is visible); seqlen_k == 0: dQ = 0 likewise
    if (pl.dtype == FA_DTYPE_BF16) return dispatch_bwd<__bf16>(pl, bp, p->seqlen_q, p->seqlen_k, stream);
    return dispatch_bwd<_Float16>(pl, bp, p->seqlen_q, p->seqlen_k, stream);
}

uint32_t fa_sink_grad_params_size(void) { return (uint32_t)sizeof(fa_sink_grad_params); }

int fa_sink_grad_validate(const fa_sink_grad_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_sink_grad_params)) return FA_ERR_BAD_ABI;
    if (p->sink_dtype != FA_DTYPE_BF16 && p->sink_dtype != FA_DTYPE_FP32) return FA_ERR_BAD_DTYPE;
    if (p->b <= 0 || p->h <= 0 || p->seqlen_q < 0) return FA_ERR_BAD_SHAPE;
    if (p->cu_seqlens_q && p->total_q < 0) return FA_ERR_BAD_SHAPE;
    if (!p->learnable_sink || !p->dsink) return FA_ERR_NULL_POINTER;
    const int64_t rows = p->cu_seqlens_q ? (int64_t)p->total_q : (int64_t)p->seqlen_q;
    if (rows > 0 && (!p->softmax_lse || !p->softmax_d)) return FA_ERR_NULL_POINTER;
    if (p->softmax_d_row_len < rows) return FA_ERR_BAD_SHAPE;
    if (reinterpret_cast<uintptr_t>(p->learnable_sink) % (p->sink_dtype == FA_DTYPE_FP32 ? 4 : 2) != 0 ||
        reinterpret_cast<uintptr_t>(p->dsink) % 4 != 0 || reinterpret_cast<uintptr_t>(p->softmax_lse) % 4 != 0 ||
        reinterpret_cast<uintptr_t>(p->softmax_d) % 4 != 0)
        return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int fa_sink_grad(const fa_sink_grad_params *p, void *stream_) {
    const int st = fa_sink_grad_validate(p);
    if (st != FA_OK) return st;
    hipLaunchKernelGGL(fa::sink_grad_kernel, dim3((unsigned)p->h), dim3(256), 0, static_cast<hipStream_t>(stream_), *p);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

}  // extern "C"
