// fa_fwd_kernel_qv.h — gfx950 forward for small q/k head dims beside a wide V, with the FA3 `qv` score term.
//
// Role of the reference's has_qv mainloop (hopper/mainloop_fwd_sm90_tma_gmma_ws.hpp, hopper/flash_api.cpp:1028-1048): the
// score is  S = Q.K^T + Qv.V^T  with Q, K of width d <= 64 and Qv, V of width d_v in [256, 512] (DeepSeek-style MLA decode:
// K is the rope part, V the latent cache, read both as a key and as a value).  Without qv the same kernel serves d <= 64 /
// d_v >= 256 on paged caches and with split-KV, which the 256-column launches of the generic kernel cannot.
//
// Design (wave64, MFMA 32x32x16, 4 waves, one workgroup per CU):
//   * GQA is packed inside the kernel: a workgroup's 32 rows are (query row, head of the kv group) pairs, row
//     pr -> query row pr / g, head kv_head * g + pr % g (g = h / h_k).  All heads of one kv head share one pass over K/V;
//     masks use the query row.
//   * each 64-key tile stages K (64 columns) and V (DVT columns) in LDS once.  V is read from there twice: as the A operand
//     of the score product (ds_read_b128 along a V row) and as the A operand of O^T += V^T.P^T (ds_read_b64_tr_b16).
//   * the score contraction (d + d_v columns) is split over the waves: wave w takes Q k-step w and Qv / V columns
//     [w DVT/4, (w+1) DVT/4).  The four partial S^T tiles meet in LDS and every wave sums them in the same order, so all
//     waves hold bit-identical scores, softmax state and P -- no P or rescale factors need to travel.
//   * wave w accumulates O^T for its DVT/4 columns of all 32 rows: 4 (DVT 512) or 2 (DVT 256) f32x16 accumulators.
//   * the next tile's K/V rows are loaded into registers before the compute of the current one and written to LDS behind
//     it (single LDS buffer, barriers between the phases).
// Softcap, element mask, online softmax, P^T pack, the transposed PV product of a column block and the fp32 split-partial
// store are fa_fwd_tile_step.h's, shared with the pk / kv8 / bs kernels.  This file owns the rest: the work-item decode, the
// K + V staging of different widths, the per-wave partial score products (one K step, KSV steps along V rows: not scores_16's
// D / 16 steps over one tile) and their meeting in LDS behind a barrier of its own, the attention_chunk limits, and the
// epilogue that stores O rows straight from the accumulators.
#pragma once

#include "fa_fwd_tile_step.h"

namespace fa {

struct QvParams {
    KParams p;                 // p.d = q/k head dim (<= 64), p.dv = V / O head dim (<= DVT)
    const void *qv;            // (.., h, dv) rows beside q; NULL = no second score product
    int64_t qv_batch_stride, qv_row_stride, qv_head_stride;
    int32_t num_pblocks;       // 32-row blocks of packed rows per (batch, kv head): ceil(seqlen_q * g / 32)
    int32_t num_groups;        // b * h_k * splits: (batch, kv head, split) work groups
};

constexpr int QV_NWAVES = 4;

template <int DVT>
constexpr int smem_bytes_qv() {
    return BLOCK_N * 64 * 2 + BLOCK_N * DVT * 2 + QV_NWAVES * 32 * 64 * 4;  // K tile, V tile, partial scores
}

template <typename T, int DVT, bool SOFTCAP>
__global__ __launch_bounds__(QV_NWAVES * 64, 1) void fwd_kernel_qv(const QvParams qa) {
    const KParams &p = qa.p;
    constexpr int NT = QV_NWAVES * 64;
    constexpr int CPW = DVT / QV_NWAVES;       // V / O columns per wave
    constexpr int KSV = CPW / 16;              // Qv k-steps per wave
    constexpr int DBW = CPW / 32;              // O^T row blocks per wave
    constexpr int K_BYTES = BLOCK_N * 64 * 2;
    constexpr int V_BYTES = BLOCK_N * DVT * 2;
    constexpr int CHK = 64 / 8, CHV = DVT / 8;  // 16-byte chunks per K / V row
    constexpr int LDK = BLOCK_N * CHK / NT, LDV = BLOCK_N * CHV / NT;
    constexpr int RPK = NT / CHK, RPV = NT / CHV;  // rows per pass of the workgroup
    static_assert(KSV >= 1 && DBW >= 1 && LDK >= 1 && LDV >= 1, "tile shape");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *kbuf = smem;
    char *vbuf = smem + K_BYTES;
    char *sred = smem + K_BYTES + V_BYTES;  // [wave][8][64 lanes] float4

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int hh = lane >> 5;

    // ---- work item: groups of (batch, kv head, split) dealt round-robin over the 8 XCDs, the row blocks of one group on
    // one XCD (they stream the same K/V: L2 hits) -----------------------------------------------------------------------
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int group = (slot / qa.num_pblocks) * 8 + xcd, pb = slot % qa.num_pblocks;
    if (group >= qa.num_groups) return;  // whole workgroup (padding)
    const int splits = p.num_splits > 1 ? p.num_splits : 1;
    const int unit = group / splits, split = group % splits;
    const int batch = unit / p.h_k, kv_head = unit % p.h_k;
    const int g = p.h_ratio;

    int sq, sk, q0 = 0;
    int64_t k_base, v_base;
    if (p.cu_seqlens_q) {
        q0 = p.cu_seqlens_q[batch];
        sq = p.seqused_q ? p.seqused_q[batch] : p.cu_seqlens_q[batch + 1] - q0;
    } else {
        sq = p.seqused_q ? p.seqused_q[batch] : p.seqlen_q;
    }
    if (p.cu_seqlens_k) {
        const int k0 = p.cu_seqlens_k[batch];
        sk = p.seqused_k ? p.seqused_k[batch] : p.cu_seqlens_k[batch + 1] - k0;
        k_base = (int64_t)k0 * p.k_row_stride;
        v_base = (int64_t)k0 * p.v_row_stride;
    } else {
        sk = p.seqused_k ? p.seqused_k[batch] : p.seqlen_k;
        const int kv_batch = p.kv_batch_idx ? p.kv_batch_idx[batch] : batch;
        k_base = (int64_t)kv_batch * p.k_batch_stride;
        v_base = (int64_t)kv_batch * p.v_batch_stride;
    }
    const int prows = sq * g;  // packed rows of this (batch, kv head)
    const int pr_lo = pb * 32;
    if (pr_lo >= prows) return;  // whole workgroup
    if (p.leftpad_k) {
        const int lp = p.leftpad_k[batch];
        sk = max(sk - lp, 0);
        k_base += (int64_t)lp * p.k_row_stride;
        v_base += (int64_t)lp * p.v_row_stride;
    }
    if (p.block_table) k_base = v_base = 0;
    const int32_t *pages = p.block_table ? p.block_table + (int64_t)batch * p.bt_bs : nullptr;
    const T *kp = (const T *)p.k + k_base + (int64_t)kv_head * p.k_head_stride;
    const T *vp = (const T *)p.v + v_base + (int64_t)kv_head * p.v_head_stride;
    const Scales sc = load_scales(p, batch, kv_head);

    // ---- the lane's packed row, its query row and head ---------------------------------------------------------------
    const int pr = pr_lo + r;
    const bool row_ok = pr < prows;
    const int prc = min(pr, prows - 1);
    const int my_row = prc / g;                       // query row (masks)
    const int head = kv_head * g + prc % g;
    const int qr_lo = pr_lo / g, qr_hi = min(prows - 1, pr_lo + 31) / g;  // query rows of the block (inclusive)

    // ---- key range of the block -------------------------------------------------------------------------------------
    const int shift = sk - sq;
    int key_hi = sk, key_lo = 0;
    if (p.window_right >= 0) key_hi = min(sk, qr_hi + 1 + shift + p.window_right);
    if (p.window_left >= 0) key_lo = max(0, qr_lo + shift - p.window_left);
    if (p.chunk > 0) {
        key_lo = max(key_lo, chunk_floor(qr_lo + shift, p.chunk));
        key_hi = min(key_hi, chunk_floor(qr_hi + shift, p.chunk) + p.chunk);
    }
    int n_min = key_lo / BLOCK_N;
    int n_max = key_hi > 0 ? (key_hi + BLOCK_N - 1) / BLOCK_N : 0;
    split_range(p, split, n_min, n_max);

    // ---- Q / Qv fragments: B operands of S^T = K.Q^T + V.Qv^T; lane (r, hh) holds row r, columns 16 ks + 8 hh .. +8 ----
    const u32x4 z4 = {0, 0, 0, 0};
    u32x4 qf, qvf[KSV];
    {
        const int64_t row_q = p.cu_seqlens_q ? (int64_t)(q0 + my_row) : (int64_t)my_row;
        const int64_t bq = p.cu_seqlens_q ? 0 : batch;
        const T *qr = (const T *)p.q + bq * p.q_batch_stride + row_q * p.q_row_stride + (int64_t)head * p.q_head_stride;
        const int c = 16 * wave + 8 * hh;
        qf = *(const u32x4 *)(qr + (c < p.d ? c : 0));
        qf = (c < p.d && row_ok) ? qf : z4;
        const bool has_qv = qa.qv != nullptr;
        const T *qvr = has_qv ? (const T *)qa.qv + bq * qa.qv_batch_stride + row_q * qa.qv_row_stride +
                                    (int64_t)head * qa.qv_head_stride
                              : qr;
#pragma unroll
        for (int ks = 0; ks < KSV; ++ks) {
            const int cv = CPW * wave + 16 * ks + 8 * hh;
            qvf[ks] = *(const u32x4 *)(qvr + (has_qv && cv < p.dv ? cv : 0));
        }
#pragma unroll
        for (int ks = 0; ks < KSV; ++ks)
            qvf[ks] = (has_qv && CPW * wave + 16 * ks + 8 * hh < p.dv && row_ok) ? qvf[ks] : z4;
    }
    const bool has_qv = qa.qv != nullptr;

    f32x16 o_acc[DBW];
#pragma unroll
    for (int db = 0; db < DBW; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) o_acc[db][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    // ---- K/V staging (clamped rows / chunks as in fwd_kernel: duplicates are masked or meet zero Q columns) -----------
    u32x4 kreg[LDK], vreg[LDV];
    const int ldk_row0 = tid / CHK, ldv_row0 = tid / CHV;
    const int ldk_col = ((tid % CHK) * 8 < p.d) ? (tid % CHK) * 8 : 0;
    const int ldv_col = ((tid % CHV) * 8 < p.dv) ? (tid % CHV) * 8 : 0;
    const int k_rs = (int)p.k_row_stride, v_rs = (int)p.v_row_stride;  // host guarantees 64 * stride < 2^31
    auto load_tile = [&](int n) {
        const int k0 = n * BLOCK_N;
        const T *kt = kp + (int64_t)k0 * p.k_row_stride;
        const T *vt = vp + (int64_t)k0 * p.v_row_stride;
        const int last = sk - 1 - k0;
        if (pages) {
            if (p.page_size % BLOCK_N == 0) {
                const int page = pages[k0 / p.page_size], in_page = k0 % p.page_size;
                kt = kp + (int64_t)page * p.k_batch_stride + (int64_t)in_page * p.k_row_stride;
                vt = vp + (int64_t)page * p.v_batch_stride + (int64_t)in_page * p.v_row_stride;
            } else {
#pragma unroll
                for (int i = 0; i < LDK; ++i) {
                    const int row = k0 + min(ldk_row0 + i * RPK, last);
                    const int pi = row / p.page_size;
                    kreg[i] = *(const u32x4 *)(kp + (int64_t)pages[pi] * p.k_batch_stride +
                                               (int64_t)(row - pi * p.page_size) * p.k_row_stride + ldk_col);
                }
#pragma unroll
                for (int i = 0; i < LDV; ++i) {
                    const int row = k0 + min(ldv_row0 + i * RPV, last);
                    const int pi = row / p.page_size;
                    vreg[i] = *(const u32x4 *)(vp + (int64_t)pages[pi] * p.v_batch_stride +
                                               (int64_t)(row - pi * p.page_size) * p.v_row_stride + ldv_col);
                }
                return;
            }
        }
#pragma unroll
        for (int i = 0; i < LDK; ++i) kreg[i] = *(const u32x4 *)(kt + (uint32_t)(min(ldk_row0 + i * RPK, last) * k_rs + ldk_col));
#pragma unroll
        for (int i = 0; i < LDV; ++i) vreg[i] = *(const u32x4 *)(vt + (uint32_t)(min(ldv_row0 + i * RPV, last) * v_rs + ldv_col));
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < LDK; ++i) {
            const int c = tid + i * NT;
            *(u32x4 *)(kbuf + lds_off<64>(c / CHK, c % CHK)) = kreg[i];
        }
#pragma unroll
        for (int i = 0; i < LDV; ++i) {
            const int c = tid + i * NT;
            *(u32x4 *)(vbuf + lds_off<DVT>(c / CHV, c % CHV)) = vreg[i];
        }
    };

    // lane-constant parts of the LDS addresses (the swizzle XORs chunk bits 0-3 only: see fa_fwd_kernel.h)
    const int i16 = lane & 15, g1 = (lane >> 4) & 1;
    const int kbase = lds_off<64>(r, hh) ^ (32 * wave);        // K row r, chunk 2 wave + hh
    const int vsbase = lds_off<DVT>(r, hh);                    // V row r, chunk hh (score reads)
    const int vbase = lds_off<DVT>(4 * hh + (i16 >> 2), 2 * g1 + ((i16 >> 1) & 1)) + 8 * (i16 & 1);  // transposed reads

    if (n_min < n_max) {
        load_tile(n_min);
        store_tile();
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): Q / Qv retired here, not in front of the first MFMA of every tile
    __syncthreads();

    for (int n = n_min; n < n_max; ++n) {
        const bool has_next = n + 1 < n_max;
        if (has_next) load_tile(n + 1);
        const int k0 = n * BLOCK_N;
        // workgroup-uniform tile classification (every wave has the same 32 rows)
        bool skip = false, need_mask = k0 + BLOCK_N > sk;
        if (p.window_right >= 0) {
            skip = skip || (k0 > qr_hi + shift + p.window_right);
            need_mask = need_mask || (k0 + BLOCK_N - 1 > qr_lo + shift + p.window_right);
        }
        if (p.window_left >= 0) {
            skip = skip || (k0 + BLOCK_N - 1 < qr_lo + shift - p.window_left);
            need_mask = need_mask || (k0 < qr_hi + shift - p.window_left);
        }
        if (p.chunk > 0) {
            const int w_lo = chunk_floor(qr_lo + shift, p.chunk), w_in_lo = chunk_floor(qr_hi + shift, p.chunk);
            skip = skip || (k0 + BLOCK_N - 1 < w_lo) || (k0 >= w_in_lo + p.chunk);
            need_mask = need_mask || (k0 < w_in_lo) || (k0 + BLOCK_N > w_lo + p.chunk);
        }

        if (!skip) {
            // ---- partial S^T of this wave: K step `wave` + its quarter of the V columns --------------------------------
            f32x16 s[2];
            zero_scores(s);
            {
                const u32x4 kf0 = *(const u32x4 *)(kbuf + kbase);
                const u32x4 kf1 = *(const u32x4 *)(kbuf + kbase + 32 * 64 * 2);
                s[0] = Elem<T>::mma(kf0, qf, s[0]);
                s[1] = Elem<T>::mma(kf1, qf, s[1]);
            }
            if (has_qv) {
#pragma unroll
                for (int ks = 0; ks < KSV; ++ks) {
                    const int off = vsbase ^ (32 * (KSV * wave + ks));  // = lds_off<DVT>(r, 2 (KSV wave + ks) + hh)
                    const u32x4 vf0 = *(const u32x4 *)(vbuf + off);
                    const u32x4 vf1 = *(const u32x4 *)(vbuf + off + 32 * DVT * 2);
                    s[0] = Elem<T>::mma(vf0, qvf[ks], s[0]);
                    s[1] = Elem<T>::mma(vf1, qvf[ks], s[1]);
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const f32x16 &sv = s[j >> 2];
                const int b4 = 4 * (j & 3);
                *(float4 *)(sred + ((wave * 8 + j) * 64 + lane) * 16) = make_float4(sv[b4], sv[b4 + 1], sv[b4 + 2], sv[b4 + 3]);
            }
            __syncthreads();
            // ---- full S^T: the four partials summed in wave order (identical in every wave) ---------------------------
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float4 a = *(const float4 *)(sred + ((0 * 8 + j) * 64 + lane) * 16);
#pragma unroll
                for (int w = 1; w < QV_NWAVES; ++w) {
                    const float4 b = *(const float4 *)(sred + ((w * 8 + j) * 64 + lane) * 16);
                    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
                }
                const int b4 = 4 * (j & 3);
                s[j >> 2][b4] = a.x; s[j >> 2][b4 + 1] = a.y; s[j >> 2][b4 + 2] = a.z; s[j >> 2][b4 + 3] = a.w;
            }

            if constexpr (SOFTCAP) softcap_scores(s, sc);
            if (need_mask) {
                int lim_hi = sk, lim_lo = 0;
                if (p.window_right >= 0) lim_hi = min(sk, my_row + shift + p.window_right + 1);
                if (p.window_left >= 0) lim_lo = max(0, my_row + shift - p.window_left);
                if (p.chunk > 0) {
                    const int c_lo = chunk_floor(my_row + shift, p.chunk);
                    lim_lo = max(lim_lo, c_lo);
                    lim_hi = min(lim_hi, c_lo + p.chunk);
                }
                mask_scores(s, k0, hh, lim_lo, lim_hi);
            }

            u32x4 pf[4];  // online softmax (lane = packed row; identical in every wave)
            softmax_step<T, DBW>(s, m_run, l_run, o_acc, sc, pf);
            // ---- O^T += V^T.P^T over this wave's column blocks ----------------------------------------------------------
#pragma unroll
            for (int dbl = 0; dbl < DBW; ++dbl) pv_16<T, DVT * 2>(vbuf, vbase, DBW * wave + dbl, pf, o_acc[dbl]);
        }
        __syncthreads();  // every read of the K/V tile and of the partial scores is done
        if (has_next) {
            store_tile();
            __syncthreads();
        }
    }

    // ---- epilogue: normalise, LSE, O rows straight from the accumulators (decode: O is small beside the cache) ---------
    const float l_tot = half_swap_sum(l_run);
    const bool empty = (l_tot == 0.f) || (l_tot != l_tot);
    const float inv = empty ? 1.f : 1.f / l_tot;
    if (!row_ok) return;
    const int64_t row_o = p.cu_seqlens_q ? (int64_t)(q0 + my_row) : (int64_t)my_row;
    if (wave == 0 && hh == 0) {
        const int64_t li = (p.cu_seqlens_q ? (int64_t)head * p.total_q + row_o : ((int64_t)batch * p.h + head) * p.seqlen_q + my_row) +
                           split * p.lse_split_stride;
        p.lse[li] = empty ? INFINITY : m_run * sc.scale + __logf(l_tot);
    }
    const int64_t o_off = (p.cu_seqlens_q ? 0 : (int64_t)batch * p.o_batch_stride) + row_o * p.o_row_stride +
                          (int64_t)head * p.o_head_stride;
    if (p.num_splits > 1) {
        store_split_partial((float *)p.o + split * p.o_split_stride + o_off, o_acc, inv, CPW * wave, hh, p.dv);
    } else {
        T *op = (T *)p.o + o_off;
#pragma unroll
        for (int dbl = 0; dbl < DBW; ++dbl)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int col = CPW * wave + dbl * 32 + 8 * g4 + 4 * hh;
                u32x2 w;
                w[0] = Elem<T>::pack2(o_acc[dbl][4 * g4] * inv, o_acc[dbl][4 * g4 + 1] * inv);
                w[1] = Elem<T>::pack2(o_acc[dbl][4 * g4 + 2] * inv, o_acc[dbl][4 * g4 + 3] * inv);
                if (col < p.dv) *(u32x2 *)(op + col) = w;
            }
    }
}

}  // namespace fa
