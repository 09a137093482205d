// fa_bwd_kernel_bs.h — block-sparse backward (fa_bwd_block_sparse, include/fa_bwd.h): the two tile loops of fa_bwd_kernel.h
// walking tiles they take from lists in device memory instead of a contiguous range.
//
// The reference has no such backward: its cute surface returns the DENSE gradient for a block-sparse forward
// (flash_attn/cute/interface.py:1055-1069).  The shape here is this project's own backward -- one producer per output element,
// no atomics, no workspace -- with the lists as the loop bounds:
//   * bs_bwd_dq_kernel: one workgroup = one 128-row query block = one row of the forward's two lists.  It walks
//     2 x (full_cnt + mask_cnt) tiles of 64 keys exactly as bs_fwd_kernel (fa_fwd_kernel_bs.h) walks them: counts clamped to
//     [0, nk], the index of tile t + 2 fetched at the top of iteration t, K / V of tile t + 1 issued before tile t is computed.
//   * bs_bwd_dkdv_kernel: one workgroup = one 128-key block of a (batch, kv head).  For every query head of its GQA group, in
//     ascending order, it walks that head's KEY-MAJOR list (q_block_cnt / q_block_idx: the query blocks that visit this key
//     block) and, per listed query block, its two 64-row Q / dO tiles.  The walk over all heads is one pipeline: the position
//     two tiles ahead is fetched while the current tile is computed, across head boundaries too.
//   * a listed tile that cannot hold a visible (row, key) pair -- past seqlen_q / seqlen_k, outside the causal / window range of
//     the workgroup's block, or an index outside [0, nm) / [0, nk) -- is neither loaded nor computed.  The decision is
//     workgroup-uniform, and it is what keeps any list content from reading outside Q / dO / K / V;
//   * the call's own mask is applied element-wise in the tiles a boundary crosses, by the per-wave rule of fa_bwd_kernel.h;
//   * rows with LSE = +inf (no visible key, no sink) give P = exp2(-inf) = 0 and D = 0: dS = 0, never NaN;
//   * a key block nobody visits ends with dK = dV = 0, a query block with both counts 0 with dQ = 0: the accumulators start
//     at zero and the epilogue always runs.
// The accumulation order is the list order: equal lists give bit-equal gradients.
// Both kernels are the NB = 1 C++ tile paths of bwd_dq_kernel / bwd_dkdv_kernel (staging by LDS-DMA, swizzle, bwd_point, the
// register -> LDS -> coalesced-row epilogue) without dropout and ALiBi and with d_v == d, restated here: a fix to the mask
// rule, the swizzle or the epilogue has to be made in both files.  (That they are instantiated in a unit of their own,
// fa_bwd_bs_api.hip, keeps fa_bwd_api.hip's kernels what tests/test_bwd_plan.py counts; it does not ask for the copy.  A shared
// header was cut and kept out for its code objects: profiles/bwd_tile_step_refactor.md.)  No generated asm block.
#pragma once

#include "fa_bwd_kernel.h"
#include "fa_fwd_kernel_bs.h"  // BsList, BS_BLOCK

namespace fa {

struct BsBwdParams {
    BParams p;          // dense layout (no cu_seqlens, no ALiBi, no dropout: fa_bwd_block_sparse_validate); num_blocks = nm or nk
    BsList full, mask;  // the forward's lists, (b, h, nm[, nk]): read by bs_bwd_dq_kernel.  full.cnt == NULL: no full list
    BsList keyq;        // key-major, cnt (b, h, nk), idx (b, h, nk, nm): read by bs_bwd_dkdv_kernel (cnt_ms / idx_ms step a key block)
    int32_t nm, nk;     // ceil(seqlen_q / 128), ceil(seqlen_k / 128): counts are clamped to them, indices outside name no tile
};

// ------------------------------------------------------------------------------------------------------------------
// dQ: 4 waves x 32 query rows, Q / dO fragments resident (AGPRs), LSE and D per-lane scalars.
// ------------------------------------------------------------------------------------------------------------------
template <typename T, int D, bool SOFTCAP>
__global__ __launch_bounds__(256, 1) void bs_bwd_dq_kernel(const BsBwdParams bp) {
    const BParams &p = bp.p;
    constexpr int BLOCK_M = BS_BLOCK;
    constexpr int KSTEPS = D / 16;
    constexpr int DBLOCKS = D / 32;
    constexpr int CH_PER_ROW = D / 8;
    constexpr int TILE_BYTES = BLOCK_N * D * 2;
    constexpr int LD_PER_THREAD = BLOCK_N * CH_PER_ROW / 256;
    static_assert(LD_PER_THREAD == 2 || LD_PER_THREAD == 4, "head-dim tiles 64 and 128: 2 / 4 LDS-DMA pieces per wave");
    constexpr int O_ROW_BYTES = D * 2 + 16;
    constexpr int ROWB = D * 2;
    constexpr float LOG2E = 1.4426950408889634f;

    extern __shared__ __attribute__((aligned(16))) char smem[];  // [K0 | K1 | V0 | V1], reused by the epilogue

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int i16 = lane & 15, g1 = (lane >> 4) & 1;
    const int kbase = lds_off<D>(r, hh);
    const int vbase = lds_off<D>(4 * hh + (i16 >> 2), 2 * g1 + ((i16 >> 1) & 1)) + 8 * (i16 & 1);

    int m_block, head, batch;
    if (!decode_block(p, m_block, head, batch, p.h)) return;
    const int kv_head = head / p.h_ratio;
    const BSeq sq_ = bwd_seq(p, batch);
    const int sq = sq_.sq, sk = sq_.sk;
    const int row_lo = m_block * BLOCK_M;
    if (row_lo >= sq) return;
    const int shift = sk - sq;  // bottom-right aligned masks

    // ---- this query block's row of the forward's lists (indexed by the QUERY head; workgroup-uniform) ------------------
    const int32_t *f_idx = nullptr;
    int f_cnt = 0;
    if (bp.full.cnt) {
        f_cnt = bp.full.cnt[batch * bp.full.cnt_bs + head * bp.full.cnt_hs + m_block * bp.full.cnt_ms];
        f_idx = bp.full.idx + batch * bp.full.idx_bs + head * bp.full.idx_hs + m_block * bp.full.idx_ms;
    }
    int m_cnt = bp.mask.cnt[batch * bp.mask.cnt_bs + head * bp.mask.cnt_hs + m_block * bp.mask.cnt_ms];
    const int32_t *m_idx = bp.mask.idx + batch * bp.mask.idx_bs + head * bp.mask.idx_hs + m_block * bp.mask.idx_ms;
    f_cnt = __builtin_amdgcn_readfirstlane(min(max(f_cnt, 0), bp.nk));  // (a count past nk would read past the row)
    m_cnt = __builtin_amdgcn_readfirstlane(min(max(m_cnt, 0), bp.nk));
    const int num_walk = 2 * (f_cnt + m_cnt);  // 64-key tiles: two per listed block, the full list first
    const int64_t f_ns = bp.full.idx_ns, m_ns = bp.mask.idx_ns;
    auto tile_at = [&](int t) -> int {  // 64-key tile of walk position t, -1 behind the end
        if (t >= num_walk) return -1;
        const int e = t >> 1;
        const int blk = e < f_cnt ? f_idx[e * f_ns] : m_idx[(e - f_cnt) * m_ns];
        return __builtin_amdgcn_readfirstlane(2 * blk + (t & 1));
    };

    // ---- keys this row block can see at all: tiles outside are dead -----------------------------------------------------
    const int row_hi = min(sq, row_lo + BLOCK_M);
    int key_hi = sk, key_lo = 0;
    if (p.window_right >= 0) key_hi = min(sk, row_hi + shift + p.window_right);
    if (p.window_left >= 0) key_lo = max(0, row_lo + shift - p.window_left);
    // (also what keeps a wrong index from reading outside K / V: 0 <= n * 64 < key_hi <= seqlen_k)
    auto live = [&](int n) -> bool { return n >= 0 && n < (1 << 24) && n * BLOCK_N < key_hi && n * BLOCK_N + BLOCK_N > key_lo; };

    const int wrow = row_lo + wave * 32;
    const int my_row = wrow + r;
    const bool wave_active = wrow < sq;

    const T *qp = (const T *)p.q + sq_.q_base + (int64_t)head * p.q_head_stride;
    const T *gp = (const T *)p.dout + sq_.do_base + (int64_t)head * p.do_head_stride;
    const T *kp = (const T *)p.k + sq_.k_base + (int64_t)kv_head * p.k_head_stride;
    const T *vp = (const T *)p.v + sq_.v_base + (int64_t)kv_head * p.v_head_stride;

    // ---- Q, dO fragments (B operands), LSE and D of this lane's row -------------------------------------------------------
    u32x4 qf[KSTEPS], gf[KSTEPS];
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
        const int d0 = ks * 16 + hh * 8;
        u32x4 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
        if (my_row < sq && d0 < p.d) {
            a = *(const u32x4 *)(qp + (int64_t)my_row * p.q_row_stride + d0);
            b = *(const u32x4 *)(gp + (int64_t)my_row * p.do_row_stride + d0);
        }
        qf[ks] = a;
        gf[ks] = b;
        asm volatile("; pin Q" : "+a"(qf[ks]));   // B operands of every score MFMA: AGPR residents
        asm volatile("; pin dO" : "+a"(gf[ks]));
    }
    float lse2 = INFINITY, dsum = 0.f;  // rows past the end of q: P = exp2(-inf) = 0
    if (my_row < sq) {
        lse2 = p.lse[sq_.stat_base + (int64_t)head * sq_.lse_hs + my_row] * LOG2E;  // (+inf stays +inf)
        dsum = p.dsum[sq_.dsum_base + (int64_t)head * sq_.dsum_hs + my_row];
    }

    f32x16 dq_acc[DBLOCKS];  // AGPRs
    {
        const u32x4 z4 = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < DBLOCKS; ++i) Mfma<T>::o_zero(dq_acc[i], z4);
    }

    // ---- K / V staging by LDS-DMA: rows past the sequence end clamp to the last row (masked), chunks past d to chunk 0 -----
    int dma_row[LD_PER_THREAD], dma_col[LD_PER_THREAD];
    uint32_t k_off[LD_PER_THREAD], v_off[LD_PER_THREAD];
    const int k_rs = (int)p.k_row_stride, v_rs = (int)p.v_row_stride;  // host guarantees < 2^24
#pragma unroll
    for (int i = 0; i < LD_PER_THREAD; ++i) {
        const int slot = wave * (LD_PER_THREAD * 64) + i * 64 + lane;  // 16-byte slot inside the tile image
        const int row = slot / CH_PER_ROW;
        int ch;  // inverse of lds_off<D>: the chunk stored at this slot
        if constexpr (D == 64) ch = (slot % CH_PER_ROW) ^ ((((row >> 1) & 1) << 2) | ((row >> 2) & 3));
        else ch = (slot % CH_PER_ROW) ^ (((row & 3) << 2) | ((row >> 2) & 3));
        dma_row[i] = row;
        dma_col[i] = (ch * 8 < p.d) ? ch * 8 : 0;
        k_off[i] = (uint32_t)(row * k_rs + dma_col[i]) * 2u;
        v_off[i] = (uint32_t)(row * v_rs + dma_col[i]) * 2u;
    }
    const uint32_t lds_wave = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)smem + wave * (LD_PER_THREAD * 1024);
    auto load_tile = [&](int n, int buf) {  // n is live: 0 <= n * 64 < seqlen_k
        const int k0 = n * BLOCK_N;
        const T *kt = kp + (int64_t)k0 * p.k_row_stride, *vt = vp + (int64_t)k0 * p.v_row_stride;  // wave-uniform
        if (k0 + BLOCK_N <= sk) {
            lds_dma<LD_PER_THREAD>(lds_wave + buf * TILE_BYTES, kt, k_off);
            lds_dma<LD_PER_THREAD>(lds_wave + (2 + buf) * TILE_BYTES, vt, v_off);
        } else {
            uint32_t ko[LD_PER_THREAD], vo[LD_PER_THREAD];
#pragma unroll
            for (int i = 0; i < LD_PER_THREAD; ++i) {
                const int rel = min(k0 + dma_row[i], sk - 1) - k0;
                ko[i] = (uint32_t)(rel * k_rs + dma_col[i]) * 2u;
                vo[i] = (uint32_t)(rel * v_rs + dma_col[i]) * 2u;
            }
            lds_dma<LD_PER_THREAD>(lds_wave + buf * TILE_BYTES, kt, ko);
            lds_dma<LD_PER_THREAD>(lds_wave + (2 + buf) * TILE_BYTES, vt, vo);
        }
    };

    int n_cur = tile_at(0), n_next = tile_at(1);
    if (live(n_cur)) load_tile(n_cur, 0);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): see fa_fwd_kernel.h
    tile_barrier<0>();

    for (int t = 0; t < num_walk; ++t) {
        const int cur = t & 1;
        const int n_after = tile_at(t + 2);  // consumed by the NEXT iteration's load_tile: a tile of compute hides the chase
        if (live(n_next)) load_tile(n_next, cur ^ 1);  // (buffer cur ^ 1 was last read before the previous barrier)

        const int k0 = n_cur * BLOCK_N;
        bool skip = !wave_active || !live(n_cur);
        if (p.window_right >= 0) skip = skip || (k0 > wrow + 31 + shift + p.window_right);
        if (p.window_left >= 0) skip = skip || (k0 + BLOCK_N - 1 < wrow + shift - p.window_left);
        // masks only where a boundary crosses this (32 rows x 64 keys) block (rows past the end of q: LSE = +inf)
        bool need_mask = (k0 + BLOCK_N > sk);
        if (p.window_right >= 0) need_mask = need_mask || (k0 + BLOCK_N - 1 > wrow + shift + p.window_right);
        if (p.window_left >= 0) need_mask = need_mask || (k0 < wrow + 31 + shift - p.window_left);

        if (!skip) {
            const char *kbuf = smem + cur * TILE_BYTES;
            const char *vbuf = smem + (2 + cur) * TILE_BYTES;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {  // two 32-key halves, one after the other
                // ---- S^T = K Q^T, dP^T = V dO^T: 32 keys, query on the lane ----------------------------------
                f32x16 s[1], dp[1];
                constexpr int PF = 2;  // LDS fragments are fetched PF steps ahead of their MFMAs (see bwd_dkdv_kernel)
                auto row_frag = [&](const char *buf, int ks) {
                    return *(const u32x4 *)(buf + ((kbase ^ (32 * ks)) + kb * (32 * ROWB)));
                };
                u32x4 ka_r[PF + 1], va_r[PF + 1];
#pragma unroll
                for (int i = 0; i < PF; ++i) { ka_r[i] = row_frag(kbuf, i); va_r[i] = row_frag(vbuf, i); }
#pragma unroll
                for (int ks = 0; ks < KSTEPS; ++ks) {
                    if (ks + PF < KSTEPS) {
                        ka_r[(ks + PF) % (PF + 1)] = row_frag(kbuf, ks + PF);
                        va_r[(ks + PF) % (PF + 1)] = row_frag(vbuf, ks + PF);
                    }
                    const u32x4 ka = ka_r[ks % (PF + 1)], va = va_r[ks % (PF + 1)];
                    if (ks == 0) { Mfma<T>::s_first(s[0], ka, qf[ks]); Mfma<T>::s_first(dp[0], va, gf[ks]); }
                    else { Mfma<T>::s_acc(s[0], ka, qf[ks]); Mfma<T>::s_acc(dp[0], va, gf[ks]); }
                    __builtin_amdgcn_sched_barrier(0);
                }
                drain_tiles<1>(s, dp);
                auto pointwise = [&](auto mask_c) {
                    constexpr bool MASK = decltype(mask_c)::value;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int key = k0 + kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
                        const int rel = my_row + shift - key;
                        bool vis = true;
                        if constexpr (MASK) {
                            vis = key < sk;
                            if (p.window_right >= 0) vis = vis && (rel + p.window_right >= 0);
                            if (p.window_left >= 0) vis = vis && (rel <= p.window_left);
                        }
                        float pv, ds;
                        bwd_point<SOFTCAP, MASK, false>(p, s[0][i], dp[0][i], lse2, dsum, 0.f, rel, vis, 0u, pv, ds);
                        dp[0][i] = ds;
                    }
                };
                if (need_mask) pointwise(std::true_type{});
                else pointwise(std::false_type{});
                u32x4 dsf[2];
#pragma unroll
                for (int st = 0; st < 2; ++st)
#pragma unroll
                    for (int j = 0; j < 4; ++j) dsf[st][j] = Elem<T>::pack2(dp[0][8 * st + 2 * j], dp[0][8 * st + 2 * j + 1]);
                __builtin_amdgcn_sched_barrier(0);
                // ---- dQ^T += K^T dS^T (K^T through transposing reads of the same K tile) ---------------------------
                auto tr_frag = [&](int tt) {  // step tt = (db, st)
                    const int db = tt >> 1, st = tt & 1;
                    u32x4 f;
#pragma unroll
                    for (int j2 = 0; j2 < 2; ++j2) {
                        const int off = (vbase ^ (64 * db + 32 * j2)) + (32 * kb + 16 * st + 8 * j2) * ROWB;
                        const u32x2 a = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (__attribute__((address_space(3))) s16x4 *)(kbuf + off)));
                        f[2 * j2] = a[0];
                        f[2 * j2 + 1] = a[1];
                    }
                    return f;
                };
                constexpr int NT2 = 2 * DBLOCKS;
                u32x4 kt_r[PF + 1];
#pragma unroll
                for (int i = 0; i < PF; ++i) kt_r[i] = tr_frag(i);
#pragma unroll
                for (int tt = 0; tt < NT2; ++tt) {
                    if (tt + PF < NT2) kt_r[(tt + PF) % (PF + 1)] = tr_frag(tt + PF);
                    Mfma<T>::o_acc_pad(dq_acc[tt >> 1], kt_r[tt % (PF + 1)], dsf[tt & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }

        tile_barrier<0>();  // next tile's LDS-DMA landed (vmcnt(0)), workgroup barrier
        n_cur = n_next;
        n_next = n_after;
    }

    // ---- epilogue: dQ^T registers (lane = row, registers = head dim) -> LDS -> coalesced rows ----------------------------
    drain_acc(dq_acc);  // asm MFMA results -> VALU readers
    T *dqp = (T *)p.dq + sq_.dq_base + (int64_t)head * p.dq_head_stride;
    char *obuf = smem + wave * (32 * O_ROW_BYTES);
#pragma unroll
    for (int db = 0; db < DBLOCKS; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const f32x16 &acc = dq_acc[db];
            u32x2 w;
            w[0] = Elem<T>::pack2(acc[4 * g4] * p.out_scale, acc[4 * g4 + 1] * p.out_scale);
            w[1] = Elem<T>::pack2(acc[4 * g4 + 2] * p.out_scale, acc[4 * g4 + 3] * p.out_scale);
            *(u32x2 *)(obuf + r * O_ROW_BYTES + (db * 32 + 8 * g4 + 4 * hh) * 2) = w;
        }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < (32 * CH_PER_ROW) / 64; ++i) {
        const int c = lane + i * 64;
        const int row = c / CH_PER_ROW, ch = c % CH_PER_ROW;
        const int qrow = wrow + row;
        if (qrow < sq && ch * 8 < p.d) {
            const u32x4 val = *(const u32x4 *)(obuf + row * O_ROW_BYTES + ch * 16);
            *(u32x4 *)(dqp + (int64_t)qrow * p.dq_row_stride + ch * 8) = val;
        }
    }
}

template <int D>
constexpr int smem_bytes_bs_dq() {
    constexpr int kv = 4 * BLOCK_N * D * 2;
    constexpr int o = 4 * 32 * (D * 2 + 16);
    return kv > o ? kv : o;
}

// ------------------------------------------------------------------------------------------------------------------
// dK / dV: 4 waves x 32 keys, K / V fragments resident (arch VGPRs), both accumulator sets in AGPRs; Q / dO tiles of 64 rows
// by LDS-DMA, their LSE / D rows alongside.
// ------------------------------------------------------------------------------------------------------------------
template <typename T, int D, bool SOFTCAP>
__global__ __launch_bounds__(256, 1) void bs_bwd_dkdv_kernel(const BsBwdParams bp) {
    const BParams &p = bp.p;
    constexpr int BLOCK_K = BS_BLOCK;
    constexpr int BM = 64;  // query rows per streamed tile
    constexpr int KSTEPS = D / 16;
    constexpr int DBLOCKS = D / 32;
    constexpr int CH_PER_ROW = D / 8;
    constexpr int TILE_BYTES = BM * D * 2;
    constexpr int LD_PER_THREAD = BM * CH_PER_ROW / 256;
    static_assert(LD_PER_THREAD == 2 || LD_PER_THREAD == 4, "head-dim tiles 64 and 128: 2 / 4 LDS-DMA pieces per wave");
    constexpr int O_ROW_BYTES = D * 2 + 16;
    constexpr int ROWB = D * 2;
    constexpr float LOG2E = 1.4426950408889634f;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    // [Q0 | Q1 | dO0 | dO1 | lse[2][64] | dsum[2][64]]; the epilogue reuses the front as 4 x [32][O_ROW_BYTES]
    float *lse_s = (float *)(smem + 4 * TILE_BYTES);
    float *dsum_s = lse_s + 2 * BM;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int i16 = lane & 15, g1 = (lane >> 4) & 1;
    const int kbase = lds_off<D>(r, hh);
    const int vbase = lds_off<D>(4 * hh + (i16 >> 2), 2 * g1 + ((i16 >> 1) & 1)) + 8 * (i16 & 1);

    int n_block, kv_head, batch;
    if (!decode_block(p, n_block, kv_head, batch, p.h_k)) return;
    const BSeq sq_ = bwd_seq(p, batch);
    const int sq = sq_.sq, sk = sq_.sk;
    const int n0 = n_block * BLOCK_K;
    if (n0 >= sk) return;
    const int shift = sk - sq;

    // ---- query rows that can see any key of this block: tiles outside are dead ------------------------------------------
    const int last_key = min(sk, n0 + BLOCK_K) - 1;
    int row_lo = 0, row_hi = sq;
    if (p.window_right >= 0) row_lo = max(0, n0 - shift - p.window_right);
    if (p.window_left >= 0) row_hi = min(sq, last_key - shift + p.window_left + 1);
    // (also what keeps a wrong index from reading outside Q / dO / LSE / D: 0 <= m * 64 < row_hi <= seqlen_q)
    auto live = [&](int m) -> bool { return m >= 0 && m < (1 << 24) && m * BM < row_hi && m * BM + BM > row_lo; };

    // ---- the walk: for every query head of the group, ascending, the first cnt entries of its key-major row, two 64-row
    //      tiles per entry.  fetch() returns the position under the cursor and steps it (workgroup-uniform scalars). --------
    const BsList &kl = bp.keyq;
    const int head0 = kv_head * p.h_ratio;
    int w_hi = -1, w_t = 0, w_cnt2 = 0;
    const int32_t *w_idx = nullptr;
    auto fetch = [&](int &head, int &m_tile) {
        while (w_t >= w_cnt2) {  // next head with entries (the first call starts the first head)
            if (++w_hi >= p.h_ratio) { w_hi = p.h_ratio; head = -1; m_tile = -1; return; }
            const int hq = head0 + w_hi;
            const int c = kl.cnt[batch * kl.cnt_bs + hq * kl.cnt_hs + n_block * kl.cnt_ms];
            w_cnt2 = __builtin_amdgcn_readfirstlane(2 * min(max(c, 0), bp.nm));  // (a count past nm would read past the row)
            w_idx = kl.idx + batch * kl.idx_bs + hq * kl.idx_hs + n_block * kl.idx_ms;
            w_t = 0;
        }
        head = head0 + w_hi;
        m_tile = __builtin_amdgcn_readfirstlane(2 * w_idx[(w_t >> 1) * kl.idx_ns] + (w_t & 1));
        ++w_t;
    };

    const int key_w0 = n0 + wave * 32;

    // ---- K, V fragments of this wave's keys: B operands of S = Q K^T and dP = dO V^T ---------------------------------------
    const T *kp = (const T *)p.k + sq_.k_base + (int64_t)kv_head * p.k_head_stride;
    const T *vp = (const T *)p.v + sq_.v_base + (int64_t)kv_head * p.v_head_stride;
    u32x4 kf[KSTEPS], vf[KSTEPS];
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
        const int key = key_w0 + r;
        const int d0 = ks * 16 + hh * 8;
        u32x4 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
        if (key < sk && d0 < p.d) {
            a = *(const u32x4 *)(kp + (int64_t)key * p.k_row_stride + d0);
            b = *(const u32x4 *)(vp + (int64_t)key * p.v_row_stride + d0);
        }
        kf[ks] = a;
        vf[ks] = b;
    }

    f32x16 dk_acc[DBLOCKS], dv_acc[DBLOCKS];  // AGPRs, pinned by asm MFMAs
    {
        const u32x4 z4 = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < DBLOCKS; ++i) {
            Mfma<T>::o_zero(dk_acc[i], z4);
            Mfma<T>::o_zero(dv_acc[i], z4);
        }
        drain_acc(dk_acc);
        drain_acc(dv_acc);
    }

    // ---- Q / dO tile staging by LDS-DMA: rows clamped into the sequence (clamped rows are masked) -------------------------
    float stat_reg = 0.f;
    int dma_row[LD_PER_THREAD], dma_col[LD_PER_THREAD];
    uint32_t q_off[LD_PER_THREAD], g_off[LD_PER_THREAD];
    const int q_rs = (int)p.q_row_stride, g_rs = (int)p.do_row_stride;  // host guarantees < 2^24
#pragma unroll
    for (int i = 0; i < LD_PER_THREAD; ++i) {
        const int slot = wave * (LD_PER_THREAD * 64) + i * 64 + lane;
        const int row = slot / CH_PER_ROW;
        int ch;  // inverse of lds_off<D>
        if constexpr (D == 64) ch = (slot % CH_PER_ROW) ^ ((((row >> 1) & 1) << 2) | ((row >> 2) & 3));
        else ch = (slot % CH_PER_ROW) ^ (((row & 3) << 2) | ((row >> 2) & 3));
        dma_row[i] = row;
        dma_col[i] = (ch * 8 < p.d) ? ch * 8 : 0;
        q_off[i] = (uint32_t)(row * q_rs + dma_col[i]) * 2u;
        g_off[i] = (uint32_t)(row * g_rs + dma_col[i]) * 2u;
    }
    const uint32_t lds_wave = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)smem + wave * (LD_PER_THREAD * 1024);
    auto load_tile = [&](int head, int m_tile, int buf) {  // m_tile is live: 0 <= m_tile * 64 < seqlen_q
        const int row0 = m_tile * BM;
        const T *qt = (const T *)p.q + sq_.q_base + (int64_t)head * p.q_head_stride + (int64_t)row0 * p.q_row_stride;  // wave-uniform
        const T *gt = (const T *)p.dout + sq_.do_base + (int64_t)head * p.do_head_stride + (int64_t)row0 * p.do_row_stride;
        if (row0 + BM <= sq) {
            lds_dma<LD_PER_THREAD>(lds_wave + buf * TILE_BYTES, qt, q_off);
            lds_dma<LD_PER_THREAD>(lds_wave + (2 + buf) * TILE_BYTES, gt, g_off);
        } else {
            uint32_t qo[LD_PER_THREAD], go[LD_PER_THREAD];
#pragma unroll
            for (int i = 0; i < LD_PER_THREAD; ++i) {
                const int rel = min(row0 + dma_row[i], sq - 1) - row0;
                qo[i] = (uint32_t)(rel * q_rs + dma_col[i]) * 2u;
                go[i] = (uint32_t)(rel * g_rs + dma_col[i]) * 2u;
            }
            lds_dma<LD_PER_THREAD>(lds_wave + buf * TILE_BYTES, qt, qo);
            lds_dma<LD_PER_THREAD>(lds_wave + (2 + buf) * TILE_BYTES, gt, go);
        }
        if (tid < 2 * BM) {  // threads 0..63: LSE (log2 units), 64..127: D
            const int row = min(row0 + (tid & (BM - 1)), sq - 1);
            if (tid < BM) stat_reg = p.lse[sq_.stat_base + (int64_t)head * sq_.lse_hs + row] * LOG2E;  // (+inf stays +inf: P = 0)
            else stat_reg = p.dsum[sq_.dsum_base + (int64_t)head * sq_.dsum_hs + row];
        }
    };
    auto store_stats = [&](int buf) {
        if (tid < BM) lse_s[buf * BM + tid] = stat_reg;
        else if (tid < 2 * BM) dsum_s[buf * BM + tid - BM] = stat_reg;
    };

    int h_cur, m_cur, h_next, m_next;
    fetch(h_cur, m_cur);
    fetch(h_next, m_next);
    if (live(m_cur)) {
        load_tile(h_cur, m_cur, 0);
        store_stats(0);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): see fa_fwd_kernel.h
    tile_barrier<0>();

    for (int cur = 0; h_cur >= 0; cur ^= 1) {
        int h_after, m_after;
        fetch(h_after, m_after);  // consumed by the NEXT iteration's load_tile: a tile of compute hides the chase
        const bool has_next = live(m_next);  // (behind the end: m_next = -1)
        if (has_next) load_tile(h_next, m_next, cur ^ 1);  // (buffer cur ^ 1 was last read before the previous barrier)

        const int row0 = m_cur * BM;
        // wave-level skip: no (row, key) pair of this tile x this wave's keys is visible
        bool skip = key_w0 >= sk || !live(m_cur);
        if (p.window_right >= 0) skip = skip || (key_w0 > row0 + BM - 1 + shift + p.window_right);
        if (p.window_left >= 0) skip = skip || (key_w0 + 31 < row0 + shift - p.window_left);
        // masks only where a boundary crosses this (64 rows x 32 keys) block; rows past the end of q are clamped copies
        bool need_mask = (key_w0 + 32 > sk) || (row0 + BM > sq);
        if (p.window_right >= 0) need_mask = need_mask || (key_w0 + 31 > row0 + shift + p.window_right);
        if (p.window_left >= 0) need_mask = need_mask || (key_w0 < row0 + BM - 1 + shift - p.window_left);

        if (!skip) {
            const char *qbuf = smem + cur * TILE_BYTES;
            const char *gbuf = smem + (2 + cur) * TILE_BYTES;
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                // ---- S = Q K^T and dP = dO V^T for 32 query rows x this wave's keys -----------------------
                f32x16 s[1], dp[1];
                constexpr int PF = 2;  // LDS fragments are fetched PF steps ahead of the MFMAs that consume them
                auto row_frag = [&](const char *buf, int ks) {
                    return *(const u32x4 *)(buf + ((kbase ^ (32 * ks)) + rb * (32 * ROWB)));
                };
                u32x4 qa_r[PF + 1], ga_r[PF + 1];
#pragma unroll
                for (int i = 0; i < PF; ++i) { qa_r[i] = row_frag(qbuf, i); ga_r[i] = row_frag(gbuf, i); }
#pragma unroll
                for (int ks = 0; ks < KSTEPS; ++ks) {
                    if (ks + PF < KSTEPS) {
                        qa_r[(ks + PF) % (PF + 1)] = row_frag(qbuf, ks + PF);
                        ga_r[(ks + PF) % (PF + 1)] = row_frag(gbuf, ks + PF);
                    }
                    const u32x4 qa = qa_r[ks % (PF + 1)], ga = ga_r[ks % (PF + 1)];
                    if (ks == 0) { BMfma<T>::s_first_v(s[0], qa, kf[ks]); BMfma<T>::s_first_v(dp[0], ga, vf[ks]); }
                    else { BMfma<T>::s_acc_v(s[0], qa, kf[ks]); BMfma<T>::s_acc_v(dp[0], ga, vf[ks]); }
                    __builtin_amdgcn_sched_barrier(0);
                }
                drain_tiles<1>(s, dp);
                // ---- P and dS: key on the lane, query row = register ----------------------------------
                auto pointwise = [&](auto mask_c) {
                    constexpr bool MASK = decltype(mask_c)::value;
                    const int my_key = key_w0 + r;
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) {
                        const int rbase = 32 * rb + 8 * g4 + 4 * hh;
                        const float4 l4 = *(const float4 *)(lse_s + cur * BM + rbase);
                        const float4 d4 = *(const float4 *)(dsum_s + cur * BM + rbase);
                        const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dsv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int i = 4 * g4 + e;
                            const int qi = row0 + rbase + e;
                            const int rel = qi + shift - my_key;
                            bool vis = true;
                            if constexpr (MASK) {
                                vis = (my_key < sk) && (qi < sq);
                                if (p.window_right >= 0) vis = vis && (rel + p.window_right >= 0);
                                if (p.window_left >= 0) vis = vis && (rel <= p.window_left);
                            }
                            float pv, ds;
                            bwd_point<SOFTCAP, MASK, false>(p, s[0][i], dp[0][i], lv[e], dsv[e], 0.f, rel, vis, 0u, pv, ds);
                            s[0][i] = pv;
                            dp[0][i] = ds;
                        }
                    }
                };
                __builtin_amdgcn_sched_barrier(0);
                if (need_mask) pointwise(std::true_type{});
                else pointwise(std::false_type{});
                u32x4 pf[2], dsf[2];
#pragma unroll
                for (int st = 0; st < 2; ++st)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        pf[st][j] = Elem<T>::pack2(s[0][8 * st + 2 * j], s[0][8 * st + 2 * j + 1]);
                        dsf[st][j] = Elem<T>::pack2(dp[0][8 * st + 2 * j], dp[0][8 * st + 2 * j + 1]);
                    }
                __builtin_amdgcn_sched_barrier(0);
                // ---- dV^T += dO^T P,  dK^T += Q^T dS  (A operands through transposing LDS reads) ----------
                auto tr_frag = [&](const char *buf, int tt) {  // step tt = (db, st)
                    const int db = tt >> 1, st = tt & 1;
                    u32x4 f;
#pragma unroll
                    for (int j2 = 0; j2 < 2; ++j2) {
                        const int off = (vbase ^ (64 * db + 32 * j2)) + (32 * rb + 16 * st + 8 * j2) * ROWB;
                        const u32x2 a = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (__attribute__((address_space(3))) s16x4 *)(buf + off)));
                        f[2 * j2] = a[0];
                        f[2 * j2 + 1] = a[1];
                    }
                    return f;
                };
                constexpr int NT2 = 2 * DBLOCKS;
                u32x4 gt_r[PF + 1], qt_r[PF + 1];
#pragma unroll
                for (int i = 0; i < PF; ++i) { gt_r[i] = tr_frag(gbuf, i); qt_r[i] = tr_frag(qbuf, i); }
#pragma unroll
                for (int tt = 0; tt < NT2; ++tt) {
                    if (tt + PF < NT2) {
                        gt_r[(tt + PF) % (PF + 1)] = tr_frag(gbuf, tt + PF);
                        qt_r[(tt + PF) % (PF + 1)] = tr_frag(qbuf, tt + PF);
                    }
                    Mfma<T>::o_acc_pad(dv_acc[tt >> 1], gt_r[tt % (PF + 1)], pf[tt & 1]);
                    Mfma<T>::o_acc_pad(dk_acc[tt >> 1], qt_r[tt % (PF + 1)], dsf[tt & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }

        if (has_next) store_stats(cur ^ 1);
        tile_barrier<0>();  // next tile's LDS-DMA landed (vmcnt(0)), LDS writes visible, workgroup barrier
        h_cur = h_next; m_cur = m_next;
        h_next = h_after; m_next = m_after;
    }

    // ---- epilogue: dK^T / dV^T registers (lane = key, registers = head dim) -> LDS -> coalesced rows ------------
    drain_acc(dk_acc);  // asm MFMA results -> VALU readers
    drain_acc(dv_acc);
    T *dkp = (T *)p.dk + sq_.dk_base + (int64_t)kv_head * p.dk_head_stride;
    T *dvp = (T *)p.dv + sq_.dv_base + (int64_t)kv_head * p.dv_head_stride;
    char *obuf = smem + wave * (32 * O_ROW_BYTES);
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        const float f = which == 0 ? p.out_scale : 1.f;
        T *dst = which == 0 ? dkp : dvp;
        const int64_t rs = which == 0 ? p.dk_row_stride : p.dv_row_stride;
#pragma unroll
        for (int db = 0; db < DBLOCKS; ++db)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x16 &acc = (which == 0 ? dk_acc : dv_acc)[db];
                u32x2 w;
                w[0] = Elem<T>::pack2(acc[4 * g4] * f, acc[4 * g4 + 1] * f);
                w[1] = Elem<T>::pack2(acc[4 * g4 + 2] * f, acc[4 * g4 + 3] * f);
                *(u32x2 *)(obuf + r * O_ROW_BYTES + (db * 32 + 8 * g4 + 4 * hh) * 2) = w;
            }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < (32 * CH_PER_ROW) / 64; ++i) {
            const int c = lane + i * 64;
            const int row = c / CH_PER_ROW, ch = c % CH_PER_ROW;
            const int key = key_w0 + row;
            if (key < sk && ch * 8 < p.d) {
                const u32x4 val = *(const u32x4 *)(obuf + row * O_ROW_BYTES + ch * 16);
                *(u32x4 *)(dst + (int64_t)key * rs + ch * 8) = val;
            }
        }
        __syncthreads();
    }
}

template <int D>
constexpr int smem_bytes_bs_dkdv() { return smem_bytes_dkdv<D>(); }

}  // namespace fa
