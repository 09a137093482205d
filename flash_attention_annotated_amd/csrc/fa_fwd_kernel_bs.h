// fa_fwd_kernel_bs.h — block-sparse forward (fa_fwd_block_sparse, include/fa_fwd.h): the tile loop of fwd_kernel
// (fa_fwd_kernel.h) walking key tiles it takes from two lists in device memory instead of a contiguous n_min .. n_max.
//
// Role of the block-sparse mainloop of the reference's cute forward (flash_attn/cute/block_sparse_utils.py:265-419 consumes
// the lists, flash_attn/cute/block_sparsity.py:33-115 defines them), re-derived for the compiler-scheduled 4-wave x 32-row
// shape of fa_fwd_kernel.h:
//   * one workgroup = one 128-row query block = one row of the lists: the sparse block is the work item;
//   * the workgroup reads its two counts once and walks 2 x (full_cnt + mask_cnt) tiles of 64 keys, two per listed block;
//   * the walk is double-buffered like fwd_kernel's: the loads of tile t + 1 are issued before the compute of tile t.  The
//     tile index of t + 2 is fetched (a wave-uniform load) at the top of iteration t, so the pointer chase is a whole tile
//     ahead of the K / V loads that depend on it;
//   * a listed tile that cannot hold a visible key for this query block -- past seqlen_k (the second half of a ragged last
//     block), outside the causal / window range of the block's rows, or an index outside [0, nk) -- is neither loaded nor
//     computed (workgroup-uniform), so unvisited blocks and dead tiles cost no K / V traffic and no MFMA;
//   * the call's own mask (sequence end, causal / window edges) is applied element-wise in the tiles that need it, by the
//     rule of fwd_kernel.  That rule does not look at which list a block came from: a causal diagonal block in the full list
//     is masked all the same (the reference masks inside full blocks too, flash_attn/cute/flash_fwd.py:1985-1994);
//   * rows without a visible key -- both counts 0 included -- end with l = 0: O = 0 and LSE = +inf, or the sink.
// The per-tile step -- softcap, element mask, online softmax, P^T pack, the 16-bit score and PV products, the pack of O into
// LDS rows -- is fa_fwd_tile_step.h's, shared with the pk / kv8 / qv kernels.  This file owns the walk: the list chase and
// liveness, the tile classification, fwd_kernel's staging (dv-aware V columns), the Q_IN_AGPR score product of D = 256 (asm
// MFMAs on AGPR-pinned Q: scores_16 serves the other head dims) and fwd_kernel's epilogue (sink, rows stored by the wave's
// own row index, no destination in the row padding).  fwd_kernel itself does not use the shared step, so its own
// instantiations stay byte for byte what they were (tests/test_fwd_plan.py counts them).
#pragma once

#include "fa_fwd_tile_step.h"

namespace fa {

constexpr int BS_BLOCK = 128;   // rows of a query block = keys of a key block (the reference's tile under block sparsity)
constexpr int BS_NWAVES = BS_BLOCK / 32;

// One list tensor through element strides: cnt (b, h, nm), idx (b, h, nm, nk); a broadcast dimension has stride 0.
struct BsList {
    const int32_t *cnt, *idx;
    int64_t cnt_bs, cnt_hs, cnt_ms;
    int64_t idx_bs, idx_hs, idx_ms, idx_ns;
};
struct BsParams {
    KParams p;       // num_m_blocks = ceil(seqlen_q / 128); dense layout, no split, no pages (fa_fwd_block_sparse_validate)
    BsList full, mask;  // full.cnt == NULL: no full list
    int32_t nk;      // ceil(seqlen_k / 128): counts are clamped to it, indices outside [0, nk) name no tile
};

template <typename T, int D, bool SOFTCAP>
__global__ __launch_bounds__(BS_NWAVES * 64, (D <= 128 ? 2 : 1)) void bs_fwd_kernel(const BsParams bp) {
    const KParams &p = bp.p;
    constexpr int NWAVES = BS_NWAVES;
    constexpr int NT = NWAVES * 64;
    constexpr int BLOCK_M = BS_BLOCK;
    constexpr int KSTEPS = D / 16;
    constexpr int DBLOCKS = D / 32;
    constexpr int CH_PER_ROW = D / 8;
    constexpr int TILE_BYTES = BLOCK_N * D * 2;
    constexpr int CHUNKS = BLOCK_N * CH_PER_ROW;
    constexpr int LD_PER_THREAD = CHUNKS / NT;
    static_assert(CHUNKS % NT == 0, "tile must divide over the workgroup");
    static_assert(NT % CH_PER_ROW == 0, "a pass of the workgroup covers whole rows");
    constexpr int O_ROW_BYTES = D * 2 + 16;

    extern __shared__ __attribute__((aligned(16))) char smem[];  // [K0 | K1 | V0 | V1], reused by the epilogue

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int hh = lane >> 5;

    int m_block, head, batch, split;
    if (!decode_tile(p, m_block, head, batch, split)) return;  // whole workgroup (padding)
    const int kv_head = head / p.h_ratio;
    const int sq = p.seqlen_q, sk = p.seqlen_k;
    const int row_lo = m_block * BLOCK_M;
    const int64_t lse_base = ((int64_t)batch * p.h + head) * p.seqlen_q;
    const Scales sc = load_scales(p, batch, kv_head);
    const T *qp = (const T *)p.q + (int64_t)batch * p.q_batch_stride + (int64_t)head * p.q_head_stride;
    const T *kp = (const T *)p.k + (int64_t)batch * p.k_batch_stride + (int64_t)kv_head * p.k_head_stride;
    const T *vp = (const T *)p.v + (int64_t)batch * p.v_batch_stride + (int64_t)kv_head * p.v_head_stride;
    T *op = (T *)p.o + (int64_t)batch * p.o_batch_stride + (int64_t)head * p.o_head_stride;

    // ---- this query block's row of the lists: the counts once, the entries as the walk needs them ----------------------
    // (indexed by the QUERY head; everything here is workgroup-uniform)
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

    // ---- keys this row block can see at all (BlockMN::get_n_block_min_max role): tiles outside are dead --------------
    const int shift = sk - sq;  // bottom-right aligned masks
    const int row_hi = min(sq, row_lo + BLOCK_M);
    int key_hi = sk, key_lo = 0;
    if (p.window_right >= 0) key_hi = min(sk, row_hi + shift + p.window_right);
    if (p.window_left >= 0) key_lo = max(0, row_lo + shift - p.window_left);
    // (also what keeps a wrong index from reading outside K / V: 0 <= n * 64 < key_hi <= seqlen_k)
    auto live = [&](int n) -> bool { return n >= 0 && n < (1 << 24) && n * BLOCK_N < key_hi && n * BLOCK_N + BLOCK_N > key_lo; };

    const int wrow = row_lo + wave * 32;          // first row of this wave
    const int my_row = wrow + r;                  // the query row this lane owns
    const bool wave_active = wrow < sq;

    // ---- Q fragments: B operand of S^T = K.Q^T; lane (r,hh) holds Q[row r][16ks + 8hh .. +8] ------
    u32x4 qf[KSTEPS];
    {
        const T *qr = qp + (int64_t)min(my_row, sq - 1) * p.q_row_stride;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const int d0 = ks * 16 + hh * 8;
            qf[ks] = *(const u32x4 *)(qr + (d0 < p.d ? d0 : 0));
        }
        const u32x4 z4 = {0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) qf[ks] = (ks * 16 + hh * 8 < p.d && my_row < sq) ? qf[ks] : z4;
    }
    constexpr bool Q_IN_AGPR = (D == 256);  // (see fwd_kernel: 64 registers only MFMAs read)
    if constexpr (Q_IN_AGPR) {
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) asm volatile("; pin Q" : "+a"(qf[ks]));
    }

    f32x16 o_acc[DBLOCKS];
#pragma unroll
    for (int db = 0; db < DBLOCKS; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) o_acc[db][i] = 0.f;
    float m_run = -INFINITY;  // running row max (unscaled scores), same in both lane halves
    float l_run = 0.f;        // running row sum, PARTIAL per lane half (combined in the epilogue)

    // ---- K/V staging: fwd_kernel's branch-free loads (rows past the sequence end clamp to the last row, head-dim chunks
    // past d / dv to chunk 0; the duplicates are masked or meet zeros) ----------------------------------------------------
    u32x4 kreg[LD_PER_THREAD], vreg[LD_PER_THREAD];
    constexpr int ROWS_PER_PASS = NT / CH_PER_ROW;
    const int ld_row0 = tid / CH_PER_ROW;
    const int ld_col0 = ((tid % CH_PER_ROW) * 8 < p.d) ? (tid % CH_PER_ROW) * 8 : 0;
    const int ld_col0v = ((tid % CH_PER_ROW) * 8 < p.dv) ? (tid % CH_PER_ROW) * 8 : 0;
    const int k_rs = (int)p.k_row_stride, v_rs = (int)p.v_row_stride;  // host guarantees 64 * stride < 2^31
    auto load_tile = [&](int n) {  // n is live: 0 <= n * 64 < seqlen_k
        const int k0 = n * BLOCK_N;
        const T *kt = kp + (int64_t)k0 * p.k_row_stride;  // scalar
        const T *vt = vp + (int64_t)k0 * p.v_row_stride;
        const int last = sk - 1 - k0;
#pragma unroll
        for (int i = 0; i < LD_PER_THREAD; ++i) {
            const int row = min(ld_row0 + i * ROWS_PER_PASS, last);
            kreg[i] = *(const u32x4 *)(kt + (uint32_t)(row * k_rs + ld_col0));
            vreg[i] = *(const u32x4 *)(vt + (uint32_t)(row * v_rs + ld_col0v));
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < LD_PER_THREAD; ++i) {
            const int c = tid + i * NT;
            const int row = c / CH_PER_ROW, ch = c % CH_PER_ROW;
            const int off = lds_off<D>(row, ch);
            *(u32x4 *)(smem + buf * TILE_BYTES + off) = kreg[i];
            *(u32x4 *)(smem + (2 + buf) * TILE_BYTES + off) = vreg[i];
        }
    };

    const int i16 = lane & 15;
    const int g1 = (lane >> 4) & 1;
    const int kbase = lds_off<D>(r, hh);
    const int vbase = lds_off<D>(4 * hh + (i16 >> 2), 2 * g1 + ((i16 >> 1) & 1)) + 8 * (i16 & 1);

    int n_cur = tile_at(0), n_next = tile_at(1);
    if (live(n_cur)) {
        load_tile(n_cur);
        store_tile(0);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): retire the prologue loads (Q included) in front of the loop, as fwd_kernel
    __syncthreads();

    for (int t = 0; t < num_walk; ++t) {
        const int cur = t & 1;
        const int n_after = tile_at(t + 2);  // consumed by the NEXT iteration's load_tile: a tile of compute hides the chase
        const bool has_next = live(n_next);
        if (has_next) load_tile(n_next);

        const int k0 = n_cur * BLOCK_N;
        // wave-uniform tile classification, fwd_kernel's
        bool skip = !wave_active || !live(n_cur);
        bool need_mask = (k0 + BLOCK_N > sk);
        if (p.window_right >= 0) {
            skip = skip || (k0 > wrow + 31 + shift + p.window_right);
            need_mask = need_mask || (k0 + BLOCK_N - 1 > wrow + shift + p.window_right);
        }
        if (p.window_left >= 0) {
            skip = skip || (k0 + BLOCK_N - 1 < wrow + shift - p.window_left);
            need_mask = need_mask || (k0 < wrow + 31 + shift - p.window_left);
        }

        if (!skip) {
            const char *kbuf = smem + cur * TILE_BYTES;
            const char *vbuf = smem + (2 + cur) * TILE_BYTES;

            // ---- S^T = K.Q^T : two 32-key blocks ------------------------------------------------
            f32x16 s[2];
            zero_scores(s);
            if constexpr (Q_IN_AGPR) {
#pragma unroll
                for (int ks = 0; ks < KSTEPS; ++ks) {
                    const int off = kbase ^ (32 * ks);
                    const u32x4 kf0 = *(const u32x4 *)(kbuf + off);
                    const u32x4 kf1 = *(const u32x4 *)(kbuf + off + 32 * D * 2);
                    Elem<T>::mma_qa(s[0], kf0, qf[ks]);
                    Elem<T>::mma_qa(s[1], kf1, qf[ks]);
                }
                asm volatile("s_nop 15\n\ts_nop 7" : "+v"(s[0]), "+v"(s[1]));  // asm MFMA results -> VALU
            } else {
                scores_16<T, D>(kbuf, kbase, qf, s);
            }

            if constexpr (SOFTCAP) softcap_scores(s, sc);

            // ---- the call's own mask (boundary tiles only) ------------------------------------------
            if (need_mask) {
                int lim_hi = sk;  // exclusive
                int lim_lo = 0;   // inclusive
                if (p.window_right >= 0) lim_hi = min(sk, my_row + shift + p.window_right + 1);
                if (p.window_left >= 0) lim_lo = max(0, my_row + shift - p.window_left);
                mask_scores(s, k0, hh, lim_lo, lim_hi);
            }

            u32x4 pf[4];  // online softmax (per lane = per query row), then O^T += V^T.P^T
            softmax_step<T, DBLOCKS>(s, m_run, l_run, o_acc, sc, pf);
#pragma unroll
            for (int db = 0; db < DBLOCKS; ++db) pv_16<T, D * 2>(vbuf, vbase, db, pf, o_acc[db]);
        }

        if (has_next) store_tile(cur ^ 1);
        __syncthreads();
        n_cur = n_next;
        n_next = n_after;
    }

    // ---- epilogue (fwd_kernel's): normalise, sink, LSE, O^T regs -> LDS -> coalesced rows -------------------------------
    const float l_tot = half_swap_sum(l_run);
    const bool empty = (l_tot == 0.f) || (l_tot != l_tot);
    float inv = empty ? 1.f : 1.f / l_tot;
    float lse_row = empty ? INFINITY : m_run * sc.scale + __logf(l_tot);
    if (p.sink)
        sink_finalize(my_row < sq ? load_sink(p, head, my_row) : -INFINITY, m_run * sc.scale, l_tot, empty, inv, lse_row);
    if (wave_active) {
        if (hh == 0 && my_row < sq) p.lse[lse_base + my_row] = lse_row;
        char *obuf = smem + wave * (32 * O_ROW_BYTES);
        stage_o_rows<T, D>(obuf, r, hh, o_acc, inv);
    }
    __syncthreads();
    if (wave_active) {
        const char *obuf = smem + wave * (32 * O_ROW_BYTES);
        constexpr int NCH = (32 * CH_PER_ROW) / 64;
        u32x4 val[NCH];
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = lane + i * 64;
            val[i] = *(const u32x4 *)(obuf + (c / CH_PER_ROW) * O_ROW_BYTES + (c % CH_PER_ROW) * 16);
        }
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = lane + i * 64;
            const int row = c / CH_PER_ROW, ch = c % CH_PER_ROW;
            if (wrow + row < sq && ch * 8 < p.dv) *(u32x4 *)(op + (int64_t)(wrow + row) * p.o_row_stride + ch * 8) = val[i];
        }
    }
}

}  // namespace fa
