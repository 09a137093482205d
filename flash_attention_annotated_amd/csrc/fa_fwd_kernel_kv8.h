// fa_fwd_kernel_kv8.h — gfx950 forward of 16-bit queries over an fp8 (OCP e4m3fn) KV cache: `kv_cache_dtype = fp8` of a
// serving stack.  q and o are bf16 / fp16; K and V are read from HBM as bytes, sit in LDS as bytes (half the traffic and half
// the LDS of the 16-bit tile) and are converted to T on the way to the MFMA operands.  The conversion is exact -- every finite
// e4m3fn value, subnormals and -0 included, is a bf16 and an fp16 value -- so both products are the 16-bit MFMAs with fp32
// accumulation and the kernel computes what the 16-bit kernels compute on the expanded cache.
//
// Work shape: pk_fwd_kernel's (fa_fwd_kernel_pk.h).  The rows of a workgroup are (query row, head of the GQA group) pairs of
// ONE kv head, 4 waves x 32 rows, 64-key tiles double-buffered in LDS: K / V stream once per kv head whatever h / h_k is
// (h == h_k: one head per workgroup).  Dense caches (seqused_k, kv_batch_idx, leftpad_k), paged caches (pages that are multiples
// of 64 keys resolve one page per tile, any other size one page per staged row), dense and ragged queries, causal / both window
// sides, softcap, split-KV.
//
// What differs from pk_fwd_kernel:
//   * LDS tile image: [64 keys][D bytes], 16-byte chunk c of key row at row * D + 16 * (c ^ kv8_swz<D>(row)).  The swizzle keeps
//     the ds_read_b128 row reads of K (16 rows per lane group, one chunk each) and the ds_read_b64_tr_b8 transposed reads of V
//     (8 rows x 32 bytes per 32 lanes) on distinct banks.
//   * K operand: a lane reads 16 contiguous bytes of its key row -- head-dim columns 32 j + 16 hh + [0, 16) -- and feeds them to
//     TWO k-steps of S^T = K.Q^T, 8 columns each.  The product contracts over the head dim, so the order is free as long as Q
//     agrees: the lane's Q fragments of k-steps 2 j and 2 j + 1 are columns 32 j + 16 hh + [0, 8) and + [8, 16).
//   * V operand: one ds_read_b64_tr_b8 per (32 columns, 16 keys) gives the lane the 8 keys its P^T fragment holds (the lane
//     pair 2 k, 2 k + 1 of a 16-lane group addresses key (k & 3) + 8 (k >> 2) + 4 hh of the step: the accumulator's key order).
//   * e4m3 -> T: v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0, two elements per instruction.
//   * k_descale[b, h_k] multiplies the score scale (under softcap: the factor in front of the tanh), v_descale[b, h_k] the final
//     normalisation; q_descale is not read (q is not quantised).
//   * split-KV partials follow fa_fwd_combine's convention (the merge is that entry point): a part without a visible key writes
//     LSE = -inf and carries no weight; a row without a visible key in ANY part writes +inf in every part, which the merge turns
//     into O = 0, LSE = +inf -- what the unsplit kernel writes.
// 64-bit addressing: every tile is addressed from a 64-bit base that is rebuilt per tile (cache entry or page, first key row of
// the tile, kv head); the lane offset inside a tile is below 64 row strides, and the host keeps the row stride below 2^24 bytes.
// A cache entry of 2 GiB or more is therefore read correctly; nothing is refused for its extent.
// No sink, ALiBi, dropout, attention_chunk, qv or V head dim of its own (fa_fwd_kv8_validate).
#pragma once

#include "fa_fwd_kernel_pk.h"

namespace fa {

typedef int kv8_i32x2 __attribute__((ext_vector_type(2)));

// byte offset of 16-byte chunk `ch` of key row `row` in a [64][D]-byte tile
template <int D>
__device__ __forceinline__ int kv8_off(int row, int ch) {
    if constexpr (D == 64) {
        const int s = (((row >> 3) & 1) << 1) | ((row >> 2) & 1);
        return row * 64 + 16 * (ch ^ s);
    } else {
        const int s = (((row >> 3) & 1) << 2) | (row & 2) | ((row >> 2) & 1);
        return row * 128 + 16 * (ch ^ s);
    }
}

// two e4m3 bytes (the low or the high half of w) -> two T, packed
template <typename T> struct Kv8Cvt;
template <> struct Kv8Cvt<__bf16> {
    template <bool HI> static __device__ __forceinline__ uint32_t pk(uint32_t w) {
        return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
    }
};
template <> struct Kv8Cvt<_Float16> {
    template <bool HI> static __device__ __forceinline__ uint32_t pk(uint32_t w) {
        return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, HI));
    }
};
// eight e4m3 bytes -> one MFMA operand of eight T
template <typename T>
__device__ __forceinline__ u32x4 kv8_expand(uint32_t lo, uint32_t hi) {
    u32x4 f;
    f[0] = Kv8Cvt<T>::template pk<false>(lo);
    f[1] = Kv8Cvt<T>::template pk<true>(lo);
    f[2] = Kv8Cvt<T>::template pk<false>(hi);
    f[3] = Kv8Cvt<T>::template pk<true>(hi);
    return f;
}

template <int D>
constexpr int smem_bytes_kv8() {
    constexpr int tiles = 4 * BLOCK_N * D, epilogue = PK_NWAVES * 32 * (D * 2 + 16);
    return tiles > epilogue ? tiles : epilogue;
}

template <typename T, int D, bool SOFTCAP>
__global__ __launch_bounds__(PK_NWAVES * 64, 2) void kv8_fwd_kernel(const PkParams pa) {
    const KParams &p = pa.p;
    constexpr int NT = PK_NWAVES * 64;
    constexpr int KSTEPS = D / 16;
    constexpr int DBLOCKS = D / 32;
    constexpr int CH_PER_ROW = D / 16;         // 16-byte chunks of a key row
    constexpr int TILE_BYTES = BLOCK_N * D;
    constexpr int CHUNKS = BLOCK_N * CH_PER_ROW;
    constexpr int LD_PER_THREAD = CHUNKS / NT;
    static_assert(CHUNKS % NT == 0, "tile must divide over the workgroup");
    constexpr int O_ROW_BYTES = D * 2 + 16;    // padded epilogue row; the padding carries the row's O offset

    extern __shared__ __attribute__((aligned(16))) char smem[];
    // [K0 | K1 | V0 | V1]; the epilogue reuses the region as PK_NWAVES x [32][O_ROW_BYTES] (smem_bytes_kv8 holds the larger)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int hh = lane >> 5;

    // ---- work item (pk_fwd_kernel's) ---------------------------------------------------------------------------------------
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int group = (slot / pa.num_pblocks) * 8 + xcd, pb = slot % pa.num_pblocks;
    if (group >= pa.num_groups) return;  // whole workgroup (padding)
    const int splits = p.num_splits > 1 ? p.num_splits : 1;
    const int unit = group / splits, split = group % splits;
    const int batch = unit / p.h_k, kv_head = unit % p.h_k;
    const int g = p.h_ratio;

    // ---- sequence bookkeeping ----------------------------------------------------------------------------------------------
    int sq, sk, q0 = 0;
    if (p.cu_seqlens_q) {
        q0 = p.cu_seqlens_q[batch];
        sq = p.seqused_q ? p.seqused_q[batch] : p.cu_seqlens_q[batch + 1] - q0;
    } else {
        sq = p.seqused_q ? p.seqused_q[batch] : p.seqlen_q;
    }
    sk = p.seqused_k ? p.seqused_k[batch] : p.seqlen_k;
    sk = min(sk, p.seqlen_k);  // never past the capacity
    const int kv_batch = p.kv_batch_idx ? p.kv_batch_idx[batch] : batch;
    int64_t k_base = (int64_t)kv_batch * p.k_batch_stride;
    int64_t v_base = (int64_t)kv_batch * p.v_batch_stride;
    const int prows = sq * g;  // packed rows of this (batch, kv head); the host keeps seqlen_q * g below 2^31
    const int pr_lo = pb * PK_BLOCK_M;
    if (pr_lo >= prows) return;  // whole workgroup: nothing to do (ragged / padded grid)
    if (p.leftpad_k) {
        const int lp = p.leftpad_k[batch];
        sk = max(sk - lp, 0);
        k_base += (int64_t)lp * p.k_row_stride;
        v_base += (int64_t)lp * p.v_row_stride;
    }
    if (p.block_table) k_base = v_base = 0;  // paged: the page supplies the batch offset
    const int32_t *pages = p.block_table ? p.block_table + (int64_t)batch * p.bt_bs : nullptr;
    const uint8_t *kp = (const uint8_t *)p.k + k_base + (int64_t)kv_head * p.k_head_stride;
    const uint8_t *vp = (const uint8_t *)p.v + v_base + (int64_t)kv_head * p.v_head_stride;
    const Scales sc = load_scales(p, batch, kv_head);  // (q_descale is NULL here)

    // ---- the wave's packed rows, the lane's query row and head -----------------------------------------------------------------
    const int wpr = pr_lo + wave * 32;            // first packed row of this wave
    const bool wave_active = wpr < prows;
    const int wq_lo = wpr / g;                    // first and last query row of the wave (inclusive)
    const int wq_hi = min(prows - 1, wpr + 31) / g;
    const int pr = wpr + r;
    const bool row_ok = pr < prows;
    const int prc = min(pr, prows - 1);
    const int my_row = prc / g;                   // the query row this lane owns (masks)
    const int head = kv_head * g + (prc - my_row * g);
    const int64_t row_g = (int64_t)q0 + my_row;   // row of q / o (ragged: in the whole batch)
    const int64_t bq = p.cu_seqlens_q ? 0 : batch;

    // ---- key range of this block: from its first and last query row --------------------------------------------------------
    const int shift = sk - sq;  // bottom-right aligned masks
    const int qr_lo = pr_lo / g, qr_hi = min(prows - 1, pr_lo + PK_BLOCK_M - 1) / g;
    int key_hi = sk, key_lo = 0;
    if (p.window_right >= 0) key_hi = min(sk, qr_hi + 1 + shift + p.window_right);
    if (p.window_left >= 0) key_lo = max(0, qr_lo + shift - p.window_left);
    int n_min = key_lo / BLOCK_N;
    int n_max = key_hi > 0 ? (key_hi + BLOCK_N - 1) / BLOCK_N : 0;
    split_range(p, split, n_min, n_max);

    // the lane's own key range [lim_lo, lim_hi): the element mask, and whether the row sees a key at all
    int lim_hi = sk, lim_lo = 0;
    if (p.window_right >= 0) lim_hi = min(sk, my_row + shift + p.window_right + 1);
    if (p.window_left >= 0) lim_lo = max(0, my_row + shift - p.window_left);

    // ---- Q fragments: B operand of S^T = K.Q^T; k-step 2 j + e of lane (r, hh) is Q[row][32 j + 16 hh + 8 e .. + 8] -- the
    // columns its 16 K bytes of chunk 2 j + hh hold (branch-free, zeroed by selects)
    u32x4 qf[KSTEPS];
    {
        const T *qr = (const T *)p.q + bq * p.q_batch_stride + row_g * p.q_row_stride + (int64_t)head * p.q_head_stride;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const int d0 = (ks >> 1) * 32 + hh * 16 + (ks & 1) * 8;
            qf[ks] = *(const u32x4 *)(qr + (d0 < p.d ? d0 : 0));
        }
        const u32x4 z4 = {0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) qf[ks] = ((ks >> 1) * 32 + hh * 16 + (ks & 1) * 8 < p.d && row_ok) ? qf[ks] : z4;
    }

    f32x16 o_acc[DBLOCKS];
#pragma unroll
    for (int db = 0; db < DBLOCKS; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) o_acc[db][i] = 0.f;
    float m_run = -INFINITY;  // running row max (unscaled scores), same in both lane halves
    float l_run = 0.f;        // running row sum, PARTIAL per lane half (combined in the epilogue)

    // ---- K/V staging: 16 bytes = 16 head-dim columns per load (clamped rows / chunks: the duplicates are masked or meet zero
    // Q columns; every staged byte comes from a valid key row) ----------------------------------------------------------------
    u32x4 kreg[LD_PER_THREAD], vreg[LD_PER_THREAD];
    static_assert(NT % CH_PER_ROW == 0, "a pass of the workgroup covers whole rows");
    constexpr int ROWS_PER_PASS = NT / CH_PER_ROW;
    const int ld_row0 = tid / CH_PER_ROW;
    const int ld_col0 = ((tid % CH_PER_ROW) * 16 < p.d) ? (tid % CH_PER_ROW) * 16 : 0;
    const int k_rs = (int)p.k_row_stride, v_rs = (int)p.v_row_stride;  // host guarantees 64 * stride < 2^31
    auto load_tile = [&](int n) {
        const int k0 = n * BLOCK_N;
        const uint8_t *kt = kp + (int64_t)k0 * p.k_row_stride;  // 64-bit base of the tile
        const uint8_t *vt = vp + (int64_t)k0 * p.v_row_stride;
        const int last = sk - 1 - k0;                     // >= 0 for every tile in [n_min, n_max)
        if (pages) {
            if (p.page_size % BLOCK_N == 0) {  // a 64-key tile lies inside one page
                const int page = pages[k0 / p.page_size], in_page = k0 % p.page_size;
                kt = kp + (int64_t)page * p.k_batch_stride + (int64_t)in_page * p.k_row_stride;
                vt = vp + (int64_t)page * p.v_batch_stride + (int64_t)in_page * p.v_row_stride;
            } else {  // any other page size: the page is looked up per row
#pragma unroll
                for (int i = 0; i < LD_PER_THREAD; ++i) {
                    const int row = k0 + min(ld_row0 + i * ROWS_PER_PASS, last);
                    const int pi = row / p.page_size;
                    const int64_t page = pages[pi];
                    const int in_page = row - pi * p.page_size;
                    kreg[i] = *(const u32x4 *)(kp + page * p.k_batch_stride + (int64_t)in_page * p.k_row_stride + ld_col0);
                    vreg[i] = *(const u32x4 *)(vp + page * p.v_batch_stride + (int64_t)in_page * p.v_row_stride + ld_col0);
                }
                return;
            }
        }
#pragma unroll
        for (int i = 0; i < LD_PER_THREAD; ++i) {
            const int row = min(ld_row0 + i * ROWS_PER_PASS, last);
            kreg[i] = *(const u32x4 *)(kt + (uint32_t)(row * k_rs + ld_col0));
            vreg[i] = *(const u32x4 *)(vt + (uint32_t)(row * v_rs + ld_col0));
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < LD_PER_THREAD; ++i) {
            const int c = tid + i * NT;
            const int off = kv8_off<D>(c / CH_PER_ROW, c % CH_PER_ROW);
            *(u32x4 *)(smem + buf * TILE_BYTES + off) = kreg[i];
            *(u32x4 *)(smem + (2 + buf) * TILE_BYTES + off) = vreg[i];
        }
    };

    // lane-constant pieces of the LDS read addresses
    //   K: chunk 2 j + hh of key row r (+ 32): kbase ^ (32 j) (+ 32 D)
    //   V: lane pair k = i16 >> 1 of 16-lane group g1 addresses key (k & 3) + 8 (k >> 2) + 4 hh (+ 16 st), columns
    //      32 db + 16 g1 + 8 (i16 & 1) .. + 8: vbase ^ (32 db) (+ 16 st D).  Rows + 16 st and + 32 leave the swizzle alone.
    const int i16 = lane & 15;
    const int g1 = (lane >> 4) & 1;
    const int kbase = kv8_off<D>(r, hh);
    const int vk = i16 >> 1;
    const int vbase = kv8_off<D>((vk & 3) + 8 * (vk >> 2) + 4 * hh, g1) + 8 * (i16 & 1);

    if (n_min < n_max) {
        load_tile(n_min);
        store_tile(0);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): Q retired here, not in front of the first MFMA of every tile
    __syncthreads();

    for (int n = n_min; n < n_max; ++n) {
        const int cur = (n - n_min) & 1;
        const bool has_next = (n + 1 < n_max);
        if (has_next) load_tile(n + 1);

        const int k0 = n * BLOCK_N;
        // wave-uniform tile classification from the wave's first and last query row
        bool skip = !wave_active;
        bool need_mask = (k0 + BLOCK_N > sk);
        if (p.window_right >= 0) {
            skip = skip || (k0 > wq_hi + shift + p.window_right);
            need_mask = need_mask || (k0 + BLOCK_N - 1 > wq_lo + shift + p.window_right);
        }
        if (p.window_left >= 0) {
            skip = skip || (k0 + BLOCK_N - 1 < wq_lo + shift - p.window_left);
            need_mask = need_mask || (k0 < wq_hi + shift - p.window_left);
        }

        if (!skip) {  // (wave-uniform: EXEC is full at the transposed reads below)
            const char *kbuf = smem + cur * TILE_BYTES;
            const char *vbuf = smem + (2 + cur) * TILE_BYTES;

            // ---- S^T = K.Q^T : two 32-key blocks, 16 K bytes = two k-steps ----------------------------------------------------
            f32x16 s[2];
#pragma unroll
            for (int i = 0; i < 16; ++i) { s[0][i] = 0.f; s[1][i] = 0.f; }
#pragma unroll
            for (int j = 0; j < KSTEPS / 2; ++j) {
                const int off = kbase ^ (32 * j);  // = kv8_off<D>(r, 2 j + hh)
                const u32x4 kb0 = *(const u32x4 *)(kbuf + off);
                const u32x4 kb1 = *(const u32x4 *)(kbuf + off + 32 * D);
                s[0] = Elem<T>::mma(kv8_expand<T>(kb0[0], kb0[1]), qf[2 * j], s[0]);
                s[1] = Elem<T>::mma(kv8_expand<T>(kb1[0], kb1[1]), qf[2 * j], s[1]);
                s[0] = Elem<T>::mma(kv8_expand<T>(kb0[2], kb0[3]), qf[2 * j + 1], s[0]);
                s[1] = Elem<T>::mma(kv8_expand<T>(kb1[2], kb1[3]), qf[2 * j + 1], s[1]);
            }

            if constexpr (SOFTCAP) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) s[kb][i] = fast_tanh(s[kb][i] * sc.softcap_pre);
            }

            // ---- mask (boundary tiles only): the lane's QUERY row ----------------------------------------------------------
            if (need_mask) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int key = k0 + kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
                        if (key >= lim_hi || key < lim_lo) s[kb][i] = -INFINITY;
                    }
            }

            // ---- online softmax (per lane = per packed row) ---------------------------------------------------------------
            float mx = max3(s[0][0], s[1][0], m_run);
#pragma unroll
            for (int i = 1; i < 16; ++i) mx = max3(mx, s[0][i], s[1][i]);
            const float m_new = half_swap_max(mx);  // >= m_run (m_run is identical in both halves)
            const float m_use = (m_new == -INFINITY) ? 0.f : m_new;  // fully masked so far
            const float mc = m_use * sc.scale_log2;
            if (__any(m_new > m_run)) {  // wave-uniform; bit-identical to always rescaling
                const float alpha = __builtin_amdgcn_exp2f(m_run * sc.scale_log2 - mc);
                l_run *= alpha;
#pragma unroll
                for (int db = 0; db < DBLOCKS; ++db)
#pragma unroll
                    for (int i = 0; i < 16; ++i) o_acc[db][i] *= alpha;
            }
            m_run = m_new;
            float psum = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float pv = __builtin_amdgcn_exp2f(s[kb][i] * sc.scale_log2 - mc);
                    s[kb][i] = pv;
                    psum += pv;
                }
            l_run += psum;

            // ---- P^T fragments: accumulator registers ARE the B operand of O^T += V^T.P^T ------------------------------------
            u32x4 pf[4];
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const int kb = st >> 1, b8 = (st & 1) * 8;
#pragma unroll
                for (int j = 0; j < 4; ++j) pf[st][j] = Elem<T>::pack2(s[kb][b8 + 2 * j], s[kb][b8 + 2 * j + 1]);
            }

            // ---- O^T += V^T.P^T : one transposed 8-byte read per (32 columns, 16 keys) ------------------------------------------
#pragma unroll
            for (int db = 0; db < DBLOCKS; ++db) {
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    const int off = (vbase ^ (32 * db)) + 16 * st * D;
                    const kv8_i32x2 t = __builtin_amdgcn_ds_read_tr8_b64_v2i32(
                        (__attribute__((address_space(3))) kv8_i32x2 *)(vbuf + off));
                    o_acc[db] = Elem<T>::mma(kv8_expand<T>((uint32_t)t[0], (uint32_t)t[1]), pf[st], o_acc[db]);
                }
            }
        }

        if (has_next) store_tile(cur ^ 1);
        __syncthreads();
    }

    // ---- epilogue: normalise (v_descale rides in the factor), LSE, O^T regs -> LDS -> 16-byte stores of (query row, head) rows
    // (the loop's last barrier has retired every K/V read, so the region can be reused)
    const float l_tot = half_swap_sum(l_run);
    const bool empty = (l_tot == 0.f) || (l_tot != l_tot);
    const float inv = empty ? 0.f : sc.v_descale / l_tot;
    float lse_row = empty ? INFINITY : m_run * sc.scale + __logf(l_tot);  // +inf for rows with no valid key, as fwd_kernel
    // a part of a split that holds none of the row's keys: no weight in fa_fwd_combine (-inf); a row without any key keeps +inf
    if (p.num_splits > 1 && empty && lim_lo < lim_hi) lse_row = -INFINITY;
    const int64_t o_off = bq * p.o_batch_stride + row_g * p.o_row_stride + (int64_t)head * p.o_head_stride;
    if (wave_active) {
        if (hh == 0 && row_ok) {
            const int64_t li = p.cu_seqlens_q ? (int64_t)head * p.total_q + row_g : ((int64_t)batch * p.h + head) * p.seqlen_q + my_row;
            p.lse[li + split * p.lse_split_stride] = lse_row;
        }
        if (p.num_splits > 1) {
            // split-KV partial: fp32 in the caller's workspace, straight from the accumulators (fwd_kernel's layout)
            float *opf = (float *)p.o + split * p.o_split_stride + o_off;
            if (row_ok) {
#pragma unroll
                for (int db = 0; db < DBLOCKS; ++db)
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) {
                        const int col = db * 32 + 8 * g4 + 4 * hh;
                        if (col < p.d)
                            *(float4 *)(opf + col) = make_float4(o_acc[db][4 * g4] * inv, o_acc[db][4 * g4 + 1] * inv,
                                                                 o_acc[db][4 * g4 + 2] * inv, o_acc[db][4 * g4 + 3] * inv);
                    }
            }
        } else {
            char *obuf = smem + wave * (32 * O_ROW_BYTES);
#pragma unroll
            for (int db = 0; db < DBLOCKS; ++db)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    u32x2 w;
                    w[0] = Elem<T>::pack2(o_acc[db][4 * g4] * inv, o_acc[db][4 * g4 + 1] * inv);
                    w[1] = Elem<T>::pack2(o_acc[db][4 * g4 + 2] * inv, o_acc[db][4 * g4 + 3] * inv);
                    *(u32x2 *)(obuf + r * O_ROW_BYTES + (db * 32 + 8 * g4 + 4 * hh) * 2) = w;
                }
            // the row's destination rides in the padding of its LDS row: the lanes that store a row are not the lane that owns it
            if (hh == 0) {
                *(int64_t *)(obuf + r * O_ROW_BYTES + D * 2) = o_off;
                *(int32_t *)(obuf + r * O_ROW_BYTES + D * 2 + 8) = row_ok ? 1 : 0;
            }
        }
    }
    if (p.num_splits > 1) return;  // (uniform over the launch: no wave is left waiting at the barrier below)
    __syncthreads();
    if (wave_active) {
        const char *obuf = smem + wave * (32 * O_ROW_BYTES);
        // (LDS reads outside the predicate: all of them are issued before the first store)
        constexpr int OCH = D / 8;  // 16-byte chunks of an O row
        constexpr int NCH = (32 * OCH) / 64;
        u32x4 val[NCH];
        int64_t dst[NCH];
        int32_t ok[NCH];
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = lane + i * 64;
            const char *row = obuf + (c / OCH) * O_ROW_BYTES;
            val[i] = *(const u32x4 *)(row + (c % OCH) * 16);
            dst[i] = *(const int64_t *)(row + D * 2);
            ok[i] = *(const int32_t *)(row + D * 2 + 8);
        }
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int ch = (lane + i * 64) % OCH;
            if (ok[i] && ch * 8 < p.d) *(u32x4 *)((T *)p.o + dst[i] + ch * 8) = val[i];
        }
    }
}

}  // namespace fa
