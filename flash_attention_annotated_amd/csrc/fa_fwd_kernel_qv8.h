// fa_fwd_kernel_qv8.h — gfx950 forward of the MLA decode shape over an fp8 (OCP e4m3fn) KV cache: 16-bit q / qv / o, q/k head
// dim <= 64 beside a V / latent head dim in [256, 512], K and V read from HBM as bytes (fa_fwd_qv8, include/fa_fwd.h).
//
// qv8_fwd_kernel joins two kernels that exist: the work shape of fwd_kernel_qv (fa_fwd_kernel_qv.h) and the byte tile of
// kv8_fwd_kernel (fa_fwd_kernel_kv8.h).
//   * from fwd_kernel_qv: 4 waves, 32 packed (query row, head of the GQA group) rows of one kv head per workgroup, 64-key
//     tiles, the work-item decode, the key range and the workgroup-uniform tile classification; the score contraction split
//     over the waves (wave w: K k-step w and V columns [w DVT/4, (w+1) DVT/4)), the four partial S^T tiles summed from LDS in
//     wave order so that every wave holds bit-identical scores; wave w accumulates O^T for its DVT/4 columns; dense and paged
//     staging (pages that are multiples of 64 keys resolve one page per tile, any other size one page per staged row).
//   * from kv8: kv8_expand<T> (the exact e4m3 -> T conversion between LDS and the MFMA operand), kv8_off<64> (the K image),
//     Kv8::q_col (a 16-byte row read feeds two k-steps, so Q agrees on the column order) and Kv8::pv (one ds_read_b64_tr_b8
//     per (32 columns, 16 keys)), here with row stride DVT.
//   * from fa_fwd_tile_step.h: softcap, the element mask, softmax_step, the pack2 of P^T and the split-partial store.
// No cu_seqlens_k, attention_chunk, sink, ALiBi or dropout (fa_fwd_qv8_validate).  qa.qv == NULL: the same shape without the
// second score product (a lane-uniform flag, as in fwd_kernel_qv).
//
// What this file owns:
//
// The tile in bytes.  K is [64 keys][64 bytes] at kv8_off<64>, V is [64 keys][DVT bytes] at qv8_voff<DVT> below.
//
// The V image, derived.  A V row is 256 or 512 bytes: a whole number of 256-byte bank rows, so without a swizzle chunk c of
// every key row sits on the same four banks.  The 16-byte chunk c of key row `row` is stored at
//     row * DVT + 16 * (c ^ s(row)),   s(row) = b2 | b0 << 1 | b1 << 2 | b3 << 3   (b_i = bit i of row),
// which moves bits 0-3 of the chunk index only: the 16-byte slot of the bank row is (c ^ s) & 15, bit 4 of c (DVT 512) picks
// the 256-byte half and never the bank.  Two read patterns have to stay on distinct banks (bank of byte a = (a / 4) % 64 for
// both instructions):
//   (a) ds_read_b128 of the score product: lane (r, hh) reads chunk c0 + hh of key row r.  The hardware serves the lanes in
//       four groups of 16, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32: one chunk, 16 key rows.  By
//       (b4 b3 b2) the rows of the first group are {000, 011, 101, 110} and of the second {001, 010, 100, 111}, each with
//       every (b1 b0).  Inside a group b3 and b2 take all four pairs once, so s, which holds b0 b1 b2 b3, takes 16 different
//       values: 16 different slots.
//   (b) ds_read_b64_tr_b8 of the PV product: the 32 lanes of a half read 8 key rows x 32 bytes, rows a + {0-3, 8-11}
//       (a = 4 hh + 16 st) x chunks {2 db, 2 db + 1}, two lanes per chunk on its two 8-byte halves.  Over these rows
//       b0 b1 b3 take all eight values and b2 is fixed: s >> 1 takes eight different values, and (c ^ s) & 15 with the two
//       values of c's bit 0 sixteen.
//   s does not read b4 or b5, so the operand addresses of key rows + 16 st and + 32 are the lane's base plus a constant, and
//   a column block is an XOR on the base (Kv8::pv's arithmetic).
// These counts are COMPUTED from the bank rules, for ds_read_b64_tr_b8 under the rule measured for ds_read_b64_tr_b16 (two
// groups of 32 lanes); they are not counted on the device.  A different rule costs LDS cycles, never a result.
//
// The K product.  K has four k-steps of 16 columns, one 16-byte chunk each, and a 16-byte read would feed two of them: two
// waves would carry all of K.  Instead every wave takes one k-step, as in fwd_kernel_qv, and reads 8 bytes of the chunk
// (ds_read_b64: chunk `wave`, half hh = Q columns 16 wave + 8 hh + [0, 8)): the MFMAs between two barriers stay equal over
// the waves (2 + 16 + 16 at DVT 512), at the price of a 2-way conflict of that one read (kv8_off<64> does not read b4, so
// key rows r and r + 16 of a 32-lane group meet: 4 LDS cycles instead of 2, twice per tile, beside ~64 for V).
//
// The V score product.  Lane (r, hh) reads chunk (DVT / 64) wave + 2 j + hh of key row r and r + 32 and feeds each 16-byte
// read to k-steps 2 j and 2 j + 1; the lane's Qv fragment of k-step ks holds columns (DVT / 4) wave + Kv8::q_col(ks, hh).
//
// Descales, in fp32 on the products: S = (kd . Q.K8^T + vd . Qv.V8^T) . scale, O = vd . P.V8 / l, kd = k_descale[b, h_k],
// vd = v_descale[b, h_k] (NULL = 1; q_descale is not read).  The two score terms carry different factors, so a wave keeps its
// K product and its V product in accumulators of their own and joins them as kd sK + vd sV when the partial goes to LDS.  The
// Scales of the softmax are built here, not by load_scales: k_descale must not enter a second time.  Under softcap both
// factors therefore act in front of the tanh.  vd / l_tot is the final normalisation, as in kv8.
//
// Staging: a double buffer.  At DVT 512 a tile is 4 + 32 KiB; two of them and the 32 KiB of partial scores are 104 KiB of the
// CU's 160.  fwd_kernel_qv keeps one buffer because two 16-bit tiles (144 KiB) and the partials do not fit: it pays a second
// barrier per tile, with every wave idle while the next tile's registers go to LDS.  Here the next tile is loaded into
// registers in front of the compute (36 VGPRs at DVT 512, half the 16-bit kernel's), stored to the other buffer behind it,
// and one barrier ends the tile.  One workgroup per CU as today (launch bounds 256, 1), no scratch.
//
// 64-bit addressing, as kv8: a tile is addressed from a 64-bit base that is rebuilt per tile (cache entry or page, first key
// row, kv head); the lane offset is 32-bit, below 64 row strides, and the host keeps the row stride below 2^24 bytes.
//
// Empty parts and rows follow fa_fwd_combine's convention exactly as kv8 does: a split part without a visible key of the row
// writes LSE = -inf; a row without a visible key in any part writes +inf in every part; unsplit that row gets O = 0 and
// LSE = +inf.  seqused_k is clamped to the capacity.
#pragma once

#include "fa_fwd_kernel_kv8.h"
#include "fa_fwd_kernel_qv.h"

namespace fa {

// byte offset of 16-byte chunk `ch` of key row `row` in the [64][DVT]-byte V tile (derivation above)
template <int DVT>
__device__ __forceinline__ int qv8_voff(int row, int ch) {
    const int s = ((row >> 2) & 1) | ((row & 3) << 1) | (((row >> 3) & 1) << 3);
    return row * DVT + 16 * (ch ^ s);
}

template <int DVT>
constexpr int smem_bytes_qv8() {
    return 2 * BLOCK_N * 64 + 2 * BLOCK_N * DVT + QV_NWAVES * 32 * 64 * 4;  // K0 K1 | V0 V1 | partial scores
}

template <typename T, int DVT, bool SOFTCAP>
__global__ __launch_bounds__(QV_NWAVES * 64, 1) void qv8_fwd_kernel(const QvParams qa) {
    typedef Kv8<T, DVT> Tile;  // q_col and pv: neither reads the K image
    const KParams &p = qa.p;
    constexpr int NT = QV_NWAVES * 64;
    constexpr int CPW = DVT / QV_NWAVES;       // V / O columns (= bytes of a V row) per wave
    constexpr int KSV = CPW / 16;              // Qv k-steps per wave
    constexpr int DBW = CPW / 32;              // O^T row blocks per wave = 16-byte score reads per wave and key block
    constexpr int K_BYTES = BLOCK_N * 64;
    constexpr int V_BYTES = BLOCK_N * DVT;
    constexpr int CHK = 64 / 16, CHV = DVT / 16;  // 16-byte chunks per K / V row
    constexpr int LDK = BLOCK_N * CHK / NT, LDV = BLOCK_N * CHV / NT;
    constexpr int RPK = NT / CHK, RPV = NT / CHV;  // rows per pass of the workgroup
    static_assert(DVT == 256 || DVT == 512, "the V image is derived for whole bank rows");
    static_assert(LDK == 1 && LDV >= 1 && DBW >= 1 && KSV == 2 * DBW, "tile shape");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *sred = smem + 2 * K_BYTES + 2 * V_BYTES;  // [wave][8][64 lanes] float4

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int hh = lane >> 5;

    // ---- work item (fwd_kernel_qv's decode) --------------------------------------------------------------------------
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int group = (slot / qa.num_pblocks) * 8 + xcd, pb = slot % qa.num_pblocks;
    if (group >= qa.num_groups) return;  // whole workgroup (padding)
    const int splits = p.num_splits > 1 ? p.num_splits : 1;
    const int unit = group / splits, split = group % splits;
    const int batch = unit / p.h_k, kv_head = unit % p.h_k;
    const int g = p.h_ratio;

    int sq, q0 = 0;
    if (p.cu_seqlens_q) {
        q0 = p.cu_seqlens_q[batch];
        sq = p.seqused_q ? p.seqused_q[batch] : p.cu_seqlens_q[batch + 1] - q0;
    } else {
        sq = p.seqused_q ? p.seqused_q[batch] : p.seqlen_q;
    }
    int sk = min(p.seqused_k ? p.seqused_k[batch] : p.seqlen_k, p.seqlen_k);  // a cache: never past the capacity
    const int kv_batch = p.kv_batch_idx ? p.kv_batch_idx[batch] : batch;
    int64_t k_base = (int64_t)kv_batch * p.k_batch_stride, v_base = (int64_t)kv_batch * p.v_batch_stride;
    const int prows = sq * g;  // packed rows of this (batch, kv head)
    const int pr_lo = pb * 32;
    if (pr_lo >= prows) return;  // whole workgroup
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
    // descales stay factors of the fp32 products; the softmax's Scales carry the plain scale (never k_descale again)
    const float kd = p.k_descale ? p.k_descale[batch * p.kd_bs + kv_head * p.kd_hs] : 1.f;
    const float vd = p.v_descale ? p.v_descale[batch * p.vd_bs + kv_head * p.vd_hs] : 1.f;
    Scales sc;
    sc.scale = p.scale; sc.scale_log2 = p.scale_log2; sc.softcap_pre = p.softcap_pre; sc.v_descale = vd;

    // ---- the lane's packed row, its query row and head ---------------------------------------------------------------
    const int pr = pr_lo + r;
    const bool row_ok = pr < prows;
    const int prc = min(pr, prows - 1);
    const int my_row = prc / g;                       // query row (masks)
    const int head = kv_head * g + prc % g;
    const int qr_lo = pr_lo / g, qr_hi = min(prows - 1, pr_lo + 31) / g;  // query rows of the block (inclusive)

    // ---- key range of the block, and of the lane's own row (element mask; whether the row sees a key at all) ---------
    const int shift = sk - sq;
    int key_hi = sk, key_lo = 0;
    if (p.window_right >= 0) key_hi = min(sk, qr_hi + 1 + shift + p.window_right);
    if (p.window_left >= 0) key_lo = max(0, qr_lo + shift - p.window_left);
    int n_min = key_lo / BLOCK_N;
    int n_max = key_hi > 0 ? (key_hi + BLOCK_N - 1) / BLOCK_N : 0;
    split_range(p, split, n_min, n_max);
    int lim_hi = sk, lim_lo = 0;
    if (p.window_right >= 0) lim_hi = min(sk, my_row + shift + p.window_right + 1);
    if (p.window_left >= 0) lim_lo = max(0, my_row + shift - p.window_left);

    // ---- Q / Qv fragments: B operands of S^T = K.Q^T + V.Qv^T.  Q: row r, columns 16 wave + 8 hh + [0, 8) (the 8 K bytes the
    // lane reads); Qv k-step ks: columns CPW wave + Tile::q_col(ks, hh) + [0, 8) (half of the 16 V bytes it reads) ------------
    const bool has_qv = qa.qv != nullptr;
    const u32x4 z4 = {0, 0, 0, 0};
    u32x4 qf, qvf[KSV];
    {
        const int64_t row_q = p.cu_seqlens_q ? (int64_t)(q0 + my_row) : (int64_t)my_row;
        const int64_t bq = p.cu_seqlens_q ? 0 : batch;
        const T *qr = (const T *)p.q + bq * p.q_batch_stride + row_q * p.q_row_stride + (int64_t)head * p.q_head_stride;
        const int c = 16 * wave + 8 * hh;
        qf = *(const u32x4 *)(qr + (c < p.d ? c : 0));
        qf = (c < p.d && row_ok) ? qf : z4;
        const T *qvr = has_qv ? (const T *)qa.qv + bq * qa.qv_batch_stride + row_q * qa.qv_row_stride +
                                    (int64_t)head * qa.qv_head_stride
                              : qr;
#pragma unroll
        for (int ks = 0; ks < KSV; ++ks) {
            const int cv = CPW * wave + Tile::q_col(ks, hh);
            qvf[ks] = *(const u32x4 *)(qvr + (has_qv && cv < p.dv ? cv : 0));
        }
#pragma unroll
        for (int ks = 0; ks < KSV; ++ks)
            qvf[ks] = (has_qv && CPW * wave + Tile::q_col(ks, hh) < p.dv && row_ok) ? qvf[ks] : z4;
    }

    f32x16 o_acc[DBW];
#pragma unroll
    for (int db = 0; db < DBW; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) o_acc[db][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    // ---- K/V staging, 16 bytes per load (clamped rows / chunks as in fwd_kernel_qv: duplicates are masked or meet zero Q
    // columns; every staged chunk comes from a valid key row).  64-bit base per tile, 32-bit lane offset ------------------
    u32x4 kreg, vreg[LDV];
    const int ldk_row0 = tid / CHK, ldv_row0 = tid / CHV;
    const int ldk_col = ((tid % CHK) * 16 < p.d) ? (tid % CHK) * 16 : 0;
    const int ldv_col = ((tid % CHV) * 16 < p.dv) ? (tid % CHV) * 16 : 0;
    const int k_rs = (int)p.k_row_stride, v_rs = (int)p.v_row_stride;  // host keeps both below 2^24: 64 * stride < 2^31
    static_assert(RPK == BLOCK_N, "one pass of the workgroup stages the K tile");
    auto load_tile = [&](int n) {
        const int k0 = n * BLOCK_N;
        const uint8_t *kt = kp + (int64_t)k0 * p.k_row_stride;
        const uint8_t *vt = vp + (int64_t)k0 * p.v_row_stride;
        const int last = sk - 1 - k0;  // >= 0 for every tile in [n_min, n_max)
        if (pages) {
            if (p.page_size % BLOCK_N == 0) {  // a 64-key tile lies inside one page
                const int page = pages[k0 / p.page_size], in_page = k0 % p.page_size;
                kt = kp + (int64_t)page * p.k_batch_stride + (int64_t)in_page * p.k_row_stride;
                vt = vp + (int64_t)page * p.v_batch_stride + (int64_t)in_page * p.v_row_stride;
            } else {  // any other page size: the page is looked up per row
                {
                    const int row = k0 + min(ldk_row0, last);
                    const int pi = row / p.page_size;
                    kreg = *(const u32x4 *)(kp + (int64_t)pages[pi] * p.k_batch_stride +
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
        kreg = *(const u32x4 *)(kt + (uint32_t)(min(ldk_row0, last) * k_rs + ldk_col));
#pragma unroll
        for (int i = 0; i < LDV; ++i) vreg[i] = *(const u32x4 *)(vt + (uint32_t)(min(ldv_row0 + i * RPV, last) * v_rs + ldv_col));
    };
    auto store_tile = [&](int buf) {
        *(u32x4 *)(smem + buf * K_BYTES + kv8_off<64>(tid / CHK, tid % CHK)) = kreg;
#pragma unroll
        for (int i = 0; i < LDV; ++i) {
            const int c = tid + i * NT;
            *(u32x4 *)(smem + 2 * K_BYTES + buf * V_BYTES + qv8_voff<DVT>(c / CHV, c % CHV)) = vreg[i];
        }
    };

    // lane-constant parts of the LDS addresses (both swizzles XOR chunk bits only and do not read row bits 4, 5)
    const int kbase = kv8_off<64>(r, wave) + 8 * hh;                   // K row r, chunk `wave`, half hh
    const int vsbase = qv8_voff<DVT>(r, hh) ^ (16 * KSV * wave);       // V row r, chunk KSV wave + hh (score reads)
    const int vi16 = lane & 15, vg1 = (lane >> 4) & 1, vk = vi16 >> 1;
    const int vbase = qv8_voff<DVT>((vk & 3) + 8 * (vk >> 2) + 4 * hh, vg1) + 8 * (vi16 & 1);  // Kv8::vbase over this image

    if (n_min < n_max) {
        load_tile(n_min);
        store_tile(0);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): Q / Qv retired here, not in front of the first MFMA of every tile
    __syncthreads();

    for (int n = n_min; n < n_max; ++n) {
        const int cur = (n - n_min) & 1;
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

        if (!skip) {  // (workgroup-uniform: the barrier inside is met by all, EXEC is full at the transposed reads)
            const char *kbuf = smem + cur * K_BYTES;
            const char *vbuf = smem + 2 * K_BYTES + cur * V_BYTES;
            // ---- partial S^T of this wave: K step `wave` and its quarter of the V columns, in accumulators of their own ----
            f32x16 s[2], sv[2];
            zero_scores(s);
            {
                const u32x2 kb0 = *(const u32x2 *)(kbuf + kbase);
                const u32x2 kb1 = *(const u32x2 *)(kbuf + kbase + 32 * 64);
                s[0] = Elem<T>::mma(kv8_expand<T>(kb0[0], kb0[1]), qf, s[0]);
                s[1] = Elem<T>::mma(kv8_expand<T>(kb1[0], kb1[1]), qf, s[1]);
            }
            if (has_qv) {
                zero_scores(sv);
#pragma unroll
                for (int j = 0; j < DBW; ++j) {
                    const int off = vsbase ^ (32 * j);  // = qv8_voff<DVT>(r, KSV wave + 2 j + hh)
                    const u32x4 vb0 = *(const u32x4 *)(vbuf + off);
                    const u32x4 vb1 = *(const u32x4 *)(vbuf + off + 32 * DVT);
                    sv[0] = Elem<T>::mma(kv8_expand<T>(vb0[0], vb0[1]), qvf[2 * j], sv[0]);
                    sv[1] = Elem<T>::mma(kv8_expand<T>(vb1[0], vb1[1]), qvf[2 * j], sv[1]);
                    sv[0] = Elem<T>::mma(kv8_expand<T>(vb0[2], vb0[3]), qvf[2 * j + 1], sv[0]);
                    sv[1] = Elem<T>::mma(kv8_expand<T>(vb1[2], vb1[3]), qvf[2 * j + 1], sv[1]);
                }
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) s[kb][i] = kd * s[kb][i] + vd * sv[kb][i];
            } else {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) s[kb][i] *= kd;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const f32x16 &sp = s[j >> 2];
                const int b4 = 4 * (j & 3);
                *(float4 *)(sred + ((wave * 8 + j) * 64 + lane) * 16) = make_float4(sp[b4], sp[b4 + 1], sp[b4 + 2], sp[b4 + 3]);
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
            if (need_mask) mask_scores(s, k0, hh, lim_lo, lim_hi);

            u32x4 pf[4];  // online softmax (lane = packed row; identical in every wave)
            softmax_step<T, DBW>(s, m_run, l_run, o_acc, sc, pf);
            // ---- O^T += V^T.P^T over this wave's column blocks ----------------------------------------------------------
#pragma unroll
            for (int dbl = 0; dbl < DBW; ++dbl) Tile::pv(vbuf, vbase, DBW * wave + dbl, pf, o_acc[dbl]);
        }
        // the other buffer was last read in tile n - 1, behind whose closing barrier every wave is; the partial scores of
        // this tile are read by all in front of the barrier below, and written again behind it
        if (has_next) store_tile(cur ^ 1);
        __syncthreads();
    }

    // ---- epilogue: normalise (v_descale rides in the factor), LSE, O rows straight from the accumulators ---------------
    const float l_tot = half_swap_sum(l_run);
    const bool empty = (l_tot == 0.f) || (l_tot != l_tot);
    const float inv = empty ? 0.f : vd / l_tot;
    float lse_row = empty ? INFINITY : m_run * sc.scale + __logf(l_tot);
    // fa_fwd_combine's convention: a part that holds none of the row's keys carries no weight; a row without any key keeps +inf
    if (p.num_splits > 1 && empty && lim_lo < lim_hi) lse_row = -INFINITY;
    if (!row_ok) return;
    const int64_t row_o = p.cu_seqlens_q ? (int64_t)(q0 + my_row) : (int64_t)my_row;
    if (wave == 0 && hh == 0) {
        const int64_t li = (p.cu_seqlens_q ? (int64_t)head * p.total_q + row_o : ((int64_t)batch * p.h + head) * p.seqlen_q + my_row) +
                           split * p.lse_split_stride;
        p.lse[li] = lse_row;
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
