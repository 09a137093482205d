// fa_fwd_kernel_tk.h — gfx950 MLA decode over the key POSITIONS a top-k list names per query token (fa_fwd_topk_kv,
// include/fa_fwd.h): the attention half of DeepSeek-V3.2-style sparse attention.  The cache is the latent cache fwd_kernel_qv
// reads (K of width d <= 64, V of width d_v in [256, 512], S = Q.K^T + Qv.V^T); the list is the mask.
//
// Design (wave64, MFMA 32x32x16, 4 waves, one workgroup per CU):
//   * a work item is (batch, query token, kv head, split, 32-row block).  Lists are per token, so the 32 rows of a workgroup
//     are 32 HEADS of one token: row pr -> head kv_head * g + pb * 32 + pr (fwd_kernel_qv's packed rows mix query rows).  The
//     row blocks of one (batch, token, kv head) gather the same cache rows and stay on one XCD (L2 hits).
//   * a tile is 64 list positions.  Lane l of every wave loads entry 64 t + l (one coalesced 256-byte load); the ballot of
//     (uint32_t)entry < sk, cut to the list length, is the tile's validity word: identical in every wave, applied to S^T by
//     bit test.  An invalid entry never forms an address: its row is staged from the first valid entry of the tile and its
//     score is masked.  A tile without a valid entry loads no K/V row and is passed over.
//   * the walk is a pipeline of three loads, each issued one tile-compute ahead of its use: the entries of tile t + 3 (a
//     per-lane vector load), the page numbers of tile t + 2 (one page-table lookup per lane = per entry, not per staged
//     chunk), the K/V rows of tile t + 1 (global -> registers, written to LDS behind the compute of tile t).  Every lane
//     holds the element offsets of "its" entry's K and V row; the staging takes them across lanes: V rows are wave-uniform
//     (DVT 512: one whole 1 KiB row per load instruction), so their offsets come by v_readlane into a scalar base; K rows
//     (8 per wave and pass) by ds_bpermute.
//   * the score contraction split over the waves, the meeting of the four partial S^T in LDS in wave order and the DVT/4
//     columns of O^T per wave are fwd_kernel_qv's, restated here (sharing the block as a function moved instructions in
//     that kernel's code objects, which its tests pin).  Online softmax, P^T pack, pv_16 and the split-partial store are
//     fa_fwd_tile_step.h's.  With every position listed in order the operations and their order are fwd_kernel_qv's.
//   * split-KV partitions the TILES OF THE LIST.  A part that met no valid entry writes LSE = -inf when another part of the
//     list holds one, +inf when none does (it looks through the whole list: ceil(topk / 64) loads, on such parts only), so
//     fa_fwd_combine gives out = 0, lse = +inf for a row nothing is visible to.
// Known limit: at g > 32 the row blocks of a token gather the same rows again (from L2).
#pragma once

#include "fa_fwd_tile_step.h"
#include "fa_fwd_kernel_qv.h"

namespace fa {

struct TkParams {
    QvParams qa;               // qa.num_pblocks = ceil(g / 32); qa.num_groups = b * seqlen_q * h_k * splits
    const int32_t *indices;    // (b, seqlen_q, h_k | 1, topk) behind element strides; the last stride is 1
    int64_t idx_batch_stride, idx_row_stride, idx_head_stride;
    int32_t topk;
};

template <int DVT>
constexpr int smem_bytes_tk() { return smem_bytes_qv<DVT>(); }  // the entries live in registers

// the 32-bit value lane `src` of the wave holds
__device__ __forceinline__ int lane_read(int v, int src) { return __builtin_amdgcn_ds_bpermute(src << 2, v); }

template <typename T, int DVT>
__global__ __launch_bounds__(QV_NWAVES * 64, 1) void tk_fwd_kernel(const TkParams ta) {
    const QvParams &qa = ta.qa;
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
    static_assert(KSV >= 1 && DBW >= 1 && LDK >= 1 && LDV >= 1 && (CHV == 64 || CHV == 32), "tile shape");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *kbuf = smem;
    char *vbuf = smem + K_BYTES;
    char *sred = smem + K_BYTES + V_BYTES;  // [wave][8][64 lanes] float4

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int hh = lane >> 5;

    // ---- work item: groups of (batch, token, kv head, split) dealt round-robin over the 8 XCDs, the row blocks of one group
    // on one XCD ---------------------------------------------------------------------------------------------------------------
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int group = (slot / qa.num_pblocks) * 8 + xcd, pb = slot % qa.num_pblocks;
    if (group >= qa.num_groups) return;  // whole workgroup (padding)
    const int splits = p.num_splits > 1 ? p.num_splits : 1;
    const int unit = group / splits, split = group % splits;
    const int kv_head = unit % p.h_k, bt = unit / p.h_k;
    const int batch = bt / p.seqlen_q, token = bt % p.seqlen_q;
    const int g = p.h_ratio;

    int sk = p.seqused_k ? p.seqused_k[batch] : p.seqlen_k;
    sk = max(min(sk, p.seqlen_k), 0);  // a cache: never past the capacity
    const int kv_batch = p.kv_batch_idx ? p.kv_batch_idx[batch] : batch;
    const int32_t *pages = p.block_table ? p.block_table + (int64_t)batch * p.bt_bs : nullptr;
    const T *kp = (const T *)p.k + (pages ? 0 : (int64_t)kv_batch * p.k_batch_stride) + (int64_t)kv_head * p.k_head_stride;
    const T *vp = (const T *)p.v + (pages ? 0 : (int64_t)kv_batch * p.v_batch_stride) + (int64_t)kv_head * p.v_head_stride;
    const Scales sc = load_scales(p, batch, kv_head);
    const int32_t *list = ta.indices + (int64_t)batch * ta.idx_batch_stride + (int64_t)token * ta.idx_row_stride +
                          (int64_t)kv_head * ta.idx_head_stride;

    // ---- the lane's row = a head of the group ---------------------------------------------------------------------------------
    const int hr = pb * 32 + r;
    const bool row_ok = hr < g;
    const int head = kv_head * g + min(hr, g - 1);

    // ---- tiles of the list ------------------------------------------------------------------------------------------------------
    const int n_tiles = (ta.topk + BLOCK_N - 1) / BLOCK_N;
    int t_lo = 0, t_hi = n_tiles;
    split_range(p, split, t_lo, t_hi);

    // ---- Q / Qv fragments: B operands of S^T = K.Q^T + V.Qv^T; lane (r, hh) holds row r, columns 16 ks + 8 hh .. +8 ----------
    const u32x4 z4 = {0, 0, 0, 0};
    const bool has_qv = qa.qv != nullptr;
    u32x4 qf, qvf[KSV];
    {
        const T *qr = (const T *)p.q + (int64_t)batch * p.q_batch_stride + (int64_t)token * p.q_row_stride + (int64_t)head * p.q_head_stride;
        const int c = 16 * wave + 8 * hh;
        qf = *(const u32x4 *)(qr + (c < p.d ? c : 0));
        qf = (c < p.d && row_ok) ? qf : z4;
        const T *qvr = has_qv ? (const T *)qa.qv + (int64_t)batch * qa.qv_batch_stride + (int64_t)token * qa.qv_row_stride +
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

    f32x16 o_acc[DBW];
#pragma unroll
    for (int db = 0; db < DBW; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) o_acc[db][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    // ---- the walk's pipeline: stage A the raw entries, stage B position + page number, stage C row offsets ---------------------
    // Validity is decided once, in stage B, by an unsigned compare against sk in front of every address formed from an entry.
    auto valid_word = [&](int t, int raw) -> uint64_t {
        const bool ok = t < t_hi && BLOCK_N * t + lane < ta.topk && (uint32_t)raw < (uint32_t)sk;
        return __ballot(ok);
    };
    int raw_a = 0;                       // A: entries of a tile (in flight)
    uint64_t word_b = 0;                 // B: validity word, the lane's clamped position in its page, the page number (in flight)
    int inpage_b = 0, page_b = 0;
    uint64_t word_c = 0;                 // C: validity word, element offsets of the lane's K and V row
    int64_t koff_c = 0, voff_c = 0;
    auto issue_entries = [&](int t) {
        if (t < t_hi) raw_a = list[min(BLOCK_N * t + lane, ta.topk - 1)];
    };
    auto resolve = [&](int t) {  // B <- A
        word_b = valid_word(t, raw_a);
        if (word_b == 0) return;
        const int first = __builtin_ctzll(word_b);
        const int fix = __builtin_amdgcn_readlane(raw_a, first);
        const int pos = ((word_b >> lane) & 1) ? raw_a : fix;  // in [0, sk)
        if (pages) {
            const int pi = pos / p.page_size;
            inpage_b = pos - pi * p.page_size;
            page_b = pages[pi];
        } else {
            inpage_b = pos;
            page_b = 0;
        }
    };
    auto offsets = [&]() {  // C <- B
        word_c = word_b;
        koff_c = (int64_t)page_b * p.k_batch_stride + (int64_t)inpage_b * p.k_row_stride;
        voff_c = (int64_t)page_b * p.v_batch_stride + (int64_t)inpage_b * p.v_row_stride;
    };

    // ---- K/V staging from the offsets of stage C (clamped chunks as in fwd_kernel_qv: duplicates meet zero Q columns) ---------
    u32x4 kreg[LDK], vreg[LDV];
    const int ldk_row0 = lane / CHK;  // (the wave's first row of a pass: + 8 wave below)
    const int ldk_col = ((tid % CHK) * 8 < p.d) ? (tid % CHK) * 8 : 0;
    const int ldv_col = ((tid % CHV) * 8 < p.dv) ? (tid % CHV) * 8 : 0;
    auto load_tile = [&]() {
        const int klo = (int)koff_c, khi = (int)(koff_c >> 32), vlo = (int)voff_c, vhi = (int)(voff_c >> 32);
#pragma unroll
        for (int i = 0; i < LDK; ++i) {
            const int row = 8 * wave + ldk_row0 + i * RPK;
            const int64_t off = ((int64_t)lane_read(khi, row) << 32) | (uint32_t)lane_read(klo, row);
            kreg[i] = *(const u32x4 *)(kp + off + ldk_col);
        }
#pragma unroll
        for (int i = 0; i < LDV; ++i) {
            int64_t off;
            if constexpr (CHV == 64) {  // one row per wave and pass: a scalar base
                const int row = wave + i * RPV;
                off = ((int64_t)__builtin_amdgcn_readlane(vhi, row) << 32) | (uint32_t)__builtin_amdgcn_readlane(vlo, row);
            } else {                    // two rows per wave and pass
                const int row = 2 * wave + hh + i * RPV;
                off = ((int64_t)lane_read(vhi, row) << 32) | (uint32_t)lane_read(vlo, row);
            }
            vreg[i] = *(const u32x4 *)(vp + off + ldv_col);
        }
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

    // lane-constant parts of the LDS addresses (fwd_kernel_qv's)
    const int i16 = lane & 15, g1 = (lane >> 4) & 1;
    const int kbase = lds_off<64>(r, hh) ^ (32 * wave);        // K row r, chunk 2 wave + hh
    const int vsbase = lds_off<DVT>(r, hh);                    // V row r, chunk hh (score reads)
    const int vbase = lds_off<DVT>(4 * hh + (i16 >> 2), 2 * g1 + ((i16 >> 1) & 1)) + 8 * (i16 & 1);  // transposed reads

    // ---- prologue: fill the pipeline; tile t_lo goes to LDS ----------------------------------------------------------------------
    issue_entries(t_lo);
    resolve(t_lo);
    offsets();
    uint64_t word_cur = word_c;
    if (word_cur) {
        load_tile();
        store_tile();
    }
    issue_entries(t_lo + 1);
    resolve(t_lo + 1);
    offsets();
    issue_entries(t_lo + 2);
    resolve(t_lo + 2);
    issue_entries(t_lo + 3);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): Q / Qv retired here, not in front of the first MFMA of every tile
    __syncthreads();

    bool seen = false;  // the part met a valid entry (workgroup-uniform)
    for (int t = t_lo; t < t_hi; ++t) {
        const uint64_t word_next = word_c;  // tile t + 1
        if (word_next) load_tile();
        offsets();                          // tile t + 2: its page numbers were asked for one tile ago
        resolve(t + 3);                     // ... the entries of tile t + 3 too
        issue_entries(t + 4);

        if (word_cur) {
            seen = true;
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

            // ---- the list is the mask: list position kb * 32 + (i & 3) + 8 (i >> 2) + 4 hh of the tile stays iff its bit is set
            if (word_cur != ~uint64_t(0)) {
                const uint64_t wl = word_cur >> (4 * hh);
                const uint32_t half[2] = {(uint32_t)wl, (uint32_t)(wl >> 32)};
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        if (!((half[kb] >> ((i & 3) + 8 * (i >> 2))) & 1u)) s[kb][i] = -INFINITY;
            }

            u32x4 pf[4];  // online softmax (lane = head; identical in every wave)
            softmax_step<T, DBW>(s, m_run, l_run, o_acc, sc, pf);
            // ---- O^T += V^T.P^T over this wave's column blocks ----------------------------------------------------------
#pragma unroll
            for (int dbl = 0; dbl < DBW; ++dbl) pv_16<T, DVT * 2>(vbuf, vbase, DBW * wave + dbl, pf, o_acc[dbl]);
        }
        __syncthreads();  // every read of the K/V tile and of the partial scores is done
        if (word_next) {
            store_tile();
            __syncthreads();
        }
        word_cur = word_next;
    }

    // ---- an empty part of a split call: does the list hold a valid entry at all? (all lanes: the ballot needs them) -------------
    float lse_empty = INFINITY;
    if (p.num_splits > 1 && !seen) {
        for (int t = 0; t < n_tiles; ++t) {
            const int raw = list[min(BLOCK_N * t + lane, ta.topk - 1)];
            if (__ballot(BLOCK_N * t + lane < ta.topk && (uint32_t)raw < (uint32_t)sk) != 0) {
                lse_empty = -INFINITY;
                break;
            }
        }
    }

    // ---- epilogue: normalise, LSE, O rows straight from the accumulators ---------------------------------------------------------
    const float l_tot = half_swap_sum(l_run);
    const bool empty = (l_tot == 0.f) || (l_tot != l_tot);
    const float inv = empty ? 1.f : 1.f / l_tot;
    if (!row_ok) return;
    if (wave == 0 && hh == 0) {
        const int64_t li = ((int64_t)batch * p.h + head) * p.seqlen_q + token + split * p.lse_split_stride;
        p.lse[li] = empty ? lse_empty : m_run * sc.scale + __logf(l_tot);
    }
    const int64_t o_off = (int64_t)batch * p.o_batch_stride + (int64_t)token * p.o_row_stride + (int64_t)head * p.o_head_stride;
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
