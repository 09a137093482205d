// fa_fwd_kernel_tk8.h — gfx950 MLA decode over the key POSITIONS a top-k list names per query token, on the fp8 (OCP e4m3fn)
// latent KV cache (fa_fwd_topk_kv8, include/fa_fwd.h): tk_fwd_kernel's work item and list rules (fa_fwd_kernel_tk.h) over
// qv8_fwd_kernel's byte tile and arithmetic (fa_fwd_kernel_qv8.h), with a gather walk of its own.
//
// Taken as they are:
//   * from tk_fwd_kernel: the work item (batch, token, kv head, split, block of 32 heads) and its XCD dealing; tiles of 64 list
//     positions; lane l of every wave holds entry 64 t + l; the ballot of (uint32_t)entry < sk, cut to the list length, is the
//     tile's validity word, applied to S^T by bit test; an invalid entry's row is staged from the tile's first valid entry; a
//     tile whose word is 0 issues no K/V load and no compute; split-KV over the tiles of the list and the look through the list
//     of a part that met no valid entry.
//   * from qv8_fwd_kernel: the K image kv8_off<64> and the V image qv8_voff<DVT>, kv8_expand at the MFMA operand, Kv8::q_col and
//     Kv8::pv, the K and V products in accumulators of their own joined as kd sK + vd sV when the partial goes to LDS, the LDS
//     double buffer with one barrier per tile, the Scales (k_descale never enters a second time) and vd / l as normalisation.
//   * from fa_fwd_tile_step.h: softmax_step and the split-partial store.  The four partials meet in LDS in wave order.
//   With every position listed in order the operations and their order are qv8_fwd_kernel's.
//
// The gather over byte rows (this file's).  Every lane resolves its own entry: one pos / page_size, one page-table load, and
// holds the 64-bit BYTE offsets of its entry's K and V row.  A V row is DVT bytes = DVT / 16 lanes x 16 bytes, so one load
// instruction of a wave fetches 2 (DVT 512) or 4 (DVT 256) rows and the workgroup 8 or 16; the whole K tile (64 rows x 4 chunks)
// is one pass of the workgroup.  The row offsets cross lanes by ds_bpermute.  The chunk -> (row, chunk) mapping of a pass is
// qv8_fwd_kernel's store_tile mapping, so the LDS images are its images.
//
// Depth: the rows of TWO tiles are in flight per workgroup.  A byte tile is 36 VGPRs per lane at DVT 512 (the 16-bit tile is
// 72), so two register sets r0 / r1 fit beside the accumulators; the loop is unrolled by two so that each set is named
// statically (step(t, r0, r1), step(t + 1, r1, r0)).  In step t
//     the page numbers of tile t + 3 become the offsets of stage C, the entries of tile t + 4 become positions and ask for
//     their page numbers (stage B), the entries of tile t + 5 are asked for (stage A)   -- the small loads first --
//     the rows of tile t + 2 are asked for, into the set the step before last stored from,
//     tile t is computed from LDS buffer t & 1,
//     the rows of tile t + 1, asked for one step ago, go from registers to the other LDS buffer; one barrier.
// Loads retire in order and the waits are counted (vmcnt), so the number of load instructions of a step must not depend on the
// path: every step issues exactly two small loads and 1 + LDV row loads (see issue_entries / resolve / load_rows below for what
// a tile without a valid entry reads instead of the cache).  The build then waits with vmcnt(1 + LDV) in front of a step's use
// of its entries and page numbers -- the rows of tile t + 1 stay in flight over it -- and with vmcnt(2 LDV + 3 ... LDV + 3) in
// front of the LDS stores of tile t + 1, behind the issue of tile t + 2.  (With the small or the row loads under branches the
// compiler fell back to vmcnt(0) there, and an explicit vmcnt(0) on the skipping path did not restore the count.)
//
// Empty parts and rows: tk_fwd_kernel's rules (LSE = -inf for a part without a valid entry when another part holds one, +inf
// when none does; unsplit O = 0, LSE = +inf).
#pragma once

#include "fa_fwd_kernel_qv8.h"
#include "fa_fwd_kernel_tk.h"

namespace fa {

template <int DVT>
constexpr int smem_bytes_tk8() { return smem_bytes_qv8<DVT>(); }  // K0 K1 | V0 V1 | partial scores; the entries live in registers

// the staged rows of one tile: this lane's 16-byte chunks
template <int LDV>
struct Tk8Rows {
    u32x4 k, v[LDV];
};

template <typename T, int DVT>
__global__ __launch_bounds__(QV_NWAVES * 64, 1) void tk8_fwd_kernel(const TkParams ta) {
    typedef Kv8<T, DVT> Tile;  // q_col and pv: neither reads the K image
    const QvParams &qa = ta.qa;
    const KParams &p = qa.p;
    constexpr int NT = QV_NWAVES * 64;
    constexpr int CPW = DVT / QV_NWAVES;       // V / O columns (= bytes of a V row) per wave
    constexpr int KSV = CPW / 16;              // Qv k-steps per wave
    constexpr int DBW = CPW / 32;              // O^T row blocks per wave = 16-byte score reads per wave and key block
    constexpr int K_BYTES = BLOCK_N * 64;
    constexpr int V_BYTES = BLOCK_N * DVT;
    constexpr int CHK = 64 / 16, CHV = DVT / 16;  // 16-byte chunks per K / V row
    constexpr int LDV = BLOCK_N * CHV / NT;       // V loads per lane and tile
    constexpr int RPV = NT / CHV;                 // V rows per pass of the workgroup (64 / CHV per wave and load instruction)
    static_assert(DVT == 256 || DVT == 512, "the V image is derived for whole bank rows");
    static_assert(BLOCK_N * CHK == NT && LDV >= 1 && DBW >= 1 && KSV == 2 * DBW && 64 % CHV == 0, "tile shape");
    typedef Tk8Rows<LDV> Rows;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *sred = smem + 2 * K_BYTES + 2 * V_BYTES;  // [wave][8][64 lanes] float4

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int hh = lane >> 5;

    // ---- work item (tk_fwd_kernel's) -------------------------------------------------------------------------------------------
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
    const uint8_t *kp = (const uint8_t *)p.k + (pages ? 0 : (int64_t)kv_batch * p.k_batch_stride) + (int64_t)kv_head * p.k_head_stride;
    const uint8_t *vp = (const uint8_t *)p.v + (pages ? 0 : (int64_t)kv_batch * p.v_batch_stride) + (int64_t)kv_head * p.v_head_stride;
    // descales stay factors of the fp32 products; the softmax's Scales carry the plain scale (never k_descale again)
    const float kd = p.k_descale ? p.k_descale[batch * p.kd_bs + kv_head * p.kd_hs] : 1.f;
    const float vd = p.v_descale ? p.v_descale[batch * p.vd_bs + kv_head * p.vd_hs] : 1.f;
    Scales sc;
    sc.scale = p.scale; sc.scale_log2 = p.scale_log2; sc.softcap_pre = p.softcap_pre; sc.v_descale = vd;
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

    // ---- Q / Qv fragments (qv8_fwd_kernel's columns): Q row r, columns 16 wave + 8 hh + [0, 8); Qv k-step ks: columns
    // CPW wave + Tile::q_col(ks, hh) + [0, 8) ------------------------------------------------------------------------------------
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

    // ---- the walk's small stages: A the raw entries, B position + page number, C byte offsets of the lane's K and V row -------
    // Validity is decided once, in stage B, by an unsigned compare against sk in front of every address formed from an entry.
    int raw_a = 0;                       // A: entries of a tile (in flight)
    uint64_t word_b = 0;                 // B: validity word, the lane's clamped position in its page, the page number (in flight)
    int inpage_b = 0, page_b = 0;
    uint64_t word_c = 0;                 // C: validity word, byte offsets of the lane's K and V row
    int64_t koff_c = 0, voff_c = 0;
    // Both small loads are issued on every path, one each per step, so that the load count between a load and its use does not
    // depend on the path and the counted waits hold: the entry index is clamped into the list (a tile past the part's end reads
    // the list's last entry and is cut by t < t_hi in the word); the page lookup of a tile without a valid entry, of a dense
    // cache and of a cache without capacity reads table[0] of a table that always has an entry (the page table, else the list)
    // and its value is not used.
    const bool paged = pages != nullptr && p.seqlen_k > 0;  // (a paged cache with capacity has a page table of >= 1 entry)
    const int32_t *table = paged ? pages : list;
    const int page_size = paged ? p.page_size : 0x7fffffff;  // dense: pos / page_size = 0, the position is the row
    auto issue_entries = [&](int t) { raw_a = list[min(BLOCK_N * t + lane, ta.topk - 1)]; };
    auto resolve = [&](int t) {  // B <- A
        const bool ok = t < t_hi && BLOCK_N * t + lane < ta.topk && (uint32_t)raw_a < (uint32_t)sk;
        word_b = __ballot(ok);
        const int first = word_b ? __builtin_ctzll(word_b) : 0;
        const int fix = word_b ? __builtin_amdgcn_readlane(raw_a, first) : 0;
        const int pos = ((word_b >> lane) & 1) ? raw_a : fix;  // in [0, sk); 0 when the tile has no valid entry
        const int pi = pos / page_size;
        inpage_b = pos - pi * page_size;
        const int entry = table[pi];
        page_b = paged ? entry : 0;
    };
    auto offsets = [&]() {  // C <- B
        word_c = word_b;
        koff_c = (int64_t)page_b * p.k_batch_stride + (int64_t)inpage_b * p.k_row_stride;
        voff_c = (int64_t)page_b * p.v_batch_stride + (int64_t)inpage_b * p.v_row_stride;
    };

    // ---- the gather: rows of stage C's tile -> a register set -> an LDS buffer (clamped chunks as in qv8_fwd_kernel: duplicates
    // meet zero Q columns) ----------------------------------------------------------------------------------------------------------
    const int ldk_row = 16 * wave + (lane >> 2);  // = tid / CHK
    const int ldv_row0 = tid / CHV;               // DVT 512: 2 wave + hh; DVT 256: 4 wave + lane / 16
    const int ldk_col = ((tid % CHK) * 16 < p.d) ? (tid % CHK) * 16 : 0;
    const int ldv_col = ((tid % CHV) * 16 < p.dv) ? (tid % CHV) * 16 : 0;
    // The number of load instructions is the same on every path (the counted waits depend on it; with the row loads under a
    // branch the build fell back to vmcnt(0) in front of every use of an entry or a page number, which forced the rows of the
    // tile before to land first).  A tile without a valid entry therefore issues the same 1 + LDV instructions, but not one of
    // them on the cache: every lane reads the first 16 bytes of its own q row again (valid, aligned, in the nearest cache) and
    // the registers are never stored or computed on.  No address is formed from the offsets of such a tile.
    const uint8_t *q_safe = (const uint8_t *)((const T *)p.q + (int64_t)batch * p.q_batch_stride + (int64_t)token * p.q_row_stride +
                                              (int64_t)head * p.q_head_stride);
    auto load_rows = [&](Rows &x, uint64_t word, int64_t koff, int64_t voff) __attribute__((always_inline)) {
        const int klo = (int)koff, khi = (int)(koff >> 32), vlo = (int)voff, vhi = (int)(voff >> 32);
        {
            const int64_t off = ((int64_t)lane_read(khi, ldk_row) << 32) | (uint32_t)lane_read(klo, ldk_row);
            x.k = *(const u32x4 *)(word ? kp + off + ldk_col : q_safe);
        }
#pragma unroll
        for (int i = 0; i < LDV; ++i) {
            const int row = ldv_row0 + i * RPV;
            const int64_t off = ((int64_t)lane_read(vhi, row) << 32) | (uint32_t)lane_read(vlo, row);
            x.v[i] = *(const u32x4 *)(word ? vp + off + ldv_col : q_safe);
        }
    };
    auto store_rows = [&](const Rows &x, int buf) __attribute__((always_inline)) {
        *(u32x4 *)(smem + buf * K_BYTES + kv8_off<64>(tid / CHK, tid % CHK)) = x.k;
#pragma unroll
        for (int i = 0; i < LDV; ++i) {
            const int c = tid + i * NT;
            *(u32x4 *)(smem + 2 * K_BYTES + buf * V_BYTES + qv8_voff<DVT>(c / CHV, c % CHV)) = x.v[i];
        }
    };

    // lane-constant parts of the LDS addresses (qv8_fwd_kernel's)
    const int kbase = kv8_off<64>(r, wave) + 8 * hh;                   // K row r, chunk `wave`, half hh
    const int vsbase = qv8_voff<DVT>(r, hh) ^ (16 * KSV * wave);       // V row r, chunk KSV wave + hh (score reads)
    const int vi16 = lane & 15, vg1 = (lane >> 4) & 1, vk = vi16 >> 1;
    const int vbase = qv8_voff<DVT>((vk & 3) + 8 * (vk >> 2) + 4 * hh, vg1) + 8 * (vi16 & 1);  // Kv8::vbase over this image

    // ---- one tile from LDS buffer `cur` under its validity word (workgroup-uniform) -----------------------------------------------
    auto compute = [&](uint64_t word, int cur) __attribute__((always_inline)) {
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

        // ---- the list is the mask: list position kb * 32 + (i & 3) + 8 (i >> 2) + 4 hh of the tile stays iff its bit is set
        if (word != ~uint64_t(0)) {
            const uint64_t wl = word >> (4 * hh);
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
        for (int dbl = 0; dbl < DBW; ++dbl) Tile::pv(vbuf, vbase, DBW * wave + dbl, pf, o_acc[dbl]);
    };

    // ---- prologue: the small stages run ahead first (C = tile t_lo + 2, B = tile t_lo + 3, A = tile t_lo + 4), then the rows of
    // tiles t_lo and t_lo + 1 are asked for together; tile t_lo goes to LDS buffer 0, tile t_lo + 1 stays on its way to r0 -------
    Rows r0, r1;
    issue_entries(t_lo);
    resolve(t_lo);
    offsets();
    uint64_t word_cur = word_c;  // tile t
    const int64_t koff_0 = koff_c, voff_0 = voff_c;
    issue_entries(t_lo + 1);
    resolve(t_lo + 1);
    offsets();
    uint64_t word_1 = word_c;    // tile t + 1
    const int64_t koff_1 = koff_c, voff_1 = voff_c;
    issue_entries(t_lo + 2);
    resolve(t_lo + 2);
    offsets();
    issue_entries(t_lo + 3);
    resolve(t_lo + 3);
    issue_entries(t_lo + 4);
    load_rows(r1, word_cur, koff_0, voff_0);
    load_rows(r0, word_1, koff_1, voff_1);
    if (word_cur) store_rows(r1, 0);
    __syncthreads();  // (the waits in front of the first tile are the compiler's: Q / Qv and the store above)

    bool seen = false;  // the part met a valid entry (workgroup-uniform)
    // x: the set that holds the rows of tile t + 1; y: the set the rows of tile t + 2 go to; cur: the LDS buffer of tile t
    auto step = [&](int t, Rows &x, Rows &y, int cur) __attribute__((always_inline)) {
        const uint64_t word_2 = word_c;  // tile t + 2, its offsets
        const int64_t koff_2 = koff_c, voff_2 = voff_c;
        offsets();                       // tile t + 3: its page numbers were asked for one step ago
        resolve(t + 4);                  // ... the entries of tile t + 4 too
        issue_entries(t + 5);
        load_rows(y, word_2, koff_2, voff_2);
        if (word_cur) {
            seen = true;
            compute(word_cur, cur);
        }
        // buffer cur ^ 1 was last read in tile t - 1, behind whose closing barrier every wave is; the partial scores of this tile
        // are read by all in front of the barrier below, and written again behind it
        if (word_1) store_rows(x, cur ^ 1);
        __syncthreads();
        word_cur = word_1;
        word_1 = word_2;
    };
    for (int t = t_lo; t < t_hi; t += 2) {
        step(t, r0, r1, 0);
        if (t + 1 < t_hi) step(t + 1, r1, r0, 1);
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

    // ---- epilogue: normalise (v_descale rides in the factor), LSE, O rows straight from the accumulators -----------------------
    const float l_tot = half_swap_sum(l_run);
    const bool empty = (l_tot == 0.f) || (l_tot != l_tot);
    const float inv = empty ? 0.f : vd / l_tot;
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
