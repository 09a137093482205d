// fa_fwd_kernel_pk.h — gfx950 forward with the GQA group packed into the rows of a tile (PackGQA), and the body it shares
// with the forward over an fp8 KV cache (kv8_fwd_kernel, fa_fwd_kernel_kv8.h).
//
// Role of the reference's PackGQA (hopper/pack_gqa.h:18-255; requested through `pack_gqa`, FA_FLAG_PACK_GQA here): the
// g = h / h_k query heads of one kv head share one pass over that head's K/V.  A workgroup owns a block of PACKED rows of one
// (batch, kv head[, split]): packed row pr is query row pr / g of head kv_head * g + pr % g, prows = seqlen_q(batch) * g.
// Short query ranges (a verify step of a few tokens, the decode rows of a mixed step, short ragged prompts) fill a tile with
// g times as many valid rows, and K/V are streamed and multiplied once per kv head instead of once per query head.
//
// The tile loop is fwd_kernel's 4-wave x 32-row shape (fa_fwd_kernel.h: lane owns a row, S^T = K.Q^T, O^T = V^T.P^T, 64-key
// tiles double-buffered in LDS, two workgroups per CU); its per-tile step and the row-staged epilogue are the shared pieces
// of fa_fwd_tile_step.h.  packed_rows_fwd owns everything that reads the row mapping:
//   * work item: (batch, kv head, split) groups dealt round-robin over the 8 XCDs, the row blocks of one group on one XCD
//     (fwd_kernel_qv's decode);
//   * Q load: per-lane address from (query row, head);
//   * key range of a block / tile classification of a wave: from the first and last QUERY row in it;
//   * element masks: the lane's query row, never the packed row;
//   * sink logit: the lane's own head; load_scales stays per kv head;
//   * epilogue: O and LSE address (query row, head).  Split partials use the layouts of fwd_kernel, so the merge is shared;
// and the dense / paged staging of a K/V tile.  What a staged tile IS -- element type, LDS image, the Q columns a k-step
// contracts, the two operand products -- comes from the policy KV: Kv16 below (pk_fwd_kernel: K/V of type T, fwd_kernel's
// tile) or Kv8 (fa_fwd_kernel_kv8.h: e4m3 bytes).  KV::FP8_CACHE also selects, at compile time, the contract of the entry
// point a kernel serves; every use says what differs.
// What WALKS the key tiles is the policy WALK: RangeWalk (pk_fwd_kernel, kv8_fwd_kernel: every 64-key tile of the block's key
// range, in order) or ListWalk (sp_fwd_kernel, fa_fwd_kernel_sp.h: the tiles of the key blocks a per-kv-head list names, in list
// order).  Both run the same load_tile / tile step / store_tile; every use of WALK::SPARSE says what differs.
// What a query row SEES of the walked tiles is the policy MASK: RangeMask (all three kernels above: the lane's key range
// [lim_lo, lim_hi) from is_causal / the window, bottom-right aligned) or TreeMask (tr_fwd_kernel, fa_fwd_kernel_tr.h: the whole
// committed prefix and, of the sq draft keys at the end of the cache, the ones a 64-bit word per query row names).  Every use
// of MASK::TREE says what differs; with RangeMask nothing of it is compiled in.
// Not here (the plan keeps such calls on the other kernels): all-fp8, ALiBi, dropout, attention_chunk, a V head dim of its
// own, qv, head dims above 128.
#pragma once

#include "fa_fwd_tile_step.h"

namespace fa {

constexpr int PK_NWAVES = 4;
constexpr int PK_BLOCK_M = PK_NWAVES * 32;  // packed rows per workgroup

struct PkParams {
    KParams p;
    int32_t num_pblocks;  // PK_BLOCK_M-row blocks of packed rows per (batch, kv head): ceil(seqlen_q * g / PK_BLOCK_M)
    int32_t num_groups;   // b * h_k * splits: (batch, kv head, split) work groups
};

// K/V tile of pk_fwd_kernel: [64][D] elements of T, the LDS image and the operand reads of fwd_kernel
template <typename T, int D>
struct Kv16 {
    typedef T E;  // staged element
    static constexpr bool FP8_CACHE = false;
    static __device__ __forceinline__ int off(int row, int ch) { return lds_off<D>(row, ch); }
    static __device__ __forceinline__ int q_col(int ks, int hh) { return ks * 16 + hh * 8; }  // Q columns of k-step ks: + [0, 8)
    static __device__ __forceinline__ int kbase(int r, int hh) { return lds_off<D>(r, hh); }
    static __device__ __forceinline__ int vbase(int lane) {
        const int i16 = lane & 15, g1 = (lane >> 4) & 1, hh = lane >> 5;
        return lds_off<D>(4 * hh + (i16 >> 2), 2 * g1 + ((i16 >> 1) & 1)) + 8 * (i16 & 1);
    }
    static __device__ __forceinline__ void scores(const char *kbuf, int kb, const u32x4 (&qf)[D / 16], f32x16 (&s)[2]) {
        scores_16<T, D>(kbuf, kb, qf, s);
    }
    static __device__ __forceinline__ void pv(const char *vbuf, int vb, int db, const u32x4 (&pf)[4], f32x16 &o) {
        pv_16<T, D * 2>(vbuf, vb, db, pf, o);
    }
};

// ---- the walk over the key tiles of a (batch, kv head[, split]) -------------------------------------------------------------
// every tile of the block's key range [n_min, n_max), ascending; split-KV partitions that range
struct RangeWalk {
    static constexpr bool SPARSE = false;
};
// Block-sparse: kv head `g` of batch `b` reads the first min(block_cnt[b, g], max_blocks) entries of block_idx[b, g, :], each a
// block of block_size keys (a multiple of BLOCK_N) = block_size / BLOCK_N tiles.  List position t maps to entry t / sub,
// sub-tile t % sub, logical tile n = entry * sub + t % sub; split-KV partitions the positions.  An entry outside
// [0, ceil(sk / block_size)) and a tile outside the block's key range are passed over before anything is loaded for them;
// entries at or behind the count are never read for their meaning.  Lists are int32 behind element strides (0 = broadcast).
struct ListWalk {
    static constexpr bool SPARSE = true;
    const int32_t *block_cnt, *block_idx;
    int64_t cnt_batch_stride, cnt_head_stride, idx_batch_stride, idx_head_stride;
    int32_t max_blocks, block_size;
};


// ---- what a query row sees of the keys ---------------------------------------------------------------------------------------
// the lane's own key range [lim_lo, lim_hi): is_causal / window, bottom-right aligned on sk
struct RangeMask {
    static constexpr bool TREE = false;
};
// Token tree of a speculative-decoding verify step: the sq query rows of a batch entry are the tree's nodes, their keys the last
// sq rows of the cache.  With shift = sk - sq and t = key - shift: t < 0 (the committed prefix) is seen by every row, a tree key
// by the rows whose word has bit t set; bits at or above sq and tree keys with t >= 64 count as not set.  Words are int64 behind
// element strides, addressed like q: (batch, row) for dense queries, row of the whole batch (batch stride unused) for ragged ones.
struct TreeMask {
    static constexpr bool TREE = true;
    const int64_t *words;
    int64_t batch_stride, row_stride;
};

template <typename T, int D, bool SOFTCAP, typename KV, typename WALK = RangeWalk, typename MASK = RangeMask>
__device__ __forceinline__ void packed_rows_fwd(const PkParams &pa, const WALK &walk = WALK(), const MASK &mask = MASK()) {
    typedef typename KV::E E;
    const KParams &p = pa.p;
    constexpr int NT = PK_NWAVES * 64;
    constexpr int KSTEPS = D / 16;
    constexpr int DBLOCKS = D / 32;
    constexpr int EPC = 16 / (int)sizeof(E);   // staged elements per 16-byte chunk
    constexpr int CH_PER_ROW = D / EPC;        // 16-byte chunks of a key row
    constexpr int TILE_BYTES = BLOCK_N * D * (int)sizeof(E);
    constexpr int CHUNKS = BLOCK_N * CH_PER_ROW;
    constexpr int LD_PER_THREAD = CHUNKS / NT;
    static_assert(CHUNKS % NT == 0, "tile must divide over the workgroup");
    constexpr int O_ROW_BYTES = o_row_bytes(D);  // padded epilogue row; the padding carries the row's O offset

    extern __shared__ __attribute__((aligned(16))) char smem[];
    // [K0 | K1 | V0 | V1]; the epilogue reuses the region as PK_NWAVES x [32][O_ROW_BYTES] (the launch sizes it for the larger)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int hh = lane >> 5;

    // ---- work item (fwd_kernel_qv's decode) --------------------------------------------------------------------------------
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int group = (slot / pa.num_pblocks) * 8 + xcd, pb = slot % pa.num_pblocks;
    if (group >= pa.num_groups) return;  // whole workgroup (padding)
    const int splits = p.num_splits > 1 ? p.num_splits : 1;
    const int unit = group / splits, split = group % splits;
    const int batch = unit / p.h_k, kv_head = unit % p.h_k;
    const int g = p.h_ratio;

    // ---- sequence bookkeeping ----------------------------------------------------------------------------------------------
    int sq, sk, q0 = 0;
    int64_t k_base, v_base;
    if (p.cu_seqlens_q) {
        q0 = p.cu_seqlens_q[batch];
        sq = p.seqused_q ? p.seqused_q[batch] : p.cu_seqlens_q[batch + 1] - q0;
    } else {
        sq = p.seqused_q ? p.seqused_q[batch] : p.seqlen_q;
    }
    bool ragged_k = false;
    if constexpr (!KV::FP8_CACHE && !WALK::SPARSE && !MASK::TREE) ragged_k = p.cu_seqlens_k != nullptr;  // (fa_fwd_kv8_validate / fa_fwd_sparse_kv_validate / fa_fwd_tree_validate refuse cu_seqlens_k)
    if (ragged_k) {
        const int k0 = p.cu_seqlens_k[batch];
        sk = p.seqused_k ? p.seqused_k[batch] : p.cu_seqlens_k[batch + 1] - k0;
        k_base = (int64_t)k0 * p.k_row_stride;
        v_base = (int64_t)k0 * p.v_row_stride;
    } else {
        sk = p.seqused_k ? p.seqused_k[batch] : p.seqlen_k;
        if constexpr (KV::FP8_CACHE || WALK::SPARSE || MASK::TREE) sk = min(sk, p.seqlen_k);  // a cache: never past the capacity
        const int kv_batch = p.kv_batch_idx ? p.kv_batch_idx[batch] : batch;
        k_base = (int64_t)kv_batch * p.k_batch_stride;
        v_base = (int64_t)kv_batch * p.v_batch_stride;
    }
    const int prows = sq * g;  // packed rows of this (batch, kv head); the host keeps seqlen_q * g below 2^31
    const int pr_lo = pb * PK_BLOCK_M;
    if (pr_lo >= prows) return;  // whole workgroup: nothing to do (varlen / padded grid)
    if (p.leftpad_k) {
        const int lp = p.leftpad_k[batch];
        sk = max(sk - lp, 0);
        k_base += (int64_t)lp * p.k_row_stride;
        v_base += (int64_t)lp * p.v_row_stride;
    }
    if (p.block_table) k_base = v_base = 0;  // paged: the page supplies the batch offset
    const int32_t *pages = p.block_table ? p.block_table + (int64_t)batch * p.bt_bs : nullptr;
    const E *kp = (const E *)p.k + k_base + (int64_t)kv_head * p.k_head_stride;
    const E *vp = (const E *)p.v + v_base + (int64_t)kv_head * p.v_head_stride;
    const Scales sc = load_scales(p, batch, kv_head);

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
    // ListWalk: [n_min, n_max) stays the block's key range (what a listed tile is checked against) and the parts of a split
    // call are ranges of list positions [t_lo, t_hi)
    int t_lo = 0, t_hi = 0, sub = 1, nblk = 0;
    const int32_t *list = nullptr;
    if constexpr (WALK::SPARSE) {
        sub = walk.block_size / BLOCK_N;
        nblk = sk > 0 ? (sk + walk.block_size - 1) / walk.block_size : 0;
        const int cnt = walk.block_cnt[(int64_t)batch * walk.cnt_batch_stride + (int64_t)kv_head * walk.cnt_head_stride];
        list = walk.block_idx + (int64_t)batch * walk.idx_batch_stride + (int64_t)kv_head * walk.idx_head_stride;
        t_hi = max(min(cnt, walk.max_blocks), 0) * sub;  // (the host keeps max_blocks * block_size below 2^31)
        split_range(p, split, t_lo, t_hi);
    } else {
        split_range(p, split, n_min, n_max);
    }

    // the lane's own key range [lim_lo, lim_hi), from its QUERY row: the element mask of the boundary tiles, and (the fp8
    // cache's split convention below) whether the row sees a key at all
    int lim_hi = sk, lim_lo = 0;
    if (p.window_right >= 0) lim_hi = min(sk, my_row + shift + p.window_right + 1);
    if (p.window_left >= 0) lim_lo = max(0, my_row + shift - p.window_left);
    // TreeMask (fa_fwd_tree_validate refuses is_causal and the windows: the block's key range is all of [0, sk) and the lane's
    // range is not used): the word of the lane's own QUERY row, loaded once and cut to the bits that name a key of this entry,
    // t in [max(0, -shift), min(sq, 64)) -- so a set bit is a key below sk, and `sees` says whether the row has a key at all
    uint64_t word = 0;
    bool sees = false;
    if constexpr (MASK::TREE) {
        word = (uint64_t)mask.words[bq * mask.batch_stride + row_g * mask.row_stride];
        if (sq < 64) word &= (uint64_t(1) << max(sq, 0)) - 1;
        if (shift < 0) word = shift > -64 ? word >> -shift << -shift : 0;
        sees = shift > 0 || word != 0;
    }

    // ---- Q fragments: B operand of S^T = K.Q^T; k-step ks of lane (r, hh) holds Q[row r][KV::q_col(ks, hh) .. + 8]
    // (branch-free, zeroed by selects)
    u32x4 qf[KSTEPS];
    {
        const T *qr = (const T *)p.q + bq * p.q_batch_stride + row_g * p.q_row_stride + (int64_t)head * p.q_head_stride;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const int d0 = KV::q_col(ks, hh);
            qf[ks] = *(const u32x4 *)(qr + (d0 < p.d ? d0 : 0));
        }
        const u32x4 z4 = {0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) qf[ks] = (KV::q_col(ks, hh) < p.d && row_ok) ? qf[ks] : z4;
    }

    f32x16 o_acc[DBLOCKS];
#pragma unroll
    for (int db = 0; db < DBLOCKS; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) o_acc[db][i] = 0.f;
    float m_run = -INFINITY;  // running row max (unscaled scores), same in both lane halves
    float l_run = 0.f;        // running row sum, PARTIAL per lane half (combined in the epilogue)

    // ---- K/V staging, 16 bytes per load (fwd_kernel's: clamped rows / chunks, the duplicates are masked or meet zero Q
    // columns; every staged chunk comes from a valid key row).  Every tile is addressed from a 64-bit base that is rebuilt per
    // tile (cache entry or page, first key row of the tile, kv head); the lane offset inside a tile is 32-bit ---------------
    u32x4 kreg[LD_PER_THREAD], vreg[LD_PER_THREAD];
    static_assert(NT % CH_PER_ROW == 0, "a pass of the workgroup covers whole rows");
    constexpr int ROWS_PER_PASS = NT / CH_PER_ROW;
    const int ld_row0 = tid / CH_PER_ROW;
    const int ld_col0 = ((tid % CH_PER_ROW) * EPC < p.d) ? (tid % CH_PER_ROW) * EPC : 0;
    const int k_rs = (int)p.k_row_stride, v_rs = (int)p.v_row_stride;  // host guarantees 64 * stride < 2^31
    auto load_tile = [&](int n) {
        const int k0 = n * BLOCK_N;
        const E *kt = kp + (int64_t)k0 * p.k_row_stride;
        const E *vt = vp + (int64_t)k0 * p.v_row_stride;
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
            const int off = KV::off(c / CH_PER_ROW, c % CH_PER_ROW);
            *(u32x4 *)(smem + buf * TILE_BYTES + off) = kreg[i];
            *(u32x4 *)(smem + (2 + buf) * TILE_BYTES + off) = vreg[i];
        }
    };

    // lane-constant pieces of the LDS read addresses
    const int kbase = KV::kbase(r, hh);
    const int vbase = KV::vbase(lane);

    // ---- the walk: n_first() / the loop head below give the tile to compute and the one to stage beside it.  RangeWalk: n,
    // n + 1 of [n_min, n_max).  ListWalk (all of it uniform over the workgroup: scalar loads and scalar compares): next_tile()
    // gives the logical tile of the next list position that is to be read, or -1 behind the last; positions whose entry lies
    // outside [0, nblk) or whose tile lies outside the block's key range [n_min, n_max) are passed over there, before any load
    // is issued for them (so load_tile's `last` stays >= 0).  The entry of the NEXT list slot is fetched when the walk enters a
    // slot -- one step ahead, beside the K/V loads of the tile in flight -- so the tile address never waits for it.  That
    // fetch is a VECTOR load on purpose (a scalar load is not to be had behind the loop's barrier, and a uniform vector load
    // is made scalar where it is issued, which waits for it there): the opaque zero `vz` keeps its address per-lane in the
    // compiler's eyes, the value stays in a VGPR over the step, and the wait sits at the readfirstlane that consumes it.
    int t = t_lo, ent = t_lo / sub, st = t_lo - ent * sub;
    int e_cur = 0, e_next = 0, vz = 0;
    bool enter = true;
    if constexpr (WALK::SPARSE) {
        asm volatile("" : "+v"(vz));
        e_next = (t_lo < t_hi) ? list[ent + vz] : 0;
    }
    auto next_tile = [&]() -> int {
        while (t < t_hi) {
            if (enter) {
                e_cur = __builtin_amdgcn_readfirstlane(e_next);
                if ((ent + 1) * sub < t_hi) e_next = list[ent + 1 + vz];  // (a slot in front of the count)
                enter = false;
            }
            const bool inside = (uint32_t)e_cur < (uint32_t)nblk;
            const int n = inside ? e_cur * sub + st : -1;
            ++t;
            if (++st == sub) {
                st = 0;
                ++ent;
                enter = true;
            }
            if (n >= n_min && n < n_max) return n;
        }
        return -1;
    };

    int n_first = n_min;
    if constexpr (WALK::SPARSE) n_first = next_tile();
    if (WALK::SPARSE ? n_first >= 0 : n_min < n_max) {
        load_tile(n_first);
        store_tile(0);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): Q retired here, not in front of the first MFMA of every tile
    __syncthreads();

    int n_next = -1, parity = 0;  // (ListWalk only)
    for (int n = n_first; WALK::SPARSE ? n >= 0 : n < n_max; n = WALK::SPARSE ? n_next : n + 1) {
        int cur;
        bool has_next;
        if constexpr (WALK::SPARSE) {
            cur = parity;
            parity ^= 1;
            n_next = next_tile();
            has_next = n_next >= 0;
            if (has_next) load_tile(n_next);
        } else {
            cur = (n - n_min) & 1;
            has_next = (n + 1 < n_max);
            if (has_next) load_tile(n + 1);
        }

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
        if constexpr (MASK::TREE) need_mask = k0 + BLOCK_N > shift;  // reaches sk or a draft key: at most two tiles (sq <= 64)

        if (!skip) {  // (wave-uniform: EXEC is full at the transposed reads)
            const char *kbuf = smem + cur * TILE_BYTES;
            const char *vbuf = smem + (2 + cur) * TILE_BYTES;

            f32x16 s[2];  // S^T = K.Q^T : two 32-key blocks
            zero_scores(s);
            KV::scores(kbuf, kbase, qf, s);
            if constexpr (SOFTCAP) softcap_scores(s, sc);
            if constexpr (MASK::TREE) {
                if (need_mask) mask_scores(s, k0, hh, shift, word);  // the tiles of the draft keys only
            } else {
                if (need_mask) mask_scores(s, k0, hh, lim_lo, lim_hi);  // boundary tiles only
            }
            u32x4 pf[4];
            softmax_step<T, DBLOCKS>(s, m_run, l_run, o_acc, sc, pf);
#pragma unroll
            for (int db = 0; db < DBLOCKS; ++db) KV::pv(vbuf, vbase, db, pf, o_acc[db]);  // O^T += V^T.P^T
        }

        if (has_next) store_tile(cur ^ 1);
        __syncthreads();
    }

    // ---- epilogue: normalise, LSE, O^T regs -> LDS -> 16-byte stores of (query row, head) rows -----------------------------
    // (the loop's last barrier has retired every K/V read, so the region can be reused)
    const float l_tot = half_swap_sum(l_run);
    const bool empty = (l_tot == 0.f) || (l_tot != l_tot);
    float inv;
    float lse_row = empty ? INFINITY : m_run * sc.scale + __logf(l_tot);  // +inf for rows with no valid key, as fwd_kernel
    if constexpr (KV::FP8_CACHE) {
        inv = empty ? 0.f : sc.v_descale / l_tot;  // v_descale rides in the factor
    } else {
        inv = empty ? 1.f : 1.f / l_tot;
    }
    if constexpr (MASK::TREE) {
        // kv8's split convention below, for both cache types (the merge is fa_fwd_combine): a part without a key of the row
        // writes -inf when the row sees a key anywhere, +inf when its word and an empty prefix leave it none.  No sink
        if (p.num_splits > 1 && empty && sees) lse_row = -INFINITY;
    } else if constexpr (WALK::SPARSE) {
        // kv8's split convention below, for both cache types (the merge is fa_fwd_combine); "the row sees a key" means a
        // LISTED key here: an empty part looks through the whole list (uniform addresses, entries in front of the count
        // only) for a block in range that meets the row's key range.  Rare: only the rows of a part that found nothing
        if (p.num_splits > 1 && empty && lim_lo < lim_hi) {
            bool seen = false;
            const int slots = max(min(walk.block_cnt[(int64_t)batch * walk.cnt_batch_stride + (int64_t)kv_head * walk.cnt_head_stride], walk.max_blocks), 0);
            for (int i = 0; i < slots && !seen; ++i) {
                const int e = list[i];
                if ((uint32_t)e < (uint32_t)nblk) seen = max(e * walk.block_size, lim_lo) < min((e + 1) * walk.block_size, lim_hi);
            }
            if (seen) lse_row = -INFINITY;
        }
    } else if constexpr (KV::FP8_CACHE) {
        // split-KV partials follow fa_fwd_combine's convention (the merge of fa_fwd_kv8 is that entry point): a part that holds
        // none of the row's keys carries no weight (-inf); a row without any key keeps +inf.  No sink (fa_fwd_kv8_validate)
        if (p.num_splits > 1 && empty && lim_lo < lim_hi) lse_row = -INFINITY;
    } else {
        if (p.sink)  // the lane's own head
            sink_finalize(row_ok ? load_sink(p, head, my_row) : -INFINITY, m_run * sc.scale, l_tot, empty, inv, lse_row);
    }
    const int64_t o_off = bq * p.o_batch_stride + row_g * p.o_row_stride + (int64_t)head * p.o_head_stride;
    if (wave_active) {
        if (hh == 0 && row_ok) {
            const int64_t li = p.cu_seqlens_q ? (int64_t)head * p.total_q + row_g : ((int64_t)batch * p.h + head) * p.seqlen_q + my_row;
            p.lse[li + split * p.lse_split_stride] = lse_row;
        }
        if (p.num_splits > 1) {
            if (row_ok) store_split_partial((float *)p.o + split * p.o_split_stride + o_off, o_acc, inv, 0, hh, p.d);
        } else {
            char *obuf = smem + wave * (32 * O_ROW_BYTES);
            stage_o_rows<T, D>(obuf, r, hh, o_acc, inv);
            if (hh == 0) stage_o_dest<D>(obuf, r, o_off, row_ok);
        }
    }
    if (p.num_splits > 1) return;  // (uniform over the launch: no wave is left waiting at the barrier below)
    __syncthreads();
    if (wave_active) store_staged_rows<T, D>(smem + wave * (32 * O_ROW_BYTES), lane, (T *)p.o, p.d);
}

template <typename T, int D, bool SOFTCAP>
__global__ __launch_bounds__(PK_NWAVES * 64, 2) void pk_fwd_kernel(const PkParams pa) {
    packed_rows_fwd<T, D, SOFTCAP, Kv16<T, D>>(pa);
}

}  // namespace fa
