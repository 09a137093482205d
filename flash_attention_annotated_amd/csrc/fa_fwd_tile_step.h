// fa_fwd_tile_step.h — the per-tile step of the 4-wave x 32-row "lane owns a query row" forward shape, shared by the kernels
// that took fwd_kernel's tile loop and changed what walks it: pk_fwd_kernel / kv8_fwd_kernel (fa_fwd_kernel_pk.h,
// fa_fwd_kernel_kv8.h), bs_fwd_kernel (fa_fwd_kernel_bs.h) and fwd_kernel_qv (fa_fwd_kernel_qv.h).
//
// Layout all pieces assume (fa_fwd_kernel.h): lane (r, hh) = (lane & 31, lane >> 5) owns row r of the wave; s[kb][i] is the
// score of key kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh of the 64-key tile (the C layout of MFMA 32x32x16 for S^T = K.Q^T),
// so the two lane halves of a row hold disjoint keys: the row maximum is exchanged per tile (half_swap_max), the row sum
// stays partial per half until the epilogue.  o[db][i] is O^T of head-dim column db * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh.
//
// Everything here is __forceinline__ and takes its register arrays by reference: after inlining hipcc sees the text the
// kernels used to spell out themselves (profiles/tile_step_refactor.md compares the code objects).  fwd_kernel keeps its own
// step: it carries dropout, ALiBi, S_dmask and EXTRA in the middle of it.
#pragma once

#include "fa_fwd_kernel.h"

namespace fa {

__device__ __forceinline__ void zero_scores(f32x16 (&s)[2]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) { s[0][i] = 0.f; s[1][i] = 0.f; }
}

// softcap: scores -> tanh(scores * softcap_pre); the cap itself rides in sc.scale / sc.scale_log2 (load_scales)
__device__ __forceinline__ void softcap_scores(f32x16 (&s)[2], const Scales &sc) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) s[kb][i] = fast_tanh(s[kb][i] * sc.softcap_pre);
}

// element mask of a boundary tile: the keys of the tile at k0 outside the lane's own range [lim_lo, lim_hi) get -inf
__device__ __forceinline__ void mask_scores(f32x16 (&s)[2], int k0, int hh, int lim_lo, int lim_hi) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = k0 + kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
            if (key >= lim_hi || key < lim_lo) s[kb][i] = -INFINITY;
        }
}

// element mask of a tile that holds draft keys of a token tree (TreeMask, fa_fwd_kernel_pk.h): key p of the tile at k0 stays iff
// p < shift (the committed prefix) or bit p - shift < 64 of the lane's word is set; the caller has cut the word to the bits
// that name a key below sk
__device__ __forceinline__ void mask_scores(f32x16 (&s)[2], int k0, int hh, int shift, uint64_t word) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int t = k0 + kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh - shift;
            const bool seen = t < 0 || (t < 64 && ((word >> (t & 63)) & 1) != 0);
            if (!seen) s[kb][i] = -INFINITY;
        }
}

// Online softmax of one tile (per lane = per row): new running maximum, rescale of l_run and of the NDB accumulator blocks
// (skipped, wave-uniformly, when no row's maximum moved), s -> exp2 weights, row sum, and the weights packed to T: the
// accumulator registers ARE the B operand of O^T += V^T.P^T (pf[st] = keys 16 st .. 16 st + 15 of the tile).
template <typename T, int NDB>
__device__ __forceinline__ void softmax_step(f32x16 (&s)[2], float &m_run, float &l_run, f32x16 (&o_acc)[NDB], const Scales &sc,
                                             u32x4 (&pf)[4]) {
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
        for (int db = 0; db < NDB; ++db)
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
#pragma unroll
    for (int st = 0; st < 4; ++st) {
        const int kb = st >> 1, b8 = (st & 1) * 8;
#pragma unroll
        for (int j = 0; j < 4; ++j) pf[st][j] = Elem<T>::pack2(s[kb][b8 + 2 * j], s[kb][b8 + 2 * j + 1]);
    }
}

// S^T += K.Q^T over a 16-bit [64][D] tile (lds_off<D>): two 32-key blocks, D / 16 k-steps, one ds_read_b128 each.
// kbase = lds_off<D>(r, hh); qf[ks] = Q[row][16 ks + 8 hh .. + 8].
template <typename T, int D>
__device__ __forceinline__ void scores_16(const char *kbuf, int kbase, const u32x4 (&qf)[D / 16], f32x16 (&s)[2]) {
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
        const int off = kbase ^ (32 * ks);  // = lds_off<D>(r, 2 ks + hh): the swizzle XORs chunk bits 0-3 only
        const u32x4 kf0 = *(const u32x4 *)(kbuf + off);
        const u32x4 kf1 = *(const u32x4 *)(kbuf + off + 32 * D * 2);
        s[0] = Elem<T>::mma(kf0, qf[ks], s[0]);
        s[1] = Elem<T>::mma(kf1, qf[ks], s[1]);
    }
}

// o += V^T.P^T for head-dim columns 32 db .. 32 db + 31 of a 16-bit tile of ROWB bytes per key row: two ds_read_b64_tr_b16
// per 16 keys.  vbase = lds_off(4 hh + (i16 >> 2), 2 g1 + ((i16 >> 1) & 1)) + 8 (i16 & 1), i16 = lane & 15, g1 = (lane >> 4) & 1.
template <typename T, int ROWB>
__device__ __forceinline__ void pv_16(const char *vbuf, int vbase, int db, const u32x4 (&pf)[4], f32x16 &o) {
#pragma unroll
    for (int st = 0; st < 4; ++st) {
        u32x4 vf;
#pragma unroll
        for (int j2 = 0; j2 < 2; ++j2) {
            const int off = (vbase ^ (64 * db + 32 * j2)) + (16 * st + 8 * j2) * ROWB;
            const s16x4 t = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(vbuf + off));
            const u32x2 t2 = __builtin_bit_cast(u32x2, t);
            vf[2 * j2] = t2[0];
            vf[2 * j2 + 1] = t2[1];
        }
        o = Elem<T>::mma(vf, pf[st], o);
    }
}

// ---- epilogue pieces ---------------------------------------------------------------------------------------------------------
constexpr int o_row_bytes(int D) { return D * 2 + 16; }  // padded LDS row of the staged epilogue

// split-KV partial: fp32 in the caller's workspace, straight from the accumulators (fwd_kernel's layout).  opf = the row,
// col0 = the head-dim column of o[0]; columns at or past dlim are not written.
template <int NDB>
__device__ __forceinline__ void store_split_partial(float *opf, const f32x16 (&o)[NDB], float inv, int col0, int hh, int dlim) {
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int col = col0 + db * 32 + 8 * g4 + 4 * hh;
            if (col < dlim)
                *(float4 *)(opf + col) = make_float4(o[db][4 * g4] * inv, o[db][4 * g4 + 1] * inv, o[db][4 * g4 + 2] * inv,
                                                     o[db][4 * g4 + 3] * inv);
        }
}

// O^T accumulators * inv -> T -> row r of the wave's [32][o_row_bytes(D)] LDS image
template <typename T, int D>
__device__ __forceinline__ void stage_o_rows(char *obuf, int r, int hh, const f32x16 (&o)[D / 32], float inv) {
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            u32x2 w;
            w[0] = Elem<T>::pack2(o[db][4 * g4] * inv, o[db][4 * g4 + 1] * inv);
            w[1] = Elem<T>::pack2(o[db][4 * g4 + 2] * inv, o[db][4 * g4 + 3] * inv);
            *(u32x2 *)(obuf + r * o_row_bytes(D) + (db * 32 + 8 * g4 + 4 * hh) * 2) = w;
        }
}
// The row's destination rides in the padding of its LDS row (the lanes that store a row are not the lane that owns it):
// o_off = element offset of the row in o, row_ok = whether the row exists.  One lane half writes it.
template <int D>
__device__ __forceinline__ void stage_o_dest(char *obuf, int r, int64_t o_off, bool row_ok) {
    *(int64_t *)(obuf + r * o_row_bytes(D) + D * 2) = o_off;
    *(int32_t *)(obuf + r * o_row_bytes(D) + D * 2 + 8) = row_ok ? 1 : 0;
}
// the wave's staged rows -> o: 16-byte stores, predicated by the row's flag and by the head dim d
// (LDS reads outside the predicate: all of them are issued before the first store)
template <typename T, int D>
__device__ __forceinline__ void store_staged_rows(const char *obuf, int lane, T *o, int d) {
    constexpr int OCH = D / 8;  // 16-byte chunks of an O row
    constexpr int NCH = (32 * OCH) / 64;
    u32x4 val[NCH];
    int64_t dst[NCH];
    int32_t ok[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = lane + i * 64;
        const char *row = obuf + (c / OCH) * o_row_bytes(D);
        val[i] = *(const u32x4 *)(row + (c % OCH) * 16);
        dst[i] = *(const int64_t *)(row + D * 2);
        ok[i] = *(const int32_t *)(row + D * 2 + 8);
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int ch = (lane + i * 64) % OCH;
        if (ok[i] && ch * 8 < d) *(u32x4 *)(o + dst[i] + ch * 8) = val[i];
    }
}

}  // namespace fa
