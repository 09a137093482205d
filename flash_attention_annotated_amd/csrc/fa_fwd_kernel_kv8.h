// fa_fwd_kernel_kv8.h — gfx950 forward of 16-bit queries over an fp8 (OCP e4m3fn) KV cache: `kv_cache_dtype = fp8` of a
// serving stack.  q and o are bf16 / fp16; K and V are read from HBM as bytes, sit in LDS as bytes (half the traffic and half
// the LDS of the 16-bit tile) and are converted to T on the way to the MFMA operands.  The conversion is exact -- every finite
// e4m3fn value, subnormals and -0 included, is a bf16 and an fp16 value -- so both products are the 16-bit MFMAs with fp32
// accumulation and the kernel computes what the 16-bit kernels compute on the expanded cache.
//
// kv8_fwd_kernel is packed_rows_fwd (fa_fwd_kernel_pk.h) over the tile policy Kv8 below: the work shape, the row mapping, the
// dense / paged staging skeleton, the tile step (fa_fwd_tile_step.h) and the epilogue are pk_fwd_kernel's code, not a copy of
// it.  The rows of a workgroup are (query row, head of the GQA group) pairs of ONE kv head, 4 waves x 32 rows, 64-key tiles
// double-buffered in LDS: K / V stream once per kv head whatever h / h_k is (h == h_k: one head per workgroup).  Dense caches
// (seqused_k, kv_batch_idx, leftpad_k), paged caches (pages that are multiples of 64 keys resolve one page per tile, any other
// size one page per staged row), dense and ragged queries, causal / both window sides, softcap, split-KV.
//
// What this file owns -- the tile:
//   * LDS tile image: [64 keys][D bytes], 16-byte chunk c of key row at row * D + 16 * (c ^ kv8_swz<D>(row)).  The swizzle keeps
//     the ds_read_b128 row reads of K (16 rows per lane group, one chunk each) and the ds_read_b64_tr_b8 transposed reads of V
//     (8 rows x 32 bytes per 32 lanes) on distinct banks.
//   * K operand: a lane reads 16 contiguous bytes of its key row -- head-dim columns 32 j + 16 hh + [0, 16) -- and feeds them to
//     TWO k-steps of S^T = K.Q^T, 8 columns each.  The product contracts over the head dim, so the order is free as long as Q
//     agrees: the lane's Q fragments of k-steps 2 j and 2 j + 1 are columns 32 j + 16 hh + [0, 8) and + [8, 16) (q_col).
//   * V operand: one ds_read_b64_tr_b8 per (32 columns, 16 keys) gives the lane the 8 keys its P^T fragment holds (the lane
//     pair 2 k, 2 k + 1 of a 16-lane group addresses key (k & 3) + 8 (k >> 2) + 4 hh of the step: the accumulator's key order).
//   * e4m3 -> T: v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0, two elements per instruction.
// What FP8_CACHE selects in packed_rows_fwd -- the contract of fa_fwd_kv8:
//   * k_descale[b, h_k] multiplies the score scale (under softcap: the factor in front of the tanh; load_scales), v_descale[b, h_k]
//     the final normalisation; q_descale is not read (q is not quantised).
//   * split-KV partials follow fa_fwd_combine's convention (the merge is that entry point): a part without a visible key writes
//     LSE = -inf and carries no weight; a row without a visible key in ANY part writes +inf in every part, which the merge turns
//     into O = 0, LSE = +inf -- what the unsplit kernel writes.
//   * seqused_k is clamped to the capacity; no cu_seqlens_k and no sink (fa_fwd_kv8_validate refuses both).
// 64-bit addressing: every tile is addressed from a 64-bit base that is rebuilt per tile (cache entry or page, first key row of
// the tile, kv head); the lane offset inside a tile is below 64 row strides, and the host keeps the row stride below 2^24 bytes.
// A cache entry of 2 GiB or more is therefore read correctly; nothing is refused for its extent.
// No ALiBi, dropout, attention_chunk, qv or V head dim of its own (fa_fwd_kv8_validate).
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

// K/V tile of kv8_fwd_kernel: [64][D] e4m3 bytes, expanded to T between LDS and the MFMA operands
template <typename T, int D>
struct Kv8 {
    typedef uint8_t E;  // staged element
    static constexpr bool FP8_CACHE = true;
    static __device__ __forceinline__ int off(int row, int ch) { return kv8_off<D>(row, ch); }
    // k-step 2 j + e of lane (r, hh) contracts Q columns 32 j + 16 hh + 8 e + [0, 8): what its 16 K bytes of chunk 2 j + hh hold
    static __device__ __forceinline__ int q_col(int ks, int hh) { return (ks >> 1) * 32 + hh * 16 + (ks & 1) * 8; }
    // K: chunk 2 j + hh of key row r (+ 32): kbase ^ (32 j) (+ 32 D)
    static __device__ __forceinline__ int kbase(int r, int hh) { return kv8_off<D>(r, hh); }
    // V: lane pair k = i16 >> 1 of 16-lane group g1 addresses key (k & 3) + 8 (k >> 2) + 4 hh (+ 16 st), columns
    //    32 db + 16 g1 + 8 (i16 & 1) .. + 8: vbase ^ (32 db) (+ 16 st D).  Rows + 16 st and + 32 leave the swizzle alone.
    static __device__ __forceinline__ int vbase(int lane) {
        const int i16 = lane & 15, g1 = (lane >> 4) & 1, hh = lane >> 5, vk = i16 >> 1;
        return kv8_off<D>((vk & 3) + 8 * (vk >> 2) + 4 * hh, g1) + 8 * (i16 & 1);
    }
    // S^T += K.Q^T : two 32-key blocks, 16 K bytes = two k-steps
    static __device__ __forceinline__ void scores(const char *kbuf, int kb, const u32x4 (&qf)[D / 16], f32x16 (&s)[2]) {
#pragma unroll
        for (int j = 0; j < D / 32; ++j) {
            const int off = kb ^ (32 * j);  // = kv8_off<D>(r, 2 j + hh)
            const u32x4 kb0 = *(const u32x4 *)(kbuf + off);
            const u32x4 kb1 = *(const u32x4 *)(kbuf + off + 32 * D);
            s[0] = Elem<T>::mma(kv8_expand<T>(kb0[0], kb0[1]), qf[2 * j], s[0]);
            s[1] = Elem<T>::mma(kv8_expand<T>(kb1[0], kb1[1]), qf[2 * j], s[1]);
            s[0] = Elem<T>::mma(kv8_expand<T>(kb0[2], kb0[3]), qf[2 * j + 1], s[0]);
            s[1] = Elem<T>::mma(kv8_expand<T>(kb1[2], kb1[3]), qf[2 * j + 1], s[1]);
        }
    }
    // o += V^T.P^T for columns 32 db .. 32 db + 31: one transposed 8-byte read per 16 keys (EXEC is full: the caller's skip is
    // wave-uniform)
    static __device__ __forceinline__ void pv(const char *vbuf, int vb, int db, const u32x4 (&pf)[4], f32x16 &o) {
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const int off = (vb ^ (32 * db)) + 16 * st * D;
            const kv8_i32x2 t = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) kv8_i32x2 *)(vbuf + off));
            o = Elem<T>::mma(kv8_expand<T>((uint32_t)t[0], (uint32_t)t[1]), pf[st], o);
        }
    }
};

template <typename T, int D, bool SOFTCAP>
__global__ __launch_bounds__(PK_NWAVES * 64, 2) void kv8_fwd_kernel(const PkParams pa) {
    packed_rows_fwd<T, D, SOFTCAP, Kv8<T, D>>(pa);
}

}  // namespace fa
