// fa_rotary.h — rotary embedding on 16-byte chunks (8 elements of a 16-bit type), and the ragged-row work shape, shared by the
// 16-bit passes of fa_fwd_api.hip (rotary_kernel, kvcache_append_kernel and their ragged forms) and the quantising append of
// fa_kvcache_append_kv8.hip: one rotation code, so what lands in an fp8 cache is the quantisation of what the 16-bit append
// writes.
#pragma once
#include "fa_fwd_kernel.h"

#include <algorithm>

namespace fa {

// ---- 16-byte chunks (8 elements), fp32 math, round to the storage type ---------------------------------------------
template <typename T>
__device__ __forceinline__ void unpack8(const uint4 &w, float (&x)[8]) {
    const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (sizeof(T) == 2 && __is_same(T, __bf16)) {
            x[2 * j] = __uint_as_float(u[j] << 16);
            x[2 * j + 1] = __uint_as_float(u[j] & 0xffff0000u);
        } else {
            x[2 * j] = (float)__builtin_bit_cast(_Float16, (uint16_t)(u[j] & 0xffffu));
            x[2 * j + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(u[j] >> 16));
        }
    }
}
template <typename T>
__device__ __forceinline__ uint4 pack8(const float (&x)[8]) {
    uint32_t u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = fa::Elem<T>::pack2(x[2 * j], x[2 * j + 1]);
    return make_uint4(u[0], u[1], u[2], u[3]);
}
// One work item = one pair of chunks.  Interleaved: chunk c holds pairs (2j, 2j+1): rotated in place with cos/sin
// [4c, 4c+4).  Otherwise chunk c (< rotary_dim/16) pairs with chunk c + rotary_dim/16, cos/sin [8c, 8c+8).
// Chunks past rotary_dim are passed through.  `slot` enumerates ceil(d/16) slots per (row, head): slot j covers chunk j (first
// half of the rotary part), its partner, and -- past the rotary part -- the plain chunks 2 per slot.
// put(c, w) receives chunk c of the result as 8 elements of T (rotated chunks rounded to T): the 16-bit passes store it, the
// quantising append converts it further.
template <typename T, typename Put>
__device__ __forceinline__ void rotary_slot_to(const T *src, int d, int rd, bool interleaved, int slot, const T *cos_row,
                                               const T *sin_row, Put &&put) {
    const int chunks = d >> 3, rchunks = rd >> 3;
    int c0, c1;  // the two chunks of this slot (c1 = -1: none)
    if (slot < rchunks / 2 + (rchunks & 1)) {
        if (interleaved) { c0 = 2 * slot; c1 = 2 * slot + 1 < rchunks ? 2 * slot + 1 : -1; }
        else { c0 = slot; c1 = slot + rchunks / 2; }
    } else {  // plain chunks behind the rotary part, two per slot
        const int k = slot - (rchunks / 2 + (rchunks & 1));
        c0 = rchunks + 2 * k;
        c1 = c0 + 1 < chunks ? c0 + 1 : -1;
        if (c0 >= chunks) return;
        put(c0, *reinterpret_cast<const uint4 *>(src + c0 * 8));
        if (c1 >= 0) put(c1, *reinterpret_cast<const uint4 *>(src + c1 * 8));
        return;
    }
    if (interleaved) {
        const int cs[2] = {c0, c1};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int c = cs[q];
            if (c < 0) continue;
            float x[8], cv[8], sv[8], y[8];
            unpack8<T>(*reinterpret_cast<const uint4 *>(src + c * 8), x);
            // 4 cos/sin values for this chunk: load the aligned 8 and pick the half
            unpack8<T>(*reinterpret_cast<const uint4 *>(cos_row + (c >> 1) * 8), cv);
            unpack8<T>(*reinterpret_cast<const uint4 *>(sin_row + (c >> 1) * 8), sv);
            const int h = (c & 1) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float co = cv[h + j], si = sv[h + j];
                y[2 * j] = x[2 * j] * co - x[2 * j + 1] * si;
                y[2 * j + 1] = x[2 * j + 1] * co + x[2 * j] * si;
            }
            put(c, pack8<T>(y));
        }
    } else {
        float x1[8], x2[8], cv[8], sv[8], y1[8], y2[8];
        unpack8<T>(*reinterpret_cast<const uint4 *>(src + c0 * 8), x1);
        unpack8<T>(*reinterpret_cast<const uint4 *>(src + c1 * 8), x2);
        unpack8<T>(*reinterpret_cast<const uint4 *>(cos_row + c0 * 8), cv);
        unpack8<T>(*reinterpret_cast<const uint4 *>(sin_row + c0 * 8), sv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            y1[j] = x1[j] * cv[j] - x2[j] * sv[j];
            y2[j] = x2[j] * cv[j] + x1[j] * sv[j];
        }
        put(c0, pack8<T>(y1));
        put(c1, pack8<T>(y2));
    }
}
// ... into a 16-bit destination row of the same layout (dst may alias src)
template <typename T>
__device__ __forceinline__ void rotary_slot(const T *src, T *dst, int d, int rd, bool interleaved, int slot,
                                            const T *cos_row, const T *sin_row) {
    rotary_slot_to<T>(src, d, rd, interleaved, slot, cos_row, sin_row,
                      [&](int c, const uint4 &w) { *reinterpret_cast<uint4 *>(dst + c * 8) = w; });
}

// ---- ragged rows (a (total, h, d) tensor with cu_seqlens) -> wavefronts ------------------------------------------------------
// Shared by kvcache_append_varlen_kernel, rotary_varlen_kernel and kvcache_append_kv8_kernel.  One workgroup = 4 wavefronts x RAGGED_ROWS_PER_WAVE
// consecutive rows; a wavefront works on one row at a time, its lanes on the row's 16-byte chunks in address order.  The row,
// its sequence and everything looked up per sequence (fill level, cache entry, page, rotary position) are wave-uniform:
// they come from blockIdx and the wave id through readfirstlane, so the lookups are one address per wavefront, not a gather.
//  * max_len > 0 (the caller knows an upper bound of the lengths): grid (row blocks of max_len) x b, blockIdx.y = sequence;
//  * max_len == 0: flat row blocks; cu_seqlens (b + 1 entries) is read once per workgroup into LDS and every wavefront
//    finds the sequence of its row by a binary search there (in global memory past RAGGED_LDS_SEQS sequences).
// Nothing loops over the batch.  body(seq, i, row) is called with row = cu[seq] + i, i < the sequence's length.
constexpr int RAGGED_ROWS_PER_WAVE = 4, RAGGED_ROWS_PER_WG = 4 * RAGGED_ROWS_PER_WAVE, RAGGED_LDS_SEQS = 16383;

__device__ __forceinline__ int ragged_find_seq(const int32_t *cu, int b, int row) {
    int lo = 0, hi = b;  // the last s in [0, b) with cu[s] <= row: empty sequences in front of it are stepped over
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (__builtin_amdgcn_readfirstlane(cu[mid]) <= row) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <typename F>
__device__ __forceinline__ void for_ragged_rows(const int32_t *__restrict__ cu, int b, int total, int max_len, F &&body) {
    extern __shared__ int32_t ragged_cu_lds[];
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int first = (int)blockIdx.x * RAGGED_ROWS_PER_WG + wave * RAGGED_ROWS_PER_WAVE;
    if (max_len > 0) {
        const int seq = blockIdx.y, c0 = cu[seq], len = min(cu[seq + 1], total) - c0;
        for (int j = 0; j < RAGGED_ROWS_PER_WAVE && first + j < len; ++j) body(seq, first + j, c0 + first + j);
        return;
    }
    const bool in_lds = b <= RAGGED_LDS_SEQS;  // (uniform: a kernel argument)
    if (in_lds) {
        for (int t = threadIdx.x; t <= b; t += blockDim.x) ragged_cu_lds[t] = cu[t];
        __syncthreads();
    }
    const int end = min(total, in_lds ? ragged_cu_lds[b] : cu[b]);
    for (int j = 0; j < RAGGED_ROWS_PER_WAVE && first + j < end; ++j) {
        const int row = first + j;
        const int seq = in_lds ? ragged_find_seq(ragged_cu_lds, b, row) : ragged_find_seq(cu, b, row);
        const int c0 = __builtin_amdgcn_readfirstlane(in_lds ? ragged_cu_lds[seq] : cu[seq]);
        body(seq, row - c0, row);
    }
}

// grid and LDS bytes of a for_ragged_rows launch over `total` rows of `b` sequences whose grid also holds `min_threads` threads
// (the 2-D grid has a workgroup per sequence: at least b threads)
inline void ragged_launch_shape(int b, int total, int max_len, int64_t min_threads, dim3 &grid, size_t &smem) {
    if (max_len > 0) {
        grid = dim3((unsigned)((max_len + RAGGED_ROWS_PER_WG - 1) / RAGGED_ROWS_PER_WG), (unsigned)b);
        smem = 0;
    } else {
        const int64_t row_blocks = ((int64_t)total + RAGGED_ROWS_PER_WG - 1) / RAGGED_ROWS_PER_WG;
        grid = dim3((unsigned)std::max<int64_t>({1, row_blocks, (min_threads + 255) / 256}));
        smem = b <= RAGGED_LDS_SEQS ? sizeof(int32_t) * ((size_t)b + 1) : 0;
    }
}

}  // namespace fa
