// fa_kvcache_append_kv8.h — what the two quantising appends to an fp8 (e4m3) KV cache share: fa_kvcache_append_kv8
// (fa_kvcache_append_kv8.hip, d <= 128 with d_v = d) and fa_kvcache_append_qv8 (fa_kvcache_append_qv8.hip, the MLA shape: d <= 64
// beside d_v in [256, 512]).  One conversion, one placement of a new row, one distribution of the rows over the wavefronts, one
// validation and one launch shape; the units differ in the head-dim rule and in how a wavefront's lanes cover a row.
#pragma once
#include "fa_fwd.h"
#include "fa_rotary.h"

#include <algorithm>

namespace fa {

// 8 elements of T (one 16-byte chunk) -> 8 e4m3 bytes:  byte = e4m3fn_rne(min(max(float(x) * inv, -448), 448)).
// v_med3_f32 is the clamp (+-inf -> +-448, -0 keeps its sign), v_cvt_pk_fp8_f32 rounds to nearest even (subnormals included).
template <typename T>
__device__ __forceinline__ uint2 quantise8(uint4 w, float inv) {
    float x[8];
    fa::unpack8<T>(w, x);
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = __builtin_amdgcn_fmed3f(x[j] * inv, -448.0f, 448.0f);
    int lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], lo, true);
    int hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[4], x[5], 0, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[6], x[7], hi, true);
    return make_uint2((uint32_t)lo, (uint32_t)hi);
}

// One new row as its wavefront sees it: source and destination of head 0 (64-bit addresses from a per-row base), the rotary
// tables at the row's position and the descale rows of its sequence.  Everything looked up per sequence -- fill level, cache
// entry, page, rotary position, the descale rows -- is wave-uniform.
template <typename T>
struct Kv8AppendRow {
    const T *ks, *vs;
    uint8_t *kd, *vd;
    int rd;             // rotary_dim, 0 without rotary
    const T *cr, *sr;
    const float *kds, *vds;  // NULL = 1.0
};

// false: the row lies past the capacity and is dropped (wave-uniform)
template <typename T>
__device__ __forceinline__ bool kv8_append_row(const fa_kvcache_append_kv8_params &p, int seq, int i, int64_t k_off, int64_t v_off,
                                               Kv8AppendRow<T> &r) {
    const int fill = p.cache_seqlens[seq];
    int dst_row = fill + i;
    if (dst_row < 0 || dst_row >= p.seqlen_cache) return false;
    const int pos = (p.rotary_seqlens ? p.rotary_seqlens[seq] : fill) + i;
    int cb = p.cache_batch_idx ? p.cache_batch_idx[seq] : seq;
    if (p.block_table) {
        cb = p.block_table[seq * p.block_table_batch_stride + dst_row / p.page_block_size];
        dst_row %= p.page_block_size;
    }
    r.ks = (const T *)p.k_new + k_off;
    r.vs = (const T *)p.v_new + v_off;
    r.kd = (uint8_t *)p.k_cache + (int64_t)cb * p.kcache_batch_stride + (int64_t)dst_row * p.kcache_row_stride;
    r.vd = (uint8_t *)p.v_cache + (int64_t)cb * p.vcache_batch_stride + (int64_t)dst_row * p.vcache_row_stride;
    r.rd = p.rotary_cos ? p.rotary_dim : 0;
    r.cr = (const T *)p.rotary_cos + (int64_t)pos * (r.rd / 2);
    r.sr = (const T *)p.rotary_sin + (int64_t)pos * (r.rd / 2);
    r.kds = p.k_descale ? p.k_descale + seq * p.k_descale_batch_stride : nullptr;
    r.vds = p.v_descale ? p.v_descale + seq * p.v_descale_batch_stride : nullptr;
    return true;
}

// The body of both kernels (256 threads): the fill levels behind the append, then row(seq, i, k_off, v_off) for every new row
// by one wavefront.  Dense rows (cu_seqlens_k_new == NULL): the wavefronts of a flat grid stride over the b * seqlen_new rows;
// ragged rows: for_ragged_rows, the launch shapes of fa_kvcache_append_varlen.
template <typename Row>
__device__ __forceinline__ void kv8_append_rows(const fa_kvcache_append_kv8_params &p, Row &&row) {
    const bool ragged = p.cu_seqlens_k_new != nullptr;
    // the fill levels behind the append: one entry per thread of the first workgroups (the grid holds >= b threads)
    const int64_t gid = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
    if (p.seqused_out && gid < p.b) {
        const int s = (int)gid;
        const int len = ragged ? p.cu_seqlens_k_new[s + 1] - p.cu_seqlens_k_new[s] : p.seqlen_new;
        p.seqused_out[s] = min(p.cache_seqlens[s] + len, p.seqlen_cache);
    }
    if (ragged) {
        // (always_inline: for_ragged_rows calls its body from several places, and a call would put the params on the stack)
        fa::for_ragged_rows(p.cu_seqlens_k_new, p.b, p.total_k_new, p.max_seqlen_k_new,
                            [&](int seq, int i, int r) __attribute__((always_inline)) {
            row(seq, i, (int64_t)r * p.knew_row_stride, (int64_t)r * p.vnew_row_stride);
        });
        return;
    }
    const int64_t rows = (int64_t)p.b * p.seqlen_new, waves = (int64_t)gridDim.x * 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += waves) {
        const int seq = (int)(r / p.seqlen_new), i = (int)(r % p.seqlen_new);
        row(seq, i, seq * p.knew_batch_stride + i * p.knew_row_stride, seq * p.vnew_batch_stride + i * p.vnew_row_stride);
    }
}

inline bool kv8_append_misaligned(const void *ptr, uintptr_t to) { return reinterpret_cast<uintptr_t>(ptr) % to != 0; }

// Every rule of both entry points in one order; wide_v picks the head-dim rule: false -- d <= 128, d_v 0 or d (what fa_fwd_kv8
// reads); true -- d <= 64 beside d_v in [256, 512] (what fa_fwd_qv8 reads).
inline int kv8_append_validate(const fa_kvcache_append_kv8_params *p, bool wide_v) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_kvcache_append_kv8_params)) return FA_ERR_BAD_ABI;
    if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16) return FA_ERR_BAD_DTYPE;
    const bool ragged = p->cu_seqlens_k_new != nullptr;
    if (p->b <= 0 || p->h_k <= 0 || p->seqlen_cache < 0) return FA_ERR_BAD_SHAPE;
    if (ragged ? (p->total_k_new < 0 || p->max_seqlen_k_new < 0) : p->seqlen_new < 0) return FA_ERR_BAD_SHAPE;
    if (p->d <= 0 || p->d > (wide_v ? 64 : 128) || p->d % 16 != 0) return FA_ERR_BAD_HEAD_DIM;
    if (wide_v ? (p->d_v < 256 || p->d_v > 512 || p->d_v % 16 != 0) : (p->d_v != 0 && p->d_v != p->d)) return FA_ERR_BAD_HEAD_DIM;
    if (!p->cache_seqlens || (ragged && !p->seqused_out)) return FA_ERR_NULL_POINTER;
    if (p->seqused_out == p->cache_seqlens) return FA_ERR_BAD_SHAPE;
    const int64_t rows = ragged ? p->total_k_new : (int64_t)p->b * p->seqlen_new;
    if (rows > 0 && (!p->k_new || !p->v_new || !p->k_cache || !p->v_cache)) return FA_ERR_NULL_POINTER;
    if (p->block_table && (p->page_block_size <= 0 || p->cache_batch_idx)) return FA_ERR_BAD_SHAPE;
    if (p->block_table && (p->block_table_batch_stride < 0 || p->block_table_batch_stride > 0x7fffffff)) return FA_ERR_BAD_STRIDE;
    if (p->rotary_cos || p->rotary_sin) {
        if (!p->rotary_cos || !p->rotary_sin) return FA_ERR_NULL_POINTER;
        if (p->rotary_dim <= 0 || p->rotary_dim > p->d || p->rotary_dim % 16 != 0) return FA_ERR_BAD_SHAPE;
        if (kv8_append_misaligned(p->rotary_cos, 16) || kv8_append_misaligned(p->rotary_sin, 16)) return FA_ERR_BAD_STRIDE;
    }
    // new rows: 16-byte chunks of 16-bit elements (the batch strides are read in the dense form only)
    const int64_t new_strides[] = {p->knew_row_stride, p->knew_head_stride, p->vnew_row_stride, p->vnew_head_stride,
                                   ragged ? 0 : p->knew_batch_stride, ragged ? 0 : p->vnew_batch_stride};
    for (int64_t s : new_strides)
        if (s % 8 != 0) return FA_ERR_BAD_STRIDE;
    if (kv8_append_misaligned(p->k_new, 16) || kv8_append_misaligned(p->v_new, 16)) return FA_ERR_BAD_STRIDE;
    // the cache: 8-byte stores of e4m3 bytes, strides in bytes
    const int64_t cache_strides[] = {p->kcache_batch_stride, p->kcache_row_stride, p->kcache_head_stride,
                                     p->vcache_batch_stride, p->vcache_row_stride, p->vcache_head_stride};
    for (int64_t s : cache_strides)
        if (s % 8 != 0) return FA_ERR_BAD_STRIDE;
    if (kv8_append_misaligned(p->k_cache, 8) || kv8_append_misaligned(p->v_cache, 8)) return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

// The launch of a validated call: one wavefront per new row, 4 to a workgroup; `fp16` / `bf16` are the unit's two kernels.
using Kv8AppendKernel = void (*)(const fa_kvcache_append_kv8_params);
inline int kv8_append_launch(const fa_kvcache_append_kv8_params *p, Kv8AppendKernel fp16, Kv8AppendKernel bf16, void *stream_) {
    fa_kvcache_append_kv8_params kp = *p;
    const bool ragged = kp.cu_seqlens_k_new != nullptr;
    dim3 grid;
    size_t smem = 0;
    if (ragged) {
        if (kp.b > 65535 || kp.total_k_new == 0) kp.max_seqlen_k_new = 0;  // (grid.y; no rows: the launch only writes seqused_out)
        fa::ragged_launch_shape(kp.b, kp.total_k_new, kp.max_seqlen_k_new, kp.b, grid, smem);
    } else {
        const int64_t rows = (int64_t)kp.b * kp.seqlen_new;
        if (rows == 0 && !kp.seqused_out) return FA_OK;
        const int64_t fill_blocks = kp.seqused_out ? ((int64_t)kp.b + 255) / 256 : 0;  // (seqused_out: >= b threads)
        grid = dim3((unsigned)std::max<int64_t>({1, std::min<int64_t>((rows + 3) / 4, 256 * 8), fill_blocks}));
    }
    hipLaunchKernelGGL(kp.dtype == FA_DTYPE_FP16 ? fp16 : bf16, grid, dim3(256), smem, static_cast<hipStream_t>(stream_), kp);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

}  // namespace fa
