// fa_rotary_emb.hip — fa_rotary_emb (include/fa_rotary.h): the rotary embedding layer, forward and (conjugate) backward, dense
// and ragged, in place or into a tensor of its own.  A translation unit of its own: the kernel set of fa_fwd_api.hip is pinned.
//
// One row (all heads of one token) by one wavefront, RAGGED_ROWS_PER_WAVE rows after each other.  The row, its sequence and
// its position are wave-uniform: they come from blockIdx and the wave id (readfirstlane), so cu_seqlens and the offsets are
// read with one address per wavefront, and whether the position lies in the tables is one uniform branch.  A 64-bit base per
// row; 32-bit offsets inside a row.
//  * vector path: the lanes lie along the row's (head, slot) items in address order, a slot being the pair of 16-byte chunks
//    that fa::rotary_slot_to rotates together.  A lane keeps the cos / sin chunk of its slot in registers while it walks the
//    heads (its slot stays the same when 64 % slots == 0), so the tables are read once per row, not once per head.
//  * element path: the same rows, the lanes on (head, pair) items with scalar accesses.
#include "../../include/fa_rotary.h"
#include "fa_rotary.h"

#include <hip/hip_runtime.h>

namespace {

using fa::RAGGED_ROWS_PER_WAVE;
using fa::RAGGED_ROWS_PER_WG;

template <typename T> __device__ __forceinline__ float to_f32(T v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f32(float v) { return (T)v; }  // round-to-nearest-even

// position of row i of sequence `seq` and whether the tables hold it
__device__ __forceinline__ bool row_position(const fa_rotary_emb_params &p, int seq, int i, int64_t &pos) {
    int64_t off = p.seqlen_offset;
    if (p.seqlen_offsets)
        off = p.offsets_int64 ? static_cast<const int64_t *>(p.seqlen_offsets)[seq]
                              : (int64_t) static_cast<const int32_t *>(p.seqlen_offsets)[seq];
    pos = off + i;
    return pos >= 0 && pos < (int64_t)p.seqlen_ro;
}

// ---- vector path: 16-bit T, tables of T, unit last strides, 16-byte aligned rows, d % 8 == 0, rotary_dim % 16 == 0 ----------
template <typename T>
__device__ __forceinline__ void rotate_row_vec(const fa_rotary_emb_params &p, int lane, int seq, int i, int64_t x_off, int64_t o_off) {
    const T *x_row = static_cast<const T *>(p.x) + x_off;
    T *o_row = static_cast<T *>(p.out) + o_off;
    const bool in_place = p.x == p.out, interleaved = p.interleaved != 0;
    const int rd = p.rotary_dim, rslots = rd >> 4;
    const int slots = in_place ? rslots : (p.d / 8 + 1) / 2;  // (in place the chunks past rotary_dim are nobody's work)
    const int items = p.h * slots;
    int64_t pos;
    const bool in_tables = row_position(p, seq, i, pos);
    const T *cos_row = static_cast<const T *>(p.cos) + pos * (rd / 2);  // (not dereferenced unless in_tables)
    const T *sin_row = static_cast<const T *>(p.sin) + pos * (rd / 2);
    const uint32_t one2 = fa::Elem<T>::pack2(1.0f, 1.0f), flip = p.conjugate ? 0x80008000u : 0u;
    uint4 cw = make_uint4(one2, one2, one2, one2), sw = make_uint4(0, 0, 0, 0);
    int have = -1;  // the slot whose cos / sin chunk cw / sw hold
    for (int it = lane; it < items; it += 64) {
        const int hd = it / slots, slot = it - hd * slots;
        const T *src = x_row + (int64_t)hd * p.x_head_stride;
        T *dst = o_row + (int64_t)hd * p.out_head_stride;
        if (slot >= rslots) {  // plain chunks behind the rotary part
            fa::rotary_slot_to<T>(src, p.d, rd, interleaved, slot, cos_row, sin_row,
                                  [&](int c, const uint4 &w) { *reinterpret_cast<uint4 *>(dst + c * 8) = w; });
            continue;
        }
        if (in_tables && slot != have) {
            cw = *reinterpret_cast<const uint4 *>(cos_row + slot * 8);
            sw = *reinterpret_cast<const uint4 *>(sin_row + slot * 8);
            sw = make_uint4(sw.x ^ flip, sw.y ^ flip, sw.z ^ flip, sw.w ^ flip);
            have = slot;
        }
        // the slot as slot 0 of the row that starts at its first chunk: rotary_slot_to then reads chunk 0 of the tables it is
        // given, which are the two registers
        const int first = interleaved ? 2 * slot : slot;
        fa::rotary_slot_to<T>(src + first * 8, p.d, interleaved ? rd - 16 * slot : rd, interleaved, 0,
                              reinterpret_cast<const T *>(&cw), reinterpret_cast<const T *>(&sw),
                              [&](int c, const uint4 &w) { *reinterpret_cast<uint4 *>(dst + (first + c) * 8) = w; });
    }
}

// ---- element path: any of the three types, tables of T or fp32, any strides --------------------------------------------------
template <typename T, typename CS>
__device__ __forceinline__ void rotate_row_elem(const fa_rotary_emb_params &p, int lane, int seq, int i, int64_t x_off, int64_t o_off) {
    const T *x_row = static_cast<const T *>(p.x) + x_off;
    T *o_row = static_cast<T *>(p.out) + o_off;
    const int rd = p.rotary_dim, half = rd >> 1;
    int64_t pos;
    const bool in_tables = row_position(p, seq, i, pos);
    const CS *cos_row = static_cast<const CS *>(p.cos) + pos * half;
    const CS *sin_row = static_cast<const CS *>(p.sin) + pos * half;
    for (int it = lane; it < p.h * half; it += 64) {
        const int hd = it / half, j = it - hd * half;
        const int j0 = p.interleaved ? 2 * j : j, j1 = p.interleaved ? 2 * j + 1 : j + half;
        const T *src = x_row + (int64_t)hd * p.x_head_stride;
        T *dst = o_row + (int64_t)hd * p.out_head_stride;
        const float x0 = to_f32(src[j0 * p.x_dim_stride]), x1 = to_f32(src[j1 * p.x_dim_stride]);
        float c = 1.0f, s = 0.0f;
        if (in_tables) {
            c = to_f32(cos_row[j]);
            s = to_f32(sin_row[j]);
            if (p.conjugate) s = -s;
        }
        dst[j0 * p.out_dim_stride] = from_f32<T>(x0 * c - x1 * s);
        dst[j1 * p.out_dim_stride] = from_f32<T>(x1 * c + x0 * s);
    }
    if (p.x == p.out) return;
    const int rest = p.d - rd;
    for (int it = lane; it < p.h * rest; it += 64) {
        const int hd = it / rest, j = rd + it - hd * rest;
        o_row[(int64_t)hd * p.out_head_stride + j * p.out_dim_stride] = x_row[(int64_t)hd * p.x_head_stride + j * p.x_dim_stride];
    }
}

// T: storage type of x / out; CS: of the tables; VEC: the vector path (CS = T)
template <typename T, typename CS, bool VEC>
__global__ __launch_bounds__(256) void rotary_emb_kernel(const fa_rotary_emb_params p) {
    const int lane = threadIdx.x & 63;
    auto row = [&](int seq, int i, int64_t x_off, int64_t o_off) __attribute__((always_inline)) {
        if constexpr (VEC) rotate_row_vec<T>(p, lane, seq, i, x_off, o_off);
        else rotate_row_elem<T, CS>(p, lane, seq, i, x_off, o_off);
    };
    if (p.cu_seqlens) {  // ragged: the 2-D grid of for_ragged_rows where max_seqlen bounds the lengths
        fa::for_ragged_rows(p.cu_seqlens, p.b, p.total, p.max_seqlen, [&](int seq, int i, int r) __attribute__((always_inline)) {
            row(seq, i, (int64_t)r * p.x_row_stride, (int64_t)r * p.out_row_stride);
        });
        return;
    }
    // dense: the b * seqlen rows in order over the workgroups
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int64_t first = (int64_t)blockIdx.x * RAGGED_ROWS_PER_WG + wave * RAGGED_ROWS_PER_WAVE, rows = (int64_t)p.b * p.seqlen;
    for (int j = 0; j < RAGGED_ROWS_PER_WAVE && first + j < rows; ++j) {
        const int seq = (int)((first + j) / p.seqlen), i = (int)((first + j) - (int64_t)seq * p.seqlen);
        row(seq, i, seq * p.x_batch_stride + i * p.x_row_stride, seq * p.out_batch_stride + i * p.out_row_stride);
    }
}

int elem_bytes(int dtype) { return dtype == FA_DTYPE_FP32 ? 4 : 2; }

bool vector_path(const fa_rotary_emb_params &p) {
    if (p.dtype == FA_DTYPE_FP32 || p.cos_dtype != p.dtype) return false;
    if (p.x_dim_stride != 1 || p.out_dim_stride != 1 || p.d % 8 != 0 || p.rotary_dim % 16 != 0 || p.rotary_dim == 0) return false;
    const int64_t strides[] = {p.x_batch_stride, p.x_row_stride, p.x_head_stride, p.out_batch_stride, p.out_row_stride, p.out_head_stride};
    for (int i = 0; i < 6; ++i)
        if (strides[i] % 8 != 0 && !(p.cu_seqlens && i % 3 == 0)) return false;  // (no batch stride with cu_seqlens)
    const void *ptrs[] = {p.x, p.out, p.cos, p.sin};
    for (const void *q : ptrs)
        if (reinterpret_cast<uintptr_t>(q) % 16 != 0) return false;
    return true;
}

}  // namespace

extern "C" {

uint32_t fa_rotary_emb_params_size(void) { return (uint32_t)sizeof(fa_rotary_emb_params); }

int fa_rotary_emb_validate(const fa_rotary_emb_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_rotary_emb_params)) return FA_ERR_BAD_ABI;
    if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16 && p->dtype != FA_DTYPE_FP32) return FA_ERR_BAD_DTYPE;
    if (p->cos_dtype != p->sin_dtype) return FA_ERR_BAD_DTYPE;
    if (p->cos_dtype != p->dtype && p->cos_dtype != FA_DTYPE_FP32) return FA_ERR_BAD_DTYPE;
    if (p->b < 0 || p->seqlen < 0 || p->total < 0 || p->max_seqlen < 0 || p->h < 0 || p->seqlen_ro < 0) return FA_ERR_BAD_SHAPE;
    if (p->d <= 0 || p->d > 256) return FA_ERR_BAD_HEAD_DIM;
    if (p->rotary_dim < 0 || p->rotary_dim % 2 != 0 || p->rotary_dim > p->d) return FA_ERR_BAD_SHAPE;
    if (p->cu_seqlens && p->max_seqlen <= 0) return FA_ERR_BAD_SHAPE;
    if (!p->x || !p->out || !p->cos || !p->sin) return FA_ERR_NULL_POINTER;    const int eb = elem_bytes(p->dtype), tb = elem_bytes(p->cos_dtype);  // scalar accesses need their natural alignment
    if (reinterpret_cast<uintptr_t>(p->x) % eb != 0 || reinterpret_cast<uintptr_t>(p->out) % eb != 0) return FA_ERR_BAD_STRIDE;
    if (reinterpret_cast<uintptr_t>(p->cos) % tb != 0 || reinterpret_cast<uintptr_t>(p->sin) % tb != 0) return FA_ERR_BAD_STRIDE;
    if (reinterpret_cast<uintptr_t>(p->cu_seqlens) % 4 != 0) return FA_ERR_BAD_STRIDE;
    if (reinterpret_cast<uintptr_t>(p->seqlen_offsets) % (p->offsets_int64 ? 8 : 4) != 0) return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int fa_rotary_emb(const fa_rotary_emb_params *p, void *stream_) {
    const int st = fa_rotary_emb_validate(p);
    if (st != FA_OK) return st;
    const int64_t rows = p->cu_seqlens ? (int64_t)p->total : (int64_t)p->b * p->seqlen;
    if (rows == 0 || p->b == 0 || p->h == 0) return FA_OK;
    if (p->x == p->out && p->rotary_dim == 0) return FA_OK;
    dim3 grid;
    size_t smem = 0;
    fa_rotary_emb_params kp = *p;
    if (p->cu_seqlens) {
        if (kp.b > 65535) kp.max_seqlen = 0;  // (grid.y: the flat form of for_ragged_rows, which finds the sequence by search)
        fa::ragged_launch_shape(kp.b, kp.total, kp.max_seqlen, 0, grid, smem);
    } else {
        grid = dim3((unsigned)((rows + RAGGED_ROWS_PER_WG - 1) / RAGGED_ROWS_PER_WG));
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const bool vec = vector_path(*p), cs32 = p->cos_dtype == FA_DTYPE_FP32;
#define FA_ROTARY_EMB_LAUNCH(T, CS, VEC) hipLaunchKernelGGL((rotary_emb_kernel<T, CS, VEC>), grid, dim3(256), smem, stream, kp)
    if (p->dtype == FA_DTYPE_FP32) FA_ROTARY_EMB_LAUNCH(float, float, false);
    else if (p->dtype == FA_DTYPE_BF16) {
        if (vec) FA_ROTARY_EMB_LAUNCH(__bf16, __bf16, true);
        else if (cs32) FA_ROTARY_EMB_LAUNCH(__bf16, float, false);
        else FA_ROTARY_EMB_LAUNCH(__bf16, __bf16, false);
    } else {
        if (vec) FA_ROTARY_EMB_LAUNCH(_Float16, _Float16, true);
        else if (cs32) FA_ROTARY_EMB_LAUNCH(_Float16, float, false);
        else FA_ROTARY_EMB_LAUNCH(_Float16, _Float16, false);
    }
#undef FA_ROTARY_EMB_LAUNCH
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

}  // extern "C"
