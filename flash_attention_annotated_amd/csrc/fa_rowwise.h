// fa_rowwise.h — what the row-streaming units (fa_norm.hip, fa_dropout_norm.hip, fa_xent.hip, fa_act.hip, fa_sample.hip) share: the chunk
// loads and stores between a tensor's dtype and fp32 registers, the sums over a wavefront and a workgroup, the exclusive scan
// over a workgroup, the avalanche of the counter hashes, the ordered reduce of fp32 partial rows, and the host's dtype and
// alignment predicates.  Everything here is an inline function: including it
// adds no kernel to a unit and renames none, so the kernel set of every unit stays what its tests pin.
#pragma once

#include "../../include/fa_fwd.h"

#include <hip/hip_runtime.h>

namespace fa_row {

constexpr int WAVE = 64;
constexpr int MAX_WAVES = 16;  // of a workgroup

__host__ __device__ __forceinline__ int esize(int dt) { return dt == FA_DTYPE_FP32 ? 4 : 2; }

__device__ __forceinline__ const char *row_of(const void *base, int dt, int64_t row, int64_t stride) {
    return static_cast<const char *>(base) + row * stride * esize(dt);
}
__device__ __forceinline__ char *row_of(void *base, int dt, int64_t row, int64_t stride) {
    return static_cast<char *>(base) + row * stride * esize(dt);
}

// CW elements at column ucol + lcol of a row of dtype `dt`, as fp32: 16-byte accesses where CW > 1.  ucol is the wave-uniform
// part of the column: with a uniform row it goes into the scalar base of the access, and the lane's part is one 32-bit offset
// for all chunks of a thread.  The offsets are added to a pointer of the element's type, which is what keeps that split
template <int CW>
__device__ __forceinline__ void load_chunk(const void *row, int dt, int ucol, int lcol, float (&v)[CW]) {
    if (dt == FA_DTYPE_FP32) {
        const float *p = static_cast<const float *>(row) + ucol + (uint32_t)lcol;
        if constexpr (CW == 1) {
            v[0] = *p;
        } else {
#pragma unroll
            for (int i = 0; i < CW; i += 4) {
                const float4 q = *reinterpret_cast<const float4 *>(p + i);
                v[i] = q.x; v[i + 1] = q.y; v[i + 2] = q.z; v[i + 3] = q.w;
            }
        }
        return;
    }
    const uint16_t *p = static_cast<const uint16_t *>(row) + ucol + (uint32_t)lcol;
    uint32_t h[CW];
    if constexpr (CW == 8) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p);
        h[0] = q.x & 0xffffu; h[1] = q.x >> 16; h[2] = q.y & 0xffffu; h[3] = q.y >> 16;
        h[4] = q.z & 0xffffu; h[5] = q.z >> 16; h[6] = q.w & 0xffffu; h[7] = q.w >> 16;
    } else if constexpr (CW == 4) {
        const uint2 q = *reinterpret_cast<const uint2 *>(p);
        h[0] = q.x & 0xffffu; h[1] = q.x >> 16; h[2] = q.y & 0xffffu; h[3] = q.y >> 16;
    } else {
        h[0] = *p;
    }
    if (dt == FA_DTYPE_BF16) {
#pragma unroll
        for (int i = 0; i < CW; ++i) v[i] = __uint_as_float(h[i] << 16);
    } else {
#pragma unroll
        for (int i = 0; i < CW; ++i) v[i] = (float)__builtin_bit_cast(_Float16, (uint16_t)h[i]);
    }
}

// ... and back: one rounding to nearest even
template <int CW>
__device__ __forceinline__ void store_chunk(void *row, int dt, int ucol, int lcol, const float (&v)[CW]) {
    if (dt == FA_DTYPE_FP32) {
        float *p = static_cast<float *>(row) + ucol + (uint32_t)lcol;
        if constexpr (CW == 1) {
            *p = v[0];
        } else {
#pragma unroll
            for (int i = 0; i < CW; i += 4) *reinterpret_cast<float4 *>(p + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
        }
        return;
    }
    uint32_t h[CW];
    if (dt == FA_DTYPE_BF16) {
#pragma unroll
        for (int i = 0; i < CW; ++i) h[i] = __builtin_bit_cast(uint16_t, (__bf16)v[i]);
    } else {
#pragma unroll
        for (int i = 0; i < CW; ++i) h[i] = __builtin_bit_cast(uint16_t, (_Float16)v[i]);
    }
    uint16_t *p = static_cast<uint16_t *>(row) + ucol + (uint32_t)lcol;
    if constexpr (CW == 8) {
        *reinterpret_cast<uint4 *>(p) = make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
    } else if constexpr (CW == 4) {
        *reinterpret_cast<uint2 *>(p) = make_uint2(h[0] | h[1] << 16, h[2] | h[3] << 16);
    } else {
        *p = (uint16_t)h[0];
    }
}

// the same at a formed address q
template <int CW>
__device__ __forceinline__ void load_chunk(const void *q, int dt, float (&v)[CW]) {
    load_chunk<CW>(q, dt, 0, 0, v);
}
template <int CW>
__device__ __forceinline__ void store_chunk(void *q, int dt, const float (&v)[CW]) {
    store_chunk<CW>(q, dt, 0, 0, v);
}

// v as the value a tensor of dtype `dt` holds after one rounding
template <int CW>
__device__ __forceinline__ void round_to(int dt, float (&v)[CW]) {
    if (dt == FA_DTYPE_BF16) {
#pragma unroll
        for (int i = 0; i < CW; ++i) v[i] = (float)(__bf16)v[i];
    } else if (dt == FA_DTYPE_FP16) {
#pragma unroll
        for (int i = 0; i < CW; ++i) v[i] = (float)(_Float16)v[i];
    }
}

__device__ __forceinline__ float load_one(const void *base, int dt, int64_t i) {
    float v[1];
    load_chunk<1>(static_cast<const char *>(base) + i * esize(dt), dt, v);
    return v[0];
}

// a butterfly of cross-lane swaps over all 64 lanes: every lane gets the sum
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// every thread of the team gets the team's sums of v[0..NV).  The caller says whether a wavefront is the whole team: by
// `team_wave` where it plans teams (several per workgroup), by SMALL_WG where the team is always the workgroup, which may be a
// single wavefront.  Else the team is the workgroup, all of whose threads call this together; `phase` picks the LDS slot, the
// two in turn, so that a slot is not written again before every wavefront has passed the barrier of the sum after the one
// that read it
template <int NV, bool SMALL_WG = false>
__device__ __forceinline__ void team_sum(float (&v)[NV], bool team_wave, float (&red)[2][NV][MAX_WAVES], int &phase) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    if (team_wave) return;
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (SMALL_WG && nw == 1) return;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) red[phase][i][wave] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float s = 0.0f;
        for (int w = 0; w < nw; ++w) s += red[phase][i][w];
        v[i] = s;
    }
    phase ^= 1;
}

// the exclusive prefix sum of v over the threads of the workgroup (whole wavefronts) in thread order, and the sum over all of
// them in `total`; every thread calls it together.  64-bit integers: the sums are exact, whatever the order.  `part` is free
// again on return
__device__ __forceinline__ uint64_t shfl_up_64(uint64_t v, int o) {
    const uint32_t lo = __shfl_up((uint32_t)v, o, WAVE), hi = __shfl_up((uint32_t)(v >> 32), o, WAVE);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t wg_exclusive_scan(uint64_t v, uint64_t (&part)[MAX_WAVES], uint64_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint64_t up = shfl_up_64(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == WAVE - 1) part[wave] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
    for (int w = 0; w < nw; ++w) {
        const uint64_t s = part[w];
        before += w < wave ? s : 0;
        all += s;
    }
    __syncthreads();
    total = all;
    return before + inc - v;
}

// ---- counters to bits ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
    x ^= x >> 16; x *= 0x7FEB352Du;
    x ^= x >> 15; x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}
// rng_state = {seed, offset} on the device as one word
__device__ __forceinline__ uint32_t seed_mix(const uint64_t *rng_state) {
    const uint64_t seed = rng_state[0], off = rng_state[1];
    uint32_t x = (uint32_t)seed ^ (uint32_t)(seed >> 32) * 0x27D4EB2Fu ^ (uint32_t)off * 0xC2B2AE3Du ^ (uint32_t)(off >> 32);
    x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 12;
    return x;
}

constexpr int REDUCE_COLS = 64;  // columns per workgroup of an ordered reduce

// The ordered reduce of the P fp32 partial rows src[0..P)[N], by a workgroup of MAX_WAVES wavefronts over the REDUCE_COLS
// columns of blockIdx.x: dst[col] = their sum, of dtype `dt`.  Wavefront v adds the rows v, v + 16, ..., the 16 sums are added
// in wave order.  A fixed order: the same bits every time.  A kernel calls it once per column sum it has, with the same `comb`
__device__ __forceinline__ void reduce_partial_rows(const float *src, int P, int N, void *dst, int dt,
                                                    float (&comb)[MAX_WAVES][REDUCE_COLS]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = blockIdx.x * REDUCE_COLS + lane;
    float s = 0.0f;
    if (col < N)
        for (int q = wave; q < P; q += MAX_WAVES) s += src[(int64_t)q * N + col];
    comb[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && col < N) {
        float total[1] = {0.0f};
        for (int v = 0; v < MAX_WAVES; ++v) total[0] += comb[v][lane];
        store_chunk<1>(dst, dt, 0, col, total);
    }
    __syncthreads();
}

// ---- host -------------------------------------------------------------------------------------------------------------------
inline bool known_dtype(int dt) { return dt == FA_DTYPE_FP16 || dt == FA_DTYPE_BF16 || dt == FA_DTYPE_FP32; }

// NULL passes: an absent tensor constrains nothing
inline bool aligned_to(const void *q, int bytes) { return reinterpret_cast<uintptr_t>(q) % bytes == 0; }
// 16-byte accesses of a tensor of rows need its base and its pitch in bytes to be multiples of 16 ...
inline bool rows_16_bytes(const void *q, int dt, int64_t stride) { return !q || (aligned_to(q, 16) && (stride * esize(dt)) % 16 == 0); }
// ... and of a vector of N elements whose tail is not taken by elements, its base and its length in bytes
inline bool vector_16_bytes(const void *q, int dt, int N) { return !q || (aligned_to(q, 16) && ((int64_t)N * esize(dt)) % 16 == 0); }

}  // namespace fa_row
