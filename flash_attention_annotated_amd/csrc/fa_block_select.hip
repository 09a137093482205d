// fa_block_select.hip — the producer half of block-sparse decode over a KV cache (include/fa_block_select.h): the per-block
// minimum / maximum summaries of the keys, and the Quest selection that writes the lists the sparse read takes.  A translation
// unit of its own.  The chunk loads, the workgroup scan and the host predicates are fa_rowwise.h's; the order-preserving key of a
// score is the one of fa_sample_device.h, whose descent over histograms in LDS the selection follows with a radix of 8 bits.
//
// summary_update_kernel<L>: one workgroup per (block of the written range, kv head, batch entry).  L lanes hold the 8-channel
//   chunks of a row (L = 16: d > 64, else 8), 256 / L row groups walk the rows, LDS folds the groups, the first L threads merge
//   with the stored summary where the block began before the range, and store.
// block_score_kernel<L>: one workgroup per (chunk of 1024 / L blocks, kv head, batch entry).  The s_q * g query rows lie in LDS as
//   they are; a group of L lanes holds min and max of 4 blocks in registers (8 loads of 16 bytes in flight per lane), forms
//   max(q * min, q * max) over its 8 channels per row, a butterfly over the L lanes adds them up, and the rows are reduced.
// block_select_kernel: one workgroup per (kv head, batch entry): keys of the scores in LDS, the cut by four 8-bit passes, the ties
//   by index, the ascending compaction by two scans.  Integer logic only: a NaN score is a key like any other.
#include "../../include/fa_block_select.h"
#include "fa_sample_device.h"

#include <cstdio>

namespace {

using namespace fa_row;
using fa_sample_dev::full_key;

constexpr int THREADS = 256;               // of the update and the scoring
constexpr int NB = 4;                      // blocks a lane group scores at once
constexpr int CW = 8;                      // channels per lane: 16 bytes of a 16-bit row, 8 of an e4m3 one
constexpr int SELECT_SMALL = 256, SELECT_LARGE = 1024, SELECT_SMALL_BLOCKS = 1024;  // the selection's workgroup by max_blocks
constexpr int RADIX_BITS = 8, BINS = 1 << RADIX_BITS;

__host__ __device__ constexpr int lanes_of(int d) { return d > 64 ? 16 : 8; }
__host__ __device__ constexpr int score_chunk(int L) { return THREADS / L * NB; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// 8 channels at `q` as fp32: a 16-byte load of a 16-bit row, or an 8-byte load of e4m3 bytes, each value converted exactly
__device__ __forceinline__ void load8(const char *q, int dt, float (&v)[CW]) {
    if (dt == FA_DTYPE_FP8_E4M3) {
        const uint2 w = *reinterpret_cast<const uint2 *>(q);
        const auto a = __builtin_amdgcn_cvt_pk_f32_fp8(w.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(w.x, true);
        const auto c = __builtin_amdgcn_cvt_pk_f32_fp8(w.y, false), e = __builtin_amdgcn_cvt_pk_f32_fp8(w.y, true);
        v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1]; v[4] = c[0]; v[5] = c[1]; v[6] = e[0]; v[7] = e[1];
    } else {
        load_chunk<CW>(q, dt, v);
    }
}

// ---- summaries --------------------------------------------------------------------------------------------------------------
template <int L>
__global__ __launch_bounds__(THREADS) void summary_update_kernel(const fa_block_summary_params p) {
    constexpr int G = THREADS / L;  // row groups
    __shared__ float red[2][G][L * CW];
    const int b = blockIdx.z, hk = blockIdx.y, B = p.block_size;
    const int nw = clampi(p.seqlens_new[b], 0, p.capacity);
    const int od = p.seqlens_old ? clampi(p.seqlens_old[b], 0, nw) : 0;
    if (od >= nw) return;  // (an empty range; uniform)
    const int j = od / B + (int)blockIdx.x;
    if ((int64_t)j * B >= nw || j >= p.max_blocks) return;
    const int lo = od > j * B ? od : j * B, hi = nw < (j + 1) * B ? nw : (j + 1) * B;
    const bool merge = od > j * B;  // the block began before the range
    const int c = threadIdx.x % L, grp = threadIdx.x / L;
    const bool live = c * CW < p.d;
    const int ces = p.cache_dtype == FA_DTYPE_FP8_E4M3 ? 1 : 2;
    const int64_t slot = p.page_table ? b : p.cache_batch_idx ? p.cache_batch_idx[b] : b;
    const char *cache = static_cast<const char *>(p.k_cache);

    float mn[CW], mx[CW];
#pragma unroll
    for (int i = 0; i < CW; ++i) { mn[i] = INFINITY; mx[i] = -INFINITY; }
    if (live) {
        for (int t = lo + grp; t < hi; t += G) {
            int64_t at;
            if (p.page_table) {
                const int64_t page = p.page_table[b * p.page_table_batch_stride + t / p.page_size];
                at = page * p.cache_batch_stride + (int64_t)(t % p.page_size) * p.cache_row_stride;
            } else {
                at = slot * p.cache_batch_stride + (int64_t)t * p.cache_row_stride;
            }
            float v[CW];
            load8(cache + (at + hk * p.cache_head_stride + c * CW) * ces, p.cache_dtype, v);
#pragma unroll
            for (int i = 0; i < CW; ++i) { mn[i] = fminf(mn[i], v[i]); mx[i] = fmaxf(mx[i], v[i]); }
        }
    }
#pragma unroll
    for (int i = 0; i < CW; ++i) { red[0][grp][c * CW + i] = mn[i]; red[1][grp][c * CW + i] = mx[i]; }
    __syncthreads();
    if (threadIdx.x < L && live) {
        for (int g = 1; g < G; ++g) {
#pragma unroll
            for (int i = 0; i < CW; ++i) {
                mn[i] = fminf(mn[i], red[0][g][c * CW + i]);
                mx[i] = fmaxf(mx[i], red[1][g][c * CW + i]);
            }
        }
        char *s0 = static_cast<char *>(p.k_summary) +
                   (slot * p.sum_slot_stride + (int64_t)j * p.sum_block_stride + hk * p.sum_head_stride + c * CW) * 2;
        char *s1 = s0 + p.sum_side_stride * 2;
        if (merge) {
            float a[CW], z[CW];
            load_chunk<CW>(s0, p.summary_dtype, a);
            load_chunk<CW>(s1, p.summary_dtype, z);
#pragma unroll
            for (int i = 0; i < CW; ++i) { mn[i] = fminf(mn[i], a[i]); mx[i] = fmaxf(mx[i], z[i]); }
        }
        store_chunk<CW>(s0, p.summary_dtype, mn);  // (values of the dtype, or e4m3 values: the rounding changes nothing)
        store_chunk<CW>(s1, p.summary_dtype, mx);
    }
}

// ---- scores -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int blocks_of(const fa_block_select_params &p, int b) {
    const int64_t cap = (int64_t)p.max_blocks * p.block_size;  // (< 2^31: validated)
    const int sk = clampi(p.cache_seqlens[b], 0, (int)cap);
    return (sk + p.block_size - 1) / p.block_size;
}

template <int L>
__global__ __launch_bounds__(THREADS) void block_score_kernel(const fa_block_select_params p) {
    constexpr int G = THREADS / L, CHUNK = G * NB;
    __shared__ uint4 qs[FA_BLOCK_SELECT_MAX_ROWS * L];  // the query rows of (b, hk) as they are: row r, chunk c at r * L + c
    const int b = blockIdx.z, hk = blockIdx.y, j0 = blockIdx.x * CHUNK;
    const int n = blocks_of(p, b), g = p.h / p.h_k, R = p.s_q * g, chunks = p.d / CW;
    const int c = threadIdx.x % L, grp = threadIdx.x / L;
    float *out = p.scores + b * p.scores_batch_stride + hk * p.scores_head_stride;
    if (j0 >= n) {  // nothing filled here: -inf, and nothing is read (uniform)
        for (int j = j0 + threadIdx.x; j < j0 + CHUNK && j < p.max_blocks; j += THREADS) out[j] = -INFINITY;
        return;
    }
    for (int x = threadIdx.x; x < R * L; x += THREADS) {
        const int r = x / L, cc = x % L;
        if (cc < chunks) {
            const int64_t at = b * p.q_batch_stride + (int64_t)(r / g) * p.q_row_stride + (int64_t)(hk * g + r % g) * p.q_head_stride + cc * CW;
            qs[x] = *reinterpret_cast<const uint4 *>(static_cast<const char *>(p.q) + at * 2);
        }
    }
    const bool live = c < chunks;
    const int64_t slot = p.cache_batch_idx ? p.cache_batch_idx[b] : b;
    const char *sum = static_cast<const char *>(p.k_summary) + (slot * p.sum_slot_stride + hk * p.sum_head_stride + c * CW) * 2;
    float mn[NB][CW], mx[NB][CW], acc[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const int j = j0 + k * G + grp;
#pragma unroll
        for (int i = 0; i < CW; ++i) mn[k][i] = mx[k][i] = 0.0f;  // (a dead lane or block adds +0)
        if (live && j < n) {
            const char *at = sum + (int64_t)j * p.sum_block_stride * 2;
            load_chunk<CW>(at, p.dtype, mn[k]);
            load_chunk<CW>(at + p.sum_side_stride * 2, p.dtype, mx[k]);
        }
        acc[k] = p.group_reduce == FA_BLOCK_REDUCE_MAX ? -INFINITY : 0.0f;
    }
    __syncthreads();
    for (int r = 0; r < R; ++r) {
        float qf[CW];
        load_chunk<CW>(&qs[r * L + (live ? c : 0)], p.dtype, qf);
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < CW; ++i) s += fmaxf(qf[i] * mn[k][i], qf[i] * mx[k][i]);
#pragma unroll
            for (int o = L / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, L);
            acc[k] = p.group_reduce == FA_BLOCK_REDUCE_MAX ? fmaxf(acc[k], s) : acc[k] + s;
        }
    }
    if (c == 0) {
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int j = j0 + k * G + grp;
            if (j < p.max_blocks) out[j] = j < n ? acc[k] + 0.0f : -INFINITY;  // (+ 0: -0 is stored as +0)
        }
    }
}

// ---- selection --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SELECT_LARGE) void block_select_kernel(const fa_block_select_params p) {
    __shared__ uint32_t keys[FA_BLOCK_SELECT_MAX_BLOCKS];
    __shared__ uint32_t hist[BINS];
    __shared__ uint64_t part[MAX_WAVES];
    __shared__ uint32_t cut_digit, cut_above;
    const int hk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, T = blockDim.x;
    const int n = blocks_of(p, b);
    const int K = p.num_blocks < n ? p.num_blocks : n;
    const int sink = p.sink_blocks, tail = n - p.local_blocks;  // forced: j < sink or j >= tail
    const bool all_forced = (int64_t)p.sink_blocks + p.local_blocks >= n;
    const int rest = all_forced ? 0 : K - p.sink_blocks - p.local_blocks;  // places of the unforced blocks (K >= sink + local)
    const float *u = p.scores + b * p.scores_batch_stride + hk * p.scores_head_stride;
    const auto forced = [&](int j) { return j < sink || j >= tail; };

    for (int j = tid; j < n; j += T) keys[j] = full_key(u[j] + 0.0f);
    // the cut: the key `cut` of which `ties_in` >= 1 entries are chosen beside every unforced entry above it
    uint32_t cut = 0xffffffffu;
    int ties_in = 0;
    if (rest > 0) {  // (uniform)
        uint32_t prefix = 0, want = (uint32_t)rest;
        for (int shift = 32 - RADIX_BITS; shift >= 0; shift -= RADIX_BITS) {
            for (int x = tid; x < BINS; x += T) hist[x] = 0;
            __syncthreads();  // (orders the keys as well)
            for (int j = tid; j < n; j += T) {
                const uint32_t key = keys[j];
                if (forced(j) || (shift + RADIX_BITS < 32 && key >> (shift + RADIX_BITS) != prefix)) continue;
                atomicAdd(&hist[(key >> shift) & (BINS - 1)], 1u);  // (counts: any order gives the same histogram)
            }
            __syncthreads();
            const uint64_t mine = tid < BINS ? hist[BINS - 1 - tid] : 0u;  // thread t: digit 255 - t; `above`: the higher digits
            uint64_t total;
            const uint64_t above = wg_exclusive_scan(mine, part, total);
            if (tid < BINS && above < want && want <= above + mine) { cut_digit = BINS - 1 - tid; cut_above = (uint32_t)above; }
            __syncthreads();  // (one thread wrote: at least `rest` unforced entries carry the prefix)
            prefix = prefix << RADIX_BITS | cut_digit;
            want -= cut_above;
        }
        cut = prefix;
        ties_in = (int)want;
    } else {
        __syncthreads();
    }

    // ascending compaction: thread t owns the indices [t * per, (t + 1) * per)
    const int per = (n + T - 1) / T, a0 = tid * per < n ? tid * per : n, a1 = a0 + per < n ? a0 + per : n;
    uint64_t ties = 0, total;
    for (int j = a0; j < a1; ++j) ties += !forced(j) && keys[j] == cut;
    const uint64_t ties_before = wg_exclusive_scan(ties, part, total);
    const auto walk = [&](auto &&chosen) {
        int rank = (int)ties_before;
        for (int j = a0; j < a1; ++j) {
            const uint32_t key = keys[j];
            bool in = forced(j);
            if (!in && rest > 0) {
                if (key > cut) in = true;
                else if (key == cut) in = rank++ < ties_in;
            }
            if (in) chosen(j);
        }
    };
    uint64_t count = 0;
    walk([&](int) { ++count; });
    int at = (int)wg_exclusive_scan(count, part, total);
    int32_t *idx = p.block_idx + b * p.idx_batch_stride + hk * p.idx_head_stride;
    walk([&](int j) {
        if (at < p.list_width) idx[at] = j;  // (at < K <= list_width; the guard costs nothing)
        ++at;
    });
    for (int x = K + tid; x < p.list_width; x += T) idx[x] = -1;
    if (tid == 0) p.block_cnt[b * p.cnt_batch_stride + hk * p.cnt_head_stride] = K;
}

// ---- host -------------------------------------------------------------------------------------------------------------------
bool sixteen_bit(int dt) { return dt == FA_DTYPE_FP16 || dt == FA_DTYPE_BF16; }
bool strides_8(std::initializer_list<int64_t> strides) {
    for (const int64_t s : strides)
        if (s % 8 != 0) return false;
    return true;
}

struct SummaryForm {
    int L, grid_x;
};
SummaryForm summary_form(const fa_block_summary_params *p) {
    const int64_t touched = ((int64_t)p->max_seqlen_new + p->block_size - 1) / p->block_size + 1;
    return {lanes_of(p->d), (int)(touched < p->max_blocks ? touched : p->max_blocks)};
}

struct SelectForm {
    int L, chunks, threads;
};
SelectForm select_form(const fa_block_select_params *p) {
    const int L = lanes_of(p->d), chunk = score_chunk(L);
    return {L, (p->max_blocks + chunk - 1) / chunk, p->max_blocks <= SELECT_SMALL_BLOCKS ? SELECT_SMALL : SELECT_LARGE};
}

}  // namespace

extern "C" {

uint32_t fa_block_summary_params_size(void) { return (uint32_t)sizeof(fa_block_summary_params); }
uint32_t fa_block_select_params_size(void) { return (uint32_t)sizeof(fa_block_select_params); }

int fa_block_summary_update_validate(const fa_block_summary_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_block_summary_params)) return FA_ERR_BAD_ABI;
    if (!sixteen_bit(p->summary_dtype)) return FA_ERR_BAD_DTYPE;
    if (p->cache_dtype != p->summary_dtype && p->cache_dtype != FA_DTYPE_FP8_E4M3) return FA_ERR_BAD_DTYPE;
    if (p->d < 16 || p->d > 128 || p->d % 16 != 0) return FA_ERR_BAD_HEAD_DIM;
    if (p->cache_leftpad || p->cu_seqlens_k_new) return FA_ERR_UNSUPPORTED;
    if (p->block_size <= 0 || p->block_size % 64 != 0) return FA_ERR_BAD_SHAPE;
    if (p->b < 0 || p->b > 65535 || p->h_k < 1 || p->h_k > 65535 || p->capacity < 0 || p->max_blocks < 0 || p->max_seqlen_new < 0)
        return FA_ERR_BAD_SHAPE;
    if ((int64_t)p->max_blocks * p->block_size > 0x7fffffff) return FA_ERR_BAD_SHAPE;
    if ((int64_t)p->max_blocks * p->block_size < p->capacity) return FA_ERR_BAD_SHAPE;  // the summary covers the capacity
    if (p->page_table && (p->page_size <= 0 || p->capacity % p->page_size != 0 || p->cache_batch_idx)) return FA_ERR_BAD_SHAPE;
    if (!p->k_summary || !p->k_cache || !p->seqlens_new) return FA_ERR_NULL_POINTER;
    const bool fp8 = p->cache_dtype == FA_DTYPE_FP8_E4M3;
    if (!aligned_to(p->k_summary, 16) || !aligned_to(p->k_cache, fp8 ? 8 : 16) || !aligned_to(p->seqlens_old, 4) ||
        !aligned_to(p->seqlens_new, 4) || !aligned_to(p->cache_batch_idx, 4) || !aligned_to(p->page_table, 4))
        return FA_ERR_BAD_STRIDE;
    if (!strides_8({p->sum_slot_stride, p->sum_block_stride, p->sum_side_stride, p->sum_head_stride, p->cache_batch_stride,
                    p->cache_row_stride, p->cache_head_stride}))
        return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int64_t fa_block_summary_update_workspace_size(const fa_block_summary_params *p) {
    const int st = fa_block_summary_update_validate(p);
    return st != FA_OK ? st : 0;
}

const char *fa_block_summary_update_plan_name(const fa_block_summary_params *p) {
    if (fa_block_summary_update_validate(p) != FA_OK) return nullptr;
    thread_local char name[128];
    const SummaryForm f = summary_form(p);
    std::snprintf(name, sizeof name, "summary_update_kernel<%d> cache=%s %s grid=(%d,%d,%d)", f.L,
                  p->cache_dtype == FA_DTYPE_FP8_E4M3 ? "e4m3" : "16", p->page_table ? "paged" : "dense", f.grid_x, p->h_k, p->b);
    return name;
}

int fa_block_summary_update(const fa_block_summary_params *p, void *stream_) {
    const int st = fa_block_summary_update_validate(p);
    if (st != FA_OK) return st;
    const SummaryForm f = summary_form(p);
    if (p->b == 0 || f.grid_x == 0 || p->capacity == 0) return FA_OK;  // (no zero grid)
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(f.grid_x, p->h_k, p->b);
    if (f.L == 16) hipLaunchKernelGGL(summary_update_kernel<16>, grid, dim3(THREADS), 0, stream, *p);
    else hipLaunchKernelGGL(summary_update_kernel<8>, grid, dim3(THREADS), 0, stream, *p);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

int fa_block_select_validate(const fa_block_select_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_block_select_params)) return FA_ERR_BAD_ABI;
    if (!sixteen_bit(p->dtype)) return FA_ERR_BAD_DTYPE;
    if (p->d < 16 || p->d > 128 || p->d % 16 != 0) return FA_ERR_BAD_HEAD_DIM;
    if (p->h_k < 1 || p->h_k > 65535 || p->h < 1 || p->h % p->h_k != 0) return FA_ERR_BAD_HEADS;
    if (p->cu_seqlens_q || p->cache_leftpad) return FA_ERR_UNSUPPORTED;
    if (p->group_reduce != FA_BLOCK_REDUCE_MAX && p->group_reduce != FA_BLOCK_REDUCE_SUM) return FA_ERR_UNSUPPORTED;
    if (p->block_size <= 0 || p->block_size % 64 != 0) return FA_ERR_BAD_SHAPE;
    if (p->b < 0 || p->b > 65535 || p->s_q < 1 || (int64_t)p->s_q * (p->h / p->h_k) > FA_BLOCK_SELECT_MAX_ROWS) return FA_ERR_BAD_SHAPE;
    if (p->max_blocks < 1 || p->max_blocks > FA_BLOCK_SELECT_MAX_BLOCKS) return FA_ERR_BAD_SHAPE;
    if ((int64_t)p->max_blocks * p->block_size > 0x7fffffff) return FA_ERR_BAD_SHAPE;
    if (p->sink_blocks < 0 || p->local_blocks < 0 || p->num_blocks < (int64_t)p->sink_blocks + p->local_blocks) return FA_ERR_BAD_SHAPE;
    if (p->list_width < p->num_blocks) return FA_ERR_BAD_SHAPE;
    if (!p->q || !p->k_summary || !p->cache_seqlens || !p->scores || !p->block_cnt || !p->block_idx) return FA_ERR_NULL_POINTER;
    if (!aligned_to(p->q, 16) || !aligned_to(p->k_summary, 16) || !aligned_to(p->cache_seqlens, 4) || !aligned_to(p->cache_batch_idx, 4) ||
        !aligned_to(p->scores, 4) || !aligned_to(p->block_cnt, 4) || !aligned_to(p->block_idx, 4))
        return FA_ERR_BAD_STRIDE;
    if (!strides_8({p->q_batch_stride, p->q_row_stride, p->q_head_stride, p->sum_slot_stride, p->sum_block_stride, p->sum_side_stride,
                    p->sum_head_stride}))
        return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int64_t fa_block_select_workspace_size(const fa_block_select_params *p) {
    const int st = fa_block_select_validate(p);
    return st != FA_OK ? st : (int64_t)p->b * p->h_k * p->max_blocks * (int64_t)sizeof(float);
}

const char *fa_block_select_plan_name(const fa_block_select_params *p) {
    if (fa_block_select_validate(p) != FA_OK) return nullptr;
    thread_local char name[160];
    const SelectForm f = select_form(p);
    std::snprintf(name, sizeof name, "block_score_kernel<%d> %s split=%d grid=(%d,%d,%d) + block_select_kernel threads=%d", f.L,
                  p->group_reduce == FA_BLOCK_REDUCE_MAX ? "max" : "sum", f.chunks, f.chunks, p->h_k, p->b, f.threads);
    return name;
}

int fa_block_select(const fa_block_select_params *p, void *stream_) {
    const int st = fa_block_select_validate(p);
    if (st != FA_OK) return st;
    if (p->b == 0) return FA_OK;  // (no zero grid)
    const SelectForm f = select_form(p);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(f.chunks, p->h_k, p->b);
    if (f.L == 16) hipLaunchKernelGGL(block_score_kernel<16>, grid, dim3(THREADS), 0, stream, *p);
    else hipLaunchKernelGGL(block_score_kernel<8>, grid, dim3(THREADS), 0, stream, *p);
    hipLaunchKernelGGL(block_select_kernel, dim3(p->h_k, p->b), dim3(f.threads), 0, stream, *p);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

}  // extern "C"
