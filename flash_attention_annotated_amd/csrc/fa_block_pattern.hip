// fa_block_pattern.hip — the producer of block-sparse prefill / training patterns (include/fa_block_pattern.h, which states the
// rule): mean-pooled block scores of q against k, a top-k per query block with forced sink and local blocks, written as the
// lists the block-sparse forward and backward of the cute surface read.  A translation unit of its own.  The chunk loads, the
// workgroup scan and the host predicates are fa_rowwise.h's; the order-preserving key of a score is the one of
// fa_sample_device.h.  The cut is found as fa_block_select.hip finds its own: a descent over 8-bit digits of the keys in LDS.
//
// pool_kernel<VEC>: one workgroup per (b, head, block) of q, then of k.  L lanes hold the 8-channel chunks of a row (L = 16:
//   d > 64, else 8), 256 / L row groups walk the rows, LDS folds the groups in ascending order, d threads store fp32.
// pattern_kernel: one workgroup per (m, h, b).  A group of L lanes forms one score per step from qs[m] in registers and a row of
//   km (two 16-byte loads per lane, a butterfly over the L lanes); the keys of the visible scores lie in LDS; the cut by four
//   8-bit passes, the ties by index, the two lists by one scan of a packed pair of counts.  Integer logic only from the keys on:
//   a NaN score is a key like any other.
// transpose_kernel: one workgroup per (n, h, b): bit n of the nm membership rows, compacted ascending by a scan.
#include "../../include/fa_block_pattern.h"
#include "fa_sample_device.h"

#include <cstdio>

namespace {

using namespace fa_row;
using fa_sample_dev::full_key;

constexpr int B = FA_BLOCK_PATTERN_BLOCK;
constexpr int THREADS = 256;  // of the pooling and the transpose
constexpr int CW = 8;         // channels per lane
constexpr int SELECT_SMALL = 256, SELECT_LARGE = 1024, SELECT_SMALL_BLOCKS = 1024;  // the selection's workgroup by nk
constexpr int RADIX_BITS = 8, BINS = 1 << RADIX_BITS;

__host__ __device__ constexpr int lanes_of(int d) { return d > 64 ? 16 : 8; }
__host__ __device__ constexpr int blocks_of(int s) { return (s + B - 1) / B; }

// ---- pooling ----------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(THREADS) void pool_kernel(const fa_block_pattern_params p, float *qs, float *km) {
    __shared__ float red[THREADS * CW];  // [row group][L * CW]
    const int nm = blocks_of(p.sq), nk = blocks_of(p.sk);
    const int64_t q_items = (int64_t)p.b * p.h * nm;
    int64_t w = blockIdx.x;
    const bool keys = w >= q_items;  // (uniform)
    if (keys) w -= q_items;
    const int heads = keys ? p.h_k : p.h, blocks = keys ? nk : nm, len = keys ? p.sk : p.sq;
    const int blk = (int)(w % blocks), head = (int)(w / blocks % heads), b = (int)(w / blocks / heads);
    const int64_t bs = keys ? p.k_batch_stride : p.q_batch_stride, rs = keys ? p.k_row_stride : p.q_row_stride,
                  hs = keys ? p.k_head_stride : p.q_head_stride;
    const int r0 = blk * B, rows = len - r0 < B ? len - r0 : B;  // rows >= 1
    const int L = lanes_of(p.d), G = THREADS / L, c = threadIdx.x % L, grp = threadIdx.x / L;
    const bool live = c * CW < p.d;
    const char *base = static_cast<const char *>(keys ? p.k : p.q) + (b * bs + head * hs + c * CW) * 2;

    float acc[CW];
#pragma unroll
    for (int i = 0; i < CW; ++i) acc[i] = 0.0f;
    if (live) {
        for (int t = grp; t < rows; t += G) {
            const char *at = base + (int64_t)(r0 + t) * rs * 2;
            float v[CW];
            if constexpr (VEC) {
                load_chunk<CW>(at, p.dtype, v);
            } else {
#pragma unroll
                for (int i = 0; i < CW; ++i) v[i] = load_one(at, p.dtype, i);
            }
#pragma unroll
            for (int i = 0; i < CW; ++i) acc[i] += v[i];
        }
    }
#pragma unroll
    for (int i = 0; i < CW; ++i) red[grp * (L * CW) + c * CW + i] = acc[i];
    __syncthreads();
    if ((int)threadIdx.x < p.d) {
        float s = red[threadIdx.x];
        for (int g = 1; g < G; ++g) s += red[g * (L * CW) + threadIdx.x];
        if (keys) s *= 1.0f / (float)rows;
        (keys ? km : qs)[w * p.d + threadIdx.x] = s;
    }
}

// ---- scores and selection ---------------------------------------------------------------------------------------------------
// the visible key blocks [lo, hi] of query block m (empty: lo > hi), and whether a visible block is full
struct Band {
    int lo, hi;
    int64_t full_lo, full_hi;  // block n is full iff full_lo <= n B and (n + 1) B - 1 <= full_hi
};
__device__ __forceinline__ Band band_of(const fa_block_pattern_params &p, int m) {
    const int64_t left = p.window_size_left, right = p.is_causal ? 0 : p.window_size_right;
    const int64_t i_lo = (int64_t)m * B, i_hi = ((int64_t)(m + 1) * B < p.sq ? (int64_t)(m + 1) * B : p.sq) - 1, off = (int64_t)p.sk - p.sq;
    int64_t j_min = left < 0 ? 0 : i_lo + off - left, j_max = right < 0 ? p.sk - 1 : i_hi + off + right;
    j_min = j_min < 0 ? 0 : j_min;
    j_max = j_max > p.sk - 1 ? p.sk - 1 : j_max;
    Band v;
    v.lo = j_min <= j_max ? (int)(j_min / B) : 1;
    v.hi = j_min <= j_max ? (int)(j_max / B) : 0;
    // every pair visible: the keys lie between the lower bound of the last row and the upper bound of the first; all B keys exist
    v.full_lo = left < 0 ? 0 : i_hi + off - left;
    v.full_hi = right < 0 ? (int64_t)p.sk - 1 : i_lo + off + right;
    v.full_hi = v.full_hi > (int64_t)p.sk - 1 ? (int64_t)p.sk - 1 : v.full_hi;
    return v;
}

__global__ __launch_bounds__(SELECT_LARGE) void pattern_kernel(const fa_block_pattern_params p, const float *qs, const float *km,
                                                               uint32_t *bitmap) {
    __shared__ uint32_t keys[FA_BLOCK_PATTERN_MAX_BLOCKS];
    __shared__ uint32_t hist[BINS];
    __shared__ uint64_t part[MAX_WAVES];
    __shared__ uint32_t cut_digit, cut_above;
    const int m = blockIdx.x, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, T = blockDim.x;
    const int nm = blocks_of(p.sq), nk = blocks_of(p.sk), hk = h / (p.h / p.h_k);
    const int64_t row = ((int64_t)b * p.h + h) * nm + m;
    const Band v = band_of(p, m);
    const int first = v.lo, n = v.lo <= v.hi ? v.hi - v.lo + 1 : 0;  // |V|; entry j of V is block first + j
    const int64_t full_lo = v.full_lo, full_hi = v.full_hi;
    const auto is_full = [=](int blk) { return full_lo <= (int64_t)blk * B && (int64_t)(blk + 1) * B - 1 <= full_hi; };
    float *u = p.scores ? p.scores + row * nk : nullptr;

    {  // the scores of the visible blocks: keys[j], and u
        const int L = lanes_of(p.d), G = T / L, c = tid % L, grp = tid / L;
        const bool live = c * CW < p.d;
        float qv[CW];
#pragma unroll
        for (int i = 0; i < CW; ++i) qv[i] = 0.0f;
        if (live) load_chunk<CW>(qs + row * p.d + c * CW, FA_DTYPE_FP32, qv);
        const float *kb = km + (((int64_t)b * p.h_k + hk) * nk + first) * p.d + c * CW;
        for (int j0 = 0; j0 < n; j0 += G) {  // (uniform bounds: every lane takes part in the butterfly)
            const int j = j0 + grp;
            float s = 0.0f;
            if (live && j < n) {
                float kv[CW];
                load_chunk<CW>(kb + (int64_t)j * p.d, FA_DTYPE_FP32, kv);
#pragma unroll
                for (int i = 0; i < CW; ++i) s = fmaf(qv[i], kv[i], s);
            }
            for (int o = L / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, L);
            if (c == 0 && j < n) {
                s += 0.0f;  // (-0 is stored as +0)
                keys[j] = full_key(s);
                if (u) u[first + j] = s;
            }
        }
        if (u)
            for (int x = tid; x < nk; x += T)
                if (x < first || x >= first + n) u[x] = -INFINITY;
    }

    const int K = p.num_blocks < n ? p.num_blocks : n;
    const int sink = p.sink_blocks, tail = n - p.local_blocks;  // forced: j < sink or j >= tail
    const bool all_forced = (int64_t)p.sink_blocks + p.local_blocks >= n;
    const int rest = all_forced ? 0 : K - p.sink_blocks - p.local_blocks;  // places of the unforced blocks (K >= sink + local)
    const auto forced = [&](int j) { return j < sink || j >= tail; };

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

    // ascending compaction: thread t owns the entries [t * per, (t + 1) * per) of V
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
            chosen(j, in);
        }
    };
    uint64_t count = 0;  // full blocks in the high word, the others in the low one
    walk([&](int j, bool in) {
        if (in) count += is_full(first + j) ? (uint64_t)1 << 32 : 1u;
    });
    const uint64_t before = wg_exclusive_scan(count, part, total);
    int at_full = (int)(before >> 32), at_mask = (int)(uint32_t)before;
    const int n_full = (int)(total >> 32), n_mask = (int)(uint32_t)total;  // n_full + n_mask = K <= nk
    int32_t *full_idx = p.full_block_idx + row * nk, *mask_idx = p.mask_block_idx + row * nk;
    walk([&](int j, bool in) {
        if (in) {
            const int blk = first + j;
            const bool f = is_full(blk);
            const int at = f ? at_full : at_mask;
            if (at < nk) (f ? full_idx : mask_idx)[at] = blk;  // (at < K <= nk; the guard costs nothing)
            at_full += f;
            at_mask += !f;
        }
        if (bitmap) keys[j] = in;  // (this thread's own entries: read above, not read again before the barrier)
    });
    for (int x = n_full + tid; x < nk; x += T) full_idx[x] = 0;
    for (int x = n_mask + tid; x < nk; x += T) mask_idx[x] = 0;
    if (tid == 0) {
        p.full_block_cnt[row] = n_full;
        p.mask_block_cnt[row] = n_mask;
    }
    if (bitmap) {  // (uniform) the membership of row m: bit n % 32 of word n / 32
        __syncthreads();
        const int words = (nk + 31) / 32;
        for (int wd = tid; wd < words; wd += T) {
            uint32_t bits = 0;
            for (int i = 0; i < 32; ++i) {
                const int j = wd * 32 + i - first;
                if (j >= 0 && j < n && keys[j]) bits |= 1u << i;
            }
            bitmap[row * words + wd] = bits;
        }
    }
}

// ---- key-major lists --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void transpose_kernel(const fa_block_pattern_params p, const uint32_t *bitmap) {
    __shared__ uint64_t part[MAX_WAVES];
    const int n = blockIdx.x, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int nm = blocks_of(p.sq), nk = blocks_of(p.sk), words = (nk + 31) / 32;
    const int64_t head = (int64_t)b * p.h + h;
    const uint32_t *col = bitmap + head * nm * words + n / 32;
    const uint32_t bit = 1u << (n % 32);
    const int per = (nm + THREADS - 1) / THREADS, a0 = tid * per < nm ? tid * per : nm, a1 = a0 + per < nm ? a0 + per : nm;
    uint64_t count = 0, total;
    for (int m = a0; m < a1; ++m) count += (col[(int64_t)m * words] & bit) != 0;
    int at = (int)wg_exclusive_scan(count, part, total);
    int32_t *idx = p.q_block_idx + (head * nk + n) * nm;
    for (int m = a0; m < a1; ++m)
        if (col[(int64_t)m * words] & bit) {
            if (at < nm) idx[at] = m;
            ++at;
        }
    for (int x = (int)total + tid; x < nm; x += THREADS) idx[x] = 0;
    if (tid == 0) p.q_block_cnt[head * nk + n] = (int)total;
}

// ---- host -------------------------------------------------------------------------------------------------------------------
struct Form {
    bool vec, transpose;
    int L, threads, nm, nk;
    int64_t pool_grid, qs_bytes, km_bytes, bitmap_bytes;
};
int64_t round16(int64_t x) { return (x + 15) / 16 * 16; }
Form form_of(const fa_block_pattern_params *p) {
    Form f;
    f.nm = blocks_of(p->sq);
    f.nk = blocks_of(p->sk);
    f.vec = aligned_to(p->q, 16) && aligned_to(p->k, 16);
    for (const int64_t s : {p->q_batch_stride, p->q_row_stride, p->q_head_stride, p->k_batch_stride, p->k_row_stride, p->k_head_stride})
        f.vec = f.vec && s % 8 == 0;
    f.transpose = p->q_block_cnt != nullptr;
    f.L = lanes_of(p->d);
    f.threads = f.nk <= SELECT_SMALL_BLOCKS ? SELECT_SMALL : SELECT_LARGE;
    f.pool_grid = (int64_t)p->b * p->h * f.nm + (int64_t)p->b * p->h_k * f.nk;
    f.qs_bytes = round16((int64_t)p->b * p->h * f.nm * p->d * 4);
    f.km_bytes = round16((int64_t)p->b * p->h_k * f.nk * p->d * 4);
    f.bitmap_bytes = f.transpose ? round16((int64_t)p->b * p->h * f.nm * ((f.nk + 31) / 32) * 4) : 0;
    return f;
}

// every check but the workspace's
int check(const fa_block_pattern_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_block_pattern_params)) return FA_ERR_BAD_ABI;
    if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16) return FA_ERR_BAD_DTYPE;
    if (p->d < 16 || p->d > 128 || p->d % 16 != 0) return FA_ERR_BAD_HEAD_DIM;
    if (p->h_k < 1 || p->h < 1 || p->h > 65535 || p->h % p->h_k != 0) return FA_ERR_BAD_HEADS;
    if (p->b < 0 || p->b > 65535 || p->sq < 1 || p->sk < 1) return FA_ERR_BAD_SHAPE;
    if (p->sk > FA_BLOCK_PATTERN_MAX_BLOCKS * B || p->sq > 0x7fffffff - B) return FA_ERR_BAD_SHAPE;
    if (p->sink_blocks < 0 || p->local_blocks < 0 || p->num_blocks < (int64_t)p->sink_blocks + p->local_blocks) return FA_ERR_BAD_SHAPE;
    if ((int64_t)p->b * p->h * blocks_of(p->sq) + (int64_t)p->b * p->h_k * blocks_of(p->sk) > 0x7fffffff) return FA_ERR_BAD_SHAPE;
    if (!p->q || !p->k || !p->full_block_cnt || !p->full_block_idx || !p->mask_block_cnt || !p->mask_block_idx) return FA_ERR_NULL_POINTER;
    if (!p->q_block_cnt != !p->q_block_idx) return FA_ERR_NULL_POINTER;
    if (!aligned_to(p->q, 2) || !aligned_to(p->k, 2) || !aligned_to(p->full_block_cnt, 4) || !aligned_to(p->full_block_idx, 4) ||
        !aligned_to(p->mask_block_cnt, 4) || !aligned_to(p->mask_block_idx, 4) || !aligned_to(p->q_block_cnt, 4) ||
        !aligned_to(p->q_block_idx, 4) || !aligned_to(p->scores, 4))
        return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

}  // namespace

extern "C" {

uint32_t fa_block_pattern_params_size(void) { return (uint32_t)sizeof(fa_block_pattern_params); }

int64_t fa_block_pattern_workspace_size(const fa_block_pattern_params *p) {
    const int st = check(p);
    if (st != FA_OK) return st;
    const Form f = form_of(p);
    return f.qs_bytes + f.km_bytes + f.bitmap_bytes;
}

int fa_block_pattern_validate(const fa_block_pattern_params *p) {
    const int st = check(p);
    if (st != FA_OK) return st;
    if (p->b == 0) return FA_OK;  // (nothing is launched, nothing is needed)
    if (!p->workspace || p->workspace_bytes < (uint64_t)fa_block_pattern_workspace_size(p)) return FA_ERR_WORKSPACE;
    if (!aligned_to(p->workspace, 16)) return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

const char *fa_block_pattern_plan_name(const fa_block_pattern_params *p) {
    if (check(p) != FA_OK) return nullptr;
    thread_local char name[256];
    const Form f = form_of(p);
    int at = std::snprintf(name, sizeof name, "pool_kernel<%s> L=%d grid=(%lld) + pattern_kernel m_per_wg=1 threads=%d grid=(%d,%d,%d)",
                           f.vec ? "16B" : "elem", f.L, (long long)f.pool_grid, f.threads, f.nm, p->h, p->b);
    if (f.transpose) std::snprintf(name + at, sizeof name - at, " + transpose_kernel grid=(%d,%d,%d)", f.nk, p->h, p->b);
    else std::snprintf(name + at, sizeof name - at, " + no transpose");
    return name;
}

int fa_block_pattern(const fa_block_pattern_params *p, void *stream_) {
    const int st = fa_block_pattern_validate(p);
    if (st != FA_OK) return st;
    if (p->b == 0) return FA_OK;  // (no zero grid)
    const Form f = form_of(p);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    char *ws = static_cast<char *>(p->workspace);
    float *qs = reinterpret_cast<float *>(ws), *km = reinterpret_cast<float *>(ws + f.qs_bytes);
    uint32_t *bitmap = f.transpose ? reinterpret_cast<uint32_t *>(ws + f.qs_bytes + f.km_bytes) : nullptr;
    if (f.vec) hipLaunchKernelGGL(pool_kernel<true>, dim3((uint32_t)f.pool_grid), dim3(THREADS), 0, stream, *p, qs, km);
    else hipLaunchKernelGGL(pool_kernel<false>, dim3((uint32_t)f.pool_grid), dim3(THREADS), 0, stream, *p, qs, km);
    hipLaunchKernelGGL(pattern_kernel, dim3(f.nm, p->h, p->b), dim3(f.threads), 0, stream, *p, qs, km, bitmap);
    if (f.transpose) hipLaunchKernelGGL(transpose_kernel, dim3(f.nk, p->h, p->b), dim3(THREADS), 0, stream, *p, bitmap);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

}  // extern "C"
