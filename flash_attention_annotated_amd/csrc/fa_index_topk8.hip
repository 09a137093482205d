// fa_index_topk8.hip — the lightning indexer over an fp8 (e4m3) index-key cache with one fp32 scale per token, and the
// quantising append that fills that cache (include/fa_index_topk8.h).  A translation unit of its own: fa_index_topk.hip and
// fa_index_prefill.hip stay what their tests pin.  The selection is fa_index_select.h's text, the e4m3 -> 16-bit conversion
// fa_fwd_kernel_kv8.h's kv8_expand, the 16-bit -> e4m3 conversion fa_kvcache_append_kv8.h's quantise8.
//
// index_logits8_kernel<DT, D, MB>: index_logits_kernel's work shape (one workgroup of 4 waves per (chunk of keys, batch entry),
//   the query fragments of a token group in LDS in MFMA operand order, S (heads x keys) = Q . K^T on v_mfma_f32_32x32x16 with the
//   head sum in-lane but for one swap with lane ^ 32) over a BYTE tile: lane (fr, fh) loads the 16 bytes 32 j + 16 fh of the
//   rows fr and 32 + fr, j < D / 32 -- 32 contiguous bytes per row and load instruction, half the load instructions of the
//   16-bit tile -- and feeds the low 8 bytes to k-step 2 j and the high 8 to k-step 2 j + 1.  The query staging writes its
//   fragments in the same permuted channel order (q_channel), so A and B agree.  The bytes are expanded to DT once per tile,
//   before the token loop, and the expanded tile is what the tokens of the group reuse; the bytes of the wave's NEXT tile are
//   loaded before the products of this one start (32 VGPRs at D = 128: what the byte tile makes affordable).  The lane that
//   resolved a key row for the B operand holds its accumulator column: it loads the row's scale with the page it already has
//   and multiplies the head sum once before the store.
// index_select_kernel: one workgroup per (token, batch entry) runs index_select_row over the token's row of logits.
// index_append8_kernel<T, D>: D / 8 lanes per new row (16 bytes of 16-bit input each), 64 / (D / 8) rows per wave and pass; the
//   amax in-lane over 8 values, then across the row's lanes by shuffles; the exponent of the scale from the bits of amax; one
//   8-byte store per lane, the scale by the row's first lane.  No LDS, no atomics.
#include "../../include/fa_index_topk8.h"
#include "fa_fwd_kernel_kv8.h"
#include "fa_index_select.h"
#include "fa_kvcache_append_kv8.h"

#include <algorithm>
#include <cstdio>

namespace {

using namespace fa_row;
using namespace fa_index_sel;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int THREADS = 256, WAVES = THREADS / WAVE;  // of the logits and of the append
constexpr int TILE = 64;                              // key rows of a wave's tile
constexpr int CHUNK_MIN = WAVES * TILE, CHUNK_MAX = 1024, GRID_AIM = 1024;
constexpr int Q_LDS_BYTES = 48 * 1024;  // of the query fragments of a token group
constexpr int APPEND_GRID_MAX = 2048;

template <int DT> struct Elem16;
template <> struct Elem16<FA_DTYPE_BF16> { typedef __bf16 T; };
template <> struct Elem16<FA_DTYPE_FP16> { typedef _Float16 T; };

__host__ __device__ constexpr int tokens_per_group(int D, int MB) {
    return Q_LDS_BYTES / (MB * 32 * D * 2) < FA_INDEX_MAX_ROWS ? Q_LDS_BYTES / (MB * 32 * D * 2) : FA_INDEX_MAX_ROWS;
}

// keys per workgroup: the smallest of 256, 512, 1024 that keeps the grid at or below GRID_AIM workgroups (1024 where none does)
__host__ __device__ inline int chunk_of(int b, int capacity) {
    int c = CHUNK_MIN;
    while (c < CHUNK_MAX && (int64_t)b * ((capacity + c - 1) / c) > GRID_AIM) c *= 2;
    return c;
}

// the first of the 8 channels half fh of a lane contracts in k-step ks: what bytes [8 (ks & 1), +8) of its 16-byte load
// 32 (ks >> 1) + 16 fh hold
__device__ __forceinline__ int q_channel(int ks, int fh) { return (ks >> 1) * 32 + fh * 16 + (ks & 1) * 8; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__device__ __forceinline__ int fill_of(const fa_index_topk8_params &p, int b) { return clampi(p.cache_seqlens[b], 0, p.capacity); }
// n(b, i): the candidates of token i
__device__ __forceinline__ int visible_of(const fa_index_topk8_params &p, int sk, int i) {
    return p.is_causal ? clampi(sk - (p.s_q - 1 - i), 0, sk) : sk;
}

template <int DT>
__device__ __forceinline__ f32x16 mfma(const uint4 a, const fa::u32x4 b, const f32x16 c) {
    if constexpr (DT == FA_DTYPE_BF16)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// ---- logits -----------------------------------------------------------------------------------------------------------------
// The bytes of a wave's tile as its lanes hold them, and the scale of the key the lane stores (row t0 + lane).
template <int D>
struct ByteTile {
    uint4 kb[2][D / 32];
    float scale;
};

// Tile t0 (t0 < sk).  A row at or behind sk is never read: it takes the tile's first row's address, and its logit is -inf
// whatever is loaded here.  One page resolve per row; the scale's address comes from the same page.
template <int D>
__device__ __forceinline__ void load_tile(const fa_index_topk8_params &p, const int32_t *table, int64_t slot, int t0, int sk, int fr, int fh,
                                          ByteTile<D> &t) {
    const char *cache = static_cast<const char *>(p.k_index_cache);
    int64_t scale_at = 0;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int s = t0 + nb * 32 + fr;
        const int row = s < sk ? s : t0;
        int64_t entry = slot, in = row;
        if (table) {
            const uint32_t pg = (uint32_t)row / (uint32_t)p.page_size;
            entry = table[pg];
            in = (uint32_t)row - pg * (uint32_t)p.page_size;
        }
        const char *src = cache + entry * p.cache_batch_stride + in * p.cache_row_stride + fh * 16;
#pragma unroll
        for (int j = 0; j < D / 32; ++j) t.kb[nb][j] = *reinterpret_cast<const uint4 *>(src + j * 32);
        if (nb == fh) scale_at = entry * p.scale_batch_stride + in;
    }
    t.scale = p.k_index_scale[scale_at];
}

template <int DT, int D, int MB>
__global__ __launch_bounds__(THREADS) void index_logits8_kernel(const fa_index_topk8_params p) {
    typedef typename Elem16<DT>::T T;
    constexpr int KS = D / 16, TG = tokens_per_group(D, MB), HP = MB * 32;
    __shared__ uint4 qs[TG * MB * KS * WAVE];  // fragment (token, m block, k step) of lane l at ((token * MB + mb) * KS + ks) * 64 + l
    __shared__ __attribute__((aligned(16))) float ws[TG][HP];
    const int b = blockIdx.y, chunk = chunk_of(p.b, p.capacity), c0 = blockIdx.x * chunk;
    const int c1 = c0 + chunk < p.capacity ? c0 + chunk : p.capacity;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 31, fh = lane >> 5;
    const int sk = fill_of(p, b);
    float *out = p.logits + b * p.logits_batch_stride;
    if (c0 >= sk) {  // nothing filled here: -inf, and nothing is read (uniform)
        for (int i = 0; i < p.s_q; ++i)
            for (int s = c0 + tid; s < c1; s += THREADS) out[i * p.logits_row_stride + s] = -INFINITY;
        return;
    }
    const char *q = static_cast<const char *>(p.q_index) + b * p.q_batch_stride * 2;
    const float *w = p.weights + b * p.w_batch_stride;
    const int64_t slot = p.cache_batch_idx ? p.cache_batch_idx[b] : b;
    const int32_t *table = p.page_table ? p.page_table + b * p.page_table_batch_stride : nullptr;

    for (int g0 = 0; g0 < p.s_q; g0 += TG) {
        const int tg = p.s_q - g0 < TG ? p.s_q - g0 : TG;
        if (g0) __syncthreads();  // (every wave is done with the group before)
        for (int x = tid; x < tg * MB * KS * WAVE; x += THREADS) {
            const int l = x & 63, at = x >> 6, ks = at % KS, mb = at / KS % MB, tok = at / (KS * MB);
            const int head = mb * 32 + (l & 31), ch = q_channel(ks, l >> 5);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (head < p.h_i) v = *reinterpret_cast<const uint4 *>(q + ((g0 + tok) * p.q_row_stride + head * p.q_head_stride + ch) * 2);
            qs[x] = v;
        }
        for (int x = tid; x < tg * HP; x += THREADS) {
            const int tok = x / HP, head = x % HP;
            ws[tok][head] = head < p.h_i ? w[(g0 + tok) * p.w_row_stride + head] : 0.0f;
        }
        __syncthreads();

        const int first = c0 + wave * TILE;  // (wave-uniform; first < sk: the tile is loaded)
        ByteTile<D> next;
        if (first < c1 && first < sk) load_tile<D>(p, table, slot, first, sk, fr, fh, next);
        for (int t0 = first; t0 < c1; t0 += WAVES * TILE) {
            const int key = t0 + lane;  // the key this lane stores
            if (t0 >= sk) {             // (wave-uniform: a tile behind the fill level loads nothing, and none behind it does)
                if (key < c1)
                    for (int tok = 0; tok < tg; ++tok) out[(g0 + tok) * p.logits_row_stride + key] = -INFINITY;
                continue;
            }
            // the tile expanded once, for every token of the group; then the next tile's bytes go in flight
            fa::u32x4 kf[2][KS];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int j = 0; j < D / 32; ++j) {
                    kf[nb][2 * j] = fa::kv8_expand<T>(next.kb[nb][j].x, next.kb[nb][j].y);
                    kf[nb][2 * j + 1] = fa::kv8_expand<T>(next.kb[nb][j].z, next.kb[nb][j].w);
                }
            const float scale = next.scale;
            const int tn = t0 + WAVES * TILE;
            if (tn < c1 && tn < sk) load_tile<D>(p, table, slot, tn, sk, fr, fh, next);
            for (int tok = 0; tok < tg; ++tok) {
                f32x16 acc[MB][2];
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[mb][nb][e] = 0.0f;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) {
                        const uint4 a = qs[((tok * MB + mb) * KS + ks) * WAVE + lane];
#pragma unroll
                        for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = mfma<DT>(a, kf[nb][ks], acc[mb][nb]);
                    }
                }
                // C of a 32 x 32 MFMA: column (key) lane & 31, row (head) (e & 3) + 8 (e >> 2) + 4 fh
                float r[2];
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    float s = 0.0f;
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
                        for (int e = 0; e < 16; ++e)
                            s += ws[tok][mb * 32 + 8 * (e >> 2) + 4 * fh + (e & 3)] * fmaxf(acc[mb][nb][e], 0.0f);
                    }
                    r[nb] = s + __shfl_xor(s, 32, WAVE);
                }
                const int i = g0 + tok;
                const float v = (fh ? r[1] : r[0]) * scale;  // (row nb = fh, fr of this lane: the one whose scale it loaded)
                if (key < c1) out[i * p.logits_row_stride + key] = key < visible_of(p, sk, i) ? v + 0.0f : -INFINITY;  // (+ 0: -0 is stored as +0)
            }
        }
    }
}

// ---- selection --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SELECT_LARGE) void index_select_kernel(const fa_index_topk8_params p) {
    const int i = blockIdx.x, b = blockIdx.y;
    index_select_row(p.logits + b * p.logits_batch_stride + i * p.logits_row_stride, p.indices + b * p.idx_batch_stride + i * p.idx_row_stride,
                     visible_of(p, fill_of(p, b), i), p.topk);
}

// ---- append -----------------------------------------------------------------------------------------------------------------
// e of scale = 2^e from the bits of amax >= 0 (finite): amax = 1.M * 2^(E - 127) and 448 = 1.75 * 2^8, so the smallest e with
// amax * 2^-e <= 448 is E - 127 - 8 where 1.M <= 1.75 and one more above it.  An fp32 subnormal (E = 0) clamps to -126; 0 gives 0.
__device__ __forceinline__ int scale_exponent(float amax) {
    const uint32_t u = __builtin_bit_cast(uint32_t, amax);
    if (u == 0u) return 0;
    const int E = (int)(u >> 23), M = (int)(u & 0x7fffffu);
    return clampi(E - 127 - 8 + (M > 0x600000 ? 1 : 0), -126, 127);
}

template <typename T, int D>
__global__ __launch_bounds__(THREADS) void index_append8_kernel(const fa_index_append8_params p) {
    constexpr int LPR = D / 8, RPW = WAVE / LPR;  // lanes per row, rows per wave and pass
    const int lane = threadIdx.x & 63, sub = lane % LPR, rw = lane / LPR;
    const int64_t gid = (int64_t)blockIdx.x * THREADS + threadIdx.x, nthreads = (int64_t)gridDim.x * THREADS;
    const bool ragged = p.cu_seqlens_k_new != nullptr;
    for (int64_t s = gid; s < p.b; s += nthreads) {  // the fill levels behind the append
        const int len = ragged ? p.cu_seqlens_k_new[s + 1] - p.cu_seqlens_k_new[s] : p.s_new;
        p.seqused_out[s] = min(p.cache_seqlens[s] + len, p.capacity);
    }
    const int64_t rows = ragged ? p.total_new : (int64_t)p.b * p.s_new;
    const T *src_rows = static_cast<const T *>(p.k_index_new);
    for (int64_t r0 = (gid >> 6) * RPW; r0 < rows; r0 += (nthreads >> 6) * RPW) {  // (wave-uniform bounds: every lane shuffles)
        const int64_t r = r0 + rw;
        bool live = r < rows;
        int seq = 0, i = 0;
        int64_t src = 0;
        if (live && ragged) {  // the entry whose range holds row r: the last seq with cu[seq] <= r
            int lo = 0, hi = p.b;  // (cu[lo] <= r where any is; the answer is in [lo, hi))
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (p.cu_seqlens_k_new[mid] <= r) lo = mid; else hi = mid;
            }
            seq = lo;
            i = (int)(r - p.cu_seqlens_k_new[seq]);
            live = i >= 0 && r < p.cu_seqlens_k_new[seq + 1];  // (rows of total_new outside every range are not appended)
            src = r * p.new_row_stride;
        } else if (live) {
            seq = (int)(r / p.s_new), i = (int)(r % p.s_new);
            src = seq * p.new_batch_stride + i * p.new_row_stride;
        }
        int dst = 0;
        if (live) {
            dst = p.cache_seqlens[seq] + i;
            live = dst >= 0 && dst < p.capacity;  // past the capacity: dropped
        }
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (live) w = *reinterpret_cast<const uint4 *>(src_rows + src + sub * 8);
        float x[8];
        fa::unpack8<T>(w, x);
        float amax = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(x[j]));
#pragma unroll
        for (int m = 1; m < LPR; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m, WAVE));
        const int e = scale_exponent(amax);
        if (!live) continue;
        int64_t entry = p.cache_batch_idx ? p.cache_batch_idx[seq] : seq, in = dst;
        if (p.page_table) {
            const int pg = dst / p.page_size;
            entry = p.page_table[seq * p.page_table_batch_stride + pg];
            in = dst - pg * p.page_size;
        }
        // x * 2^-e is exact and within +-448; 2^-e by ldexp: 2^-127 is an fp32 subnormal
        const uint2 bytes = fa::quantise8<T>(w, __builtin_amdgcn_ldexpf(1.0f, -e));
        *reinterpret_cast<uint2 *>(static_cast<char *>(p.k_index_cache) + entry * p.cache_batch_stride + in * p.cache_row_stride + sub * 8) = bytes;
        if (sub == 0) p.k_index_scale[entry * p.scale_batch_stride + in] = __builtin_bit_cast(float, (uint32_t)(e + 127) << 23);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
bool sixteen_bit(int dt) { return dt == FA_DTYPE_FP16 || dt == FA_DTYPE_BF16; }

struct Form {
    int chunk, chunks, threads;
};
Form form_of(const fa_index_topk8_params *p) {
    const int chunk = chunk_of(p->b, p->capacity);
    return {chunk, (p->capacity + chunk - 1) / chunk, select_threads(p->capacity)};
}

template <int DT, int D>
void launch_logits(const fa_index_topk8_params &p, dim3 grid, hipStream_t stream) {
    if (p.h_i > 32) hipLaunchKernelGGL((index_logits8_kernel<DT, D, 2>), grid, dim3(THREADS), 0, stream, p);
    else hipLaunchKernelGGL((index_logits8_kernel<DT, D, 1>), grid, dim3(THREADS), 0, stream, p);
}

int64_t append_rows(const fa_index_append8_params *p) { return p->cu_seqlens_k_new ? p->total_new : (int64_t)p->b * p->s_new; }
// workgroups: a wave per pass of 64 / (d_i / 8) rows, 4 waves each, at most APPEND_GRID_MAX (the waves then stride)
int append_grid(const fa_index_append8_params *p) {
    const int rows_per_wg = WAVES * (WAVE * 8 / p->d_i);
    return (int)std::max<int64_t>(1, std::min<int64_t>((append_rows(p) + rows_per_wg - 1) / rows_per_wg, APPEND_GRID_MAX));
}

}  // namespace

extern "C" {

uint32_t fa_index_topk8_params_size(void) { return (uint32_t)sizeof(fa_index_topk8_params); }

int fa_index_topk8_validate(const fa_index_topk8_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_index_topk8_params)) return FA_ERR_BAD_ABI;
    if (!sixteen_bit(p->dtype)) return FA_ERR_BAD_DTYPE;
    if (sixteen_bit(p->cache_dtype)) return FA_ERR_UNSUPPORTED;  // (the 16-bit index cache is fa_index_topk's)
    if (p->cache_dtype != FA_DTYPE_FP8_E4M3) return FA_ERR_BAD_DTYPE;
    if (p->d_i != 64 && p->d_i != 128) return FA_ERR_BAD_HEAD_DIM;
    if (p->h_i < 16 || p->h_i > FA_INDEX_MAX_HEADS || p->h_i % 16 != 0) return FA_ERR_BAD_HEADS;
    if (p->cu_seqlens_q || p->cache_leftpad) return FA_ERR_UNSUPPORTED;
    if (p->b < 0 || p->b > 65535 || p->s_q < 1 || p->s_q > FA_INDEX_MAX_ROWS) return FA_ERR_BAD_SHAPE;
    if (p->capacity < 1 || p->capacity > FA_INDEX_MAX_KEYS) return FA_ERR_BAD_SHAPE;
    if (p->topk < 1 || p->list_width < p->topk || p->logits_width < p->capacity) return FA_ERR_BAD_SHAPE;
    if (p->page_table && (p->page_size <= 0 || p->capacity % p->page_size != 0 || p->cache_batch_idx)) return FA_ERR_BAD_SHAPE;
    if (!p->q_index || !p->k_index_cache || !p->k_index_scale || !p->weights || !p->cache_seqlens || !p->logits || !p->indices)
        return FA_ERR_NULL_POINTER;
    if (!aligned_to(p->q_index, 16) || !aligned_to(p->k_index_cache, 16) || !aligned_to(p->k_index_scale, 4) || !aligned_to(p->weights, 4) ||
        !aligned_to(p->cache_seqlens, 4) || !aligned_to(p->cache_batch_idx, 4) || !aligned_to(p->page_table, 4) || !aligned_to(p->logits, 4) ||
        !aligned_to(p->indices, 4))
        return FA_ERR_BAD_STRIDE;
    for (const int64_t s : {p->q_batch_stride, p->q_row_stride, p->q_head_stride})
        if (s % 8 != 0) return FA_ERR_BAD_STRIDE;
    if (p->cache_batch_stride % 16 != 0 || p->cache_row_stride % 16 != 0 || p->scale_batch_stride < 0) return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int64_t fa_index_topk8_workspace_size(const fa_index_topk8_params *p) {
    const int st = fa_index_topk8_validate(p);
    return st != FA_OK ? st : (int64_t)p->b * p->s_q * p->capacity * (int64_t)sizeof(float);
}

const char *fa_index_topk8_plan_name(const fa_index_topk8_params *p) {
    if (fa_index_topk8_validate(p) != FA_OK) return nullptr;
    thread_local char name[160];
    const Form f = form_of(p);
    std::snprintf(name, sizeof name, "index_logits8_kernel d=%d heads=%d sq=%d chunk=%d grid=(%d,%d) | index_select_kernel threads=%d passes=%d",
                  p->d_i, p->h_i, p->s_q, f.chunk, f.chunks, p->b, f.threads, PASSES);
    return name;
}

int fa_index_topk8(const fa_index_topk8_params *p, void *stream_) {
    const int st = fa_index_topk8_validate(p);
    if (st != FA_OK) return st;
    if (p->b == 0) return FA_OK;  // (no zero grid)
    const Form f = form_of(p);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(f.chunks, p->b);
    if (p->dtype == FA_DTYPE_BF16) {
        if (p->d_i == 128) launch_logits<FA_DTYPE_BF16, 128>(*p, grid, stream);
        else launch_logits<FA_DTYPE_BF16, 64>(*p, grid, stream);
    } else {
        if (p->d_i == 128) launch_logits<FA_DTYPE_FP16, 128>(*p, grid, stream);
        else launch_logits<FA_DTYPE_FP16, 64>(*p, grid, stream);
    }
    hipLaunchKernelGGL(index_select_kernel, dim3(p->s_q, p->b), dim3(f.threads), 0, stream, *p);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

uint32_t fa_index_append8_params_size(void) { return (uint32_t)sizeof(fa_index_append8_params); }

int fa_index_append8_validate(const fa_index_append8_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_index_append8_params)) return FA_ERR_BAD_ABI;
    if (!sixteen_bit(p->dtype)) return FA_ERR_BAD_DTYPE;
    if (p->d_i != 64 && p->d_i != 128) return FA_ERR_BAD_HEAD_DIM;
    const bool ragged = p->cu_seqlens_k_new != nullptr;
    if (p->b < 1 || p->capacity < 1 || p->capacity > FA_INDEX_MAX_KEYS || (ragged ? p->total_new < 0 : p->s_new < 0)) return FA_ERR_BAD_SHAPE;
    if (p->page_table && (p->page_size <= 0 || p->capacity % p->page_size != 0 || p->cache_batch_idx)) return FA_ERR_BAD_SHAPE;
    if (!p->cache_seqlens || !p->seqused_out) return FA_ERR_NULL_POINTER;
    if (p->seqused_out == p->cache_seqlens) return FA_ERR_BAD_SHAPE;
    if (append_rows(p) > 0 && (!p->k_index_new || !p->k_index_cache || !p->k_index_scale)) return FA_ERR_NULL_POINTER;
    if (!aligned_to(p->k_index_new, 16) || !aligned_to(p->k_index_cache, 8) || !aligned_to(p->k_index_scale, 4) ||
        !aligned_to(p->cache_seqlens, 4) || !aligned_to(p->cache_batch_idx, 4) || !aligned_to(p->page_table, 4) ||
        !aligned_to(p->cu_seqlens_k_new, 4) || !aligned_to(p->seqused_out, 4))
        return FA_ERR_BAD_STRIDE;
    if (p->new_row_stride % 8 != 0 || (!ragged && p->new_batch_stride % 8 != 0)) return FA_ERR_BAD_STRIDE;
    if (p->cache_batch_stride % 8 != 0 || p->cache_row_stride % 8 != 0 || p->scale_batch_stride < 0) return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

const char *fa_index_append8_plan_name(const fa_index_append8_params *p) {
    if (fa_index_append8_validate(p) != FA_OK) return nullptr;
    thread_local char name[96];
    std::snprintf(name, sizeof name, "index_append8_kernel d=%d rows_per_wave=%d grid=%d", p->d_i, WAVE * 8 / p->d_i, append_grid(p));
    return name;
}

int fa_index_append8(const fa_index_append8_params *p, void *stream_) {
    const int st = fa_index_append8_validate(p);
    if (st != FA_OK) return st;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(append_grid(p));
    if (p->dtype == FA_DTYPE_BF16) {
        if (p->d_i == 128) hipLaunchKernelGGL((index_append8_kernel<__bf16, 128>), grid, dim3(THREADS), 0, stream, *p);
        else hipLaunchKernelGGL((index_append8_kernel<__bf16, 64>), grid, dim3(THREADS), 0, stream, *p);
    } else {
        if (p->d_i == 128) hipLaunchKernelGGL((index_append8_kernel<_Float16, 128>), grid, dim3(THREADS), 0, stream, *p);
        else hipLaunchKernelGGL((index_append8_kernel<_Float16, 64>), grid, dim3(THREADS), 0, stream, *p);
    }
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

}  // extern "C"
