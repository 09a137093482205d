// fa_index_topk.hip — the lightning indexer of DeepSeek-V3.2-style sparse attention (include/fa_index_topk.h): the index logits
// of a decode-sized step against the indexer's single-head key cache, and the top-k positions of every query token as the list
// the token-sparse MLA decode reads.  A translation unit of its own.  The workgroup scan and the host predicates are
// fa_rowwise.h's, the order-preserving key of a logit is the one of fa_sample_device.h; the descent is the method of
// fa_block_select.hip's block_select_kernel over a row that lives in global memory (a copy: that unit stays what its tests pin),
// and its text is fa_index_select.h's, shared with the prefill-sized unit fa_index_prefill.hip.
//
// index_logits_kernel<DT, D, MB>: one workgroup of 4 waves per (chunk of keys, batch entry).  The query fragments of a group of
//   TG tokens lie in LDS in MFMA operand order (slot (token, m block, k step), then lane: every fragment read is 64 consecutive
//   16-byte words) with their weights; heads behind h_i are zero rows.  A wave owns tiles of 64 key rows: lane (fr, fh) loads
//   the 8 channels 16 ks + 8 fh of the rows fr and 32 + fr by 16-byte loads straight into the B operand (a row is one wave's:
//   no LDS for K), the page of a row is resolved once per row.  S (heads x keys) = Q . K^T on v_mfma_f32_32x32x16: the
//   accumulator holds 16 heads of ONE key per lane, so ReLU, the weights and the head sum are in-lane but for one swap with
//   lane ^ 32.  The tokens of the group loop over the resident tile; a logit per key leaves as one 256-byte store per wave.
// index_select_kernel: one workgroup per (token, batch entry) runs fa_index_select.h's index_select_row over the token's row of
//   logits.
#include "../../include/fa_index_topk.h"
#include "fa_index_select.h"

#include <cstdio>

namespace {

using namespace fa_row;
using namespace fa_index_sel;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int THREADS = 256, WAVES = THREADS / WAVE;  // of the logits
constexpr int TILE = 64;                              // key rows of a wave's tile
constexpr int CHUNK_MIN = WAVES * TILE, CHUNK_MAX = 1024, GRID_AIM = 1024;
constexpr int Q_LDS_BYTES = 48 * 1024;                // of the query fragments of a token group

__host__ __device__ constexpr int tokens_per_group(int D, int MB) {
    return Q_LDS_BYTES / (MB * 32 * D * 2) < FA_INDEX_MAX_ROWS ? Q_LDS_BYTES / (MB * 32 * D * 2) : FA_INDEX_MAX_ROWS;
}

// keys per workgroup: the smallest of 256, 512, 1024 that keeps the grid at or below GRID_AIM workgroups (1024 where none does)
__host__ __device__ inline int chunk_of(int b, int capacity) {
    int c = CHUNK_MIN;
    while (c < CHUNK_MAX && (int64_t)b * ((capacity + c - 1) / c) > GRID_AIM) c *= 2;
    return c;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__device__ __forceinline__ int fill_of(const fa_index_topk_params &p, int b) { return clampi(p.cache_seqlens[b], 0, p.capacity); }
// n(b, i): the candidates of token i
__device__ __forceinline__ int visible_of(const fa_index_topk_params &p, int sk, int i) {
    return p.is_causal ? clampi(sk - (p.s_q - 1 - i), 0, sk) : sk;
}

template <int DT>
__device__ __forceinline__ f32x16 mfma(const uint4 a, const uint4 b, const f32x16 c) {
    if constexpr (DT == FA_DTYPE_BF16)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// ---- logits -----------------------------------------------------------------------------------------------------------------
template <int DT, int D, int MB>
__global__ __launch_bounds__(THREADS) void index_logits_kernel(const fa_index_topk_params p) {
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
    const char *cache = static_cast<const char *>(p.k_index_cache);
    const int64_t slot = p.cache_batch_idx ? p.cache_batch_idx[b] : b;
    const int32_t *table = p.page_table ? p.page_table + b * p.page_table_batch_stride : nullptr;

    for (int g0 = 0; g0 < p.s_q; g0 += TG) {
        const int tg = p.s_q - g0 < TG ? p.s_q - g0 : TG;
        if (g0) __syncthreads();  // (every wave is done with the group before)
        for (int x = tid; x < tg * MB * KS * WAVE; x += THREADS) {
            const int l = x & 63, at = x >> 6, ks = at % KS, mb = at / KS % MB, tok = at / (KS * MB);
            const int head = mb * 32 + (l & 31), ch = ks * 16 + (l >> 5) * 8;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (head < p.h_i) v = *reinterpret_cast<const uint4 *>(q + ((g0 + tok) * p.q_row_stride + head * p.q_head_stride + ch) * 2);
            qs[x] = v;
        }
        for (int x = tid; x < tg * HP; x += THREADS) {
            const int tok = x / HP, head = x % HP;
            ws[tok][head] = head < p.h_i ? w[(g0 + tok) * p.w_row_stride + head] : 0.0f;
        }
        __syncthreads();

        for (int t0 = c0 + wave * TILE; t0 < c1; t0 += WAVES * TILE) {
            const int key = t0 + lane;  // the key this lane stores
            if (t0 >= sk) {             // (wave-uniform: a tile behind the fill level loads nothing)
                if (key < c1)
                    for (int tok = 0; tok < tg; ++tok) out[(g0 + tok) * p.logits_row_stride + key] = -INFINITY;
                continue;
            }
            uint4 kf[2][KS];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const int s = t0 + nb * 32 + fr;
                const int row = s < sk ? s : t0;  // (a row at or behind sk is never read: its logit is -inf whatever is loaded here)
                int64_t at;
                if (table) {
                    const uint32_t pg = (uint32_t)row / (uint32_t)p.page_size;
                    at = (int64_t)table[pg] * p.cache_batch_stride + (int64_t)((uint32_t)row - pg * (uint32_t)p.page_size) * p.cache_row_stride;
                } else {
                    at = slot * p.cache_batch_stride + (int64_t)row * p.cache_row_stride;
                }
                const char *src = cache + (at + fh * 8) * 2;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) kf[nb][ks] = *reinterpret_cast<const uint4 *>(src + ks * 32);
            }
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
                const float v = fh ? r[1] : r[0];
                if (key < c1) out[i * p.logits_row_stride + key] = key < visible_of(p, sk, i) ? v + 0.0f : -INFINITY;  // (+ 0: -0 is stored as +0)
            }
        }
    }
}

// ---- selection --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SELECT_LARGE) void index_select_kernel(const fa_index_topk_params p) {
    const int i = blockIdx.x, b = blockIdx.y;
    index_select_row(p.logits + b * p.logits_batch_stride + i * p.logits_row_stride, p.indices + b * p.idx_batch_stride + i * p.idx_row_stride,
                     visible_of(p, fill_of(p, b), i), p.topk);
}

// ---- host -------------------------------------------------------------------------------------------------------------------
bool sixteen_bit(int dt) { return dt == FA_DTYPE_FP16 || dt == FA_DTYPE_BF16; }

struct Form {
    int chunk, chunks, threads;
};
Form form_of(const fa_index_topk_params *p) {
    const int chunk = chunk_of(p->b, p->capacity);
    return {chunk, (p->capacity + chunk - 1) / chunk, select_threads(p->capacity)};
}

template <int DT, int D>
void launch_logits(const fa_index_topk_params &p, dim3 grid, hipStream_t stream) {
    if (p.h_i > 32) hipLaunchKernelGGL((index_logits_kernel<DT, D, 2>), grid, dim3(THREADS), 0, stream, p);
    else hipLaunchKernelGGL((index_logits_kernel<DT, D, 1>), grid, dim3(THREADS), 0, stream, p);
}

}  // namespace

extern "C" {

uint32_t fa_index_topk_params_size(void) { return (uint32_t)sizeof(fa_index_topk_params); }

int fa_index_topk_validate(const fa_index_topk_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_index_topk_params)) return FA_ERR_BAD_ABI;
    if (!sixteen_bit(p->dtype)) return FA_ERR_BAD_DTYPE;
    if (p->cache_dtype == FA_DTYPE_FP8_E4M3) return FA_ERR_UNSUPPORTED;  // (the e4m3 index cache is not built)
    if (p->cache_dtype != p->dtype) return FA_ERR_BAD_DTYPE;
    if (p->d_i != 64 && p->d_i != 128) return FA_ERR_BAD_HEAD_DIM;
    if (p->h_i < 16 || p->h_i > FA_INDEX_MAX_HEADS || p->h_i % 16 != 0) return FA_ERR_BAD_HEADS;
    if (p->cu_seqlens_q || p->cache_leftpad) return FA_ERR_UNSUPPORTED;
    if (p->b < 0 || p->b > 65535 || p->s_q < 1 || p->s_q > FA_INDEX_MAX_ROWS) return FA_ERR_BAD_SHAPE;
    if (p->capacity < 1 || p->capacity > FA_INDEX_MAX_KEYS) return FA_ERR_BAD_SHAPE;
    if (p->topk < 1 || p->list_width < p->topk || p->logits_width < p->capacity) return FA_ERR_BAD_SHAPE;
    if (p->page_table && (p->page_size <= 0 || p->capacity % p->page_size != 0 || p->cache_batch_idx)) return FA_ERR_BAD_SHAPE;
    if (!p->q_index || !p->k_index_cache || !p->weights || !p->cache_seqlens || !p->logits || !p->indices) return FA_ERR_NULL_POINTER;
    if (!aligned_to(p->q_index, 16) || !aligned_to(p->k_index_cache, 16) || !aligned_to(p->weights, 4) || !aligned_to(p->cache_seqlens, 4) ||
        !aligned_to(p->cache_batch_idx, 4) || !aligned_to(p->page_table, 4) || !aligned_to(p->logits, 4) || !aligned_to(p->indices, 4))
        return FA_ERR_BAD_STRIDE;
    for (const int64_t s : {p->q_batch_stride, p->q_row_stride, p->q_head_stride, p->cache_batch_stride, p->cache_row_stride})
        if (s % 8 != 0) return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int64_t fa_index_topk_workspace_size(const fa_index_topk_params *p) {
    const int st = fa_index_topk_validate(p);
    return st != FA_OK ? st : (int64_t)p->b * p->s_q * p->capacity * (int64_t)sizeof(float);
}

const char *fa_index_topk_plan_name(const fa_index_topk_params *p) {
    if (fa_index_topk_validate(p) != FA_OK) return nullptr;
    thread_local char name[160];
    const Form f = form_of(p);
    std::snprintf(name, sizeof name, "index_logits_kernel d=%d heads=%d sq=%d chunk=%d grid=(%d,%d) | index_select_kernel threads=%d passes=%d",
                  p->d_i, p->h_i, p->s_q, f.chunk, f.chunks, p->b, f.threads, PASSES);
    return name;
}

int fa_index_topk(const fa_index_topk_params *p, void *stream_) {
    const int st = fa_index_topk_validate(p);
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

}  // extern "C"
