// fa_index_prefill8.hip — the prefill-sized lightning indexer over an fp8 (e4m3) index-key cache with one fp32 scale per token
// (include/fa_index_prefill8.h): the index logits of a prompt against the cache fa_index_append8 fills and the top-k positions of
// every query token, in rounds over a workspace of logit rows.  A translation unit of its own beside fa_index_prefill.hip (whose
// work split it takes) and fa_index_topk8.hip (whose rule it follows bit for bit); the selection is fa_index_select.h's text, the
// e4m3 -> 16-bit conversion fa_fwd_kernel_kv8.h's kv8_expand.
//
// index_logits_prefill8_kernel<DT, D, MB>: one workgroup of 4 waves per (token block of BLOCK = 8 tokens, chunk of keys); the
//   QUERY fragments of the block live in registers for the whole item (a wave owns TW = 4 / MB tokens), loaded in the permuted
//   channel order the byte operand dictates (q_channel).  The KEY tiles are BYTES, KT = 128 rows each, global -> registers -> LDS,
//   double-buffered: 2 x 128 x d_i bytes, what the 16-bit kernel spends on 64-row tiles, so one barrier per 128 MFMAs of a wave.
//   Wave w stages the rows 32 w + [0, 32) of a tile: lane (fr, fh) resolves the page of row 32 w + fr once and loads its bytes
//   [32 j + 16 fh, +16), j < d_i / 32 -- 32 contiguous bytes per row and load instruction -- and the lanes fh = 0 load the row's
//   scale from the same page.  LDS is in operand order for bytes: the 16-byte word of lane l for (n block nb, pair j) at
//   (nb * J + j) * 64 + l, so a wave writes and reads 64 consecutive words; one 16-byte read feeds TWO k-steps (low 8 bytes: step
//   2 j, high 8: step 2 j + 1), 8 MFMAs, and the bytes become 16-bit values only there, at the operand, between the MFMAs of the
//   fragment before.  The scales sit beside the bytes, 128 floats a buffer: the lane that stores key t0 + .. reads its scale
//   back and multiplies the head sum once, after the swap with lane ^ 32.
//   MB = 2: the four waves own two tokens each and walk the four 32-key blocks of a tile; MB = 1: two waves own four tokens
//   each, and the two pairs of waves take two 32-key blocks each.  Two 32-key blocks make one 256-byte store per wave and token.
//   A tile at or behind the block's largest n(b, i) is not loaded; nothing is stored at or behind a token's n(b, i).
// index_select_prefill_kernel: one workgroup per token of the round runs index_select_row over the token's workspace row.
#include "../../include/fa_index_prefill8.h"
#include "fa_fwd_kernel_kv8.h"
#include "fa_index_select.h"

#include <cstdio>

namespace {

using namespace fa_row;
using namespace fa_index_sel;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int THREADS = 256, WAVES = THREADS / WAVE, BLOCK = FA_INDEX_PREFILL_BLOCK;
constexpr int KT = FA_INDEX_PREFILL8_TILE, NB = KT / 32;  // key rows of a tile in LDS; its 32-key blocks
constexpr int CHUNK_MIN = 256, CHUNK_MAX = 4096, GRID_AIM = 4096;
constexpr int64_t ROUND_MAX_BLOCKS = 1 << 20;  // of one round: both grids stay far below 2^31
static_assert(NB == WAVES && CHUNK_MIN % KT == 0, "a wave stages one 32-key block of a tile; a chunk is whole tiles");

template <int DT> struct Elem16;
template <> struct Elem16<FA_DTYPE_BF16> { typedef __bf16 T; };
template <> struct Elem16<FA_DTYPE_FP16> { typedef _Float16 T; };

// keys per work item: fa_index_prefill.hip's rule
inline int chunk_of(int64_t blocks, int capacity) {
    int c = CHUNK_MIN;
    while (c < CHUNK_MAX && blocks * ((capacity + c - 1) / c) > GRID_AIM) c *= 2;
    return c;
}

// the first of the 8 channels half fh of a lane contracts in k-step ks: what bytes [8 (ks & 1), +8) of the 16-byte word
// 32 (ks >> 1) + 16 fh of a key row hold (fa_index_topk8.hip's order)
__device__ __forceinline__ int q_channel(int ks, int fh) { return (ks >> 1) * 32 + fh * 16 + (ks & 1) * 8; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__device__ __forceinline__ int fill_of(const fa_index_prefill8_params &p, int b) { return clampi(p.cache_seqlens[b], 0, p.capacity); }
// n(b, i): the candidates of token i
__device__ __forceinline__ int visible_of(const fa_index_prefill8_params &p, int sk, int i) {
    return p.is_causal ? clampi(sk - (p.s_q - 1 - i), 0, sk) : sk;
}

template <int DT>
__device__ __forceinline__ f32x16 mfma(const uint4 a, const fa::u32x4 b, const f32x16 c) {
    if constexpr (DT == FA_DTYPE_BF16)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// a thread's part of a tile: the J 16-byte words of its row and half
template <int J>
struct Staged {
    uint4 v[J];
};

// the blocks [first, first + count) of the call in this round, `chunks` chunks of `chunk` keys each
struct Round {
    int first, count, chunk, chunks;
};

// ---- logits -----------------------------------------------------------------------------------------------------------------
template <int DT, int D, int MB>
__global__ __launch_bounds__(THREADS) void index_logits_prefill8_kernel(const fa_index_prefill8_params p, const Round rd) {
    typedef typename Elem16<DT>::T T;
    constexpr int KS = D / 16, J = D / 32, TW = 4 / MB, WT = BLOCK / TW, WK = WAVES / WT, NBW = NB / WK;
    static_assert(NBW % 2 == 0, "a wave stores its 32-key blocks in pairs");
    __shared__ uint4 kt[2][NB * J * WAVE];  // the word of lane l for (n block, pair j) at (nb * J + j) * 64 + l
    __shared__ float sc[2][KT];             // the scales of the tile's rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 31, fh = lane >> 5;
    const int wt = wave % WT, wk = wave / WT;
    // the item: chunk c of block g; the later blocks of a causal prompt see more keys, and they go first
    const int c = blockIdx.x % rd.chunks, g = rd.first + (rd.count - 1 - blockIdx.x / rd.chunks);
    const int nblk = (p.s_q + BLOCK - 1) / BLOCK, b = g / nblk, i0 = (g - b * nblk) * BLOCK;
    const int sk = fill_of(p, b);
    const int last = i0 + BLOCK < p.s_q ? i0 + BLOCK - 1 : p.s_q - 1;
    const int seen = visible_of(p, sk, last);  // the largest n of the block (n grows with i)
    const int c0 = c * rd.chunk, c1 = c0 + rd.chunk < seen ? c0 + rd.chunk : seen;
    if (c0 >= c1) return;  // nothing visible here: no load, no store (uniform)

    const char *qb = static_cast<const char *>(p.q_index) + b * p.q_batch_stride * 2;
    const float *wb = p.weights + b * p.w_batch_stride;
    const char *cache = static_cast<const char *>(p.k_index_cache);
    const int64_t slot = p.cache_batch_idx ? p.cache_batch_idx[b] : b;
    const int32_t *table = p.page_table ? p.page_table + b * p.page_table_batch_stride : nullptr;
    const bool pow2 = table && (p.page_size & (p.page_size - 1)) == 0;
    const int shift = __ffs(p.page_size) - 1;

    // this wave's tokens: fragments (k-step ks holds the channels q_channel(ks, fh) + [0, 8): A agrees with the byte operand),
    // weights, candidates and workspace rows.  A token behind s_q takes the last one's operands and stores nothing (n = 0)
    uint4 q[TW][MB][KS];
    float w[TW][MB][16];
    int nv[TW];
    float *out[TW];
#pragma unroll
    for (int t = 0; t < TW; ++t) {
        const int it = i0 + wt * TW + t, i = it < p.s_q ? it : p.s_q - 1;
        nv[t] = it < p.s_q ? visible_of(p, sk, it) : 0;
        out[t] = p.workspace + ((int64_t)(g - rd.first) * BLOCK + wt * TW + t) * p.workspace_row_stride;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const int head = mb * 32 + fr;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);  // (heads behind h_i are zero rows)
                if (head < p.h_i) v = *reinterpret_cast<const uint4 *>(qb + (i * p.q_row_stride + head * p.q_head_stride + q_channel(ks, fh)) * 2);
                q[t][mb][ks] = v;
            }
            // C of a 32 x 32 MFMA: column (key) lane & 31, row (head) (e & 3) + 8 (e >> 2) + 4 fh
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int hw = mb * 32 + 8 * (e >> 2) + 4 * fh + (e & 3);
                w[t][mb][e] = hw < p.h_i ? wb[i * p.w_row_stride + hw] : 0.0f;
            }
        }
    }

    // a thread's part of the tile at t0: row t0 + 32 wave + fr, its page resolved once, J words and the scale.  A row at or
    // behind sk is never read, and neither is its scale: it takes the tile's first row, and its logit is not stored
    float next_scale;  // (beside the staged words, not in their struct: a mixed struct is kept in scratch)
    auto load_tile = [&](const int t0) {
        Staged<J> r;
        const int s = t0 + wave * 32 + fr, row = s < sk ? s : t0;
        int64_t entry = slot, in = row;
        if (table) {
            const uint32_t pg = pow2 ? (uint32_t)row >> shift : (uint32_t)row / (uint32_t)p.page_size;
            entry = table[pg];
            in = (uint32_t)row - pg * (uint32_t)p.page_size;
        }
        const char *src = cache + entry * p.cache_batch_stride + in * p.cache_row_stride + fh * 16;
#pragma unroll
        for (int j = 0; j < J; ++j) r.v[j] = *reinterpret_cast<const uint4 *>(src + j * 32);
        next_scale = p.k_index_scale[entry * p.scale_batch_stride + in];
        return r;
    };

    Staged<J> next = load_tile(c0);
#pragma unroll
    for (int j = 0; j < J; ++j) kt[0][(wave * J + j) * WAVE + lane] = next.v[j];
    if (fh == 0) sc[0][wave * 32 + fr] = next_scale;
    __syncthreads();

    int buf = 0;
    for (int t0 = c0; t0 < c1; t0 += KT, buf ^= 1) {
        const bool more = t0 + KT < c1;  // (uniform)
        if (more) next = load_tile(t0 + KT);  // in flight under this tile's MFMAs
#pragma unroll
        for (int pr = 0; pr < NBW / 2; ++pr) {  // (unrolled: the epilogue of one 32-key block issues between the MFMAs of the next)
            float r0[TW], r1[TW];  // the sums of the pair's first and second 32-key block (two arrays: no indexing by fh)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int nb = wk * NBW + pr * 2 + n;
                f32x16 acc[TW][MB];
#pragma unroll
                for (int t = 0; t < TW; ++t)
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[t][mb][e] = 0.0f;
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const uint4 kw = kt[buf][(nb * J + j) * WAVE + lane];
                    const fa::u32x4 lo = fa::kv8_expand<T>(kw.x, kw.y);
#pragma unroll
                    for (int t = 0; t < TW; ++t)
#pragma unroll
                        for (int mb = 0; mb < MB; ++mb) acc[t][mb] = mfma<DT>(q[t][mb][2 * j], lo, acc[t][mb]);
                    const fa::u32x4 hi = fa::kv8_expand<T>(kw.z, kw.w);  // (under the four MFMAs above)
#pragma unroll
                    for (int t = 0; t < TW; ++t)
#pragma unroll
                        for (int mb = 0; mb < MB; ++mb) acc[t][mb] = mfma<DT>(q[t][mb][2 * j + 1], hi, acc[t][mb]);
                }
#pragma unroll
                for (int t = 0; t < TW; ++t) {
                    float s = 0.0f;
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
                        for (int e = 0; e < 16; ++e) s += w[t][mb][e] * fmaxf(acc[t][mb][e], 0.0f);
                    }
                    (n ? r1[t] : r0[t]) = s + __shfl_xor(s, 32, WAVE);
                }
            }
            // both 32-key blocks of the pair: one 256-byte store per wave and token, the key's scale from beside the bytes
            const int at = (wk * NBW + pr * 2) * 32 + lane, key = t0 + at;
            const float scale = sc[buf][at];
#pragma unroll
            for (int t = 0; t < TW; ++t) {
                const float v = (fh ? r1[t] : r0[t]) * scale;
                if (key < nv[t]) out[t][key] = v + 0.0f;  // (+ 0: -0 is stored as +0)
            }
        }
        if (more) {
#pragma unroll
            for (int j = 0; j < J; ++j) kt[buf ^ 1][(wave * J + j) * WAVE + lane] = next.v[j];
            if (fh == 0) sc[buf ^ 1][wave * 32 + fr] = next_scale;
        }
        __syncthreads();  // (the next tile is whole; every wave is done with this one)
    }
}

// ---- selection --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SELECT_LARGE) void index_select_prefill_kernel(const fa_index_prefill8_params p, const Round rd) {
    const int row = blockIdx.x, g = rd.first + row / BLOCK;
    const int nblk = (p.s_q + BLOCK - 1) / BLOCK, b = g / nblk, i = (g - b * nblk) * BLOCK + row % BLOCK;
    if (i >= p.s_q) return;  // (the short last block of an entry; uniform)
    index_select_row(p.workspace + (int64_t)row * p.workspace_row_stride, p.indices + b * p.idx_batch_stride + i * p.idx_row_stride,
                     visible_of(p, fill_of(p, b), i), p.topk);
}

// ---- host -------------------------------------------------------------------------------------------------------------------
bool sixteen_bit(int dt) { return dt == FA_DTYPE_FP16 || dt == FA_DTYPE_BF16; }

struct Form {
    int64_t blocks, per_round, rounds;  // token blocks of the call, of a round; rounds
    int chunk, chunks, threads;
};
Form form_of(const fa_index_prefill8_params *p) {
    Form f;
    f.blocks = (int64_t)p->b * ((p->s_q + BLOCK - 1) / BLOCK);
    f.per_round = p->workspace_rows / BLOCK < ROUND_MAX_BLOCKS ? p->workspace_rows / BLOCK : ROUND_MAX_BLOCKS;
    if (f.per_round > f.blocks) f.per_round = f.blocks;
    f.rounds = f.blocks ? (f.blocks + f.per_round - 1) / f.per_round : 0;
    f.chunk = chunk_of(f.blocks, p->capacity);
    f.chunks = (p->capacity + f.chunk - 1) / f.chunk;
    f.threads = select_threads(p->capacity);
    return f;
}

template <int DT, int D>
void launch_logits(const fa_index_prefill8_params &p, const Round &rd, hipStream_t stream) {
    const dim3 grid((uint32_t)rd.count * (uint32_t)rd.chunks);
    if (p.h_i > 32) hipLaunchKernelGGL((index_logits_prefill8_kernel<DT, D, 2>), grid, dim3(THREADS), 0, stream, p, rd);
    else hipLaunchKernelGGL((index_logits_prefill8_kernel<DT, D, 1>), grid, dim3(THREADS), 0, stream, p, rd);
}

// everything but the workspace
int validate_call(const fa_index_prefill8_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_index_prefill8_params)) return FA_ERR_BAD_ABI;
    if (!sixteen_bit(p->dtype)) return FA_ERR_BAD_DTYPE;
    if (sixteen_bit(p->cache_dtype)) return FA_ERR_UNSUPPORTED;  // (the 16-bit index cache is fa_index_prefill's)
    if (p->cache_dtype != FA_DTYPE_FP8_E4M3) return FA_ERR_BAD_DTYPE;
    if (p->d_i != 64 && p->d_i != 128) return FA_ERR_BAD_HEAD_DIM;
    if (p->h_i < 16 || p->h_i > FA_INDEX_MAX_HEADS || p->h_i % 16 != 0) return FA_ERR_BAD_HEADS;
    if (p->cu_seqlens_q || p->cache_leftpad) return FA_ERR_UNSUPPORTED;
    if (p->b < 0 || p->s_q < 1 || (int64_t)p->b * p->s_q > 0x7fffffffll) return FA_ERR_BAD_SHAPE;
    if (p->capacity < 1 || p->capacity > FA_INDEX_MAX_KEYS) return FA_ERR_BAD_SHAPE;
    if (p->topk < 1 || p->list_width < p->topk) return FA_ERR_BAD_SHAPE;
    if (p->page_table && (p->page_size <= 0 || p->capacity % p->page_size != 0 || p->cache_batch_idx)) return FA_ERR_BAD_SHAPE;
    if (!p->q_index || !p->k_index_cache || !p->k_index_scale || !p->weights || !p->cache_seqlens || !p->indices) return FA_ERR_NULL_POINTER;
    if (!aligned_to(p->q_index, 16) || !aligned_to(p->k_index_cache, 16) || !aligned_to(p->k_index_scale, 4) || !aligned_to(p->weights, 4) ||
        !aligned_to(p->cache_seqlens, 4) || !aligned_to(p->cache_batch_idx, 4) || !aligned_to(p->page_table, 4) || !aligned_to(p->indices, 4))
        return FA_ERR_BAD_STRIDE;
    for (const int64_t s : {p->q_batch_stride, p->q_row_stride, p->q_head_stride})
        if (s % 8 != 0) return FA_ERR_BAD_STRIDE;
    if (p->cache_batch_stride % 16 != 0 || p->cache_row_stride % 16 != 0 || p->scale_batch_stride < 0) return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

}  // namespace

extern "C" {

uint32_t fa_index_prefill8_params_size(void) { return (uint32_t)sizeof(fa_index_prefill8_params); }

int fa_index_prefill8_validate(const fa_index_prefill8_params *p) {
    const int st = validate_call(p);
    if (st != FA_OK) return st;
    if (p->workspace_width < p->capacity || p->workspace_rows < BLOCK || p->workspace_row_stride < p->workspace_width) return FA_ERR_BAD_SHAPE;
    if (!p->workspace) return FA_ERR_NULL_POINTER;
    if (!aligned_to(p->workspace, 4)) return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int64_t fa_index_prefill8_workspace_size(const fa_index_prefill8_params *p, int32_t one_round) {
    const int st = validate_call(p);
    if (st != FA_OK) return st;
    const int64_t blocks = one_round ? (int64_t)p->b * ((p->s_q + BLOCK - 1) / BLOCK) : 1;
    return (blocks > 1 ? blocks : 1) * BLOCK * p->capacity * (int64_t)sizeof(float);
}

const char *fa_index_prefill8_plan_name(const fa_index_prefill8_params *p) {
    if (fa_index_prefill8_validate(p) != FA_OK) return nullptr;
    thread_local char name[256];
    const Form f = form_of(p);
    std::snprintf(name, sizeof name,
                  "index_logits_prefill8_kernel d=%d heads=%d sq=%d block=%d tile=%d chunk=%d grid=%lld | index_select_prefill_kernel threads=%d "
                  "passes=%d grid=%lld | rounds=%lld",
                  p->d_i, p->h_i, p->s_q, BLOCK, KT, f.chunk, (long long)(f.per_round * f.chunks), f.threads, PASSES,
                  (long long)(f.per_round * BLOCK), (long long)f.rounds);
    return name;
}

int fa_index_prefill8(const fa_index_prefill8_params *p, void *stream_) {
    const int st = fa_index_prefill8_validate(p);
    if (st != FA_OK) return st;
    if (p->b == 0) return FA_OK;  // (no zero grid)
    const Form f = form_of(p);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    for (int64_t first = 0; first < f.blocks; first += f.per_round) {
        const Round rd = {(int)first, (int)(f.blocks - first < f.per_round ? f.blocks - first : f.per_round), f.chunk, f.chunks};
        if (p->dtype == FA_DTYPE_BF16) {
            if (p->d_i == 128) launch_logits<FA_DTYPE_BF16, 128>(*p, rd, stream);
            else launch_logits<FA_DTYPE_BF16, 64>(*p, rd, stream);
        } else {
            if (p->d_i == 128) launch_logits<FA_DTYPE_FP16, 128>(*p, rd, stream);
            else launch_logits<FA_DTYPE_FP16, 64>(*p, rd, stream);
        }
        hipLaunchKernelGGL(index_select_prefill_kernel, dim3((uint32_t)rd.count * BLOCK), dim3(f.threads), 0, stream, *p, rd);
    }
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

}  // extern "C"
