// fa_index_prefill.hip — the prefill-sized lightning indexer (include/fa_index_prefill.h): the index logits of a prompt against
// the indexer's single-head key cache and the top-k positions of every query token, in rounds over a workspace of logit rows.
// A translation unit of its own beside fa_index_topk.hip, whose rule it follows bit for bit; the selection is that unit's text
// (fa_index_select.h).
//
// index_logits_prefill_kernel<DT, D, MB>: one workgroup of 4 waves per (token block of BLOCK = 8 tokens, chunk of keys).  A GEMM
//   with M = tokens x heads, N = keys, K = d_i, so the roles are swapped against the decode kernel: the QUERY fragments of the
//   block live in registers for the whole item (a wave owns TW = 4 / MB tokens: 4 x KS fragments = 128 VGPRs at d_i 128, with
//   their 64 weights), the KEY tiles of 64 rows stream global -> registers -> LDS, double-buffered, shared by the four waves, in
//   MFMA operand order (fragment (n block, k step), then lane: a read is 64 consecutive 16-byte words, and so is a write).
//   S (heads x keys) = Q . K^T on v_mfma_f32_32x32x16, 16 channels a step ascending: a lane holds 16 heads of ONE key, so ReLU,
//   the weights and the head sum are in-lane but for one swap with lane ^ 32 -- the order fa_index_topk.h pins.  MB = 2: the
//   four waves own two tokens each and walk both 32-key blocks of a tile; MB = 1: two waves own four tokens each, and the two
//   pairs of waves take one 32-key block each.  Either way a B fragment read from LDS feeds TW * MB = 4 MFMAs.
//   A tile at or behind the block's largest n(b, i) is not loaded; nothing is stored at or behind a token's n(b, i).
// index_select_prefill_kernel: one workgroup per token of the round runs index_select_row over the token's workspace row.
#include "../../include/fa_index_prefill.h"
#include "fa_index_select.h"

#include <cstdio>

namespace {

using namespace fa_row;
using namespace fa_index_sel;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int THREADS = 256, WAVES = THREADS / WAVE, BLOCK = FA_INDEX_PREFILL_BLOCK;
constexpr int KT = 64;  // key rows of a tile in LDS
constexpr int CHUNK_MIN = 256, CHUNK_MAX = 4096, GRID_AIM = 4096;
constexpr int64_t ROUND_MAX_BLOCKS = 1 << 20;  // of one round: both grids stay far below 2^31

// keys per work item: the smallest of 256 ... 4096 that keeps (token blocks of the call) x chunks at or below GRID_AIM (4096
// where none does): one token block over a long cache still spreads over the chip, a long prompt amortises its query loads
inline int chunk_of(int64_t blocks, int capacity) {
    int c = CHUNK_MIN;
    while (c < CHUNK_MAX && blocks * ((capacity + c - 1) / c) > GRID_AIM) c *= 2;
    return c;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__device__ __forceinline__ int fill_of(const fa_index_prefill_params &p, int b) { return clampi(p.cache_seqlens[b], 0, p.capacity); }
// n(b, i): the candidates of token i
__device__ __forceinline__ int visible_of(const fa_index_prefill_params &p, int sk, int i) {
    return p.is_causal ? clampi(sk - (p.s_q - 1 - i), 0, sk) : sk;
}

template <int DT>
__device__ __forceinline__ f32x16 mfma(const uint4 a, const uint4 b, const f32x16 c) {
    if constexpr (DT == FA_DTYPE_BF16)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

template <int N>
struct Regs {
    uint4 v[N];
};

// the blocks [first, first + count) of the call in this round, `chunks` chunks of `chunk` keys each
struct Round {
    int first, count, chunk, chunks;
};

// ---- logits -----------------------------------------------------------------------------------------------------------------
template <int DT, int D, int MB>
__global__ __launch_bounds__(THREADS) void index_logits_prefill_kernel(const fa_index_prefill_params p, const Round rd) {
    constexpr int KS = D / 16, TW = 4 / MB, WT = BLOCK / TW, WK = WAVES / WT, NB = KT / 32, NBW = NB / WK;
    constexpr int FRAGS = NB * KS, LOADS = FRAGS / WAVES;  // fragments of a tile; 16-byte loads of a thread per tile
    static_assert(KS % WAVES == 0 && NB % WK == 0, "a thread's loads of a tile: n block (WAVES * j) / KS, k step wave + (WAVES * j) % KS");
    __shared__ uint4 kt[2][FRAGS * WAVE];  // fragment (n block, k step) of lane l at (nb * KS + ks) * 64 + l
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

    // this wave's tokens: fragments, weights, candidates and workspace rows.  A token behind s_q takes the last one's operands
    // and stores nothing (n = 0)
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
                if (head < p.h_i) v = *reinterpret_cast<const uint4 *>(qb + (i * p.q_row_stride + head * p.q_head_stride + ks * 16 + fh * 8) * 2);
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

    // a thread's part of the tile at t0: LOADS 16-byte words in operand order; the page of a row is resolved once per row.  A
    // row at or behind sk is never read: it takes the tile's first row, and its logit is not stored
    auto load_tile = [&](const int t0) {
        Regs<LOADS> r;
        const char *src[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int s = t0 + nb * 32 + fr, row = s < sk ? s : t0;
            int64_t at;
            if (table) {
                const uint32_t pg = pow2 ? (uint32_t)row >> shift : (uint32_t)row / (uint32_t)p.page_size;
                at = (int64_t)table[pg] * p.cache_batch_stride + (int64_t)((uint32_t)row - pg * (uint32_t)p.page_size) * p.cache_row_stride;
            } else {
                at = slot * p.cache_batch_stride + (int64_t)row * p.cache_row_stride;
            }
            src[nb] = cache + (at + fh * 8) * 2;
        }
#pragma unroll
        for (int j = 0; j < LOADS; ++j) r.v[j] = *reinterpret_cast<const uint4 *>(src[(WAVES * j) / KS] + (wave + (WAVES * j) % KS) * 32);
        return r;
    };

    Regs<LOADS> next = load_tile(c0);
#pragma unroll
    for (int j = 0; j < LOADS; ++j) kt[0][(wave + WAVES * j) * WAVE + lane] = next.v[j];
    __syncthreads();

    int buf = 0;
    for (int t0 = c0; t0 < c1; t0 += KT, buf ^= 1) {
        const bool more = t0 + KT < c1;  // (uniform)
        if (more) next = load_tile(t0 + KT);  // in flight under this tile's MFMAs
        float r0[TW], r1[TW];  // the sums of this wave's first and second 32-key block (two arrays: no indexing by fh)
#pragma unroll
        for (int n = 0; n < NBW; ++n) {  // (unrolled: the epilogue of one 32-key block issues between the MFMAs of the next)
            const int nb = wk * NBW + n;
            f32x16 acc[TW][MB];
#pragma unroll
            for (int t = 0; t < TW; ++t)
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[t][mb][e] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const uint4 kf = kt[buf][(nb * KS + ks) * WAVE + lane];
#pragma unroll
                for (int t = 0; t < TW; ++t)
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) acc[t][mb] = mfma<DT>(q[t][mb][ks], kf, acc[t][mb]);
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
#pragma unroll
        for (int t = 0; t < TW; ++t) {
            if constexpr (NBW == 2) {  // both 32-key halves of the tile: one 256-byte store per wave and token
                const int key = t0 + lane;
                const float v = fh ? r1[t] : r0[t];
                if (key < nv[t]) out[t][key] = v + 0.0f;  // (+ 0: -0 is stored as +0)
            } else {
                const int key = t0 + wk * 32 + fr;
                if (fh == 0 && key < nv[t]) out[t][key] = r0[t] + 0.0f;
            }
        }
        if (more) {
#pragma unroll
            for (int j = 0; j < LOADS; ++j) kt[buf ^ 1][(wave + WAVES * j) * WAVE + lane] = next.v[j];
        }
        __syncthreads();  // (the next tile is whole; every wave is done with this one)
    }
}

// ---- selection --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SELECT_LARGE) void index_select_prefill_kernel(const fa_index_prefill_params p, const Round rd) {
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
Form form_of(const fa_index_prefill_params *p) {
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
void launch_logits(const fa_index_prefill_params &p, const Round &rd, hipStream_t stream) {
    const dim3 grid((uint32_t)rd.count * (uint32_t)rd.chunks);
    if (p.h_i > 32) hipLaunchKernelGGL((index_logits_prefill_kernel<DT, D, 2>), grid, dim3(THREADS), 0, stream, p, rd);
    else hipLaunchKernelGGL((index_logits_prefill_kernel<DT, D, 1>), grid, dim3(THREADS), 0, stream, p, rd);
}

// everything but the workspace
int validate_call(const fa_index_prefill_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_index_prefill_params)) return FA_ERR_BAD_ABI;
    if (!sixteen_bit(p->dtype)) return FA_ERR_BAD_DTYPE;
    if (p->cache_dtype == FA_DTYPE_FP8_E4M3) return FA_ERR_UNSUPPORTED;  // (the e4m3 index cache is not built)
    if (p->cache_dtype != p->dtype) return FA_ERR_BAD_DTYPE;
    if (p->d_i != 64 && p->d_i != 128) return FA_ERR_BAD_HEAD_DIM;
    if (p->h_i < 16 || p->h_i > FA_INDEX_MAX_HEADS || p->h_i % 16 != 0) return FA_ERR_BAD_HEADS;
    if (p->cu_seqlens_q || p->cache_leftpad) return FA_ERR_UNSUPPORTED;
    if (p->b < 0 || p->s_q < 1 || (int64_t)p->b * p->s_q > 0x7fffffffll) return FA_ERR_BAD_SHAPE;
    if (p->capacity < 1 || p->capacity > FA_INDEX_MAX_KEYS) return FA_ERR_BAD_SHAPE;
    if (p->topk < 1 || p->list_width < p->topk) return FA_ERR_BAD_SHAPE;
    if (p->page_table && (p->page_size <= 0 || p->capacity % p->page_size != 0 || p->cache_batch_idx)) return FA_ERR_BAD_SHAPE;
    if (!p->q_index || !p->k_index_cache || !p->weights || !p->cache_seqlens || !p->indices) return FA_ERR_NULL_POINTER;
    if (!aligned_to(p->q_index, 16) || !aligned_to(p->k_index_cache, 16) || !aligned_to(p->weights, 4) || !aligned_to(p->cache_seqlens, 4) ||
        !aligned_to(p->cache_batch_idx, 4) || !aligned_to(p->page_table, 4) || !aligned_to(p->indices, 4))
        return FA_ERR_BAD_STRIDE;
    for (const int64_t s : {p->q_batch_stride, p->q_row_stride, p->q_head_stride, p->cache_batch_stride, p->cache_row_stride})
        if (s % 8 != 0) return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

}  // namespace

extern "C" {

uint32_t fa_index_prefill_params_size(void) { return (uint32_t)sizeof(fa_index_prefill_params); }

int fa_index_prefill_validate(const fa_index_prefill_params *p) {
    const int st = validate_call(p);
    if (st != FA_OK) return st;
    if (p->workspace_width < p->capacity || p->workspace_rows < BLOCK || p->workspace_row_stride < p->workspace_width) return FA_ERR_BAD_SHAPE;
    if (!p->workspace) return FA_ERR_NULL_POINTER;
    if (!aligned_to(p->workspace, 4)) return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int64_t fa_index_prefill_workspace_size(const fa_index_prefill_params *p, int32_t one_round) {
    const int st = validate_call(p);
    if (st != FA_OK) return st;
    const int64_t blocks = one_round ? (int64_t)p->b * ((p->s_q + BLOCK - 1) / BLOCK) : 1;
    return (blocks > 1 ? blocks : 1) * BLOCK * p->capacity * (int64_t)sizeof(float);
}

const char *fa_index_prefill_plan_name(const fa_index_prefill_params *p) {
    if (fa_index_prefill_validate(p) != FA_OK) return nullptr;
    thread_local char name[256];
    const Form f = form_of(p);
    std::snprintf(name, sizeof name,
                  "index_logits_prefill_kernel d=%d heads=%d sq=%d block=%d tile=%d chunk=%d grid=%lld | index_select_prefill_kernel threads=%d "
                  "passes=%d grid=%lld | rounds=%lld",
                  p->d_i, p->h_i, p->s_q, BLOCK, KT, f.chunk, (long long)(f.per_round * f.chunks), f.threads, PASSES,
                  (long long)(f.per_round * BLOCK), (long long)f.rounds);
    return name;
}

int fa_index_prefill(const fa_index_prefill_params *p, void *stream_) {
    const int st = fa_index_prefill_validate(p);
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
