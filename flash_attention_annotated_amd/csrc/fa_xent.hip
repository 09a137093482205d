// fa_xent.hip — fa_xent_fwd / fa_xent_bwd (include/fa_xent.h): the fused cross-entropy loss, forward and backward.
// A translation unit of its own: no kernel comes from another unit or goes to one, because the kernel set of every unit is
// pinned by its tests.  That rule is about kernels: the chunk loads and stores and the host predicates are the inline
// functions of fa_rowwise.h, shared with the other row units.
//
// A row of any pitch and base is three pieces: an element *head* up to the first 16-byte boundary (at most CW - 1 elements), a
// *body* of 16-byte chunks of CW elements (8 of a 16-bit dtype, 4 of fp32), and an element *tail* (at most CW - 1).  The head is
// taken by the first lanes of wavefront 0, the tail by the first lanes of wavefront 1, and thread t of 256 owns the body chunks
// k * 256 + t: neighbouring lanes read neighbouring 16 bytes whatever the phase of the row.  The dtype is a kernel argument,
// hence wave-uniform; the kernels are instantiated by CW only (CW = 1: the body is elements, no head or tail).
// Forward: one workgroup per row.  Every thread keeps a running (max, sum-exp, sum) over its chunks in the base-2 domain,
// x * (logit_scale * log2 e), rescaling its sum once per FWD_UNROLL chunks; one butterfly over the 64 lanes and one LDS exchange
// between the 4 wavefronts per row.  The label's logit is one load by thread 0, issued before the walk.
// Backward: a 2-D grid, blockIdx.y the row and blockIdx.x a slab of 256 * BWD_CHUNKS body chunks (16 KiB of a row); a thread
// loads its BWD_CHUNKS chunks, then computes and stores them: in place it overwrites only what it has read.  The rows of a
// slab column are consecutive workgroups.  No atomics anywhere.
#include "../../include/fa_xent.h"
#include "fa_rowwise.h"

#include <cmath>

namespace {

using namespace fa_row;

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int FWD_UNROLL = 4;           // body chunks a thread has in flight, and absorbs with one rescale
constexpr int FWD_MAX_GRID = 1 << 20;   // workgroups of the forward; further rows are walked by the same workgroups
constexpr int LSE_GIVEN_MAX_GRID = 65536;  // ... of the lse_given forward, 256 rows each
constexpr int BWD_CHUNKS = 4;           // body chunks per thread and slab
constexpr int BWD_SLAB = THREADS * BWD_CHUNKS;
constexpr int BWD_MAX_SLABS = 256;      // grid.x; further slabs are walked
constexpr int BWD_MAX_ROWS = 65535;     // grid.y; further rows are walked
constexpr float LOG2E = 1.44269504088896340736f, LN2 = 0.69314718055994530942f;

__device__ __forceinline__ int64_t load_label(const void *labels, int dt, int64_t r) {
    return dt == FA_XENT_LABELS_INT32 ? (int64_t) static_cast<const int32_t *>(labels)[r] : static_cast<const int64_t *>(labels)[r];
}

// the three pieces of a row of N elements at `row`: columns [0, head), nbody chunks of CW from column head, `tail` columns
// from column head + nbody * CW.  CW * esize(dt) is 16 (or CW is 1); the row is aligned to its element
struct Pieces {
    int head, nbody, tail;
};

template <int CW>
__device__ __forceinline__ Pieces pieces_of(const char *row, int dt, int N) {
    Pieces g;
    if constexpr (CW == 1) {
        g.head = 0; g.nbody = N; g.tail = 0;
    } else {
        const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 15);
        const int head = mis ? (16 - mis) / esize(dt) : 0;
        g.head = head < N ? head : N;
        g.nbody = (N - g.head) / CW;
        g.tail = N - g.head - g.nbody * CW;
    }
    return g;
}

// the column this thread takes of the head (the first lanes of wavefront 0) or the tail (of wavefront 1), or -1
__device__ __forceinline__ int edge_column(const Pieces &g, int cw, int t) {
    if (t < g.head) return t;
    if (t >= WAVE && t - WAVE < g.tail) return g.head + g.nbody * cw + (t - WAVE);
    return -1;
}

// exp2 of a finite-or-minus-infinity difference to a running maximum; a maximum of -inf (nothing but -inf so far) counts as 0
__device__ __forceinline__ float finite_max(float m) { return m == -INFINITY ? 0.0f : m; }

// NV raw logits into the thread's running (m, s, sum): m the maximum of x2 = raw * k2, s = sum(exp2(x2 - m)), sum = sum(raw)
template <int NV>
__device__ __forceinline__ void absorb(const float (&v)[NV], float k2, float &m, float &s, float &sum) {
    float vmax = v[0];
#pragma unroll
    for (int i = 1; i < NV; ++i) vmax = fmaxf(vmax, v[i]);
    const float m_new = fmaxf(m, vmax * k2), ref = finite_max(m_new);
    float acc = s * __builtin_amdgcn_exp2f(m - ref);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        acc += __builtin_amdgcn_exp2f(fmaf(v[i], k2, -ref));
        sum += v[i];
    }
    m = m_new;
    s = acc;
}

__device__ __forceinline__ void merge(float &m, float &s, float mo, float so) {
    const float m_new = fmaxf(m, mo), ref = finite_max(m_new);
    s = s * __builtin_amdgcn_exp2f(m - ref) + so * __builtin_amdgcn_exp2f(mo - ref);
    m = m_new;
}

// the loss of row r from its lse, sum_x = sum(x) and xl = x[lab] (include/fa_xent.h)
__device__ __forceinline__ void finish_row(const fa_xent_fwd_params &p, int64_t r, float lse, float sum_x, float xl, bool ignored,
                                           bool in_range) {
    const bool split = (p.flags & FA_XENT_SPLIT) != 0, smooth = p.smoothing > 0.0f;
    float loss = 0.0f, z_loss = 0.0f;
    if (!ignored) {
        const float base = split ? 0.0f : lse, mean_x = smooth ? sum_x / (float)p.total_classes : 0.0f;
        if (in_range) loss = base - p.smoothing * mean_x - (1.0f - p.smoothing) * xl;
        else loss = smooth ? p.smoothing * (base - mean_x) : 0.0f;
        if (!split) {
            z_loss = p.lse_square_scale * lse * lse;
            loss += z_loss;
        }
    }
    p.losses[r] = loss;
    if (!split) p.z_losses[r] = z_loss;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
template <int CW>
__global__ __launch_bounds__(THREADS) void xent_fwd_kernel(const fa_xent_fwd_params p) {
    __shared__ float red[2][3][WAVES];
    const int t = threadIdx.x, N = p.N, dt = p.logits_dtype;
    const float k2 = p.logit_scale * LOG2E;
    int phase = 0;  // the LDS slot, the two in turn: a slot is written again only after the barrier of the row between
    for (int64_t r = blockIdx.x; r < p.M; r += gridDim.x) {
        const char *row = static_cast<const char *>(p.logits) + r * p.logits_row_stride * esize(dt);
        const int64_t label = load_label(p.labels, p.labels_dtype, r), lab = label - p.class_start_idx;
        const bool ignored = label == p.ignore_index, in_range = lab >= 0 && lab < N;
        float xl = 0.0f;
        if (t == 0 && !ignored && in_range) xl = load_one(row, dt, lab) * p.logit_scale;
        const Pieces g = pieces_of<CW>(row, dt, N);
        float m = -INFINITY, s = 0.0f, sum = 0.0f;
        const int edge = edge_column(g, CW, t);
        if (edge >= 0) {
            const float v[1] = {load_one(row, dt, edge)};
            absorb<1>(v, k2, m, s, sum);
        }
        const char *body = row + g.head * esize(dt);  // 16-byte aligned where CW > 1
        const int cb = CW == 1 ? esize(dt) : 16;      // bytes of a chunk
        int c = t;
        for (; c + (FWD_UNROLL - 1) * THREADS < g.nbody; c += FWD_UNROLL * THREADS) {
            float v[FWD_UNROLL * CW];
#pragma unroll
            for (int u = 0; u < FWD_UNROLL; ++u) {
                float q[CW];
                load_chunk<CW>(body + (int64_t)(c + u * THREADS) * cb, dt, q);
#pragma unroll
                for (int i = 0; i < CW; ++i) v[u * CW + i] = q[i];
            }
            absorb<FWD_UNROLL * CW>(v, k2, m, s, sum);
        }
        for (; c < g.nbody; c += THREADS) {
            float q[CW];
            load_chunk<CW>(body + (int64_t)c * cb, dt, q);
            absorb<CW>(q, k2, m, s, sum);
        }
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            const float mo = __shfl_xor(m, o, WAVE), so = __shfl_xor(s, o, WAVE);
            sum += __shfl_xor(sum, o, WAVE);
            merge(m, s, mo, so);
        }
        if ((t & (WAVE - 1)) == 0) {
            red[phase][0][t >> 6] = m;
            red[phase][1][t >> 6] = s;
            red[phase][2][t >> 6] = sum;
        }
        __syncthreads();
        if (t == 0) {
            float mt = red[phase][0][0], st = red[phase][1][0], sumt = red[phase][2][0];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) {
                merge(mt, st, red[phase][0][w], red[phase][1][w]);
                sumt += red[phase][2][w];
            }
            const float lse = (mt + __log2f(st)) * LN2;
            p.lse[r] = lse;
            finish_row(p, r, lse, sumt * p.logit_scale, xl, ignored, in_range);
        }
        phase ^= 1;
    }
}

// FA_XENT_PRECOMPUTED_LSE: a thread per row; of the logits only the label's is read (logit_scale is 1, smoothing 0)
__global__ __launch_bounds__(THREADS) void xent_fwd_lse_given_kernel(const fa_xent_fwd_params p) {
    for (int64_t r = (int64_t)blockIdx.x * THREADS + threadIdx.x; r < p.M; r += (int64_t)gridDim.x * THREADS) {
        const int64_t label = load_label(p.labels, p.labels_dtype, r), lab = label - p.class_start_idx;
        const bool ignored = label == p.ignore_index, in_range = lab >= 0 && lab < p.N;
        float xl = 0.0f;
        if (!ignored && in_range)
            xl = load_one(static_cast<const char *>(p.logits) + r * p.logits_row_stride * esize(p.logits_dtype), p.logits_dtype, lab);
        finish_row(p, r, p.lse[r], 0.0f, xl, ignored, in_range);
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// what a row's elements share: dlogits = e * a - (b, or b_lab at the label's column), e = exp(x - lse)
struct RowGrad {
    float scale, lse, a, b, b_lab;
    __device__ __forceinline__ float at(float v, bool is_label) const {
        const float e = __builtin_amdgcn_exp2f(fmaf(v, scale, -lse) * LOG2E);
        return fmaf(e, a, -(is_label ? b_lab : b));
    }
};

template <int CW>
__global__ __launch_bounds__(THREADS) void xent_bwd_kernel(const fa_xent_bwd_params p) {
    const int t = threadIdx.x, N = p.N, dt = p.logits_dtype, es = esize(dt);
    const int cb = CW == 1 ? es : 16;  // bytes of a chunk
    const float off = p.smoothing / (float)p.total_classes, hit = 1.0f - p.smoothing;
    for (int64_t r = blockIdx.y; r < p.M; r += gridDim.y) {
        const char *row = static_cast<const char *>(p.logits) + r * p.logits_row_stride * es;
        char *out = static_cast<char *>(p.dlogits) + r * p.dlogits_row_stride * es;
        const int64_t label = load_label(p.labels, p.labels_dtype, r), lab64 = label - p.class_start_idx;
        const bool ignored = label == p.ignore_index;
        const int lab = lab64 >= 0 && lab64 < N ? (int)lab64 : -1;
        const Pieces g = pieces_of<CW>(row, dt, N);  // (the same for `out`: the host sends other phases to CW = 1)
        RowGrad w = {};
        if (!ignored) {
            const float lse = p.lse[r], d = p.dloss[r * p.dloss_stride] * p.logit_scale;
            w.scale = p.logit_scale;
            w.lse = lse;
            w.a = d * (1.0f + 2.0f * p.lse_square_scale * lse);
            w.b = d * off;
            w.b_lab = d * (off + hit);
        }
        const char *body = row + g.head * es;
        char *body_out = out + g.head * es;
        const int edge = blockIdx.x == 0 ? edge_column(g, CW, t) : -1;
        if (ignored) {  // zeros, and nothing of the row is read
            const float zero[CW] = {}, zero_1[1] = {};
            if (edge >= 0) store_chunk<1>(out + (int64_t)edge * es, dt, zero_1);
            for (int64_t c0 = (int64_t)blockIdx.x * BWD_SLAB; c0 < g.nbody; c0 += (int64_t)gridDim.x * BWD_SLAB) {  // (64 bits: CW = 1 has N chunks)
#pragma unroll
                for (int k = 0; k < BWD_CHUNKS; ++k) {
                    const int64_t c = c0 + k * THREADS + t;
                    if (c < g.nbody) store_chunk<CW>(body_out + c * cb, dt, zero);
                }
            }
            continue;
        }
        if (edge >= 0) {
            const float v[1] = {w.at(load_one(row, dt, edge), edge == lab)};
            store_chunk<1>(out + (int64_t)edge * es, dt, v);
        }
        for (int64_t c0 = (int64_t)blockIdx.x * BWD_SLAB; c0 < g.nbody; c0 += (int64_t)gridDim.x * BWD_SLAB) {  // (64 bits: CW = 1 has N chunks)
            float v[BWD_CHUNKS][CW];
#pragma unroll
            for (int k = 0; k < BWD_CHUNKS; ++k) {
                const int64_t c = c0 + k * THREADS + t;
                if (c < g.nbody) load_chunk<CW>(body + c * cb, dt, v[k]);
            }
#pragma unroll
            for (int k = 0; k < BWD_CHUNKS; ++k) {
                const int64_t c = c0 + k * THREADS + t;
                if (c < g.nbody) {
                    const int rel = lab - (g.head + (int)c * CW);  // the label's place in this chunk, if in [0, CW)
                    float y[CW];
#pragma unroll
                    for (int i = 0; i < CW; ++i) y[i] = w.at(v[k][i], i == rel);
                    store_chunk<CW>(body_out + c * cb, dt, y);
                }
            }
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
bool known_labels(int dt) { return dt == FA_XENT_LABELS_INT64 || dt == FA_XENT_LABELS_INT32; }

int check_numbers(int64_t M, int N, int64_t total_classes, float smoothing, float logit_scale) {
    if (M < 0 || N < 1 || total_classes < N) return FA_ERR_BAD_SHAPE;
    if (!(logit_scale > 0.0f) || !(smoothing >= 0.0f && smoothing <= 1.0f)) return FA_ERR_BAD_SHAPE;  // (NaN fails both)
    return FA_OK;
}

// the launch of a valid forward call
fa_xent_plan fwd_launch(const fa_xent_fwd_params *p) {
    fa_xent_plan l;
    l.lse_given = (p->flags & FA_XENT_PRECOMPUTED_LSE) != 0;
    l.grid_y = 1;
    if (l.lse_given) {  // a thread per row, one element of it
        const int64_t wgs = (p->M + THREADS - 1) / THREADS;
        l.cw = 1;
        l.grid_x = (int32_t)(wgs < LSE_GIVEN_MAX_GRID ? wgs : LSE_GIVEN_MAX_GRID);
    } else {
        l.cw = 16 / esize(p->logits_dtype);
        l.grid_x = (int32_t)(p->M < FWD_MAX_GRID ? p->M : FWD_MAX_GRID);
    }
    return l;
}

// ... of a valid backward call: 16-byte accesses where every row of logits has the phase of the same row of dlogits
fa_xent_plan bwd_launch(const fa_xent_bwd_params *p) {
    fa_xent_plan l;
    const int es = esize(p->logits_dtype), cw = 16 / es;
    const bool vec = (reinterpret_cast<uintptr_t>(p->logits) - reinterpret_cast<uintptr_t>(p->dlogits)) % 16 == 0 &&
                     (p->M == 1 || ((p->logits_row_stride - p->dlogits_row_stride) * es) % 16 == 0);
    const int64_t chunks = vec ? ((int64_t)p->N + cw - 1) / cw : p->N;  // (at least the body chunks of any row)
    const int64_t slabs = (chunks + BWD_SLAB - 1) / BWD_SLAB;
    l.lse_given = 0;
    l.cw = vec ? cw : 1;
    l.grid_x = (int32_t)(slabs < BWD_MAX_SLABS ? slabs : BWD_MAX_SLABS);
    l.grid_y = (int32_t)(p->M < BWD_MAX_ROWS ? p->M : BWD_MAX_ROWS);
    return l;
}

}  // namespace

extern "C" {

uint32_t fa_xent_fwd_params_size(void) { return (uint32_t)sizeof(fa_xent_fwd_params); }
uint32_t fa_xent_bwd_params_size(void) { return (uint32_t)sizeof(fa_xent_bwd_params); }

int fa_xent_fwd_validate(const fa_xent_fwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_xent_fwd_params)) return FA_ERR_BAD_ABI;
    if (!known_dtype(p->logits_dtype) || !known_labels(p->labels_dtype)) return FA_ERR_BAD_DTYPE;
    const int st = check_numbers(p->M, p->N, p->total_classes, p->smoothing, p->logit_scale);
    if (st != FA_OK) return st;
    if ((p->flags & FA_XENT_PRECOMPUTED_LSE) && (p->smoothing != 0.0f || p->logit_scale != 1.0f)) return FA_ERR_BAD_SHAPE;
    if (!p->logits || !p->labels || !p->losses || !p->lse || (!(p->flags & FA_XENT_SPLIT) && !p->z_losses)) return FA_ERR_NULL_POINTER;
    if (!aligned_to(p->logits, esize(p->logits_dtype)) || !aligned_to(p->labels, p->labels_dtype == FA_XENT_LABELS_INT32 ? 4 : 8) ||
        !aligned_to(p->losses, 4) || !aligned_to(p->lse, 4) || !aligned_to(p->z_losses, 4))
        return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int fa_xent_fwd(const fa_xent_fwd_params *p, void *stream_) {
    const int st = fa_xent_fwd_validate(p);
    if (st != FA_OK) return st;
    if (p->M == 0) return FA_OK;  // (no zero grid)
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const fa_xent_plan l = fwd_launch(p);
    const dim3 grid(l.grid_x, l.grid_y);
    if (l.lse_given) hipLaunchKernelGGL(xent_fwd_lse_given_kernel, grid, dim3(THREADS), 0, stream, *p);
    else if (l.cw == 4) hipLaunchKernelGGL((xent_fwd_kernel<4>), grid, dim3(THREADS), 0, stream, *p);
    else hipLaunchKernelGGL((xent_fwd_kernel<8>), grid, dim3(THREADS), 0, stream, *p);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

int fa_xent_fwd_plan(const fa_xent_fwd_params *p, fa_xent_plan *plan) {
    const int st = fa_xent_fwd_validate(p);
    if (st != FA_OK) return st;
    if (!plan) return FA_ERR_NULL_POINTER;
    *plan = fwd_launch(p);
    return FA_OK;
}

int fa_xent_bwd_validate(const fa_xent_bwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_xent_bwd_params)) return FA_ERR_BAD_ABI;
    if (!known_dtype(p->logits_dtype) || !known_labels(p->labels_dtype)) return FA_ERR_BAD_DTYPE;
    const int st = check_numbers(p->M, p->N, p->total_classes, p->smoothing, p->logit_scale);
    if (st != FA_OK) return st;
    if (!p->logits || !p->labels || !p->lse || !p->dloss || !p->dlogits) return FA_ERR_NULL_POINTER;
    if (!aligned_to(p->logits, esize(p->logits_dtype)) || !aligned_to(p->dlogits, esize(p->logits_dtype)) ||
        !aligned_to(p->labels, p->labels_dtype == FA_XENT_LABELS_INT32 ? 4 : 8) || !aligned_to(p->lse, 4) || !aligned_to(p->dloss, 4))
        return FA_ERR_BAD_STRIDE;
    if (p->M > 1 && p->dlogits_row_stride < p->N) return FA_ERR_BAD_STRIDE;  // (rows that are written do not overlap)
    return FA_OK;
}

int fa_xent_bwd_plan(const fa_xent_bwd_params *p, fa_xent_plan *plan) {
    const int st = fa_xent_bwd_validate(p);
    if (st != FA_OK) return st;
    if (!plan) return FA_ERR_NULL_POINTER;
    *plan = bwd_launch(p);
    return FA_OK;
}

int fa_xent_bwd(const fa_xent_bwd_params *p, void *stream_) {
    const int st = fa_xent_bwd_validate(p);
    if (st != FA_OK) return st;
    if (p->M == 0) return FA_OK;
    const fa_xent_plan l = bwd_launch(p);
    const dim3 grid(l.grid_x, l.grid_y);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (l.cw == 1) hipLaunchKernelGGL((xent_bwd_kernel<1>), grid, dim3(THREADS), 0, stream, *p);
    else if (l.cw == 4) hipLaunchKernelGGL((xent_bwd_kernel<4>), grid, dim3(THREADS), 0, stream, *p);
    else hipLaunchKernelGGL((xent_bwd_kernel<8>), grid, dim3(THREADS), 0, stream, *p);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

}  // extern "C"
