// fa_act.hip — fa_act_fwd / fa_act_bwd (include/fa_act.h): the activation between the two GEMMs of an MLP, plain
// (act(pre + bias)) and gated (act(gate) * up), forward and backward.  A translation unit of its own: no kernel comes from
// another unit or goes to one, because the kernel set of every unit is pinned by its tests.  That rule is about kernels.  The
// chunk loads and stores and the host predicates are the inline functions of fa_rowwise.h, shared with the other row units,
// and the activations are those of fa_act_math.h, the one definition this unit and fa_gemm_act.hip have.
//
// A pure stream.  A row is H / CW chunks of 16 bytes (CW = 8 elements of a 16-bit dtype, 4 of fp32) and an element tail of
// H % CW columns, where every tensor of the call is 16-byte aligned in every row; otherwise every column is an element
// (CW = 1).  A workgroup of 256 threads owns a slab of 256 chunks (blockIdx.x; further slabs are walked) times blocks of
// rows (blockIdx.y; further blocks are walked): thread t owns chunk slab * 256 + t of every row of its blocks, so neighbouring
// lanes touch neighbouring 16 bytes, and the bias chunk and the dbias sums of its columns stay in its registers.  The tail
// columns go to the first lanes of the workgroups of slab 0.  Forward: FWD_ROWS rows in flight per thread.  Backward:
// BWD_ROWS rows per block, BWD_UNROLL in flight; with dbias a thread adds the unrounded dpre of all its rows in fp32 and
// writes its columns of partial row blockIdx.y; act_dbias_reduce_kernel adds the gridDim.y partial rows in their order.
// Dtype, activation, gating, bias, dbias and recompute are kernel arguments, hence wave-uniform: the kernels are
// instantiated by CW only.  No atomics, no LDS.
#include "../../include/fa_act.h"
#include "fa_act_math.h"
#include "fa_rowwise.h"

namespace {

using namespace fa_row;
using namespace fa_act_math;

constexpr int THREADS = 256;
constexpr int FWD_ROWS = 4;          // rows of a forward block, all in flight
constexpr int BWD_ROWS = 32;         // rows of a backward block: M / 32 partial rows of dbias
constexpr int BWD_UNROLL = 2;        // ... of which in flight
constexpr int MAX_SLABS = 256;       // grid.x; further slabs are walked
constexpr int FWD_MAX_BLOCKS = 65535;  // grid.y of the forward; further row blocks are walked
constexpr int BWD_MAX_BLOCKS = 1024;   // ... of the backward: at most 1024 partial rows

// the forward's value of one element: the one rounding follows in store_chunk
__device__ __forceinline__ float out_of(float a, float u, bool gated) {
#pragma clang fp contract(off)
    return gated ? a * u : a;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
// columns [col, col + NC) of every row of this workgroup's row blocks
template <int NC>
__device__ __forceinline__ void fwd_columns(const fa_act_fwd_params &p, int64_t col) {
    const int dt = p.pre_dtype, es = esize(dt);
    const bool gated = (p.flags & FA_ACT_GATED) != 0;
    float b[NC] = {};
    if (p.bias) load_chunk<NC>(static_cast<const char *>(p.bias) + col * esize(p.bias_dtype), p.bias_dtype, b);
    const char *pre = static_cast<const char *>(p.pre) + col * es, *up = static_cast<const char *>(p.up) + col * es;
    char *out = static_cast<char *>(p.out) + col * es;
    const int64_t nblocks = (p.M + FWD_ROWS - 1) / FWD_ROWS;
    for (int64_t rb = blockIdx.y; rb < nblocks; rb += gridDim.y) {
        const int64_t r0 = rb * FWD_ROWS;
        float x[FWD_ROWS][NC], u[FWD_ROWS][NC];
#pragma unroll
        for (int k = 0; k < FWD_ROWS; ++k) {
            if (r0 + k < p.M) {
                load_chunk<NC>(pre + (r0 + k) * p.pre_row_stride * es, dt, x[k]);
                if (gated) load_chunk<NC>(up + (r0 + k) * p.pre_row_stride * es, dt, u[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < FWD_ROWS; ++k) {
            if (r0 + k < p.M) {
                float a[NC], dg[NC], y[NC];
#pragma unroll
                for (int i = 0; i < NC; ++i) x[k][i] += b[i];
                eval_chunk<NC>(p.activation, x[k], b, a, dg);  // (dg is not used: its arithmetic is dropped)
#pragma unroll
                for (int i = 0; i < NC; ++i) y[i] = out_of(a[i], gated ? u[k][i] : 0.0f, gated);
                store_chunk<NC>(out + (r0 + k) * p.out_row_stride * es, dt, y);
            }
        }
    }
}

template <int CW>
__global__ __launch_bounds__(THREADS) void act_fwd_kernel(const fa_act_fwd_params p) {
    const int64_t nbody = p.H / CW;  // (64 bits: CW = 1 has H chunks, and the walk's step is added to it)
    for (int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x; c < nbody; c += (int64_t)gridDim.x * THREADS) fwd_columns<CW>(p, c * CW);
    if constexpr (CW > 1) {
        const int tail = p.H - (int)nbody * CW;
        if (blockIdx.x == 0 && (int)threadIdx.x < tail) fwd_columns<1>(p, nbody * CW + threadIdx.x);
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// the pitch of a partial row of dbias in the workspace, in floats: chunks of partial rows are 16-byte aligned
__host__ __device__ __forceinline__ int64_t partial_pitch(int H) { return ((int64_t)H + 3) / 4 * 4; }

template <int NC>
__device__ __forceinline__ void bwd_columns(const fa_act_bwd_params &p, int64_t col) {
    const int dt = p.pre_dtype, es = esize(dt);
    const bool gated = (p.flags & FA_ACT_GATED) != 0;
    float b[NC] = {}, acc[NC] = {};
    if (p.bias) load_chunk<NC>(static_cast<const char *>(p.bias) + col * esize(p.bias_dtype), p.bias_dtype, b);
    const char *pre = static_cast<const char *>(p.pre) + col * es, *up = static_cast<const char *>(p.up) + col * es;
    const char *dout = static_cast<const char *>(p.dout) + col * es;
    char *dpre = static_cast<char *>(p.dpre) + col * es, *dup = static_cast<char *>(p.dup) + col * es;
    char *out = static_cast<char *>(p.recompute_out) + col * es;
    const int64_t nblocks = (p.M + BWD_ROWS - 1) / BWD_ROWS;
    for (int64_t rb = blockIdx.y; rb < nblocks; rb += gridDim.y) {
        const int64_t r0 = rb * BWD_ROWS;
        for (int k0 = 0; k0 < BWD_ROWS && r0 + k0 < p.M; k0 += BWD_UNROLL) {
            float x[BWD_UNROLL][NC], u[BWD_UNROLL][NC], g[BWD_UNROLL][NC];
#pragma unroll
            for (int k = 0; k < BWD_UNROLL; ++k) {
                const int64_t r = r0 + k0 + k;
                if (r < p.M) {
                    load_chunk<NC>(pre + r * p.pre_row_stride * es, dt, x[k]);
                    load_chunk<NC>(dout + r * p.dout_row_stride * es, dt, g[k]);
                    if (gated) load_chunk<NC>(up + r * p.pre_row_stride * es, dt, u[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < BWD_UNROLL; ++k) {
                const int64_t r = r0 + k0 + k;
                if (r < p.M) {
                    float a[NC], dg[NC], y[NC];
#pragma unroll
                    for (int i = 0; i < NC; ++i) x[k][i] += b[i];
                    eval_chunk<NC>(p.activation, x[k], gated ? u[k] : g[k], a, dg);  // (act' * up, or act' * dout)
                    if (gated) {
#pragma unroll
                        for (int i = 0; i < NC; ++i) y[i] = dg[i] * g[k][i];  // (act' * up first: up * dout may overflow where act' is 0)
                        store_chunk<NC>(dpre + r * p.dpre_row_stride * es, dt, y);
#pragma unroll
                        for (int i = 0; i < NC; ++i) y[i] = a[i] * g[k][i];
                        store_chunk<NC>(dup + r * p.dpre_row_stride * es, dt, y);
                    } else {
#pragma unroll
                        for (int i = 0; i < NC; ++i) {
                            y[i] = dg[i];
                            acc[i] += y[i];
                        }
                        store_chunk<NC>(dpre + r * p.dpre_row_stride * es, dt, y);
                    }
                    if (p.recompute_out) {
#pragma unroll
                        for (int i = 0; i < NC; ++i) y[i] = out_of(a[i], gated ? u[k][i] : 0.0f, gated);
                        store_chunk<NC>(out + r * p.out_row_stride * es, dt, y);
                    }
                }
            }
        }
    }
    if (p.dbias)  // partial row blockIdx.y: every workgroup has at least one row block, and every column one thread
        store_chunk<NC>(reinterpret_cast<char *>(static_cast<float *>(p.workspace) + (int64_t)blockIdx.y * partial_pitch(p.H) + col),
                        FA_DTYPE_FP32, acc);
}

template <int CW>
__global__ __launch_bounds__(THREADS) void act_bwd_kernel(const fa_act_bwd_params p) {
    const int64_t nbody = p.H / CW;
    for (int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x; c < nbody; c += (int64_t)gridDim.x * THREADS) bwd_columns<CW>(p, c * CW);
    if constexpr (CW > 1) {
        const int tail = p.H - (int)nbody * CW;
        if (blockIdx.x == 0 && (int)threadIdx.x < tail) bwd_columns<1>(p, nbody * CW + threadIdx.x);
    }
}

// dbias[c] = the sum of the P partial rows at column c, in their order, cast once
__global__ __launch_bounds__(THREADS) void act_dbias_reduce_kernel(const float *partials, int P, int H, void *dbias, int dt) {
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x, pitch = partial_pitch(H);
    if (c >= H) return;
    float sum = 0.0f;
    for (int j = 0; j < P; ++j) sum += partials[j * pitch + c];
    const float v[1] = {sum};
    store_chunk<1>(static_cast<char *>(dbias) + c * esize(dt), dt, v);
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// a tensor of rows: 16-byte accesses need its base and (more than one row) its pitch in bytes to be multiples of 16
bool rows_allow_16(const void *q, int dt, int64_t row_stride, int64_t M) { return M <= 1 ? aligned_to(q, 16) : rows_16_bytes(q, dt, row_stride); }

int32_t slabs_of(int H, int cw) {
    const int64_t chunks = (int64_t)H / cw, slabs = (chunks + THREADS - 1) / THREADS;
    return (int32_t)(slabs < 1 ? 1 : slabs < MAX_SLABS ? slabs : MAX_SLABS);  // (H < cw: the tail alone, by slab 0)
}

int32_t blocks_of(int64_t M, int rows, int cap) {
    const int64_t blocks = (M + rows - 1) / rows;
    return (int32_t)(blocks < cap ? blocks : cap);
}

// the launch of a valid forward call
fa_act_plan fwd_launch(const fa_act_fwd_params *p) {
    const int dt = p->pre_dtype, es = esize(dt);
    const void *up = (p->flags & FA_ACT_GATED) ? p->up : nullptr;  // (the plain form ignores the field, whatever it holds)
    const bool vec = rows_allow_16(p->pre, dt, p->pre_row_stride, p->M) && rows_allow_16(up, dt, p->pre_row_stride, p->M) &&
                     rows_allow_16(p->out, dt, p->out_row_stride, p->M) && aligned_to(p->bias, 16);
    fa_act_plan l;
    l.cw = vec ? 16 / es : 1;
    l.threads = THREADS;
    l.rows_per_wg = FWD_ROWS;
    l.grid_x = slabs_of(p->H, l.cw);
    l.grid_y = blocks_of(p->M, FWD_ROWS, FWD_MAX_BLOCKS);
    return l;
}

// ... of a valid backward call (the workspace is 16-byte aligned by validation, and its partial rows by their pitch)
fa_act_plan bwd_launch(const fa_act_bwd_params *p) {
    const int dt = p->pre_dtype, es = esize(dt);
    const bool gated = (p->flags & FA_ACT_GATED) != 0;  // (the plain form ignores up and dup, whatever the fields hold)
    const void *up = gated ? p->up : nullptr, *dup = gated ? p->dup : nullptr;
    const bool vec = rows_allow_16(p->pre, dt, p->pre_row_stride, p->M) && rows_allow_16(up, dt, p->pre_row_stride, p->M) &&
                     rows_allow_16(p->dout, dt, p->dout_row_stride, p->M) && rows_allow_16(p->dpre, dt, p->dpre_row_stride, p->M) &&
                     rows_allow_16(dup, dt, p->dpre_row_stride, p->M) && rows_allow_16(p->recompute_out, dt, p->out_row_stride, p->M) &&
                     aligned_to(p->bias, 16);
    fa_act_plan l;
    l.cw = vec ? 16 / es : 1;
    l.threads = THREADS;
    l.rows_per_wg = BWD_ROWS;
    l.grid_x = slabs_of(p->H, l.cw);
    l.grid_y = blocks_of(p->M, BWD_ROWS, BWD_MAX_BLOCKS);
    return l;
}

// what both directions ask of the numbers and of the input side
int check_common(int64_t M, int H, int activation, int flags, int pre_dtype, int up_dtype, int bias_dtype, const void *pre, const void *up,
                 const void *bias, int64_t pre_row_stride) {
    const bool gated = (flags & FA_ACT_GATED) != 0;
    if (!known_dtype(pre_dtype) || (gated && up_dtype != pre_dtype)) return FA_ERR_BAD_DTYPE;
    if (bias && bias_dtype != pre_dtype && bias_dtype != FA_DTYPE_FP32) return FA_ERR_BAD_DTYPE;
    if (!known_activation(activation)) return FA_ERR_UNSUPPORTED;
    if (M < 0 || H < 1 || (flags & ~FA_ACT_GATED)) return FA_ERR_BAD_SHAPE;
    if (gated && bias) return FA_ERR_BAD_SHAPE;
    if (!pre || (gated && !up)) return FA_ERR_NULL_POINTER;
    const int es = esize(pre_dtype);
    if (!aligned_to(pre, es) || (gated && !aligned_to(up, es)) || (bias && !aligned_to(bias, esize(bias_dtype)))) return FA_ERR_BAD_STRIDE;
    if (M > 1 && pre_row_stride < H) return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

}  // namespace

extern "C" {

uint32_t fa_act_fwd_params_size(void) { return (uint32_t)sizeof(fa_act_fwd_params); }
uint32_t fa_act_bwd_params_size(void) { return (uint32_t)sizeof(fa_act_bwd_params); }

int fa_act_fwd_validate(const fa_act_fwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_act_fwd_params)) return FA_ERR_BAD_ABI;
    const int st = check_common(p->M, p->H, p->activation, p->flags, p->pre_dtype, p->up_dtype, p->bias_dtype, p->pre, p->up, p->bias,
                                p->pre_row_stride);
    if (st != FA_OK) return st;
    if (p->out_dtype != p->pre_dtype) return FA_ERR_BAD_DTYPE;
    if (!p->out) return FA_ERR_NULL_POINTER;
    if (!aligned_to(p->out, esize(p->out_dtype)) || (p->M > 1 && p->out_row_stride < p->H)) return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int fa_act_fwd_plan(const fa_act_fwd_params *p, fa_act_plan *plan) {
    const int st = fa_act_fwd_validate(p);
    if (st != FA_OK) return st;
    if (!plan) return FA_ERR_NULL_POINTER;
    *plan = fwd_launch(p);
    return FA_OK;
}

int fa_act_fwd(const fa_act_fwd_params *p_, void *stream_) {
    const int st = fa_act_fwd_validate(p_);
    if (st != FA_OK) return st;
    if (p_->M == 0) return FA_OK;  // (no zero grid)
    fa_act_fwd_params p = *p_;
    if (!(p.flags & FA_ACT_GATED)) p.up = nullptr;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const fa_act_plan l = fwd_launch(&p);
    const dim3 grid(l.grid_x, l.grid_y);
    if (l.cw == 1) hipLaunchKernelGGL((act_fwd_kernel<1>), grid, dim3(THREADS), 0, stream, p);
    else if (l.cw == 4) hipLaunchKernelGGL((act_fwd_kernel<4>), grid, dim3(THREADS), 0, stream, p);
    else hipLaunchKernelGGL((act_fwd_kernel<8>), grid, dim3(THREADS), 0, stream, p);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

uint64_t fa_act_bwd_workspace_bytes(const fa_act_bwd_params *p) {
    if (!p || !p->dbias || p->M < 1 || p->H < 1) return 0;
    return (uint64_t)blocks_of(p->M, BWD_ROWS, BWD_MAX_BLOCKS) * (uint64_t)partial_pitch(p->H) * sizeof(float);
}

int fa_act_bwd_validate(const fa_act_bwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_act_bwd_params)) return FA_ERR_BAD_ABI;
    const int st = check_common(p->M, p->H, p->activation, p->flags, p->pre_dtype, p->up_dtype, p->bias_dtype, p->pre, p->up, p->bias,
                                p->pre_row_stride);
    if (st != FA_OK) return st;
    const bool gated = (p->flags & FA_ACT_GATED) != 0;
    const int dt = p->pre_dtype, es = esize(dt);
    if (p->dout_dtype != dt || p->dpre_dtype != dt || (gated && p->dup_dtype != dt) || (p->recompute_out && p->out_dtype != dt)) return FA_ERR_BAD_DTYPE;
    if (p->dbias && p->dbias_dtype != dt && p->dbias_dtype != FA_DTYPE_FP32) return FA_ERR_BAD_DTYPE;
    if (gated && p->dbias) return FA_ERR_BAD_SHAPE;
    if (!p->dout || !p->dpre || (gated && !p->dup)) return FA_ERR_NULL_POINTER;
    if (!aligned_to(p->dout, es) || !aligned_to(p->dpre, es) || (gated && !aligned_to(p->dup, es)) || !aligned_to(p->recompute_out, es) ||
        (p->dbias && !aligned_to(p->dbias, esize(p->dbias_dtype))))
        return FA_ERR_BAD_STRIDE;
    if (p->M > 1 && (p->dout_row_stride < p->H || p->dpre_row_stride < p->H || (p->recompute_out && p->out_row_stride < p->H))) return FA_ERR_BAD_STRIDE;
    const uint64_t need = fa_act_bwd_workspace_bytes(p);
    if (need > 0 && (!p->workspace || p->workspace_bytes < need)) return FA_ERR_WORKSPACE;
    if (need > 0 && !aligned_to(p->workspace, 16)) return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int fa_act_bwd_plan(const fa_act_bwd_params *p, fa_act_plan *plan) {
    const int st = fa_act_bwd_validate(p);
    if (st != FA_OK) return st;
    if (!plan) return FA_ERR_NULL_POINTER;
    *plan = bwd_launch(p);
    return FA_OK;
}

int fa_act_bwd(const fa_act_bwd_params *p_, void *stream_) {
    const int st = fa_act_bwd_validate(p_);
    if (st != FA_OK) return st;
    if (p_->M == 0) return FA_OK;
    fa_act_bwd_params p = *p_;
    if (!(p.flags & FA_ACT_GATED)) p.up = p.dup = nullptr;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const fa_act_plan l = bwd_launch(&p);
    const dim3 grid(l.grid_x, l.grid_y);
    if (l.cw == 1) hipLaunchKernelGGL((act_bwd_kernel<1>), grid, dim3(THREADS), 0, stream, p);
    else if (l.cw == 4) hipLaunchKernelGGL((act_bwd_kernel<4>), grid, dim3(THREADS), 0, stream, p);
    else hipLaunchKernelGGL((act_bwd_kernel<8>), grid, dim3(THREADS), 0, stream, p);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    if (p.dbias) {
        hipLaunchKernelGGL(act_dbias_reduce_kernel, dim3((uint32_t)(((int64_t)p.H + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream,
                           static_cast<const float *>(p.workspace), l.grid_y, p.H, p.dbias, p.dbias_dtype);
        if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    }
    return FA_OK;
}

}  // extern "C"
