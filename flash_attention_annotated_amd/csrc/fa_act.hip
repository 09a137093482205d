// fa_act.hip — fa_act_fwd / fa_act_bwd (include/fa_act.h): the activation between the two GEMMs of an MLP, plain
// (act(pre + bias)) and gated (act(gate) * up), forward and backward.  A translation unit of its own with nothing from the
// other units (the chunk loads and stores restate those of fa_xent.hip): the kernel sets of the other units are pinned.
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

#include <hip/hip_runtime.h>

#include <cmath>

namespace {

constexpr int THREADS = 256;
constexpr int FWD_ROWS = 4;          // rows of a forward block, all in flight
constexpr int BWD_ROWS = 32;         // rows of a backward block: M / 32 partial rows of dbias
constexpr int BWD_UNROLL = 2;        // ... of which in flight
constexpr int MAX_SLABS = 256;       // grid.x; further slabs are walked
constexpr int FWD_MAX_BLOCKS = 65535;  // grid.y of the forward; further row blocks are walked
constexpr int BWD_MAX_BLOCKS = 1024;   // ... of the backward: at most 1024 partial rows

__host__ __device__ __forceinline__ int esize(int dt) { return dt == FA_DTYPE_FP32 ? 4 : 2; }

// CW elements of dtype `dt` at q, as fp32: 16-byte accesses where CW > 1
template <int CW>
__device__ __forceinline__ void load_chunk(const char *q, int dt, float (&v)[CW]) {
    if (dt == FA_DTYPE_FP32) {
        const float *p = reinterpret_cast<const float *>(q);
        if constexpr (CW == 1) {
            v[0] = *p;
        } else {
#pragma unroll
            for (int i = 0; i < CW; i += 4) {
                const float4 f = *reinterpret_cast<const float4 *>(p + i);
                v[i] = f.x; v[i + 1] = f.y; v[i + 2] = f.z; v[i + 3] = f.w;
            }
        }
        return;
    }
    uint32_t h[CW];
    if constexpr (CW == 8) {
        const uint4 f = *reinterpret_cast<const uint4 *>(q);
        h[0] = f.x & 0xffffu; h[1] = f.x >> 16; h[2] = f.y & 0xffffu; h[3] = f.y >> 16;
        h[4] = f.z & 0xffffu; h[5] = f.z >> 16; h[6] = f.w & 0xffffu; h[7] = f.w >> 16;
    } else if constexpr (CW == 4) {
        const uint2 f = *reinterpret_cast<const uint2 *>(q);
        h[0] = f.x & 0xffffu; h[1] = f.x >> 16; h[2] = f.y & 0xffffu; h[3] = f.y >> 16;
    } else {
        h[0] = *reinterpret_cast<const uint16_t *>(q);
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
__device__ __forceinline__ void store_chunk(char *q, int dt, const float (&v)[CW]) {
    if (dt == FA_DTYPE_FP32) {
        float *p = reinterpret_cast<float *>(q);
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
    if constexpr (CW == 8) {
        *reinterpret_cast<uint4 *>(q) = make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
    } else if constexpr (CW == 4) {
        *reinterpret_cast<uint2 *>(q) = make_uint2(h[0] | h[1] << 16, h[2] | h[3] << 16);
    } else {
        *reinterpret_cast<uint16_t *>(q) = (uint16_t)h[0];
    }
}

// ---- the activations ----------------------------------------------------------------------------------------------------------
// a = act(x) and dg = act'(x) * g for a downstream factor g (include/fa_act.h).  One definition for the forward and the backward, with contraction off: the backward's
// recomputed output has the forward's bits.
struct Sig {
    float s, c;  // sigmoid(z) and 1 - sigmoid(z), neither by a subtraction
};

__device__ __forceinline__ Sig sigmoid_parts(float z) {
#pragma clang fp contract(off)
    const float e = expf(-fabsf(z));  // in [0, 1]: never overflows, 0 at saturation
    const float hi = 1.0f / (1.0f + e), lo = e * hi;
    Sig g;
    g.s = z >= 0.0f ? hi : lo;
    g.c = z >= 0.0f ? lo : hi;
    return g;
}

template <int ACT>
__device__ __forceinline__ void eval(float x, float g, float &a, float &dg) {
#pragma clang fp contract(off)
    float da;
    if constexpr (ACT == FA_ACT_GELU_TANH) {
        const float x2 = x * x;  // inf once |x| > 1.8e19: z is then +-inf, s (1 - s) is 0 and the second term is dropped
        const Sig g = sigmoid_parts((1.59576912f * x) * (1.0f + 0.044715f * x2));
        const float w = g.s * g.c;
        a = x * g.s;
        da = g.s + (w > 0.0f ? (x * w) * (1.59576912f + 0.2140644486f * x2) : 0.0f);
    } else if constexpr (ACT == FA_ACT_GELU_ERF) {
        const float y = x * 0.70710678118654752f;
        const float phi = x >= 0.0f ? 0.5f * (1.0f + erff(y)) : 0.5f * erfcf(-y);
        a = x * phi;
        da = phi + x * (0.39894228040143268f * expf(-0.5f * (x * x)));  // (x^2 = inf: exp is 0 and x is finite)
    } else if constexpr (ACT == FA_ACT_RELU) {
        a = x > 0.0f ? x : (x == x ? 0.0f : x);  // (NaN stays NaN)
        da = x > 0.0f ? 1.0f : 0.0f;
    } else if constexpr (ACT == FA_ACT_SQRELU) {
        const float r = x > 0.0f ? x : (x == x ? 0.0f : x);
        a = r * r;
        dg = (r * g) * 2.0f;  // (2 r alone overflows for r above half the largest value, where the product with g may not)
        return;
    } else if constexpr (ACT == FA_ACT_SILU) {
        const Sig g = sigmoid_parts(x);
        a = x * g.s;
        da = g.s + x * (g.s * g.c);
    } else if constexpr (ACT == FA_ACT_SIGMOID) {
        const Sig g = sigmoid_parts(x);
        a = g.s;
        da = g.s * g.c;
    } else {
        a = x;
        da = 1.0f;
    }
    dg = da * g;
}

template <int NC>
__device__ __forceinline__ void eval_chunk(int act, const float (&x)[NC], const float (&g)[NC], float (&a)[NC], float (&dg)[NC]) {
#define FA_ACT_CASE(A)                                        \
    case A:                                                   \
        _Pragma("unroll") for (int i = 0; i < NC; ++i) eval<A>(x[i], g[i], a[i], dg[i]); \
        break;
    switch (act) {
        FA_ACT_CASE(FA_ACT_GELU_TANH)
        FA_ACT_CASE(FA_ACT_GELU_ERF)
        FA_ACT_CASE(FA_ACT_RELU)
        FA_ACT_CASE(FA_ACT_SQRELU)
        FA_ACT_CASE(FA_ACT_SILU)
        FA_ACT_CASE(FA_ACT_SIGMOID)
    default:
        _Pragma("unroll") for (int i = 0; i < NC; ++i) eval<FA_ACT_IDENTITY>(x[i], g[i], a[i], dg[i]);
    }
#undef FA_ACT_CASE
}

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
bool known_dtype(int dt) { return dt == FA_DTYPE_FP16 || dt == FA_DTYPE_BF16 || dt == FA_DTYPE_FP32; }
bool known_activation(int a) { return a >= FA_ACT_GELU_TANH && a <= FA_ACT_IDENTITY; }
bool aligned_to(const void *q, int bytes) { return reinterpret_cast<uintptr_t>(q) % bytes == 0; }

// a tensor of rows: 16-byte accesses need its base and (more than one row) its pitch in bytes to be multiples of 16
bool rows_allow_16(const void *q, int64_t row_stride, int es, int64_t M) { return !q || (aligned_to(q, 16) && (M <= 1 || (row_stride * es) % 16 == 0)); }

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
    const int es = esize(p->pre_dtype);
    const void *up = (p->flags & FA_ACT_GATED) ? p->up : nullptr;  // (the plain form ignores the field, whatever it holds)
    const bool vec = rows_allow_16(p->pre, p->pre_row_stride, es, p->M) && rows_allow_16(up, p->pre_row_stride, es, p->M) &&
                     rows_allow_16(p->out, p->out_row_stride, es, p->M) && aligned_to(p->bias, 16);
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
    const int es = esize(p->pre_dtype);
    const bool gated = (p->flags & FA_ACT_GATED) != 0;  // (the plain form ignores up and dup, whatever the fields hold)
    const void *up = gated ? p->up : nullptr, *dup = gated ? p->dup : nullptr;
    const bool vec = rows_allow_16(p->pre, p->pre_row_stride, es, p->M) && rows_allow_16(up, p->pre_row_stride, es, p->M) &&
                     rows_allow_16(p->dout, p->dout_row_stride, es, p->M) && rows_allow_16(p->dpre, p->dpre_row_stride, es, p->M) &&
                     rows_allow_16(dup, p->dpre_row_stride, es, p->M) && rows_allow_16(p->recompute_out, p->out_row_stride, es, p->M) &&
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
