// fa_norm.hip — fa_norm_fwd / fa_norm_bwd (include/fa_norm.h): fused residual-add + LayerNorm / RMSNorm, forward and backward.
// A translation unit of its own: no kernel comes from another unit or goes to one, because the kernel set of every unit is
// pinned by its tests.  That rule is about kernels: the chunk loads and stores, the wavefront and team sums, the ordered
// reduce of partial rows and the host predicates are the inline functions of fa_rowwise.h, shared with the other row units.
//
// A row is the work of a *team*: one wavefront where a lane has at most C columns (four teams, so four rows at a time, in a
// workgroup of 256), else the whole workgroup of 256 / 512 / 1024 threads (the smallest that gives a thread at most C columns);
// C = 16 in the forward and 8 in the backward, which keeps five values per column.  Thread t of a team of `ts` threads owns the
// chunks (k * ts + t) of CW columns, k < K = C / CW: neighbouring lanes read neighbouring 16 bytes.  A workgroup takes a
// contiguous block of rows, so what does not depend on the row -- the weight and the bias, in fp32 registers -- is read once per
// workgroup.  The dtype of every tensor is a kernel argument, hence wave-uniform: loads and stores branch on it in the scalar
// unit, and the kernels are instantiated by access shape only:
//   CW = 8   16-byte accesses of a 16-bit x (two of them per chunk of an fp32 tensor beside it)
//   CW = 4   16-byte accesses of an fp32 x (8 bytes of a 16-bit tensor beside it)
//   CW = 1   element accesses: any N >= 1, any alignment
// Forward: the row is read once and stays in fp32 registers between the statistics and the normalise step.  Sums are taken
// inside a wavefront by a butterfly of cross-lane swaps over all 64 lanes, and between the wavefronts of a workgroup through
// 16 floats of LDS per sum (two slots in turn: one barrier per sum).
// Backward: xhat and w * dy stay in registers between the two row sums and dx, dw / db columns are summed in registers over the
// workgroup's rows and written as one fp32 partial row per workgroup; norm_reduce_kernel adds the partial rows in a fixed
// order.  No atomics anywhere.
// Rows wider than 1024 * C do not fit the registers of 1024 threads (128 each) and have forms of their own, which never spill:
// the forward walks such a row three times (norm_fwd_wide_kernel), the backward takes the row sums in a launch of their own
// (norm_bwd_row_sums_kernel) and then splits the columns into slabs of 1024 * C over blockIdx.y of the same norm_bwd_kernel.
#include "../../include/fa_norm.h"
#include "fa_rowwise.h"

namespace {

using namespace fa_row;

constexpr int WAVE_TEAMS = 4;         // wavefronts (rows in flight) of a workgroup of wavefront teams
constexpr int FWD_COLS = 16;          // columns per thread of the forward forms that keep weight and bias in registers
constexpr int BWD_COLS = 8;           // ... of the backward forms that keep xhat, w * dy and the weight in registers
constexpr int BWD_WAVE_ROW_N = WAVE * BWD_COLS;  // the widest row a single wavefront takes in the backward
constexpr int BWD_PARTIALS = 1024;    // the backward aims at this many workgroups ...
constexpr int BWD_MIN_ROWS = 16;      // ... of at least this many rows each

struct Plan {
    int32_t team_wave;    // a team is a wavefront (else the workgroup)
    int32_t rows_per_wg;  // the contiguous block of rows of a workgroup
};

// the team of this thread and the rows it takes: r = first, first + step, ... < last
struct Team {
    bool wave;
    int ts, tid;
    int64_t first, last;
    int step;
    __device__ __forceinline__ Team(const Plan &plan, int64_t M) {
        wave = plan.team_wave != 0;
        ts = wave ? WAVE : (int)blockDim.x;
        tid = wave ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
        step = wave ? (int)(blockDim.x >> 6) : 1;
        const int64_t r0 = (int64_t)blockIdx.x * plan.rows_per_wg;
        first = r0 + (wave ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0);  // (uniform: rows have scalar bases)
        last = r0 + plan.rows_per_wg < M ? r0 + plan.rows_per_wg : M;
    }
};

// weight (+ 1) and bias of the thread's chunks
template <int CW, int K>
__device__ __forceinline__ void load_wb(const Team &t, int N, const void *weight, int wdt, const void *bias, int bdt, float wadd,
                                        float (&w)[K * CW], float (&b)[K * CW]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int ucol = k * t.ts * CW, lcol = t.tid * CW, col = ucol + lcol;
        float wv[CW], bv[CW];
#pragma unroll
        for (int i = 0; i < CW; ++i) wv[i] = bv[i] = 0.0f;
        if (col < N) {
            load_chunk<CW>(weight, wdt, ucol, lcol, wv);
#pragma unroll
            for (int i = 0; i < CW; ++i) wv[i] += wadd;
            if (bias) load_chunk<CW>(bias, bdt, ucol, lcol, bv);
        }
#pragma unroll
        for (int i = 0; i < CW; ++i) { w[k * CW + i] = wv[i]; b[k * CW + i] = bv[i]; }
    }
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
// weight and bias in registers over the workgroup's rows, the row in registers from its one read to the store of y
template <int CW, int K>
__global__ __launch_bounds__(1024) void norm_fwd_kernel(const fa_norm_fwd_params p, const Plan plan) {
    __shared__ float red[2][1][MAX_WAVES];
    const Team t(plan, p.M);
    const int N = p.N;
    const bool rms = (p.flags & FA_NORM_RMS) != 0;
    const float wadd = (p.flags & FA_NORM_ZERO_CENTERED) ? 1.0f : 0.0f, inv_n = 1.0f / (float)N;
    float w[K * CW], b[K * CW];
    load_wb<CW, K>(t, N, p.weight, p.weight_dtype, p.bias, p.bias_dtype, wadd, w, b);
    int phase = 0;
    for (int64_t r = t.first; r < t.last; r += t.step) {
        const char *x_row = row_of(p.x, p.x_dtype, r, p.x_row_stride);
        const char *res_row = p.residual ? row_of(p.residual, p.residual_dtype, r, p.residual_row_stride) : nullptr;
        char *ro_row = p.residual_out ? row_of(p.residual_out, p.residual_out_dtype, r, p.residual_out_row_stride) : nullptr;
        char *y_row = row_of(p.y, p.y_dtype, r, p.y_row_stride);
        const float rs = p.rowscale ? load_one(p.rowscale, p.rowscale_dtype, r) : 1.0f;
        float z[K * CW];
        float sum[1] = {0.0f};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int ucol = k * t.ts * CW, lcol = t.tid * CW, col = ucol + lcol;
            float v[CW];
#pragma unroll
            for (int i = 0; i < CW; ++i) v[i] = 0.0f;
            if (col < N) {
                load_chunk<CW>(x_row, p.x_dtype, ucol, lcol, v);
                if (p.rowscale) {
#pragma unroll
                    for (int i = 0; i < CW; ++i) v[i] *= rs;
                }
                if (res_row) {
                    float q[CW];
                    load_chunk<CW>(res_row, p.residual_dtype, ucol, lcol, q);
#pragma unroll
                    for (int i = 0; i < CW; ++i) v[i] += q[i];
                }
                if (ro_row) store_chunk<CW>(ro_row, p.residual_out_dtype, ucol, lcol, v);
            }
#pragma unroll
            for (int i = 0; i < CW; ++i) { z[k * CW + i] = v[i]; sum[0] += v[i]; }
        }
        float mean = 0.0f;
        if (!rms) {
            team_sum<1>(sum, t.wave, red, phase);
            mean = sum[0] * inv_n;
        }
        float sq[1] = {0.0f};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if ((k * t.ts + t.tid) * CW < N) {
#pragma unroll
                for (int i = 0; i < CW; ++i) {
                    const float d = z[k * CW + i] - mean;
                    sq[0] += d * d;
                }
            }
        }
        team_sum<1>(sq, t.wave, red, phase);
        const float rstd = 1.0f / sqrtf(sq[0] * inv_n + p.eps);
        if (t.tid == 0) {
            if (!rms) p.mean[r] = mean;
            p.rstd[r] = rstd;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int ucol = k * t.ts * CW, lcol = t.tid * CW, col = ucol + lcol;
            if (col < N) {
                float y[CW];
#pragma unroll
                for (int i = 0; i < CW; ++i) y[i] = (z[k * CW + i] - mean) * rstd * w[k * CW + i] + b[k * CW + i];
                store_chunk<CW>(y_row, p.y_dtype, ucol, lcol, y);
            }
        }
    }
}

// z = x * rowscale + residual at one chunk
template <int CW>
__device__ __forceinline__ void fwd_z(const fa_norm_fwd_params &p, const char *x_row, const char *res_row, float rs, int col,
                                      float (&v)[CW]) {
    load_chunk<CW>(x_row, p.x_dtype, 0, col, v);
    if (p.rowscale) {
#pragma unroll
        for (int i = 0; i < CW; ++i) v[i] *= rs;
    }
    if (res_row) {
        float q[CW];
        load_chunk<CW>(res_row, p.residual_dtype, 0, col, q);
#pragma unroll
        for (int i = 0; i < CW; ++i) v[i] += q[i];
    }
}

// The wide form (N > 1024 * FWD_COLS: a thread of 1024 has no registers for 32 columns of the row beside what the chunks in
// flight need).  One row per workgroup of 1024, three walks over it: the sum, the squares, the stores.  The second and third
// read x and the residual again -- 64 KiB a tensor, just read by the same workgroup -- and form the same fp32 z; nothing
// is written before the third walk, so residual_out may be the residual.
template <int CW>
__global__ __launch_bounds__(1024) void norm_fwd_wide_kernel(const fa_norm_fwd_params p) {
    __shared__ float red[2][1][MAX_WAVES];
    const int N = p.N, tid = threadIdx.x, span = 1024 * CW;
    const bool rms = (p.flags & FA_NORM_RMS) != 0;
    const float wadd = (p.flags & FA_NORM_ZERO_CENTERED) ? 1.0f : 0.0f, inv_n = 1.0f / (float)N;
    const int64_t r = blockIdx.x;
    const char *x_row = row_of(p.x, p.x_dtype, r, p.x_row_stride);
    const char *res_row = p.residual ? row_of(p.residual, p.residual_dtype, r, p.residual_row_stride) : nullptr;
    char *ro_row = p.residual_out ? row_of(p.residual_out, p.residual_out_dtype, r, p.residual_out_row_stride) : nullptr;
    char *y_row = row_of(p.y, p.y_dtype, r, p.y_row_stride);
    const float rs = p.rowscale ? load_one(p.rowscale, p.rowscale_dtype, r) : 1.0f;
    int phase = 0;
    float mean = 0.0f;
    if (!rms) {
        float sum[1] = {0.0f};
        for (int col = tid * CW; col < N; col += span) {
            float v[CW];
            fwd_z<CW>(p, x_row, res_row, rs, col, v);
#pragma unroll
            for (int i = 0; i < CW; ++i) sum[0] += v[i];
        }
        team_sum<1>(sum, false, red, phase);
        mean = sum[0] * inv_n;
    }
    float sq[1] = {0.0f};
    for (int col = tid * CW; col < N; col += span) {
        float v[CW];
        fwd_z<CW>(p, x_row, res_row, rs, col, v);
#pragma unroll
        for (int i = 0; i < CW; ++i) sq[0] += (v[i] - mean) * (v[i] - mean);
    }
    team_sum<1>(sq, false, red, phase);
    const float rstd = 1.0f / sqrtf(sq[0] * inv_n + p.eps);
    if (tid == 0) {
        if (!rms) p.mean[r] = mean;
        p.rstd[r] = rstd;
    }
    for (int col = tid * CW; col < N; col += span) {
        float v[CW], wv[CW], bv[CW], y[CW];
        fwd_z<CW>(p, x_row, res_row, rs, col, v);
        if (ro_row) store_chunk<CW>(ro_row, p.residual_out_dtype, 0, col, v);
        load_chunk<CW>(p.weight, p.weight_dtype, 0, col, wv);
#pragma unroll
        for (int i = 0; i < CW; ++i) bv[i] = 0.0f;
        if (p.bias) load_chunk<CW>(p.bias, p.bias_dtype, 0, col, bv);
#pragma unroll
        for (int i = 0; i < CW; ++i) y[i] = (v[i] - mean) * rstd * (wv[i] + wadd) + bv[i];
        store_chunk<CW>(y_row, p.y_dtype, 0, col, y);
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// The two row sums of a wide row (N > 1024 * BWD_COLS), for the column slabs of norm_bwd_kernel: one row per workgroup of 1024,
// row_sums[r] = {sum(xhat * w * dy), sum(w * dy)}
template <int CW>
__global__ __launch_bounds__(1024) void norm_bwd_row_sums_kernel(const fa_norm_bwd_params p, float *row_sums) {
    __shared__ float red[2][2][MAX_WAVES];
    const int N = p.N, tid = threadIdx.x, span = 1024 * CW;
    const float wadd = (p.flags & FA_NORM_ZERO_CENTERED) ? 1.0f : 0.0f;
    const int64_t r = blockIdx.x;
    const char *x_row = row_of(p.x, p.x_dtype, r, p.x_row_stride);
    const char *dy_row = row_of(p.dy, p.dy_dtype, r, p.dy_row_stride);
    const float mean = (p.flags & FA_NORM_RMS) ? 0.0f : p.mean[r], rstd = p.rstd[r];
    float c[2] = {0.0f, 0.0f};
    for (int col = tid * CW; col < N; col += span) {
        float v[CW], g[CW], wv[CW];
        load_chunk<CW>(x_row, p.x_dtype, 0, col, v);
        load_chunk<CW>(dy_row, p.dy_dtype, 0, col, g);
        load_chunk<CW>(p.weight, p.weight_dtype, 0, col, wv);
#pragma unroll
        for (int i = 0; i < CW; ++i) {
            const float wd = (wv[i] + wadd) * g[i];
            c[0] += (v[i] - mean) * rstd * wd;
            c[1] += wd;
        }
    }
    int phase = 0;
    team_sum<2>(c, false, red, phase);
    if (tid == 0) {
        row_sums[2 * r] = c[0];
        row_sums[2 * r + 1] = c[1];
    }
}

// A workgroup takes the rows of blockIdx.x and -- wide rows only -- the slab of 1024 * BWD_COLS columns of blockIdx.y, with the
// row sums read from `row_sums`; a row that fits one slab (row_sums == NULL) has its sums taken here.  xhat, w * dy and the
// weight stay in registers between the sums and dx, the dw / db columns over all rows of the workgroup.
template <int CW, int K>
__global__ __launch_bounds__(1024) void norm_bwd_kernel(const fa_norm_bwd_params p, const Plan plan, const float *row_sums) {
    __shared__ float red[2][2][MAX_WAVES];
    const Team t(plan, p.M);
    const int N = p.N, slab = blockIdx.y * (1024 * BWD_COLS);
    const bool rms = (p.flags & FA_NORM_RMS) != 0;
    const float wadd = (p.flags & FA_NORM_ZERO_CENTERED) ? 1.0f : 0.0f, inv_n = 1.0f / (float)N;
    float w[K * CW], b[K * CW], dw[K * CW], db[K * CW];
#pragma unroll
    for (int j = 0; j < K * CW; ++j) dw[j] = db[j] = 0.0f;
#pragma unroll
    for (int k = 0; k < K; ++k) {  // (the bias is read only for y)
        const int ucol = slab + k * t.ts * CW, lcol = t.tid * CW;
        float wv[CW], bv[CW];
#pragma unroll
        for (int i = 0; i < CW; ++i) wv[i] = bv[i] = 0.0f;
        if (ucol + lcol < N) {
            load_chunk<CW>(p.weight, p.weight_dtype, ucol, lcol, wv);
#pragma unroll
            for (int i = 0; i < CW; ++i) wv[i] += wadd;
            if (p.y && p.bias) load_chunk<CW>(p.bias, p.bias_dtype, ucol, lcol, bv);
        }
#pragma unroll
        for (int i = 0; i < CW; ++i) { w[k * CW + i] = wv[i]; b[k * CW + i] = bv[i]; }
    }
    int phase = 0;
    for (int64_t r = t.first; r < t.last; r += t.step) {
        const char *x_row = row_of(p.x, p.x_dtype, r, p.x_row_stride);
        const char *dy_row = row_of(p.dy, p.dy_dtype, r, p.dy_row_stride);
        const float mean = rms ? 0.0f : p.mean[r], rstd = p.rstd[r];
        const float rs = p.rowscale ? load_one(p.rowscale, p.rowscale_dtype, r) : 1.0f;
        float xh[K * CW], wd[K * CW];
        float c[2] = {0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int ucol = slab + k * t.ts * CW, lcol = t.tid * CW;
            float v[CW], g[CW];
#pragma unroll
            for (int i = 0; i < CW; ++i) xh[k * CW + i] = wd[k * CW + i] = 0.0f;
            if (ucol + lcol < N) {
                load_chunk<CW>(x_row, p.x_dtype, ucol, lcol, v);
                load_chunk<CW>(dy_row, p.dy_dtype, ucol, lcol, g);
#pragma unroll
                for (int i = 0; i < CW; ++i) {
                    const float xc = (v[i] - mean) * rstd, wc = w[k * CW + i] * g[i];
                    dw[k * CW + i] += g[i] * xc;
                    db[k * CW + i] += g[i];
                    c[0] += xc * wc;
                    c[1] += wc;
                    xh[k * CW + i] = xc;
                    wd[k * CW + i] = wc;
                }
                if (p.y) {
                    float y[CW];
#pragma unroll
                    for (int i = 0; i < CW; ++i) y[i] = xh[k * CW + i] * w[k * CW + i] + b[k * CW + i];
                    store_chunk<CW>(row_of(p.y, p.y_dtype, r, p.y_row_stride), p.y_dtype, ucol, lcol, y);
                }
            }
        }
        if (row_sums) {
            c[0] = row_sums[2 * r];
            c[1] = row_sums[2 * r + 1];
        } else {
            team_sum<2>(c, t.wave, red, phase);
        }
        const float c1 = c[0] * inv_n, c2 = rms ? 0.0f : c[1] * inv_n;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int ucol = slab + k * t.ts * CW, lcol = t.tid * CW;
            if (ucol + lcol < N) {
                float dx[CW];
#pragma unroll
                for (int i = 0; i < CW; ++i) dx[i] = (wd[k * CW + i] - (xh[k * CW + i] * c1 + c2)) * rstd;
                if (p.dresidual) {
                    float q[CW];
                    load_chunk<CW>(row_of(p.dresidual, p.dresidual_dtype, r, p.dresidual_row_stride), p.dresidual_dtype, ucol, lcol, q);
#pragma unroll
                    for (int i = 0; i < CW; ++i) dx[i] += q[i];
                }
                if (p.dresidual_in)
                    store_chunk<CW>(row_of(p.dresidual_in, p.dresidual_in_dtype, r, p.dresidual_in_row_stride), p.dresidual_in_dtype,
                                    ucol, lcol, dx);
                if (p.rowscale) {
#pragma unroll
                    for (int i = 0; i < CW; ++i) dx[i] *= rs;
                }
                store_chunk<CW>(row_of(p.dx, p.dx_dtype, r, p.dx_row_stride), p.dx_dtype, ucol, lcol, dx);
            }
        }
    }
    // one partial row of dw and one of db per workgroup row block: workspace[0][blockIdx.x][N], workspace[1][blockIdx.x][N]
    float *dw_part = static_cast<float *>(p.workspace) + (int64_t)blockIdx.x * N;
    float *db_part = dw_part + (int64_t)gridDim.x * N;
    if (!t.wave) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int ucol = slab + k * t.ts * CW, lcol = t.tid * CW;
            if (ucol + lcol < N) {
                float a[CW], c[CW];
#pragma unroll
                for (int i = 0; i < CW; ++i) { a[i] = dw[k * CW + i]; c[i] = db[k * CW + i]; }
                store_chunk<CW>(dw_part, FA_DTYPE_FP32, ucol, lcol, a);
                store_chunk<CW>(db_part, FA_DTYPE_FP32, ucol, lcol, c);
            }
        }
        return;
    }
    // wavefront teams (N <= BWD_WAVE_ROW_N, one slab): the wavefronts' columns are added through LDS, in wave order
    __shared__ float comb[WAVE_TEAMS * BWD_WAVE_ROW_N];
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int which = 0; which < 2; ++which) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int col = (k * t.ts + t.tid) * CW;
            if (col < N) {
#pragma unroll
                for (int i = 0; i < CW; ++i) comb[wave * BWD_WAVE_ROW_N + col + i] = which ? db[k * CW + i] : dw[k * CW + i];
            }
        }
        __syncthreads();
        float *part = which ? db_part : dw_part;
        for (int col = threadIdx.x; col < N; col += blockDim.x) {
            float s = 0.0f;
            for (int v = 0; v < nw; ++v) s += comb[v * BWD_WAVE_ROW_N + col];
            part[col] = s;
        }
        __syncthreads();
    }
}

// dw[col] = sum over the P partial rows, db likewise, in the fixed order of reduce_partial_rows
__global__ __launch_bounds__(1024) void norm_reduce_kernel(const float *workspace, int P, int N, void *dw, int dw_dtype, void *db,
                                                           int db_dtype) {
    __shared__ float comb[MAX_WAVES][REDUCE_COLS];
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        void *dst = which ? db : dw;
        if (!dst) continue;
        reduce_partial_rows(workspace + (int64_t)which * P * N, P, N, dst, which ? db_dtype : dw_dtype, comb);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
struct Launch {
    int cw;         // 8 / 4: 16-byte accesses of x; 1: element accesses
    bool wide;      // rows of more than 1024 * cols columns
    int threads;
    int grid;       // workgroups of plan.rows_per_wg rows
    int slabs;      // grid.y: the column slabs of a wide backward, else 1
    Plan plan;
};

// the shape of a launch over M rows of N columns; `vec`: what the operands' alignment allows
Launch launch_shape(int64_t M, int N, int x_dtype, bool vec, bool backward) {
    Launch l;
    const int cols = backward ? BWD_COLS : FWD_COLS;  // per thread, unless wide
    l.cw = !vec ? 1 : x_dtype == FA_DTYPE_FP32 ? 4 : 8;
    l.plan.team_wave = N <= WAVE * cols;
    l.wide = N > 1024 * cols;
    l.slabs = backward && l.wide ? (N + 1024 * cols - 1) / (1024 * cols) : 1;
    if (l.plan.team_wave) l.threads = WAVE * WAVE_TEAMS;
    else l.threads = N <= 256 * cols ? 256 : N <= 512 * cols ? 512 : 1024;
    const int teams = l.plan.team_wave ? WAVE_TEAMS : 1;
    int64_t rows;
    if (backward) {  // (a function of M alone: the partial count must not depend on the access shape)
        rows = (M + BWD_PARTIALS - 1) / BWD_PARTIALS;
        if (rows < BWD_MIN_ROWS) rows = BWD_MIN_ROWS;
        rows = (rows + WAVE_TEAMS - 1) / WAVE_TEAMS * WAVE_TEAMS;
    } else if (l.wide) {  // one row per workgroup
        rows = 1;
    } else {  // enough rows to pay for reading weight and bias, enough workgroups to fill the device
        rows = M / (2048 * teams);
        rows = rows < 1 ? 1 : rows > 8 ? 8 : rows;
        rows *= teams;
    }
    l.plan.rows_per_wg = (int32_t)rows;
    l.grid = (int)((M + rows - 1) / rows);
    return l;
}

// the launch of a valid forward call: 16-byte accesses where N and every operand's base and row pitch allow them
Launch fwd_launch(const fa_norm_fwd_params *p) {
    const bool vec = p->N % (p->x_dtype == FA_DTYPE_FP32 ? 4 : 8) == 0 && rows_16_bytes(p->x, p->x_dtype, p->x_row_stride) &&
                     rows_16_bytes(p->residual, p->residual_dtype, p->residual_row_stride) &&
                     rows_16_bytes(p->y, p->y_dtype, p->y_row_stride) &&
                     rows_16_bytes(p->residual_out, p->residual_out_dtype, p->residual_out_row_stride) &&
                     aligned_to(p->weight, 16) && aligned_to(p->bias, 16);
    return launch_shape(p->M, p->N, p->x_dtype, vec, false);
}

// ... of a valid backward call (the bias is read only for y)
Launch bwd_launch(const fa_norm_bwd_params *p) {
    const bool vec = p->N % (p->x_dtype == FA_DTYPE_FP32 ? 4 : 8) == 0 && rows_16_bytes(p->x, p->x_dtype, p->x_row_stride) &&
                     rows_16_bytes(p->dy, p->dy_dtype, p->dy_row_stride) &&
                     rows_16_bytes(p->dresidual, p->dresidual_dtype, p->dresidual_row_stride) &&
                     rows_16_bytes(p->dx, p->dx_dtype, p->dx_row_stride) &&
                     rows_16_bytes(p->dresidual_in, p->dresidual_in_dtype, p->dresidual_in_row_stride) &&
                     rows_16_bytes(p->y, p->y_dtype, p->y_row_stride) && aligned_to(p->weight, 16) &&
                     (!p->y || aligned_to(p->bias, 16));
    return launch_shape(p->M, p->N, p->x_dtype, vec, true);
}

void fill_plan(const Launch &l, fa_norm_plan *plan) {
    plan->cw = l.cw;
    plan->threads = l.threads;
    plan->team_wave = l.plan.team_wave;
    plan->wide = l.wide;
    plan->rows_per_wg = l.plan.rows_per_wg;
    plan->grid_x = l.grid;
    plan->grid_y = l.slabs;
}

int64_t bwd_partials(int64_t M, int N) { return launch_shape(M, N, FA_DTYPE_BF16, false, true).grid; }

int check_shape(int64_t M, int N, int x_dtype, bool backward) {
    if (M < 0 || N < 1) return FA_ERR_BAD_SHAPE;
    // (the wide forms take one row per workgroup in grid.x)
    if (N > 1024 * (backward ? BWD_COLS : FWD_COLS) && M > INT32_MAX) return FA_ERR_BAD_SHAPE;
    if ((int64_t)N * esize(x_dtype) > FA_NORM_MAX_ROW_BYTES) return FA_ERR_BAD_SHAPE;
    if (M > ((int64_t)1 << 33)) return FA_ERR_BAD_SHAPE;  // (the grid: at least 8 rows per workgroup from M = 2^14)
    return FA_OK;
}

}  // namespace

extern "C" {

uint32_t fa_norm_fwd_params_size(void) { return (uint32_t)sizeof(fa_norm_fwd_params); }
uint32_t fa_norm_bwd_params_size(void) { return (uint32_t)sizeof(fa_norm_bwd_params); }

int fa_norm_fwd_validate(const fa_norm_fwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_norm_fwd_params)) return FA_ERR_BAD_ABI;
    if (!known_dtype(p->x_dtype) || !known_dtype(p->weight_dtype) || !known_dtype(p->y_dtype)) return FA_ERR_BAD_DTYPE;
    if (p->bias && !known_dtype(p->bias_dtype)) return FA_ERR_BAD_DTYPE;
    if (p->rowscale && !known_dtype(p->rowscale_dtype)) return FA_ERR_BAD_DTYPE;
    if (p->residual && p->residual_dtype != p->x_dtype && p->residual_dtype != FA_DTYPE_FP32) return FA_ERR_BAD_DTYPE;
    if (p->residual_out && p->residual_out_dtype != p->x_dtype && p->residual_out_dtype != FA_DTYPE_FP32) return FA_ERR_BAD_DTYPE;
    const int st = check_shape(p->M, p->N, p->x_dtype, false);
    if (st != FA_OK) return st;
    if (!p->x || !p->weight || !p->y || !p->rstd || (!(p->flags & FA_NORM_RMS) && !p->mean)) return FA_ERR_NULL_POINTER;
    // element accesses keep their natural alignment
    if (!aligned_to(p->x, esize(p->x_dtype)) || !aligned_to(p->residual, esize(p->residual_dtype)) ||
        !aligned_to(p->y, esize(p->y_dtype)) || !aligned_to(p->residual_out, esize(p->residual_out_dtype)) ||
        !aligned_to(p->weight, esize(p->weight_dtype)) || !aligned_to(p->bias, esize(p->bias_dtype)) ||
        !aligned_to(p->rowscale, esize(p->rowscale_dtype)) || !aligned_to(p->mean, 4) || !aligned_to(p->rstd, 4))
        return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int fa_norm_fwd(const fa_norm_fwd_params *p, void *stream_) {
    const int st = fa_norm_fwd_validate(p);
    if (st != FA_OK) return st;
    if (p->M == 0) return FA_OK;  // (no zero grid)
    const Launch l = fwd_launch(p);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
#define FA_NORM_FWD_LAUNCH(CW) \
    hipLaunchKernelGGL((norm_fwd_kernel<CW, FWD_COLS / CW>), dim3(l.grid), dim3(l.threads), 0, stream, *p, l.plan)
#define FA_NORM_FWD_WIDE_LAUNCH(CW) hipLaunchKernelGGL((norm_fwd_wide_kernel<CW>), dim3(l.grid), dim3(l.threads), 0, stream, *p)
    if (l.wide) {  // (16-bit x: a row of fp32 has at most 1024 * FWD_COLS columns)
        if (l.cw == 8) FA_NORM_FWD_WIDE_LAUNCH(8);
        else FA_NORM_FWD_WIDE_LAUNCH(1);
    } else if (l.cw == 8) FA_NORM_FWD_LAUNCH(8);
    else if (l.cw == 4) FA_NORM_FWD_LAUNCH(4);
    else FA_NORM_FWD_LAUNCH(1);
#undef FA_NORM_FWD_LAUNCH
#undef FA_NORM_FWD_WIDE_LAUNCH
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

// workspace: dw partials [P][N], db partials [P][N], then -- wide rows -- the row sums [M][2]
uint64_t fa_norm_bwd_workspace_bytes(const fa_norm_bwd_params *p) {
    if (!p || p->M <= 0 || p->N < 1) return 0;
    const uint64_t partials = (uint64_t)bwd_partials(p->M, p->N) * (uint64_t)p->N * 2 * sizeof(float);
    return partials + (p->N > 1024 * BWD_COLS ? (uint64_t)p->M * 2 * sizeof(float) : 0);
}

int fa_norm_fwd_plan(const fa_norm_fwd_params *p, fa_norm_plan *plan) {
    const int st = fa_norm_fwd_validate(p);
    if (st != FA_OK) return st;
    if (!plan) return FA_ERR_NULL_POINTER;
    fill_plan(fwd_launch(p), plan);
    return FA_OK;
}

int fa_norm_bwd_validate(const fa_norm_bwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_norm_bwd_params)) return FA_ERR_BAD_ABI;
    if (!known_dtype(p->x_dtype) || !known_dtype(p->dy_dtype) || !known_dtype(p->weight_dtype) || !known_dtype(p->dx_dtype))
        return FA_ERR_BAD_DTYPE;
    if ((p->db || (p->y && p->bias)) && !known_dtype(p->bias_dtype)) return FA_ERR_BAD_DTYPE;
    if (p->y && !known_dtype(p->y_dtype)) return FA_ERR_BAD_DTYPE;
    if (p->rowscale && !known_dtype(p->rowscale_dtype)) return FA_ERR_BAD_DTYPE;
    // x is the residual stream: of the input's dtype or fp32; its gradients are of its dtype
    if (p->x_dtype != p->dx_dtype && p->x_dtype != FA_DTYPE_FP32) return FA_ERR_BAD_DTYPE;
    if (p->dresidual && p->dresidual_dtype != p->x_dtype) return FA_ERR_BAD_DTYPE;
    if (p->dresidual_in && p->dresidual_in_dtype != p->x_dtype) return FA_ERR_BAD_DTYPE;
    const int st = check_shape(p->M, p->N, p->x_dtype, true);
    if (st != FA_OK) return st;
    if (!p->x || !p->dy || !p->weight || !p->rstd || !p->dx || !p->dw || (!(p->flags & FA_NORM_RMS) && !p->mean))
        return FA_ERR_NULL_POINTER;
    const uint64_t need = fa_norm_bwd_workspace_bytes(p);
    if (need > 0 && (!p->workspace || p->workspace_bytes < need)) return FA_ERR_WORKSPACE;
    if (!aligned_to(p->workspace, 16)) return FA_ERR_BAD_STRIDE;
    if (!aligned_to(p->x, esize(p->x_dtype)) || !aligned_to(p->dy, esize(p->dy_dtype)) ||
        !aligned_to(p->dresidual, esize(p->dresidual_dtype)) || !aligned_to(p->dx, esize(p->dx_dtype)) ||
        !aligned_to(p->dresidual_in, esize(p->dresidual_in_dtype)) || !aligned_to(p->y, esize(p->y_dtype)) ||
        !aligned_to(p->weight, esize(p->weight_dtype)) || !aligned_to(p->bias, esize(p->bias_dtype)) ||
        !aligned_to(p->dw, esize(p->weight_dtype)) || !aligned_to(p->db, esize(p->bias_dtype)) ||
        !aligned_to(p->rowscale, esize(p->rowscale_dtype)) || !aligned_to(p->mean, 4) || !aligned_to(p->rstd, 4))
        return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int fa_norm_bwd_plan(const fa_norm_bwd_params *p, fa_norm_plan *plan) {
    const int st = fa_norm_bwd_validate(p);
    if (st != FA_OK) return st;
    if (!plan) return FA_ERR_NULL_POINTER;
    fill_plan(bwd_launch(p), plan);
    return FA_OK;
}

int fa_norm_bwd(const fa_norm_bwd_params *p, void *stream_) {
    const int st = fa_norm_bwd_validate(p);
    if (st != FA_OK) return st;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int partials = 0;
    if (p->M > 0) {
        const Launch l = bwd_launch(p);
        partials = l.grid;
        float *row_sums = nullptr;
        const dim3 grid(l.grid, l.slabs);
        if (l.wide) {  // the row sums first, then one workgroup per row block and slab of 1024 * BWD_COLS columns
            row_sums = static_cast<float *>(p->workspace) + (int64_t)l.grid * p->N * 2;
#define FA_NORM_BWD_SUMS_LAUNCH(CW) \
    hipLaunchKernelGGL((norm_bwd_row_sums_kernel<CW>), dim3((unsigned)p->M), dim3(1024), 0, stream, *p, row_sums)
            if (l.cw == 8) FA_NORM_BWD_SUMS_LAUNCH(8);
            else if (l.cw == 4) FA_NORM_BWD_SUMS_LAUNCH(4);
            else FA_NORM_BWD_SUMS_LAUNCH(1);
#undef FA_NORM_BWD_SUMS_LAUNCH
            if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
        }
#define FA_NORM_BWD_LAUNCH(CW) \
    hipLaunchKernelGGL((norm_bwd_kernel<CW, BWD_COLS / CW>), grid, dim3(l.threads), 0, stream, *p, l.plan, (const float *)row_sums)
        if (l.cw == 8) FA_NORM_BWD_LAUNCH(8);
        else if (l.cw == 4) FA_NORM_BWD_LAUNCH(4);
        else FA_NORM_BWD_LAUNCH(1);
#undef FA_NORM_BWD_LAUNCH
        if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    }
    // (no rows: no partials, and the sums are zero)
    hipLaunchKernelGGL(norm_reduce_kernel, dim3((p->N + REDUCE_COLS - 1) / REDUCE_COLS), dim3(WAVE * MAX_WAVES), 0, stream,
                       static_cast<const float *>(p->workspace), partials, p->N, p->dw, p->weight_dtype, p->db, p->bias_dtype);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

}  // extern "C"
