// fa_dropout_norm.hip — fa_dropout_norm_fwd / fa_dropout_norm_bwd (include/fa_dropout_norm.h): dropout on the branch output(s)
// fused into the residual add and the LayerNorm / RMSNorm, forward and backward.  A translation unit of its own: no kernel
// comes from another unit or goes to one, fa_norm.hip included, because the kernel set of every unit is pinned by its tests.
// That rule is about kernels: the chunk loads and stores, the sums, the ordered reduce of partial rows and the host predicates
// are the inline functions of fa_rowwise.h, shared with the other row units.  The avalanche of the counter hash and the
// mix of (seed, offset) are there too; the keying (a key per row, groups of 4 columns) is this unit's own.
//
// A workgroup of 64 / 256 / 512 / 1024 threads (the smallest that gives a thread at most C columns) takes one row at a
// time out of a contiguous block of rows; C = 16 / 8 / 2 (CW = 8 / 4 / 1) in the forward, 8 / 4 / 2 in the backward.  Thread t of `ts` owns the chunks
// (k * ts + t) of CW columns, k < K = C / CW: neighbouring lanes read neighbouring 16 bytes.  The dtype of every tensor and
// the presence of every optional operand are kernel arguments, hence wave-uniform: they branch in the scalar unit.  The
// kernels are instantiated by access shape and by whether decisions are drawn (DROP: p > 0), never by a run-time p:
//   CW = 8   16-byte accesses of a 16-bit x0 (two of them per chunk of an fp32 tensor beside it, 8 bytes of a mask)
//   CW = 4   16-byte accesses of an fp32 x0 (8 bytes of a 16-bit tensor beside it, 4 of a mask)
//   CW = 1   element accesses: any N >= 1, any alignment
// Forward: the row is read once, rounded to the stream dtype and kept in fp32 registers between the statistics and the
// normalise step; the weights and biases are read per row (cache hits): the registers they would take are what keeps every
// form free of spills.
// Backward: xhat and the weighted dz stay in registers between the two row sums and the gradients; up to four column sums
// (dw0, db0, then dw1 and db1 of the two-weight form or dcolscale of the scaled form, which exclude each other) are kept in
// registers over the workgroup's rows and written as fp32 partial rows; dropout_norm_reduce_kernel adds them in a fixed order.
// Rows wider than 1024 * C have forms that never spill: the forward walks such a row three times inside the same kernel
// (plan.wide), the backward takes the row sums in a launch of their own (dropout_norm_bwd_row_sums_kernel) and then splits the
// columns into slabs of 1024 * C over blockIdx.y of the same dropout_norm_bwd_kernel.  No atomics anywhere.
#include "../../include/fa_dropout_norm.h"
#include "fa_rowwise.h"

namespace {

using namespace fa_row;

// columns per thread: of the forward, and of the backward, which keeps six values per column.  Fewer with the narrower
// accesses: a thread has that many more chunks in flight, and their addresses and loads must fit beside the row
__host__ __device__ constexpr int fwd_cols(int cw) { return cw == 8 ? 16 : cw == 4 ? 8 : 2; }
__host__ __device__ constexpr int bwd_cols(int cw) { return cw == 8 ? 8 : cw == 4 ? 4 : 2; }
constexpr int MIN_FWD_COLS = 2, MIN_BWD_COLS = 2;
constexpr int BWD_PARTIALS = 1024;  // the backward aims at this many workgroups ...
constexpr int BWD_MIN_ROWS = 16;    // ... of at least this many rows each
constexpr int MAX_SUMS = 4;         // column sums of a backward

struct Plan {
    int32_t rows_per_wg;  // the contiguous block of rows of a workgroup
    int32_t wide;         // forward: three walks over the row
    uint32_t keep_max;    // an element is kept iff its byte <= keep_max
    float inv_keep;       // 1 / (1 - p)
};

// ---- dropout decisions (restated) ---------------------------------------------------------------------------------
// the key of (row, stream): a bijection of the row's lower half for a given seed, upper half and stream, so two rows of a
// call differ in their keys
__device__ __forceinline__ uint32_t row_key(uint32_t mix, int64_t row, uint32_t stream) {
    const uint32_t lo = (uint32_t)row, hi = (uint32_t)((uint64_t)row >> 32);
    return lowbias32((mix ^ hi * 0x2545F491u ^ stream * 0x68E31DA4u) ^ lo * 0x9E3779B1u);
}
// the four bytes of column group g (columns 4 g .. 4 g + 3) of the row of `key`; a bijection of g for a given key
__device__ __forceinline__ uint32_t group_bytes(uint32_t key, uint32_t g) { return lowbias32(key ^ (g * 0x85EBCA77u + 0x165667B1u)); }

// keep[i] of the CW columns from `col` on (col a multiple of CW where CW > 1)
template <int CW>
__device__ __forceinline__ void decide(uint32_t key, int col, uint32_t keep_max, bool (&keep)[CW]) {
    if constexpr (CW == 1) {
        keep[0] = ((group_bytes(key, (uint32_t)col >> 2) >> (8 * (col & 3))) & 255u) <= keep_max;
    } else {
#pragma unroll
        for (int g = 0; g < CW / 4; ++g) {
            const uint32_t h = group_bytes(key, ((uint32_t)col >> 2) + g);
#pragma unroll
            for (int i = 0; i < 4; ++i) keep[4 * g + i] = ((h >> (8 * i)) & 255u) <= keep_max;
        }
    }
}

// 1 = kept, at column `col` of a dense row of bytes
template <int CW>
__device__ __forceinline__ void store_mask(uint8_t *row, int col, const bool (&keep)[CW]) {
    if constexpr (CW == 1) {
        row[col] = keep[0] ? 1 : 0;
    } else {
        uint32_t w[CW / 4];
#pragma unroll
        for (int g = 0; g < CW / 4; ++g)
            w[g] = (keep[4 * g] ? 1u : 0u) | (keep[4 * g + 1] ? 0x100u : 0u) | (keep[4 * g + 2] ? 0x10000u : 0u) |
                   (keep[4 * g + 3] ? 0x1000000u : 0u);
        if constexpr (CW == 8) *reinterpret_cast<uint2 *>(row + col) = make_uint2(w[0], w[1]);
        else *reinterpret_cast<uint32_t *>(row + col) = w[0];
    }
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
// what the chunks of one row share
struct FwdRow {
    const char *x0, *x1, *res;
    uint8_t *dm0, *dm1;
    float rs;
    uint32_t key0, key1;
};

template <bool DROP>
__device__ __forceinline__ FwdRow fwd_row(const fa_dropout_norm_fwd_params &p, uint32_t mix, int64_t r) {
    FwdRow f;
    f.x0 = row_of(p.x0, p.x0_dtype, r, p.x0_row_stride);
    f.x1 = p.x1 ? row_of(p.x1, p.x0_dtype, r, p.x1_row_stride) : nullptr;
    f.res = p.residual ? row_of(p.residual, p.residual_dtype, r, p.residual_row_stride) : nullptr;
    f.dm0 = DROP && p.dmask0 ? p.dmask0 + r * p.N : nullptr;
    f.dm1 = DROP && p.dmask1 ? p.dmask1 + r * p.N : nullptr;
    f.rs = p.rowscale ? load_one(p.rowscale, p.rowscale_dtype, r) : 1.0f;
    f.key0 = DROP ? row_key(mix, r, 0u) : 0u;
    f.key1 = DROP ? row_key(mix, r, 1u) : 0u;
    return f;
}

// the stream at one chunk: scaled, dropped, added, rounded to the stream dtype; the masks where `masks`
template <int CW, bool DROP>
__device__ __forceinline__ void fwd_x(const fa_dropout_norm_fwd_params &p, const Plan &plan, const FwdRow &f, int ucol, int lcol,
                                      bool masks, float (&v)[CW]) {
    load_chunk<CW>(f.x0, p.x0_dtype, ucol, lcol, v);
    if (p.rowscale) {
#pragma unroll
        for (int i = 0; i < CW; ++i) v[i] *= f.rs;
    }
    if (p.colscale) {
        float c[CW];
        load_chunk<CW>(p.colscale, p.colscale_dtype, ucol, lcol, c);
#pragma unroll
        for (int i = 0; i < CW; ++i) v[i] *= c[i];
    }
    if constexpr (DROP) {
        bool keep[CW];
        decide<CW>(f.key0, ucol + lcol, plan.keep_max, keep);
#pragma unroll
        for (int i = 0; i < CW; ++i) v[i] = keep[i] ? v[i] * plan.inv_keep : 0.0f;
        if (masks && f.dm0) store_mask<CW>(f.dm0, ucol + lcol, keep);
    }
    if (f.x1) {
        float q[CW];
        load_chunk<CW>(f.x1, p.x0_dtype, ucol, lcol, q);
        if constexpr (DROP) {
            bool keep[CW];
            decide<CW>(f.key1, ucol + lcol, plan.keep_max, keep);
#pragma unroll
            for (int i = 0; i < CW; ++i) q[i] = keep[i] ? q[i] * plan.inv_keep : 0.0f;
            if (masks && f.dm1) store_mask<CW>(f.dm1, ucol + lcol, keep);
        }
#pragma unroll
        for (int i = 0; i < CW; ++i) v[i] += q[i];
    }
    if (f.res) {
        float q[CW];
        load_chunk<CW>(f.res, p.residual_dtype, ucol, lcol, q);
#pragma unroll
        for (int i = 0; i < CW; ++i) v[i] += q[i];
    }
    round_to<CW>(p.x_dtype, v);
}

// z = (x - mu) * rsigma * w + b at one chunk, w / b read from memory
template <int CW>
__device__ __forceinline__ void store_z(const fa_dropout_norm_fwd_params &p, char *z_row, const void *weight, const void *bias,
                                        int ucol, int lcol, float mu, float rsigma, const float (&x)[CW]) {
    float wv[CW], bv[CW], z[CW];
    load_chunk<CW>(weight, p.weight_dtype, ucol, lcol, wv);
#pragma unroll
    for (int i = 0; i < CW; ++i) bv[i] = 0.0f;
    if (bias) load_chunk<CW>(bias, p.weight_dtype, ucol, lcol, bv);
#pragma unroll
    for (int i = 0; i < CW; ++i) z[i] = (x[i] - mu) * rsigma * wv[i] + bv[i];
    store_chunk<CW>(z_row, p.z_dtype, ucol, lcol, z);
}

// The wide form (N > 1024 * fwd_cols(CW)): one row per workgroup of 1024, three walks over it -- the sum, the squares, the stores.
// The second and third form the same x again from the same reads and the same decisions
template <int CW, bool DROP>
__device__ __forceinline__ void fwd_wide_row(const fa_dropout_norm_fwd_params &p, const Plan &plan, uint32_t mix,
                                             float (&red)[2][1][MAX_WAVES]) {
    const int N = p.N, tid = threadIdx.x, span = 1024 * CW;
    const bool rms = (p.flags & FA_DROPOUT_NORM_RMS) != 0;
    const float inv_n = 1.0f / (float)N;
    const int64_t r = blockIdx.x;
    const FwdRow f = fwd_row<DROP>(p, mix, r);
    int phase = 0;
    float mu = 0.0f;
    if (!rms) {
        float sum[1] = {0.0f};
        for (int col = tid * CW; col < N; col += span) {
            float v[CW];
            fwd_x<CW, DROP>(p, plan, f, 0, col, false, v);
#pragma unroll
            for (int i = 0; i < CW; ++i) sum[0] += v[i];
        }
        team_sum<1, true>(sum, false, red, phase);
        mu = sum[0] * inv_n;
    }
    float sq[1] = {0.0f};
    for (int col = tid * CW; col < N; col += span) {
        float v[CW];
        fwd_x<CW, DROP>(p, plan, f, 0, col, false, v);
#pragma unroll
        for (int i = 0; i < CW; ++i) sq[0] += (v[i] - mu) * (v[i] - mu);
    }
    team_sum<1, true>(sq, false, red, phase);
    const float rsigma = 1.0f / sqrtf(sq[0] * inv_n + p.eps);
    if (tid == 0) {
        if (!rms) p.mu[r] = mu;
        p.rsigma[r] = rsigma;
    }
    char *x_row = p.x ? row_of(p.x, p.x_dtype, r, p.x_row_stride) : nullptr;
    char *z0_row = row_of(p.z0, p.z_dtype, r, p.z0_row_stride);
    char *z1_row = p.weight1 ? row_of(p.z1, p.z_dtype, r, p.z1_row_stride) : nullptr;
    for (int col = tid * CW; col < N; col += span) {
        float v[CW];
        fwd_x<CW, DROP>(p, plan, f, 0, col, true, v);
        if (x_row) store_chunk<CW>(x_row, p.x_dtype, 0, col, v);
        store_z<CW>(p, z0_row, p.weight0, p.bias0, 0, col, mu, rsigma, v);
        if (z1_row) store_z<CW>(p, z1_row, p.weight1, p.bias1, 0, col, mu, rsigma, v);
    }
}

template <int CW, bool DROP>
__global__ __launch_bounds__(1024) void dropout_norm_fwd_kernel(const fa_dropout_norm_fwd_params p, const Plan plan) {
    constexpr int K = fwd_cols(CW) / CW;
    __shared__ float red[2][1][MAX_WAVES];
    const uint32_t mix = DROP ? seed_mix(p.rng_state) : 0u;
    if (plan.wide) {
        fwd_wide_row<CW, DROP>(p, plan, mix, red);
        return;
    }
    const int N = p.N, ts = blockDim.x, tid = threadIdx.x;
    const bool rms = (p.flags & FA_DROPOUT_NORM_RMS) != 0;
    const float inv_n = 1.0f / (float)N;
    const int64_t first = (int64_t)blockIdx.x * plan.rows_per_wg;
    const int64_t last = first + plan.rows_per_wg < p.M ? first + plan.rows_per_wg : p.M;
    int phase = 0;
    for (int64_t r = first; r < last; ++r) {
        const FwdRow f = fwd_row<DROP>(p, mix, r);
        char *x_row = p.x ? row_of(p.x, p.x_dtype, r, p.x_row_stride) : nullptr;
        char *z0_row = row_of(p.z0, p.z_dtype, r, p.z0_row_stride);
        float x[K * CW];
        float sum[1] = {0.0f};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int ucol = k * ts * CW, lcol = tid * CW;
            float v[CW];
#pragma unroll
            for (int i = 0; i < CW; ++i) v[i] = 0.0f;
            if (ucol + lcol < N) {
                fwd_x<CW, DROP>(p, plan, f, ucol, lcol, true, v);
                if (x_row) store_chunk<CW>(x_row, p.x_dtype, ucol, lcol, v);
            }
#pragma unroll
            for (int i = 0; i < CW; ++i) { x[k * CW + i] = v[i]; sum[0] += v[i]; }
        }
        float mu = 0.0f;
        if (!rms) {
            team_sum<1, true>(sum, false, red, phase);
            mu = sum[0] * inv_n;
        }
        float sq[1] = {0.0f};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if ((k * ts + tid) * CW < N) {
#pragma unroll
                for (int i = 0; i < CW; ++i) {
                    const float d = x[k * CW + i] - mu;
                    sq[0] += d * d;
                }
            }
        }
        team_sum<1, true>(sq, false, red, phase);
        const float rsigma = 1.0f / sqrtf(sq[0] * inv_n + p.eps);
        if (tid == 0) {
            if (!rms) p.mu[r] = mu;
            p.rsigma[r] = rsigma;
        }
        char *z1_row = p.weight1 ? row_of(p.z1, p.z_dtype, r, p.z1_row_stride) : nullptr;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int ucol = k * ts * CW, lcol = tid * CW;
            if (ucol + lcol < N) {
                float v[CW];
#pragma unroll
                for (int i = 0; i < CW; ++i) v[i] = x[k * CW + i];
                store_z<CW>(p, z0_row, p.weight0, p.bias0, ucol, lcol, mu, rsigma, v);
                if (z1_row) store_z<CW>(p, z1_row, p.weight1, p.bias1, ucol, lcol, mu, rsigma, v);
            }
        }
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// The two row sums of a wide row (N > 1024 * bwd_cols(CW)), for the column slabs of dropout_norm_bwd_kernel: one row per workgroup
// of 1024, row_sums[r] = {sum(xhat * wdz), sum(wdz)}.  No decisions are needed for them
template <int CW>
__global__ __launch_bounds__(1024) void dropout_norm_bwd_row_sums_kernel(const fa_dropout_norm_bwd_params p, float *row_sums) {
    __shared__ float red[2][2][MAX_WAVES];
    const int N = p.N, tid = threadIdx.x, span = 1024 * CW;
    const int64_t r = blockIdx.x;
    const char *x_row = row_of(p.x, p.x_dtype, r, p.x_row_stride);
    const char *dz0_row = row_of(p.dz0, p.dz_dtype, r, p.dz0_row_stride);
    const char *dz1_row = p.weight1 ? row_of(p.dz1, p.dz_dtype, r, p.dz1_row_stride) : nullptr;
    const float mu = (p.flags & FA_DROPOUT_NORM_RMS) ? 0.0f : p.mu[r], rsigma = p.rsigma[r];
    float c[2] = {0.0f, 0.0f};
    for (int col = tid * CW; col < N; col += span) {
        float v[CW], g[CW], wv[CW], wd[CW];
        load_chunk<CW>(x_row, p.x_dtype, 0, col, v);
        load_chunk<CW>(dz0_row, p.dz_dtype, 0, col, g);
        load_chunk<CW>(p.weight0, p.weight_dtype, 0, col, wv);
#pragma unroll
        for (int i = 0; i < CW; ++i) wd[i] = wv[i] * g[i];
        if (dz1_row) {
            load_chunk<CW>(dz1_row, p.dz_dtype, 0, col, g);
            load_chunk<CW>(p.weight1, p.weight_dtype, 0, col, wv);
#pragma unroll
            for (int i = 0; i < CW; ++i) wd[i] += wv[i] * g[i];
        }
#pragma unroll
        for (int i = 0; i < CW; ++i) {
            c[0] += (v[i] - mu) * rsigma * wd[i];
            c[1] += wd[i];
        }
    }
    int phase = 0;
    team_sum<2, true>(c, false, red, phase);
    if (tid == 0) {
        row_sums[2 * r] = c[0];
        row_sums[2 * r + 1] = c[1];
    }
}

// A workgroup takes the rows of blockIdx.x and -- wide rows only -- the slab of 1024 * bwd_cols(CW) columns of blockIdx.y, with the
// row sums read from `row_sums`; a row that fits one slab (row_sums == NULL) has its sums taken here.  Column sums a0 .. a3:
// dw0, db0, then dw1 / db1 (weight1) or dcolscale (colscale) in a2; `sums` of them are written, as fp32 partial rows
// workspace[s][blockIdx.x][N]
template <int CW, bool DROP>
__global__ __launch_bounds__(1024) void dropout_norm_bwd_kernel(const fa_dropout_norm_bwd_params p, const Plan plan, int sums,
                                                                const float *row_sums) {
    constexpr int K = bwd_cols(CW) / CW;
    __shared__ float red[2][2][MAX_WAVES];
    const int N = p.N, ts = blockDim.x, tid = threadIdx.x, slab = blockIdx.y * (1024 * bwd_cols(CW));
    const bool rms = (p.flags & FA_DROPOUT_NORM_RMS) != 0;
    const float inv_n = 1.0f / (float)N;
    const uint32_t mix = DROP ? seed_mix(p.rng_state) : 0u;
    float a0[K * CW], a1[K * CW], a2[K * CW], a3[K * CW];
#pragma unroll
    for (int j = 0; j < K * CW; ++j) a0[j] = a1[j] = a2[j] = a3[j] = 0.0f;
    const int64_t first = (int64_t)blockIdx.x * plan.rows_per_wg;
    const int64_t last = first + plan.rows_per_wg < p.M ? first + plan.rows_per_wg : p.M;
    int phase = 0;
    for (int64_t r = first; r < last; ++r) {
        const char *x_row = row_of(p.x, p.x_dtype, r, p.x_row_stride);
        const char *dz0_row = row_of(p.dz0, p.dz_dtype, r, p.dz0_row_stride);
        const char *dz1_row = p.weight1 ? row_of(p.dz1, p.dz_dtype, r, p.dz1_row_stride) : nullptr;
        const float mu = rms ? 0.0f : p.mu[r], rsigma = p.rsigma[r];
        const float rs = p.rowscale ? load_one(p.rowscale, p.rowscale_dtype, r) : 1.0f;
        float xh[K * CW], wd[K * CW];
        float c[2] = {0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int ucol = slab + k * ts * CW, lcol = tid * CW;
#pragma unroll
            for (int i = 0; i < CW; ++i) xh[k * CW + i] = wd[k * CW + i] = 0.0f;
            if (ucol + lcol < N) {
                float v[CW], g[CW], wv[CW];
                load_chunk<CW>(x_row, p.x_dtype, ucol, lcol, v);
                load_chunk<CW>(dz0_row, p.dz_dtype, ucol, lcol, g);
                load_chunk<CW>(p.weight0, p.weight_dtype, ucol, lcol, wv);
#pragma unroll
                for (int i = 0; i < CW; ++i) {
                    const float xc = (v[i] - mu) * rsigma;
                    a0[k * CW + i] += g[i] * xc;
                    a1[k * CW + i] += g[i];
                    xh[k * CW + i] = xc;
                    wd[k * CW + i] = wv[i] * g[i];
                }
                if (dz1_row) {
                    load_chunk<CW>(dz1_row, p.dz_dtype, ucol, lcol, g);
                    load_chunk<CW>(p.weight1, p.weight_dtype, ucol, lcol, wv);
#pragma unroll
                    for (int i = 0; i < CW; ++i) {
                        a2[k * CW + i] += g[i] * xh[k * CW + i];
                        a3[k * CW + i] += g[i];
                        wd[k * CW + i] += wv[i] * g[i];
                    }
                }
#pragma unroll
                for (int i = 0; i < CW; ++i) {
                    c[0] += xh[k * CW + i] * wd[k * CW + i];
                    c[1] += wd[k * CW + i];
                }
            }
        }
        if (row_sums) {
            c[0] = row_sums[2 * r];
            c[1] = row_sums[2 * r + 1];
        } else {
            team_sum<2, true>(c, false, red, phase);
        }
        const float c1 = c[0] * inv_n, c2 = rms ? 0.0f : c[1] * inv_n;
        const uint32_t key0 = DROP ? row_key(mix, r, 0u) : 0u, key1 = DROP ? row_key(mix, r, 1u) : 0u;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int ucol = slab + k * ts * CW, lcol = tid * CW;
            if (ucol + lcol < N) {
                float dx[CW], d0[CW];
#pragma unroll
                for (int i = 0; i < CW; ++i) dx[i] = (wd[k * CW + i] - (xh[k * CW + i] * c1 + c2)) * rsigma;
                if (p.dx) {
                    float q[CW];
                    load_chunk<CW>(row_of(p.dx, p.x_dtype, r, p.dx_row_stride), p.x_dtype, ucol, lcol, q);
#pragma unroll
                    for (int i = 0; i < CW; ++i) dx[i] += q[i];
                }
                if (p.dresidual) store_chunk<CW>(row_of(p.dresidual, p.x_dtype, r, p.dresidual_row_stride), p.x_dtype, ucol, lcol, dx);
#pragma unroll
                for (int i = 0; i < CW; ++i) d0[i] = dx[i];
                if constexpr (DROP) {
                    bool keep[CW];
                    decide<CW>(key0, ucol + lcol, plan.keep_max, keep);
#pragma unroll
                    for (int i = 0; i < CW; ++i) d0[i] = keep[i] ? dx[i] * plan.inv_keep : 0.0f;
                }
                if (p.rowscale) {
#pragma unroll
                    for (int i = 0; i < CW; ++i) d0[i] *= rs;
                }
                if (p.colscale) {
                    float q[CW], cs[CW];
                    load_chunk<CW>(row_of(p.x0, p.x0_dtype, r, p.x0_row_stride), p.x0_dtype, ucol, lcol, q);
                    load_chunk<CW>(p.colscale, p.colscale_dtype, ucol, lcol, cs);
#pragma unroll
                    for (int i = 0; i < CW; ++i) {
                        a2[k * CW + i] += d0[i] * q[i];
                        d0[i] *= cs[i];
                    }
                }
                store_chunk<CW>(row_of(p.dx0, p.x0_dtype, r, p.dx0_row_stride), p.x0_dtype, ucol, lcol, d0);
                if (p.dx1) {
                    if constexpr (DROP) {
                        bool keep[CW];
                        decide<CW>(key1, ucol + lcol, plan.keep_max, keep);
#pragma unroll
                        for (int i = 0; i < CW; ++i) dx[i] = keep[i] ? dx[i] * plan.inv_keep : 0.0f;
                    }
                    store_chunk<CW>(row_of(p.dx1, p.x0_dtype, r, p.dx1_row_stride), p.x0_dtype, ucol, lcol, dx);
                }
            }
        }
    }
    float *part = static_cast<float *>(p.workspace) + (int64_t)blockIdx.x * N;
    const int64_t slot = (int64_t)gridDim.x * N;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int ucol = slab + k * ts * CW, lcol = tid * CW;
        if (ucol + lcol < N) {
            float s[CW];
#pragma unroll
            for (int i = 0; i < CW; ++i) s[i] = a0[k * CW + i];
            store_chunk<CW>(part, FA_DTYPE_FP32, ucol, lcol, s);
#pragma unroll
            for (int i = 0; i < CW; ++i) s[i] = a1[k * CW + i];
            store_chunk<CW>(part + slot, FA_DTYPE_FP32, ucol, lcol, s);
            if (sums > 2) {
#pragma unroll
                for (int i = 0; i < CW; ++i) s[i] = a2[k * CW + i];
                store_chunk<CW>(part + 2 * slot, FA_DTYPE_FP32, ucol, lcol, s);
            }
            if (sums > 3) {
#pragma unroll
                for (int i = 0; i < CW; ++i) s[i] = a3[k * CW + i];
                store_chunk<CW>(part + 3 * slot, FA_DTYPE_FP32, ucol, lcol, s);
            }
        }
    }
}

struct Reduce {
    void *dst[MAX_SUMS];  // NULL: not wanted
    int32_t dtype[MAX_SUMS];
};

// dst[s][col] = sum over the P partial rows of sum s, in the fixed order of reduce_partial_rows
__global__ __launch_bounds__(1024) void dropout_norm_reduce_kernel(const float *workspace, int P, int N, int sums, const Reduce out) {
    __shared__ float comb[MAX_WAVES][REDUCE_COLS];
#pragma unroll
    for (int which = 0; which < MAX_SUMS; ++which) {
        if (which >= sums || !out.dst[which]) continue;
        reduce_partial_rows(workspace + (int64_t)which * P * N, P, N, out.dst[which], out.dtype[which], comb);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// a tensor of rows that are N wide, no element tail
bool rows_16_bytes(const void *q, int dt, int64_t stride, int N) { return fa_row::rows_16_bytes(q, dt, stride) && vector_16_bytes(q, dt, N); }
bool mask_16_bytes(const void *q, int N) { return !q || (aligned_to(q, 16) && N % 16 == 0); }

struct Launch {
    int cw;     // 8 / 4: 16-byte accesses of x0; 1: element accesses
    bool wide;  // rows of more than 1024 * cols columns
    int threads;
    int grid;   // workgroups of plan.rows_per_wg rows
    int slabs;  // grid.y: the column slabs of a wide backward, else 1
    Plan plan;
};

// the shape of a launch over M rows of N columns; `vec`: what the operands allow
Launch launch_shape(int64_t M, int N, int x0_dtype, bool vec, bool backward, float p_dropout) {
    Launch l;
    l.cw = !vec ? 1 : x0_dtype == FA_DTYPE_FP32 ? 4 : 8;
    const int cols = backward ? bwd_cols(l.cw) : fwd_cols(l.cw);  // per thread, unless wide
    l.wide = N > 1024 * cols;
    l.slabs = backward && l.wide ? (N + 1024 * cols - 1) / (1024 * cols) : 1;
    // (the workgroup sizes of fa_norm.hip, its wavefront team being a workgroup of one wavefront here: with p = 0 the forward
    // adds a row of a 16-bit x0 in the same order)
    l.threads = N <= WAVE * cols ? WAVE : N <= 256 * cols ? 256 : N <= 512 * cols ? 512 : 1024;
    int64_t rows;
    if (backward) {  // (a function of M alone: the partial count must not depend on the access shape)
        rows = (M + BWD_PARTIALS - 1) / BWD_PARTIALS;
        if (rows < BWD_MIN_ROWS) rows = BWD_MIN_ROWS;
    } else if (l.wide) {  // one row per workgroup
        rows = 1;
    } else {  // enough rows to pay for reading weight and bias, enough workgroups to fill the device
        rows = M / 2048;
        rows = rows < 1 ? 1 : rows > 8 ? 8 : rows;
    }
    l.plan.rows_per_wg = (int32_t)rows;
    l.plan.wide = !backward && l.wide;
    // (255 (1 - p) in double: p = 0.9f is a little above 0.9, and the grid value is that of the p the caller gave)
    l.plan.keep_max = (uint32_t)(255.0 * (1.0 - (double)p_dropout));
    l.plan.inv_keep = (float)(1.0 / (1.0 - (double)p_dropout));
    l.grid = (int)((M + rows - 1) / rows);
    return l;
}

Launch fwd_launch(const fa_dropout_norm_fwd_params *p) {
    const int N = p->N;
    const bool vec = rows_16_bytes(p->x0, p->x0_dtype, p->x0_row_stride, N) && rows_16_bytes(p->x1, p->x0_dtype, p->x1_row_stride, N) &&
                     rows_16_bytes(p->residual, p->residual_dtype, p->residual_row_stride, N) &&
                     rows_16_bytes(p->z0, p->z_dtype, p->z0_row_stride, N) &&
                     rows_16_bytes(p->weight1 ? p->z1 : nullptr, p->z_dtype, p->z1_row_stride, N) &&
                     rows_16_bytes(p->x, p->x_dtype, p->x_row_stride, N) && vector_16_bytes(p->weight0, p->weight_dtype, N) &&
                     vector_16_bytes(p->bias0, p->weight_dtype, N) && vector_16_bytes(p->weight1, p->weight_dtype, N) &&
                     vector_16_bytes(p->weight1 ? p->bias1 : nullptr, p->weight_dtype, N) &&
                     vector_16_bytes(p->colscale, p->colscale_dtype, N) &&
                     (p->p_dropout <= 0.0f || (mask_16_bytes(p->dmask0, N) && mask_16_bytes(p->x1 ? p->dmask1 : nullptr, N)));
    return launch_shape(p->M, N, p->x0_dtype, vec, false, p->p_dropout);
}

Launch bwd_launch(const fa_dropout_norm_bwd_params *p) {
    const int N = p->N;
    const bool vec = rows_16_bytes(p->dz0, p->dz_dtype, p->dz0_row_stride, N) &&
                     rows_16_bytes(p->weight1 ? p->dz1 : nullptr, p->dz_dtype, p->dz1_row_stride, N) &&
                     rows_16_bytes(p->dx, p->x_dtype, p->dx_row_stride, N) && rows_16_bytes(p->x, p->x_dtype, p->x_row_stride, N) &&
                     rows_16_bytes(p->colscale ? p->x0 : nullptr, p->x0_dtype, p->x0_row_stride, N) &&
                     rows_16_bytes(p->dx0, p->x0_dtype, p->dx0_row_stride, N) && rows_16_bytes(p->dx1, p->x0_dtype, p->dx1_row_stride, N) &&
                     rows_16_bytes(p->dresidual, p->x_dtype, p->dresidual_row_stride, N) &&
                     vector_16_bytes(p->weight0, p->weight_dtype, N) && vector_16_bytes(p->weight1, p->weight_dtype, N) &&
                     vector_16_bytes(p->colscale, p->colscale_dtype, N);
    return launch_shape(p->M, N, p->x0_dtype, vec, true, p->p_dropout);
}

int bwd_sums(const fa_dropout_norm_bwd_params *p) { return p->weight1 ? 4 : p->colscale ? 3 : 2; }

void fill_plan(const Launch &l, float p_dropout, bool two_weights, int sums, fa_dropout_norm_plan *plan) {
    plan->cw = l.cw;
    plan->threads = l.wide ? 1024 : l.threads;
    plan->wide = l.wide;
    plan->dropout = p_dropout > 0.0f;
    plan->two_weights = two_weights;
    plan->sums = sums;
    plan->rows_per_wg = l.plan.rows_per_wg;
    plan->grid_x = l.grid;
    plan->grid_y = l.slabs;
}

int check_shape(int64_t M, int N, int x0_dtype, int x_dtype, bool backward) {
    if (M < 0 || N < 1) return FA_ERR_BAD_SHAPE;
    // (the wide forms take one row per workgroup in grid.x)
    if (N > 1024 * (backward ? MIN_BWD_COLS : MIN_FWD_COLS) && M > INT32_MAX) return FA_ERR_BAD_SHAPE;
    if ((int64_t)N * esize(x0_dtype) > FA_NORM_MAX_ROW_BYTES || (int64_t)N * esize(x_dtype) > FA_NORM_MAX_ROW_BYTES)
        return FA_ERR_BAD_SHAPE;
    if (M > ((int64_t)1 << 33)) return FA_ERR_BAD_SHAPE;  // (the grid: at least 8 rows per workgroup from M = 2^14)
    return FA_OK;
}

bool bad_p(float p) { return !(p >= 0.0f && p < 1.0f); }

}  // namespace

extern "C" {

uint32_t fa_dropout_norm_fwd_params_size(void) { return (uint32_t)sizeof(fa_dropout_norm_fwd_params); }
uint32_t fa_dropout_norm_bwd_params_size(void) { return (uint32_t)sizeof(fa_dropout_norm_bwd_params); }

int fa_dropout_norm_fwd_validate(const fa_dropout_norm_fwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_dropout_norm_fwd_params)) return FA_ERR_BAD_ABI;
    if (!known_dtype(p->x0_dtype) || !known_dtype(p->weight_dtype) || !known_dtype(p->z_dtype)) return FA_ERR_BAD_DTYPE;
    if (p->rowscale && !known_dtype(p->rowscale_dtype)) return FA_ERR_BAD_DTYPE;
    if (p->colscale && !known_dtype(p->colscale_dtype)) return FA_ERR_BAD_DTYPE;
    if (p->x_dtype != p->x0_dtype && p->x_dtype != FA_DTYPE_FP32) return FA_ERR_BAD_DTYPE;
    if (p->residual && p->residual_dtype != p->x_dtype) return FA_ERR_BAD_DTYPE;  // (the stream keeps the residual's dtype)
    if (bad_p(p->p_dropout)) return FA_ERR_BAD_SHAPE;
    const int st = check_shape(p->M, p->N, p->x0_dtype, p->x_dtype, false);
    if (st != FA_OK) return st;
    if (!p->x0 || !p->weight0 || !p->z0 || !p->rsigma || (!(p->flags & FA_DROPOUT_NORM_RMS) && !p->mu)) return FA_ERR_NULL_POINTER;
    if (p->weight1 && !p->z1) return FA_ERR_NULL_POINTER;
    if (p->p_dropout > 0.0f && !p->rng_state) return FA_ERR_NULL_POINTER;
    if ((p->x1 || p->weight1) && (p->rowscale || p->colscale)) return FA_ERR_UNSUPPORTED;
    if (p->bias1 && !p->weight1) return FA_ERR_UNSUPPORTED;
    // a mask is of a decision that is drawn
    if ((p->dmask0 || p->dmask1) && !(p->p_dropout > 0.0f)) return FA_ERR_UNSUPPORTED;
    if (p->dmask1 && !p->x1) return FA_ERR_UNSUPPORTED;
    // element accesses keep their natural alignment
    if (!aligned_to(p->x0, esize(p->x0_dtype)) || !aligned_to(p->x1, esize(p->x0_dtype)) ||
        !aligned_to(p->residual, esize(p->residual_dtype)) || !aligned_to(p->z0, esize(p->z_dtype)) ||
        !aligned_to(p->z1, esize(p->z_dtype)) || !aligned_to(p->x, esize(p->x_dtype)) ||
        !aligned_to(p->weight0, esize(p->weight_dtype)) || !aligned_to(p->bias0, esize(p->weight_dtype)) ||
        !aligned_to(p->weight1, esize(p->weight_dtype)) || !aligned_to(p->bias1, esize(p->weight_dtype)) ||
        !aligned_to(p->rowscale, esize(p->rowscale_dtype)) || !aligned_to(p->colscale, esize(p->colscale_dtype)) ||
        !aligned_to(p->rng_state, 8) || !aligned_to(p->mu, 4) || !aligned_to(p->rsigma, 4))
        return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int fa_dropout_norm_fwd(const fa_dropout_norm_fwd_params *p, void *stream_) {
    const int st = fa_dropout_norm_fwd_validate(p);
    if (st != FA_OK) return st;
    if (p->M == 0) return FA_OK;  // (no zero grid)
    const Launch l = fwd_launch(p);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(l.grid), block(l.wide ? 1024 : l.threads);
#define FA_DN_FWD_LAUNCH(CW)                                                                                         \
    do {                                                                                                             \
        if (p->p_dropout > 0.0f) hipLaunchKernelGGL((dropout_norm_fwd_kernel<CW, true>), grid, block, 0, stream, *p, l.plan); \
        else hipLaunchKernelGGL((dropout_norm_fwd_kernel<CW, false>), grid, block, 0, stream, *p, l.plan);          \
    } while (0)
    if (l.cw == 8) FA_DN_FWD_LAUNCH(8);
    else if (l.cw == 4) FA_DN_FWD_LAUNCH(4);
    else FA_DN_FWD_LAUNCH(1);
#undef FA_DN_FWD_LAUNCH
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

// workspace: `sums` times the partials [P][N], then -- rows that are wide with some access shape -- the row sums [M][2]: a
// function of the shape, not of the operands' alignment
uint64_t fa_dropout_norm_bwd_workspace_bytes(const fa_dropout_norm_bwd_params *p) {
    if (!p || p->M <= 0 || p->N < 1) return 0;
    const uint64_t P = (uint64_t)launch_shape(p->M, p->N, FA_DTYPE_BF16, false, true, 0.0f).grid;
    const uint64_t partials = P * (uint64_t)p->N * bwd_sums(p) * sizeof(float);
    return partials + (p->N > 1024 * MIN_BWD_COLS ? (uint64_t)p->M * 2 * sizeof(float) : 0);
}

int fa_dropout_norm_fwd_plan(const fa_dropout_norm_fwd_params *p, fa_dropout_norm_plan *plan) {
    const int st = fa_dropout_norm_fwd_validate(p);
    if (st != FA_OK) return st;
    if (!plan) return FA_ERR_NULL_POINTER;
    fill_plan(fwd_launch(p), p->p_dropout, p->weight1 != nullptr, 0, plan);
    return FA_OK;
}

int fa_dropout_norm_bwd_validate(const fa_dropout_norm_bwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_dropout_norm_bwd_params)) return FA_ERR_BAD_ABI;
    if (!known_dtype(p->x_dtype) || !known_dtype(p->dz_dtype) || !known_dtype(p->weight_dtype) || !known_dtype(p->x0_dtype))
        return FA_ERR_BAD_DTYPE;
    if (p->rowscale && !known_dtype(p->rowscale_dtype)) return FA_ERR_BAD_DTYPE;
    if (p->colscale && !known_dtype(p->colscale_dtype)) return FA_ERR_BAD_DTYPE;
    if (p->x_dtype != p->x0_dtype && p->x_dtype != FA_DTYPE_FP32) return FA_ERR_BAD_DTYPE;
    if (bad_p(p->p_dropout)) return FA_ERR_BAD_SHAPE;
    const int st = check_shape(p->M, p->N, p->x0_dtype, p->x_dtype, true);
    if (st != FA_OK) return st;
    if (!p->x || !p->dz0 || !p->weight0 || !p->rsigma || !p->dx0 || !p->dw0 || (!(p->flags & FA_DROPOUT_NORM_RMS) && !p->mu))
        return FA_ERR_NULL_POINTER;
    if (p->weight1 && (!p->dz1 || !p->dw1)) return FA_ERR_NULL_POINTER;
    if (p->colscale && (!p->x0 || !p->dcolscale)) return FA_ERR_NULL_POINTER;
    if (p->p_dropout > 0.0f && !p->rng_state) return FA_ERR_NULL_POINTER;
    if ((p->dx1 || p->weight1) && (p->rowscale || p->colscale)) return FA_ERR_UNSUPPORTED;
    if ((p->dw1 || p->db1) && !p->weight1) return FA_ERR_UNSUPPORTED;
    if (p->dcolscale && !p->colscale) return FA_ERR_UNSUPPORTED;
    const uint64_t need = fa_dropout_norm_bwd_workspace_bytes(p);
    if (need > 0 && (!p->workspace || p->workspace_bytes < need)) return FA_ERR_WORKSPACE;
    if (!aligned_to(p->workspace, 16)) return FA_ERR_BAD_STRIDE;
    if (!aligned_to(p->dz0, esize(p->dz_dtype)) || !aligned_to(p->dz1, esize(p->dz_dtype)) || !aligned_to(p->dx, esize(p->x_dtype)) ||
        !aligned_to(p->x, esize(p->x_dtype)) || !aligned_to(p->x0, esize(p->x0_dtype)) || !aligned_to(p->dx0, esize(p->x0_dtype)) ||
        !aligned_to(p->dx1, esize(p->x0_dtype)) || !aligned_to(p->dresidual, esize(p->x_dtype)) ||
        !aligned_to(p->weight0, esize(p->weight_dtype)) || !aligned_to(p->weight1, esize(p->weight_dtype)) ||
        !aligned_to(p->dw0, esize(p->weight_dtype)) || !aligned_to(p->db0, esize(p->weight_dtype)) ||
        !aligned_to(p->dw1, esize(p->weight_dtype)) || !aligned_to(p->db1, esize(p->weight_dtype)) ||
        !aligned_to(p->rowscale, esize(p->rowscale_dtype)) || !aligned_to(p->colscale, esize(p->colscale_dtype)) ||
        !aligned_to(p->dcolscale, esize(p->colscale_dtype)) || !aligned_to(p->rng_state, 8) || !aligned_to(p->mu, 4) ||
        !aligned_to(p->rsigma, 4))
        return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int fa_dropout_norm_bwd_plan(const fa_dropout_norm_bwd_params *p, fa_dropout_norm_plan *plan) {
    const int st = fa_dropout_norm_bwd_validate(p);
    if (st != FA_OK) return st;
    if (!plan) return FA_ERR_NULL_POINTER;
    fill_plan(bwd_launch(p), p->p_dropout, p->weight1 != nullptr, bwd_sums(p), plan);
    return FA_OK;
}

int fa_dropout_norm_bwd(const fa_dropout_norm_bwd_params *p, void *stream_) {
    const int st = fa_dropout_norm_bwd_validate(p);
    if (st != FA_OK) return st;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int sums = bwd_sums(p);
    int partials = 0;
    if (p->M > 0) {
        const Launch l = bwd_launch(p);
        partials = l.grid;
        float *row_sums = nullptr;
        const dim3 grid(l.grid, l.slabs), block(l.wide ? 1024 : l.threads);
        if (l.wide) {  // the row sums first, then one workgroup per row block and slab of 1024 * bwd_cols(CW) columns
            row_sums = static_cast<float *>(p->workspace) + (int64_t)l.grid * p->N * sums;
#define FA_DN_BWD_SUMS_LAUNCH(CW) \
    hipLaunchKernelGGL((dropout_norm_bwd_row_sums_kernel<CW>), dim3((unsigned)p->M), dim3(1024), 0, stream, *p, row_sums)
            if (l.cw == 8) FA_DN_BWD_SUMS_LAUNCH(8);
            else if (l.cw == 4) FA_DN_BWD_SUMS_LAUNCH(4);
            else FA_DN_BWD_SUMS_LAUNCH(1);
#undef FA_DN_BWD_SUMS_LAUNCH
            if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
        }
#define FA_DN_BWD_LAUNCH(CW)                                                                                                      \
    do {                                                                                                                          \
        if (p->p_dropout > 0.0f)                                                                                                  \
            hipLaunchKernelGGL((dropout_norm_bwd_kernel<CW, true>), grid, block, 0, stream, *p, l.plan, sums, (const float *)row_sums);  \
        else                                                                                                                      \
            hipLaunchKernelGGL((dropout_norm_bwd_kernel<CW, false>), grid, block, 0, stream, *p, l.plan, sums, (const float *)row_sums); \
    } while (0)
        if (l.cw == 8) FA_DN_BWD_LAUNCH(8);
        else if (l.cw == 4) FA_DN_BWD_LAUNCH(4);
        else FA_DN_BWD_LAUNCH(1);
#undef FA_DN_BWD_LAUNCH
        if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    }
    // (no rows: no partials, and the sums are zero)
    Reduce out;
    out.dst[0] = p->dw0; out.dst[1] = p->db0;
    out.dst[2] = p->weight1 ? p->dw1 : p->dcolscale; out.dst[3] = p->db1;
    out.dtype[0] = out.dtype[1] = out.dtype[3] = p->weight_dtype;
    out.dtype[2] = p->weight1 ? p->weight_dtype : p->colscale_dtype;
    hipLaunchKernelGGL(dropout_norm_reduce_kernel, dim3((p->N + REDUCE_COLS - 1) / REDUCE_COLS), dim3(WAVE * MAX_WAVES), 0, stream,
                       static_cast<const float *>(p->workspace), partials, p->N, sums, out);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

}  // extern "C"
