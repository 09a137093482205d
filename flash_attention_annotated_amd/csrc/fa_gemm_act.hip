// fa_gemm_act.hip — fa_gemm_act_fwd / fa_gemm_act_dgrad (include/fa_gemm_act.h): a 16-bit GEMM on MFMA with the bias, the
// activation (forward) or the activation's derivative and the dbias sums (dgrad) in its epilogue.  A translation unit of its
// own: no kernel comes from another unit or goes to one, because the kernel set of every unit is pinned by its tests.  That
// rule is about kernels: the activations are the inline functions of fa_act_math.h, the one definition this unit and
// fa_act.hip have (tests/test_gemm_act_gpu.py pins the two units to each other bit for bit).  Of fa_rowwise.h this unit needs
// nothing: its accesses are 16-byte chunks of one 16-bit dtype, a template argument here.
//
// Both directions are C(M, N) = A(M, K) · B, A row-major: forward B[k][n] = weight[n][k] (rows of K), dgrad B[k][n] =
// weight[k][n] (rows of N).  A workgroup of 256 threads (4 waves as 2 x 2) owns one BM x 128 tile of C, BM = 128 or (M <= 64)
// 64, and walks K in steps of 64.  A step's A and B tiles go global -> registers -> LDS as 16-byte chunks, two LDS buffers: the
// loads of step t + 1 are issued before the MFMAs of step t and written to the other buffer after them, one barrier per step.
// Both LDS images are [row][64 k] with 128-byte rows, the 16-byte chunk c of row r at chunk c ^ swz(r): the forward's weight
// tile is copied as it is, the dgrad's is transposed on the way (a thread loads 4 k-rows of 8 columns and writes 8 columns of
// 4 k).  Every global load is issued at a clamped, in-bounds address and replaced by zero where it is past an edge of M, N or
// K, so ragged tiles add zeros.  Each wave computes (BM / 2) x 64 with v_mfma_f32_32x32x16_{bf16,f16}.
// Epilogue: a 32 x 32 accumulator block goes through a wave-private LDS patch, so that a lane holds 8 consecutive columns of
// a row: bias, activation, rounding and 16-byte stores happen there.  Dgrad with dbias: the column sums of the unrounded
// products are reduced over the lanes by shuffles, over the two wave rows through LDS in a fixed order, and written as
// partial row tile_m; gemm_act_dbias_reduce_kernel adds the partial rows in their order.  No atomics.
// Block -> tile: blockIdx.x is made contiguous per XCD (a bijective remap) and then walks GROUP_M row tiles per column tile.
#include "../../include/fa_gemm_act.h"
#include "fa_act_math.h"

namespace {

using namespace fa_act_math;

constexpr int THREADS = 256;
constexpr int BN = 128;      // columns of a tile
constexpr int BK = 64;       // a K-step: 128-byte rows in LDS
constexpr int BM_MAIN = 128, BM_SMALL = 64;
constexpr int SMALL_M = 64;  // M <= SMALL_M: the 64-row tile
constexpr int GROUP_M = 8;
constexpr int EP_PITCH = 36;                          // floats of a row of a wave's 32 x 32 epilogue patch (16-byte rows, off the banks)
constexpr int EP_FLOATS = 4 * 32 * EP_PITCH;          // the four patches; the dbias sums of the two wave rows follow
constexpr int REDUCE_THREADS = 256;

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// what a kernel reads, either direction
struct GemmArgs {
    const char *a;       // (M, K)
    const char *b;       // forward (N, K), dgrad (K, N)
    const char *bias;    // forward: (N) or null
    const char *act_in;  // dgrad: act_input (M, N) or null
    char *out;           // out / grad_in (M, N)
    char *act_out;       // forward: act_input (M, N) or null
    float *partials;     // dgrad: partial rows of dbias or null
    int64_t a_stride, b_stride, out_stride, act_stride;  // in elements
    int64_t M;
    int32_t N, K, activation, tiles_m, tiles_n;
};

// ---- 16-byte chunks of 8 elements ------------------------------------------------------------------------------------------------
template <int DT>
__device__ __forceinline__ void unpack8(const uint4 f, float (&v)[8]) {
    const uint32_t w[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (DT == FA_DTYPE_BF16) {
            v[2 * i] = __uint_as_float(w[i] << 16);
            v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        } else {
            v[2 * i] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[i] & 0xffffu));
            v[2 * i + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[i] >> 16));
        }
    }
}

// one rounding to nearest even
template <int DT>
__device__ __forceinline__ uint4 pack8(const float (&v)[8]) {
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if constexpr (DT == FA_DTYPE_BF16) h[i] = __builtin_bit_cast(uint16_t, (__bf16)v[i]);
        else h[i] = __builtin_bit_cast(uint16_t, (_Float16)v[i]);
    }
    return make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
}

template <int DT>
__device__ __forceinline__ f32x16 mfma(const uint4 a, const uint4 b, const f32x16 c) {
    if constexpr (DT == FA_DTYPE_BF16)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// the chunk swizzle of an LDS row: a permutation of the 8 chunks within every 8 consecutive rows (the fragment reads), and
// distinct for rows 8 apart (the dgrad's transposing writes)
__device__ __forceinline__ int swz(int row) { return (row ^ (row >> 3)) & 7; }

// byte offset of chunk `c` (0..7) of row `row` in an image of 128-byte rows
__device__ __forceinline__ int lds_chunk(int row, int c) { return row * (BK * 2) + ((c ^ swz(row)) << 4); }

// a clamped 16-byte load, zero where `valid` is false (the address is in bounds either way)
__device__ __forceinline__ uint4 load16(const char *base, int64_t row, int64_t stride, int64_t col, bool valid) {
    const uint4 v = *reinterpret_cast<const uint4 *>(base + (row * stride + col) * 2);
    return valid ? v : make_uint4(0u, 0u, 0u, 0u);
}

template <int DT, int BM, bool DGRAD>
__device__ __forceinline__ void gemm_tile(const GemmArgs &g) {
    constexpr int WM = BM / 2, MI = WM / 32, NI = 2;  // a wave: WM x 64 as MI x NI blocks of 32 x 32
    constexpr int A_IT = BM / 32, B_IT = BN / 32;     // 16-byte chunks of a step's tiles per thread
    constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, BUF_BYTES = A_BYTES + B_BYTES;
    static_assert(2 * BUF_BYTES >= (EP_FLOATS + 2 * BN) * 4, "the epilogue reuses the staging buffers");
    __shared__ __attribute__((aligned(16))) char lds[2 * BUF_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;

    // block -> tile: contiguous per XCD, then GROUP_M row tiles per column tile
    const uint32_t nwg = (uint32_t)g.tiles_m * (uint32_t)g.tiles_n, orig = blockIdx.x, xcd = orig & 7u, q = nwg >> 3, r = nwg & 7u;
    const uint32_t id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
    const uint32_t width = (uint32_t)GROUP_M * (uint32_t)g.tiles_n, first = id / width * GROUP_M;
    const uint32_t gsize = (uint32_t)g.tiles_m - first < (uint32_t)GROUP_M ? (uint32_t)g.tiles_m - first : (uint32_t)GROUP_M;
    const uint32_t tile_m = first + id % width % gsize, tile_n = id % width / gsize;
    const int64_t m0 = (int64_t)tile_m * BM;
    const int n0 = (int)tile_n * BN;

    // the staging of A (and of the forward's B): chunk (tid & 7) of rows (tid >> 3) + 32 i
    const int st_row = tid >> 3, st_c = tid & 7;
    // the dgrad's B: columns n0 + 8 (tid & 15) ... + 7 of k-rows 4 (tid >> 4) + i
    const int tb_n = tid & 15, tb_k = tid >> 4;

    uint4 ra[A_IT], rb[B_IT];
    auto load_tiles = [&](int kt) {
        const int k0 = kt * BK;
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
            const int64_t row = m0 + st_row + 32 * i;
            const int k = k0 + st_c * 8;
            const bool valid = row < g.M && k < g.K;
            ra[i] = load16(g.a, row < g.M ? row : g.M - 1, g.a_stride, k < g.K ? k : 0, valid);
        }
        if constexpr (!DGRAD) {
#pragma unroll
            for (int i = 0; i < B_IT; ++i) {
                const int n = n0 + st_row + 32 * i, k = k0 + st_c * 8;
                const bool valid = n < g.N && k < g.K;
                rb[i] = load16(g.b, n < g.N ? n : g.N - 1, g.b_stride, k < g.K ? k : 0, valid);
            }
        } else {
            const int n = n0 + tb_n * 8;
#pragma unroll
            for (int i = 0; i < B_IT; ++i) {
                const int k = k0 + tb_k * 4 + i;
                const bool valid = n < g.N && k < g.K;
                rb[i] = load16(g.b, k < g.K ? k : g.K - 1, g.b_stride, n < g.N ? n : 0, valid);
            }
        }
    };
    auto store_tiles = [&](int buf) {
        char *as = lds + buf * BUF_BYTES, *bs = as + A_BYTES;
#pragma unroll
        for (int i = 0; i < A_IT; ++i) *reinterpret_cast<uint4 *>(as + lds_chunk(st_row + 32 * i, st_c)) = ra[i];
        if constexpr (!DGRAD) {
#pragma unroll
            for (int i = 0; i < B_IT; ++i) *reinterpret_cast<uint4 *>(bs + lds_chunk(st_row + 32 * i, st_c)) = rb[i];
        } else {
            // rb[i] holds k-row i of 8 columns: column j gets its 4 k as 8 bytes at k offset 4 tb_k of row 8 tb_n + j
            const uint32_t w[4][4] = {{rb[0].x, rb[0].y, rb[0].z, rb[0].w}, {rb[1].x, rb[1].y, rb[1].z, rb[1].w},
                                      {rb[2].x, rb[2].y, rb[2].z, rb[2].w}, {rb[3].x, rb[3].y, rb[3].z, rb[3].w}};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                uint2 v;
                if (j & 1) {
                    v.x = (w[0][j >> 1] >> 16) | (w[1][j >> 1] & 0xffff0000u);
                    v.y = (w[2][j >> 1] >> 16) | (w[3][j >> 1] & 0xffff0000u);
                } else {
                    v.x = (w[0][j >> 1] & 0xffffu) | (w[1][j >> 1] << 16);
                    v.y = (w[2][j >> 1] & 0xffffu) | (w[3][j >> 1] << 16);
                }
                *reinterpret_cast<uint2 *>(bs + lds_chunk(tb_n * 8 + j, tb_k >> 1) + (tb_k & 1) * 8) = v;
            }
        }
    };

    f32x16 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.0f;

    const int nk = (g.K + BK - 1) / BK;
    load_tiles(0);
    store_tiles(0);
    __syncthreads();
    const int fr = lane & 31, fh = lane >> 5;  // a fragment: row fr, k = 8 fh + j of a 16-deep MFMA step
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;
        if (more) load_tiles(kt + 1);
        const char *as = lds + (kt & 1) * BUF_BYTES, *bs = as + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            uint4 af[MI], bf[NI];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) af[mi] = *reinterpret_cast<const uint4 *>(as + lds_chunk(wr * WM + mi * 32 + fr, ks * 2 + fh));
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) bf[ni] = *reinterpret_cast<const uint4 *>(bs + lds_chunk(wc * 64 + ni * 32 + fr, ks * 2 + fh));
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = mfma<DT>(af[mi], bf[ni], acc[mi][ni]);
        }
        if (more) store_tiles((kt + 1) & 1);
        __syncthreads();  // the other buffer is written, and this one is free for the step after
    }

    // ---- epilogue: (the last barrier of the loop has passed: the staging buffers are free)
    float *ep = reinterpret_cast<float *>(lds) + wave * (32 * EP_PITCH);
    float *dsum = reinterpret_cast<float *>(lds) + EP_FLOATS;  // [2 wave rows][BN]
    const int cc = lane & 3;  // this lane's 8 columns of a 32-column block, for every row it visits
    float csum[NI][8] = {};
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            // C of a 32 x 32 MFMA: column lane & 31, row (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
#pragma unroll
            for (int e = 0; e < 16; ++e) ep[((e & 3) + 8 * (e >> 2) + 4 * fh) * EP_PITCH + fr] = acc[mi][ni][e];
            __syncthreads();
            const int col = n0 + wc * 64 + ni * 32 + cc * 8;
            float bias[8] = {};
            if constexpr (!DGRAD) {
                if (g.bias && col < g.N) unpack8<DT>(*reinterpret_cast<const uint4 *>(g.bias + (int64_t)col * 2), bias);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int prow = (lane >> 2) + 16 * i;
                const int64_t row = m0 + wr * WM + mi * 32 + prow;
                const bool valid = row < g.M && col < g.N;
                const float4 lo = *reinterpret_cast<const float4 *>(ep + prow * EP_PITCH + cc * 8);
                const float4 hi = *reinterpret_cast<const float4 *>(ep + prow * EP_PITCH + cc * 8 + 4);
                float s[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}, a[8], dg[8];
                if constexpr (!DGRAD) {
                    if (valid) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) s[e] += bias[e];
                        if (g.act_out) *reinterpret_cast<uint4 *>(g.act_out + (row * g.act_stride + col) * 2) = pack8<DT>(s);
                        eval_chunk(g.activation, s, bias, a, dg);  // (dg is not used: its arithmetic is dropped)
                        *reinterpret_cast<uint4 *>(g.out + (row * g.out_stride + col) * 2) = pack8<DT>(a);
                    }
                } else {
                    if (valid) {
                        if (g.act_in) {
                            float x[8];
                            unpack8<DT>(*reinterpret_cast<const uint4 *>(g.act_in + (row * g.act_stride + col) * 2), x);
                            eval_chunk(g.activation, x, s, a, dg);
                        } else {
#pragma unroll
                            for (int e = 0; e < 8; ++e) dg[e] = s[e];
                        }
                        *reinterpret_cast<uint4 *>(g.out + (row * g.out_stride + col) * 2) = pack8<DT>(dg);
#pragma unroll
                        for (int e = 0; e < 8; ++e) csum[ni][e] += dg[e];
                    }
                }
            }
            __syncthreads();
        }
    }
    if constexpr (DGRAD) {
        if (g.partials) {
            // the 16 lanes of one cc hold the rows: a fixed tree over them, then the two wave rows in their order
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float v = csum[ni][e];
                    v += __shfl_xor(v, 4);
                    v += __shfl_xor(v, 8);
                    v += __shfl_xor(v, 16);
                    v += __shfl_xor(v, 32);
                    if (lane < 4) dsum[wr * BN + wc * 64 + ni * 32 + cc * 8 + e] = v;
                }
            __syncthreads();
            const int col = n0 + tid * 4;
            if (tid < BN / 4 && col < g.N) {
                const float4 u = *reinterpret_cast<const float4 *>(dsum + tid * 4), v = *reinterpret_cast<const float4 *>(dsum + BN + tid * 4);
                *reinterpret_cast<float4 *>(g.partials + (int64_t)tile_m * g.N + col) = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
            }
        }
    }
}

template <int DT, int BM>
__global__ __launch_bounds__(THREADS) void gemm_act_fwd_kernel(const GemmArgs g) {
    gemm_tile<DT, BM, false>(g);
}

template <int DT, int BM>
__global__ __launch_bounds__(THREADS) void gemm_act_dgrad_kernel(const GemmArgs g) {
    gemm_tile<DT, BM, true>(g);
}

// dbias[c ... c + 7] = the sums of the P partial rows at those columns, in their order, cast once
__global__ __launch_bounds__(REDUCE_THREADS) void gemm_act_dbias_reduce_kernel(const float *partials, int P, int N, void *dbias, int dt) {
    const int64_t c = ((int64_t)blockIdx.x * REDUCE_THREADS + threadIdx.x) * 8;
    if (c >= N) return;
    float sum[8] = {};
    for (int64_t j = 0; j < P; ++j) {
        const float4 lo = *reinterpret_cast<const float4 *>(partials + j * N + c), hi = *reinterpret_cast<const float4 *>(partials + j * N + c + 4);
        sum[0] += lo.x; sum[1] += lo.y; sum[2] += lo.z; sum[3] += lo.w;
        sum[4] += hi.x; sum[5] += hi.y; sum[6] += hi.z; sum[7] += hi.w;
    }
    *reinterpret_cast<uint4 *>(static_cast<char *>(dbias) + c * 2) = dt == FA_DTYPE_BF16 ? pack8<FA_DTYPE_BF16>(sum) : pack8<FA_DTYPE_FP16>(sum);
}

// ---- host -------------------------------------------------------------------------------------------------------------------
bool half_dtype(int dt) { return dt == FA_DTYPE_FP16 || dt == FA_DTYPE_BF16; }
bool aligned16(const void *q) { return reinterpret_cast<uintptr_t>(q) % 16 == 0; }
// rows of `len` elements at a pitch of `stride`: 16-byte rows (one row needs no pitch)
bool rows_ok(int64_t stride, int64_t len, int64_t rows) { return rows <= 1 || (stride >= len && stride % 8 == 0); }

int64_t tile_rows(int64_t M) { return M <= SMALL_M ? BM_SMALL : BM_MAIN; }
int64_t tiles_of(int64_t n, int64_t tile) { return (n + tile - 1) / tile; }

// what both directions ask of the shape: every tile has an index below 2^31
int check_shape(int64_t M, int32_t N, int32_t K, int activation) {
    if (!known_activation(activation)) return FA_ERR_UNSUPPORTED;
    if (M < 0 || N < 8 || K < 8 || N % 8 || K % 8) return FA_ERR_BAD_SHAPE;
    if (tiles_of(M, tile_rows(M)) * tiles_of(N, BN) > INT32_MAX) return FA_ERR_BAD_SHAPE;
    return FA_OK;
}

// the launch of a valid call
fa_gemm_act_plan plan_of(int64_t M, int32_t N, int32_t K, int dtype, bool dgrad, bool dbias) {
    fa_gemm_act_plan l{};
    l.tile_m = (int32_t)tile_rows(M);
    l.tile_n = BN;
    l.tile_k = BK;
    l.threads = THREADS;
    l.tiles_m = (int32_t)tiles_of(M, l.tile_m);
    l.tiles_n = (int32_t)tiles_of(N, BN);
    l.grid_x = l.tiles_m * l.tiles_n;
    l.k_steps = (int32_t)tiles_of(K, BK);
    l.ragged_m = M % l.tile_m != 0;
    l.ragged_n = N % BN != 0;
    l.ragged_k = K % BK != 0;
    l.group_m = GROUP_M;
    l.partial_rows = dbias ? l.tiles_m : 0;
    l.reduce_grid_x = dbias && M > 0 ? (int32_t)tiles_of(N / 8, REDUCE_THREADS) : 0;
    l.dtype = dtype;
    l.dgrad = dgrad;
    return l;
}

template <int DT, int BM>
void launch(bool dgrad, const fa_gemm_act_plan &l, const GemmArgs &g, hipStream_t stream) {
    if (dgrad) hipLaunchKernelGGL((gemm_act_dgrad_kernel<DT, BM>), dim3(l.grid_x), dim3(THREADS), 0, stream, g);
    else hipLaunchKernelGGL((gemm_act_fwd_kernel<DT, BM>), dim3(l.grid_x), dim3(THREADS), 0, stream, g);
}

int launch_gemm(bool dgrad, const fa_gemm_act_plan &l, const GemmArgs &g, hipStream_t stream) {
    if (l.dtype == FA_DTYPE_BF16) {
        if (l.tile_m == BM_SMALL) launch<FA_DTYPE_BF16, BM_SMALL>(dgrad, l, g, stream);
        else launch<FA_DTYPE_BF16, BM_MAIN>(dgrad, l, g, stream);
    } else {
        if (l.tile_m == BM_SMALL) launch<FA_DTYPE_FP16, BM_SMALL>(dgrad, l, g, stream);
        else launch<FA_DTYPE_FP16, BM_MAIN>(dgrad, l, g, stream);
    }
    return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

}  // namespace

extern "C" {

uint32_t fa_gemm_act_fwd_params_size(void) { return (uint32_t)sizeof(fa_gemm_act_fwd_params); }
uint32_t fa_gemm_act_dgrad_params_size(void) { return (uint32_t)sizeof(fa_gemm_act_dgrad_params); }

int fa_gemm_act_fwd_validate(const fa_gemm_act_fwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_gemm_act_fwd_params)) return FA_ERR_BAD_ABI;
    const int dt = p->x_dtype;
    if (!half_dtype(dt) || p->weight_dtype != dt || p->out_dtype != dt || (p->bias && p->bias_dtype != dt) ||
        (p->act_input && p->act_input_dtype != dt))
        return FA_ERR_BAD_DTYPE;
    const int st = check_shape(p->M, p->N, p->K, p->activation);
    if (st != FA_OK) return st;
    if (!p->x || !p->weight || !p->out) return FA_ERR_NULL_POINTER;
    if (!aligned16(p->x) || !aligned16(p->weight) || !aligned16(p->out) || !aligned16(p->bias) || !aligned16(p->act_input))
        return FA_ERR_BAD_STRIDE;
    if (!rows_ok(p->x_row_stride, p->K, p->M) || !rows_ok(p->weight_row_stride, p->K, p->N) || !rows_ok(p->out_row_stride, p->N, p->M) ||
        (p->act_input && !rows_ok(p->act_input_row_stride, p->N, p->M)))
        return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int fa_gemm_act_fwd_plan(const fa_gemm_act_fwd_params *p, fa_gemm_act_plan *plan) {
    const int st = fa_gemm_act_fwd_validate(p);
    if (st != FA_OK) return st;
    if (!plan) return FA_ERR_NULL_POINTER;
    *plan = plan_of(p->M, p->N, p->K, p->x_dtype, false, false);
    return FA_OK;
}

int fa_gemm_act_fwd(const fa_gemm_act_fwd_params *p, void *stream) {
    const int st = fa_gemm_act_fwd_validate(p);
    if (st != FA_OK) return st;
    if (p->M == 0) return FA_OK;  // (no zero grid)
    GemmArgs g{};
    g.a = static_cast<const char *>(p->x);
    g.b = static_cast<const char *>(p->weight);
    g.bias = static_cast<const char *>(p->bias);
    g.out = static_cast<char *>(p->out);
    g.act_out = static_cast<char *>(p->act_input);
    g.a_stride = p->x_row_stride; g.b_stride = p->weight_row_stride; g.out_stride = p->out_row_stride; g.act_stride = p->act_input_row_stride;
    g.M = p->M; g.N = p->N; g.K = p->K; g.activation = p->activation;
    const fa_gemm_act_plan l = plan_of(p->M, p->N, p->K, p->x_dtype, false, false);
    g.tiles_m = l.tiles_m; g.tiles_n = l.tiles_n;
    return launch_gemm(false, l, g, static_cast<hipStream_t>(stream));
}

uint64_t fa_gemm_act_dgrad_workspace_bytes(const fa_gemm_act_dgrad_params *p) {
    if (!p || !p->dbias || p->M < 1 || p->N < 1) return 0;
    return (uint64_t)tiles_of(p->M, tile_rows(p->M)) * (uint64_t)p->N * sizeof(float);
}

int fa_gemm_act_dgrad_validate(const fa_gemm_act_dgrad_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_gemm_act_dgrad_params)) return FA_ERR_BAD_ABI;
    const int dt = p->grad_out_dtype;
    if (!half_dtype(dt) || p->weight_dtype != dt || p->grad_in_dtype != dt || (p->act_input && p->act_input_dtype != dt) ||
        (p->dbias && p->dbias_dtype != dt))
        return FA_ERR_BAD_DTYPE;
    const int st = check_shape(p->M, p->N, p->K, p->activation);
    if (st != FA_OK) return st;
    if (!p->grad_out || !p->weight || !p->grad_in || (!p->act_input && p->activation != FA_ACT_IDENTITY)) return FA_ERR_NULL_POINTER;
    if (!aligned16(p->grad_out) || !aligned16(p->weight) || !aligned16(p->grad_in) || !aligned16(p->act_input) || !aligned16(p->dbias))
        return FA_ERR_BAD_STRIDE;
    if (!rows_ok(p->grad_out_row_stride, p->K, p->M) || !rows_ok(p->weight_row_stride, p->N, p->K) || !rows_ok(p->grad_in_row_stride, p->N, p->M) ||
        (p->act_input && !rows_ok(p->act_input_row_stride, p->N, p->M)))
        return FA_ERR_BAD_STRIDE;
    const uint64_t need = fa_gemm_act_dgrad_workspace_bytes(p);
    if (need > 0 && (!p->workspace || p->workspace_bytes < need)) return FA_ERR_WORKSPACE;
    if (need > 0 && !aligned16(p->workspace)) return FA_ERR_BAD_STRIDE;
    return FA_OK;
}

int fa_gemm_act_dgrad_plan(const fa_gemm_act_dgrad_params *p, fa_gemm_act_plan *plan) {
    const int st = fa_gemm_act_dgrad_validate(p);
    if (st != FA_OK) return st;
    if (!plan) return FA_ERR_NULL_POINTER;
    *plan = plan_of(p->M, p->N, p->K, p->grad_out_dtype, true, p->dbias != nullptr);
    return FA_OK;
}

int fa_gemm_act_dgrad(const fa_gemm_act_dgrad_params *p, void *stream_) {
    const int st = fa_gemm_act_dgrad_validate(p);
    if (st != FA_OK) return st;
    if (p->M == 0) return FA_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    GemmArgs g{};
    g.a = static_cast<const char *>(p->grad_out);
    g.b = static_cast<const char *>(p->weight);
    g.act_in = p->activation == FA_ACT_IDENTITY ? nullptr : static_cast<const char *>(p->act_input);  // (act' = 1: nothing to read)
    g.out = static_cast<char *>(p->grad_in);
    g.partials = p->dbias ? static_cast<float *>(p->workspace) : nullptr;
    g.a_stride = p->grad_out_row_stride; g.b_stride = p->weight_row_stride; g.out_stride = p->grad_in_row_stride; g.act_stride = p->act_input_row_stride;
    g.M = p->M; g.N = p->N; g.K = p->K; g.activation = p->activation;
    const fa_gemm_act_plan l = plan_of(p->M, p->N, p->K, p->grad_out_dtype, true, p->dbias != nullptr);
    g.tiles_m = l.tiles_m; g.tiles_n = l.tiles_n;
    const int ls = launch_gemm(true, l, g, stream);
    if (ls != FA_OK) return ls;
    if (p->dbias) {
        hipLaunchKernelGGL(gemm_act_dbias_reduce_kernel, dim3(l.reduce_grid_x), dim3(REDUCE_THREADS), 0, stream,
                           static_cast<const float *>(p->workspace), l.partial_rows, p->N, p->dbias, p->dbias_dtype);
        if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    }
    return FA_OK;
}

}  // extern "C"
