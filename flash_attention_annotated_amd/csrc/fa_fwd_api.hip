// fa_fwd_api.hip — C-ABI entry points declared in include/fa_fwd.h.
//
// Host-side role of mha_fwd / mha_varlen_fwd (csrc/flash_attn/flash_api.cpp:350-512, 514-755),
// set_params_fprop (:26-159) and run_mha_fwd (:243-255): validate, fill the kernel params,
// pick the instantiation, launch on the caller's stream.  No allocation, no synchronisation.
// What every forward route does the same way -- the params fill, the window rule, the softmax scales, the split-KV workspace
// layout, the packed-row grid -- is in fa_fwd_internal.h.
#include "fa_fwd.h"
#include "fa_fwd_kernel.h"
#include "fa_fwd_kernel_w64.h"
#include "fa_fwd_kernel_fp8.h"
#include "fa_fwd_kernel_d256.h"
#include "fa_fwd_kernel_qv.h"
#include "fa_fwd_kernel_bs.h"
#include "fa_fwd_kernel_pk.h"
#include "fa_fwd_internal.h"
#include "fa_rotary.h"
#include "fa_launch.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>

namespace {

std::atomic<int> g_default_variant{0};
std::atomic<int> g_persist_mode{0};  // test hook: 0 = the library's choice, -1 = never the persistent kernel, 1 = whenever it can run

// ---- fp8 e4m3 -> bf16 expansion (exact), strided source -> contiguous (rows, heads, d) destination ------------------
// One thread = 8 elements (8-byte load, 16-byte store).  HBM-bound elementwise pass.
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__global__ void expand_fp8_kernel(const uint8_t *__restrict__ src, uint32_t *__restrict__ dst, int64_t rows,
                                  int rows_per_batch, int heads, int d, int64_t batch_stride, int64_t row_stride,
                                  int64_t head_stride) {
    const int chunks = d >> 3;
    const int64_t total = rows * heads * chunks;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % chunks);
        const int64_t rh = i / chunks;
        const int hd = (int)(rh % heads);
        const int64_t row = rh / heads;
        const int64_t b = rows_per_batch > 0 ? row / rows_per_batch : 0;
        const int64_t r = rows_per_batch > 0 ? row % rows_per_batch : row;
        const uint2 v = *reinterpret_cast<const uint2 *>(src + b * batch_stride + r * row_stride + hd * head_stride + c * 8);
        uint32_t out[4];
        const uint32_t w[2] = {v.x, v.y};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[k], false);
            const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[k], true);
            const bf16x2_t a = {(__bf16)lo[0], (__bf16)lo[1]};
            const bf16x2_t bq = {(__bf16)hi[0], (__bf16)hi[1]};
            out[2 * k] = __builtin_bit_cast(uint32_t, a);
            out[2 * k + 1] = __builtin_bit_cast(uint32_t, bq);
        }
        *reinterpret_cast<uint4 *>(dst + i * 4) = make_uint4(out[0], out[1], out[2], out[3]);
    }
}

using fa::unpack8;
using fa::pack8;
using fa::rotary_slot;
using fa::for_ragged_rows;
using fa::ragged_launch_shape;
using fa::SplitPlan;
using fa::align256;
using fa::query_rows;

template <typename T>
__global__ void rotary_kernel(const fa_rotary_params p) {
    const int slots = (p.d / 8 + 1) / 2;
    const int64_t total = (int64_t)p.b * p.s * p.h * slots;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int slot = (int)(i % slots);
        int64_t t = i / slots;
        const int hd = (int)(t % p.h);
        t /= p.h;
        const int row = (int)(t % p.s);
        const int b = (int)(t / p.s);
        const int pos = p.seqlen_offsets[b] + (p.per_row_positions ? row : 0);
        const T *src = (const T *)p.src + b * p.src_batch_stride + row * p.src_row_stride + hd * p.src_head_stride;
        T *dst = (T *)p.dst + b * p.dst_batch_stride + row * p.dst_row_stride + hd * p.dst_head_stride;
        const T *cr = (const T *)p.rotary_cos + (int64_t)pos * (p.rotary_dim / 2);
        const T *sr = (const T *)p.rotary_sin + (int64_t)pos * (p.rotary_dim / 2);
        rotary_slot<T>(src, dst, p.d, p.rotary_dim, p.rotary_interleaved != 0, slot, cr, sr);
    }
}

// ---- KV-cache append: k_new/v_new rows -> cache rows [cache_seqlens[b], +seqlen_new), keys optionally rotated.
// One thread = one slot of two 16-byte chunks of K and the same chunks of V.  HBM-bound elementwise pass.
template <typename T>
__global__ void kvcache_append_kernel(const fa_kvcache_append_params p) {
    const int dv = p.d_v > 0 ? p.d_v : p.d;  // (ABI v13: V rows of their own width; slots past K's chunks copy V only)
    const int slots = max((p.d / 8 + 1) / 2, (dv / 8 + 1) / 2), chunks = dv >> 3;
    const int64_t total = (int64_t)p.b * p.seqlen_new * p.h_k * slots;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int slot = (int)(i % slots);
        int64_t t = i / slots;
        const int hd = (int)(t % p.h_k);
        t /= p.h_k;
        const int row = (int)(t % p.seqlen_new);
        const int b = (int)(t / p.seqlen_new);
        int dst_row = p.cache_seqlens[b] + row;
        if (dst_row < 0 || dst_row >= p.seqlen_cache) continue;
        const int pos = p.rotary_seqlens ? p.rotary_seqlens[b] + row : dst_row;   // (FA3 seqlens_rotary; default: the cache row)
        int cb = p.cache_batch_idx ? p.cache_batch_idx[b] : b;
        if (p.block_table) {
            cb = p.block_table[b * p.block_table_batch_stride + dst_row / p.page_block_size];
            dst_row %= p.page_block_size;
        }
        const T *ks = (const T *)p.k_new + b * p.knew_batch_stride + row * p.knew_row_stride + hd * p.knew_head_stride;
        const T *vs = (const T *)p.v_new + b * p.vnew_batch_stride + row * p.vnew_row_stride + hd * p.vnew_head_stride;
        T *kd = (T *)p.k_cache + cb * p.kcache_batch_stride + dst_row * p.kcache_row_stride + hd * p.kcache_head_stride;
        T *vd = (T *)p.v_cache + cb * p.vcache_batch_stride + dst_row * p.vcache_row_stride + hd * p.vcache_head_stride;
        const int rd = p.rotary_cos ? p.rotary_dim : 0;
        const T *cr = (const T *)p.rotary_cos + (int64_t)pos * (rd / 2);
        const T *sr = (const T *)p.rotary_sin + (int64_t)pos * (rd / 2);
        rotary_slot<T>(ks, kd, p.d, rd, p.rotary_interleaved != 0, slot, cr, sr);
        // V: the same enumeration without a rotary part (slot -> chunks 2 slot, 2 slot + 1)
        const int c0 = 2 * slot, c1 = 2 * slot + 1;
        if (c0 < chunks) *reinterpret_cast<uint4 *>(vd + c0 * 8) = *reinterpret_cast<const uint4 *>(vs + c0 * 8);
        if (c1 < chunks) *reinterpret_cast<uint4 *>(vd + c1 * 8) = *reinterpret_cast<const uint4 *>(vs + c1 * 8);
    }
}

// ---- ragged KV-cache append (fa_kvcache_append_varlen): one pass over the new rows, 16-byte loads and stores, no atomics; the
// lanes of a wavefront walk one row's (head, slot) items in address order (rotary_slot: two chunks of K, the same of V).
template <typename T>
__global__ __launch_bounds__(256) void kvcache_append_varlen_kernel(const fa_kvcache_append_varlen_params p) {
    const int dv = p.d_v > 0 ? p.d_v : p.d;
    const int slots = max((p.d / 8 + 1) / 2, (dv / 8 + 1) / 2), chunks = dv >> 3, items = p.h_k * slots;
    const int lane = threadIdx.x & 63;
    // the fill levels the attention launch reads: one entry per thread of the first workgroups (the grid holds >= b threads)
    const int64_t gid = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
    if (gid < p.b) {
        const int s = (int)gid;
        p.seqused_out[s] = min(p.cache_seqlens[s] + (p.cu_seqlens_k_new[s + 1] - p.cu_seqlens_k_new[s]), p.seqlen_cache);
    }
    for_ragged_rows(p.cu_seqlens_k_new, p.b, p.total_k_new, p.max_seqlen_k_new, [&](int seq, int i, int row) {
        const int fill = p.cache_seqlens[seq];
        int dst_row = fill + i;
        if (dst_row < 0 || dst_row >= p.seqlen_cache) return;  // past the capacity: dropped (wave-uniform)
        const int pos = (p.rotary_seqlens ? p.rotary_seqlens[seq] : fill) + i;
        int cb = p.cache_batch_idx ? p.cache_batch_idx[seq] : seq;
        if (p.block_table) {
            cb = p.block_table[seq * p.block_table_batch_stride + dst_row / p.page_block_size];
            dst_row %= p.page_block_size;
        }
        const T *ks_row = (const T *)p.k_new + (int64_t)row * p.knew_row_stride;
        const T *vs_row = (const T *)p.v_new + (int64_t)row * p.vnew_row_stride;
        T *kd_row = (T *)p.k_cache + cb * p.kcache_batch_stride + dst_row * p.kcache_row_stride;
        T *vd_row = (T *)p.v_cache + cb * p.vcache_batch_stride + dst_row * p.vcache_row_stride;
        const int rd = p.rotary_cos ? p.rotary_dim : 0;
        const T *cr = (const T *)p.rotary_cos + (int64_t)pos * (rd / 2);
        const T *sr = (const T *)p.rotary_sin + (int64_t)pos * (rd / 2);
        for (int it = lane; it < items; it += 64) {
            const int hd = it / slots, slot = it % slots;
            rotary_slot<T>(ks_row + hd * p.knew_head_stride, kd_row + hd * p.kcache_head_stride, p.d, rd,
                           p.rotary_interleaved != 0, slot, cr, sr);
            const T *vs = vs_row + hd * p.vnew_head_stride;
            T *vd = vd_row + hd * p.vcache_head_stride;
            const int c0 = 2 * slot, c1 = 2 * slot + 1;
            if (c0 < chunks) *reinterpret_cast<uint4 *>(vd + c0 * 8) = *reinterpret_cast<const uint4 *>(vs + c0 * 8);
            if (c1 < chunks) *reinterpret_cast<uint4 *>(vd + c1 * 8) = *reinterpret_cast<const uint4 *>(vs + c1 * 8);
        }
    });
}

// ---- rotary embedding of a ragged tensor (fa_rotary_apply_varlen): the same launch shape and sequence lookup
template <typename T>
__global__ __launch_bounds__(256) void rotary_varlen_kernel(const fa_rotary_varlen_params p) {
    const int slots = (p.d / 8 + 1) / 2, items = p.h * slots;
    const int lane = threadIdx.x & 63;
    for_ragged_rows(p.cu_seqlens_q, p.b, p.total_q, p.max_seqlen_q, [&](int seq, int i, int row) {
        const int pos = p.offsets[seq] + (p.per_row_positions ? i : 0);
        const T *src_row = (const T *)p.src + (int64_t)row * p.src_row_stride;
        T *dst_row = (T *)p.dst + (int64_t)row * p.dst_row_stride;
        const T *cr = (const T *)p.rotary_cos + (int64_t)pos * (p.rotary_dim / 2);
        const T *sr = (const T *)p.rotary_sin + (int64_t)pos * (p.rotary_dim / 2);
        for (int it = lane; it < items; it += 64) {
            const int hd = it / slots, slot = it % slots;
            rotary_slot<T>(src_row + hd * p.src_head_stride, dst_row + hd * p.dst_head_stride, p.d, p.rotary_dim,
                           p.rotary_interleaved != 0, slot, cr, sr);
        }
    });
}

// ---- sign-encoded S_dmask (FA_FLAG_SDMASK_SIGNED, include/fa_fwd.h): what the reference's CUDA forward returns for
// return_softmax under dropout (csrc/flash_attn/src/flash_fwd_kernel.h:350-360, 412-422; src/dropout.h:26-33), restated as a
// pass of its own -- a testing aid there and here, not on the hot path.  One workgroup = 8 query rows of one (batch, head);
// per row: all scores (fp32 dot products, scaled, + ALiBi, masked) into LDS, the row maximum of every key block of `block_n`
// keys, their suffix maxima (the running maximum of a sweep from the last block to the first), then
// exp(score - suffix max of its block), negated where fa_rand8 (the forward's hash) drops the element.
template <typename T>
__global__ __launch_bounds__(256) void sdmask_kernel(const fa::KParams p, T *out, int rows_r, int cols_r, int block_n) {
    extern __shared__ __attribute__((aligned(16))) char smem_[];
    constexpr int ROWS = 8;
    const int nrb = (p.seqlen_q + ROWS - 1) / ROWS;
    const int rb = blockIdx.x % nrb, head = (blockIdx.x / nrb) % p.h, batch = blockIdx.x / (nrb * p.h);
    const int kv_head = head / p.h_ratio;
    int sq, sk;
    int64_t q_base, k_base;
    if (p.cu_seqlens_q) {
        const int q0 = p.cu_seqlens_q[batch], k0 = p.cu_seqlens_k[batch];
        sq = p.seqused_q ? p.seqused_q[batch] : p.cu_seqlens_q[batch + 1] - q0;
        sk = p.seqused_k ? p.seqused_k[batch] : p.cu_seqlens_k[batch + 1] - k0;
        q_base = (int64_t)q0 * p.q_row_stride;
        k_base = (int64_t)k0 * p.k_row_stride;
    } else {
        sq = p.seqused_q ? p.seqused_q[batch] : p.seqlen_q;
        sk = p.seqused_k ? p.seqused_k[batch] : p.seqlen_k;
        q_base = (int64_t)batch * p.q_batch_stride;
        k_base = (int64_t)batch * p.k_batch_stride;
    }
    if (rb * ROWS >= sq || sk <= 0) return;
    const T *qp = (const T *)p.q + q_base + (int64_t)head * p.q_head_stride;
    const T *kp = (const T *)p.k + k_base + (int64_t)kv_head * p.k_head_stride;
    T *op = out + (((int64_t)batch * p.h + head) * rows_r) * cols_r;
    const fa::Scales sc = fa::load_scales(p, batch, kv_head);
    const float alibi = p.alibi ? p.alibi[(int64_t)batch * p.alibi_bs + head] : 0.f;
    const uint32_t seed_mix = fa::fa_seed_mix(p.rng_state, batch * p.h + head);
    const int shift = sk - sq;
    float *qs = (float *)smem_;                // [ROWS][d]
    float *scs = qs + ROWS * p.d;              // [sk]
    float *bm = scs + ((sk + 3) & ~3);         // [nblk]
    const int nblk = (sk + block_n - 1) / block_n;
    for (int i = threadIdx.x; i < ROWS * p.d; i += 256) {
        const int r = rb * ROWS + i / p.d;
        qs[i] = r < sq ? (float)qp[(int64_t)r * p.q_row_stride + i % p.d] : 0.f;
    }
    __syncthreads();
    for (int rr = 0; rr < ROWS; ++rr) {
        const int row = rb * ROWS + rr;
        if (row >= sq) break;   // (uniform)
        const float *qr = qs + rr * p.d;
        for (int key = threadIdx.x; key < sk; key += 256) {
            const T *kr = kp + (int64_t)key * p.k_row_stride;
            float acc = 0.f;
            for (int c = 0; c < p.d; c += 8) {
                const uint4 w = *reinterpret_cast<const uint4 *>(kr + c);
                float x[8];
                unpack8<T>(w, x);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc += qr[c + e] * x[e];
            }
            float sv = acc * sc.scale - alibi * fabsf((float)(row + shift - key));
            bool vis = true;
            if (p.window_right >= 0) vis = vis && key <= row + shift + p.window_right;
            if (p.window_left >= 0) vis = vis && key >= row + shift - p.window_left;
            scs[key] = vis ? sv : -INFINITY;
        }
        __syncthreads();
        for (int j = threadIdx.x; j < nblk; j += 256) {
            float m = -INFINITY;
            for (int key = j * block_n; key < min(sk, (j + 1) * block_n); ++key) m = fmaxf(m, scs[key]);
            bm[j] = m;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int j = nblk - 2; j >= 0; --j) bm[j] = fmaxf(bm[j], bm[j + 1]);
        __syncthreads();
        for (int key = threadIdx.x; key < sk; key += 256) {
            const float m = bm[key / block_n];
            const float pv = (scs[key] == -INFINITY || m == -INFINITY) ? 0.f : __expf(scs[key] - m);
            const bool keep = fa::fa_rand8(seed_mix, (uint32_t)row, (uint32_t)key) <= (uint32_t)p.drop_thr;
            op[(int64_t)row * cols_r + key] = (T)(keep ? pv : -pv);
        }
        __syncthreads();
    }
}

// ---- forward routing ----------------------------------------------------------------------------------------------------
// plan_fwd() is the one place that decides which kernel a problem runs, with which template arguments, grid, split-KV plan
// and fp8 workspace.  It is host code without HIP calls: fa_fwd_validate, fa_fwd_workspace_size, fa_fwd and fa_fwd_plan_name
// (the test hook that names the plan, tests/test_fwd_plan.py) all read the same plan.

struct Fp8Plan {
    int64_t rows_q, rows_k, q_bytes, kv_bytes, total;
};
Fp8Plan fp8_plan(const fa_fwd_params *p) {
    Fp8Plan pl;
    pl.rows_q = p->cu_seqlens_q ? p->total_q : (int64_t)p->b * p->seqlen_q;
    pl.rows_k = p->cu_seqlens_q ? p->total_k : (int64_t)p->b * p->seqlen_k;
    pl.q_bytes = align256(pl.rows_q * p->h * p->d * 2);
    pl.kv_bytes = align256(pl.rows_k * p->h_k * p->d * 2);
    pl.total = pl.q_bytes + 2 * pl.kv_bytes;
    return pl;
}

int head_dim_tile(int d) {
    if (d <= 64) return 64;
    if (d <= 128) return 128;
    return 256;
}
int block_m_of(int variant, int d) { return (variant == 2 || head_dim_tile(d) == 256) ? 128 : 256; }

// ABI v12: attention_chunk and a V head dim of its own exist in fwd_kernel only (the compiler-scheduled shape)
inline bool own_dv(const fa_fwd_params *p) { return p->d_v > 0 && p->d_v != p->d; }
inline bool generic_only(const fa_fwd_params *p) { return p->attention_chunk > 0 || own_dv(p); }
inline int wide_dim(const fa_fwd_params *p) { return own_dv(p) ? std::max(p->d, std::min(p->d_v, 256)) : p->d; }  // what the LDS tile has to hold
// ABI v13: the qv kernel (fa_fwd_kernel_qv.h) serves q/k head dims <= 64 beside a V head dim in [256, 512] -- every call with
// qv, and without qv the paged / split-KV calls of that shape (the 256-column launches cannot split or page).  The dense
// and varlen calls without qv keep the 256-column launches.
inline int dv_of(const fa_fwd_params *p) { return p->d_v > 0 ? p->d_v : p->d; }
inline bool qv_shape(const fa_fwd_params *p) {
    return p->dtype != FA_DTYPE_FP8_E4M3 && p->d <= 64 && dv_of(p) >= 256 && dv_of(p) <= 512;
}
inline bool qv_route(const fa_fwd_params *p) { return p->qv || (qv_shape(p) && (p->block_table || p->num_splits > 1)); }
// a left window that masks anything (the FA2 rule drops one of seqlen_k or more: fa::normalise_window)
inline bool left_window(const fa_fwd_params *p) {
    int32_t wl = p->window_size_left, wr = p->window_size_right;
    fa::normalise_window(p->is_causal, p->flags, p->seqlen_k, wl, wr);
    return wl >= 0;
}
// FA_FLAG_PACK_GQA is a hint: the pk kernel (fa_fwd_kernel_pk.h) honours it for GQA / MQA calls of 16-bit types at head dims
// <= 128 without ALiBi, dropout, attention_chunk, a V head dim of its own or qv; every other call is planned as without it.
// (The kernel counts packed rows in 32 bits.)
inline bool pk_route(const fa_fwd_params *p) {
    if (!(p->flags & FA_FLAG_PACK_GQA) || p->h_k <= 0 || p->h % p->h_k != 0 || p->h / p->h_k <= 1) return false;
    if (p->dtype == FA_DTYPE_FP8_E4M3 || p->d > 128 || p->alibi_slopes || p->p_dropout > 0.f || generic_only(p)) return false;
    if ((int64_t)p->seqlen_q * (p->h / p->h_k) > 0x7fffffff) return false;
    return !qv_route(p);
}
// 1 / (1 - p_dropout) as the kernels get it: the dropout instantiations run exactly when it is not 1
inline float rp_dropout(const fa_fwd_params *p) { return p->p_dropout > 0.f ? 1.f / (1.f - p->p_dropout) : 1.f; }

// fp8 inputs run natively (fa_fwd_kernel_fp8.h: e4m3 operands straight into the block-scaled MFMA, no expansion pass, no
// workspace) for the shape BASELINE config 5 names -- head dim 128, dense or varlen, full / causal / right-window masks.  The
// rest of the fp8 surface (other head dims, softcap, left windows) and an explicit kernel_variant take the exact
// e4m3 -> bf16 expansion in front of the 16-bit kernels.
bool fp8_native(const fa_fwd_params *p) {
    if (p->dtype != FA_DTYPE_FP8_E4M3 || p->d != 128 || generic_only(p)) return false;
    const int variant = p->kernel_variant ? p->kernel_variant : g_default_variant.load();
    if (variant != 0) return false;
    if (p->softcap > 0.f || p->alibi_slopes || p->block_table || p->kv_batch_idx || p->leftpad_k || p->p_dropout > 0.f) return false;
    if (left_window(p)) return false;
    const int64_t strides[] = {p->q_row_stride, p->q_head_stride, p->k_row_stride, p->k_head_stride, p->v_row_stride,
                               p->v_head_stride, p->cu_seqlens_q ? 0 : p->q_batch_stride, p->cu_seqlens_q ? 0 : p->k_batch_stride,
                               p->cu_seqlens_q ? 0 : p->v_batch_stride};
    for (int64_t st : strides)
        if (st % 16 != 0) return false;
    const void *ptrs[] = {p->q, p->k, p->v};
    for (const void *ptr : ptrs)
        if (reinterpret_cast<uintptr_t>(ptr) % 16 != 0) return false;
    // The kernel addresses one (batch, kv head)'s K and V through raw buffer descriptors: 32-bit byte offsets (num_records,
    // soffset = tile * row_stride) and int row strides.  A K or V of 2 GiB or more per batch entry has no safe path in the
    // native kernel (its generic tile uses the same descriptors): those shapes take the expansion path, whose 16-bit kernels
    // address with 64-bit tile bases.
    const int64_t rows_k = p->cu_seqlens_q ? p->total_k : p->seqlen_k;
    if (p->k_row_stride >= (int64_t(1) << 31) || p->v_row_stride >= (int64_t(1) << 31)) return false;
    if (rows_k * p->k_row_stride >= (int64_t(1) << 31) || rows_k * p->v_row_stride >= (int64_t(1) << 31)) return false;
    return true;
}

// Kernel shape of a 16-bit (or fp8-expanded) problem.  0 = the library's choice: the 256-row software-pipelined kernel, except
//  * paged caches -> the 64-key-aligned 8-wave shape (variant 1);
//  * short dense query blocks (seqlen_q <= 128: decode steps, short prefill chunks) -> 4 waves x 32 rows (variant 2):
//    a 256-row tile would leave 2-3 of its 4 waves without rows, and this shape fits two workgroups per CU
//    (measured on decode b8 hq32/hkv8 cache 8192: 149 -> 59 us, b32: 255 -> 219 us).
int effective_variant(const fa_fwd_params *p) {
    int variant = p->kernel_variant ? p->kernel_variant : g_default_variant.load();
    if (variant < 0 || variant > 3) variant = 0;
    if (p->p_dropout > 0.f) return 1;  // dropout lives in the compiler-scheduled shape only
    if (generic_only(p)) {
        // fwd_kernel, EXTRA instantiations: 8 waves x 32 rows (4 x 32 at head-dim tile 256) -- except a V head dim of its own
        // on the wide tile, which plan_fwd hands to the generated-loop kernel when the features are plain
        if (p->attention_chunk == 0 && head_dim_tile(wide_dim(p)) == 256 && variant == 0) return 0;
        return 1;
    }
    if (variant == 0 || variant == 3) {
        if (p->block_table) variant = 1;
        else if (!p->cu_seqlens_q && p->seqlen_q <= 128) variant = 2;
        else if (variant == 0) {
            // Short key ranges: a 256-row workgroup sweeps only a handful of 64-key tiles, so its fixed cost (~13 us) and,
            // under a causal mask, the idle time of the waves whose rows end early (all four meet at every tile barrier)
            // outweigh the pipelined loop.  Measured on the reference's benchmark grid (16k tokens, tools/fwd_grid.py):
            //   d64  causal s512/1024/2048: 178/255/379 -> 235/332/431 TFLOP/s (4 waves x 32 rows); non-causal s512 421 -> 459
            //   d128 causal s512/1024:      230/345     -> 293/364      TFLOP/s (8 waves x 32 rows)
            const bool causal_like = p->is_causal || (p->window_size_right == 0 && p->window_size_left < 0);
            const int tile = head_dim_tile(p->d);
            // (round 2: at head-dim tile 128 the generated loop applies the causal mask itself -- the diagonal tiles no longer
            //  run the generic half-step -- and the 256-row kernel wins from seqlen 512 on: causal s512 / s1024 308 / 379
            //  (8 waves x 32 rows) -> 319 / 485 TFLOP/s.  Head-dim tile 64 has its generated loop too (FastLoop64), but with twice
            //  the VALU per MFMA the 4-wave x 32-row shape still wins on short key ranges: causal s512 / 1024 / 2048 278 / 394 / 518
            //  against 227 / 331 / 497, non-causal s512 490 against 443 (profiles/r2_fwd_grid.txt): the rule stays)
            if (tile == 64 && ((causal_like && p->seqlen_k <= 2048) || p->seqlen_k <= 512)) variant = 2;
        }
    }
    return variant;
}

// ---- split-KV plan (role of num_splits_heuristic / set_params_splitkv, csrc/flash_attn/flash_api.cpp:257-329) ---------
// 16-bit problems over dense K/V split: dense queries, and ragged queries over a batched cache (ragged_cache()); the
// cu_seqlens_q + cu_seqlens_k problems never do.  Heuristic (num_splits == 0): split when the tiles leave most of the
// 256 CUs idle, so that tiles x splits reaches ~2 workgroups per CU, with at least 4 key blocks (256 keys) per split.
// The partials: fa::split_layout.
// ragged queries over a batched / paged cache: cu_seqlens_q without cu_seqlens_k, fill levels in seqused_k (include/fa_fwd.h)
inline bool ragged_cache(const fa_fwd_params *p) { return p->cu_seqlens_q && !p->cu_seqlens_k; }
// an upper bound of the problem's row blocks of `bm` rows: the host knows total_q and max_seqlen_q of a ragged batch, not the
// lengths (no sync) -- every non-empty sequence has at most len / bm + 1 blocks, and at most ceil(max_seqlen_q / bm)
inline int64_t row_blocks_bound(const fa_fwd_params *p, int64_t bm, int64_t rows_per_query = 1) {
    const int64_t per_seq = (p->seqlen_q * rows_per_query + bm - 1) / bm;
    if (!p->cu_seqlens_q) return per_seq * p->b;
    const int64_t seqs = std::min<int64_t>(p->b, p->total_q);
    return std::min(seqs * per_seq, p->total_q * rows_per_query / bm + seqs);
}
SplitPlan split_plan(const fa_fwd_params *p, int variant, bool pk = false) {
    SplitPlan sp{1, 0, 0, 0};
    if (p->cu_seqlens_k || p->dtype == FA_DTYPE_FP8_E4M3 || p->seqlen_q <= 0 || p->seqlen_k <= 0) return sp;
    if (p->cu_seqlens_q && p->total_q <= 0) return sp;
    if (p->p_dropout > 0.f) return sp;  // (the reference does not split under dropout either: flash_api.cpp:307)
    // attention_chunk / a V head dim of its own (the EXTRA instantiations): never split.  The partials and the merge are laid
    // out for d columns, and no entry point asks for a split beside attention_chunk (the dense FA3 route plans one part): like
    // dropout, a num_splits above 1 is planned as 1 rather than run on a store path nothing exercises
    if (generic_only(p)) return sp;
    int n = p->num_splits;
    const int n_blocks = (p->seqlen_k + 63) / 64;
    if (n == 0) {
        const int bm = block_m_of(variant, wide_dim(p));
        // (the pk kernel: blocks of packed rows per kv head, in the 4-wave shape -- the caller passes variant 2)
        const int64_t tiles = pk ? row_blocks_bound(p, bm, p->h / p->h_k) * p->h_k : row_blocks_bound(p, bm) * p->h;
        // two workgroups of the 4-wave shape fit a CU: aim at ~4 per CU there, ~2 per CU for the 256-row kernel
        const int64_t cap = (variant == 2) ? 512 : 128, target = (variant == 2) ? 1024 : 512;
        n = 1;
        if (tiles > 0 && tiles <= cap && n_blocks >= 8) {
            n = (int)std::min<int64_t>((target + tiles - 1) / tiles, n_blocks / 4);
            n = std::max(1, std::min(n, 64));
        }
    }
    return fa::split_layout(p, std::min(n, std::min(n_blocks, 128)), p->d);
}

// Split plan of the qv kernel: the problems split_plan takes.  Heuristic (num_splits == 0): one workgroup fills a CU
// (its LDS), so the (batch, kv head, row block) groups are multiplied up to ~2 workgroups per CU of 256, with at least 4 key
// blocks per split.  Partials: O (splits, b, seqlen_q, h, d_v), LSE (splits, b, h, seqlen_q), fp32
// (ragged queries: (splits, total_q, h, d_v) and (splits, h, total_q)).
SplitPlan split_plan_qv(const fa_fwd_params *p) {
    SplitPlan sp{1, 0, 0, 0};
    if (p->cu_seqlens_k || p->seqlen_q <= 0 || p->seqlen_k <= 0 || (p->cu_seqlens_q && p->total_q <= 0)) return sp;
    int n = p->num_splits;
    const int n_blocks = (p->seqlen_k + 63) / 64;
    if (n == 0) {
        const int64_t groups = row_blocks_bound(p, 32, p->h / p->h_k) * p->h_k;
        n = 1;
        if (groups < 512 && n_blocks >= 8) n = (int)std::max<int64_t>(1, std::min<int64_t>((512 + groups - 1) / groups, n_blocks / 4));
        n = std::min(n, 64);
    }
    return fa::split_layout(p, std::min(n, std::min(n_blocks, 128)), dv_of(p));
}

enum class Family { fp8, qv, w64, d256, generic, pk };  // fwd_kernel_fp8, fwd_kernel_qv, fwd_kernel_w64, fwd_kernel_d256, fwd_kernel, pk_fwd_kernel

struct FwdPlan {
    Family family;
    int d;           // head-dim tile D of fwd_kernel / fwd_kernel_w64 / fwd_kernel_fp8
    int deff;        // fwd_kernel_w64: DEFF; fwd_kernel_d256: its width W; fwd_kernel_qv: the V tile DVT
    int waves;
    bool softcap, alibi, dropout, extra, persist;  // template forms (alibi: fwd_kernel_d256 only)
    int block_m;     // query rows per workgroup
    int32_t num_m_blocks;
    int64_t tiles, unit_tiles, whole_slots, grid;  // scheduling of the row blocks over the XCDs (tile_of_wg; pk: grid holds the splits too)
    int status;      // FA_ERR_BAD_SHAPE when the grid does not fit 31 bits
    bool nothing;    // no query or no key: no split, no fp8 expansion, no S_dmask pass
    SplitPlan split;
    bool fp8_expand; // fp8 inputs the 16-bit kernels read as bf16 copies, made by expand_fp8_kernel in the workspace
    Fp8Plan fp8;
    int cols;        // calls of 256 V columns each (d_v > 256 without the qv kernel); the kernel fields plan the first
    int64_t workspace;
};

// The persistent form of the 256-row kernel (fa_fwd_kernel_w64.h, PERSIST): plain dense problems at head dims 97..128 whose
// every work item sweeps at least three 64-key tiles and whose K / V tensors one 32-bit raw buffer descriptor can span.
bool persist_ok(const fa_fwd_params *p, const FwdPlan &pl, int num_cus) {
    const int mode = g_persist_mode.load();
    if (mode < 0) return false;
    const bool fp8 = p->dtype == FA_DTYPE_FP8_E4M3;
    if (p->cu_seqlens_q || p->cu_seqlens_k || p->seqused_q || p->seqused_k || p->leftpad_k || p->kv_batch_idx || p->block_table) return false;
    if (p->alibi_slopes || (fp8 && (p->q_descale || p->k_descale || p->v_descale)) || pl.split.splits > 1 || rp_dropout(p) != 1.f) return false;
    if (p->d <= 96 || p->d > 128) return false;   // (left windows: the next item's first tile is its own n_min, round 3)
    if (p->seqlen_k % 64 != 0 || p->seqlen_k < 192 || p->seqlen_q > p->seqlen_k) return false;  // (causal: bottom-right aligned, shift >= 0)
    if ((num_cus & ~7) < 8) return false;
    // the kernel decodes its chain once into 32-bit entries (m_block 12 bits, head 10, batch 10), one lane per round
    if (pl.grid > 64 * (num_cus & ~7) || pl.num_m_blocks > 4096 || p->h > 1024 || p->b > 1024) return false;
    // K and V as the kernel reads them: the fp8 expansion leaves contiguous (rows, h_k, d) copies
    int64_t kbs = p->k_batch_stride, khs = p->k_head_stride, krs = p->k_row_stride;
    int64_t vbs = p->v_batch_stride, vhs = p->v_head_stride, vrs = p->v_row_stride;
    if (pl.fp8_expand) {
        krs = vrs = (int64_t)p->h_k * p->d;
        khs = vhs = p->d;
        kbs = vbs = krs * p->seqlen_k;
    }
    auto extent = [&](int64_t bs, int64_t hs, int64_t rs, int lead) {
        return ((int64_t)(p->b - 1) * bs + (int64_t)(p->h_k - 1) * hs + (int64_t)(p->seqlen_k - 1 + lead) * rs + 128) * 2;
    };
    if (kbs < 0 || khs < 0 || krs <= 0 || vbs < 0 || vhs < 0 || vrs <= 0) return false;
    if (extent(kbs, khs, krs, 32) >= (1ll << 32) - 65536 || extent(vbs, vhs, vrs, 0) >= (1ll << 32) - 65536) return false;
    if ((int64_t)p->seqlen_k * krs >= (1ll << 30) || (int64_t)p->seqlen_k * vrs >= (1ll << 30)) return false;
    if (mode > 0) return true;
    // left windows: supported (bit-identical to the hand-over kernel, tests/test_persistent_gpu.py) but measured SLOWER there --
    // b4 s4096 window (1024, 0) 538 -> 472, (512, 512) 530 -> 469, s16384 (4096, 0) 825 -> 782 TFLOP/s: a windowed item spends its
    // first tiles on the generic half-step (the left edge), where the cross-item look-ahead stream buys nothing -- not dispatched
    if (left_window(p)) return false;
    // chains of one item gain nothing; from two items per CU on the persistent form wins or ties on the whole benchmark grid
    // (profiles/r3_persist_sweep.txt: non-causal s512 .. 16k +10 / +5 / +2 / 0 %, causal +21 / +26 / +15 / +11 / +3 / +1 %)
    return pl.grid > (num_cus & ~7);
}

// The plan of one fa_fwd call on a device of `num_cus` compute units (which decide the persistent form only).  Reads only `p`,
// `num_cus`, g_default_variant and g_persist_mode.  Safe on parameters fa_fwd_validate has not finished with: it is part of it.
FwdPlan plan_fwd(const fa_fwd_params *p, int num_cus) {
    const bool qv = qv_route(p);
    if (p->d_v > 256 && !qv) {
        // V head dims above the widest tile (hopper/flash_api.cpp:783-792 allows up to 512 beside q/k <= 64): fa_fwd makes one
        // call per 256 columns of V and O
        fa_fwd_params first = *p;
        first.d_v = 256;
        FwdPlan pl = plan_fwd(&first, num_cus);
        pl.cols = (p->d_v + 255) / 256;
        pl.split = SplitPlan{1, 0, 0, 0};  // (the whole call has a V head dim of its own: never split)
        pl.workspace = pl.fp8_expand ? pl.fp8.total : 0;
        return pl;
    }
    FwdPlan pl{};
    pl.cols = 1;
    pl.status = FA_OK;
    const bool fp8 = p->dtype == FA_DTYPE_FP8_E4M3, native = fp8_native(p);
    const bool softcap = p->softcap > 0.f, alibi = p->alibi_slopes != nullptr, dropout = rp_dropout(p) != 1.f;
    const bool pk = pk_route(p);
    const int variant = native ? 0 : pk ? 2 : effective_variant(p);  // (fp8 native: one shape, 4 waves x 64 rows; pk: 4 x 32)
    pl.nothing = p->seqlen_q == 0 || p->seqlen_k == 0 || (p->cu_seqlens_q && p->total_q == 0);
    pl.fp8_expand = fp8 && !native;
    if (fp8) pl.fp8 = fp8_plan(p);
    pl.split = pl.nothing ? SplitPlan{1, 0, 0, 0} : qv ? split_plan_qv(p) : split_plan(p, variant, pk);
    pl.workspace = fp8 ? (native ? 0 : pl.fp8.total) : pl.split.total;

    if (pk) {
        // pk_fwd_kernel: blocks of PK_BLOCK_M packed rows per (batch, kv head, split) group (fa::packed_grid)
        pl.family = Family::pk;
        pl.d = pl.deff = head_dim_tile(p->d);
        pl.waves = fa::PK_NWAVES;
        pl.softcap = softcap;
        pl.block_m = fa::PK_BLOCK_M;
        const fa::PackedGrid g = fa::packed_grid(p, fa::PK_BLOCK_M, pl.split.splits);
        pl.tiles = g.pblocks * p->h_k * p->b;
        pl.grid = g.grid;
        pl.status = g.status;
        pl.num_m_blocks = pl.status == FA_OK ? (int32_t)g.pblocks : 0;
        return pl;
    }

    // softcap or ALiBi at head dims <= 128 (measured b4 s4096: softcap d128 471, d64 322, ALiBi 231 / 182 TFLOP/s through the C++
    // paths of the 256-row kernel): the generated loops that cap / bias scores exist for the 32-row-per-wave shape only ->
    // fwd_kernel_d256 at widths 64 / 96 / 128
    const bool capped = softcap != alibi && variant == 0 && p->d <= 128 && !generic_only(p) && !pl.nothing && pl.split.splits <= 1;
    const int tile = head_dim_tile(wide_dim(p));
    pl.block_m = capped ? 128 : block_m_of(variant, wide_dim(p));

    // scheduling (tile_of_wg): whole (batch, kv head) units -- everything that streams one head's K/V stays on one XCD -- for as
    // many units as deal evenly over the 8 XCDs, the remaining heads by m_block of the GQA group; problems with fewer than two
    // units per XCD entirely by m_block (fill the chip first, L2 reuse second).  (20 units used to be dealt 3+3+3+3+2+2+2+2:
    // the launch took as long as 24, tools/hdim_bench.py d192 b2 h10 2.88 ms instead of 2.41.)
    pl.num_m_blocks = (p->seqlen_q + pl.block_m - 1) / pl.block_m;
    pl.tiles = (int64_t)pl.num_m_blocks * p->h * p->b;
    const int h_ratio = p->h / p->h_k;
    if (h_ratio > 0) {  // (h < h_k fails validation)
        const int64_t bk_units = (int64_t)p->b * p->h_k, per_kvh = (int64_t)h_ratio * pl.num_m_blocks;
        const int64_t whole_units = bk_units >= 16 ? bk_units / 8 * 8 : 0;
        pl.unit_tiles = per_kvh;
        pl.whole_slots = whole_units / 8 * per_kvh;
        const int64_t rem_units = (pl.tiles - pl.whole_slots * 8 + h_ratio - 1) / h_ratio;
        pl.grid = 8 * (pl.whole_slots + (rem_units + 7) / 8 * h_ratio);
    }
    if (pl.tiles > 0x7fffffff || pl.whole_slots > 0x7fffffff || pl.grid * pl.split.splits > 0x7fffffff) pl.status = FA_ERR_BAD_SHAPE;

    // the generated-loop kernel of head-dim tile 256 (fa_fwd_kernel_d256.h): plain problems, softcap or ALiBi (not both)
    const bool d256_ok = (variant == 0 || variant == 3) && !(softcap && alibi) && !p->block_table && pl.split.splits <= 1 &&
                         !dropout && p->attention_chunk == 0;
    pl.d = pl.deff = tile;
    pl.waves = 4;
    if (native) {  // e4m3 operands straight into the block-scaled MFMA
        pl.family = Family::fp8;
    } else if (qv) {
        pl.family = Family::qv;
        pl.deff = dv_of(p) <= 256 ? 256 : 512;
        pl.waves = fa::QV_NWAVES;
        pl.softcap = softcap;
    } else if (tile == 256 ? d256_ok : capped) {
        // 4 waves x 32 rows around FastLoop256: head-dim tiles 160 / 192 / 256 (hopper/tile_size.h:20-45) skip the zero padding,
        // a V head dim of its own takes the larger of the two (the kernel reads p.dv for V and O)
        pl.family = Family::d256;
        const int w = wide_dim(p);
        pl.deff = tile == 256 ? (w <= 160 ? 160 : w <= 192 ? 192 : 256) : tile == 128 ? (p->d <= 96 ? 96 : 128) : 64;
        pl.softcap = softcap;
        pl.alibi = !softcap && alibi;
    } else if (tile != 256 && (variant == 0 || variant == 3)) {
        // 4 waves x 64 rows, one wave per SIMD, software-pipelined (fa_fwd_kernel_w64.h) -- the default.  D = 256 does not fit
        // its register budget (O alone would be 256 registers).
        pl.family = Family::w64;
        pl.softcap = softcap;
        if (!softcap && tile == 128 && p->d <= 96) pl.deff = 96;  // head-dim tile 96 (hopper/tile_size.h:10-54)
        else if (!softcap && tile == 128) pl.persist = persist_ok(p, pl, num_cus);
    } else {
        // the compiler-scheduled shape (fa_fwd_kernel.h): 8 waves x 32 rows (variant 1), 4 x 32 (variant 2 and head-dim tile
        // 256).  attention_chunk / a V head dim of its own (FA3 surface, ABI v12) run its EXTRA instantiations, dropout (p > 0,
        // also when its 8-bit threshold keeps everything) its DROPOUT ones -- neither with softcap (fa_fwd_validate).  (A DEFF = 192
        // instantiation at head-dim tile 256 -- 12 + 12 instead of 16 + 16 MFMAs per 32-key block -- was measured at exactly the
        // per-workgroup time of the 256 one, tools/hdim_bench.py: this shape is bound by its register-staged K/V rows, which stay
        // 512 B wide, not by the matrix pipe.)
        pl.family = Family::generic;
        pl.waves = (tile == 256 || variant == 2) ? 4 : 8;
        pl.extra = generic_only(p);
        pl.dropout = !pl.extra && dropout;
        pl.softcap = !pl.dropout && softcap;
    }
    return pl;
}

// the text of a plan (fa_fwd_plan_name, fa_fwd_last_plan_name); NULL for a plan whose grid does not fit
const char *plan_text(const FwdPlan &pl, char (&name)[160]) {
    if (pl.status != FA_OK) return nullptr;
    static const char *const kernels[] = {"fwd_kernel_fp8 D=", "fwd_kernel_qv DVT=", "fwd_kernel_w64 D=", "fwd_kernel_d256 W=",
                                          "fwd_kernel D=", "pk_fwd_kernel D="};
    const bool by_width = pl.family == Family::qv || pl.family == Family::d256;
    int n = snprintf(name, sizeof(name), "%s%d", kernels[static_cast<int>(pl.family)], by_width ? pl.deff : pl.d);
    if (pl.family == Family::w64) n += snprintf(name + n, sizeof(name) - n, " DEFF=%d", pl.deff);
    n += snprintf(name + n, sizeof(name) - n, " waves=%d%s%s%s%s%s block_m=%d splits=%d%s", pl.waves, pl.softcap ? " SOFTCAP" : "",
                  pl.alibi ? " ALIBI" : "", pl.dropout ? " DROPOUT" : "", pl.extra ? " EXTRA" : "", pl.persist ? " PERSIST" : "",
                  pl.block_m, pl.split.splits, pl.fp8_expand ? " fp8_expand" : "");
    if (pl.cols > 1) snprintf(name + n, sizeof(name) - n, " cols=%d", pl.cols);
    return name;
}

// the plan the calling thread's most recent fa_fwd launched (fa_fwd_last_plan_name): a struct copy on the call path, the text
// is made when asked
thread_local FwdPlan t_last_plan;
thread_local bool t_last_plan_set = false;
// ... or, when that call was fa_fwd_block_sparse, the head-dim tile of its bs_fwd_kernel (0 = it was not) and its softcap form
thread_local int t_last_bs_tile = 0;
thread_local bool t_last_bs_softcap = false;
// ... or the text an entry point of another translation unit left (fa::fwd_set_last_plan_text: fa_fwd_kv8); "" = none
thread_local char t_last_ext_text[160] = "";

// compute units of the current device (cached per device ordinal)
int device_cus() {
    static std::atomic<int> cus[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    int n = cus[dev & 63].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev & 63].store(n, std::memory_order_relaxed);
    }
    return n;
}

// ---- split-KV merge: out = sum_s w_s O_s / sum_s w_s, w_s = exp(lse_s - max lse); lse = max + log sum w.  One thread =
// one 16-byte chunk of one (batch, row, head); splits with LSE = +inf (no key in their range) carry no weight.
// A learnable sink (fa_fwd_sink) joins here, once: the splits wrote sink-free partials, the merge takes the sink's logit as
// one more weight without a value, rebased like the others on the largest of them (fa::sink_finalize's rule).
template <typename T>
__global__ void combine_splits_kernel(const float *__restrict__ o_acc, const float *__restrict__ lse_acc, T *__restrict__ out,
                                      float *__restrict__ lse_out, int splits, int b, int sq, int h, int d,
                                      int64_t o_bs, int64_t o_rs, int64_t o_hs, const fa::KParams sk) {
    const int chunks = d >> 3;
    const int64_t total = (int64_t)b * sq * h * chunks;
    const int64_t o_split = (int64_t)b * sq * h * d, lse_split = (int64_t)b * h * sq;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % chunks);
        int64_t t = i / chunks;
        const int hd = (int)(t % h);
        t /= h;
        const int row = (int)(t % sq);
        const int bb = (int)(t / sq);
        const int64_t lse_idx = ((int64_t)bb * h + hd) * sq + row;
        float mx = -INFINITY;
        for (int s = 0; s < splits; ++s) {
            const float l = lse_acc[s * lse_split + lse_idx];
            if (l != INFINITY) mx = fmaxf(mx, l);
        }
        const float z = sk.sink ? fa::load_sink(sk, hd, row) : -INFINITY;
        const bool with_sink = z != -INFINITY;  // (z = -inf: the merge without a sink, bit for bit)
        const bool keyless = mx == -INFINITY;
        if (with_sink) mx = fmaxf(mx, z);
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float wsum = with_sink ? __expf(z - mx) : 0.f;
        if (!keyless) {
            for (int s = 0; s < splits; ++s) {
                const float l = lse_acc[s * lse_split + lse_idx];
                if (l == INFINITY) continue;
                const float w = __expf(l - mx);
                wsum += w;
                const float4 *src = reinterpret_cast<const float4 *>(o_acc + s * o_split + (((int64_t)bb * sq + row) * h + hd) * d + c * 8);
                const float4 x0 = src[0], x1 = src[1];
                const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += w * x[j];
            }
            const float inv = 1.f / wsum;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] *= inv;
        }
        *reinterpret_cast<uint4 *>(out + bb * o_bs + row * o_rs + hd * o_hs + c * 8) = pack8<T>(acc);
        if (c == 0) lse_out[lse_idx] = (mx == -INFINITY) ? INFINITY : keyless ? z : mx + __logf(wsum);
    }
}

// ---- fa_fwd_combine: the same merge over caller-provided fp32 partials with arbitrary strides.  One thread = 4
// consecutive head-dim elements of one (batch, row, head); the work is one pass over out_partial (HBM-bound), the LSE
// column of a row is re-read by the d/4 threads that share it (L1/L2 hits).
template <typename TO>
__device__ __forceinline__ void store_out(TO *dst, float x) { *dst = (TO)x; }
template <typename TO>
__global__ void combine_partials_kernel(const fa_combine_params p) {
    const int chunks = (p.d + 3) >> 2;
    const int64_t total = (int64_t)p.b * p.seqlen * p.h * chunks;
    const bool vec = (p.d % 4 == 0) && (p.op_split_stride % 4 == 0) && (p.op_batch_stride % 4 == 0) &&
                     (p.op_row_stride % 4 == 0) && (p.op_head_stride % 4 == 0) &&
                     (reinterpret_cast<uintptr_t>(p.out_partial) % 16 == 0);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % chunks);
        int64_t t = i / chunks;
        const int hd = (int)(t % p.h);
        t /= p.h;
        const int row = (int)(t % p.seqlen);
        const int bb = (int)(t / p.seqlen);
        const float *lp = p.lse_partial + bb * p.lp_batch_stride + row * p.lp_row_stride + hd * p.lp_head_stride;
        const float *op = p.out_partial + bb * p.op_batch_stride + row * p.op_row_stride + hd * p.op_head_stride + c * 4;
        float mx = -INFINITY;
        for (int s = 0; s < p.num_splits; ++s) mx = fmaxf(mx, lp[s * p.lp_split_stride]);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        float wsum = 0.f;
        const int n = min(4, p.d - c * 4);
        if (mx != -INFINITY && mx != INFINITY) {
            for (int s = 0; s < p.num_splits; ++s) {
                const float l = lp[s * p.lp_split_stride];
                if (l == -INFINITY) continue;  // (short-circuit: the partial of an empty split is never read)
                const float w = __expf(l - mx);
                wsum += w;
                const float *src = op + s * p.op_split_stride;
                if (vec) {
                    const float4 x = *reinterpret_cast<const float4 *>(src);
                    acc[0] += w * x.x; acc[1] += w * x.y; acc[2] += w * x.z; acc[3] += w * x.w;
                } else {
                    for (int j = 0; j < n; ++j) acc[j] += w * src[j];
                }
            }
            const float inv = 1.f / wsum;
            for (int j = 0; j < 4; ++j) acc[j] *= inv;
        }
        TO *dst = reinterpret_cast<TO *>(p.out) + bb * p.o_batch_stride + row * p.o_row_stride + hd * p.o_head_stride + c * 4;
        for (int j = 0; j < n; ++j) store_out<TO>(dst + j, acc[j]);
        if (c == 0)
            p.softmax_lse[bb * p.lse_batch_stride + row * p.lse_row_stride + hd * p.lse_head_stride] =
                (mx == -INFINITY || mx == INFINITY) ? mx : mx + __logf(wsum);
    }
}

// ---- the plan -> the template instantiation ------------------------------------------------------------------------------
template <typename T, int D, int NWAVES, bool SOFTCAP, bool DROPOUT = false, bool EXTRA = false>
int launch_fwd_kernel(const fa::KParams &kp, hipStream_t stream) {
    return fa::launch_kernel<fa::fwd_kernel<T, D, NWAVES, SOFTCAP, DROPOUT, D, EXTRA>>(
        fa::smem_bytes<D, NWAVES>(), (int64_t)kp.grid * kp.num_splits, NWAVES * 64, stream, kp);
}
template <typename T, int D>
int launch_generic(const FwdPlan &pl, const fa::KParams &kp, hipStream_t stream) {
    constexpr int NW = D == 256 ? 4 : 8;  // (the EXTRA and DROPOUT shapes)
    if (pl.extra) return pl.softcap ? launch_fwd_kernel<T, D, NW, true, false, true>(kp, stream) : launch_fwd_kernel<T, D, NW, false, false, true>(kp, stream);
    if (pl.dropout) return launch_fwd_kernel<T, D, NW, false, true>(kp, stream);
    if constexpr (NW == 8) {
        if (pl.waves == 8) return pl.softcap ? launch_fwd_kernel<T, D, 8, true>(kp, stream) : launch_fwd_kernel<T, D, 8, false>(kp, stream);
    }
    return pl.softcap ? launch_fwd_kernel<T, D, 4, true>(kp, stream) : launch_fwd_kernel<T, D, 4, false>(kp, stream);
}

template <typename T, int D, bool SOFTCAP, int DEFF = D, bool PERSIST = false>
int launch_w64(const fa::KParams &kp, hipStream_t stream) {
    // PERSIST: one workgroup per CU (a multiple of 8: ids go round-robin over the XCDs), each walks its chain of the slot list
    const int64_t wgs = PERSIST ? std::min(kp.grid, kp.num_cus & ~7) : (int64_t)kp.grid * kp.num_splits;
    return fa::launch_kernel<fa::fwd_kernel_w64<T, D, SOFTCAP, DEFF, PERSIST>>(fa::smem_bytes_w64<D>(), wgs, 256, stream, kp);
}
template <typename T, int D>
int launch_w64_form(const FwdPlan &pl, const fa::KParams &kp, hipStream_t stream) {
    if (pl.softcap) return launch_w64<T, D, true>(kp, stream);
    if constexpr (D == 128) {
        if (pl.deff == 96) return launch_w64<T, 128, false, 96>(kp, stream);
        if (pl.persist) return launch_w64<T, 128, false, 128, true>(kp, stream);
    }
    return launch_w64<T, D, false>(kp, stream);
}

template <typename T, int W>
int launch_d256_form(const FwdPlan &pl, const fa::KParams &kp, hipStream_t stream) {
    constexpr int smem = fa::smem_bytes_d256();
    if (pl.softcap) return fa::launch_kernel<fa::fwd_kernel_d256<T, W, true, false>>(smem, kp.grid, 256, stream, kp);
    if (pl.alibi) return fa::launch_kernel<fa::fwd_kernel_d256<T, W, false, true>>(smem, kp.grid, 256, stream, kp);
    if constexpr (W >= 160) return fa::launch_kernel<fa::fwd_kernel_d256<T, W, false, false>>(smem, kp.grid, 256, stream, kp);
    return FA_ERR_UNSUPPORTED;  // (plain head dims <= 128 run fwd_kernel_w64: never planned)
}

template <typename T, int DVT, bool SOFTCAP>
int launch_qv_form(const fa::QvParams &qa, int64_t grid, hipStream_t stream) {
    return fa::launch_kernel<fa::fwd_kernel_qv<T, DVT, SOFTCAP>>(fa::smem_bytes_qv<DVT>(), grid, fa::QV_NWAVES * 64, stream, qa);
}
// the qv kernel (fa_fwd_kernel_qv.h): V tile 256 (d_v = 256) or 512 columns (d_v in (256, 512])
template <typename T>
int launch_qv(const FwdPlan &pl, const fa_fwd_params *p, const fa::KParams &kp, hipStream_t stream) {
    fa::QvParams qa{};
    qa.p = kp;
    qa.qv = p->qv;
    qa.qv_batch_stride = p->qv_batch_stride; qa.qv_row_stride = p->qv_row_stride; qa.qv_head_stride = p->qv_head_stride;
    const fa::PackedGrid g = fa::packed_grid(p, 32, kp.num_splits);
    if (g.pblocks == 0 || g.groups == 0) return FA_OK;
    if (g.status != FA_OK) return g.status;
    qa.num_pblocks = (int32_t)g.pblocks;
    qa.num_groups = (int32_t)g.groups;
    if (pl.deff == 256) return pl.softcap ? launch_qv_form<T, 256, true>(qa, g.grid, stream) : launch_qv_form<T, 256, false>(qa, g.grid, stream);
    return pl.softcap ? launch_qv_form<T, 512, true>(qa, g.grid, stream) : launch_qv_form<T, 512, false>(qa, g.grid, stream);
}

// the pk kernel (fa_fwd_kernel_pk.h): head-dim tile 64 or 128, plain or softcap
template <typename T, int D>
int launch_pk_form(const FwdPlan &pl, const fa::PkParams &pa, hipStream_t stream) {
    constexpr int smem = fa::smem_bytes<D, fa::PK_NWAVES>(), NT = fa::PK_NWAVES * 64;
    return pl.softcap ? fa::launch_kernel<fa::pk_fwd_kernel<T, D, true>>(smem, pl.grid, NT, stream, pa)
                      : fa::launch_kernel<fa::pk_fwd_kernel<T, D, false>>(smem, pl.grid, NT, stream, pa);
}
template <typename T>
int launch_pk(const FwdPlan &pl, const fa::KParams &kp, hipStream_t stream) {
    fa::PkParams pa{};
    pa.p = kp;
    pa.num_pblocks = pl.num_m_blocks;
    pa.num_groups = kp.b * kp.h_k * kp.num_splits;
    return pl.d == 64 ? launch_pk_form<T, 64>(pl, pa, stream) : launch_pk_form<T, 128>(pl, pa, stream);
}

template <typename T>
int launch_plan(const FwdPlan &pl, const fa_fwd_params *p, const fa::KParams &kp, hipStream_t stream) {
    switch (pl.family) {
        case Family::pk: return launch_pk<T>(pl, kp, stream);
        case Family::fp8: return fa::launch_kernel<fa::fwd_kernel_fp8>(fa::smem_bytes_fp8(), kp.grid, 256, stream, kp);
        case Family::qv: return launch_qv<T>(pl, p, kp, stream);
        case Family::w64: return pl.d == 64 ? launch_w64_form<T, 64>(pl, kp, stream) : launch_w64_form<T, 128>(pl, kp, stream);
        case Family::d256:
            switch (pl.deff) {
                case 64: return launch_d256_form<T, 64>(pl, kp, stream);
                case 96: return launch_d256_form<T, 96>(pl, kp, stream);
                case 128: return launch_d256_form<T, 128>(pl, kp, stream);
                case 160: return launch_d256_form<T, 160>(pl, kp, stream);
                case 192: return launch_d256_form<T, 192>(pl, kp, stream);
                default: return launch_d256_form<T, 256>(pl, kp, stream);
            }
        case Family::generic:
            if (pl.d == 64) return launch_generic<T, 64>(pl, kp, stream);
            if (pl.d == 128) return launch_generic<T, 128>(pl, kp, stream);
            return launch_generic<T, 256>(pl, kp, stream);
    }
    return FA_ERR_UNSUPPORTED;
}

}  // namespace

// ---- fa_fwd_internal.h: what fa_fwd_kv8_api.hip and fa_fwd_qv8_api.hip share with this file ---------------------------------------------------------
namespace fa {
int fwd_pk_split_count(const fa_fwd_params *p) { return split_plan(p, 2, true).splits; }
int fwd_qv_split_count(const fa_fwd_params *p) { return split_plan_qv(p).splits; }
void fwd_set_last_plan_text(const char *text) {
    snprintf(t_last_ext_text, sizeof(t_last_ext_text), "%s", text ? text : "");
    if (t_last_ext_text[0]) {
        t_last_plan_set = false;
        t_last_bs_tile = 0;
    }
}
int fwd_device_cus() { return device_cus(); }
}  // namespace fa

extern "C" {

uint32_t fa_fwd_params_size(void) { return (uint32_t)sizeof(fa_fwd_params); }
uint32_t fa_abi_version(void) { return FA_ABI_VERSION; }

#ifdef FA_TIMING
// developer-only: copy the phase timestamps of the last fwd_kernel_w64 launch (see fa_fwd_kernel_w64.h) to the host
int fa_debug_read_timing(unsigned long long *dst, int n_wg) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(fa::fa_timing_buf), sizeof(unsigned long long) * 32 * n_wg) == hipSuccess ? 0 : -1;
}
#endif
#ifdef FA_F8_DEBUG
// developer-only: read and clear the fp8 block-run counters (see fa_fwd_kernel_fp8.h)
int fa_debug_read_f8(unsigned long long *dst) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(fa::fa_f8_dbg), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(fa::fa_f8_dbg), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif
#ifdef FA_CYCLES
// developer-only: copy the fast-loop cycle stamps of the last fwd_kernel_w64 launch (see fa_fwd_kernel_w64.h) to the host
int fa_debug_read_cycles(unsigned long long *dst) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(fa::fa_cycle_buf), sizeof(unsigned long long) * 256 * 4 * 64) == hipSuccess ? 0 : -1;
}
#endif
void fa_set_default_variant(int32_t variant) { g_default_variant.store(variant); }
void fa_set_persist_mode(int32_t mode) { g_persist_mode.store(mode); }

const char *fa_strerror(int status) {
    switch (status) {
        case FA_OK: return "ok";
        case FA_ERR_NULL_POINTER: return "a required tensor pointer is NULL";
        case FA_ERR_BAD_DTYPE: return "FlashAttention only support fp16 and bf16 data type";
        case FA_ERR_BAD_HEAD_DIM:
            return "FlashAttention forward only supports head dimension at most 256, and head_size must be a multiple of 8";
        case FA_ERR_BAD_HEADS: return "Number of heads in key/value must divide number of heads in query";
        case FA_ERR_BAD_SHAPE: return "batch size must be positive and sequence lengths non-negative";
        case FA_ERR_BAD_STRIDE: return "tensor base pointers and row/head/batch strides must keep rows 16-byte aligned";
        case FA_ERR_UNSUPPORTED: return "feature not supported by this build of the forward";
        case FA_ERR_LAUNCH: return "kernel launch failed";
        case FA_ERR_BAD_ABI: return "fa_fwd_params abi_version/struct_size mismatch";
        case FA_ERR_NO_DEVICE: return "no gfx950 device";
        case FA_ERR_WORKSPACE: return "fp8 inputs need a 256-byte aligned workspace of fa_fwd_workspace_size() bytes";
        default: return "unknown status";
    }
}

int fa_fwd_tile_shape(int32_t d, int32_t dtype, int32_t is_causal, int32_t *block_m, int32_t *block_n) {
    (void)dtype;
    (void)is_causal;
    if (d <= 0 || d > 256 || d % 8) return FA_ERR_BAD_HEAD_DIM;
    if (block_m) *block_m = block_m_of(g_default_variant.load(), d);
    if (block_n) *block_n = fa::BLOCK_N;
    return FA_OK;
}

uint32_t fa_kvcache_append_params_size(void) { return (uint32_t)sizeof(fa_kvcache_append_params); }

int fa_kvcache_append(const fa_kvcache_append_params *p, void *stream_) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_kvcache_append_params)) return FA_ERR_BAD_ABI;
    if (p->b <= 0 || p->h_k <= 0 || p->seqlen_new < 0 || p->seqlen_cache < 0) return FA_ERR_BAD_SHAPE;
    if (p->d <= 0 || p->d > 256 || p->d % 8 != 0) return FA_ERR_BAD_HEAD_DIM;
    if (p->d_v < 0 || p->d_v > 512 || p->d_v % 8 != 0) return FA_ERR_BAD_HEAD_DIM;  // 0 = d
    if (p->seqlen_new == 0) return FA_OK;
    if (!p->k_new || !p->v_new || !p->k_cache || !p->v_cache || !p->cache_seqlens) return FA_ERR_NULL_POINTER;
    if (p->block_table && (p->page_block_size <= 0 || p->cache_batch_idx)) return FA_ERR_BAD_SHAPE;
    if (p->rotary_cos) {
        if (!p->rotary_sin) return FA_ERR_NULL_POINTER;
        if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16) return FA_ERR_BAD_DTYPE;
        if (p->rotary_dim <= 0 || p->rotary_dim > p->d || p->rotary_dim % 16 != 0) return FA_ERR_BAD_SHAPE;  // (:1409-1410)
        if (reinterpret_cast<uintptr_t>(p->rotary_cos) % 16 != 0 || reinterpret_cast<uintptr_t>(p->rotary_sin) % 16 != 0)
            return FA_ERR_BAD_STRIDE;
    }
    const int64_t strides[] = {p->knew_batch_stride, p->knew_row_stride, p->knew_head_stride, p->vnew_batch_stride,
                               p->vnew_row_stride, p->vnew_head_stride, p->kcache_batch_stride, p->kcache_row_stride,
                               p->kcache_head_stride, p->vcache_batch_stride, p->vcache_row_stride, p->vcache_head_stride};
    for (int64_t s : strides)
        if (s % 8 != 0) return FA_ERR_BAD_STRIDE;
    const void *ptrs[] = {p->k_new, p->v_new, p->k_cache, p->v_cache};
    for (const void *ptr : ptrs)
        if (reinterpret_cast<uintptr_t>(ptr) % 16 != 0) return FA_ERR_BAD_STRIDE;
    const int dv = p->d_v > 0 ? p->d_v : p->d;
    const int64_t total = (int64_t)p->b * p->seqlen_new * p->h_k * std::max((p->d / 8 + 1) / 2, (dv / 8 + 1) / 2);
    const int blocks = (int)std::min<int64_t>((total + 255) / 256, 256 * 8);
    if (p->rotary_cos && p->dtype == FA_DTYPE_FP16)
        hipLaunchKernelGGL(kvcache_append_kernel<_Float16>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream_), *p);
    else  // (without rotary the element type does not matter: plain 16-byte copies)
        hipLaunchKernelGGL(kvcache_append_kernel<__bf16>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream_), *p);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

uint32_t fa_rotary_params_size(void) { return (uint32_t)sizeof(fa_rotary_params); }

int fa_rotary_apply(const fa_rotary_params *p, void *stream_) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_rotary_params)) return FA_ERR_BAD_ABI;
    if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16) return FA_ERR_BAD_DTYPE;
    if (p->b <= 0 || p->h <= 0 || p->s < 0) return FA_ERR_BAD_SHAPE;
    if (p->d <= 0 || p->d > 256 || p->d % 8 != 0) return FA_ERR_BAD_HEAD_DIM;
    if (p->rotary_dim <= 0 || p->rotary_dim > p->d || p->rotary_dim % 16 != 0) return FA_ERR_BAD_SHAPE;
    if (p->s == 0) return FA_OK;
    if (!p->src || !p->dst || !p->rotary_cos || !p->rotary_sin || !p->seqlen_offsets) return FA_ERR_NULL_POINTER;
    const int64_t strides[] = {p->src_batch_stride, p->src_row_stride, p->src_head_stride, p->dst_batch_stride,
                               p->dst_row_stride, p->dst_head_stride};
    for (int64_t s : strides)
        if (s % 8 != 0) return FA_ERR_BAD_STRIDE;
    const void *ptrs[] = {p->src, p->dst, p->rotary_cos, p->rotary_sin};
    for (const void *ptr : ptrs)
        if (reinterpret_cast<uintptr_t>(ptr) % 16 != 0) return FA_ERR_BAD_STRIDE;
    const int64_t total = (int64_t)p->b * p->s * p->h * ((p->d / 8 + 1) / 2);
    const int blocks = (int)std::min<int64_t>((total + 255) / 256, 256 * 8);
    if (p->dtype == FA_DTYPE_FP16)
        hipLaunchKernelGGL(rotary_kernel<_Float16>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream_), *p);
    else
        hipLaunchKernelGGL(rotary_kernel<__bf16>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream_), *p);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

uint32_t fa_kvcache_append_varlen_params_size(void) { return (uint32_t)sizeof(fa_kvcache_append_varlen_params); }

int fa_kvcache_append_varlen(const fa_kvcache_append_varlen_params *p, void *stream_) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_kvcache_append_varlen_params)) return FA_ERR_BAD_ABI;
    if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16) return FA_ERR_BAD_DTYPE;
    if (p->b <= 0 || p->h_k <= 0 || p->total_k_new < 0 || p->max_seqlen_k_new < 0 || p->seqlen_cache < 0) return FA_ERR_BAD_SHAPE;
    if (p->d <= 0 || p->d > 256 || p->d % 8 != 0) return FA_ERR_BAD_HEAD_DIM;
    if (p->d_v < 0 || p->d_v > 512 || p->d_v % 8 != 0) return FA_ERR_BAD_HEAD_DIM;  // 0 = d
    if (!p->cu_seqlens_k_new || !p->cache_seqlens || !p->seqused_out) return FA_ERR_NULL_POINTER;
    if (p->total_k_new > 0 && (!p->k_new || !p->v_new || !p->k_cache || !p->v_cache)) return FA_ERR_NULL_POINTER;
    if (p->block_table && (p->page_block_size <= 0 || p->cache_batch_idx)) return FA_ERR_BAD_SHAPE;
    if (p->block_table && (p->block_table_batch_stride < 0 || p->block_table_batch_stride > 0x7fffffff)) return FA_ERR_BAD_STRIDE;
    if (p->rotary_cos) {
        if (!p->rotary_sin) return FA_ERR_NULL_POINTER;
        if (p->rotary_dim <= 0 || p->rotary_dim > p->d || p->rotary_dim % 16 != 0) return FA_ERR_BAD_SHAPE;
        if (reinterpret_cast<uintptr_t>(p->rotary_cos) % 16 != 0 || reinterpret_cast<uintptr_t>(p->rotary_sin) % 16 != 0)
            return FA_ERR_BAD_STRIDE;
    }
    const int64_t strides[] = {p->knew_row_stride, p->knew_head_stride, p->vnew_row_stride, p->vnew_head_stride,
                               p->kcache_batch_stride, p->kcache_row_stride, p->kcache_head_stride,
                               p->vcache_batch_stride, p->vcache_row_stride, p->vcache_head_stride};
    for (int64_t s : strides)
        if (s % 8 != 0) return FA_ERR_BAD_STRIDE;
    const void *ptrs[] = {p->k_new, p->v_new, p->k_cache, p->v_cache};
    for (const void *ptr : ptrs)
        if (reinterpret_cast<uintptr_t>(ptr) % 16 != 0) return FA_ERR_BAD_STRIDE;
    fa_kvcache_append_varlen_params kp = *p;
    if (kp.b > 65535 || kp.total_k_new == 0) kp.max_seqlen_k_new = 0;  // (grid.y; no rows: the launch only writes seqused_out)
    dim3 grid;
    size_t smem;
    ragged_launch_shape(kp.b, kp.total_k_new, kp.max_seqlen_k_new, kp.b, grid, smem);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (p->dtype == FA_DTYPE_FP16) hipLaunchKernelGGL(kvcache_append_varlen_kernel<_Float16>, grid, dim3(256), smem, stream, kp);
    else hipLaunchKernelGGL(kvcache_append_varlen_kernel<__bf16>, grid, dim3(256), smem, stream, kp);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

uint32_t fa_rotary_varlen_params_size(void) { return (uint32_t)sizeof(fa_rotary_varlen_params); }

int fa_rotary_apply_varlen(const fa_rotary_varlen_params *p, void *stream_) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_rotary_varlen_params)) return FA_ERR_BAD_ABI;
    if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16) return FA_ERR_BAD_DTYPE;
    if (p->b <= 0 || p->h <= 0 || p->total_q < 0 || p->max_seqlen_q < 0) return FA_ERR_BAD_SHAPE;
    if (p->d <= 0 || p->d > 256 || p->d % 8 != 0) return FA_ERR_BAD_HEAD_DIM;
    if (p->rotary_dim <= 0 || p->rotary_dim > p->d || p->rotary_dim % 16 != 0) return FA_ERR_BAD_SHAPE;
    if (p->total_q == 0) return FA_OK;
    if (!p->src || !p->dst || !p->rotary_cos || !p->rotary_sin || !p->cu_seqlens_q || !p->offsets) return FA_ERR_NULL_POINTER;
    const int64_t strides[] = {p->src_row_stride, p->src_head_stride, p->dst_row_stride, p->dst_head_stride};
    for (int64_t s : strides)
        if (s % 8 != 0) return FA_ERR_BAD_STRIDE;
    const void *ptrs[] = {p->src, p->dst, p->rotary_cos, p->rotary_sin};
    for (const void *ptr : ptrs)
        if (reinterpret_cast<uintptr_t>(ptr) % 16 != 0) return FA_ERR_BAD_STRIDE;
    fa_rotary_varlen_params kp = *p;
    if (kp.b > 65535) kp.max_seqlen_q = 0;  // (grid.y)
    dim3 grid;
    size_t smem;
    ragged_launch_shape(kp.b, kp.total_q, kp.max_seqlen_q, 0, grid, smem);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (p->dtype == FA_DTYPE_FP16) hipLaunchKernelGGL(rotary_varlen_kernel<_Float16>, grid, dim3(256), smem, stream, kp);
    else hipLaunchKernelGGL(rotary_varlen_kernel<__bf16>, grid, dim3(256), smem, stream, kp);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

uint32_t fa_combine_params_size(void) { return (uint32_t)sizeof(fa_combine_params); }

int fa_fwd_combine(const fa_combine_params *p, void *stream_) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_combine_params)) return FA_ERR_BAD_ABI;
    if (p->out_dtype != FA_DTYPE_FP32 && p->out_dtype != FA_DTYPE_FP16 && p->out_dtype != FA_DTYPE_BF16) return FA_ERR_BAD_DTYPE;
    if (p->num_splits <= 0 || p->num_splits > 256) return FA_ERR_BAD_SHAPE;  // "combine only supports num_splits at most 256"
    if (p->b < 0 || p->seqlen < 0 || p->h <= 0 || p->d <= 0) return FA_ERR_BAD_SHAPE;
    if (p->b == 0 || p->seqlen == 0) return FA_OK;
    if (!p->out_partial || !p->lse_partial || !p->out || !p->softmax_lse) return FA_ERR_NULL_POINTER;
    const int64_t total = (int64_t)p->b * p->seqlen * p->h * ((p->d + 3) / 4);
    const int blocks = (int)std::min<int64_t>((total + 255) / 256, 256 * 16);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (p->out_dtype == FA_DTYPE_FP32) hipLaunchKernelGGL(combine_partials_kernel<float>, dim3(blocks), dim3(256), 0, stream, *p);
    else if (p->out_dtype == FA_DTYPE_FP16) hipLaunchKernelGGL(combine_partials_kernel<_Float16>, dim3(blocks), dim3(256), 0, stream, *p);
    else hipLaunchKernelGGL(combine_partials_kernel<__bf16>, dim3(blocks), dim3(256), 0, stream, *p);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

int64_t fa_fwd_workspace_size(const fa_fwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_fwd_params)) return FA_ERR_BAD_ABI;
    if (p->b <= 0 || p->h <= 0 || p->h_k <= 0 || p->d <= 0 || p->seqlen_q < 0 || p->seqlen_k < 0) return FA_ERR_BAD_SHAPE;
    if (p->cu_seqlens_q && (p->total_q < 0 || p->total_k < 0)) return FA_ERR_BAD_SHAPE;
    return plan_fwd(p, 0).workspace;
}

int fa_fwd_validate(const fa_fwd_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_fwd_params)) return FA_ERR_BAD_ABI;
    if (p->dtype != FA_DTYPE_FP16 && p->dtype != FA_DTYPE_BF16 && p->dtype != FA_DTYPE_FP8_E4M3) return FA_ERR_BAD_DTYPE;
    if (p->b <= 0 || p->h <= 0 || p->h_k <= 0 || p->seqlen_q < 0 || p->seqlen_k < 0) return FA_ERR_BAD_SHAPE;
    if (p->d <= 0 || p->d > 256 || p->d % 8 != 0) return FA_ERR_BAD_HEAD_DIM;
    const bool fp8 = p->dtype == FA_DTYPE_FP8_E4M3;
    if (fp8 && p->d % 16 != 0) return FA_ERR_BAD_HEAD_DIM;  // hopper/flash_api.cpp:854-856
    if (p->attention_chunk < 0) return FA_ERR_BAD_SHAPE;
    if (p->d_v < 0 || p->d_v > 512 || p->d_v % 8 != 0) return FA_ERR_BAD_HEAD_DIM;  // 0 = d
    const FwdPlan pl = plan_fwd(p, 0);  // (the CU count decides the persistent form only)
    if (p->qv) {  // ABI v13 (hopper/flash_api.cpp:1028-1048): d <= 64, 256 <= d_v <= 512, 16-bit; no ALiBi / dropout in FA3
        if (fp8 || !qv_shape(p) || p->alibi_slopes || p->p_dropout > 0.f) return FA_ERR_UNSUPPORTED;
        if (p->qv_row_stride % 8 != 0 || p->qv_head_stride % 8 != 0 || (!p->cu_seqlens_q && p->qv_batch_stride % 8 != 0) ||
            reinterpret_cast<uintptr_t>(p->qv) % 16 != 0)
            return FA_ERR_BAD_STRIDE;
    }
    const bool qv_kernel = pl.family == Family::qv;
    if (own_dv(p) && (fp8 || p->block_table || p->num_splits > 1) && !qv_kernel) return FA_ERR_UNSUPPORTED;
    if (qv_kernel && p->alibi_slopes) return FA_ERR_UNSUPPORTED;
    if (generic_only(p) && p->p_dropout > 0.f) return FA_ERR_UNSUPPORTED;  // (no dropout on the FA3 surface)
    if (p->attention_chunk > 0 && p->s_dmask) return FA_ERR_UNSUPPORTED;  // (the S_dmask pass knows windows only)
    if (p->h % p->h_k != 0) return FA_ERR_BAD_HEADS;
    if (p->cu_seqlens_k && !p->cu_seqlens_q) return FA_ERR_BAD_SHAPE;
    const bool ragged = ragged_cache(p);  // ragged queries over a batched cache: the fill levels come through seqused_k
    if (ragged && !p->seqused_k) return FA_ERR_BAD_SHAPE;
    if (ragged && (fp8 || p->p_dropout > 0.f || p->alibi_slopes)) return FA_ERR_UNSUPPORTED;  // (what the FA3 cache route refuses)
    if (p->cu_seqlens_q && p->total_q < 0) return FA_ERR_BAD_SHAPE;
    const bool empty = (p->seqlen_q == 0) || (p->cu_seqlens_q && p->total_q == 0);
    if (!empty) {
        if (!p->q || !p->o || !p->softmax_lse) return FA_ERR_NULL_POINTER;
        if (p->seqlen_k > 0 && (!p->k || !p->v)) return FA_ERR_NULL_POINTER;
    }
    // 16-byte vector loads/stores: bases and strides must keep every row 16-byte aligned
    // (fp8 sources are read 8 bytes at a time by the expansion pass: same multiple-of-8-elements rule)
    const int64_t strides[] = {p->q_row_stride, p->q_head_stride, p->k_row_stride, p->k_head_stride,
                               p->v_row_stride, p->v_head_stride, p->o_row_stride, p->o_head_stride};
    for (int64_t s : strides)
        if (s % 8 != 0) return FA_ERR_BAD_STRIDE;
    // the kernel addresses a K/V tile as 64-bit tile base + 32-bit (row * stride) lane offset
    if (p->k_row_stride < 0 || p->v_row_stride < 0 || p->k_row_stride >= (1 << 24) || p->v_row_stride >= (1 << 24))
        return FA_ERR_BAD_STRIDE;
    if (!p->cu_seqlens_q) {
        const int64_t bs[] = {p->q_batch_stride, p->k_batch_stride, p->v_batch_stride, p->o_batch_stride};
        for (int64_t s : bs)
            if (s % 8 != 0) return FA_ERR_BAD_STRIDE;
    } else if (ragged && (p->k_batch_stride % 8 != 0 || p->v_batch_stride % 8 != 0)) {
        return FA_ERR_BAD_STRIDE;
    }
    const void *ptrs[] = {p->q, p->k, p->v, p->o};
    for (const void *ptr : ptrs)
        if (reinterpret_cast<uintptr_t>(ptr) % (fp8 && ptr != p->o ? 8 : 16) != 0) return FA_ERR_BAD_STRIDE;
    if (pl.fp8_expand && !pl.nothing && fa::workspace_short(p, pl.fp8.total)) return FA_ERR_WORKSPACE;
    if (p->num_splits < 0) return FA_ERR_BAD_SHAPE;
    if (pl.split.splits > 1 && fa::workspace_short(p, pl.split.total)) return FA_ERR_WORKSPACE;
    if (p->softcap < 0.f || std::isnan(p->softcap) || std::isnan(p->softmax_scale)) return FA_ERR_BAD_SHAPE;
    if (p->alibi_slopes && (reinterpret_cast<uintptr_t>(p->alibi_slopes) % 4 != 0 || p->alibi_slopes_batch_stride < 0 ||
                            p->alibi_slopes_batch_stride > 0x7fffffff))
        return FA_ERR_BAD_STRIDE;
    if (!(p->p_dropout >= 0.f && p->p_dropout < 1.f)) return FA_ERR_BAD_SHAPE;  // "p_dropout must be in [0, 1)"
    if (p->p_dropout > 0.f) {
        if (fp8 || p->block_table || p->kv_batch_idx || p->leftpad_k) return FA_ERR_UNSUPPORTED;  // training path only
        if (p->softcap > 0.f) return FA_ERR_UNSUPPORTED;  // "Softcapping does not support dropout for now" (flash_api.cpp:377)
        if (!p->rng_state || reinterpret_cast<uintptr_t>(p->rng_state) % 8 != 0) return FA_ERR_NULL_POINTER;
    } else if (p->s_dmask) {
        return FA_ERR_UNSUPPORTED;  // the randval tensor only exists under dropout
    }
    if ((p->flags & FA_FLAG_SDMASK_SIGNED) && p->s_dmask) {
        if (p->s_dmask_rows < p->seqlen_q || p->s_dmask_cols < p->seqlen_k || p->s_dmask_block_n <= 0) return FA_ERR_BAD_SHAPE;
        if (p->seqlen_k > 32768) return FA_ERR_UNSUPPORTED;  // (one row of scores in LDS)
    }
    if (p->kv_batch_idx && (p->cu_seqlens_k || fp8)) return FA_ERR_UNSUPPORTED;  // dense 16-bit caches only (ragged queries included)
    if (p->leftpad_k && (p->block_table || fp8)) return FA_ERR_UNSUPPORTED;  // (:1396 "Paged KV and leftpad_k" not together)
    if (p->block_table) {
        if (fp8 || p->kv_batch_idx) return FA_ERR_UNSUPPORTED;  // "Paged KVcache does not support cache_batch_idx" (:1247)
        if (p->page_block_size <= 0) return FA_ERR_BAD_SHAPE;  // any size (the FA2 entry point keeps its % 256 rule in Python)
        if (p->block_table_batch_stride < 0 || p->block_table_batch_stride > 0x7fffffff) return FA_ERR_BAD_STRIDE;
    }
    return FA_OK;
}

const char *fa_fwd_plan_name(const fa_fwd_params *p, int32_t num_cus) {
    if (fa_fwd_validate(p) != FA_OK) return nullptr;
    thread_local char name[160];
    return plan_text(plan_fwd(p, num_cus), name);
}

const char *fa_fwd_last_plan_name(void) {
    thread_local char name[160];
    if (t_last_ext_text[0]) return t_last_ext_text;
    if (t_last_bs_tile) {  // the block-sparse kernel has one shape: 4 waves x 32 rows = one 128-row block, never split
        snprintf(name, sizeof(name), "bs_fwd_kernel D=%d waves=%d%s block_m=%d splits=1", t_last_bs_tile, fa::BS_NWAVES,
                 t_last_bs_softcap ? " SOFTCAP" : "", fa::BS_BLOCK);
        return name;
    }
    return t_last_plan_set ? plan_text(t_last_plan, name) : nullptr;
}

uint32_t fa_sink_params_size(void) { return (uint32_t)sizeof(fa_sink_params); }

// The sink's own checks come first: what a sink cannot go with is refused as such, whatever else those params lack.
int fa_fwd_sink_validate(const fa_fwd_params *p, const fa_sink_params *s) {
    if (!p || !s) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_fwd_params)) return FA_ERR_BAD_ABI;
    if (s->abi_version != FA_ABI_VERSION || s->struct_size != sizeof(fa_sink_params)) return FA_ERR_BAD_ABI;
    if (!s->learnable_sink) return FA_ERR_NULL_POINTER;
    if (s->sink_dtype != FA_DTYPE_BF16 && s->sink_dtype != FA_DTYPE_FP32) return FA_ERR_BAD_DTYPE;
    if (reinterpret_cast<uintptr_t>(s->learnable_sink) % (s->sink_dtype == FA_DTYPE_FP32 ? 4 : 2) != 0) return FA_ERR_BAD_STRIDE;
    if (s->sink_head_stride < 0 || s->sink_row_stride < 0) return FA_ERR_BAD_STRIDE;
    if (s->sink_row_stride != 0 && p->cu_seqlens_q) return FA_ERR_BAD_STRIDE;  // (rows of a ragged batch are not rows of a GQA group)
    // the reference's sink surface has none of these (flash_attn/cute/interface.py)
    if (p->dtype == FA_DTYPE_FP8_E4M3 || p->qv || p->p_dropout > 0.f || p->alibi_slopes || p->s_dmask) return FA_ERR_UNSUPPORTED;
    const int st = fa_fwd_validate(p);
    if (st != FA_OK) return st;
    const Family f = plan_fwd(p, 0).family;  // (q/k <= 64 beside a paged or split V of 256..512 columns runs the qv kernel)
    if (f == Family::qv || f == Family::fp8) return FA_ERR_UNSUPPORTED;
    return FA_OK;
}

static int fwd_run(const fa_fwd_params *p, const fa_sink_params *sink, void *stream_);

int fa_fwd(const fa_fwd_params *p, void *stream_) { return fwd_run(p, nullptr, stream_); }

int fa_fwd_sink(const fa_fwd_params *p, const fa_sink_params *sink, void *stream_) {
    if (!sink) return FA_ERR_NULL_POINTER;
    return fwd_run(p, sink, stream_);
}

// fa_fwd and fa_fwd_sink: the plan is made from `p` alone -- a sink never changes it
static int fwd_run(const fa_fwd_params *p, const fa_sink_params *sink, void *stream_) {
    const int st = sink ? fa_fwd_sink_validate(p, sink) : fa_fwd_validate(p);
    t_last_plan_set = false;
    t_last_bs_tile = 0;
    t_last_ext_text[0] = 0;
    if (st != FA_OK) return st;
    hipStream_t stream = static_cast<hipStream_t>(stream_);

    const int num_cus = device_cus();
    const FwdPlan pl = plan_fwd(p, num_cus);
    t_last_plan = pl;
    t_last_plan_set = true;
    if (pl.cols > 1) {
        // one call per 256 columns of V and O -- the scores are formed again for each (d <= 64: a small part of the work), the LSE
        // is written by every call with the same value.  Strides are untouched: the calls differ in the V / O column offset only.
        for (int c = 0; c < p->d_v; c += 256) {
            fa_fwd_params part = *p;
            part.v = static_cast<const char *>(p->v) + (size_t)c * 2;
            part.o = static_cast<char *>(p->o) + (size_t)c * 2;
            part.d_v = std::min(256, p->d_v - c);
            const int st_part = fwd_run(&part, sink, stream_);
            if (st_part != FA_OK) return st_part;
        }
        t_last_plan = pl;  // (the outer plan, "... cols=2": the parts recorded theirs)
        t_last_plan_set = true;
        return FA_OK;
    }

    fa::KParams kp{};
    fa::fwd_fill_params(p, own_dv(p) ? p->d_v : p->d, kp);
    const bool fp8 = p->dtype == FA_DTYPE_FP8_E4M3;
    int64_t ws_q_row = 0, ws_k_row = 0;
    if (pl.fp8_expand && !pl.nothing) {
        const Fp8Plan &fp = pl.fp8;
        char *ws = static_cast<char *>(p->workspace);
        const int rpb_q = p->cu_seqlens_q ? 0 : p->seqlen_q, rpb_k = p->cu_seqlens_q ? 0 : p->seqlen_k;
        auto expand = [&](const void *src, void *dst, int64_t rows, int rpb, int heads, int64_t bs, int64_t rs, int64_t hs) {
            const int64_t total = rows * heads * (p->d / 8);
            if (total == 0) return;
            const int blocks = (int)std::min<int64_t>((total + 255) / 256, 256 * 8);
            hipLaunchKernelGGL(expand_fp8_kernel, dim3(blocks), dim3(256), 0, stream, static_cast<const uint8_t *>(src),
                               static_cast<uint32_t *>(dst), rows, rpb, heads, p->d, bs, rs, hs);
        };
        expand(p->q, ws, fp.rows_q, rpb_q, p->h, p->q_batch_stride, p->q_row_stride, p->q_head_stride);
        expand(p->k, ws + fp.q_bytes, fp.rows_k, rpb_k, p->h_k, p->k_batch_stride, p->k_row_stride, p->k_head_stride);
        expand(p->v, ws + fp.q_bytes + fp.kv_bytes, fp.rows_k, rpb_k, p->h_k, p->v_batch_stride, p->v_row_stride, p->v_head_stride);
        if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
        kp.q = ws; kp.k = ws + fp.q_bytes; kp.v = ws + fp.q_bytes + fp.kv_bytes;
        ws_q_row = (int64_t)p->h * p->d;
        ws_k_row = (int64_t)p->h_k * p->d;
    }
    if (fp8) {
        if (pl.fp8_expand) {  // the expanded copies are contiguous (rows, heads, d)
            kp.q_row_stride = ws_q_row; kp.q_head_stride = p->d; kp.q_batch_stride = ws_q_row * p->seqlen_q;
            kp.k_row_stride = kp.v_row_stride = ws_k_row; kp.k_head_stride = kp.v_head_stride = p->d;
            kp.k_batch_stride = kp.v_batch_stride = ws_k_row * p->seqlen_k;
        }
        kp.q_descale = p->q_descale;  // (16-bit calls: the kernels get no descales, whatever the caller's fields hold)
        kp.qd_bs = (int32_t)p->q_descale_batch_stride; kp.qd_hs = (int32_t)p->q_descale_head_stride;
        fa::fwd_fill_kv_descales(p, kp);
    }
    kp.chunk = p->attention_chunk;
    kp.num_m_blocks = pl.num_m_blocks;
    if (pl.tiles == 0) return FA_OK;  // nothing to compute (seqlen_q == 0)
    if (pl.status != FA_OK) return pl.status;
    kp.num_tiles = (int32_t)pl.tiles;
    kp.unit_tiles = (int32_t)pl.unit_tiles;
    kp.whole_slots = (int32_t)pl.whole_slots;
    kp.grid = (int32_t)pl.grid;
    kp.num_cus = num_cus;
    // split-KV: `splits` copies of the grid; partial results go to the workspace and are merged below
    // (kp.dv columns: d_v on the qv kernel's path, d on the others -- they never split with a V head dim of its own)
    const SplitPlan &sp = pl.split;
    kp.num_splits = sp.splits;
    if (sp.splits > 1) fa::split_redirect(p, sp, kp);

    kp.alibi = p->alibi_slopes;
    kp.alibi_bs = (int32_t)p->alibi_slopes_batch_stride;
    // dropout: keep iff randval <= floor(255 (1 - p)); 255 = everything kept = the branch is off
    // (the 8-bit quantisation of the reference's ROCm back-end: any p > 0 gives a threshold <= 254, i.e. at least 1/256 of the
    //  elements are dropped however small p is; the kept ones are scaled by 1 / (1 - p))
    kp.drop_thr = p->p_dropout > 0.f ? (int32_t)std::floor(255.0 * (1.0 - (double)p->p_dropout)) : 255;
    kp.rp_dropout = rp_dropout(p);
    kp.rng_state = p->rng_state;
    const bool sdmask_signed = (p->flags & FA_FLAG_SDMASK_SIGNED) && p->s_dmask;
    kp.s_dmask = sdmask_signed ? nullptr : p->s_dmask;
    // the sink: an epilogue term of the kernel, or -- split-KV: the parts write sink-free partials -- of the merge
    fa::KParams sink_kp{};
    if (sink) {
        sink_kp.sink = sink->learnable_sink;
        sink_kp.sink_hs = sink->sink_head_stride; sink_kp.sink_rs = sink->sink_row_stride;
        sink_kp.sink_fp32 = sink->sink_dtype == FA_DTYPE_FP32;
        if (sp.splits <= 1) {
            kp.sink = sink_kp.sink; kp.sink_hs = sink_kp.sink_hs; kp.sink_rs = sink_kp.sink_rs; kp.sink_fp32 = sink_kp.sink_fp32;
        }
    }

    const bool bf16 = p->dtype == FA_DTYPE_BF16 || fp8;  // fp8: out is bf16
    const int st_main = bf16 ? launch_plan<__bf16>(pl, p, kp, stream) : launch_plan<_Float16>(pl, p, kp, stream);
    if (st_main == FA_OK && sdmask_signed && !pl.nothing) {
        const int nrb = (p->seqlen_q + 7) / 8;
        const int64_t blocks = (int64_t)nrb * p->h * p->b;
        const int nblk = (p->seqlen_k + p->s_dmask_block_n - 1) / p->s_dmask_block_n;
        const size_t smem = sizeof(float) * ((size_t)8 * p->d + ((p->seqlen_k + 3) & ~3) + nblk + 4);
        if (blocks > 0x7fffffff) return FA_ERR_BAD_SHAPE;
        auto launch_sd = [&](auto tag) -> int {
            using T = decltype(tag);
            auto kernel = sdmask_kernel<T>;
            if (smem > 65536 &&
                hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) {
                (void)hipGetLastError();
                return FA_ERR_LAUNCH;
            }
            hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), smem, stream, kp, reinterpret_cast<T *>(p->s_dmask),
                               p->s_dmask_rows, p->s_dmask_cols, p->s_dmask_block_n);
            return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
        };
        const int st_sd = bf16 ? launch_sd(__bf16{}) : launch_sd(_Float16{});
        if (st_sd != FA_OK) return st_sd;
    }
    if (st_main != FA_OK || sp.splits <= 1) return st_main;
    // merge the partial results into the caller's out / softmax_lse.  Ragged queries are one "batch" of total_q rows to the
    // merge: its partials are then (splits, 1, total_q, h, d) / (splits, 1, h, total_q) and out / lse (total_q, h, d) / (h, total_q)
    const int dw = dv_of(p);  // (= d on every path but the qv kernel's: the others never split with a V head dim of its own)
    const int mb = p->cu_seqlens_q ? 1 : p->b, msq = p->cu_seqlens_q ? p->total_q : p->seqlen_q;
    const int64_t total = (int64_t)mb * msq * p->h * (dw / 8);
    const int blocks = (int)std::min<int64_t>((total + 255) / 256, 256 * 8);
    if (bf16)
        hipLaunchKernelGGL(combine_splits_kernel<__bf16>, dim3(blocks), dim3(256), 0, stream, static_cast<const float *>(kp.o),
                           kp.lse, static_cast<__bf16 *>(p->o), p->softmax_lse, sp.splits, mb, msq, p->h, dw,
                           p->o_batch_stride, p->o_row_stride, p->o_head_stride, sink_kp);
    else
        hipLaunchKernelGGL(combine_splits_kernel<_Float16>, dim3(blocks), dim3(256), 0, stream,
                           static_cast<const float *>(kp.o), kp.lse, static_cast<_Float16 *>(p->o), p->softmax_lse,
                           sp.splits, mb, msq, p->h, dw, p->o_batch_stride, p->o_row_stride, p->o_head_stride, sink_kp);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

// ---- block-sparse forward (include/fa_fwd.h, fa_fwd_kernel_bs.h) ---------------------------------------------------------
uint32_t fa_block_sparse_params_size(void) { return (uint32_t)sizeof(fa_block_sparse_params); }

// the params as the block-sparse launch reads them: never split (num_splits 0 / 1 both mean one part)
static fa_fwd_params bs_dense_params(const fa_fwd_params *p) {
    fa_fwd_params q = *p;
    q.num_splits = 1;
    return q;
}

// The refusals come first: what block sparsity cannot go with is refused as such, whatever else those params lack.
int fa_fwd_block_sparse_validate(const fa_fwd_params *p, const fa_block_sparse_params *s, const fa_sink_params *sink) {
    if (!p || !s) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_fwd_params)) return FA_ERR_BAD_ABI;
    if (s->abi_version != FA_ABI_VERSION || s->struct_size != sizeof(fa_block_sparse_params)) return FA_ERR_BAD_ABI;
    if (s->block_m != fa::BS_BLOCK || s->block_n != fa::BS_BLOCK) return FA_ERR_UNSUPPORTED;
    // the reference refuses block sparsity with varlen too (flash_attn/cute/interface.py); the others have no list semantics here
    if (p->cu_seqlens_q || p->cu_seqlens_k || p->seqused_q || p->seqused_k || p->block_table || p->kv_batch_idx || p->leftpad_k)
        return FA_ERR_UNSUPPORTED;
    if (p->dtype == FA_DTYPE_FP8_E4M3 || p->qv || p->p_dropout > 0.f || p->s_dmask || p->alibi_slopes || p->attention_chunk != 0 ||
        p->num_splits > 1 || p->d_v > 256)
        return FA_ERR_UNSUPPORTED;
    if (!s->mask_block_cnt || !s->mask_block_idx) return FA_ERR_NULL_POINTER;
    if ((s->full_block_cnt == nullptr) != (s->full_block_idx == nullptr)) return FA_ERR_NULL_POINTER;
    const void *lists[] = {s->full_block_cnt, s->full_block_idx, s->mask_block_cnt, s->mask_block_idx};
    for (const void *l : lists)
        if (reinterpret_cast<uintptr_t>(l) % 4 != 0) return FA_ERR_BAD_STRIDE;
    const int64_t *strides[] = {s->full_cnt_stride, s->full_idx_stride, s->mask_cnt_stride, s->mask_idx_stride};
    for (const int64_t *st : strides)
        for (int i = 0; i < 4; ++i)
            if (st[i] < 0) return FA_ERR_BAD_STRIDE;
    const fa_fwd_params dense = bs_dense_params(p);
    return sink ? fa_fwd_sink_validate(&dense, sink) : fa_fwd_validate(&dense);
}

}  // extern "C"

namespace {
template <typename T>
int launch_bs(int tile, bool softcap, const fa::BsParams &bp, hipStream_t stream) {
    const int64_t grid = bp.p.grid;
    constexpr int NT = fa::BS_NWAVES * 64;
#define FA_BS_LAUNCH(D)                                                                                                        \
    return softcap ? fa::launch_kernel<fa::bs_fwd_kernel<T, D, true>>(fa::smem_bytes<D, fa::BS_NWAVES>(), grid, NT, stream, bp) \
                   : fa::launch_kernel<fa::bs_fwd_kernel<T, D, false>>(fa::smem_bytes<D, fa::BS_NWAVES>(), grid, NT, stream, bp)
    if (tile == 64) { FA_BS_LAUNCH(64); }
    if (tile == 128) { FA_BS_LAUNCH(128); }
    FA_BS_LAUNCH(256);
#undef FA_BS_LAUNCH
}
}  // namespace

extern "C" {

int fa_fwd_block_sparse(const fa_fwd_params *p_, const fa_block_sparse_params *s, const fa_sink_params *sink, void *stream_) {
    const int st = fa_fwd_block_sparse_validate(p_, s, sink);
    t_last_plan_set = false;
    t_last_bs_tile = 0;
    t_last_ext_text[0] = 0;
    if (st != FA_OK) return st;
    const fa_fwd_params dense = bs_dense_params(p_), *p = &dense;
    hipStream_t stream = static_cast<hipStream_t>(stream_);

    fa::BsParams bp{};
    fa::KParams &kp = bp.p;
    // (the call's own mask is bottom-right aligned, fa_fwd's window rule; the sequence-length and cache fields validate has
    // seen NULL, and bs_fwd_kernel reads neither them nor total_q / bt_bs / page_size)
    fa::fwd_fill_params(p, dv_of(p), kp);
    kp.num_splits = 1;
    kp.num_cus = device_cus();
    // one work item per (batch, head, 128-row block): fwd_kernel's scheduling (tile_of_wg) with block_m = 128
    const int64_t nm = ((int64_t)p->seqlen_q + fa::BS_BLOCK - 1) / fa::BS_BLOCK;
    const int64_t tiles = nm * p->h * p->b;
    if (tiles == 0) return FA_OK;  // no query row
    const int64_t bk_units = (int64_t)p->b * p->h_k, per_kvh = (int64_t)kp.h_ratio * nm;
    const int64_t whole_units = bk_units >= 16 ? bk_units / 8 * 8 : 0;
    const int64_t whole_slots = whole_units / 8 * per_kvh;
    const int64_t rem_units = (tiles - whole_slots * 8 + kp.h_ratio - 1) / kp.h_ratio;
    const int64_t grid = 8 * (whole_slots + (rem_units + 7) / 8 * kp.h_ratio);
    if (tiles > 0x7fffffff || grid > 0x7fffffff) return FA_ERR_BAD_SHAPE;
    kp.num_m_blocks = (int32_t)nm;
    kp.num_tiles = (int32_t)tiles;
    kp.unit_tiles = (int32_t)per_kvh;
    kp.whole_slots = (int32_t)whole_slots;
    kp.grid = (int32_t)grid;

    if (sink) {
        kp.sink = sink->learnable_sink;
        kp.sink_hs = sink->sink_head_stride; kp.sink_rs = sink->sink_row_stride;
        kp.sink_fp32 = sink->sink_dtype == FA_DTYPE_FP32;
    }
    const bool softcap = p->softcap > 0.f;

    auto list = [](const int32_t *cnt, const int32_t *idx, const int64_t *cs, const int64_t *is) {
        return fa::BsList{cnt, idx, cs[0], cs[1], cs[2], is[0], is[1], is[2], is[3]};
    };
    bp.full = list(s->full_block_cnt, s->full_block_idx, s->full_cnt_stride, s->full_idx_stride);
    bp.mask = list(s->mask_block_cnt, s->mask_block_idx, s->mask_cnt_stride, s->mask_idx_stride);
    bp.nk = (int32_t)(((int64_t)p->seqlen_k + fa::BS_BLOCK - 1) / fa::BS_BLOCK);

    const int tile = head_dim_tile(std::max(p->d, dv_of(p)));
    t_last_bs_tile = tile;
    t_last_bs_softcap = softcap;
    return p->dtype == FA_DTYPE_BF16 ? launch_bs<__bf16>(tile, softcap, bp, stream) : launch_bs<_Float16>(tile, softcap, bp, stream);
}

}  // extern "C"
