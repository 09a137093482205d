// fa_sample.hip — fa_sample (include/fa_sample.h): top-k / top-p filtering and the draw of a token from a row of logits in one
// launch.  A translation unit of its own: no kernel comes from another unit or goes to one.  The chunk loads and stores, the
// workgroup scan and the counter hash are the inline functions of fa_rowwise.h, shared with the other row units.
//
// One workgroup per row (256 threads up to 1024 accesses per row, else 1024), and no sort.  The row is walked several times; after
// the first walk it comes out of L2.  Thread t owns the accesses k * threads + t: neighbouring lanes read neighbouring 16 bytes.
// Every candidate set of include/fa_sample.h is a pair (K, J): the entries whose key is above K, and of those with key K the ones
// with index below J.  The key is the order-preserving 32-bit image of s (sign-flip), cut down to its significant bits.  A
// phase turns a target into such a pair by *radix descent*: the smallest coordinate x with
//     sum of w over the set's entries of coordinate <= x   >   T
// found 11 bits at a time, each pass a walk that adds w into a histogram of 2048 bins in LDS, a scan over the bins, and the bin
// that holds T.  All w are 64-bit integers (a count, or e * 2^F), so the LDS atomics commute: the same bits every time.
//   top-k         coordinate ~key, w = 1, T = k - 1: the key of the k-th largest entry, the count above it and the count of its ties
//   ties by index coordinate index over the tied entries, w = 1, T = (ties to keep) - 1: the index bound J
//   top-p         coordinate key, w = e * 2^F, T = floor((1 - top_p) Z): the first key that stays; of its ties (all of one
//                 weight) floor((T - below) / w) leave, those of the highest indices: ties by index again
//   draw          coordinate index over the kept set, w = e * 2^F, T = floor(u Z_kept): the token
// Kernels: sample_greedy_kernel<CW> (top_k == 1: one walk, a 64-bit maximum of key and inverted index) and
// sample_kernel<CW, MODE> for FA_SAMPLE_DRAW / FA_SAMPLE_FILTER, CW = 8 / 4 (16-byte accesses) or 1 (elements).
#include "../../include/fa_sample.h"
#include "fa_rowwise.h"

#include <cmath>

namespace {

using namespace fa_row;

constexpr int MAX_THREADS = 1024, SMALL_THREADS = 256;
constexpr int SMALL_ACCESSES = 1024;  // a row of up to this many accesses has the small workgroup
constexpr int RADIX = 11, BINS = 1 << RADIX;
constexpr int MAX_GRID = 65535;  // workgroups; further rows are walked by the same workgroups
constexpr int MAX_FRAC = 40;
constexpr float LOG2E = 1.44269504088896340736f;

struct Shared {
    uint64_t hist[BINS];
    uint64_t part[MAX_WAVES];
    uint64_t below, at;  // of the bin a pass chose
    uint64_t best;       // a 64-bit maximum
    uint32_t digit;
};

// what the walks of one row share
struct Row {
    char *base;
    int dt, V, key_shift;
    float temperature, m, scale;  // m: the maximum of s; scale: 2^F
    bool unit_temperature;
    __device__ __forceinline__ float s(float x) const { return (unit_temperature ? x : x / temperature) + 0.0f; }
    __device__ __forceinline__ uint64_t weight(float sv) const {
        return (uint64_t)(__builtin_amdgcn_exp2f((sv - m) * LOG2E) * scale);
    }
};

__device__ __forceinline__ uint32_t full_key(float s) {
    const uint32_t b = __float_as_uint(s);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t key) {
    return __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu));
}
// the s of a key that was cut by `shift` bits: those bits are zeros of a positive s and ones (inverted zeros) of a negative one
__device__ __forceinline__ float value_of_cut(uint32_t key, int shift) {
    uint32_t full = key << shift;
    if (!(full >> 31)) full |= (1u << shift) - 1u;
    return value_of(full);
}

struct Set {
    uint32_t K;
    int J;
    __device__ __forceinline__ bool has(uint32_t key, int i) const { return key > K || (key == K && i < J); }
};

// f(first column, CW values) over the accesses of this thread
template <int CW, class F>
__device__ __forceinline__ void walk(const Row &r, F &&f) {
    const uint32_t n = (uint32_t)r.V / CW;  // (the plan gives CW > 1 only to a V that is a multiple of it)
    const int cb = CW * esize(r.dt);
    for (uint32_t c = threadIdx.x; c < n; c += blockDim.x) {  // (c + blockDim.x < 2^32: n < 2^31)
        float v[CW];
        load_chunk<CW>(r.base + (int64_t)c * cb, r.dt, v);
        f((int)(c * CW), v);
    }
}

struct Found {
    uint32_t x;
    uint64_t below, at;  // the sums of w over the coordinates below x and at x
};

// The radix descent over the `bits` low bits of a coordinate.  elem(i, x, coordinate &, w &) -> whether the entry takes part.
// T is below the sum of all w; where it is not (a row that changed between walks, a NaN), the descent ends at some coordinate
// of `bits` bits and nothing is out of bounds.  Every thread calls it together and gets the same Found
template <int CW, class E>
__device__ __forceinline__ Found descend(Shared &sh, const Row &r, int bits, uint64_t T, E &&elem) {
    Found f = {0u, 0u, 0u};
    for (int top = bits; top > 0; top -= RADIX) {
        const int low = top > RADIX ? top - RADIX : 0;
        const uint32_t mask = (1u << (top - low)) - 1u;
        for (int b = threadIdx.x; b < BINS; b += blockDim.x) sh.hist[b] = 0;
        __syncthreads();
        const uint32_t prefix = top < 32 ? f.x >> top : 0u;
        walk<CW>(r, [&](int i0, const float (&v)[CW]) {
            uint32_t d_run = 0;  // a run of entries of one bin is one atomic
            uint64_t w_run = 0;
#pragma unroll
            for (int i = 0; i < CW; ++i) {
                uint32_t c;
                uint64_t w;
                if (!elem(i0 + i, v[i], c, w)) continue;
                if (top < bits && (c >> top) != prefix) continue;
                const uint32_t d = (c >> low) & mask;
                if (d != d_run && w_run) {
                    atomicAdd(reinterpret_cast<unsigned long long *>(&sh.hist[d_run]), (unsigned long long)w_run);
                    w_run = 0;
                }
                d_run = d;
                w_run += w;
            }
            if (w_run) atomicAdd(reinterpret_cast<unsigned long long *>(&sh.hist[d_run]), (unsigned long long)w_run);
        });
        __syncthreads();
        const int per = BINS / blockDim.x, b0 = threadIdx.x * per;
        uint64_t mine = 0, total;
        for (int j = 0; j < per; ++j) mine += sh.hist[b0 + j];
        const uint64_t before = wg_exclusive_scan(mine, sh.part, total), rest = T - f.below;
        if (rest >= total) {  // (not reached by a consistent row)
            if (threadIdx.x == 0) { sh.digit = 0; sh.below = 0; sh.at = 0; }
        } else if (before <= rest && rest < before + mine) {
            uint64_t acc = before;
            for (int j = 0; j < per; ++j) {
                const uint64_t h = sh.hist[b0 + j];
                if (rest < acc + h) {
                    sh.digit = (uint32_t)(b0 + j); sh.below = acc; sh.at = h;
                    break;
                }
                acc += h;
            }
        }
        __syncthreads();
        f.x |= sh.digit << low;
        f.below += sh.below;
        f.at = sh.at;
    }
    return f;
}

__device__ __forceinline__ uint64_t shfl_xor_64(uint64_t v, int o) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, WAVE), hi = __shfl_xor((uint32_t)(v >> 32), o, WAVE);
    return (uint64_t)hi << 32 | lo;
}

// the maximum of v over the workgroup, to every thread
__device__ __forceinline__ uint64_t wg_max(Shared &sh, uint64_t v) {
    if (threadIdx.x == 0) sh.best = 0;
    __syncthreads();
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        const uint64_t other = shfl_xor_64(v, o);
        v = other > v ? other : v;
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) atomicMax(reinterpret_cast<unsigned long long *>(&sh.best), (unsigned long long)v);
    __syncthreads();
    const uint64_t best = sh.best;
    __syncthreads();
    return best;
}

__device__ __forceinline__ Row row_of_call(const fa_sample_params &p, const fa_sample_form &f, int64_t r) {
    Row row;
    row.base = row_of(p.logits, p.logits_dtype, r, p.logits_row_stride);
    row.dt = p.logits_dtype;
    row.V = p.V;
    row.key_shift = 32 - f.key_bits;
    row.temperature = p.temperature;
    row.unit_temperature = p.temperature == 1.0f;
    row.m = 0.0f;
    row.scale = __uint_as_float((uint32_t)(127 + f.frac_bits) << 23);
    return row;
}

// ---- top_k == 1 ---------------------------------------------------------------------------------------------------------------
template <int CW>
__global__ __launch_bounds__(MAX_THREADS) void sample_greedy_kernel(const fa_sample_params p, const fa_sample_form f) {
    __shared__ Shared sh;
    for (int64_t r = blockIdx.x; r < p.B; r += gridDim.x) {
        const Row row = row_of_call(p, f, r);
        uint64_t best = 0;  // (key, ~index): the largest key, and of equal keys the lowest index
        walk<CW>(row, [&](int i0, const float (&v)[CW]) {
#pragma unroll
            for (int i = 0; i < CW; ++i) {
                const uint64_t e = (uint64_t)full_key(row.s(v[i])) << 32 | (uint32_t)~(uint32_t)(i0 + i);
                best = e > best ? e : best;
            }
        });
        best = wg_max(sh, best);
        if (threadIdx.x == 0) p.token[r] = (int64_t)(uint32_t)~(uint32_t)best;  // (nothing but -inf: index 0)
    }
}

// ---- top-k, top-p, and the draw or the filter --------------------------------------------------------------------------------
template <int CW, int MODE>
__global__ __launch_bounds__(MAX_THREADS) void sample_kernel(const fa_sample_params p, const fa_sample_form f) {
    __shared__ Shared sh;
    const int V = p.V;
    const uint32_t mix = (MODE == FA_SAMPLE_DRAW && p.rng_state) ? seed_mix(p.rng_state) : 0u;
    const uint32_t key_mask = f.key_bits == 32 ? 0xffffffffu : (1u << f.key_bits) - 1u;
    for (int64_t r = blockIdx.x; r < p.B; r += gridDim.x) {
        Row row = row_of_call(p, f, r);
        const int shift = row.key_shift;
        uint64_t top = 0;
        walk<CW>(row, [&](int, const float (&v)[CW]) {
#pragma unroll
            for (int i = 0; i < CW; ++i) {
                const uint64_t e = full_key(row.s(v[i]));
                top = e > top ? e : top;
            }
        });
        row.m = value_of((uint32_t)wg_max(sh, top));
        if (row.m == -INFINITY) {  // nothing but -inf (uniform over the workgroup)
            if (threadIdx.x == 0) {
                if (MODE == FA_SAMPLE_DRAW) p.token[r] = 0;
                if (p.kept) p.kept[r] = 0;
                if (p.mass) p.mass[r] = 0.0f;
            }
            continue;
        }

        Set set = {0u, V};  // everything
        if (f.topk) {
            const Found t = descend<CW>(sh, row, f.key_bits, (uint64_t)(f.k - 1), [&](int, float x, uint32_t &c, uint64_t &w) {
                c = ~(full_key(row.s(x)) >> shift) & key_mask;
                w = 1;
                return true;
            });
            set.K = ~t.x & key_mask;
            const uint64_t ties_in = (uint64_t)f.k - t.below;  // of the t.at entries with the k-th key
            if (MODE == FA_SAMPLE_DRAW && ties_in < t.at) {    // (the filter keeps them all)
                const uint32_t K = set.K;
                const Found n = descend<CW>(sh, row, f.index_bits, ties_in - 1, [&](int i, float x, uint32_t &c, uint64_t &w) {
                    c = (uint32_t)i;
                    w = 1;
                    return full_key(row.s(x)) >> shift == K;
                });
                set.J = (int)n.x + 1;
            }
        }

        uint64_t mine = 0, Z;
        {
            const Set in = set;
            walk<CW>(row, [&](int i0, const float (&v)[CW]) {
#pragma unroll
                for (int i = 0; i < CW; ++i) {
                    const float sv = row.s(v[i]);
                    if (in.has(full_key(sv) >> shift, i0 + i)) mine += row.weight(sv);
                }
            });
        }
        wg_exclusive_scan(mine, sh.part, Z);
        uint64_t Zk = Z;

        if (f.topp) {
            const Set in = set;
            uint64_t T = (uint64_t)((double)(1.0f - p.top_p) * (double)Z);
            T = T < Z ? T : Z - 1;  // (1 - top_p rounds to 1: all but the largest entry leave)
            const Found t = descend<CW>(sh, row, f.key_bits, T, [&](int i, float x, uint32_t &c, uint64_t &w) {
                const float sv = row.s(x);
                c = full_key(sv) >> shift;
                w = row.weight(sv);
                return in.has(c, i);
            });
            const uint64_t w_tie = row.weight(value_of_cut(t.x, shift));
            const uint64_t ties = w_tie ? t.at / w_tie : 0, leave = w_tie ? (T - t.below) / w_tie : 0;  // leave < ties
            Zk = Z - t.below - leave * w_tie;
            set.J = t.x == in.K ? in.J : V;
            set.K = t.x;
            if (leave > 0 && leave < ties) {
                const uint32_t K = t.x;
                const Found n = descend<CW>(sh, row, f.index_bits, ties - leave - 1, [&](int i, float x, uint32_t &c, uint64_t &w) {
                    c = (uint32_t)i;
                    w = 1;
                    return full_key(row.s(x)) >> shift == K && in.has(K, i);
                });
                set.J = (int)n.x + 1;
            }
        }

        const Set kept = set;
        if (p.kept) {
            uint64_t count = 0, all;
            walk<CW>(row, [&](int i0, const float (&v)[CW]) {
#pragma unroll
                for (int i = 0; i < CW; ++i) count += kept.has(full_key(row.s(v[i])) >> shift, i0 + i) ? 1 : 0;
            });
            wg_exclusive_scan(count, sh.part, all);
            if (threadIdx.x == 0) p.kept[r] = (int32_t)all;
        }
        if (p.mass && threadIdx.x == 0) p.mass[r] = (float)((double)Zk / (double)Z);

        if (MODE == FA_SAMPLE_DRAW) {
            float u;
            if (p.u) {
                u = p.u[r];
            } else {
                const uint32_t lo = (uint32_t)r, hi = (uint32_t)((uint64_t)r >> 32);
                u = (float)(lowbias32((mix ^ hi * 0x2545F491u) ^ lo * 0x9E3779B1u) >> 8) * 0x1p-24f;
            }
            uint64_t T = (uint64_t)((double)fmaxf(u, 0.0f) * (double)Zk);
            T = T < Zk ? T : Zk - 1;  // (Zk >= 1: the largest entry weighs 2^F.  Only a u >= 1 gets here)
            const Found d = descend<CW>(sh, row, f.index_bits, T, [&](int i, float x, uint32_t &c, uint64_t &w) {
                const float sv = row.s(x);
                c = (uint32_t)i;
                w = row.weight(sv);
                return kept.has(full_key(sv) >> shift, i);
            });
            if (threadIdx.x == 0) p.token[r] = d.x < (uint32_t)V ? (int64_t)d.x : (int64_t)V - 1;
        } else {
            walk<CW>(row, [&](int i0, const float (&v)[CW]) {
                float y[CW];
#pragma unroll
                for (int i = 0; i < CW; ++i) y[i] = kept.has(full_key(row.s(v[i])) >> shift, i0 + i) ? v[i] : -INFINITY;
                store_chunk<CW>(row.base + (int64_t)i0 * esize(row.dt), row.dt, y);
            });
            __syncthreads();  // (the next row of this workgroup is another row: nothing of this one is read again)
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
int ceil_log2(int64_t n) {  // n >= 1
    int b = 0;
    while (((int64_t)1 << b) < n) ++b;
    return b;
}

// the form of a valid call
fa_sample_form form_of(const fa_sample_params *p) {
    fa_sample_form l{};
    const int es = esize(p->logits_dtype);
    const bool wide = aligned_to(p->logits, 16) && ((int64_t)p->V * es) % 16 == 0 && (p->B <= 1 || (p->logits_row_stride * es) % 16 == 0);
    l.cw = wide ? 16 / es : 1;
    l.threads = p->V / l.cw <= SMALL_ACCESSES ? SMALL_THREADS : MAX_THREADS;
    l.mode = p->mode;
    l.greedy = p->mode == FA_SAMPLE_DRAW && p->top_k == 1;
    const int first = p->mode == FA_SAMPLE_DRAW ? 2 : 1;  // the lowest top_k that selects
    l.topk = !l.greedy && p->top_k >= first && p->top_k < p->V;  // (from V on nothing is below the k-th value)
    l.k = l.topk ? p->top_k : 0;
    l.topp = !l.greedy && p->top_p > 0.0f && p->top_p < 1.0f;
    l.draw = !l.greedy && p->mode == FA_SAMPLE_DRAW;
    l.key_bits = p->temperature != 1.0f ? 32 : p->logits_dtype == FA_DTYPE_BF16 ? 16 : p->logits_dtype == FA_DTYPE_FP16 ? 19 : 32;
    l.key_passes = (l.key_bits + RADIX - 1) / RADIX;
    l.index_bits = ceil_log2(p->V) > 0 ? ceil_log2(p->V) : 1;
    l.index_passes = (l.index_bits + RADIX - 1) / RADIX;
    const int room = 62 - ceil_log2(p->V);
    l.frac_bits = room < MAX_FRAC ? room : MAX_FRAC;
    l.grid_x = (int32_t)(p->B < MAX_GRID ? p->B : MAX_GRID);
    return l;
}

template <int CW>
void launch(const fa_sample_params *p, const fa_sample_form &l, hipStream_t stream) {
    const dim3 grid(l.grid_x), block(l.threads);
    if (l.greedy) hipLaunchKernelGGL((sample_greedy_kernel<CW>), grid, block, 0, stream, *p, l);
    else if (l.mode == FA_SAMPLE_DRAW) hipLaunchKernelGGL((sample_kernel<CW, FA_SAMPLE_DRAW>), grid, block, 0, stream, *p, l);
    else hipLaunchKernelGGL((sample_kernel<CW, FA_SAMPLE_FILTER>), grid, block, 0, stream, *p, l);
}

}  // namespace

extern "C" {

uint32_t fa_sample_params_size(void) { return (uint32_t)sizeof(fa_sample_params); }

int fa_sample_validate(const fa_sample_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_sample_params)) return FA_ERR_BAD_ABI;
    if (!known_dtype(p->logits_dtype)) return FA_ERR_BAD_DTYPE;
    if (p->mode != FA_SAMPLE_DRAW && p->mode != FA_SAMPLE_FILTER) return FA_ERR_BAD_SHAPE;
    if (p->B < 0 || p->V < 1 || p->top_k < 0) return FA_ERR_BAD_SHAPE;  // (V < 2^31 by its type)
    if (!(p->temperature > 0.0f) || !(p->top_p >= 0.0f && p->top_p <= 1.0f)) return FA_ERR_BAD_SHAPE;  // (NaN fails both)
    const bool draw = p->mode == FA_SAMPLE_DRAW, greedy = draw && p->top_k == 1;
    if (!p->logits || (draw && !p->token)) return FA_ERR_NULL_POINTER;
    if (greedy && (p->kept || p->mass)) return FA_ERR_BAD_SHAPE;
    if (draw && !greedy) {
        if (!p->u && !p->rng_state) return FA_ERR_NULL_POINTER;
        if (p->u && p->rng_state) return FA_ERR_BAD_SHAPE;
    }
    if (!aligned_to(p->logits, esize(p->logits_dtype)) || !aligned_to(p->u, 4) || !aligned_to(p->rng_state, 8) ||
        !aligned_to(p->token, 8) || !aligned_to(p->kept, 4) || !aligned_to(p->mass, 4))
        return FA_ERR_BAD_STRIDE;
    if (!draw && p->B > 1 && p->logits_row_stride < p->V) return FA_ERR_BAD_STRIDE;  // (rows that are written do not overlap)
    return FA_OK;
}

int fa_sample_plan(const fa_sample_params *p, fa_sample_form *plan) {
    const int st = fa_sample_validate(p);
    if (st != FA_OK) return st;
    if (!plan) return FA_ERR_NULL_POINTER;
    *plan = form_of(p);
    return FA_OK;
}

int fa_sample(const fa_sample_params *p, void *stream_) {
    const int st = fa_sample_validate(p);
    if (st != FA_OK) return st;
    if (p->B == 0) return FA_OK;  // (no zero grid)
    const fa_sample_form l = form_of(p);
    if (p->mode == FA_SAMPLE_FILTER && !l.topk && !l.topp && !p->kept && !p->mass) return FA_OK;  // nothing leaves, nothing is asked
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (l.cw == 8) launch<8>(p, l, stream);
    else if (l.cw == 4) launch<4>(p, l, stream);
    else launch<1>(p, l, stream);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

}  // extern "C"
