// fa_sample_device.h — what the sampling units (fa_sample.hip: the draw and the filter; fa_spec_sample.hip: the verification of
// a chain of draft tokens; fa_tree_sample.hip: of a tree of them) share: the row walks, the order-preserving key, the candidate set as a pair (K, J), the radix descent over
// histograms in LDS, and the selection of a row's candidate set by top-k and top-p.  Everything here is an inline function:
// including it adds no kernel to a unit and renames none.  The rule these functions implement is written out in
// include/fa_sample.h; how a descent works, at the head of fa_sample.hip.
#pragma once

#include "fa_rowwise.h"

#include <cmath>

namespace fa_sample_dev {

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
    __device__ __forceinline__ float scaled_e(float sv) const { return __builtin_amdgcn_exp2f((sv - m) * LOG2E) * scale; }  // e 2^F
    __device__ __forceinline__ uint64_t weight(float sv) const { return (uint64_t)scaled_e(sv); }
};

// two rows of one width and dtype walked together: the entries of a walk are pairs
struct Pair {
    float p, q;
};
struct Row2 {
    Row p, q;
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
// ... and f(first column, CW pairs) over those of two rows
template <int CW, class F>
__device__ __forceinline__ void walk(const Row2 &r, F &&f) {
    const uint32_t n = (uint32_t)r.p.V / CW;
    const int cb = CW * esize(r.p.dt);
    for (uint32_t c = threadIdx.x; c < n; c += blockDim.x) {
        float a[CW], b[CW];
        load_chunk<CW>(r.p.base + (int64_t)c * cb, r.p.dt, a);
        load_chunk<CW>(r.q.base + (int64_t)c * cb, r.q.dt, b);
        Pair v[CW];
#pragma unroll
        for (int i = 0; i < CW; ++i) v[i] = {a[i], b[i]};
        f((int)(c * CW), v);
    }
}

struct Found {
    uint32_t x;
    uint64_t below, at;  // the sums of w over the coordinates below x and at x
};

// The radix descent over the `bits` low bits of a coordinate.  elem(i, x, coordinate &, w &) -> whether the entry takes part;
// x is the entry of a Row, or the pair of entries of a Row2.
// T is below the sum of all w; where it is not (a row that changed between walks, a NaN), the descent ends at some coordinate
// of `bits` bits and nothing is out of bounds.  Every thread calls it together and gets the same Found
template <int CW, class R, class E>
__device__ __forceinline__ Found descend(Shared &sh, const R &r, int bits, uint64_t T, E &&elem) {
    Found f = {0u, 0u, 0u};
    for (int top = bits; top > 0; top -= RADIX) {
        const int low = top > RADIX ? top - RADIX : 0;
        const uint32_t mask = (1u << (top - low)) - 1u;
        for (int b = threadIdx.x; b < BINS; b += blockDim.x) sh.hist[b] = 0;
        __syncthreads();
        const uint32_t prefix = top < 32 ? f.x >> top : 0u;
        walk<CW>(r, [&](int i0, const auto &v) {
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

// a row of V entries of dtype `dt` at `base`, its keys cut to key_bits, sums with frac_bits fraction bits; m is not yet known
__device__ __forceinline__ Row make_row(void *base, int dt, int V, float temperature, int key_bits, int frac_bits) {
    Row row;
    row.base = static_cast<char *>(base);
    row.dt = dt;
    row.V = V;
    row.key_shift = 32 - key_bits;
    row.temperature = temperature;
    row.unit_temperature = temperature == 1.0f;
    row.m = 0.0f;
    row.scale = __uint_as_float((uint32_t)(127 + frac_bits) << 23);
    return row;
}

// the maximum of s over the row (one walk), to every thread; -inf: a row of nothing but -inf
template <int CW>
__device__ __forceinline__ float row_max(Shared &sh, const Row &row) {
    uint64_t top = 0;
    walk<CW>(row, [&](int, const float (&v)[CW]) {
#pragma unroll
        for (int i = 0; i < CW; ++i) {
            const uint64_t e = full_key(row.s(v[i]));
            top = e > top ? e : top;
        }
    });
    return value_of((uint32_t)wg_max(sh, top));
}

// how a candidate set is selected: top-k to k entries where topk, top-p where topp
struct Selection {
    int topk, topp, k, key_bits, index_bits;
    float top_p;
};
struct Kept {
    Set set;
    uint64_t Z, Zk;  // the sums of the weights over what top-k left, and over the set
};

// The candidate set of a row whose maximum row.m is finite: top-k (EXACT_K: exactly k entries, of equal ones the lower
// indices; else every entry equal to the k-th stays) and then top-p.  Every thread calls it together and gets the same Kept
template <int CW, bool EXACT_K>
__device__ __forceinline__ Kept select_set(Shared &sh, const Row &row, const Selection &q) {
    const int V = row.V, shift = row.key_shift;
    const uint32_t key_mask = q.key_bits == 32 ? 0xffffffffu : (1u << q.key_bits) - 1u;
    Set set = {0u, V};  // everything
    if (q.topk) {
        const Found t = descend<CW>(sh, row, q.key_bits, (uint64_t)(q.k - 1), [&](int, float x, uint32_t &c, uint64_t &w) {
            c = ~(full_key(row.s(x)) >> shift) & key_mask;
            w = 1;
            return true;
        });
        set.K = ~t.x & key_mask;
        const uint64_t ties_in = (uint64_t)q.k - t.below;  // of the t.at entries with the k-th key
        if (EXACT_K && ties_in < t.at) {                   // (the filter keeps them all)
            const uint32_t K = set.K;
            const Found n = descend<CW>(sh, row, q.index_bits, ties_in - 1, [&](int i, float x, uint32_t &c, uint64_t &w) {
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

    if (q.topp) {
        const Set in = set;
        uint64_t T = (uint64_t)((double)(1.0f - q.top_p) * (double)Z);
        T = T < Z ? T : Z - 1;  // (1 - top_p rounds to 1: all but the largest entry leave)
        const Found t = descend<CW>(sh, row, q.key_bits, T, [&](int i, float x, uint32_t &c, uint64_t &w) {
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
            const Found n = descend<CW>(sh, row, q.index_bits, ties - leave - 1, [&](int i, float x, uint32_t &c, uint64_t &w) {
                c = (uint32_t)i;
                w = 1;
                return full_key(row.s(x)) >> shift == K && in.has(K, i);
            });
            set.J = (int)n.x + 1;
        }
    }
    return {set, Z, Zk};
}

// What a selection leaves behind of a row for a later launch (the verification units: a chain, fa_spec_sample.hip, and a tree,
// fa_tree_sample.hip): 24 bytes in the workspace
struct Record {
    float m;  // the maximum of s; -inf: the row keeps nothing
    uint32_t K;
    int32_t J;
    int32_t flags;  // the unit's own
    uint64_t Zk;    // the sum of the weights of the kept set
};

// the record of a row, and its maximum into row.m
template <int CW>
__device__ __forceinline__ Record select_row(Shared &sh, Row &row, const Selection &how) {
    row.m = row_max<CW>(sh, row);
    if (row.m == -INFINITY) return {row.m, 0xffffffffu, 0, 0, 0u};  // (no key is above K and no index below J)
    const Kept sel = select_set<CW, false>(sh, row, how);
    return {row.m, sel.set.K, sel.set.J, 0, sel.Zk};
}

// P of the entry x at column i of a row with the record `rec` (row.m == rec.m)
__device__ __forceinline__ float prob_of(const Row &row, const Record &rec, float x, int i) {
    const float sv = row.s(x);
    const Set kept = {rec.K, rec.J};
    if (rec.Zk == 0 || !kept.has(full_key(sv) >> row.key_shift, i)) return 0.0f;
    return (float)((double)row.scaled_e(sv) / (double)rec.Zk);  // (e, not its truncated weight: the smallest P keeps its digits)
}

// the uniform of row r under the seed mix `mix` (include/fa_sample.h)
__device__ __forceinline__ float uniform_of(uint32_t mix, int64_t r) {
    const uint32_t lo = (uint32_t)r, hi = (uint32_t)((uint64_t)r >> 32);
    return (float)(lowbias32((mix ^ hi * 0x2545F491u) ^ lo * 0x9E3779B1u) >> 8) * 0x1p-24f;
}

// The draw: the first index of `kept` whose inclusive cumulative weight exceeds floor(u * Zk) (Zk >= 1), the last kept index
// where a u >= 1 leaves none
template <int CW>
__device__ __forceinline__ int draw_index(Shared &sh, const Row &row, const Set &kept, uint64_t Zk, float u, int index_bits) {
    const int shift = row.key_shift;
    uint64_t T = (uint64_t)((double)fmaxf(u, 0.0f) * (double)Zk);
    T = T < Zk ? T : Zk - 1;  // (Zk >= 1: the largest entry weighs 2^F.  Only a u >= 1 gets here)
    const Found d = descend<CW>(sh, row, index_bits, T, [&](int i, float x, uint32_t &c, uint64_t &w) {
        const float sv = row.s(x);
        c = (uint32_t)i;
        w = row.weight(sv);
        return kept.has(full_key(sv) >> shift, i);
    });
    return d.x < (uint32_t)row.V ? (int)d.x : row.V - 1;
}

// ---- host -------------------------------------------------------------------------------------------------------------------
inline int ceil_log2(int64_t n) {  // n >= 1
    int b = 0;
    while (((int64_t)1 << b) < n) ++b;
    return b;
}
// the significant bits of the key of s: 16 / 19 of a bf16 / fp16 row at temperature 1, else 32
inline int key_bits_of(int dt, float temperature) {
    return temperature != 1.0f ? 32 : dt == FA_DTYPE_BF16 ? 16 : dt == FA_DTYPE_FP16 ? 19 : 32;
}
inline int index_bits_of(int V) { return ceil_log2(V) > 0 ? ceil_log2(V) : 1; }
inline int frac_bits_of(int V) {
    const int room = 62 - ceil_log2(V);
    return room < MAX_FRAC ? room : MAX_FRAC;
}
inline int passes_of(int bits) { return (bits + RADIX - 1) / RADIX; }
inline int threads_of(int V, int cw) { return V / cw <= SMALL_ACCESSES ? SMALL_THREADS : MAX_THREADS; }

}  // namespace fa_sample_dev
