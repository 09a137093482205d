// fa_sample.hip — fa_sample (include/fa_sample.h): top-k / top-p filtering and the draw of a token from a row of logits in one
// launch.  A translation unit of its own: no kernel comes from another unit or goes to one.  The chunk loads and stores, the
// workgroup scan and the counter hash are the inline functions of fa_rowwise.h, shared with the other row units; the walks, the
// descent and the selection of a candidate set are those of fa_sample_device.h, shared with fa_spec_sample.hip.
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
#include "fa_sample_device.h"

namespace {

using namespace fa_sample_dev;

__device__ __forceinline__ Row row_of_call(const fa_sample_params &p, const fa_sample_form &f, int64_t r) {
    return make_row(row_of(p.logits, p.logits_dtype, r, p.logits_row_stride), p.logits_dtype, p.V, p.temperature, f.key_bits, f.frac_bits);
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
    const uint32_t mix = (MODE == FA_SAMPLE_DRAW && p.rng_state) ? seed_mix(p.rng_state) : 0u;
    const Selection how = {f.topk, f.topp, f.k, f.key_bits, f.index_bits, p.top_p};
    for (int64_t r = blockIdx.x; r < p.B; r += gridDim.x) {
        Row row = row_of_call(p, f, r);
        const int shift = row.key_shift;
        row.m = row_max<CW>(sh, row);
        if (row.m == -INFINITY) {  // nothing but -inf (uniform over the workgroup)
            if (threadIdx.x == 0) {
                if (MODE == FA_SAMPLE_DRAW) p.token[r] = 0;
                if (p.kept) p.kept[r] = 0;
                if (p.mass) p.mass[r] = 0.0f;
            }
            continue;
        }

        const Kept sel = select_set<CW, MODE == FA_SAMPLE_DRAW>(sh, row, how);
        const Set kept = sel.set;
        if (p.kept) {
            uint64_t count = 0, all;
            walk<CW>(row, [&](int i0, const float (&v)[CW]) {
#pragma unroll
                for (int i = 0; i < CW; ++i) count += kept.has(full_key(row.s(v[i])) >> shift, i0 + i) ? 1 : 0;
            });
            wg_exclusive_scan(count, sh.part, all);
            if (threadIdx.x == 0) p.kept[r] = (int32_t)all;
        }
        if (p.mass && threadIdx.x == 0) p.mass[r] = (float)((double)sel.Zk / (double)sel.Z);

        if (MODE == FA_SAMPLE_DRAW) {
            const float u = p.u ? p.u[r] : uniform_of(mix, r);
            const int token = draw_index<CW>(sh, row, kept, sel.Zk, u, f.index_bits);
            if (threadIdx.x == 0) p.token[r] = (int64_t)token;
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
// the form of a valid call
fa_sample_form form_of(const fa_sample_params *p) {
    fa_sample_form l{};
    const int es = esize(p->logits_dtype);
    const bool wide = aligned_to(p->logits, 16) && ((int64_t)p->V * es) % 16 == 0 && (p->B <= 1 || (p->logits_row_stride * es) % 16 == 0);
    l.cw = wide ? 16 / es : 1;
    l.threads = threads_of(p->V, l.cw);
    l.mode = p->mode;
    l.greedy = p->mode == FA_SAMPLE_DRAW && p->top_k == 1;
    const int first = p->mode == FA_SAMPLE_DRAW ? 2 : 1;  // the lowest top_k that selects
    l.topk = !l.greedy && p->top_k >= first && p->top_k < p->V;  // (from V on nothing is below the k-th value)
    l.k = l.topk ? p->top_k : 0;
    l.topp = !l.greedy && p->top_p > 0.0f && p->top_p < 1.0f;
    l.draw = !l.greedy && p->mode == FA_SAMPLE_DRAW;
    l.key_bits = key_bits_of(p->logits_dtype, p->temperature);
    l.key_passes = passes_of(l.key_bits);
    l.index_bits = index_bits_of(p->V);
    l.index_passes = passes_of(l.index_bits);
    l.frac_bits = frac_bits_of(p->V);
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
