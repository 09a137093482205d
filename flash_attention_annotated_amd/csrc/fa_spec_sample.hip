// fa_spec_sample.hip — fa_spec_sample (include/fa_spec_sample.h): the verification step of speculative sampling in two launches.
// A translation unit of its own; the walks, the keys, the candidate set (K, J), the radix descent and the selection by top-k
// and top-p, the Record of a row and the probability of an entry are the inline functions of fa_sample_device.h, shared with
// fa_sample.hip, whose head says how a descent works, and with fa_tree_sample.hip.
//
// Phase A, spec_select_kernel<CW>: one workgroup per position (b, t), t <= S.  It selects the kept set of the target row and,
// where t < S, of the draft row, exactly as the filter of fa_sample.hip does (all ties of the k-th value stay), writes a Record
// per row, and one thread forms P(x), Q(x) of the draft token x from the two entries it needs and the acceptance of (b, t).
// Phase B, spec_resample_kernel<CW>: one workgroup per sequence.  n_b is the first flag that is 0.  The rows at n_b are walked
// together with their records, nothing is selected again: one walk sums the residual weights, a descent over the index bits
// finds the token.  The launch boundary is what orders the phases: there is no ticket and no atomic between workgroups.
#include "../../include/fa_spec_sample.h"
#include "fa_sample_device.h"

namespace {

using namespace fa_sample_dev;

static_assert(sizeof(Record) == FA_SPEC_RECORD_BYTES, "the record layout of include/fa_spec_sample.h");

__device__ __forceinline__ Row target_row(const fa_spec_sample_params &p, const fa_spec_sample_form &f, int64_t b, int t) {
    const int64_t at = b * p.logits_batch_stride + (int64_t)t * p.logits_pos_stride;
    return make_row(const_cast<char *>(row_of(p.logits, p.logits_dtype, at, 1)), p.logits_dtype, p.V, p.temperature, f.key_bits, f.frac_bits);
}
__device__ __forceinline__ Row draft_row(const fa_spec_sample_params &p, const fa_spec_sample_form &f, int64_t b, int t) {
    const int64_t at = b * p.draft_batch_stride + (int64_t)t * p.draft_pos_stride;
    return make_row(const_cast<char *>(row_of(p.logits_draft, p.logits_dtype, at, 1)), p.logits_dtype, p.V, p.temperature, f.key_bits, f.frac_bits);
}

__device__ __forceinline__ int64_t draft_token(const fa_spec_sample_params &p, int64_t b, int t) {
    const int64_t at = b * p.tokens_draft_batch_stride + t;
    return p.tokens_dtype == FA_SPEC_TOKENS_INT64 ? static_cast<const int64_t *>(p.tokens_draft)[at]
                                                  : (int64_t) static_cast<const int32_t *>(p.tokens_draft)[at];
}

// ---- phase A: the kept sets and the acceptance of every position -------------------------------------------------------------
template <int CW>
__global__ __launch_bounds__(MAX_THREADS) void spec_select_kernel(const fa_spec_sample_params p, const fa_spec_sample_form f) {
    __shared__ Shared sh;
    const int S = p.S;
    const int64_t rows = p.B * (S + 1);
    Record *rec_p = static_cast<Record *>(p.workspace), *rec_q = rec_p + rows;
    const uint32_t mix = p.rng_state ? seed_mix(p.rng_state) : 0u;
    const Selection how = {f.topk, f.topp, f.k, f.key_bits, f.index_bits, p.top_p};
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const int64_t b = r / (S + 1);
        const int t = (int)(r - b * (S + 1));
        Row rp = target_row(p, f, b, t);
        Record a = select_row<CW>(sh, rp, how);
        if (t < S) {
            Row rq = draft_row(p, f, b, t);
            const Record d = select_row<CW>(sh, rq, how);
            if (threadIdx.x == 0) {
                const int64_t x = draft_token(p, b, t), at = b * S + t;
                float P = 0.0f, Q = 0.0f;
                if (x >= 0 && x < p.V) {  // (else rejected, and nothing is read)
                    P = prob_of(rp, a, load_one(rp.base, rp.dt, x), (int)x);
                    Q = prob_of(rq, d, load_one(rq.base, rq.dt, x), (int)x);
                    const float u = p.u_acc ? p.u_acc[at] : uniform_of(mix, at);
                    a.flags = (double)u * (double)Q <= (double)P ? 1 : 0;
                }
                rec_q[at] = d;
                if (p.p_tok) p.p_tok[at] = P;
                if (p.q_tok) p.q_tok[at] = Q;
                if (p.accepted) p.accepted[at] = a.flags;
            }
        }
        if (threadIdx.x == 0) rec_p[r] = a;
    }
}

// ---- phase B: the first rejection and the token drawn there ------------------------------------------------------------------
template <int CW>
__global__ __launch_bounds__(MAX_THREADS) void spec_resample_kernel(const fa_spec_sample_params p, const fa_spec_sample_form f) {
    __shared__ Shared sh;
    const int S = p.S;
    const Record *rec_p = static_cast<const Record *>(p.workspace), *rec_q = rec_p + p.B * (S + 1);
    const uint32_t mix = p.rng_state ? seed_mix(p.rng_state) : 0u;
    for (int64_t b = blockIdx.x; b < p.B; b += gridDim.x) {
        int n = S;  // (the same loads in every thread)
        for (int t = S - 1; t >= 0; --t) n = rec_p[b * (S + 1) + t].flags ? n : t;
        const Record a = rec_p[b * (S + 1) + n];
        Row rp = target_row(p, f, b, n);
        rp.m = a.m;
        const float u = p.u_res ? p.u_res[b] : uniform_of(mix, p.B * S + b);
        int token = 0;  // (of a target row that keeps nothing)
        if (a.Zk > 0) {
            bool drawn = false;
            if (n < S) {
                const Record d = rec_q[b * S + n];
                Row rq = draft_row(p, f, b, n);
                rq.m = d.m;
                const Row2 both = {rp, rq};
                const auto residual = [&](int i, const Pair &x) -> uint64_t {
                    const float diff = prob_of(rp, a, x.p, i) - prob_of(rq, d, x.q, i);
                    return diff > 0.0f ? (uint64_t)(diff * rp.scale) : 0u;
                };
                uint64_t mine = 0, R;
                walk<CW>(both, [&](int i0, const Pair (&v)[CW]) {
#pragma unroll
                    for (int i = 0; i < CW; ++i) mine += residual(i0 + i, v[i]);
                });
                wg_exclusive_scan(mine, sh.part, R);
                if (R > 0) {
                    uint64_t T = (uint64_t)((double)fmaxf(u, 0.0f) * (double)R);
                    T = T < R ? T : R - 1;  // (only a u >= 1 gets here: the last index of positive weight)
                    const Found at = descend<CW>(sh, both, f.index_bits, T, [&](int i, const Pair &x, uint32_t &c, uint64_t &w) {
                        c = (uint32_t)i;
                        w = residual(i, x);
                        return w > 0;
                    });
                    token = at.x < (uint32_t)p.V ? (int)at.x : p.V - 1;
                    drawn = true;
                }
            }
            if (!drawn) token = draw_index<CW>(sh, rp, {a.K, a.J}, a.Zk, u, f.index_bits);
        }
        for (int t = threadIdx.x; t <= S; t += blockDim.x) {
            const int64_t x = t == n ? (int64_t)token : t < S ? draft_token(p, b, t) : 0;
            if (p.tokens_dtype == FA_SPEC_TOKENS_INT64) static_cast<int64_t *>(p.tokens)[b * (S + 1) + t] = x;
            else static_cast<int32_t *>(p.tokens)[b * (S + 1) + t] = (int32_t)x;
        }
        if (threadIdx.x == 0) p.num_generated[b] = n + 1;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// the form of a valid call
fa_spec_sample_form form_of(const fa_spec_sample_params *p) {
    fa_spec_sample_form l{};
    const int es = esize(p->logits_dtype);
    const auto pitch_ok = [&](int64_t stride, bool used) { return !used || (stride * es) % 16 == 0; };
    bool wide = aligned_to(p->logits, 16) && ((int64_t)p->V * es) % 16 == 0 && pitch_ok(p->logits_batch_stride, p->B > 1) &&
                pitch_ok(p->logits_pos_stride, p->S >= 1);
    if (p->S >= 1)
        wide = wide && aligned_to(p->logits_draft, 16) && pitch_ok(p->draft_batch_stride, p->B > 1) && pitch_ok(p->draft_pos_stride, p->S > 1);
    l.cw = wide ? 16 / es : 1;
    l.threads = threads_of(p->V, l.cw);
    l.topk = p->top_k >= 1 && p->top_k < p->V;  // (from V on nothing is below the k-th value)
    l.k = l.topk ? p->top_k : 0;
    l.topp = p->top_p > 0.0f && p->top_p < 1.0f;
    l.key_bits = key_bits_of(p->logits_dtype, p->temperature);
    l.key_passes = passes_of(l.key_bits);
    l.index_bits = index_bits_of(p->V);
    l.index_passes = passes_of(l.index_bits);
    l.frac_bits = frac_bits_of(p->V);
    const int64_t rows = p->B * (p->S + 1);
    l.grid_a = (int32_t)(rows < MAX_GRID ? rows : MAX_GRID);
    l.grid_b = (int32_t)(p->B < MAX_GRID ? p->B : MAX_GRID);
    return l;
}

template <int CW>
void launch(const fa_spec_sample_params *p, const fa_spec_sample_form &l, hipStream_t stream) {
    const dim3 block(l.threads);
    hipLaunchKernelGGL((spec_select_kernel<CW>), dim3(l.grid_a), block, 0, stream, *p, l);
    hipLaunchKernelGGL((spec_resample_kernel<CW>), dim3(l.grid_b), block, 0, stream, *p, l);
}

}  // namespace

extern "C" {

uint32_t fa_spec_sample_params_size(void) { return (uint32_t)sizeof(fa_spec_sample_params); }

int64_t fa_spec_sample_workspace_size(int64_t B, int32_t S) {
    if (B < 0 || S < 0) return 0;
    return B * (2 * (int64_t)S + 1) * FA_SPEC_RECORD_BYTES;
}

int fa_spec_sample_validate(const fa_spec_sample_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_spec_sample_params)) return FA_ERR_BAD_ABI;
    if (!known_dtype(p->logits_dtype)) return FA_ERR_BAD_DTYPE;
    if (p->tokens_dtype != FA_SPEC_TOKENS_INT32 && p->tokens_dtype != FA_SPEC_TOKENS_INT64) return FA_ERR_BAD_DTYPE;
    if (p->B < 0 || p->S < 0 || p->V < 1 || p->top_k < 0) return FA_ERR_BAD_SHAPE;  // (V < 2^31 by its type)
    if (p->B > ((int64_t)1 << 31) - 1 || p->B * (2 * (int64_t)p->S + 1) > ((int64_t)1 << 31) - 1) return FA_ERR_BAD_SHAPE;
    if (!(p->temperature > 0.0f) || !(p->top_p >= 0.0f && p->top_p <= 1.0f)) return FA_ERR_BAD_SHAPE;  // (NaN fails both)
    const bool drafts = p->S > 0;
    if (!p->logits || !p->tokens || !p->num_generated || (drafts && (!p->logits_draft || !p->tokens_draft))) return FA_ERR_NULL_POINTER;
    if (!p->u_res && !p->rng_state) return FA_ERR_NULL_POINTER;
    if (p->rng_state && (p->u_res || p->u_acc)) return FA_ERR_BAD_SHAPE;
    if (p->u_res && drafts && !p->u_acc) return FA_ERR_NULL_POINTER;
    const int es = esize(p->logits_dtype), ts = p->tokens_dtype == FA_SPEC_TOKENS_INT64 ? 8 : 4;
    if (!aligned_to(p->logits, es) || !aligned_to(p->logits_draft, es) || !aligned_to(p->tokens_draft, ts) || !aligned_to(p->tokens, ts) ||
        !aligned_to(p->u_acc, 4) || !aligned_to(p->u_res, 4) || !aligned_to(p->rng_state, 8) || !aligned_to(p->num_generated, 8) ||
        !aligned_to(p->p_tok, 4) || !aligned_to(p->q_tok, 4) || !aligned_to(p->accepted, 4) || !aligned_to(p->workspace, 8))
        return FA_ERR_BAD_STRIDE;
    const int64_t need = fa_spec_sample_workspace_size(p->B, p->S);
    if (need > 0 && (!p->workspace || p->workspace_bytes < need)) return FA_ERR_WORKSPACE;
    return FA_OK;
}

int fa_spec_sample_plan(const fa_spec_sample_params *p, fa_spec_sample_form *plan) {
    const int st = fa_spec_sample_validate(p);
    if (st != FA_OK) return st;
    if (!plan) return FA_ERR_NULL_POINTER;
    *plan = form_of(p);
    return FA_OK;
}

int fa_spec_sample(const fa_spec_sample_params *p, void *stream_) {
    const int st = fa_spec_sample_validate(p);
    if (st != FA_OK) return st;
    if (p->B == 0) return FA_OK;  // (no zero grid)
    const fa_spec_sample_form l = form_of(p);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (l.cw == 8) launch<8>(p, l, stream);
    else if (l.cw == 4) launch<4>(p, l, stream);
    else launch<1>(p, l, stream);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

}  // extern "C"
