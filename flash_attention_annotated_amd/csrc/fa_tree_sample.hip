// fa_tree_sample.hip — fa_tree_sample (include/fa_tree_sample.h): the acceptance walk over a tree of draft tokens in two launches.
// A translation unit of its own; the walks, the keys, the candidate set (K, J), the radix descent, the selection by top-k and
// top-p, the Record of a row and the probability of an entry are the inline functions of fa_sample_device.h, shared with
// fa_sample.hip, whose head says how a descent works, and with fa_spec_sample.hip, whose phases these mirror.
//
// Phase A, tree_select_kernel<CW>: one workgroup per row (b, n).  It selects the kept set of the target row and, with draft rows,
// of the draft row of a node that has a child, exactly as the filter of fa_sample.hip does, and writes a Record per row.
// Phase B, tree_walk_kernel<CW>: one workgroup per sequence.  Thread i forms P(x), Q(x) (one-hot: w_x) of node i from the two
// entries it needs and the records of the parent; then every thread walks down from the root over the same LDS words, so all
// take the same branches.  A rejection under draft rows is one walk of the two rows at n for R(c); under the one-hot rule it is
// a subtraction.  A descent over the index bits finds the token.  The launch boundary is what orders the phases: there is no
// ticket and no atomic between workgroups.
#include "../../include/fa_tree_sample.h"
#include "fa_sample_device.h"

namespace {

using namespace fa_sample_dev;

constexpr int MAX_NODES = FA_TREE_SAMPLE_MAX_NODES;
static_assert(sizeof(Record) == FA_TREE_RECORD_BYTES, "the record layout of include/fa_tree_sample.h");

// what phase B keeps of a sequence, per node
struct Nodes {
    int64_t tok[MAX_NODES];
    uint64_t w[MAX_NODES];  // one-hot: the weight of the node's token in its parent's target row, 0 outside the kept set
    float u[MAX_NODES], P[MAX_NODES], Q[MAX_NODES];
    int32_t par[MAX_NODES];  // -1: absent
    int32_t visited[MAX_NODES], accepted[MAX_NODES], path[MAX_NODES];
    int32_t skip[MAX_NODES];  // one-hot: the tokens the draw leaves out
    int32_t skips;
    uint64_t bloom;  // bit (token & 63) of every one of them
};

__device__ __forceinline__ Row target_row(const fa_tree_sample_params &p, const fa_tree_sample_form &f, int64_t b, int n) {
    const int64_t at = b * p.logits_batch_stride + (int64_t)n * p.logits_node_stride;
    return make_row(const_cast<char *>(row_of(p.logits, p.logits_dtype, at, 1)), p.logits_dtype, p.V, p.temperature, f.key_bits, f.frac_bits);
}
__device__ __forceinline__ Row draft_row(const fa_tree_sample_params &p, const fa_tree_sample_form &f, int64_t b, int n) {
    const int64_t at = b * p.draft_batch_stride + (int64_t)n * p.draft_node_stride;
    return make_row(const_cast<char *>(row_of(p.logits_draft, p.logits_dtype, at, 1)), p.logits_dtype, p.V, p.temperature, f.key_bits, f.frac_bits);
}

__device__ __forceinline__ int64_t draft_token(const fa_tree_sample_params &p, int64_t b, int i) {
    const int64_t at = b * p.tokens_draft_batch_stride + i;
    return p.tokens_dtype == FA_TREE_TOKENS_INT64 ? static_cast<const int64_t *>(p.tokens_draft)[at]
                                                  : (int64_t) static_cast<const int32_t *>(p.tokens_draft)[at];
}

// the parent of node i > 0, -1 where it has none in [0, i)
__device__ __forceinline__ int parent_of(const fa_tree_sample_params &p, int64_t b, int i) {
    const int32_t q = p.parents[b * p.parents_batch_stride + i];
    return q >= 0 && q < i ? q : -1;
}

// r_i(c) of the entries P, Q of a column
__device__ __forceinline__ uint64_t residual_of(float c, float P, float Q, float scale) {
    const float diff = __fmaf_rn(-c, Q, P);
    return diff > 0.0f ? (uint64_t)(diff * scale) : 0u;
}

// ---- phase A: the kept sets of every row ---------------------------------------------------------------------------------------
template <int CW>
__global__ __launch_bounds__(MAX_THREADS) void tree_select_kernel(const fa_tree_sample_params p, const fa_tree_sample_form f) {
    __shared__ Shared sh;
    const int T = p.T;
    const int64_t rows = p.B * T;
    Record *rec_p = static_cast<Record *>(p.workspace), *rec_q = rec_p + rows;
    const Selection how = {f.topk, f.topp, f.k, f.key_bits, f.index_bits, p.top_p};
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const int64_t b = r / T;
        const int n = (int)(r - b * T);
        Row rp = target_row(p, f, b, n);
        const Record a = select_row<CW>(sh, rp, how);
        if (threadIdx.x == 0) rec_p[r] = a;
        if (!f.drafts) continue;
        bool parent = false;  // (the same loads in every thread)
        for (int i = n + 1; i < T; ++i) parent = parent || parent_of(p, b, i) == n;
        if (!parent) continue;  // (a leaf's draft row is never read)
        Row rq = draft_row(p, f, b, n);
        const Record d = select_row<CW>(sh, rq, how);
        if (threadIdx.x == 0) rec_q[r] = d;
    }
}

// ---- phase B: the walk from the root and the token drawn where it ends ---------------------------------------------------------
template <int CW>
__global__ __launch_bounds__(MAX_THREADS) void tree_walk_kernel(const fa_tree_sample_params p, const fa_tree_sample_form f) {
    __shared__ Shared sh;
    __shared__ Nodes nd;
    const int T = p.T;
    const bool drafts = f.drafts != 0;
    const Record *rec_p = static_cast<const Record *>(p.workspace), *rec_q = rec_p + p.B * T;
    const uint32_t mix = p.rng_state ? seed_mix(p.rng_state) : 0u;
    for (int64_t b = blockIdx.x; b < p.B; b += gridDim.x) {
        // node i: its parent, token and uniform, and P(x), Q(x) of round 0 from the rows of the parent
        for (int i = threadIdx.x; i < T; i += blockDim.x) {
            const int par = i > 0 ? parent_of(p, b, i) : -1;
            const int64_t x = i > 0 ? draft_token(p, b, i) : 0;
            float P = 0.0f, Q = 0.0f;
            uint64_t w = 0;
            if (par >= 0 && x >= 0 && x < p.V) {  // (else nothing is read)
                const Record a = rec_p[b * T + par];
                Row rp = target_row(p, f, b, par);
                rp.m = a.m;
                const float e = load_one(rp.base, rp.dt, x);
                P = prob_of(rp, a, e, (int)x);
                Q = 1.0f;
                if (drafts) {
                    const Record d = rec_q[b * T + par];
                    Row rq = draft_row(p, f, b, par);
                    rq.m = d.m;
                    Q = prob_of(rq, d, load_one(rq.base, rq.dt, x), (int)x);
                } else if (P > 0.0f) {
                    w = rp.weight(rp.s(e));
                }
            }
            nd.par[i] = par;
            nd.tok[i] = x;
            nd.u[i] = i == 0 ? 0.0f : p.u_acc ? p.u_acc[b * T + i] : uniform_of(mix, b * T + i);
            nd.P[i] = P;
            nd.Q[i] = Q;
            nd.w[i] = w;
            nd.visited[i] = 0;
            nd.accepted[i] = 0;
        }
        if (threadIdx.x == 0) nd.path[0] = 0;
        __syncthreads();

        // the walk: every thread reads the same words and takes the same branches; thread 0 records it
        int n = 0, len = 1, m = 0;  // m: the rejections at n
        float c = 0.0f;
        uint64_t R = 0;  // R(c) under draft rows; Z_r under the one-hot rule
        Record a = rec_p[b * T], d = a;
        Row rp = target_row(p, f, b, 0), rq = rp;
        rp.m = a.m;
        if (!drafts) R = a.Zk;
        for (int i = 1; i < T; ++i) {
            if (nd.par[i] != n) continue;
            const int64_t x = nd.tok[i];
            const bool inside = x >= 0 && x < p.V;
            const float u = nd.u[i], P = nd.P[i], Q = nd.Q[i];
            bool ok;
            if (drafts) {
                if (m == 0) ok = (double)u * (double)Q <= (double)P;
                else ok = (double)u * (double)Q * (double)R <= (double)residual_of(c, P, Q, rp.scale);
                ok = ok && inside;
            } else {
                uint64_t w = nd.w[i];
                for (int j = n + 1; j < i; ++j) w = nd.par[j] == n && nd.tok[j] == x ? 0u : w;  // (rejected before at n)
                ok = w > 0 && (double)u * (double)R <= (double)w;
                if (!ok) R -= w;
            }
            if (threadIdx.x == 0) {
                nd.visited[i] = 1;
                nd.accepted[i] = ok ? 1 : 0;
                if (ok) nd.path[len] = i;
            }
            if (ok) {  // down to i: its rounds begin
                n = i;
                ++len;
                m = 0;
                c = 0.0f;
                a = rec_p[b * T + n];
                rp = target_row(p, f, b, n);
                rp.m = a.m;
                R = drafts ? 0u : a.Zk;
                continue;
            }
            ++m;
            if (drafts) {
                c = m == 1 ? 1.0f : (float)((double)c + (double)R * (1.0 / (double)rp.scale));
                if (m == 1) {
                    d = rec_q[b * T + n];
                    rq = draft_row(p, f, b, n);
                    rq.m = d.m;
                }
                uint64_t mine = 0;
                if (a.Zk > 0) {  // (else P = 0 and so is every r_i)
                    const Row2 both = {rp, rq};
                    walk<CW>(both, [&](int i0, const Pair (&v)[CW]) {
#pragma unroll
                        for (int k = 0; k < CW; ++k)
                            mine += residual_of(c, prob_of(rp, a, v[k].p, i0 + k), prob_of(rq, d, v[k].q, i0 + k), rp.scale);
                    });
                }
                wg_exclusive_scan(mine, sh.part, R);
            }
            if (R == 0) break;  // (nothing is left to accept: the siblings behind i are not tried)
        }

        const float u = p.u_res ? p.u_res[b] : uniform_of(mix, p.B * T + b);
        int token = 0;  // (of a target row that keeps nothing, or of which nothing is left)
        if (drafts) {
            if (m > 0 && R > 0) {
                const Row2 both = {rp, rq};
                uint64_t at = (uint64_t)((double)fmaxf(u, 0.0f) * (double)R);
                at = at < R ? at : R - 1;  // (only a u >= 1 gets here: the last index of positive weight)
                const Found hit = descend<CW>(sh, both, f.index_bits, at, [&](int i, const Pair &x, uint32_t &col, uint64_t &w) {
                    col = (uint32_t)i;
                    w = residual_of(c, prob_of(rp, a, x.p, i), prob_of(rq, d, x.q, i), rp.scale);
                    return w > 0;
                });
                token = hit.x < (uint32_t)p.V ? (int)hit.x : p.V - 1;
            } else if (a.Zk > 0) {
                token = draw_index<CW>(sh, rp, {a.K, a.J}, a.Zk, u, f.index_bits);
            }
        } else if (R > 0) {
            if (m == 0) {
                token = draw_index<CW>(sh, rp, {a.K, a.J}, a.Zk, u, f.index_bits);
            } else {
                if (threadIdx.x == 0) {  // the tokens rejected at n: of its children, all of which were tried
                    int cnt = 0;
                    uint64_t bloom = 0;
                    for (int i = n + 1; i < T; ++i)
                        if (nd.par[i] == n && nd.w[i] > 0) {
                            nd.skip[cnt++] = (int32_t)nd.tok[i];
                            bloom |= (uint64_t)1 << (nd.tok[i] & 63);
                        }
                    nd.skips = cnt;
                    nd.bloom = bloom;
                }
                __syncthreads();
                const int cnt = nd.skips, shift = rp.key_shift;
                const uint64_t bloom = nd.bloom;
                const Set kept = {a.K, a.J};
                uint64_t at = (uint64_t)((double)fmaxf(u, 0.0f) * (double)R);
                at = at < R ? at : R - 1;
                const Found hit = descend<CW>(sh, rp, f.index_bits, at, [&](int i, float x, uint32_t &col, uint64_t &w) {
                    const float sv = rp.s(x);
                    col = (uint32_t)i;
                    w = rp.weight(sv);
                    bool in = kept.has(full_key(sv) >> shift, i);
                    if (in && (bloom >> (i & 63) & 1))
                        for (int k = 0; k < cnt; ++k) in = in && nd.skip[k] != i;
                    return in;
                });
                token = hit.x < (uint32_t)p.V ? (int)hit.x : p.V - 1;
            }
        }
        __syncthreads();  // (thread 0's record of the walk)

        for (int j = threadIdx.x; j < T; j += blockDim.x) {
            const int64_t at = b * T + j;
            const int64_t x = j == len - 1 ? (int64_t)token : j < len - 1 ? nd.tok[nd.path[j + 1]] : 0;
            if (p.tokens_dtype == FA_TREE_TOKENS_INT64) static_cast<int64_t *>(p.tokens)[at] = x;
            else static_cast<int32_t *>(p.tokens)[at] = (int32_t)x;
            p.path[at] = j < len ? nd.path[j] : 0;
            if (p.p_tok) p.p_tok[at] = nd.P[j];
            if (p.q_tok) p.q_tok[at] = nd.Q[j];
            if (p.visited) p.visited[at] = nd.visited[j];
            if (p.accepted) p.accepted[at] = nd.accepted[j];
        }
        if (threadIdx.x == 0) {
            p.path_len[b] = len;
            p.num_generated[b] = len;
        }
        __syncthreads();  // (the next sequence overwrites nd)
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// the form of a valid call
fa_tree_sample_form form_of(const fa_tree_sample_params *p) {
    fa_tree_sample_form l{};
    const int es = esize(p->logits_dtype);
    const auto pitch_ok = [&](int64_t stride, bool used) { return !used || (stride * es) % 16 == 0; };
    bool wide = aligned_to(p->logits, 16) && ((int64_t)p->V * es) % 16 == 0 && pitch_ok(p->logits_batch_stride, p->B > 1) &&
                pitch_ok(p->logits_node_stride, p->T > 1);
    l.drafts = p->logits_draft != nullptr;
    if (l.drafts)
        wide = wide && aligned_to(p->logits_draft, 16) && pitch_ok(p->draft_batch_stride, p->B > 1) && pitch_ok(p->draft_node_stride, p->T > 1);
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
    const int64_t rows = p->B * p->T;
    l.grid_a = (int32_t)(rows < MAX_GRID ? rows : MAX_GRID);
    l.grid_b = (int32_t)(p->B < MAX_GRID ? p->B : MAX_GRID);
    return l;
}

template <int CW>
void launch(const fa_tree_sample_params *p, const fa_tree_sample_form &l, hipStream_t stream) {
    const dim3 block(l.threads);
    hipLaunchKernelGGL((tree_select_kernel<CW>), dim3(l.grid_a), block, 0, stream, *p, l);
    hipLaunchKernelGGL((tree_walk_kernel<CW>), dim3(l.grid_b), block, 0, stream, *p, l);
}

}  // namespace

extern "C" {

uint32_t fa_tree_sample_params_size(void) { return (uint32_t)sizeof(fa_tree_sample_params); }

int64_t fa_tree_sample_workspace_size(int64_t B, int32_t T) {
    if (B < 0 || T < 1) return 0;
    return B * 2 * (int64_t)T * FA_TREE_RECORD_BYTES;
}

int fa_tree_sample_validate(const fa_tree_sample_params *p) {
    if (!p) return FA_ERR_NULL_POINTER;
    if (p->abi_version != FA_ABI_VERSION || p->struct_size != sizeof(fa_tree_sample_params)) return FA_ERR_BAD_ABI;
    if (!known_dtype(p->logits_dtype)) return FA_ERR_BAD_DTYPE;
    if (p->tokens_dtype != FA_TREE_TOKENS_INT32 && p->tokens_dtype != FA_TREE_TOKENS_INT64) return FA_ERR_BAD_DTYPE;
    if (p->B < 0 || p->T < 1 || p->T > MAX_NODES || p->V < 1 || p->top_k < 0) return FA_ERR_BAD_SHAPE;  // (V < 2^31 by its type)
    if (p->B > ((int64_t)1 << 31) - 1 || p->B * 2 * (int64_t)p->T > ((int64_t)1 << 31) - 1) return FA_ERR_BAD_SHAPE;
    if (!(p->temperature > 0.0f) || !(p->top_p >= 0.0f && p->top_p <= 1.0f)) return FA_ERR_BAD_SHAPE;  // (NaN fails both)
    if (!p->logits || !p->tokens_draft || !p->parents || !p->path || !p->path_len || !p->tokens || !p->num_generated) return FA_ERR_NULL_POINTER;
    if (!p->u_res && !p->u_acc && !p->rng_state) return FA_ERR_NULL_POINTER;
    if (p->rng_state && (p->u_res || p->u_acc)) return FA_ERR_BAD_SHAPE;
    if (!p->rng_state && (!p->u_res || (p->T > 1 && !p->u_acc))) return FA_ERR_NULL_POINTER;
    const int es = esize(p->logits_dtype), ts = p->tokens_dtype == FA_TREE_TOKENS_INT64 ? 8 : 4;
    if (!aligned_to(p->logits, es) || !aligned_to(p->logits_draft, es) || !aligned_to(p->tokens_draft, ts) || !aligned_to(p->tokens, ts) ||
        !aligned_to(p->parents, 4) || !aligned_to(p->path, 4) || !aligned_to(p->path_len, 4) || !aligned_to(p->u_acc, 4) ||
        !aligned_to(p->u_res, 4) || !aligned_to(p->rng_state, 8) || !aligned_to(p->num_generated, 8) || !aligned_to(p->p_tok, 4) ||
        !aligned_to(p->q_tok, 4) || !aligned_to(p->visited, 4) || !aligned_to(p->accepted, 4) || !aligned_to(p->workspace, 8))
        return FA_ERR_BAD_STRIDE;
    const int64_t need = fa_tree_sample_workspace_size(p->B, p->T);
    if (need > 0 && (!p->workspace || p->workspace_bytes < need)) return FA_ERR_WORKSPACE;
    return FA_OK;
}

int fa_tree_sample_plan(const fa_tree_sample_params *p, fa_tree_sample_form *plan) {
    const int st = fa_tree_sample_validate(p);
    if (st != FA_OK) return st;
    if (!plan) return FA_ERR_NULL_POINTER;
    *plan = form_of(p);
    return FA_OK;
}

int fa_tree_sample(const fa_tree_sample_params *p, void *stream_) {
    const int st = fa_tree_sample_validate(p);
    if (st != FA_OK) return st;
    if (p->B == 0) return FA_OK;  // (no zero grid)
    const fa_tree_sample_form l = form_of(p);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (l.cw == 8) launch<8>(p, l, stream);
    else if (l.cw == 4) launch<4>(p, l, stream);
    else launch<1>(p, l, stream);
    if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
    return FA_OK;
}

}  // extern "C"
