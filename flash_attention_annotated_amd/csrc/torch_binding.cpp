// torch_binding.cpp — compiled `flash_attn_2_cuda` and `flash_attn_3_cuda` surfaces over the C-ABI (include/fa_fwd.h,
// include/fa_bwd.h).
//
// The pybind module of csrc/flash_attn/flash_api.cpp:1478-1485: fwd / varlen_fwd / bwd / varlen_bwd / fwd_kvcache with the
// reference's positional argument lists, doing the host work of mha_fwd (:350-512), mha_varlen_fwd (:514-755), mha_bwd
// (:767-971), mha_varlen_bwd (:973-1200) and mha_fwd_kvcache (:1202-1476) -- TORCH_CHECKs with the reference's texts, output /
// LSE / softmax_d allocation, the params struct -- and enqueueing the gfx950 kernels on torch's current stream.  Beside them
// the FA3 operators of hopper/flash_api.cpp: fa3_fwd (mha_fwd, :672-1198), fa3_bwd (mha_bwd, :1259-1570) and
// fa3_fwd_combine (mha_combine, :1569-1670).  Host code only: built by plain g++ against the torch headers (no hipify, no
// device code here), linked to libfa_fwd_gfx950.so.  This is the only host path of both surfaces: flash_attn_2_cuda.py and
// flash_attn_3_cuda.py re-export these functions as they are, flash_attn_3_ops.py registers them under the FA3 op schemas.
#include <torch/extension.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <tuple>
#include <variant>
#include <vector>

#include "fa_bwd.h"
#include "fa_fwd.h"
#include "../../include/fa_rotary.h"  // ("fa_rotary.h" from here is the device header next to this file)
#include "fa_norm.h"
#include "fa_xent.h"
#include "fa_sample.h"
#include "fa_spec_sample.h"
#include "fa_tree_sample.h"
#include "fa_block_select.h"
#include "fa_block_pattern.h"
#include "fa_act.h"
#include "fa_gemm_act.h"
#include "fa_dropout_norm.h"

namespace {

using at::Tensor;
using OptTensor = c10::optional<at::Tensor>;

#define CHECK_DEVICE(x, name) TORCH_CHECK((x).is_cuda(), name " must be on CUDA")
#define CHECK_SHAPE(x, name, ...) \
    TORCH_CHECK((x).sizes() == c10::IntArrayRef({__VA_ARGS__}), name " must have shape (" #__VA_ARGS__ ")")
#define CHECK_LAST_CONTIGUOUS(x, msg) TORCH_CHECK((x).stride(-1) == 1, msg)

int dtype_code(const Tensor &t) {
    if (t.scalar_type() == at::kHalf) return FA_DTYPE_FP16;
    if (t.scalar_type() == at::kBFloat16) return FA_DTYPE_BF16;
    if (t.scalar_type() == at::kFloat8_e4m3fn) return FA_DTYPE_FP8_E4M3;
    TORCH_CHECK(false, "FlashAttention only support fp16 and bf16 data type");
    return -1;
}

// the kernels move 16-byte vectors (the fp8 expansion pass 8-byte ones): bases and the non-unit strides must keep rows
// aligned (views that do not are copied)
bool aligned(const Tensor &t) {
    if (reinterpret_cast<uintptr_t>(t.data_ptr()) % (t.element_size() == 2 ? 16 : 8) != 0) return false;
    for (int64_t i = 0; i + 1 < t.dim(); ++i)
        if (t.stride(i) % 8 != 0) return false;
    return true;
}
// (clone, not contiguous(): a contiguous tensor whose base is off the boundary must move to a fresh allocation as well)
Tensor aligned_or_copy(const Tensor &t) { return aligned(t) ? t : t.clone(at::MemoryFormat::Contiguous); }

void *ptr(const OptTensor &t) { return t.has_value() ? t->data_ptr() : nullptr; }
void *ptr(const Tensor &t) { return t.data_ptr(); }

int64_t round128(int64_t x) { return (x + 127) / 128 * 128; }

// kBlockN of the reference's forward for this head dim (flash_attn/flash_attn_interface.py:23-46, a device that is neither
// sm8x nor sm90): the key-block width behind the running maxima of S_dmask
int sdmask_block_n(int64_t head_dim, bool is_dropout, bool /*is_causal*/) {
    if (head_dim <= 32) return 128;
    if (head_dim <= 64) return is_dropout ? 64 : 128;
    if (head_dim <= 96) return 64;
    if (head_dim <= 128) return is_dropout ? 32 : 64;
    return 64;
}

void check_dropout(double p_dropout, bool return_softmax) {
    TORCH_CHECK(p_dropout >= 0.0 && p_dropout < 1.0, "p_dropout must be in [0, 1)");
    if (return_softmax) TORCH_CHECK(p_dropout > 0.0, "return_softmax is only supported when p_dropout > 0.0");
}

// (seed, offset) of this call, drawn ON THE DEVICE from gen_ / the default generator (role of philox_cuda_state, :486-493)
Tensor dropout_state(double p_dropout, const c10::optional<at::Generator> &gen, const Tensor &like) {
    auto opts = like.options().dtype(at::kLong);
    if (p_dropout <= 0.0) return at::zeros({2}, opts);
    return at::randint(-(int64_t(1) << 62), int64_t(1) << 62, {2}, gen, opts);
}

OptTensor check_alibi(const OptTensor &a, int64_t batch_size, int64_t num_heads) {
    if (!a.has_value()) return a;
    TORCH_CHECK(a->scalar_type() == at::kFloat, "ALiBi slopes must have dtype fp32");
    CHECK_DEVICE(*a, "alibi_slopes");
    TORCH_CHECK(a->stride(-1) == 1, "ALiBi slopes tensor must have contiguous last dimension");
    TORCH_CHECK(a->sizes() == c10::IntArrayRef({num_heads}) || a->sizes() == c10::IntArrayRef({batch_size, num_heads}),
                "alibi_slopes must have shape (num_heads) or (batch_size, num_heads)");
    return a;
}

void check_leftpad(const OptTensor &lp, int64_t batch_size, bool paged) {
    if (!lp.has_value()) return;
    TORCH_CHECK(!paged, "We don't support Paged KV and leftpad_k running at the same time yet");
    TORCH_CHECK(lp->scalar_type() == at::kInt, "leftpad_k must have dtype int32");
    CHECK_DEVICE(*lp, "leftpad_k");
    TORCH_CHECK(lp->is_contiguous(), "leftpad_k must be contiguous");
    CHECK_SHAPE(*lp, "leftpad_k", batch_size);
}

// returns (page_block_size, max_num_blocks_per_seq)
std::pair<int64_t, int64_t> check_block_table(const Tensor &bt, const Tensor &kcache, int64_t batch_size, int64_t page_multiple) {
    CHECK_DEVICE(bt, "block_table");
    TORCH_CHECK(bt.scalar_type() == at::kInt, "block_table must have dtype torch.int32");
    TORCH_CHECK(bt.stride(-1) == 1, "block_table must have contiguous last dimension");
    TORCH_CHECK(kcache.dim() == 4, "paged k/v must have shape (num_blocks, page_block_size, num_heads_k, head_size)");
    const int64_t page = kcache.size(1);
    TORCH_CHECK(page % page_multiple == 0, "Paged KV cache block size must be divisible by ", page_multiple);
    TORCH_CHECK(bt.dim() == 2 && bt.size(0) == batch_size, "block_table must have shape (batch_size, max_num_blocks_per_seq)");
    return {page, bt.size(1)};
}

hipStream_t current_stream(const Tensor &t) {
    return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.get_device()).stream();
}

struct FwdArgs {
    bool varlen = false;
    int64_t batch = 0, max_seqlen_q = 0, max_seqlen_k = 0;
    double softmax_scale = 1.0, softcap = 0.0, p_dropout = 0.0;
    bool causal = false;
    int64_t window_left = -1, window_right = -1;
    OptTensor cu_seqlens_q, cu_seqlens_k, seqused_k, alibi, kv_batch_idx, block_table, leftpad_k, rng_state, s_dmask, qv;
    int num_splits = 1, s_dmask_block_n = 0;
    // FA3 only (the FA2 entry points leave them unset): per-(batch, kv head) fp8 descales, the FA3 window rule
    OptTensor seqused_q, q_descale, k_descale, v_descale;
    bool fa3_window = false;
    int64_t attention_chunk = 0;
    // cute surface only: the learnable sink, (num_heads,) bf16 or fp32, and how the kernel's (head, row) finds its logit --
    // (1, 0), or (ngroups, 1) when the decode route has folded the GQA group into the rows (include/fa_fwd.h)
    OptTensor sink;
    int sink_head_stride = 1, sink_row_stride = 0;
    // FA3 / cute pack_gqa = True: FA_FLAG_PACK_GQA, a hint the plan honours where the pk kernel serves the call (include/fa_fwd.h)
    bool pack_gqa = false;
};

// fa_fwd_params of one forward call: every entry point's filler -- the 16-bit and fp8 routes, the fp8-cache reads and the
// block-sparse ones alike (q/k/v/out: last stride 1, aligned(); a KV cache: cache_aligned())
fa_fwd_params fill_fwd_params(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &out, const Tensor &lse, const FwdArgs &a) {
    fa_fwd_params p{};
    p.abi_version = FA_ABI_VERSION;
    p.struct_size = sizeof(fa_fwd_params);
    p.q = q.data_ptr(); p.k = k.data_ptr(); p.v = v.data_ptr(); p.o = out.data_ptr();
    p.softmax_lse = static_cast<float *>(lse.data_ptr());
    const bool paged = a.block_table.has_value();
    if (a.varlen) {
        p.q_row_stride = q.stride(0); p.q_head_stride = q.stride(1);
        p.o_row_stride = out.stride(0); p.o_head_stride = out.stride(1);
        if (paged || k.dim() == 4) {  // k, v: (num_blocks, page_block_size, h_k, d), or a batched cache under ragged queries
            p.k_batch_stride = k.stride(0); p.k_row_stride = k.stride(1); p.k_head_stride = k.stride(2);
            p.v_batch_stride = v.stride(0); p.v_row_stride = v.stride(1); p.v_head_stride = v.stride(2);
        } else {
            p.k_row_stride = k.stride(0); p.k_head_stride = k.stride(1);
            p.v_row_stride = v.stride(0); p.v_head_stride = v.stride(1);
        }
        p.total_q = (int32_t)q.size(0);
        p.total_k = k.dim() == 4 ? 0 : (int32_t)k.size(0);
        p.h = (int32_t)q.size(1); p.h_k = (int32_t)k.size(-2); p.d = (int32_t)q.size(2);
    } else {
        p.q_batch_stride = q.stride(0); p.q_row_stride = q.stride(1); p.q_head_stride = q.stride(2);
        p.k_batch_stride = k.stride(0); p.k_row_stride = k.stride(1); p.k_head_stride = k.stride(2);
        p.v_batch_stride = v.stride(0); p.v_row_stride = v.stride(1); p.v_head_stride = v.stride(2);
        p.o_batch_stride = out.stride(0); p.o_row_stride = out.stride(1); p.o_head_stride = out.stride(2);
        p.h = (int32_t)q.size(2); p.h_k = (int32_t)k.size(2); p.d = (int32_t)q.size(3);
    }
    p.b = (int32_t)a.batch; p.seqlen_q = (int32_t)a.max_seqlen_q; p.seqlen_k = (int32_t)a.max_seqlen_k;
    p.dtype = dtype_code(q);
    p.cu_seqlens_q = static_cast<const int32_t *>(ptr(a.cu_seqlens_q));
    p.cu_seqlens_k = static_cast<const int32_t *>(ptr(a.cu_seqlens_k));
    p.seqused_q = static_cast<const int32_t *>(ptr(a.seqused_q));
    p.seqused_k = static_cast<const int32_t *>(ptr(a.seqused_k));
    p.softmax_scale = (float)a.softmax_scale;
    p.softcap = (float)a.softcap;
    p.is_causal = a.causal ? 1 : 0;
    p.window_size_left = (int32_t)a.window_left; p.window_size_right = (int32_t)a.window_right;
#define FA_SET_DESCALE(name)                                                                                \
    if (a.name##_descale.has_value()) {  /* (b, h_k) fp32 */                                               \
        p.name##_descale = static_cast<const float *>(a.name##_descale->data_ptr());                       \
        p.name##_descale_batch_stride = a.name##_descale->stride(0);                                       \
        p.name##_descale_head_stride = a.name##_descale->stride(1);                                        \
    }
    FA_SET_DESCALE(q) FA_SET_DESCALE(k) FA_SET_DESCALE(v)
#undef FA_SET_DESCALE
    if (a.alibi.has_value()) {  // (h) or (b, h) fp32
        p.alibi_slopes = static_cast<const float *>(a.alibi->data_ptr());
        p.alibi_slopes_batch_stride = a.alibi->dim() == 2 ? a.alibi->stride(0) : 0;
    }
    p.kv_batch_idx = static_cast<const int32_t *>(ptr(a.kv_batch_idx));
    p.leftpad_k = static_cast<const int32_t *>(ptr(a.leftpad_k));
    p.p_dropout = (float)a.p_dropout;
    p.rng_state = static_cast<const uint64_t *>(ptr(a.rng_state));
    p.s_dmask = static_cast<uint8_t *>(ptr(a.s_dmask));
    p.flags = a.fa3_window ? FA_FLAG_FA3_WINDOW : 0;  // a missing window side is unbounded (hopper/flash_api.cpp:152-153)
    if (a.pack_gqa) p.flags |= FA_FLAG_PACK_GQA;
    if (a.s_dmask.has_value() && a.s_dmask_block_n > 0) {
        p.flags |= FA_FLAG_SDMASK_SIGNED;
        p.s_dmask_rows = (int32_t)a.s_dmask->size(-2);
        p.s_dmask_cols = (int32_t)a.s_dmask->size(-1);
        p.s_dmask_block_n = a.s_dmask_block_n;
    }
    p.num_splits = a.num_splits;
    p.attention_chunk = (int32_t)a.attention_chunk;
    if (v.size(-1) != q.size(-1)) p.d_v = (int32_t)v.size(-1);  // FA3 headdim_v (ABI v12)
    if (a.qv.has_value()) {  // FA3 qv, laid out like q with V's head dim (ABI v13)
        p.qv = a.qv->data_ptr();
        p.qv_batch_stride = a.varlen ? 0 : a.qv->stride(0);
        p.qv_row_stride = a.qv->stride(-3); p.qv_head_stride = a.qv->stride(-2);
    }
    if (paged) {
        p.block_table = static_cast<const int32_t *>(a.block_table->data_ptr());
        p.block_table_batch_stride = a.block_table->stride(0);
        p.page_block_size = (int32_t)k.size(1);
    }
    return p;
}

// `need` bytes of scratch (what the entry's _workspace_size answered: fp8 expansion, split-KV partials) from torch's caching
// allocator -- the callee never allocates -- on a 256-byte boundary; the tensor returned keeps them alive over the launch
Tensor set_workspace(fa_fwd_params &p, int64_t need, const Tensor &like) {
    Tensor workspace;
    if (need > 0) {
        workspace = at::empty({need + 256}, like.options().dtype(at::kByte));
        const uintptr_t base = (reinterpret_cast<uintptr_t>(workspace.data_ptr()) + 255) / 256 * 256;
        p.workspace = reinterpret_cast<void *>(base);
        p.workspace_bytes = (uint64_t)need;
    }
    return workspace;
}

// the learnable sink beside the forward params: (1, 0), or the strides of FwdArgs behind the decode route's GQA swap
fa_sink_params fill_sink_params(const Tensor &sink, int head_stride = 1, int row_stride = 0) {
    fa_sink_params s{};
    s.abi_version = FA_ABI_VERSION;
    s.struct_size = sizeof(fa_sink_params);
    s.learnable_sink = sink.data_ptr();
    s.sink_dtype = sink.scalar_type() == at::kFloat ? FA_DTYPE_FP32 : FA_DTYPE_BF16;
    s.sink_head_stride = head_stride; s.sink_row_stride = row_stride;
    return s;
}

// torch tensors -> fa_fwd_params -> fa_fwd (with a sink: fa_fwd_sink, same params, same plan, same workspace) on torch's
// current stream
void launch_fwd(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &out, const Tensor &lse, const FwdArgs &a) {
    fa_fwd_params p = fill_fwd_params(q, k, v, out, lse, a);
    const int64_t need = fa_fwd_workspace_size(&p);
    TORCH_CHECK(need >= 0, "fa_fwd_workspace_size failed (", need, "): ", fa_strerror((int)need));
    const Tensor workspace = set_workspace(p, need, q);
    if (a.sink.has_value()) {
        const fa_sink_params s = fill_sink_params(*a.sink, a.sink_head_stride, a.sink_row_stride);
        const int st = fa_fwd_sink(&p, &s, current_stream(q));
        TORCH_CHECK(st == 0, "fa_fwd_sink failed (", st, "): ", fa_strerror(st));
        return;
    }
    const int st = fa_fwd(&p, current_stream(q));
    TORCH_CHECK(st == 0, "fa_fwd failed (", st, "): ", fa_strerror(st));
}

// A forward's out: the caller's tensor and the one the kernel writes -- the caller's own where it is aligned(), else a fresh
// contiguous one of its shape and dtype (aligned() for every head dim the entry points admit: a multiple of 8 on a fresh
// allocation), which finish() copies back
struct OutPath {
    Tensor given, work;
    explicit OutPath(const Tensor &out) : given(out), work(aligned(out) ? out : at::empty(out.sizes(), out.options())) {}
    void finish() const {
        if (!work.is_same(given)) given.copy_(work);
    }
};

constexpr float kInf = std::numeric_limits<float>::infinity();

// The result of a problem without keys: zeros, LSE = +inf -- with a sink the logsumexp of the sink alone, its (num_heads,)
// viewed as `lse_layout` to broadcast over the rows of this route's LSE: (1, h, 1), ragged (h, 1), behind the decode swap
// (1, h_k, ngroups)
void fill_empty(const Tensor &out, const Tensor &lse, const OptTensor &sink = c10::nullopt, c10::IntArrayRef lse_layout = {}) {
    out.zero_();
    lse.fill_(kInf);
    if (sink.has_value()) lse.copy_(sink->to(at::kFloat).view(lse_layout));
}

std::vector<Tensor> mha_fwd(Tensor &q, const Tensor &k, const Tensor &v, OptTensor &out_, OptTensor &alibi_slopes_,
                            const double p_dropout, const double softmax_scale, bool is_causal, int64_t window_size_left,
                            int64_t window_size_right, const double softcap, const bool return_softmax,
                            c10::optional<at::Generator> gen_) {
    const auto q_dtype = q.scalar_type();
    TORCH_CHECK(q_dtype == at::kHalf || q_dtype == at::kBFloat16, "FlashAttention only support fp16 and bf16 data type");
    TORCH_CHECK(k.scalar_type() == q_dtype, "query and key must have the same dtype");
    TORCH_CHECK(v.scalar_type() == q_dtype, "query and value must have the same dtype");
    CHECK_DEVICE(q, "q"); CHECK_DEVICE(k, "k"); CHECK_DEVICE(v, "v");
    CHECK_LAST_CONTIGUOUS(q, "Input tensor must have contiguous last dimension");
    CHECK_LAST_CONTIGUOUS(k, "Input tensor must have contiguous last dimension");
    CHECK_LAST_CONTIGUOUS(v, "Input tensor must have contiguous last dimension");
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, "q, k, v must have 4 dimensions");
    const int64_t batch_size = q.size(0), seqlen_q = q.size(1), num_heads = q.size(2), head_size = q.size(3);
    const int64_t seqlen_k = k.size(1), num_heads_k = k.size(2);
    TORCH_CHECK(batch_size > 0, "batch size must be positive");
    TORCH_CHECK(head_size <= 256, "FlashAttention forward only supports head dimension at most 256");
    TORCH_CHECK(head_size % 8 == 0, "query, key, value, and out_ must have a head_size that is a multiple of 8");
    TORCH_CHECK(num_heads % num_heads_k == 0, "Number of heads in key/value must divide number of heads in query");
    if (softcap > 0.0) TORCH_CHECK(p_dropout == 0.0, "Softcapping does not support dropout for now");
    check_dropout(p_dropout, return_softmax);
    const OptTensor alibi = check_alibi(alibi_slopes_, batch_size, num_heads);
    if (seqlen_q == 1 && !alibi_slopes_.has_value()) is_causal = false;  // causal=true is the same as causal=false here (:402)
    CHECK_SHAPE(q, "q", batch_size, seqlen_q, num_heads, head_size);
    CHECK_SHAPE(k, "k", batch_size, seqlen_k, num_heads_k, head_size);
    CHECK_SHAPE(v, "v", batch_size, seqlen_k, num_heads_k, head_size);
    Tensor out;
    if (out_.has_value()) {
        out = out_.value();
        TORCH_CHECK(out.scalar_type() == q_dtype, "Output must have the same dtype as inputs");
        CHECK_DEVICE(out, "out");
        TORCH_CHECK(out.stride(-1) == 1, "Output tensor must have contiguous last dimension");
        CHECK_SHAPE(out, "out", batch_size, seqlen_q, num_heads, head_size);
    } else {
        out = at::empty_like(q);
    }
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(q.device());
    auto opts = q.options();
    Tensor softmax_lse = at::empty({batch_size, num_heads, seqlen_q}, opts.dtype(at::kFloat));
    // return_softmax: S_dmask (b, h, seqlen_q r128, seqlen_k r128) in the input dtype (csrc/flash_attn/flash_api.cpp:436-449)
    Tensor p = return_softmax ? at::zeros({batch_size, num_heads, round128(seqlen_q), round128(seqlen_k)}, opts) : at::empty({0}, opts);
    Tensor rng_state = dropout_state(p_dropout, gen_, q);
    if (seqlen_k > 0 && seqlen_q > 0) {
        const Tensor qc = aligned_or_copy(q), kc = aligned_or_copy(k), vc = aligned_or_copy(v);
        const OutPath o(out);
        FwdArgs a;
        a.batch = batch_size; a.max_seqlen_q = seqlen_q; a.max_seqlen_k = seqlen_k;
        a.softmax_scale = softmax_scale; a.causal = is_causal; a.window_left = window_size_left; a.window_right = window_size_right;
        a.softcap = softcap; a.alibi = alibi; a.p_dropout = p_dropout;
        if (p_dropout > 0) a.rng_state = rng_state;
        if (return_softmax) a.s_dmask = p;
        a.s_dmask_block_n = sdmask_block_n(head_size, p_dropout > 0, is_causal);
        a.num_splits = p_dropout == 0.0 ? 0 : 1;  // the split heuristic runs whenever there is no dropout (:453-456)
        launch_fwd(qc, kc, vc, o.work, softmax_lse, a);
        o.finish();
    } else if (seqlen_q > 0) {
        fill_empty(out, softmax_lse);  // seqlen_k == 0: empty attention (:499-504)
    }
    return {out, softmax_lse, p, rng_state};
}

std::vector<Tensor> mha_varlen_fwd(Tensor &q, const Tensor &k, const Tensor &v, OptTensor &out_, const Tensor &cu_seqlens_q,
                                   const Tensor &cu_seqlens_k, OptTensor &seqused_k, OptTensor &leftpad_k_,
                                   OptTensor &block_table_, OptTensor &alibi_slopes_, int64_t max_seqlen_q,
                                   const int64_t max_seqlen_k, const double p_dropout, const double softmax_scale,
                                   const bool zero_tensors, bool is_causal, int64_t window_size_left, int64_t window_size_right,
                                   const double softcap, const bool return_softmax, c10::optional<at::Generator> gen_) {
    const auto q_dtype = q.scalar_type();
    TORCH_CHECK(q_dtype == at::kHalf || q_dtype == at::kBFloat16, "FlashAttention only support fp16 and bf16 data type");
    TORCH_CHECK(k.scalar_type() == q_dtype, "query and key must have the same dtype");
    TORCH_CHECK(v.scalar_type() == q_dtype, "query and value must have the same dtype");
    TORCH_CHECK(cu_seqlens_q.scalar_type() == at::kInt, "cu_seqlens_q must have dtype int32");
    TORCH_CHECK(cu_seqlens_k.scalar_type() == at::kInt, "cu_seqlens_k must have dtype int32");
    CHECK_DEVICE(q, "q"); CHECK_DEVICE(k, "k"); CHECK_DEVICE(v, "v");
    CHECK_DEVICE(cu_seqlens_q, "cu_seqlens_q"); CHECK_DEVICE(cu_seqlens_k, "cu_seqlens_k");
    const bool paged = block_table_.has_value();
    CHECK_LAST_CONTIGUOUS(q, "Input tensor must have contiguous last dimension");
    CHECK_LAST_CONTIGUOUS(k, "Input tensor must have contiguous last dimension");
    CHECK_LAST_CONTIGUOUS(v, "Input tensor must have contiguous last dimension");
    TORCH_CHECK(cu_seqlens_q.is_contiguous(), "cu_seqlens_q must be contiguous");
    TORCH_CHECK(cu_seqlens_k.is_contiguous(), "cu_seqlens_k must be contiguous");
    TORCH_CHECK(q.dim() == 3, "q must have shape (total_q, num_heads, head_size)");
    const int64_t total_q = q.size(0), num_heads = q.size(1), head_size = q.size(2);
    const int64_t batch_size = cu_seqlens_q.numel() - 1;
    int64_t total_k = 0, num_heads_k = 0;
    if (paged) {  // k, v: (num_blocks, page_block_size, h_k, d), rows found through block_table (:554-560, :608-612)
        check_block_table(*block_table_, k, batch_size, 256);
        num_heads_k = k.size(2);
    } else {
        TORCH_CHECK(k.dim() == 3, "k must have shape (total_k, num_heads_k, head_size)");
        total_k = k.size(0); num_heads_k = k.size(1);
    }
    TORCH_CHECK(batch_size > 0, "batch size must be positive");
    TORCH_CHECK(head_size <= 256, "FlashAttention forward only supports head dimension at most 256");
    TORCH_CHECK(head_size % 8 == 0, "query, key, value, and out_ must have a head_size that is a multiple of 8");
    TORCH_CHECK(num_heads % num_heads_k == 0, "Number of heads in key/value must divide number of heads in query");
    if (softcap > 0.0) TORCH_CHECK(p_dropout == 0.0, "Softcapping does not support dropout for now");
    check_dropout(p_dropout, return_softmax);
    if (p_dropout > 0.0)
        TORCH_CHECK(!paged && !leftpad_k_.has_value(), "dropout is not supported with a paged or left-padded KV cache");
    const OptTensor alibi = check_alibi(alibi_slopes_, batch_size, num_heads);
    if (max_seqlen_q == 1 && !alibi_slopes_.has_value()) is_causal = false;  // (:590)
    CHECK_SHAPE(q, "q", total_q, num_heads, head_size);
    if (paged) {
        CHECK_SHAPE(k, "k", k.size(0), k.size(1), num_heads_k, head_size);
        CHECK_SHAPE(v, "v", k.size(0), k.size(1), num_heads_k, head_size);
    } else {
        CHECK_SHAPE(k, "k", total_k, num_heads_k, head_size);
        CHECK_SHAPE(v, "v", total_k, num_heads_k, head_size);
    }
    CHECK_SHAPE(cu_seqlens_q, "cu_seqlens_q", batch_size + 1);
    CHECK_SHAPE(cu_seqlens_k, "cu_seqlens_k", batch_size + 1);
    check_leftpad(leftpad_k_, batch_size, paged);
    if (seqused_k.has_value()) {
        TORCH_CHECK(seqused_k->scalar_type() == at::kInt, "seqused_k must have dtype int32");
        CHECK_DEVICE(*seqused_k, "seqused_k");
        TORCH_CHECK(seqused_k->is_contiguous(), "seqused_k must be contiguous");
        CHECK_SHAPE(*seqused_k, "seqused_k", batch_size);
    }
    Tensor out;
    if (out_.has_value()) {
        out = out_.value();
        TORCH_CHECK(out.scalar_type() == q_dtype, "Output must have the same dtype as inputs");
        CHECK_DEVICE(out, "out");
        TORCH_CHECK(out.stride(-1) == 1, "Output tensor must have contiguous last dimension");
        CHECK_SHAPE(out, "out", total_q, num_heads, head_size);
    } else {
        out = at::empty_like(q);
    }
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(q.device());
    auto opts = q.options();
    Tensor softmax_lse = at::empty({num_heads, total_q}, opts.dtype(at::kFloat));
    Tensor p = return_softmax ? at::zeros({batch_size, num_heads, round128(max_seqlen_q), round128(max_seqlen_k)}, opts)
                              : at::empty({0}, opts);
    Tensor rng_state = dropout_state(p_dropout, gen_, q);
    if (zero_tensors) {
        out.zero_();
        softmax_lse.fill_(-kInf);
    }
    if (max_seqlen_k > 0 && total_q > 0 && max_seqlen_q > 0) {
        const Tensor qc = aligned_or_copy(q), kc = aligned_or_copy(k), vc = aligned_or_copy(v);
        const OutPath o(out);
        FwdArgs a;
        a.varlen = true; a.batch = batch_size; a.max_seqlen_q = max_seqlen_q; a.max_seqlen_k = max_seqlen_k;
        a.softmax_scale = softmax_scale; a.causal = is_causal; a.window_left = window_size_left; a.window_right = window_size_right;
        a.softcap = softcap; a.cu_seqlens_q = cu_seqlens_q; a.cu_seqlens_k = cu_seqlens_k; a.seqused_k = seqused_k;
        a.alibi = alibi; a.block_table = block_table_; a.leftpad_k = leftpad_k_; a.p_dropout = p_dropout;
        if (p_dropout > 0) a.rng_state = rng_state;
        if (return_softmax) a.s_dmask = p;
        a.s_dmask_block_n = sdmask_block_n(head_size, p_dropout > 0, is_causal);
        launch_fwd(qc, kc, vc, o.work, softmax_lse, a);
        o.finish();
    } else if (total_q > 0) {
        fill_empty(out, softmax_lse);
    }
    return {out, softmax_lse, p, rng_state};
}

Tensor grad_out(const OptTensor &given, const Tensor &like, const char *name, c10::IntArrayRef shape) {
    if (!given.has_value()) return at::empty_like(like);
    TORCH_CHECK(given->scalar_type() == like.scalar_type(), name, " must have the same dtype as q");
    TORCH_CHECK(given->is_cuda(), name, " must be on CUDA");
    TORCH_CHECK(given->stride(-1) == 1, name, " must have contiguous last dimension");
    TORCH_CHECK(given->sizes() == shape, name, " must have shape ", shape);
    return given.value();
}

struct BwdArgs {
    bool varlen = false;
    int64_t batch = 0, max_seqlen_q = 0, max_seqlen_k = 0;
    double softmax_scale = 1.0, softcap = 0.0, p_dropout = 0.0;
    bool causal = false, deterministic = false;
    int64_t window_left = -1, window_right = -1;
    OptTensor cu_seqlens_q, cu_seqlens_k, alibi, rng_state;
    bool fa3_window = false;  // the window rule of the FA3 surface (fa3_bwd)
};

// fa_bwd_params of one backward call (every entry point's filler, the block-sparse one's too)
fa_bwd_params fill_bwd_params(const Tensor &dout, const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &out, const Tensor &lse,
                              const Tensor &dq, const Tensor &dk, const Tensor &dv, const Tensor &softmax_d, const BwdArgs &a) {
    fa_bwd_params p{};
    p.abi_version = FA_ABI_VERSION;
    p.struct_size = sizeof(fa_bwd_params);
    p.q = q.data_ptr(); p.k = k.data_ptr(); p.v = v.data_ptr(); p.o = out.data_ptr(); p.dout = dout.data_ptr();
    p.softmax_lse = static_cast<const float *>(lse.data_ptr());
    p.softmax_d = static_cast<float *>(softmax_d.data_ptr());
    p.dq = dq.data_ptr(); p.dk = dk.data_ptr(); p.dv = dv.data_ptr();
    const int o = a.varlen ? 0 : 1;  // index of the row stride
#define FA_SET_STRIDES(name, t)                                                                   \
    p.name##_batch_stride = a.varlen ? 0 : (t).stride(0);                                         \
    p.name##_row_stride = (t).stride(o);                                                          \
    p.name##_head_stride = (t).stride(o + 1);
    FA_SET_STRIDES(q, q) FA_SET_STRIDES(k, k) FA_SET_STRIDES(v, v) FA_SET_STRIDES(o, out) FA_SET_STRIDES(do, dout)
    FA_SET_STRIDES(dq, dq) FA_SET_STRIDES(dk, dk) FA_SET_STRIDES(dv, dv)
#undef FA_SET_STRIDES
    if (a.varlen) {
        p.total_q = (int32_t)q.size(0); p.total_k = (int32_t)k.size(0);
        p.h = (int32_t)q.size(1); p.h_k = (int32_t)k.size(1); p.d = (int32_t)q.size(2);
    } else {
        p.h = (int32_t)q.size(2); p.h_k = (int32_t)k.size(2); p.d = (int32_t)q.size(3);
    }
    if (v.size(-1) != q.size(-1)) p.d_v = (int32_t)v.size(-1);  // FA3 headdim_v (ABI v12)
    p.softmax_d_row_len = softmax_d.size(-1);
    p.b = (int32_t)a.batch; p.seqlen_q = (int32_t)a.max_seqlen_q; p.seqlen_k = (int32_t)a.max_seqlen_k;
    p.dtype = dtype_code(q);
    p.cu_seqlens_q = static_cast<const int32_t *>(ptr(a.cu_seqlens_q));
    p.cu_seqlens_k = static_cast<const int32_t *>(ptr(a.cu_seqlens_k));
    p.softmax_scale = (float)a.softmax_scale; p.softcap = (float)a.softcap;
    p.is_causal = a.causal ? 1 : 0;
    p.window_size_left = (int32_t)a.window_left; p.window_size_right = (int32_t)a.window_right;
    if (a.alibi.has_value()) {
        p.alibi_slopes = static_cast<const float *>(a.alibi->data_ptr());
        p.alibi_slopes_batch_stride = a.alibi->dim() == 2 ? a.alibi->stride(0) : 0;
    }
    p.flags = a.fa3_window ? FA_FLAG_FA3_WINDOW : 0;
    p.deterministic = a.deterministic ? 1 : 0;
    p.p_dropout = (float)a.p_dropout;
    p.rng_state = static_cast<const uint64_t *>(ptr(a.rng_state));
    return p;
}

void launch_bwd(const Tensor &dout, const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &out, const Tensor &lse,
                const Tensor &dq, const Tensor &dk, const Tensor &dv, const Tensor &softmax_d, const BwdArgs &a) {
    const fa_bwd_params p = fill_bwd_params(dout, q, k, v, out, lse, dq, dk, dv, softmax_d, a);
    const int st = fa_bwd(&p, current_stream(q));
    TORCH_CHECK(st == 0, "fa_bwd failed (", st, "): ", fa_strerror(st));
}

// What every backward entry point does after its checks: softmax_d (b, h, seqlen_q rounded to 128) or, varlen,
// (h, total_q + 128 b); aligned copies of the views that are not; the launch when `nonempty` (each entry point keeps its
// own empty-input condition), zero gradients otherwise; the copy-back into the caller's gradients.
std::vector<Tensor> run_bwd(const Tensor &dout, const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &out,
                            const Tensor &softmax_lse, const Tensor &dq, const Tensor &dk, const Tensor &dv, const BwdArgs &a,
                            bool nonempty, bool zero_tensors = false) {
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(q.device());
    const int64_t num_heads = q.size(-2);
    Tensor softmax_d = a.varlen ? at::empty({num_heads, q.size(0) + 128 * a.batch}, q.options().dtype(at::kFloat))
                                : at::empty({a.batch, num_heads, round128(a.max_seqlen_q)}, q.options().dtype(at::kFloat));
    if (zero_tensors) { dq.zero_(); dk.zero_(); dv.zero_(); softmax_d.zero_(); }
    if (nonempty) {
        const Tensor doc = aligned_or_copy(dout), qc = aligned_or_copy(q), kc = aligned_or_copy(k), vc = aligned_or_copy(v),
                     oc = aligned_or_copy(out);
        Tensor dqc = aligned(dq) ? dq : at::empty_like(dq, at::MemoryFormat::Contiguous);
        Tensor dkc = aligned(dk) ? dk : at::empty_like(dk, at::MemoryFormat::Contiguous);
        Tensor dvc = aligned(dv) ? dv : at::empty_like(dv, at::MemoryFormat::Contiguous);
        const Tensor lse = softmax_lse.is_contiguous() ? softmax_lse : softmax_lse.contiguous();
        launch_bwd(doc, qc, kc, vc, oc, lse, dqc, dkc, dvc, softmax_d, a);
        if (!dqc.is_same(dq)) dq.copy_(dqc);
        if (!dkc.is_same(dk)) dk.copy_(dkc);
        if (!dvc.is_same(dv)) dv.copy_(dvc);
    } else {
        dq.zero_(); dk.zero_(); dv.zero_(); softmax_d.zero_();  // (:953-958)
    }
    return {dq, dk, dv, softmax_d};
}

void bwd_common_checks(const Tensor &dout, const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &out,
                       const Tensor &softmax_lse) {
    const auto q_dtype = q.scalar_type();
    TORCH_CHECK(q_dtype == at::kHalf || q_dtype == at::kBFloat16, "FlashAttention only support fp16 and bf16 data type");
    TORCH_CHECK(k.scalar_type() == q_dtype, "query and key must have the same dtype");
    TORCH_CHECK(v.scalar_type() == q_dtype, "query and value must have the same dtype");
    TORCH_CHECK(out.scalar_type() == q_dtype, "query and out must have the same dtype");
    TORCH_CHECK(dout.scalar_type() == q_dtype, "query and dout must have the same dtype");
    CHECK_DEVICE(q, "q"); CHECK_DEVICE(k, "k"); CHECK_DEVICE(v, "v"); CHECK_DEVICE(out, "out"); CHECK_DEVICE(dout, "dout");
    CHECK_DEVICE(softmax_lse, "softmax_lse");
    CHECK_LAST_CONTIGUOUS(q, "Input tensor must have contiguous last dimension");
    CHECK_LAST_CONTIGUOUS(k, "Input tensor must have contiguous last dimension");
    CHECK_LAST_CONTIGUOUS(v, "Input tensor must have contiguous last dimension");
    CHECK_LAST_CONTIGUOUS(out, "out tensor must have contiguous last dimension");
    CHECK_LAST_CONTIGUOUS(dout, "dout tensor must have contiguous last dimension");
}

OptTensor bwd_rng_state(double p_dropout, c10::optional<at::Generator> &gen_, OptTensor &rng_state, const Tensor &q) {
    TORCH_CHECK(p_dropout >= 0.0 && p_dropout < 1.0, "p_dropout must be in [0, 1)");
    if (p_dropout <= 0.0) return c10::nullopt;
    // the forward's (seed, offset); without it a fresh pair is drawn like the reference (:895-910)
    Tensor rs = rng_state.has_value() ? rng_state.value() : dropout_state(p_dropout, gen_, q);
    TORCH_CHECK(rs.scalar_type() == at::kLong && rs.numel() == 2 && rs.is_cuda() && rs.is_contiguous(),
                "rng_state must be a contiguous int64 CUDA tensor with 2 elements");
    return rs;
}

// FA3 = true: the window rule of the FA3 surface (fa3_bwd); the bound `bwd` / `varlen_bwd` are the <false> instances
template <bool FA3>
std::vector<Tensor> mha_bwd(const Tensor &dout, const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &out,
                            const Tensor &softmax_lse, OptTensor &dq_, OptTensor &dk_, OptTensor &dv_, OptTensor &alibi_slopes_,
                            const double p_dropout, const double softmax_scale, const bool is_causal, int64_t window_size_left,
                            int64_t window_size_right, const double softcap, const bool deterministic,
                            c10::optional<at::Generator> gen_, OptTensor &rng_state) {
    bwd_common_checks(dout, q, k, v, out, softmax_lse);
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4, "q, k must have 4 dimensions");
    const int64_t batch_size = q.size(0), seqlen_q = q.size(1), num_heads = q.size(2), head_size = q.size(3);
    const int64_t seqlen_k = k.size(1), num_heads_k = k.size(2);
    TORCH_CHECK(batch_size > 0, "batch size must be positive");
    TORCH_CHECK(head_size % 8 == 0, "head_size should be a multiple of 8");
    TORCH_CHECK(head_size <= 256, "FlashAttention backward only supports head dimension at most 256");
    TORCH_CHECK(num_heads % num_heads_k == 0, "Number of heads in key/value must divide number of heads in query");
    if (softcap > 0.0) TORCH_CHECK(p_dropout == 0.0, "Softcapping does not support dropout for now");
    const OptTensor rs = bwd_rng_state(p_dropout, gen_, rng_state, q);
    const OptTensor alibi = check_alibi(alibi_slopes_, batch_size, num_heads);
    CHECK_SHAPE(q, "q", batch_size, seqlen_q, num_heads, head_size);
    CHECK_SHAPE(k, "k", batch_size, seqlen_k, num_heads_k, head_size);
    CHECK_SHAPE(v, "v", batch_size, seqlen_k, num_heads_k, head_size);
    CHECK_SHAPE(out, "out", batch_size, seqlen_q, num_heads, head_size);
    CHECK_SHAPE(dout, "dout", batch_size, seqlen_q, num_heads, head_size);
    Tensor dq = grad_out(dq_, q, "dq", {batch_size, seqlen_q, num_heads, head_size});
    Tensor dk = grad_out(dk_, k, "dk", {batch_size, seqlen_k, num_heads_k, head_size});
    Tensor dv = grad_out(dv_, v, "dv", {batch_size, seqlen_k, num_heads_k, head_size});
    BwdArgs a;
    a.batch = batch_size; a.max_seqlen_q = seqlen_q; a.max_seqlen_k = seqlen_k; a.softmax_scale = softmax_scale;
    a.causal = is_causal; a.window_left = window_size_left; a.window_right = window_size_right; a.softcap = softcap;
    a.alibi = alibi; a.deterministic = deterministic; a.p_dropout = p_dropout; a.rng_state = rs; a.fa3_window = FA3;
    return run_bwd(dout, q, k, v, out, softmax_lse, dq, dk, dv, a, seqlen_q > 0 && seqlen_k > 0);
}

template <bool FA3>
std::vector<Tensor> mha_varlen_bwd(const Tensor &dout, const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &out,
                                   const Tensor &softmax_lse, OptTensor &dq_, OptTensor &dk_, OptTensor &dv_,
                                   const Tensor &cu_seqlens_q, const Tensor &cu_seqlens_k, OptTensor &alibi_slopes_,
                                   const int64_t max_seqlen_q, const int64_t max_seqlen_k, const double p_dropout,
                                   const double softmax_scale, const bool zero_tensors, const bool is_causal,
                                   int64_t window_size_left, int64_t window_size_right, const double softcap,
                                   const bool deterministic, c10::optional<at::Generator> gen_, OptTensor &rng_state) {
    bwd_common_checks(dout, q, k, v, out, softmax_lse);
    TORCH_CHECK(cu_seqlens_q.scalar_type() == at::kInt, "cu_seqlens_q must have dtype int32");
    TORCH_CHECK(cu_seqlens_k.scalar_type() == at::kInt, "cu_seqlens_k must have dtype int32");
    CHECK_DEVICE(cu_seqlens_q, "cu_seqlens_q"); CHECK_DEVICE(cu_seqlens_k, "cu_seqlens_k");
    TORCH_CHECK(cu_seqlens_q.is_contiguous(), "cu_seqlens_q must be contiguous");
    TORCH_CHECK(cu_seqlens_k.is_contiguous(), "cu_seqlens_k must be contiguous");
    TORCH_CHECK(q.dim() == 3 && k.dim() == 3, "q, k must have 3 dimensions");
    const int64_t total_q = q.size(0), num_heads = q.size(1), head_size = q.size(2);
    const int64_t batch_size = cu_seqlens_q.numel() - 1;
    const int64_t total_k = k.size(0), num_heads_k = k.size(1);
    TORCH_CHECK(batch_size > 0, "batch size must be positive");
    TORCH_CHECK(head_size % 8 == 0, "head_size should be a multiple of 8");
    TORCH_CHECK(head_size <= 256, "FlashAttention backward only supports head dimension at most 256");
    TORCH_CHECK(num_heads % num_heads_k == 0, "Number of heads in key/value must divide number of heads in query");
    if (softcap > 0.0) TORCH_CHECK(p_dropout == 0.0, "Softcapping does not support dropout for now");
    const OptTensor rs = bwd_rng_state(p_dropout, gen_, rng_state, q);
    const OptTensor alibi = check_alibi(alibi_slopes_, batch_size, num_heads);
    CHECK_SHAPE(q, "q", total_q, num_heads, head_size);
    CHECK_SHAPE(k, "k", total_k, num_heads_k, head_size);
    CHECK_SHAPE(v, "v", total_k, num_heads_k, head_size);
    CHECK_SHAPE(out, "out", total_q, num_heads, head_size);
    CHECK_SHAPE(dout, "dout", total_q, num_heads, head_size);
    CHECK_SHAPE(cu_seqlens_q, "cu_seqlens_q", batch_size + 1);
    CHECK_SHAPE(cu_seqlens_k, "cu_seqlens_k", batch_size + 1);
    Tensor dq = grad_out(dq_, q, "dq", {total_q, num_heads, head_size});
    Tensor dk = grad_out(dk_, k, "dk", {total_k, num_heads_k, head_size});
    Tensor dv = grad_out(dv_, v, "dv", {total_k, num_heads_k, head_size});
    BwdArgs a;
    a.varlen = true; a.batch = batch_size; a.max_seqlen_q = max_seqlen_q; a.max_seqlen_k = max_seqlen_k;
    a.softmax_scale = softmax_scale; a.causal = is_causal; a.window_left = window_size_left; a.window_right = window_size_right;
    a.softcap = softcap; a.cu_seqlens_q = cu_seqlens_q; a.cu_seqlens_k = cu_seqlens_k; a.alibi = alibi;
    a.deterministic = deterministic; a.p_dropout = p_dropout; a.rng_state = rs; a.fa3_window = FA3;
    return run_bwd(dout, q, k, v, out, softmax_lse, dq, dk, dv, a, max_seqlen_q > 0 && total_q > 0 && total_k > 0, zero_tensors);
}

// ---- the KV-cache host path: what its routes share (the dense step fwd_kvcache_core, the ragged step fwd_kvcache_ragged, the
// fp8 read fwd_kv8, the fp8 append kvcache_append_kv8 and the fp8 step fwd_kv8_step) ----------------------------------------------

// The cache side of one call as check_cache found it: batched (batch_size_c entries of seqlen_k rows, picked by an optional
// batch index) or pages behind a page table (then seqlen_k is the capacity of one sequence's pages and batch_size_c the batch:
// csrc :1266-1268).
struct CacheSide {
    bool paged = false;
    int64_t batch_size_c = 0, seqlen_k = 0, page_block_size = 0, num_heads_k = 0, head_size = 0, head_size_v = 0;
};

// What differs between the routes: the page-size rule, what the kernels need of the cache's memory (base address and
// non-unit strides, in elements' bytes), and the wording of the refusals, which callers know and which therefore stays.
struct CacheRules {
    int64_t page_multiple = 1, base_grain = 16, stride_grain = 8;
    const char *misaligned = "the KV cache must be 16-byte aligned with row/head/batch strides that are multiples of 8";
    std::string k_shape, v_shape;                                    // whole texts
    const char *fill_name = "seqused_k";
    const char *fill_dtype, *fill_device, *fill_contiguous, *fill_shape;  // follow the name of the fill levels
    bool fill_any_dims = false;                                      // the fp8 read only counts the elements
    const char *idx_name = "cache_batch_idx";
    const char *idx_contiguous = " must be contiguous", *idx_length = " must have shape (batch_size)";
    bool idx_longer_ok = false;                                      // the dense 16-bit route serves a longer index today
};

// fill levels (seqlens_k / seqused_q / seqused_k / cache_seqlens): int32, on the device, contiguous, one per sequence
void check_fill_levels(const Tensor &t, const std::string &name, int64_t batch_size, const CacheRules &r) {
    TORCH_CHECK(t.scalar_type() == at::kInt, name, r.fill_dtype);
    TORCH_CHECK(t.is_cuda(), name, r.fill_device);
    TORCH_CHECK(t.is_contiguous(), name, r.fill_contiguous);
    TORCH_CHECK((r.fill_any_dims || t.dim() == 1) && t.numel() == batch_size, name, r.fill_shape);
}

bool cache_aligned(const Tensor &t, int64_t base_grain, int64_t stride_grain) {
    bool ok = reinterpret_cast<uintptr_t>(t.data_ptr()) % base_grain == 0;
    for (int64_t i = 0; i < 3; ++i) ok = ok && t.stride(i) % stride_grain == 0;
    return ok;
}

// Every check of the cache side, once, in one order: the fill levels, paging, the shapes of k and v, leftpad_k, the batch index
// (or an entry per sequence), alignment.  k and v are 4-D (each route says that under its own text first).
CacheSide check_cache(const Tensor &k, const Tensor &v, const OptTensor &page_table, const OptTensor &batch_idx, const OptTensor &fill,
                      const OptTensor &leftpad_k, int64_t batch_size, int64_t head_size, int64_t head_size_v, const CacheRules &r) {
    if (fill.has_value()) check_fill_levels(*fill, r.fill_name, batch_size, r);
    CacheSide c;
    c.paged = page_table.has_value();
    if (c.paged) TORCH_CHECK(!batch_idx.has_value(), "Paged KVcache does not support cache_batch_idx");
    c.batch_size_c = k.size(0); c.seqlen_k = k.size(1); c.num_heads_k = k.size(2); c.head_size = head_size; c.head_size_v = head_size_v;
    if (c.paged) {
        const auto pr = check_block_table(*page_table, k, batch_size, r.page_multiple);
        c.page_block_size = pr.first;
        c.seqlen_k = pr.second * pr.first; c.batch_size_c = batch_size;
    }
    TORCH_CHECK(k.size(3) == head_size, r.k_shape);
    TORCH_CHECK(v.sizes() == c10::IntArrayRef({k.size(0), k.size(1), k.size(2), head_size_v}), r.v_shape);
    check_leftpad(leftpad_k, batch_size, c.paged);
    if (batch_idx.has_value()) {
        TORCH_CHECK(batch_idx->is_cuda(), r.idx_name, " must be on CUDA");
        TORCH_CHECK(batch_idx->is_contiguous(), r.idx_name, r.idx_contiguous);
        TORCH_CHECK(batch_idx->scalar_type() == at::kInt, r.idx_name, " must have dtype int32");
        TORCH_CHECK(batch_idx->numel() == batch_size || (r.idx_longer_ok && batch_idx->numel() > batch_size), r.idx_name, r.idx_length);
    } else {
        TORCH_CHECK(c.batch_size_c >= batch_size, "the KV cache must have at least batch_size entries");
    }
    TORCH_CHECK(cache_aligned(k, r.base_grain, r.stride_grain) && cache_aligned(v, r.base_grain, r.stride_grain), r.misaligned);
    return c;
}

// New rows beside cu_seqlens_k_new (ragged, (total_k_new, h_k, d)) or without (dense, (b, s_new, h_k, d)); hopper :929-975.
// `size_of_k_new`: how the route's text spells k_new's own extent ("k_new->size" / "k_new.size"); `v_dim`: its name of V's width.
void check_new_rows(const Tensor &k_new, const Tensor &v_new, const OptTensor &cu_seqlens_k_new, int64_t batch_size, int64_t num_heads_k,
                    int64_t head_size, int64_t head_size_v, const char *size_of_k_new, const char *v_dim) {
    if (cu_seqlens_k_new.has_value()) {
        CHECK_DEVICE(*cu_seqlens_k_new, "cu_seqlens_k_new");
        TORCH_CHECK(cu_seqlens_k_new->is_contiguous(), "cu_seqlens_k_new must be contiguous");
        TORCH_CHECK(cu_seqlens_k_new->scalar_type() == at::kInt, "cu_seqlens_k_new must have dtype torch.int32");  // :939
        TORCH_CHECK(k_new.dim() == 3, "k_new must have shape (total_k_new, num_heads_k, head_size) with cu_seqlens_k_new");
        TORCH_CHECK(k_new.sizes() == c10::IntArrayRef({k_new.size(0), num_heads_k, head_size}), "k_new must have shape (", size_of_k_new,
                    "(0), num_heads_k, head_size)");
        TORCH_CHECK(v_new.sizes() == c10::IntArrayRef({k_new.size(0), num_heads_k, head_size_v}), "v_new must have shape (", size_of_k_new,
                    "(0), num_heads_k, ", v_dim, ")");
        CHECK_SHAPE(*cu_seqlens_k_new, "cu_seqlens_k_new", batch_size + 1);
    } else {
        TORCH_CHECK(k_new.dim() == 4, "k_new must have shape (batch_size, seqlen_k_new, num_heads_k, head_size) without cu_seqlens_k_new");
        TORCH_CHECK(k_new.sizes() == c10::IntArrayRef({batch_size, k_new.size(1), num_heads_k, head_size}), "k_new must have shape (batch_size, ",
                    size_of_k_new, "(1), num_heads_k, head_size)");
        TORCH_CHECK(v_new.sizes() == c10::IntArrayRef({batch_size, k_new.size(1), num_heads_k, head_size_v}), "v_new must have shape (batch_size, ",
                    size_of_k_new, "(1), num_heads_k, ", v_dim, ")");
    }
}

// rotary_cos / rotary_sin (seqlen_ro, rotary_dim / 2) against the head dim, the cache's capacity and the dtype of `like` (the
// tensor they rotate: "query", "k_new"); hopper :1050-1072.  per_tensor: the reference's texts (csrc :1404-1428), which name one
// table each -- and rotary_cos for the dtype of either.
void check_rotary_tables(const Tensor &cos, const Tensor &sin, int64_t head_size, int64_t capacity, at::ScalarType dtype, const char *like,
                         bool per_tensor = false) {
    const auto text = [&](const char *table, const char *rule) { return std::string(per_tensor ? table : "rotary_cos / rotary_sin") + rule; };
    CHECK_DEVICE(cos, "rotary_cos"); CHECK_DEVICE(sin, "rotary_sin");
    TORCH_CHECK(cos.dim() == 2, text("rotary_cos", " must have shape (seqlen_ro, rotary_dim / 2)"));
    TORCH_CHECK(sin.sizes() == cos.sizes(), text("rotary_sin", " must have shape (seqlen_ro, rotary_dim / 2)"));
    const int64_t rotary_dim = cos.size(1) * 2;
    TORCH_CHECK(rotary_dim <= head_size, "rotary_dim must be <= headdim");
    TORCH_CHECK(rotary_dim % 16 == 0, "Only rotary dimensions divisible by 16 are currently supported");
    TORCH_CHECK(cos.size(0) >= capacity, "cos/sin seqlen must be at least the seqlen of KV cache");
    TORCH_CHECK(cos.is_contiguous(), text("rotary_cos", " must be contiguous"));
    TORCH_CHECK(sin.is_contiguous(), text("rotary_sin", " must be contiguous"));
    TORCH_CHECK(cos.scalar_type() == dtype && sin.scalar_type() == dtype, text("rotary_cos", " must have the same dtype as "), like);
}

// What the three append structs (fa_kvcache_append_params, fa_kvcache_append_varlen_params, fa_kvcache_append_kv8_params) name
// alike: the cache and its strides, the paging fields, the fill levels, the batch index and the rotary group.
template <class P>
void fill_append_common(P &p, const Tensor &k_cache, const Tensor &v_cache, const Tensor &cache_seqlens, const OptTensor &cache_batch_idx,
                        const OptTensor &block_table, const OptTensor &rotary_cos, const OptTensor &rotary_sin, bool rotary_interleaved,
                        const OptTensor &rotary_seqlens) {
    p.abi_version = FA_ABI_VERSION;
    p.struct_size = sizeof(P);
    p.k_cache = k_cache.data_ptr(); p.v_cache = v_cache.data_ptr();
    p.kcache_batch_stride = k_cache.stride(0); p.kcache_row_stride = k_cache.stride(1); p.kcache_head_stride = k_cache.stride(2);
    p.vcache_batch_stride = v_cache.stride(0); p.vcache_row_stride = v_cache.stride(1); p.vcache_head_stride = v_cache.stride(2);
    p.seqlen_cache = (int32_t)k_cache.size(1);
    if (block_table.has_value()) {
        p.block_table = static_cast<const int32_t *>(block_table->data_ptr());
        p.block_table_batch_stride = block_table->stride(0);
        p.page_block_size = (int32_t)k_cache.size(1);
        p.seqlen_cache = (int32_t)(block_table->size(1) * k_cache.size(1));
    }
    p.cache_seqlens = static_cast<const int32_t *>(cache_seqlens.data_ptr());
    p.cache_batch_idx = static_cast<const int32_t *>(ptr(cache_batch_idx));
    if (rotary_cos.has_value()) {
        p.rotary_cos = rotary_cos->data_ptr(); p.rotary_sin = rotary_sin->data_ptr();
        p.rotary_dim = (int32_t)rotary_cos->size(1) * 2;
        p.rotary_interleaved = rotary_interleaved ? 1 : 0;
        p.rotary_seqlens = static_cast<const int32_t *>(ptr(rotary_seqlens));   // FA3 seqlens_rotary (NULL: the cache fill levels)
    }
}

void kvcache_append(const Tensor &k_new, const Tensor &v_new, const Tensor &k_cache, const Tensor &v_cache,
                    const Tensor &cache_seqlens, const OptTensor &cache_batch_idx, const OptTensor &block_table,
                    const OptTensor &rotary_cos, const OptTensor &rotary_sin, bool rotary_interleaved,
                    const OptTensor &rotary_seqlens) {
    fa_kvcache_append_params p{};
    fill_append_common(p, k_cache, v_cache, cache_seqlens, cache_batch_idx, block_table, rotary_cos, rotary_sin, rotary_interleaved,
                       rotary_seqlens);
    p.k_new = k_new.data_ptr(); p.v_new = v_new.data_ptr();
    p.knew_batch_stride = k_new.stride(0); p.knew_row_stride = k_new.stride(1); p.knew_head_stride = k_new.stride(2);
    p.vnew_batch_stride = v_new.stride(0); p.vnew_row_stride = v_new.stride(1); p.vnew_head_stride = v_new.stride(2);
    p.b = (int32_t)k_new.size(0); p.seqlen_new = (int32_t)k_new.size(1); p.h_k = (int32_t)k_new.size(2); p.d = (int32_t)k_new.size(3);
    if (v_cache.size(3) != k_cache.size(3)) p.d_v = (int32_t)v_cache.size(3);  // V rows of their own width (ABI v13)
    p.dtype = dtype_code(k_new);
    const int st = fa_kvcache_append(&p, current_stream(k_new));
    TORCH_CHECK(st == 0, "fa_kvcache_append failed (", st, "): ", fa_strerror(st));
}

void kvcache_append_varlen(const Tensor &k_new, const Tensor &v_new, const Tensor &cu_seqlens_k_new, const Tensor &k_cache,
                           const Tensor &v_cache, const Tensor &cache_seqlens, const Tensor &seqused_out,
                           const OptTensor &cache_batch_idx, const OptTensor &block_table, const OptTensor &rotary_cos,
                           const OptTensor &rotary_sin, bool rotary_interleaved, const OptTensor &rotary_seqlens) {
    fa_kvcache_append_varlen_params p{};
    fill_append_common(p, k_cache, v_cache, cache_seqlens, cache_batch_idx, block_table, rotary_cos, rotary_sin, rotary_interleaved,
                       rotary_seqlens);
    p.k_new = k_new.data_ptr(); p.v_new = v_new.data_ptr();
    p.knew_row_stride = k_new.stride(0); p.knew_head_stride = k_new.stride(1);
    p.vnew_row_stride = v_new.stride(0); p.vnew_head_stride = v_new.stride(1);
    p.b = (int32_t)cache_seqlens.numel(); p.total_k_new = (int32_t)k_new.size(0); p.h_k = (int32_t)k_new.size(1);
    p.d = (int32_t)k_new.size(2);
    p.max_seqlen_k_new = 0;  // (the FA3 call carries no bound of the new lengths, hopper/flash_api.cpp:948: the launch searches)
    if (v_cache.size(3) != k_cache.size(3)) p.d_v = (int32_t)v_cache.size(3);
    p.cu_seqlens_k_new = static_cast<const int32_t *>(cu_seqlens_k_new.data_ptr());
    p.seqused_out = static_cast<int32_t *>(seqused_out.data_ptr());
    p.dtype = dtype_code(k_new);
    const int st = fa_kvcache_append_varlen(&p, current_stream(k_new));
    TORCH_CHECK(st == 0, "fa_kvcache_append_varlen failed (", st, "): ", fa_strerror(st));
}

// what fa_rotary_params and fa_rotary_varlen_params name alike
template <class P>
void fill_rotary_common(P &p, const Tensor &src, const Tensor &dst, const Tensor &cos, const Tensor &sin, bool interleaved, bool per_row) {
    p.abi_version = FA_ABI_VERSION;
    p.struct_size = sizeof(P);
    p.src = src.data_ptr(); p.dst = dst.data_ptr();
    p.dtype = dtype_code(src);
    p.rotary_dim = (int32_t)cos.size(1) * 2;
    p.rotary_interleaved = interleaved ? 1 : 0;
    p.per_row_positions = per_row ? 1 : 0;
    p.rotary_cos = cos.data_ptr(); p.rotary_sin = sin.data_ptr();
}

// q rotated for this step, as a copy: dense (b, s, h, d), or ragged (total_q, h, d) with cu_seqlens_q.  Positions: causal / local ->
// row i of a sequence sits at its offset + i, otherwise every row at the offset (flash_attn/flash_attn_interface.py:1516-1524,
// src/flash_fwd_kernel.h:753-775); the offset is seqlens_rotary where given, else the fill level in front of the append.
Tensor rotate_q(const Tensor &q, const OptTensor &cu_seqlens_q, int64_t max_seqlen_q, const Tensor &cos, const Tensor &sin,
                const OptTensor &seqlens_rotary, const Tensor &fill, bool interleaved, bool is_causal, int64_t window_size_left,
                int64_t window_size_right) {
    const bool per_row = is_causal || window_size_left >= 0 || window_size_right >= 0;
    const Tensor &offsets = seqlens_rotary.has_value() ? *seqlens_rotary : fill;
    Tensor dst = at::empty_like(q, at::MemoryFormat::Contiguous);
    if (cu_seqlens_q.has_value()) {
        fa_rotary_varlen_params p{};
        fill_rotary_common(p, q, dst, cos, sin, interleaved, per_row);
        p.src_row_stride = q.stride(0); p.src_head_stride = q.stride(1);
        p.dst_row_stride = dst.stride(0); p.dst_head_stride = dst.stride(1);
        p.b = (int32_t)offsets.numel(); p.total_q = (int32_t)q.size(0); p.max_seqlen_q = (int32_t)max_seqlen_q;
        p.h = (int32_t)q.size(1); p.d = (int32_t)q.size(2);
        p.cu_seqlens_q = static_cast<const int32_t *>(cu_seqlens_q->data_ptr());
        p.offsets = static_cast<const int32_t *>(offsets.data_ptr());
        const int st = fa_rotary_apply_varlen(&p, current_stream(q));
        TORCH_CHECK(st == 0, "fa_rotary_apply_varlen failed (", st, "): ", fa_strerror(st));
    } else {
        fa_rotary_params p{};
        fill_rotary_common(p, q, dst, cos, sin, interleaved, per_row);
        p.src_batch_stride = q.stride(0); p.src_row_stride = q.stride(1); p.src_head_stride = q.stride(2);
        p.dst_batch_stride = dst.stride(0); p.dst_row_stride = dst.stride(1); p.dst_head_stride = dst.stride(2);
        p.b = (int32_t)q.size(0); p.s = (int32_t)q.size(1); p.h = (int32_t)q.size(2); p.d = (int32_t)q.size(3);
        p.seqlen_offsets = static_cast<const int32_t *>(offsets.data_ptr());
        const int st = fa_rotary_apply(&p, current_stream(q));
        TORCH_CHECK(st == 0, "fa_rotary_apply failed (", st, "): ", fa_strerror(st));
    }
    return dst;
}

// The arguments of the dense cache step beside q and the cache; what a caller leaves unset is not passed.
struct KvcacheArgs {
    OptTensor k_new, v_new, seqlens_k, rotary_cos, rotary_sin, cache_batch_idx, leftpad_k, block_table, alibi_slopes, out;
    double softmax_scale = 1.0, softcap = 0.0;
    bool is_causal = false, is_rotary_interleaved = false;
    int64_t window_size_left = -1, window_size_right = -1, num_splits = 0;
    int64_t page_multiple = 1;  // the page-size rule of the calling surface: FA2 256, FA3 any
    OptTensor seqlens_rotary, qv;  // FA3
    OptTensor sink;  // the cute surface's learnable sink, (num_heads,) -- checked by its caller; no other surface passes one
    bool pack_gqa = false;
};

// mha_fwd_kvcache, csrc/flash_attn/flash_api.cpp:1202-1476
std::vector<Tensor> fwd_kvcache_core(Tensor q, const Tensor &kcache, const Tensor &vcache, const KvcacheArgs &args) {
    const OptTensor &k_ = args.k_new, &v_ = args.v_new, &seqlens_k_ = args.seqlens_k, &rotary_cos_ = args.rotary_cos,
                    &rotary_sin_ = args.rotary_sin, &cache_batch_idx_ = args.cache_batch_idx, &leftpad_k_ = args.leftpad_k,
                    &block_table_ = args.block_table, &out_ = args.out, &seqlens_rotary_ = args.seqlens_rotary, &qv_ = args.qv,
                    &sink_ = args.sink;
    bool is_causal = args.is_causal;
    const int64_t window_size_left = args.window_size_left;
    int64_t window_size_right = args.window_size_right;
    const auto q_dtype = q.scalar_type();
    TORCH_CHECK(q_dtype == at::kHalf || q_dtype == at::kBFloat16, "FlashAttention only support fp16 and bf16 data type");
    TORCH_CHECK(kcache.scalar_type() == q_dtype, "query and key must have the same dtype");
    TORCH_CHECK(vcache.scalar_type() == q_dtype, "query and value must have the same dtype");
    CHECK_DEVICE(q, "q"); CHECK_DEVICE(kcache, "kcache"); CHECK_DEVICE(vcache, "vcache");
    CHECK_LAST_CONTIGUOUS(q, "Input tensor must have contiguous last dimension");
    CHECK_LAST_CONTIGUOUS(kcache, "Input tensor must have contiguous last dimension");
    CHECK_LAST_CONTIGUOUS(vcache, "Input tensor must have contiguous last dimension");
    TORCH_CHECK(q.dim() == 4 && kcache.dim() == 4, "q, kcache must have 4 dimensions");
    const int64_t batch_size = q.size(0), head_size_og = q.size(3);
    int64_t seqlen_q = q.size(1), num_heads = q.size(2);
    const int64_t num_heads_k = kcache.size(2);
    // FA3: V head dim of its own for q/k <= 64 beside v in [256, 512] (MLA: the qv kernel), hopper/flash_api.cpp:783-792
    const int64_t head_size_v = vcache.dim() == 4 ? vcache.size(3) : head_size_og;
    const bool wide_v = head_size_og <= 64 && head_size_v >= 256 && head_size_v <= 512 && head_size_v % 8 == 0;
    TORCH_CHECK(head_size_v == head_size_og || wide_v,
                "If V headdim is different from Q/K dim, this KV-cache path only supports Q/K <= 64 and V in [256, 512]");
    if (qv_.has_value()) {  // hopper/flash_api.cpp:1028-1048
        TORCH_CHECK(wide_v, "This flash attention build does not support qv here: q_v is only supported for head_size <= 64 and "
                            "hdim_v >= 256 (<= 512)");
        TORCH_CHECK(qv_->scalar_type() == q_dtype, "q_v must have the same dtype as query");
        CHECK_DEVICE(*qv_, "q_v");
        TORCH_CHECK(qv_->get_device() == q.get_device(), "q_v must be on the same device as query");
        CHECK_LAST_CONTIGUOUS(*qv_, "q_v tensor must have contiguous last dimension");
        CHECK_SHAPE(*qv_, "q_v", q.size(0), q.size(1), q.size(2), head_size_v);
    }
    TORCH_CHECK(batch_size > 0, "batch size must be positive");
    TORCH_CHECK(head_size_og <= 256, "FlashAttention forward only supports head dimension at most 256");
    TORCH_CHECK(head_size_og % 8 == 0, "This flash attention build needs head_size to be a multiple of 8 in fwd_kvcache");
    TORCH_CHECK(num_heads % num_heads_k == 0, "Number of heads in key/value must divide number of heads in query");
    CacheRules rules;  // (the reference's texts: its CHECK_SHAPE prints the expression it compares with)
    rules.page_multiple = args.page_multiple;
    const std::string rows = block_table_.has_value() ? "(kcache.size(0), page_block_size, num_heads_k, " : "(batch_size_c, seqlen_k, num_heads_k, ";
    rules.k_shape = "kcache must have shape " + rows + "head_size_og)"; rules.v_shape = "vcache must have shape " + rows + "head_size_v)";
    rules.fill_name = "seqlens_k"; rules.fill_dtype = " must have dtype int32"; rules.fill_device = " must be on CUDA";
    rules.fill_contiguous = " must be contiguous"; rules.fill_shape = " must have shape (batch_size)";
    rules.idx_longer_ok = true;
    const CacheSide cache = check_cache(kcache, vcache, block_table_, cache_batch_idx_, seqlens_k_, leftpad_k_, batch_size, head_size_og,
                                        head_size_v, rules);
    const int64_t seqlen_k = cache.seqlen_k;
    const OptTensor alibi = check_alibi(args.alibi_slopes, batch_size, num_heads);
    if (seqlen_q == 1 && !alibi.has_value()) is_causal = false;  // (:1270)
    if (is_causal) window_size_right = 0;
    // (b, 1, (h_k ngroups), d) -> (b, ngroups, h_k, d): one pass over the cache serves the whole GQA group (:1272-1285)
    // (not with qv: the qv kernel packs the GQA group into its rows itself, for any seqlen_q)
    const bool swapped = seqlen_q == 1 && num_heads > num_heads_k && window_size_left < 0 && window_size_right < 0 && !alibi.has_value() &&
                         !qv_.has_value();
    if (swapped) {
        const int64_t ngroups = num_heads / num_heads_k;
        q = q.reshape({batch_size, num_heads_k, ngroups, head_size_og}).transpose(1, 2);
        seqlen_q = ngroups; num_heads = num_heads_k;
    }
    CHECK_SHAPE(q, "q", batch_size, seqlen_q, num_heads, head_size_og);
    Tensor out;
    if (out_.has_value() && !swapped) {
        out = out_.value();
        TORCH_CHECK(out.scalar_type() == q_dtype, "Output must have the same dtype as inputs");
        CHECK_DEVICE(out, "out");
        TORCH_CHECK(out.stride(-1) == 1, "Output tensor must have contiguous last dimension");
        CHECK_SHAPE(out, "out", batch_size, seqlen_q, num_heads, head_size_v);
    } else {
        out = at::empty({batch_size, seqlen_q, num_heads, head_size_v}, q.options());
    }
    int64_t seqlen_knew = 0;
    if (k_.has_value()) {
        TORCH_CHECK(v_.has_value(), "If key is supplied, value must also be passed in");
        TORCH_CHECK(seqlens_k_.has_value(), "If key is supplied, seqlens_k must also be passed in");
        TORCH_CHECK(seqlen_q <= seqlen_k, "If key is supplied, it must have seqlen <= the seqlen of the KV cache");
        TORCH_CHECK(k_->scalar_type() == q_dtype, "Key must have the same dtype as query");
        TORCH_CHECK(v_->scalar_type() == q_dtype, "Value must have the same dtype as query");
        CHECK_DEVICE(*k_, "k"); CHECK_DEVICE(*v_, "v");
        TORCH_CHECK(k_->stride(-1) == 1, "Key tensor must have contiguous last dimension");
        TORCH_CHECK(v_->stride(-1) == 1, "Value tensor must have contiguous last dimension");
        seqlen_knew = k_->size(1);
        CHECK_SHAPE(*k_, "k", batch_size, seqlen_knew, num_heads_k, head_size_og);
        CHECK_SHAPE(*v_, "v", batch_size, seqlen_knew, num_heads_k, head_size_v);
    }
    const bool rotary = rotary_cos_.has_value();
    if (rotary) {
        TORCH_CHECK(k_.has_value(), "If rotary cos/sin are provided, new key / value to be appended to KV cache must also be provided");
        TORCH_CHECK(rotary_sin_.has_value(), "If rotary cos is provided, rotary sin must also be provided");
        check_rotary_tables(*rotary_cos_, *rotary_sin_, head_size_og, seqlen_k, q_dtype, "query", /*per_tensor=*/true);
    }
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(q.device());
    Tensor softmax_lse = at::empty({batch_size, num_heads, seqlen_q}, q.options().dtype(at::kFloat));
    OptTensor seqused = seqlens_k_;
    if (seqlen_knew > 0) {  // "Append_KV": new rows land at [seqlens_k, seqlens_k + seqlen_knew) of each cache entry
        const Tensor kn = aligned_or_copy(*k_), vn = aligned_or_copy(*v_);
        kvcache_append(kn, vn, kcache, vcache, *seqlens_k_, cache_batch_idx_, block_table_, rotary_cos_, rotary_sin_,
                       args.is_rotary_interleaved, seqlens_rotary_);
        seqused = *seqlens_k_ + seqlen_knew;
    }
    Tensor qc = aligned_or_copy(q);
    if (rotary)
        qc = rotate_q(qc, c10::nullopt, 0, *rotary_cos_, *rotary_sin_, seqlens_rotary_, *seqlens_k_, args.is_rotary_interleaved, is_causal,
                      window_size_left, window_size_right);
    if (seqlen_k > 0) {
        const OutPath o(out);
        FwdArgs a;
        a.batch = batch_size; a.max_seqlen_q = seqlen_q; a.max_seqlen_k = seqlen_k; a.softmax_scale = args.softmax_scale;
        a.causal = is_causal; a.window_left = window_size_left; a.window_right = window_size_right; a.softcap = args.softcap;
        a.seqused_k = seqused; a.alibi = alibi; a.kv_batch_idx = cache_batch_idx_; a.block_table = block_table_;
        a.num_splits = (int)args.num_splits; a.leftpad_k = leftpad_k_;
        a.pack_gqa = args.pack_gqa;  // (behind the single-token GQA swap h == h_k: the hint has nothing to pack there)
        if (qv_.has_value()) a.qv = aligned_or_copy(*qv_);
        if (sink_.has_value()) {
            a.sink = sink_;
            if (swapped) {  // kernel head g, row r = query head g * ngroups + r
                a.sink_head_stride = (int)seqlen_q; a.sink_row_stride = 1;
            }
        }
        launch_fwd(qc, kcache, vcache, o.work, softmax_lse, a);
        o.finish();
    } else {  // (swapped: the heads lie along (h_k, ngroups))
        fill_empty(out, softmax_lse, sink_, {1, num_heads, swapped ? seqlen_q : 1});
    }
    if (swapped) {
        out = out.transpose(1, 2).reshape({batch_size, 1, num_heads_k * seqlen_q, head_size_v});
        softmax_lse = softmax_lse.reshape({batch_size, num_heads_k * seqlen_q, 1});
        if (out_.has_value()) {
            out_->copy_(out);
            out = out_.value();
        }
    }
    return {out, softmax_lse};
}

std::vector<Tensor> mha_fwd_kvcache(Tensor &q, const Tensor &kcache, const Tensor &vcache, OptTensor &k_, OptTensor &v_,
                                    OptTensor &seqlens_k_, OptTensor &rotary_cos_, OptTensor &rotary_sin_,
                                    OptTensor &cache_batch_idx_, OptTensor &leftpad_k_, OptTensor &block_table_,
                                    OptTensor &alibi_slopes_, OptTensor &out_, const double softmax_scale, bool is_causal,
                                    int64_t window_size_left, int64_t window_size_right, const double softcap,
                                    bool is_rotary_interleaved, int64_t num_splits) {
    // (the FA2 surface keeps one head dim for q, k and v: a V of its own width is an FA3 argument)
    if (vcache.dim() == 4 && kcache.dim() == 4 && vcache.size(3) != kcache.size(3))
        TORCH_CHECK(false, block_table_.has_value() ? "vcache must have shape (kcache.size(0), page_block_size, num_heads_k, head_size_og)"
                                                    : "vcache must have shape (batch_size_c, seqlen_k, num_heads_k, head_size_og)");
    KvcacheArgs a;
    a.k_new = k_; a.v_new = v_; a.seqlens_k = seqlens_k_; a.rotary_cos = rotary_cos_; a.rotary_sin = rotary_sin_;
    a.cache_batch_idx = cache_batch_idx_; a.leftpad_k = leftpad_k_; a.block_table = block_table_; a.alibi_slopes = alibi_slopes_;
    a.out = out_; a.softmax_scale = softmax_scale; a.is_causal = is_causal; a.window_size_left = window_size_left;
    a.window_size_right = window_size_right; a.softcap = softcap; a.is_rotary_interleaved = is_rotary_interleaved;
    a.num_splits = num_splits;
    a.page_multiple = 256;  // the reference's page rule (:1265)
    return fwd_kvcache_core(q, kcache, vcache, a);
}

// a shape as Python prints a tuple: "(2, 128, 8, 512)", "(7,)"
std::string tuple_str(c10::IntArrayRef s) {
    std::string r = "(";
    for (size_t i = 0; i < s.size(); ++i) r += (i ? ", " : "") + std::to_string(s[i]);
    return r + (s.size() == 1 ? ",)" : ")");
}

// window normalisation of the FA3 entry points (hopper/flash_api.cpp:796-797, 1360-1361): a side that cannot mask anything
// becomes -1 = unbounded and stays unbounded (FA_FLAG_FA3_WINDOW)
void fa3_window(int64_t seqlen_q, int64_t seqlen_k, int64_t &left, int64_t &right) {
    if (left >= seqlen_k - 1) left = -1;
    if (right >= seqlen_q - 1) right = -1;
}

// seqlens_rotary (hopper/flash_api.cpp:1074-1079): the rotary positions where they are not the cache fill levels
void check_seqlens_rotary(const Tensor &t, int64_t batch_size) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous(), "seqlens_rotary must be a contiguous CUDA tensor");
    TORCH_CHECK(t.scalar_type() == at::kInt, "seqlens_rotary must have dtype torch.int32");
    TORCH_CHECK(t.sizes() == c10::IntArrayRef({batch_size}), "seqlens_rotary must have shape (batch_size,)");
}

// One continuous-batching step over a KV cache (flash_attn_with_kvcache(..., cu_seqlens_q=, cu_seqlens_k_new=, max_seqlen_q=),
// hopper/flash_api.cpp:736-760, 929-975): q is ragged (total_q, h, d) with cu_seqlens_q, k / v the batched or paged cache with
// its fill levels in seqused_k, the new keys / values dense (b, s_new, h_k, .) or ragged with cu_seqlens_k_new.  The append
// (fa_kvcache_append_varlen writes the new fill levels on the device) and the rotary pass of q run in front of one fa_fwd
// on the ragged-queries-over-a-cache form; nothing here reads device data, so the step can be captured in a graph.
// max_seqlen_q == 1 with total_q == batch_size is, by shapes alone, one query row per sequence: q is viewed as (b, 1, h, d)
// and the step takes the dense decode route (its GQA swap and split heuristic), the results viewed back to the ragged shapes.
std::tuple<Tensor, Tensor> fwd_kvcache_ragged(const Tensor &q, const Tensor &kcache, const Tensor &vcache, const OptTensor &k_new,
                                              const OptTensor &v_new, const OptTensor &qv, const OptTensor &out_,
                                              const Tensor &cu_seqlens_q, const OptTensor &cu_seqlens_k_new,
                                              const OptTensor &seqused_q, const OptTensor &seqused_k, int64_t max_seqlen_q,
                                              const OptTensor &page_table, const OptTensor &kv_batch_idx, const OptTensor &leftpad_k,
                                              const OptTensor &rotary_cos, const OptTensor &rotary_sin, const OptTensor &seqlens_rotary,
                                              double softmax_scale, bool is_causal, int64_t window_size_left,
                                              int64_t window_size_right, double softcap, bool is_rotary_interleaved, int64_t num_splits,
                                              const OptTensor &sink = c10::nullopt, bool pack_gqa = false) {
    const auto q_dtype = q.scalar_type();
    CHECK_DEVICE(cu_seqlens_q, "cu_seqlens_q");
    TORCH_CHECK(cu_seqlens_q.is_contiguous(), "cu_seqlens_q must be contiguous");
    TORCH_CHECK(cu_seqlens_q.scalar_type() == at::kInt, "cu_seqlens_q must have dtype torch.int32");  // :744
    TORCH_CHECK(max_seqlen_q >= 0, "max_seqlen_q must be provided if cu_seqlens_q is provided");      // :745
    TORCH_CHECK(q.dim() == 3, "q must have shape (total_q, num_heads, head_size)");
    TORCH_CHECK(seqused_k.has_value(), "seqused_k must be provided for a KV-cache call with cu_seqlens_q");
    TORCH_CHECK(kcache.dim() == 4 && vcache.dim() == 4, "kcache, vcache must have 4 dimensions");
    const int64_t total_q = q.size(0), num_heads = q.size(1), head_size = q.size(2);
    const int64_t batch_size = cu_seqlens_q.numel() - 1;
    const int64_t num_heads_k = kcache.size(2), head_size_v = vcache.size(3);
    TORCH_CHECK(batch_size > 0, "batch size must be positive");
    TORCH_CHECK(head_size <= 256, "FlashAttention forward only supports head dimension at most 256");
    TORCH_CHECK(head_size % 8 == 0, "head_size should be a multiple of 8");
    TORCH_CHECK(num_heads_k > 0 && num_heads % num_heads_k == 0, "Number of heads in key/value must divide number of heads in query");
    CacheRules rules;  // (user-visible legacy texts: "pr.first" was the page size in the expression an older CHECK_SHAPE printed)
    const std::string rows = page_table.has_value() ? "(kcache.size(0), pr.first, num_heads_k, " : "(batch_size_c, seqlen_k, num_heads_k, ";
    rules.k_shape = "kcache must have shape " + rows + "head_size)"; rules.v_shape = "vcache must have shape " + rows + "head_size_v)";
    rules.fill_dtype = " must have dtype int32";  // :830, :836
    rules.fill_device = rules.fill_contiguous = rules.fill_shape = " must be a contiguous CUDA tensor of shape (batch_size,)";
    rules.idx_name = "kv_batch_idx";  // :1088
    if (seqused_q.has_value()) check_fill_levels(*seqused_q, "seqused_q", batch_size, rules);
    const CacheSide cache = check_cache(kcache, vcache, page_table, kv_batch_idx, seqused_k, leftpad_k, batch_size, head_size, head_size_v, rules);
    const int64_t seqlen_k = cache.seqlen_k;
    const bool ragged_new = cu_seqlens_k_new.has_value();
    if (k_new.has_value()) {  // :929-975
        TORCH_CHECK(k_new->scalar_type() == q_dtype, "k_new must have the same dtype as query");
        TORCH_CHECK(v_new->scalar_type() == q_dtype, "v_new must have the same dtype as query");
        CHECK_DEVICE(*k_new, "k_new"); CHECK_DEVICE(*v_new, "v_new");
        TORCH_CHECK(k_new->stride(-1) == 1, "k_new tensor must have contiguous last dimension");
        TORCH_CHECK(v_new->stride(-1) == 1, "v_new tensor must have contiguous last dimension");
        check_new_rows(*k_new, *v_new, cu_seqlens_k_new, batch_size, num_heads_k, head_size, head_size_v, "k_new->size", "head_size_v");
    } else {
        TORCH_CHECK(!ragged_new, "cu_seqlens_k_new needs k_new and v_new");
    }
    const bool rotary = rotary_cos.has_value();
    if (rotary) {
        TORCH_CHECK(k_new.has_value(), "If rotary cos/sin are provided, new key / value to be appended to KV cache must also be provided");
        check_rotary_tables(*rotary_cos, *rotary_sin, head_size, seqlen_k, q_dtype, "query");
    }
    std::vector<int64_t> out_shape = {total_q, num_heads, head_size_v};
    if (out_.has_value()) {
        TORCH_CHECK(out_->scalar_type() == q_dtype, "Output must have the same dtype as inputs");
        TORCH_CHECK(out_->is_cuda() && out_->stride(-1) == 1 && out_->sizes() == c10::IntArrayRef(out_shape),
                    "out must have shape (..., num_heads, head_size_v)");
    }
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(q.device());
    const auto int_opts = q.options().dtype(at::kInt);

    // ---- the append: new fill levels stay on the device
    Tensor seqused = *seqused_k;
    bool appended = false;
    const bool single_token = max_seqlen_q == 1 && total_q == batch_size && !seqused_q.has_value();
    if (k_new.has_value() && ragged_new) {
        const Tensor kn = aligned_or_copy(*k_new), vn = aligned_or_copy(*v_new);
        seqused = at::empty({batch_size}, int_opts);
        kvcache_append_varlen(kn, vn, *cu_seqlens_k_new, kcache, vcache, *seqused_k, seqused, kv_batch_idx, page_table, rotary_cos,
                              rotary_sin, is_rotary_interleaved, seqlens_rotary);
        appended = true;
    } else if (k_new.has_value() && !single_token && k_new->size(1) > 0) {
        const Tensor kn = aligned_or_copy(*k_new), vn = aligned_or_copy(*v_new);
        kvcache_append(kn, vn, kcache, vcache, *seqused_k, kv_batch_idx, page_table, rotary_cos, rotary_sin, is_rotary_interleaved,
                       seqlens_rotary);
        seqused = *seqused_k + k_new->size(1);
        appended = true;
    }
    // one row per sequence: the dense decode route on q viewed as (b, 1, h, d), its results viewed back.  `decode`: what both uses pass
    KvcacheArgs decode;
    if (single_token) {
        if (out_.has_value()) decode.out = out_->unsqueeze(1);
        if (qv.has_value()) decode.qv = qv->unsqueeze(1);
        decode.cache_batch_idx = kv_batch_idx; decode.leftpad_k = leftpad_k; decode.block_table = page_table;
        decode.softmax_scale = softmax_scale; decode.is_causal = is_causal; decode.window_size_left = window_size_left;
        decode.window_size_right = window_size_right; decode.softcap = softcap; decode.num_splits = num_splits;
        decode.sink = sink; decode.pack_gqa = pack_gqa;
    }
    const auto as_ragged = [&](const std::vector<Tensor> &r) -> std::tuple<Tensor, Tensor> {
        return {r[0].reshape(out_shape), r[1].reshape({batch_size, num_heads}).transpose(0, 1)};
    };
    if (single_token && !appended) {  // a pure decode step in ragged clothes: exactly the dense FA3 call, its append and rotary included
        decode.k_new = k_new; decode.v_new = v_new; decode.seqlens_k = seqused_k; decode.rotary_cos = rotary_cos;
        decode.rotary_sin = rotary_sin; decode.is_rotary_interleaved = is_rotary_interleaved; decode.seqlens_rotary = seqlens_rotary;
        return as_ragged(fwd_kvcache_core(q.unsqueeze(1), kcache, vcache, decode));
    }
    Tensor qc = aligned_or_copy(q);
    if (rotary && total_q > 0)
        qc = rotate_q(qc, cu_seqlens_q, max_seqlen_q, *rotary_cos, *rotary_sin, seqlens_rotary, *seqused_k, is_rotary_interleaved, is_causal,
                      window_size_left, window_size_right);
    if (single_token) {  // behind a ragged append: the read alone, on the fill levels the append wrote
        decode.seqlens_k = seqused;
        return as_ragged(fwd_kvcache_core(qc.unsqueeze(1), kcache, vcache, decode));
    }
    Tensor out = out_.has_value() ? *out_ : at::empty(out_shape, q.options());
    Tensor softmax_lse = at::empty({num_heads, total_q}, q.options().dtype(at::kFloat));
    if (total_q == 0) return {out, softmax_lse};
    if (seqlen_k > 0 && max_seqlen_q > 0) {
        fa3_window(max_seqlen_q, seqlen_k, window_size_left, window_size_right);  // :796-805, on the bounds of the lengths
        if (is_causal) window_size_right = 0;
        const OutPath o(out);
        FwdArgs a;
        a.varlen = true; a.batch = batch_size; a.max_seqlen_q = max_seqlen_q; a.max_seqlen_k = seqlen_k;
        a.softmax_scale = softmax_scale; a.causal = is_causal; a.window_left = window_size_left; a.window_right = window_size_right;
        a.softcap = softcap; a.cu_seqlens_q = cu_seqlens_q; a.seqused_q = seqused_q; a.seqused_k = seqused;
        a.kv_batch_idx = kv_batch_idx; a.block_table = page_table; a.leftpad_k = leftpad_k; a.fa3_window = true;
        a.num_splits = (int)num_splits; a.sink = sink; a.pack_gqa = pack_gqa;
        if (qv.has_value()) a.qv = aligned_or_copy(*qv);
        launch_fwd(qc, kcache, vcache, o.work, softmax_lse, a);
        o.finish();
    } else {
        fill_empty(out, softmax_lse, sink, {num_heads, 1});
    }
    return {out, softmax_lse};
}

// q of the fp8-cache step and of the block-sparse read over a cache: dense (b, s, h, d), or ragged (total_q, h, d) beside
// cu_seqlens_q and a bound of its lengths.  (fwd_kvcache_ragged says the same under the reference's texts and keeps them.)
void check_ragged_q(const Tensor &q, const OptTensor &cu_seqlens_q, c10::optional<int64_t> max_seqlen_q_) {
    const bool ragged = cu_seqlens_q.has_value();
    CHECK_DEVICE(q, "q"); CHECK_LAST_CONTIGUOUS(q, "Input tensor must have contiguous last dimension");
    TORCH_CHECK(q.dim() == (ragged ? 3 : 4), ragged ? "q must have shape (total_q, num_heads, head_size) with cu_seqlens_q"
                                                    : "q must have shape (batch_size, seqlen_q, num_heads, head_size)");
    if (ragged) {
        TORCH_CHECK(cu_seqlens_q->scalar_type() == at::kInt && cu_seqlens_q->is_contiguous() && cu_seqlens_q->is_cuda(),
                    "cu_seqlens_q must be a contiguous int32 CUDA tensor");
        TORCH_CHECK(max_seqlen_q_.has_value() && *max_seqlen_q_ > 0, "max_seqlen_q must be provided with cu_seqlens_q");
    }
}

void check_kv8_descale(const Tensor &t, const char *name, int64_t batch_size, int64_t num_heads_k) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.sizes() == c10::IntArrayRef({batch_size, num_heads_k}), name,
                " must be fp32 (batch_size, num_heads_k)");
}

// The block lists of fwd_kvcache_sparse (include/fa_fwd.h, fa_sparse_kv_params), checked there
struct SparseLists {
    Tensor cnt, idx;     // int32 (b | 1, h_k | 1) and (b | 1, h_k | 1, max_blocks)
    int64_t block_size;  // B
    bool fp8_cache;      // e4m3 caches (else 16-bit caches of q's dtype)
};

// The words of fwd_kvcache_tree (include/fa_fwd.h, fa_tree_params), checked there
struct TreeWords {
    Tensor mask;     // int64 (b, seqlen_q), or (total_q,) beside cu_seqlens_q
    bool fp8_cache;  // e4m3 caches (else 16-bit caches of q's dtype)
};

// 16-bit queries over an fp8 (e4m3) KV cache -- kv_cache_dtype = fp8 of a serving stack (include/fa_fwd.h, fa_fwd_kv8): q and
// out fp16 / bf16, k / v the cache as Float8_e4m3fn, (b_cache, seqlen_k, h_k, d) or pages behind page_table, k_descale /
// v_descale fp32 (b, h_k).  Dense q (b, seqlen_q, h, d) or ragged q (total_q, h, d) with cu_seqlens_q; cache_seqlens in
// seqused_k.  One kernel for every h / h_k (it packs the GQA group into its rows itself: no swap, pack_gqa is moot).
// The read half of fwd_kv8_step below, which has checked q and cu_seqlens_q, appended the step's new rows, rotated q and
// refused what the route does not serve (qv, attention_chunk, head dims).
// mla: the MLA decode shape (fa_fwd_qv8: head_size <= 64 beside v.size(-1) in [256, 512], qv optional, out (..., h, d_v)); every
// other argument is handled alike, so fwd_qv8 below is this function with mla set.
// sparse: the block-sparse read (fa_fwd_sparse_kv) of fwd_kvcache_sparse below, over an e4m3 cache or -- the one case where k / v
// are 16-bit here -- a cache of q's dtype; the lists ride beside the same params, everything else is handled alike.
// tree: tree attention (fa_fwd_tree) of fwd_kvcache_tree below, over either cache type as well; the words ride beside the params.
std::tuple<Tensor, Tensor> fwd_kv8(const Tensor &q, const Tensor &k, const Tensor &v, const OptTensor &out_,
                                   const OptTensor &cu_seqlens_q, const OptTensor &seqused_q, const OptTensor &seqused_k,
                                   c10::optional<int64_t> max_seqlen_q_, const OptTensor &page_table, const OptTensor &kv_batch_idx,
                                   const OptTensor &leftpad_k, const OptTensor &k_descale, const OptTensor &v_descale,
                                   double softmax_scale, bool is_causal, int64_t window_size_left, int64_t window_size_right,
                                   double softcap, int64_t num_splits, const OptTensor &qv = c10::nullopt, bool mla = false,
                                   const SparseLists *sparse = nullptr, const TreeWords *tree = nullptr) {
    const bool wide_cache = (sparse && !sparse->fp8_cache) || (tree && !tree->fp8_cache);  // 16-bit k / v: strides in 2-byte elements
    CHECK_DEVICE(k, "k"); CHECK_LAST_CONTIGUOUS(k, "Input tensor must have contiguous last dimension");
    CHECK_DEVICE(v, "v"); CHECK_LAST_CONTIGUOUS(v, "Input tensor must have contiguous last dimension");
    const bool ragged = cu_seqlens_q.has_value();
    TORCH_CHECK(k.dim() == 4 && v.dim() == 4, sparse || tree ? "k / v" : "an fp8 k / v",
                " must be a KV cache of shape (batch or num_pages, seqlen or page_size, num_heads_k, head_size)");
    const int64_t head_size = q.size(-1), num_heads = q.size(-2), num_heads_k = k.size(2);
    const int64_t head_size_v = mla ? v.size(3) : head_size;
    std::vector<int64_t> out_shape = q.sizes().vec();  // q's with V's head dim
    out_shape.back() = head_size_v;
    int64_t batch_size, seqlen_q, total_q;
    if (ragged) {
        TORCH_CHECK(seqused_k.has_value(), "seqused_k (the cache fill levels) must be provided with cu_seqlens_q over a KV cache");
        batch_size = cu_seqlens_q->numel() - 1; seqlen_q = *max_seqlen_q_; total_q = q.size(0);
    } else {
        TORCH_CHECK(!seqused_q.has_value(),
                    "This flash attention build does not support KV-cache arguments together with seqused_q without cu_seqlens_q.");
        batch_size = q.size(0); seqlen_q = q.size(1); total_q = batch_size * seqlen_q;
    }
    TORCH_CHECK(batch_size > 0, "batch size must be positive");
    TORCH_CHECK(num_heads_k > 0 && num_heads % num_heads_k == 0, "Number of heads in key/value must divide number of heads in query");
    CacheRules rules;
    if (!wide_cache) {
        rules.base_grain = rules.stride_grain = 16;
        rules.misaligned = "the fp8 KV cache must be 16-byte aligned with row/head/batch strides that are multiples of 16";
    }
    rules.k_shape = "k must have shape (..., " + std::to_string(num_heads_k) + ", " + std::to_string(head_size) + ")";
    rules.v_shape = mla ? "v must have the shape of k with its own head_size_v" : "v must have the shape of k";
    rules.fill_dtype = rules.fill_device = rules.fill_contiguous = rules.fill_shape = " must be int32 of shape (batch_size,)";
    rules.fill_any_dims = true;
    rules.idx_contiguous = rules.idx_length = " must be contiguous, (batch_size,)";
    if (seqused_q.has_value()) check_fill_levels(*seqused_q, "seqused_q", batch_size, rules);
    const CacheSide cache = check_cache(k, v, page_table, kv_batch_idx, seqused_k, leftpad_k, batch_size, head_size, head_size_v, rules);
    if (qv.has_value()) {
        TORCH_CHECK(qv->scalar_type() == q.scalar_type(), "q_v must have the same dtype as query");
        TORCH_CHECK(qv->is_cuda() && qv->device() == q.device(), "q_v must be on the same CUDA device as query");
        CHECK_LAST_CONTIGUOUS(*qv, "q_v tensor must have contiguous last dimension");
        TORCH_CHECK(qv->sizes() == c10::IntArrayRef(out_shape), "q_v must have shape ", tuple_str(out_shape));
    }
    const int64_t seqlen_k = cache.seqlen_k;
    if (leftpad_k.has_value()) TORCH_CHECK(seqused_k.has_value(), "seqused_k must be provided with k_new / leftpad_k");
    for (const auto &[t, name] : {std::make_pair(&k_descale, "k_descale"), std::make_pair(&v_descale, "v_descale")})
        if (t->has_value()) check_kv8_descale(**t, name, batch_size, num_heads_k);
    Tensor out;
    if (out_.has_value()) {
        out = *out_;
        TORCH_CHECK(out.scalar_type() == q.scalar_type(), "Output must have the same dtype as the query");
        TORCH_CHECK(out.is_cuda() && out.stride(-1) == 1 && out.sizes() == c10::IntArrayRef(out_shape),
                    mla ? "out must have the shape of q with the head dim of v" : "out must have the shape of q");
    } else {
        out = at::empty(out_shape, q.options());
    }
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(q.device());
    Tensor softmax_lse = ragged ? at::empty({num_heads, total_q}, q.options().dtype(at::kFloat))
                                : at::empty({batch_size, num_heads, seqlen_q}, q.options().dtype(at::kFloat));
    if (total_q == 0) return {out, softmax_lse};
    if (sparse) {  // one list per kv head, or one for all of a dimension of size 1
        TORCH_CHECK(sparse->cnt.size(0) == 1 || sparse->cnt.size(0) == batch_size, "kv_block_cnt must have shape (batch_size | 1, num_heads_k | 1)");
        TORCH_CHECK(sparse->cnt.size(1) == 1 || sparse->cnt.size(1) == num_heads_k, "kv_block_cnt must have shape (batch_size | 1, num_heads_k | 1)");
        TORCH_CHECK(sparse->idx.size(0) == 1 || sparse->idx.size(0) == batch_size, "kv_block_idx must have shape (batch_size | 1, num_heads_k | 1, max_blocks)");
        TORCH_CHECK(sparse->idx.size(1) == 1 || sparse->idx.size(1) == num_heads_k, "kv_block_idx must have shape (batch_size | 1, num_heads_k | 1, max_blocks)");
    }
    if (tree)
        TORCH_CHECK(tree->mask.sizes() == (ragged ? c10::IntArrayRef({total_q}) : c10::IntArrayRef({batch_size, seqlen_q})),
                    "tree_mask must have shape (batch_size, seqlen_q), or (total_q,) with cu_seqlens_q");
    if (seqlen_k == 0 || seqlen_q == 0) {
        fill_empty(out, softmax_lse);
        return {out, softmax_lse};
    }
    const Tensor qc = aligned_or_copy(q);
    const OutPath o(out);
    FwdArgs a;  // (the cache's strides count elements = bytes; its 4 dims take the batched-cache branch under ragged queries)
    a.varlen = ragged; a.batch = batch_size; a.max_seqlen_q = seqlen_q; a.max_seqlen_k = seqlen_k;
    a.softmax_scale = softmax_scale; a.softcap = softcap; a.causal = is_causal; a.fa3_window = true;
    a.window_left = std::max<int64_t>(window_size_left, -1); a.window_right = std::max<int64_t>(window_size_right, -1);
    a.cu_seqlens_q = cu_seqlens_q; a.seqused_q = seqused_q; a.seqused_k = seqused_k; a.k_descale = k_descale; a.v_descale = v_descale;
    a.kv_batch_idx = kv_batch_idx; a.leftpad_k = leftpad_k; a.block_table = page_table;
    a.num_splits = (int)std::max<int64_t>(num_splits, 0);
    if (qv.has_value()) a.qv = aligned_or_copy(*qv);
    fa_fwd_params p = fill_fwd_params(qc, k, v, o.work, softmax_lse, a);
    fa_sparse_kv_params sp{};
    if (sparse) {
        sp.abi_version = FA_ABI_VERSION;
        sp.struct_size = sizeof(fa_sparse_kv_params);
        sp.block_cnt = static_cast<const int32_t *>(sparse->cnt.data_ptr());
        sp.block_idx = static_cast<const int32_t *>(sparse->idx.data_ptr());
        sp.cnt_batch_stride = sparse->cnt.size(0) == 1 ? 0 : sparse->cnt.stride(0);
        sp.cnt_head_stride = sparse->cnt.size(1) == 1 ? 0 : sparse->cnt.stride(1);
        sp.idx_batch_stride = sparse->idx.size(0) == 1 ? 0 : sparse->idx.stride(0);
        sp.idx_head_stride = sparse->idx.size(1) == 1 ? 0 : sparse->idx.stride(1);
        sp.max_blocks = (int32_t)sparse->idx.size(2);
        sp.block_size = (int32_t)sparse->block_size;
        sp.fp8_cache = sparse->fp8_cache ? 1 : 0;
    }
    fa_tree_params tp{};
    if (tree) {
        tp.abi_version = FA_ABI_VERSION;
        tp.struct_size = sizeof(fa_tree_params);
        tp.tree_mask = static_cast<const int64_t *>(tree->mask.data_ptr());
        tp.batch_stride = ragged ? 0 : tree->mask.stride(0);
        tp.row_stride = tree->mask.stride(-1);
        tp.fp8_cache = tree->fp8_cache ? 1 : 0;
    }
    const char *entry = tree ? "fa_fwd_tree" : sparse ? "fa_fwd_sparse_kv" : mla ? "fa_fwd_qv8" : "fa_fwd_kv8";
    const int64_t need = tree     ? fa_fwd_tree_workspace_size(&p, &tp)
                         : sparse ? fa_fwd_sparse_kv_workspace_size(&p, &sp)
                         : mla    ? fa_fwd_qv8_workspace_size(&p)
                                  : fa_fwd_kv8_workspace_size(&p);
    TORCH_CHECK(need >= 0, entry, "_workspace_size failed (", need, "): ", fa_strerror((int)need));
    const Tensor workspace = set_workspace(p, need, q);  // split-KV partials
    const int st = tree     ? fa_fwd_tree(&p, &tp, current_stream(q))
                   : sparse ? fa_fwd_sparse_kv(&p, &sp, current_stream(q))
                   : mla    ? fa_fwd_qv8(&p, current_stream(q))
                            : fa_fwd_kv8(&p, current_stream(q));
    TORCH_CHECK(st == 0, entry, " failed (", st, "): ", fa_strerror(st));
    o.finish();
    return {out, softmax_lse};
}

// hopper_interface.flash_attn_with_kvcache_sparse / torch.ops.flash_attn_3.fwd_kvcache_sparse: attention of a decode, verify or
// ragged serving step over the key blocks of the cache that kv_block_cnt / kv_block_idx list per kv head (include/fa_fwd.h,
// fa_fwd_sparse_kv).  16-bit caches of q's dtype or e4m3 caches with both descales; read-only (the appends are the other calls').
// The refusals by argument stand here; the cache side, out, the workspace and the launch are fwd_kv8's.  Nothing of the lists is
// read on the host.
std::tuple<Tensor, Tensor> fwd_kvcache_sparse(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &kv_block_cnt,
                                              const Tensor &kv_block_idx, int64_t kv_block_size, const OptTensor &seqused_k,
                                              const OptTensor &kv_batch_idx, const OptTensor &leftpad_k, const OptTensor &page_table,
                                              const OptTensor &cu_seqlens_q, c10::optional<int64_t> max_seqlen_q_,
                                              const OptTensor &k_descale, const OptTensor &v_descale, c10::optional<double> softmax_scale_,
                                              bool is_causal, int64_t window_size_left, int64_t window_size_right, double softcap,
                                              int64_t num_splits) {
    const auto q_dtype = q.scalar_type();
    TORCH_CHECK(q_dtype == at::kHalf || q_dtype == at::kBFloat16,
                "This flash attention build supports block-sparse attention over a KV cache for fp16 / bf16 queries only");
    TORCH_CHECK(k.scalar_type() == v.scalar_type(), "k_cache and v_cache must have the same dtype");
    const bool fp8_cache = k.scalar_type() == at::kFloat8_e4m3fn;
    TORCH_CHECK(fp8_cache || k.scalar_type() == q_dtype,
                "k_cache / v_cache must have the dtype of the query or be torch.float8_e4m3fn under an fp16 / bf16 query");
    if (fp8_cache) {
        TORCH_CHECK(k_descale.has_value() && v_descale.has_value(), "k_descale and v_descale must be provided with an fp8 KV cache");
    } else {
        TORCH_CHECK(!k_descale.has_value() && !v_descale.has_value(), "k_descale / v_descale belong to an fp8 KV cache");
    }
    TORCH_CHECK(kv_block_size > 0 && kv_block_size % 64 == 0, "kv_block_size must be a positive multiple of 64, got ", kv_block_size);
    for (const auto &[t, name] : {std::make_pair(&kv_block_cnt, "kv_block_cnt"), std::make_pair(&kv_block_idx, "kv_block_idx")}) {
        TORCH_CHECK(t->scalar_type() == at::kInt, name, " must have dtype int32");
        TORCH_CHECK(t->is_cuda() && t->device() == q.device(), name, " must be on the same CUDA device as query");
    }
    TORCH_CHECK(kv_block_cnt.dim() == 2, "kv_block_cnt must have shape (batch_size | 1, num_heads_k | 1)");
    TORCH_CHECK(kv_block_idx.dim() == 3, "kv_block_idx must have shape (batch_size | 1, num_heads_k | 1, max_blocks)");
    TORCH_CHECK(kv_block_idx.size(2) == 0 || kv_block_idx.stride(2) == 1, "kv_block_idx must have contiguous last dimension");
    TORCH_CHECK(kv_block_idx.size(2) * kv_block_size <= 0x7fffffff, "max_blocks * kv_block_size must stay below 2^31");
    TORCH_CHECK(k.dim() == 4 && v.dim() == 4 && v.size(-1) == q.size(-1) && k.size(-1) == q.size(-1),
                "This flash attention build does not support a V headdim of its own with block-sparse attention over a KV cache.");
    TORCH_CHECK(q.size(-1) <= 128 && q.size(-1) % 16 == 0,
                "This flash attention build supports block-sparse attention over a KV cache for head_size <= 128 that is a multiple "
                "of 16, got ", q.size(-1));
    check_ragged_q(q, cu_seqlens_q, max_seqlen_q_);
    const double softmax_scale = softmax_scale_.has_value() ? *softmax_scale_ : 1.0 / std::sqrt((double)q.size(-1));
    const SparseLists lists{kv_block_cnt, kv_block_idx, kv_block_size, fp8_cache};
    return fwd_kv8(q, k, v, c10::nullopt, cu_seqlens_q, c10::nullopt, seqused_k, max_seqlen_q_, page_table, kv_batch_idx, leftpad_k,
                   k_descale, v_descale, softmax_scale, is_causal, window_size_left, window_size_right, softcap, num_splits, c10::nullopt,
                   false, &lists);
}

// hopper_interface.flash_attn_with_kvcache_tree / torch.ops.flash_attn_3.fwd_kvcache_tree: the verify step of speculative decoding
// over a token tree (include/fa_fwd.h, fa_fwd_tree): every query row sees the committed prefix of the cache and the draft keys
// its int64 word names.  16-bit caches of q's dtype or e4m3 caches with both descales; read-only, no causal / window / rotary
// argument (the words are the mask; positions in a tree are depths, so the caller rotates before the append).  The refusals by
// argument stand here; the cache side, out, the workspace and the launch are fwd_kv8's.  Nothing of the words is read on the host.
std::tuple<Tensor, Tensor> fwd_kvcache_tree(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &tree_mask,
                                            const OptTensor &seqused_k, const OptTensor &kv_batch_idx, const OptTensor &leftpad_k,
                                            const OptTensor &page_table, const OptTensor &cu_seqlens_q,
                                            c10::optional<int64_t> max_seqlen_q_, const OptTensor &k_descale, const OptTensor &v_descale,
                                            c10::optional<double> softmax_scale_, double softcap, int64_t num_splits) {
    const auto q_dtype = q.scalar_type();
    TORCH_CHECK(q_dtype == at::kHalf || q_dtype == at::kBFloat16,
                "This flash attention build supports tree attention over a KV cache for fp16 / bf16 queries only");
    TORCH_CHECK(k.scalar_type() == v.scalar_type(), "k_cache and v_cache must have the same dtype");
    const bool fp8_cache = k.scalar_type() == at::kFloat8_e4m3fn;
    TORCH_CHECK(fp8_cache || k.scalar_type() == q_dtype,
                "k_cache / v_cache must have the dtype of the query or be torch.float8_e4m3fn under an fp16 / bf16 query");
    if (fp8_cache) {
        TORCH_CHECK(k_descale.has_value() && v_descale.has_value(), "k_descale and v_descale must be provided with an fp8 KV cache");
    } else {
        TORCH_CHECK(!k_descale.has_value() && !v_descale.has_value(), "k_descale / v_descale belong to an fp8 KV cache");
    }
    TORCH_CHECK(tree_mask.scalar_type() == at::kLong, "tree_mask must have dtype int64");
    TORCH_CHECK(tree_mask.is_cuda() && tree_mask.device() == q.device(), "tree_mask must be on the same CUDA device as query");
    TORCH_CHECK(k.dim() == 4 && v.dim() == 4 && v.size(-1) == q.size(-1) && k.size(-1) == q.size(-1),
                "This flash attention build does not support a V headdim of its own with tree attention over a KV cache.");
    TORCH_CHECK(q.size(-1) <= 128 && q.size(-1) % 16 == 0,
                "This flash attention build supports tree attention over a KV cache for head_size <= 128 that is a multiple of 16, "
                "got ", q.size(-1));
    check_ragged_q(q, cu_seqlens_q, max_seqlen_q_);
    const int64_t nodes = cu_seqlens_q.has_value() ? *max_seqlen_q_ : q.size(1);
    TORCH_CHECK(nodes <= 64, "This flash attention build supports token trees of at most 64 nodes (one int64 word per query row), got ",
                nodes);
    const double softmax_scale = softmax_scale_.has_value() ? *softmax_scale_ : 1.0 / std::sqrt((double)q.size(-1));
    const TreeWords words{tree_mask, fp8_cache};
    return fwd_kv8(q, k, v, c10::nullopt, cu_seqlens_q, c10::nullopt, seqused_k, max_seqlen_q_, page_table, kv_batch_idx, leftpad_k,
                   k_descale, v_descale, softmax_scale, false, -1, -1, softcap, num_splits, c10::nullopt, false, nullptr, &words);
}

// The MLA decode shape over an fp8 KV cache (include/fa_fwd.h, fa_fwd_qv8): q (.., h, d <= 64) and the optional qv (.., h, d_v)
// fp16 / bf16, k (.., h_k, d) and v (.., h_k, d_v in [256, 512]) Float8_e4m3fn, out (.., h, d_v) in q's dtype.  Descales,
// num_splits and the workspace as fwd_kv8 handles them: it is that function.
std::tuple<Tensor, Tensor> fwd_qv8(const Tensor &q, const Tensor &k, const Tensor &v, const OptTensor &qv, const OptTensor &out_,
                                   const OptTensor &cu_seqlens_q, const OptTensor &seqused_q, const OptTensor &seqused_k,
                                   c10::optional<int64_t> max_seqlen_q_, const OptTensor &page_table, const OptTensor &kv_batch_idx,
                                   const OptTensor &leftpad_k, const OptTensor &k_descale, const OptTensor &v_descale,
                                   double softmax_scale, bool is_causal, int64_t window_size_left, int64_t window_size_right,
                                   double softcap, int64_t num_splits) {
    return fwd_kv8(q, k, v, out_, cu_seqlens_q, seqused_q, seqused_k, max_seqlen_q_, page_table, kv_batch_idx, leftpad_k, k_descale,
                   v_descale, softmax_scale, is_causal, window_size_left, window_size_right, softcap, num_splits, qv, true);
}

// The write half of an fp8 (e4m3) KV cache (include/fa_fwd.h, fa_kvcache_append_kv8): new 16-bit rows -- dense (b, s_new, h_k, d)
// or ragged (total_k_new, h_k, d) with cu_seqlens_k_new -- are rotated (keys), divided by the descale of their (sequence, kv
// head), converted to e4m3 and stored at cache_seqlens[s] + i of the batched or paged cache.  Every check runs before the one
// launch; nothing reads device data.  Returns the new fill levels min(cache_seqlens + new rows, capacity), written by the launch.
// A cache of the MLA shape (head_size <= 64 beside a latent / V head dim in [256, 512], the shape fwd_qv8 reads) goes to
// fa_kvcache_append_qv8 under the same checks: k_new is the k_pe row, v_new the latent row.
Tensor kvcache_append_kv8(const Tensor &k_cache, const Tensor &v_cache, const Tensor &k_new, const Tensor &v_new,
                          const Tensor &cache_seqlens, const Tensor &k_descale, const Tensor &v_descale,
                          const OptTensor &cu_seqlens_k_new, int64_t max_seqlen_k_new, const OptTensor &cache_batch_idx,
                          const OptTensor &page_table, const OptTensor &rotary_cos, const OptTensor &rotary_sin,
                          const OptTensor &rotary_seqlens, bool rotary_interleaved) {
    TORCH_CHECK(k_cache.scalar_type() == at::kFloat8_e4m3fn && v_cache.scalar_type() == at::kFloat8_e4m3fn,
                "the fp8 KV cache must have dtype torch.float8_e4m3fn");
    TORCH_CHECK(k_new.scalar_type() != at::kFloat8_e4m3fn && v_new.scalar_type() != at::kFloat8_e4m3fn,
                "This flash attention build does not support fp8 k_new / v_new with an fp8 KV cache: the new rows are fp16 / "
                "bf16 and are quantised by the append.");
    const auto new_dtype = k_new.scalar_type();
    TORCH_CHECK(new_dtype == at::kHalf || new_dtype == at::kBFloat16, "k_new / v_new must be fp16 or bf16");
    TORCH_CHECK(v_new.scalar_type() == new_dtype, "k_new and v_new must have the same dtype");
    CHECK_DEVICE(k_cache, "k_cache"); CHECK_DEVICE(v_cache, "v_cache"); CHECK_DEVICE(k_new, "k_new"); CHECK_DEVICE(v_new, "v_new");
    TORCH_CHECK(k_cache.dim() == 4 && v_cache.dim() == 4,
                "an fp8 k / v must be a KV cache of shape (batch or num_pages, seqlen or page_size, num_heads_k, head_size)");
    CHECK_LAST_CONTIGUOUS(k_cache, "Input tensor must have contiguous last dimension");
    CHECK_LAST_CONTIGUOUS(v_cache, "Input tensor must have contiguous last dimension");
    TORCH_CHECK(k_new.stride(-1) == 1, "k_new tensor must have contiguous last dimension");
    TORCH_CHECK(v_new.stride(-1) == 1, "v_new tensor must have contiguous last dimension");
    const int64_t num_heads_k = k_cache.size(2), head_size = k_cache.size(3);
    TORCH_CHECK(head_size <= 128 && head_size % 16 == 0,
                "This flash attention build supports an fp8 KV cache for head_size <= 128 that is a multiple of 16, got ", head_size);
    // the MLA shape (what fa_fwd_qv8 reads): a latent / V head dim in [256, 512] beside head_size <= 64, pages / rows / heads
    // those of K; any other V that is not K's shape keeps its refusal below
    const bool mla = head_size <= 64 && v_cache.size(3) >= 256 && v_cache.size(3) <= 512 && v_cache.size(3) % 16 == 0 &&
                     v_cache.sizes().slice(0, 3) == k_cache.sizes().slice(0, 3);
    const int64_t head_size_v = mla ? v_cache.size(3) : head_size;
    CacheRules rules;
    rules.base_grain = 8;
    rules.misaligned = "the fp8 KV cache must be 8-byte aligned with row/head/batch strides that are multiples of 8 to be appended to";
    rules.v_shape = "v must have the shape of k";
    rules.fill_name = "cache_seqlens";
    rules.fill_dtype = rules.fill_device = rules.fill_contiguous = rules.fill_shape =
        " must be a contiguous int32 CUDA tensor of shape (batch_size,)";
    rules.idx_contiguous = rules.idx_length = " must be contiguous, (batch_size,)";
    // (the batch is the number of fill levels, one at the least)
    const int64_t batch_size = std::max<int64_t>(cache_seqlens.numel(), 1);
    const CacheSide cache = check_cache(k_cache, v_cache, page_table, cache_batch_idx, cache_seqlens, c10::nullopt, batch_size, head_size,
                                        head_size_v, rules);
    const bool ragged = cu_seqlens_k_new.has_value();
    check_new_rows(k_new, v_new, cu_seqlens_k_new, batch_size, num_heads_k, head_size, head_size_v, "k_new.size",
                   mla ? "head_size_v" : "head_size");
    if (ragged) TORCH_CHECK(max_seqlen_k_new >= 0, "max_seqlen_k_new must be non-negative");
    check_kv8_descale(k_descale, "k_descale", batch_size, num_heads_k);
    check_kv8_descale(v_descale, "v_descale", batch_size, num_heads_k);
    TORCH_CHECK(rotary_cos.has_value() == rotary_sin.has_value(), "rotary_cos and rotary_sin must be passed together");
    if (rotary_cos.has_value()) check_rotary_tables(*rotary_cos, *rotary_sin, head_size, cache.seqlen_k, new_dtype, "k_new");
    if (rotary_seqlens.has_value()) check_seqlens_rotary(*rotary_seqlens, batch_size);
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(k_cache.device());
    const Tensor kn = aligned_or_copy(k_new), vn = aligned_or_copy(v_new);
    Tensor seqused_out = at::empty({batch_size}, cache_seqlens.options());
    fa_kvcache_append_kv8_params p{};
    fill_append_common(p, k_cache, v_cache, cache_seqlens, cache_batch_idx, page_table, rotary_cos, rotary_sin, rotary_interleaved,
                       rotary_seqlens);  // (cache strides: elements = bytes)
    p.k_new = kn.data_ptr(); p.v_new = vn.data_ptr();
    if (ragged) {
        p.knew_row_stride = kn.stride(0); p.knew_head_stride = kn.stride(1);
        p.vnew_row_stride = vn.stride(0); p.vnew_head_stride = vn.stride(1);
        p.total_k_new = (int32_t)kn.size(0);
        p.max_seqlen_k_new = (int32_t)max_seqlen_k_new;
        p.cu_seqlens_k_new = static_cast<const int32_t *>(cu_seqlens_k_new->data_ptr());
    } else {
        p.knew_batch_stride = kn.stride(0); p.knew_row_stride = kn.stride(1); p.knew_head_stride = kn.stride(2);
        p.vnew_batch_stride = vn.stride(0); p.vnew_row_stride = vn.stride(1); p.vnew_head_stride = vn.stride(2);
        p.seqlen_new = (int32_t)kn.size(1);
    }
    p.b = (int32_t)batch_size; p.h_k = (int32_t)num_heads_k; p.d = (int32_t)head_size;
    p.dtype = dtype_code(kn);
    p.seqused_out = static_cast<int32_t *>(seqused_out.data_ptr());
    p.k_descale = static_cast<const float *>(k_descale.data_ptr());
    p.k_descale_batch_stride = k_descale.stride(0); p.k_descale_head_stride = k_descale.stride(1);
    p.v_descale = static_cast<const float *>(v_descale.data_ptr());
    p.v_descale_batch_stride = v_descale.stride(0); p.v_descale_head_stride = v_descale.stride(1);
    if (mla) p.d_v = (int32_t)head_size_v;
    const int st = mla ? fa_kvcache_append_qv8(&p, current_stream(k_cache)) : fa_kvcache_append_kv8(&p, current_stream(k_cache));
    TORCH_CHECK(st == 0, mla ? "fa_kvcache_append_qv8 failed (" : "fa_kvcache_append_kv8 failed (", st, "): ", fa_strerror(st));
    return seqused_out;
}

// hopper_interface.kvcache_append_fp8 / torch.ops.flash_attn_3.kvcache_append_fp8: the append alone, for stacks that fill the
// cache apart from attention.
Tensor kvcache_append_fp8(const Tensor &k_cache, const Tensor &v_cache, const Tensor &k, const Tensor &v, const Tensor &cache_seqlens,
                          const Tensor &k_descale, const Tensor &v_descale, const OptTensor &cu_seqlens_k_new,
                          c10::optional<int64_t> max_seqlen_k_new, const OptTensor &cache_batch_idx, const OptTensor &page_table,
                          const OptTensor &rotary_cos, const OptTensor &rotary_sin, const OptTensor &rotary_seqlens,
                          bool rotary_interleaved) {
    return kvcache_append_kv8(k_cache, v_cache, k, v, cache_seqlens, k_descale, v_descale, cu_seqlens_k_new,
                              max_seqlen_k_new.value_or(0), cache_batch_idx, page_table, rotary_cos, rotary_sin, rotary_seqlens,
                              rotary_interleaved);
}

// One serving step of 16-bit queries over an fp8 KV cache, the counterpart of fwd_kvcache_core / fwd_kvcache_ragged: refusals by
// argument, the quantising append, the rotary pass of q, the read (fwd_kv8) on the new fill levels.
// With both descales the step may write: new rows (16-bit, dense or ragged with cu_seqlens_k_new beside cu_seqlens_q) are
// quantised into the cache in place (kvcache_append_kv8) and q is rotated by the 16-bit pass.  Without them the scale of the
// new rows would be an implied 1, which is almost never meant: those calls keep their refusals.
std::tuple<Tensor, Tensor> fwd_kv8_step(const Tensor &q, const Tensor &k, const Tensor &v, const OptTensor &k_new, const OptTensor &v_new,
                                        const OptTensor &qv, const OptTensor &out_, const OptTensor &cu_seqlens_q,
                                        const OptTensor &cu_seqlens_k, const OptTensor &cu_seqlens_k_new, const OptTensor &seqused_q,
                                        const OptTensor &seqused_k, c10::optional<int64_t> max_seqlen_q_, const OptTensor &page_table,
                                        const OptTensor &kv_batch_idx, const OptTensor &leftpad_k, const OptTensor &rotary_cos,
                                        const OptTensor &rotary_sin, OptTensor seqlens_rotary, const OptTensor &k_descale,
                                        const OptTensor &v_descale, double softmax_scale, bool is_causal, int64_t window_size_left,
                                        int64_t window_size_right, int64_t attention_chunk, double softcap, bool is_rotary_interleaved,
                                        int64_t num_splits, const OptTensor &sink) {
    const auto q_dtype = q.scalar_type();
    // the MLA decode shape (fa_fwd_qv8): q/k head dim <= 64 beside a V / latent head dim in [256, 512], qv optional
    const bool mla = q.size(-1) <= 64 && q.size(-1) % 16 == 0 && v.size(-1) >= 256 && v.size(-1) <= 512 && v.size(-1) % 16 == 0;
    if (mla) {  // the fused call only reads this shape; its step is two calls: kvcache_append_fp8 (fa_kvcache_append_qv8: k_pe
                // rotated and quantised, the latent quantised), then this read on the fill levels that call returns
        TORCH_CHECK(!k_new.has_value() && !v_new.has_value() && !cu_seqlens_k_new.has_value(),
                    "This flash attention build does not support k_new / v_new with an fp8 KV cache of the MLA shape (head_size <= 64 "
                    "beside head_size_v in [256, 512]): it is read only.");
        TORCH_CHECK(!rotary_cos.has_value() && !rotary_sin.has_value(),
                    "This flash attention build does not support rotary_cos / rotary_sin with an fp8 KV cache of the MLA shape "
                    "(head_size <= 64 beside head_size_v in [256, 512]): it is read only.");
    }
    if (!(k_descale.has_value() && v_descale.has_value())) {
        TORCH_CHECK(!k_new.has_value() && !v_new.has_value() && !cu_seqlens_k_new.has_value(),
                    "This flash attention build does not support k_new / v_new with an fp8 KV cache: appending to it (quantising "
                    "the new rows) is the caller's job.");
        TORCH_CHECK(!rotary_cos.has_value() && !rotary_sin.has_value(),
                    "This flash attention build does not support rotary_cos / rotary_sin with an fp8 KV cache.");
    }
    TORCH_CHECK(mla || !qv.has_value(), "This flash attention build does not support qv with an fp8 KV cache.");
    TORCH_CHECK(mla || v.size(-1) == q.size(-1),
                "This flash attention build does not support a V headdim of its own with an fp8 KV cache.");
    TORCH_CHECK(attention_chunk == 0, "This flash attention build does not support attention_chunk with an fp8 KV cache.");
    TORCH_CHECK(q.size(-1) <= 128 && q.size(-1) % 16 == 0,
                "This flash attention build supports an fp8 KV cache for head_size <= 128 that is a multiple of 16, got ", q.size(-1));
    TORCH_CHECK(!cu_seqlens_k.has_value(), "This flash attention build does not support cu_seqlens_k with an fp8 KV cache.");
    TORCH_CHECK(!sink.has_value(), "This flash attention build does not support a learnable sink with an fp8 KV cache.");
    const bool appends = k_new || v_new || cu_seqlens_k_new || rotary_cos || rotary_sin;
    if (appends) {
        TORCH_CHECK(k_new.has_value() && v_new.has_value(),
                    rotary_cos || rotary_sin
                        ? "If rotary cos/sin are provided, new key / value to be appended to KV cache must also be provided"
                        : "k_new and v_new must be passed together");
        TORCH_CHECK(rotary_cos.has_value() == rotary_sin.has_value(), "rotary_cos and rotary_sin must be passed together");
        TORCH_CHECK(!cu_seqlens_k_new.has_value() || cu_seqlens_q.has_value(),
                    "This flash attention build does not support cu_seqlens_k_new without cu_seqlens_q.");
        TORCH_CHECK(k_new->scalar_type() == at::kFloat8_e4m3fn || (k_new->scalar_type() == q_dtype && v_new->scalar_type() == q_dtype),
                    "k_new and v_new must have the same dtype as query");
        TORCH_CHECK(seqused_k.has_value(), "seqused_k must be provided with k_new / leftpad_k");
    }
    // q and cu_seqlens_q, once for the append, the rotary pass and the read
    const bool ragged = cu_seqlens_q.has_value();
    check_ragged_q(q, cu_seqlens_q, max_seqlen_q_);
    if (mla)
        return fwd_qv8(q, k, v, qv, out_, cu_seqlens_q, seqused_q, seqused_k, max_seqlen_q_, page_table, kv_batch_idx, leftpad_k, k_descale,
                       v_descale, softmax_scale, is_causal, window_size_left, window_size_right, softcap, num_splits);
    OptTensor fill = seqused_k;
    Tensor qc = q;
    if (appends) {
        const int64_t batch_size = ragged ? cu_seqlens_q->numel() - 1 : q.size(0);
        TORCH_CHECK(seqused_k->dim() == 1 && seqused_k->numel() == batch_size, "seqused_k must be int32 of shape (batch_size,)");
        TORCH_CHECK(k.dim() == 4 && k.size(3) == q.size(-1) && k.size(2) > 0 && q.size(-2) % k.size(2) == 0,
                    "Number of heads in key/value must divide number of heads in query");
        check_leftpad(leftpad_k, batch_size, page_table.has_value());
        if (!rotary_cos.has_value()) seqlens_rotary = c10::nullopt;  // (only read with rotary)
        // the append first: what the read sees are the new fill levels -- dense rows: seqused_k + seqlen_new, like the 16-bit
        // route; ragged rows: what the launch wrote
        const Tensor written = kvcache_append_kv8(k, v, *k_new, *v_new, *seqused_k, *k_descale, *v_descale, cu_seqlens_k_new, 0,
                                                  kv_batch_idx, page_table, rotary_cos, rotary_sin, seqlens_rotary,
                                                  is_rotary_interleaved);
        fill = cu_seqlens_k_new.has_value() ? written : *seqused_k + k_new->size(-3);
        if (rotary_cos.has_value() && q.numel() > 0) {
            const Tensor qa = aligned_or_copy(q);
            c10::hip::HIPGuardMasqueradingAsCUDA device_guard(q.device());
            qc = rotate_q(qa, cu_seqlens_q, max_seqlen_q_.value_or(0), *rotary_cos, *rotary_sin, seqlens_rotary, *seqused_k,
                          is_rotary_interleaved, is_causal, window_size_left, window_size_right);
        }
    }
    return fwd_kv8(qc, k, v, out_, cu_seqlens_q, seqused_q, fill, max_seqlen_q_, page_table, kv_batch_idx, leftpad_k, k_descale,
                   v_descale, softmax_scale, is_causal, window_size_left, window_size_right, softcap, num_splits);
}

// flash_attn_3::fwd, hopper/flash_api.cpp:672-1198 (schema :1672-1707): the 34 positional arguments of
// hopper/flash_attn_interface.py:66, returns (out, softmax_lse, None, None).
// Built: fp16 / bf16 / fp8 e4m3 inputs (fp8 -> bf16 output, :859), per-(batch, kv head) q/k/v descales (:1115-1146), dense
// and varlen (`cu_seqlens_*`, `seqused_*`), causal / sliding window / softcap / attention_chunk, GQA, a V head dim of its
// own.  KV-cache arguments (dense q, 16-bit: k_new / v_new appended in place at seqused_k, page_table of any page size,
// kv_batch_idx, leftpad_k, rotary) and plain decode over a cache go to fwd_kvcache_core; the same arguments with ragged
// queries (cu_seqlens_q + max_seqlen_q, k_new dense or ragged with cu_seqlens_k_new, seqused_q) to fwd_kvcache_ragged.  qv
// (MLA absorbed attention, :1028-1048: scores = (q.k + qv.v) * scale, d <= 64 beside d_v in [256, 512], 16-bit) on every
// route.  Accepted and rejected by message, like the reference does for compiled-out features (:1148-1165):
// cu_seqlens_k_new without cu_seqlens_q, qv of any other shape or with fp8, KV-cache arguments together with cu_seqlens_k,
// attention_chunk or fp8.  `scheduler_metadata` and `sm_margin` are performance hints and do not change results: ignored.
// 16-bit q beside a Float8_e4m3fn k / v (an fp8 KV cache with k_descale / v_descale, out in q's dtype): recognised here and
// served by fwd_kv8_step above, the fp8 counterpart of the two 16-bit cache steps (its refusals, append, rotary pass and read).
// The MLA shape over that cache (head_size <= 64 beside head_size_v in [256, 512], qv optional) is read by fwd_qv8 (fa_fwd_qv8).
// `pack_gqa` is a hint too: True asks every route below for the pk kernel (FA_FLAG_PACK_GQA: honoured for GQA / MQA calls of
// 16-bit types at head dims <= 128 without attention_chunk, a V head dim of its own or qv; a no-op elsewhere and behind the
// single-token GQA swap); False and None keep the unpacked routes (no automatic rule yet).
// (`sink`, `cute`: the cute surface, below -- its learnable sink, and num_splits honoured on the dense route too)
std::tuple<Tensor, Tensor, OptTensor, OptTensor> fa3_fwd_core(
        const Tensor &q, const Tensor &k, const Tensor &v, const OptTensor &k_new, const OptTensor &v_new, const OptTensor &qv,
        const OptTensor &out_, const OptTensor &cu_seqlens_q, const OptTensor &cu_seqlens_k, const OptTensor &cu_seqlens_k_new,
        const OptTensor &seqused_q, const OptTensor &seqused_k, c10::optional<int64_t> max_seqlen_q_,
        c10::optional<int64_t> max_seqlen_k_, const OptTensor &page_table, const OptTensor &kv_batch_idx,
        const OptTensor &leftpad_k, const OptTensor &rotary_cos, const OptTensor &rotary_sin, OptTensor seqlens_rotary,
        const OptTensor &q_descale, const OptTensor &k_descale, const OptTensor &v_descale, c10::optional<double> softmax_scale_,
        bool is_causal, int64_t window_size_left, int64_t window_size_right, c10::optional<int64_t> attention_chunk_,
        double softcap, bool is_rotary_interleaved, const OptTensor & /*scheduler_metadata*/, int64_t num_splits,
        c10::optional<bool> pack_gqa_, int64_t /*sm_margin*/, const OptTensor &sink, bool cute) {
    const bool pack_gqa = pack_gqa_.value_or(false);
    const auto q_dtype = q.scalar_type();
    const bool is_fp8 = q_dtype == at::kFloat8_e4m3fn;
    TORCH_CHECK(q_dtype == at::kHalf || q_dtype == at::kBFloat16 || is_fp8,
                "FlashAttention only supports fp16, bf16, and fp8_e4m3 data type");  // hopper/flash_api.cpp:714-722
    if (!is_fp8 && k.scalar_type() == at::kFloat8_e4m3fn && v.scalar_type() == at::kFloat8_e4m3fn) {
        // 16-bit queries over an fp8 KV cache: the kv8 step (what it does not serve is refused by argument there)
        auto r = fwd_kv8_step(q, k, v, k_new, v_new, qv, out_, cu_seqlens_q, cu_seqlens_k, cu_seqlens_k_new, seqused_q, seqused_k,
                              max_seqlen_q_, page_table, kv_batch_idx, leftpad_k, rotary_cos, rotary_sin, seqlens_rotary, k_descale,
                              v_descale, softmax_scale_.value_or(std::pow(double(q.size(-1) + (qv.has_value() ? v.size(-1) : 0)), -0.5)), is_causal,
                              window_size_left,
                              window_size_right, attention_chunk_.value_or(0), softcap, is_rotary_interleaved, num_splits, sink);
        return {std::get<0>(r), std::get<1>(r), c10::nullopt, c10::nullopt};
    }
    TORCH_CHECK(k.scalar_type() == q_dtype, "query and key must have the same dtype");
    TORCH_CHECK(v.scalar_type() == q_dtype, "query and value must have the same dtype");
    CHECK_DEVICE(q, "q"); CHECK_LAST_CONTIGUOUS(q, "Input tensor must have contiguous last dimension");
    CHECK_DEVICE(k, "k"); CHECK_LAST_CONTIGUOUS(k, "Input tensor must have contiguous last dimension");
    CHECK_DEVICE(v, "v"); CHECK_LAST_CONTIGUOUS(v, "Input tensor must have contiguous last dimension");
    TORCH_CHECK(!cu_seqlens_k_new.has_value() || cu_seqlens_q.has_value(),
                "This flash attention build does not support cu_seqlens_k_new without cu_seqlens_q.");
    const int64_t attention_chunk = attention_chunk_.value_or(0);
    TORCH_CHECK(attention_chunk >= 0, "attention_chunk must be non-negative");
    const int64_t head_size = q.size(-1), head_size_v = v.size(-1);  // :764
    // MLA shape (:783-792, 1028-1048): q/k <= 64 beside a V head dim in [256, 512] -- the qv kernel's
    const bool wide_v = head_size <= 64 && head_size_v >= 256 && head_size_v <= 512 && head_size_v % 8 == 0 && !is_fp8;
    std::vector<int64_t> out_shape = q.sizes().vec();  // q's with V's head dim
    out_shape.back() = head_size_v;
    if (qv.has_value()) {
        TORCH_CHECK(wide_v, "This flash attention build does not support qv here: q_v is only supported for head_size <= 64 "
                            "and hdim_v >= 256 (<= 512), with fp16 / bf16 inputs");
        TORCH_CHECK(qv->scalar_type() == q_dtype, "q_v must have the same dtype as query");
        TORCH_CHECK(qv->is_cuda() && qv->device() == q.device(), "q_v must be on the same CUDA device as query");
        CHECK_LAST_CONTIGUOUS(*qv, "q_v tensor must have contiguous last dimension");
        TORCH_CHECK(qv->sizes() == c10::IntArrayRef(out_shape), "q_v must have shape ", tuple_str(out_shape));
    }
    if (head_size_v != head_size) {  // :782-792 (the "Only Hopper" line is the one check that does not carry over)
        TORCH_CHECK((head_size > 128 && head_size <= 192 && head_size_v > 96 && head_size_v <= 128) ||
                        (head_size <= 64 && head_size_v <= 512),
                    "If V headdim is different from Q/K dim, we only support Q/K headdim in (128, 192] and V headdim in (96, 128], "
                    "or (Q/K <= 64 and V <= 512).");
        TORCH_CHECK(!is_fp8, "This flash attention build does not support a V headdim of its own with fp8 inputs.");
        TORCH_CHECK(head_size_v % 8 == 0, "head_size_v should be a multiple of 8");  // :856
    }
    if (seqlens_rotary.has_value()) {  // :1074-1079; only read together with k_new + rotary (hopper/seqlen.h:89)
        check_seqlens_rotary(*seqlens_rotary, cu_seqlens_q.has_value() ? cu_seqlens_q->numel() - 1 : q.size(0));
        if (!k_new.has_value() || !rotary_cos.has_value()) seqlens_rotary = c10::nullopt;
    }
    const double default_scale = std::pow(double(head_size + (qv.has_value() ? head_size_v : 0)), -0.5);
    // (ragged queries over a 4-D cache with its fill levels are a KV-cache step with or without any of the other arguments)
    const bool ragged_cache = cu_seqlens_q.has_value() && !cu_seqlens_k.has_value() && seqused_k.has_value() && k.dim() == 4;
    if (k_new || v_new || page_table || kv_batch_idx || leftpad_k || rotary_cos || rotary_sin || ragged_cache) {
        // KV-cache step (:736-760, 935-1060): k / v are the cache, seqused_k its fill levels
        TORCH_CHECK(!cu_seqlens_k, "This flash attention build does not support KV-cache arguments together with cu_seqlens_k.");
        TORCH_CHECK(cu_seqlens_q.has_value() || !seqused_q,
                    "This flash attention build does not support KV-cache arguments together with seqused_q without cu_seqlens_q.");
        TORCH_CHECK(!is_fp8, "This flash attention build does not support KV-cache arguments with fp8 inputs.");
        TORCH_CHECK(!attention_chunk && (head_size_v == head_size || wide_v),
                    "This flash attention build does not support attention_chunk or a V headdim of its own with KV-cache "
                    "arguments (except Q/K <= 64 beside V in [256, 512]).");
        TORCH_CHECK(k_new.has_value() == v_new.has_value(), "k_new and v_new must be passed together");
        TORCH_CHECK(rotary_cos.has_value() == rotary_sin.has_value(), "rotary_cos and rotary_sin must be passed together");
        if (k_new || leftpad_k) TORCH_CHECK(seqused_k.has_value(), "seqused_k must be provided with k_new / leftpad_k");
        if (cu_seqlens_q.has_value()) {  // ragged queries: one continuous-batching step
            auto r = fwd_kvcache_ragged(q, k, v, k_new, v_new, qv, out_, *cu_seqlens_q, cu_seqlens_k_new, seqused_q, seqused_k,
                                        max_seqlen_q_.value_or(-1), page_table, kv_batch_idx, leftpad_k, rotary_cos, rotary_sin,
                                        seqlens_rotary, softmax_scale_.value_or(default_scale), is_causal, window_size_left,
                                        window_size_right, softcap, is_rotary_interleaved, num_splits, sink, pack_gqa);
            return {std::get<0>(r), std::get<1>(r), c10::nullopt, c10::nullopt};
        }
        KvcacheArgs a;
        a.k_new = k_new; a.v_new = v_new; a.seqlens_k = seqused_k; a.rotary_cos = rotary_cos; a.rotary_sin = rotary_sin;
        a.cache_batch_idx = kv_batch_idx; a.leftpad_k = leftpad_k; a.block_table = page_table; a.out = out_;
        a.softmax_scale = softmax_scale_.value_or(default_scale); a.is_causal = is_causal; a.window_size_left = window_size_left;
        a.window_size_right = window_size_right; a.softcap = softcap; a.is_rotary_interleaved = is_rotary_interleaved;
        a.num_splits = num_splits; a.seqlens_rotary = seqlens_rotary; a.qv = qv; a.sink = sink; a.pack_gqa = pack_gqa;
        auto r = fwd_kvcache_core(q, k, v, a);
        return {r[0], r[1], c10::nullopt, c10::nullopt};
    }
    if (!cu_seqlens_q && !cu_seqlens_k && !seqused_q && seqused_k && !is_fp8 && q.dim() == 4 && q.size(1) <= 128 &&
        window_size_left < 0 && (window_size_right < 0 || is_causal) && !out_ && !attention_chunk &&
        (head_size_v == head_size || wide_v)) {
        // plain decode over a cache (flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=...)): the same routine as
        // the append / paged calls, which brings the split-KV heuristic (num_splits = 0) and the (b, 1, h) -> (b, ngroups, h_k)
        // GQA swap (:935-1060 runs them for every call with seqused_k)
        KvcacheArgs a;
        a.seqlens_k = seqused_k; a.softmax_scale = softmax_scale_.value_or(default_scale); a.is_causal = is_causal; a.softcap = softcap;
        a.num_splits = num_splits; a.qv = qv; a.sink = sink; a.pack_gqa = pack_gqa;
        auto r = fwd_kvcache_core(q, k, v, a);
        return {r[0], r[1], c10::nullopt, c10::nullopt};
    }
    const bool varlen = cu_seqlens_q.has_value();
    TORCH_CHECK(varlen == cu_seqlens_k.has_value(), "This flash attention build needs cu_seqlens_q and cu_seqlens_k together.");
    int64_t batch_size, seqlen_q, seqlen_k, total_q, num_heads, num_heads_k;
    if (varlen) {
        TORCH_CHECK(cu_seqlens_q->scalar_type() == at::kInt && cu_seqlens_k->scalar_type() == at::kInt,
                    "cu_seqlens must have dtype torch.int32");
        TORCH_CHECK(cu_seqlens_q->is_contiguous() && cu_seqlens_k->is_contiguous(), "cu_seqlens must be contiguous");
        TORCH_CHECK(max_seqlen_q_.has_value() && max_seqlen_k_.has_value(), "max_seqlen_q/k must be provided with cu_seqlens");
        TORCH_CHECK(q.dim() == 3, "q must have shape (total_q, num_heads, head_size)");
        total_q = q.size(0); num_heads = q.size(1); num_heads_k = k.size(1);
        batch_size = cu_seqlens_q->numel() - 1;
        seqlen_q = *max_seqlen_q_; seqlen_k = *max_seqlen_k_;
    } else {
        TORCH_CHECK(q.dim() == 4, "q must have shape (batch_size, seqlen_q, num_heads, head_size)");
        batch_size = q.size(0); seqlen_q = q.size(1); num_heads = q.size(2);
        seqlen_k = k.size(1); num_heads_k = k.size(2);
        total_q = batch_size * seqlen_q;
    }
    TORCH_CHECK(batch_size > 0, "batch size must be positive");
    // CHECK_SHAPE(k, ..., num_heads_k, head_size) / CHECK_SHAPE(v, ..., num_heads_k, head_size_v), :813-819
    TORCH_CHECK(k.size(-1) == head_size, "k must have shape (..., ", num_heads_k, ", ", head_size, ")");
    std::vector<int64_t> v_shape = k.sizes().vec();
    v_shape.back() = head_size_v;
    TORCH_CHECK(v.sizes() == c10::IntArrayRef(v_shape), "v must have shape ", tuple_str(v_shape));
    TORCH_CHECK(head_size <= 256, "FlashAttention forward only supports head dimension at most 256");
    TORCH_CHECK(head_size % (is_fp8 ? 16 : 8) == 0, "head_size should be a multiple of ", is_fp8 ? 16 : 8);  // :854-856
    TORCH_CHECK(num_heads_k > 0 && num_heads % num_heads_k == 0,
                "Number of heads in key/value must divide number of heads in query");
    for (const auto &[t, name] : {std::make_pair(&seqused_q, "seqused_q"), std::make_pair(&seqused_k, "seqused_k")})
        if (t->has_value())
            TORCH_CHECK((*t)->scalar_type() == at::kInt && (*t)->is_contiguous() && (*t)->numel() == batch_size, name,
                        " must be int32 of shape (batch_size,)");
    for (const auto &[t, name] : {std::make_pair(&q_descale, "q_descale"), std::make_pair(&k_descale, "k_descale"),
                                  std::make_pair(&v_descale, "v_descale")})
        if (t->has_value()) {
            TORCH_CHECK(is_fp8, name, " is only supported with fp8 inputs");
            TORCH_CHECK((*t)->scalar_type() == at::kFloat && (*t)->sizes() == c10::IntArrayRef({batch_size, num_heads_k}), name,
                        " must be fp32 (batch_size, num_heads_k)");
        }
    const double softmax_scale = softmax_scale_.value_or(default_scale);
    fa3_window(seqlen_q, seqlen_k, window_size_left, window_size_right);  // :796-805
    if (seqlen_q == 1 && window_size_left == -1 && window_size_right == -1 && attention_chunk == 0)
        is_causal = false;  // causal=true is the same as causal=false in this case
    if (is_causal) window_size_right = 0;
    const auto out_dtype = is_fp8 ? at::kBFloat16 : q_dtype;  // :859
    Tensor out;
    if (out_.has_value()) {
        out = *out_;
        TORCH_CHECK(out.scalar_type() == out_dtype,
                    is_fp8 ? "For FP8 input, output must have dtype BF16" : "Output must have the same dtype as inputs");
        TORCH_CHECK(out.is_cuda() && out.stride(-1) == 1 && out.sizes() == c10::IntArrayRef(out_shape),
                    "out must have shape (..., num_heads, head_size_v)");  // :866-870
    } else {
        out = at::empty(out_shape, q.options().dtype(out_dtype));  // :872-874
    }
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(q.device());
    Tensor softmax_lse = varlen ? at::empty({num_heads, total_q}, q.options().dtype(at::kFloat))
                                : at::empty({batch_size, num_heads, seqlen_q}, q.options().dtype(at::kFloat));
    if (seqlen_k > 0 && total_q > 0 && seqlen_q > 0) {
        const Tensor qc = aligned_or_copy(q), kc = aligned_or_copy(k), vc = aligned_or_copy(v);
        const OutPath o(out);
        FwdArgs a;
        a.varlen = varlen; a.batch = batch_size; a.max_seqlen_q = seqlen_q; a.max_seqlen_k = seqlen_k;
        a.softmax_scale = softmax_scale; a.causal = is_causal; a.window_left = window_size_left; a.window_right = window_size_right;
        a.softcap = softcap; a.cu_seqlens_q = cu_seqlens_q; a.cu_seqlens_k = cu_seqlens_k; a.seqused_q = seqused_q;
        a.seqused_k = seqused_k; a.q_descale = q_descale; a.k_descale = k_descale; a.v_descale = v_descale;
        a.fa3_window = true; a.attention_chunk = attention_chunk;
        if (qv.has_value()) a.qv = aligned_or_copy(*qv);
        a.num_splits = cute ? (int)num_splits : 1;  // no split-KV: the decode calls of the FA3 surface take the fwd_kvcache_core routes above
        a.sink = sink; a.pack_gqa = pack_gqa;
        launch_fwd(qc, kc, vc, o.work, softmax_lse, a);
        o.finish();
    } else if (total_q > 0) {  // :1190-1194
        fill_empty(out, softmax_lse, sink, varlen ? std::vector<int64_t>{num_heads, 1} : std::vector<int64_t>{1, num_heads, 1});
    }
    return {out, softmax_lse, c10::nullopt, c10::nullopt};
}

std::tuple<Tensor, Tensor, OptTensor, OptTensor> fa3_fwd(
        const Tensor &q, const Tensor &k, const Tensor &v, const OptTensor &k_new, const OptTensor &v_new, const OptTensor &qv,
        const OptTensor &out_, const OptTensor &cu_seqlens_q, const OptTensor &cu_seqlens_k, const OptTensor &cu_seqlens_k_new,
        const OptTensor &seqused_q, const OptTensor &seqused_k, c10::optional<int64_t> max_seqlen_q_,
        c10::optional<int64_t> max_seqlen_k_, const OptTensor &page_table, const OptTensor &kv_batch_idx,
        const OptTensor &leftpad_k, const OptTensor &rotary_cos, const OptTensor &rotary_sin, OptTensor seqlens_rotary,
        const OptTensor &q_descale, const OptTensor &k_descale, const OptTensor &v_descale, c10::optional<double> softmax_scale_,
        bool is_causal, int64_t window_size_left, int64_t window_size_right, c10::optional<int64_t> attention_chunk_,
        double softcap, bool is_rotary_interleaved, const OptTensor &scheduler_metadata, int64_t num_splits,
        c10::optional<bool> pack_gqa, int64_t sm_margin) {
    return fa3_fwd_core(q, k, v, k_new, v_new, qv, out_, cu_seqlens_q, cu_seqlens_k, cu_seqlens_k_new, seqused_q, seqused_k,
                        max_seqlen_q_, max_seqlen_k_, page_table, kv_batch_idx, leftpad_k, rotary_cos, rotary_sin, seqlens_rotary,
                        q_descale, k_descale, v_descale, softmax_scale_, is_causal, window_size_left, window_size_right,
                        attention_chunk_, softcap, is_rotary_interleaved, scheduler_metadata, num_splits, pack_gqa, sm_margin,
                        c10::nullopt, false);
}

// flash_attn_3::bwd, hopper/flash_api.cpp:1259-1570 (22 arguments of the schema), on the FA2-shaped backward of this build
// (16-bit types).  Returns (dq, dk, dv, softmax_d) and four empty fp32 tensors (softmax_lse_log2, dq/dk/dv_accum: none here).
std::vector<Tensor> fa3_bwd(const Tensor &dout, const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &out,
                            const Tensor &softmax_lse, OptTensor dq_, OptTensor dk_, OptTensor dv_, const OptTensor &cu_seqlens_q,
                            const OptTensor &cu_seqlens_k, const OptTensor &seqused_q, const OptTensor &seqused_k,
                            c10::optional<int64_t> max_seqlen_q, c10::optional<int64_t> max_seqlen_k,
                            c10::optional<double> softmax_scale_, bool is_causal, int64_t window_size_left,
                            int64_t window_size_right, double softcap, bool deterministic, int64_t /*sm_margin*/) {
    TORCH_CHECK(!seqused_q && !seqused_k, "This flash attention build does not support seqused_q / seqused_k in the backward.");
    const bool varlen = cu_seqlens_q.has_value();
    const int64_t d = q.size(-1), d_v = v.size(-1);
    const bool own_dv = d_v != d;
    if (own_dv) {  // v / out / dout / dv carry head_size_v (:1345-1369, 1399-1412, 1462-1464); built for max(d, d_v) in (128, 256]
        TORCH_CHECK(q.scalar_type() == at::kHalf || q.scalar_type() == at::kBFloat16,
                    "FlashAttention only support fp16 and bf16 data type");
        TORCH_CHECK(k.scalar_type() == q.scalar_type(), "query and key must have the same dtype");
        TORCH_CHECK(v.scalar_type() == q.scalar_type(), "query and value must have the same dtype");
        TORCH_CHECK(out.scalar_type() == q.scalar_type(), "query and out must have the same dtype");
        TORCH_CHECK(dout.scalar_type() == q.scalar_type(), "query and dout must have the same dtype");
        TORCH_CHECK(d % 8 == 0, "head_size should be a multiple of 8");
        TORCH_CHECK(d_v % 8 == 0, "head_size_v should be a multiple of 8");
        TORCH_CHECK(std::max(d, d_v) <= 256, "FlashAttention backward only supports head dimension at most 256");
        TORCH_CHECK(std::max(d, d_v) > 128, "This flash attention build supports a V headdim different from the Q/K headdim in "
                                            "the backward only when the larger of the two is above 128.");
        TORCH_CHECK(k.size(-1) == d && v.sizes().slice(0, v.dim() - 1) == k.sizes().slice(0, k.dim() - 1),
                    "k / v shapes do not match");
        std::vector<int64_t> out_shape = q.sizes().vec();
        out_shape.back() = d_v;
        TORCH_CHECK(out.sizes() == c10::IntArrayRef(out_shape) && dout.sizes() == out.sizes(), "out / dout must be (..., head_size_v)");
    }
    const double softmax_scale = softmax_scale_.value_or(std::pow(double(d), -0.5));
    if (varlen) TORCH_CHECK(max_seqlen_q && max_seqlen_k, "max_seqlen_q/k must be provided with cu_seqlens");
    const int64_t sq_max = varlen ? *max_seqlen_q : q.size(1), sk_max = varlen ? *max_seqlen_k : k.size(1);
    fa3_window(sq_max, sk_max, window_size_left, window_size_right);
    if (is_causal) window_size_right = 0;
    std::vector<Tensor> r;
    if (!own_dv) {  // the FA2 entry points' checks and texts, with the FA3 window rule
        OptTensor none;
        if (varlen) {
            TORCH_CHECK(cu_seqlens_k.has_value(), "This flash attention build needs cu_seqlens_q and cu_seqlens_k together.");
            r = mha_varlen_bwd<true>(dout, q, k, v, out, softmax_lse, dq_, dk_, dv_, *cu_seqlens_q, *cu_seqlens_k, none, sq_max,
                                     sk_max, 0.0, softmax_scale, false, is_causal, window_size_left, window_size_right, softcap,
                                     deterministic, c10::nullopt, none);
        } else {
            r = mha_bwd<true>(dout, q, k, v, out, softmax_lse, dq_, dk_, dv_, none, 0.0, softmax_scale, is_causal,
                              window_size_left, window_size_right, softcap, deterministic, c10::nullopt, none);
        }
    } else {
        auto grad = [](const OptTensor &given, const Tensor &like, const char *name) {
            if (!given.has_value()) return at::empty_like(like);
            TORCH_CHECK(given->scalar_type() == like.scalar_type() && given->is_cuda() && given->stride(-1) == 1 &&
                            given->sizes() == like.sizes(), name, " must have the dtype, device and shape of its tensor");
            return *given;
        };
        const Tensor dq = grad(dq_, q, "dq"), dk = grad(dk_, k, "dk"), dv = grad(dv_, v, "dv");
        CHECK_DEVICE(q, "q"); CHECK_DEVICE(k, "k"); CHECK_DEVICE(v, "v"); CHECK_DEVICE(out, "out"); CHECK_DEVICE(dout, "dout");
        CHECK_DEVICE(softmax_lse, "softmax_lse");
        BwdArgs a;
        a.varlen = varlen; a.batch = varlen ? cu_seqlens_q->numel() - 1 : q.size(0); a.max_seqlen_q = sq_max;
        a.max_seqlen_k = sk_max; a.softmax_scale = softmax_scale; a.causal = is_causal; a.window_left = window_size_left;
        a.window_right = window_size_right; a.softcap = softcap; a.cu_seqlens_q = cu_seqlens_q; a.cu_seqlens_k = cu_seqlens_k;
        a.deterministic = deterministic; a.fa3_window = true;
        r = run_bwd(dout, q, k, v, out, softmax_lse, dq, dk, dv, a, q.numel() > 0 && k.numel() > 0);
    }
    for (int i = 0; i < 4; ++i) r.push_back(at::empty({0}, q.options().dtype(at::kFloat)));
    return r;
}

// ---- the cute surface (flash_attn/cute/interface.py:1141-1210): flash_attn_func / flash_attn_varlen_func with learnable_sink ----
// The sink is (num_heads,) bf16 (the reference's) or fp32, on q's device, contiguous; cute_interface.py has the reference's
// checks and texts, these are the ones the launch depends on.
void check_sink(const OptTensor &sink, const Tensor &q) {
    if (!sink.has_value()) return;
    TORCH_CHECK(sink->is_cuda() && sink->device() == q.device(), "inputs must be on CUDA device");
    TORCH_CHECK(sink->scalar_type() == at::kBFloat16 || sink->scalar_type() == at::kFloat, "learnable_sink must be bfloat16 (or float32)");
    TORCH_CHECK(sink->dim() == 1 && sink->size(0) == q.size(-2) && sink->is_contiguous(), "learnable_sink must be contiguous of shape (num_head,)");
}

// Routes like fa3_fwd (KV-cache steps with their GQA swap and split heuristic, ragged queries over a cache, dense, varlen);
// pack_gqa: fa3_fwd_core's hint (True = FA_FLAG_PACK_GQA).  max_seqlen_q / max_seqlen_k are upper bounds the caller derives from shapes (the cute signatures carry none): the grid
// is made from them, the kernels read the lengths on the device.  Returns (out, softmax_lse).
std::tuple<Tensor, Tensor> cute_fwd(const Tensor &q, const Tensor &k, const Tensor &v, const OptTensor &cu_seqlens_q,
                                    const OptTensor &cu_seqlens_k, const OptTensor &seqused_q, const OptTensor &seqused_k,
                                    c10::optional<int64_t> max_seqlen_q, c10::optional<int64_t> max_seqlen_k,
                                    const OptTensor &page_table, c10::optional<double> softmax_scale, bool is_causal,
                                    int64_t window_size_left, int64_t window_size_right, const OptTensor &learnable_sink,
                                    double softcap, int64_t num_splits, c10::optional<bool> pack_gqa) {
    check_sink(learnable_sink, q);
    const OptTensor none;
    auto r = fa3_fwd_core(q, k, v, none, none, none, none, cu_seqlens_q, cu_seqlens_k, none, seqused_q, seqused_k, max_seqlen_q,
                          max_seqlen_k, page_table, none, none, none, none, none, none, none, none, softmax_scale, is_causal,
                          window_size_left, window_size_right, c10::nullopt, softcap, false, none, num_splits, pack_gqa, 0,
                          learnable_sink, true);
    return {std::get<0>(r), std::get<1>(r)};
}

// ---- block-sparse forward of the cute surface (include/fa_fwd.h fa_fwd_block_sparse): flash_attn_func with
// full_block_cnt / full_block_idx / mask_block_cnt / mask_block_idx.  The checks of normalize_block_sparse_tensors
// (flash_attn/cute/block_sparsity.py:33-115) on shapes and dtypes; the lists are handed over through their strides -- a size-1
// batch / head dimension as stride 0 -- and never read, copied or expanded here.  Allocates lse, and out unless the caller passes one (q / k / v
// views whose rows are not 16-byte aligned are copied, as on every surface).
void check_block_list(const OptTensor &cnt, const OptTensor &idx, const char *name, const Tensor &q, int64_t nm, int64_t nk) {
    TORCH_CHECK(cnt.has_value() == idx.has_value(), name, "_block_cnt and ", name, "_block_idx must be specified together");
    if (!cnt.has_value()) return;
    TORCH_CHECK(cnt->scalar_type() == at::kInt && idx->scalar_type() == at::kInt, name, "_block_cnt and ", name, "_block_idx must be int32");
    TORCH_CHECK(cnt->is_cuda() && idx->is_cuda() && cnt->device() == q.device() && idx->device() == q.device(),
                name, "_block_cnt and ", name, "_block_idx must be on the device of q");
    const int64_t b = q.size(0), h = q.size(2);
    TORCH_CHECK(cnt->dim() == 3 && (cnt->size(0) == b || cnt->size(0) == 1) && (cnt->size(1) == h || cnt->size(1) == 1) && cnt->size(2) == nm,
                name, "_block_cnt must have shape (", b, " or 1, ", h, " or 1, ", nm, "), got ", cnt->sizes());
    TORCH_CHECK(idx->dim() == 4 && (idx->size(0) == b || idx->size(0) == 1) && (idx->size(1) == h || idx->size(1) == 1) && idx->size(2) == nm &&
                    idx->size(3) == nk,
                name, "_block_idx must have shape (", b, " or 1, ", h, " or 1, ", nm, ", ", nk, "), got ", idx->sizes());
}
void set_list_strides(const Tensor &t, int64_t (&st)[4]) {
    for (int64_t i = 0; i < 4; ++i) st[i] = i < t.dim() ? t.stride(i) : 0;
    if (t.size(0) == 1) st[0] = 0;  // broadcast over the batch / the heads
    if (t.size(1) == 1) st[1] = 0;
}

std::tuple<Tensor, Tensor> cute_fwd_block_sparse(const Tensor &q_, const Tensor &k_, const Tensor &v_, double softmax_scale, bool is_causal,
                                                 int64_t window_size_left, int64_t window_size_right, const OptTensor &learnable_sink,
                                                 double softcap, int64_t num_splits, const OptTensor &full_block_cnt,
                                                 const OptTensor &full_block_idx, const OptTensor &mask_block_cnt,
                                                 const OptTensor &mask_block_idx, const OptTensor &out_) {
    CHECK_DEVICE(q_, "q"); CHECK_DEVICE(k_, "k"); CHECK_DEVICE(v_, "v");
    TORCH_CHECK(q_.dim() == 4 && k_.dim() == 4 && v_.dim() == 4, "block sparsity needs dense q (b, sq, h, d) and k / v (b, sk, h_k, d)");
    TORCH_CHECK(q_.scalar_type() == at::kHalf || q_.scalar_type() == at::kBFloat16, "inputs must be float16 or bfloat16");
    TORCH_CHECK(k_.scalar_type() == q_.scalar_type() && v_.scalar_type() == q_.scalar_type(), "inputs must have the same dtype");
    CHECK_LAST_CONTIGUOUS(q_, "q must have contiguous last dimension");
    CHECK_LAST_CONTIGUOUS(k_, "k must have contiguous last dimension");
    CHECK_LAST_CONTIGUOUS(v_, "v must have contiguous last dimension");
    const int64_t b = q_.size(0), sq = q_.size(1), h = q_.size(2), d = q_.size(3), sk = k_.size(1), h_k = k_.size(2), dv = v_.size(3);
    TORCH_CHECK(k_.size(0) == b && v_.size(0) == b && v_.size(1) == sk && v_.size(2) == h_k && k_.size(3) == d, "q, k, v shapes do not match");
    TORCH_CHECK(mask_block_cnt.has_value() && mask_block_idx.has_value(), "mask_block_cnt and mask_block_idx are required");
    check_sink(learnable_sink, q_);
    const int64_t nm = (sq + 127) / 128, nk = (sk + 127) / 128;
    check_block_list(mask_block_cnt, mask_block_idx, "mask", q_, nm, nk);
    check_block_list(full_block_cnt, full_block_idx, "full", q_, nm, nk);
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(q_.device());
    const Tensor q = aligned_or_copy(q_), k = aligned_or_copy(k_), v = aligned_or_copy(v_);
    Tensor given;  // the caller's out (as every forward entry point takes one); a view that is not aligned() is filled by a copy
    if (out_.has_value()) {
        given = *out_;
        TORCH_CHECK(given.scalar_type() == q.scalar_type(), "Output must have the same dtype as inputs");
        TORCH_CHECK(given.is_cuda() && given.stride(-1) == 1 && given.sizes() == c10::IntArrayRef({b, sq, h, dv}),
                    "out must have shape (batch_size, seqlen_q, num_head, head_dim_v)");
    } else {
        given = at::empty({b, sq, h, dv}, q.options());
    }
    const OutPath o(given);
    Tensor lse = at::empty({b, h, sq}, q.options().dtype(at::kFloat));

    FwdArgs a;
    a.batch = b; a.max_seqlen_q = sq; a.max_seqlen_k = sk; a.softmax_scale = softmax_scale; a.softcap = softcap; a.causal = is_causal;
    a.window_left = window_size_left; a.window_right = window_size_right;
    a.fa3_window = true;  // a missing window side is unbounded, as on the rest of this surface
    a.num_splits = (int)num_splits;
    const fa_fwd_params p = fill_fwd_params(q, k, v, o.work, lse, a);

    fa_block_sparse_params s{};
    s.abi_version = FA_ABI_VERSION;
    s.struct_size = sizeof(fa_block_sparse_params);
    s.block_m = s.block_n = 128;
    s.mask_block_cnt = static_cast<const int32_t *>(mask_block_cnt->data_ptr());
    s.mask_block_idx = static_cast<const int32_t *>(mask_block_idx->data_ptr());
    set_list_strides(*mask_block_cnt, s.mask_cnt_stride);
    set_list_strides(*mask_block_idx, s.mask_idx_stride);
    if (full_block_cnt.has_value()) {
        s.full_block_cnt = static_cast<const int32_t *>(full_block_cnt->data_ptr());
        s.full_block_idx = static_cast<const int32_t *>(full_block_idx->data_ptr());
        set_list_strides(*full_block_cnt, s.full_cnt_stride);
        set_list_strides(*full_block_idx, s.full_idx_stride);
    }
    fa_sink_params sink{};
    if (learnable_sink.has_value()) sink = fill_sink_params(*learnable_sink);
    const int st = fa_fwd_block_sparse(&p, &s, learnable_sink.has_value() ? &sink : nullptr, current_stream(q));
    TORCH_CHECK(st != FA_ERR_UNSUPPORTED, "fa_fwd_block_sparse: block sparsity does not go with this call (num_splits > 1, or a head dim "
                "of V above 256): ", fa_strerror(st));
    TORCH_CHECK(st == 0, "fa_fwd_block_sparse failed (", st, "): ", fa_strerror(st));
    o.finish();
    return {given, lse};
}

// dsink (num_heads,) fp32 from the LSE of a forward with a sink and the softmax_d of its fa_bwd (include/fa_bwd.h)
Tensor sink_grad(const Tensor &softmax_lse, const Tensor &softmax_d, const Tensor &learnable_sink, const OptTensor &cu_seqlens_q,
                 const OptTensor &seqused_q, int64_t batch, int64_t seqlen_q) {
    TORCH_CHECK(softmax_lse.scalar_type() == at::kFloat && softmax_d.scalar_type() == at::kFloat, "softmax_lse / softmax_d must be fp32");
    TORCH_CHECK(softmax_lse.is_cuda() && softmax_d.is_cuda() && learnable_sink.is_cuda(), "inputs must be on CUDA device");
    TORCH_CHECK(softmax_d.is_contiguous(), "softmax_d must be contiguous");
    const bool varlen = cu_seqlens_q.has_value();
    TORCH_CHECK(softmax_lse.dim() == (varlen ? 2 : 3), "softmax_lse must be (b, h, seqlen_q) or, varlen, (h, total_q)");
    const int64_t h = learnable_sink.size(0);
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(softmax_lse.device());
    const Tensor lse = softmax_lse.is_contiguous() ? softmax_lse : softmax_lse.contiguous();
    Tensor dsink = at::empty({h}, softmax_lse.options());
    fa_sink_grad_params p{};
    p.abi_version = FA_ABI_VERSION;
    p.struct_size = sizeof(fa_sink_grad_params);
    p.softmax_lse = static_cast<const float *>(lse.data_ptr());
    p.softmax_d = static_cast<const float *>(softmax_d.data_ptr());
    p.learnable_sink = learnable_sink.data_ptr();
    p.dsink = static_cast<float *>(dsink.data_ptr());
    p.cu_seqlens_q = static_cast<const int32_t *>(ptr(cu_seqlens_q));
    p.seqused_q = static_cast<const int32_t *>(ptr(seqused_q));
    p.softmax_d_row_len = softmax_d.size(-1);
    p.b = (int32_t)batch; p.seqlen_q = (int32_t)seqlen_q; p.h = (int32_t)h;
    p.total_q = varlen ? (int32_t)lse.size(1) : 0;
    p.sink_dtype = learnable_sink.scalar_type() == at::kFloat ? FA_DTYPE_FP32 : FA_DTYPE_BF16;
    const int st = fa_sink_grad(&p, current_stream(lse));
    TORCH_CHECK(st == 0, "fa_sink_grad failed (", st, "): ", fa_strerror(st));
    return dsink;
}

// The backward of cute_fwd's dense and varlen calls: fa3_bwd as it stands -- the LSE holds the sink, and the sink's column has
// no value -- and, with a sink, its own gradient in the sink's dtype.  Returns (dq, dk, dv, dsink or None).
std::tuple<Tensor, Tensor, Tensor, OptTensor> cute_bwd(const Tensor &dout, const Tensor &q, const Tensor &k, const Tensor &v,
                                                       const Tensor &out, const Tensor &softmax_lse, const OptTensor &cu_seqlens_q,
                                                       const OptTensor &cu_seqlens_k, c10::optional<int64_t> max_seqlen_q,
                                                       c10::optional<int64_t> max_seqlen_k, c10::optional<double> softmax_scale,
                                                       bool is_causal, int64_t window_size_left, int64_t window_size_right,
                                                       double softcap, const OptTensor &learnable_sink) {
    check_sink(learnable_sink, q);
    const OptTensor none;
    auto r = fa3_bwd(dout, q, k, v, out, softmax_lse, none, none, none, cu_seqlens_q, cu_seqlens_k, none, none, max_seqlen_q,
                     max_seqlen_k, softmax_scale, is_causal, window_size_left, window_size_right, softcap, true, 0);
    OptTensor dsink;
    if (learnable_sink.has_value()) {
        const bool varlen = cu_seqlens_q.has_value();
        const int64_t batch = varlen ? cu_seqlens_q->numel() - 1 : q.size(0);
        if (q.numel() > 0)
            dsink = sink_grad(softmax_lse, r[3], *learnable_sink, cu_seqlens_q, none, batch, varlen ? 0 : q.size(1)).to(learnable_sink->scalar_type());
        else
            dsink = at::zeros_like(*learnable_sink);
    }
    return {r[0], r[1], r[2], dsink};
}

// The backward of cute_fwd_block_sparse (include/fa_bwd.h fa_bwd_block_sparse): the forward's four lists for the dQ sweep and
// the caller's key-major lists q_block_cnt (b | 1, h | 1, nk) / q_block_idx (b | 1, h | 1, nk, nm) for the dK / dV sweep, all
// handed over through their strides and never read here.  With a sink, its gradient from the LSE and the D this call wrote.
// Returns (dq, dk, dv, dsink or None).
std::tuple<Tensor, Tensor, Tensor, OptTensor> cute_bwd_block_sparse(
    const Tensor &dout_, const Tensor &q_, const Tensor &k_, const Tensor &v_, const Tensor &out_, const Tensor &softmax_lse,
    double softmax_scale, bool is_causal, int64_t window_size_left, int64_t window_size_right, double softcap,
    const OptTensor &learnable_sink, const OptTensor &full_block_cnt, const OptTensor &full_block_idx,
    const OptTensor &mask_block_cnt, const OptTensor &mask_block_idx, const OptTensor &q_block_cnt, const OptTensor &q_block_idx) {
    CHECK_DEVICE(q_, "q"); CHECK_DEVICE(k_, "k"); CHECK_DEVICE(v_, "v"); CHECK_DEVICE(out_, "out"); CHECK_DEVICE(dout_, "dout");
    CHECK_DEVICE(softmax_lse, "softmax_lse");
    TORCH_CHECK(q_.dim() == 4 && k_.dim() == 4 && v_.dim() == 4, "block sparsity needs dense q (b, sq, h, d) and k / v (b, sk, h_k, d)");
    bwd_common_checks(dout_, q_, k_, v_, out_, softmax_lse);
    const int64_t b = q_.size(0), sq = q_.size(1), h = q_.size(2), d = q_.size(3), sk = k_.size(1), h_k = k_.size(2);
    TORCH_CHECK(d <= 128 && v_.size(3) == d, "the block-sparse backward supports head dims up to 128 with the same head dim for V");
    TORCH_CHECK(k_.size(0) == b && k_.size(3) == d && v_.sizes() == k_.sizes() && out_.sizes() == q_.sizes() && dout_.sizes() == q_.sizes(),
                "q, k, v, out, dout shapes do not match");
    TORCH_CHECK(softmax_lse.scalar_type() == at::kFloat && softmax_lse.dim() == 3 && softmax_lse.size(0) == b &&
                    softmax_lse.size(1) == h && softmax_lse.size(2) == sq, "softmax_lse must be fp32 (b, h, seqlen_q)");
    TORCH_CHECK(mask_block_cnt.has_value() && mask_block_idx.has_value(), "mask_block_cnt and mask_block_idx are required");
    TORCH_CHECK(q_block_cnt.has_value() && q_block_idx.has_value(), "q_block_cnt and q_block_idx are required");
    check_sink(learnable_sink, q_);
    const int64_t nm = (sq + 127) / 128, nk = (sk + 127) / 128;
    check_block_list(mask_block_cnt, mask_block_idx, "mask", q_, nm, nk);
    check_block_list(full_block_cnt, full_block_idx, "full", q_, nm, nk);
    check_block_list(q_block_cnt, q_block_idx, "q", q_, nk, nm);
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(q_.device());
    const Tensor dout = aligned_or_copy(dout_), q = aligned_or_copy(q_), k = aligned_or_copy(k_), v = aligned_or_copy(v_),
                 out = aligned_or_copy(out_);
    const Tensor lse = softmax_lse.is_contiguous() ? softmax_lse : softmax_lse.contiguous();
    Tensor dq = at::empty_like(q, at::MemoryFormat::Contiguous), dk = at::empty_like(k, at::MemoryFormat::Contiguous),
           dv = at::empty_like(v, at::MemoryFormat::Contiguous);
    Tensor softmax_d = at::empty({b, h, round128(sq)}, q.options().dtype(at::kFloat));
    OptTensor dsink;
    if (q.numel() == 0 || k.numel() == 0) {
        dq.zero_(); dk.zero_(); dv.zero_();
        if (learnable_sink.has_value()) dsink = at::zeros_like(*learnable_sink);
        return {dq, dk, dv, dsink};
    }
    BwdArgs a;
    a.batch = b; a.max_seqlen_q = sq; a.max_seqlen_k = sk; a.softmax_scale = softmax_scale; a.causal = is_causal;
    a.window_left = window_size_left; a.window_right = window_size_right; a.softcap = softcap; a.deterministic = true;
    a.fa3_window = true;  // a missing window side is unbounded, as in the forward
    const fa_bwd_params p = fill_bwd_params(dout, q, k, v, out, lse, dq, dk, dv, softmax_d, a);

    fa_block_sparse_params s{};
    s.abi_version = FA_ABI_VERSION;
    s.struct_size = sizeof(fa_block_sparse_params);
    s.block_m = s.block_n = 128;
    s.mask_block_cnt = static_cast<const int32_t *>(mask_block_cnt->data_ptr());
    s.mask_block_idx = static_cast<const int32_t *>(mask_block_idx->data_ptr());
    set_list_strides(*mask_block_cnt, s.mask_cnt_stride);
    set_list_strides(*mask_block_idx, s.mask_idx_stride);
    if (full_block_cnt.has_value()) {
        s.full_block_cnt = static_cast<const int32_t *>(full_block_cnt->data_ptr());
        s.full_block_idx = static_cast<const int32_t *>(full_block_idx->data_ptr());
        set_list_strides(*full_block_cnt, s.full_cnt_stride);
        set_list_strides(*full_block_idx, s.full_idx_stride);
    }
    fa_block_sparse_bwd_params kl{};
    kl.abi_version = FA_ABI_VERSION;
    kl.struct_size = sizeof(fa_block_sparse_bwd_params);
    kl.block_m = kl.block_n = 128;
    kl.q_block_cnt = static_cast<const int32_t *>(q_block_cnt->data_ptr());
    kl.q_block_idx = static_cast<const int32_t *>(q_block_idx->data_ptr());
    set_list_strides(*q_block_cnt, kl.q_cnt_stride);
    set_list_strides(*q_block_idx, kl.q_idx_stride);
    const int st = fa_bwd_block_sparse(&p, &s, &kl, current_stream(q));
    TORCH_CHECK(st == 0, "fa_bwd_block_sparse failed (", st, "): ", fa_strerror(st));
    if (learnable_sink.has_value()) {
        const OptTensor none;
        dsink = sink_grad(lse, softmax_d, *learnable_sink, none, none, b, sq).to(learnable_sink->scalar_type());
    }
    return {dq, dk, dv, dsink};
}

// flash_attn_3::fwd_combine, hopper/flash_api.cpp:1569-1670: merge caller-held split-KV partials.  out_partial
// (num_splits, b, seqlen, h, d) fp32, lse_partial (num_splits, b, seqlen, h) fp32 -> (out, softmax_lse (b, seqlen, h)).
std::tuple<Tensor, Tensor> fa3_fwd_combine(const Tensor &out_partial, const Tensor &lse_partial, const OptTensor &out_,
                                           c10::optional<at::ScalarType> out_dtype) {
    TORCH_CHECK(out_partial.scalar_type() == at::kFloat, "Attention combine function only support fp32 data type");
    TORCH_CHECK(lse_partial.scalar_type() == at::kFloat, "Attention combine function only support fp32 data type");
    TORCH_CHECK(out_partial.is_cuda() && lse_partial.is_cuda(), "out_partial must be on CUDA");
    CHECK_LAST_CONTIGUOUS(out_partial, "Input tensor must have contiguous last dimension");
    TORCH_CHECK(lse_partial.stride(-2) == 1, "LSE tensor must be contiguous in the seqlen dimension");
    TORCH_CHECK(out_partial.dim() == 5, "out_partial must have shape (num_splits, batch_size, seqlen, num_heads, head_size)");
    const int64_t num_splits = out_partial.size(0), batch_size = out_partial.size(1), seqlen = out_partial.size(2),
                  num_heads = out_partial.size(3), head_size = out_partial.size(4);
    TORCH_CHECK(num_splits <= 256, "FlashAttention combine only supports num_splits at most 256");
    CHECK_SHAPE(lse_partial, "lse_partial", num_splits, batch_size, seqlen, num_heads);
    const auto out_type = out_dtype.value_or(out_partial.scalar_type());
    TORCH_CHECK(out_type == at::kFloat || out_type == at::kHalf || out_type == at::kBFloat16,
                "Output type must be FP32, FP16 or BF16");
    Tensor out;
    if (out_.has_value()) {
        out = *out_;
        TORCH_CHECK(out.scalar_type() == out_type, "out must have the requested output type");
        CHECK_DEVICE(out, "out");
        TORCH_CHECK(out.stride(-1) == 1, "Output tensor must have contiguous last dimension");
        CHECK_SHAPE(out, "out", batch_size, seqlen, num_heads, head_size);
    } else {
        out = at::empty({batch_size, seqlen, num_heads, head_size}, out_partial.options().dtype(out_type));
    }
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(out_partial.device());
    Tensor softmax_lse = at::empty({batch_size, num_heads, seqlen}, out_partial.options()).transpose(1, 2);  // (:1632)
    if (seqlen > 0 && batch_size > 0) {
        fa_combine_params p{};
        p.abi_version = FA_ABI_VERSION;
        p.struct_size = sizeof(fa_combine_params);
        p.out_partial = static_cast<const float *>(out_partial.data_ptr());
        p.lse_partial = static_cast<const float *>(lse_partial.data_ptr());
        p.out = out.data_ptr(); p.softmax_lse = static_cast<float *>(softmax_lse.data_ptr());
        p.op_split_stride = out_partial.stride(0); p.op_batch_stride = out_partial.stride(1);
        p.op_row_stride = out_partial.stride(2); p.op_head_stride = out_partial.stride(3);
        p.lp_split_stride = lse_partial.stride(0); p.lp_batch_stride = lse_partial.stride(1);
        p.lp_row_stride = lse_partial.stride(2); p.lp_head_stride = lse_partial.stride(3);
        p.o_batch_stride = out.stride(0); p.o_row_stride = out.stride(1); p.o_head_stride = out.stride(2);
        p.lse_batch_stride = softmax_lse.stride(0); p.lse_row_stride = softmax_lse.stride(1); p.lse_head_stride = softmax_lse.stride(2);
        p.num_splits = (int32_t)num_splits; p.b = (int32_t)batch_size; p.seqlen = (int32_t)seqlen; p.h = (int32_t)num_heads;
        p.d = (int32_t)head_size;
        p.out_dtype = out_type == at::kFloat ? FA_DTYPE_FP32 : dtype_code(out);
        const int st = fa_fwd_combine(&p, current_stream(out));
        TORCH_CHECK(st == 0, "fa_fwd_combine failed (", st, "): ", fa_strerror(st));
    }
    return {out, softmax_lse};
}

// The rotary embedding layer (flash_attn.layers.rotary -> apply_rotary, flash_attn/ops/triton/rotary.py:102-185): x (b, s, h, d), or
// (total, h, d) with cu_seqlens and max_seqlen; cos / sin (seqlen_ro, rotary_dim / 2); seqlen_offsets an int or a (b) tensor of
// int32 / int64 that stays on the device.  One launch on the current stream, no synchronisation, nothing allocated but `out`
// (x itself with inplace): capturable in a HIP graph.  conjugate: the gradient of the rotation.
Tensor rotary_emb(const Tensor &x, const Tensor &cos_, const Tensor &sin_, const std::variant<Tensor, int64_t> &seqlen_offsets,
                  const OptTensor &cu_seqlens_, c10::optional<int64_t> max_seqlen, bool interleaved, bool inplace, bool conjugate) {
    CHECK_DEVICE(x, "x"); CHECK_DEVICE(cos_, "cos"); CHECK_DEVICE(sin_, "sin");
    const auto type = x.scalar_type();
    TORCH_CHECK(type == at::kHalf || type == at::kBFloat16 || type == at::kFloat, "rotary_emb only supports fp16, bf16 and fp32 x");
    const bool varlen = cu_seqlens_.has_value();
    int64_t batch, seqlen;
    Tensor cu_seqlens;
    if (!varlen) {
        TORCH_CHECK(x.dim() == 4, "x must have shape (batch, seqlen, nheads, headdim)");
        batch = x.size(0); seqlen = x.size(1);
    } else {
        TORCH_CHECK(max_seqlen.has_value(), "If cu_seqlens is passed in, then max_seqlen must be passed");
        TORCH_CHECK(x.dim() == 3, "x must have shape (total_seqlen, nheads, headdim) with cu_seqlens");
        CHECK_DEVICE(*cu_seqlens_, "cu_seqlens");
        TORCH_CHECK(cu_seqlens_->scalar_type() == at::kInt && cu_seqlens_->dim() == 1 && cu_seqlens_->numel() >= 1,
                    "cu_seqlens must be an int32 tensor of shape (batch + 1)");
        cu_seqlens = cu_seqlens_->contiguous();
        batch = cu_seqlens.numel() - 1; seqlen = *max_seqlen;
        TORCH_CHECK(seqlen > 0, "max_seqlen must be positive");
    }
    const int64_t nheads = x.size(-2), headdim = x.size(-1);
    TORCH_CHECK(cos_.dim() == 2, "cos must have shape (seqlen_ro, rotary_dim / 2)");
    TORCH_CHECK(sin_.sizes() == cos_.sizes(), "sin must have the shape of cos");
    TORCH_CHECK(cos_.scalar_type() == sin_.scalar_type(), "cos and sin must have the same dtype");
    TORCH_CHECK(cos_.scalar_type() == type || cos_.scalar_type() == at::kFloat, "cos and sin must have the dtype of x or fp32");
    const int64_t seqlen_ro = cos_.size(0), rotary_dim = 2 * cos_.size(1);
    TORCH_CHECK(rotary_dim > 0, "rotary_dim must be positive");
    TORCH_CHECK(rotary_dim <= headdim, "rotary_dim must be <= headdim");
    TORCH_CHECK(headdim <= 256, "Only support headdim <= 256");
    TORCH_CHECK(seqlen_ro >= seqlen, "seqlen_ro must be >= seqlen");
    TORCH_CHECK(x.numel() == 0 || (batch <= INT32_MAX && seqlen <= INT32_MAX && x.size(0) <= INT32_MAX && nheads <= INT32_MAX &&
                                   seqlen_ro <= INT32_MAX), "rotary_emb: a dimension of 2^31 or more");
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(x.device());
    const Tensor cos = cos_.contiguous(), sin = sin_.contiguous();
    Tensor offsets;
    fa_rotary_emb_params p{};
    if (const Tensor *t = std::get_if<Tensor>(&seqlen_offsets)) {
        CHECK_DEVICE(*t, "seqlen_offsets");
        TORCH_CHECK(t->dim() == 1 && t->size(0) == batch, "seqlen_offsets must have shape (batch)");
        TORCH_CHECK(t->scalar_type() == at::kInt || t->scalar_type() == at::kLong, "seqlen_offsets must have dtype int32 or int64");
        offsets = t->contiguous();
        p.seqlen_offsets = offsets.data_ptr();
        p.offsets_int64 = offsets.scalar_type() == at::kLong ? 1 : 0;
    } else {
        p.seqlen_offset = std::get<int64_t>(seqlen_offsets);
        TORCH_CHECK(p.seqlen_offset + seqlen <= seqlen_ro, "seqlen_offsets + seqlen must be <= seqlen_ro");
    }
    Tensor out = inplace ? x : at::empty_like(x);
    if (x.numel() == 0) return out;
    p.abi_version = FA_ABI_VERSION;
    p.struct_size = sizeof(fa_rotary_emb_params);
    p.x = x.data_ptr(); p.out = out.data_ptr();
    p.x_batch_stride = varlen ? 0 : x.stride(0); p.out_batch_stride = varlen ? 0 : out.stride(0);
    p.x_row_stride = x.stride(-3); p.x_head_stride = x.stride(-2); p.x_dim_stride = x.stride(-1);
    p.out_row_stride = out.stride(-3); p.out_head_stride = out.stride(-2); p.out_dim_stride = out.stride(-1);
    p.cos = cos.data_ptr(); p.sin = sin.data_ptr();
    p.cu_seqlens = varlen ? static_cast<const int32_t *>(cu_seqlens.data_ptr()) : nullptr;
    p.b = (int32_t)batch; p.seqlen = varlen ? 0 : (int32_t)seqlen; p.total = varlen ? (int32_t)x.size(0) : 0;
    p.max_seqlen = varlen ? (int32_t)seqlen : 0;
    p.h = (int32_t)nheads; p.d = (int32_t)headdim; p.rotary_dim = (int32_t)rotary_dim; p.seqlen_ro = (int32_t)seqlen_ro;
    p.dtype = type == at::kFloat ? FA_DTYPE_FP32 : dtype_code(x);
    p.cos_dtype = p.sin_dtype = cos.scalar_type() == at::kFloat ? FA_DTYPE_FP32 : dtype_code(cos);
    p.interleaved = interleaved ? 1 : 0; p.conjugate = conjugate ? 1 : 0;
    const int st = fa_rotary_emb(&p, current_stream(x));
    TORCH_CHECK(st == 0, "fa_rotary_emb failed (", st, "): ", fa_strerror(st));
    return out;
}

// ---- fused residual-add + LayerNorm / RMSNorm (flash_attn.ops.triton.layer_norm -> _layer_norm_fwd_impl / _layer_norm_bwd_impl,
// flash_attn/ops/triton/layer_norm.py:355-468, 702-843, without dropout and the parallel form).  Launches on the current stream,
// no synchronisation; mean / rstd, the gradients and the workspace come from the caching allocator: capturable in a HIP graph.
// The dtype code of a tensor of the row operators (norm, cross-entropy, activations, GEMM + activation), and the shape checks
// they share; `prefix` is the operator's name as its messages start
int row_dtype_code(const char *prefix, at::ScalarType t, const char *what, bool fp32 = true) {
    if (t == at::kHalf) return FA_DTYPE_FP16;
    if (t == at::kBFloat16) return FA_DTYPE_BF16;
    if (t == at::kFloat && fp32) return FA_DTYPE_FP32;
    TORCH_CHECK(false, prefix, what, fp32 ? " must be fp16, bf16 or fp32" : " must be fp16 or bf16");
    return -1;
}

at::ScalarType norm_scalar_type(int64_t code) {
    TORCH_CHECK(code == FA_DTYPE_FP16 || code == FA_DTYPE_BF16 || code == FA_DTYPE_FP32, "layer_norm: unknown dtype code");
    return code == FA_DTYPE_FP16 ? at::kHalf : code == FA_DTYPE_BF16 ? at::kBFloat16 : at::kFloat;
}

void check_rows(const char *prefix, const char *shape, const Tensor &t, const char *name, int64_t M, int64_t N) {
    TORCH_CHECK(t.is_cuda(), prefix, name, " must be on CUDA");
    TORCH_CHECK(t.dim() == 2 && t.size(0) == M && t.size(1) == N, prefix, name, " must have shape ", shape);
    TORCH_CHECK(t.stride(-1) == 1, prefix, name, " must have contiguous last dimension");
}

void check_vector(const char *prefix, const Tensor &t, const char *name, int64_t n, const char *shape, bool contiguous = true) {
    TORCH_CHECK(t.is_cuda(), prefix, name, " must be on CUDA");
    TORCH_CHECK(t.dim() == 1 && t.size(0) == n, prefix, name, " must have shape ", shape);
    TORCH_CHECK(!contiguous || t.is_contiguous(), prefix, name, " must be contiguous");
}

void check_norm_width(const Tensor &x) {
    TORCH_CHECK_WITH(Error, x.size(1) * x.element_size() <= FA_NORM_MAX_ROW_BYTES, "This layer norm doesn't support feature dim >= 64KB.");
    TORCH_CHECK(x.size(1) >= 1, "layer_norm: the feature dim must be at least 1");
}

// what every X_impl below is made with.  X_impl(args..., plan *) is the one definition of a row operator: with plan == nullptr
// it launches, with a plan it allocates and fills the params as for the launch and only asks the C entry point for the form.
// def_row_op (before the module, below) makes the module's `X` and `X_plan` of it
template <class P> P new_params() {
    P p{};
    p.abi_version = FA_ABI_VERSION;
    p.struct_size = sizeof(P);
    return p;
}

// the launch on the current stream of `on`, or with `plan` the form; `name`: the C entry point of the launch
template <class P, class Plan>
void launch_or_plan(const char *name, int (*launch)(const P *, void *), int (*form)(const P *, Plan *), const P &p, Plan *plan,
                    const Tensor &on) {
    const int st = plan ? form(&p, plan) : launch(&p, current_stream(on));
    TORCH_CHECK(st == 0, name, plan ? "_plan" : "", " failed (", st, "): ", fa_strerror(st));
}

// the placeholder of an output there is none of (one tensor each: outputs of an op do not alias)
Tensor none(const at::TensorOptions &options) { return at::empty({0}, options); }

// a plan struct (all int32_t fields, as the _lib.Fa*Plan mirrors have them) as a dict in the order of `names`, its fields
template <class Plan, size_t N> py::dict plan_dict(const Plan &plan, const char *const (&names)[N]) {
    static_assert(sizeof(Plan) == N * sizeof(int32_t), "a field was added to the plan struct and not to its list of names");
    int32_t fields[N];
    std::memcpy(fields, &plan, sizeof(fields));
    py::dict d;
    for (size_t i = 0; i < N; ++i) d[names[i]] = fields[i];
    return d;
}

py::dict norm_plan_dict(const fa_norm_plan &l) {
    return plan_dict(l, {"cw", "threads", "team_wave", "wide", "rows_per_wg", "grid_x", "grid_y"});
}

// y and (optionally) residual_out are written in place; returns (mean, rstd), mean empty with is_rms_norm.  With `plan` nothing
// is launched: the params are filled as for the launch and *plan is what fa_norm_fwd_plan says of them
std::tuple<Tensor, Tensor> norm_fwd_impl(const Tensor &x, const Tensor &weight, const OptTensor &bias, const OptTensor &residual,
                                         const OptTensor &rowscale, Tensor out, OptTensor residual_out, double eps,
                                         bool zero_centered_weight, bool is_rms_norm, fa_norm_plan *plan) {
    TORCH_CHECK(x.is_cuda(), "layer_norm: x must be on CUDA");
    TORCH_CHECK(x.dim() == 2, "layer_norm: x must have shape (M, N)");
    const int64_t M = x.size(0), N = x.size(1);
    check_rows("layer_norm: ", "(M, N)", x, "x", M, N);
    check_rows("layer_norm: ", "(M, N)", out, "out", M, N);
    check_vector("layer_norm: ", weight, "weight", N, "(N)");
    if (bias.has_value()) check_vector("layer_norm: ", *bias, "bias", N, "(N)");
    if (residual.has_value()) check_rows("layer_norm: ", "(M, N)", *residual, "residual", M, N);
    if (residual_out.has_value()) check_rows("layer_norm: ", "(M, N)", *residual_out, "residual_out", M, N);
    if (rowscale.has_value()) check_vector("layer_norm: ", *rowscale, "rowscale", M, "(M)");
    check_norm_width(x);
    auto p = new_params<fa_norm_fwd_params>();
    p.x_dtype = row_dtype_code("layer_norm: ", x.scalar_type(), "x");
    p.weight_dtype = row_dtype_code("layer_norm: ", weight.scalar_type(), "weight");
    p.y_dtype = row_dtype_code("layer_norm: ", out.scalar_type(), "out");
    p.bias_dtype = bias.has_value() ? row_dtype_code("layer_norm: ", bias->scalar_type(), "bias") : p.weight_dtype;
    p.residual_dtype = residual.has_value() ? row_dtype_code("layer_norm: ", residual->scalar_type(), "residual") : p.x_dtype;
    p.residual_out_dtype = residual_out.has_value() ? row_dtype_code("layer_norm: ", residual_out->scalar_type(), "residual_out") : p.x_dtype;
    p.rowscale_dtype = rowscale.has_value() ? row_dtype_code("layer_norm: ", rowscale->scalar_type(), "rowscale") : p.x_dtype;
    TORCH_CHECK(p.residual_dtype == p.x_dtype || p.residual_dtype == FA_DTYPE_FP32, "layer_norm: residual must have the dtype of x or fp32");
    TORCH_CHECK(p.residual_out_dtype == p.x_dtype || p.residual_out_dtype == FA_DTYPE_FP32,
                "layer_norm: residual_out must have the dtype of x or fp32");
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(x.device());
    const auto stats = x.options().dtype(at::kFloat);
    Tensor mean = at::empty({is_rms_norm ? 0 : M}, stats), rstd = at::empty({M}, stats);
    TORCH_CHECK(M > 0 || !plan, "layer_norm: a plan needs at least one row");
    if (M == 0) return {mean, rstd};
    p.x = x.data_ptr(); p.weight = weight.data_ptr(); p.bias = ptr(bias); p.residual = ptr(residual); p.rowscale = ptr(rowscale);
    p.y = out.data_ptr(); p.residual_out = ptr(residual_out);
    p.mean = is_rms_norm ? nullptr : static_cast<float *>(mean.data_ptr());
    p.rstd = static_cast<float *>(rstd.data_ptr());
    p.x_row_stride = x.stride(0); p.y_row_stride = out.stride(0);
    p.residual_row_stride = residual.has_value() ? residual->stride(0) : 0;
    p.residual_out_row_stride = residual_out.has_value() ? residual_out->stride(0) : 0;
    p.M = M; p.N = (int32_t)N; p.eps = (float)eps;
    p.flags = (is_rms_norm ? FA_NORM_RMS : 0) | (zero_centered_weight ? FA_NORM_ZERO_CENTERED : 0);
    launch_or_plan("fa_norm_fwd", fa_norm_fwd, fa_norm_fwd_plan, p, plan, x);
    return {mean, rstd};
}

// x: what the forward returned as residual_out.  Returns (dx, dw, db, dresidual_in, y); db, dresidual_in and y are empty tensors
// where there is none (no bias; no residual, or dx serves as dresidual_in; no recompute_output)
// With `plan` nothing is launched: the outputs and the workspace are allocated and the params filled as for the launch, and *plan
// is what fa_norm_bwd_plan says of them
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> norm_bwd_impl(const Tensor &dy, const Tensor &x, const Tensor &weight, const OptTensor &bias,
                                                                 const OptTensor &mean, const Tensor &rstd, const OptTensor &dresidual,
                                                                 const OptTensor &rowscale, bool has_residual, bool zero_centered_weight,
                                                                 bool is_rms_norm, int64_t dx_dtype, bool recompute_output,
                                                                 fa_norm_plan *plan) {
    TORCH_CHECK(x.is_cuda(), "layer_norm: x must be on CUDA");
    TORCH_CHECK(x.dim() == 2, "layer_norm: x must have shape (M, N)");
    const int64_t M = x.size(0), N = x.size(1);
    check_rows("layer_norm: ", "(M, N)", x, "x", M, N);
    check_rows("layer_norm: ", "(M, N)", dy, "dy", M, N);
    check_vector("layer_norm: ", weight, "weight", N, "(N)");
    if (bias.has_value()) check_vector("layer_norm: ", *bias, "bias", N, "(N)");
    if (dresidual.has_value()) check_rows("layer_norm: ", "(M, N)", *dresidual, "dresidual", M, N);
    if (rowscale.has_value()) check_vector("layer_norm: ", *rowscale, "rowscale", M, "(M)");
    TORCH_CHECK(is_rms_norm || mean.has_value(), "layer_norm: mean is required unless is_rms_norm");
    if (!is_rms_norm) check_vector("layer_norm: ", *mean, "mean", M, "(M)");
    check_vector("layer_norm: ", rstd, "rstd", M, "(M)");
    TORCH_CHECK(rstd.scalar_type() == at::kFloat && (is_rms_norm || mean->scalar_type() == at::kFloat), "layer_norm: mean and rstd must be fp32");
    check_norm_width(x);
    auto p = new_params<fa_norm_bwd_params>();
    p.x_dtype = row_dtype_code("layer_norm: ", x.scalar_type(), "x");
    p.dy_dtype = row_dtype_code("layer_norm: ", dy.scalar_type(), "dy");
    p.weight_dtype = row_dtype_code("layer_norm: ", weight.scalar_type(), "weight");
    p.bias_dtype = bias.has_value() ? row_dtype_code("layer_norm: ", bias->scalar_type(), "bias") : p.weight_dtype;
    p.dx_dtype = (int32_t)dx_dtype;
    p.dresidual_dtype = dresidual.has_value() ? row_dtype_code("layer_norm: ", dresidual->scalar_type(), "dresidual") : p.x_dtype;
    p.dresidual_in_dtype = p.x_dtype;
    p.y_dtype = p.dy_dtype;
    p.rowscale_dtype = rowscale.has_value() ? row_dtype_code("layer_norm: ", rowscale->scalar_type(), "rowscale") : p.x_dtype;
    TORCH_CHECK(p.dresidual_dtype == p.x_dtype, "layer_norm: dresidual must have the dtype of x");
    TORCH_CHECK(p.x_dtype == p.dx_dtype || p.x_dtype == FA_DTYPE_FP32, "layer_norm: x must have the dtype of dx or fp32");
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(x.device());
    Tensor dx = at::empty({M, N}, x.options().dtype(norm_scalar_type(dx_dtype)));
    // (the reference's rule: where dx has the residual's dtype and is not scaled, it is dresidual_in)
    const bool own_dresidual = has_residual && (p.dx_dtype != p.x_dtype || rowscale.has_value());
    Tensor dresidual_in = own_dresidual ? at::empty({M, N}, x.options()) : none(x.options());
    Tensor y = recompute_output ? at::empty({M, N}, dy.options()) : none(x.options());
    Tensor dw = at::empty({N}, weight.options()), db = bias.has_value() ? at::empty({N}, bias->options()) : none(x.options());
    TORCH_CHECK(M > 0 || !plan, "layer_norm: a plan needs at least one row");
    if (M == 0) {  // (empty tensors have no storage to point at: no rows, zero sums, nothing of ours launched)
        dw.zero_();
        if (bias.has_value()) db.zero_();
        return {dx, dw, db, dresidual_in, y};
    }
    p.M = M; p.N = (int32_t)N;
    p.workspace_bytes = fa_norm_bwd_workspace_bytes(&p);
    Tensor workspace = at::empty({(int64_t)p.workspace_bytes}, x.options().dtype(at::kByte));
    p.workspace = p.workspace_bytes ? workspace.data_ptr() : nullptr;
    p.x = x.data_ptr(); p.dy = dy.data_ptr(); p.weight = weight.data_ptr(); p.bias = ptr(bias); p.dresidual = ptr(dresidual);
    p.rowscale = ptr(rowscale); p.mean = is_rms_norm ? nullptr : static_cast<const float *>(mean->data_ptr());
    p.rstd = static_cast<const float *>(rstd.data_ptr());
    p.dx = dx.data_ptr(); p.dresidual_in = own_dresidual ? dresidual_in.data_ptr() : nullptr;
    p.dw = dw.data_ptr(); p.db = bias.has_value() ? db.data_ptr() : nullptr; p.y = recompute_output ? y.data_ptr() : nullptr;
    p.x_row_stride = x.stride(0); p.dy_row_stride = dy.stride(0); p.dx_row_stride = N; p.dresidual_in_row_stride = N; p.y_row_stride = N;
    p.dresidual_row_stride = dresidual.has_value() ? dresidual->stride(0) : 0;
    p.eps = 0.0f;  // (rstd is read, not formed)
    p.flags = (is_rms_norm ? FA_NORM_RMS : 0) | (zero_centered_weight ? FA_NORM_ZERO_CENTERED : 0);
    launch_or_plan("fa_norm_bwd", fa_norm_bwd, fa_norm_bwd_plan, p, plan, x);
    return {dx, dw, db, dresidual_in, y};
}

// ---- fused dropout + residual-add + LayerNorm / RMSNorm (flash_attn.ops.layer_norm -> dropout_layer_norm.dropout_add_ln_fwd /
// _bwd and the parallel_residual forms, flash_attn/ops/layer_norm.py:16-108, 212-308, without the subset form).  Launches on the
// current stream, no synchronisation; (seed, offset) are drawn on the device as the attention forward draws them, and every
// output comes from the caching allocator: capturable in a HIP graph.
py::dict dropout_norm_plan_dict(const fa_dropout_norm_plan &l) {
    return plan_dict(l, {"cw", "threads", "wide", "dropout", "two_weights", "sums", "rows_per_wg", "grid_x", "grid_y"});
}

using DropoutNormFwdOut = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>;

// -> (z0, z1, x, dmask0, dmask1, mu, rsigma, rng_state); an output there is none of is an empty tensor: z1 without weight1, x
// where the stream is x0 itself and want_x does not ask for it, the masks unless return_dmask and p > 0 (dmask1: and x1), mu
// with is_rms_norm.  With `plan` nothing is launched and no (seed, offset) is drawn
DropoutNormFwdOut dropout_norm_fwd_impl(const Tensor &x0, const OptTensor &x1, const OptTensor &residual, const Tensor &weight0,
                                        const OptTensor &bias0, const OptTensor &weight1, const OptTensor &bias1,
                                        const OptTensor &rowscale, const OptTensor &colscale, double p_dropout, double eps,
                                        bool residual_in_fp32, bool is_rms_norm, bool want_x, bool return_dmask,
                                        fa_dropout_norm_plan *plan) {
    TORCH_CHECK(x0.is_cuda(), "dropout_add_layer_norm: x0 must be on CUDA");
    TORCH_CHECK(x0.dim() == 2, "dropout_add_layer_norm: x0 must have shape (M, N)");
    TORCH_CHECK(p_dropout >= 0.0 && p_dropout < 1.0, "dropout_add_layer_norm: dropout_p must be in [0, 1)");
    const int64_t M = x0.size(0), N = x0.size(1);
    check_rows("layer_norm: ", "(M, N)", x0, "x0", M, N);
    if (x1.has_value()) check_rows("layer_norm: ", "(M, N)", *x1, "x1", M, N);
    if (residual.has_value()) check_rows("layer_norm: ", "(M, N)", *residual, "residual", M, N);
    check_vector("layer_norm: ", weight0, "weight0", N, "(N)");
    for (const OptTensor *t : {&bias0, &weight1, &bias1}) {
        if (!t->has_value()) continue;
        check_vector("layer_norm: ", **t, "bias0 / weight1 / bias1", N, "(N)");
        TORCH_CHECK((*t)->scalar_type() == weight0.scalar_type(), "dropout_add_layer_norm: the weights and biases must have one dtype");
    }
    if (rowscale.has_value()) check_vector("layer_norm: ", *rowscale, "rowscale", M, "(M)");
    if (colscale.has_value()) check_vector("layer_norm: ", *colscale, "colscale", N, "(N)");
    TORCH_CHECK(!(x1.has_value() || weight1.has_value()) || !(rowscale.has_value() || colscale.has_value()),
                "dropout_add_layer_norm: rowscale / colscale are not supported with the parallel form");
    TORCH_CHECK(!bias1.has_value() || weight1.has_value(), "dropout_add_layer_norm: bias1 needs weight1");
    TORCH_CHECK(!x1.has_value() || x1->scalar_type() == x0.scalar_type(), "dropout_add_layer_norm: x1 must have the dtype of x0");
    check_norm_width(x0);
    auto p = new_params<fa_dropout_norm_fwd_params>();
    p.x0_dtype = row_dtype_code("layer_norm: ", x0.scalar_type(), "x0");
    p.weight_dtype = row_dtype_code("layer_norm: ", weight0.scalar_type(), "weight0");
    p.z_dtype = p.x0_dtype;
    p.residual_dtype = residual.has_value() ? row_dtype_code("layer_norm: ", residual->scalar_type(), "residual") : p.x0_dtype;
    p.x_dtype = residual.has_value() ? p.residual_dtype : residual_in_fp32 ? FA_DTYPE_FP32 : p.x0_dtype;
    p.rowscale_dtype = rowscale.has_value() ? row_dtype_code("layer_norm: ", rowscale->scalar_type(), "rowscale") : p.x0_dtype;
    p.colscale_dtype = colscale.has_value() ? row_dtype_code("layer_norm: ", colscale->scalar_type(), "colscale") : p.x0_dtype;
    TORCH_CHECK(p.x_dtype == p.x0_dtype || p.x_dtype == FA_DTYPE_FP32, "dropout_add_layer_norm: residual must have the dtype of x0 or fp32");
    const at::ScalarType stream_type = norm_scalar_type(p.x_dtype);
    TORCH_CHECK_WITH(Error, N * (int64_t)c10::elementSize(stream_type) <= FA_NORM_MAX_ROW_BYTES,
                     "This layer norm doesn't support feature dim >= 64KB.");
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(x0.device());
    const bool dropout = p_dropout > 0.0;
    const bool own_x = want_x || dropout || residual.has_value() || x1.has_value() || rowscale.has_value() || colscale.has_value() ||
                       p.x_dtype != p.x0_dtype;
    const auto stats = x0.options().dtype(at::kFloat), bytes = x0.options().dtype(at::kByte);
    Tensor z0 = at::empty({M, N}, x0.options()), z1 = weight1.has_value() ? at::empty({M, N}, x0.options()) : none(x0.options());
    Tensor x = own_x ? at::empty({M, N}, x0.options().dtype(stream_type)) : none(x0.options().dtype(stream_type));
    Tensor dmask0 = return_dmask && dropout ? at::empty({M, N}, bytes) : none(bytes);
    Tensor dmask1 = return_dmask && dropout && x1.has_value() ? at::empty({M, N}, bytes) : none(bytes);
    Tensor mu = at::empty({is_rms_norm ? 0 : M}, stats), rsigma = at::empty({M}, stats);
    Tensor rng_state = plan ? at::zeros({2}, x0.options().dtype(at::kLong)) : dropout_state(p_dropout, c10::nullopt, x0);
    TORCH_CHECK(M > 0 || !plan, "dropout_add_layer_norm: a plan needs at least one row");
    if (M == 0) return {z0, z1, x, dmask0, dmask1, mu, rsigma, rng_state};
    p.x0 = x0.data_ptr(); p.x1 = ptr(x1); p.residual = ptr(residual); p.weight0 = weight0.data_ptr(); p.bias0 = ptr(bias0);
    p.weight1 = ptr(weight1); p.bias1 = ptr(bias1); p.rowscale = ptr(rowscale); p.colscale = ptr(colscale);
    p.rng_state = dropout ? static_cast<const uint64_t *>(rng_state.data_ptr()) : nullptr;
    p.z0 = z0.data_ptr(); p.z1 = weight1.has_value() ? z1.data_ptr() : nullptr; p.x = own_x ? x.data_ptr() : nullptr;
    p.dmask0 = dmask0.numel() ? static_cast<uint8_t *>(dmask0.data_ptr()) : nullptr;
    p.dmask1 = dmask1.numel() ? static_cast<uint8_t *>(dmask1.data_ptr()) : nullptr;
    p.mu = is_rms_norm ? nullptr : static_cast<float *>(mu.data_ptr());
    p.rsigma = static_cast<float *>(rsigma.data_ptr());
    p.x0_row_stride = x0.stride(0); p.x1_row_stride = x1.has_value() ? x1->stride(0) : 0;
    p.residual_row_stride = residual.has_value() ? residual->stride(0) : 0;
    p.z0_row_stride = N; p.z1_row_stride = N; p.x_row_stride = N;
    p.M = M; p.N = (int32_t)N; p.eps = (float)eps; p.p_dropout = (float)p_dropout;
    p.flags = is_rms_norm ? FA_DROPOUT_NORM_RMS : 0;
    launch_or_plan("fa_dropout_norm_fwd", fa_dropout_norm_fwd, fa_dropout_norm_fwd_plan, p, plan, x0);
    return {z0, z1, x, dmask0, dmask1, mu, rsigma, rng_state};
}

using DropoutNormBwdOut = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>;

// x: the stream of the forward (its x, or x0 where it returned none).  -> (dx0, dx1, dresidual, dw0, db0, dw1, db1, dcolscale);
// empty tensors where there is none: dx1 without has_x1, dresidual without has_residual or where dx0 serves (the reference's
// rule: no dropout, no scale, one dtype), db0 / db1 without has_bias, dw1 / db1 without weight1, dcolscale without colscale
DropoutNormBwdOut dropout_norm_bwd_impl(const Tensor &dz0, const OptTensor &dz1, const OptTensor &dx, const Tensor &x,
                                        const OptTensor &x0, const OptTensor &mu, const Tensor &rsigma, const Tensor &weight0,
                                        const OptTensor &weight1, const OptTensor &rowscale, const OptTensor &colscale,
                                        const Tensor &rng_state, double p_dropout, bool has_x1, bool has_residual, bool has_bias,
                                        bool is_rms_norm, int64_t x0_dtype, fa_dropout_norm_plan *plan) {
    TORCH_CHECK(x.is_cuda(), "dropout_add_layer_norm: x must be on CUDA");
    TORCH_CHECK(x.dim() == 2, "dropout_add_layer_norm: x must have shape (M, N)");
    const int64_t M = x.size(0), N = x.size(1);
    check_rows("layer_norm: ", "(M, N)", x, "x", M, N);
    check_rows("layer_norm: ", "(M, N)", dz0, "dz0", M, N);
    TORCH_CHECK(dz1.has_value() == weight1.has_value(), "dropout_add_layer_norm: dz1 goes with weight1");
    if (dz1.has_value()) {
        check_rows("layer_norm: ", "(M, N)", *dz1, "dz1", M, N);
        TORCH_CHECK(dz1->scalar_type() == dz0.scalar_type(), "dropout_add_layer_norm: dz1 must have the dtype of dz0");
        check_vector("layer_norm: ", *weight1, "weight1", N, "(N)");
        TORCH_CHECK(weight1->scalar_type() == weight0.scalar_type(), "dropout_add_layer_norm: the weights must have one dtype");
    }
    if (dx.has_value()) {
        check_rows("layer_norm: ", "(M, N)", *dx, "dx", M, N);
        TORCH_CHECK(dx->scalar_type() == x.scalar_type(), "dropout_add_layer_norm: dx must have the dtype of x");
    }
    check_vector("layer_norm: ", weight0, "weight0", N, "(N)");
    if (rowscale.has_value()) check_vector("layer_norm: ", *rowscale, "rowscale", M, "(M)");
    if (colscale.has_value()) {
        check_vector("layer_norm: ", *colscale, "colscale", N, "(N)");
        TORCH_CHECK(x0.has_value(), "dropout_add_layer_norm: x0 is required to compute the gradient of colscale");
        check_rows("layer_norm: ", "(M, N)", *x0, "x0", M, N);
        TORCH_CHECK(row_dtype_code("layer_norm: ", x0->scalar_type(), "x0") == x0_dtype, "dropout_add_layer_norm: x0 must have the dtype x0_dtype names");
    }
    TORCH_CHECK(!(has_x1 || weight1.has_value()) || !(rowscale.has_value() || colscale.has_value()),
                "dropout_add_layer_norm: rowscale / colscale are not supported with the parallel form");
    TORCH_CHECK(is_rms_norm || mu.has_value(), "dropout_add_layer_norm: mu is required unless is_rms_norm");
    if (!is_rms_norm) check_vector("layer_norm: ", *mu, "mu", M, "(M)");
    check_vector("layer_norm: ", rsigma, "rsigma", M, "(M)");
    TORCH_CHECK(rsigma.scalar_type() == at::kFloat && (is_rms_norm || mu->scalar_type() == at::kFloat),
                "dropout_add_layer_norm: mu and rsigma must be fp32");
    TORCH_CHECK(rng_state.is_cuda() && rng_state.scalar_type() == at::kLong && rng_state.numel() == 2 && rng_state.is_contiguous(),
                "dropout_add_layer_norm: rng_state must be two int64 on the device");
    TORCH_CHECK(p_dropout >= 0.0 && p_dropout < 1.0, "dropout_add_layer_norm: dropout_p must be in [0, 1)");
    check_norm_width(x);
    auto p = new_params<fa_dropout_norm_bwd_params>();
    p.x_dtype = row_dtype_code("layer_norm: ", x.scalar_type(), "x");
    p.dz_dtype = row_dtype_code("layer_norm: ", dz0.scalar_type(), "dz0");
    p.weight_dtype = row_dtype_code("layer_norm: ", weight0.scalar_type(), "weight0");
    p.x0_dtype = (int32_t)x0_dtype;
    p.rowscale_dtype = rowscale.has_value() ? row_dtype_code("layer_norm: ", rowscale->scalar_type(), "rowscale") : p.x0_dtype;
    p.colscale_dtype = colscale.has_value() ? row_dtype_code("layer_norm: ", colscale->scalar_type(), "colscale") : p.x0_dtype;
    const at::ScalarType in_type = norm_scalar_type(x0_dtype);
    TORCH_CHECK(p.x_dtype == p.x0_dtype || p.x_dtype == FA_DTYPE_FP32, "dropout_add_layer_norm: x must have the dtype of x0 or fp32");
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(x.device());
    const bool dropout = p_dropout > 0.0;
    const bool own_dresidual = has_residual && (dropout || rowscale.has_value() || colscale.has_value() || p.x_dtype != p.x0_dtype);
    const auto in = x.options().dtype(in_type), w = weight0.options();
    Tensor dx0 = at::empty({M, N}, in);
    Tensor dx1 = has_x1 ? at::empty({M, N}, in) : none(in);
    Tensor dresidual = own_dresidual ? at::empty({M, N}, x.options()) : none(x.options());
    Tensor dw0 = at::empty({N}, w), db0 = has_bias ? at::empty({N}, w) : none(w);
    Tensor dw1 = weight1.has_value() ? at::empty({N}, w) : none(w);
    Tensor db1 = weight1.has_value() && has_bias ? at::empty({N}, w) : none(w);
    Tensor dcolscale = colscale.has_value() ? at::empty({N}, colscale->options()) : none(w);
    TORCH_CHECK(M > 0 || !plan, "dropout_add_layer_norm: a plan needs at least one row");
    if (M == 0) {  // (empty tensors have no storage to point at: no rows, zero sums, nothing of ours launched)
        for (Tensor *t : {&dw0, &db0, &dw1, &db1, &dcolscale}) t->zero_();
        return {dx0, dx1, dresidual, dw0, db0, dw1, db1, dcolscale};
    }
    p.M = M; p.N = (int32_t)N;
    p.weight1 = ptr(weight1); p.colscale = ptr(colscale);  // (the workspace depends on which sums there are)
    p.workspace_bytes = fa_dropout_norm_bwd_workspace_bytes(&p);
    Tensor workspace = at::empty({(int64_t)p.workspace_bytes}, x.options().dtype(at::kByte));
    p.workspace = p.workspace_bytes ? workspace.data_ptr() : nullptr;
    p.dz0 = dz0.data_ptr(); p.dz1 = ptr(dz1); p.dx = ptr(dx); p.x = x.data_ptr(); p.x0 = colscale.has_value() ? ptr(x0) : nullptr;
    p.weight0 = weight0.data_ptr(); p.rowscale = ptr(rowscale);
    p.rng_state = dropout ? static_cast<const uint64_t *>(rng_state.data_ptr()) : nullptr;
    p.mu = is_rms_norm ? nullptr : static_cast<const float *>(mu->data_ptr());
    p.rsigma = static_cast<const float *>(rsigma.data_ptr());
    p.dx0 = dx0.data_ptr(); p.dx1 = has_x1 ? dx1.data_ptr() : nullptr; p.dresidual = own_dresidual ? dresidual.data_ptr() : nullptr;
    p.dw0 = dw0.data_ptr(); p.db0 = has_bias ? db0.data_ptr() : nullptr;
    p.dw1 = weight1.has_value() ? dw1.data_ptr() : nullptr; p.db1 = weight1.has_value() && has_bias ? db1.data_ptr() : nullptr;
    p.dcolscale = colscale.has_value() ? dcolscale.data_ptr() : nullptr;
    p.dz0_row_stride = dz0.stride(0); p.dz1_row_stride = dz1.has_value() ? dz1->stride(0) : 0;
    p.dx_row_stride = dx.has_value() ? dx->stride(0) : 0; p.x_row_stride = x.stride(0);
    p.x0_row_stride = colscale.has_value() ? x0->stride(0) : 0;
    p.dx0_row_stride = N; p.dx1_row_stride = N; p.dresidual_row_stride = N;
    p.p_dropout = (float)p_dropout;
    p.flags = is_rms_norm ? FA_DROPOUT_NORM_RMS : 0;
    launch_or_plan("fa_dropout_norm_bwd", fa_dropout_norm_bwd, fa_dropout_norm_bwd_plan, p, plan, x);
    return {dx0, dx1, dresidual, dw0, db0, dw1, db1, dcolscale};
}

// ---- fused cross-entropy loss (flash_attn.ops.triton.cross_entropy -> CrossEntropyLoss.forward / backward,
// flash_attn/ops/triton/cross_entropy.py:149-289; the collectives of a vocabulary split stay in Python).  Launches on the
// current stream, no synchronisation; losses, lse and z_losses come from the caching allocator: capturable in a HIP graph.
int xent_labels_code(at::ScalarType t) {
    if (t == at::kLong) return FA_XENT_LABELS_INT64;
    if (t == at::kInt) return FA_XENT_LABELS_INT32;
    TORCH_CHECK(false, "cross_entropy: labels must be int64 or int32");
    return -1;
}

void check_xent_rows(const Tensor &t, const char *name) {
    TORCH_CHECK(t.is_cuda(), "cross_entropy: ", name, " must be on CUDA");
    TORCH_CHECK(t.dim() == 2, "cross_entropy: ", name, " must have shape (M, N)");
    TORCH_CHECK(t.size(1) >= 1 && t.size(1) <= std::numeric_limits<int32_t>::max(), "cross_entropy: ", name, " must have 1 <= N < 2^31 columns");
    TORCH_CHECK(t.stride(-1) == 1, "cross_entropy: ", name, " must have contiguous last dimension");
}

py::dict xent_plan_dict(const fa_xent_plan &l) { return plan_dict(l, {"cw", "grid_x", "grid_y", "lse_given"}); }

// (losses, lse, z_losses).  With precomputed_lse that tensor is read and the lse returned is empty; with split the columns are
// one rank's part of total_classes, losses lack the lse and the z-loss, and the z_losses returned are empty
// With `plan` nothing is launched: *plan is what fa_xent_fwd_plan says of the params the launch would get
std::tuple<Tensor, Tensor, Tensor> xent_fwd_impl(const Tensor &logits, const Tensor &labels, const OptTensor &precomputed_lse, double smoothing,
                                                 double logit_scale, double lse_square_scale, int64_t ignore_index, int64_t class_start_idx,
                                                 int64_t total_classes, bool split, fa_xent_plan *plan) {
    check_xent_rows(logits, "logits");
    const int64_t M = logits.size(0), N = logits.size(1);
    check_vector("cross_entropy: ", labels, "labels", M, "(M)", true);
    if (precomputed_lse.has_value()) {
        check_vector("cross_entropy: ", *precomputed_lse, "precomputed_lse", M, "(M)", true);
        TORCH_CHECK(precomputed_lse->scalar_type() == at::kFloat, "cross_entropy: precomputed_lse must be fp32");
    }
    auto p = new_params<fa_xent_fwd_params>();
    p.logits_dtype = row_dtype_code("cross_entropy: ", logits.scalar_type(), "logits");
    p.labels_dtype = xent_labels_code(labels.scalar_type());
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(logits.device());
    const auto fp32 = logits.options().dtype(at::kFloat);
    Tensor losses = at::empty({M}, fp32), lse = at::empty({precomputed_lse.has_value() ? 0 : M}, fp32), z_losses = at::empty({split ? 0 : M}, fp32);
    TORCH_CHECK(M > 0 || !plan, "cross_entropy: a plan needs at least one row");
    if (M == 0) return {losses, lse, z_losses};
    p.logits = logits.data_ptr(); p.labels = labels.data_ptr();
    p.losses = static_cast<float *>(losses.data_ptr());
    p.lse = static_cast<float *>(precomputed_lse.has_value() ? precomputed_lse->data_ptr() : lse.data_ptr());
    p.z_losses = split ? nullptr : static_cast<float *>(z_losses.data_ptr());
    p.logits_row_stride = logits.stride(0);
    p.M = M; p.N = (int32_t)N;
    p.ignore_index = ignore_index; p.class_start_idx = class_start_idx; p.total_classes = total_classes;
    p.smoothing = (float)smoothing; p.logit_scale = (float)logit_scale; p.lse_square_scale = (float)lse_square_scale;
    p.flags = (precomputed_lse.has_value() ? FA_XENT_PRECOMPUTED_LSE : 0) | (split ? FA_XENT_SPLIT : 0);
    launch_or_plan("fa_xent_fwd", fa_xent_fwd, fa_xent_fwd_plan, p, plan, logits);
    return {losses, lse, z_losses};
}

// writes dlogits, which may be logits.  With `plan` nothing is launched: *plan is what fa_xent_bwd_plan says of the params
void xent_bwd_impl(const Tensor &dloss, const Tensor &logits, const Tensor &labels, const Tensor &lse, Tensor dlogits, double smoothing,
                   double logit_scale, double lse_square_scale, int64_t ignore_index, int64_t class_start_idx, int64_t total_classes,
                   fa_xent_plan *plan) {
    check_xent_rows(logits, "logits");
    check_xent_rows(dlogits, "dlogits");
    const int64_t M = logits.size(0), N = logits.size(1);
    TORCH_CHECK(dlogits.size(0) == M && dlogits.size(1) == N, "cross_entropy: dlogits must have the shape of logits");
    TORCH_CHECK(dlogits.scalar_type() == logits.scalar_type(), "cross_entropy: dlogits must have the dtype of logits");
    check_vector("cross_entropy: ", labels, "labels", M, "(M)", true);
    check_vector("cross_entropy: ", lse, "lse", M, "(M)", true);
    check_vector("cross_entropy: ", dloss, "dloss", M, "(M)", false);
    TORCH_CHECK(lse.scalar_type() == at::kFloat && dloss.scalar_type() == at::kFloat, "cross_entropy: lse and dloss must be fp32");
    auto p = new_params<fa_xent_bwd_params>();
    p.logits_dtype = row_dtype_code("cross_entropy: ", logits.scalar_type(), "logits");
    p.labels_dtype = xent_labels_code(labels.scalar_type());
    TORCH_CHECK(M > 0 || !plan, "cross_entropy: a plan needs at least one row");
    if (M == 0) return;
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(logits.device());
    p.logits = logits.data_ptr(); p.labels = labels.data_ptr(); p.dlogits = dlogits.data_ptr();
    p.lse = static_cast<const float *>(lse.data_ptr()); p.dloss = static_cast<const float *>(dloss.data_ptr());
    p.logits_row_stride = logits.stride(0); p.dlogits_row_stride = dlogits.stride(0); p.dloss_stride = dloss.stride(0);
    p.M = M; p.N = (int32_t)N;
    p.ignore_index = ignore_index; p.class_start_idx = class_start_idx; p.total_classes = total_classes;
    p.smoothing = (float)smoothing; p.logit_scale = (float)logit_scale; p.lse_square_scale = (float)lse_square_scale;
    launch_or_plan("fa_xent_bwd", fa_xent_bwd, fa_xent_bwd_plan, p, plan, logits);
}

// ---- fused top-k / top-p token sampling (flash_attn.utils.generation: sample, modify_logits_for_top_k_filtering,
// modify_logits_for_top_p_filtering, flash_attn/utils/generation.py:45-95; include/fa_sample.h).  Launches on the current
// stream, no synchronisation; token, kept and mass come from the caching allocator: capturable in a HIP graph.
py::dict sample_plan_dict(const fa_sample_form &l) {
    return plan_dict(l, {"cw", "threads", "mode", "greedy", "topk", "topp", "draw", "k", "key_bits", "key_passes", "index_bits",
                         "index_passes", "frac_bits", "grid_x"});
}

// (token, kept, mass); kept and mass are empty without `stats`, token is empty in the filter mode.  A draw (top_k != 1) takes
// the uniforms `u`, or `rng_state` = (seed, offset) on the device, or with neither draws that pair on the device from the default
// generator.  With `plan` nothing is launched and nothing is drawn: *plan is what fa_sample_plan says of the params the launch
// would get
std::tuple<Tensor, Tensor, Tensor> sample_impl(const Tensor &logits, int64_t top_k, double top_p, double temperature, const OptTensor &u,
                                               const OptTensor &rng_state, bool stats, int mode, fa_sample_form *plan) {
    TORCH_CHECK(logits.is_cuda(), "sample: logits must be on CUDA");
    TORCH_CHECK(logits.dim() == 2, "sample: logits must have shape (batch_size, vocab_size)");
    TORCH_CHECK(logits.size(1) >= 1 && logits.size(1) <= std::numeric_limits<int32_t>::max(), "sample: logits must have 1 <= vocab_size < 2^31 columns");
    TORCH_CHECK(logits.stride(-1) == 1 || logits.size(1) == 1, "sample: logits must have contiguous last dimension");
    TORCH_CHECK(top_k >= 0 && top_k <= std::numeric_limits<int32_t>::max(), "sample: top_k must be in [0, 2^31)");
    const int64_t B = logits.size(0), V = logits.size(1);
    const bool draw = mode == FA_SAMPLE_DRAW, greedy = draw && top_k == 1;
    TORCH_CHECK(!(u.has_value() && rng_state.has_value()), "sample: u and rng_state exclude each other");
    if (u.has_value()) {
        check_vector("sample: ", *u, "u", B, "(batch_size)", true);
        TORCH_CHECK(u->scalar_type() == at::kFloat, "sample: u must be fp32");
    }
    if (rng_state.has_value())
        TORCH_CHECK(rng_state->is_cuda() && rng_state->scalar_type() == at::kLong && rng_state->numel() == 2 && rng_state->is_contiguous(),
                    "sample: rng_state must be two int64 on the device");
    auto p = new_params<fa_sample_params>();
    p.logits_dtype = row_dtype_code("sample: ", logits.scalar_type(), "logits");
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(logits.device());
    stats = stats && !greedy;
    Tensor token = at::empty({draw ? B : 0}, logits.options().dtype(at::kLong));
    Tensor kept = at::empty({stats ? B : 0}, logits.options().dtype(at::kInt)), mass = at::empty({stats ? B : 0}, logits.options().dtype(at::kFloat));
    TORCH_CHECK(B > 0 || !plan, "sample: a plan needs at least one row");
    if (B == 0) return {token, kept, mass};
    Tensor state;  // (kept alive to the launch)
    if (draw && !greedy) {
        if (u.has_value()) p.u = static_cast<const float *>(u->data_ptr());
        else if (rng_state.has_value()) p.rng_state = static_cast<const uint64_t *>(rng_state->data_ptr());
        else if (plan) p.rng_state = reinterpret_cast<const uint64_t *>(uintptr_t(16));  // (a plan reads no memory)
        else {
            state = dropout_state(1.0, c10::nullopt, logits);
            p.rng_state = static_cast<const uint64_t *>(state.data_ptr());
        }
    }
    p.logits = logits.data_ptr();
    p.token = draw ? static_cast<int64_t *>(token.data_ptr()) : nullptr;
    p.kept = stats ? static_cast<int32_t *>(kept.data_ptr()) : nullptr;
    p.mass = stats ? static_cast<float *>(mass.data_ptr()) : nullptr;
    p.logits_row_stride = logits.stride(0);
    p.B = B; p.V = (int32_t)V;
    p.mode = mode; p.top_k = (int32_t)top_k; p.top_p = (float)top_p; p.temperature = (float)temperature;
    launch_or_plan("fa_sample", fa_sample, fa_sample_plan, p, plan, logits);
    return {token, kept, mass};
}

std::tuple<Tensor, Tensor, Tensor> sample(const Tensor &logits, int64_t top_k, double top_p, double temperature, const OptTensor &u,
                                          const OptTensor &rng_state, bool stats) {
    return sample_impl(logits, top_k, top_p, temperature, u, rng_state, stats, FA_SAMPLE_DRAW, nullptr);
}

// -inf over the entries of logits that top-k (all ties of the k-th value stay) and then top-p remove, in place; (kept, mass)
std::tuple<Tensor, Tensor> sample_filter_(Tensor logits, int64_t top_k, double top_p, bool stats) {
    auto out = sample_impl(logits, top_k, top_p, 1.0, c10::nullopt, c10::nullopt, stats, FA_SAMPLE_FILTER, nullptr);
    return {std::get<1>(out), std::get<2>(out)};
}

// the form sample (filter: sample_filter_) takes with these arguments (fa_sample_form as a dict); at least one row
py::dict sample_plan(const Tensor &logits, int64_t top_k, double top_p, double temperature, bool filter, bool stats) {
    fa_sample_form plan{};
    sample_impl(logits, top_k, top_p, temperature, c10::nullopt, c10::nullopt, stats, filter ? FA_SAMPLE_FILTER : FA_SAMPLE_DRAW, &plan);
    return sample_plan_dict(plan);
}

// ---- fused verification of speculative sampling (flash_attn.utils.generation.sample_speculative,
// flash_attn/utils/generation.py:209-265; include/fa_spec_sample.h).  Launches on the current stream, no synchronisation; the
// outputs and the records' workspace come from the caching allocator: capturable in a HIP graph.
py::dict spec_sample_plan_dict(const fa_spec_sample_form &l) {
    return plan_dict(l, {"cw", "threads", "topk", "topp", "k", "key_bits", "key_passes", "index_bits", "index_passes", "frac_bits",
                         "grid_a", "grid_b"});
}

// (tokens (B, S + 1) of the dtype of tokens_draft, num_generated (B) int64, p_tok, q_tok (B, S) fp32, accepted (B, S) int32); the
// last three are empty without `stats`.  The uniforms are (u_acc, u_res), or `rng_state` = (seed, offset) on the device, or with
// neither that pair drawn on the device from the default generator
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> sample_speculative_impl(const Tensor &logits, const Tensor &logits_draft,
                                                                           const Tensor &tokens_draft, int64_t top_k, double top_p,
                                                                           double temperature, const OptTensor &u_acc, const OptTensor &u_res,
                                                                           const OptTensor &rng_state, bool stats, fa_spec_sample_form *plan) {
    const char *op = "sample_speculative: ";
    TORCH_CHECK(logits.is_cuda() && logits_draft.is_cuda() && tokens_draft.is_cuda(), op, "logits, logits_draft and tokens_draft must be on CUDA");
    TORCH_CHECK(logits.dim() == 3 && logits.size(1) >= 1, op, "logits must have shape (batch_size, seqlen + 1, vocab_size)");
    const int64_t B = logits.size(0), S = logits.size(1) - 1, V = logits.size(2);
    TORCH_CHECK(V >= 1 && V <= std::numeric_limits<int32_t>::max(), op, "logits must have 1 <= vocab_size < 2^31 columns");
    TORCH_CHECK(B * (2 * S + 1) <= std::numeric_limits<int32_t>::max(), op, "batch_size * (2 seqlen + 1) must be below 2^31");
    TORCH_CHECK(logits_draft.dim() == 3 && logits_draft.size(0) == B && logits_draft.size(1) == S && logits_draft.size(2) == V, op,
                "logits_draft must have shape (batch_size, seqlen, vocab_size)");
    TORCH_CHECK(tokens_draft.dim() == 2 && tokens_draft.size(0) == B && tokens_draft.size(1) == S, op,
                "tokens_draft must have shape (batch_size, seqlen)");
    TORCH_CHECK(logits.stride(-1) == 1 || V == 1, op, "logits must have contiguous last dimension");
    TORCH_CHECK(logits_draft.stride(-1) == 1 || V == 1, op, "logits_draft must have contiguous last dimension");
    TORCH_CHECK(tokens_draft.stride(-1) == 1 || S <= 1, op, "tokens_draft must have contiguous last dimension");
    TORCH_CHECK(logits_draft.scalar_type() == logits.scalar_type(), op, "logits_draft must have the dtype of logits");
    TORCH_CHECK(tokens_draft.scalar_type() == at::kLong || tokens_draft.scalar_type() == at::kInt, op, "tokens_draft must be int32 or int64");
    TORCH_CHECK(top_k >= 0 && top_k <= std::numeric_limits<int32_t>::max(), op, "top_k must be in [0, 2^31)");
    TORCH_CHECK(u_acc.has_value() == u_res.has_value(), op, "u_acc and u_res come together");
    TORCH_CHECK(!(u_res.has_value() && rng_state.has_value()), op, "u and rng_state exclude each other");
    if (u_res.has_value()) {
        check_vector(op, *u_res, "u_res", B, "(batch_size)", true);
        TORCH_CHECK(u_acc->is_cuda() && u_acc->dim() == 2 && u_acc->size(0) == B && u_acc->size(1) == S && u_acc->is_contiguous(), op,
                    "u_acc must have shape (batch_size, seqlen) and be contiguous");
        TORCH_CHECK(u_res->scalar_type() == at::kFloat && u_acc->scalar_type() == at::kFloat, op, "u_acc and u_res must be fp32");
    }
    if (rng_state.has_value())
        TORCH_CHECK(rng_state->is_cuda() && rng_state->scalar_type() == at::kLong && rng_state->numel() == 2 && rng_state->is_contiguous(),
                    op, "rng_state must be two int64 on the device");
    auto p = new_params<fa_spec_sample_params>();
    p.logits_dtype = row_dtype_code(op, logits.scalar_type(), "logits");
    p.tokens_dtype = tokens_draft.scalar_type() == at::kLong ? FA_SPEC_TOKENS_INT64 : FA_SPEC_TOKENS_INT32;
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(logits.device());
    const auto f32 = logits.options().dtype(at::kFloat);
    Tensor tokens = at::empty({B, S + 1}, tokens_draft.options()), num = at::empty({B}, logits.options().dtype(at::kLong));
    Tensor p_tok = stats ? at::empty({B, S}, f32) : none(f32), q_tok = stats ? at::empty({B, S}, f32) : none(f32);
    Tensor accepted = stats ? at::empty({B, S}, logits.options().dtype(at::kInt)) : none(logits.options().dtype(at::kInt));
    TORCH_CHECK(B > 0 || !plan, op, "a plan needs at least one sequence");
    if (B == 0) return {tokens, num, p_tok, q_tok, accepted};
    Tensor state;  // (kept alive to the launch)
    if (u_res.has_value()) {
        p.u_res = static_cast<const float *>(u_res->data_ptr());
        p.u_acc = S > 0 ? static_cast<const float *>(u_acc->data_ptr()) : nullptr;
    } else if (rng_state.has_value()) {
        p.rng_state = static_cast<const uint64_t *>(rng_state->data_ptr());
    } else if (plan) {
        p.rng_state = reinterpret_cast<const uint64_t *>(uintptr_t(16));  // (a plan reads no memory)
    } else {
        state = dropout_state(1.0, c10::nullopt, logits);
        p.rng_state = static_cast<const uint64_t *>(state.data_ptr());
    }
    p.workspace_bytes = fa_spec_sample_workspace_size(B, (int32_t)S);
    Tensor workspace = at::empty({p.workspace_bytes}, logits.options().dtype(at::kByte));
    p.workspace = workspace.data_ptr();
    p.logits = logits.data_ptr();
    p.logits_draft = S > 0 ? logits_draft.data_ptr() : nullptr;
    p.tokens_draft = S > 0 ? tokens_draft.data_ptr() : nullptr;
    p.tokens = tokens.data_ptr();
    p.num_generated = static_cast<int64_t *>(num.data_ptr());
    if (stats && S > 0) {
        p.p_tok = static_cast<float *>(p_tok.data_ptr()); p.q_tok = static_cast<float *>(q_tok.data_ptr());
        p.accepted = static_cast<int32_t *>(accepted.data_ptr());
    }
    p.logits_batch_stride = logits.stride(0); p.logits_pos_stride = logits.stride(1);
    p.draft_batch_stride = logits_draft.stride(0); p.draft_pos_stride = logits_draft.stride(1);
    p.tokens_draft_batch_stride = tokens_draft.stride(0);
    p.B = B; p.S = (int32_t)S; p.V = (int32_t)V;
    p.top_k = (int32_t)top_k; p.top_p = (float)top_p; p.temperature = (float)temperature;
    launch_or_plan("fa_spec_sample", fa_spec_sample, fa_spec_sample_plan, p, plan, logits);
    return {tokens, num, p_tok, q_tok, accepted};
}

// ---- fused acceptance walk over a tree of draft tokens (utils.generation.sample_speculative_tree; include/fa_tree_sample.h).
// Launches on the current stream, no synchronisation; the outputs and the records' workspace come from the caching allocator:
// capturable in a HIP graph.
py::dict tree_sample_plan_dict(const fa_tree_sample_form &l) {
    return plan_dict(l, {"cw", "threads", "drafts", "topk", "topp", "k", "key_bits", "key_passes", "index_bits", "index_passes",
                         "frac_bits", "grid_a", "grid_b"});
}

// (tokens (B, T) of the dtype of tokens_draft, num_generated (B) int64, path (B, T) int32, path_len (B) int32, p_tok, q_tok (B, T)
// fp32, visited, accepted (B, T) int32); the last four are empty without `stats`.  logits_draft absent: the one-hot rule.  The
// uniforms are (u_acc, u_res), or `rng_state` = (seed, offset) on the device, or with neither that pair drawn on the device from
// the default generator
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> sample_speculative_tree_impl(
    const Tensor &logits, const OptTensor &logits_draft, const Tensor &tokens_draft, const Tensor &parents, int64_t top_k, double top_p,
    double temperature, const OptTensor &u_acc, const OptTensor &u_res, const OptTensor &rng_state, bool stats, fa_tree_sample_form *plan) {
    const char *op = "sample_speculative_tree: ";
    TORCH_CHECK(logits.is_cuda() && tokens_draft.is_cuda() && parents.is_cuda(), op, "logits, tokens_draft and parents must be on CUDA");
    TORCH_CHECK(logits.dim() == 3 && logits.size(1) >= 1 && logits.size(1) <= FA_TREE_SAMPLE_MAX_NODES, op,
                "logits must have shape (batch_size, nodes, vocab_size) with 1 <= nodes <= 64");
    const int64_t B = logits.size(0), T = logits.size(1), V = logits.size(2);
    TORCH_CHECK(V >= 1 && V <= std::numeric_limits<int32_t>::max(), op, "logits must have 1 <= vocab_size < 2^31 columns");
    TORCH_CHECK(B * 2 * T <= std::numeric_limits<int32_t>::max(), op, "batch_size * 2 nodes must be below 2^31");
    TORCH_CHECK(tokens_draft.dim() == 2 && tokens_draft.size(0) == B && tokens_draft.size(1) == T, op,
                "tokens_draft must have shape (batch_size, nodes)");
    TORCH_CHECK(parents.dim() == 2 && parents.size(0) == B && parents.size(1) == T && parents.scalar_type() == at::kInt, op,
                "parents must be int32 of shape (batch_size, nodes)");
    TORCH_CHECK(logits.stride(-1) == 1 || V == 1, op, "logits must have contiguous last dimension");
    TORCH_CHECK((tokens_draft.stride(-1) == 1 && parents.stride(-1) == 1) || T == 1, op,
                "tokens_draft and parents must have contiguous last dimension");
    TORCH_CHECK(tokens_draft.scalar_type() == at::kLong || tokens_draft.scalar_type() == at::kInt, op, "tokens_draft must be int32 or int64");
    if (logits_draft.has_value()) {
        TORCH_CHECK(logits_draft->is_cuda() && logits_draft->dim() == 3 && logits_draft->size(0) == B && logits_draft->size(1) == T &&
                        logits_draft->size(2) == V, op, "logits_draft must be on CUDA with shape (batch_size, nodes, vocab_size)");
        TORCH_CHECK(logits_draft->stride(-1) == 1 || V == 1, op, "logits_draft must have contiguous last dimension");
        TORCH_CHECK(logits_draft->scalar_type() == logits.scalar_type(), op, "logits_draft must have the dtype of logits");
    }
    TORCH_CHECK(top_k >= 0 && top_k <= std::numeric_limits<int32_t>::max(), op, "top_k must be in [0, 2^31)");
    TORCH_CHECK(u_acc.has_value() == u_res.has_value(), op, "u_acc and u_res come together");
    TORCH_CHECK(!(u_res.has_value() && rng_state.has_value()), op, "u and rng_state exclude each other");
    if (u_res.has_value()) {
        check_vector(op, *u_res, "u_res", B, "(batch_size)", true);
        TORCH_CHECK(u_acc->is_cuda() && u_acc->dim() == 2 && u_acc->size(0) == B && u_acc->size(1) == T && u_acc->is_contiguous(), op,
                    "u_acc must have shape (batch_size, nodes) and be contiguous");
        TORCH_CHECK(u_res->scalar_type() == at::kFloat && u_acc->scalar_type() == at::kFloat, op, "u_acc and u_res must be fp32");
    }
    if (rng_state.has_value())
        TORCH_CHECK(rng_state->is_cuda() && rng_state->scalar_type() == at::kLong && rng_state->numel() == 2 && rng_state->is_contiguous(),
                    op, "rng_state must be two int64 on the device");
    auto p = new_params<fa_tree_sample_params>();
    p.logits_dtype = row_dtype_code(op, logits.scalar_type(), "logits");
    p.tokens_dtype = tokens_draft.scalar_type() == at::kLong ? FA_TREE_TOKENS_INT64 : FA_TREE_TOKENS_INT32;
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(logits.device());
    const auto f32 = logits.options().dtype(at::kFloat), i32 = logits.options().dtype(at::kInt);
    Tensor tokens = at::empty({B, T}, tokens_draft.options()), num = at::empty({B}, logits.options().dtype(at::kLong));
    Tensor path = at::empty({B, T}, i32), path_len = at::empty({B}, i32);
    Tensor p_tok = stats ? at::empty({B, T}, f32) : none(f32), q_tok = stats ? at::empty({B, T}, f32) : none(f32);
    Tensor visited = stats ? at::empty({B, T}, i32) : none(i32), accepted = stats ? at::empty({B, T}, i32) : none(i32);
    TORCH_CHECK(B > 0 || !plan, op, "a plan needs at least one sequence");
    if (B == 0) return {tokens, num, path, path_len, p_tok, q_tok, visited, accepted};
    Tensor state;  // (kept alive to the launch)
    if (u_res.has_value()) {
        p.u_res = static_cast<const float *>(u_res->data_ptr());
        p.u_acc = static_cast<const float *>(u_acc->data_ptr());
    } else if (rng_state.has_value()) {
        p.rng_state = static_cast<const uint64_t *>(rng_state->data_ptr());
    } else if (plan) {
        p.rng_state = reinterpret_cast<const uint64_t *>(uintptr_t(16));  // (a plan reads no memory)
    } else {
        state = dropout_state(1.0, c10::nullopt, logits);
        p.rng_state = static_cast<const uint64_t *>(state.data_ptr());
    }
    p.workspace_bytes = fa_tree_sample_workspace_size(B, (int32_t)T);
    Tensor workspace = at::empty({p.workspace_bytes}, logits.options().dtype(at::kByte));
    p.workspace = workspace.data_ptr();
    p.logits = logits.data_ptr();
    p.logits_draft = logits_draft.has_value() ? logits_draft->data_ptr() : nullptr;
    p.tokens_draft = tokens_draft.data_ptr();
    p.parents = static_cast<const int32_t *>(parents.data_ptr());
    p.path = static_cast<int32_t *>(path.data_ptr()); p.path_len = static_cast<int32_t *>(path_len.data_ptr());
    p.tokens = tokens.data_ptr();
    p.num_generated = static_cast<int64_t *>(num.data_ptr());
    if (stats) {
        p.p_tok = static_cast<float *>(p_tok.data_ptr()); p.q_tok = static_cast<float *>(q_tok.data_ptr());
        p.visited = static_cast<int32_t *>(visited.data_ptr()); p.accepted = static_cast<int32_t *>(accepted.data_ptr());
    }
    p.logits_batch_stride = logits.stride(0); p.logits_node_stride = logits.stride(1);
    if (logits_draft.has_value()) { p.draft_batch_stride = logits_draft->stride(0); p.draft_node_stride = logits_draft->stride(1); }
    p.tokens_draft_batch_stride = tokens_draft.stride(0); p.parents_batch_stride = parents.stride(0);
    p.B = B; p.T = (int32_t)T; p.V = (int32_t)V;
    p.top_k = (int32_t)top_k; p.top_p = (float)top_p; p.temperature = (float)temperature;
    launch_or_plan("fa_tree_sample", fa_tree_sample, fa_tree_sample_plan, p, plan, logits);
    return {tokens, num, path, path_len, p_tok, q_tok, visited, accepted};
}

// ---- block summaries of the keys and the Quest block selection (hopper_interface.kvcache_block_summary_update /
// kvcache_select_blocks; include/fa_block_select.h): what produces the lists fwd_kvcache_sparse reads.  Launches on the current
// stream, nothing is read on the host; every tensor the launches write is an argument: capturable in a HIP graph.  plan: the
// form the call takes as text, and nothing is launched.
void check_fill(const Tensor &t, const char *name, int64_t batch_size, const Tensor &on) {
    TORCH_CHECK(t.scalar_type() == at::kInt && t.is_cuda() && t.device() == on.device() && t.dim() == 1 && t.size(0) == batch_size &&
                    t.is_contiguous(),
                name, " must be a contiguous int32 CUDA tensor of shape (batch_size,)");
}

void check_summary(const Tensor &s, int64_t block_size) {
    TORCH_CHECK(block_size > 0 && block_size % 64 == 0, "kv_block_size must be a positive multiple of 64, got ", block_size);
    TORCH_CHECK(s.is_cuda() && s.dim() == 5 && s.size(2) == 2, "k_summary must be a CUDA tensor of shape (slots, max_blocks, 2, num_heads_k, head_size)");
    TORCH_CHECK(s.scalar_type() == at::kHalf || s.scalar_type() == at::kBFloat16, "k_summary must be fp16 or bf16");
    TORCH_CHECK(s.stride(-1) == 1, "k_summary must have contiguous last dimension");
    TORCH_CHECK(s.size(4) <= 128 && s.size(4) % 16 == 0, "k_summary: head_size must be a multiple of 16, at most 128, got ", s.size(4));
}

std::string block_summary_update_impl(const Tensor &k_summary, const Tensor &k_cache, const OptTensor &seqlens_old,
                                      const Tensor &seqlens_new, int64_t kv_block_size, c10::optional<int64_t> max_seqlen_new,
                                      const OptTensor &cache_batch_idx, const OptTensor &page_table, bool plan) {
    check_summary(k_summary, kv_block_size);
    const bool fp8 = k_cache.scalar_type() == at::kFloat8_e4m3fn;
    TORCH_CHECK(fp8 || k_cache.scalar_type() == k_summary.scalar_type(), "k_cache must have the dtype of k_summary or be torch.float8_e4m3fn");
    TORCH_CHECK(k_cache.is_cuda() && k_cache.device() == k_summary.device() && k_cache.dim() == 4,
                "k_cache must be a KV cache of shape (batch or num_pages, seqlen or page_size, num_heads_k, head_size) on the device of k_summary");
    CHECK_LAST_CONTIGUOUS(k_cache, "k_cache must have contiguous last dimension");
    TORCH_CHECK(k_cache.size(2) == k_summary.size(3) && k_cache.size(3) == k_summary.size(4), "k_summary must have the heads and the head_size of k_cache");
    const int64_t batch_size = seqlens_new.numel();
    check_fill(seqlens_new, "seqlens_new", batch_size, k_summary);
    if (seqlens_old.has_value()) check_fill(*seqlens_old, "seqlens_old", batch_size, k_summary);
    int64_t capacity;
    if (page_table.has_value()) {
        TORCH_CHECK(!cache_batch_idx.has_value(), "Paged KVcache does not support cache_batch_idx");
        capacity = check_block_table(*page_table, k_cache, batch_size, 1).second * k_cache.size(1);
        TORCH_CHECK(k_summary.size(0) == batch_size, "k_summary of a paged cache must have one slot per batch entry");
    } else {
        capacity = k_cache.size(1);
        TORCH_CHECK(k_summary.size(0) == k_cache.size(0), "k_summary must have one slot per slot of the cache");
        if (cache_batch_idx.has_value()) check_fill(*cache_batch_idx, "cache_batch_idx", batch_size, k_summary);
        else TORCH_CHECK(batch_size <= k_cache.size(0), "the batch must fit the cache without cache_batch_idx");
    }
    TORCH_CHECK(capacity <= 0x7fffffff, "the capacity must stay below 2^31");
    TORCH_CHECK(k_summary.size(1) * kv_block_size >= capacity, "k_summary: max_blocks * kv_block_size must cover the capacity (", capacity, ")");
    const int64_t bound = max_seqlen_new.value_or(capacity);
    TORCH_CHECK(bound >= 0, "max_seqlen_new must be non-negative");
    auto p = new_params<fa_block_summary_params>();
    p.k_summary = k_summary.data_ptr(); p.k_cache = k_cache.data_ptr();
    p.seqlens_old = static_cast<const int32_t *>(ptr(seqlens_old));
    p.seqlens_new = static_cast<const int32_t *>(seqlens_new.data_ptr());
    p.cache_batch_idx = static_cast<const int32_t *>(ptr(cache_batch_idx));
    p.page_table = static_cast<const int32_t *>(ptr(page_table));
    p.sum_slot_stride = k_summary.stride(0); p.sum_block_stride = k_summary.stride(1); p.sum_side_stride = k_summary.stride(2);
    p.sum_head_stride = k_summary.stride(3);
    p.cache_batch_stride = k_cache.stride(0); p.cache_row_stride = k_cache.stride(1); p.cache_head_stride = k_cache.stride(2);
    if (page_table.has_value()) { p.page_table_batch_stride = page_table->stride(0); p.page_size = (int32_t)k_cache.size(1); }
    p.b = (int32_t)batch_size; p.capacity = (int32_t)capacity; p.h_k = (int32_t)k_cache.size(2); p.d = (int32_t)k_cache.size(3);
    p.max_blocks = (int32_t)k_summary.size(1); p.block_size = (int32_t)kv_block_size;
    p.max_seqlen_new = (int32_t)std::min<int64_t>(bound, capacity);
    p.summary_dtype = dtype_code(k_summary); p.cache_dtype = dtype_code(k_cache);
    if (plan) {
        const char *name = fa_block_summary_update_plan_name(&p);
        TORCH_CHECK(name, "fa_block_summary_update refused (", fa_block_summary_update_validate(&p), "): ",
                    fa_strerror(fa_block_summary_update_validate(&p)));
        return name;
    }
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(k_summary.device());
    const int st = fa_block_summary_update(&p, current_stream(k_summary));
    TORCH_CHECK(st == 0, "fa_block_summary_update failed (", st, "): ", fa_strerror(st));
    return {};
}

std::string block_select_impl(const Tensor &q, const Tensor &k_summary, const Tensor &cache_seqlens, int64_t num_blocks,
                              int64_t kv_block_size, int64_t sink_blocks, int64_t local_blocks, const std::string &group_reduce,
                              const OptTensor &cache_batch_idx, const Tensor &kv_block_cnt, const Tensor &kv_block_idx,
                              const Tensor &scores, bool plan) {
    check_summary(k_summary, kv_block_size);
    TORCH_CHECK(q.is_cuda() && q.device() == k_summary.device() && q.scalar_type() == k_summary.scalar_type(),
                "q must be on the device of k_summary and have its dtype");
    TORCH_CHECK(q.dim() == 4, "q must have shape (batch_size, seqlen_q, num_heads, head_size); ragged queries are not supported");
    CHECK_LAST_CONTIGUOUS(q, "q must have contiguous last dimension");
    const int64_t batch_size = q.size(0), seqlen_q = q.size(1), num_heads = q.size(2), head_size = q.size(3);
    const int64_t max_blocks = k_summary.size(1), num_heads_k = k_summary.size(3);
    TORCH_CHECK(head_size == k_summary.size(4), "q must have the head_size of k_summary");
    TORCH_CHECK(num_heads_k > 0 && num_heads % num_heads_k == 0, "Number of heads in key/value must divide number of heads in query");
    TORCH_CHECK(seqlen_q >= 1 && seqlen_q * (num_heads / num_heads_k) <= FA_BLOCK_SELECT_MAX_ROWS,
                "seqlen_q * (num_heads / num_heads_k) must be in [1, ", FA_BLOCK_SELECT_MAX_ROWS, "]");
    TORCH_CHECK(max_blocks >= 1 && max_blocks <= FA_BLOCK_SELECT_MAX_BLOCKS, "k_summary: max_blocks must be in [1, ", FA_BLOCK_SELECT_MAX_BLOCKS,
                "], got ", max_blocks);
    TORCH_CHECK(group_reduce == "max" || group_reduce == "sum", "group_reduce must be \"max\" or \"sum\", got \"", group_reduce, "\"");
    TORCH_CHECK(sink_blocks >= 0 && local_blocks >= 0 && num_blocks >= sink_blocks + local_blocks,
                "num_blocks must be at least sink_blocks + local_blocks, both non-negative");
    check_fill(cache_seqlens, "cache_seqlens", batch_size, q);
    if (cache_batch_idx.has_value()) check_fill(*cache_batch_idx, "cache_batch_idx", batch_size, q);
    else TORCH_CHECK(batch_size <= k_summary.size(0), "the batch must fit the slots of k_summary without cache_batch_idx");
    for (const auto &[t, name] : {std::make_pair(&kv_block_cnt, "kv_block_cnt"), std::make_pair(&kv_block_idx, "kv_block_idx")})
        TORCH_CHECK(t->scalar_type() == at::kInt && t->is_cuda() && t->device() == q.device(), name, " must be an int32 tensor on the device of q");
    TORCH_CHECK(kv_block_cnt.sizes() == c10::IntArrayRef({batch_size, num_heads_k}), "kv_block_cnt must have shape (batch_size, num_heads_k)");
    TORCH_CHECK(kv_block_idx.dim() == 3 && kv_block_idx.size(0) == batch_size && kv_block_idx.size(1) == num_heads_k &&
                    (kv_block_idx.size(2) == 0 || kv_block_idx.stride(2) == 1),
                "kv_block_idx must have shape (batch_size, num_heads_k, width) with contiguous last dimension");
    TORCH_CHECK(kv_block_idx.size(2) >= num_blocks, "kv_block_idx must be at least num_blocks (", num_blocks, ") wide");
    TORCH_CHECK(scores.scalar_type() == at::kFloat && scores.is_cuda() && scores.device() == q.device() &&
                    scores.sizes() == c10::IntArrayRef({batch_size, num_heads_k, max_blocks}) && scores.stride(2) == 1,
                "scores must be fp32 (batch_size, num_heads_k, max_blocks) with contiguous last dimension");
    const Tensor qc = aligned_or_copy(q);
    auto p = new_params<fa_block_select_params>();
    p.q = qc.data_ptr(); p.k_summary = k_summary.data_ptr();
    p.cache_seqlens = static_cast<const int32_t *>(cache_seqlens.data_ptr());
    p.cache_batch_idx = static_cast<const int32_t *>(ptr(cache_batch_idx));
    p.scores = static_cast<float *>(scores.data_ptr());
    p.block_cnt = static_cast<int32_t *>(kv_block_cnt.data_ptr()); p.block_idx = static_cast<int32_t *>(kv_block_idx.data_ptr());
    p.q_batch_stride = qc.stride(0); p.q_row_stride = qc.stride(1); p.q_head_stride = qc.stride(2);
    p.sum_slot_stride = k_summary.stride(0); p.sum_block_stride = k_summary.stride(1); p.sum_side_stride = k_summary.stride(2);
    p.sum_head_stride = k_summary.stride(3);
    p.scores_batch_stride = scores.stride(0); p.scores_head_stride = scores.stride(1);
    p.cnt_batch_stride = kv_block_cnt.stride(0); p.cnt_head_stride = kv_block_cnt.stride(1);
    p.idx_batch_stride = kv_block_idx.stride(0); p.idx_head_stride = kv_block_idx.stride(1);
    p.b = (int32_t)batch_size; p.s_q = (int32_t)seqlen_q; p.h = (int32_t)num_heads; p.h_k = (int32_t)num_heads_k; p.d = (int32_t)head_size;
    p.max_blocks = (int32_t)max_blocks; p.list_width = (int32_t)kv_block_idx.size(2); p.block_size = (int32_t)kv_block_size;
    p.num_blocks = (int32_t)std::min<int64_t>(num_blocks, 0x7fffffff);
    p.sink_blocks = (int32_t)std::min<int64_t>(sink_blocks, 0x7fffffff); p.local_blocks = (int32_t)std::min<int64_t>(local_blocks, 0x7fffffff);
    p.group_reduce = group_reduce == "max" ? FA_BLOCK_REDUCE_MAX : FA_BLOCK_REDUCE_SUM;
    p.dtype = dtype_code(q);
    if (plan) {
        const char *name = fa_block_select_plan_name(&p);
        TORCH_CHECK(name, "fa_block_select refused (", fa_block_select_validate(&p), "): ", fa_strerror(fa_block_select_validate(&p)));
        return name;
    }
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(q.device());
    const int st = fa_block_select(&p, current_stream(q));
    TORCH_CHECK(st == 0, "fa_block_select failed (", st, "): ", fa_strerror(st));
    return {};
}

// ---- block-sparse prefill patterns (cute_interface.block_sparse_select; include/fa_block_pattern.h): what produces the lists
// cute_fwd_block_sparse / cute_bwd_block_sparse read.  Launches on the current stream, nothing is read on the host; every tensor
// the launches write, the workspace included, is an argument: capturable in a HIP graph.  The params of a call, checked; the
// three entries below launch with them, name their form, or size the workspace (`workspace` absent).
fa_block_pattern_params block_pattern_params(const Tensor &q, const Tensor &k, const Tensor &full_block_cnt, const Tensor &full_block_idx,
                                             const Tensor &mask_block_cnt, const Tensor &mask_block_idx, const OptTensor &q_block_cnt,
                                             const OptTensor &q_block_idx, const OptTensor &scores, const OptTensor &workspace,
                                             int64_t num_blocks, bool causal, int64_t window_left, int64_t window_right,
                                             int64_t sink_blocks, int64_t local_blocks) {
    TORCH_CHECK(q.is_cuda() && k.is_cuda() && k.device() == q.device(), "q and k must be on the same CUDA device");
    TORCH_CHECK(q.scalar_type() == at::kHalf || q.scalar_type() == at::kBFloat16, "q must be fp16 or bf16");
    TORCH_CHECK(k.scalar_type() == q.scalar_type(), "q and k must have the same dtype");
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4, "q must have shape (batch_size, seqlen_q, num_heads, head_size), k (batch_size, seqlen_k, num_heads_k, head_size)");
    CHECK_LAST_CONTIGUOUS(q, "q must have contiguous last dimension");
    CHECK_LAST_CONTIGUOUS(k, "k must have contiguous last dimension");
    const int64_t b = q.size(0), sq = q.size(1), h = q.size(2), d = q.size(3), sk = k.size(1), h_k = k.size(2);
    TORCH_CHECK(k.size(0) == b && k.size(3) == d, "k must have the batch size and the head_size of q");
    TORCH_CHECK(d <= 128 && d % 16 == 0, "head_size must be a multiple of 16, at most 128, got ", d);
    TORCH_CHECK(h_k > 0 && h % h_k == 0, "Number of heads in key/value must divide number of heads in query");
    TORCH_CHECK(sq >= 1 && sk >= 1 && sq <= 0x7fffff00, "seqlen_q and seqlen_k must be at least 1, seqlen_q below 2^31 - 256");
    const int64_t B = FA_BLOCK_PATTERN_BLOCK, nm = (sq + B - 1) / B, nk = (sk + B - 1) / B;
    TORCH_CHECK(nk <= FA_BLOCK_PATTERN_MAX_BLOCKS, "seqlen_k must give at most ", FA_BLOCK_PATTERN_MAX_BLOCKS, " key blocks, got ", nk);
    TORCH_CHECK(sink_blocks >= 0 && local_blocks >= 0 && num_blocks >= sink_blocks + local_blocks,
                "num_blocks must be at least sink_blocks + local_blocks, both non-negative");
    const auto check_out = [&](const Tensor &t, const char *name, at::ScalarType dtype, c10::IntArrayRef shape) {
        TORCH_CHECK(t.scalar_type() == dtype && t.is_cuda() && t.device() == q.device() && t.sizes() == shape && t.is_contiguous(), name,
                    " must be a contiguous ", dtype, " tensor of shape ", shape, " on the device of q");
    };
    check_out(full_block_cnt, "full_block_cnt", at::kInt, {b, h, nm});
    check_out(full_block_idx, "full_block_idx", at::kInt, {b, h, nm, nk});
    check_out(mask_block_cnt, "mask_block_cnt", at::kInt, {b, h, nm});
    check_out(mask_block_idx, "mask_block_idx", at::kInt, {b, h, nm, nk});
    TORCH_CHECK(q_block_cnt.has_value() == q_block_idx.has_value(), "q_block_cnt and q_block_idx must be specified together");
    if (q_block_cnt.has_value()) {
        check_out(*q_block_cnt, "q_block_cnt", at::kInt, {b, h, nk});
        check_out(*q_block_idx, "q_block_idx", at::kInt, {b, h, nk, nm});
    }
    if (scores.has_value()) check_out(*scores, "scores", at::kFloat, {b, h, nm, nk});
    if (workspace.has_value())
        TORCH_CHECK(workspace->is_cuda() && workspace->device() == q.device() && workspace->is_contiguous() && workspace->scalar_type() == at::kByte,
                    "workspace must be a contiguous uint8 tensor on the device of q");
    const auto clamp32 = [](int64_t v) { return (int32_t)std::max<int64_t>(std::min<int64_t>(v, 0x7fffffff), -1); };
    auto p = new_params<fa_block_pattern_params>();
    p.q = q.data_ptr(); p.k = k.data_ptr();
    p.full_block_cnt = static_cast<int32_t *>(full_block_cnt.data_ptr()); p.full_block_idx = static_cast<int32_t *>(full_block_idx.data_ptr());
    p.mask_block_cnt = static_cast<int32_t *>(mask_block_cnt.data_ptr()); p.mask_block_idx = static_cast<int32_t *>(mask_block_idx.data_ptr());
    p.q_block_cnt = static_cast<int32_t *>(ptr(q_block_cnt)); p.q_block_idx = static_cast<int32_t *>(ptr(q_block_idx));
    p.scores = static_cast<float *>(ptr(scores));
    p.workspace = ptr(workspace); p.workspace_bytes = workspace.has_value() ? (uint64_t)workspace->numel() : 0;
    p.q_batch_stride = q.stride(0); p.q_row_stride = q.stride(1); p.q_head_stride = q.stride(2);
    p.k_batch_stride = k.stride(0); p.k_row_stride = k.stride(1); p.k_head_stride = k.stride(2);
    p.b = (int32_t)b; p.sq = (int32_t)sq; p.sk = (int32_t)sk; p.h = (int32_t)h; p.h_k = (int32_t)h_k; p.d = (int32_t)d;
    p.num_blocks = clamp32(num_blocks); p.sink_blocks = clamp32(sink_blocks); p.local_blocks = clamp32(local_blocks);
    p.is_causal = causal; p.window_size_left = clamp32(window_left); p.window_size_right = clamp32(window_right);
    p.dtype = dtype_code(q);
    return p;
}

// ---- fused MLP activations (flash_attn.ops.activations, the epilogues of flash_attn.ops.fused_dense; include/fa_act.h).
// Launches on the current stream, no synchronisation; outputs and the dbias workspace come from the caching allocator:
// capturable in a HIP graph.
void check_act_rows(const Tensor &t, const char *name, int64_t M, int64_t H, at::ScalarType dtype) {
    check_rows("activation: ", "(M, H)", t, name, M, H);
    TORCH_CHECK(t.scalar_type() == dtype, "activation: ", name, " must have the dtype of pre");
}

void check_act_bias(const Tensor &t, int64_t H, at::ScalarType dtype) {
    TORCH_CHECK(t.is_cuda(), "activation: bias must be on CUDA");
    TORCH_CHECK(t.dim() == 1 && t.size(0) == H && t.is_contiguous(), "activation: bias must have shape (H) and be contiguous");
    TORCH_CHECK(t.scalar_type() == dtype || t.scalar_type() == at::kFloat, "activation: bias must have the dtype of pre or fp32");
}

// what both directions check of pre, up and bias; returns (M, H)
std::pair<int64_t, int64_t> check_act_inputs(const Tensor &pre, const OptTensor &up, const OptTensor &bias) {
    TORCH_CHECK(pre.is_cuda(), "activation: pre must be on CUDA");
    TORCH_CHECK(pre.dim() == 2, "activation: pre must have shape (M, H)");
    const int64_t M = pre.size(0), H = pre.size(1);
    TORCH_CHECK(H >= 1 && H <= std::numeric_limits<int32_t>::max(), "activation: pre must have 1 <= H < 2^31 columns");
    row_dtype_code("activation: ", pre.scalar_type(), "pre");
    check_act_rows(pre, "pre", M, H, pre.scalar_type());
    if (up.has_value()) {
        check_act_rows(*up, "up", M, H, pre.scalar_type());
        TORCH_CHECK(M <= 1 || up->stride(0) == pre.stride(0), "activation: gate and up must have the same row stride");
        TORCH_CHECK(!bias.has_value(), "activation: the gated form takes no bias");
    }
    if (bias.has_value()) check_act_bias(*bias, H, pre.scalar_type());
    return {M, H};
}

py::dict act_plan_dict(const fa_act_plan &l) { return plan_dict(l, {"cw", "threads", "grid_x", "grid_y", "rows_per_wg"}); }

// out (M, H) = act(pre + bias), or act(pre) * up with `up` (pre is then the gate).  With `plan` nothing is launched: *plan is
// what fa_act_fwd_plan says of the params the launch would get
Tensor act_fwd_impl(const Tensor &pre, const OptTensor &up, const OptTensor &bias, int64_t activation, fa_act_plan *plan) {
    const auto [M, H] = check_act_inputs(pre, up, bias);
    auto p = new_params<fa_act_fwd_params>();
    p.pre_dtype = p.up_dtype = p.out_dtype = row_dtype_code("activation: ", pre.scalar_type(), "pre");
    p.bias_dtype = bias.has_value() ? row_dtype_code("activation: ", bias->scalar_type(), "bias") : p.pre_dtype;
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(pre.device());
    Tensor out = at::empty({M, H}, pre.options());
    TORCH_CHECK(M > 0 || !plan, "activation: a plan needs at least one row");
    if (M == 0) return out;
    p.pre = pre.data_ptr(); p.up = ptr(up); p.bias = ptr(bias); p.out = out.data_ptr();
    p.pre_row_stride = pre.stride(0); p.out_row_stride = H;
    p.M = M; p.H = (int32_t)H; p.activation = (int32_t)activation; p.flags = up.has_value() ? FA_ACT_GATED : 0;
    launch_or_plan("fa_act_fwd", fa_act_fwd, fa_act_fwd_plan, p, plan, pre);
    return out;
}

// (dpre, dup, dbias, out).  Plain: dpre (M, H); dup empty.  Gated: dpre is dgate and dup (M, H) each, or with `packed` dpre is one
// (M, 2H) tensor whose first half is dup and whose second half is dgate (the order of F.glu: value, gate) and dup is empty.
// dbias (H, the dtype of bias, or of pre without one) with want_dbias, out (M, H) with recompute_out; empty otherwise
std::tuple<Tensor, Tensor, Tensor, Tensor> act_bwd_impl(const Tensor &dout, const Tensor &pre, const OptTensor &up, const OptTensor &bias,
                                                        int64_t activation, bool want_dbias, bool recompute_out, bool packed,
                                                        fa_act_plan *plan) {
    const auto [M, H] = check_act_inputs(pre, up, bias);
    check_act_rows(dout, "dout", M, H, pre.scalar_type());
    const bool gated = up.has_value();
    TORCH_CHECK(!(gated && want_dbias), "activation: the gated form has no dbias");
    TORCH_CHECK(gated || !packed, "activation: a packed gradient needs the gated form");
    auto p = new_params<fa_act_bwd_params>();
    p.pre_dtype = p.up_dtype = p.dout_dtype = p.dpre_dtype = p.dup_dtype = p.out_dtype = row_dtype_code("activation: ", pre.scalar_type(), "pre");
    p.bias_dtype = p.dbias_dtype = bias.has_value() ? row_dtype_code("activation: ", bias->scalar_type(), "bias") : p.pre_dtype;
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(pre.device());
    Tensor dpre = at::empty({M, packed ? 2 * H : H}, pre.options());
    Tensor dup = gated && !packed ? at::empty({M, H}, pre.options()) : none(pre.options());
    Tensor dbias = want_dbias ? at::empty({H}, bias.has_value() ? bias->options() : pre.options()) : none(pre.options());
    Tensor out = recompute_out ? at::empty({M, H}, pre.options()) : none(pre.options());
    TORCH_CHECK(M > 0 || !plan, "activation: a plan needs at least one row");
    if (M == 0) {  // (no rows, a zero sum, nothing of ours launched)
        if (want_dbias) dbias.zero_();
        return {dpre, dup, dbias, out};
    }
    p.M = M; p.H = (int32_t)H; p.activation = (int32_t)activation; p.flags = gated ? FA_ACT_GATED : 0;
    p.dbias = want_dbias ? dbias.data_ptr() : nullptr;
    p.workspace_bytes = fa_act_bwd_workspace_bytes(&p);
    Tensor workspace = at::empty({(int64_t)p.workspace_bytes}, pre.options().dtype(at::kByte));
    p.workspace = p.workspace_bytes ? workspace.data_ptr() : nullptr;
    p.pre = pre.data_ptr(); p.up = ptr(up); p.bias = ptr(bias); p.dout = dout.data_ptr();
    const int64_t es = pre.element_size();
    p.dpre = packed ? static_cast<char *>(dpre.data_ptr()) + H * es : dpre.data_ptr();
    p.dup = !gated ? nullptr : packed ? dpre.data_ptr() : dup.data_ptr();
    p.recompute_out = recompute_out ? out.data_ptr() : nullptr;
    p.pre_row_stride = pre.stride(0); p.dout_row_stride = dout.stride(0); p.dpre_row_stride = packed ? 2 * H : H; p.out_row_stride = H;
    launch_or_plan("fa_act_bwd", fa_act_bwd, fa_act_bwd_plan, p, plan, pre);
    return {dpre, dup, dbias, out};
}

// ---- GEMM with a fused bias + activation epilogue (flash_attn.ops.triton.linear; include/fa_gemm_act.h).  Launches on the
// current stream, no synchronisation; outputs and the dbias workspace come from the caching allocator: capturable in a HIP graph.
void check_gemm_act_matrix(const Tensor &t, const char *name, int64_t rows, int64_t cols, const Tensor &like) {
    TORCH_CHECK(t.is_cuda() && t.device() == like.device(), "gemm_act: ", name, " must be on the device of the first operand");
    TORCH_CHECK(t.dim() == 2 && t.size(0) == rows && t.size(1) == cols, "gemm_act: ", name, " has the wrong shape");
    TORCH_CHECK(t.stride(-1) == 1, "gemm_act: ", name, " must have contiguous last dimension");
    TORCH_CHECK(t.scalar_type() == like.scalar_type(), "gemm_act: ", name, " must have the dtype of the first operand");
}

py::dict gemm_act_plan_dict(const fa_gemm_act_plan &l) {
    return plan_dict(l, {"tile_m", "tile_n", "tile_k", "threads", "tiles_m", "tiles_n", "grid_x", "k_steps", "ragged_m", "ragged_n",
                         "ragged_k", "group_m", "partial_rows", "reduce_grid_x", "dtype", "dgrad"});
}

// (out, act_input) = act(x · weightᵀ + bias) and, with save_act_input, its argument; act_input is empty otherwise.  With `plan`
// nothing is launched: *plan is what fa_gemm_act_fwd_plan says of the params the launch would get
std::tuple<Tensor, Tensor> gemm_act_fwd_impl(const Tensor &x, const Tensor &weight, const OptTensor &bias, int64_t activation,
                                             bool save_act_input, fa_gemm_act_plan *plan) {
    TORCH_CHECK(x.is_cuda(), "gemm_act: x must be on CUDA");
    TORCH_CHECK(x.dim() == 2 && weight.dim() == 2, "gemm_act: x must have shape (M, K) and weight (N, K)");
    const int64_t M = x.size(0), K = x.size(1), N = weight.size(0);
    TORCH_CHECK(N <= std::numeric_limits<int32_t>::max() && K <= std::numeric_limits<int32_t>::max(), "gemm_act: N and K must be below 2^31");
    check_gemm_act_matrix(x, "x", M, K, x);
    check_gemm_act_matrix(weight, "weight", N, K, x);
    if (bias.has_value()) {
        TORCH_CHECK(bias->is_cuda() && bias->dim() == 1 && bias->size(0) == N && bias->is_contiguous(), "gemm_act: bias must have shape (N) and be contiguous");
        TORCH_CHECK(bias->scalar_type() == x.scalar_type(), "gemm_act: bias must have the dtype of x");
    }
    auto p = new_params<fa_gemm_act_fwd_params>();
    p.x_dtype = p.weight_dtype = p.bias_dtype = p.out_dtype = p.act_input_dtype = row_dtype_code("gemm_act: ", x.scalar_type(), "tensors", false);
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(x.device());
    Tensor out = at::empty({M, N}, x.options());
    Tensor act_input = save_act_input ? at::empty({M, N}, x.options()) : none(x.options());
    if (M == 0 && !plan) return {out, act_input};  // (the GEMM alone has a plan without a row, in both directions: no tiles)
    p.x = x.data_ptr(); p.weight = weight.data_ptr(); p.bias = ptr(bias); p.out = out.data_ptr();
    p.act_input = save_act_input ? act_input.data_ptr() : nullptr;
    if (M == 0) p.x = p.out = weight.data_ptr();  // (a plan: without a row x and out have no storage to point at, and it reads none)
    p.x_row_stride = x.stride(0); p.weight_row_stride = weight.stride(0); p.out_row_stride = N; p.act_input_row_stride = N;
    p.M = M; p.N = (int32_t)N; p.K = (int32_t)K; p.activation = (int32_t)activation;
    launch_or_plan("fa_gemm_act_fwd", fa_gemm_act_fwd, fa_gemm_act_fwd_plan, p, plan, x);
    return {out, act_input};
}

// (grad_in, dbias) = (grad_out · weight) ∘ act'(act_input) and, with want_dbias, its column sums; dbias is empty otherwise
std::tuple<Tensor, Tensor> gemm_act_dgrad_impl(const Tensor &grad_out, const Tensor &weight, const OptTensor &act_input, int64_t activation,
                                               bool want_dbias, fa_gemm_act_plan *plan) {
    TORCH_CHECK(grad_out.is_cuda(), "gemm_act: grad_out must be on CUDA");
    TORCH_CHECK(grad_out.dim() == 2 && weight.dim() == 2, "gemm_act: grad_out must have shape (M, K) and weight (K, N)");
    const int64_t M = grad_out.size(0), K = grad_out.size(1), N = weight.size(1);
    TORCH_CHECK(N <= std::numeric_limits<int32_t>::max() && K <= std::numeric_limits<int32_t>::max(), "gemm_act: N and K must be below 2^31");
    check_gemm_act_matrix(grad_out, "grad_out", M, K, grad_out);
    check_gemm_act_matrix(weight, "weight", K, N, grad_out);
    if (act_input.has_value()) check_gemm_act_matrix(*act_input, "act_input", M, N, grad_out);
    auto p = new_params<fa_gemm_act_dgrad_params>();
    p.grad_out_dtype = p.weight_dtype = p.act_input_dtype = p.grad_in_dtype = p.dbias_dtype = row_dtype_code("gemm_act: ", grad_out.scalar_type(), "tensors", false);
    c10::hip::HIPGuardMasqueradingAsCUDA device_guard(grad_out.device());
    Tensor grad_in = at::empty({M, N}, grad_out.options());
    Tensor dbias = want_dbias ? at::empty({N}, grad_out.options()) : none(grad_out.options());
    if (M == 0 && !plan) {  // (no rows, a zero sum, nothing of ours launched)
        if (want_dbias) dbias.zero_();
        return {grad_in, dbias};
    }
    p.M = M; p.N = (int32_t)N; p.K = (int32_t)K; p.activation = (int32_t)activation;
    p.dbias = want_dbias ? dbias.data_ptr() : nullptr;
    p.workspace_bytes = fa_gemm_act_dgrad_workspace_bytes(&p);
    Tensor workspace = at::empty({(int64_t)p.workspace_bytes}, grad_out.options().dtype(at::kByte));
    p.workspace = p.workspace_bytes ? workspace.data_ptr() : nullptr;
    p.grad_out = grad_out.data_ptr(); p.weight = weight.data_ptr(); p.act_input = ptr(act_input); p.grad_in = grad_in.data_ptr();
    if (M == 0) {  // (a plan, as in the forward: the tensors without a row have no storage to point at, and it reads none)
        p.grad_out = p.grad_in = weight.data_ptr();
        if (act_input.has_value()) p.act_input = weight.data_ptr();
    }
    p.grad_out_row_stride = grad_out.stride(0); p.weight_row_stride = weight.stride(0);
    p.act_input_row_stride = act_input.has_value() ? act_input->stride(0) : N; p.grad_in_row_stride = N;
    launch_or_plan("fa_gemm_act_dgrad", fa_gemm_act_dgrad, fa_gemm_act_dgrad_plan, p, plan, grad_out);
    return {grad_in, dbias};
}

// ---- the module's two entries of a row operator, both made of its one X_impl(args..., Plan *): `name` forwards args... and no
// plan; `name_plan` forwards the same args... and a zeroed Plan and returns it as a dict.  The signatures, the py::arg names
// and the arguments X_impl sees are those of one list, so "the plan of this call" cannot describe another call.
// (A parameter pack before a trailing parameter is not deduced: A... is the whole list and I... the positions before Plan *)
template <size_t... I, class R, class... A, class Plan, class... PyArg>
void def_row_op_at(std::index_sequence<I...>, py::module_ &m, const std::string &name, R (*impl)(A...),
                   py::dict (*to_dict)(const Plan &), const char *doc, const PyArg &...args) {
    using List = std::tuple<A...>;
    static_assert(sizeof...(A) == sizeof...(I) + 1 && std::is_same_v<std::tuple_element_t<sizeof...(I), List>, Plan *>,
                  "a row operator is X_impl(one argument per py::arg..., Plan *)");
    m.def(name.c_str(), [impl](std::tuple_element_t<I, List>... a) { return impl(std::forward<std::tuple_element_t<I, List>>(a)..., nullptr); },
          doc, args...);
    m.def((name + "_plan").c_str(),
          [impl, to_dict](std::tuple_element_t<I, List>... a) {
              Plan plan{};
              impl(std::forward<std::tuple_element_t<I, List>>(a)..., &plan);
              return to_dict(plan);
          },
          ("the form " + name + " takes with these arguments: its plan struct as a dict, nothing launched").c_str(), args...);
}

template <class Impl, class ToDict, class... PyArg>
void def_row_op(py::module_ &m, const char *name, Impl impl, ToDict to_dict, const char *doc, const PyArg &...args) {
    def_row_op_at(std::index_sequence_for<PyArg...>{}, m, name, impl, to_dict, doc, args...);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "FlashAttention (MI355X / gfx950 native kernels behind the flash_attn_2_cuda and flash_attn_3_cuda surfaces)";
    m.def("fwd", &mha_fwd, "Forward pass");
    m.def("varlen_fwd", &mha_varlen_fwd, "Forward pass (variable length)");
    m.def("bwd", &mha_bwd<false>, "Backward pass");
    m.def("varlen_bwd", &mha_varlen_bwd<false>, "Backward pass (variable length)");
    m.def("fwd_kvcache", &mha_fwd_kvcache, "Forward pass, with KV-cache");
    m.def("_fwd_kvcache_impl",  // fwd_kvcache_core under the positional list the Python surfaces call it by
          [](Tensor q, const Tensor &kcache, const Tensor &vcache, OptTensor k, OptTensor v, OptTensor seqlens_k, OptTensor rotary_cos,
             OptTensor rotary_sin, OptTensor cache_batch_idx, OptTensor leftpad_k, OptTensor block_table, OptTensor alibi_slopes,
             OptTensor out, double softmax_scale, bool is_causal, int64_t window_size_left, int64_t window_size_right, double softcap,
             bool is_rotary_interleaved, int64_t num_splits, int64_t page_multiple, OptTensor seqlens_rotary, OptTensor qv) {
              KvcacheArgs a;
              a.k_new = k; a.v_new = v; a.seqlens_k = seqlens_k; a.rotary_cos = rotary_cos; a.rotary_sin = rotary_sin;
              a.cache_batch_idx = cache_batch_idx; a.leftpad_k = leftpad_k; a.block_table = block_table; a.alibi_slopes = alibi_slopes;
              a.out = out; a.softmax_scale = softmax_scale; a.is_causal = is_causal; a.window_size_left = window_size_left;
              a.window_size_right = window_size_right; a.softcap = softcap; a.is_rotary_interleaved = is_rotary_interleaved;
              a.num_splits = num_splits; a.page_multiple = page_multiple; a.seqlens_rotary = seqlens_rotary; a.qv = qv;
              return fwd_kvcache_core(q, kcache, vcache, a);
          },
          "fwd_kvcache with the page-size rule of the calling surface (+ FA3 seqlens_rotary)",
          py::arg("q"), py::arg("kcache"), py::arg("vcache"), py::arg("k"), py::arg("v"), py::arg("seqlens_k"), py::arg("rotary_cos"),
          py::arg("rotary_sin"), py::arg("cache_batch_idx"), py::arg("leftpad_k"), py::arg("block_table"), py::arg("alibi_slopes"),
          py::arg("out"), py::arg("softmax_scale"), py::arg("is_causal"), py::arg("window_size_left"), py::arg("window_size_right"),
          py::arg("softcap"), py::arg("is_rotary_interleaved"), py::arg("num_splits"), py::arg("page_multiple"),
          py::arg("seqlens_rotary") = py::none(), py::arg("qv") = py::none());
    m.def("fa3_fwd", &fa3_fwd, "FA3 forward pass (flash_attn_3::fwd)");
    m.def("kvcache_append_fp8", &kvcache_append_fp8, "quantising in-place append of 16-bit rows to an fp8 (e4m3) KV cache; returns the new fill levels",
          py::arg("k_cache"), py::arg("v_cache"), py::arg("k"), py::arg("v"), py::arg("cache_seqlens"), py::arg("k_descale"),
          py::arg("v_descale"), py::arg("cu_seqlens_k_new") = py::none(), py::arg("max_seqlen_k_new") = py::none(),
          py::arg("cache_batch_idx") = py::none(), py::arg("page_table") = py::none(), py::arg("rotary_cos") = py::none(),
          py::arg("rotary_sin") = py::none(), py::arg("rotary_seqlens") = py::none(), py::arg("rotary_interleaved") = true);
    m.def("fwd_kvcache_sparse", &fwd_kvcache_sparse,
          "block-sparse attention over a KV cache: only the key blocks listed per kv head are read; returns (out, softmax_lse)",
          py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("kv_block_cnt"), py::arg("kv_block_idx"), py::arg("kv_block_size") = 128,
          py::arg("cache_seqlens") = py::none(), py::arg("cache_batch_idx") = py::none(), py::arg("cache_leftpad") = py::none(),
          py::arg("page_table") = py::none(), py::arg("cu_seqlens_q") = py::none(), py::arg("max_seqlen_q") = py::none(),
          py::arg("k_descale") = py::none(), py::arg("v_descale") = py::none(), py::arg("softmax_scale") = py::none(),
          py::arg("is_causal") = false, py::arg("window_size_left") = -1, py::arg("window_size_right") = -1, py::arg("softcap") = 0.0,
          py::arg("num_splits") = 0);
    m.def("fwd_kvcache_tree", &fwd_kvcache_tree,
          "tree attention over a KV cache: every query row sees the committed prefix and the draft keys its word names; returns (out, softmax_lse)",
          py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("tree_mask"), py::arg("cache_seqlens") = py::none(),
          py::arg("cache_batch_idx") = py::none(), py::arg("cache_leftpad") = py::none(), py::arg("page_table") = py::none(),
          py::arg("cu_seqlens_q") = py::none(), py::arg("max_seqlen_q") = py::none(), py::arg("k_descale") = py::none(),
          py::arg("v_descale") = py::none(), py::arg("softmax_scale") = py::none(), py::arg("softcap") = 0.0, py::arg("num_splits") = 0);
    for (const bool plan : {false, true}) {
        m.def(plan ? "kvcache_block_summary_update_plan" : "kvcache_block_summary_update",
              [plan](const Tensor &k_summary, const Tensor &k_cache, const OptTensor &seqlens_old, const Tensor &seqlens_new,
                     int64_t kv_block_size, c10::optional<int64_t> max_seqlen_new, const OptTensor &cache_batch_idx,
                     const OptTensor &page_table) {
                  return block_summary_update_impl(k_summary, k_cache, seqlens_old, seqlens_new, kv_block_size, max_seqlen_new,
                                                   cache_batch_idx, page_table, plan);
              },
              plan ? "the form kvcache_block_summary_update takes with these arguments, as text; nothing is launched"
                   : "per-block min / max summaries of the keys, updated in place for the rows [seqlens_old, seqlens_new) of a KV cache",
              py::arg("k_summary"), py::arg("k_cache"), py::arg("seqlens_old"), py::arg("seqlens_new"), py::arg("kv_block_size") = 128,
              py::arg("max_seqlen_new") = py::none(), py::arg("cache_batch_idx") = py::none(), py::arg("page_table") = py::none());
        m.def(plan ? "kvcache_select_blocks_plan" : "kvcache_select_blocks",
              [plan](const Tensor &q, const Tensor &k_summary, const Tensor &cache_seqlens, int64_t num_blocks, int64_t kv_block_size,
                     int64_t sink_blocks, int64_t local_blocks, const std::string &group_reduce, const OptTensor &cache_batch_idx,
                     const Tensor &kv_block_cnt, const Tensor &kv_block_idx, const Tensor &scores) {
                  return block_select_impl(q, k_summary, cache_seqlens, num_blocks, kv_block_size, sink_blocks, local_blocks, group_reduce,
                                           cache_batch_idx, kv_block_cnt, kv_block_idx, scores, plan);
              },
              plan ? "the form kvcache_select_blocks takes with these arguments, as text; nothing is launched"
                   : "Quest selection of key blocks from the block summaries: writes kv_block_cnt, kv_block_idx and scores",
              py::arg("q"), py::arg("k_summary"), py::arg("cache_seqlens"), py::arg("num_blocks"), py::arg("kv_block_size"),
              py::arg("sink_blocks"), py::arg("local_blocks"), py::arg("group_reduce"), py::arg("cache_batch_idx"),
              py::arg("kv_block_cnt"), py::arg("kv_block_idx"), py::arg("scores"));
    }
    for (const int mode : {0, 1, 2}) {  // the launch, the form, the workspace's bytes
        m.def(mode == 0 ? "block_pattern" : mode == 1 ? "block_pattern_plan" : "block_pattern_workspace_size",
              [mode](const Tensor &q, const Tensor &k, const Tensor &full_block_cnt, const Tensor &full_block_idx, const Tensor &mask_block_cnt,
                     const Tensor &mask_block_idx, const OptTensor &q_block_cnt, const OptTensor &q_block_idx, const OptTensor &scores,
                     const OptTensor &workspace, int64_t num_blocks, bool causal, int64_t window_size_left, int64_t window_size_right,
                     int64_t sink_blocks, int64_t local_blocks) -> py::object {
                  const auto p = block_pattern_params(q, k, full_block_cnt, full_block_idx, mask_block_cnt, mask_block_idx, q_block_cnt, q_block_idx,
                                                      scores, workspace, num_blocks, causal, window_size_left, window_size_right, sink_blocks,
                                                      local_blocks);
                  if (mode == 0) {
                      c10::hip::HIPGuardMasqueradingAsCUDA device_guard(q.device());
                      const int st = fa_block_pattern(&p, current_stream(q));
                      TORCH_CHECK(st == 0, "fa_block_pattern failed (", st, "): ", fa_strerror(st));
                      return py::none();
                  }
                  const int64_t bytes = fa_block_pattern_workspace_size(&p);
                  TORCH_CHECK(bytes >= 0, "fa_block_pattern refused (", bytes, "): ", fa_strerror((int)bytes));
                  if (mode == 2) return py::int_(bytes);
                  return py::str(fa_block_pattern_plan_name(&p));
              },
              mode == 0   ? "block-sparse pattern from pooled q . k scores: writes the forward lists, and the key-major lists and scores where given"
              : mode == 1 ? "the form block_pattern takes with these arguments, as text; nothing is launched"
                          : "the bytes of the workspace block_pattern needs with these arguments; nothing is launched",
              py::arg("q"), py::arg("k"), py::arg("full_block_cnt"), py::arg("full_block_idx"), py::arg("mask_block_cnt"),
              py::arg("mask_block_idx"), py::arg("q_block_cnt"), py::arg("q_block_idx"), py::arg("scores"), py::arg("workspace"),
              py::arg("num_blocks"), py::arg("causal"), py::arg("window_size_left"), py::arg("window_size_right"), py::arg("sink_blocks"),
              py::arg("local_blocks"));
    }
    m.def("fa3_bwd", &fa3_bwd, "FA3 backward pass (flash_attn_3::bwd)");
    m.def("fa3_fwd_combine", &fa3_fwd_combine, "FA3 merge of split-KV partials (flash_attn_3::fwd_combine)");
    m.def("cute_fwd", &cute_fwd, "cute surface forward (flash_attn.cute.interface, with learnable_sink)", py::arg("q"), py::arg("k"),
          py::arg("v"), py::arg("cu_seqlens_q"), py::arg("cu_seqlens_k"), py::arg("seqused_q"), py::arg("seqused_k"),
          py::arg("max_seqlen_q"), py::arg("max_seqlen_k"), py::arg("page_table"), py::arg("softmax_scale"), py::arg("is_causal"),
          py::arg("window_size_left"), py::arg("window_size_right"), py::arg("learnable_sink"), py::arg("softcap"),
          py::arg("num_splits"), py::arg("pack_gqa") = py::none());
    m.def("cute_fwd_block_sparse", &cute_fwd_block_sparse, "cute surface forward restricted to listed 128 x 128 blocks", py::arg("q"),
          py::arg("k"), py::arg("v"), py::arg("softmax_scale"), py::arg("causal"), py::arg("window_size_left"), py::arg("window_size_right"),
          py::arg("learnable_sink"), py::arg("softcap"), py::arg("num_splits"), py::arg("full_block_cnt"), py::arg("full_block_idx"),
          py::arg("mask_block_cnt"), py::arg("mask_block_idx"), py::arg("out") = py::none());
    m.def("cute_bwd", &cute_bwd, "cute surface backward: (dq, dk, dv, dsink)");
    m.def("cute_bwd_block_sparse", &cute_bwd_block_sparse, "cute surface backward over listed 128 x 128 blocks: (dq, dk, dv, dsink)");
    m.def("rotary_emb", &rotary_emb, "rotary embedding layer (apply_rotary): out = rotate(x), conjugate for the gradient", py::arg("x"),
          py::arg("cos"), py::arg("sin"), py::arg("seqlen_offsets") = 0, py::arg("cu_seqlens") = py::none(), py::arg("max_seqlen") = py::none(),
          py::arg("interleaved") = false, py::arg("inplace") = false, py::arg("conjugate") = false);
    def_row_op(m, "norm_fwd", norm_fwd_impl, norm_plan_dict,
               "fused residual-add + LayerNorm / RMSNorm forward: writes out (and residual_out); returns (mean, rstd)", py::arg("x"),
               py::arg("weight"), py::arg("bias"), py::arg("residual"), py::arg("rowscale"), py::arg("out"), py::arg("residual_out"),
               py::arg("eps"), py::arg("zero_centered_weight"), py::arg("is_rms_norm"));
    def_row_op(m, "norm_bwd", norm_bwd_impl, norm_plan_dict, "fused LayerNorm / RMSNorm backward: (dx, dw, db, dresidual_in, y)",
               py::arg("dy"), py::arg("x"), py::arg("weight"), py::arg("bias"), py::arg("mean"), py::arg("rstd"), py::arg("dresidual"),
               py::arg("rowscale"), py::arg("has_residual"), py::arg("zero_centered_weight"), py::arg("is_rms_norm"),
               py::arg("dx_dtype"), py::arg("recompute_output"));
    def_row_op(m, "xent_fwd", xent_fwd_impl, xent_plan_dict, "fused cross-entropy forward: (losses, lse, z_losses)", py::arg("logits"),
               py::arg("labels"), py::arg("precomputed_lse"), py::arg("smoothing"), py::arg("logit_scale"), py::arg("lse_square_scale"),
               py::arg("ignore_index"), py::arg("class_start_idx"), py::arg("total_classes"), py::arg("split"));
    def_row_op(m, "xent_bwd", xent_bwd_impl, xent_plan_dict, "fused cross-entropy backward: writes dlogits, which may be logits",
               py::arg("dloss"), py::arg("logits"), py::arg("labels"), py::arg("lse"), py::arg("dlogits"), py::arg("smoothing"),
               py::arg("logit_scale"), py::arg("lse_square_scale"), py::arg("ignore_index"), py::arg("class_start_idx"),
               py::arg("total_classes"));
    def_row_op(m, "act_fwd", act_fwd_impl, act_plan_dict, "fused MLP activation forward: act(pre + bias), or act(pre) * up",
               py::arg("pre"), py::arg("up"), py::arg("bias"), py::arg("activation"));
    def_row_op(m, "act_bwd", act_bwd_impl, act_plan_dict, "fused MLP activation backward: (dpre, dup, dbias, out)", py::arg("dout"),
               py::arg("pre"), py::arg("up"), py::arg("bias"), py::arg("activation"), py::arg("want_dbias"), py::arg("recompute_out"),
               py::arg("packed"));
    def_row_op(m, "gemm_act_fwd", gemm_act_fwd_impl, gemm_act_plan_dict,
               "GEMM with fused bias + activation: (out, act_input) of act(x @ weight.T + bias)", py::arg("x"), py::arg("weight"),
               py::arg("bias"), py::arg("activation"), py::arg("save_act_input"));
    def_row_op(m, "gemm_act_dgrad", gemm_act_dgrad_impl, gemm_act_plan_dict,
               "GEMM with the activation's derivative fused: (grad_in, dbias) of (grad_out @ weight) * act'(act_input)",
               py::arg("grad_out"), py::arg("weight"), py::arg("act_input"), py::arg("activation"), py::arg("want_dbias"));
    def_row_op(m, "dropout_norm_fwd", dropout_norm_fwd_impl, dropout_norm_plan_dict,
               "fused dropout + residual-add + LayerNorm / RMSNorm forward: (z0, z1, x, dmask0, dmask1, mu, rsigma, rng_state)",
               py::arg("x0"), py::arg("x1"), py::arg("residual"), py::arg("weight0"), py::arg("bias0"), py::arg("weight1"),
               py::arg("bias1"), py::arg("rowscale"), py::arg("colscale"), py::arg("p_dropout"), py::arg("eps"),
               py::arg("residual_in_fp32"), py::arg("is_rms_norm"), py::arg("want_x"), py::arg("return_dmask"));
    def_row_op(m, "dropout_norm_bwd", dropout_norm_bwd_impl, dropout_norm_plan_dict,
               "fused dropout + residual-add + LayerNorm / RMSNorm backward: (dx0, dx1, dresidual, dw0, db0, dw1, db1, dcolscale)",
               py::arg("dz0"), py::arg("dz1"), py::arg("dx"), py::arg("x"), py::arg("x0"), py::arg("mu"), py::arg("rsigma"),
               py::arg("weight0"), py::arg("weight1"), py::arg("rowscale"), py::arg("colscale"), py::arg("rng_state"),
               py::arg("p_dropout"), py::arg("has_x1"), py::arg("has_residual"), py::arg("has_bias"), py::arg("is_rms_norm"),
               py::arg("x0_dtype"));
    def_row_op(m, "sample_speculative", sample_speculative_impl, spec_sample_plan_dict,
               "fused verification of draft tokens (speculative sampling): (tokens, num_generated, p_tok, q_tok, accepted)",
               py::arg("logits"), py::arg("logits_draft"), py::arg("tokens_draft"), py::arg("top_k"), py::arg("top_p"),
               py::arg("temperature"), py::arg("u_acc"), py::arg("u_res"), py::arg("rng_state"), py::arg("stats"));
    def_row_op(m, "sample_speculative_tree", sample_speculative_tree_impl, tree_sample_plan_dict,
               "fused acceptance walk over a tree of draft tokens: (tokens, num_generated, path, path_len, p_tok, q_tok, visited, accepted)",
               py::arg("logits"), py::arg("logits_draft"), py::arg("tokens_draft"), py::arg("parents"), py::arg("top_k"), py::arg("top_p"),
               py::arg("temperature"), py::arg("u_acc"), py::arg("u_res"), py::arg("rng_state"), py::arg("stats"));
    m.def("sample", &sample, "fused top-k / top-p sampling of a token per row: (token, kept, mass)", py::arg("logits"), py::arg("top_k"),
          py::arg("top_p"), py::arg("temperature"), py::arg("u"), py::arg("rng_state"), py::arg("stats"));
    m.def("sample_filter_", &sample_filter_, "-inf over the entries top-k and top-p remove, in place: (kept, mass)", py::arg("logits"),
          py::arg("top_k"), py::arg("top_p"), py::arg("stats"));
    m.def("sample_plan", &sample_plan, "the form sample / sample_filter_ takes with these arguments: fa_sample_form as a dict, nothing launched",
          py::arg("logits"), py::arg("top_k"), py::arg("top_p"), py::arg("temperature"), py::arg("filter"), py::arg("stats"));
    m.def("sink_grad", &sink_grad, "gradient of a learnable sink from softmax_lse and softmax_d");
}
