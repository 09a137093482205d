// fa_kvcache_append_kv8.hip — fa_kvcache_append_kv8 (include/fa_fwd.h): the write half of an fp8 (e4m3) KV cache.  New 16-bit
// keys / values are rotated (keys only, the rotation code of the 16-bit appends: fa_rotary.h), divided by the descale of their
// (sequence, kv head), clamped to +-448, converted to e4m3 with round-to-nearest-even and stored at the rows the 16-bit appends
// would have written.  A translation unit of its own: fa_fwd_api.hip and fa_fwd_kv8_api.hip have their kernel sets pinned.
#include "fa_kvcache_append_kv8.h"

namespace {

// One new row by one wavefront: its lanes on the row's (head, slot) items in address order (rotary_slot_to: two 16-byte chunks
// of K, the same chunks of V; 8-byte stores).  Everything looked up per sequence -- fill level, cache entry, page, rotary
// position, the descale rows -- is wave-uniform.  64-bit addresses from a per-row base.
template <typename T>
__device__ __forceinline__ void append_row_kv8(const fa_kvcache_append_kv8_params &p, int lane, int seq, int i, int64_t k_off,
                                               int64_t v_off) {
    fa::Kv8AppendRow<T> r;
    if (!fa::kv8_append_row<T>(p, seq, i, k_off, v_off, r)) return;  // past the capacity: dropped (wave-uniform)
    const int slots = (p.d / 8 + 1) / 2, chunks = p.d >> 3, items = p.h_k * slots;
    for (int it = lane; it < items; it += 64) {
        const int hd = it / slots, slot = it % slots;
        const float k_inv = 1.0f / (r.kds ? r.kds[hd * p.k_descale_head_stride] : 1.0f);
        const float v_inv = 1.0f / (r.vds ? r.vds[hd * p.v_descale_head_stride] : 1.0f);
        uint8_t *kd = r.kd + hd * p.kcache_head_stride;
        fa::rotary_slot_to<T>(r.ks + hd * p.knew_head_stride, p.d, r.rd, p.rotary_interleaved != 0, slot, r.cr, r.sr,
                              [&](int c, uint4 w) { *reinterpret_cast<uint2 *>(kd + c * 8) = fa::quantise8<T>(w, k_inv); });
        // V: the same enumeration without a rotary part (slot -> chunks 2 slot, 2 slot + 1)
        const T *vs = r.vs + hd * p.vnew_head_stride;
        uint8_t *vd = r.vd + hd * p.vcache_head_stride;
        const int c0 = 2 * slot, c1 = 2 * slot + 1;
        if (c0 < chunks) *reinterpret_cast<uint2 *>(vd + c0 * 8) = fa::quantise8<T>(*reinterpret_cast<const uint4 *>(vs + c0 * 8), v_inv);
        if (c1 < chunks) *reinterpret_cast<uint2 *>(vd + c1 * 8) = fa::quantise8<T>(*reinterpret_cast<const uint4 *>(vs + c1 * 8), v_inv);
    }
}

// (the rows over the wavefronts: fa::kv8_append_rows)
template <typename T>
__global__ __launch_bounds__(256) void kvcache_append_kv8_kernel(const fa_kvcache_append_kv8_params p) {
    const int lane = threadIdx.x & 63;
    fa::kv8_append_rows(p, [&](int seq, int i, int64_t k_off, int64_t v_off) __attribute__((always_inline)) {
        append_row_kv8<T>(p, lane, seq, i, k_off, v_off);
    });
}

}  // namespace

extern "C" {

uint32_t fa_kvcache_append_kv8_params_size(void) { return (uint32_t)sizeof(fa_kvcache_append_kv8_params); }

int fa_kvcache_append_kv8_validate(const fa_kvcache_append_kv8_params *p) { return fa::kv8_append_validate(p, false); }

int fa_kvcache_append_kv8(const fa_kvcache_append_kv8_params *p, void *stream) {
    const int st = fa_kvcache_append_kv8_validate(p);
    if (st != FA_OK) return st;
    return fa::kv8_append_launch(p, kvcache_append_kv8_kernel<_Float16>, kvcache_append_kv8_kernel<__bf16>, stream);
}

}  // extern "C"
