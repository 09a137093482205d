// fa_kvcache_append_qv8.hip — fa_kvcache_append_qv8 (include/fa_fwd.h): the write half of an fp8 (e4m3) KV cache of the MLA
// shape, what fa_fwd_qv8 reads: a rotated k_pe row (head dim d <= 64) into k_cache and the latent row (d_v in [256, 512]) into
// v_cache, both as e4m3 bytes.  Conversion, placement, rotation and the rows over the wavefronts are those of
// fa_kvcache_append_kv8 (fa_kvcache_append_kv8.h); the lane-to-chunk map of a row is this unit's.  A translation unit of its
// own: fa_kvcache_append_kv8.hip has its kernel set pinned.
#include "fa_kvcache_append_kv8.h"

namespace {

// One new row by one wavefront.  A head of the row is d_v / 8 (32 ... 64) 16-byte chunks of V beside ceil(d / 16) (1 ... 4)
// rotary slots of K (rotary_slot_to: two chunks each), so the (head, slot) items of fa_kvcache_append_kv8 would leave the V
// chunks to 4 lanes.  Here a pass of the wavefront covers 64 consecutive V chunks of the row, counted through its heads -- lane
// l loads chunk `base + l` (16 bytes, 1 KiB per wavefront in address order) and stores its 8 bytes (512 B in address order) --
// and the K slots are counted from the other end: K item `base + 63 - l`.  They fall on the lanes a row's V chunks leave idle
// (h_k 1, d_v 256: lanes 0 ... 31 V, lanes 60 ... 63 K) and otherwise ride in the same pass, their loads issued behind the
// lane's V load and in front of its use (h_k 1, d 64 / d_v 512: one pass, 64 V chunks, lanes 60 ... 63 a K slot more).  There
// are never more K items than V chunks (4 against 32 per head), so the V chunks bound the passes.
template <typename T>
__device__ __forceinline__ void append_row_qv8(const fa_kvcache_append_kv8_params &p, int lane, int seq, int i, int64_t k_off,
                                               int64_t v_off) {
    fa::Kv8AppendRow<T> r;
    if (!fa::kv8_append_row<T>(p, seq, i, k_off, v_off, r)) return;  // past the capacity: dropped (wave-uniform)
    const int v_chunks = p.d_v >> 3, k_slots = (p.d / 8 + 1) / 2;
    const int v_items = p.h_k * v_chunks, k_items = p.h_k * k_slots;
    for (int base = 0; base < v_items; base += 64) {
        const int vi = base + lane, ki = base + 63 - lane;
        const int v_hd = vi / v_chunks, v_c = vi % v_chunks;
        uint4 v_w = make_uint4(0, 0, 0, 0);
        if (vi < v_items) v_w = *reinterpret_cast<const uint4 *>(r.vs + v_hd * p.vnew_head_stride + v_c * 8);
        if (ki < k_items) {
            const int hd = ki / k_slots, slot = ki % k_slots;
            const float k_inv = 1.0f / (r.kds ? r.kds[hd * p.k_descale_head_stride] : 1.0f);
            uint8_t *kd = r.kd + hd * p.kcache_head_stride;
            fa::rotary_slot_to<T>(r.ks + hd * p.knew_head_stride, p.d, r.rd, p.rotary_interleaved != 0, slot, r.cr, r.sr,
                                  [&](int c, uint4 w) { *reinterpret_cast<uint2 *>(kd + c * 8) = fa::quantise8<T>(w, k_inv); });
        }
        if (vi < v_items) {
            const float v_inv = 1.0f / (r.vds ? r.vds[v_hd * p.v_descale_head_stride] : 1.0f);
            *reinterpret_cast<uint2 *>(r.vd + v_hd * p.vcache_head_stride + v_c * 8) = fa::quantise8<T>(v_w, v_inv);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void kvcache_append_qv8_kernel(const fa_kvcache_append_kv8_params p) {
    const int lane = threadIdx.x & 63;
    fa::kv8_append_rows(p, [&](int seq, int i, int64_t k_off, int64_t v_off) __attribute__((always_inline)) {
        append_row_qv8<T>(p, lane, seq, i, k_off, v_off);
    });
}

}  // namespace

extern "C" {

int fa_kvcache_append_qv8_validate(const fa_kvcache_append_kv8_params *p) { return fa::kv8_append_validate(p, true); }

int fa_kvcache_append_qv8(const fa_kvcache_append_kv8_params *p, void *stream) {
    const int st = fa_kvcache_append_qv8_validate(p);
    if (st != FA_OK) return st;
    return fa::kv8_append_launch(p, kvcache_append_qv8_kernel<_Float16>, kvcache_append_qv8_kernel<__bf16>, stream);
}

}  // extern "C"
