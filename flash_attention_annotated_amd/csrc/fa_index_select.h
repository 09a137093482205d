// fa_index_select.h — the token top-k of the lightning indexer over one row of index logits that lives in global memory: the one
// text of the selection both units launch (fa_index_topk.hip: a decode-sized step, the row in the logits output;
// fa_index_prefill.hip: a token of a prompt, the row in the round's workspace).  What differs between them -- where the row and
// the list of a token lie and how many candidates n(b, i) it has -- is the caller's: the kernels around this body compute it.
//
// index_select_row: the whole workgroup calls it (blockDim.x a multiple of 64, at most 1024).  The cut by four 8-bit passes over
//   the order-preserving keys of the row (read from L2 each pass; equal digits of a wave are counted by ballot, so a row of equal
//   logits does not serialise on one LDS word), then wave w compacts its contiguous segment by ballots behind the counts of the
//   waves before it.  Integer logic only: a NaN logit is a key like any other.  Reads u[0, n) and nothing else.
#ifndef FA_INDEX_SELECT_H_
#define FA_INDEX_SELECT_H_

#include "fa_sample_device.h"

namespace fa_index_sel {

using namespace fa_row;
using fa_sample_dev::full_key;

constexpr int SELECT_SMALL = 256, SELECT_LARGE = 1024, SELECT_SMALL_KEYS = 4096;  // the selection's workgroup by capacity
constexpr int RADIX_BITS = 8, BINS = 1 << RADIX_BITS, PASSES = 32 / RADIX_BITS;

inline int select_threads(int capacity) { return capacity <= SELECT_SMALL_KEYS ? SELECT_SMALL : SELECT_LARGE; }

// idx[0, K) = the K = min(topk, n) positions of the highest u[0, n) ascending (equal logits: the lower position), idx[K, topk) = -1
__device__ __forceinline__ void index_select_row(const float *u, int32_t *idx, const int n, const int topk) {
    __shared__ uint32_t hist[BINS];
    __shared__ uint64_t part[MAX_WAVES];
    __shared__ uint32_t cut_digit, cut_above;
    __shared__ uint32_t wave_gt[MAX_WAVES], wave_eq[MAX_WAVES];
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = T >> 6;
    const int K = topk < n ? topk : n;
    for (int x = K + tid; x < topk; x += T) idx[x] = -1;
    if (K == n) {  // every candidate is chosen (uniform; n = 0 as well)
        for (int j = tid; j < n; j += T) idx[j] = j;
        return;
    }

    // the cut: the key `cut` of which `ties_in` >= 1 entries are chosen beside every entry above it (1 <= K < n)
    uint32_t prefix = 0, want = (uint32_t)K;
    for (int shift = 32 - RADIX_BITS; shift >= 0; shift -= RADIX_BITS) {
        for (int x = tid; x < BINS; x += T) hist[x] = 0;
        __syncthreads();
        for (int j0 = 0; j0 < n; j0 += T) {  // (uniform bounds: every lane takes part in the ballots)
            const int j = j0 + tid;
            const uint32_t key = j < n ? full_key(u[j] + 0.0f) : 0u;
            const bool in = j < n && (shift + RADIX_BITS == 32 || key >> (shift + RADIX_BITS) == prefix);
            const uint32_t digit = (key >> shift) & (BINS - 1);
            uint64_t todo = __ballot(in);
            for (int round = 0; round < 4 && todo; ++round) {  // the four most frequent-first digits of the wave: one add each
                const int leader = __ffsll((unsigned long long)todo) - 1;
                const uint32_t dl = __shfl(digit, leader, WAVE);
                const uint64_t same = __ballot(in && digit == dl);
                if (lane == leader) atomicAdd(&hist[dl], (uint32_t)__popcll(same));  // (counts: any order gives the same histogram)
                todo &= ~same;
            }
            if (todo >> lane & 1) atomicAdd(&hist[digit], 1u);
        }
        __syncthreads();
        const uint64_t mine = tid < BINS ? hist[BINS - 1 - tid] : 0u;  // thread t: digit 255 - t; `above`: the higher digits
        uint64_t total;
        const uint64_t above = wg_exclusive_scan(mine, part, total);
        if (tid < BINS && above < want && want <= above + mine) { cut_digit = BINS - 1 - tid; cut_above = (uint32_t)above; }
        __syncthreads();  // (one thread wrote: at least `want` entries carry the prefix)
        prefix = prefix << RADIX_BITS | cut_digit;
        want -= cut_above;
    }
    const uint32_t cut = prefix, ties_in = want;

    // ascending compaction: wave w owns the positions [w * seg, (w + 1) * seg), walked 64 at a time
    const int seg = ((n + nw - 1) / nw + WAVE - 1) / WAVE * WAVE;
    const int lo = wave * seg < n ? wave * seg : n, hi = lo + seg < n ? lo + seg : n;
    uint32_t gt = 0, eq = 0;
    for (int j0 = lo; j0 < hi; j0 += WAVE) {
        const int j = j0 + lane;
        const uint32_t key = j < hi ? full_key(u[j] + 0.0f) : 0u;
        gt += (uint32_t)__popcll(__ballot(j < hi && key > cut));
        eq += (uint32_t)__popcll(__ballot(j < hi && key == cut));
    }
    if (lane == 0) { wave_gt[wave] = gt; wave_eq[wave] = eq; }
    __syncthreads();
    uint32_t tie_run = 0, at = 0;  // the ties and the chosen positions before this wave's segment
    for (int v = 0; v < wave; ++v) {
        const uint32_t e = wave_eq[v], left = ties_in > tie_run ? ties_in - tie_run : 0u;
        at += wave_gt[v] + (e < left ? e : left);
        tie_run += e;
    }
    const uint64_t before = (1ull << lane) - 1ull;
    for (int j0 = lo; j0 < hi; j0 += WAVE) {
        const int j = j0 + lane;
        const uint32_t key = j < hi ? full_key(u[j] + 0.0f) : 0u;
        const bool is_eq = j < hi && key == cut;
        const uint64_t beq = __ballot(is_eq);
        const uint32_t rank = tie_run + (uint32_t)__popcll(beq & before);
        const bool chosen = j < hi && (key > cut || (is_eq && rank < ties_in));
        const uint64_t bc = __ballot(chosen);
        const uint32_t pos = at + (uint32_t)__popcll(bc & before);
        if (chosen && pos < (uint32_t)K) idx[pos] = j;  // (pos < K always with finite logits; the guard costs nothing)
        at += (uint32_t)__popcll(bc);
        tie_run += (uint32_t)__popcll(beq);
    }
}

}  // namespace fa_index_sel

#endif  // FA_INDEX_SELECT_H_
