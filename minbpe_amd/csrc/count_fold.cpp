// count_fold.cpp -- from one histogram of token ids to the histogram at any smaller vocabulary and to the token count at
// every vocabulary size (bpe_count_fold).
//
// Undoing merge t -> (a, b) turns every t into an a and a b: the stream grows by h[t] tokens, and h[t] moves into h[a] and
// h[b].  Walking t from the top of the merge list down applies DESIGN 4.6's E(t) to the counts instead of the ids, one
// merge at a time, so after the merges above k are undone h is the histogram the tokenizer of 256 + k entries makes.
//
// Host side on purpose: a chain of M dependent steps over 8 (256 + M) bytes that stay in the cache -- microseconds here,
// M dependent L2 round trips in one workgroup on the device.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "bpe_hip.h"

namespace {

inline bool add_to(uint64_t &x, uint64_t y) { return !__builtin_add_overflow(x, y, &x); }

// the shape bpe_project_set_merges asks for: merge r makes 256 + r out of ids below it, no pair twice
bool training_shape(const int32_t *merges, int32_t M) {
    std::vector<uint64_t> seen;
    seen.reserve((size_t)M);
    for (int32_t r = 0; r < M; r++) {
        const int32_t a = merges[2 * (size_t)r], b = merges[2 * (size_t)r + 1];
        if (a < 0 || b < 0 || a >= 256 + r || b >= 256 + r) return false;
        seen.push_back(((uint64_t)(uint32_t)a << 32) | (uint32_t)b);
    }
    std::sort(seen.begin(), seen.end());
    return std::adjacent_find(seen.begin(), seen.end()) == seen.end();
}

}  // namespace

extern "C" int bpe_count_fold(const int32_t *merges, int32_t M, const uint64_t *counts, uint64_t n_bins, int32_t vocab_size,
                              uint64_t *folded, uint64_t *curve) {
    if (M < 0 || (!merges && M) || !counts) return BPE_E_ARG;
    const int64_t top = 256 + (int64_t)M;
    if (vocab_size < 256 || (int64_t)vocab_size > top || n_bins < (uint64_t)top) return BPE_E_ARG;
    if (!training_shape(merges, M)) return BPE_E_ARG;
    std::vector<uint64_t> h(counts, counts + n_bins);
    if (curve) {
        uint64_t total = 0;
        for (uint64_t i = 0; i < n_bins; i++)
            if (!add_to(total, h[i])) return BPE_E_LIMIT;
        curve[M] = total;
    }
    const int64_t stop = curve ? 256 : (int64_t)vocab_size;  // the curve needs every merge undone, the histogram those above vocab_size
    for (int64_t t = top - 1; t >= stop; t--) {
        if (t == (int64_t)vocab_size - 1 && folded) std::copy(h.begin(), h.end(), folded);
        const uint64_t moved = h[(size_t)t];
        if (curve) {
            curve[t - 256] = curve[t - 255];
            if (!add_to(curve[t - 256], moved)) return BPE_E_LIMIT;
        }
        if (!add_to(h[(size_t)merges[2 * (size_t)(t - 256)]], moved)) return BPE_E_LIMIT;
        if (!add_to(h[(size_t)merges[2 * (size_t)(t - 256) + 1]], moved)) return BPE_E_LIMIT;
        h[(size_t)t] = 0;
    }
    // (vocab_size 256 with a curve, or no curve: the walk ended where the histogram is wanted)
    if (folded && (vocab_size == stop)) std::copy(h.begin(), h.end(), folded);
    return BPE_OK;
}
