// k_ngram.hip -- n-gram overlap: which documents of an id stream hold a window of w consecutive ids that also occurs in a
// reference stream (bpe_ngram_index_resident, bpe_ngram_overlap_resident).
// Part of bpe_kernels.hip, which includes the parts in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bpe_device.h"
#include "k_common.hip"
#include "k_dupdocs.hip"
#include "k_seldocs.hip"

namespace bpe {

// ---------------------------------------------------------------------------
// index: R [n_ref] + roff [n_ref_docs + 1] + w -> table of the distinct windows R[i : i + w) that lie inside one document
// overlap: ids [n] + off [n_docs + 1] (+ max_len, tail) + that table -> hits, first, ref_pos [n_docs], starts [n]
//   key(d) = ids[s_d : s_d + l_d], (s_d, l_d) = seldocs_slice of document d: what selection would emit for it.
//   A window starts at every key position k with k + w <= l_d (a key shorter than w has none); it is a hit when its w
//   ids equal, by value, those of a reference window.  hits[d] = the hit positions, first[d] = (s_d - off[d]) + the
//   lowest of them, ref_pos[d] = the lowest reference position at which that window starts.
// ONE pass serves both calls (k_ng_pass): laid out by the STREAM, a tile of positions per workgroup, the ids of a chunk
// of the tile and their halo of w - 1 positions in LDS, a lane per position: its document, its key, the hash of the
// window that starts there, and a walk through the open-addressing table from hash & mask.  A slot is tag << 32 | pos:
// the upper half of the hash next to the reference position whose window claimed the slot, which it holds for good; low
// [slot] is the lowest position of that window.  The hash only chooses where to look: a tag that agrees is followed by
// the comparison of the w ids, the window's own from LDS against the index's 64-bit copy of the reference.  The build
// runs the pass over that copy and claims or joins a slot; the query runs it over the corpus and only reads the table.
// No kernel waits for another workgroup.

constexpr uint32_t NG_THREADS = 256;
constexpr uint32_t NG_TILE_MAX = 65536;
constexpr uint32_t NG_CHUNK = 2048;       // positions of a tile whose ids are in LDS at a time (a smaller tile: all of it)
constexpr uint32_t NG_NGRAM_MAX = 64;
constexpr uint32_t NG_STAGE = 1024;       // documents of a tile whose starts are staged in LDS
constexpr uint32_t NG_AGG_ROUNDS = 2;     // documents a wave folds for all their lanes at once before each lane folds alone
constexpr uint32_t NG_NONE = ~0u;         // "no position": low[] of a free slot
constexpr unsigned long long NG_EMPTY = ~0ull;  // a free slot, and the (first, ref_pos) of a document without a hit: no
                                                // position reaches 2^32 - 1

// the hash of a window: its ids in order, each at its full width sign-extended to 64 bits (an int32 id and the int64 id
// of the same value hash alike), through a multiply and a fold that is not linear in them; ng_fin ends it
__device__ __forceinline__ unsigned long long ng_step(unsigned long long h, unsigned long long id) {
    h = (h ^ id) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 32);
}
// ... cut to `bits` bits (option "ng_hash_bits"; 0: every window starts at slot 0 with tag 0, every probe a comparison)
__device__ __forceinline__ unsigned long long ng_fin(unsigned long long h, uint32_t w, uint32_t bits) {
    h = dup_fmix(h + (unsigned long long)w * 0xD6E8FEB86659FD93ull);
    return bits >= 64 ? h : h & ((1ull << bits) - 1);
}

// the reference at 64 bits: the index's own copy of R[p0 : p1)
template <typename T>
__global__ void __launch_bounds__(256)
k_ng_widen(const T *__restrict__ ids, uint64_t p0, uint64_t p1, long long *__restrict__ ref) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = p0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p1; i += stride)  // bound: (p1 - p0) / stride + 1
        ref[i] = (long long)ids[i];
}

struct NgArgs {
    const void *ids;
    const unsigned long long *off;  // n_docs + 1 entries that passed k_rows_check
    unsigned long long n_docs;
    unsigned long long p0, p1;      // off[0] < off[n_docs]: the stream positions that belong to a document
    unsigned long long max_len;
    uint32_t tail, tile, ngram, hash_bits;
    const long long *ref;           // the index's copy of the reference, sign-extended
    unsigned long long *tab;        // tmask + 1 slots, a power of two above twice the reference windows
    uint32_t *low;                  // per slot: the lowest position of its window
    unsigned long long tmask;
    // the query: per document the hit count (zeroed) and first << 32 | ref_pos (NG_EMPTY); per position a byte (zeroed), or null
    uint32_t *cnt;
    unsigned long long *fmin;
    uint8_t *starts;
    // the build: {windows, distinct windows} (zeroed)
    unsigned long long *counters;
};

// The pass, laid out by the STREAM as k_mh_sig and k_dup_hash are: a workgroup owns a tile of A.tile consecutive
// positions in units of g = p + a, a = the elements by which `ids` is past a 16-byte boundary.  Position p lies in the
// document j with off[j] <= p < off[j + 1]; the documents of the tile's first and last position by one wave search each,
// the starts between them staged in LDS as 32-bit distances from the first (more than NG_STAGE of them: the same search
// over global memory).  The tile goes through LDS a chunk at a time:
//   1. the ids of the chunk's positions and of up to ngram - 1 beyond its end -- the halo: as far as the stream's
//      documents reach, whatever tile, chunk or document that is in; nothing outside [p0, p1) is read.
//   2. a lane per position, a wave on 64 consecutive ones (a strip): its document, the key of that (seldocs_slice), and
//      -- if a whole window of the key starts here -- the hash of its ids and the probe.  A window reads ids of its own
//      key alone: positions below s + l, whatever tile, chunk or document comes after.
//   3. BUILD: a free slot is claimed by atomicCAS with tag << 32 | p and holds that for good; a slot whose window equals
//      this one is joined; either way p folds into low[slot] by atomicMin.  Equal windows walk the same slots and pass
//      none that holds their ids, so they all stop at one entry; the table has more slots than there are windows, so a
//      free one is found before the table is through.
//      QUERY: the table is read-only.  A free slot ends the walk: no hit.  A hit counts 1 for its document and folds
//      (first << 32 | low[slot]) into the document's minimum; equal windows share one low, so the minimum is that of the
//      lowest hit.  The hits of a strip that belong to one document are folded by its lowest lane, for the first
//      NG_AGG_ROUNDS documents of the strip; sums and minima combine in any order, so nothing depends on scheduling.
template <typename T, bool BUILD>
__global__ void __launch_bounds__(NG_THREADS)
k_ng_pass(const NgArgs A) {
    __shared__ unsigned long long s_j[2];  // first and last document of the tile
    __shared__ uint32_t s_st[NG_STAGE + 4];
    __shared__ __attribute__((aligned(16))) T s_id[NG_CHUNK + NG_NGRAM_MAX];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const unsigned long long a = (unsigned long long)(((uintptr_t)A.ids & 15) / sizeof(T));
    const T *const ids_al = (const T *)A.ids - a;  // ids_al[g] is position g - a
    const unsigned long long G0 = a + A.p0, G1 = a + A.p1;
    const unsigned long long *const off = A.off;
    const uint32_t w = A.ngram;
    const uint32_t chunk = min(A.tile, NG_CHUNK);  // a power of two >= 64
    uint32_t n_win = 0, n_new = 0;  // BUILD: windows and claimed slots of this lane (below 2^32: so are the positions)
    const uint64_t t0 = G0 / A.tile, t1 = (G1 + A.tile - 1) / A.tile;
    for (uint64_t tile = t0 + blockIdx.x; tile < t1; tile += gridDim.x) {  // bound: the stream's tiles / gridDim.x + 1
        const unsigned long long g0 = tile * A.tile, g1 = min(g0 + (unsigned long long)A.tile, G1);
        const unsigned long long gb = max(g0, G0);
        const unsigned long long p_lo = gb - a, p_hi = g1 - a;  // the tile's positions: [p_lo, p_hi), never empty
        __syncthreads();  // (the staging area of the tile before is free)
        if (tid < 128) {
            const unsigned long long j = seldocs_wave_search(off, A.n_docs, tid < 64 ? p_lo : p_hi - 1, lane);
            if (lane == 0) s_j[tid >> 6] = j;
        }
        __syncthreads();
        const unsigned long long j_lo = s_j[0], j_hi = s_j[1];
        const unsigned long long cnt = j_hi - j_lo + 2;  // off[j_lo] .. off[j_hi + 1], j_hi + 1 <= n_docs
        const unsigned long long base = off[j_lo];       // (every offset is below 2^32: the distances fit)
        const bool staged = cnt <= (unsigned long long)NG_STAGE + 1;
        if (staged)
            for (uint32_t k = tid; k < (uint32_t)cnt; k += NG_THREADS)  // bound: (NG_STAGE + 1) / NG_THREADS + 1
                s_st[k] = (uint32_t)(off[j_lo + k] - base);
        for (unsigned long long c0 = g0; c0 < g1; c0 += chunk) {  // bound: A.tile / chunk <= 32
            const unsigned long long c1 = min(c0 + (unsigned long long)chunk, g1), cb = max(c0, gb);
            if (c1 <= cb) continue;  // (a chunk in front of the first document; the same in every lane)
            __syncthreads();         // (the staged starts are there; the chunk before is through)
            const unsigned long long te = min(c1 + w - 1, G1);
            for (unsigned long long g = cb + tid; g < te; g += NG_THREADS)  // bound: (chunk + ngram) / NG_THREADS + 1
                s_id[g - c0] = ids_al[g];
            __syncthreads();
            // bound: chunk / NG_THREADS + 1 <= 8 rounds, the same count in every lane: the ballots below see whole waves
            for (uint32_t i0 = 0; i0 < chunk; i0 += NG_THREADS) {
                const uint32_t i = i0 + tid;
                const unsigned long long g = c0 + i;
                bool win = false, hit = false;
                uint32_t D = NG_NONE, pos = 0, first = 0, lowv = 0;
                if (i < chunk && g >= cb && g < c1) {
                    const unsigned long long p = g - a;  // p_lo <= p < p_hi: off[j_lo] <= p < off[j_hi + 1]
                    unsigned long long j, o0, o1;
                    if (staged) {
                        const uint32_t pr = (uint32_t)(p - base);
                        uint32_t lo = 1, hi = (uint32_t)(j_hi - j_lo) + 1;
                        while (lo < hi) {  // bound: log2 of the staged starts
                            const uint32_t mid = (lo + hi) >> 1;
                            if (s_st[mid] > pr) hi = mid; else lo = mid + 1;
                        }
                        j = j_lo + lo - 1;
                        o0 = base + s_st[lo - 1];
                        o1 = base + s_st[lo];
                    } else {
                        unsigned long long lo = j_lo + 1, hi = j_hi + 1;
                        while (lo < hi) {  // bound: log2 of the tile's documents
                            const unsigned long long mid = lo + ((hi - lo) >> 1);
                            if (off[mid] > p) hi = mid; else lo = mid + 1;
                        }
                        j = lo - 1;
                        o0 = off[j];
                        o1 = off[j + 1];
                    }
                    uint32_t kl, ks;
                    seldocs_slice(o0, o1, A.max_len, A.tail, kl, ks);
                    const uint32_t kk = (uint32_t)p - ks;  // (p < ks wraps beyond every length)
                    // its ids are key[kk .. kk + w), kk + w <= kl: positions below ks + kl <= p1, and below
                    // c1 + w - 1 -- all of them among the ids above
                    win = (uint32_t)p >= ks && kl >= w && kk <= kl - w;
                    D = (uint32_t)j;  // n_docs < 2^32 - 1
                    pos = (uint32_t)p;
                    first = (ks - (uint32_t)o0) + kk;
                }
                if (win) {
                    unsigned long long h = 0;
                    for (uint32_t k = 0; k < w; k++) h = ng_step(h, (unsigned long long)(long long)s_id[i + k]);  // bound: w <= 64
                    h = ng_fin(h, w, A.hash_bits);
                    const uint32_t tag = (uint32_t)(h >> 32);
                    unsigned long long slot = h & A.tmask;
                    if (BUILD) n_win++;
                    for (unsigned long long probe = 0; probe <= A.tmask; probe++, slot = (slot + 1) & A.tmask) {  // bound: the table's slots
                        unsigned long long v;
                        if (BUILD) {
                            v = __hip_atomic_load(&A.tab[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (v == NG_EMPTY) {
                                v = atomicCAS(&A.tab[slot], NG_EMPTY, ((unsigned long long)tag << 32) | pos);
                                if (v == NG_EMPTY) {  // claimed: the slot holds this window from now on
                                    atomicMin(&A.low[slot], pos);
                                    n_new++;
                                    break;
                                }
                            }
                        } else {
                            v = A.tab[slot];
                            if (v == NG_EMPTY) break;
                        }
                        if ((uint32_t)(v >> 32) != tag) continue;
                        // (the copy of the reference is read-only for both passes: the window at v can be read at once)
                        const long long *const r = A.ref + (uint32_t)v;
                        bool eq = true;
                        for (uint32_t k = 0; k < w; k++)  // bound: w <= 64, early exit on the first difference
                            if ((long long)s_id[i + k] != r[k]) {
                                eq = false;
                                break;
                            }
                        if (!eq) continue;
                        if (BUILD) {
                            atomicMin(&A.low[slot], pos);
                        } else {
                            hit = true;
                            lowv = A.low[slot];
                        }
                        break;
                    }
                }
                if (!BUILD) {
                    if (hit && A.starts) A.starts[pos] = 1;
                    const unsigned long long key = ((unsigned long long)first << 32) | lowv;
                    bool open = hit;
                    for (uint32_t round = 0; round < NG_AGG_ROUNDS; round++) {  // bound: a constant
                        const unsigned long long bal = __ballot(open);
                        if (!bal) break;
                        const int src = (int)__ffsll(bal) - 1;
                        const uint32_t d0 = __shfl(D, src);
                        const bool same = open && D == d0;
                        const unsigned long long m = __ballot(same);
                        // (src is the lowest lane of m: the lowest position, so the lowest `first`, is its own)
                        if ((int)lane == src) {
                            atomicAdd(&A.cnt[d0], (uint32_t)__popcll(m));
                            atomicMin(&A.fmin[d0], key);
                        }
                        open = open && !same;
                    }
                    if (open) {
                        atomicAdd(&A.cnt[D], 1u);
                        atomicMin(&A.fmin[D], key);
                    }
                }
            }
        }
    }
    if (BUILD) {
#pragma unroll
        for (int d = 32; d; d >>= 1) {  // bound: 6 steps
            n_win += __shfl_down(n_win, d);
            n_new += __shfl_down(n_new, d);
        }
        if (lane == 0 && n_win) {
            atomicAdd(&A.counters[0], (unsigned long long)n_win);
            if (n_new) atomicAdd(&A.counters[1], (unsigned long long)n_new);
        }
    }
}

// Finish pass of the query: the packed rows into the caller's int64 columns (first and ref_pos may be null); the number
// of documents with a hit by one atomicAdd per workgroup.
__global__ void __launch_bounds__(256)
k_ng_finish(const uint32_t *__restrict__ cnt, const unsigned long long *__restrict__ fmin, uint64_t n_docs,
            long long *__restrict__ hits, long long *__restrict__ first, long long *__restrict__ ref_pos,
            unsigned long long *hit_docs) {
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    uint32_t mine = 0;  // (a thread sees n_docs / stride + 1 < 2^32 documents)
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n_docs; d += stride) {  // bound: n_docs / stride + 1
        const uint32_t c = cnt ? cnt[d] : 0;
        const unsigned long long m = c ? fmin[d] : NG_EMPTY;
        hits[d] = (long long)c;
        if (first) first[d] = c ? (long long)(m >> 32) : -1ll;
        if (ref_pos) ref_pos[d] = c ? (long long)(uint32_t)m : -1ll;
        mine += c != 0;
    }
#pragma unroll
    for (int k = 32; k; k >>= 1) mine += __shfl_down(mine, k);  // bound: 6 steps
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_n, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(hit_docs, (unsigned long long)s_n);
}

}  // namespace bpe
