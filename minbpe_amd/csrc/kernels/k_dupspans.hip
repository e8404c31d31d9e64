// k_dupspans.hip -- span de-duplication: which windows of w consecutive ids of a document were already seen in an EARLIER
// document of the same stream, or anywhere earlier in it (bpe_dup_spans_resident).
// Part of bpe_kernels.hip, which includes the parts in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bpe_device.h"
#include "k_common.hip"
#include "k_dupdocs.hip"
#include "k_ngram.hip"
#include "k_repeat.hip"
#include "k_seldocs.hip"

namespace bpe {

// ---------------------------------------------------------------------------
// ids [n] + off [n_docs + 1] (+ max_len, tail) + w -> per document: seen windows, covered positions, the first seen
// window and where its ids first stand; per position a mark byte.
//   key(d) = ids[s_d : s_d + l_d], (s_d, l_d) = seldocs_slice of document d: what selection would emit for it.
//   A window starts at every stream position p with s_d <= p, p + w <= s_d + l_d.  Windows of ALL documents are compared
//   with one another, by the ids at their full width; low(W) = the lowest position at which a window equal to W starts.
//   The window at p of document d is SEEN if low(W) < s_d (an equal window starts inside an earlier document's key), with
//   `anywhere` if low(W) < p (every occurrence but the stream's first).  A key position i is COVERED if some seen k has
//   k <= i < k + w.
// Four passes, in stream order, none of which waits for another workgroup:
//   build  (k_ds_pass<T, true>)   every window into ONE open-addressing table over the stream: a slot (DsSlot, 16 bytes:
//                                 one line of memory per probe) is tag << 32 | position of the window that claimed it,
//                                 and the lowest position of its class
//   query  (k_ds_pass<T, false>)  the same walk, the table read-only: every window finds the slot of its class, reads its
//                                 lowest and applies the scope rule -- bit 0 of its mark byte, 1 into its document's
//                                 seen, first << 32 | low into its document's minimum
//   cover  (k_rp_cover)           k_repeat.hip's, unchanged, over this call's marks and rows: bit 0 means to it what it
//                                 means here
//   finish (k_ds_finish)          the packed rows into the caller's int64 columns
// Both k_ds_pass are laid out as k_ng_pass is (k_ngram.hip).  The hash only chooses where to look.  A slot is joined when
// its w ids equal this window's, the lane's own from LDS against the stream itself at the slot's position: the stream is
// read-only, and that position's window lies inside its own key.  Sums and minima: nothing depends on scheduling.

constexpr uint32_t DS_THREADS = 256;
constexpr uint32_t DS_TILE_MAX = 65536;
constexpr uint32_t DS_CHUNK = RP_CHUNK;       // the staging helpers and the cover pass are k_repeat.hip's: the same geometry
constexpr uint32_t DS_NGRAM_MAX = RP_NGRAM_MAX;
constexpr uint32_t DS_AGG_ROUNDS = 2;         // documents a wave folds for all their lanes at once before each lane folds alone

// A slot of the table.  Prefilled with 0xFF bytes: key = NG_EMPTY (free), low = NG_NONE.
struct __attribute__((aligned(16))) DsSlot {
    unsigned long long key;  // tag << 32 | the position of the window that claimed the slot, for good
    uint32_t low;            // the lowest position of its class
    uint32_t pad;
};
static_assert(sizeof(DsSlot) == 16, "a slot is 16 bytes");

struct DsArgs {
    const void *ids;
    const unsigned long long *off;  // n_docs + 1 entries that passed k_rows_check
    unsigned long long n_docs;
    unsigned long long p0, p1;      // off[0] < off[n_docs]: the stream positions that belong to a document
    unsigned long long max_len;
    uint32_t tail, tile, ngram, hash_bits;
    uint32_t anywhere;              // the scope: 0 = seen in an earlier document, 1 = seen anywhere earlier
    DsSlot *tab;                    // `slots` slots (0xFF bytes)
    unsigned long long slots;       // 2 (p1 - p0) + 1: more than twice the windows, so a walk ends before the table is through
    uint8_t *marks;                 // [n], zeroed inside [p0, p1): bit 0 where a seen window starts (query)
    uint32_t *seen;                 // per document: its seen windows (zeroed)
    unsigned long long *fmin;       // per document: first << 32 | low of its first seen window (NG_EMPTY)
    unsigned long long *counters;   // {windows, distinct windows, windows the query did not find} (zeroed)
};

// The build and the query, laid out by the STREAM exactly as k_ng_pass: a workgroup owns a tile of A.tile consecutive
// positions in units of g = p + a, a = the elements by which `ids` is past a 16-byte boundary; the tile goes through LDS
// a chunk at a time, the ids of the chunk's positions and of up to ngram - 1 beyond its end (the halo: as far as the
// stream's documents reach; nothing outside [p0, p1) is read); a lane per position, a wave on 64 consecutive ones.  A
// window reads ids of its own key alone.
// A window walks the table from (its hash spread over the slots) on and wraps.
//   BUILD: a free slot is claimed by atomicCAS with tag << 32 | p and holds that for good; a slot whose window equals
//     this one is joined; either way p folds into the slot's low by atomicMin (a joiner only if a load of low does not
//     already show a lower position).  Equal windows walk the same slots and
//     pass none that holds their ids, so they all stop at one entry; the table has more slots than there are windows, so
//     a free one is found before the table is through.
//   QUERY: after the build has completed (kernel order on the stream).  Every window finds the slot of its class; one
//     that does not adds to counters[2] and the call fails.
template <typename T, bool BUILD>
__global__ void __launch_bounds__(DS_THREADS)
k_ds_pass(const DsArgs A) {
    __shared__ unsigned long long s_j[2];  // first and last document of the tile
    __shared__ uint32_t s_st[RP_STAGE + 4];
    __shared__ __attribute__((aligned(16))) T s_id[DS_CHUNK + DS_NGRAM_MAX];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const unsigned long long a = (unsigned long long)(((uintptr_t)A.ids & 15) / sizeof(T));
    const T *const ids = (const T *)A.ids;
    const T *const ids_al = ids - a;  // ids_al[g] is position g - a
    const unsigned long long G0 = a + A.p0, G1 = a + A.p1;
    const unsigned long long *const off = A.off;
    const uint32_t w = A.ngram;
    const uint32_t chunk = min(A.tile, DS_CHUNK);  // a power of two >= 64
    uint32_t n_win = 0, n_new = 0;  // BUILD: windows and claimed slots of this lane (below 2^32: so are the positions)
    const uint64_t t0 = G0 / A.tile, t1 = (G1 + A.tile - 1) / A.tile;
    for (uint64_t tile = t0 + blockIdx.x; tile < t1; tile += gridDim.x) {  // bound: the stream's tiles / gridDim.x + 1
        const unsigned long long g0 = tile * A.tile, g1 = min(g0 + (unsigned long long)A.tile, G1);
        const unsigned long long gb = max(g0, G0);
        __syncthreads();  // (the staging area of the tile before is free)
        const RpDocs R = rp_docs_of_tile(off, A.n_docs, gb - a, g1 - a, s_j, s_st);  // [gb - a, g1 - a) is never empty
        for (unsigned long long c0 = g0; c0 < g1; c0 += chunk) {  // bound: A.tile / chunk <= 32
            const unsigned long long c1 = min(c0 + (unsigned long long)chunk, g1), cb = max(c0, gb);
            if (c1 <= cb) continue;  // (a chunk in front of the first document; the same in every lane)
            __syncthreads();         // (the staged starts are there; the chunk before is through)
            const unsigned long long te = min(c1 + w - 1, G1);
            for (unsigned long long g = cb + tid; g < te; g += DS_THREADS)  // bound: (chunk + ngram) / DS_THREADS + 1
                s_id[g - c0] = ids_al[g];
            __syncthreads();
            // bound: chunk / DS_THREADS + 1 <= 8 rounds, the same count in every lane: the ballots below see whole waves
            for (uint32_t i0 = 0; i0 < chunk; i0 += DS_THREADS) {
                const uint32_t i = i0 + tid;
                const unsigned long long g = c0 + i;
                bool win = false, seen = false;
                uint32_t D = NG_NONE, pos = 0, first = 0, lowv = 0, ks = 0;
                if (i < chunk && g >= cb && g < c1) {
                    const unsigned long long p = g - a;  // off[j_lo] <= p < off[j_hi + 1]
                    unsigned long long o0, o1;
                    const unsigned long long j = rp_doc_of(R, off, s_st, p, o0, o1);
                    uint32_t kl;
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
                    const uint32_t tag = (uint32_t)h ^ (uint32_t)(h >> 32);
                    // (the cut hash spread over the slots: the upper word of a 128-bit product is below `slots`)
                    unsigned long long at = __umul64hi(h * 0x9E3779B97F4A7C15ull, A.slots);
                    bool found = false;
                    if (BUILD) n_win++;
                    for (unsigned long long probe = 0; probe < A.slots; probe++, at = at + 1 == A.slots ? 0 : at + 1) {  // bound: the table's slots
                        DsSlot *const sl = A.tab + at;
                        unsigned long long v;
                        if (BUILD) {
                            v = __hip_atomic_load(&sl->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (v == NG_EMPTY) {
                                v = atomicCAS(&sl->key, NG_EMPTY, ((unsigned long long)tag << 32) | pos);
                                if (v == NG_EMPTY) {  // claimed: the slot holds this window from now on
                                    atomicMin(&sl->low, pos);
                                    n_new++;
                                    break;
                                }
                            }
                        } else {
                            v = sl->key;
                            if (v == NG_EMPTY) break;  // (never: the build put this window in)
                        }
                        if ((uint32_t)(v >> 32) != tag) continue;
                        const uint32_t q = (uint32_t)v;  // a window of some key: q + w <= p1
                        bool eq = true;
                        if (q != pos) {
                            const T *const r = ids + q;  // (the stream is read-only: the window at q can be read at once)
                            for (uint32_t k = 0; k < w; k++)  // bound: w <= 64, early exit on the first difference
                                if (s_id[i + k] != r[k]) {
                                    eq = false;
                                    break;
                                }
                        }
                        if (!eq) continue;
                        if (BUILD) {
                            // (low only falls: a position that a plain load already finds undercut has nothing to
                            // fold -- a block that a million documents share would otherwise queue a million atomics
                            // on each of its slots; a stale load only sends an atomicMin that changes nothing)
                            if (__hip_atomic_load(&sl->low, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > pos) atomicMin(&sl->low, pos);
                        } else {
                            found = true;
                            lowv = sl->low;  // <= pos: this window folded itself in
                            seen = lowv < (A.anywhere ? pos : ks);
                        }
                        break;
                    }
                    if (!BUILD && !found) atomicAdd(&A.counters[2], 1ull);
                }
                if (!BUILD) {
                    if (seen) A.marks[pos] = 1;
                    const unsigned long long key = ((unsigned long long)first << 32) | lowv;
                    bool open = seen;
                    for (uint32_t round = 0; round < DS_AGG_ROUNDS; round++) {  // bound: a constant
                        const unsigned long long bal = __ballot(open);
                        if (!bal) break;
                        const int src = (int)__ffsll(bal) - 1;
                        const uint32_t d0 = __shfl(D, src);
                        const bool same = open && D == d0;
                        const unsigned long long m = __ballot(same);
                        // (src is the lowest lane of m: the lowest position, so the lowest `first`, is its own)
                        if ((int)lane == src) {
                            atomicAdd(&A.seen[d0], (uint32_t)__popcll(m));
                            atomicMin(&A.fmin[d0], key);
                        }
                        open = open && !same;
                    }
                    if (open) {
                        atomicAdd(&A.seen[D], 1u);
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

// Finish pass: the packed rows into the caller's int64 columns, each of which may be null (so may seen, cov and fmin:
// no key held a window); the number of documents with a seen window by one atomicAdd per workgroup.
__global__ void __launch_bounds__(256)
k_ds_finish(const unsigned long long *__restrict__ off, uint64_t n_docs, unsigned long long max_len, uint32_t tail,
            uint32_t w, const uint32_t *__restrict__ seen, const uint32_t *__restrict__ cov,
            const unsigned long long *__restrict__ fmin, long long *__restrict__ length, long long *__restrict__ windows,
            long long *__restrict__ seen_out, long long *__restrict__ covered, long long *__restrict__ first,
            long long *__restrict__ src_pos, unsigned long long *seen_docs) {
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    uint32_t mine = 0;  // (a thread sees n_docs / stride + 1 < 2^32 documents)
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n_docs; d += stride) {  // bound: n_docs / stride + 1
        uint32_t kl, ks;
        seldocs_slice(off[d], off[d + 1], max_len, tail, kl, ks);
        const uint32_t nw = kl >= w ? kl - w + 1 : 0;
        const uint32_t c = seen && nw ? seen[d] : 0;
        const unsigned long long m = c ? fmin[d] : NG_EMPTY;
        if (length) length[d] = (long long)kl;
        if (windows) windows[d] = (long long)nw;
        if (seen_out) seen_out[d] = (long long)c;
        if (covered) covered[d] = cov && c ? (long long)cov[d] : 0ll;
        if (first) first[d] = c ? (long long)(m >> 32) : -1ll;
        if (src_pos) src_pos[d] = c ? (long long)(uint32_t)m : -1ll;
        mine += c != 0;
    }
#pragma unroll
    for (int k = 32; k; k >>= 1) mine += __shfl_down(mine, k);  // bound: 6 steps
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_n, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(seen_docs, (unsigned long long)s_n);
}

}  // namespace bpe
