// k_repeat.hip -- repetition statistics: how often the windows of w consecutive ids of a document occur again inside the
// SAME document (bpe_repeat_stats_resident).
// Part of bpe_kernels.hip, which includes the parts in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bpe_device.h"
#include "k_common.hip"
#include "k_dupdocs.hip"
#include "k_ngram.hip"
#include "k_seldocs.hip"

namespace bpe {

// ---------------------------------------------------------------------------
// ids [n] + off [n_docs + 1] (+ max_len, tail) + w -> per document: repeats, covered positions, the top window; per
// position a mark byte.
//   key(d) = ids[s_d : s_d + l_d], (s_d, l_d) = seldocs_slice of document d: what selection would emit for it.
//   A window starts at every key position k with k + w <= l_d.  Two windows of one document are equal when they hold the
//   same ids at their full width; position k is a REPEAT if an equal window starts at a lower position of the same key.
//   A key position i is COVERED if some repeat k has k <= i < k + w.  The top window is the one of the largest
//   multiplicity, among several the one whose first start is lowest.
// Four passes, in stream order, none of which waits for another workgroup:
//   insert (k_rp_pass<T, true>)   every window into an open-addressing table: a slot (RpSlot, 16 bytes: one line of
//                                 memory per probe) is tag << 32 | position of the window that claimed it, the lowest
//                                 position of its class and the size of the class.  The table is two slots per stream
//                                 position and every KEY has a region of its own in it, the 2 l_d slots of its
//                                 positions: windows of different documents never meet, and the slots a tile walks
//                                 are as local as its ids
//   read   (k_rp_pass<T, false>)  the same walk, the table read-only: a position that is not its slot's lowest is a
//                                 repeat -- bit 0 of its mark byte, 1 into its document's repeats --, the position that
//                                 is speaks for its class: count << 32 | ~lowest into the document's top by atomicMax
//   cover  (k_rp_cover)           the repeat marks of a chunk and of the 64 positions before it as one bit each in LDS; a
//                                 position is covered if one of the w bits that end at it is set, inside its own key
//   finish (k_rp_finish)          the packed rows into the caller's int64 columns
// Both k_rp_pass are laid out as k_ng_pass is (k_ngram.hip).  The hash only chooses where in the key's region to look.
// A slot is joined when its w ids equal this window's, the lane's own from LDS against the stream itself at the slot's
// position (a position of the same key: the region holds no other): the stream is read-only.  Sums, minima and one
// maximum: nothing depends on scheduling.

constexpr uint32_t RP_THREADS = 256;
constexpr uint32_t RP_TILE_MAX = 65536;
constexpr uint32_t RP_CHUNK = 2048;       // positions of a tile that are in LDS at a time (a smaller tile: all of it)
constexpr uint32_t RP_NGRAM_MAX = 64;
constexpr uint32_t RP_STAGE = 1024;       // documents of a tile whose starts are staged in LDS
constexpr uint32_t RP_AGG_ROUNDS = 2;     // documents a wave folds for all their lanes at once before each lane folds alone
constexpr uint32_t RP_STRIPS = RP_CHUNK / 64;

// A slot of the table.  Prefilled with 0xFF bytes: key = NG_EMPTY (free), low = NG_NONE, cnt = 2^32 - 1 -- the count of
// the class LESS ONE, mod 2^32, so that the first window brings it to 0 and one prefill serves all three.
struct __attribute__((aligned(16))) RpSlot {
    unsigned long long key;  // tag << 32 | the position of the window that claimed the slot, for good
    uint32_t low;            // the lowest position of its class
    uint32_t cnt;            // the windows of its class, less one
};
static_assert(sizeof(RpSlot) == 16, "a slot is 16 bytes");

// The documents of a tile [p_lo, p_hi) of stream positions, off[0] <= p_lo < p_hi <= off[n_docs]: the first and the last
// by one wave search each, the starts between them staged in LDS as 32-bit distances from the first (more than RP_STAGE
// of them: rp_doc_of searches global memory).  Called by the whole workgroup; a __syncthreads() must follow before
// rp_doc_of and one must have come since the last use of s_j and s_st.
struct RpDocs {
    unsigned long long j_lo, j_hi, base;
    bool staged;
};

__device__ __forceinline__ RpDocs rp_docs_of_tile(const unsigned long long *off, unsigned long long n_docs,
                                                  unsigned long long p_lo, unsigned long long p_hi,
                                                  unsigned long long *s_j, uint32_t *s_st) {
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    if (tid < 128) {
        const unsigned long long j = seldocs_wave_search(off, n_docs, tid < 64 ? p_lo : p_hi - 1, lane);
        if (lane == 0) s_j[tid >> 6] = j;
    }
    __syncthreads();
    RpDocs R;
    R.j_lo = s_j[0];
    R.j_hi = s_j[1];
    const unsigned long long cnt = R.j_hi - R.j_lo + 2;  // off[j_lo] .. off[j_hi + 1], j_hi + 1 <= n_docs
    R.base = off[R.j_lo];                                // (every offset is below 2^32: the distances fit)
    R.staged = cnt <= (unsigned long long)RP_STAGE + 1;
    if (R.staged)
        for (uint32_t k = tid; k < (uint32_t)cnt; k += RP_THREADS)  // bound: (RP_STAGE + 1) / RP_THREADS + 1
            s_st[k] = (uint32_t)(off[R.j_lo + k] - R.base);
    return R;
}

// the document j of position p of that tile, off[j] <= p < off[j + 1], and its two offsets
__device__ __forceinline__ unsigned long long rp_doc_of(const RpDocs &R, const unsigned long long *off, const uint32_t *s_st,
                                                        unsigned long long p, unsigned long long &o0,
                                                        unsigned long long &o1) {
    if (R.staged) {
        const uint32_t pr = (uint32_t)(p - R.base);
        uint32_t lo = 1, hi = (uint32_t)(R.j_hi - R.j_lo) + 1;
        while (lo < hi) {  // bound: log2 of the staged starts
            const uint32_t mid = (lo + hi) >> 1;
            if (s_st[mid] > pr) hi = mid; else lo = mid + 1;
        }
        o0 = R.base + s_st[lo - 1];
        o1 = R.base + s_st[lo];
        return R.j_lo + lo - 1;
    }
    unsigned long long lo = R.j_lo + 1, hi = R.j_hi + 1;
    while (lo < hi) {  // bound: log2 of the tile's documents
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        if (off[mid] > p) hi = mid; else lo = mid + 1;
    }
    o0 = off[lo - 1];
    o1 = off[lo];
    return lo - 1;
}

// 1 into sum[D] for every lane with `open`: the lanes of a strip that belong to one document are folded by its lowest
// lane, for the first RP_AGG_ROUNDS documents of the strip, then each lane alone.  Called by whole waves.
__device__ __forceinline__ void rp_wave_count(uint32_t *sum, uint32_t D, bool open, uint32_t lane) {
    for (uint32_t round = 0; round < RP_AGG_ROUNDS; round++) {  // bound: a constant
        const unsigned long long bal = __ballot(open);
        if (!bal) return;
        const int src = (int)__ffsll(bal) - 1;
        const uint32_t d0 = __shfl(D, src);
        const bool same = open && D == d0;
        const unsigned long long m = __ballot(same);
        if ((int)lane == src) atomicAdd(&sum[d0], (uint32_t)__popcll(m));
        open = open && !same;
    }
    if (open) atomicAdd(&sum[D], 1u);
}

struct RpArgs {
    const void *ids;
    const unsigned long long *off;  // n_docs + 1 entries that passed k_rows_check
    unsigned long long n_docs;
    unsigned long long p0, p1;      // off[0] < off[n_docs]: the stream positions that belong to a document
    unsigned long long max_len;
    uint32_t tail, tile, ngram, hash_bits;
    RpSlot *tab;                    // 2 (p1 - p0) slots (0xFF bytes): the key at [s, s + l) owns [2 (s - p0), 2 (s - p0) + 2 l)
    uint8_t *marks;                 // [n], zeroed: bit 0 where a repeat starts (read pass), bit 1 where covered (cover pass)
    uint32_t *rep;                  // per document: its repeats (zeroed)
    uint32_t *cov;                  // per document: its covered positions (zeroed)
    unsigned long long *top;        // per document: cnt << 32 | ~low of the classes of two windows and more (zeroed)
    uint32_t write_cover;           // cover pass: set bit 1 of the marks (they are the caller's)
};

// The insert pass and the read pass, laid out by the STREAM exactly as k_ng_pass: a workgroup owns a tile of A.tile
// consecutive positions in units of g = p + a, a = the elements by which `ids` is past a 16-byte boundary; the tile goes
// through LDS a chunk at a time, the ids of the chunk's positions and of up to ngram - 1 beyond its end (the halo: as
// far as the stream's documents reach; nothing outside [p0, p1) is read); a lane per position, a wave on 64 consecutive
// ones.  A window reads ids of its own key alone.
// A window walks the region of its key from hash % size on, size = min(2 l, 2^32 - 1) slots, and wraps inside it.
//   INSERT: a free slot is claimed by atomicCAS with tag << 32 | p and holds that for good; a slot whose window equals
//     this one is joined; either way p folds into the slot's low by atomicMin and 1 into its cnt.  Equal windows walk
//     the same slots and pass none that holds their ids, so they all stop at one entry; the region has as many slots
//     as the key has windows at the least (twice as many, but for a key of 2^31 ids and more), so every window finds
//     its slot before the region is through.
//   READ: after the insert pass has completed (kernel order on the stream).  Every window finds the slot of its class.
template <typename T, bool INSERT>
__global__ void __launch_bounds__(RP_THREADS)
k_rp_pass(const RpArgs A) {
    __shared__ unsigned long long s_j[2];  // first and last document of the tile
    __shared__ uint32_t s_st[RP_STAGE + 4];
    __shared__ __attribute__((aligned(16))) T s_id[RP_CHUNK + RP_NGRAM_MAX];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const unsigned long long a = (unsigned long long)(((uintptr_t)A.ids & 15) / sizeof(T));
    const T *const ids = (const T *)A.ids;
    const T *const ids_al = ids - a;  // ids_al[g] is position g - a
    const unsigned long long G0 = a + A.p0, G1 = a + A.p1;
    const unsigned long long *const off = A.off;
    const uint32_t w = A.ngram;
    const uint32_t chunk = min(A.tile, RP_CHUNK);  // a power of two >= 64
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
            for (unsigned long long g = cb + tid; g < te; g += RP_THREADS)  // bound: (chunk + ngram) / RP_THREADS + 1
                s_id[g - c0] = ids_al[g];
            __syncthreads();
            // bound: chunk / RP_THREADS + 1 <= 8 rounds, the same count in every lane: the ballots below see whole waves
            for (uint32_t i0 = 0; i0 < chunk; i0 += RP_THREADS) {
                const uint32_t i = i0 + tid;
                const unsigned long long g = c0 + i;
                bool win = false, repeat = false;
                uint32_t D = NG_NONE, pos = 0, size = 0;
                RpSlot *region = nullptr;
                if (i < chunk && g >= cb && g < c1) {
                    const unsigned long long p = g - a;  // off[j_lo] <= p < off[j_hi + 1]
                    unsigned long long o0, o1;
                    const unsigned long long j = rp_doc_of(R, off, s_st, p, o0, o1);
                    uint32_t kl, ks;
                    seldocs_slice(o0, o1, A.max_len, A.tail, kl, ks);
                    const uint32_t kk = (uint32_t)p - ks;  // (p < ks wraps beyond every length)
                    // its ids are key[kk .. kk + w), kk + w <= kl: positions below ks + kl <= p1, and below
                    // c1 + w - 1 -- all of them among the ids above
                    win = (uint32_t)p >= ks && kl >= w && kk <= kl - w;
                    D = (uint32_t)j;  // n_docs < 2^32 - 1
                    pos = (uint32_t)p;
                    region = A.tab + 2 * ((unsigned long long)ks - A.p0);  // (win: p0 <= ks, and ks + kl <= p1)
                    size = (uint32_t)min(2ull * kl, 0xFFFFFFFFull);
                }
                if (win) {
                    unsigned long long h = 0;
                    for (uint32_t k = 0; k < w; k++) h = ng_step(h, (unsigned long long)(long long)s_id[i + k]);  // bound: w <= 64
                    h = ng_fin(h, w, A.hash_bits);
                    const uint32_t tag = (uint32_t)(h >> 32);
                    uint32_t at = (uint32_t)h % size;
                    for (uint32_t probe = 0; probe < size; probe++, at = at + 1 == size ? 0 : at + 1) {  // bound: the region's slots
                        RpSlot *const sl = region + at;
                        unsigned long long v;
                        if (INSERT) {
                            v = __hip_atomic_load(&sl->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (v == NG_EMPTY) {
                                v = atomicCAS(&sl->key, NG_EMPTY, ((unsigned long long)tag << 32) | pos);
                                if (v == NG_EMPTY) {  // claimed: the slot holds this window from now on
                                    atomicMin(&sl->low, pos);
                                    atomicAdd(&sl->cnt, 1u);
                                    break;
                                }
                            }
                        } else {
                            v = sl->key;
                            if (v == NG_EMPTY) break;  // (never: the insert pass put this window in)
                        }
                        if ((uint32_t)(v >> 32) != tag) continue;
                        const uint32_t q = (uint32_t)v;  // a window of this key: q + w <= ks + kl <= p1
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
                        if (INSERT) {
                            atomicMin(&sl->low, pos);
                            atomicAdd(&sl->cnt, 1u);
                        } else if (sl->low != pos) {
                            repeat = true;
                        } else {
                            // the lowest of its class speaks for it.  A class of one window never beats the key's
                            // first window, which the finish pass stands in for: only classes of two and more fold
                            const uint32_t c = sl->cnt + 1u;
                            if (c > 1) atomicMax(&A.top[D], ((unsigned long long)c << 32) | (uint32_t)~pos);
                        }
                        break;
                    }
                }
                if (!INSERT) {
                    if (repeat) A.marks[pos] = 1;
                    rp_wave_count(A.rep, D, repeat, lane);
                }
            }
        }
    }
}

// The cover pass, laid out by the stream positions themselves: a workgroup owns a tile of A.tile consecutive positions
// p (tiles count from 0, so a strip of 64 positions begins at a multiple of 64), a chunk of it at a time.  Bit 0 of the
// marks of the chunk's strips and of the strip before it (the backward halo: w - 1 <= 63 positions) go to LDS as one
// 64-bit word per strip, by ballot; a chunk without a repeat in them is through.  Otherwise a lane per position: its
// document, its key, and the bits of the positions [max(s, p - w + 1), p] out of two words.
__global__ void __launch_bounds__(RP_THREADS)
k_rp_cover(const RpArgs A) {
    __shared__ unsigned long long s_j[2];
    __shared__ uint32_t s_st[RP_STAGE + 4];
    __shared__ unsigned long long s_bits[RP_STRIPS + 1];  // [0]: the strip before the chunk
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long *const off = A.off;
    const uint32_t w = A.ngram;
    const uint32_t chunk = min(A.tile, RP_CHUNK);  // a power of two >= 64
    const uint32_t strips = chunk / 64;
    const uint64_t t0 = A.p0 / A.tile, t1 = (A.p1 + A.tile - 1) / A.tile;
    for (uint64_t tile = t0 + blockIdx.x; tile < t1; tile += gridDim.x) {  // bound: the stream's tiles / gridDim.x + 1
        const unsigned long long g0 = tile * A.tile, g1 = min(g0 + (unsigned long long)A.tile, A.p1);
        const unsigned long long gb = max(g0, A.p0);
        __syncthreads();  // (the staging area of the tile before is free)
        const RpDocs R = rp_docs_of_tile(off, A.n_docs, gb, g1, s_j, s_st);  // [gb, g1) is never empty
        for (unsigned long long c0 = g0; c0 < g1; c0 += chunk) {  // bound: A.tile / chunk <= 32
            const unsigned long long c1 = min(c0 + (unsigned long long)chunk, g1), cb = max(c0, gb);
            if (c1 <= cb) continue;  // (a chunk in front of the first document; the same in every lane)
            __syncthreads();         // (the staged starts are there; the chunk before is through)
            int any = 0;
            for (uint32_t s = wave; s <= strips; s += RP_THREADS / 64) {  // bound: (RP_STRIPS + 1) / 4 + 1
                // strip s - 1 of the chunk; s = 0: the 64 positions before c0 (c0 is a multiple of 64)
                const long long p = (long long)c0 + 64ll * ((long long)s - 1) + lane;
                const bool in = p >= (long long)A.p0 && p < (long long)A.p1;  // (marks are read inside [p0, p1) only)
                const unsigned long long bits = __ballot(in && (A.marks[in ? p : (long long)A.p0] & 1));
                if (lane == 0) s_bits[s] = bits;
                any |= bits != 0;
            }
            if (!__syncthreads_or(any)) continue;  // no repeat reaches into this chunk (the same in every lane)
            // bound: chunk / RP_THREADS + 1 <= 8 rounds, the same count in every lane: the ballots below see whole waves
            for (uint32_t i0 = 0; i0 < chunk; i0 += RP_THREADS) {
                const uint32_t i = i0 + tid;
                const unsigned long long p = c0 + i;
                bool covered = false;
                uint32_t D = NG_NONE, own = 0;
                if (i < chunk && p >= cb && p < c1) {
                    unsigned long long o0, o1;
                    D = (uint32_t)rp_doc_of(R, off, s_st, p, o0, o1);
                    uint32_t kl, ks;
                    seldocs_slice(o0, o1, A.max_len, A.tail, kl, ks);
                    const uint32_t kk = (uint32_t)p - ks;  // (p < ks wraps beyond every length)
                    if ((uint32_t)p >= ks && kk < kl) {
                        const uint32_t sp = (i >> 6) + 1, bp = i & 63;  // (c0 is a multiple of 64: p's bit in its word)
                        const unsigned long long cur = s_bits[sp], prev = s_bits[sp - 1];
                        // bit 63 - j of x is position p - j, j = 0 .. 63
                        const unsigned long long x = (cur << (63 - bp)) | (bp == 63 ? 0ull : prev >> (bp + 1));
                        const uint32_t len = min(kk, w - 1) + 1;  // the positions [p - len + 1, p]: 1 .. 64 of them, all in the key
                        covered = (x >> (64 - len)) != 0;
                        own = (uint32_t)(cur >> bp) & 1u;
                    }
                }
                if (covered && A.write_cover) A.marks[p] = (uint8_t)(own | 2u);  // (bit 0 as it was: its readers see the same)
                rp_wave_count(A.cov, D, covered, lane);
            }
        }
    }
}

// Finish pass: the packed rows into the caller's int64 columns, each of which may be null (so may rep, cov and top:
// no key held a window); the number of documents with a repeat by one atomicAdd per workgroup.
__global__ void __launch_bounds__(256)
k_rp_finish(const unsigned long long *__restrict__ off, uint64_t n_docs, unsigned long long max_len, uint32_t tail,
            uint32_t w, const uint32_t *__restrict__ rep, const uint32_t *__restrict__ cov,
            const unsigned long long *__restrict__ top, long long *__restrict__ length, long long *__restrict__ windows,
            long long *__restrict__ distinct, long long *__restrict__ covered, long long *__restrict__ top_count,
            long long *__restrict__ top_pos, unsigned long long *repeat_docs) {
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    uint32_t mine = 0;  // (a thread sees n_docs / stride + 1 < 2^32 documents)
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n_docs; d += stride) {  // bound: n_docs / stride + 1
        const unsigned long long o0 = off[d], o1 = off[d + 1];
        uint32_t kl, ks;
        seldocs_slice(o0, o1, max_len, tail, kl, ks);
        const uint32_t nw = kl >= w ? kl - w + 1 : 0;
        const uint32_t r = rep && nw ? rep[d] : 0;
        const unsigned long long t = top && nw ? top[d] : 0;
        if (length) length[d] = (long long)kl;
        if (windows) windows[d] = (long long)nw;
        if (distinct) distinct[d] = (long long)(nw - r);
        if (covered) covered[d] = cov && nw ? (long long)cov[d] : 0ll;
        // no class of two windows: every window occurs once, and the first of the key is the lowest of them
        if (top_count) top_count[d] = !nw ? 0ll : t ? (long long)(t >> 32) : 1ll;
        if (top_pos) top_pos[d] = !nw ? -1ll : (long long)((t ? (unsigned long long)(uint32_t)~(uint32_t)t : ks) - o0);
        mine += r != 0;
    }
#pragma unroll
    for (int k = 32; k; k >>= 1) mine += __shfl_down(mine, k);  // bound: 6 steps
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_n, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(repeat_docs, (unsigned long long)s_n);
}

}  // namespace bpe
