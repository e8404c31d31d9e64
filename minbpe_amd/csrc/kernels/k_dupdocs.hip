// k_dupdocs.hip -- exact document de-duplication: the first copy of every document of an id stream (bpe_dup_docs_resident,
// DESIGN 4.9).
// Part of bpe_kernels.hip, which includes the parts in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bpe_device.h"
#include "k_common.hip"
#include "k_seldocs.hip"

namespace bpe {

// ---------------------------------------------------------------------------
// dup: ids [n] + off [n_docs + 1] (+ max_len, tail) -> first [n_docs]
//   key(d) = ids[s_d : s_d + l_d], (s_d, l_d) = seldocs_slice of document d: what selection would emit for it.
//   first[d] = the lowest e with key(e) == key(d): the same length and the same ids at their full width.
// Three passes.  hash: H(d) = sum_k mix(id_k, k) mod 2^64 over the key, one read of the stream, laid out by the ids.
// insert: every document goes into an open-addressing table of document numbers, probing from fin(H, l) & mask; a slot
// that is taken holds a document for good, which is compared id by id -- the hash only chooses where to look and spares
// comparisons; rep[d] = the table entry with d's key, and d folds its number into gmin[rep].  finish: first[d] =
// gmin[rep[d]].  No kernel waits for another workgroup.

constexpr uint32_t DUP_THREADS = 256;
constexpr uint32_t DUP_V = 4;               // consecutive stream positions per lane: 16 bytes of int32, 2 x 16 bytes of int64
constexpr uint32_t DUP_TILE_MAX = 65536;
constexpr uint32_t DUP_STAGE = 1024;        // documents of a tile whose starts and partial sums are staged in LDS
constexpr uint32_t DUP_WAVE_LEN_MAX = 1024; // option "dup_wave_len" at its largest
constexpr uint32_t DUP_EMPTY = ~0u;         // "no document": a free table slot, a group minimum nobody has folded into
constexpr uint32_t DUP_AGG_ROUNDS = 4;      // representatives a wave folds for all their lanes at once before each lane folds alone
constexpr size_t DUP_HASH_LDS = 2 * sizeof(unsigned long long) + DUP_STAGE * sizeof(unsigned long long) +
                                (DUP_STAGE + 4) * sizeof(uint32_t);

// the finaliser of splitmix64: every input bit reaches every output bit
__device__ __forceinline__ unsigned long long dup_fmix(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// what the id at position k of a key adds to the key's sum
__device__ __forceinline__ unsigned long long dup_mix(unsigned long long id, uint32_t k) {
    return dup_fmix(id ^ ((unsigned long long)(k + 1) * 0x9E3779B97F4A7C15ull));
}
// the hash a document is placed and filtered by: the sum with the key's length folded in, cut to `bits` bits (option
// "dup_hash_bits"; 0: every document starts at slot 0 and every probe is a full comparison)
__device__ __forceinline__ unsigned long long dup_fin(unsigned long long sum, uint32_t l, uint32_t bits) {
    const unsigned long long h = dup_fmix(sum + (unsigned long long)l * 0xD6E8FEB86659FD93ull);
    return bits >= 64 ? h : h & ((1ull << bits) - 1);
}

// every document's sum, group minimum and count, and every table slot, as the passes expect to find them
__global__ void __launch_bounds__(256)
k_dup_init(unsigned long long *__restrict__ hash, uint32_t *__restrict__ gmin, uint32_t *__restrict__ cnt, uint64_t n_docs,
           uint32_t *__restrict__ tab, uint64_t slots) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += stride) {  // bound: slots / stride + 1 (slots > n_docs)
        tab[i] = DUP_EMPTY;
        if (i < n_docs) {
            hash[i] = 0;
            gmin[i] = DUP_EMPTY;
            cnt[i] = 0;
        }
    }
}

struct DupHashArgs {
    const void *ids;
    const unsigned long long *off;  // n_docs + 1 entries that passed k_rows_check
    unsigned long long n_docs;
    unsigned long long p0, p1;      // off[0] < off[n_docs]: the stream positions that belong to a document
    unsigned long long max_len;
    uint32_t tail, tile;
    unsigned long long *hash;       // zeroed
};

// one lane's sum for document j, into the tile's staging area or straight into the column
__device__ __forceinline__ void dup_flush(const DupHashArgs &A, bool staged, unsigned long long *s_h, unsigned long long j_lo,
                                          unsigned long long j, unsigned long long acc) {
    if (staged) atomicAdd(&s_h[j - j_lo], acc);
    else atomicAdd(&A.hash[j], acc);
}

// Hash pass, laid out by the STREAM as the placement kernels are by their output: a workgroup owns a tile of A.tile
// consecutive positions in units of g = p + a, a = the elements by which `ids` is past a 16-byte boundary, so that a
// lane's V positions at g % 4 == 0 are one or two aligned 16-byte loads; the groups at the two ends of [p0, p1) are read
// as elements: nothing outside is read.  Position p lies in the document j with off[j] <= p < off[j + 1], j =
// upper_bound(off, p) - 1 (of documents that share a start -- empty ones -- the last).  One search each, over all
// documents, for those of the tile's first and last position; the starts between them staged in LDS as 32-bit distances
// from the first, and a 64-bit sum per document next to them.  A lane adds up mix(id, k) while the document stays the
// same (positions outside the key -- beyond max_len -- add nothing); a wave whose lanes all end in one document adds them
// up first.  When the tile is through, a document that lies wholly inside it is ONE plain store of its sum; one that
// crosses the tile's ends (at most two) is a 64-bit atomicAdd into the zeroed column: sums combine in any order, so H
// does not depend on scheduling.  More documents than the staging area holds: the same search over global memory, and
// every lane adds into the column itself.
template <typename T>
__global__ void __launch_bounds__(DUP_THREADS)
k_dup_hash(const DupHashArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_dup[];
    unsigned long long *const s_h = s_dup + 2;        // s_dup[0], s_dup[1]: first and last document of the tile
    uint32_t *const s_st = (uint32_t *)(s_h + DUP_STAGE);
    constexpr uint32_t V = DUP_V;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const unsigned long long a = (unsigned long long)(((uintptr_t)A.ids & 15) / sizeof(T));
    const T *const ids_al = (const T *)A.ids - a;  // 16-byte aligned; ids_al[g] is position g - a
    const unsigned long long G0 = a + A.p0, G1 = a + A.p1;
    const unsigned long long *const off = A.off;
    const uint64_t t0 = G0 / A.tile, t1 = (G1 + A.tile - 1) / A.tile;
    for (uint64_t tile = t0 + blockIdx.x; tile < t1; tile += gridDim.x) {  // bound: the stream's tiles / gridDim.x + 1
        const unsigned long long g0 = tile * A.tile, g1 = min(g0 + (unsigned long long)A.tile, G1);
        const unsigned long long gb = max(g0, G0);
        const unsigned long long p_lo = gb - a, p_hi = g1 - a;  // the tile's positions: [p_lo, p_hi), never empty
        __syncthreads();  // (the staging area of the tile before is free)
        if (tid < 128) {
            const unsigned long long j = seldocs_wave_search(off, A.n_docs, tid < 64 ? p_lo : p_hi - 1, lane);
            if (lane == 0) s_dup[tid >> 6] = j;
        }
        __syncthreads();
        const unsigned long long j_lo = s_dup[0], j_hi = s_dup[1];
        const unsigned long long cnt = j_hi - j_lo + 2;  // off[j_lo] .. off[j_hi + 1], j_hi + 1 <= n_docs
        const unsigned long long base = off[j_lo];       // (every offset is below 2^32: the distances fit)
        const bool staged = cnt <= (unsigned long long)DUP_STAGE + 1;
        if (staged)
            for (uint32_t k = tid; k < (uint32_t)cnt; k += DUP_THREADS) {  // bound: (DUP_STAGE + 1) / DUP_THREADS + 1
                s_st[k] = (uint32_t)(off[j_lo + k] - base);
                if (k + 1 < (uint32_t)cnt) s_h[k] = 0;
            }
        __syncthreads();
        // bound: A.tile / (DUP_THREADS V) + 1 <= 65 rounds, the same count in every lane: the wave sums below need all of them
        for (uint32_t tb = 0; tb < A.tile; tb += DUP_THREADS * V) {
            const unsigned long long g = g0 + tb + tid * V;
            const unsigned long long gf = max(g, gb), gl = min(g + V, g1);
            const bool active = tb + tid * V < A.tile && gf < gl;
            const uint32_t k0 = active ? (uint32_t)(gf - g) : 0, k1 = active ? (uint32_t)(gl - g) : 0;
            T v[V] = {};
            if (k0 == 0 && k1 == V) {
                if constexpr (sizeof(T) == 4) {
                    const int4 q = *(const int4 *)(ids_al + g);
                    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                } else {
                    const longlong2 q0 = *(const longlong2 *)(ids_al + g), q1 = *(const longlong2 *)(ids_al + g + 2);
                    v[0] = q0.x, v[1] = q0.y, v[2] = q1.x, v[3] = q1.y;
                }
            } else {
#pragma unroll
                for (uint32_t k = 0; k < V; k++)  // bound: V
                    if (k >= k0 && k < k1) v[k] = ids_al[g + k];
            }
            unsigned long long p = gf - a, s_n = 0, j = 0, acc = 0;
            uint32_t ks = 0, kl = 0;  // the key of document j: positions [ks, ks + kl)
            bool have = false;
#pragma unroll
            for (uint32_t k = 0; k < V; k++) {  // bound: V
                if (k < k0 || k >= k1) continue;
                if (!have || p >= s_n) {  // the first of the lane's positions, or one past its document
                    if (have && acc) dup_flush(A, staged, s_h, j_lo, j, acc);
                    acc = 0;
                    // p_lo <= p < p_hi: off[j_lo] <= p < off[j_hi + 1]
                    unsigned long long o0;
                    if (staged) {
                        const uint32_t pr = (uint32_t)(p - base);
                        uint32_t lo = 1, hi = (uint32_t)(j_hi - j_lo) + 1;
                        while (lo < hi) {  // bound: log2 of the staged starts
                            const uint32_t mid = (lo + hi) >> 1;
                            if (s_st[mid] > pr) hi = mid; else lo = mid + 1;
                        }
                        j = j_lo + lo - 1;
                        o0 = base + s_st[lo - 1];
                        s_n = base + s_st[lo];
                    } else {
                        unsigned long long lo = j_lo + 1, hi = j_hi + 1;
                        while (lo < hi) {  // bound: log2 of the tile's documents
                            const unsigned long long mid = lo + ((hi - lo) >> 1);
                            if (off[mid] > p) hi = mid; else lo = mid + 1;
                        }
                        j = lo - 1;
                        o0 = off[j];
                        s_n = off[j + 1];
                    }
                    seldocs_slice(o0, s_n, A.max_len, A.tail, kl, ks);
                    have = true;
                }
                const uint32_t kk = (uint32_t)p - ks;  // (p < ks wraps beyond every length)
                if ((uint32_t)p >= ks && kk < kl) acc += dup_mix((unsigned long long)v[k], kk);
                p++;
            }
            // the lane's last document: one add for the wave where every lane that has one has the same
            const unsigned long long bal = __ballot(have);
            if (bal) {
                const unsigned long long jf = __shfl(j, (int)__ffsll(bal) - 1);
                if (__all(!have || j == jf)) {
                    unsigned long long sum = have ? acc : 0;
#pragma unroll
                    for (int d = 32; d; d >>= 1) sum += __shfl_down(sum, d);  // bound: 6 steps
                    if (lane == 0 && sum) dup_flush(A, staged, s_h, j_lo, jf, sum);
                } else if (have && acc) {
                    dup_flush(A, staged, s_h, j_lo, j, acc);
                }
            }
        }
        if (staged) {
            __syncthreads();
            for (uint32_t k = tid; k + 1 < (uint32_t)cnt; k += DUP_THREADS) {  // bound: DUP_STAGE / DUP_THREADS
                const unsigned long long h = s_h[k];
                if (base + s_st[k] >= p_lo && base + s_st[k + 1] <= p_hi) A.hash[j_lo + k] = h;  // no other tile sees it
                else if (h) atomicAdd(&A.hash[j_lo + k], h);
            }
        }
    }
}

struct DupInsArgs {
    const void *ids;
    const unsigned long long *off;
    unsigned long long n_docs;
    unsigned long long max_len;
    unsigned long long tmask;  // tmask + 1 table slots, a power of two > n_docs
    uint32_t tail, wave_len, hash_bits;
    const unsigned long long *hash;
    uint32_t *tab, *rep, *gmin, *cnt;
    uint32_t want_counts;
};

// l ids at x and at y, compared by one lane; early exit on the first difference.  Bound: l <= dup_wave_len.
template <typename T>
__device__ __forceinline__ bool dup_equal_lane(const T *x, const T *y, uint32_t l) {
    for (uint32_t k = 0; k < l; k++)  // bound: l
        if (x[k] != y[k]) return false;
    return true;
}

// ... by a whole wave (the arguments are the same in every lane), 64 pieces at a time, early exit after the first piece
// that differs.  16-byte loads where the two sides sit alike on their 16 bytes, after the up to 3 elements in front of
// the boundary; otherwise, and for what is left behind the last whole 16 bytes, one id per lane.  Bound: l.
template <typename T>
__device__ __forceinline__ bool dup_equal_wave(const T *x, const T *y, uint32_t l, uint32_t lane) {
    constexpr uint32_t E = 16 / sizeof(T);
    uint32_t k = 0;
    if ((((uintptr_t)x ^ (uintptr_t)y) & 15) == 0) {
        const uint32_t head = min(l, (uint32_t)(((16 - ((uintptr_t)x & 15)) & 15) / sizeof(T)));  // < E
        if (__any(lane < head && x[lane] != y[lane])) return false;
        const uint32_t nvec = (l - head) / E;
        for (uint32_t v0 = 0; v0 < nvec; v0 += 64) {  // bound: l / (64 E) + 1
            bool ne = false;
            if (v0 + lane < nvec) {
                const int4 p = *(const int4 *)(x + head + (size_t)(v0 + lane) * E);
                const int4 q = *(const int4 *)(y + head + (size_t)(v0 + lane) * E);
                ne = p.x != q.x || p.y != q.y || p.z != q.z || p.w != q.w;
            }
            if (__any(ne)) return false;
        }
        k = head + nvec * E;
    }
    for (; k < l; k += 64)  // bound: l / 64 + 1
        if (__any(k + lane < l && x[k + lane] != y[k + lane])) return false;
    return true;
}

// Insert pass.  A wave takes 64 documents at a time, one per lane.  Keys of up to A.wave_len ids are inserted by their
// lane; the longer ones afterwards, one at a time, by the whole wave.  Either way: linear probing from fin & tmask; a
// free slot is claimed by atomicCAS, and a slot that is taken holds the number of a document e for good -- the ids are
// read-only for the whole call, so e's key can be read at once: when the hashes, the lengths and then the ids
// themselves agree, rep[d] = e; otherwise the next slot.  Documents with one key walk the same slots and pass none that
// holds their key, so they all stop at the same entry.  The table has more slots than there are documents: a free one
// is always found, and no loop runs longer than the table.  Nothing here waits for another lane's work.
// Then every document, its representative included, folds its number into gmin[rep] (prefilled with DUP_EMPTY) and 1
// into cnt[rep]: for the first few representatives of a wave one lane does that for all the lanes that share it -- a
// corpus of copies has them all on one address -- and the lanes that are left fold for themselves.
template <typename T>
__global__ void __launch_bounds__(DUP_THREADS)
k_dup_insert(const DupInsArgs A) {
    const uint32_t lane = threadIdx.x & 63;
    const T *const ids = (const T *)A.ids;
    const uint64_t nwaves = (uint64_t)gridDim.x * (DUP_THREADS / 64);
    const uint64_t chunks = (A.n_docs + 63) / 64;
    for (uint64_t ch = (uint64_t)blockIdx.x * (DUP_THREADS / 64) + (threadIdx.x >> 6); ch < chunks; ch += nwaves) {  // bound: chunks / nwaves + 1
        const uint64_t d64 = ch * 64 + lane;
        const bool valid = d64 < A.n_docs;
        const uint32_t d = (uint32_t)d64;  // n_docs < 2^32 - 1
        uint32_t l = 0, s = 0, r = DUP_EMPTY;
        unsigned long long fin = 0;
        if (valid) {
            seldocs_slice(A.off[d64], A.off[d64 + 1], A.max_len, A.tail, l, s);
            fin = dup_fin(A.hash[d64], l, A.hash_bits);
        }
        const bool is_long = valid && l > A.wave_len;
        const bool by_lane = valid && !is_long;
        // Lanes that start at the slot the wave's first such lane starts at -- copies of one document, mostly -- share
        // the look at it: that lane reads it, claims it if it is free, and hands on whom it holds.  64 lanes reading one
        // word past their L1 are 64 accesses, and a corpus of copies has every wave on that word.
        bool shared = false;
        uint32_t e_shared = DUP_EMPTY;
        if (const unsigned long long bal = __ballot(by_lane)) {
            const int src = (int)__ffsll(bal) - 1;
            const unsigned long long slot0 = __shfl(fin, src) & A.tmask;
            const bool same = by_lane && (fin & A.tmask) == slot0;
            if (__popcll(__ballot(same)) > 1) {
                uint32_t e = 0;
                if ((int)lane == src) {
                    e = __hip_atomic_load(&A.tab[slot0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (e == DUP_EMPTY) e = atomicCAS(&A.tab[slot0], DUP_EMPTY, d);
                    if (e == DUP_EMPTY) e = d;  // (claimed: the slot holds this lane's document from now on)
                }
                e_shared = __shfl(e, src);
                shared = same;
            }
        }
        if (by_lane) {
            unsigned long long slot = fin & A.tmask;
            for (unsigned long long probe = 0; probe <= A.tmask; probe++, slot = (slot + 1) & A.tmask) {  // bound: the table's slots
                uint32_t e = e_shared;
                if (!shared || probe) {
                    e = __hip_atomic_load(&A.tab[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (e == DUP_EMPTY) e = atomicCAS(&A.tab[slot], DUP_EMPTY, d);
                }
                if (e == DUP_EMPTY || e == d) {
                    r = d;
                    break;
                }
                uint32_t el, es;
                seldocs_slice(A.off[e], A.off[(uint64_t)e + 1], A.max_len, A.tail, el, es);
                if (el == l && dup_fin(A.hash[e], el, A.hash_bits) == fin && dup_equal_lane(ids + s, ids + es, l)) {
                    r = e;
                    break;
                }
            }
        }
        // bound: 64 rounds, one per lane with a long key
        for (unsigned long long todo = __ballot(is_long); todo; todo &= todo - 1) {
            const int src = (int)__ffsll(todo) - 1;
            const uint32_t wd = (uint32_t)(ch * 64 + (uint64_t)src), wl = __shfl(l, src), ws = __shfl(s, src);
            const unsigned long long wfin = __shfl(fin, src);
            unsigned long long slot = wfin & A.tmask;
            uint32_t wr = DUP_EMPTY;
            for (unsigned long long probe = 0; probe <= A.tmask; probe++, slot = (slot + 1) & A.tmask) {  // bound: the table's slots
                uint32_t e = 0;
                if (lane == 0) {
                    e = __hip_atomic_load(&A.tab[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (e == DUP_EMPTY) e = atomicCAS(&A.tab[slot], DUP_EMPTY, wd);
                }
                e = __shfl(e, 0);
                if (e == DUP_EMPTY) {
                    wr = wd;
                    break;
                }
                uint32_t el, es;
                seldocs_slice(A.off[e], A.off[(uint64_t)e + 1], A.max_len, A.tail, el, es);
                if (el == wl && dup_fin(A.hash[e], el, A.hash_bits) == wfin && dup_equal_wave(ids + ws, ids + es, wl, lane)) {
                    wr = e;
                    break;
                }
            }
            if ((int)lane == src) r = wr;
        }
        if (valid) A.rep[d64] = r;
        bool open = valid && r != DUP_EMPTY;  // (always: see above -- a slot is found before the table is through)
        for (uint32_t round = 0; round < DUP_AGG_ROUNDS; round++) {  // bound: a constant
            const unsigned long long bal = __ballot(open);
            if (!bal) break;
            const int src = (int)__ffsll(bal) - 1;
            const uint32_t r0 = __shfl(r, src);
            const bool same = open && r == r0;
            const unsigned long long m = __ballot(same);  // (holds src: its lowest lane is the lowest document)
            if ((int)lane == src) {
                atomicMin(&A.gmin[r0], (uint32_t)(ch * 64) + (uint32_t)__ffsll(m) - 1);
                if (A.want_counts) atomicAdd(&A.cnt[r0], (uint32_t)__popcll(m));
            }
            open = open && !same;
        }
        if (open) {
            atomicMin(&A.gmin[r], d);
            if (A.want_counts) atomicAdd(&A.cnt[r], 1u);
        }
    }
}

// Finish pass: first[d] = gmin[rep[d]]; counts[d] = the group's size at its first document and 0 elsewhere; the number
// of groups by one atomicAdd per workgroup.
__global__ void __launch_bounds__(256)
k_dup_finish(const uint32_t *__restrict__ rep, const uint32_t *__restrict__ gmin, const uint32_t *__restrict__ cnt,
             uint64_t n_docs, long long *__restrict__ first, unsigned long long *__restrict__ counts,
             unsigned long long *distinct) {
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    uint32_t mine = 0;  // (a thread sees n_docs / stride + 1 < 2^32 documents)
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n_docs; d += stride) {  // bound: n_docs / stride + 1
        const uint32_t r = rep[d], f = r == DUP_EMPTY ? DUP_EMPTY : gmin[r];
        first[d] = (long long)f;
        if (counts) counts[d] = f == (uint32_t)d && r != DUP_EMPTY ? (unsigned long long)cnt[r] : 0ull;
        mine += f == (uint32_t)d;
    }
#pragma unroll
    for (int k = 32; k; k >>= 1) mine += __shfl_down(mine, k);  // bound: 6 steps
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_n, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(distinct, (unsigned long long)s_n);
}

}  // namespace bpe
