// k_seldocs.hip -- document selection: gather, filter and shuffle the documents of an id stream (bpe_select_docs_resident,
// DESIGN 4.8).
// Part of bpe_kernels.hip, which includes the parts in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bpe_device.h"
#include "k_common.hip"

namespace bpe {

// ---------------------------------------------------------------------------
// select: ids [n] + off [n_docs + 1] + index [m] -> out = ids[s_0 : s_0 + l_0] | ids[s_1 : s_1 + l_1] | ...
//   len(d) = off[d + 1] - off[d];  for selection j with d = index[j]:  l_j = len(d), or min(len(d), max_len) when
//   max_len != 0;  s_j = off[d], or off[d + 1] - l_j with `tail`.  oo[j] = l_0 + ... + l_{j-1}, oo[m] = the total.

constexpr uint32_t SEL_THREADS = 256;
constexpr uint32_t SEL_V = 8;             // consecutive output elements per lane: 2 x 16 bytes of int32, 4 x 16 bytes of int64
constexpr uint32_t SEL_TILE_MAX = 65536;  // (distances inside a tile fit 32 bits with room to spare)
constexpr uint32_t SEL_STAGE_MAX = 4096;  // output starts a tile stages in LDS, 4 bytes each (relative to the tile's first)

// What goes on of the document ids[o0 : o1): its length l and its first position s.  The one statement of the rule
// above: bpe_dup_docs_resident (k_dupdocs.hip) compares documents by the same slices.
__device__ __forceinline__ void seldocs_slice(unsigned long long o0, unsigned long long o1, unsigned long long max_len,
                                              uint32_t tail, uint32_t &l, uint32_t &s) {
    const unsigned long long L = o1 - o0, lj = max_len ? min(L, max_len) : L;
    l = (uint32_t)lj;
    s = (uint32_t)(tail ? o1 - lj : o0);
}

// j = upper_bound(oo, e) - 1 over the m + 1 ascending entries oo[0] <= e < oo[m], by one wave (e is the same in all its
// lanes), 64 probes at a time: log64(m) dependent loads where a lane on its own would wait for log2(m)
__device__ __forceinline__ unsigned long long seldocs_wave_search(const unsigned long long *oo, unsigned long long m,
                                                                  unsigned long long e, uint32_t lane) {
    unsigned long long lo = 1, hi = m;  // the first j in [lo, hi] with oo[j] > e: oo[m] > e
    // bound: log64(m) + 2 rounds -- a round leaves at most span / 64 + 1 of the span, and a span below 64 is probed at every
    // entry; lo and hi come from the ballot, the same in all lanes
    while (lo < hi) {
        const unsigned long long base = lo, span = hi - lo;
        const unsigned long long p = base + ((span * lane) >> 6);  // base = p_0 <= ... <= p_63 < hi
        const unsigned long long beyond = __ballot(oo[p] > e);     // (oo ascends: a suffix of the lanes)
        if (beyond == 0) {
            lo = base + ((span * 63) >> 6) + 1;
        } else {
            const uint32_t f = (uint32_t)__ffsll(beyond) - 1;
            hi = base + ((span * f) >> 6);
            if (f) lo = base + ((span * (f - 1)) >> 6) + 1;
        }
    }
    return lo - 1;
}

// Length pass, one selection per thread.  The offsets have passed k_rows_check (ascending, none beyond n < 2^32), so l_j
// and s_j fit 32 bits.  An index is compared at its full 64 bits; bad = the lowest j whose index lies outside [0, n_docs).
__global__ void __launch_bounds__(256)
k_seldocs_len(const unsigned long long *__restrict__ off, uint64_t n_docs, const long long *__restrict__ index, uint64_t m,
              unsigned long long max_len, uint32_t tail, uint32_t *__restrict__ len, uint32_t *__restrict__ src,
              unsigned long long *bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
        const long long d = index[j];
        uint32_t l = 0, s = 0;
        if (d < 0 || (unsigned long long)d >= n_docs) {
            atomicMin(bad, (unsigned long long)j);
        } else {
            seldocs_slice(off[d], off[d + 1], max_len, tail, l, s);
        }
        len[j] = l;
        src[j] = s;
    }
}

struct SelArgs {
    const void *ids;
    void *out;
    const unsigned long long *oo;  // m + 1 output offsets: the scan of the lengths, oo[m] = total
    const uint32_t *src;           // s_j of every selection
    unsigned long long m, total;   // total > 0
    uint32_t tile, stage;
};

// V values of one lane to out_al[g .. g + V), of which [k0, k1) are the tile's own: all of them as 16-byte stores
// (g % 4 == 0: out_al + g is 16-byte aligned by construction), a part of them as element stores.  rows_store with values
// of the output's own width: a 64-bit id is moved whole, where a row's value is an int32 that is sign-extended
template <typename T>
__device__ __forceinline__ void seldocs_store(T *out_al, unsigned long long g, const T *v, uint32_t k0, uint32_t k1) {
    if (k0 == 0 && k1 == SEL_V) {
#pragma unroll
        for (uint32_t h = 0; h < SEL_V; h += 4) {
            if constexpr (sizeof(T) == 4) {
                *(int4 *)(out_al + g + h) = make_int4(v[h], v[h + 1], v[h + 2], v[h + 3]);
            } else {
                *(longlong2 *)(out_al + g + h) = make_longlong2(v[h], v[h + 1]);
                *(longlong2 *)(out_al + g + h + 2) = make_longlong2(v[h + 2], v[h + 3]);
            }
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < SEL_V; k++)
            if (k >= k0 && k < k1) out_al[g + k] = v[k];
    }
}

// Placement, laid out by the OUTPUT as k_rows_pack is.  Output element e lies in the selection j with oo[j] <= e <
// oo[j + 1]: oo ascends, oo[0] = 0, oo[m] = total, so j = upper_bound(oo, e) - 1 (of selections that share a start --
// empty ones -- the last, the one that holds e), and out[e] = ids[s_j + (e - oo[j])].  A workgroup owns a tile of A.tile
// consecutive elements in units of g = e + a, a = the elements by which `out` is past a 16-byte boundary, so that a lane's
// V elements at g % 4 == 0 are 16-byte aligned addresses; the tiles at the two ends write their partial groups as
// element stores: nothing outside [0, total) elements is written.  One search each, over all selections, for those of
// the tile's first and last element; the output starts between them staged in LDS as 32-bit distances from the first,
// and every lane searches there -- once per run of consecutive positions, again when a position leaves its selection.
// More starts than the staging area holds (A.stage; thousands of empty selections in a row), or starts 2^32 apart (a
// selection longer than that ends in the tile): the same search over global memory.
// The index s_j + (e - oo[j]) lies inside [s_j, s_j + l_j), which k_seldocs_len took from inside [off[d], off[d + 1]) of
// offsets that passed k_rows_check: inside [off[0], off[n_docs]) of ids [n].
template <typename T>
__global__ void __launch_bounds__(SEL_THREADS)
k_seldocs_place(const SelArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_sel[];
    uint32_t *const s_st = (uint32_t *)(s_sel + 2);  // s_sel[0], s_sel[1]: first and last selection of the tile
    constexpr uint32_t V = SEL_V;
    const uint32_t tid = threadIdx.x;
    const T *const ids = (const T *)A.ids;
    const unsigned long long a = (unsigned long long)(((uintptr_t)A.out & 15) / sizeof(T));
    T *const out_al = (T *)A.out - a;  // 16-byte aligned; out_al[g] is element g - a
    const unsigned long long G = a + A.total;
    const unsigned long long *const oo = A.oo;
    const uint32_t *const src = A.src;
    const uint64_t ntiles = (G + A.tile - 1) / A.tile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const unsigned long long g0 = tile * A.tile, g1 = min(g0 + (unsigned long long)A.tile, G);
        const unsigned long long e_lo = max(g0, a) - a, e_hi = g1 - a;  // the tile's elements: [e_lo, e_hi), never empty
        __syncthreads();  // (the staging area of the tile before is free)
        if (tid < 128) {
            // waves 0 and 1, one for e_lo and one for e_hi - 1, over ALL selections: oo[m] = total > e
            const unsigned long long j = seldocs_wave_search(oo, A.m, tid < 64 ? e_lo : e_hi - 1, tid & 63);
            if ((tid & 63) == 0) s_sel[tid >> 6] = j;
        }
        __syncthreads();
        const unsigned long long j_lo = s_sel[0], j_hi = s_sel[1];
        const unsigned long long cnt = j_hi - j_lo + 2;  // oo[j_lo] .. oo[j_hi + 1], j_hi + 1 <= m
        const unsigned long long base = oo[j_lo];
        const bool staged = cnt <= (unsigned long long)A.stage && oo[j_hi + 1] - base <= 0xFFFFFFFFull;
        if (staged)
            for (uint32_t k = tid; k < (uint32_t)cnt; k += SEL_THREADS) s_st[k] = (uint32_t)(oo[j_lo + k] - base);
        __syncthreads();
        for (uint32_t t = tid * V; t < A.tile; t += SEL_THREADS * V) {
            const unsigned long long g = g0 + t;
            const unsigned long long gf = max(g, a), gl = min(g + V, g1);
            if (gf >= gl) continue;
            const uint32_t k0 = (uint32_t)(gf - g), k1 = (uint32_t)(gl - g);
            T v[V] = {};
            unsigned long long e = gf - a, s_n = 0, from = 0;  // from: out[e] = ids[e + from] inside the selection, mod 2^64
            bool have = false;
#pragma unroll
            for (uint32_t k = 0; k < V; k++) {
                if (k < k0 || k >= k1) continue;
                if (!have || e >= s_n) {  // the first of a run of consecutive positions, or one past its selection
                    // e_lo <= e < e_hi: oo[j_lo] <= e < oo[j_hi + 1]
                    unsigned long long j, s_j;
                    if (staged) {  // 32-bit: entry k is oo[j_lo + k] - base, e - base < entry j_hi + 1 - j_lo
                        const uint32_t er = (uint32_t)(e - base);
                        uint32_t lo = 1, hi = (uint32_t)(j_hi - j_lo) + 1;
                        while (lo < hi) {
                            const uint32_t mid = (lo + hi) >> 1;
                            if (s_st[mid] > er) hi = mid; else lo = mid + 1;
                        }
                        j = j_lo + lo - 1;
                        s_j = base + s_st[lo - 1];
                        s_n = base + s_st[lo];
                    } else {
                        unsigned long long lo = j_lo + 1, hi = j_hi + 1;
                        while (lo < hi) {
                            const unsigned long long mid = lo + ((hi - lo) >> 1);
                            if (oo[mid] > e) hi = mid; else lo = mid + 1;
                        }
                        j = lo - 1;
                        s_j = oo[j];
                        s_n = oo[j + 1];
                    }
                    from = (unsigned long long)src[j] - s_j;
                    have = true;
                }
                v[k] = ids[e + from];
                e++;
            }
            seldocs_store<T>(out_al, g, v, k0, k1);
        }
    }
}

}  // namespace bpe
