// k_rows.hip -- resident training rows: a flat id stream with document offsets to fixed-length rows.
// Part of bpe_kernels.hip, which includes the parts in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bpe_device.h"
#include "k_common.hip"

namespace bpe {

// ---------------------------------------------------------------------------
// rows (bpe_rows_resident): ids [n] int32 + doc_offsets [n_docs + 1] uint64 -> rows [R, L] int32 / int64
//
// The stream: seq_d = ids[off[d] : off[d + 1]) (+ [sep]), stream = seq_0 | seq_1 | ..., T = its length.  Stream position q
// lies in the document d with sh(d) <= q < sh(d + 1), where sh(d) = off[d] - off[0] (+ d with a separator) is the
// document's SHIFTED start: sh ascends (strictly with a separator), sh(0) = 0, sh(n_docs) = T, so d = upper_bound(sh, q) - 1
// (of documents that share a start -- empty ones, no separator -- the last, the one that holds q).

constexpr uint32_t ROWS_THREADS = 256;
constexpr uint32_t ROWS_V = 4;             // consecutive output elements per lane: 16 bytes of int32, 2 x 16 bytes of int64
constexpr uint32_t ROWS_V_DOC = 8;         // ... of the pack kernel that searches: one search serves twice as many
constexpr uint32_t ROWS_TILE_MAX = 65536;  // (offsets inside a tile fit 32 bits with room to spare)
constexpr uint32_t ROWS_STAGE_MAX = 4096;  // shifted starts a tile stages in LDS, 4 bytes each (relative to the tile's first)

// offsets as bpe_rows_resident states them: ascending, none beyond n.  bad = the first entry that is not; ends[0] =
// off[0], ends[1] = off[n_docs] (the same transfer brings all three to the host).
__global__ void __launch_bounds__(256)
k_rows_check(const unsigned long long *__restrict__ off, uint64_t n_docs, uint64_t n, unsigned long long *bad,
             unsigned long long *ends) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_docs; i += stride) {
        const unsigned long long o = off[i];
        if (o > n || (i && o < off[i - 1])) atomicMin(bad, (unsigned long long)i);
        if (i == 0) ends[0] = o;
        if (i == n_docs) ends[1] = o;
    }
}

struct RowsArgs {
    const int32_t *ids;
    const unsigned long long *off;  // n_docs + 1 entries, validated (k_rows_check) before any kernel below is launched
    unsigned long long n_docs;
    unsigned long long off0;        // off[0]
    unsigned long long T;           // length of the stream (pack mode)
    unsigned long long L, S;        // row length, row stride in stream positions (pack mode)
    unsigned long long E;           // output elements: R L
    int32_t sep, pad;
    uint32_t has_sep, trunc_left, pad_left;
    void *rows;
    int32_t *doc_index, *pos, *lengths;
    uint32_t tile, stage;
};

// (row, column) of output element e, given those of the tile's first element e_lo <= e < e_lo + ROWS_TILE_MAX:
// one 32-bit division (row lengths beyond 32 bits are longer than a tile: the quotient is 0)
__device__ __forceinline__ void rows_rc(unsigned long long e, unsigned long long e_lo, unsigned long long r0,
                                        unsigned long long j0, unsigned long long L, unsigned long long &r,
                                        unsigned long long &j) {
    const unsigned long long x = j0 + (e - e_lo);
    if (x < L) {
        r = r0;
        j = x;
        return;
    }
    const uint32_t y = (uint32_t)(x - L);  // < e - e_lo < ROWS_TILE_MAX
    const uint32_t Lc = L > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)L;
    const uint32_t dr = y / Lc;
    r = r0 + 1 + dr;
    j = y - dr * Lc;
}

// V values of one lane to out_al[g .. g + V), of which [k0, k1) are the tile's own: all of them as 16-byte stores
// (g % 4 == 0: out_al + g is 16-byte aligned by construction), a part of them as element stores
template <typename OutT, uint32_t V>
__device__ __forceinline__ void rows_store(OutT *out_al, unsigned long long g, const int32_t *v, uint32_t k0, uint32_t k1) {
    if (k0 == 0 && k1 == V) {
#pragma unroll
        for (uint32_t h = 0; h < V; h += 4) {
            if constexpr (sizeof(OutT) == 4) {
                *(int4 *)(out_al + g + h) = make_int4(v[h], v[h + 1], v[h + 2], v[h + 3]);
            } else {
                *(longlong2 *)(out_al + g + h) = make_longlong2((long long)v[h], (long long)v[h + 1]);  // (sign-extended)
                *(longlong2 *)(out_al + g + h + 2) = make_longlong2((long long)v[h + 2], (long long)v[h + 3]);
            }
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < V; k++)
            if (k >= k0 && k < k1) out_al[g + k] = (OutT)v[k];
    }
}

// a companion (int32) has an alignment of its own: p + e is written as one 16-byte store where that address allows
template <uint32_t V>
__device__ __forceinline__ void rows_store_comp(int32_t *p, unsigned long long e, const int32_t *v, uint32_t k0, uint32_t k1) {
    if (k0 == 0 && k1 == V && (((uintptr_t)(p + e)) & 15) == 0) {
#pragma unroll
        for (uint32_t h = 0; h < V; h += 4) *(int4 *)(p + e + h) = make_int4(v[h], v[h + 1], v[h + 2], v[h + 3]);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < V; k++)
            if (k >= k0 && k < k1) p[e + k - k0] = v[k];
    }
}

// Pack mode, laid out by the OUTPUT.  Element e = r L + j holds stream[r S + j] (pad beyond T).  A workgroup owns a tile
// of A.tile consecutive elements in units of g = e + a, a = the elements by which `rows` is past a 16-byte boundary, so
// that a lane's V elements at g % 4 == 0 are 16-byte aligned addresses; the tiles at the two ends write their
// partial groups as element stores: nothing outside [0, E) elements is written.  The tile's stream positions lie in
// [qlo, qhi]: one search each for the documents of the two, the shifted starts between them staged in LDS as 32-bit
// distances from the first, and every lane searches there -- once per run of consecutive positions, again when a position
// leaves its document or its row.  More starts than the staging area holds (A.stage; thousands of empty documents in a
// row), or starts 2^32 apart: the same search over global memory.
// DOC = false (no separator, no companions): stream[q] = ids[off[0] + q], no search at all.
template <typename OutT, bool DOC>
__global__ void __launch_bounds__(ROWS_THREADS)
k_rows_pack(const RowsArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_rows[];
    uint32_t *const s_sh = (uint32_t *)(s_rows + 2);  // s_rows[0], s_rows[1]: first and last document of the tile
    constexpr uint32_t V = DOC ? ROWS_V_DOC : ROWS_V;
    const uint32_t tid = threadIdx.x;
    const unsigned long long a = (unsigned long long)(((uintptr_t)A.rows & 15) / sizeof(OutT));
    OutT *const out_al = (OutT *)A.rows - a;  // 16-byte aligned; out_al[g] is element g - a
    const unsigned long long G = a + A.E, L = A.L, S = A.S, T = A.T;
    const unsigned long long sepd = A.has_sep ? 1ull : 0ull;
    const unsigned long long *const off = A.off;
    const uint64_t ntiles = (G + A.tile - 1) / A.tile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const unsigned long long g0 = tile * A.tile, g1 = min(g0 + (unsigned long long)A.tile, G);
        const unsigned long long e_lo = max(g0, a) - a, e_hi = g1 - a;  // the tile's elements: [e_lo, e_hi), never empty
        const unsigned long long r0 = e_lo / L, j0 = e_lo - r0 * L;
        unsigned long long d_lo = 0, d_hi = 0, base = 0;  // base = sh(d_lo)
        bool staged = false;
        if constexpr (DOC) {
            unsigned long long r1, j1;
            rows_rc(e_hi - 1, e_lo, r0, j0, L, r1, j1);
            unsigned long long qlo = r0 * S + j0, qhi = r1 * S + j1;
            if (r1 > r0) {  // (a later row starts at r S, further back than the row before it ended)
                qlo = r0 * S + min(j0, S);
                qhi = max(qhi, (r1 - 1) * S + L - 1);
            }
            __syncthreads();  // (the staging area of the tile before is free)
            if (qlo < T) {
                qhi = min(qhi, T - 1);
                if (tid < 128) {
                    // waves 0 and 1, one for qlo and one for qhi: d = upper_bound(sh, q) - 1 over ALL documents, 64 probes
                    // at a time -- log64(n_docs) dependent loads where a lane on its own would wait for log2(n_docs)
                    const uint32_t lane = tid & 63;
                    const unsigned long long q = tid < 64 ? qlo : qhi;
                    unsigned long long lo = 1, hi = A.n_docs;  // the first d in [lo, hi] with sh(d) > q: sh(n_docs) = T > q
                    while (lo < hi) {  // (lo and hi come from the ballot: the same in all lanes)
                        const unsigned long long base = lo, span = hi - lo;
                        const unsigned long long p = base + ((span * lane) >> 6);  // base = p_0 <= ... <= p_63 < hi
                        const unsigned long long beyond = __ballot(off[p] - A.off0 + sepd * p > q);  // (sh ascends: a suffix of the lanes)
                        if (beyond == 0) {
                            lo = base + ((span * 63) >> 6) + 1;
                        } else {
                            const uint32_t f = (uint32_t)__ffsll(beyond) - 1;
                            hi = base + ((span * f) >> 6);
                            if (f) lo = base + ((span * (f - 1)) >> 6) + 1;
                        }
                    }
                    if (lane == 0) s_rows[tid >> 6] = lo - 1;
                }
                __syncthreads();
                d_lo = s_rows[0];
                d_hi = s_rows[1];
                const unsigned long long cnt = d_hi - d_lo + 2;  // sh(d_lo) .. sh(d_hi + 1), d_hi + 1 <= n_docs
                base = off[d_lo] - A.off0 + sepd * d_lo;
                staged = cnt <= (unsigned long long)A.stage &&
                         off[d_hi + 1] - A.off0 + sepd * (d_hi + 1) - base <= 0xFFFFFFFFull;
                if (staged)
                    for (uint32_t k = tid; k < (uint32_t)cnt; k += ROWS_THREADS)
                        s_sh[k] = (uint32_t)(off[d_lo + k] - A.off0 + sepd * (d_lo + k) - base);
                __syncthreads();
            }
        }
        for (uint32_t t = tid * V; t < A.tile; t += ROWS_THREADS * V) {
            const unsigned long long g = g0 + t;
            const unsigned long long gf = max(g, a), gl = min(g + V, g1);
            if (gf >= gl) continue;
            const uint32_t k0 = (uint32_t)(gf - g), k1 = (uint32_t)(gl - g);
            unsigned long long r, j;
            rows_rc(gf - a, e_lo, r0, j0, L, r, j);
            int32_t v[V] = {}, vd[V] = {}, vp[V] = {};
            unsigned long long d = 0, s_d = 0, s_n = 0, q = r * S + j;
            bool have = false;
#pragma unroll
            for (uint32_t k = 0; k < V; k++) {
                if (k < k0 || k >= k1) continue;
                if (q >= T) {
                    v[k] = A.pad;
                    vd[k] = -1;
                    vp[k] = 0;
                } else if constexpr (DOC) {
                    if (!have || q >= s_n) {  // the first of a run of consecutive positions, or one past its document
                        // qlo <= q <= qhi: sh(d_lo) <= q < sh(d_hi + 1)
                        if (staged) {  // 32-bit: entry k is sh(d_lo + k) - base, q - base < entry d_hi + 1 - d_lo
                            const uint32_t qr = (uint32_t)(q - base);
                            uint32_t lo = 1, hi = (uint32_t)(d_hi - d_lo) + 1;
                            while (lo < hi) {
                                const uint32_t mid = (lo + hi) >> 1;
                                if (s_sh[mid] > qr) hi = mid; else lo = mid + 1;
                            }
                            d = d_lo + lo - 1;
                            s_d = base + s_sh[lo - 1];
                            s_n = base + s_sh[lo];
                        } else {
                            unsigned long long lo = d_lo + 1, hi = d_hi + 1;
                            while (lo < hi) {
                                const unsigned long long mid = lo + ((hi - lo) >> 1);
                                if (off[mid] - A.off0 + sepd * mid > q) hi = mid; else lo = mid + 1;
                            }
                            d = lo - 1;
                            s_d = off[d] - A.off0 + sepd * d;
                            s_n = off[d + 1] - A.off0 + sepd * (d + 1);
                        }
                        have = true;
                    }
                    // the offsets passed k_rows_check and sh(d) <= q < sh(d + 1): the index off[0] + q (- d) is
                    // off[d] + (q - sh(d)), inside [off[d], off[d + 1]) and so inside [off[0], off[n_docs]) of ids [n]
                    v[k] = (sepd && q == s_n - 1) ? A.sep : A.ids[A.off0 + q - sepd * d];
                    vd[k] = (int32_t)d;
                    vp[k] = (int32_t)(q - s_d);
                } else {
                    v[k] = A.ids[A.off0 + q];  // q < T = off[n_docs] - off[0]: inside [off[0], off[n_docs]), validated
                }
                q++;
                if (++j == L) {  // the next row starts over at r S: search again
                    j = 0;
                    r++;
                    q = r * S;
                    have = false;
                }
            }
            rows_store<OutT, V>(out_al, g, v, k0, k1);
            if constexpr (DOC) {
                if (A.doc_index) rows_store_comp<V>(A.doc_index, gf - a, vd, k0, k1);
                if (A.pos) rows_store_comp<V>(A.pos, gf - a, vp, k0, k1);
            }
        }
    }
}

// Per-document mode: row d is seq_d cut to L -- the head, or (trunc_left) the tail -- and padded on the right or
// (pad_left) the left; lengths[d] = min(len(seq_d), L).  The same tiles and stores; the row IS the document, so there
// is nothing to search.
template <typename OutT>
__global__ void __launch_bounds__(ROWS_THREADS)
k_rows_per_doc(const RowsArgs A) {
    const uint32_t tid = threadIdx.x;
    const unsigned long long a = (unsigned long long)(((uintptr_t)A.rows & 15) / sizeof(OutT));
    OutT *const out_al = (OutT *)A.rows - a;
    const unsigned long long G = a + A.E, L = A.L;
    const unsigned long long sepd = A.has_sep ? 1ull : 0ull;
    const uint64_t ntiles = (G + A.tile - 1) / A.tile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const unsigned long long g0 = tile * A.tile, g1 = min(g0 + (unsigned long long)A.tile, G);
        const unsigned long long e_lo = max(g0, a) - a;
        const unsigned long long r0 = e_lo / L, j0 = e_lo - r0 * L;
        for (uint32_t t = tid * ROWS_V; t < A.tile; t += ROWS_THREADS * ROWS_V) {
            const unsigned long long g = g0 + t;
            const unsigned long long gf = max(g, a), gl = min(g + ROWS_V, g1);
            if (gf >= gl) continue;
            const uint32_t k0 = (uint32_t)(gf - g), k1 = (uint32_t)(gl - g);
            unsigned long long d, j;
            rows_rc(gf - a, e_lo, r0, j0, L, d, j);
            int32_t v[ROWS_V] = {0, 0, 0, 0};
            unsigned long long o0 = 0, nid = 0, m = 0, start = 0, lead = 0;
            bool have = false;
#pragma unroll
            for (uint32_t k = 0; k < ROWS_V; k++) {
                if (k < k0 || k >= k1) continue;
                if (!have) {  // d < n_docs: E = n_docs L
                    o0 = A.off[d];
                    nid = A.off[d + 1] - o0;
                    const unsigned long long len = nid + sepd;
                    m = min(len, L);
                    start = A.trunc_left ? len - m : 0;
                    lead = A.pad_left ? L - m : 0;
                    have = true;
                }
                if (j == 0 && A.lengths) A.lengths[d] = (int32_t)m;
                int32_t val = A.pad;
                if (j >= lead && j - lead < m) {
                    const unsigned long long i = start + (j - lead);  // < len
                    // i < nid: the index lies inside [off[d], off[d + 1]), offsets that passed k_rows_check
                    val = i < nid ? A.ids[o0 + i] : A.sep;
                }
                v[k] = val;
                if (++j == L) {
                    j = 0;
                    d++;
                    have = false;
                }
            }
            rows_store<OutT, ROWS_V>(out_al, g, v, k0, k1);
        }
    }
}

}  // namespace bpe
