// k_minhash.hip -- near-duplicate documents: the MinHash signature of every document of an id stream
// (bpe_minhash_resident) and the agreement of pairs of signatures (bpe_minhash_agree_resident), DESIGN 4.10.
// Part of bpe_kernels.hip, which includes the parts in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bpe_device.h"
#include "k_common.hip"
#include "k_seldocs.hip"

namespace bpe {

// ---------------------------------------------------------------------------
// minhash: ids [n] + off [n_docs + 1] (+ max_len, tail) + ngram w + A, B [P] -> sig [n_docs][P]
//   key(d) = ids[s_d : s_d + l_d], (s_d, l_d) = seldocs_slice of document d: what selection would emit for it.
//   ww = min(w, l_d); the key holds m_d = l_d - ww + 1 shingles (none when l_d == 0), shingle i over key[i : i + ww):
//   s = 0; s = s * 0x01000193 + tok(id) for its ids in order; S_i = fmix32(s ^ seed ^ ww), all mod 2^32.
//   sig[d][p] = min_i ((A_p S_i + B_p) mod 2^64) >> 33, and 0x7FFFFFFF where there is no shingle.
// Two passes.  prefill: the rows that the signature pass folds into by atomicMin, and those it never writes, are set to
// 0x7FFFFFFF.  signature: laid out by the STREAM, a tile of positions per workgroup; per chunk of a tile the shingle
// that starts at every position goes to LDS with its document's number, then every wave walks its strip of the chunk
// with a permutation per lane.  No kernel waits for another workgroup.

constexpr uint32_t MH_THREADS = 256;
constexpr uint32_t MH_WAVES = MH_THREADS / 64;
constexpr uint32_t MH_TILE_MAX = 65536;
constexpr uint32_t MH_CHUNK = 2048;       // positions of a tile whose shingles are in LDS at a time (a smaller tile: all of it)
constexpr uint32_t MH_NGRAM_MAX = 64;
constexpr uint32_t MH_PERM_MAX = 1024;
constexpr uint32_t MH_STAGE = 1024;       // documents of a tile whose starts are staged in LDS
constexpr uint32_t MH_NONE = ~0u;         // "no shingle starts here"
constexpr uint32_t MH_EMPTY = 0x7FFFFFFFu;  // the signature word of no shingle: above every value >> 33 can give, or equal to the largest

// positions of a strip: what one wave walks of a chunk; strips begin at multiples of their length in units of g (below)
__host__ __device__ __forceinline__ uint32_t mh_strip(uint32_t tile) { return (tile < MH_CHUNK ? tile : MH_CHUNK) / MH_WAVES; }

// the finaliser of murmur3's 32-bit hash: every input bit reaches every output bit
__device__ __forceinline__ uint32_t mh_fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}
// what an id adds to its shingles: the id at its full width, sign-extended to 64 bits (an int32 id and the int64 id of
// the same value hash alike; two int64 ids that differ only above bit 32 do not)
template <typename T>
__device__ __forceinline__ uint32_t mh_tok(T x) {
    const unsigned long long v = (unsigned long long)(long long)x;
    return mh_fmix32((uint32_t)v ^ ((uint32_t)(v >> 32) * 0x9E3779B1u));
}
// the shingles of a key of l ids
__device__ __forceinline__ uint32_t mh_count(uint32_t l, uint32_t w) { return l == 0 ? 0 : l - min(w, l) + 1; }
// whether the m > 0 shingles that start at stream positions [ks, ks + m) lie in more than one strip: the ONE statement of
// which rows are folded by atomicMin (and so prefilled) and which are stored plainly
__device__ __forceinline__ bool mh_split(unsigned long long a, uint32_t ks, uint32_t m, uint32_t strip_shift) {
    return ((a + ks) >> strip_shift) != ((a + ks + m - 1) >> strip_shift);
}

// Prefill pass.  A wave takes 64 documents at a time, one per lane, and sets the rows of those among them that have no
// shingle (an empty key: the signature pass never writes the row) or whose shingles lie in more than one strip (it folds
// into the row) -- a few in a hundred of a corpus of short documents, so that the signature is written once, not twice.
__global__ void __launch_bounds__(256)
k_mh_prefill(const unsigned long long *__restrict__ off, uint64_t n_docs, unsigned long long max_len, uint32_t tail,
             uint32_t w, uint32_t P, unsigned long long a, uint32_t strip_shift, int32_t *__restrict__ sig) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = (uint64_t)gridDim.x * 4;
    const uint64_t chunks = (n_docs + 63) / 64;
    for (uint64_t ch = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); ch < chunks; ch += nwaves) {  // bound: chunks / nwaves + 1
        const uint64_t d64 = ch * 64 + lane;
        bool need = false;
        if (d64 < n_docs) {
            uint32_t l, s;
            seldocs_slice(off[d64], off[d64 + 1], max_len, tail, l, s);
            const uint32_t m = mh_count(l, w);
            need = m == 0 || mh_split(a, s, m, strip_shift);
        }
        for (unsigned long long todo = __ballot(need); todo; todo &= todo - 1) {  // bound: 64 rounds, one per lane
            int32_t *const row = sig + (ch * 64 + (uint64_t)(__ffsll(todo) - 1)) * P;
            for (uint32_t p = lane; p < P; p += 64) row[p] = (int32_t)MH_EMPTY;  // bound: P / 64 + 1 <= 16
        }
    }
}

struct MhArgs {
    const void *ids;
    const unsigned long long *off;  // n_docs + 1 entries that passed k_rows_check
    unsigned long long n_docs;
    unsigned long long p0, p1;      // off[0] < off[n_docs]: the stream positions that belong to a document
    unsigned long long max_len;
    uint32_t tail, tile, ngram, n_perm, seed32;
    const unsigned long long *ab;   // A_0 .. A_{P-1} | B_0 .. B_{P-1}
    int32_t *sig;                   // prefilled by k_mh_prefill
};

// Signature pass, laid out by the STREAM as k_dup_hash is: a workgroup owns a tile of A.tile consecutive positions in
// units of g = p + a, a = the elements by which `ids` is past a 16-byte boundary.  Position p lies in the document j with
// off[j] <= p < off[j + 1]; the documents of the tile's first and last position by one wave search each, the starts
// between them staged in LDS as 32-bit distances from the first (more than MH_STAGE of them: the same search over global
// memory).  The tile goes through LDS a chunk at a time:
//   1. tok(id) of the chunk's positions and of up to ngram - 1 beyond its end -- the halo: as far as the stream's
//      documents reach, whatever tile, chunk or document that is in; nothing outside [p0, p1) is read.
//   2. a lane per position: its document, the key of that (seldocs_slice), and -- if one of the key's shingles starts
//      here -- the shingle over s_tok into s_S, the document's number into s_D (MH_NONE otherwise: positions outside the
//      key, and those whose window would pass the key's end; a key shorter than the window is one shingle at its start).
//      A shingle reads ids of its own key alone: it stops where the key stops, not where the tile or the chunk does.
//   3. a wave per strip of the chunk, a permutation per lane, A_p and B_p in registers, 64 permutations at a time: every
//      lane reads the same shingle from LDS (a broadcast) and keeps a running minimum, which goes out when the document
//      changes -- at the same position in every lane.  A document whose shingles all lie in this strip is ONE plain store
//      per permutation; one that has shingles in other strips too folds by atomicMin into its prefilled row: minima
//      combine in any order, so sig does not depend on scheduling.
template <typename T>
__global__ void __launch_bounds__(MH_THREADS)
k_mh_sig(const MhArgs A) {
    __shared__ unsigned long long s_j[2];  // first and last document of the tile
    __shared__ uint32_t s_st[MH_STAGE + 4];
    __shared__ __attribute__((aligned(16))) uint32_t s_tok[MH_CHUNK + MH_NGRAM_MAX];
    __shared__ __attribute__((aligned(16))) uint32_t s_S[MH_CHUNK];
    __shared__ __attribute__((aligned(16))) uint32_t s_D[MH_CHUNK];
    __shared__ uint8_t s_X[MH_CHUNK];  // the shingles of the document lie in more than one strip
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const unsigned long long a = (unsigned long long)(((uintptr_t)A.ids & 15) / sizeof(T));
    const T *const ids_al = (const T *)A.ids - a;  // ids_al[g] is position g - a
    const unsigned long long G0 = a + A.p0, G1 = a + A.p1;
    const unsigned long long *const off = A.off;
    const uint32_t w = A.ngram, P = A.n_perm;
    const uint32_t chunk = min(A.tile, MH_CHUNK), SL = chunk / MH_WAVES;  // powers of two, SL >= 16
    const uint32_t strip_shift = (uint32_t)__ffs(SL) - 1;
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
        const bool staged = cnt <= (unsigned long long)MH_STAGE + 1;
        if (staged)
            for (uint32_t k = tid; k < (uint32_t)cnt; k += MH_THREADS)  // bound: (MH_STAGE + 1) / MH_THREADS + 1
                s_st[k] = (uint32_t)(off[j_lo + k] - base);
        for (unsigned long long c0 = g0; c0 < g1; c0 += chunk) {  // bound: A.tile / chunk <= 32
            const unsigned long long c1 = min(c0 + (unsigned long long)chunk, g1), cb = max(c0, gb);
            if (c1 <= cb) continue;  // (a chunk in front of the first document; the same in every lane)
            __syncthreads();         // (the staged starts are there; the chunk before is through)
            const unsigned long long te = min(c1 + w - 1, G1);
            for (unsigned long long g = cb + tid; g < te; g += MH_THREADS)  // bound: (chunk + ngram) / MH_THREADS + 1
                s_tok[g - c0] = mh_tok<T>(ids_al[g]);
            __syncthreads();
            for (uint32_t i = tid; i < chunk; i += MH_THREADS) {  // bound: chunk / MH_THREADS + 1
                const unsigned long long g = c0 + i;
                uint32_t S = 0, D = MH_NONE, X = 0;
                if (g >= cb && g < c1) {
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
                    const uint32_t ww = min(w, kl), m = mh_count(kl, w);
                    const uint32_t kk = (uint32_t)p - ks;  // (p < ks wraps beyond every count)
                    if ((uint32_t)p >= ks && kk < m) {
                        // its ids are key[kk .. kk + ww), kk + ww <= kl: positions below ks + kl <= p1, and below
                        // c1 + w - 1 -- all of them among the tokens above
                        uint32_t s = 0;
                        for (uint32_t k = 0; k < ww; k++) s = s * 0x01000193u + s_tok[i + k];  // bound: ww <= 64
                        S = mh_fmix32(s ^ (A.seed32 ^ ww));
                        D = (uint32_t)j;  // n_docs < 2^32 - 1
                        X = mh_split(a, ks, m, strip_shift) ? 1u : 0u;
                    }
                }
                s_S[i] = S;
                s_D[i] = D;
                s_X[i] = (uint8_t)X;
            }
            __syncthreads();
            const uint32_t i0 = (tid >> 6) * SL;
            for (uint32_t pb = 0; pb < P; pb += 64) {  // bound: P / 64 + 1 <= 16
                const uint32_t perm = pb + lane;
                const bool active = perm < P;
                const unsigned long long Ap = active ? A.ab[perm] : 0ull, Bp = active ? A.ab[P + perm] : 0ull;
                uint32_t cur = MH_NONE, mn = MH_EMPTY, curx = 0;
                auto flush = [&]() {
                    if (cur == MH_NONE || !active) return;
                    int32_t *const word = A.sig + (unsigned long long)cur * P + perm;
                    if (curx) atomicMin(word, (int32_t)mn);
                    else *word = (int32_t)mn;
                };
                auto step = [&](uint32_t dv, uint32_t sv, uint32_t i) {
                    const uint32_t d = __builtin_amdgcn_readfirstlane(dv);  // (the same in every lane: a broadcast read)
                    if (d == MH_NONE) return;
                    if (d != cur) {
                        flush();
                        cur = d;
                        curx = s_X[i];
                        mn = MH_EMPTY;
                    }
                    mn = min(mn, (uint32_t)((Ap * sv + Bp) >> 33));
                };
                for (uint32_t i = i0; i < i0 + SL; i += 4) {  // bound: SL / 4 <= 128
                    const uint4 d4 = *(const uint4 *)&s_D[i], s4 = *(const uint4 *)&s_S[i];
                    const uint32_t dx = __builtin_amdgcn_readfirstlane(d4.x);
                    if (dx == cur && dx != MH_NONE && d4.y == dx && d4.z == dx && d4.w == dx) {  // four more of the document at hand
                        const uint32_t h0 = (uint32_t)((Ap * s4.x + Bp) >> 33), h1 = (uint32_t)((Ap * s4.y + Bp) >> 33);
                        const uint32_t h2 = (uint32_t)((Ap * s4.z + Bp) >> 33), h3 = (uint32_t)((Ap * s4.w + Bp) >> 33);
                        mn = min(mn, min(min(h0, h1), min(h2, h3)));
                    } else {
                        step(d4.x, s4.x, i);
                        step(d4.y, s4.y, i + 1);
                        step(d4.z, s4.z, i + 2);
                        step(d4.w, s4.w, i + 3);
                    }
                }
                flush();
            }
        }
    }
}

// ---------------------------------------------------------------------------
// agreement: sig [n_docs][P] + a, b [m] -> agree[j] = #{p : sig[a_j][p] == sig[b_j][p]}

// an index is compared at its full 64 bits; bad = the lowest j with a_j or b_j outside [0, n_docs)
__global__ void __launch_bounds__(256)
k_mh_pairs_check(const long long *__restrict__ pa, const long long *__restrict__ pb, uint64_t m, uint64_t n_docs,
                 unsigned long long *bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {  // bound: m / stride + 1
        const long long x = pa[j], y = pb[j];
        if (x < 0 || (unsigned long long)x >= n_docs || y < 0 || (unsigned long long)y >= n_docs)
            atomicMin(bad, (unsigned long long)j);
    }
}

// 16 lanes per pair (its indices have passed the check above); vec: the rows are 16-byte aligned (P % 4 == 0 and sig is)
// and go by 16-byte loads, otherwise a word per lane.  Every lane makes the same number of rounds, so the sums below see
// all 16 lanes of a pair.
__global__ void __launch_bounds__(256)
k_mh_agree(const int32_t *__restrict__ sig, uint32_t P, uint32_t vec, const long long *__restrict__ pa,
           const long long *__restrict__ pb, uint64_t m, int32_t *__restrict__ agree) {
    const uint32_t sub = threadIdx.x & 15;
    const uint64_t groups = (uint64_t)gridDim.x * (blockDim.x / 16);
    const uint64_t grp = (uint64_t)blockIdx.x * (blockDim.x / 16) + (threadIdx.x >> 4);
    for (uint64_t j0 = 0; j0 < m; j0 += groups) {  // bound: m / groups + 1
        const uint64_t j = j0 + grp;
        const bool valid = j < m;
        int32_t cnt = 0;
        if (valid) {
            const int32_t *const x = sig + (unsigned long long)pa[j] * P, *const y = sig + (unsigned long long)pb[j] * P;
            if (vec) {
                for (uint32_t v = sub; v < P / 4; v += 16) {  // bound: P / 64 + 1
                    const int4 p = ((const int4 *)x)[v], q = ((const int4 *)y)[v];
                    cnt += (p.x == q.x) + (p.y == q.y) + (p.z == q.z) + (p.w == q.w);
                }
            } else {
                for (uint32_t p = sub; p < P; p += 16) cnt += x[p] == y[p];  // bound: P / 16 + 1
            }
        }
#pragma unroll
        for (int d = 8; d; d >>= 1) cnt += __shfl_xor(cnt, d, 16);  // bound: 4 steps
        if (valid && sub == 0) agree[j] = cnt;
    }
}

}  // namespace bpe
