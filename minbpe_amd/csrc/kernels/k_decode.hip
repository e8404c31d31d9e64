// k_decode.hip -- batch decode.
// Part of bpe_kernels.hip, which includes the parts in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bpe_device.h"
#include "k_common.hip"

namespace bpe {

// ---------------------------------------------------------------------------
// batch decode (N4): token id -> bytes through the vocab table resident in HBM

__global__ void __launch_bounds__(256)
k_decode_len(const int32_t *__restrict__ ids, uint64_t n, const unsigned long long *__restrict__ voff,
             uint32_t V, uint32_t *__restrict__ len, unsigned long long *bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t id = (uint32_t)ids[i];  // negative ids wrap above V
        uint32_t L = 0;
        if (id < V)
            L = (uint32_t)(voff[id + 1] - voff[id]);
        else
            atomicMin(bad, (unsigned long long)i);
        len[i] = L;
    }
}

// One token per lane.  Tokens are a few bytes each, so a wave's 64 tokens cover a few
// hundred consecutive output bytes; the table (<= a few MB) stays in L2.
__global__ void __launch_bounds__(256)
k_decode_copy(const int32_t *__restrict__ ids, uint64_t n, const unsigned long long *__restrict__ voff,
              uint32_t V, const uint8_t *__restrict__ blob, const unsigned long long *__restrict__ off,
              uint8_t *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t id = (uint32_t)ids[i];
        if (id >= V) continue;
        const unsigned long long s0 = voff[id], L = voff[id + 1] - s0, d0 = off[i];
        for (unsigned long long k = 0; k < L; k++) out[d0 + k] = blob[s0 + k];
    }
}

// dst[j] = byte offset of token position idx[j] (position n: the total).  bad (may be NULL: the caller has checked): the
// first j whose position is past n.
__global__ void __launch_bounds__(256)
k_decode_doc_offsets(const unsigned long long *__restrict__ off, uint64_t n, unsigned long long total,
                     const unsigned long long *__restrict__ idx, uint64_t k,
                     unsigned long long *__restrict__ dst, unsigned long long *bad) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const unsigned long long p = idx[j];
    if (p > n && bad) atomicMin(bad, (unsigned long long)j);
    dst[j] = p < n ? off[p] : total;
}

// ---------------------------------------------------------------------------
// resident batch decode (bpe_decode_batch_resident): ids of the caller's, 4 or 8 bytes wide, in HBM

// the table index of id v, 0xFFFFFFFF if it does not decode (shared with the length pass of k_spans.hip)
__device__ __forceinline__ uint32_t decode_resolve(long long v, uint32_t V_dense, const int32_t *__restrict__ sparse,
                                                   uint32_t n_sparse) {
    uint32_t t = 0xFFFFFFFFu;
    if (v >= 0 && v < (long long)V_dense) {
        t = (uint32_t)v;
    } else if (v >= -2147483648ll && v <= 2147483647ll) {
        uint32_t lo = 0, hi = n_sparse;  // first entry >= v
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((long long)sparse[mid] < v) lo = mid + 1; else hi = mid;
        }
        if (lo < n_sparse && (long long)sparse[lo] == v) t = V_dense + lo;
    }
    return t;
}

// Length pass.  An id in [0, V_dense) is its own table index; any other id is looked up in the sorted sparse list
// (special tokens: a few to a few hundred entries, cache resident), entry j being table index V_dense + j.  A 64-bit id is
// compared at its full width: one outside the int32 range matches nothing.  Writes the RESOLVED table index next to the
// length, so that the copy pass reads 4 bytes per token whatever the id width and never searches again.
template <typename IdT>
__global__ void __launch_bounds__(256)
k_decode_res_len(const IdT *__restrict__ ids, uint64_t n, const unsigned long long *__restrict__ voff, uint32_t V_dense,
                 const int32_t *__restrict__ sparse, uint32_t n_sparse, uint32_t *__restrict__ tidx,
                 uint32_t *__restrict__ len, unsigned long long *bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t t = decode_resolve((long long)ids[i], V_dense, sparse, n_sparse);
        uint32_t L = 0;
        if (t != 0xFFFFFFFFu)
            L = (uint32_t)(voff[t + 1] - voff[t]);
        else
            atomicMin(bad, (unsigned long long)i);
        tidx[i] = t != 0xFFFFFFFFu ? t : 0u;
        len[i] = L;
    }
}

// Copy pass, laid out by the OUTPUT.  A workgroup owns a tile of tile_tok consecutive tokens, hence one contiguous range
// of output bytes [B0, B1).  It walks that range in windows of W bytes whose starts are 16-byte aligned ADDRESSES of out:
//   stage  one token per lane: the part of the token inside the window goes from the table (L2) to the LDS window, byte
//          stores into LDS; a part longer than DEC_LONG_PART is only listed, and the whole workgroup copies listed parts
//          one byte per thread (a vocab entry may be any length, also longer than the window);
//   flush  one 16-byte slot per lane: slots that lie wholly inside [B0, B1) are one 16-byte store, the two at the ends of
//          the range byte stores of exactly the tile's own bytes -- tiles meet at arbitrary bytes, no tile writes a
//          neighbour's.
// q = byte offset + (address of out & 15), so that q % 16 == 0 <=> the address is 16-byte aligned.
constexpr uint32_t DEC_LONG_PART = 256;
constexpr uint32_t DEC_WINDOW_MAX = 32768;
constexpr uint32_t DEC_LONG_CAP = DEC_WINDOW_MAX / DEC_LONG_PART;  // parts are disjoint and each longer than DEC_LONG_PART
struct DecLong {
    unsigned long long src;  // offset into the table's bytes
    uint32_t dst, cnt;       // offset into the window, bytes
};

__global__ void __launch_bounds__(256)
k_decode_copy_staged(const uint32_t *__restrict__ tidx, uint64_t n, const unsigned long long *__restrict__ voff,
                     const uint8_t *__restrict__ blob, const unsigned long long *__restrict__ off,
                     unsigned long long total, uint8_t *__restrict__ out, uint32_t tile_tok, uint32_t W) {
    extern __shared__ uint4 s_win4[];
    uint8_t *s_win = (uint8_t *)s_win4;
    __shared__ DecLong s_long[DEC_LONG_CAP];
    __shared__ uint32_t s_nlong;
    const uint32_t tid = threadIdx.x;
    const unsigned long long a = (unsigned long long)((uintptr_t)out & 15);
    uint8_t *const out_al = out - a;  // 16-byte aligned; out_al[q] is the byte at q
    if (tid == 0) s_nlong = 0;
    __syncthreads();
    const uint64_t ntiles = (n + tile_tok - 1) / tile_tok;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * tile_tok, t1 = min(t0 + (uint64_t)tile_tok, n);
        const unsigned long long Q0 = off[t0] + a, Q1 = (t1 < n ? off[t1] : total) + a;
        for (unsigned long long ws = Q0 & ~15ull; ws < Q1; ws += W) {
            const unsigned long long we = min(ws + (unsigned long long)W, Q1);
            // ---- stage
            for (uint64_t i = t0 + tid; i < t1; i += 256) {
                const unsigned long long tq = off[i] + a;
                if (tq >= we) break;  // (positions ascend: this lane's later tokens lie further on)
                const uint32_t t = tidx[i];
                const unsigned long long s0 = voff[t], L = voff[t + 1] - s0;
                const unsigned long long lo = max(tq, ws), hi = min(tq + L, we);
                if (hi <= lo) continue;
                const unsigned long long so = s0 + (lo - tq);
                const uint32_t d = (uint32_t)(lo - ws), cnt = (uint32_t)(hi - lo);
                if (cnt > DEC_LONG_PART) {
                    const uint32_t e = atomicAdd(&s_nlong, 1u);
                    s_long[e].src = so;
                    s_long[e].dst = d;
                    s_long[e].cnt = cnt;
                    continue;
                }
                const uint8_t *src = blob + so;
                uint8_t *dst = s_win + d;
                uint32_t c = 0;
                for (; c + 4 <= cnt; c += 4) {
                    uint32_t v;
                    __builtin_memcpy(&v, src + c, 4);
                    dst[c] = (uint8_t)v;
                    dst[c + 1] = (uint8_t)(v >> 8);
                    dst[c + 2] = (uint8_t)(v >> 16);
                    dst[c + 3] = (uint8_t)(v >> 24);
                }
                for (; c < cnt; c++) dst[c] = src[c];
            }
            __syncthreads();
            const uint32_t nl = s_nlong;
            for (uint32_t e = 0; e < nl; e++) {
                const uint8_t *src = blob + s_long[e].src;
                uint8_t *dst = s_win + s_long[e].dst;
                const uint32_t cnt = s_long[e].cnt;
                for (uint32_t b = tid; b < cnt; b += 256) dst[b] = src[b];
            }
            __syncthreads();
            if (tid == 0) s_nlong = 0;
            // ---- flush
            const uint32_t nslots = (uint32_t)((we - ws + 15) >> 4);
            for (uint32_t s = tid; s < nslots; s += 256) {
                const unsigned long long sq = ws + 16ull * s;
                if (sq >= Q0 && sq + 16 <= Q1) {
                    *(uint4 *)(out_al + sq) = s_win4[s];
                } else {
                    for (uint32_t b = 0; b < 16; b++) {
                        const unsigned long long q = sq + b;
                        if (q >= Q0 && q < Q1) out_al[q] = s_win[16 * s + b];
                    }
                }
            }
            __syncthreads();  // (the window and the list are free again)
        }
    }
}

}  // namespace bpe
