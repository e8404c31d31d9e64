// k_spans.hip -- resident token spans: the byte and character offsets of every token inside its document.
// Part of bpe_kernels.hip, which includes the parts in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bpe_device.h"
#include "k_common.hip"
#include "k_decode.hip"

namespace bpe {

// ---------------------------------------------------------------------------
// token spans (bpe_token_spans_resident): ids [n] int32 / int64 (+ doc_offsets [n_docs + 1] uint64) -> byte spans and
// character spans, int64 [n][2] each
//
// e(t) = the bytes of table entry t.  A byte b is a LEAD if (b & 0xC0) != 0x80: ASCII, UTF-8 start bytes and bytes that
// are no UTF-8 at all; only 10xxxxxx is not.  len = len(e(t)), leads = the lead bytes of e(t), cont = 1 if len > 0 and
// the first byte of e(t) is no lead.  With B_i, C_i the sums of len and of leads over the tokens before i of the same
// document:  byte span = (B_i, B_i + len_i),  char span = (max(C_i - cont_i, 0), C_i + leads_i).

constexpr uint32_t SPANS_THREADS = 256;
constexpr uint32_t SPANS_TILE = 1024;       // tokens per workgroup tile of the emit pass
constexpr uint32_t SPANS_STAGE_MAX = 4096;  // document starts a tile stages in LDS, 4 bytes each (relative to the tile's first)
constexpr uint32_t SPANS_CONT = 0x80000000u;

// Table meta, one wave per entry: meta[t] = leads | cont << 31, from the blob in HBM (an entry may be 0 bytes or tens of
// thousands: the lanes stride over it).  limit: set to 1 by an entry of 2^31 lead bytes or more.
__global__ void __launch_bounds__(256)
k_spans_meta(const uint8_t *__restrict__ blob, const unsigned long long *__restrict__ voff, uint32_t V,
             uint32_t *__restrict__ meta, unsigned long long *limit) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t t = (uint64_t)blockIdx.x * 4 + (uint32_t)wave_id(); t < V; t += nwaves) {
        const unsigned long long s0 = voff[t], L = voff[t + 1] - s0;
        unsigned long long acc = 0;
        for (unsigned long long k = lane; k < L; k += 64) acc += (blob[s0 + k] & 0xC0) != 0x80;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
        if (lane == 0) {
            const uint32_t cont = (L > 0 && (blob[s0] & 0xC0) == 0x80) ? SPANS_CONT : 0u;
            if (acc >= 0x80000000ull) {
                *limit = 1ull;  // (every writer writes the same value)
                acc = 0;
            }
            meta[t] = (uint32_t)acc | cont;
        }
    }
}

// Length pass: the resolution of k_decode_res_len (decode_resolve), then len[i] and lw[i] = leads | cont << 31 of the
// entry; an id that does not decode leaves zeros and its position in bad (the first one: atomicMin).
template <typename IdT>
__global__ void __launch_bounds__(256)
k_spans_len(const IdT *__restrict__ ids, uint64_t n, const unsigned long long *__restrict__ voff,
            const uint32_t *__restrict__ meta, uint32_t V_dense, const int32_t *__restrict__ sparse, uint32_t n_sparse,
            uint32_t *__restrict__ len, uint32_t *__restrict__ lw, unsigned long long *bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t t = decode_resolve((long long)ids[i], V_dense, sparse, n_sparse);
        uint32_t L = 0, m = 0;
        if (t != 0xFFFFFFFFu) {
            L = (uint32_t)(voff[t + 1] - voff[t]);
            m = meta[t];
        } else {
            atomicMin(bad, (unsigned long long)i);
        }
        len[i] = L;
        lw[i] = m;
    }
}

// Exclusive scan of (len, leads) to 64-bit sums: k_scan_blocksum / k_scan_top / k_scan_apply (k_encode.hip) with both
// channels carried in one pass each.  No workgroup waits for another: three launches.
__global__ void __launch_bounds__(256)
k_spans_blocksum(const uint32_t *__restrict__ len, const uint32_t *__restrict__ lw, uint64_t n,
                 unsigned long long *__restrict__ bsum_b, unsigned long long *__restrict__ bsum_c) {
    __shared__ unsigned long long s_red[2][4];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
    unsigned long long ab = 0, ac = 0;
    for (uint32_t i = threadIdx.x; i < SCAN_TILE; i += 256)
        if (base + i < n) {
            ab += len[base + i];
            ac += lw[base + i] & ~SPANS_CONT;
        }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        ab += __shfl_xor(ab, d);
        ac += __shfl_xor(ac, d);
    }
    if (lane_id() == 0) {
        s_red[0][wave_id()] = ab;
        s_red[1][wave_id()] = ac;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        bsum_b[blockIdx.x] = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3];
        bsum_c[blockIdx.x] = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
    }
}
// grid of 2: workgroup 0 scans the block sums of the bytes, workgroup 1 those of the leads; totals[0], totals[1]
__global__ void __launch_bounds__(1024)
k_spans_scan_top(unsigned long long *__restrict__ bsum_b, unsigned long long *__restrict__ bsum_c, uint64_t nb,
                 unsigned long long *__restrict__ totals) {
    __shared__ unsigned long long s_part[1024];
    unsigned long long *const bsum = blockIdx.x == 0 ? bsum_b : bsum_c;
    const uint64_t R = (nb + 1023) / 1024;
    const uint64_t b0 = min((uint64_t)threadIdx.x * R, nb), b1 = min(b0 + R, nb);
    unsigned long long acc = 0;
    for (uint64_t b = b0; b < b1; b++) acc += bsum[b];
    s_part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int i = 0; i < 1024; i++) {
            const unsigned long long t = s_part[i];
            s_part[i] = run;
            run += t;
        }
        totals[blockIdx.x] = run;
    }
    __syncthreads();
    unsigned long long run = s_part[threadIdx.x];
    for (uint64_t b = b0; b < b1; b++) {
        const unsigned long long t = bsum[b];
        bsum[b] = run;
        run += t;
    }
}
// Apply pass.  A workgroup walks its SCAN_TILE values in rounds of 1024: a lane owns 4 CONSECUTIVE values per round, so that
// its loads are 16 bytes and its stores two times 16 bytes per channel, lane after lane (16 consecutive values per lane,
// as k_scan_apply has them, are 64-byte strides between the lanes of every load and store: 0.33 ms for 18.9 M tokens
// against 0.20 ms for the emit pass, which moves twice the bytes).  len, lw and the two outputs are the ctx's own
// allocations, 16-byte aligned, and a round starts at a multiple of 4.
__global__ void __launch_bounds__(256)
k_spans_scan_apply(const uint32_t *__restrict__ len, const uint32_t *__restrict__ lw, uint64_t n,
                   const unsigned long long *__restrict__ bsum_b, const unsigned long long *__restrict__ bsum_c,
                   unsigned long long *__restrict__ out_b, unsigned long long *__restrict__ out_c) {
    __shared__ unsigned long long s_w[2][4];
    constexpr uint32_t ROUND = 256 * 4;
    const uint64_t tile0 = (uint64_t)blockIdx.x * SCAN_TILE;
    unsigned long long carry_b = bsum_b[blockIdx.x], carry_c = bsum_c[blockIdx.x];
    const int lane = lane_id(), wave = wave_id();
    for (uint32_t r = 0; r < SCAN_TILE; r += ROUND) {
        if (tile0 + r >= n) break;  // (the same in every lane)
        const uint64_t base = tile0 + r + (uint64_t)threadIdx.x * 4;
        const bool whole = base + 4 <= n;
        uint32_t xb[4] = {0, 0, 0, 0}, xc[4] = {0, 0, 0, 0};
        if (whole) {
            const uint4 vb = *(const uint4 *)(len + base), vc = *(const uint4 *)(lw + base);
            xb[0] = vb.x; xb[1] = vb.y; xb[2] = vb.z; xb[3] = vb.w;
            xc[0] = vc.x; xc[1] = vc.y; xc[2] = vc.z; xc[3] = vc.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (base + i < n) {
                    xb[i] = len[base + i];
                    xc[i] = lw[base + i];
                }
        }
        unsigned long long ab = 0, ac = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            xc[i] &= ~SPANS_CONT;
            ab += xb[i];
            ac += xc[i];
        }
        unsigned long long ib = ab, ic = ac;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long ob = __shfl_up(ib, d), oc = __shfl_up(ic, d);
            if (lane >= d) {
                ib += ob;
                ic += oc;
            }
        }
        if (lane == 63) {
            s_w[0][wave] = ib;
            s_w[1][wave] = ic;
        }
        __syncthreads();
        unsigned long long rb = carry_b + ib - ab, rc = carry_c + ic - ac;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            if (w < wave) {
                rb += s_w[0][w];
                rc += s_w[1][w];
            }
            carry_b += s_w[0][w];
            carry_c += s_w[1][w];
        }
        unsigned long long yb[4], yc[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            yb[i] = rb;
            yc[i] = rc;
            rb += xb[i];
            rc += xc[i];
        }
        if (whole) {
            *(ulonglong2 *)(out_b + base) = make_ulonglong2(yb[0], yb[1]);
            *(ulonglong2 *)(out_b + base + 2) = make_ulonglong2(yb[2], yb[3]);
            *(ulonglong2 *)(out_c + base) = make_ulonglong2(yc[0], yc[1]);
            *(ulonglong2 *)(out_c + base + 2) = make_ulonglong2(yc[2], yc[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (base + i < n) {
                    out_b[base + i] = yb[i];
                    out_c[base + i] = yc[i];
                }
        }
        __syncthreads();  // (s_w is free for the next round)
    }
}

struct SpansArgs {
    const uint32_t *len, *lw;              // per token: bytes, leads | cont << 31
    const unsigned long long *sb, *sc;     // per token: exclusive sums over the BATCH of the bytes and of the leads
    unsigned long long n;
    const unsigned long long *off;         // n_docs + 1 entries, validated (k_rows_check) before the emit pass is launched
    unsigned long long n_docs;
    unsigned long long off0, offn;         // off[0], off[n_docs]
    const unsigned long long *base_b, *base_c;  // per offset entry: the sums at that token position (position n: the totals)
    long long *byte_spans, *char_spans;    // [n][2] each, either may be NULL; 8-byte aligned
    uint32_t stage;
};

// one token's pair: a 16-byte store where the array's address allows (al: uniform over the launch), two 8-byte stores
// otherwise.  Element 2 i + 1 < 2 n: nothing outside the first 2 n elements is written.
__device__ __forceinline__ void spans_store(long long *out, unsigned long long i, long long a, long long b, bool al) {
    long long *p = out + 2 * i;
    if (al) {
        *(longlong2 *)p = make_longlong2(a, b);
    } else {
        p[0] = a;
        p[1] = b;
    }
}

// Emit pass.  A workgroup owns a tile of SPANS_TILE consecutive tokens, lane after lane, so that a wave's 64 pairs are
// 1 KiB of consecutive output.  DOC: the tile's tokens that lie in a document are [lo_i, hi_e); one search each for the
// documents of the first and the last of them (d = upper_bound(off, i) - 1 over ALL documents, 64 probes at a time, as in
// k_rows_pack), the document starts between them staged in LDS as 32-bit distances from the first, and every lane
// searches there.  More starts than the staging area holds (A.stage; thousands of empty documents in a row), or starts
// 2^32 apart: the same search over global memory.  A token before off[0] or from off[n_docs] on gets (-1, -1).
// DOC = false: one document, its bases 0, no search at all.
template <bool DOC>
__global__ void __launch_bounds__(SPANS_THREADS)
k_spans_emit(const SpansArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_spans[];
    uint32_t *const s_sh = (uint32_t *)(s_spans + 2);  // s_spans[0], s_spans[1]: first and last document of the tile
    const uint32_t tid = threadIdx.x;
    const bool al_b = ((uintptr_t)A.byte_spans & 15) == 0, al_c = ((uintptr_t)A.char_spans & 15) == 0;
    const unsigned long long *const off = A.off;
    const uint64_t ntiles = (A.n + SPANS_TILE - 1) / SPANS_TILE;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const unsigned long long t0 = tile * SPANS_TILE, t1 = min(t0 + (unsigned long long)SPANS_TILE, A.n);
        unsigned long long lo_i = t0, hi_e = t1, d_lo = 0, d_hi = 0, base = 0;
        bool staged = false;
        if constexpr (DOC) {
            lo_i = max(t0, A.off0);
            hi_e = min(t1, A.offn);
            __syncthreads();  // (the staging area of the tile before is free)
            if (lo_i < hi_e) {  // off[0] <= lo_i <= hi_e - 1 < off[n_docs]: n_docs >= 1
                if (tid < 128) {
                    const uint32_t lane = tid & 63;
                    const unsigned long long q = tid < 64 ? lo_i : hi_e - 1;
                    unsigned long long lo = 1, hi = A.n_docs;  // the first d in [lo, hi] with off[d] > q: off[n_docs] > q
                    while (lo < hi) {  // (lo and hi come from the ballot: the same in all lanes)
                        const unsigned long long b = lo, span = hi - lo;
                        const unsigned long long p = b + ((span * lane) >> 6);  // b = p_0 <= ... <= p_63 < hi
                        const unsigned long long beyond = __ballot(off[p] > q);  // (off ascends: a suffix of the lanes)
                        if (beyond == 0) {
                            lo = b + ((span * 63) >> 6) + 1;
                        } else {
                            const uint32_t f = (uint32_t)__ffsll(beyond) - 1;
                            hi = b + ((span * f) >> 6);
                            if (f) lo = b + ((span * (f - 1)) >> 6) + 1;
                        }
                    }
                    if (lane == 0) s_spans[tid >> 6] = lo - 1;
                }
                __syncthreads();
                d_lo = s_spans[0];
                d_hi = s_spans[1];
                const unsigned long long cnt = d_hi - d_lo + 2;  // off[d_lo] .. off[d_hi + 1], d_hi + 1 <= n_docs
                base = off[d_lo];
                staged = cnt <= (unsigned long long)A.stage && off[d_hi + 1] - base <= 0xFFFFFFFFull;
                if (staged)
                    for (uint32_t k = tid; k < (uint32_t)cnt; k += SPANS_THREADS) s_sh[k] = (uint32_t)(off[d_lo + k] - base);
                __syncthreads();
            }
        }
        for (unsigned long long i = t0 + tid; i < t1; i += SPANS_THREADS) {
            long long b0 = -1, b1 = -1, c0 = -1, c1 = -1;
            if (i >= lo_i && i < hi_e) {
                unsigned long long bb = 0, bc = 0;
                if constexpr (DOC) {
                    unsigned long long d;  // off[d_lo] <= i < off[d_hi + 1]
                    if (staged) {  // 32-bit: entry k is off[d_lo + k] - base, i - base < entry d_hi + 1 - d_lo
                        const uint32_t qr = (uint32_t)(i - base);
                        uint32_t lo = 1, hi = (uint32_t)(d_hi - d_lo) + 1;
                        while (lo < hi) {
                            const uint32_t mid = (lo + hi) >> 1;
                            if (s_sh[mid] > qr) hi = mid; else lo = mid + 1;
                        }
                        d = d_lo + lo - 1;
                    } else {
                        unsigned long long lo = d_lo + 1, hi = d_hi + 1;
                        while (lo < hi) {
                            const unsigned long long mid = lo + ((hi - lo) >> 1);
                            if (off[mid] > i) hi = mid; else lo = mid + 1;
                        }
                        d = lo - 1;
                    }
                    bb = A.base_b[d];  // d <= n_docs - 1: inside the n_docs + 1 bases
                    bc = A.base_c[d];
                }
                const uint32_t m = A.lw[i];
                const long long pb = (long long)(A.sb[i] - bb), pc = (long long)(A.sc[i] - bc);
                b0 = pb;
                b1 = pb + (long long)A.len[i];
                c0 = max(pc - (long long)(m >> 31), 0ll);
                c1 = pc + (long long)(m & ~SPANS_CONT);
            }
            if (A.byte_spans) spans_store(A.byte_spans, i, b0, b1, al_b);
            if (A.char_spans) spans_store(A.char_spans, i, c0, c1, al_c);
        }
    }
}

}  // namespace bpe
