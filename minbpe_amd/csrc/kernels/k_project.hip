// k_project.hip -- projection of token ids onto a smaller vocabulary (bpe_project_resident).
// Part of bpe_kernels.hip, which includes the parts in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bpe_device.h"
#include "k_common.hip"
#include "k_decode.hip"

namespace bpe {

// ---------------------------------------------------------------------------
// The table of one vocab_size vs: entry e = id vs + e of the merge range [vs, hi), hi = 256 + M; its expansion is the
// int32 ids tab[toff[e] .. toff[e + 1]), every one of them below vs.  Any other legal id -- below vs, or one of the
// sorted pass ids (special tokens) -- stands for itself.

// Length pass.  A 64-bit id is compared at its full width: one outside the int32 range matches nothing.
template <typename IdT>
__global__ void __launch_bounds__(256)
k_project_len(const IdT *__restrict__ ids, uint64_t n, uint32_t vs, uint32_t hi, const uint32_t *__restrict__ toff,
              const int32_t *__restrict__ pass, uint32_t n_pass, uint32_t *__restrict__ len, unsigned long long *bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const long long v = (long long)ids[i];
        uint32_t L = 0;
        if (v >= 0 && v < (long long)vs) {
            L = 1;
        } else if (v >= (long long)vs && v < (long long)hi) {
            const uint32_t e = (uint32_t)v - vs;
            L = toff[e + 1] - toff[e];
        } else if (decode_resolve(v, 0u, pass, n_pass) != 0xFFFFFFFFu) {
            L = 1;
        } else {
            atomicMin(bad, (unsigned long long)i);
        }
        len[i] = L;
    }
}

// Placement, laid out by the OUTPUT as k_decode_copy_staged is, in elements of IdT instead of bytes.  A workgroup owns a
// tile of tile_tok consecutive tokens, hence one contiguous range of output elements [Q0, Q1), q = element offset +
// (address of out & 15) / sizeof(IdT), so that q % EPV == 0 <=> the address is 16-byte aligned (EPV = elements per 16
// bytes).
//   straight  a tile whose output count equals its token count holds only ids that stand for themselves: they go from
//             ids to out without the window.  A workgroup takes PROJ_GROUP consecutive tiles at a time and asks the same
//             of the whole group first: where nearly nothing expands (vocab_size near 256 + M) it then moves
//             PROJ_GROUP tiles per look at the offsets, while the tile itself stays small for the windows;
//   stage     otherwise the range is walked in windows of W ids (int32 in LDS whatever the id width: every legal id
//             fits).  One token per lane: the part of its expansion inside the window goes from the table (L2) to the
//             window, word stores; a part longer than PROJ_LONG_PART is only listed, and the whole workgroup copies listed
//             parts one word per thread (an expansion may be longer than the window);
//   flush     one 16-byte slot per lane: slots wholly inside [Q0, Q1) are one 16-byte store, the two at the ends of the
//             range element stores of exactly the tile's own elements -- tiles meet at arbitrary elements, no tile writes
//             a neighbour's.
// Every id has passed k_project_len: one outside the merge range stands for itself.
constexpr uint32_t PROJ_LONG_PART = 64;
constexpr uint32_t PROJ_GROUP = 4;
constexpr uint32_t PROJ_WINDOW_MAX = 8192;
constexpr uint32_t PROJ_LONG_CAP = PROJ_WINDOW_MAX / PROJ_LONG_PART;  // parts are disjoint and each longer than PROJ_LONG_PART
struct ProjLong {
    uint32_t src, dst, cnt, pad;  // offset into the table, offset into the window, ids
};
// dynamic LDS of k_project_place: the window, the list, its counter (all of it dynamic: the window stays 16-byte aligned)
constexpr size_t proj_lds_bytes(uint32_t W) { return (size_t)W * 4 + PROJ_LONG_CAP * sizeof(ProjLong) + 16; }

template <typename IdT>
__global__ void __launch_bounds__(256)
k_project_place(const IdT *__restrict__ ids, uint64_t n, uint32_t vs, uint32_t hi, const uint32_t *__restrict__ toff,
                const int32_t *__restrict__ tab, const unsigned long long *__restrict__ off, unsigned long long total,
                IdT *__restrict__ out, uint32_t tile_tok, uint32_t W) {
    extern __shared__ __attribute__((aligned(16))) int32_t s_proj[];
    constexpr uint32_t EPV = 16 / sizeof(IdT);
    struct alignas(16) Vec {
        IdT e[EPV];
    };
    int32_t *const s_win = s_proj;
    ProjLong *const s_long = (ProjLong *)(s_proj + W);
    uint32_t *const s_nlong = (uint32_t *)(s_long + PROJ_LONG_CAP);
    const uint32_t tid = threadIdx.x;
    const unsigned long long a = (unsigned long long)(((uintptr_t)out & 15) / sizeof(IdT));
    IdT *const out_al = out - a;  // 16-byte aligned; out_al[q] is the element at q
    if (tid == 0) *s_nlong = 0;
    __syncthreads();
    // ids [t0, t0 + (Q1 - Q0)) to the elements [Q0, Q1), every one standing for itself (the same for every lane of the
    // workgroup: no barrier inside)
    auto straight = [&](uint64_t t0, unsigned long long Q0, unsigned long long Q1) {
        const IdT *const src = ids + t0;
        const unsigned long long first = Q0 & ~(unsigned long long)(EPV - 1);
        const uint32_t nslots = (uint32_t)((Q1 - first + EPV - 1) / EPV);
        for (uint32_t s = tid; s < nslots; s += 256) {
            const unsigned long long sq = first + (unsigned long long)EPV * s;
            if (sq >= Q0 && sq + EPV <= Q1) {
                Vec v;
#pragma unroll
                for (uint32_t e = 0; e < EPV; e++) v.e[e] = src[sq + e - Q0];
                *(Vec *)(out_al + sq) = v;
            } else {
                for (uint32_t e = 0; e < EPV; e++) {
                    const unsigned long long q = sq + e;
                    if (q >= Q0 && q < Q1) out_al[q] = src[q - Q0];
                }
            }
        }
    };
    const uint64_t group_tok = (uint64_t)PROJ_GROUP * tile_tok, ngroups = (n + group_tok - 1) / group_tok;
    for (uint64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint64_t g0 = g * group_tok, g1 = min(g0 + group_tok, n);
        const unsigned long long G0 = off[g0] + a, G1 = (g1 < n ? off[g1] : total) + a;
        if (G1 - G0 == g1 - g0) {
            straight(g0, G0, G1);
            continue;
        }
        for (uint64_t t0 = g0; t0 < g1; t0 += tile_tok) {
            const uint64_t t1 = min(t0 + (uint64_t)tile_tok, g1);
            const unsigned long long Q0 = off[t0] + a, Q1 = (t1 < n ? off[t1] : total) + a;
            if (Q1 - Q0 == t1 - t0) {
                straight(t0, Q0, Q1);
                continue;
            }
            for (unsigned long long ws = Q0 & ~(unsigned long long)(EPV - 1); ws < Q1; ws += W) {
                const unsigned long long we = min(ws + (unsigned long long)W, Q1);
                // ---- stage
                for (uint64_t i = t0 + tid; i < t1; i += 256) {
                    const unsigned long long tq = off[i] + a;
                    if (tq >= we) break;  // (positions ascend: this lane's later tokens lie further on)
                    const long long v = (long long)ids[i];
                    if (v < (long long)vs || v >= (long long)hi) {  // stands for itself
                        if (tq >= ws) s_win[tq - ws] = (int32_t)v;
                        continue;
                    }
                    const uint32_t e = (uint32_t)v - vs;
                    const uint32_t s0 = toff[e], L = toff[e + 1] - s0;
                    const unsigned long long lo = max(tq, ws), hi_q = min(tq + L, we);
                    if (hi_q <= lo) continue;
                    const uint32_t so = s0 + (uint32_t)(lo - tq);
                    const uint32_t d = (uint32_t)(lo - ws), cnt = (uint32_t)(hi_q - lo);
                    if (cnt > PROJ_LONG_PART) {
                        const uint32_t k = atomicAdd(s_nlong, 1u);
                        s_long[k].src = so;
                        s_long[k].dst = d;
                        s_long[k].cnt = cnt;
                        continue;
                    }
                    for (uint32_t c = 0; c < cnt; c++) s_win[d + c] = tab[so + c];
                }
                __syncthreads();
                const uint32_t nl = *s_nlong;
                for (uint32_t k = 0; k < nl; k++) {
                    const int32_t *src = tab + s_long[k].src;
                    int32_t *dst = s_win + s_long[k].dst;
                    const uint32_t cnt = s_long[k].cnt;
                    for (uint32_t b = tid; b < cnt; b += 256) dst[b] = src[b];
                }
                __syncthreads();
                if (tid == 0) *s_nlong = 0;
                // ---- flush
                const uint32_t nslots = (uint32_t)((we - ws + EPV - 1) / EPV);
                for (uint32_t s = tid; s < nslots; s += 256) {
                    const unsigned long long sq = ws + (unsigned long long)EPV * s;
                    if (sq >= Q0 && sq + EPV <= Q1) {
                        Vec v;
#pragma unroll
                        for (uint32_t e = 0; e < EPV; e++) v.e[e] = (IdT)s_win[EPV * s + e];
                        *(Vec *)(out_al + sq) = v;
                    } else {
                        for (uint32_t e = 0; e < EPV; e++) {
                            const unsigned long long q = sq + e;
                            if (q >= Q0 && q < Q1) out_al[q] = (IdT)s_win[EPV * s + e];
                        }
                    }
                }
                __syncthreads();  // (the window and the list are free again)
            }
        }
    }
}

}  // namespace bpe
