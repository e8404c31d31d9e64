// k_count.hip -- histogram of token ids that live in HBM (bpe_count_resident).
// Part of bpe_kernels.hip, which includes the parts in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bpe_device.h"
#include "k_common.hip"
#include "k_decode.hip"

namespace bpe {

// ---------------------------------------------------------------------------
// Bins: bin t for a dense id 0 <= t < hi = 256 + M, bin hi + j for the j-th of the sorted pass ids (special tokens).
// BPE numbers its merges by falling pair count, so the low ids carry most of a text: the first L bins are uint32 counters
// in LDS, private to the workgroup, and only the rest -- dense ids >= L, pass ids -- are 64-bit adds to memory.
//
// The grid is fixed (the host sizes it from the CU count) and a workgroup owns one contiguous span of the stream.  The
// span is cut into 16-byte slots by ADDRESS: q = position + (address of ids & 15) / sizeof(IdT), slot s = elements
// [EPV s, EPV s + EPV), so a slot wholly inside [Q0, Q1) is one 16-byte load whatever the alignment of ids; the two slots
// at the ends of the stream are read by element, the way k_project_place treats the ends of a tile.
//   COMBINE   equal ids of one slot are added once, with their multiplicity (text has runs of one id: a lane's four
//             adds to one LDS address become one); without it every id is one add.  Measured the same to 0.001 ms at
//             every L on 18.9 M ids of text: the plain form is the default, option "count_combine".
//   flush     the LDS table goes to scratch[0, L) with one 64-bit add per nonzero counter: when the span is done, and
//             after every `period` slots of it, so that a counter holds at most period x EPV <= 2^31 whatever n is.
// A 64-bit id is compared at its full width.  An id in no bin leaves its position in *bad by atomicMin; the counts of
// such a call are never committed (k_count_commit below is launched only when *bad stayed ~0).
constexpr uint32_t COUNT_THREADS = 1024;
constexpr uint32_t COUNT_UNROLL = 4;        // slots a lane loads before it adds any of them
constexpr uint32_t COUNT_LDS_BINS_MAX = 32768;  // 128 KiB of the CU's 160

template <typename IdT, bool COMBINE>
__global__ void __launch_bounds__(COUNT_THREADS)
k_count(const IdT *__restrict__ ids, uint64_t n, uint32_t L, uint32_t hi, const int32_t *__restrict__ pass,
        uint32_t n_pass, unsigned long long *__restrict__ scratch, unsigned long long *bad, uint64_t period) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_count[];
    constexpr uint32_t EPV = 16 / sizeof(IdT);
    struct alignas(16) Vec {
        IdT e[EPV];
    };
    const uint32_t tid = threadIdx.x;
    const uint64_t a = (uint64_t)(((uintptr_t)ids & 15) / sizeof(IdT));
    const IdT *const ids_al = ids - a;  // 16-byte aligned; ids_al[q] is the element at q
    const uint64_t Q0 = a, Q1 = a + n;
    const uint64_t S = (Q1 + EPV - 1) / EPV, per = (S + gridDim.x - 1) / gridDim.x;
    const uint64_t s0 = min(per * (uint64_t)blockIdx.x, S), s1 = min(s0 + per, S);
    if (s0 == s1) return;  // (the same for every lane of the workgroup)
    for (uint32_t i = tid; i < L; i += COUNT_THREADS) s_count[i] = 0u;
    __syncthreads();
    // w copies of the id v, the first of them at element q
    auto add = [&](long long v, uint32_t w, uint64_t q) {
        if (v >= 0 && v < (long long)L) {
            atomicAdd(&s_count[(uint32_t)v], w);
        } else if (v >= (long long)L && v < (long long)hi) {
            atomicAdd(&scratch[(uint32_t)v], (unsigned long long)w);
        } else {
            const uint32_t t = decode_resolve(v, hi, pass, n_pass);  // hi + j for the j-th pass id
            if (t != 0xFFFFFFFFu)
                atomicAdd(&scratch[t], (unsigned long long)w);
            else
                atomicMin(bad, (unsigned long long)(q - a));
        }
    };
    for (uint64_t p0 = s0; p0 < s1; p0 += period) {
        const uint64_t p1 = min(p0 + period, s1);
        for (uint64_t s = p0 + tid; s < p1; s += (uint64_t)COUNT_UNROLL * COUNT_THREADS) {
            Vec v[COUNT_UNROLL];
            bool whole[COUNT_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < COUNT_UNROLL; u++) {
                const uint64_t sq = (s + (uint64_t)u * COUNT_THREADS) * EPV;
                whole[u] = s + (uint64_t)u * COUNT_THREADS < p1 && sq >= Q0 && sq + EPV <= Q1;
                if (whole[u]) v[u] = *(const Vec *)(ids_al + sq);
            }
#pragma unroll
            for (uint32_t u = 0; u < COUNT_UNROLL; u++) {
                const uint64_t su = s + (uint64_t)u * COUNT_THREADS, sq = su * EPV;
                if (whole[u]) {
#pragma unroll
                    for (uint32_t k = 0; k < EPV; k++) {
                        if (COMBINE) {
                            bool seen = false;
                            uint32_t w = 1;
#pragma unroll
                            for (uint32_t j = 0; j < EPV; j++) {
                                if (j < k) seen |= v[u].e[j] == v[u].e[k];
                                if (j > k) w += v[u].e[j] == v[u].e[k] ? 1u : 0u;
                            }
                            if (!seen) add((long long)v[u].e[k], w, sq + k);
                        } else {
                            add((long long)v[u].e[k], 1u, sq + k);
                        }
                    }
                } else if (su < p1) {  // an end of the stream: exactly its own elements
                    for (uint32_t k = 0; k < EPV; k++) {
                        const uint64_t q = sq + k;
                        if (q >= Q0 && q < Q1) add((long long)ids_al[q], 1u, q);
                    }
                }
            }
        }
        __syncthreads();
        for (uint32_t i = tid; i < L; i += COUNT_THREADS) {
            const uint32_t cnt = s_count[i];
            if (cnt) {
                atomicAdd(&scratch[i], (unsigned long long)cnt);
                s_count[i] = 0u;
            }
        }
        __syncthreads();
    }
}

// counts[i] = (accumulate ? counts[i] : 0) + scratch[i] for the B bins: the only writes to the caller's array
__global__ void __launch_bounds__(256)
k_count_commit(unsigned long long *__restrict__ counts, const unsigned long long *__restrict__ scratch, uint64_t B,
               int accumulate) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += stride)
        counts[i] = (accumulate ? counts[i] : 0ull) + scratch[i];
}

}  // namespace bpe
