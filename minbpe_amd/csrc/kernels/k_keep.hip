// k_keep.hip -- cut marked ids out of a stream (bpe_keep_ids_resident).
// Part of bpe_kernels.hip, which includes the parts in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bpe_device.h"
#include "k_common.hip"

namespace bpe {

// ---------------------------------------------------------------------------
// keep: ids [n] + mask [n] + [p0, p1) -> out = the ids at the kept positions, in order.
//   Position p is kept iff p0 <= p < p1 and ((mask[p] & bits) != 0) != drop.  The two passes of resident_two_pass: the
//   length of a position is 0 or 1, the scan of the lengths is where a kept id goes.

// Length pass, one position per thread.  The mask is read inside [p0, p1) only.
__global__ void __launch_bounds__(256)
k_keep_len(const uint8_t *__restrict__ mask, uint64_t n, uint64_t p0, uint64_t p1, uint32_t bits, uint32_t drop,
           uint32_t *__restrict__ len) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {  // bound: n / stride + 1
        uint32_t l = 0;
        if (p >= p0 && p < p1) l = (uint32_t)(((mask[p] & bits) != 0) != (drop != 0));
        len[p] = l;
    }
}

// Placement, one position per thread: a kept id goes to out[oo[p]], oo the exclusive scan of the lengths (below the
// total, which the caller's capacity holds).  Only [p0, p1) is read.
template <typename T>
__global__ void __launch_bounds__(256)
k_keep_place(const T *__restrict__ ids, uint64_t p0, uint64_t p1, const uint32_t *__restrict__ len,
             const unsigned long long *__restrict__ oo, unsigned long long total, T *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = p0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < p1; p += stride) {  // bound: (p1 - p0) / stride + 1
        if (!len[p]) continue;
        const unsigned long long e = oo[p];
        if (e < total) out[e] = ids[p];  // (always: e counts the kept positions before p)
    }
}

}  // namespace bpe
