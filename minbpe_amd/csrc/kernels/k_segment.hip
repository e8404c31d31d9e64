// k_segment.hip -- the segments (lines) of every document as a stream of its own, and per-segment verdicts back as marks
// (bpe_segment_docs_resident, bpe_segment_marks_resident).
// Part of bpe_kernels.hip, which includes the parts in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bpe_device.h"
#include "k_common.hip"

namespace bpe {

// ---------------------------------------------------------------------------
// segments: ids [n] + off [n_docs + 1] + class [n_class] -> out = the content ids of all segments, in order.
//   class(t) = cls[t] & 3 for 0 <= t < n_class at the id's full width, else 0.  Inside a document one bit of state,
//   FRESH at its start: a position without SKIP is content, content seen in state FRESH starts a segment, content sets
//   OPEN, BREAK sets FRESH behind the position, SKIP alone changes nothing.
// The state in front of a position is "the last event that is not the identity" over everything before it: a scan over
// the monoid {identity, ->FRESH, ->OPEN}, a document start being ->FRESH in front of its position.  Its three levels:
// ballots inside a wave, LDS across the waves of a tile, a summary byte per tile across tiles -- written by one launch
// (k_seg_classify), scanned by the next (k_seg_carry), read by the third (k_seg_mark).  No workgroup waits for another
// inside a launch.

constexpr uint32_t SEG_THREADS = 256;      // 4 waves: a round of a tile is 256 consecutive positions, 64 per wave
constexpr uint32_t SEG_TILE_MAX = 65536;
constexpr uint32_t SEG_STAGE_MAX = 4096;   // ranges a tile of the marks pass stages in LDS, 8 bytes each
constexpr uint32_t SEG_ID = 0, SEG_FRESH = 1, SEG_OPEN = 2;  // the monoid; FRESH and OPEN are also the two states
constexpr uint32_t SEG_F_DOC = 1;          // flag byte, bit 0: a document starts here; bits 1..2: the class of the id
constexpr uint32_t SEG_CLS_BREAK = 1, SEG_CLS_SKIP = 2;  // (BPE_SEG_BREAK, BPE_SEG_SKIP of the header)

// what position does to the state behind it, its own document start included: BREAK wins over content, content over a
// document start, and SKIP alone hands on what was there
__device__ __forceinline__ uint32_t seg_event(uint32_t f) {
    const uint32_t cls = f >> 1;
    if (cls & SEG_CLS_BREAK) return SEG_FRESH;
    if (!(cls & SEG_CLS_SKIP)) return SEG_OPEN;
    return (f & SEG_F_DOC) ? SEG_FRESH : SEG_ID;
}
// the last event of `mask` (bit l: lane l has one) that is not the identity, OPEN where `open` has the bit: 0 without one
__device__ __forceinline__ uint32_t seg_last(unsigned long long mask, unsigned long long open) {
    if (!mask) return SEG_ID;
    const uint32_t top = 63u - (uint32_t)__clzll((long long)mask);
    return ((open >> top) & 1ull) ? SEG_OPEN : SEG_FRESH;
}

// Document starts as a flag byte per position, one document per thread: flag[off[d]] = 1 for every start inside
// [p0, p1).  An empty document flags the position of the document behind it, which starts there as well, and several
// documents at one position store the same byte: both are harmless.  A start at p1 (trailing empty documents) is
// skipped: p1 may be n.  The caller has zeroed flag[p0, p1).
__global__ void __launch_bounds__(256)
k_seg_docstart(const unsigned long long *__restrict__ off, uint64_t n_docs, uint64_t p1, uint8_t *__restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n_docs; d += stride) {  // bound: n_docs / stride + 1
        const unsigned long long p = off[d];
        if (p < p1) flag[p] = (uint8_t)SEG_F_DOC;
    }
}

struct SegArgs {
    const void *ids;
    const uint8_t *cls;            // n_class entries (NULL with n_class == 0)
    unsigned long long n_class;
    unsigned long long p0, p1;     // the positions that take part, p0 < p1
    uint32_t tile, tag;            // positions per workgroup tile (a multiple of 64); 1 = a tag id in front of every segment
    uint8_t *flag;                 // [n] document start | class << 1, valid inside [p0, p1)
    uint8_t *sum;                  // per tile: its summary, after k_seg_carry the state in front of it
    uint32_t *len_o, *len_s;       // [n] output elements and segment starts per position (the two scan inputs)
};

// Launch 1, a tile per workgroup: the class of every id into its flag byte -- so that the ids and the table are read
// once -- and the tile's summary, the last event in it that is not the identity.
template <typename T>
__global__ void __launch_bounds__(SEG_THREADS)
k_seg_classify(const SegArgs A) {
    __shared__ uint32_t s_key[SEG_THREADS / 64];
    const T *const ids = (const T *)A.ids;
    const uint32_t tid = threadIdx.x;
    const uint64_t ntiles = (A.p1 - A.p0 + A.tile - 1) / A.tile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // bound: ntiles / gridDim.x + 1
        const unsigned long long base = A.p0 + t * A.tile, end = min(base + (unsigned long long)A.tile, A.p1);
        uint32_t key = 0;  // (index in the tile + 1) << 1 | OPEN of this lane's last event
        for (uint32_t r = tid; r < A.tile; r += SEG_THREADS) {  // bound: tile / 256 + 1
            const unsigned long long p = base + r;
            if (p >= end) break;
            const long long v = (long long)ids[p];  // (sign-extended: compared at its full width)
            uint32_t cls = 0;
            if (v >= 0 && (unsigned long long)v < A.n_class) cls = A.cls[v] & 3u;
            const uint32_t f = (A.flag[p] & SEG_F_DOC) | (cls << 1);
            A.flag[p] = (uint8_t)f;
            const uint32_t ev = seg_event(f);
            if (ev != SEG_ID) key = ((r + 1) << 1) | (ev == SEG_OPEN ? 1u : 0u);  // (r ascends: the last one stays)
        }
        key = wave_umax_dpp(key);
        if ((tid & 63) == 0) s_key[tid >> 6] = key;
        __syncthreads();
        if (tid == 0) {
            uint32_t k = 0;
#pragma unroll
            for (uint32_t w = 0; w < SEG_THREADS / 64; w++) k = max(k, s_key[w]);
            A.sum[t] = (uint8_t)(k == 0 ? SEG_ID : (k & 1u) ? SEG_OPEN : SEG_FRESH);
        }
        __syncthreads();  // (s_key is free for the next tile)
    }
}

// Launch 2, ONE workgroup: sum[t] = the state in front of tile t = the last summary below t that is not the identity,
// FRESH without one (a document starts at p0).  k_scan_top's shape: a thread owns R consecutive tiles, the 1024 partial
// results are scanned by one thread, then every thread rewrites its own tiles.  A run of all-identity tiles of any length
// hands the state on unchanged.
__global__ void __launch_bounds__(1024)
k_seg_carry(uint8_t *__restrict__ sum, uint64_t ntiles) {
    __shared__ uint8_t s_part[1024];
    const uint64_t R = (ntiles + 1023) / 1024;
    const uint64_t b0 = min((uint64_t)threadIdx.x * R, ntiles), b1 = min(b0 + R, ntiles);
    uint32_t acc = SEG_ID;
    for (uint64_t b = b0; b < b1; b++) {  // bound: R
        const uint32_t s = sum[b];
        if (s != SEG_ID) acc = s;
    }
    s_part[threadIdx.x] = (uint8_t)acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = SEG_FRESH;
        for (int i = 0; i < 1024; i++) {
            const uint32_t s = s_part[i];
            s_part[i] = (uint8_t)run;
            if (s != SEG_ID) run = s;
        }
    }
    __syncthreads();
    uint32_t run = s_part[threadIdx.x];
    for (uint64_t b = b0; b < b1; b++) {  // bound: R
        const uint32_t s = sum[b];
        sum[b] = (uint8_t)run;
        if (s != SEG_ID) run = s;
    }
}

// Launch 3, a tile per workgroup, a wave per 64 consecutive positions: the state in front of every position, and from it
// the two scan inputs.  Inside a wave two ballots (who sets FRESH or OPEN, who sets OPEN) and a count of leading zeros
// below the lane; across the four waves of a round their summaries in LDS; across rounds a running state; across tiles
// the byte k_seg_carry left.
__global__ void __launch_bounds__(SEG_THREADS)
k_seg_mark(const SegArgs A) {
    __shared__ uint32_t s_ws[SEG_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t ntiles = (A.p1 - A.p0 + A.tile - 1) / A.tile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // bound: ntiles / gridDim.x + 1
        const unsigned long long base = A.p0 + t * A.tile, end = min(base + (unsigned long long)A.tile, A.p1);
        uint32_t run = A.sum[t];  // FRESH or OPEN, the same in every lane
        for (uint32_t r = 0; r < A.tile; r += SEG_THREADS) {  // bound: tile / 256 + 1 (the same count in every lane)
            const unsigned long long p = base + r + tid;
            const bool valid = p < end;
            const uint32_t f = valid ? A.flag[p] : (uint32_t)(SEG_CLS_SKIP << 1);  // (past the end: no event)
            const uint32_t ev = seg_event(f);
            const unsigned long long any = __ballot(ev != SEG_ID), open = __ballot(ev == SEG_OPEN);
            if (lane == 0) s_ws[wave] = seg_last(any, open);
            __syncthreads();
            uint32_t cin = run;  // the state in front of this wave
#pragma unroll
            for (uint32_t w = 0; w < SEG_THREADS / 64; w++) {
                const uint32_t s = s_ws[w];
                if (w < wave && s != SEG_ID) cin = s;
                if (s != SEG_ID) run = s;
            }
            if (valid) {
                uint32_t st = seg_last(any & ((1ull << lane) - 1ull), open);
                if (st == SEG_ID) st = cin;
                if (f & SEG_F_DOC) st = SEG_FRESH;
                const uint32_t content = ((f >> 1) & SEG_CLS_SKIP) ? 0u : 1u;
                const uint32_t start = content & (st == SEG_FRESH ? 1u : 0u);
                A.len_s[p] = start;
                A.len_o[p] = content + (start & A.tag);
            }
            __syncthreads();  // (s_ws is free for the next round)
        }
    }
}

struct SegPlaceArgs {
    const void *ids;
    void *out;
    const unsigned long long *off;   // n_docs + 1 checked offsets
    unsigned long long n_docs, p0, p1, n_out, n_seg;
    uint32_t tag;
    const uint32_t *len_o, *len_s;
    const unsigned long long *oo, *so;  // their exclusive scans, [n] each
    unsigned long long *seg_offsets;    // n_seg + 1 words
    long long *seg_doc, *src_start, *src_end;  // n_seg words each, each may be NULL
};

// Placement, one position per thread: a content id goes to out[oo[p]] (one further with a tag in front).  A position that
// starts segment s = so[p] also writes seg_offsets[s], and -- the one search of this call, per SEGMENT, log2(n_docs + 1)
// steps -- finds its document d = the last one with off[d] <= p, which no empty document is: seg_doc[s] = d, the tag,
// src_start[s] = off[d] if s is the document's first segment (so[off[d]] == s) and p otherwise, in which case p also
// closes the range of the segment in front: src_end[s - 1] = p.  The ranges that a document's end closes are
// k_seg_ends'.  Every index is below its total, which the caller's capacities hold: e < n_out, s < n_seg.
template <typename T>
__global__ void __launch_bounds__(256)
k_seg_place(const SegPlaceArgs A) {
    const T *const ids = (const T *)A.ids;
    T *const out = (T *)A.out;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) A.seg_offsets[A.n_seg] = A.n_out;
    for (uint64_t p = A.p0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < A.p1; p += stride) {  // bound: (p1 - p0) / stride + 1
        const uint32_t lo = A.len_o[p];
        if (!lo) continue;
        unsigned long long e = A.oo[p];
        if (A.len_s[p]) {
            const unsigned long long s = A.so[p];
            if (s >= A.n_seg || e >= A.n_out) continue;  // (never: the totals are the scans' own)
            A.seg_offsets[s] = e;
            if (A.tag || A.seg_doc || A.src_start || A.src_end) {
                unsigned long long a = 0, b = A.n_docs;  // the first entry of off[0 .. n_docs] beyond p lies in (a, b]: off[0] <= p < off[n_docs]
                while (b - a > 1) {  // bound: log2(n_docs) + 1
                    const unsigned long long mid = a + ((b - a) >> 1);
                    if (A.off[mid] > p) b = mid; else a = mid;
                }
                const unsigned long long d = a;
                const bool first = A.so[A.off[d]] == s;  // (off[d] <= p < n)
                if (A.seg_doc) A.seg_doc[s] = (long long)d;
                if (A.src_start) A.src_start[s] = (long long)(first ? A.off[d] : p);
                if (A.src_end && !first) A.src_end[s - 1] = (long long)p;  // (s > so[off[d]] >= 0)
                if (A.tag) out[e] = (T)d;
            }
            e += A.tag;
        }
        if (e < A.n_out) out[e] = ids[p];  // (always)
    }
}

// The ranges a document's end closes, one document per thread: the last segment of document d, if it has one, ends at
// off[d + 1].  seg(p) = the segments that start below p: so[p] inside the stream, n_seg at its end.
__global__ void __launch_bounds__(256)
k_seg_ends(const unsigned long long *__restrict__ off, uint64_t n_docs, uint64_t n,
           const unsigned long long *__restrict__ so, unsigned long long n_seg, long long *__restrict__ src_end) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n_docs; d += stride) {  // bound: n_docs / stride + 1
        const unsigned long long q0 = off[d], q1 = off[d + 1];
        const unsigned long long s0 = q0 < n ? so[q0] : n_seg, s1 = q1 < n ? so[q1] : n_seg;
        if (s1 > s0 && s1 <= n_seg) src_end[s1 - 1] = (long long)q1;
    }
}

// ---------------------------------------------------------------------------
// marks: ranges [start[s], end[s]) of s < n_seg + a value per range -> marks[p] = val[s] inside range s, 0 elsewhere.

// Entry s is bad if start[s] < 0, end[s] < start[s], end[s] > n, or start[s] < end[s - 1]: the lowest one to *bad.
__global__ void __launch_bounds__(256)
k_segmarks_check(const long long *__restrict__ start, const long long *__restrict__ end, uint64_t n_seg, uint64_t n,
                 unsigned long long *bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_seg; s += stride) {  // bound: n_seg / stride + 1
        const long long a = start[s], b = end[s];
        if (a < 0 || b < a || (unsigned long long)b > n || (s > 0 && a < end[s - 1])) atomicMin(bad, (unsigned long long)s);
    }
}

struct SegMarksArgs {
    const long long *start, *end;  // checked: 0 <= start[s] <= end[s] <= start[s + 1], end <= n < 2^32
    const uint8_t *val;
    unsigned long long n_seg, n;
    uint32_t tile, stage;
    uint8_t *marks;
};

// The fill, laid out by the positions, a tile per workgroup, four consecutive positions per lane.  The range that can
// hold p is the first one with end > p (the ends ascend; an empty range holds nothing and is passed over).  One binary
// search per tile, over all ranges, finds that of the tile's first position; the next A.stage ranges are staged in LDS
// as 32-bit {start, end}, and a lane searches there once and walks on from position to position.  A tile that more
// ranges begin in than are staged (or A.stage == 0) searches global memory instead, position by position.
__global__ void __launch_bounds__(SEG_THREADS)
k_segmarks_fill(const SegMarksArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_rng[];  // [0]: 64-bit j_lo; then stage x {start, end}
    unsigned long long *const s_first = (unsigned long long *)s_rng;
    uint32_t *const s_se = s_rng + 4;
    const uint32_t tid = threadIdx.x;
    const uint64_t ntiles = (A.n + A.tile - 1) / A.tile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // bound: ntiles / gridDim.x + 1
        const unsigned long long g0 = t * A.tile, g1 = min(g0 + (unsigned long long)A.tile, A.n);
        __syncthreads();  // (the staging area of the tile before is free)
        if (tid == 0) {
            unsigned long long lo = 0, hi = A.n_seg;  // the first range with end > g0, n_seg without one
            while (lo < hi) {  // bound: log2(n_seg) + 1
                const unsigned long long mid = lo + ((hi - lo) >> 1);
                if ((unsigned long long)A.end[mid] > g0) hi = mid; else lo = mid + 1;
            }
            *s_first = lo;
        }
        __syncthreads();
        const unsigned long long j_lo = *s_first;
        const uint32_t cnt = (uint32_t)min((unsigned long long)A.stage, A.n_seg - j_lo);
        for (uint32_t k = tid; k < cnt; k += SEG_THREADS) {  // bound: stage / 256 + 1
            s_se[2 * k] = (uint32_t)A.start[j_lo + k];
            s_se[2 * k + 1] = (uint32_t)A.end[j_lo + k];
        }
        __syncthreads();
        // staged: every range that begins below g1 is in LDS -- all ranges are, or the last staged one begins at g1 or behind
        const bool staged = j_lo + cnt == A.n_seg || (cnt > 0 && (unsigned long long)s_se[2 * (cnt - 1)] >= g1);
        for (uint32_t r = tid * 4; r < A.tile; r += SEG_THREADS * 4) {  // bound: tile / 1024 + 1
            const unsigned long long p = g0 + r;
            if (p >= g1) break;
            const uint32_t m = (uint32_t)min(4ull, g1 - p);
            uint32_t v[4] = {0, 0, 0, 0};
            if (staged) {
                uint32_t lo = 0, hi = cnt;  // the first staged range with end > p
                while (lo < hi) {  // bound: log2(stage) + 1
                    const uint32_t mid = (lo + hi) >> 1;
                    if ((unsigned long long)s_se[2 * mid + 1] > p) hi = mid; else lo = mid + 1;
                }
                uint32_t s = lo;
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    if (k >= m) break;
                    while (s < cnt && (unsigned long long)s_se[2 * s + 1] <= p + k) s++;  // bound: cnt steps over the four positions
                    if (s < cnt && (unsigned long long)s_se[2 * s] <= p + k) v[k] = A.val[j_lo + s];
                }
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    if (k >= m) break;
                    unsigned long long lo = j_lo, hi = A.n_seg;  // the first range with end > p + k
                    while (lo < hi) {  // bound: log2(n_seg) + 1
                        const unsigned long long mid = lo + ((hi - lo) >> 1);
                        if ((unsigned long long)A.end[mid] > p + k) hi = mid; else lo = mid + 1;
                    }
                    if (lo < A.n_seg && (unsigned long long)A.start[lo] <= p + k) v[k] = A.val[lo];
                }
            }
            uint8_t *const dst = A.marks + p;
            if (m == 4 && ((uintptr_t)dst & 3) == 0) {
                *(uint32_t *)dst = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 4; k++)
                    if (k < m) dst[k] = (uint8_t)v[k];
            }
        }
    }
}

}  // namespace bpe
