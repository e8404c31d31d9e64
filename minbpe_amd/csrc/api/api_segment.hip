// api_segment.hip -- bpe_segment_docs_resident, bpe_segment_marks_resident.
// Part of bpe_api.hip, which includes the parts in order (one translation unit).

// ---------------------------------------------------------------------------
// the segments of every document as a stream of its own

// ids, offsets, the class table and every output are the caller's device buffers.  Between them: the decode scratch
// (shared with bpe_decode_batch, whose pending result this call therefore drops) holds the output lengths, their scan
// and its block sums, and -- in the words of its ids -- the start flags; the seg scratch, a group of its own, holds the
// flag byte per position, the scan of the starts with its block sums and the summary byte per tile.
// Host <-> device: the counters {first bad offset entry, off[0], off[n_docs]} and {n_out, n_seg}, nothing else.
// The launches, in order on the ctx's stream: document starts -> flag bytes; classes and tile summaries; the scan of the
// summaries; the state in front of every position and the two lengths; the two scans; after the totals have come back
// and the capacities are known to hold them, the documents' segment offsets, the placement, the ranges' ends.
extern "C" int bpe_segment_docs_resident(bpe_ctx *c, const void *d_ids, int32_t id_width, uint64_t n,
                                         const uint64_t *d_doc_offsets, uint64_t n_docs, const uint8_t *d_class,
                                         uint64_t n_class, uint32_t flags, void *d_out, uint64_t out_cap,
                                         uint64_t *d_seg_offsets, uint64_t seg_cap, int64_t *d_seg_doc,
                                         int64_t *d_src_start, int64_t *d_src_end, uint64_t *d_doc_seg_offsets,
                                         uint64_t *n_out, uint64_t *n_seg, uint64_t *bad_doc) {
    if (n_out) *n_out = 0;
    if (n_seg) *n_seg = 0;
    if (bad_doc) *bad_doc = ~0ull;
    const bool fill = d_out && out_cap;  // (otherwise a count-only call)
    if (!c || (!d_ids && n) || !d_doc_offsets || (fill && !d_seg_offsets)) return fail(c, BPE_E_ARG, "bad arguments");
    if (id_width != 4 && id_width != 8) return fail(c, BPE_E_ARG, "id_width must be 4 (int32) or 8 (int64)");
    if (flags & ~BPE_SEG_TAG_DOC) return fail(c, BPE_E_ARG, "unknown flag in 0x%x", flags);
    if (((uintptr_t)d_ids | (uintptr_t)d_out) & (uintptr_t)(id_width - 1))
        return fail(c, BPE_E_ARG, "d_ids and d_out must be aligned to id_width");
    if (((uintptr_t)d_doc_offsets | (uintptr_t)d_seg_offsets | (uintptr_t)d_seg_doc | (uintptr_t)d_src_start |
         (uintptr_t)d_src_end | (uintptr_t)d_doc_seg_offsets) & 7)
        return fail(c, BPE_E_ARG, "d_doc_offsets, d_seg_offsets, d_doc_seg_offsets and the int64 columns must be 8-byte aligned");
    if (n >= (1ull << 32)) return fail(c, BPE_E_LIMIT, "%llu ids exceed 2^32-1", (unsigned long long)n);
    if (n_docs >= (1ull << 32) - 1) return fail(c, BPE_E_LIMIT, "%llu documents exceed 2^32-2", (unsigned long long)n_docs);
    if ((flags & BPE_SEG_TAG_DOC) && id_width == 4 && n_docs > (1ull << 31))
        return fail(c, BPE_E_LIMIT, "the numbers of %llu documents do not fit the int32 tags", (unsigned long long)n_docs);
    if (n_class > (1ull << 26)) return fail(c, BPE_E_LIMIT, "%llu classes exceed 2^26", (unsigned long long)n_class);
    if (fill && n) {  // (the two ranges in bytes, now that n is known to be a size an address space holds)
        const uintptr_t i0 = (uintptr_t)d_ids, i1 = i0 + (uintptr_t)n * (uintptr_t)id_width;
        const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + (uintptr_t)out_cap * (uintptr_t)id_width;
        if (o0 < i1 && i0 < o1) return fail(c, BPE_E_ARG, "d_out overlaps d_ids");
    }
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long ends[2] = {0, 0};
    TRY(check_doc_offsets(c, d_doc_offsets, n_docs, n, bad_doc, ends));
    // from here on the offsets are known to ascend inside [0, n]
    const uint64_t p0 = ends[0], p1 = ends[1];
    if (p1 == p0) {  // no position takes part (n == 0, n_docs == 0, empty documents only): no segment
        if (d_doc_seg_offsets)
            HIPCHK(c, hipMemsetAsync(d_doc_seg_offsets, 0, (size_t)(n_docs + 1) * sizeof(uint64_t), c->stream));
        if (fill) HIPCHK(c, hipMemsetAsync(d_seg_offsets, 0, sizeof(uint64_t), c->stream));  // seg_offsets[0] = n_out = 0
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BPE_OK;
    }
    c->dec_have_result = false;
    TRY(ensure_dec_scratch(c, n));
    TRY(grow_group(c->cap_seg_n, n, [&]() -> int {
        TRY(dev_realloc(c, c->d_seg_flag, (size_t)n));
        TRY(dev_realloc(c, c->d_seg_off, (size_t)n + 1));
        TRY(dev_realloc(c, c->d_seg_bsum, (size_t)scan_tiles(n) + 1));
        return dev_realloc(c, c->d_seg_sum, (size_t)(n / 64) + 2);  // (a tile is 64 positions or more)
    }));
    auto *w = &c->d_scratch->seg;
    uint32_t *const len_o = c->d_dec_len.get(), *const len_s = (uint32_t *)c->d_dec_ids.get();
    const uint32_t tag = (flags & BPE_SEG_TAG_DOC) ? 1u : 0u;
    SegArgs A = {};
    A.ids = d_ids;
    A.cls = (d_class && n_class) ? d_class : nullptr;
    A.n_class = A.cls ? n_class : 0;
    A.p0 = p0;
    A.p1 = p1;
    A.tile = (uint32_t)c->seg_tile;
    A.tag = tag;
    A.flag = c->d_seg_flag;
    A.sum = c->d_seg_sum;
    A.len_o = len_o;
    A.len_s = len_s;
    const uint64_t ntiles = (p1 - p0 + A.tile - 1) / A.tile;
    const dim3 tgrid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, (uint64_t)c->num_cus * 8)));
    TRY(prof_begin(c, BPE_PROF_DECODE, (uint64_t)id_width * (p1 - p0)));
    HIPCHK(c, hipMemsetAsync(c->d_seg_flag + p0, 0, (size_t)(p1 - p0), c->stream));
    // (the scans run over all n positions: the ids in front of the first and behind the last document count for nothing)
    if (p0) {
        HIPCHK(c, hipMemsetAsync(len_o, 0, (size_t)p0 * sizeof(uint32_t), c->stream));
        HIPCHK(c, hipMemsetAsync(len_s, 0, (size_t)p0 * sizeof(uint32_t), c->stream));
    }
    if (p1 < n) {
        HIPCHK(c, hipMemsetAsync(len_o + p1, 0, (size_t)(n - p1) * sizeof(uint32_t), c->stream));
        HIPCHK(c, hipMemsetAsync(len_s + p1, 0, (size_t)(n - p1) * sizeof(uint32_t), c->stream));
    }
    hipLaunchKernelGGL(k_seg_docstart, dim3(grid_for(n_docs, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                       (const unsigned long long *)d_doc_offsets, n_docs, p1, c->d_seg_flag.get());
    LAUNCHCHK(c, "k_seg_docstart");
    by_width(id_width, [&](auto t) {
        hipLaunchKernelGGL(k_seg_classify<decltype(t)>, tgrid, dim3(SEG_THREADS), 0, c->stream, A);
    });
    LAUNCHCHK(c, "k_seg_classify");
    // the carry across tiles is a launch of its own: every summary is written before any is read, and no workgroup waits
    hipLaunchKernelGGL(k_seg_carry, dim3(1), dim3(1024), 0, c->stream, c->d_seg_sum.get(), ntiles);
    LAUNCHCHK(c, "k_seg_carry");
    hipLaunchKernelGGL(k_seg_mark, tgrid, dim3(SEG_THREADS), 0, c->stream, A);
    LAUNCHCHK(c, "k_seg_mark");
    TRY(scan_lengths(c, len_o, n, c->d_dec_bsum, c->d_dec_off, &w->totals[0]));
    TRY(scan_lengths(c, len_s, n, c->d_seg_bsum, c->d_seg_off, &w->totals[1]));
    TRY(prof_end(c));
    unsigned long long hb[2] = {0, 0};  // {n_out, n_seg}
    HIPCHK(c, hipMemcpyAsync(hb, w->totals, sizeof hb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t total = hb[0], nseg = hb[1];
    if (n_out) *n_out = total;
    if (n_seg) *n_seg = nseg;
    if (d_doc_seg_offsets) {  // the scan of the starts at the documents' offsets (every one is <= n: bad = NULL)
        hipLaunchKernelGGL(k_decode_doc_offsets, dim3((unsigned)((n_docs + 1 + 255) / 256)), dim3(256), 0, c->stream,
                           (const unsigned long long *)c->d_seg_off.get(), n, (unsigned long long)nseg,
                           (const unsigned long long *)d_doc_offsets, n_docs + 1, (unsigned long long *)d_doc_seg_offsets,
                           (unsigned long long *)nullptr);
        LAUNCHCHK(c, "k_decode_doc_offsets");
    }
    if (!fill || out_cap < total || seg_cap < nseg) {
        TRY(prof_drain(c));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!fill) return BPE_OK;
        return fail(c, BPE_E_CAP, "need %llu ids and %llu segments", (unsigned long long)total, (unsigned long long)nseg);
    }
    SegPlaceArgs P = {};
    P.ids = d_ids;
    P.out = d_out;
    P.off = (const unsigned long long *)d_doc_offsets;
    P.n_docs = n_docs;
    P.p0 = p0;
    P.p1 = p1;
    P.n_out = total;
    P.n_seg = nseg;
    P.tag = tag;
    P.len_o = len_o;
    P.len_s = len_s;
    P.oo = c->d_dec_off;
    P.so = c->d_seg_off;
    P.seg_offsets = (unsigned long long *)d_seg_offsets;
    P.seg_doc = (long long *)d_seg_doc;
    P.src_start = (long long *)d_src_start;
    P.src_end = (long long *)d_src_end;
    TRY(prof_begin(c, BPE_PROF_DECODE, (uint64_t)id_width * (p1 - p0 + total)));
    by_width(id_width, [&](auto t) {
        hipLaunchKernelGGL(k_seg_place<decltype(t)>, dim3(grid_for(p1 - p0, 256, c->num_cus * 8)), dim3(256), 0, c->stream, P);
    });
    LAUNCHCHK(c, "k_seg_place");
    if (d_src_end && nseg) {
        hipLaunchKernelGGL(k_seg_ends, dim3(grid_for(n_docs, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                           (const unsigned long long *)d_doc_offsets, n_docs, n, (const unsigned long long *)c->d_seg_off.get(),
                           (unsigned long long)nseg, (long long *)d_src_end);
        LAUNCHCHK(c, "k_seg_ends");
    }
    TRY(prof_end(c));
    TRY(prof_drain(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BPE_OK;
}

// ---------------------------------------------------------------------------
// per-segment values back as marks over the positions

// The ranges, the values and the marks are the caller's device buffers; no scratch but the counter word.  Host <->
// device: the counter {first bad range}, nothing else.  A check of the ranges, then -- only after it has passed -- the
// fill of all n bytes.
extern "C" int bpe_segment_marks_resident(bpe_ctx *c, const int64_t *d_src_start, const int64_t *d_src_end, uint64_t n_seg,
                                          const uint8_t *d_seg_val, uint64_t n, uint8_t *d_marks, uint64_t *bad_seg) {
    if (bad_seg) *bad_seg = ~0ull;
    if (!c || (n_seg && (!d_src_start || !d_src_end || !d_seg_val)) || (n && !d_marks)) return fail(c, BPE_E_ARG, "bad arguments");
    if (((uintptr_t)d_src_start | (uintptr_t)d_src_end) & 7)
        return fail(c, BPE_E_ARG, "d_src_start and d_src_end must be 8-byte aligned");
    if (n >= (1ull << 32)) return fail(c, BPE_E_LIMIT, "%llu positions exceed 2^32-1", (unsigned long long)n);
    if (n_seg >= (1ull << 32)) return fail(c, BPE_E_LIMIT, "%llu segments exceed 2^32-1", (unsigned long long)n_seg);
    HIPCHK(c, hipSetDevice(c->device));
    auto *w = &c->d_scratch->seg;
    if (n_seg) {
        HIPCHK(c, hipMemsetAsync(&w->bad, 0xFF, sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL(k_segmarks_check, dim3(grid_for(n_seg, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                           (const long long *)d_src_start, (const long long *)d_src_end, n_seg, n, &w->bad);
        LAUNCHCHK(c, "k_segmarks_check");
        unsigned long long hb = 0;
        HIPCHK(c, hipMemcpyAsync(&hb, &w->bad, sizeof hb, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (hb != ~0ull) {  // nothing has been written to the marks
            if (bad_seg) *bad_seg = hb;
            return fail(c, BPE_E_ARG, "range %llu: ranges must ascend without overlap inside [0, n = %llu]", hb,
                        (unsigned long long)n);
        }
    }
    if (n == 0) return BPE_OK;
    if (n_seg == 0) {
        HIPCHK(c, hipMemsetAsync(d_marks, 0, (size_t)n, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BPE_OK;
    }
    SegMarksArgs M = {};
    M.start = (const long long *)d_src_start;
    M.end = (const long long *)d_src_end;
    M.val = d_seg_val;
    M.n_seg = n_seg;
    M.n = n;
    M.tile = (uint32_t)c->seg_tile;
    M.stage = (uint32_t)c->seg_stage;
    M.marks = d_marks;
    const uint64_t ntiles = (n + M.tile - 1) / M.tile;
    const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, (uint64_t)c->num_cus * 8)));
    const size_t lds = 16 + (size_t)M.stage * 2 * sizeof(uint32_t);
    TRY(prof_begin(c, BPE_PROF_DECODE, n));
    hipLaunchKernelGGL(k_segmarks_fill, grid, dim3(SEG_THREADS), lds, c->stream, M);
    LAUNCHCHK(c, "k_segmarks_fill");
    TRY(prof_end(c));
    TRY(prof_drain(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BPE_OK;
}
