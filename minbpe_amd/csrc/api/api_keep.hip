// api_keep.hip -- bpe_keep_ids_resident.
// Part of bpe_api.hip, which includes the parts in order (one translation unit).

// ---------------------------------------------------------------------------
// cutting marked ids out of a stream

// ids, mask, offsets, the output and its offsets are the caller's device buffers; lengths, their scan and its block sums
// are the ctx's decode scratch (shared with bpe_decode_batch, whose pending result this call therefore drops); no
// other scratch is touched.  Host <-> device: the counters {first bad offset entry, off[0], off[n_docs]} and {total},
// nothing else.  The offsets are checked as bpe_rows_resident checks them, then resident_two_pass runs over the n
// positions: a length of 0 or 1 each, the scan, the gather of the documents' output offsets, the placement.
extern "C" int bpe_keep_ids_resident(bpe_ctx *c, const void *d_ids, int32_t id_width, uint64_t n,
                                     const uint64_t *d_doc_offsets, uint64_t n_docs, const uint8_t *d_mask, uint32_t bits,
                                     uint32_t flags, void *d_out, uint64_t out_cap, uint64_t *d_out_offsets,
                                     uint64_t *n_out, uint64_t *bad_doc) {
    if (n_out) *n_out = 0;
    if (bad_doc) *bad_doc = ~0ull;
    if (!c || (!d_ids && n) || (!d_mask && n) || !d_doc_offsets || !d_out_offsets) return fail(c, BPE_E_ARG, "bad arguments");
    if (id_width != 4 && id_width != 8) return fail(c, BPE_E_ARG, "id_width must be 4 (int32) or 8 (int64)");
    if (bits < 1 || bits > 255) return fail(c, BPE_E_ARG, "bits: 1..255");
    if (flags & ~BPE_KEEP_DROP) return fail(c, BPE_E_ARG, "unknown flag in 0x%x", flags);
    if (((uintptr_t)d_ids | (uintptr_t)d_out) & (uintptr_t)(id_width - 1))
        return fail(c, BPE_E_ARG, "d_ids and d_out must be aligned to id_width");
    if (((uintptr_t)d_doc_offsets | (uintptr_t)d_out_offsets) & 7)
        return fail(c, BPE_E_ARG, "d_doc_offsets and d_out_offsets must be 8-byte aligned");
    if (n >= (1ull << 32)) return fail(c, BPE_E_LIMIT, "%llu ids exceed 2^32-1", (unsigned long long)n);
    if (n_docs >= (1ull << 48)) return fail(c, BPE_E_LIMIT, "%llu documents exceed 2^48-1", (unsigned long long)n_docs);
    if (d_out && out_cap && n) {  // (the two ranges in bytes, now that n is known to be a size an address space holds)
        const uintptr_t i0 = (uintptr_t)d_ids, i1 = i0 + (uintptr_t)n * (uintptr_t)id_width;
        const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + (uintptr_t)out_cap * (uintptr_t)id_width;
        if (o0 < i1 && i0 < o1) return fail(c, BPE_E_ARG, "d_out overlaps d_ids");
    }
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long ends[2] = {0, 0};
    TRY(check_doc_offsets(c, d_doc_offsets, n_docs, n, bad_doc, ends));
    // from here on the offsets are known to ascend inside [0, n]
    const uint64_t p0 = ends[0], p1 = ends[1];
    const uint32_t drop = (flags & BPE_KEEP_DROP) ? 1u : 0u;
    const TwoPassText txt = {"position %llu", "ids", 13 + (uint64_t)id_width, (uint64_t)id_width};
    auto len = [&](unsigned long long *) -> int {  // (no position is refused)
        hipLaunchKernelGGL(k_keep_len, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream, d_mask, n, p0, p1, bits,
                           drop, c->d_dec_len.get());
        LAUNCHCHK(c, "k_keep_len");
        return BPE_OK;
    };
    auto place = [&](uint64_t total) -> int {
        if (p1 == p0) return BPE_OK;
        by_width(id_width, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_keep_place<T>, dim3(grid_for(p1 - p0, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                               (const T *)d_ids, p0, p1, (const uint32_t *)c->d_dec_len.get(),
                               (const unsigned long long *)c->d_dec_off.get(), (unsigned long long)total, (T *)d_out);
        });
        LAUNCHCHK(c, "k_keep_place");
        return BPE_OK;
    };
    // the documents' output offsets are the scan at their own offsets: out_offsets[d] = the kept positions below off[d]
    return resident_two_pass(c, id_width, n, d_doc_offsets, n_docs + 1, d_out_offsets, d_out, out_cap, n_out, nullptr, txt, len,
                             place);
}
