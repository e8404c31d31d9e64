// api_spans.hip -- bpe_token_spans_resident.
// Part of bpe_api.hip, which includes the parts in order (one translation unit).

// ---------------------------------------------------------------------------
// resident token spans

// leads | cont << 31 of every table entry, computed on the device from the blob bpe_decode_set_vocab uploaded: by the
// first spans call after it, never on the host
static int spans_meta(bpe_ctx *c) {
    if (c->dec_meta_valid) return BPE_OK;
    TRY(grow(c, c->cap_dec_meta, c->dec_V, c->d_dec_meta));
    if (c->dec_V) {
        unsigned long long *d_limit = &c->d_scratch->count;
        HIPCHK(c, hipMemsetAsync(d_limit, 0, sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL(k_spans_meta, dim3(grid_for(c->dec_V, 4, c->num_cus * 8)), dim3(256), 0, c->stream, c->d_dec_blob,
                           c->d_dec_voff, c->dec_V, c->d_dec_meta, d_limit);
        LAUNCHCHK(c, "k_spans_meta");
        unsigned long long limit = 0;
        HIPCHK(c, hipMemcpyAsync(&limit, d_limit, sizeof limit, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (limit) return fail(c, BPE_E_LIMIT, "a vocab entry holds 2^31 characters or more");
    }
    c->dec_meta_valid = true;
    return BPE_OK;
}

// ids, offsets and spans are the caller's device buffers; lengths, leads, the two scans and the documents' bases are the
// ctx's decode scratch (shared with bpe_decode_batch, whose pending result this call therefore drops) and its like.
// Host <-> device: the counters {bad position, total bytes, total leads, bad offset entry, off[0], off[n_docs]}.
extern "C" int bpe_token_spans_resident(bpe_ctx *c, const void *d_ids, int32_t id_width, uint64_t n,
                                        const uint64_t *d_doc_offsets, uint64_t n_docs, int64_t *d_byte_spans,
                                        int64_t *d_char_spans, uint64_t *n_bytes, uint64_t *n_chars, uint64_t *bad_index,
                                        uint64_t *bad_doc) {
    if (!c || (!d_ids && n)) return fail(c, BPE_E_ARG, "bad arguments");
    if (n_bytes) *n_bytes = 0;
    if (n_chars) *n_chars = 0;
    if (bad_index) *bad_index = ~0ull;
    if (bad_doc) *bad_doc = ~0ull;
    if (id_width != 4 && id_width != 8) return fail(c, BPE_E_ARG, "id_width must be 4 (int32) or 8 (int64)");
    if (!d_doc_offsets && n_docs) return fail(c, BPE_E_ARG, "d_doc_offsets is NULL");
    if (((uintptr_t)d_byte_spans | (uintptr_t)d_char_spans) & 7) return fail(c, BPE_E_ARG, "span arrays must be 8-byte aligned");
    if (n_docs >= (1ull << 32)) return fail(c, BPE_E_LIMIT, "%llu documents exceed 2^32-1", (unsigned long long)n_docs);
    if (n >= (1ull << 43)) return fail(c, BPE_E_LIMIT, "%llu ids exceed 2^43-1", (unsigned long long)n);
    if (!c->dec_have_vocab) return fail(c, BPE_E_STATE, "bpe_decode_set_vocab first");
    HIPCHK(c, hipSetDevice(c->device));
    c->dec_have_result = false;
    TRY(spans_meta(c));
    const bool docs = d_doc_offsets != nullptr;
    const uint64_t nb = scan_tiles(n);
    TRY(ensure_dec_scratch(c, n));
    TRY(grow_group(c->cap_spn_n, n, [&]() -> int {
        TRY(dev_realloc(c, c->d_spn_off, (size_t)n + 1));
        return dev_realloc(c, c->d_spn_bsum, (size_t)nb + 1);
    }));
    if (docs)
        TRY(grow_group(c->cap_spn_docs, n_docs + 1, [&]() -> int { return dev_realloc(c, c->d_spn_base, 2 * ((size_t)n_docs + 1)); }));
    // {first bad position, total bytes, total leads, first bad offset entry, off[0], off[n_docs]}
    auto *w = &c->d_scratch->spans;
    unsigned long long *d_bad = &w->bad, *d_totals = w->totals, *d_docbad = &w->docbad, *d_ends = w->ends;
    uint32_t *d_len = c->d_dec_len, *d_lw = (uint32_t *)c->d_dec_ids.get();
    HIPCHK(c, hipMemsetAsync(d_bad, 0xFF, 4 * sizeof(unsigned long long), c->stream));  // bad, totals, docbad
    if (docs) {
        hipLaunchKernelGGL(k_rows_check, dim3(grid_for(n_docs + 1, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                           (const unsigned long long *)d_doc_offsets, n_docs, n, d_docbad, d_ends);
        LAUNCHCHK(c, "k_rows_check");
    }
    if (n == 0) {  // (no launch that indexes an empty buffer)
        HIPCHK(c, hipMemsetAsync(d_totals, 0, 2 * sizeof(unsigned long long), c->stream));
    } else {
        TRY(prof_begin(c, BPE_PROF_DECODE, (uint64_t)id_width * n));
        const dim3 grid(grid_for(n, 256, c->num_cus * 8));
        by_width(id_width, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_spans_len<T>, grid, dim3(256), 0, c->stream, (const T *)d_ids, n, c->d_dec_voff,
                               c->d_dec_meta, c->dec_V_dense, c->d_dec_sparse, c->dec_n_sparse, d_len, d_lw, d_bad);
        });
        LAUNCHCHK(c, "k_spans_len");
        hipLaunchKernelGGL(k_spans_blocksum, dim3((unsigned)nb), dim3(256), 0, c->stream, d_len, d_lw, n, c->d_dec_bsum,
                           c->d_spn_bsum);
        hipLaunchKernelGGL(k_spans_scan_top, dim3(2), dim3(1024), 0, c->stream, c->d_dec_bsum, c->d_spn_bsum, nb, d_totals);
        hipLaunchKernelGGL(k_spans_scan_apply, dim3((unsigned)nb), dim3(256), 0, c->stream, d_len, d_lw, n, c->d_dec_bsum,
                           c->d_spn_bsum, c->d_dec_off, c->d_spn_off);
        LAUNCHCHK(c, "k_spans_scan_*");
        TRY(prof_end(c));
    }
    unsigned long long hb[6] = {0, 0, 0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(hb, w, sizeof hb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (hb[0] != ~0ull || hb[3] != ~0ull) {  // nothing has been written to the span arrays
        if (bad_index) *bad_index = hb[0];
        if (bad_doc) *bad_doc = hb[3];
        TRY(prof_drain(c));
        if (hb[0] != ~0ull) return fail(c, BPE_E_ARG, "invalid token id at position %llu", hb[0]);
        return fail(c, BPE_E_ARG, "doc_offsets[%llu]: offsets must ascend and stay <= n = %llu", hb[3], (unsigned long long)n);
    }
    if (n_bytes) *n_bytes = hb[1];
    if (n_chars) *n_chars = hb[2];
    if (n == 0 || (!d_byte_spans && !d_char_spans)) {  // only validate and count (or nothing to write)
        TRY(prof_drain(c));
        return BPE_OK;
    }
    // from here on the offsets are known to ascend inside [0, n]: the emit pass indexes by them without checks
    SpansArgs A;
    A.len = d_len;
    A.lw = d_lw;
    A.sb = c->d_dec_off;
    A.sc = c->d_spn_off;
    A.n = n;
    A.off = (const unsigned long long *)d_doc_offsets;
    A.n_docs = n_docs;
    A.off0 = docs ? hb[4] : 0;
    A.offn = docs ? hb[5] : n;
    A.base_b = c->d_spn_base;
    A.base_c = docs ? c->d_spn_base + (n_docs + 1) : nullptr;
    A.byte_spans = (long long *)d_byte_spans;
    A.char_spans = (long long *)d_char_spans;
    A.stage = (uint32_t)c->spans_stage;
    TRY(prof_begin(c, BPE_PROF_DECODE, 16 * n * ((d_byte_spans ? 1u : 0u) + (d_char_spans ? 1u : 0u))));
    const uint64_t ntiles = (n + SPANS_TILE - 1) / SPANS_TILE;
    const dim3 grid((unsigned)std::min<uint64_t>(ntiles, (uint64_t)c->num_cus * 16));
    if (docs) {
        // the documents' bases: one gather per channel at the n_docs + 1 offsets (position n: the total)
        const dim3 gg((unsigned)((n_docs + 1 + 255) / 256));
        hipLaunchKernelGGL(k_decode_doc_offsets, gg, dim3(256), 0, c->stream, c->d_dec_off, n, hb[1], A.off, n_docs + 1,
                           c->d_spn_base, (unsigned long long *)nullptr);
        hipLaunchKernelGGL(k_decode_doc_offsets, gg, dim3(256), 0, c->stream, c->d_spn_off, n, hb[2], A.off, n_docs + 1,
                           c->d_spn_base + (n_docs + 1), (unsigned long long *)nullptr);
        LAUNCHCHK(c, "k_decode_doc_offsets");
        const size_t lds = 2 * sizeof(unsigned long long) + (((size_t)A.stage * sizeof(uint32_t) + 15) & ~(size_t)15);
        hipLaunchKernelGGL(k_spans_emit<true>, grid, dim3(SPANS_THREADS), lds, c->stream, A);
    } else {
        hipLaunchKernelGGL(k_spans_emit<false>, grid, dim3(SPANS_THREADS), 0, c->stream, A);
    }
    LAUNCHCHK(c, "k_spans_emit");
    TRY(prof_end(c));
    TRY(prof_drain(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BPE_OK;
}
