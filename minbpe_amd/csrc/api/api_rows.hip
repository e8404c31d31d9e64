// api_rows.hip -- bpe_rows_resident.
// Part of bpe_api.hip, which includes the parts in order (one translation unit).

// ---------------------------------------------------------------------------
// resident training rows

// R of pack mode: rows of L elements every S stream positions over a stream of T (only the last row can be partial)
static inline uint64_t rows_count_pack(uint64_t T, uint64_t L, uint64_t S) {
    if (T == 0) return 0;
    if (T <= L) return 1;
    return 1 + (T - L + S - 1) / S;
}

// ids, offsets, rows and companions are the caller's device buffers; the ctx lends its counter words.  Host <-> device:
// the counters {first bad offset entry, off[0], off[n_docs]}, nothing else.
extern "C" int bpe_rows_resident(bpe_ctx *c, const int32_t *d_ids, uint64_t n, const uint64_t *d_doc_offsets,
                                 uint64_t n_docs, int32_t mode, uint32_t flags, uint64_t row_len, uint64_t stride,
                                 int32_t sep_id, int32_t pad_id, void *d_rows, int32_t row_width, uint64_t rows_cap,
                                 int32_t *d_doc_index, int32_t *d_pos, int32_t *d_lengths, uint64_t *n_rows,
                                 uint64_t *bad_doc) {
    if (!c || (!d_ids && n) || !d_doc_offsets) return fail(c, BPE_E_ARG, "bad arguments");
    if (n_rows) *n_rows = 0;
    if (bad_doc) *bad_doc = ~0ull;
    if (mode != BPE_ROWS_PACK && mode != BPE_ROWS_PER_DOC) return fail(c, BPE_E_ARG, "mode must be BPE_ROWS_PACK or BPE_ROWS_PER_DOC");
    if (flags & ~(BPE_ROWS_HAS_SEP | BPE_ROWS_TRUNC_LEFT | BPE_ROWS_PAD_LEFT)) return fail(c, BPE_E_ARG, "unknown flag in 0x%x", flags);
    if (row_len == 0) return fail(c, BPE_E_ARG, "row_len must be at least 1");
    if (row_width != 4 && row_width != 8) return fail(c, BPE_E_ARG, "row_width must be 4 (int32) or 8 (int64)");
    const bool pack = mode == BPE_ROWS_PACK;
    if (pack) {
        if (stride == 0 || stride > row_len) return fail(c, BPE_E_ARG, "stride must be 1..row_len in pack mode");
        if (flags & (BPE_ROWS_TRUNC_LEFT | BPE_ROWS_PAD_LEFT))
            return fail(c, BPE_E_ARG, "BPE_ROWS_TRUNC_LEFT / BPE_ROWS_PAD_LEFT belong to per-document mode");
        if (d_lengths) return fail(c, BPE_E_ARG, "d_lengths belongs to per-document mode");
    } else if (d_doc_index || d_pos) {
        return fail(c, BPE_E_ARG, "d_doc_index / d_pos belong to pack mode");
    }
    if (n >= (1ull << 32)) return fail(c, BPE_E_LIMIT, "%llu ids exceed 2^32-1", (unsigned long long)n);
    if ((d_doc_index || d_pos) && (n + n_docs >= (1ull << 31) || n_docs >= (1ull << 31)))
        return fail(c, BPE_E_LIMIT, "document index and position are int32: n + n_docs must stay below 2^31");
    if (n_docs >= (1ull << 48)) return fail(c, BPE_E_LIMIT, "%llu documents exceed 2^48-1", (unsigned long long)n_docs);
    HIPCHK(c, hipSetDevice(c->device));
    auto *w = &c->d_scratch->rows;
    HIPCHK(c, hipMemsetAsync(&w->bad, 0xFF, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_rows_check, dim3(grid_for(n_docs + 1, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                       (const unsigned long long *)d_doc_offsets, n_docs, n, &w->bad, w->ends);
    LAUNCHCHK(c, "k_rows_check");
    unsigned long long hb[3] = {0, 0, 0};  // {first bad entry, off[0], off[n_docs]}
    HIPCHK(c, hipMemcpyAsync(hb, w, sizeof hb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (hb[0] != ~0ull) {
        if (bad_doc) *bad_doc = hb[0];
        return fail(c, BPE_E_ARG, "doc_offsets[%llu]: offsets must ascend and stay <= n = %llu", hb[0], (unsigned long long)n);
    }
    // from here on the offsets are known to ascend inside [0, n]: the row kernels index ids by them without checks
    const bool has_sep = (flags & BPE_ROWS_HAS_SEP) != 0;
    const uint64_t T = (hb[2] - hb[1]) + (has_sep ? n_docs : 0);  // (n < 2^32 and n_docs < 2^48: no wrap)
    const uint64_t R = pack ? rows_count_pack(T, row_len, stride) : n_docs;
    if (n_rows) *n_rows = R;
    if (!d_rows || R == 0) return BPE_OK;  // only count (or nothing to write)
    if (rows_cap < R) return fail(c, BPE_E_CAP, "need %llu rows", (unsigned long long)R);
    if (R > (~0ull - 16) / row_len) return fail(c, BPE_E_LIMIT, "rows x row_len overflows");
    RowsArgs A;
    A.ids = d_ids;
    A.off = (const unsigned long long *)d_doc_offsets;
    A.n_docs = n_docs;
    A.off0 = hb[1];
    A.T = T;
    A.L = row_len;
    A.S = pack ? stride : row_len;
    A.E = R * row_len;
    A.sep = sep_id;
    A.pad = pad_id;
    A.has_sep = has_sep ? 1u : 0u;
    A.trunc_left = (flags & BPE_ROWS_TRUNC_LEFT) ? 1u : 0u;
    A.pad_left = (flags & BPE_ROWS_PAD_LEFT) ? 1u : 0u;
    A.rows = d_rows;
    A.doc_index = d_doc_index;
    A.pos = d_pos;
    A.lengths = d_lengths;
    A.tile = (uint32_t)c->rows_tile;
    A.stage = (uint32_t)c->rows_stage;
    const uint64_t ntiles = (A.E + 4 + A.tile - 1) / A.tile;  // (+ up to 3 elements of alignment)
    const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, (uint64_t)c->num_cus * 16)));
    if (pack) {
        const bool doc = has_sep || d_doc_index || d_pos;
        const size_t lds = doc ? 2 * sizeof(unsigned long long) + (((size_t)A.stage * sizeof(uint32_t) + 15) & ~(size_t)15) : 0;
        by_width(row_width, [&](auto t) {
            using T = decltype(t);
            if (doc) hipLaunchKernelGGL((k_rows_pack<T, true>), grid, dim3(ROWS_THREADS), lds, c->stream, A);
            else hipLaunchKernelGGL((k_rows_pack<T, false>), grid, dim3(ROWS_THREADS), lds, c->stream, A);
        });
        LAUNCHCHK(c, "k_rows_pack");
    } else {
        by_width(row_width, [&](auto t) {
            hipLaunchKernelGGL(k_rows_per_doc<decltype(t)>, grid, dim3(ROWS_THREADS), 0, c->stream, A);
        });
        LAUNCHCHK(c, "k_rows_per_doc");
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BPE_OK;
}
