// api_resident.hip -- what the entry points over id streams that live in HBM share: the exclusive scan of a length
// column, the decode scratch's growth, the dispatch on an id width, and the two-pass driver of bpe_decode_batch_resident
// and bpe_project_resident.
// Part of bpe_api.hip, which includes the parts in order (one translation unit).

namespace {

// f(T{}) with T the integer type of `width` bytes (4 or 8: the callers have checked it), so that a launch names its
// kernel and its arguments once:  by_width(w, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(k<T>, ...); })
template <typename F>
inline void by_width(int32_t width, F &&f) {
    if (width == 4) f(int32_t{});
    else f(int64_t{});
}

// off[i] = len[0] + ... + len[i - 1] for i < n, *d_total = the sum of all n (n > 0); bsum: scan_tiles(n) + 1 words
int scan_lengths(bpe_ctx *c, const uint32_t *len, uint64_t n, unsigned long long *bsum, unsigned long long *off,
                 unsigned long long *d_total) {
    const uint64_t nb = scan_tiles(n);
    hipLaunchKernelGGL(k_scan_blocksum, dim3((unsigned)nb), dim3(256), 0, c->stream, len, n, bsum);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, c->stream, bsum, nb, d_total);
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(256), 0, c->stream, len, n, bsum, off);
    LAUNCHCHK(c, "k_scan_*");
    return BPE_OK;
}

// the decode scratch (ids / resolved indices, lengths, their scan and its block sums) holds n tokens
int ensure_dec_scratch(bpe_ctx *c, uint64_t n) {
    return grow_group(c->cap_dec_n, n, [&]() -> int {
        TRY(dev_realloc(c, c->d_dec_ids, (size_t)n));
        TRY(dev_realloc(c, c->d_dec_len, (size_t)n));
        TRY(dev_realloc(c, c->d_dec_off, (size_t)n + 1));
        return dev_realloc(c, c->d_dec_bsum, (size_t)scan_tiles(n) + 1);
    });
}

// The offsets of a document list, checked as bpe_rows_resident states them (k_rows_check, through the `rows` counter
// words): BPE_E_ARG with *bad_doc = the first entry that descends or lies beyond n.  ends (may be null): off[0] and
// off[n_docs] come to the host in the same transfer.  The stream is synchronised when it returns.
int check_doc_offsets(bpe_ctx *c, const uint64_t *d_doc_offsets, uint64_t n_docs, uint64_t n, uint64_t *bad_doc,
                      unsigned long long *ends) {
    auto *w = &c->d_scratch->rows;
    HIPCHK(c, hipMemsetAsync(&w->bad, 0xFF, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_rows_check, dim3(grid_for(n_docs + 1, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                       (const unsigned long long *)d_doc_offsets, n_docs, n, &w->bad, w->ends);
    LAUNCHCHK(c, "k_rows_check");
    unsigned long long hb[3] = {0, 0, 0};  // {first bad entry, off[0], off[n_docs]}
    HIPCHK(c, hipMemcpyAsync(hb, &w->bad, (ends ? 3 : 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (hb[0] != ~0ull) {
        if (bad_doc) *bad_doc = hb[0];
        return fail(c, BPE_E_ARG, "doc_offsets[%llu]: offsets must ascend and stay <= n = %llu", hb[0], (unsigned long long)n);
    }
    if (ends) ends[0] = hb[1], ends[1] = hb[2];
    return BPE_OK;
}

// what a user of resident_two_pass says besides its two launches
struct TwoPassText {
    const char *bad_fmt;  // the message of an id the length pass refused: one %llu, its position
    const char *unit;     // what the output is counted in ("need %llu <unit>")
    uint64_t place_in, place_out;  // bytes the placement moves per input id and per output element (profiling)
};

// The host side of "n ids in HBM -> a variable number of output elements per id, back to back in HBM": a length pass
// into c->d_dec_len, its scan into c->d_dec_off, then a placement by those offsets.  len(d_bad) launches the length pass
// (the first id it refuses goes to *d_bad by atomicMin) and place(total) the placement; both check their launch and
// return a code.  Everything else is here: scratch, counters, the n == 0 short cut, the read-back, the bad-id exit, the
// gather of the documents' output offsets and its check, the count-only and capacity exits, profiling, the last sync.
// *n_out holds the total from the moment it is known, whatever happens after; nothing is written to the caller's
// output before the last check has passed.
template <typename Len, typename Place>
int resident_two_pass(bpe_ctx *c, int32_t id_width, uint64_t n, const uint64_t *d_doc_token_offsets, uint64_t k,
                      uint64_t *d_doc_out_offsets, const void *d_out, uint64_t out_cap, uint64_t *n_out,
                      uint64_t *bad_index, const TwoPassText &txt, Len len, Place place) {
    c->dec_have_result = false;
    TRY(ensure_dec_scratch(c, n));
    auto *w = &c->d_scratch->two_pass;
    HIPCHK(c, hipMemsetAsync(&w->bad, 0xFF, 3 * sizeof(unsigned long long), c->stream));  // bad, total, docbad
    if (n == 0) {
        HIPCHK(c, hipMemsetAsync(&w->total, 0, sizeof(unsigned long long), c->stream));
    } else {
        TRY(prof_begin(c, BPE_PROF_DECODE, (uint64_t)id_width * n));
        TRY(len(&w->bad));
        TRY(scan_lengths(c, c->d_dec_len, n, c->d_dec_bsum, c->d_dec_off, &w->total));
        TRY(prof_end(c));
    }
    unsigned long long hb[3] = {0, 0, 0};  // {first bad position, total, first bad document entry}
    HIPCHK(c, hipMemcpyAsync(hb, &w->bad, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (hb[0] != ~0ull) {  // nothing has been written to the caller's buffers
        if (bad_index) *bad_index = hb[0];
        TRY(prof_drain(c));
        return fail(c, BPE_E_ARG, txt.bad_fmt, hb[0]);
    }
    const uint64_t total = hb[1];
    if (n_out) *n_out = total;
    if (k) {
        hipLaunchKernelGGL(k_decode_doc_offsets, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, c->stream, c->d_dec_off, n,
                           (unsigned long long)total, (const unsigned long long *)d_doc_token_offsets, k,
                           (unsigned long long *)d_doc_out_offsets, &w->docbad);
        LAUNCHCHK(c, "k_decode_doc_offsets");
        HIPCHK(c, hipMemcpyAsync(hb + 2, &w->docbad, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (hb[2] != ~0ull) {
            TRY(prof_drain(c));
            return fail(c, BPE_E_ARG, "doc_token_offsets[%llu] is past the last token", hb[2]);
        }
    }
    if (!d_out || out_cap == 0 || total == 0) {  // only count (or nothing to write)
        TRY(prof_drain(c));
        return BPE_OK;
    }
    if (out_cap < total) {
        TRY(prof_drain(c));
        return fail(c, BPE_E_CAP, "need %llu %s", (unsigned long long)total, txt.unit);
    }
    TRY(prof_begin(c, BPE_PROF_DECODE, txt.place_in * n + txt.place_out * total));
    TRY(place(total));
    TRY(prof_end(c));
    TRY(prof_drain(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BPE_OK;
}

}  // namespace
