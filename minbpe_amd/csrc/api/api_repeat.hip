// api_repeat.hip -- bpe_repeat_stats_resident.
// Part of bpe_api.hip, which includes the parts in order (one translation unit).

// ---------------------------------------------------------------------------
// repetition statistics: repeated n-grams inside each document

namespace {

// the table over `positions` stream positions: two slots each, so that every key owns twice as many as it has windows
uint64_t rp_slots_for(uint64_t positions) { return 2 * positions; }

// the launch of the insert and of the read pass (k_repeat.hip: k_rp_pass)
template <bool INSERT>
int rp_launch_pass(bpe_ctx *c, int32_t id_width, const RpArgs &A) {
    const uint64_t a = ((uintptr_t)A.ids & 15) / (uint64_t)id_width;  // the kernel's tiles count from the 16-byte boundary
    const uint64_t ntiles = (a + A.p1 + A.tile - 1) / A.tile - (a + A.p0) / A.tile;
    const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, (uint64_t)c->num_cus * 8)));
    by_width(id_width, [&](auto t) {
        hipLaunchKernelGGL((k_rp_pass<decltype(t), INSERT>), grid, dim3(RP_THREADS), 0, c->stream, A);
    });
    LAUNCHCHK(c, "k_rp_pass");
    return BPE_OK;
}

}  // namespace

// ids, offsets and every output are the caller's device buffers; between them the rp scratch of the ctx, two groups of
// its own that no other entry point touches: the table (RpSlot: 16 bytes per slot) with the
// repeat marks of a call that asks for none, and the per-document rows (repeats, covered, top: 16 bytes per document).
// Host <-> device: the counters {first bad offset entry, off[0], off[n_docs]} and {documents with a repeat}, nothing
// else.  The offsets are checked as bpe_rows_resident checks them; then the table and the rows are prefilled and the
// four passes run on the ctx's stream (k_repeat.hip).
extern "C" int bpe_repeat_stats_resident(bpe_ctx *c, const void *d_ids, int32_t id_width, uint64_t n,
                                         const uint64_t *d_doc_offsets, uint64_t n_docs, uint32_t ngram, uint64_t max_len,
                                         uint32_t flags, int64_t *d_length, int64_t *d_windows, int64_t *d_distinct,
                                         int64_t *d_covered, int64_t *d_top_count, int64_t *d_top_pos, uint8_t *d_marks,
                                         uint64_t *n_repeat_docs, uint64_t *bad_doc) {
    if (n_repeat_docs) *n_repeat_docs = 0;
    if (bad_doc) *bad_doc = ~0ull;
    const bool any_col = d_length || d_windows || d_distinct || d_covered || d_top_count || d_top_pos;
    if (!c || (!d_ids && n) || !d_doc_offsets) return fail(c, BPE_E_ARG, "bad arguments");
    if (n_docs && !any_col && !d_marks) return fail(c, BPE_E_ARG, "no output: give a column or d_marks");
    if (id_width != 4 && id_width != 8) return fail(c, BPE_E_ARG, "id_width must be 4 (int32) or 8 (int64)");
    if (ngram < 1 || ngram > RP_NGRAM_MAX) return fail(c, BPE_E_ARG, "ngram: 1..%u", RP_NGRAM_MAX);
    if (flags & ~BPE_SELECT_TAIL) return fail(c, BPE_E_ARG, "unknown flag in 0x%x", flags);
    if ((flags & BPE_SELECT_TAIL) && max_len == 0) return fail(c, BPE_E_ARG, "BPE_SELECT_TAIL needs max_len");
    if ((uintptr_t)d_ids & (uintptr_t)(id_width - 1)) return fail(c, BPE_E_ARG, "d_ids must be aligned to id_width");
    if (((uintptr_t)d_doc_offsets | (uintptr_t)d_length | (uintptr_t)d_windows | (uintptr_t)d_distinct | (uintptr_t)d_covered |
         (uintptr_t)d_top_count | (uintptr_t)d_top_pos) & 7)
        return fail(c, BPE_E_ARG, "d_doc_offsets and the int64 columns must be 8-byte aligned");
    // a slot holds a position in 32 bits with ~0u for "none", and document numbers are 32-bit words with ~0u for "none"
    if (n >= (1ull << 32)) return fail(c, BPE_E_LIMIT, "%llu ids exceed 2^32-1", (unsigned long long)n);
    if (n_docs >= (1ull << 32) - 1) return fail(c, BPE_E_LIMIT, "%llu documents exceed 2^32-2", (unsigned long long)n_docs);
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long ends[2] = {0, 0};
    TRY(check_doc_offsets(c, d_doc_offsets, n_docs, n, bad_doc, ends));
    // from here on the offsets are known to ascend inside [0, n]: every key lies inside the ids
    if (d_marks && n) HIPCHK(c, hipMemsetAsync(d_marks, 0, (size_t)n, c->stream));  // (every byte; the passes set the bits)
    if (n_docs == 0) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BPE_OK;
    }
    auto *w = &c->d_scratch->rp;
    const uint64_t p0 = ends[0], p1 = ends[1];
    const bool pass = p1 >= p0 + ngram;  // (otherwise no key holds a window: no repeat, nothing covered)
    const bool cover = pass && (d_covered || d_marks);
    HIPCHK(c, hipMemsetAsync(&w->repeat_docs, 0, sizeof(unsigned long long), c->stream));
    if (pass) {
        const uint64_t slots = rp_slots_for(p1 - p0);
        // (the marks of a call without d_marks live next to the table: the group grows by the positions, and the table
        // is sized for as many)
        TRY(grow_group(c->cap_rp_pos, n, [&]() -> int {
            TRY(dev_realloc(c, c->d_rp_tab, (size_t)rp_slots_for(n)));
            return dev_realloc(c, c->d_rp_marks, (size_t)n);
        }));
        TRY(grow_group(c->cap_rp_docs, n_docs, [&]() -> int {
            TRY(dev_realloc(c, c->d_rp_rep, (size_t)n_docs));
            TRY(dev_realloc(c, c->d_rp_cov, (size_t)n_docs));
            return dev_realloc(c, c->d_rp_top, (size_t)n_docs);
        }));
        // (the prefill under a kind of its own, so that a profile tells it from the passes over the stream)
        TRY(prof_begin(c, BPE_PROF_TABLE, 0));
        HIPCHK(c, hipMemsetAsync(c->d_rp_tab, 0xFF, slots * sizeof(RpSlot), c->stream));  // free, no lowest, count - 1
        HIPCHK(c, hipMemsetAsync(c->d_rp_rep, 0, n_docs * sizeof(uint32_t), c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_rp_cov, 0, n_docs * sizeof(uint32_t), c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_rp_top, 0, n_docs * sizeof(unsigned long long), c->stream));
        if (!d_marks) HIPCHK(c, hipMemsetAsync(c->d_rp_marks + p0, 0, (size_t)(p1 - p0), c->stream));
        TRY(prof_end(c));
        RpArgs A = {};
        A.ids = d_ids;
        A.off = (const unsigned long long *)d_doc_offsets;
        A.n_docs = n_docs;
        A.p0 = p0;
        A.p1 = p1;
        A.max_len = max_len;
        A.tail = (flags & BPE_SELECT_TAIL) ? 1u : 0u;
        A.tile = (uint32_t)c->rp_tile;
        A.ngram = ngram;
        A.hash_bits = (uint32_t)c->rp_hash_bits;
        A.tab = c->d_rp_tab;
        A.marks = d_marks ? d_marks : c->d_rp_marks.get();
        A.rep = c->d_rp_rep;
        A.cov = c->d_rp_cov;
        A.top = c->d_rp_top;
        A.write_cover = d_marks ? 1u : 0u;
        TRY(prof_begin(c, BPE_PROF_DECODE, (uint64_t)id_width * (p1 - p0)));
        TRY(rp_launch_pass<true>(c, id_width, A));
        TRY(prof_end(c));
        TRY(prof_begin(c, BPE_PROF_DECODE, (uint64_t)id_width * (p1 - p0)));
        TRY(rp_launch_pass<false>(c, id_width, A));
        TRY(prof_end(c));
        if (cover) {
            TRY(prof_begin(c, BPE_PROF_DECODE, p1 - p0));
            const uint64_t ntiles = (p1 + A.tile - 1) / A.tile - p0 / A.tile;
            hipLaunchKernelGGL(k_rp_cover, dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, (uint64_t)c->num_cus * 8))),
                               dim3(RP_THREADS), 0, c->stream, A);
            LAUNCHCHK(c, "k_rp_cover");
            TRY(prof_end(c));
        }
    }
    TRY(prof_begin(c, BPE_PROF_TABLE, 0));
    hipLaunchKernelGGL(k_rp_finish, dim3(grid_for(n_docs, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                       (const unsigned long long *)d_doc_offsets, n_docs, (unsigned long long)max_len,
                       (flags & BPE_SELECT_TAIL) ? 1u : 0u, ngram, pass ? c->d_rp_rep.get() : (const uint32_t *)nullptr,
                       cover ? c->d_rp_cov.get() : (const uint32_t *)nullptr,
                       pass ? c->d_rp_top.get() : (const unsigned long long *)nullptr, (long long *)d_length,
                       (long long *)d_windows, (long long *)d_distinct, (long long *)d_covered, (long long *)d_top_count,
                       (long long *)d_top_pos, &w->repeat_docs);
    LAUNCHCHK(c, "k_rp_finish");
    TRY(prof_end(c));
    unsigned long long nr = 0;
    HIPCHK(c, hipMemcpyAsync(&nr, &w->repeat_docs, sizeof nr, hipMemcpyDeviceToHost, c->stream));
    TRY(prof_drain(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_repeat_docs) *n_repeat_docs = nr;
    return BPE_OK;
}
