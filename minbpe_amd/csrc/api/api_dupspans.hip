// api_dupspans.hip -- bpe_dup_spans_resident.
// Part of bpe_api.hip, which includes the parts in order (one translation unit).

// ---------------------------------------------------------------------------
// span de-duplication: windows an earlier document already holds

namespace {

// the table over `positions` stream positions: more than twice as many slots as they can hold windows
uint64_t ds_slots_for(uint64_t positions) { return 2 * positions + 1; }

// the launch of the build and of the query (k_dupspans.hip: k_ds_pass)
template <bool BUILD>
int ds_launch_pass(bpe_ctx *c, int32_t id_width, const DsArgs &A) {
    const uint64_t a = ((uintptr_t)A.ids & 15) / (uint64_t)id_width;  // the kernel's tiles count from the 16-byte boundary
    const uint64_t ntiles = (a + A.p1 + A.tile - 1) / A.tile - (a + A.p0) / A.tile;
    const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, (uint64_t)c->num_cus * 8)));
    by_width(id_width, [&](auto t) {
        hipLaunchKernelGGL((k_ds_pass<decltype(t), BUILD>), grid, dim3(DS_THREADS), 0, c->stream, A);
    });
    LAUNCHCHK(c, "k_ds_pass");
    return BPE_OK;
}

}  // namespace

// ids, offsets and every output are the caller's device buffers; between them the ds scratch of the ctx, two groups of
// its own that no other entry point touches: the table (DsSlot: 16 bytes per slot) with the marks of a call that asks
// for none, and the per-document rows (seen, covered, first << 32 | low: 16 bytes per document).
// Host <-> device: the counters {first bad offset entry, off[0], off[n_docs]} and {windows, distinct windows, lost
// windows, documents with a seen window}, nothing else.  The offsets are checked as bpe_rows_resident checks them; then
// the table and the rows are prefilled and the four passes run on the ctx's stream (k_dupspans.hip, k_repeat.hip's
// cover pass).
extern "C" int bpe_dup_spans_resident(bpe_ctx *c, const void *d_ids, int32_t id_width, uint64_t n,
                                      const uint64_t *d_doc_offsets, uint64_t n_docs, uint32_t ngram, uint64_t max_len,
                                      uint32_t flags, int64_t *d_length, int64_t *d_windows, int64_t *d_seen,
                                      int64_t *d_covered, int64_t *d_first, int64_t *d_src_pos, uint8_t *d_marks,
                                      uint64_t *n_docs_seen, uint64_t *n_windows, uint64_t *n_distinct, uint64_t *bad_doc) {
    if (n_docs_seen) *n_docs_seen = 0;
    if (n_windows) *n_windows = 0;
    if (n_distinct) *n_distinct = 0;
    if (bad_doc) *bad_doc = ~0ull;
    const bool any_col = d_length || d_windows || d_seen || d_covered || d_first || d_src_pos;
    if (!c || (!d_ids && n) || !d_doc_offsets) return fail(c, BPE_E_ARG, "bad arguments");
    if (n_docs && !any_col && !d_marks) return fail(c, BPE_E_ARG, "no output: give a column or d_marks");
    if (id_width != 4 && id_width != 8) return fail(c, BPE_E_ARG, "id_width must be 4 (int32) or 8 (int64)");
    if (ngram < 1 || ngram > DS_NGRAM_MAX) return fail(c, BPE_E_ARG, "ngram: 1..%u", DS_NGRAM_MAX);
    if (flags & ~(BPE_SELECT_TAIL | BPE_SPANS_ANYWHERE)) return fail(c, BPE_E_ARG, "unknown flag in 0x%x", flags);
    if ((flags & BPE_SELECT_TAIL) && max_len == 0) return fail(c, BPE_E_ARG, "BPE_SELECT_TAIL needs max_len");
    if ((uintptr_t)d_ids & (uintptr_t)(id_width - 1)) return fail(c, BPE_E_ARG, "d_ids must be aligned to id_width");
    if (((uintptr_t)d_doc_offsets | (uintptr_t)d_length | (uintptr_t)d_windows | (uintptr_t)d_seen | (uintptr_t)d_covered |
         (uintptr_t)d_first | (uintptr_t)d_src_pos) & 7)
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
    auto *w = &c->d_scratch->ds;
    const uint64_t p0 = ends[0], p1 = ends[1];
    const uint32_t tail = (flags & BPE_SELECT_TAIL) ? 1u : 0u;
    const bool pass = p1 >= p0 + ngram;  // (otherwise no key holds a window: nothing seen, nothing covered)
    const bool cover = pass && (d_covered || d_marks);
    HIPCHK(c, hipMemsetAsync(w->counts, 0, 4 * sizeof(unsigned long long), c->stream));  // counts[3] and seen_docs
    if (pass) {
        const uint64_t slots = ds_slots_for(p1 - p0);
        // (the marks of a call without d_marks live next to the table: the group grows by the positions, and the table
        // is sized for as many)
        TRY(grow_group(c->cap_ds_pos, n, [&]() -> int {
            TRY(dev_realloc(c, c->d_ds_tab, (size_t)ds_slots_for(n)));
            return dev_realloc(c, c->d_ds_marks, (size_t)n);
        }));
        TRY(grow_group(c->cap_ds_docs, n_docs, [&]() -> int {
            TRY(dev_realloc(c, c->d_ds_seen, (size_t)n_docs));
            TRY(dev_realloc(c, c->d_ds_cov, (size_t)n_docs));
            return dev_realloc(c, c->d_ds_min, (size_t)n_docs);
        }));
        // (the prefill under a kind of its own, so that a profile tells it from the passes over the stream)
        TRY(prof_begin(c, BPE_PROF_TABLE, 0));
        HIPCHK(c, hipMemsetAsync(c->d_ds_tab, 0xFF, slots * sizeof(DsSlot), c->stream));  // free, no lowest
        HIPCHK(c, hipMemsetAsync(c->d_ds_seen, 0, n_docs * sizeof(uint32_t), c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_ds_cov, 0, n_docs * sizeof(uint32_t), c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_ds_min, 0xFF, n_docs * sizeof(unsigned long long), c->stream));  // NG_EMPTY
        if (!d_marks) HIPCHK(c, hipMemsetAsync(c->d_ds_marks + p0, 0, (size_t)(p1 - p0), c->stream));
        TRY(prof_end(c));
        DsArgs A = {};
        A.ids = d_ids;
        A.off = (const unsigned long long *)d_doc_offsets;
        A.n_docs = n_docs;
        A.p0 = p0;
        A.p1 = p1;
        A.max_len = max_len;
        A.tail = tail;
        A.tile = (uint32_t)c->ds_tile;
        A.ngram = ngram;
        A.hash_bits = (uint32_t)c->ds_hash_bits;
        A.anywhere = (flags & BPE_SPANS_ANYWHERE) ? 1u : 0u;
        A.tab = c->d_ds_tab;
        A.slots = slots;
        A.marks = d_marks ? d_marks : c->d_ds_marks.get();
        A.seen = c->d_ds_seen;
        A.fmin = c->d_ds_min;
        A.counters = w->counts;
        TRY(prof_begin(c, BPE_PROF_DECODE, (uint64_t)id_width * (p1 - p0)));
        TRY(ds_launch_pass<true>(c, id_width, A));
        TRY(prof_end(c));
        TRY(prof_begin(c, BPE_PROF_DECODE, (uint64_t)id_width * (p1 - p0)));
        TRY(ds_launch_pass<false>(c, id_width, A));
        TRY(prof_end(c));
        if (cover) {
            // bit 0 of these marks is what bit 0 is to k_rp_cover: that kernel over this call's arrays, as it stands
            RpArgs R = {};
            R.off = A.off;
            R.n_docs = n_docs;
            R.p0 = p0;
            R.p1 = p1;
            R.max_len = max_len;
            R.tail = tail;
            R.tile = A.tile;
            R.ngram = ngram;
            R.marks = A.marks;
            R.cov = c->d_ds_cov;
            R.write_cover = d_marks ? 1u : 0u;
            TRY(prof_begin(c, BPE_PROF_DECODE, p1 - p0));
            const uint64_t ntiles = (p1 + R.tile - 1) / R.tile - p0 / R.tile;
            hipLaunchKernelGGL(k_rp_cover, dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, (uint64_t)c->num_cus * 8))),
                               dim3(RP_THREADS), 0, c->stream, R);
            LAUNCHCHK(c, "k_rp_cover");
            TRY(prof_end(c));
        }
    }
    TRY(prof_begin(c, BPE_PROF_TABLE, 0));
    hipLaunchKernelGGL(k_ds_finish, dim3(grid_for(n_docs, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                       (const unsigned long long *)d_doc_offsets, n_docs, (unsigned long long)max_len, tail, ngram,
                       pass ? c->d_ds_seen.get() : (const uint32_t *)nullptr,
                       cover ? c->d_ds_cov.get() : (const uint32_t *)nullptr,
                       pass ? c->d_ds_min.get() : (const unsigned long long *)nullptr, (long long *)d_length,
                       (long long *)d_windows, (long long *)d_seen, (long long *)d_covered, (long long *)d_first,
                       (long long *)d_src_pos, &w->seen_docs);
    LAUNCHCHK(c, "k_ds_finish");
    TRY(prof_end(c));
    unsigned long long hb[4] = {0, 0, 0, 0};  // {windows, distinct windows, lost windows, documents with a seen window}
    HIPCHK(c, hipMemcpyAsync(hb, w->counts, sizeof hb, hipMemcpyDeviceToHost, c->stream));
    TRY(prof_drain(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (hb[2]) return fail(c, BPE_E_INTERNAL, "%llu windows were not found in the table of their own build", hb[2]);
    if (n_docs_seen) *n_docs_seen = hb[3];
    if (n_windows) *n_windows = hb[0];
    if (n_distinct) *n_distinct = hb[1];
    return BPE_OK;
}
