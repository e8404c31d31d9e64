// api_ngram.hip -- bpe_ngram_index_resident, bpe_ngram_overlap_resident.
// Part of bpe_api.hip, which includes the parts in order (one translation unit).

// ---------------------------------------------------------------------------
// n-gram overlap with a reference set

namespace {

// the table of an index over `positions` reference positions: a power of two above twice as many slots as it can hold windows
uint64_t ng_slots_for(uint64_t positions) {
    uint64_t slots = 2;
    while (slots <= 2 * positions) slots <<= 1;
    return slots;
}

// the launch of the pass both calls share (k_ngram.hip: k_ng_pass)
template <bool BUILD>
int ng_launch_pass(bpe_ctx *c, int32_t id_width, const NgArgs &N) {
    const uint64_t a = ((uintptr_t)N.ids & 15) / (uint64_t)id_width;  // the kernel's tiles count from the 16-byte boundary
    const uint64_t ntiles = (a + N.p1 + N.tile - 1) / N.tile - (a + N.p0) / N.tile;
    const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, (uint64_t)c->num_cus * 8)));
    by_width(id_width, [&](auto t) {
        hipLaunchKernelGGL((k_ng_pass<decltype(t), BUILD>), grid, dim3(NG_THREADS), 0, c->stream, N);
    });
    LAUNCHCHK(c, "k_ng_pass");
    return BPE_OK;
}

}  // namespace

// ids and offsets are the caller's device buffers, free again when the call returns; the index is the ng scratch of the
// ctx, a group of its own that no other entry point touches: the reference at 64 bits, the table, the lowest position
// per slot.  Host <-> device: the counters {first bad offset entry, roff[0], roff[n_ref_docs]} and {windows, distinct
// windows}, nothing else.  A call that fails leaves the ctx without an index.
extern "C" int bpe_ngram_index_resident(bpe_ctx *c, const void *d_ref_ids, int32_t id_width, uint64_t n_ref,
                                        const uint64_t *d_ref_offsets, uint64_t n_ref_docs, uint32_t ngram,
                                        uint64_t *index_id, uint64_t *n_windows, uint64_t *n_distinct, uint64_t *bad_doc) {
    if (bad_doc) *bad_doc = ~0ull;
    if (c) c->ng_id = 0;
    if (!c || (!d_ref_ids && n_ref) || !d_ref_offsets || !index_id) return fail(c, BPE_E_ARG, "bad arguments");
    if (id_width != 4 && id_width != 8) return fail(c, BPE_E_ARG, "id_width must be 4 (int32) or 8 (int64)");
    if (ngram < 1 || ngram > NG_NGRAM_MAX) return fail(c, BPE_E_ARG, "ngram: 1..%u", NG_NGRAM_MAX);
    if ((uintptr_t)d_ref_ids & (uintptr_t)(id_width - 1)) return fail(c, BPE_E_ARG, "d_ref_ids must be aligned to id_width");
    if ((uintptr_t)d_ref_offsets & 7) return fail(c, BPE_E_ARG, "d_ref_offsets must be 8-byte aligned");
    // a slot holds a position in 32 bits with ~0u for "none", and the search for a document takes numbers below 2^32 - 1
    if (n_ref >= (1ull << 32)) return fail(c, BPE_E_LIMIT, "%llu ids exceed 2^32-1", (unsigned long long)n_ref);
    if (n_ref_docs >= (1ull << 32) - 1)
        return fail(c, BPE_E_LIMIT, "%llu documents exceed 2^32-2", (unsigned long long)n_ref_docs);
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long ends[2] = {0, 0};
    TRY(check_doc_offsets(c, d_ref_offsets, n_ref_docs, n_ref, bad_doc, ends));
    // from here on the offsets are known to ascend inside [0, n_ref]: every window lies inside the ids
    const uint64_t p0 = ends[0], p1 = ends[1];
    unsigned long long counts[2] = {0, 0};  // {windows, distinct windows}
    uint64_t slots = 0;
    if (n_ref_docs && p1 >= p0 + ngram) {  // (otherwise no document holds a window)
        slots = ng_slots_for(p1 - p0);
        TRY(grow_group(c->cap_ng_ref, n_ref, [&]() -> int {
            TRY(dev_realloc(c, c->d_ng_ref, (size_t)n_ref));
            TRY(dev_realloc(c, c->d_ng_tab, (size_t)ng_slots_for(n_ref)));
            return dev_realloc(c, c->d_ng_low, (size_t)ng_slots_for(n_ref));
        }));
        auto *w = &c->d_scratch->ng;
        TRY(prof_begin(c, BPE_PROF_DECODE, (uint64_t)(id_width + 8) * (p1 - p0)));
        by_width(id_width, [&](auto t) {
            hipLaunchKernelGGL(k_ng_widen<decltype(t)>, dim3(grid_for(p1 - p0, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                               (const decltype(t) *)d_ref_ids, p0, p1, c->d_ng_ref.get());
        });
        LAUNCHCHK(c, "k_ng_widen");
        TRY(prof_end(c));
        // (the table's passes under a kind of their own, so that a profile tells them from the read of the stream)
        TRY(prof_begin(c, BPE_PROF_TABLE, 0));
        HIPCHK(c, hipMemsetAsync(w->counts, 0, 2 * sizeof(unsigned long long), c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_ng_tab, 0xFF, slots * sizeof(unsigned long long), c->stream));  // NG_EMPTY
        HIPCHK(c, hipMemsetAsync(c->d_ng_low, 0xFF, slots * sizeof(uint32_t), c->stream));            // NG_NONE
        NgArgs N = {};
        N.ids = c->d_ng_ref;  // (the windows are hashed and compared at 64 bits: one template parameter for the corpus)
        N.off = (const unsigned long long *)d_ref_offsets;
        N.n_docs = n_ref_docs;
        N.p0 = p0;
        N.p1 = p1;
        N.tile = (uint32_t)c->ng_tile;
        N.ngram = ngram;
        N.hash_bits = (uint32_t)c->ng_hash_bits;
        N.ref = c->d_ng_ref;
        N.tab = c->d_ng_tab;
        N.low = c->d_ng_low;
        N.tmask = slots - 1;
        N.counters = w->counts;
        TRY(ng_launch_pass<true>(c, 8, N));
        TRY(prof_end(c));
        HIPCHK(c, hipMemcpyAsync(counts, w->counts, sizeof counts, hipMemcpyDeviceToHost, c->stream));
        TRY(prof_drain(c));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->ng_windows = counts[0];
    c->ng_slots = slots;
    c->ng_w = ngram;
    c->ng_bits = (uint32_t)c->ng_hash_bits;
    c->ng_id = ++c->ng_serial;
    *index_id = c->ng_id;
    if (n_windows) *n_windows = counts[0];
    if (n_distinct) *n_distinct = counts[1];
    return BPE_OK;
}

// ids, offsets and the four outputs are the caller's device buffers; between them the index and the per-document rows
// of the query (count, first << 32 | ref_pos), a group of their own.  Host <-> device: the counters {first bad offset
// entry, off[0], off[n_docs]} and {documents with a hit}, nothing else.  The offsets are checked as bpe_rows_resident
// checks them; then the rows are prefilled, the pass runs on the ctx's stream and the finish pass unpacks (k_ngram.hip).
extern "C" int bpe_ngram_overlap_resident(bpe_ctx *c, uint64_t index_id, const void *d_ids, int32_t id_width, uint64_t n,
                                          const uint64_t *d_doc_offsets, uint64_t n_docs, uint64_t max_len, uint32_t flags,
                                          int64_t *d_hits, int64_t *d_first, int64_t *d_ref_pos, uint8_t *d_starts,
                                          uint64_t *n_hit_docs, uint64_t *bad_doc) {
    if (n_hit_docs) *n_hit_docs = 0;
    if (bad_doc) *bad_doc = ~0ull;
    if (!c || (!d_ids && n) || !d_doc_offsets || (!d_hits && n_docs)) return fail(c, BPE_E_ARG, "bad arguments");
    if (id_width != 4 && id_width != 8) return fail(c, BPE_E_ARG, "id_width must be 4 (int32) or 8 (int64)");
    if (flags & ~BPE_SELECT_TAIL) return fail(c, BPE_E_ARG, "unknown flag in 0x%x", flags);
    if ((flags & BPE_SELECT_TAIL) && max_len == 0) return fail(c, BPE_E_ARG, "BPE_SELECT_TAIL needs max_len");
    if ((uintptr_t)d_ids & (uintptr_t)(id_width - 1)) return fail(c, BPE_E_ARG, "d_ids must be aligned to id_width");
    if (((uintptr_t)d_doc_offsets | (uintptr_t)d_hits | (uintptr_t)d_first | (uintptr_t)d_ref_pos) & 7)
        return fail(c, BPE_E_ARG, "d_doc_offsets, d_hits, d_first and d_ref_pos must be 8-byte aligned");
    // document numbers are 32-bit words with ~0u for "none", and a position of a document shares a word with one of the reference
    if (n >= (1ull << 32)) return fail(c, BPE_E_LIMIT, "%llu ids exceed 2^32-1", (unsigned long long)n);
    if (n_docs >= (1ull << 32) - 1) return fail(c, BPE_E_LIMIT, "%llu documents exceed 2^32-2", (unsigned long long)n_docs);
    if (index_id == 0 || index_id != c->ng_id)
        return fail(c, BPE_E_STATE, "index %llu is not the ctx's current n-gram index", (unsigned long long)index_id);
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long ends[2] = {0, 0};
    TRY(check_doc_offsets(c, d_doc_offsets, n_docs, n, bad_doc, ends));
    // from here on the offsets are known to ascend inside [0, n]: every key lies inside the ids
    if (d_starts && n) HIPCHK(c, hipMemsetAsync(d_starts, 0, (size_t)n, c->stream));  // (every byte; the pass sets the hits)
    if (n_docs == 0) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BPE_OK;
    }
    auto *w = &c->d_scratch->ng;
    const uint64_t p0 = ends[0], p1 = ends[1];
    const bool pass = c->ng_windows && p1 >= p0 + c->ng_w;  // (otherwise no hit: an empty index, or no key holds a window)
    HIPCHK(c, hipMemsetAsync(&w->hit_docs, 0, sizeof(unsigned long long), c->stream));
    if (pass) {
        TRY(grow_group(c->cap_ng_docs, n_docs, [&]() -> int {
            TRY(dev_realloc(c, c->d_ng_cnt, (size_t)n_docs));
            return dev_realloc(c, c->d_ng_min, (size_t)n_docs);
        }));
        // (the prefill under a kind of its own, so that a profile tells it from the pass over the stream)
        TRY(prof_begin(c, BPE_PROF_TABLE, 0));
        HIPCHK(c, hipMemsetAsync(c->d_ng_cnt, 0, n_docs * sizeof(uint32_t), c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_ng_min, 0xFF, n_docs * sizeof(unsigned long long), c->stream));  // NG_EMPTY
        TRY(prof_end(c));
        TRY(prof_begin(c, BPE_PROF_DECODE, (uint64_t)id_width * (p1 - p0) + (d_starts ? n : 0)));
        NgArgs N = {};
        N.ids = d_ids;
        N.off = (const unsigned long long *)d_doc_offsets;
        N.n_docs = n_docs;
        N.p0 = p0;
        N.p1 = p1;
        N.max_len = max_len;
        N.tail = (flags & BPE_SELECT_TAIL) ? 1u : 0u;
        N.tile = (uint32_t)c->ng_tile;
        N.ngram = c->ng_w;
        N.hash_bits = c->ng_bits;  // (the index's: where its windows were put)
        N.ref = c->d_ng_ref;
        N.tab = c->d_ng_tab;
        N.low = c->d_ng_low;
        N.tmask = c->ng_slots - 1;
        N.cnt = c->d_ng_cnt;
        N.fmin = c->d_ng_min;
        N.starts = d_starts;
        TRY(ng_launch_pass<false>(c, id_width, N));
        TRY(prof_end(c));
    }
    TRY(prof_begin(c, BPE_PROF_TABLE, 0));
    hipLaunchKernelGGL(k_ng_finish, dim3(grid_for(n_docs, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                       pass ? c->d_ng_cnt.get() : (const uint32_t *)nullptr, c->d_ng_min.get(), n_docs, (long long *)d_hits,
                       (long long *)d_first, (long long *)d_ref_pos, &w->hit_docs);
    LAUNCHCHK(c, "k_ng_finish");
    TRY(prof_end(c));
    unsigned long long nh = 0;
    HIPCHK(c, hipMemcpyAsync(&nh, &w->hit_docs, sizeof nh, hipMemcpyDeviceToHost, c->stream));
    TRY(prof_drain(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_hit_docs) *n_hit_docs = nh;
    return BPE_OK;
}
