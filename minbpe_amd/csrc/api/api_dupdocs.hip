// api_dupdocs.hip -- bpe_dup_docs_resident.
// Part of bpe_api.hip, which includes the parts in order (one translation unit).

// ---------------------------------------------------------------------------
// exact document de-duplication

// ids, offsets, first and counts are the caller's device buffers; everything between them is the dup scratch of the ctx,
// a group of its own: this call touches no other call's pending result -- not the decode scratch (unlike selection), not
// the decode, projection or count tables.  Host <-> device: the counters {first bad offset entry, off[0], off[n_docs]}
// and {groups}, nothing else.  The offsets are checked as bpe_rows_resident checks them; then init, hash pass, insert
// pass, finish pass on the ctx's stream (k_dupdocs.hip).
extern "C" int bpe_dup_docs_resident(bpe_ctx *c, const void *d_ids, int32_t id_width, uint64_t n,
                                     const uint64_t *d_doc_offsets, uint64_t n_docs, uint64_t max_len, uint32_t flags,
                                     int64_t *d_first, uint64_t *d_counts, uint64_t *n_distinct, uint64_t *bad_doc) {
    if (n_distinct) *n_distinct = 0;
    if (bad_doc) *bad_doc = ~0ull;
    if (!c || (!d_ids && n) || !d_doc_offsets || (!d_first && n_docs)) return fail(c, BPE_E_ARG, "bad arguments");
    if (id_width != 4 && id_width != 8) return fail(c, BPE_E_ARG, "id_width must be 4 (int32) or 8 (int64)");
    if (flags & ~BPE_SELECT_TAIL) return fail(c, BPE_E_ARG, "unknown flag in 0x%x", flags);
    if ((flags & BPE_SELECT_TAIL) && max_len == 0) return fail(c, BPE_E_ARG, "BPE_SELECT_TAIL needs max_len");
    if ((uintptr_t)d_ids & (uintptr_t)(id_width - 1)) return fail(c, BPE_E_ARG, "d_ids must be aligned to id_width");
    if (((uintptr_t)d_doc_offsets | (uintptr_t)d_first | (uintptr_t)d_counts) & 7)
        return fail(c, BPE_E_ARG, "d_doc_offsets, d_first and d_counts must be 8-byte aligned");
    // document numbers are 32-bit words with ~0u for "none", and so are the positions of a key
    if (n >= (1ull << 32)) return fail(c, BPE_E_LIMIT, "%llu ids exceed 2^32-1", (unsigned long long)n);
    if (n_docs >= (1ull << 32) - 1) return fail(c, BPE_E_LIMIT, "%llu documents exceed 2^32-2", (unsigned long long)n_docs);
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long ends[2] = {0, 0};
    TRY(check_doc_offsets(c, d_doc_offsets, n_docs, n, bad_doc, ends));
    if (n_docs == 0) return BPE_OK;
    // from here on the offsets are known to ascend inside [0, n]: every key lies inside the ids
    uint64_t slots = 2;
    while (slots < 2 * n_docs) slots <<= 1;
    TRY(grow_group(c->cap_dup_docs, n_docs, [&]() -> int {
        TRY(dev_realloc(c, c->d_dup_hash, (size_t)n_docs));
        TRY(dev_realloc(c, c->d_dup_rep, (size_t)n_docs));
        TRY(dev_realloc(c, c->d_dup_gmin, (size_t)n_docs));
        TRY(dev_realloc(c, c->d_dup_cnt, (size_t)n_docs));
        return dev_realloc(c, c->d_dup_tab, (size_t)slots);
    }));
    auto *w = &c->d_scratch->dup;
    const uint32_t tail = (flags & BPE_SELECT_TAIL) ? 1u : 0u;
    const uint64_t p0 = ends[0], p1 = ends[1];
    TRY(prof_begin(c, BPE_PROF_DECODE, (uint64_t)id_width * (p1 - p0)));
    HIPCHK(c, hipMemsetAsync(&w->distinct, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_dup_init, dim3(grid_for(slots, 256, c->num_cus * 8)), dim3(256), 0, c->stream, c->d_dup_hash.get(),
                       c->d_dup_gmin.get(), c->d_dup_cnt.get(), n_docs, c->d_dup_tab.get(), slots);
    LAUNCHCHK(c, "k_dup_init");
    if (p1 > p0) {  // (documents that are all empty keep the sum 0)
        DupHashArgs H;
        H.ids = d_ids;
        H.off = (const unsigned long long *)d_doc_offsets;
        H.n_docs = n_docs;
        H.p0 = p0;
        H.p1 = p1;
        H.max_len = max_len;
        H.tail = tail;
        H.tile = (uint32_t)c->dup_tile;
        H.hash = c->d_dup_hash;
        const uint64_t a = ((uintptr_t)d_ids & 15) / (uint64_t)id_width;  // the kernel's tiles count from the 16-byte boundary
        const uint64_t ntiles = (a + p1 + H.tile - 1) / H.tile - (a + p0) / H.tile;
        const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, (uint64_t)c->num_cus * 8)));
        by_width(id_width, [&](auto t) {
            hipLaunchKernelGGL(k_dup_hash<decltype(t)>, grid, dim3(DUP_THREADS), DUP_HASH_LDS, c->stream, H);
        });
        LAUNCHCHK(c, "k_dup_hash");
    }
    TRY(prof_end(c));
    // (the table's passes under a kind of their own, so that a profile tells them from the read of the stream)
    TRY(prof_begin(c, BPE_PROF_TABLE, 0));
    {
        DupInsArgs I;
        I.ids = d_ids;
        I.off = (const unsigned long long *)d_doc_offsets;
        I.n_docs = n_docs;
        I.max_len = max_len;
        I.tmask = slots - 1;
        I.tail = tail;
        I.wave_len = (uint32_t)c->dup_wave_len;
        I.hash_bits = (uint32_t)c->dup_hash_bits;
        I.hash = c->d_dup_hash;
        I.tab = c->d_dup_tab;
        I.rep = c->d_dup_rep;
        I.gmin = c->d_dup_gmin;
        I.cnt = c->d_dup_cnt;
        I.want_counts = d_counts ? 1u : 0u;
        const uint64_t chunks = (n_docs + 63) / 64;  // one wave takes 64 documents at a time
        const dim3 grid(grid_for(chunks, DUP_THREADS / 64, c->num_cus * 8));
        by_width(id_width, [&](auto t) {
            hipLaunchKernelGGL(k_dup_insert<decltype(t)>, grid, dim3(DUP_THREADS), 0, c->stream, I);
        });
        LAUNCHCHK(c, "k_dup_insert");
    }
    hipLaunchKernelGGL(k_dup_finish, dim3(grid_for(n_docs, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                       c->d_dup_rep.get(), c->d_dup_gmin.get(), c->d_dup_cnt.get(), n_docs, (long long *)d_first,
                       (unsigned long long *)d_counts, &w->distinct);
    LAUNCHCHK(c, "k_dup_finish");
    TRY(prof_end(c));
    unsigned long long nd = 0;
    HIPCHK(c, hipMemcpyAsync(&nd, &w->distinct, sizeof nd, hipMemcpyDeviceToHost, c->stream));
    TRY(prof_drain(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_distinct) *n_distinct = nd;
    return BPE_OK;
}
