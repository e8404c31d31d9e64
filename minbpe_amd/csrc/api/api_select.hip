// api_select.hip -- bpe_select_docs_resident.
// Part of bpe_api.hip, which includes the parts in order (one translation unit).

// ---------------------------------------------------------------------------
// document selection

// ids, offsets, index, the output and its offsets are the caller's device buffers; lengths, their scan, its block sums
// and the sources s_j are the ctx's decode scratch (shared with bpe_decode_batch, whose pending result this call
// therefore drops); the decode vocab table, the projection table and the count scratch are not touched.  Host <->
// device: the counters {first bad offset entry} and {first bad selection, total}, nothing else.
// The offsets are checked as bpe_rows_resident checks them, then resident_two_pass runs over the m selections: length
// pass, scan, placement.  It leaves the output offsets to its caller: they are copied out of the scratch here, after it
// has returned BPE_OK (a count-only call included) or BPE_E_CAP.
extern "C" int bpe_select_docs_resident(bpe_ctx *c, const void *d_ids, int32_t id_width, uint64_t n,
                                        const uint64_t *d_doc_offsets, uint64_t n_docs, const int64_t *d_index, uint64_t m,
                                        uint64_t max_len, uint32_t flags, void *d_out, uint64_t out_cap,
                                        uint64_t *d_out_offsets, uint64_t *n_out, uint64_t *bad_doc, uint64_t *bad_sel) {
    if (n_out) *n_out = 0;
    if (bad_doc) *bad_doc = ~0ull;
    if (bad_sel) *bad_sel = ~0ull;
    if (!c || (!d_ids && n) || (!d_index && m) || !d_doc_offsets || !d_out_offsets) return fail(c, BPE_E_ARG, "bad arguments");
    if (id_width != 4 && id_width != 8) return fail(c, BPE_E_ARG, "id_width must be 4 (int32) or 8 (int64)");
    if (flags & ~BPE_SELECT_TAIL) return fail(c, BPE_E_ARG, "unknown flag in 0x%x", flags);
    if ((flags & BPE_SELECT_TAIL) && max_len == 0) return fail(c, BPE_E_ARG, "BPE_SELECT_TAIL needs max_len");
    if (((uintptr_t)d_ids | (uintptr_t)d_out) & (uintptr_t)(id_width - 1))
        return fail(c, BPE_E_ARG, "d_ids and d_out must be aligned to id_width");
    if (((uintptr_t)d_doc_offsets | (uintptr_t)d_index | (uintptr_t)d_out_offsets) & 7)
        return fail(c, BPE_E_ARG, "d_doc_offsets, d_index and d_out_offsets must be 8-byte aligned");
    if (n >= (1ull << 32)) return fail(c, BPE_E_LIMIT, "%llu ids exceed 2^32-1", (unsigned long long)n);
    if (m >= (1ull << 32)) return fail(c, BPE_E_LIMIT, "%llu selections exceed 2^32-1", (unsigned long long)m);
    if (n_docs >= (1ull << 48)) return fail(c, BPE_E_LIMIT, "%llu documents exceed 2^48-1", (unsigned long long)n_docs);
    HIPCHK(c, hipSetDevice(c->device));
    TRY(check_doc_offsets(c, d_doc_offsets, n_docs, n, bad_doc, nullptr));
    // from here on the offsets are known to ascend inside [0, n]: every s_j, l_j of the length pass lies inside the ids
    const uint32_t tail = (flags & BPE_SELECT_TAIL) ? 1u : 0u;
    // (the scratch pointers are read inside the two launches: resident_two_pass has grown the scratch by then)
    const TwoPassText txt = {"index[%llu] names no document", "ids", 12, 2 * (uint64_t)id_width};
    auto len = [&](unsigned long long *d_bad) -> int {
        hipLaunchKernelGGL(k_seldocs_len, dim3(grid_for(m, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                           (const unsigned long long *)d_doc_offsets, n_docs, (const long long *)d_index, m,
                           (unsigned long long)max_len, tail, c->d_dec_len.get(), (uint32_t *)c->d_dec_ids.get(), d_bad);
        LAUNCHCHK(c, "k_seldocs_len");
        return BPE_OK;
    };
    auto place = [&](uint64_t total) -> int {
        // the scan left oo[0, m) in the scratch: oo[m] = total closes it for the searches
        HIPCHK(c, hipMemcpyAsync(c->d_dec_off + m, &c->d_scratch->two_pass.total, sizeof(unsigned long long),
                                 hipMemcpyDeviceToDevice, c->stream));
        SelArgs A;
        A.ids = d_ids;
        A.out = d_out;
        A.oo = c->d_dec_off;
        A.src = (const uint32_t *)c->d_dec_ids.get();
        A.m = m;
        A.total = total;
        A.tile = (uint32_t)c->sel_tile;
        A.stage = (uint32_t)c->sel_stage;
        const uint64_t ntiles = (total + 4 + A.tile - 1) / A.tile;  // (+ up to 3 elements of alignment)
        const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, (uint64_t)c->num_cus * 16)));
        const size_t lds = 2 * sizeof(unsigned long long) + (((size_t)A.stage * sizeof(uint32_t) + 15) & ~(size_t)15);
        by_width(id_width, [&](auto t) {
            hipLaunchKernelGGL(k_seldocs_place<decltype(t)>, grid, dim3(SEL_THREADS), lds, c->stream, A);
        });
        LAUNCHCHK(c, "k_seldocs_place");
        return BPE_OK;
    };
    const int rc = resident_two_pass(c, id_width, m, nullptr, 0, nullptr, d_out, out_cap, n_out, bad_sel, txt, len, place);
    if (rc != BPE_OK && rc != BPE_E_CAP) return rc;
    // the total is known and every index was good: the output offsets, whether or not the ids were written
    if (m)
        HIPCHK(c, hipMemcpyAsync(d_out_offsets, c->d_dec_off, (size_t)m * sizeof(unsigned long long), hipMemcpyDeviceToDevice,
                                 c->stream));
    HIPCHK(c, hipMemcpyAsync(d_out_offsets + m, &c->d_scratch->two_pass.total, sizeof(unsigned long long),
                             hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return rc;  // (BPE_E_CAP keeps the message resident_two_pass left)
}
