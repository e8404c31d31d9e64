// api_count.hip -- bpe_count_resident.
// Part of bpe_api.hip, which includes the parts in order (one translation unit).

// ---------------------------------------------------------------------------
// histogram of ids that live in HBM.  bpe_count_fold, the host half, is csrc/count_fold.cpp.

// ids and counts are the caller's device buffers.  The call counts into a scratch of its own (c->d_count_scr) and commits
// it to d_counts only after the host has read back that every id had a bin: one 8-byte transfer.  The merge list and the
// pass ids are those of bpe_project_set_merges; nothing else of the ctx is touched -- not the decode scratch, not a
// pending bpe_decode_batch result, not the decode or the projection table.
extern "C" int bpe_count_resident(bpe_ctx *c, const void *d_ids, int32_t id_width, uint64_t n, uint64_t *d_counts,
                                  uint64_t n_bins, int32_t accumulate, uint64_t *bad_index) {
    if (!c || (!d_ids && n) || !d_counts) return fail(c, BPE_E_ARG, "bad arguments");
    if (bad_index) *bad_index = ~0ull;
    if (id_width != 4 && id_width != 8) return fail(c, BPE_E_ARG, "id_width must be 4 (int32) or 8 (int64)");
    if (((uintptr_t)d_ids & (uintptr_t)(id_width - 1)) || ((uintptr_t)d_counts & 7))
        return fail(c, BPE_E_ARG, "d_ids must be aligned to id_width, d_counts to 8 bytes");
    if (c->proj_M < 0) return fail(c, BPE_E_STATE, "bpe_project_set_merges first");
    const uint32_t hi = 256u + (uint32_t)c->proj_M;
    const uint64_t B = (uint64_t)hi + c->proj_n_pass;
    if (n_bins != B) return fail(c, BPE_E_ARG, "n_bins is %llu, the layout has 256 + M + n_pass = %llu bins", (unsigned long long)n_bins,
                                 (unsigned long long)B);
    HIPCHK(c, hipSetDevice(c->device));
    TRY(grow(c, c->cap_count_scr, B, c->d_count_scr));
    auto *w = &c->d_scratch->hist;
    TRY(prof_begin(c, BPE_PROF_DECODE, (uint64_t)id_width * n));
    HIPCHK(c, hipMemsetAsync(c->d_count_scr, 0, B * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(&w->bad, 0xFF, sizeof(unsigned long long), c->stream));
    if (n) {
        const uint32_t L = std::min<uint32_t>(hi, (uint32_t)c->count_lds_bins);
        const size_t lds = (size_t)L * sizeof(uint32_t);
        const uint64_t epv = 16 / (uint64_t)id_width, slots = n / epv + 2;  // (at most: the ends may be partial slots)
        // two workgroups of 1024 lanes fill a CU's 32 waves when their tables fit its 160 KiB side by side
        const uint64_t per_cu = lds <= 80 * 1024 - 512 ? 2 : 1;
        const dim3 grid((unsigned)std::min<uint64_t>((uint64_t)c->num_cus * per_cu, (slots + COUNT_THREADS - 1) / COUNT_THREADS));
        const uint64_t period = (uint64_t)c->count_flush / epv;  // slots between flushes: >= 16
        by_width(id_width, [&](auto t) {
            using T = decltype(t);
            if (c->count_combine)
                hipLaunchKernelGGL((k_count<T, true>), grid, dim3(COUNT_THREADS), lds, c->stream, (const T *)d_ids, n, L, hi,
                                   c->d_proj_pass.get(), c->proj_n_pass, c->d_count_scr.get(), &w->bad, period);
            else
                hipLaunchKernelGGL((k_count<T, false>), grid, dim3(COUNT_THREADS), lds, c->stream, (const T *)d_ids, n, L, hi,
                                   c->d_proj_pass.get(), c->proj_n_pass, c->d_count_scr.get(), &w->bad, period);
        });
        LAUNCHCHK(c, "k_count");
    }
    TRY(prof_end(c));
    unsigned long long bad = ~0ull;
    if (n) {
        HIPCHK(c, hipMemcpyAsync(&bad, &w->bad, sizeof bad, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (bad != ~0ull) {  // nothing has been written to d_counts
        if (bad_index) *bad_index = bad;
        TRY(prof_drain(c));
        return fail(c, BPE_E_ARG, "token id at position %llu has no bin", bad);
    }
    if (n || !accumulate) {  // (no ids added to what is there: the array stays as it is)
        TRY(prof_begin(c, BPE_PROF_DECODE, 0));
        hipLaunchKernelGGL(k_count_commit, dim3(grid_for(B, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                           (unsigned long long *)d_counts, c->d_count_scr.get(), B, accumulate ? 1 : 0);
        LAUNCHCHK(c, "k_count_commit");
        TRY(prof_end(c));
    }
    TRY(prof_drain(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BPE_OK;
}
