// api_decode.hip -- bpe_decode_*.
// Part of bpe_api.hip, which includes the parts in order (one translation unit).

// ---------------------------------------------------------------------------
// decode (N4)

extern "C" int bpe_decode_set_vocab(bpe_ctx *c, const uint8_t *vocab_bytes, const uint64_t *vocab_offsets,
                                    int32_t V) {
    if (!c || V < 0 || !vocab_offsets) return fail(c, BPE_E_ARG, "bad arguments");
    if (vocab_offsets[0] != 0) return fail(c, BPE_E_ARG, "vocab_offsets[0] must be 0");
    for (int32_t i = 0; i < V; i++)
        if (vocab_offsets[i + 1] < vocab_offsets[i])
            return fail(c, BPE_E_ARG, "vocab_offsets must not decrease (entry %d)", i);
    const uint64_t nb = vocab_offsets[V];
    if (nb && !vocab_bytes) return fail(c, BPE_E_ARG, "vocab_bytes is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    c->dec_have_vocab = false;
    c->dec_have_result = false;
    c->dec_meta_valid = false;  // (bpe_token_spans_resident makes the entries' UTF-8 meta anew, on the device)
    TRY(grow(c, c->cap_dec_blob, nb + 16, c->d_dec_blob));
    TRY(grow(c, c->cap_dec_voff, (uint64_t)V + 1, c->d_dec_voff));
    if (nb) HIPCHK(c, hipMemcpyAsync(c->d_dec_blob, vocab_bytes, nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_dec_voff, vocab_offsets, ((size_t)V + 1) * sizeof(uint64_t),
                             hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // caller may free its buffers on return
    c->dec_V = (uint32_t)V;
    c->dec_V_dense = (uint32_t)V;  // (no sparse ids until bpe_decode_set_sparse)
    c->dec_n_sparse = 0;
    c->dec_have_vocab = true;
    return BPE_OK;
}

extern "C" int bpe_decode_set_sparse(bpe_ctx *c, const int32_t *sparse_ids, int32_t n_sparse, int32_t V_dense) {
    if (!c || n_sparse < 0 || V_dense < 0 || (!sparse_ids && n_sparse)) return fail(c, BPE_E_ARG, "bad arguments");
    if (!c->dec_have_vocab) return fail(c, BPE_E_STATE, "bpe_decode_set_vocab first");
    if ((uint64_t)V_dense + (uint64_t)n_sparse != c->dec_V)
        return fail(c, BPE_E_ARG, "V_dense + n_sparse = %lld, the vocab table has %u entries",
                    (long long)V_dense + n_sparse, c->dec_V);
    for (int32_t j = 0; j < n_sparse; j++) {
        if (sparse_ids[j] >= 0 && sparse_ids[j] < V_dense)
            return fail(c, BPE_E_ARG, "sparse_ids[%d] = %d lies inside [0, V_dense)", j, sparse_ids[j]);
        if (j && sparse_ids[j] <= sparse_ids[j - 1])
            return fail(c, BPE_E_ARG, "sparse_ids must ascend strictly (entry %d)", j);
    }
    HIPCHK(c, hipSetDevice(c->device));
    if ((uint64_t)n_sparse > c->cap_dec_sparse) {
        c->dec_V_dense = c->dec_V;  // (nothing half set if the allocation fails)
        c->dec_n_sparse = 0;
        TRY(grow(c, c->cap_dec_sparse, (uint64_t)n_sparse, c->d_dec_sparse));
    }
    if (n_sparse) {
        HIPCHK(c, hipMemcpyAsync(c->d_dec_sparse, sparse_ids, (size_t)n_sparse * sizeof(int32_t), hipMemcpyHostToDevice,
                                 c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // caller may free its buffer on return
    }
    c->dec_V_dense = (uint32_t)V_dense;
    c->dec_n_sparse = (uint32_t)n_sparse;
    return BPE_OK;
}

extern "C" int bpe_decode_batch(bpe_ctx *c, const int32_t *ids, uint64_t n, uint64_t *n_bytes,
                                uint64_t *bad_index) {
    if (!c || (!ids && n)) return fail(c, BPE_E_ARG, "bad arguments");
    if (!c->dec_have_vocab) return fail(c, BPE_E_STATE, "bpe_decode_set_vocab first");
    if (n_bytes) *n_bytes = 0;
    if (bad_index) *bad_index = ~0ull;
    c->dec_have_result = false;
    c->dec_n = n;
    c->dec_total = 0;
    if (n == 0) {
        c->dec_have_result = true;
        return BPE_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    TRY(ensure_dec_scratch(c, n));
    auto *w = &c->d_scratch->two_pass;
    HIPCHK(c, hipMemcpyAsync(c->d_dec_ids, ids, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(&w->bad, 0xFF, sizeof(unsigned long long), c->stream));
    TRY(prof_begin(c, BPE_PROF_DECODE, 4 * n));
    hipLaunchKernelGGL(k_decode_len, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                       c->d_dec_ids, n, c->d_dec_voff, c->dec_V, c->d_dec_len, &w->bad);
    LAUNCHCHK(c, "k_decode_len");
    TRY(scan_lengths(c, c->d_dec_len, n, c->d_dec_bsum, c->d_dec_off, &w->total));
    TRY(prof_end(c));
    unsigned long long hb[2] = {0, 0};  // {first bad position, total bytes}
    HIPCHK(c, hipMemcpyAsync(hb, &w->bad, sizeof hb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (hb[0] != ~0ull) {
        if (bad_index) *bad_index = hb[0];
        TRY(prof_drain(c));
        return fail(c, BPE_E_ARG, "invalid token id: %d (position %llu)", ids[hb[0]], hb[0]);
    }
    const uint64_t total = hb[1];
    TRY(grow(c, c->cap_dec_out, total + 16, c->d_dec_out));
    TRY(prof_begin(c, BPE_PROF_DECODE, total));
    hipLaunchKernelGGL(k_decode_copy, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                       c->d_dec_ids, n, c->d_dec_voff, c->dec_V, c->d_dec_blob, c->d_dec_off, c->d_dec_out);
    LAUNCHCHK(c, "k_decode_copy");
    TRY(prof_end(c));
    TRY(prof_drain(c));
    c->dec_total = total;
    c->dec_have_result = true;
    if (n_bytes) *n_bytes = total;
    return BPE_OK;
}

extern "C" int bpe_decode_read(bpe_ctx *c, uint8_t *out, uint64_t cap, const uint64_t *doc_token_offsets,
                               uint64_t k, uint64_t *doc_byte_offsets_out) {
    if (!c) return BPE_E_ARG;
    if (!c->dec_have_result) return fail(c, BPE_E_STATE, "bpe_decode_batch first");
    if (c->dec_total && (!out || cap < c->dec_total))
        return fail(c, BPE_E_CAP, "need %llu bytes", (unsigned long long)c->dec_total);
    if (k && (!doc_token_offsets || !doc_byte_offsets_out)) return fail(c, BPE_E_ARG, "offset arrays are NULL");
    for (uint64_t j = 0; j < k; j++)
        if (doc_token_offsets[j] > c->dec_n)
            return fail(c, BPE_E_ARG, "doc_token_offsets[%llu] is past the last token", (unsigned long long)j);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->dec_total)
        HIPCHK(c, hipMemcpyAsync(out, c->d_dec_out, c->dec_total, hipMemcpyDeviceToHost, c->stream));
    if (k) {
        if (c->dec_n == 0) {  // nothing was decoded: every offset is 0
            for (uint64_t j = 0; j < k; j++) doc_byte_offsets_out[j] = 0;
        } else {
            DevPtr<unsigned long long> t_idx, t_dst;
            TRY(dev_realloc(c, t_idx, k));
            TRY(dev_realloc(c, t_dst, k));
            HIPCHK(c, hipMemcpyAsync(t_idx, doc_token_offsets, k * 8, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_decode_doc_offsets, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, c->stream,
                               c->d_dec_off, c->dec_n, (unsigned long long)c->dec_total, t_idx, k,
                               t_dst, (unsigned long long *)nullptr);
            LAUNCHCHK(c, "k_decode_doc_offsets");
            HIPCHK(c, hipMemcpyAsync(doc_byte_offsets_out, t_dst, k * 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BPE_OK;
}

// Resident form: ids, document positions, bytes and byte offsets are the caller's device buffers; lengths, resolved table
// indices, offsets and block sums are the ctx's decode scratch (shared with bpe_decode_batch, whose pending result this
// call therefore drops).  Host <-> device: the counters {bad position, total, bad document entry}, nothing else.
extern "C" int bpe_decode_batch_resident(bpe_ctx *c, const void *d_ids, int32_t id_width, uint64_t n,
                                         const uint64_t *d_doc_token_offsets, uint64_t k, uint8_t *d_out,
                                         uint64_t out_cap, uint64_t *d_doc_byte_offsets, uint64_t *n_bytes,
                                         uint64_t *bad_index) {
    if (!c || (!d_ids && n)) return fail(c, BPE_E_ARG, "bad arguments");
    if (id_width != 4 && id_width != 8) return fail(c, BPE_E_ARG, "id_width must be 4 (int32) or 8 (int64)");
    if (k && (!d_doc_token_offsets || !d_doc_byte_offsets)) return fail(c, BPE_E_ARG, "offset arrays are NULL");
    if (!c->dec_have_vocab) return fail(c, BPE_E_STATE, "bpe_decode_set_vocab first");
    if (n_bytes) *n_bytes = 0;
    if (bad_index) *bad_index = ~0ull;
    HIPCHK(c, hipSetDevice(c->device));
    const TwoPassText txt = {"invalid token id at position %llu", "bytes", 0, 1};
    auto len = [&](unsigned long long *d_bad) -> int {  // also the table index of every id, into d_dec_ids
        by_width(id_width, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_decode_res_len<T>, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                               (const T *)d_ids, n, c->d_dec_voff, c->dec_V_dense, c->d_dec_sparse, c->dec_n_sparse,
                               (uint32_t *)c->d_dec_ids.get(), c->d_dec_len, d_bad);
        });
        LAUNCHCHK(c, "k_decode_res_len");
        return BPE_OK;
    };
    auto place = [&](uint64_t total) -> int {
        uint32_t *d_tidx = (uint32_t *)c->d_dec_ids.get();
        if (c->dec_copy) {
            const uint64_t ntiles = (n + (uint64_t)c->dec_tile - 1) / (uint64_t)c->dec_tile;
            const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, (uint64_t)c->num_cus * 64);
            hipLaunchKernelGGL(k_decode_copy_staged, dim3(grid), dim3(256), (size_t)c->dec_window, c->stream, d_tidx, n,
                               c->d_dec_voff, c->d_dec_blob, c->d_dec_off, (unsigned long long)total, d_out,
                               (uint32_t)c->dec_tile, (uint32_t)c->dec_window);
            LAUNCHCHK(c, "k_decode_copy_staged");
        } else {  // one token per lane over the resolved indices (every one is a table index: the check passes)
            hipLaunchKernelGGL(k_decode_copy, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                               (const int32_t *)d_tidx, n, c->d_dec_voff, c->dec_V, c->d_dec_blob, c->d_dec_off, d_out);
            LAUNCHCHK(c, "k_decode_copy");
        }
        return BPE_OK;
    };
    return resident_two_pass(c, id_width, n, d_doc_token_offsets, k, d_doc_byte_offsets, d_out, out_cap, n_bytes, bad_index,
                             txt, len, place);
}
