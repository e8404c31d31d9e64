// api_project.hip -- bpe_project_set_merges, bpe_project_resident.
// Part of bpe_api.hip, which includes the parts in order (one translation unit).

// ---------------------------------------------------------------------------
// projection onto a smaller vocabulary

extern "C" int bpe_project_set_merges(bpe_ctx *c, const int32_t *merges, int32_t M, const int32_t *pass_ids,
                                      int32_t n_pass) {
    if (!c || M < 0 || n_pass < 0 || (!merges && M) || (!pass_ids && n_pass)) return fail(c, BPE_E_ARG, "bad arguments");
    if (!merges_training_shape(merges, M))
        return fail(c, BPE_E_ARG, "the merge list does not have the shape training makes (0 <= a, b < 256 + r, no pair twice)");
    for (int32_t j = 0; j < n_pass; j++) {
        if (pass_ids[j] >= 0 && (int64_t)pass_ids[j] < 256 + (int64_t)M)
            return fail(c, BPE_E_ARG, "pass_ids[%d] = %d lies inside [0, 256 + M)", j, pass_ids[j]);
        if (j && pass_ids[j] <= pass_ids[j - 1]) return fail(c, BPE_E_ARG, "pass_ids must ascend strictly (entry %d)", j);
    }
    HIPCHK(c, hipSetDevice(c->device));
    c->proj_M = -1;  // (nothing half set if a step below fails)
    c->proj_vs = -1;
    TRY(grow(c, c->cap_proj_pass, (uint64_t)n_pass, c->d_proj_pass));
    if (n_pass) {
        HIPCHK(c, hipMemcpyAsync(c->d_proj_pass, pass_ids, (size_t)n_pass * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // caller may free its buffer on return
    }
    c->proj_merges.assign(merges, merges + 2 * (size_t)M);  // the tables are made from the host copy, one per vocab_size asked for
    c->proj_n_pass = (uint32_t)n_pass;
    c->proj_M = M;
    return BPE_OK;
}

namespace {
// most ids the expansions of one vocab_size may hold (1 GiB of int32; a 100k vocabulary at vocab_size 256 needs < 2^20).
// The cap also keeps every single expansion below 2^31 ids: the offsets are 32-bit
constexpr uint64_t PROJ_TABLE_CAP = 1ull << 28;

// The table of vocab_size vs, made on the host from the merge list: lengths first -- the limits are decided from them
// alone --, then the expansions, each the concatenation of its children's (a child below vs is itself).  O(table).
int project_table_host(bpe_ctx *c, int32_t vs, std::vector<uint32_t> &toff, std::vector<int32_t> &tab, uint64_t *maxlen) {
    const int32_t hi = 256 + c->proj_M, E = hi - vs;
    const int32_t *mg = c->proj_merges.data();
    toff.assign((size_t)E + 1, 0u);
    uint64_t sum = 0, mx = 1;
    for (int32_t e = 0; e < E; e++) {
        uint64_t L = 0;
        for (int s = 0; s < 2; s++) {
            const int32_t x = mg[2 * (size_t)(vs - 256 + e) + s];
            L += x < vs ? 1u : toff[(size_t)(x - vs) + 1] - toff[(size_t)(x - vs)];
        }
        sum += L;  // (L <= 2 PROJ_TABLE_CAP: the children's lengths come out of a table within the cap)
        if (sum > PROJ_TABLE_CAP)
            return fail(c, BPE_E_LIMIT, "the expansions at vocab_size %d hold more than 2^28 ids (id %d alone: %llu)", vs, vs + e,
                        (unsigned long long)L);
        toff[(size_t)e + 1] = (uint32_t)sum;
        mx = std::max(mx, L);
    }
    tab.resize((size_t)sum);
    for (int32_t e = 0; e < E; e++) {
        int32_t *dst = tab.data() + toff[e];
        for (int s = 0; s < 2; s++) {
            const int32_t x = mg[2 * (size_t)(vs - 256 + e) + s];
            if (x < vs) {
                *dst++ = x;
            } else {
                const uint32_t b = toff[(size_t)(x - vs)], L = toff[(size_t)(x - vs) + 1] - b;
                memcpy(dst, tab.data() + b, (size_t)L * sizeof(int32_t));
                dst += L;
            }
        }
    }
    *maxlen = mx;
    return BPE_OK;
}
}  // namespace

// ids, offsets and the output are the caller's device buffers; lengths, their scan and its block sums are the ctx's decode
// scratch (shared with bpe_decode_batch, whose pending result this call therefore drops); the decode vocab table is not
// touched.  Host <-> device: the counters {bad position, total, bad document entry}; the table of a vocab_size once.
extern "C" int bpe_project_resident(bpe_ctx *c, const void *d_ids, int32_t id_width, uint64_t n, int32_t vocab_size,
                                    const uint64_t *d_doc_token_offsets, uint64_t k, void *d_out, uint64_t out_cap,
                                    uint64_t *d_doc_out_offsets, uint64_t *n_out, uint64_t *bad_index) {
    if (!c || (!d_ids && n)) return fail(c, BPE_E_ARG, "bad arguments");
    if (n_out) *n_out = 0;
    if (bad_index) *bad_index = ~0ull;
    if (id_width != 4 && id_width != 8) return fail(c, BPE_E_ARG, "id_width must be 4 (int32) or 8 (int64)");
    if (k && (!d_doc_token_offsets || !d_doc_out_offsets)) return fail(c, BPE_E_ARG, "offset arrays are NULL");
    if (((uintptr_t)d_ids | (uintptr_t)d_out) & (uintptr_t)(id_width - 1))
        return fail(c, BPE_E_ARG, "d_ids and d_out must be aligned to id_width");
    if (c->proj_M < 0) return fail(c, BPE_E_STATE, "bpe_project_set_merges first");
    if (vocab_size < 256 || (int64_t)vocab_size > 256 + (int64_t)c->proj_M)
        return fail(c, BPE_E_ARG, "vocab_size %d outside [256, %lld]", vocab_size, 256 + (long long)c->proj_M);
    // ---- the limits, from the merge list alone: before any device work
    std::vector<uint32_t> toff;
    std::vector<int32_t> tab;
    const bool fresh = c->proj_vs != (int64_t)vocab_size;
    uint64_t maxlen = c->proj_maxlen;
    if (fresh) TRY(project_table_host(c, vocab_size, toff, tab, &maxlen));
    if (n && maxlen > (1ull << 62) / n) return fail(c, BPE_E_LIMIT, "%llu ids may expand to 2^62 ids or more", (unsigned long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    if (fresh) {  // once per vocab_size: a second call at the same size builds and uploads nothing
        c->proj_vs = -1;
        TRY(grow(c, c->cap_proj_tab, tab.size(), c->d_proj_tab));
        TRY(grow(c, c->cap_proj_toff, toff.size(), c->d_proj_toff));
        if (!tab.empty())
            HIPCHK(c, hipMemcpyAsync(c->d_proj_tab, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_proj_toff, toff.data(), toff.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (the host vectors go away with this call)
        c->proj_vs = vocab_size;
        c->proj_maxlen = maxlen;
    }
    const uint32_t vs = (uint32_t)vocab_size, hi = 256u + (uint32_t)c->proj_M;
    const TwoPassText txt = {"token id at position %llu does not project", "ids", (uint64_t)id_width, (uint64_t)id_width};
    auto len = [&](unsigned long long *d_bad) -> int {
        by_width(id_width, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_project_len<T>, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                               (const T *)d_ids, n, vs, hi, c->d_proj_toff, c->d_proj_pass, c->proj_n_pass, c->d_dec_len, d_bad);
        });
        LAUNCHCHK(c, "k_project_len");
        return BPE_OK;
    };
    auto place = [&](uint64_t total) -> int {
        const uint32_t tile = (uint32_t)c->proj_tile, W = (uint32_t)c->proj_window;
        const uint64_t group = (uint64_t)PROJ_GROUP * tile, ngroups = (n + group - 1) / group;  // a workgroup takes PROJ_GROUP tiles at a time
        const dim3 grid((unsigned)std::min<uint64_t>(ngroups, (uint64_t)c->num_cus * 32));
        by_width(id_width, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_project_place<T>, grid, dim3(256), proj_lds_bytes(W), c->stream, (const T *)d_ids, n, vs, hi,
                               c->d_proj_toff, c->d_proj_tab, c->d_dec_off, (unsigned long long)total, (T *)d_out, tile, W);
        });
        LAUNCHCHK(c, "k_project_place");
        return BPE_OK;
    };
    return resident_two_pass(c, id_width, n, d_doc_token_offsets, k, d_doc_out_offsets, d_out, out_cap, n_out, bad_index, txt,
                             len, place);
}
