// api_minhash.hip -- bpe_minhash_resident, bpe_minhash_agree_resident.
// Part of bpe_api.hip, which includes the parts in order (one translation unit).

// ---------------------------------------------------------------------------
// near-duplicate documents

namespace {

// A_p | 1 and B_p of every permutation from the seed: splitmix64, A first.  out: A_0 .. A_{P-1} | B_0 .. B_{P-1}
void mh_params(uint64_t seed, uint32_t P, std::vector<unsigned long long> &out) {
    out.resize(2 * (size_t)P);
    unsigned long long z = seed;
    auto next = [&]() {
        z += 0x9E3779B97F4A7C15ull;
        unsigned long long r = z;
        r = (r ^ (r >> 30)) * 0xBF58476D1CE4E5B9ull;
        r = (r ^ (r >> 27)) * 0x94D049BB133111EBull;
        return r ^ (r >> 31);
    };
    for (uint32_t p = 0; p < P; p++) {
        out[p] = next() | 1ull;
        out[(size_t)P + p] = next();
    }
}

}  // namespace

// ids, offsets and sig are the caller's device buffers; the scratch between them is the 16 P bytes of the permutations'
// parameters, made here from the seed and uploaded when seed or P change -- a group of its own: this call touches no
// other call's pending result.  Host <-> device: those parameters and the counters {first bad offset entry, off[0],
// off[n_docs]}, nothing else.  The offsets are checked as bpe_rows_resident checks them; then the prefill pass and the
// signature pass on the ctx's stream (k_minhash.hip).
extern "C" int bpe_minhash_resident(bpe_ctx *c, const void *d_ids, int32_t id_width, uint64_t n,
                                    const uint64_t *d_doc_offsets, uint64_t n_docs, uint64_t max_len, uint32_t flags,
                                    uint32_t ngram, uint32_t n_perm, uint64_t seed, int32_t *d_sig, uint64_t sig_cap,
                                    uint64_t *bad_doc) {
    if (bad_doc) *bad_doc = ~0ull;
    if (!c || (!d_ids && n) || !d_doc_offsets || (!d_sig && n_docs)) return fail(c, BPE_E_ARG, "bad arguments");
    if (id_width != 4 && id_width != 8) return fail(c, BPE_E_ARG, "id_width must be 4 (int32) or 8 (int64)");
    if (flags & ~BPE_SELECT_TAIL) return fail(c, BPE_E_ARG, "unknown flag in 0x%x", flags);
    if ((flags & BPE_SELECT_TAIL) && max_len == 0) return fail(c, BPE_E_ARG, "BPE_SELECT_TAIL needs max_len");
    if (ngram < 1 || ngram > MH_NGRAM_MAX) return fail(c, BPE_E_ARG, "ngram: 1..%u", MH_NGRAM_MAX);
    if (n_perm < 1 || n_perm > MH_PERM_MAX) return fail(c, BPE_E_ARG, "n_perm: 1..%u", MH_PERM_MAX);
    if ((uintptr_t)d_ids & (uintptr_t)(id_width - 1)) return fail(c, BPE_E_ARG, "d_ids must be aligned to id_width");
    if ((uintptr_t)d_doc_offsets & 7) return fail(c, BPE_E_ARG, "d_doc_offsets must be 8-byte aligned");
    if ((uintptr_t)d_sig & 3) return fail(c, BPE_E_ARG, "d_sig must be 4-byte aligned");
    // document numbers are 32-bit words with ~0u for "none", and so are the positions of a key
    if (n >= (1ull << 32)) return fail(c, BPE_E_LIMIT, "%llu ids exceed 2^32-1", (unsigned long long)n);
    if (n_docs >= (1ull << 32) - 1) return fail(c, BPE_E_LIMIT, "%llu documents exceed 2^32-2", (unsigned long long)n_docs);
    const uint64_t words = n_docs * n_perm;  // (below 2^42)
    if (words >= (1ull << 40)) return fail(c, BPE_E_LIMIT, "%llu signature words exceed 2^40-1", (unsigned long long)words);
    if (sig_cap < words) return fail(c, BPE_E_CAP, "need %llu signature words", (unsigned long long)words);
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long ends[2] = {0, 0};
    TRY(check_doc_offsets(c, d_doc_offsets, n_docs, n, bad_doc, ends));
    if (n_docs == 0) return BPE_OK;
    // from here on the offsets are known to ascend inside [0, n]: every key lies inside the ids
    std::vector<unsigned long long> ab;  // (lives until the stream is synchronised below)
    if (n_perm > c->cap_mh_perm) c->mh_perm = 0;
    TRY(grow_group(c->cap_mh_perm, n_perm, [&]() -> int { return dev_realloc(c, c->d_mh_ab, 2 * (size_t)n_perm); }));
    if (c->mh_perm != n_perm || c->mh_seed != seed) {
        c->mh_perm = 0;
        mh_params(seed, n_perm, ab);
        HIPCHK(c, hipMemcpyAsync(c->d_mh_ab, ab.data(), ab.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
    }
    const uint32_t tail = (flags & BPE_SELECT_TAIL) ? 1u : 0u;
    const uint32_t tile = (uint32_t)c->mh_tile;
    const uint64_t p0 = ends[0], p1 = ends[1];
    const uint64_t a = ((uintptr_t)d_ids & 15) / (uint64_t)id_width;  // the kernels' tiles and strips count from the 16-byte boundary
    uint32_t strip_shift = 0;
    while ((1u << strip_shift) < mh_strip(tile)) strip_shift++;
    // (the prefill under a kind of its own, so that a profile tells it from the signature pass)
    TRY(prof_begin(c, BPE_PROF_TABLE, 0));
    hipLaunchKernelGGL(k_mh_prefill, dim3(grid_for((n_docs + 63) / 64, 4, c->num_cus * 8)), dim3(256), 0, c->stream,
                       (const unsigned long long *)d_doc_offsets, n_docs, (unsigned long long)max_len, tail, ngram, n_perm,
                       (unsigned long long)a, strip_shift, d_sig);
    LAUNCHCHK(c, "k_mh_prefill");
    TRY(prof_end(c));
    TRY(prof_begin(c, BPE_PROF_DECODE, (uint64_t)id_width * (p1 - p0) + 4 * words));
    if (p1 > p0) {  // (documents that are all empty keep the prefilled rows)
        MhArgs M;
        M.ids = d_ids;
        M.off = (const unsigned long long *)d_doc_offsets;
        M.n_docs = n_docs;
        M.p0 = p0;
        M.p1 = p1;
        M.max_len = max_len;
        M.tail = tail;
        M.tile = tile;
        M.ngram = ngram;
        M.n_perm = n_perm;
        M.seed32 = (uint32_t)seed;
        M.ab = c->d_mh_ab;
        M.sig = d_sig;
        const uint64_t ntiles = (a + p1 + tile - 1) / tile - (a + p0) / tile;
        const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, (uint64_t)c->num_cus * 8)));
        by_width(id_width, [&](auto t) {
            hipLaunchKernelGGL(k_mh_sig<decltype(t)>, grid, dim3(MH_THREADS), 0, c->stream, M);
        });
        LAUNCHCHK(c, "k_mh_sig");
    }
    TRY(prof_end(c));
    TRY(prof_drain(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mh_perm = n_perm;
    c->mh_seed = seed;
    return BPE_OK;
}

// sig, the pairs and agree are the caller's device buffers.  Host <-> device: the counter {first bad pair}.  The indices
// are checked first, so that nothing is written when one of them names no document.
extern "C" int bpe_minhash_agree_resident(bpe_ctx *c, const int32_t *d_sig, uint64_t n_docs, uint32_t n_perm,
                                          const int64_t *d_a, const int64_t *d_b, uint64_t m, int32_t *d_agree,
                                          uint64_t *bad_pair) {
    if (bad_pair) *bad_pair = ~0ull;
    if (!c || (m && (!d_a || !d_b || !d_agree || (!d_sig && n_docs)))) return fail(c, BPE_E_ARG, "bad arguments");
    if (n_perm < 1 || n_perm > MH_PERM_MAX) return fail(c, BPE_E_ARG, "n_perm: 1..%u", MH_PERM_MAX);
    if (((uintptr_t)d_sig | (uintptr_t)d_agree) & 3) return fail(c, BPE_E_ARG, "d_sig and d_agree must be 4-byte aligned");
    if (((uintptr_t)d_a | (uintptr_t)d_b) & 7) return fail(c, BPE_E_ARG, "d_a and d_b must be 8-byte aligned");
    if (n_docs >= (1ull << 32) - 1) return fail(c, BPE_E_LIMIT, "%llu documents exceed 2^32-2", (unsigned long long)n_docs);
    if (n_docs * n_perm >= (1ull << 40))
        return fail(c, BPE_E_LIMIT, "%llu signature words exceed 2^40-1", (unsigned long long)(n_docs * n_perm));
    if (m == 0) return BPE_OK;
    HIPCHK(c, hipSetDevice(c->device));
    auto *w = &c->d_scratch->mh;
    HIPCHK(c, hipMemsetAsync(&w->bad, 0xFF, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_mh_pairs_check, dim3(grid_for(m, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                       (const long long *)d_a, (const long long *)d_b, m, n_docs, &w->bad);
    LAUNCHCHK(c, "k_mh_pairs_check");
    unsigned long long bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, &w->bad, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad != ~0ull) {
        if (bad_pair) *bad_pair = bad;
        return fail(c, BPE_E_ARG, "pair %llu names no document (there are %llu)", bad, (unsigned long long)n_docs);
    }
    TRY(prof_begin(c, BPE_PROF_DECODE, 8 * (uint64_t)n_perm * m));
    const uint32_t vec = (n_perm % 4 == 0 && ((uintptr_t)d_sig & 15) == 0) ? 1u : 0u;
    hipLaunchKernelGGL(k_mh_agree, dim3(grid_for(m, 16, c->num_cus * 8)), dim3(256), 0, c->stream, d_sig, n_perm, vec,
                       (const long long *)d_a, (const long long *)d_b, m, d_agree);
    LAUNCHCHK(c, "k_mh_agree");
    TRY(prof_end(c));
    TRY(prof_drain(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BPE_OK;
}
