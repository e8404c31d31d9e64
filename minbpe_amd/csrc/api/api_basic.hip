// api_basic.hip -- lifetime, options, input, the single-step functions.
// Part of bpe_api.hip, which includes the parts in order (one translation unit).

// ============================================================================
namespace {
// the end of a ctx, whole or half made: its memory and events (the members free themselves), then its stream
void ctx_free(bpe_ctx *c) {
    hipStream_t stream = c->own_stream ? c->stream : nullptr;
    delete c;
    if (stream) (void)hipStreamDestroy(stream);
}
}  // namespace

extern "C" {

const char *bpe_version(void) { return "minbpe_amd libbpe_hip 0.1 (gfx950)"; }

const char *bpe_last_error(bpe_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int bpe_create(int device_id, bpe_ctx **out) {
    if (!out) return fail(nullptr, BPE_E_ARG, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(nullptr, BPE_E_HIP, "no HIP device available: %s",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device_id < 0 || device_id >= ndev)
        return fail(nullptr, BPE_E_ARG, "device %d out of range (%d devices)", device_id, ndev);
    bpe_ctx *c = new bpe_ctx();
    c->device = device_id;
    auto bail = [&](const char *what, hipError_t er) {
        int rc = fail(nullptr, BPE_E_HIP, "%s failed: %s", what, hipGetErrorString(er));
        ctx_free(c);
        return rc;
    };
    if ((e = hipSetDevice(device_id)) != hipSuccess) return bail("hipSetDevice", e);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess)
        return bail("hipGetDeviceProperties", e);
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // the lean iterations' kernels hold up to LEAN_LDS_BYTES of static LDS per workgroup (k_lean.hip): that is a
    // gfx950 figure (160 KB per CU); on a part that offers less per workgroup the general path runs instead
    if (prop.sharedMemPerBlock < (size_t)LEAN_LDS_BYTES) c->lean = 0;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess)
        return bail("hipStreamCreate", e);
    c->own_stream = true;
    for (const void *fn : {(const void *)k_pair_count_lds, (const void *)k_pair_count_bytes, (const void *)k_pair_count_h32})
        if ((e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, PC_LDS_BYTES)) != hipSuccess)
            return bail("hipFuncSetAttribute(dynamic LDS)", e);
    if ((e = hipFuncSetAttribute((const void *)k_load_count, hipFuncAttributeMaxDynamicSharedMemorySize, LC_LDS_BYTES)) != hipSuccess)
        return bail("hipFuncSetAttribute(dynamic LDS)", e);
    if ((e = hipFuncSetAttribute((const void *)bpe::bpe_g4::k_index_build, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 bpe::bpe_g4::IDX_H * 4)) != hipSuccess)
        return bail("hipFuncSetAttribute(dynamic LDS)", e);
    for (const void *fn : {(const void *)k_count<int32_t, true>, (const void *)k_count<int32_t, false>,
                           (const void *)k_count<int64_t, true>, (const void *)k_count<int64_t, false>})
        if ((e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, COUNT_LDS_BINS_MAX * 4)) != hipSuccess)
            return bail("hipFuncSetAttribute(dynamic LDS)", e);
    if (dev_once(c, c->d_st, 1) != BPE_OK || dev_once(c, c->d_scratch, 1) != BPE_OK) {
        g_create_err = c->err;
        ctx_free(c);
        return BPE_E_HIP;
    }
    *out = c;
    return BPE_OK;
}

void bpe_destroy(bpe_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm) (void)bpe_comm_destroy(c);
    ctx_free(c);
}

int bpe_set_stream(bpe_ctx *c, void *hip_stream) {
    if (!c) return BPE_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->own_stream) HIPCHK(c, hipStreamDestroy(c->stream));
    c->stream = (hipStream_t)hip_stream;
    c->own_stream = false;
    return BPE_OK;
}

// chunk start offsets as the header states them: ascending (equal neighbours = an empty chunk),
// none beyond n.  Every entry point that takes offsets checks them: the kernels compute chunk
// lengths as differences and would index out of bounds on a descending pair.
// chunk offsets must ascend and stay <= n.  A GPT-4-split GB has 170 M of them (1.4 GB): one thread took ~40 ms over
// them before the first byte was uploaded; up to 16 threads take a segment each (the first bad index wins, so the message
// is the one the serial scan gave).
static int check_offsets(bpe_ctx *c, const uint64_t *chunk_offsets, uint64_t n_chunks, uint64_t n) {
    if (!chunk_offsets) return BPE_OK;
    auto scan = [&](uint64_t lo, uint64_t hi) -> uint64_t {  // first bad index in [lo, hi), or ~0
        uint64_t prev = lo ? chunk_offsets[lo - 1] : 0;
        for (uint64_t i = lo; i < hi; i++) {
            const uint64_t o = chunk_offsets[i];
            if (o < prev || o > n) return i;
            prev = o;
        }
        return ~0ull;
    };
    uint64_t bad = ~0ull;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const uint64_t T = n_chunks < (1ull << 22) ? 1 : std::max<uint64_t>(1, std::min<uint64_t>(16, hw / 2));
    if (T == 1) {
        bad = scan(0, n_chunks);
    } else {
        std::vector<uint64_t> first(T, ~0ull);
        std::vector<std::thread> pool;
        const uint64_t per = (n_chunks + T - 1) / T;
        for (uint64_t w = 0; w < T; w++)
            pool.emplace_back([&, w] { first[w] = scan(std::min(n_chunks, w * per), std::min(n_chunks, (w + 1) * per)); });
        for (std::thread &t : pool) t.join();
        for (uint64_t w = 0; w < T; w++) bad = std::min(bad, first[w]);
    }
    if (bad != ~0ull)
        return fail(c, BPE_E_ARG, "chunk_offsets[%llu] = %llu: offsets must ascend and stay <= n = %llu",
                    (unsigned long long)bad, (unsigned long long)chunk_offsets[bad], (unsigned long long)n);
    return BPE_OK;
}

static int load_bytes_impl(bpe_ctx *c, const uint8_t *bytes, uint64_t n, const uint64_t *chunk_offsets,
                           uint64_t n_chunks, const uint8_t *wexp) {
    if (!c || (!bytes && n)) return fail(c, BPE_E_ARG, "bytes is NULL");
    TRY(check_offsets(c, chunk_offsets, n_chunks, n));
    if (n >= (1ull << 32)) return fail(c, BPE_E_LIMIT, "stream of %llu bytes exceeds 2^32-1 per GPU",
                                       (unsigned long long)n);
    if (wexp && !chunk_offsets) return fail(c, BPE_E_ARG, "weights need chunk offsets");
    if (wexp) {  // (checked before anything is queued: no copy may outlive a failed call)
        // pair counts are 32-bit: the text the weighted chunks stand for must stay below 2^32 bytes
        unsigned __int128 stands_for = 0;
        for (uint64_t i = 0; i < n_chunks; i++) {
            if (wexp[i] > 31) return fail(c, BPE_E_ARG, "weight exponent %u of chunk %llu exceeds 31", wexp[i],
                                          (unsigned long long)i);
            const uint64_t b = chunk_offsets[i], e = i + 1 < n_chunks ? chunk_offsets[i + 1] : n;
            if (e > b && e <= n) stands_for += (unsigned __int128)(e - b) << wexp[i];
        }
        if (stands_for >= ((unsigned __int128)1 << 32))
            return fail(c, BPE_E_LIMIT, "the weighted chunks stand for >= 2^32 bytes of text (32-bit pair counts)");
    }
    HIPCHK(c, hipSetDevice(c->device));
    TRY(grow(c, c->cap_bytes, n + 16, c->d_bytes));
    if (n) TRY(upload_h2d(c, c->d_bytes, bytes, n));
    static const uint64_t zero = 0;
    if (!chunk_offsets) {
        chunk_offsets = &zero;
        n_chunks = 1;
    }
    TRY(grow(c, c->cap_offsets, n_chunks, c->d_offsets));
    if (n_chunks) TRY(upload_h2d(c, c->d_offsets, chunk_offsets, n_chunks * sizeof(uint64_t)));
    c->weighted = false;
    if (wexp && n_chunks) {
        TRY(grow(c, c->cap_wexp, n_chunks, c->d_wexp));
        TRY(upload_h2d(c, c->d_wexp, wexp, n_chunks));
        c->weighted = true;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));  // caller may free its buffers on return
    c->nbytes = n;
    c->n_chunks = n_chunks;
    c->have_bytes = true;
    TRY(ensure_table(c, 256));
    TRY(start_from_bytes(c));
    return BPE_OK;
}

int bpe_load_bytes(bpe_ctx *c, const uint8_t *bytes, uint64_t n, const uint64_t *chunk_offsets,
                   uint64_t n_chunks) {
    return load_bytes_impl(c, bytes, n, chunk_offsets, n_chunks, nullptr);
}

int bpe_load_bytes_weighted(bpe_ctx *c, const uint8_t *bytes, uint64_t n, const uint64_t *chunk_offsets,
                            uint64_t n_chunks, const uint8_t *weight_exp) {
    if (!weight_exp) return fail(c, BPE_E_ARG, "weight_exp is NULL");
    return load_bytes_impl(c, bytes, n, chunk_offsets, n_chunks, weight_exp);
}

int bpe_load_ids(bpe_ctx *c, const int32_t *ids, uint64_t n, const uint64_t *chunk_offsets,
                 uint64_t n_chunks) {
    if (!c || (!ids && n)) return fail(c, BPE_E_ARG, "ids is NULL");
    if (n >= (1ull << 32)) return fail(c, BPE_E_LIMIT, "stream too long");
    TRY(check_offsets(c, chunk_offsets, n_chunks, n));
    HIPCHK(c, hipSetDevice(c->device));
    int32_t mx = 255;
    for (uint64_t i = 0; i < n; i++) {
        if (ids[i] < 0) return fail(c, BPE_E_ARG, "negative token id at %llu", (unsigned long long)i);
        mx = std::max(mx, ids[i]);
    }
    TRY(ensure_table(c, (uint32_t)mx + 1));
    TRY(ensure_ids(c, n));
    // stage through buffer 1, then mask into buffer 0
    if (n) {
        HIPCHK(c, hipMemcpyAsync(c->d_ids[1], ids, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_load_ids, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                           (const int32_t *)c->d_ids[1].get(), c->d_ids[0], n);
        LAUNCHCHK(c, "k_load_ids");
    }
    static const uint64_t zero = 0;
    if (!chunk_offsets) {
        chunk_offsets = &zero;
        n_chunks = 1;
    }
    TRY(grow(c, c->cap_offsets, n_chunks, c->d_offsets));
    if (n && n_chunks) {
        HIPCHK(c, hipMemcpyAsync(c->d_offsets, chunk_offsets, n_chunks * sizeof(uint64_t),
                                 hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_mark_starts, dim3(grid_for(n_chunks, 256, c->num_cus * 8)), dim3(256), 0,
                           c->stream, c->d_ids[0], c->d_offsets, n_chunks, n);
        LAUNCHCHK(c, "k_mark_starts");
    }
    hipLaunchKernelGGL(k_init_state, dim3(1), dim3(1), 0, c->stream, c->d_st, (unsigned long long)n);
    LAUNCHCHK(c, "k_init_state");
    c->apply_target = 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_bytes = false;
    c->weighted = false;
    c->stream_is_bytes = false;
    c->par = 0;
    c->n = n;
    c->vcur = (uint32_t)mx + 1;
    c->have_ids = true;
    c->stats_valid = false;
    return BPE_OK;
}

int bpe_get_stats(bpe_ctx *c, uint64_t *n_pairs_out) {
    if (!c) return BPE_E_ARG;
    if (!c->have_ids) return fail(c, BPE_E_STATE, "no ids loaded");
    HIPCHK(c, hipSetDevice(c->device));
    TRY(dev_once(c, c->d_first, (size_t)c->vcap * c->vcap));  // (ensure_table drops it when the table grows)
    TRY(clear_table(c));
    HIPCHK(c, hipMemsetAsync(c->d_first, 0xFF, (size_t)c->vcur * c->vcap * sizeof(uint32_t), c->stream));
    TRY(launch_pair_count(c, true));
    HIPCHK(c, hipMemsetAsync(&c->d_scratch->count, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_count_nonzero, dim3(c->vcur), dim3(256), 0, c->stream, c->d_mat, c->vcap,
                       c->vcur, &c->d_scratch->count);
    LAUNCHCHK(c, "k_count_nonzero");
    unsigned long long np = 0;
    HIPCHK(c, hipMemcpyAsync(&np, &c->d_scratch->count, sizeof np, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stats_valid = true;
    if (n_pairs_out) *n_pairs_out = np;
    return BPE_OK;
}

int bpe_read_stats(bpe_ctx *c, int32_t *a, int32_t *b, uint64_t *cnt, uint64_t *first_pos,
                   uint64_t cap, uint64_t *n_out) {
    if (!c) return BPE_E_ARG;
    if (!c->stats_valid) return fail(c, BPE_E_STATE, "bpe_get_stats has not been run on the current ids");
    HIPCHK(c, hipSetDevice(c->device));
    DevPtr<int32_t> da, db;  // this call's scratch, released on every exit path
    DevPtr<unsigned long long> dc, df;
    const size_t capn = cap ? cap : 1;
    TRY(dev_realloc(c, da, capn));
    TRY(dev_realloc(c, db, capn));
    TRY(dev_realloc(c, dc, capn));
    TRY(dev_realloc(c, df, capn));
    HIPCHK(c, hipMemsetAsync(&c->d_scratch->count, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_dump_stats, dim3(c->vcur), dim3(256), 0, c->stream, c->d_mat, c->d_first,
                       c->vcap, c->vcur, da, db, dc, df, (unsigned long long)cap, &c->d_scratch->count);
    LAUNCHCHK(c, "k_dump_stats");
    unsigned long long np = 0;
    HIPCHK(c, hipMemcpyAsync(&np, &c->d_scratch->count, sizeof np, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int rc = BPE_OK;
    if (np > cap) {
        rc = fail(c, BPE_E_CAP, "%llu pairs but cap is %llu", np, (unsigned long long)cap);
    } else if (np) {
        HIPCHK(c, hipMemcpy(a, da, np * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(b, db, np * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(cnt, dc, np * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(first_pos, df, np * 8, hipMemcpyDeviceToHost));
    }
    if (n_out) *n_out = np;
    return rc;
}

int bpe_argmax(bpe_ctx *c, int32_t *a, int32_t *b, uint64_t *count) {
    if (!c) return BPE_E_ARG;
    if (!c->have_ids) return fail(c, BPE_E_STATE, "no ids loaded");
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_set_pair, dim3(1), dim3(1), 0, c->stream, c->d_st, 0, 0);  // clears status
    TRY(clear_table(c));
    TRY(launch_pair_count(c, false));
    c->stats_valid = false;
    TRY(launch_select(c, true));
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, c->stream, stream_ref(c), c->par, c->d_st);
    LAUNCHCHK(c, "k_finalize");
    DevState st;
    TRY(read_state(c, &st));
    if (st.status == ST_EMPTY) return fail(c, BPE_E_EMPTY_STATS, "max() arg is an empty sequence");
    if (st.status != ST_OK) return fail(c, BPE_E_INTERNAL, "device status %u", st.status);
    if (a) *a = st.a;
    if (b) *b = st.b;
    if (count) *count = st.count;
    return BPE_OK;
}

int bpe_merge(bpe_ctx *c, int32_t a, int32_t b, int32_t idx, uint64_t *new_len) {
    if (!c) return BPE_E_ARG;
    if (!c->have_ids) return fail(c, BPE_E_STATE, "no ids loaded");
    if (a < 0 || b < 0 || idx < 0) return fail(c, BPE_E_ARG, "negative id");
    HIPCHK(c, hipSetDevice(c->device));
    TRY(ensure_table(c, (uint32_t)std::max(idx, std::max(a, b)) + 1));
    hipLaunchKernelGGL(k_set_pair, dim3(1), dim3(1), 0, c->stream, c->d_st, a, b);
    LAUNCHCHK(c, "k_set_pair");
    const uint64_t n_before = c->n;
    TRY(launch_merge(c, (uint32_t)idx, 0, nullptr, false));
    DevState st;
    TRY(read_state(c, &st));
    c->n = st.n[c->par];
    if (c->profile) c->prof_bytes[BPE_PROF_MERGE] += 4 * (n_before + c->n);
    c->vcur = std::max<uint32_t>(c->vcur, (uint32_t)idx + 1);
    if (new_len) *new_len = c->n;
    return BPE_OK;
}

int bpe_len(bpe_ctx *c, uint64_t *n) {
    if (!c || !n) return BPE_E_ARG;
    if (!c->have_ids) return fail(c, BPE_E_STATE, "no ids loaded");
    *n = c->n;
    return BPE_OK;
}

int bpe_read_ids(bpe_ctx *c, int32_t *out, uint64_t cap) {
    if (!c) return BPE_E_ARG;
    if (!c->have_ids) return fail(c, BPE_E_STATE, "no ids loaded");
    if (cap < c->n) return fail(c, BPE_E_CAP, "need %llu entries", (unsigned long long)c->n);
    if (!c->n) return BPE_OK;
    HIPCHK(c, hipSetDevice(c->device));
    // strip flags into the idle ping-pong buffer, then copy out
    int32_t *tmp = (int32_t *)c->d_ids[c->par ^ 1].get();
    hipLaunchKernelGGL(k_strip_flags, dim3(grid_for(c->n, 256, c->num_cus * 8)), dim3(256), 0,
                       c->stream, c->d_ids[c->par], tmp, c->n);
    LAUNCHCHK(c, "k_strip_flags");
    HIPCHK(c, hipMemcpyAsync(out, tmp, c->n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BPE_OK;
}

int bpe_read_chunk_starts(bpe_ctx *c, uint64_t *out, uint64_t cap, uint64_t *n_out) {
    if (!c) return BPE_E_ARG;
    if (!c->have_ids) return fail(c, BPE_E_STATE, "no ids loaded");
    HIPCHK(c, hipSetDevice(c->device));
    DevPtr<unsigned long long> d_out;
    TRY(dev_realloc(c, d_out, cap ? cap : 1));
    HIPCHK(c, hipMemsetAsync(&c->d_scratch->count, 0, sizeof(unsigned long long), c->stream));
    if (c->n) {
        hipLaunchKernelGGL(k_collect_starts, dim3(grid_for(c->n, 256, c->num_cus * 8)), dim3(256), 0,
                           c->stream, c->d_ids[c->par], c->n, d_out, (unsigned long long)cap,
                           &c->d_scratch->count);
        LAUNCHCHK(c, "k_collect_starts");
    }
    unsigned long long ns = 0;
    HIPCHK(c, hipMemcpyAsync(&ns, &c->d_scratch->count, sizeof ns, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int rc = BPE_OK;
    if (ns > cap) {
        rc = fail(c, BPE_E_CAP, "%llu chunk starts but cap is %llu", ns, (unsigned long long)cap);
    } else if (ns) {
        HIPCHK(c, hipMemcpy(out, d_out, ns * 8, hipMemcpyDeviceToHost));
        std::sort(out, out + ns);
    }
    if (n_out) *n_out = ns;
    return rc;
}

}  // extern "C"
