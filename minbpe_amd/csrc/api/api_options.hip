// api_options.hip -- bpe_set_option: one table, one row per option.
// Part of bpe_api.hip, which includes the parts in order (one translation unit).
//
// An option is a field of bpe_ctx (api_ctx.hip: its default is the field's initialiser, its meaning the field's
// comment) and one row here: what values it accepts.  A new option is those two places (its row goes to OPTIONS_MORE).

namespace {

enum OptKind {
    OPT_RANGE,  // lo <= value <= hi and value % step == 0, stored as is
    OPT_POW2,   // lo <= value <= hi and value a power of two, stored as is
    OPT_FLAG,   // any value, stored as value != 0
    OPT_ANY,    // any value, stored as is (cast to the field's type)
};

struct OptRow {
    const char *name;
    void (*set)(bpe_ctx *, int64_t);
    int64_t (*get)(const bpe_ctx *);
    OptKind kind;
    int64_t lo, hi, step;
};

// the row of the option that is named like its field -- so a row cannot name one option and set another -- and of the
// four whose names differ
#define OPT_NAMED(name, field, kind, lo, hi, step)                                      \
    {name, [](bpe_ctx *c, int64_t v) { c->field = (decltype(c->field))v; },             \
     [](const bpe_ctx *c) { return (int64_t)c->field; }, kind, lo, hi, step}
#define OPT(field, lo, hi) OPT_NAMED(#field, field, OPT_RANGE, lo, hi, 1)
#define OPT_STEP(field, lo, hi, step) OPT_NAMED(#field, field, OPT_RANGE, lo, hi, step)
#define OPT_ON(field) OPT_NAMED(#field, field, OPT_FLAG, 0, 1, 1)
#define OPT_RAW(field) OPT_NAMED(#field, field, OPT_ANY, INT64_MIN, INT64_MAX, 1)

const OptRow OPTIONS[] = {
    // the engine and its variants
    OPT(mode, 0, 1),
    OPT(profile, 0, 2),
    OPT(prof_stride, 1, 1024),
    OPT(depth, 0, 64),
    OPT_RAW(k1),
    OPT_NAMED("scan_sup", scan_sup_min, OPT_RANGE, 0, 1 << 30, 1),
    OPT_NAMED("merge", merge_impl, OPT_RANGE, 0, 1, 1),
    OPT_RAW(lb_tune),
    OPT_ON(fused_rows),
    OPT_NAMED("slots", use_slots, OPT_RANGE, 0, 2, 1),
    OPT_NAMED("sparse", use_sparse, OPT_RANGE, 0, 2, 1),
    OPT(sparse_ratio, 1, 64),
    OPT(small_slots, 0, 2),
    OPT(repack_acc, 0, 10000),
    OPT(rep_max, 0, 8),
    OPT(rep_min, 0, 8),
    OPT_ON(lds_delta),
    OPT_ON(exp_no_delta),
    OPT_ON(tie_window),
    OPT_ON(tie_index),
    OPT_ON(aa_sparse),
    OPT_ON(fuse_load),
    OPT(pinned_upload, 0, 1),
    // lean iterations
    OPT(lean, 0, 2),
    OPT_ON(lean_backoff),
    OPT(lean_count, 0, INT64_MAX),
    OPT(lean_grid, 1, 65535),
    OPT(lean_scan, 1, 1024),
    OPT_ON(lean_select),
    OPT_ON(lean_chain),
    OPT_ON(lean_sum),
    // chain steps
    OPT_ON(chain),
    OPT_ON(chain_dense),
    OPT_ON(chain_prefetch),
    OPT_ON(count_is_removed),
    OPT(chain_kcap, 1, CH_KSWEEP),
    OPT(chain_scan, 1, 255),
    OPT(chain_aa, 0, 1),
    OPT(chain_share_first, 0, 1),
    OPT(chain_hash_kmin, 0, 32),
    OPT(pool_hint, 0, 128),
    OPT(fuse_step, 0, 1),
    // sharded training
    OPT_ON(dp_force_comm),
    OPT(dp_kcap, 1, DP_KCAP_MAX),
    // encode
    OPT_ON(enc_chain),
    OPT_ON(enc_cache),
    OPT(enc_hash_bits, 0, 40),
    OPT_ON(enc_long),
    OPT(enc_replay, 0, 1),
    // decode, rows, spans, projection: bytes, tokens, elements, document starts, ids
    OPT_ON(dec_copy),
    OPT_STEP(dec_window, 1024, 32768, 16),
    OPT_STEP(dec_tile, 256, 16384, 256),
    OPT_STEP(rows_tile, 64, ROWS_TILE_MAX, ROWS_V),
    OPT(rows_stage, 0, ROWS_STAGE_MAX),
    OPT(spans_stage, 0, SPANS_STAGE_MAX),
    OPT_STEP(proj_tile, 64, 16384, 64),
    OPT_STEP(proj_window, 64, PROJ_WINDOW_MAX, 4),
};

// The rows that came after tests/native/ctx_check.hip pinned the table above at the 57 it walks one by one: the same
// rows, looked up after it.  The id histogram (bpe_count_resident): bins, ids; document selection
// (bpe_select_docs_resident): elements, output starts; document de-duplication (bpe_dup_docs_resident): positions, ids, bits;
// MinHash signatures (bpe_minhash_resident): positions; n-gram overlap (bpe_ngram_index_resident,
// bpe_ngram_overlap_resident): positions, bits; repetition statistics (bpe_repeat_stats_resident): positions, bits; span
// de-duplication (bpe_dup_spans_resident): positions, bits; segments (bpe_segment_docs_resident,
// bpe_segment_marks_resident): positions, ranges
const OptRow OPTIONS_MORE[] = {
    OPT_STEP(count_lds_bins, 256, COUNT_LDS_BINS_MAX, 256),
    OPT(count_flush, 64, 1ll << 31),
    OPT_ON(count_combine),
    OPT_STEP(sel_tile, 64, SEL_TILE_MAX, 4),
    OPT(sel_stage, 0, SEL_STAGE_MAX),
    OPT_STEP(dup_tile, 64, DUP_TILE_MAX, 4),
    OPT(dup_wave_len, 4, DUP_WAVE_LEN_MAX),
    OPT(dup_hash_bits, 0, 64),
    OPT_NAMED("mh_tile", mh_tile, OPT_POW2, 64, MH_TILE_MAX, 1),
    OPT_NAMED("ng_tile", ng_tile, OPT_POW2, 64, NG_TILE_MAX, 1),
    OPT(ng_hash_bits, 0, 64),
    OPT_NAMED("rp_tile", rp_tile, OPT_POW2, 64, RP_TILE_MAX, 1),
    OPT(rp_hash_bits, 0, 64),
    OPT_NAMED("ds_tile", ds_tile, OPT_POW2, 64, DS_TILE_MAX, 1),
    OPT(ds_hash_bits, 0, 64),
    OPT_STEP(seg_tile, 64, SEG_TILE_MAX, 64),
    OPT(seg_stage, 0, SEG_STAGE_MAX),
};

#undef OPT_RAW
#undef OPT_ON
#undef OPT_STEP
#undef OPT
#undef OPT_NAMED

}  // namespace

extern "C" int bpe_set_option(bpe_ctx *c, const char *name, int64_t value) {
    if (!c || !name) return BPE_E_ARG;
    const size_t n_first = sizeof OPTIONS / sizeof OPTIONS[0], n_rows = n_first + sizeof OPTIONS_MORE / sizeof OPTIONS_MORE[0];
    for (size_t r = 0; r < n_rows; r++) {
        const OptRow &o = r < n_first ? OPTIONS[r] : OPTIONS_MORE[r - n_first];
        if (strcmp(name, o.name)) continue;
        if (o.kind == OPT_RANGE && (value < o.lo || value > o.hi || value % o.step)) {
            if (o.step > 1)
                return fail(c, BPE_E_ARG, "%s: %lld..%lld, a multiple of %lld", o.name, (long long)o.lo, (long long)o.hi,
                            (long long)o.step);
            if (o.hi == INT64_MAX) return fail(c, BPE_E_ARG, "%s: %lld or more", o.name, (long long)o.lo);
            return fail(c, BPE_E_ARG, "%s: %lld..%lld", o.name, (long long)o.lo, (long long)o.hi);
        }
        if (o.kind == OPT_POW2 && (value < o.lo || value > o.hi || (value & (value - 1))))
            return fail(c, BPE_E_ARG, "%s: %lld..%lld, a power of two", o.name, (long long)o.lo, (long long)o.hi);
        o.set(c, o.kind == OPT_FLAG ? (int64_t)(value != 0) : value);
        return BPE_OK;
    }
    return fail(c, BPE_E_ARG, "unknown option '%s'", name);
}
