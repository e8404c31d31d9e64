// ctx_check.hip -- the ctx's housekeeping, checked on the host: a stand-alone program that includes the library's
// host side and works on a bpe_ctx it constructs itself (no bpe_create, so no device is needed).
//
//   1. bpe_set_option, row by row of the option table: lowest, highest, one below, one above, one off the step --
//      the return code, the value of the field the row names, and that a refused value leaves the field alone.
//   2. Without a device every hipMalloc fails: each ensure_* and each grow site that can be reached then is called
//      twice -- a large request, then one the capacity word held before would have satisfied -- and must fail with
//      BPE_E_HIP both times, leave its capacity word 0 and its pointers null.  Deleting the ctx must be clean.
//      With a device present this part is skipped: the program touches no device memory.
//
// Built and run by tests/test_ctx_host.py; exit status 0 = every check passed.
#include "bpe_api.hip"

#include <set>
#include <type_traits>

static_assert(!std::is_copy_constructible<DevPtr<int>>::value && !std::is_copy_assignable<DevPtr<int>>::value, "DevPtr copies");
static_assert(!std::is_copy_constructible<PinnedPtr<int>>::value && !std::is_copy_constructible<EventList>::value, "owners copy");

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            failures++;                       \
            fprintf(stderr, "ctx_check: ");   \
            fprintf(stderr, __VA_ARGS__);     \
            fprintf(stderr, "\n");            \
        }                                     \
    } while (0)

static void accepted(bpe_ctx *c, const OptRow &o, int64_t value, int64_t stored) {
    const int rc = bpe_set_option(c, o.name, value);
    CHECK(rc == BPE_OK, "%s = %lld: refused (%d)", o.name, (long long)value, rc);
    CHECK(o.get(c) == stored, "%s = %lld: the field reads %lld", o.name, (long long)value, (long long)o.get(c));
}

static void refused(bpe_ctx *c, const OptRow &o, int64_t value) {
    const int64_t before = o.get(c);
    const int rc = bpe_set_option(c, o.name, value);
    CHECK(rc == BPE_E_ARG, "%s = %lld: return code %d", o.name, (long long)value, rc);
    CHECK(o.get(c) == before, "%s = %lld was refused and the field changed", o.name, (long long)value);
}

static void check_options() {
    bpe_ctx *c = new bpe_ctx();
    std::set<std::string> names;
    for (const OptRow &o : OPTIONS) {
        CHECK(names.insert(o.name).second, "%s: two rows", o.name);
        const int64_t dflt = o.get(c);
        if (o.kind == OPT_RANGE) {
            CHECK(dflt >= o.lo && dflt <= o.hi && dflt % o.step == 0, "%s: the default %lld is not a value the row accepts", o.name, (long long)dflt);
            accepted(c, o, o.hi < INT64_MAX ? o.hi : (int64_t)1 << 62, o.hi < INT64_MAX ? o.hi : (int64_t)1 << 62);
            accepted(c, o, o.lo, o.lo);
            refused(c, o, o.lo - 1);
            if (o.hi < INT64_MAX) refused(c, o, o.hi + 1);
            if (o.step > 1) {
                refused(c, o, o.lo + 1);
                refused(c, o, o.hi - 1);
                accepted(c, o, o.lo + o.step, o.lo + o.step);
            }
        } else if (o.kind == OPT_FLAG) {
            for (int64_t v : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)-1, (int64_t)1 << 40}) accepted(c, o, v, v != 0);
        } else {
            for (int64_t v : {(int64_t)0, (int64_t)7, (int64_t)0x1FF}) accepted(c, o, v, v);
            CHECK(bpe_set_option(c, o.name, -1) == BPE_OK, "%s = -1: refused", o.name);
        }
        accepted(c, o, dflt, dflt);
    }
    CHECK(names.size() == 57, "%zu options, not 57", names.size());
    // the four whose names are not their fields'
    CHECK(bpe_set_option(c, "merge", 1) == BPE_OK && c->merge_impl == 1, "merge does not set merge_impl");
    CHECK(bpe_set_option(c, "slots", 1) == BPE_OK && c->use_slots == 1, "slots does not set use_slots");
    CHECK(bpe_set_option(c, "sparse", 2) == BPE_OK && c->use_sparse == 2, "sparse does not set use_sparse");
    CHECK(bpe_set_option(c, "scan_sup", 5) == BPE_OK && c->scan_sup_min == 5, "scan_sup does not set scan_sup_min");
    for (const char *field : {"merge_impl", "use_slots", "use_sparse", "scan_sup_min"})
        CHECK(bpe_set_option(c, field, 1) == BPE_E_ARG, "%s is taken as an option", field);
    CHECK(bpe_set_option(c, "no_such_option", 1) == BPE_E_ARG && c->err == "unknown option 'no_such_option'", "unknown option: '%s'", c->err.c_str());
    CHECK(bpe_set_option(nullptr, "mode", 1) == BPE_E_ARG && bpe_set_option(c, nullptr, 1) == BPE_E_ARG, "null arguments");
    delete c;
}

// a site of the grow rule: its capacity word, as if a group of `held` had been there; call(false) asks for more than
// that, call(true) for less -- which a word left standing after a failed allocation would wave through, null pointers and all
template <typename Cap, typename Call, typename Null>
static void fails_twice(const char *what, Cap &cap, uint64_t held, Call call, Null all_null) {
    cap = (Cap)held;
    for (int small = 0; small < 2; small++) {
        const int rc = call(small != 0);
        CHECK(rc == BPE_E_HIP, "%s, %s request: return code %d", what, small ? "small" : "large", rc);
        CHECK(cap == 0, "%s, %s request: the capacity word reads %llu", what, small ? "small" : "large", (unsigned long long)cap);
        CHECK(all_null(), "%s, %s request: a pointer is not null", what, small ? "small" : "large");
    }
}

static void check_failed_allocations() {
    bpe_ctx *c = new bpe_ctx();
    int unused = 0;  // (sites without a capacity word)
    fails_twice("ensure_ids (streams)", c->cap_ids, 8 * TILE, [&](bool s) { return ensure_ids(c, s ? TILE : 100 * TILE); },
                [&] { return !c->d_ids[0] && !c->d_ids[1] && !c->d_ids2; });
    c->cap_ids = ~0ull >> 1;  // (the second group of ensure_ids on its own)
    fails_twice("ensure_ids (tiles)", c->cap_tiles, 8, [&](bool s) { return ensure_ids(c, s ? TILE : 100 * TILE); },
                [&] { return !c->d_tsum && !c->d_tile_off && !c->d_hdr2[0] && !c->d_stage && !c->d_desc && !c->d_gdesc; });
    c->cap_ids = 0;
    fails_twice("ensure_table", c->vcap, 512, [&](bool s) { return ensure_table(c, s ? 300 : 1000); },
                [&] { return !c->d_mat && !c->d_rowmax && !c->d_delta && !c->d_dirty_list && !c->d_dirty_n && !c->d_lean_res; });
    fails_twice("ensure_rec", c->rec_cap, 64, [&](bool s) { return ensure_rec(c, s ? 8 : 1000); }, [&] { return !c->h_rec; });
    fails_twice("ensure_srec", unused, 0, [&](bool) { return ensure_srec(c); }, [&] { return !c->h_srec; });
    fails_twice("ensure_dec_scratch", c->cap_dec_n, 64, [&](bool s) { return ensure_dec_scratch(c, s ? 8 : 1000); },
                [&] { return !c->d_dec_ids && !c->d_dec_len && !c->d_dec_off && !c->d_dec_bsum; });
    fails_twice("ensure_chain_buffers", unused, 0, [&](bool s) { return ensure_chain_buffers(c, s); },
                [&] { return !c->d_chain_req && !c->d_pool && !c->d_pool_gather && !c->d_step_pub && !c->d_step_bar; });
    c->idx_cap_rows = idx_h(c);
    fails_twice("index_build", c->idx_cap_words, 64, [&](bool s) { c->slot_T = s ? 32 : 32 * 1000; return index_build(c); },
                [&] { return !c->d_idx && !c->d_idx_tmp && !c->d_idx_dirty && c->idx_cap_rows == 0; });
    fails_twice("spans_meta", c->cap_dec_meta, 64, [&](bool s) { c->dec_V = s ? 8 : 1000; return spans_meta(c); },
                [&] { return !c->d_dec_meta && !c->dec_meta_valid; });
    const uint64_t offsets[4] = {0, 1, 2, 3};
    fails_twice("upload_offsets", c->cap_offsets, 64, [&](bool s) { return upload_offsets(c, offsets, s ? 4 : 1000); },
                [&] { return !c->d_offsets; });
    fails_twice("grow (one buffer)", c->cap_bytes, 64, [&](bool s) { return grow(c, c->cap_bytes, s ? 8 : 1000, c->d_bytes); },
                [&] { return !c->d_bytes; });
    DevPtr<int> scratch;  // (a call's scratch)
    CHECK(dev_realloc(c, scratch, 16) == BPE_E_HIP && !scratch, "dev_realloc of a local DevPtr");
    CHECK(!c->err.empty(), "no error text");
    delete c;
}

int main() {
    check_options();
    int ndev = 0;
    const bool no_device = hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0;
    (void)hipGetLastError();
    if (no_device) check_failed_allocations();
    printf("ctx_check: %d options; failed allocations %s; %d failure%s\n", (int)(sizeof OPTIONS / sizeof OPTIONS[0]),
           no_device ? "checked" : "skipped (a device is present)", failures, failures == 1 ? "" : "s");
    return failures ? 1 : 0;
}
