"""GPU: the single-step API (bpe_load_ids, bpe_get_stats / bpe_read_stats, bpe_argmax, bpe_merge, bpe_read_ids,
bpe_read_chunk_starts) on id lists beyond the byte range, against the CPU oracle.  The streams and what each of them
reaches are in primitive_cases.py (pinned on the CPU in test_primitive_cases_cpu.py); every comparison is exact.

The module has a ctx of its own: the pair table never shrinks, and a table of 20544 columns on the session's engine
would change the row stride of every later test."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import oracle
import primitive_cases as pc

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_CAP, E_LIMIT = -2, -4, -5, -6
DEFAULTS = {"k1": 2, "merge": 0, "scan_sup": 1024, "tie_window": 0}
SENTINEL = -77777


@pytest.fixture(scope="module")
def ctx(native):
    eng = native.Engine(0)
    yield eng
    eng.close()


@contextlib.contextmanager
def options(eng, **opts):
    assert set(opts) <= set(DEFAULTS)
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        yield eng
    finally:
        for k in opts:
            eng.set_option(k, DEFAULTS[k])


def first_max(stats):
    best = max(stats, key=lambda e: e[1])  # the first maximum in insertion order
    return best[0], best[1]


def starts_of(off_full):
    """chunk starts follow the tokens; an empty chunk leaves no mark"""
    return sorted(set(int(off_full[c]) for c in range(len(off_full) - 1) if off_full[c + 1] > off_full[c]))


def check_stats_and_argmax(eng, ids, off):
    eng.load_ids(ids, off)
    ref = oracle.get_stats(ids, off)
    assert eng.get_stats() == ref  # pairs, counts, first positions, dict order
    assert eng.argmax() == first_max(ref)
    return ref


# ---------------------------------------------------------------------------
# table width (first in the file: the module's ctx grows with it)

def test_table_widths_ascending_then_narrow_again(ctx):
    for V in pc.WIDTHS:
        for variant in pc.WIDTH_VARIANTS:
            ids, off = pc.width_case(V, variant)
            ref = check_stats_and_argmax(ctx, ids, off)
            assert first_max(ref)[0] == pc.WIDTH_PAIR[variant](V)
    # the table is 20544 columns wide now: narrow lists on it (vcur < vcap)
    for V in (300, 257):
        for variant in pc.WIDTH_VARIANTS:
            check_stats_and_argmax(ctx, *pc.width_case(V, variant))


@pytest.mark.parametrize("V", [300, 2049])
def test_table_width_on_a_fresh_ctx(native, V):
    with native.Engine(0) as eng:
        for variant in pc.WIDTH_VARIANTS:
            check_stats_and_argmax(eng, *pc.width_case(V, variant))


@pytest.mark.parametrize("k1", [0, 1, 3])
@pytest.mark.parametrize("V", [300, 1921, 2049, 20481])
def test_argmax_under_every_histogram(ctx, V, k1):
    with options(ctx, k1=k1):
        for variant in pc.WIDTH_VARIANTS:
            ids, off = pc.width_case(V, variant)
            ctx.load_ids(ids, off)
            assert ctx.argmax() == first_max(oracle.get_stats(ids, off))


# ---------------------------------------------------------------------------
# selection regimes, first occurrences

@pytest.mark.parametrize("tie_window", [0, 1])
@pytest.mark.parametrize("name", list(pc.SELECTION) + list(pc.FIRST) + list(pc.TIE_WINDOW))
def test_argmax_selection(ctx, name, tie_window):
    ids, off, reg = pc.argmax_case(name)
    with options(ctx, tie_window=tie_window):
        ctx.load_ids(ids, off)
        got = ctx.argmax()
    print(name, "tie_window", tie_window, "want", reg.pair, reg.M, "at", reg.pos, "got", got)
    assert got == (reg.pair, reg.M)


# ---------------------------------------------------------------------------
# merges

@pytest.mark.parametrize("mimpl,scan_sup", [(0, 1024), (0, 0), (1, 1024), (1, 0)])
@pytest.mark.parametrize("V", pc.MERGE_V)
def test_merge_wide_ids(native, V, mimpl, scan_sup):
    ids, off = pc.merge_stream(V)
    with native.Engine(0) as eng:  # a ctx of its own: idx = V + 1000 grows its table
        eng.set_option("merge", mimpl)
        eng.set_option("scan_sup", scan_sup)
        for pair, idx in pc.merge_cases(V):
            eng.load_ids(ids, off)
            exp_ids, off_full = oracle.merge_chunks(ids, off, pair, idx)
            assert eng.merge(pair, idx) == len(exp_ids) < len(ids)
            assert len(eng) == len(exp_ids)
            assert np.array_equal(eng.read_ids(), exp_ids)
            assert eng.read_chunk_starts().tolist() == starts_of(off_full)
            # the table after the merge (and, for idx = V + 1000, after it grew)
            assert eng.get_stats() == oracle.get_stats(exp_ids, off_full)


# ---------------------------------------------------------------------------
# the training loop by hand

@pytest.mark.parametrize("k1,mimpl", [(0, 0), (1, 0), (3, 0), (1, 1)])
def test_hand_loop(ctx, k1, mimpl):
    ids, off = pc.hand_stream()
    want = pc.hand_loop()
    with options(ctx, k1=k1, merge=mimpl):
        ctx.load_ids(ids, off)
        for i, (pair, count, _tied, length) in enumerate(want):
            assert ctx.argmax() == (pair, count), i
            assert ctx.merge(pair, pc.HAND_NEW + i) == length, i
        exp_ids, exp_off = ids, off
        for i, (pair, _, _, _) in enumerate(want):
            exp_ids, exp_off = oracle.merge_chunks(exp_ids, exp_off, pair, pc.HAND_NEW + i)
        assert np.array_equal(ctx.read_ids(), exp_ids)
        assert ctx.read_chunk_starts().tolist() == starts_of(exp_off)


# ---------------------------------------------------------------------------
# contracts of the calls themselves (raw ctypes)

def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def raw_read_stats(lib, h, cap, size):
    a = np.full(size, SENTINEL, np.int32)
    b = np.full(size, SENTINEL, np.int32)
    cnt = np.full(size, 0xABCD, np.uint64)
    first = np.full(size, 0xABCD, np.uint64)
    n = C.c_uint64(12345)
    rc = lib.bpe_read_stats(h, _p(a), _p(b), _p(cnt), _p(first), cap, C.byref(n))
    return rc, n.value, a, b, cnt, first


def test_read_calls_report_cap(native, ctx):
    lib, h = native._lib, ctx._h
    ids, off = pc.width_case(300, "row")
    ctx.load_ids(ids, off)
    ref = ctx.get_stats()
    npairs, n = len(ref), len(ids)
    assert npairs > 4
    # bpe_read_stats
    rc, got, a, b, cnt, first = raw_read_stats(lib, h, npairs - 1, npairs + 8)
    assert (rc, got) == (E_CAP, npairs)
    assert np.all(a[npairs - 1:] == SENTINEL) and np.all(b[npairs - 1:] == SENTINEL)
    assert np.all(cnt[npairs - 1:] == 0xABCD) and np.all(first[npairs - 1:] == 0xABCD)
    rc, got, a, b, cnt, first = raw_read_stats(lib, h, npairs, npairs + 8)
    assert (rc, got) == (0, npairs)
    assert np.all(a[npairs:] == SENTINEL) and np.all(b[npairs:] == SENTINEL)
    assert np.all(cnt[npairs:] == 0xABCD) and np.all(first[npairs:] == 0xABCD)
    order = np.argsort(first[:npairs], kind="stable")
    assert [((int(a[i]), int(b[i])), int(cnt[i]), int(first[i])) for i in order] == ref
    # bpe_read_chunk_starts
    nstarts = len(off)
    out = np.full(nstarts + 8, 0xABCD, np.uint64)
    got = C.c_uint64(12345)
    assert lib.bpe_read_chunk_starts(h, _p(out), nstarts - 1, C.byref(got)) == E_CAP
    assert got.value == nstarts and np.all(out[nstarts - 1:] == 0xABCD)
    assert lib.bpe_read_chunk_starts(h, _p(out), nstarts, C.byref(got)) == 0
    assert got.value == nstarts and out[:nstarts].tolist() == off.tolist() and np.all(out[nstarts:] == 0xABCD)
    # bpe_read_ids
    out = np.full(n + 8, SENTINEL, np.int32)
    assert lib.bpe_read_ids(h, _p(out), n - 1) == E_CAP
    assert np.all(out == SENTINEL)
    assert lib.bpe_read_ids(h, _p(out), n) == 0
    assert np.array_equal(out[:n], ids) and np.all(out[n:] == SENTINEL)


def test_read_stats_needs_current_stats(native):
    ids, off = pc.width_case(300, "col")
    with native.Engine(0) as eng:
        lib, h = native._lib, eng._h

        def state():
            return raw_read_stats(lib, h, 4096, 4096)[0]

        eng.load_ids(ids, off)
        assert state() == E_STATE  # loaded, never counted
        eng.get_stats()
        assert state() == 0
        eng.merge((0, 299), 258)
        assert state() == E_STATE
        eng.get_stats()
        assert state() == 0
        eng.argmax()
        assert state() == E_STATE
        eng.get_stats()
        assert state() == 0
        eng.load_ids(ids, off)
        assert state() == E_STATE
        eng.get_stats()
        assert state() == 0
        eng.merge((0, 299), 1300)  # grows the table
        assert state() == E_STATE
        ids2, off2 = oracle.merge_chunks(ids, off, (0, 299), 1300)
        assert eng.get_stats() == oracle.get_stats(ids2, off2)


def single_step_states(lib, h):
    """rc of every single-step call"""
    n = C.c_uint64(0)
    a, b = C.c_int32(0), C.c_int32(0)
    buf = np.zeros(16, np.int32)
    buf8 = np.zeros(16, np.uint64)
    return {
        "get_stats": lib.bpe_get_stats(h, C.byref(n)),
        "argmax": lib.bpe_argmax(h, C.byref(a), C.byref(b), C.byref(n)),
        "merge": lib.bpe_merge(h, 1, 2, 300, C.byref(n)),
        "len": lib.bpe_len(h, C.byref(n)),
        "read_ids": lib.bpe_read_ids(h, _p(buf), 16),
        "read_chunk_starts": lib.bpe_read_chunk_starts(h, _p(buf8), 16, C.byref(n)),
        "read_stats": raw_read_stats(lib, h, 16, 16)[0],
    }


def test_single_steps_need_loaded_ids(native):
    with native.Engine(0) as eng:
        lib, h = native._lib, eng._h
        assert set(single_step_states(lib, h).values()) == {E_STATE}
        eng.load_ids(np.array([300, 301, 300, 301, 7], np.int32))
        assert eng.argmax() == ((300, 301), 2) and len(eng) == 5
        # bpe_encode_batch reuses the id stream: the loaded ids are gone
        out, _ = eng.encode_batch(np.array([[97, 98]], np.int32), None, b"abab")
        assert out.tolist() == [256, 256]
        assert set(single_step_states(lib, h).values()) == {E_STATE}
        eng.load_ids(np.array([300, 301, 300, 301, 7], np.int32))
        assert eng.argmax() == ((300, 301), 2)


def test_load_ids_rejects_and_keeps_the_stream(native, ctx):
    lib, h = native._lib, ctx._h
    ids, off = pc.width_case(1921, "run")
    ctx.load_ids(ids, off)
    want = first_max(oracle.get_stats(ids, off))
    for bad_id, rc_want in ((65535, E_LIMIT), (-1, E_ARG), (-2 ** 31, E_ARG), (100000, E_LIMIT)):
        bad = np.array([1, 2, bad_id, 3], np.int32)
        assert lib.bpe_load_ids(h, _p(bad), len(bad), None, 0) == rc_want
        assert len(ctx) == len(ids)
        assert np.array_equal(ctx.read_ids(), ids)
        assert ctx.read_chunk_starts().tolist() == off.tolist()
        assert ctx.argmax() == want
    # (65534 is legal and is not loaded here: its table would take 2 x 17 GB)


# ---------------------------------------------------------------------------
# the drop-in helpers

def _dict_stats(ids, counts=None):
    counts = {} if counts is None else counts
    for pair in zip(ids, ids[1:]):
        counts[pair] = counts.get(pair, 0) + 1
    return counts


def test_module_helpers_beyond_bytes(native, monkeypatch):
    import minbpe_amd
    from minbpe_amd import tokenizer

    # the helpers use the process-wide engine: give them one of their own for this test, so that the lists here do
    # not widen the table of the engine every tokenizer of the session shares
    mine = {}
    monkeypatch.setattr(tokenizer, "_engines", mine)
    try:
        rng = np.random.default_rng(11)
        alphabet = [250, 255, 256, 257, 1024, 1919, 1920, 1921, 2047, 2048, 2049, 2100]
        ids = [alphabet[i] for i in rng.integers(0, len(alphabet), size=3000)]
        ids[100:131] = [2100] * 31
        got = minbpe_amd.get_stats(ids)
        want = _dict_stats(ids)
        assert got == want and list(got) == list(want)
        # accumulation into an existing dict: counts add up, new keys go behind the old ones
        other = [2100, 250, 999, 2100, 250] + ids[:50]
        acc = minbpe_amd.get_stats(ids, minbpe_amd.get_stats(other))
        want = _dict_stats(ids, _dict_stats(other))
        assert acc == want and list(acc) == list(want)
        seeded = {(2100, 2100): 1000, (5, 6): 1}
        assert minbpe_amd.get_stats(ids, seeded) is seeded
        assert seeded[(2100, 2100)] == 1000 + _dict_stats(ids)[(2100, 2100)] and seeded[(5, 6)] == 1
        for pair, idx in (((2100, 2100), 2101), ((2048, 2049), 2101), ((250, 2100), 300), ((1919, 1920), 3100)):
            assert minbpe_amd.merge(ids, pair, idx) == oracle.merge(np.array(ids, np.int32), pair, idx).tolist()
        # the engine's 65535-id limit: an error, never a host fallback
        for big in (65535, 100000):
            with pytest.raises(RuntimeError, match="65535"):
                minbpe_amd.get_stats([250, big, 250])
            with pytest.raises(RuntimeError, match="65535"):
                minbpe_amd.merge([250, big, 250], (250, big), 300)
        with pytest.raises(RuntimeError, match="65535"):
            minbpe_amd.merge([250, 251, 250], (250, 251), 65535)
    finally:
        for eng in mine.values():
            eng.close()
