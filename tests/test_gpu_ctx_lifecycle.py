"""GPU: the ctx's housekeeping -- which values every option accepts, and create / work / destroy three times over with
every scratch group growing and shrinking in between (api_ctx.hip: the owners, the grow rule; api_options.hip)."""

import numpy as np
import pytest

import encode_cases as ec
import oracle
import test_gpu_project as P
import test_gpu_resident_shared as R
import test_gpu_rows as W
import test_gpu_spans as S

pytestmark = pytest.mark.gpu

E_ARG = -2
ANY = [-(2 ** 40), -1, 0, 1, 2, 3, 2 ** 33]

# What bpe_set_option accepts, option by option, as its 57-arm ladder stood before the table replaced it:
#   (lo, hi)        lo..hi                        (hi None: no upper bound)
#   (lo, hi, step)  ... and a multiple of step
#   "flag"          any value (stored as value != 0)
#   "any"           any value (stored as is)
ACCEPTS = {
    "mode": (0, 1), "profile": (0, 2), "k1": "any", "scan_sup": (0, 1 << 30), "merge": (0, 1), "lb_tune": "any",
    "fused_rows": "flag", "slots": (0, 2), "sparse": (0, 2), "rep_max": (0, 8), "rep_min": (0, 8), "lds_delta": "flag",
    "exp_no_delta": "flag", "tie_window": "flag", "tie_index": "flag", "sparse_ratio": (1, 64), "lean": (0, 2),
    "lean_backoff": "flag", "lean_count": (0, None), "lean_grid": (1, 65535), "enc_chain": "flag", "enc_cache": "flag",
    "enc_hash_bits": (0, 40), "dec_copy": "flag", "dec_window": (1024, 32768, 16), "dec_tile": (256, 16384, 256),
    "rows_tile": (64, 65536, 4), "rows_stage": (0, 4096), "spans_stage": (0, 4096), "proj_tile": (64, 16384, 64),
    "proj_window": (64, 8192, 4), "prof_stride": (1, 1024), "lean_select": "flag", "aa_sparse": "flag",
    "dp_force_comm": "flag", "dp_kcap": (1, 15), "fuse_load": "flag", "chain_dense": "flag", "chain_prefetch": "flag",
    "count_is_removed": "flag", "enc_long": "flag", "small_slots": (0, 2), "chain_kcap": (1, 31), "enc_replay": (0, 1),
    "pinned_upload": (0, 1), "fuse_step": (0, 1), "chain_aa": (0, 1), "chain_share_first": (0, 1),
    "chain_hash_kmin": (0, 32), "pool_hint": (0, 128), "chain_scan": (1, 255), "chain": "flag", "lean_chain": "flag",
    "lean_sum": "flag", "lean_scan": (1, 1024), "repack_acc": (0, 10000), "depth": (0, 64),
}


def boundary_cases(spec):
    """[(value, accepted)]: lowest, highest, one below, one above, one off the step"""
    if spec in ("flag", "any"):
        return [(v, True) for v in ANY]
    lo, hi, step = (*spec, 1)[:3]
    cases = [(lo, True), (lo - 1, False), (lo - step, False)]
    cases += [(2 ** 62, True)] if hi is None else [(hi, True), (hi + 1, False), (hi + step, False)]
    if step > 1:
        cases += [(lo + step, True), (lo + 1, False), (hi - 1, False), (lo + step // 2, False)]
    return cases


def test_the_table_is_complete():
    assert len(ACCEPTS) == 57


def test_option_boundaries(native):
    """every option's boundary cases on an engine of its own, which never runs any work"""
    wrong = []
    with native.Engine(0) as e:
        for name, spec in ACCEPTS.items():
            for value, accepted in boundary_cases(spec):
                rc = native._lib.bpe_set_option(e._h, name.encode(), value)
                if (rc == 0) != accepted or rc not in (0, E_ARG):
                    wrong.append((name, value, rc))
        assert native._lib.bpe_set_option(e._h, b"no_such_option", 1) == E_ARG
        assert native._lib.bpe_last_error(e._h) == b"unknown option 'no_such_option'"
        assert native._lib.bpe_set_option(e._h, None, 1) == E_ARG
    assert not wrong, f"(option, value, return code): {wrong}"


# ---------------------------------------------------------------------------
# create, work, destroy

@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


MERGES = 64
_WANT = {}


def want_of(scale):
    """the text of a round, the oracle's training result and its encoding of the batch: once per size, left unchanged"""
    if scale not in _WANT:
        import minbpe_amd
        data = minbpe_amd.synth_text(65536 * scale, 3)
        trained = oracle.train(data, MERGES)
        rng = np.random.default_rng(11)
        offs = np.concatenate([[0], np.cumsum(rng.integers(1, 40, size=300 * scale - 1))]).astype(np.uint64)
        batch = data[:int(offs[-1]) + 17]
        enc_ids, enc_off = oracle.encode(trained[0], batch, ec.oracle_offsets(batch, offs))
        enc_ids.setflags(write=False)
        _WANT[scale] = (data, trained, batch, offs, enc_ids, enc_off)
    return _WANT[scale]


def work(torch, native, e, scale):
    """train, encode a batch, then the four resident entry points: each compared with the oracle or its host model the way
    its own test file does; returns what the engine itself gave back"""
    data, trained, batch, offs, enc_ids, enc_off = want_of(scale)
    e.load_bytes(data)
    res = e.train(MERGES)
    assert (res["pairs"], res["counts"], res["lens"]) == trained
    ids, out_off = e.encode_batch(np.array(trained[0], np.int32), None, batch, offs)
    assert np.array_equal(out_off, enc_off) and np.array_equal(ids, enc_ids)
    n = 3000 * scale
    sids, pids = S.random_ids(n, 500 + scale), P.random_ids(n, 500 + scale)
    R.decode_resident(torch, native, e, sids, pids, R.joined(sids))
    S.spans(torch, native, e, sids, torch.int32, doc=R.doc_of(n))
    rows = W.check_pack(torch, native, e, pids.astype(np.int32), W.offsets_of([n // 3, 0, n - n // 3]), 96, 64, W.SEP,
                        companions=True)
    P.project_checked(native, torch, e, pids, torch.int64, 256)
    return res["pairs"], res["counts"], res["lens"], ids.tobytes(), out_off.tobytes(), rows.tobytes()


def test_create_work_destroy(torch, native):
    """Three engines, one after the other.  The second runs the work at the base sizes, at twice the sizes -- every
    scratch group grows -- and at the base sizes again, on the capacity the larger run left; the work at the base sizes
    gives the same in all three."""
    base = []
    for sizes in ([1], [1, 2, 1], [1]):
        with native.Engine(0) as e:
            S._set_table(e)
            e.project_set_merges(np.array(P.MERGES, np.int32), np.array(P.PASS, np.int32))
            for scale in sizes:
                got = work(torch, native, e, scale)
                if scale == 1:
                    base.append(got)
    assert len(base) == 4 and all(b == base[0] for b in base)
