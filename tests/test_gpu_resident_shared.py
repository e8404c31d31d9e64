"""GPU: the four users of the ctx's decode scratch -- bpe_decode_batch_resident, bpe_project_resident,
bpe_token_spans_resident and the host form bpe_decode_batch -- taking turns on ONE fresh engine.  Each of them is at
least once the call that grows the scratch and at least once runs on scratch another one grew; every result is compared
with the host models of the per-family files (their tables, their helpers), and a refused id in between leaves the next
call right."""
import numpy as np
import pytest

import test_gpu_project as P
import test_gpu_spans as S

pytestmark = pytest.mark.gpu

SIZES = [1, 4095, 4096, 4097, 8193, 3]     # the seams of SCAN_TILE = 4096, then a size that shrinks
WIDTHS = ["int32", "int64"]


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def doc_of(n):
    return [0, n // 2, n]


def joined(ids):
    """(the bytes the ids decode to, the byte offset of every entry of doc_of)"""
    parts = [S.TABLE[i] for i in S.tidx_of(ids)]
    half = sum(len(p) for p in parts[:len(ids) // 2])
    return b"".join(parts), [0, half, sum(len(p) for p in parts)]


def decode_resident(torch, native, e, ids, pids, want):
    for w in WIDTHS:
        t = S.dev_ids(torch, ids, getattr(torch, w))
        d_doc = torch.tensor(doc_of(len(ids)), dtype=torch.int64, device="cuda")
        d_boff = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        out = torch.empty(len(want[0]), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        total = e.decode_batch_resident(t.data_ptr(), t.element_size(), len(ids), d_doc.data_ptr(), 3, out.data_ptr(),
                                        out.numel(), d_boff.data_ptr())
        assert total == len(want[0])
        assert out.cpu().numpy().tobytes() == want[0]
        assert d_boff.tolist() == want[1]


def project(torch, native, e, ids, pids, want):
    for w in WIDTHS:
        P.project_checked(native, torch, e, pids, getattr(torch, w), 256)


def spans(torch, native, e, ids, pids, want):
    for w in WIDTHS:
        S.spans(torch, native, e, ids, getattr(torch, w), doc=doc_of(len(ids)))


def decode_host(torch, native, e, ids, pids, want):
    got, boff = e.decode_batch(np.array(S.tidx_of(ids), np.int32), doc_of(len(ids)))
    assert got == want[0]
    assert boff.tolist() == want[1]


def refused(torch, native, e, family, ids, pids):
    """one id in the middle that the family refuses: the position comes back, nothing else happens"""
    pos = len(ids) // 2
    if family is decode_host:
        bad = np.array(S.tidx_of(ids), np.int32)
        bad[pos] = len(S.TABLE)
        with pytest.raises(native.InvalidToken) as err:
            e.decode_batch(bad)
    else:
        bad = np.array(pids if family is project else ids, dtype=np.int64)
        bad[pos] = P.TOP if family is project else S.V_DENSE
        t = S.dev_ids(torch, bad, torch.int64)
        torch.cuda.synchronize()
        with pytest.raises(native.InvalidToken) as err:
            if family is decode_resident:
                e.decode_batch_resident(t.data_ptr(), 8, len(bad), 0, 0, 0, 0, 0)
            elif family is project:
                e.project_resident(t.data_ptr(), 8, len(bad), 256)
            else:
                e.token_spans_resident(t.data_ptr(), 8, len(bad))
    assert err.value.args[0] == pos


def test_families_take_turns_on_one_scratch(torch, native):
    families = [decode_resident, project, spans, decode_host]
    with native.Engine(0) as e:
        S._set_table(e)
        e.project_set_merges(np.array(P.MERGES, np.int32), np.array(P.PASS, np.int32))
        for step, n in enumerate(SIZES):
            ids, pids = S.random_ids(n, 7000 + n), P.random_ids(n, 7000 + n)
            want = joined(ids)
            turn = families[step % 4:] + families[:step % 4]      # (the first one grows the scratch, while n grows)
            for j, family in enumerate(turn):
                family(torch, native, e, ids, pids, want)
                if j == 0:                                         # ... and is refused an id before the next one runs
                    refused(torch, native, e, family, ids, pids)
