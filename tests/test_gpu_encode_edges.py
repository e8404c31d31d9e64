"""GPU: the cases of encode_cases.py -- chunk lengths at every seam of the long-chunk tiers, a chunk cache with fewer
slots than distinct chunks, chunk counts at the tile seams of the offset scans, empty chunks, NULs and 0xFF, batches
that end at every alignment, rank tables at the 16/32-bit switch -- through every form of the batch encoder, against
oracle.encode (pinned on the same cases to the reference's loop by tests/test_encode_cases_cpu.py).  Exact equality of
the ids and of the per-chunk output offsets throughout."""
import numpy as np
import pytest

import encode_cases as ec
import oracle
from test_gpu_parity import ENC_VARIANTS

pytestmark = pytest.mark.gpu

ENC_DEFAULTS = {"enc_cache": 1, "enc_hash_bits": 0, "enc_chain": 1, "enc_long": 1}
_EXPECTED = {}


def expected(key, case):
    """oracle.encode of a case: computed once, shared by every form of the encoder"""
    if key not in _EXPECTED:
        pairs, mids, data, offs = case
        _EXPECTED[key] = oracle.encode(pairs, data, ec.oracle_offsets(data, offs), merge_ids=mids)
    return _EXPECTED[key]


def variant_options(cache, bits):
    """ENC_VARIANTS of test_gpu_parity.py as options: bits > 0 cuts the chunk hash to that many bits (every chunk takes
    the hashed list and the byte comparison), bits = -1 is the three-launch offsets + placement (enc_chain = 0)"""
    return {"enc_cache": cache, "enc_hash_bits": max(bits, 0), "enc_chain": 0 if bits < 0 else 1}


def check(engine, case, key, options):
    """engine.encode_batch under `options` == oracle.encode, ids and offsets; names the first chunk that differs"""
    pairs, mids, data, offs = case
    exp_ids, exp_off = expected(key, case)
    for k, v in options.items():
        engine.set_option(k, v)
    try:
        ids, out_off = engine.encode_batch(np.asarray(pairs, np.int32).reshape(-1, 2),
                                           None if mids is None else np.asarray(mids, np.int32), data, offs)
    finally:
        for k, v in ENC_DEFAULTS.items():
            engine.set_option(k, v)
    compare(ids, out_off, exp_ids, exp_off, data, offs, f"{key} {options}")


def compare(ids, out_off, exp_ids, exp_off, data, offs, what):
    assert len(out_off) == len(exp_off) == len(offs) + 1, what
    if not np.array_equal(out_off, exp_off):
        c = int(np.flatnonzero(np.asarray(out_off) != exp_off)[0]) - 1
        lens = np.diff(ec.oracle_offsets(data, offs).astype(np.int64))
        raise AssertionError(f"{what}: chunk {c} of {len(offs)} ({lens[c]} bytes) has {int(out_off[c + 1]) - int(out_off[c])} "
                             f"tokens, the oracle {int(exp_off[c + 1]) - int(exp_off[c])}")
    assert len(ids) == len(exp_ids), what
    if not np.array_equal(ids, exp_ids):
        p = int(np.flatnonzero(ids != exp_ids)[0])
        c = int(np.searchsorted(exp_off, p, side="right")) - 1
        s = int(exp_off[c])
        raise AssertionError(f"{what}: chunk {c} of {len(offs)} differs at its token {p - s}: "
                             f"{ids[s:s + 12].tolist()} for {exp_ids[s:s + 12].tolist()}")


# ---------------------------------------------------------------------------
# the tiers of k_enc_long

@pytest.mark.parametrize("order", ["mixed", "packed"])
@pytest.mark.parametrize("enc_long", [1, 0])
@pytest.mark.parametrize("cache", [1, 0])
@pytest.mark.parametrize("table", ["T_runs", "T_alt", "T_text"])
def test_tier_lattice(engine, table, cache, enc_long, order):
    """Chunks of 31, 32, 33 | 63, 64, 65 | 511, 512, 513 | 4095, 4096, 4097 | 9215, 9216, 9217 and 9300 bytes -- one
    below, at and one above ENC_LMAX, a ballot group and the caps of the three k_enc_long instantiations -- each as a
    run of one letter (the a == a walk across every wave), two runs that abut, abab from either letter (a site at every
    odd position, 63 | 64 and every group's end among them), inert bytes, text, and runs with a foreign byte at 63, 64
    and L - 2; with the cache and without, and with every long chunk through the stream-wide rounds (enc_long = 0)."""
    check(engine, ec.tier_lattice(table, order), ("tier_lattice", table, order), {"enc_cache": cache, "enc_long": enc_long})


@pytest.mark.parametrize("cache", [1, 0])
def test_tier_lattice_sparse_merge_ids(engine, cache):
    """the T_text lattice once more, merge r writing id 1000 + 3 r"""
    pairs, mids = ec.t_text_sparse()
    _, _, data, offs = ec.tier_lattice("T_text", "mixed")
    check(engine, (pairs, mids, data, offs), ("tier_lattice", "T_text_sparse"), {"enc_cache": cache})


def test_tier_lattice_resident(engine):
    """the T_runs lattice through bpe_encode_batch_resident: the chunks beyond ENC_LONG_TOP get their byte ranges from
    k_long_ranges"""
    torch = pytest.importorskip("torch")
    case = ec.tier_lattice("T_runs", "mixed")
    pairs, _, data, offs = case
    exp_ids, exp_off = expected(("tier_lattice", "T_runs", "mixed"), case)
    dev = torch.device("cuda", 0)
    d_bytes = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    d_offs = torch.from_numpy(offs.astype(np.int64)).to(dev)
    d_ids = torch.full((len(data),), -1, dtype=torch.int32, device=dev)
    d_ooff = torch.full((len(offs) + 1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    total = engine.encode_batch_resident(np.array(pairs, np.int32), None, d_bytes.data_ptr(), len(data), d_offs.data_ptr(),
                                         len(offs), d_ids.data_ptr(), d_ooff.data_ptr())
    assert total == len(exp_ids)
    compare(d_ids[:total].cpu().numpy(), d_ooff.cpu().numpy().astype(np.uint64), exp_ids, exp_off, data, offs, "resident")
    assert (d_ids[total:] == -1).all()  # nothing written past the batch's tokens


@pytest.mark.parametrize("cache", [1, 0])
@pytest.mark.parametrize("table", ["T_runs", "T_alt"])
def test_long_chunk_buffers_reused(engine, table, cache):
    """more chunks of the four-wave and of the sixteen-wave tier than those launches have workgroups: a workgroup's
    second chunk is encoded in the LDS buffers (tokens, ranks, flags, group counts) its first one left behind"""
    check(engine, ec.lds_reuse(table), ("lds_reuse", table), {"enc_cache": cache})


# ---------------------------------------------------------------------------
# the chunk cache, the offsets and the placement

@pytest.mark.parametrize("cache,bits", ENC_VARIANTS)
@pytest.mark.parametrize("kind", ["key", "hashed", "mixed"])
def test_cache_overflow(engine, kind, cache, bits):
    """12,000 distinct chunks for 4096 slots (24,000 for 8192 in the mix): enc_probe gives up after ENC_PROBES occupied
    slots and the chunk is encoded on its own -- 3-byte chunks in pass 1, 10-byte chunks (hashed at the full width) in
    pass 2 --, while repeats of the early chunks are served from the table"""
    check(engine, ec.cache_overflow(kind), ("cache_overflow", kind), variant_options(cache, bits))


@pytest.mark.parametrize("cache,bits", ENC_VARIANTS)
@pytest.mark.parametrize("n_chunks", ec.placement_counts())
def test_placement_tiles(engine, n_chunks, cache, bits):
    """n_chunks at a tile, a tile +- 1 and two tiles (+ 1) of the chained pass (2048) and of the three-launch form (4096),
    and 65 tiles and three chunks (the look-back passes its first group of 64; the last tile, three chunks, writes the
    total); in the batches of two tiles + 1 and in the largest, one tile holds 40 chunks of 300 tokens (more than it hands
    to the workgroup), one of exactly 256, one of 257 and one of 5000"""
    check(engine, ec.placement_tiles(n_chunks), ("placement_tiles", n_chunks), variant_options(cache, bits))


@pytest.mark.parametrize("cache,bits", ENC_VARIANTS)
def test_empty_chunks(engine, cache, bits):
    """an empty chunk first, last, five in a row, on either side of a 600-byte and of a 9300-byte chunk, and a batch
    whose only byte sits between empty chunks"""
    for label, case in ec.empties().items():
        check(engine, case, ("empties", label), variant_options(cache, bits))


@pytest.mark.parametrize("cache,bits", ENC_VARIANTS)
def test_nul_and_ff(engine, cache, bits):
    """chunks that differ only by trailing 0x00 bytes (chunk_words pads with zeros: the length alone tells them apart)
    or 0xFF bytes, behind prefixes of 1, 8, 16 and 24 bytes; all-NUL and all-0xFF chunks of 1..40 bytes; three of each"""
    check(engine, ec.nul_and_ff(), ("nul_and_ff",), variant_options(cache, bits))


@pytest.mark.parametrize("cache", [1, 0])
def test_tail_alignment(engine, cache):
    """The aligned 64-bit loads of the last chunk read up to 7 bytes past the batch, from a buffer that still holds
    an earlier, larger one: 64 KiB of 0xFF first (any of it taken for the batch's would merge with the last letter),
    then batches of every length mod 8 whose last chunk is 1, 7, 8, 9 or 32 bytes."""
    check(engine, ec.tail_prefill(), ("tail_prefill",), {"enc_cache": cache})
    for (r, last), case in ec.tail_alignment().items():
        check(engine, case, ("tail_alignment", r, last), {"enc_cache": cache})


# ---------------------------------------------------------------------------
# 16-bit or 32-bit token / rank columns

@pytest.mark.parametrize("label", list(ec.WIDTH_CASES))
def test_width_seam(engine, native, label):
    """k_encode_short<uint16_t> up to 65,280 merges without ids (the last id is 65535) and up to 65,534 with ids that
    all fit, k_encode_short<uint32_t> from one merge more or one id of 65536 on: the table's last rank fires on the
    probe, so the highest rank and the highest id go through the columns"""
    M, _, _, narrow, highest = ec.WIDTH_CASES[label]
    case = ec.width_seam(label)
    pairs, mids = case[0], case[1]
    assert len(pairs) == M
    assert native._lib.bpe_encode_uses_16bit(None if mids is None else mids.ctypes.data, M) == narrow
    exp_ids, _ = expected(("width_seam", label), case)
    assert int(exp_ids.max()) == highest
    check(engine, case, ("width_seam", label), {"enc_cache": 0})
