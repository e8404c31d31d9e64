"""Drop-in tokenizer classes backed by the MI355X engine (libbpe_hip.so).

Same public surface as karpathy/minbpe (minbpe/__init__.py:1-4): `Tokenizer`,
`BasicTokenizer`, `RegexTokenizer`, `GPT4Tokenizer`, plus the module-level
`get_stats` / `merge` helpers of minbpe/base.py:13-41.  Signatures, results,
exception types and the `.model` / `.vocab` file formats are the reference's;
the implementation is not: all pair counting, arg-max selection, merging and
encoding runs on the GPU through the C-ABI in include/bpe_hip.h.  Host Python
only does what the reference leaves to the `regex` module and to O(vocab)
bookkeeping ("out of scope as kernels").
"""
import collections
import math
import os
import unicodedata

import numpy as np
import regex as re

from . import _native

# the GPT split patterns are data (regex.py:18-19), reproduced verbatim because
# chunking must be byte-identical to the reference's
GPT2_SPLIT_PATTERN = r"""'(?:[sdmt]|ll|ve|re)| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"""
GPT4_SPLIT_PATTERN = r"""'(?i:[sdmt]|ll|ve|re)|[^\r\n\p{L}\p{N}]?+\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]++[\r\n]*|\s*[\r\n]|\s+(?!\S)|\s+"""

# compiled_pattern.pattern -> bpe_split's `which` (the scanner knows exactly these two)
_NATIVE_SPLIT = {GPT2_SPLIT_PATTERN: 2, GPT4_SPLIT_PATTERN: 4}

_engines = {}


def _default_device() -> int:
    return int(os.environ.get("MINBPE_AMD_DEVICE", os.environ.get("LOCAL_RANK", "0")))


def engine(device=None) -> "_native.Engine":
    """Process-wide engine (one ctx) per GPU, created on first use."""
    if device is None:
        device = _default_device()
    if device not in _engines:
        _engines[device] = _native.Engine(device)
    return _engines[device]


# ---------------------------------------------------------------------------
# module-level helpers (minbpe/base.py:13-41), device-backed

def get_stats(ids, counts=None):
    """Adjacent-pair counts of `ids` as a dict in first-occurrence order;
    accumulates into `counts` when given (base.py:13-22).  Ids must be below 65535, the engine's
    limit: a larger one raises RuntimeError naming that limit (there is no host path)."""
    counts = {} if counts is None else counts
    if len(ids) < 2:
        return counts
    eng = engine()
    eng.load_ids(ids)
    for pair, c, _first in eng.get_stats():
        counts[pair] = counts.get(pair, 0) + c
    return counts


def merge(ids, pair, idx):
    """Replace every left-to-right non-overlapping occurrence of `pair` in `ids`
    by `idx` (base.py:25-41).  Ids, `pair` and `idx` must be below 65535, the engine's limit: a
    larger one raises RuntimeError naming that limit (there is no host path)."""
    if len(ids) == 0:
        return []
    eng = engine()
    eng.load_ids(ids)
    eng.merge(pair, idx)
    return eng.read_ids().tolist()


# ---------------------------------------------------------------------------
# rendering helpers for the human-readable .vocab file (base.py:44-61)

def replace_control_characters(s: str) -> str:
    return "".join(ch if unicodedata.category(ch)[0] != "C" else f"\\u{ord(ch):04x}" for ch in s)


def render_token(t: bytes) -> str:
    return replace_control_characters(t.decode("utf-8", errors="replace"))


def rows_count(total, row_len, stride):
    """Rows of `row_len` elements taken every `stride` positions (1 <= stride <= row_len) from a stream of `total`
    elements, as rows_resident(mode="pack") lays them out: 0 for an empty stream, else 1 + ceil(max(total - row_len, 0)
    / stride) -- only the last row can be partial."""
    total, row_len, stride = int(total), int(row_len), int(stride)
    if row_len < 1 or not 1 <= stride <= row_len or total < 0:
        raise ValueError("rows_count needs total >= 0 and 1 <= stride <= row_len")
    if total == 0:
        return 0
    return 1 + (max(total - row_len, 0) + stride - 1) // stride


def _concat_chunks(chunks):
    """list[bytes] -> (data, start offsets) with empty chunks dropped."""
    chunks = [c for c in chunks if c]
    lens = np.fromiter((len(c) for c in chunks), dtype=np.uint64, count=len(chunks))
    offs = np.zeros(len(chunks), dtype=np.uint64)
    if len(chunks) > 1:
        np.cumsum(lens[:-1], out=offs[1:])
    return b"".join(chunks), offs


# ---------------------------------------------------------------------------
# argument handling shared by the methods over ids that live in HBM

def _cuda_device(device):
    """torch.device of one GPU from an index, a 'cuda:<index>' or None (the process-wide engine's)"""
    import torch
    if device is None:
        device = _default_device()
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    if dev.type != "cuda" or dev.index is None:
        raise ValueError("device must name one GPU: an index, or 'cuda:<index>'")
    return dev


def _host_array(ids):
    """a list or an array of integers on the host -> contiguous 1-D int64"""
    arr = np.asarray(ids)
    if arr.size and arr.dtype.kind not in "iu":
        raise TypeError("token ids must be integers")
    if arr.ndim > 1:
        raise TypeError("token ids must be a flat list or a 1-D array")
    return np.ascontiguousarray(arr.astype(np.int64, copy=False).reshape(-1))


def _check_ids(ids, dtypes, cuda=True):
    """TypeError unless `ids` is a 1-D contiguous torch tensor of one of `dtypes` on the GPU.  cuda=False leaves the last
    part out, for a method that owes its caller other errors first; it then calls again with everything."""
    import torch
    if not isinstance(ids, torch.Tensor) or (cuda and not ids.is_cuda) or ids.dim() != 1 or not ids.is_contiguous() \
            or ids.dtype not in dtypes:
        names = " or ".join(str(d).split(".")[-1] for d in dtypes)
        raise TypeError(f"ids must be a 1-D contiguous {names} torch tensor on the GPU")


def _check_doc_offsets(doc_offsets, dev, strict):
    """doc_offsets as _place_doc_offsets takes it.  A tensor must hold integers on `dev`.  strict: anything else must
    hold integers too (it comes back as an array), and there must be the n_docs + 1 >= 1 entries of a document list."""
    import torch
    if isinstance(doc_offsets, torch.Tensor):
        if doc_offsets.device != dev or doc_offsets.dtype not in (torch.int32, torch.int64):
            raise TypeError("doc_offsets must be an integer tensor on the device of ids")
        count = doc_offsets.numel()
    elif strict:
        doc_offsets = np.asarray(doc_offsets)
        if doc_offsets.size and doc_offsets.dtype.kind not in "iu":
            raise TypeError("doc_offsets must be integers")
        count = doc_offsets.size
    if strict and count < 1:
        raise ValueError("doc_offsets needs n_docs + 1 entries")
    return doc_offsets


def _place_doc_offsets(doc_offsets, dev):
    """checked doc_offsets -> flat contiguous int64 tensor on `dev`"""
    import torch
    if isinstance(doc_offsets, torch.Tensor):
        return doc_offsets.to(torch.int64).contiguous().reshape(-1)
    return torch.from_numpy(np.ascontiguousarray(doc_offsets, dtype=np.int64).reshape(-1)).to(dev)


class NgramIndex:
    """What Tokenizer.ngram_index_resident returns: the name of the n-gram index an engine holds.  ngram: the window;
    n_windows: the reference windows, repeats counted; n_distinct: the distinct ones; device: the torch.device of the GPU
    it lives on; id: the engine's number of this build.  An engine holds ONE index: the next build replaces it, and this
    object then raises RuntimeError when it is used."""
    __slots__ = ("ngram", "n_windows", "n_distinct", "device", "id")

    def __init__(self, ngram, n_windows, n_distinct, device, id):
        self.ngram, self.n_windows, self.n_distinct, self.device, self.id = ngram, n_windows, n_distinct, device, id

    def __repr__(self):
        return (f"NgramIndex(ngram={self.ngram}, n_windows={self.n_windows}, n_distinct={self.n_distinct}, "
                f"device={str(self.device)!r}, id={self.id})")


class RepetitionStats(collections.namedtuple("RepetitionStats", "length windows distinct covered top_count top_pos marks")):
    """What Tokenizer.repetition_resident returns: per document the length of the (cut) document, its windows of `ngram`
    ids, the distinct ones, the positions inside a repeated window, the multiplicity of the most frequent window and
    where it first starts; marks: a byte per id (bit 0: a repeat starts here, bit 1: covered), or None."""
    __slots__ = ()


class SpanDupStats(collections.namedtuple("SpanDupStats", "length windows seen covered first src_pos marks")):
    """What Tokenizer.duplicate_spans_resident returns: per document the length of the (cut) document, its windows of
    `ngram` ids, those of them already seen earlier in the stream, the positions inside a seen window, where in the uncut
    document the first seen window starts and the stream position at which its ids first stand (-1 without one); marks: a
    byte per id (bit 0: a seen window starts here, bit 1: covered), or None."""
    __slots__ = ()


class Segments(collections.namedtuple("Segments", "ids seg_offsets seg_doc doc_seg_offsets src_start src_end")):
    """What Tokenizer.segments_resident returns: ids, the content ids of all segments (lines) in order -- with
    tag_docs=True each preceded by one id that holds its document's number --, and seg_offsets [n_seg + 1], where each
    begins in them: together an (ids, doc_offsets) pair that every per-document method takes.  seg_doc [n_seg]: the
    segment's document; doc_seg_offsets [n_docs + 1]: the segments in the documents below; src_start, src_end [n_seg]:
    the segment's range of positions in the stream it came from -- the ranges of a document's segments tile it."""
    __slots__ = ()


class LineDupStats(collections.namedtuple("LineDupStats", "length lines dup_lines content dup_content marks")):
    """What Tokenizer.duplicate_lines_resident returns: per document its length, its lines, those of them that are
    duplicates, its content ids (the ids that belong to a line) and those of them inside a duplicate line; marks: a byte
    per id (bit 0: the id lies in the source range of a duplicate line), or None."""
    __slots__ = ()


_LINE_SPACE = b" \t\n\r\x0b\x0c"  # the six ASCII whitespace bytes (what bytes.isspace() knows)


class Tokenizer:
    """Base class: state, vocab construction, save/load (base.py:66-165)."""

    def __init__(self):
        self.merges = {}          # (int, int) -> int, insertion-ordered by idx
        self.pattern = ""
        self.special_tokens = {}  # str -> int
        self.vocab = self._build_vocab()

    def train(self, text, vocab_size, verbose=False):
        raise NotImplementedError

    def encode(self, text):
        raise NotImplementedError

    def decode(self, ids):
        raise NotImplementedError

    def _build_vocab(self):
        vocab = {i: bytes([i]) for i in range(256)}
        for (left, right), idx in self.merges.items():
            vocab[idx] = vocab[left] + vocab[right]
        for tok, idx in self.special_tokens.items():
            vocab[idx] = tok.encode("utf-8")
        return vocab

    # -- device training shared by Basic/Regex ------------------------------------
    def _train_on_device(self, data: bytes, offsets, vocab_size: int, verbose: bool, weight_exp=None):
        assert vocab_size >= 256
        num_merges = vocab_size - 256
        eng = engine()
        eng.load_bytes(data, offsets, weight_exp)
        failure = None
        try:
            res = eng.train(num_merges)
        except ValueError as e:  # stats ran empty: same exception as max() in the reference
            res, failure = eng.last_train, e
        merges, vocab = {}, {i: bytes([i]) for i in range(256)}
        for i, pair in enumerate(res["pairs"]):
            idx = 256 + i
            merges[pair] = idx
            vocab[idx] = vocab[pair[0]] + vocab[pair[1]]
            if verbose:
                print(f"merge {i+1}/{num_merges}: {pair} -> {idx} ({vocab[idx]}) had "
                      f"{res['counts'][i]} occurrences")
        if failure is not None:
            raise failure  # like the reference, merges/vocab are NOT updated
        self.merges = merges
        self.vocab = vocab

    # -- device encoding of a batch of byte chunks ----------------------------------
    def _encode_chunks(self, chunks):
        """chunks: list[bytes] -> (ids ndarray, token start offset of each
        non-empty chunk).  One device batch: K4 (bpe_encode_batch)."""
        data, offs = _concat_chunks(chunks)
        if not data:
            return np.empty(0, np.int32), np.empty(0, np.uint64)
        pairs, mids = self._merge_table()
        ids, out_off = engine().encode_batch(pairs, mids, data, offs)
        return ids, out_off[:-1]

    def _merge_table(self):
        """merges as device arrays, ordered by priority = the dict's value
        (`min(stats, key=merges.get)` in the reference, basic.py:64)."""
        # the cache holds the dict OBJECT (an id() alone can be recycled by a later dict once
        # train()/load() have dropped the old one) and its length
        key = (self.merges, len(self.merges))
        cached = getattr(self, "_mt_cache", None)
        if cached is None or cached[0][0] is not key[0] or cached[0][1] != key[1]:
            items = sorted(self.merges.items(), key=lambda kv: kv[1])
            pairs = np.array([p for p, _ in items], dtype=np.int32).reshape(-1, 2)
            mids = np.array([i for _, i in items], dtype=np.int32)
            self._mt_cache = (key, pairs, mids)
        return self._mt_cache[1], self._mt_cache[2]

    # -- device decoding of a batch of token ids ---------------------------
    def _decode_extra(self):
        """ids decode() accepts besides self.vocab: {id: str}"""
        return {}

    def _invalid_token(self, idx):
        return KeyError(idx)  # what `self.vocab[idx]` raises (basic.py:53, gpt4.py:89)

    def _finish_bytes(self, raw):
        return raw

    def _decode_table(self):
        """vocab (+ special tokens) as one dense table for the device: (blob, offsets, V,
        sparse) where ids 0..V-1 are table indices as they are and `sparse` maps every
        other known id to its index."""
        extra = self._decode_extra()
        key = (self.vocab, len(self.vocab), tuple(sorted(extra.items())))
        cached = getattr(self, "_dt_cache", None)
        if (cached is None or cached[0][0] is not key[0] or cached[0][1] != key[1]
                or cached[0][2] != key[2]):
            vocab = self.vocab
            V = 0
            while V in vocab:
                V += 1
            table = [vocab[i] for i in range(V)]
            outside = {idx: tok.encode("utf-8") for idx, tok in extra.items() if idx not in vocab}
            outside.update((idx, tok) for idx, tok in vocab.items() if not 0 <= idx < V)
            sparse = {}
            for idx in sorted(outside):  # ascending ids: the order bpe_decode_set_sparse takes them in
                sparse[idx] = len(table)
                table.append(outside[idx])
            offs = np.zeros(len(table) + 1, dtype=np.uint64)
            np.cumsum(np.fromiter((len(t) for t in table), dtype=np.uint64, count=len(table)), out=offs[1:])
            self._dt_cache = (key, b"".join(table), offs, V, sparse)
        return self._dt_cache[1:]

    def decode_batch(self, ids, doc_offsets=None):
        """The bytes decode() joins (`b"".join(vocab[idx] for idx in ids)`), produced on the
        device for a whole batch of token ids at once; not in the reference (its decode is
        a per-token Python loop).  With doc_offsets -- token positions, e.g. the start of
        every document plus len(ids) -- also returns the byte offset of each position, so
        document d is out[b[d]:b[d+1]].  Unknown ids raise what decode() raises, for the
        first such id.  Returns bytes (no UTF-8 decoding: documents are cut on bytes)."""
        arr = np.asarray(ids)
        if arr.size and arr.dtype.kind not in "iu":
            raise TypeError("token ids must be integers")
        arr = arr.astype(np.int64, copy=False).reshape(-1)
        blob, offs, V, sparse = self._decode_table()
        outside = np.flatnonzero((arr < 0) | (arr >= V))
        if len(outside):
            arr = arr.copy()
            for p in outside.tolist():
                j = sparse.get(int(arr[p]))
                if j is None:
                    raise self._invalid_token(int(arr[p]))
                arr[p] = j
        res = self._decode_engine(None, sparse=False).decode_batch(arr.astype(np.int32), doc_offsets)
        if doc_offsets is None:
            return self._finish_bytes(res)
        return self._finish_bytes(res[0]), res[1]

    def _decode_engine(self, device, sparse=True):
        """The engine of `device` with this tokenizer's decode table resident.  sparse: the table as the resident calls
        read it (_decode_table_resident) together with its sparse id list; without, the table of decode_batch, which
        resolves those ids on the host.  The table stays resident per engine: _decode_owner = (the blob uploaded, its
        sparse list is uploaded too)."""
        if sparse:
            blob, offs, V, sparse_ids = self._decode_table_resident()
        else:
            blob, offs = self._decode_table()[:2]
        eng = engine(device)
        owner = getattr(eng, "_decode_owner", (None, False))
        if owner[0] is not blob or (sparse and not owner[1]):
            eng.decode_set_vocab(blob, offs)
            if sparse:
                eng.decode_set_sparse(sparse_ids, V)
            eng._decode_owner = (blob, sparse)
        return eng

    def _resident_fill(self, ids, out, out_dtype, docs, unit, verb, native_call, count_only=False):
        """The count-then-fill protocol of decode_batch_resident and _project: out[:total], filled by
        native_call(dst pointer, dst capacity, offsets pointer, k, output offsets pointer) -> total.  out=None: sized by a
        count-only call first.  docs: (token offsets, room for the output offsets) on the device, or None.  The
        library's InvalidToken and OutputTooSmall become the caller's errors ("... <unit>, the batch <verb> to ...")."""
        import torch

        def call(dst, with_docs):
            room = (0, 0) if dst is None else (dst.data_ptr(), dst.numel())
            where = (docs[0].data_ptr(), docs[0].numel(), docs[1].data_ptr()) if with_docs else (0, 0, 0)
            try:
                return native_call(*room, *where)
            except _native.InvalidToken as e:
                raise self._invalid_token(int(ids[e.args[0]].item())) from None
            except _native.OutputTooSmall as e:
                raise ValueError(f"out holds {dst.numel()} {unit}, the batch {verb} to {e.needed}") from None

        if count_only:
            return call(None, False)
        if out is None:
            out = torch.empty(call(None, False), dtype=out_dtype, device=ids.device)
        elif out.numel() == 0 and call(None, False):  # (no room at all is a count-only call to the library)
            raise ValueError(f"out holds 0 {unit}")
        return out[:call(out, docs is not None and docs[0].numel() > 0)]

    def _resident_blob(self, blob):
        """the table bytes as the device-resident decode emits them (_finish_bytes applied to the table)"""
        return blob

    def _decode_table_resident(self):
        """_decode_table() for decode_batch_resident: (blob, offsets, V_dense, sparse_ids) -- ids 0..V_dense-1 are
        table indices as they are, sparse_ids (int32, strictly ascending) are the other known ids, the j-th being table
        entry V_dense + j; the blob already carries what _finish_bytes does to the output (a per-byte map of the
        output is the same map of the table: every output byte is a copy of a table byte)."""
        blob, offs, V, sparse = self._decode_table()
        cached = getattr(self, "_dtr_cache", None)
        if cached is None or cached[0] is not blob:
            ids = sorted(sparse, key=sparse.get)  # table order (= ascending: _decode_table)
            if any(not -2**31 <= i < 2**31 for i in ids):
                raise ValueError("decode_batch_resident needs every special token id to fit int32")
            self._dtr_cache = (blob, self._resident_blob(blob), np.array(ids, dtype=np.int32))
        return self._dtr_cache[1], offs, V, self._dtr_cache[2]

    def decode_batch_resident(self, ids, doc_offsets=None, out=None):
        """decode_batch() for token ids that live in HBM, with the bytes left in HBM: `ids` is a 1-D contiguous int32
        or int64 torch tensor on the GPU, the result a uint8 tensor there (with doc_offsets -- a tensor on the GPU or
        anything np.asarray takes -- also the int64 byte offset of each position).  Nothing but counters crosses PCIe;
        special tokens and 64-bit ids are resolved on the device.  out: a uint8 tensor on the same GPU to decode
        into (the view out[:total] is returned; ValueError if it is too small); without it the batch is measured by
        a count-only call first.  Unknown ids raise what decode() raises, for the first such id."""
        import torch
        _check_ids(ids, (torch.int32, torch.int64))
        dev = ids.device
        if out is not None and (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.uint8
                                or out.dim() != 1 or not out.is_contiguous()):
            raise TypeError("out must be a 1-D contiguous uint8 torch tensor on the device of ids")
        eng = self._decode_engine(dev.index)
        docs = None
        if doc_offsets is not None:
            doff = _place_doc_offsets(_check_doc_offsets(doc_offsets, dev, strict=False), dev)
            docs = (doff, torch.empty(doff.numel(), dtype=torch.int64, device=dev))
        torch.cuda.current_stream(dev).synchronize()  # the caller's pending writes to ids (and uploads above) are done
        res = self._resident_fill(
            ids, out, torch.uint8, docs, "bytes", "decodes",
            lambda dst, cap, d_off, k, d_boff: eng.decode_batch_resident(ids.data_ptr(), ids.element_size(), ids.numel(),
                                                                         d_off, k, dst, cap, d_boff))
        return res if doc_offsets is None else (res, docs[1])

    # -- the offset mapping of ids that live in HBM -----------------------
    _SPAN_UNITS = ("char", "byte", "both")

    def token_spans_resident(self, ids, doc_offsets=None, *, unit="char"):
        """Where every token lies in the text its document decodes to, computed on the device; not in the reference
        (whose users loop over `vocab[idx]`).  `ids` is what decode_batch_resident takes: a 1-D contiguous int32 or int64
        torch tensor on the GPU.  doc_offsets: n_docs + 1 token positions -- an integer tensor on the same GPU or anything
        np.asarray takes --, document d being ids[doc_offsets[d]:doc_offsets[d + 1]] and every span counted from its
        document's start; tokens outside every document get (-1, -1).  Without it the batch is one document.

        unit="char": an int64 [n, 2] tensor on the GPU of (start, end) in characters -- for ids that encode_ordinary made
        of a text, text[start:end] is the shortest run of characters that covers the token's bytes (the byte tokens
        that split one character all get that character; an empty token gets start == end).  unit="byte": the same in
        bytes of text.encode("utf-8").  unit="both": the pair (byte_spans, char_spans).  Unknown ids raise what decode()
        raises, for the first such id; offsets that descend or pass len(ids) raise ValueError.  Nothing but counters
        crosses PCIe."""
        import torch
        if unit not in self._SPAN_UNITS:
            raise ValueError(f"unit={unit!r} not understood: 'char', 'byte' or 'both'")
        _check_ids(ids, (torch.int32, torch.int64), cuda=False)
        dev = ids.device
        if doc_offsets is not None:
            doc_offsets = _check_doc_offsets(doc_offsets, dev, strict=True)
        _check_ids(ids, (torch.int32, torch.int64))  # (a bad doc_offsets is reported even for ids on the host)
        eng = self._decode_engine(dev.index)
        n, width = ids.numel(), ids.element_size()
        doff = None if doc_offsets is None else _place_doc_offsets(doc_offsets, dev)
        bspans = torch.empty((n, 2), dtype=torch.int64, device=dev) if unit != "char" else None
        cspans = torch.empty((n, 2), dtype=torch.int64, device=dev) if unit != "byte" else None
        torch.cuda.current_stream(dev).synchronize()  # the caller's pending writes to ids (and the upload above) are done
        try:
            eng.token_spans_resident(ids.data_ptr(), width, n, 0 if doff is None else doff.data_ptr(),
                                     0 if doff is None else doff.numel() - 1,
                                     0 if bspans is None else bspans.data_ptr(), 0 if cspans is None else cspans.data_ptr())
        except _native.InvalidToken as e:
            raise self._invalid_token(int(ids[e.args[0]].item())) from None
        return cspans if unit == "char" else bspans if unit == "byte" else (bspans, cspans)

    def token_spans(self, ids, doc_offsets=None, *, unit="char", device=None):
        """token_spans_resident() for ids on the host (a list or an array of integers): NumPy int64 [n, 2] (a pair of
        them for unit="both").  device: the GPU's index (default: the process-wide engine's)."""
        if unit not in self._SPAN_UNITS:
            raise ValueError(f"unit={unit!r} not understood: 'char', 'byte' or 'both'")
        arr = _host_array(ids)
        if doc_offsets is not None:
            doc_offsets = np.asarray(doc_offsets)
            if doc_offsets.size and doc_offsets.dtype.kind not in "iu":
                raise TypeError("doc_offsets must be integers")
        import torch
        res = self.token_spans_resident(torch.from_numpy(arr).to(_cuda_device(device)), doc_offsets, unit=unit)
        return tuple(t.cpu().numpy() for t in res) if unit == "both" else res.cpu().numpy()

    def _with_offsets(self, encode, text, unit):
        """(ids, spans) as lists: one encode plus one spans call over its ids"""
        if unit not in self._SPAN_UNITS:
            raise ValueError(f"unit={unit!r} not understood: 'char', 'byte' or 'both'")
        ids = encode(text)
        res = self.token_spans(ids, unit=unit)
        if unit == "both":
            return ids, tuple(list(map(tuple, r.tolist())) for r in res)
        return ids, list(map(tuple, res.tolist()))

    # -- what the same ids look like at a smaller vocabulary ---------------
    def _project_table(self):
        """The merge list for the device: (pairs [M, 2] int32 in id order, pass ids int32 ascending, special ids inside
        [0, 256 + M)).  ValueError unless the list has the shape training makes: merge r makes id 256 + r out of ids
        below 256 + r (a pair cannot occur twice: it is a dict key)."""
        key = (self.merges, len(self.merges), tuple(sorted(self.special_tokens.values())))
        cached = getattr(self, "_pj_cache", None)
        if cached is None or cached[0][0] is not key[0] or cached[0][1:] != key[1:]:
            items = sorted(self.merges.items(), key=lambda kv: kv[1])
            M = len(items)
            for r, ((a, b), idx) in enumerate(items):
                if idx != 256 + r or not (0 <= a < 256 + r and 0 <= b < 256 + r):
                    raise ValueError(f"merge {(a, b)} -> {idx} does not have the shape training makes: "
                                     f"merge r makes id 256 + r out of ids below it")
            pairs = np.array([p for p, _ in items], dtype=np.int32).reshape(-1, 2)
            specials = key[2]
            if any(not -2**31 <= i < 2**31 for i in specials):
                raise ValueError("projection needs every special token id to fit int32")
            pass_ids = np.array(sorted({i for i in specials if not 0 <= i < 256 + M}), dtype=np.int32)
            self._pj_cache = (key, pairs, pass_ids, [i for i in specials if 0 <= i < 256 + M])
        return self._pj_cache[1:]

    def _project_args(self, vocab_size):
        """_project_table() once vocab_size has been checked against it"""
        pairs, pass_ids, inside = self._project_table()
        top = 256 + len(pairs)
        if isinstance(vocab_size, bool) or not isinstance(vocab_size, (int, np.integer)) or not 256 <= vocab_size <= top:
            raise ValueError(f"vocab_size must be an integer in [256, {top}], not {vocab_size!r}")
        clash = [i for i in inside if i >= vocab_size]
        if clash:
            raise ValueError(f"special token id {clash[0]} lies in [{vocab_size}, {top}): the tokenizer of {vocab_size} "
                             f"entries reads it as a special token, the projection as a merge")
        return pairs, pass_ids

    def at_vocab(self, vocab_size):
        """A new tokenizer of the same class with the first vocab_size - 256 merges, the matching vocab and the same
        pattern and special tokens: the tokenizer project_resident() projects onto."""
        self._project_args(vocab_size)
        tok = type(self)()
        tok.pattern = self.pattern
        if hasattr(self, "compiled_pattern"):
            tok.compiled_pattern = self.compiled_pattern
        tok.merges = {pair: idx for pair, idx in self.merges.items() if idx < vocab_size}
        tok.vocab = {idx: b for idx, b in self.vocab.items() if not vocab_size <= idx < 256 + len(self.merges)}
        if hasattr(self, "inverse_special_tokens"):
            tok.register_special_tokens(dict(self.special_tokens))
        else:
            tok.special_tokens = dict(self.special_tokens)
        return tok

    def project_resident(self, ids, vocab_size, doc_offsets=None, out=None):
        """What at_vocab(vocab_size) makes of the text `ids` were made of, computed from the ids alone, on the device: every
        id >= vocab_size is expanded into its two children until none is left (exact: both tokenizers apply merges in
        increasing rank); special tokens pass through.  `ids` is a 1-D contiguous int32 or int64 torch tensor
        on the GPU; returns (ids', doc_offsets'): a tensor of the same dtype there, and -- with doc_offsets, token
        positions as a tensor on the GPU or anything np.asarray takes -- the int64 position of each in ids' (None
        without).  out: a tensor like ids to project into (the view out[:total] is returned; ValueError if it is too
        small); without it the batch is measured by a count-only call first.  Ids that do not project raise what
        decode() raises, for the first such id.  Nothing but counters crosses PCIe."""
        return self._project(ids, vocab_size, doc_offsets, out, False)

    def projected_count(self, ids, vocab_size):
        """len(project(ids, vocab_size)) without making the ids: the point of the compression curve at vocab_size.  ids: as
        project_resident takes them, or a list / array of integers on the host."""
        import torch
        if not isinstance(ids, torch.Tensor):
            self._project_args(vocab_size)
            ids = self._host_ids(ids)
        return self._project(ids, vocab_size, None, None, True)

    def project(self, ids, vocab_size):
        """project_resident() for ids on the host (a list or an array of integers): a list."""
        self._project_args(vocab_size)
        return self._project(self._host_ids(ids), vocab_size, None, None, False)[0].cpu().tolist()

    @staticmethod
    def _host_ids(ids):
        arr = _host_array(ids)
        import torch
        return torch.from_numpy(arr).to(_cuda_device(None))

    def _project(self, ids, vocab_size, doc_offsets, out, count_only):
        import torch
        _check_ids(ids, (torch.int32, torch.int64))
        dev = ids.device
        if out is not None and (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != ids.dtype
                                or out.dim() != 1 or not out.is_contiguous()):
            raise TypeError("out must be a 1-D contiguous torch tensor of the dtype and on the device of ids")
        if doc_offsets is not None:
            _check_doc_offsets(doc_offsets, dev, strict=False)
        pairs, pass_ids = self._project_args(vocab_size)
        eng = engine(dev.index)
        if getattr(eng, "_project_owner", None) is not pairs:  # (a new array whenever merges or special tokens changed)
            eng.project_set_merges(pairs, pass_ids)
            eng._project_owner = pairs
        docs = None
        if doc_offsets is not None:
            doff = _place_doc_offsets(doc_offsets, dev)
            docs = (doff, torch.empty(doff.numel(), dtype=torch.int64, device=dev))
        torch.cuda.current_stream(dev).synchronize()  # the caller's pending writes to ids (and uploads above) are done
        res = self._resident_fill(
            ids, out, ids.dtype, docs, "ids", "projects",
            lambda dst, cap, d_off, k, d_ooff: eng.project_resident(ids.data_ptr(), ids.element_size(), ids.numel(),
                                                                    int(vocab_size), d_off, k, dst, cap, d_ooff),
            count_only)
        return res if count_only else (res, None if docs is None else docs[1])

    # -- how often each id occurs, here and at every smaller vocabulary -----
    def count_bins(self):
        """The id each bin of a count stands for, int64 [B]: 0 .. 256 + M - 1, then the special token ids outside that
        range in ascending order."""
        pairs, pass_ids, _ = self._project_table()
        return np.concatenate([np.arange(256 + len(pairs), dtype=np.int64), pass_ids.astype(np.int64)])

    def token_counts_resident(self, ids, out=None, accumulate=False):
        """How often each id occurs in `ids`, counted on the device: an int64 tensor [B] on the device of `ids`, bin i
        standing for count_bins()[i].  `ids` is what project_resident takes: a 1-D contiguous int32 or int64 torch tensor
        on the GPU.  out: such a tensor to count into (it is returned); accumulate=True adds to what `out` holds instead
        of replacing it -- a corpus larger than HBM is counted batch by batch -- and needs `out`.  Unknown ids raise what
        decode() raises, for the first such id, and `out` is then unchanged.  Nothing but a counter crosses PCIe."""
        import torch
        _check_ids(ids, (torch.int32, torch.int64))
        dev = ids.device
        pairs, pass_ids, _ = self._project_table()
        B = 256 + len(pairs) + len(pass_ids)
        if out is not None and (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.int64
                                or out.dim() != 1 or not out.is_contiguous() or out.numel() != B):
            raise TypeError(f"out must be a 1-D contiguous int64 torch tensor of {B} bins on the device of ids")
        if accumulate and out is None:
            raise TypeError("accumulate=True needs out, the counts to add to")
        eng = engine(dev.index)
        if getattr(eng, "_project_owner", None) is not pairs:  # (shared with _project: one upload per state of the tokenizer)
            eng.project_set_merges(pairs, pass_ids)
            eng._project_owner = pairs
        if out is None:
            out = torch.empty(B, dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()  # the caller's pending writes to ids and out are done
        try:
            eng.count_resident(ids.data_ptr(), ids.element_size(), ids.numel(), out.data_ptr(), B, bool(accumulate))
        except _native.InvalidToken as e:
            raise self._invalid_token(int(ids[e.args[0]].item())) from None
        return out

    def token_counts(self, ids):
        """token_counts_resident() for ids on the host (a list or an array of integers): NumPy int64 [B]."""
        self._project_table()
        return self.token_counts_resident(self._host_ids(ids)).cpu().numpy()

    def _host_counts(self, counts):
        """counts of the calls above, or any array of B integers -> (pairs, uint64-able array [B]) on the host"""
        pairs, pass_ids, _ = self._project_table()
        if hasattr(counts, "detach") and hasattr(counts, "cpu"):  # (a torch tensor, on any device)
            counts = counts.detach().cpu().numpy()
        arr = np.asarray(counts)
        if arr.ndim != 1 or (arr.size and arr.dtype.kind not in "iu"):
            raise TypeError("counts must be a flat array of integers")
        if arr.size != 256 + len(pairs) + len(pass_ids):
            raise ValueError(f"counts holds {arr.size} bins, count_bins() has {256 + len(pairs) + len(pass_ids)}")
        return pairs, arr

    def counts_at_vocab(self, counts, vocab_size):
        """The counts at_vocab(vocab_size) would give on the same text, from the counts alone: every id >= vocab_size hands
        its count to its two children, from the last merge down (exact: DESIGN 4.7).  counts: what token_counts() or
        token_counts_resident() returned, or any array of B integers.  NumPy int64 [B]; host only."""
        self._project_args(vocab_size)
        pairs, arr = self._host_counts(counts)
        folded, _ = _native.count_fold(pairs, arr, int(vocab_size), want_curve=False)
        if len(folded) and int(folded.max()) >= 2**63:
            raise OverflowError("the folded counts pass 2^63")
        return folded.astype(np.int64)

    def compression_curve(self, counts):
        """Tokens of the counted text at every vocabulary size: NumPy int64 [M + 1], entry k = the length of what
        at_vocab(256 + k) makes of it -- projected_count() at all sizes from one histogram.  Host only."""
        self._project_args(256)
        pairs, arr = self._host_counts(counts)
        return _native.count_fold(pairs, arr, None, want_curve=True)[1]

    # -- which documents, in what order: gather, filter, shuffle -----------
    @staticmethod
    def _select_values(max_len, keep):
        """(max_len, flags) of the library from the keywords; ValueError for values it does not know"""
        if keep not in ("head", "tail"):
            raise ValueError(f"keep={keep!r} not understood: 'head' or 'tail'")
        if max_len is None:
            return 0, 0
        if isinstance(max_len, bool) or not isinstance(max_len, (int, np.integer)) or max_len < 1:
            raise ValueError("max_len must be a positive integer or None")
        return min(int(max_len), 2**64 - 1), _native.SELECT_TAIL if keep == "tail" else 0

    @staticmethod
    def _select_index(index, n_docs, dev):
        """`index` as select_docs_resident states it -> a 1-D int64 tensor on `dev` (its upload happens here), checked as
        far as that needs no look at the values: TypeError for anything but integers or a mask, or more than one
        dimension; ValueError for a mask that does not have n_docs entries."""
        import torch
        if isinstance(index, torch.Tensor):
            if index.device != dev:
                raise TypeError("index must be on the device of ids (or a sequence on the host)")
            if index.dtype not in (torch.bool, torch.int32, torch.int64):
                raise TypeError("index must hold int64 or int32 document numbers, or be a bool mask")
            if index.dim() != 1:
                raise TypeError("index must be 1-D")
            if index.dtype == torch.bool:
                if index.numel() != n_docs:
                    raise ValueError(f"the mask holds {index.numel()} entries, there are {n_docs} documents")
                return torch.nonzero(index).reshape(-1)
            return index.to(torch.int64).contiguous()
        arr = np.asarray(index)
        if arr.size and arr.dtype.kind not in "iub":
            raise TypeError("index must hold integers (or be a bool mask)")
        if arr.ndim > 1:
            raise TypeError("index must be a flat sequence or a 1-D array")
        arr = arr.reshape(-1)
        if arr.dtype.kind == "b":
            if arr.size != n_docs:
                raise ValueError(f"the mask holds {arr.size} entries, there are {n_docs} documents")
            arr = np.flatnonzero(arr)
        elif arr.dtype.kind == "u" and arr.size and int(arr.max()) >= 2**63:
            raise IndexError(f"index[{int(np.argmax(arr >= 2**63))}] names no document")
        return torch.from_numpy(np.ascontiguousarray(arr.astype(np.int64, copy=False))).to(dev)

    def select_docs_resident(self, ids, doc_offsets, index, *, max_len=None, keep="head", out=None):
        """The documents `index` names, in its order, as a new id stream, made on the device: a shuffle, a filter or a
        sample in front of rows_resident, decode_batch_resident, token_spans_resident, project_resident and the counts;
        not in the reference.  `ids` is a 1-D contiguous int32 or int64 torch tensor on the GPU, `doc_offsets` n_docs + 1
        token positions -- an integer tensor on the same GPU or anything np.asarray takes --, document d being
        ids[doc_offsets[d]:doc_offsets[d + 1]].  index: a 1-D int64 or int32 tensor on that GPU; a bool tensor of exactly
        n_docs entries there, which keeps those documents in order; or a sequence / array of integers on the host, which is
        uploaded.  Documents may repeat, come in any order and be left out; a number outside [0, n_docs) -- a negative
        one included: nothing wraps -- raises IndexError with the lowest such position.  max_len: keep at most that many
        ids of each document, its head (keep="head") or its tail (keep="tail").

        Returns (ids', doc_offsets'): the selected ids in the dtype of `ids`, and the int64 [len(index) + 1] offsets of
        the selected documents in ids', both on the GPU.  out: a tensor like ids to select into (the view out[:total] is
        returned; ValueError if it is too small); without it the selection is measured by a count-only call first.
        Offsets that descend or pass len(ids) raise ValueError.  Nothing but counters crosses PCIe."""
        import torch
        max_len, flags = self._select_values(max_len, keep)
        _check_ids(ids, (torch.int32, torch.int64), cuda=False)
        dev = ids.device
        doc_offsets = _check_doc_offsets(doc_offsets, dev, strict=True)
        n_docs = (doc_offsets.numel() if isinstance(doc_offsets, torch.Tensor) else doc_offsets.size) - 1
        if out is not None and (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != ids.dtype
                                or out.dim() != 1 or not out.is_contiguous()):
            raise TypeError("out must be a 1-D contiguous torch tensor of the dtype and on the device of ids")
        idx = self._select_index(index, n_docs, dev)
        _check_ids(ids, (torch.int32, torch.int64))
        doff = _place_doc_offsets(doc_offsets, dev)
        ooff = torch.empty(idx.numel() + 1, dtype=torch.int64, device=dev)
        eng = engine(dev.index)
        torch.cuda.current_stream(dev).synchronize()  # the caller's pending writes to ids (and uploads above) are done
        res = self._resident_fill(
            ids, out, ids.dtype, None, "ids", "selects",
            lambda dst, cap, *_: eng.select_docs_resident(ids.data_ptr(), ids.element_size(), ids.numel(), doff.data_ptr(),
                                                          n_docs, idx.data_ptr(), idx.numel(), max_len, flags, dst, cap,
                                                          ooff.data_ptr()))
        return res, ooff

    def select_docs(self, ids, doc_offsets, index, *, device=None, **kw):
        """select_docs_resident() for ids on the host (a list or an array of integers): NumPy (ids', doc_offsets'), the
        ids int32 if an int32 array came in and int64 otherwise.  device: the GPU's index (default: the process-wide
        engine's)."""
        import torch
        self._select_values(kw.get("max_len"), kw.get("keep", "head"))
        if kw.get("out") is not None:
            raise TypeError("select_docs makes its own output")
        arr = np.asarray(ids)
        arr = np.ascontiguousarray(arr) if arr.dtype == np.int32 and arr.ndim == 1 else _host_array(ids)
        doc_offsets = _check_doc_offsets(doc_offsets, torch.device("cpu"), strict=True)
        if isinstance(doc_offsets, torch.Tensor):
            doc_offsets = doc_offsets.numpy()
        # (its errors, before a device is named; a mask is resolved here, on the host)
        index = self._select_index(index, doc_offsets.size - 1, torch.device("cpu")).numpy()
        res, ooff = self.select_docs_resident(torch.from_numpy(arr).to(_cuda_device(device)), doc_offsets, index, **kw)
        return res.cpu().numpy(), ooff.cpu().numpy()

    # -- which documents are copies of an earlier one ----------------------
    @property
    def n_distinct_docs(self):
        """The number of distinct documents the last duplicate_docs_resident() / unique_docs_resident() of this
        tokenizer found (and their host forms); None before the first.  Read-only: it came back as a counter."""
        return getattr(self, "_n_distinct_docs", None)

    def duplicate_docs_resident(self, ids, doc_offsets, *, max_len=None, keep="head", return_counts=False):
        """For every document the number of its first copy, found on the device: first[d] = the lowest e whose document
        equals document d -- the same length and the same ids at their full width; not in the reference.  first[d] <= d,
        first[first] == first, and first == arange(n_docs) is the mask "keep one copy of each" that select_docs_resident
        takes.  `ids` and `doc_offsets` are what select_docs_resident takes.  max_len / keep: documents are compared by
        what select_docs_resident would emit for them with the same values -- their first (keep="head") or last
        (keep="tail") max_len ids.  Exact: a hash only chooses where to look, every equality is established by
        comparing the ids; the result does not depend on scheduling.

        Returns first, an int64 tensor [n_docs] on the device of `ids`; with return_counts=True (first, counts), counts
        int64 [n_docs]: the number of copies at every d with first[d] == d and 0 elsewhere.  n_distinct_docs then holds
        the number of distinct documents.  Offsets that descend or pass len(ids) raise ValueError.  Nothing but counters
        crosses PCIe."""
        first, counts, self._n_distinct_docs = self._duplicate_docs(ids, doc_offsets, max_len, keep, return_counts)
        return (first, counts) if return_counts else first

    def _duplicate_docs(self, ids, doc_offsets, max_len=None, keep="head", return_counts=False):
        """duplicate_docs_resident() without its counter: (first, counts or None, the number of distinct documents) --
        for the methods that run it on a stream of their own making and owe the caller no n_distinct_docs"""
        import torch
        max_len, flags = self._select_values(max_len, keep)
        _check_ids(ids, (torch.int32, torch.int64), cuda=False)
        dev = ids.device
        doc_offsets = _check_doc_offsets(doc_offsets, dev, strict=True)
        _check_ids(ids, (torch.int32, torch.int64))
        doff = _place_doc_offsets(doc_offsets, dev)
        n_docs = doff.numel() - 1
        first = torch.empty(n_docs, dtype=torch.int64, device=dev)
        counts = torch.empty(n_docs, dtype=torch.int64, device=dev) if return_counts else None
        eng = engine(dev.index)
        torch.cuda.current_stream(dev).synchronize()  # the caller's pending writes to ids (and the upload above) are done
        n_distinct = eng.dup_docs_resident(ids.data_ptr(), ids.element_size(), ids.numel(), doff.data_ptr(), n_docs, max_len,
                                           flags, first.data_ptr(), counts.data_ptr() if return_counts else 0)
        return first, counts, n_distinct

    def unique_docs_resident(self, ids, doc_offsets, *, max_len=None, keep="head", out=None):
        """One copy of every document, the first, in the order of the stream: duplicate_docs_resident() and
        select_docs_resident() over first == arange in one call.  Returns (ids', doc_offsets', index, counts): the id
        stream of the kept documents and its offsets as select_docs_resident returns them, index int64 [k] the kept
        document numbers and counts int64 [k] how many copies each had, all on the device of `ids`.  With max_len the
        kept documents are cut the same way they were compared.  out: as in select_docs_resident."""
        import torch
        first, counts = self.duplicate_docs_resident(ids, doc_offsets, max_len=max_len, keep=keep, return_counts=True)
        index = torch.nonzero(first == torch.arange(first.numel(), dtype=torch.int64, device=first.device)).reshape(-1)
        res, ooff = self.select_docs_resident(ids, doc_offsets, index, max_len=max_len, keep=keep, out=out)
        return res, ooff, index, counts[index]

    def _host_docs(self, ids, doc_offsets, device, kw):
        """the arguments of duplicate_docs / unique_docs, checked before a device is named -> (ids on the GPU, offsets)"""
        import torch
        self._select_values(kw.get("max_len"), kw.get("keep", "head"))
        arr, doc_offsets = self._host_stream(ids, doc_offsets)
        return torch.from_numpy(arr).to(_cuda_device(device)), doc_offsets

    @staticmethod
    def _host_stream(ids, doc_offsets):
        """ids and offsets on the host, checked -> (contiguous int32 or int64 array, offsets); no device is named"""
        import torch
        arr = np.asarray(ids)
        arr = np.ascontiguousarray(arr) if arr.dtype == np.int32 and arr.ndim == 1 else _host_array(ids)
        doc_offsets = _check_doc_offsets(doc_offsets, torch.device("cpu"), strict=True)
        if isinstance(doc_offsets, torch.Tensor):
            doc_offsets = doc_offsets.numpy()
        return arr, doc_offsets

    def duplicate_docs(self, ids, doc_offsets, *, device=None, **kw):
        """duplicate_docs_resident() for ids on the host (a list or an array of integers; an int32 array is compared as
        int32, anything else as int64): NumPy first, or (first, counts).  device: the GPU's index (default: the
        process-wide engine's)."""
        d_ids, doc_offsets = self._host_docs(ids, doc_offsets, device, kw)
        res = self.duplicate_docs_resident(d_ids, doc_offsets, **kw)
        return tuple(t.cpu().numpy() for t in res) if isinstance(res, tuple) else res.cpu().numpy()

    def unique_docs(self, ids, doc_offsets, *, device=None, **kw):
        """unique_docs_resident() for ids on the host: NumPy (ids', doc_offsets', index, counts), the ids int32 if an
        int32 array came in and int64 otherwise."""
        if kw.get("out") is not None:
            raise TypeError("unique_docs makes its own output")
        d_ids, doc_offsets = self._host_docs(ids, doc_offsets, device, kw)
        return tuple(t.cpu().numpy() for t in self.unique_docs_resident(d_ids, doc_offsets, **kw))

    # -- which documents are nearly copies of an earlier one --------------
    @staticmethod
    def _minhash_values(n_perm, ngram):
        """ValueError for a number of permutations or a window the library does not take"""
        for name, v, hi in (("n_perm", n_perm, 1024), ("ngram", ngram, 64)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= hi:
                raise ValueError(f"{name} must be an integer from 1 to {hi}")
        return int(n_perm), int(ngram)

    @staticmethod
    def _minhash_seed(seed):
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2**64:
            raise ValueError("seed must be an integer from 0 to 2^64 - 1")
        return int(seed)

    def minhash_resident(self, ids, doc_offsets, *, n_perm=128, ngram=5, seed=0, max_len=None, keep="head", out=None):
        """The MinHash signature of every document, made on the device; not in the reference.  `ids` and `doc_offsets`
        are what select_docs_resident takes.  A document is the set of its windows of `ngram` consecutive ids (one shorter
        than the window: the one window that is all of it); row d of the result holds, for each of n_perm hash functions
        made from `seed`, the smallest hash among document d's windows, so that the share of positions at which two rows
        agree estimates the Jaccard similarity of the two sets (standard error about sqrt(J (1 - J) / n_perm)).  An
        int32 id and the int64 id of the same value hash alike.  max_len / keep: documents are cut as
        select_docs_resident cuts them with the same values.  n_perm 1..1024, ngram 1..64.  The definition is in
        include/bpe_hip.h; the result does not depend on scheduling.

        Returns sig, an int32 tensor [n_docs, n_perm] on the device of `ids`; a document without ids is a row of
        0x7FFFFFFF.  out: a contiguous int32 tensor of at least n_docs * n_perm elements on the same GPU to write into
        (the view of the rows written is returned; ValueError if it is too small).  Offsets that descend or pass
        len(ids) raise ValueError.  Nothing but the hash parameters and counters crosses PCIe."""
        import torch
        max_len, flags = self._select_values(max_len, keep)
        n_perm, ngram = self._minhash_values(n_perm, ngram)
        seed = self._minhash_seed(seed)
        _check_ids(ids, (torch.int32, torch.int64), cuda=False)
        dev = ids.device
        doc_offsets = _check_doc_offsets(doc_offsets, dev, strict=True)
        n_docs = (doc_offsets.numel() if isinstance(doc_offsets, torch.Tensor) else doc_offsets.size) - 1
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.int32 or not out.is_contiguous():
                raise TypeError("out must be a contiguous int32 torch tensor on the device of ids")
            if out.numel() < n_docs * n_perm:
                raise ValueError(f"out holds {out.numel()} elements, the signatures need {n_docs * n_perm}")
        _check_ids(ids, (torch.int32, torch.int64))
        doff = _place_doc_offsets(doc_offsets, dev)
        if out is None:
            out = torch.empty(n_docs * n_perm, dtype=torch.int32, device=dev)
        eng = engine(dev.index)
        torch.cuda.current_stream(dev).synchronize()  # the caller's pending writes to ids (and the upload above) are done
        eng.minhash_resident(ids.data_ptr(), ids.element_size(), ids.numel(), doff.data_ptr(), n_docs, max_len, flags,
                             ngram, n_perm, seed, out.data_ptr(), out.numel())
        return out.reshape(-1)[:n_docs * n_perm].view(n_docs, n_perm)

    def minhash(self, ids, doc_offsets, *, device=None, **kw):
        """minhash_resident() for ids on the host (a list or an array of integers; an int32 array goes up as int32,
        anything else as int64 -- the signatures are the same): NumPy int32 [n_docs, n_perm].  device: the GPU's index
        (default: the process-wide engine's)."""
        self._minhash_values(kw.get("n_perm", 128), kw.get("ngram", 5))
        self._minhash_seed(kw.get("seed", 0))
        if kw.get("out") is not None:
            raise TypeError("minhash makes its own output")
        d_ids, doc_offsets = self._host_docs(ids, doc_offsets, device, kw)
        return self.minhash_resident(d_ids, doc_offsets, **kw).cpu().numpy()

    def minhash_agreement_resident(self, sig, a, b):
        """At how many positions rows a[j] and b[j] of a signature matrix agree, counted on the device: int32 [m];
        divided by n_perm, the estimate of the two documents' Jaccard similarity.  `sig` is what minhash_resident
        returned (a contiguous int32 [n_docs, n_perm] tensor on the GPU); a and b are equally long 1-D int64 or int32
        tensors on that GPU, or sequences of integers on the host, which are uploaded.  An index outside [0, n_docs) --
        a negative one included: nothing wraps -- raises IndexError with the lowest such position."""
        import torch
        if not isinstance(sig, torch.Tensor) or sig.dim() != 2 or sig.dtype != torch.int32 or not sig.is_contiguous():
            raise TypeError("sig must be a contiguous int32 [n_docs, n_perm] torch tensor on the GPU")
        n_docs, n_perm = sig.shape
        self._minhash_values(n_perm, 1)
        dev = sig.device
        pairs = [self._select_index(x, n_docs, dev) if not (isinstance(x, torch.Tensor) and x.dtype == torch.bool)
                 else None for x in (a, b)]
        if pairs[0] is None or pairs[1] is None:
            raise TypeError("a and b must hold int64 or int32 document numbers")
        if pairs[0].numel() != pairs[1].numel():
            raise ValueError(f"a holds {pairs[0].numel()} documents and b {pairs[1].numel()}")
        if not sig.is_cuda:
            raise TypeError("sig must be a contiguous int32 [n_docs, n_perm] torch tensor on the GPU")
        agree = torch.empty(pairs[0].numel(), dtype=torch.int32, device=dev)
        eng = engine(dev.index)
        torch.cuda.current_stream(dev).synchronize()  # the caller's pending writes to sig (and the uploads above) are done
        eng.minhash_agree_resident(sig.data_ptr(), n_docs, n_perm, pairs[0].data_ptr(), pairs[1].data_ptr(),
                                   pairs[0].numel(), agree.data_ptr())
        return agree

    @staticmethod
    def _near_values(threshold, n_perm, bands):
        """(rows per band, agreeing positions needed) from the keywords; ValueError for values that make no banding"""
        if isinstance(bands, bool) or not isinstance(bands, (int, np.integer)) or bands < 1 or n_perm % bands:
            raise ValueError("bands must be a positive integer that divides n_perm")
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) \
                or not 0 < threshold <= 1:
            raise ValueError("threshold must be a number in (0, 1]")
        return n_perm // int(bands), int(math.ceil(float(threshold) * n_perm))

    def near_duplicate_docs_resident(self, ids, doc_offsets, *, threshold=0.8, n_perm=128, bands=32, ngram=5, seed=0,
                                     max_len=None, keep="head", return_signatures=False):
        """For every document the lowest document number of its group of near-duplicates, found on the device: MinHash
        signatures (minhash_resident), locality-sensitive banding, verification, connected components; not in the
        reference.  The signature is cut into `bands` bands of n_perm / bands positions.  In every band a document is a
        candidate for the FIRST document whose band equals its own (duplicate_docs_resident on the signatures), and the
        two are joined if their whole signatures agree at ceil(threshold * n_perm) positions or more
        (minhash_agreement_resident); first[d] is the lowest document of d's connected component.  A candidate is verified
        against the first document of its bucket only: that is the definition.  Documents without ids form one group.
        first[d] <= d, first[first] == first, and first == arange(n_docs) is the mask "keep one document of each group"
        that select_docs_resident takes.  Exact copies are always in one group, so the result is coarser than or equal
        to duplicate_docs_resident's.  The other arguments are minhash_resident's; n_docs * n_perm must stay below 2^32.

        Returns first, an int64 tensor [n_docs] on the device of `ids`; with return_signatures=True (first, sig).
        n_distinct_docs then holds the number of groups.  Nothing but hash parameters and counters crosses PCIe."""
        import torch
        max_len_v, _ = self._select_values(max_len, keep)
        n_perm, ngram = self._minhash_values(n_perm, ngram)
        seed = self._minhash_seed(seed)
        rows, need = self._near_values(threshold, n_perm, bands)
        _check_ids(ids, (torch.int32, torch.int64), cuda=False)
        dev = ids.device
        doc_offsets = _check_doc_offsets(doc_offsets, dev, strict=True)
        n_docs = (doc_offsets.numel() if isinstance(doc_offsets, torch.Tensor) else doc_offsets.size) - 1
        if n_docs * n_perm >= 2**32:
            raise ValueError(f"{n_docs} documents of {n_perm} positions: the signatures must stay below 2^32 words")
        _check_ids(ids, (torch.int32, torch.int64))
        sig = self.minhash_resident(ids, doc_offsets, n_perm=n_perm, ngram=ngram, seed=seed, max_len=max_len, keep=keep)
        arange = torch.arange(n_docs, dtype=torch.int64, device=dev)
        flat = sig.view(-1)
        band_off = torch.arange(n_docs + 1, dtype=torch.int64, device=dev) * n_perm
        labels = arange.clone()
        edges_a, edges_b = [], []
        for band in range(n_perm // rows):
            # document d of this stream is sig[d, band * rows : (band + 1) * rows] and nothing else
            off_b = torch.clamp(band_off + band * rows, max=n_docs * n_perm)
            first_b = self.duplicate_docs_resident(flat, off_b, max_len=rows)
            cand = torch.nonzero(first_b != arange).reshape(-1)
            if cand.numel() == 0:
                continue
            rep = first_b[cand]
            ok = self.minhash_agreement_resident(sig, cand, rep) >= need
            edges_a.append(cand[ok])
            edges_b.append(rep[ok])
        if edges_a:
            ea, eb = torch.cat(edges_a), torch.cat(edges_b)
            # min-label propagation with pointer jumping: a label only ever decreases and names a document of the same
            # component, so this ends, at the component's lowest document
            while ea.numel():
                low = torch.minimum(labels[ea], labels[eb])
                new = labels.clone()
                new.scatter_reduce_(0, ea, low, "amin")
                new.scatter_reduce_(0, eb, low, "amin")
                new = new[new]
                if torch.equal(new, labels):
                    break
                labels = new
        self._n_distinct_docs = int((labels == arange).sum())
        return (labels, sig) if return_signatures else labels

    def near_duplicate_docs(self, ids, doc_offsets, *, device=None, **kw):
        """near_duplicate_docs_resident() for ids on the host (a list or an array of integers): NumPy first, or
        (first, sig).  device: the GPU's index (default: the process-wide engine's)."""
        n_perm, _ = self._minhash_values(kw.get("n_perm", 128), kw.get("ngram", 5))
        self._minhash_seed(kw.get("seed", 0))
        self._near_values(kw.get("threshold", 0.8), n_perm, kw.get("bands", 32))
        d_ids, doc_offsets = self._host_docs(ids, doc_offsets, device, kw)
        res = self.near_duplicate_docs_resident(d_ids, doc_offsets, **kw)
        return tuple(t.cpu().numpy() for t in res) if isinstance(res, tuple) else res.cpu().numpy()

    # -- which documents share a window with a held-out set --------------
    @property
    def n_overlapping_docs(self):
        """The number of documents with a hit that the last ngram_overlap_resident() / decontaminate_docs_resident() of
        this tokenizer found (and their host forms); None before the first.  Read-only: it came back as a counter."""
        return getattr(self, "_n_overlapping_docs", None)

    @staticmethod
    def _ngram_value(ngram):
        if isinstance(ngram, bool) or not isinstance(ngram, (int, np.integer)) or not 1 <= ngram <= 64:
            raise ValueError("ngram must be an integer from 1 to 64")
        return int(ngram)

    def ngram_index_resident(self, ref_ids, ref_doc_offsets=None, *, ngram=13):
        """The index of a held-out set -- benchmarks, eval splits, a block list -- that ngram_overlap_resident looks a
        corpus up in, made on the device; not in the reference.  `ref_ids` is a 1-D contiguous int32 or int64 torch
        tensor on the GPU, `ref_doc_offsets` its n_ref_docs + 1 token positions as select_docs_resident takes them (None:
        one document, all of ref_ids).  Every run of `ngram` consecutive ids inside one reference document is a
        reference window; a document shorter than that contributes none.  The engine of that GPU keeps its own copy of
        the ids and ONE index: this one replaces the one before, whose NgramIndex then raises RuntimeError when used.
        Returns an NgramIndex (ngram, n_windows, n_distinct, device, id).  Offsets that descend or pass len(ref_ids)
        raise ValueError.  Nothing but counters crosses PCIe."""
        import torch
        ngram = self._ngram_value(ngram)
        _check_ids(ref_ids, (torch.int32, torch.int64), cuda=False)
        dev = ref_ids.device
        if ref_doc_offsets is None:
            ref_doc_offsets = np.array([0, ref_ids.numel()], np.int64)
        ref_doc_offsets = _check_doc_offsets(ref_doc_offsets, dev, strict=True)
        _check_ids(ref_ids, (torch.int32, torch.int64))
        roff = _place_doc_offsets(ref_doc_offsets, dev)
        eng = engine(dev.index)
        torch.cuda.current_stream(dev).synchronize()  # the caller's pending writes to ref_ids (and the upload above) are done
        iid, n_windows, n_distinct = eng.ngram_index_resident(ref_ids.data_ptr(), ref_ids.element_size(), ref_ids.numel(),
                                                              roff.data_ptr(), roff.numel() - 1, ngram)
        return NgramIndex(ngram, n_windows, n_distinct, dev, iid)

    def ngram_index(self, ref_ids, ref_doc_offsets=None, *, ngram=13, device=None):
        """ngram_index_resident() for reference ids on the host (a list or an array of integers; an int32 array goes up
        as int32, anything else as int64 -- the index is the same).  device: the GPU's index (default: the process-wide
        engine's)."""
        import torch
        self._ngram_value(ngram)
        arr, ref_doc_offsets = self._host_reference(ref_ids, ref_doc_offsets)
        return self.ngram_index_resident(torch.from_numpy(arr).to(_cuda_device(device)), ref_doc_offsets, ngram=ngram)

    def _host_reference(self, ref_ids, ref_doc_offsets):
        """_host_stream of a reference, whose offsets may be None: one document"""
        if ref_doc_offsets is None:
            ref_doc_offsets = [0, int(np.asarray(ref_ids).size)]
        return self._host_stream(ref_ids, ref_doc_offsets)

    @staticmethod
    def _ngram_index_on(index, dev):
        """ValueError unless `index` (an NgramIndex: checked) was made on `dev`"""
        if index.device != dev:
            raise ValueError(f"the index was made on {index.device}, the ids are on {dev}")

    def ngram_overlap_resident(self, index, ids, doc_offsets, *, max_len=None, keep="head", return_first=False,
                               return_starts=False):
        """How many windows of every document also occur in a held-out set, counted on the device: hits[d] = the
        positions k of document d at which the index.ngram ids d[k : k + ngram] equal, by value, a window of the
        reference `index` was made from (ngram_index_resident); not in the reference.  `ids` and `doc_offsets` are what
        select_docs_resident takes; an int32 corpus may be looked up in an index of int64 ids and the reverse.  max_len /
        keep: documents are cut as select_docs_resident cuts them with the same values, and a window lies inside the cut.
        A document shorter than ngram has no window.  Exact: a hash only chooses where to look, every equality is
        established by comparing the ids; the result does not depend on scheduling.

        Returns hits, an int64 tensor [n_docs] on the device of `ids`; with return_first=True (hits, first, ref_pos):
        first[d] the position inside the uncut document d at which its first hit starts -- it indexes what
        token_spans_resident returns --, ref_pos[d] the lowest position of the reference at which that window starts, both
        -1 where hits is 0; with return_starts=True also a uint8 tensor [len(ids)] that is 1 where a hit window starts.
        n_overlapping_docs then holds the number of documents with a hit.  Offsets that descend or pass len(ids) raise
        ValueError, an index that is no longer its engine's current one RuntimeError.  Nothing but counters crosses PCIe."""
        import torch
        max_len, flags = self._select_values(max_len, keep)
        if not isinstance(index, NgramIndex):
            raise TypeError("index must be an NgramIndex (what ngram_index_resident returns)")
        _check_ids(ids, (torch.int32, torch.int64), cuda=False)
        dev = ids.device
        doc_offsets = _check_doc_offsets(doc_offsets, dev, strict=True)
        self._ngram_index_on(index, dev)
        _check_ids(ids, (torch.int32, torch.int64))
        doff = _place_doc_offsets(doc_offsets, dev)
        n_docs = doff.numel() - 1
        hits = torch.empty(n_docs, dtype=torch.int64, device=dev)
        first = torch.empty(n_docs, dtype=torch.int64, device=dev) if return_first else None
        ref_pos = torch.empty(n_docs, dtype=torch.int64, device=dev) if return_first else None
        starts = torch.empty(ids.numel(), dtype=torch.uint8, device=dev) if return_starts else None
        eng = engine(dev.index)
        torch.cuda.current_stream(dev).synchronize()  # the caller's pending writes to ids (and the upload above) are done
        self._n_overlapping_docs = eng.ngram_overlap_resident(
            index.id, ids.data_ptr(), ids.element_size(), ids.numel(), doff.data_ptr(), n_docs, max_len, flags,
            hits.data_ptr(), first.data_ptr() if return_first else 0, ref_pos.data_ptr() if return_first else 0,
            starts.data_ptr() if return_starts else 0)
        res = (hits, first, ref_pos) if return_first else (hits,)
        if return_starts:
            res += (starts,)
        return res if len(res) > 1 else hits

    def ngram_overlap(self, index_or_ref, ids, doc_offsets, *, device=None, ngram=13, ref_doc_offsets=None, **kw):
        """ngram_overlap_resident() for ids on the host (a list or an array of integers): NumPy hits, or the tuple.
        index_or_ref: an NgramIndex, or the reference ids on the host, of which an index is made first (ngram,
        ref_doc_offsets: as in ngram_index; they are not looked at when an NgramIndex comes in).  device: the GPU's
        index (default: the process-wide engine's)."""
        import torch
        self._select_values(kw.get("max_len"), kw.get("keep", "head"))
        ref = None
        if not isinstance(index_or_ref, NgramIndex):
            self._ngram_value(ngram)
            ref = self._host_reference(index_or_ref, ref_doc_offsets)
        arr, doc_offsets = self._host_stream(ids, doc_offsets)
        dev = _cuda_device(device)
        if ref is None:
            self._ngram_index_on(index_or_ref, dev)
        else:
            index_or_ref = self.ngram_index_resident(torch.from_numpy(ref[0]).to(dev), ref[1], ngram=ngram)
        res = self.ngram_overlap_resident(index_or_ref, torch.from_numpy(arr).to(dev), doc_offsets, **kw)
        return tuple(t.cpu().numpy() for t in res) if isinstance(res, tuple) else res.cpu().numpy()

    def decontaminate_docs_resident(self, index, ids, doc_offsets, *, min_hits=1, max_len=None, keep="head", out=None):
        """The documents that share fewer than `min_hits` windows with a held-out set, in the order of the stream:
        ngram_overlap_resident() and select_docs_resident() over hits < min_hits in one call.  Returns (ids',
        doc_offsets', kept, hits): the id stream of the kept documents and its offsets as select_docs_resident returns
        them, kept int64 [k] the kept document numbers and hits int64 [n_docs] the hits of ALL documents, all on the
        device of `ids`.  With max_len the kept documents are cut the same way they were looked up.  out: as in
        select_docs_resident."""
        import torch
        if isinstance(min_hits, bool) or not isinstance(min_hits, (int, np.integer)) or min_hits < 1:
            raise ValueError("min_hits must be a positive integer")
        _check_ids(ids, (torch.int32, torch.int64), cuda=False)
        if out is not None and (not isinstance(out, torch.Tensor) or out.device != ids.device or out.dtype != ids.dtype
                                or out.dim() != 1 or not out.is_contiguous()):
            raise TypeError("out must be a 1-D contiguous torch tensor of the dtype and on the device of ids")
        hits = self.ngram_overlap_resident(index, ids, doc_offsets, max_len=max_len, keep=keep)
        kept = torch.nonzero(hits < int(min_hits)).reshape(-1)
        res, ooff = self.select_docs_resident(ids, doc_offsets, kept, max_len=max_len, keep=keep, out=out)
        return res, ooff, kept, hits

    # -- repeated n-grams inside each document ----------------------------
    @property
    def n_repetitive_docs(self):
        """The number of documents that the last repetitive_docs_resident() / drop_repetitive_docs_resident() of this
        tokenizer flagged; None before the first."""
        return getattr(self, "_n_repetitive_docs", None)

    @staticmethod
    def _repetition_rules(top, dup):
        """the rule lists of repetitive_docs_resident -> ((w, t), ...) twice, checked; ValueError for anything else"""
        out = []
        for name, rules in (("top", top), ("dup", dup)):
            try:
                rules = tuple(tuple(r) for r in rules)
            except TypeError:
                raise ValueError(f"{name} must be a sequence of (ngram, threshold) pairs") from None
            for r in rules:
                if len(r) != 2:
                    raise ValueError(f"{name} must be a sequence of (ngram, threshold) pairs")
                w, t = r
                if isinstance(w, bool) or not isinstance(w, (int, np.integer)) or not 1 <= w <= 64:
                    raise ValueError(f"{name}: an ngram must be an integer from 1 to 64")
                if isinstance(t, bool) or not isinstance(t, (int, float, np.integer, np.floating)) or not t >= 0 \
                        or t == float("inf"):
                    raise ValueError(f"{name}: a threshold must be a real number >= 0")
            out.append(tuple((int(w), float(t)) for w, t in rules))
        if not out[0] and not out[1]:
            raise ValueError("top and dup are both empty: no rule")
        return out[0], out[1]

    @staticmethod
    def _repetition_flags(stats, top, dup):
        """the rule of repetitive_docs_resident on stats = {w: RepetitionStats}: bool [n_docs], both sides in float64"""
        import torch
        length = next(iter(stats.values())).length
        flagged = torch.zeros(length.numel(), dtype=torch.bool, device=length.device)
        flen = length.to(torch.float64)
        for rules, column in ((top, "top_count"), (dup, "covered")):
            for w, t in rules:
                lhs = getattr(stats[w], column)
                lhs = (lhs * w if column == "top_count" else lhs).to(torch.float64)
                flagged |= lhs > t * flen
        flagged &= length > 0
        return flagged

    def repetition_resident(self, ids, doc_offsets, *, ngram=5, max_len=None, keep="head", return_marks=False):
        """How much of every document repeats itself, counted on the device: the statistics of the windows of `ngram`
        consecutive ids of each document that occur more than once inside that SAME document -- what the repetition
        filters of the Gopher / MassiveText rules are made of; not in the reference.  `ids` and `doc_offsets` are what
        select_docs_resident takes.  max_len / keep: documents are cut as select_docs_resident cuts them with the same
        values, and a window lies inside the cut; a document shorter than ngram has no window.  A window that equals
        one starting earlier in the document is a repeat.  Exact: a hash only chooses where to look, every equality is
        established by comparing the ids at their full width; the result does not depend on scheduling.

        Returns a RepetitionStats of int64 tensors [n_docs] on the device of `ids`: length (of the cut document), windows,
        distinct (windows - repeats), covered (the positions that lie inside a window at a repeat), top_count (the
        largest multiplicity of a window, 0 without one), top_pos (where in the uncut document the lowest window of
        that multiplicity starts, -1 without one); marks is None, or with return_marks=True a uint8 tensor [len(ids)]:
        bit 0 where a repeat starts, bit 1 where the position is covered.  Offsets that descend or pass len(ids) raise
        ValueError.  Nothing but counters crosses PCIe."""
        return self._repetition(ids, doc_offsets, ngram, max_len, keep, return_marks)[0]

    def _repetition(self, ids, doc_offsets, ngram, max_len, keep, return_marks, columns=None, doff=None):
        """(RepetitionStats, n_repeat_docs, the offsets on the device); columns: the fields wanted (None: all)"""
        import torch
        ngram = self._ngram_value(ngram)
        max_len, flags = self._select_values(max_len, keep)
        _check_ids(ids, (torch.int32, torch.int64), cuda=False)
        dev = ids.device
        if doff is None:
            doc_offsets = _check_doc_offsets(doc_offsets, dev, strict=True)
        _check_ids(ids, (torch.int32, torch.int64))
        if doff is None:
            doff = _place_doc_offsets(doc_offsets, dev)
        n_docs = doff.numel() - 1
        names = RepetitionStats._fields[:6]
        cols = {name: torch.empty(n_docs, dtype=torch.int64, device=dev) if columns is None or name in columns else None
                for name in names}
        marks = torch.empty(ids.numel(), dtype=torch.uint8, device=dev) if return_marks else None
        eng = engine(dev.index)
        torch.cuda.current_stream(dev).synchronize()  # the caller's pending writes to ids (and the upload above) are done
        n_rep = eng.repeat_stats_resident(ids.data_ptr(), ids.element_size(), ids.numel(), doff.data_ptr(), n_docs, ngram,
                                          max_len, flags, *[0 if cols[name] is None else cols[name].data_ptr() for name in names],
                                          marks.data_ptr() if return_marks else 0)
        return RepetitionStats(*[cols[name] for name in names], marks), n_rep, doff

    def repetition(self, ids, doc_offsets, *, device=None, ngram=5, **kw):
        """repetition_resident() for ids on the host (a list or an array of integers; an int32 array goes up as int32,
        anything else as int64): a RepetitionStats of NumPy arrays.  device: the GPU's index (default: the process-wide
        engine's)."""
        self._ngram_value(ngram)
        d_ids, doc_offsets = self._host_docs(ids, doc_offsets, device, kw)
        res = self.repetition_resident(d_ids, doc_offsets, ngram=ngram, **kw)
        return RepetitionStats(*[None if t is None else t.cpu().numpy() for t in res])

    def repetitive_docs_resident(self, ids, doc_offsets, *, top=((2, .20), (3, .18), (4, .16)),
                                 dup=((5, .15), (6, .14), (7, .13), (8, .12), (9, .11), (10, .10)), max_len=None,
                                 keep="head"):
        """The documents the repetition filters of the Gopher / MassiveText rules drop, found on the device: flagged, a
        bool tensor [n_docs] on the device of `ids`.  A document is flagged if for some (w, t) of `top` its most
        frequent window of w ids makes up more than t of it -- top_count_w * w > t * length -- or if for some (w, t) of
        `dup` more than t of it lies inside repeated windows of w ids -- covered_w > t * length --, the columns those of
        repetition_resident(ngram=w), both sides compared in float64.  The defaults are Gopher's thresholds.  A document
        of length 0 is never flagged.  One engine call per distinct w.  n_repetitive_docs then holds the number of
        flagged documents."""
        import torch
        top, dup = self._repetition_rules(top, dup)
        self._select_values(max_len, keep)
        _check_ids(ids, (torch.int32, torch.int64), cuda=False)
        doc_offsets = _check_doc_offsets(doc_offsets, ids.device, strict=True)
        _check_ids(ids, (torch.int32, torch.int64))
        want = {}
        for rules, column in ((top, "top_count"), (dup, "covered")):
            for w, _ in rules:
                want.setdefault(w, {"length"}).add(column)
        stats, doff = {}, None
        for w in sorted(want):
            stats[w], _, doff = self._repetition(ids, doc_offsets, w, max_len, keep, False, columns=want[w], doff=doff)
        flagged = self._repetition_flags(stats, top, dup)
        self._n_repetitive_docs = int(flagged.sum().item())
        return flagged

    def drop_repetitive_docs_resident(self, ids, doc_offsets, *, top=((2, .20), (3, .18), (4, .16)),
                                      dup=((5, .15), (6, .14), (7, .13), (8, .12), (9, .11), (10, .10)), max_len=None,
                                      keep="head", out=None):
        """The documents that repetitive_docs_resident() does not flag, in the order of the stream: that call and
        select_docs_resident() in one.  Returns (ids', doc_offsets', kept, flagged): the id stream of the kept
        documents and its offsets as select_docs_resident returns them, kept int64 [k] the kept document numbers and
        flagged bool [n_docs] the flags of ALL documents, all on the device of `ids`.  With max_len the kept documents
        are cut the same way they were judged.  out: as in select_docs_resident."""
        import torch
        self._repetition_rules(top, dup)
        self._select_values(max_len, keep)
        _check_ids(ids, (torch.int32, torch.int64), cuda=False)
        if out is not None and (not isinstance(out, torch.Tensor) or out.device != ids.device or out.dtype != ids.dtype
                                or out.dim() != 1 or not out.is_contiguous()):
            raise TypeError("out must be a 1-D contiguous torch tensor of the dtype and on the device of ids")
        flagged = self.repetitive_docs_resident(ids, doc_offsets, top=top, dup=dup, max_len=max_len, keep=keep)
        kept = torch.nonzero(~flagged).reshape(-1)
        res, ooff = self.select_docs_resident(ids, doc_offsets, kept, max_len=max_len, keep=keep, out=out)
        return res, ooff, kept, flagged

    # -- windows an earlier document already holds ------------------------
    @property
    def n_docs_with_duplicate_spans(self):
        """The number of documents with a seen window that the last duplicate_spans_resident() /
        drop_duplicate_spans_resident() of this tokenizer found (and their host forms); None before the first."""
        return getattr(self, "_n_docs_with_duplicate_spans", None)

    @property
    def n_span_windows(self):
        """The windows of all documents in that call, repeats counted; None before the first."""
        return getattr(self, "_n_span_windows", None)

    @property
    def n_distinct_span_windows(self):
        """The distinct windows of all documents in that call; None before the first."""
        return getattr(self, "_n_distinct_span_windows", None)

    @staticmethod
    def _scope_value(scope):
        """the library's flag of a scope; ValueError for a scope it does not know"""
        if not isinstance(scope, str) or scope not in ("earlier_doc", "anywhere"):
            raise ValueError(f"scope={scope!r} not understood: 'earlier_doc' or 'anywhere'")
        return _native.SPANS_ANYWHERE if scope == "anywhere" else 0

    @staticmethod
    def _check_out(out, ids):
        """TypeError unless `out` is None or a tensor that select_docs_resident would take for `ids`"""
        import torch
        if out is not None and (not isinstance(out, torch.Tensor) or out.device != ids.device or out.dtype != ids.dtype
                                or out.dim() != 1 or not out.is_contiguous()):
            raise TypeError("out must be a 1-D contiguous torch tensor of the dtype and on the device of ids")

    def duplicate_spans_resident(self, ids, doc_offsets, *, ngram=50, scope="earlier_doc", max_len=None, keep="head",
                                 return_marks=False):
        """Which stretches of every document were already seen in an EARLIER document of the same stream, found on the
        device: the licence text, the menu, the signature that otherwise different documents share -- the
        exact-substring de-duplication of Lee et al. (windows of 50 tokens) and RefinedWeb's span removal; not in the
        reference.  `ids` and `doc_offsets` are what select_docs_resident takes.  max_len / keep: documents are cut as
        select_docs_resident cuts them with the same values, and a window lies inside the cut; a document shorter than
        ngram has no window.  The windows of ALL documents are compared with one another; a window is seen if an equal
        one starts inside an earlier document (scope="earlier_doc"), or anywhere earlier in the stream, in-document
        repeats included (scope="anywhere": every occurrence but the first).  Exact: a hash only chooses where to look,
        every equality is established by comparing the ids at their full width; the result does not depend on scheduling.

        Returns a SpanDupStats of int64 tensors [n_docs] on the device of `ids`: length (of the cut document), windows,
        seen, covered (the positions that lie inside a seen window), first (where in the uncut document the first seen
        window starts, -1 without one), src_pos (the stream position at which that window's ids first stand, -1;
        searchsorted(doc_offsets, src_pos, right=True) - 1 is the source document); marks is None, or with
        return_marks=True a uint8 tensor [len(ids)]: bit 0 where a seen window starts, bit 1 where the position is covered
        -- what keep_ids_resident(bits=2, drop=True) cuts out.  n_docs_with_duplicate_spans, n_span_windows and
        n_distinct_span_windows then hold the counters.  Offsets that descend or pass len(ids) raise ValueError.  Nothing
        but counters crosses PCIe."""
        return self._duplicate_spans(ids, doc_offsets, ngram, scope, max_len, keep, return_marks)[0]

    def _duplicate_spans(self, ids, doc_offsets, ngram, scope, max_len, keep, return_marks):
        """(SpanDupStats, the offsets on the device)"""
        import torch
        ngram = self._ngram_value(ngram)
        flags = self._scope_value(scope)
        max_len, tail = self._select_values(max_len, keep)
        _check_ids(ids, (torch.int32, torch.int64), cuda=False)
        dev = ids.device
        doc_offsets = _check_doc_offsets(doc_offsets, dev, strict=True)
        _check_ids(ids, (torch.int32, torch.int64))
        doff = _place_doc_offsets(doc_offsets, dev)
        n_docs = doff.numel() - 1
        cols = [torch.empty(n_docs, dtype=torch.int64, device=dev) for _ in range(6)]
        marks = torch.empty(ids.numel(), dtype=torch.uint8, device=dev) if return_marks else None
        eng = engine(dev.index)
        torch.cuda.current_stream(dev).synchronize()  # the caller's pending writes to ids (and the upload above) are done
        counters = eng.dup_spans_resident(ids.data_ptr(), ids.element_size(), ids.numel(), doff.data_ptr(), n_docs, ngram,
                                          max_len, flags | tail, *[col.data_ptr() for col in cols],
                                          marks.data_ptr() if return_marks else 0)
        self._n_docs_with_duplicate_spans, self._n_span_windows, self._n_distinct_span_windows = counters
        return SpanDupStats(*cols, marks), doff

    def duplicate_spans(self, ids, doc_offsets, *, device=None, ngram=50, scope="earlier_doc", **kw):
        """duplicate_spans_resident() for ids on the host (a list or an array of integers; an int32 array goes up as
        int32, anything else as int64): a SpanDupStats of NumPy arrays.  device: the GPU's index (default: the
        process-wide engine's)."""
        self._ngram_value(ngram)
        self._scope_value(scope)
        d_ids, doc_offsets = self._host_docs(ids, doc_offsets, device, kw)
        res = self.duplicate_spans_resident(d_ids, doc_offsets, ngram=ngram, scope=scope, **kw)
        return SpanDupStats(*[None if t is None else t.cpu().numpy() for t in res])

    @staticmethod
    def _keep_values(bits, drop):
        """(bits, flags) of the library from the keywords; ValueError for values it does not know"""
        if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not 1 <= bits <= 255:
            raise ValueError("bits must be an integer from 1 to 255")
        if not isinstance(drop, (bool, np.bool_)):
            raise ValueError("drop must be True or False")
        return int(bits), _native.KEEP_DROP if drop else 0

    def keep_ids_resident(self, ids, doc_offsets, mask, *, bits=0xFF, drop=False, out=None):
        """The ids at the marked positions of every document, cut out of the stream on the device -- or, with drop=True,
        the ids at the unmarked ones; not in the reference.  `ids` and `doc_offsets` are what select_docs_resident takes.
        mask: a uint8 or bool tensor [len(ids)] on the device of `ids` -- the marks of duplicate_spans_resident and of
        repetition_resident and the starts of ngram_overlap_resident as they are.  A position inside a document is kept
        iff mask & bits is not 0 (drop=True: iff it is 0); ids in front of the first and behind the last document are
        dropped.

        Returns (ids', doc_offsets'): the kept ids in order, in the dtype of `ids`, and the int64 [n_docs + 1] offsets of
        the same documents in ids' -- one that loses everything stays as an empty document, and document numbers do not
        change --, both on the GPU.  out: as in select_docs_resident; it must not overlap `ids`.  Offsets that descend
        or pass len(ids) raise ValueError.  Nothing but counters crosses PCIe."""
        import torch
        bits, flags = self._keep_values(bits, drop)
        _check_ids(ids, (torch.int32, torch.int64), cuda=False)
        dev = ids.device
        doc_offsets = _check_doc_offsets(doc_offsets, dev, strict=True)
        self._check_out(out, ids)
        if not isinstance(mask, torch.Tensor) or mask.device != dev or mask.dtype not in (torch.uint8, torch.bool) \
                or mask.dim() != 1 or not mask.is_contiguous():
            raise TypeError("mask must be a 1-D contiguous uint8 or bool torch tensor on the device of ids")
        if mask.numel() != ids.numel():
            raise ValueError(f"the mask holds {mask.numel()} entries, there are {ids.numel()} ids")
        _check_ids(ids, (torch.int32, torch.int64))
        if mask.dtype == torch.bool:
            mask, bits = mask.view(torch.uint8), 1  # (a bool is one byte, 0 or 1: its one bit is the mark)
        doff = _place_doc_offsets(doc_offsets, dev)
        n_docs = doff.numel() - 1
        ooff = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
        eng = engine(dev.index)
        torch.cuda.current_stream(dev).synchronize()  # the caller's pending writes to ids and mask are done
        res = self._resident_fill(
            ids, out, ids.dtype, None, "ids", "keeps",
            lambda dst, cap, *_: eng.keep_ids_resident(ids.data_ptr(), ids.element_size(), ids.numel(), doff.data_ptr(),
                                                       n_docs, mask.data_ptr(), bits, flags, dst, cap, ooff.data_ptr()))
        return res, ooff

    def keep_ids(self, ids, doc_offsets, mask, *, device=None, **kw):
        """keep_ids_resident() for ids and a mask on the host (the mask: anything np.asarray makes a flat uint8 or bool
        array of): NumPy (ids', doc_offsets'), the ids int32 if an int32 array came in and int64 otherwise."""
        import torch
        self._keep_values(kw.get("bits", 0xFF), kw.get("drop", False))
        if kw.get("out") is not None:
            raise TypeError("keep_ids makes its own output")
        arr, doc_offsets = self._host_stream(ids, doc_offsets)
        m = np.asarray(mask)
        if m.dtype not in (np.uint8, np.bool_) or m.ndim != 1:
            raise TypeError("mask must be a flat uint8 or bool array")
        if m.size != arr.size:
            raise ValueError(f"the mask holds {m.size} entries, there are {arr.size} ids")
        dev = _cuda_device(device)
        res, ooff = self.keep_ids_resident(torch.from_numpy(arr).to(dev), doc_offsets,
                                           torch.from_numpy(np.ascontiguousarray(m)).to(dev), **kw)
        return res.cpu().numpy(), ooff.cpu().numpy()

    def drop_duplicate_spans_resident(self, ids, doc_offsets, *, ngram=50, scope="earlier_doc", out=None):
        """The stream without the stretches an earlier document already holds: duplicate_spans_resident() over whole
        documents and keep_ids_resident(marks, bits=2, drop=True) in one call -- every position inside a seen window
        goes, the first occurrence of every window stays.  Returns (ids', doc_offsets', stats): the id stream and the
        offsets of the same documents in it as keep_ids_resident returns them, and the SpanDupStats with its marks;
        stats.covered says what each document lost.  out: as in select_docs_resident."""
        import torch
        self._ngram_value(ngram)
        self._scope_value(scope)
        _check_ids(ids, (torch.int32, torch.int64), cuda=False)
        self._check_out(out, ids)
        stats, doff = self._duplicate_spans(ids, doc_offsets, ngram, scope, None, "head", True)
        res, ooff = self.keep_ids_resident(ids, doff, stats.marks, bits=2, drop=True, out=out)
        return res, ooff, stats

    # -- the lines of every document as a stream of their own -------------
    @property
    def n_segments(self):
        """The number of segments the last segments_resident() of this tokenizer found (and the methods built on it,
        and their host forms); None before the first."""
        return getattr(self, "_n_segments", None)

    @property
    def n_segment_ids(self):
        """The ids of that call's segment stream, tags included; None before the first."""
        return getattr(self, "_n_segment_ids", None)

    @property
    def n_duplicate_lines(self):
        """The number of duplicate lines the last duplicate_lines_resident() of this tokenizer found (and the methods
        built on it, and their host forms); None before the first."""
        return getattr(self, "_n_duplicate_lines", None)

    @property
    def n_docs_with_duplicate_lines(self):
        """The documents with a duplicate line in that call; None before the first."""
        return getattr(self, "_n_docs_with_duplicate_lines", None)

    @staticmethod
    def _segment_unit(unit):
        """ValueError for a unit that is not offered"""
        if not isinstance(unit, str) or unit != "line":
            raise ValueError(f"unit={unit!r} not understood: 'line'")

    def segment_classes(self, unit="line"):
        """The class of every one of the 256 + M dense ids for splitting documents into lines, a uint8 array computed
        from the vocabulary: SEG_SKIP (2) for a token whose bytes are all ASCII whitespace (space, \\t, \\n, \\r, \\x0b,
        \\x0c) -- it belongs to no line --, SEG_BREAK (1) for a token that contains \\n -- a line ends behind it.  A
        newline token itself has both.  Special tokens and ids outside the table have class 0: content that ends no
        line.  The rule is token-granular: a newline in the MIDDLE of a token ends the line behind the whole token, so
        the whole token belongs to the line it ends.  The GPT-2 and GPT-4 split patterns never let a merge put a
        letter behind a newline, so this can only happen with BasicTokenizer.  Only unit="line" is offered."""
        self._segment_unit(unit)
        cached = getattr(self, "_segment_classes", None)
        if cached is not None and cached[0] is self.vocab and cached[1] == len(self.merges):
            return cached[2].copy()
        n = 256 + len(self.merges)
        cls = np.zeros(n, dtype=np.uint8)
        for idx in range(n):
            tok = self.vocab[idx]
            if tok and not tok.strip(_LINE_SPACE):
                cls[idx] |= _native.SEG_SKIP
            if b"\n" in tok:
                cls[idx] |= _native.SEG_BREAK
        self._segment_classes = (self.vocab, len(self.merges), cls)
        return cls.copy()

    def _segment_classes_arg(self, unit, classes):
        """the class table a call splits by, checked: the caller's (a flat uint8 array or tensor), else this
        vocabulary's for `unit`"""
        import torch
        self._segment_unit(unit)
        if classes is None:
            return self.segment_classes(unit)
        if isinstance(classes, torch.Tensor):
            if classes.dtype != torch.uint8 or classes.dim() != 1 or not classes.is_contiguous():
                raise TypeError("classes must be a flat contiguous uint8 array or tensor")
            return classes
        arr = np.asarray(classes)
        if arr.dtype != np.uint8 or arr.ndim != 1:
            raise TypeError("classes must be a flat contiguous uint8 array or tensor")
        return np.ascontiguousarray(arr)

    @staticmethod
    def _tag_value(tag_docs):
        """the library's flag; ValueError for a value that is no truth value"""
        if not isinstance(tag_docs, (bool, np.bool_)):
            raise ValueError("tag_docs must be True or False")
        return _native.SEG_TAG_DOC if tag_docs else 0

    def segments_resident(self, ids, doc_offsets, *, unit="line", classes=None, tag_docs=False, out=None):
        """The lines of every document as an id stream of their own, made on the device; not in the reference.  `ids`
        and `doc_offsets` are what select_docs_resident takes.  A document is walked id by id: an id without SEG_SKIP
        is content, the first content after a boundary starts a segment, an id with SEG_BREAK puts a boundary behind
        itself, and a document's end is one -- so no segment is empty, a document may have none, and whitespace in any
        amount between two lines belongs to neither.  classes: a uint8 array or tensor of the caller's own, one class
        per id (ids outside it have class 0), to split at a special token or at sentence ends instead; it overrides unit.

        Returns a Segments of tensors on the device of `ids`; (segments.ids, segments.seg_offsets) is an (ids,
        doc_offsets) pair: duplicate_docs_resident on it is exact line de-duplication, minhash_resident near-duplicate
        lines, ngram_overlap_resident contamination per line.  tag_docs=True puts the document's number in front of
        every segment as one id, so that those calls compare the lines of one document only.  out: as in
        select_docs_resident.  n_segments and n_segment_ids then hold the counters.  Offsets that descend or pass
        len(ids) raise ValueError.  Nothing but counters crosses PCIe (and, once per vocabulary and device, the classes)."""
        return self._segments(ids, doc_offsets, unit, classes, tag_docs, out)[0]

    def _segments(self, ids, doc_offsets, unit, classes, tag_docs, out):
        """(Segments, the offsets on the device)"""
        import torch
        cls = self._segment_classes_arg(unit, classes)
        flags = self._tag_value(tag_docs)
        _check_ids(ids, (torch.int32, torch.int64), cuda=False)
        dev = ids.device
        doc_offsets = _check_doc_offsets(doc_offsets, dev, strict=True)
        self._check_out(out, ids)
        if isinstance(cls, torch.Tensor) and cls.device != dev:
            raise TypeError("classes must be on the device of ids")
        _check_ids(ids, (torch.int32, torch.int64))
        doff = _place_doc_offsets(doc_offsets, dev)
        n_docs = doff.numel() - 1
        if isinstance(cls, torch.Tensor):
            d_cls = cls
        else:  # (this vocabulary's table stays on the device it was last used on)
            held = getattr(self, "_segment_classes_dev", None)
            if classes is None and held is not None and held[0] is self._segment_classes[2] and held[1] == dev:
                d_cls = held[2]
            else:
                d_cls = torch.from_numpy(cls).to(dev)
                if classes is None:
                    self._segment_classes_dev = (self._segment_classes[2], dev, d_cls)
        dso = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
        eng = engine(dev.index)
        torch.cuda.current_stream(dev).synchronize()  # the caller's pending writes to ids (and the uploads above) are done
        cols, totals = [], [0, 0]

        def run(dst, cap):
            room = (0, 0, 0, 0, 0, 0, 0) if not cols else (dst, cap, cols[0].data_ptr(), cols[1].numel(),
                                                           cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr())
            totals[:] = eng.segment_docs_resident(ids.data_ptr(), ids.element_size(), ids.numel(), doff.data_ptr(), n_docs,
                                                  d_cls.data_ptr(), d_cls.numel(), flags, *room, dso.data_ptr())
            return totals[0]

        def native_call(dst, cap, *_):
            if not cols:  # the count comes first: it sizes the per-segment columns
                run(0, 0)
                cols.append(torch.zeros(totals[1] + 1, dtype=torch.int64, device=dev))
                cols.extend(torch.empty(totals[1], dtype=torch.int64, device=dev) for _ in range(3))
                torch.cuda.current_stream(dev).synchronize()
            return run(dst, cap) if dst and cap else totals[0]

        res = self._resident_fill(ids, out, ids.dtype, None, "ids", "segments", native_call)
        self._n_segment_ids, self._n_segments = totals
        return Segments(res, cols[0], cols[1], dso, cols[2], cols[3]), doff

    def segment_marks_resident(self, segments, values, n):
        """A verdict per segment as a mark per id: marks[p] = values[s] for every position p of the source range of
        segment s, 0 at every other of the n positions -- the mask keep_ids_resident takes.  segments: what
        segments_resident returned for a stream of n ids; values: a uint8 or bool tensor [n_segments] on its device.
        Returns a uint8 tensor [n]."""
        import torch
        if not isinstance(segments, Segments):
            raise TypeError("segments must be what segments_resident returned")
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
            raise ValueError("n must be the number of ids of the stream the segments came from")
        start, end = segments.src_start, segments.src_end
        for t in (start, end):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int64 or t.dim() != 1 \
                    or not t.is_contiguous() or t.numel() != start.numel() or t.device != start.device:
                raise TypeError("segments must hold the int64 tensors on the GPU that segments_resident returned")
        if not isinstance(values, torch.Tensor) or values.device != start.device or values.dim() != 1 \
                or values.dtype not in (torch.uint8, torch.bool) or not values.is_contiguous():
            raise TypeError("values must be a 1-D contiguous uint8 or bool torch tensor on the device of the segments")
        if values.numel() != start.numel():
            raise ValueError(f"there are {values.numel()} values for {start.numel()} segments")
        dev = start.device
        if values.dtype == torch.bool:
            values = values.view(torch.uint8)
        marks = torch.empty(int(n), dtype=torch.uint8, device=dev)
        eng = engine(dev.index)
        torch.cuda.current_stream(dev).synchronize()  # the caller's pending writes to the values are done
        try:
            eng.segment_marks_resident(start.data_ptr(), end.data_ptr(), start.numel(), values.data_ptr(), int(n),
                                       marks.data_ptr())
        except _native.BadSegment as e:
            raise ValueError(f"segment {e.index}: its source range does not fit a stream of {n} ids") from None
        return marks

    @staticmethod
    def _line_scope(scope):
        """tag_docs of a scope; ValueError for a scope that is not known"""
        if not isinstance(scope, str) or scope not in ("in_doc", "stream"):
            raise ValueError(f"scope={scope!r} not understood: 'in_doc' or 'stream'")
        return scope == "in_doc"

    @staticmethod
    def _min_len_value(min_len):
        if isinstance(min_len, bool) or not isinstance(min_len, (int, np.integer)) or min_len < 1:
            raise ValueError("min_len must be an integer of 1 or more")
        return int(min_len)

    def duplicate_lines_resident(self, ids, doc_offsets, *, scope="in_doc", min_len=1, unit="line", classes=None,
                                 return_marks=False):
        """Which lines of every document are copies of an earlier line, found on the device: the line half of the
        Gopher / MassiveText repetition rules (scope="in_doc": an equal line stands earlier in the SAME document) and
        CCNet-style line de-duplication (scope="stream": an equal line stands anywhere earlier in the stream -- menus,
        cookie banners, "read more"); not in the reference.  segments_resident() with tag_docs=(scope == "in_doc"), then
        duplicate_docs_resident() on the segment stream: a line is a duplicate iff it is not the first of its copies and
        has at least min_len content ids.  Lines are compared as their content ids, exactly, whitespace ids left out.
        unit, classes: as in segments_resident.

        Returns a LineDupStats of int64 tensors [n_docs] on the device of `ids`: length, lines, dup_lines, content (the
        ids that belong to a line), dup_content (those of them in a duplicate line); marks is None, or with
        return_marks=True a uint8 tensor [len(ids)] with bit 0 set over the whole source range of every duplicate line
        -- the line, and the whitespace behind it -- which keep_ids_resident(bits=1, drop=True) cuts out.
        n_duplicate_lines and n_docs_with_duplicate_lines then hold the counters."""
        return self._duplicate_lines(ids, doc_offsets, scope, min_len, unit, classes, return_marks)[0]

    def _duplicate_lines(self, ids, doc_offsets, scope, min_len, unit, classes, return_marks):
        """(LineDupStats, the offsets on the device)"""
        import torch
        tag = self._line_scope(scope)
        min_len = self._min_len_value(min_len)
        seg, doff = self._segments(ids, doc_offsets, unit, classes, tag, None)
        dev = ids.device
        n_seg, n_docs = seg.seg_doc.numel(), doff.numel() - 1
        content_len = seg.seg_offsets[1:] - seg.seg_offsets[:-1] - int(tag)
        if n_seg:
            first = self._duplicate_docs(seg.ids, seg.seg_offsets)[0]  # (n_distinct_docs speaks of the caller's documents)
            dup = (first != torch.arange(n_seg, dtype=torch.int64, device=dev)) & (content_len >= min_len)
        else:
            dup = torch.zeros(0, dtype=torch.bool, device=dev)

        def fold(values):
            return torch.zeros(n_docs, dtype=torch.int64, device=dev).index_add_(0, seg.seg_doc, values)

        stats = LineDupStats(doff[1:] - doff[:-1], seg.doc_seg_offsets[1:] - seg.doc_seg_offsets[:-1],
                             fold(dup.to(torch.int64)), fold(content_len), fold(content_len * dup),
                             self.segment_marks_resident(seg, dup, ids.numel()) if return_marks else None)
        self._n_duplicate_lines = int(dup.sum().item())
        self._n_docs_with_duplicate_lines = int((stats.dup_lines > 0).sum().item())
        return stats, doff

    @staticmethod
    def _line_fractions(line_frac, content_frac):
        for name, v in (("line_frac", line_frac), ("content_frac", content_frac)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0 <= v <= 1:
                raise ValueError(f"{name} must be a number from 0 to 1")
        return float(line_frac), float(content_frac)

    def repetitive_line_docs_resident(self, ids, doc_offsets, *, line_frac=.30, content_frac=.20, min_len=1, unit="line",
                                      classes=None):
        """The line half of the Gopher / MassiveText repetition rules, on the device: flagged, a bool tensor [n_docs]:
        document d is flagged iff dup_lines > line_frac * lines or dup_content > content_frac * content of
        duplicate_lines_resident(scope="in_doc"), both sides compared in float64; a document without a line is never
        flagged.  The defaults are Gopher's: more than 30 % of the lines, or 20 % of the content, are duplicate lines.
        (repetitive_docs_resident is the n-gram half.)"""
        line_frac, content_frac = self._line_fractions(line_frac, content_frac)
        st = self._duplicate_lines(ids, doc_offsets, "in_doc", min_len, unit, classes, False)[0]
        return (st.dup_lines.double() > line_frac * st.lines.double()) | \
            (st.dup_content.double() > content_frac * st.content.double())

    def drop_duplicate_lines_resident(self, ids, doc_offsets, *, scope="stream", min_len=1, unit="line", classes=None,
                                      out=None):
        """The stream without its duplicate lines: duplicate_lines_resident(return_marks=True) and
        keep_ids_resident(marks, bits=1, drop=True) in one call -- every duplicate line goes with the whitespace behind
        it, the first copy of every line stays.  Returns (ids', doc_offsets', stats) as drop_duplicate_spans_resident
        does; stats.dup_lines says what each document lost.  out: as in select_docs_resident."""
        import torch
        self._line_scope(scope)
        self._min_len_value(min_len)
        self._segment_classes_arg(unit, classes)
        _check_ids(ids, (torch.int32, torch.int64), cuda=False)
        self._check_out(out, ids)
        stats, doff = self._duplicate_lines(ids, doc_offsets, scope, min_len, unit, classes, True)
        res, ooff = self.keep_ids_resident(ids, doff, stats.marks, bits=1, drop=True, out=out)
        return res, ooff, stats

    def _host_lines(self, ids, doc_offsets, device, kw):
        """the arguments of the host forms, checked before a device is named -> (ids on the GPU, offsets)"""
        import torch
        if kw.get("out") is not None:
            raise TypeError("the host forms make their own output")
        self._segment_classes_arg(kw.get("unit", "line"), kw.get("classes"))
        if "tag_docs" in kw:
            self._tag_value(kw["tag_docs"])
        if "scope" in kw:
            self._line_scope(kw["scope"])
        self._min_len_value(kw.get("min_len", 1))
        arr, doc_offsets = self._host_stream(ids, doc_offsets)
        dev = _cuda_device(device)
        if isinstance(kw.get("classes"), torch.Tensor):
            kw["classes"] = kw["classes"].to(dev)
        return torch.from_numpy(arr).to(dev), doc_offsets

    def segments(self, ids, doc_offsets, *, device=None, **kw):
        """segments_resident() for ids on the host (a list or an array of integers; an int32 array goes up as int32,
        anything else as int64): a Segments of NumPy arrays.  device: the GPU's index (default: the process-wide
        engine's)."""
        d_ids, doc_offsets = self._host_lines(ids, doc_offsets, device, kw)
        return Segments(*[t.cpu().numpy() for t in self.segments_resident(d_ids, doc_offsets, **kw)])

    def duplicate_lines(self, ids, doc_offsets, *, device=None, **kw):
        """duplicate_lines_resident() for ids on the host: a LineDupStats of NumPy arrays."""
        d_ids, doc_offsets = self._host_lines(ids, doc_offsets, device, kw)
        res = self.duplicate_lines_resident(d_ids, doc_offsets, **kw)
        return LineDupStats(*[None if t is None else t.cpu().numpy() for t in res])

    def drop_duplicate_lines(self, ids, doc_offsets, *, device=None, **kw):
        """drop_duplicate_lines_resident() for ids on the host: NumPy (ids', doc_offsets', stats), the ids int32 if an
        int32 array came in and int64 otherwise."""
        d_ids, doc_offsets = self._host_lines(ids, doc_offsets, device, kw)
        res, ooff, stats = self.drop_duplicate_lines_resident(d_ids, doc_offsets, **kw)
        return res.cpu().numpy(), ooff.cpu().numpy(), LineDupStats(*[None if t is None else t.cpu().numpy() for t in stats])

    # -- fixed-length rows from ids that live in HBM ---------------------
    def rows_resident(self, ids, doc_offsets, row_len, *, stride=None, sep=None, pad=0, mode="pack", truncate="right",
                      pad_side="right", dtype=None, drop_last=False, return_doc_index=False, return_positions=False,
                      out=None, _total=None):
        """Fixed-length rows for a model from token ids that live in HBM, made on the device; not in the reference.
        `ids` is a 1-D contiguous int32 torch tensor on the GPU (what encode_ordinary_batch_resident returns),
        `doc_offsets` n_docs + 1 token positions -- an integer tensor on the same GPU or anything np.asarray takes --,
        document d being ids[doc_offsets[d]:doc_offsets[d + 1]].  sep: an id (or the text of a registered special token)
        appended to every document; pad: the id that fills what is left.  dtype: torch.int64 (default) or torch.int32.

        mode="pack": the documents joined into one stream and cut into rows of row_len every `stride` positions
        (default row_len: disjoint rows; row_len - 1: input and target overlap by one token).  Returns the [R, row_len]
        tensor, R = rows_count(len(stream), row_len, stride); with return_doc_index / return_positions also int32
        tensors of the same shape: the document of every element (pad: -1) and its index inside its document (pad: 0).
        drop_last drops the last row if it is partial.

        mode="per_doc": one row per document, cut to row_len (truncate="right" keeps the head, "left" the tail) and padded
        on pad_side.  Returns (rows [n_docs, row_len], lengths int32 [n_docs]).

        out: a contiguous tensor of `dtype` on the same GPU to write the rows into (the view of the rows written is
        returned; ValueError if it is too small).  Nothing but counters crosses PCIe."""
        import torch
        # -- values: checked before any tensor is looked at, and all of it before the engine exists
        if isinstance(row_len, bool) or not isinstance(row_len, (int, np.integer)) or row_len < 1:
            raise ValueError("row_len must be a positive integer")
        row_len = int(row_len)
        if mode not in ("pack", "per_doc"):
            raise ValueError(f"mode={mode!r} not understood: 'pack' or 'per_doc'")
        pack = mode == "pack"
        if truncate not in ("right", "left") or pad_side not in ("right", "left"):
            raise ValueError("truncate and pad_side are 'right' or 'left'")
        if pack:
            if truncate != "right" or pad_side != "right":
                raise ValueError("truncate / pad_side belong to mode='per_doc'")
            stride = row_len if stride is None else stride
            if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or not 1 <= stride <= row_len:
                raise ValueError("stride must be an integer in 1..row_len")
            stride = int(stride)
        else:
            if stride is not None or drop_last or return_doc_index or return_positions:
                raise ValueError("stride, drop_last, return_doc_index and return_positions belong to mode='pack'")
            stride = row_len
        if isinstance(sep, str):
            sep = self.special_tokens[sep]  # (KeyError: not a registered special token)
        for name, v in (("sep", sep), ("pad", pad)):
            if v is None and name == "sep":
                continue
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -2**31 <= v < 2**31:
                raise ValueError(f"{name} must be an integer that fits int32")
        dtype = torch.int64 if dtype is None else dtype
        if dtype not in (torch.int32, torch.int64):
            raise ValueError("dtype must be torch.int32 or torch.int64")
        # -- tensors
        _check_ids(ids, (torch.int32,), cuda=False)
        dev = ids.device
        doc_offsets = _check_doc_offsets(doc_offsets, dev, strict=True)
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != dtype or not out.is_contiguous():
                raise TypeError("out must be a contiguous tensor of `dtype` on the device of ids")
        _check_ids(ids, (torch.int32,))
        # -- the device
        doff = _place_doc_offsets(doc_offsets, dev)
        n, n_docs = ids.numel(), doff.numel() - 1
        flags = (_native.ROWS_HAS_SEP if sep is not None else 0) | (_native.ROWS_TRUNC_LEFT if truncate == "left" else 0) \
            | (_native.ROWS_PAD_LEFT if pad_side == "left" else 0)
        width = 4 if dtype == torch.int32 else 8
        eng = engine(dev.index)
        torch.cuda.current_stream(dev).synchronize()  # the caller's pending writes to ids (and the upload above) are done

        def call(dst, cap, comps=(None, None, None)):
            try:
                return eng.rows_resident(ids.data_ptr(), n, doff.data_ptr(), n_docs,
                                         _native.ROWS_PACK if pack else _native.ROWS_PER_DOC, flags, row_len, stride,
                                         0 if sep is None else int(sep), int(pad), 0 if dst is None else dst.data_ptr(),
                                         width, cap, *(0 if t is None else t.data_ptr() for t in comps))
            except _native.RowsTooSmall as e:
                raise ValueError(f"out holds {cap} rows of {row_len}, the batch makes {e.needed}") from None

        if not pack:
            R = n_docs
        elif _total is not None:  # (the caller knows the stream's length: no counting call)
            R = rows_count(_total, row_len, stride)
        else:
            R = call(None, 0)
        cap = R if out is None else out.numel() // row_len
        if out is None:
            out = torch.empty((R, row_len), dtype=dtype, device=dev)
        elif cap == 0 and R:  # (no room at all is a count-only call to the library)
            raise ValueError(f"out holds 0 rows of {row_len}, the batch makes {R}")
        comps = [None, None, None]
        if return_doc_index:
            comps[0] = torch.empty((R, row_len), dtype=torch.int32, device=dev)
        if return_positions:
            comps[1] = torch.empty((R, row_len), dtype=torch.int32, device=dev)
        if not pack:
            comps[2] = torch.empty(n_docs, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        R = call(out, cap, comps)
        rows = out.reshape(-1)[:R * row_len].view(R, row_len)
        if not pack:
            return rows, comps[2]
        keep = R
        if drop_last and R:
            total = _total if _total is not None else \
                int((doff[-1] - doff[0]).item()) + (n_docs if sep is not None else 0)
            if (R - 1) * stride + row_len > total:
                keep = R - 1
        res = [rows[:keep]] + [t[:keep] for t in comps[:2] if t is not None]
        return res[0] if len(res) == 1 else tuple(res)

    # -- persistence (file formats of base.py:97-165, byte for byte) -----------------
    def save(self, file_prefix):
        lines = ["minbpe v1", f"{self.pattern}", f"{len(self.special_tokens)}"]
        lines += [f"{tok} {idx}" for tok, idx in self.special_tokens.items()]
        lines += [f"{a} {b}" for a, b in self.merges]
        with open(file_prefix + ".model", "w") as f:
            f.write("\n".join(lines) + "\n")
        parents = {idx: pair for pair, idx in self.merges.items()}
        with open(file_prefix + ".vocab", "w", encoding="utf-8") as f:
            for idx, tok in self.vocab.items():
                shown = render_token(tok)
                if idx in parents:
                    a, b = parents[idx]
                    f.write(f"[{render_token(self.vocab[a])}][{render_token(self.vocab[b])}]"
                            f" -> [{shown}] {idx}\n")
                else:
                    f.write(f"[{shown}] {idx}\n")

    def load(self, model_file):
        assert model_file.endswith(".model")
        with open(model_file, "r", encoding="utf-8") as f:
            assert f.readline().strip() == "minbpe v1"
            self.pattern = f.readline().strip()
            specials = {}
            for _ in range(int(f.readline().strip())):
                tok, idx = f.readline().strip().split()
                specials[tok] = int(idx)
            merges = {}
            for idx, line in enumerate(f, start=256):
                a, b = map(int, line.split())
                merges[(a, b)] = idx
        self.merges = merges
        self.special_tokens = specials
        self.vocab = self._build_vocab()


class BasicTokenizer(Tokenizer):
    """Byte-level BPE over the whole text as one chunk (basic.py:15-74)."""

    def __init__(self):
        super().__init__()

    def train(self, text, vocab_size, verbose=False):
        # (a long text is encoded by all host threads: _native.utf8_encode -- the same bytes as text.encode("utf-8"))
        self._train_on_device(_native.utf8_encode(text), None, vocab_size, verbose)

    def decode(self, ids):
        return b"".join(self.vocab[i] for i in ids).decode("utf-8", errors="replace")

    def encode(self, text):
        ids, _ = self._encode_chunks([text.encode("utf-8")])
        return ids.tolist()

    def encode_with_offsets(self, text, unit="char"):
        """(ids, spans): encode(text) and, for every token, its (start, end) in `text` -- in characters (unit="char":
        text[start:end] covers the token), in bytes of text.encode("utf-8") (unit="byte"), or the pair of both lists
        (unit="both").  One encode plus one token_spans call; not in the reference."""
        return self._with_offsets(self.encode, text, unit)


class RegexTokenizer(Tokenizer):
    """BPE over regex-split chunks with optional special tokens (regex.py:22-164)."""

    def __init__(self, pattern=None):
        super().__init__()
        self.pattern = GPT4_SPLIT_PATTERN if pattern is None else pattern
        self.compiled_pattern = re.compile(self.pattern)
        self.special_tokens = {}
        self.inverse_special_tokens = {}

    def _split(self, text):
        return [piece.encode("utf-8") for piece in re.findall(self.compiled_pattern, text)]

    def _chunked(self, text, for_training=False):
        """(utf-8 bytes of the chunks back to back, chunk start offsets) -- what
        re.findall(self.compiled_pattern, text) yields (regex.py:41,114).  The two GPT
        patterns go through the native scanner (bpe_split, checked against `regex` in
        tests/test_split.py); any other pattern through the `regex` module itself."""
        which = _NATIVE_SPLIT.get(self.compiled_pattern.pattern)
        if which is not None:
            # (train() takes any buffer of bytes: a long text is encoded by all host threads there)
            data = _native.utf8_encode(text) if for_training else text.encode("utf-8")
            return data, _native.split_offsets(data, which)
        return _concat_chunks(self._split(text))

    # Train on the DISTINCT chunks, each weighted by how often it occurs (bpe_dedup_chunks):
    # same merges, counts and tie-breaks as over the full chunk list, a fraction
    # of the stream.  True / False force it.  "auto": round 1's engine made the host pass worth
    # ~1500 device merges over the full list, so it was on from 2000 merges (DEDUP_AUTO_MERGES:
    # still the rule of the sharded path, dist.py); since round 6 the device trains 1 GB to
    # vocab 32000 in 0.58 s against 0.19 s on the distinct chunks, and the host pass costs
    # 0.45-0.6 s per GB on a 256-thread host (profiles/r6_final_bench.json: the whole call 0.88 s
    # without it, 1.09 s with it) -- so a single process turns it on only for texts of
    # DEDUP_AUTO_BYTES or more, where the stream nears the 2^32-byte limit of one GPU
    #  and the distinct chunks are what still fits.
    dedup = "auto"
    DEDUP_AUTO_MERGES = 2000
    DEDUP_AUTO_BYTES = 1 << 31

    def train(self, text, vocab_size, verbose=False):
        data, offs = self._chunked(text, for_training=True)
        wexp = None
        want = (len(data) >= self.DEDUP_AUTO_BYTES) if self.dedup == "auto" else bool(self.dedup)
        if want and len(offs) > 1:
            data, offs, wexp, _ = _native.dedup_chunks(data, offs)
        self._train_on_device(data, offs, vocab_size, verbose, wexp)

    def register_special_tokens(self, special_tokens):
        self.special_tokens = special_tokens
        self.inverse_special_tokens = {idx: tok for tok, idx in special_tokens.items()}

    def decode(self, ids):
        parts = []
        for idx in ids:
            if idx in self.vocab:
                parts.append(self.vocab[idx])
            elif idx in self.inverse_special_tokens:
                parts.append(self.inverse_special_tokens[idx].encode("utf-8"))
            else:
                raise ValueError(f"invalid token id: {idx}")
        return b"".join(parts).decode("utf-8", errors="replace")

    def _decode_extra(self):
        return self.inverse_special_tokens

    def _invalid_token(self, idx):
        return ValueError(f"invalid token id: {idx}")  # regex.py:87

    def _prepare_chunk(self, chunk_bytes):
        return chunk_bytes  # GPT4Tokenizer permutes bytes here (a per-byte map)

    def _encode_chunk(self, text_bytes):
        ids, _ = self._encode_chunks([self._prepare_chunk(text_bytes)])
        return ids.tolist()

    def _encode_flat(self, data, offs):
        """encode chunks given as one byte string + start offsets (one device batch)"""
        if not data:
            return np.empty(0, np.int32), np.zeros(1, np.uint64)
        pairs, mids = self._merge_table()
        return engine().encode_batch(pairs, mids, self._prepare_chunk(data), offs)

    def encode_ordinary(self, text):
        data, offs = self._chunked(text)
        return self._encode_flat(data, offs)[0].tolist()

    def encode_ordinary_with_offsets(self, text, unit="char"):
        """(ids, spans): encode_ordinary(text) and, for every token, its (start, end) in `text` -- in characters
        (unit="char": text[start:end] covers the token), in bytes of text.encode("utf-8") (unit="byte"), or the pair of
        both lists (unit="both").  One encode plus one token_spans call; not in the reference."""
        return self._with_offsets(self.encode_ordinary, text, unit)

    def encode_ordinary_batch(self, texts):
        """encode_ordinary() of every text, as one device batch (not in the reference, whose
        encode takes one string).  Returns (ids, doc_offsets): int32 ids of all texts back to
        back and len(texts) + 1 offsets, text d being ids[doc_offsets[d]:doc_offsets[d + 1]].
        Every text is split on its own, so the ids are those of a loop over encode_ordinary."""
        enc = [t.encode("utf-8") for t in texts]
        if not enc:
            return np.empty(0, np.int32), np.zeros(1, np.uint64)
        data, offs, first = self._split_texts(texts, enc)
        ids, out_off = self._encode_flat(data, offs)
        return ids, out_off[first]

    def _split_texts(self, texts, enc):
        """Every text (enc: their UTF-8 bytes, at least one) split on its own: (the chunks' bytes back to back, chunk
        start offsets, int64 index of every text's first chunk and, last, the number of chunks)."""
        which = _NATIVE_SPLIT.get(self.compiled_pattern.pattern)
        if which is not None:
            data = b"".join(enc)
            doff = np.zeros(len(enc), dtype=np.uint64)
            np.cumsum(np.fromiter((len(e) for e in enc[:-1]), dtype=np.uint64, count=len(enc) - 1), out=doff[1:])
            offs, first = _native.split_docs(data, doff, which)
        else:  # any other pattern: the regex module, one text at a time
            pieces, first = [], [0]
            for t in texts:
                pieces += [p for p in self._split(t) if p]
                first.append(len(pieces))
            data, offs = _concat_chunks(pieces)
        return data, offs, np.ascontiguousarray(first, dtype=np.int64)

    def encode_ordinary_batch_resident(self, texts, device=None):
        """encode_ordinary_batch() with the ids left in HBM: returns (ids, doc_offsets), an int32 torch tensor on the
        GPU holding the ids of all texts back to back (a view of the buffer the engine wrote) and len(texts) + 1 int64
        offsets on the same GPU.  The host splits the texts and uploads their bytes once; ids and offsets never come
        back.  device: the GPU's index (default: the process-wide engine's)."""
        import torch
        dev = _cuda_device(device)
        enc = [t.encode("utf-8") for t in texts]
        if not any(enc):  # nothing to encode: no engine call
            return torch.empty(0, dtype=torch.int32, device=dev), torch.zeros(len(enc) + 1, dtype=torch.int64, device=dev)
        data, offs, first = self._split_texts(texts, enc)
        pairs, mids = self._merge_table()
        data = self._prepare_chunk(data)
        d_bytes = torch.from_numpy(np.frombuffer(bytearray(data), dtype=np.uint8)).to(dev)
        d_offs = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.uint64).view(np.int64)).to(dev)
        d_first = torch.from_numpy(first).to(dev)
        d_ids = torch.empty(len(data), dtype=torch.int32, device=dev)
        d_ooff = torch.empty(len(offs) + 1, dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()  # the uploads are done
        total = engine(dev.index).encode_batch_resident(pairs, mids, d_bytes.data_ptr(), len(data), d_offs.data_ptr(),
                                                        len(offs), d_ids.data_ptr(), d_ooff.data_ptr())
        return d_ids[:total], d_ooff[d_first]

    def encode_batch_rows(self, texts, row_len, device=None, **kw):
        """encode_ordinary_batch_resident() and rows_resident() in one call: texts to fixed-length rows on the GPU
        (keywords as rows_resident's).  The stream's length is known here, so the rows are sized by rows_count()."""
        ids, doff = self.encode_ordinary_batch_resident(texts, device)
        if kw.get("mode", "pack") == "pack" and "_total" not in kw:
            kw["_total"] = ids.numel() + (len(doff) - 1 if kw.get("sep") is not None else 0)
        return self.rows_resident(ids, doff, row_len, **kw)

    def encode(self, text, allowed_special="none_raise"):
        if allowed_special == "all":
            special = self.special_tokens
        elif allowed_special == "none":
            special = {}
        elif allowed_special == "none_raise":
            special = {}
            assert all(tok not in text for tok in self.special_tokens)
        elif isinstance(allowed_special, set):
            special = {k: v for k, v in self.special_tokens.items() if k in allowed_special}
        else:
            raise ValueError(f"allowed_special={allowed_special} not understood")
        if not special:
            return self.encode_ordinary(text)
        splitter = "(" + "|".join(re.escape(k) for k in special) + ")"
        parts = re.split(splitter, text)
        # one device batch for all ordinary parts; specials spliced back in order
        datas, offs_list, nchunks, base = [], [], [], 0
        for part in parts:
            if part in special:
                nchunks.append(None)
                continue
            d, o = self._chunked(part)
            datas.append(d)
            offs_list.append(o + np.uint64(base))
            nchunks.append(len(o))
            base += len(d)
        data = b"".join(datas)
        offs = np.concatenate(offs_list) if offs_list else np.empty(0, np.uint64)
        ids, out_off = self._encode_flat(data, offs)
        out, ci = [], 0
        for part, k in zip(parts, nchunks):
            if k is None:
                out.append(special[part])
            elif k:
                out.extend(ids[int(out_off[ci]):int(out_off[ci + k])].tolist())
                ci += k
        return out


class GPT4Tokenizer(RegexTokenizer):
    """cl100k_base through the same engine (gpt4.py:57-130).  Needs `tiktoken`
    for the published ranks; without it construction raises ImportError."""

    SPECIAL_TOKENS = {
        '<|endoftext|>': 100257, '<|fim_prefix|>': 100258, '<|fim_middle|>': 100259,
        '<|fim_suffix|>': 100260, '<|endofprompt|>': 100276,
    }

    def __init__(self, ranks=None):
        """ranks: None -> cl100k_base from the `tiktoken` package, as the reference does
        (gpt4.py:63-64); or the same table given directly -- a {token bytes: rank} dict, or the
        path of a `.tiktoken` file (lines of "<base64 token> <rank>") -- for machines without
        the package or without network access."""
        super().__init__(pattern=GPT4_SPLIT_PATTERN)
        if ranks is None:
            try:
                import tiktoken
                get_encoding = tiktoken.get_encoding  # (a namespace stub or a broken install is no tiktoken either)
            except (ImportError, AttributeError) as e:
                raise ImportError("GPT4Tokenizer needs the `tiktoken` package for cl100k_base ranks "
                                  "(or pass ranks= a dict / a .tiktoken file)") from e
            ranks = get_encoding("cl100k_base")._mergeable_ranks
        elif not isinstance(ranks, dict):
            ranks = load_tiktoken_ranks(ranks)
        self.merges = _recover_merges(ranks)
        vocab = {i: bytes([i]) for i in range(256)}
        for (a, b), idx in self.merges.items():
            vocab[idx] = vocab[a] + vocab[b]
        self.vocab = vocab
        self.byte_shuffle = {i: ranks[bytes([i])] for i in range(256)}
        self.inverse_byte_shuffle = {v: k for k, v in self.byte_shuffle.items()}
        self._shuffle_lut = bytes(self.byte_shuffle[i] for i in range(256))
        self._unshuffle_lut = bytes(self.inverse_byte_shuffle[i] for i in range(256))
        self.register_special_tokens(self.SPECIAL_TOKENS)

    def _prepare_chunk(self, chunk_bytes):
        return chunk_bytes.translate(self._shuffle_lut)

    def decode(self, ids):
        raw = b"".join(self.vocab[i] for i in ids).translate(self._unshuffle_lut)
        return raw.decode("utf-8", errors="replace")

    def _decode_extra(self):
        return {}  # gpt4.py:89 looks ids up in self.vocab only

    def _invalid_token(self, idx):
        return KeyError(idx)

    def _finish_bytes(self, raw):
        return raw.translate(self._unshuffle_lut)

    def _resident_blob(self, blob):
        return blob.translate(self._unshuffle_lut)

    def train(self, text, vocab_size, verbose=False):
        raise NotImplementedError

    def at_vocab(self, vocab_size):
        raise NotImplementedError  # (as train(): a GPT4Tokenizer is cl100k_base, whole)

    def save(self, file_prefix):
        raise NotImplementedError("GPT4Tokenizer cannot be saved.")

    def load(self, model_file):
        raise NotImplementedError("GPT4Tokenizer cannot be loaded.")

    def save_vocab(self, vocab_file):
        vocab = {i: bytes([self.inverse_byte_shuffle[i]]) for i in range(256)}
        for (a, b), idx in self.merges.items():
            vocab[idx] = vocab[a] + vocab[b]
        parents = {idx: pair for pair, idx in self.merges.items()}
        with open(vocab_file, "w", encoding="utf-8") as f:
            for idx, tok in vocab.items():
                if idx in parents:
                    a, b = parents[idx]
                    f.write(f"[{render_token(vocab[a])}][{render_token(vocab[b])}]"
                            f" -> [{render_token(tok)}] {idx}\n")
                else:
                    f.write(f"[{render_token(tok)}] {idx}\n")


def load_tiktoken_ranks(path):
    """A `.tiktoken` rank file -> {token bytes: rank}."""
    import base64
    ranks = {}
    with open(path, "rb") as f:
        for line in f:
            if line.strip():
                tok, rank = line.split()
                ranks[base64.b64decode(tok)] = int(rank)
    return ranks


def _split_by_ranks(ranks, token, max_rank):
    """Re-run BPE on one token's bytes using only ranks below max_rank
    (gpt4.py:11-26): the two parts left are the pair that was merged."""
    parts = [bytes([b]) for b in token]
    while True:
        best = None
        for i in range(len(parts) - 1):
            r = ranks.get(parts[i] + parts[i + 1])
            if r is not None and (best is None or r < best[0]):
                best = (r, i)
        if best is None or (max_rank is not None and best[0] >= max_rank):
            return parts
        i = best[1]
        parts[i:i + 2] = [parts[i] + parts[i + 1]]


def _recover_merges(ranks):
    """mergeable_ranks (bytes -> rank) -> {(id, id): rank}  (gpt4.py:29-46)."""
    merges = {}
    for token, rank in ranks.items():
        if len(token) == 1:
            continue
        pair = _split_by_ranks(ranks, token, rank)
        assert len(pair) == 2
        merges[(ranks[pair[0]], ranks[pair[1]])] = rank
    return merges
