"""ctypes binding of libbpe_hip.so (include/bpe_hip.h).

The HIP library is the product: there is no CPU fallback.  If the shared
library has not been built, importing this module raises ImportError with the
build command; if no GPU is present, Engine() raises RuntimeError.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MINBPE_AMD_LIB", os.path.join(_HERE, "lib", "libbpe_hip.so"))

BPE_OK = 0
BPE_E_HIP = -1
BPE_E_ARG = -2
BPE_E_EMPTY_STATS = -3
BPE_E_STATE = -4
BPE_E_CAP = -5
BPE_E_LIMIT = -6
BPE_E_INTERNAL = -7

PROF_KINDS = ("widen", "pair_count", "argmax", "merge", "table", "encode", "decode")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -m minbpe_amd.build` "
        "(hipcc --offload-arch=gfx950). minbpe_amd has no CPU fallback.")



def _load_library():
    """PyTorch ships private copies of libamdhip64 / libhsa-runtime64.  Two HIP runtimes cannot
    both bring up the same GPU in one process (the second one reports "No HIP GPUs are
    available"; measured, tools/gpu_probe.sh), and which copy a process ends up with is decided
    by load order: with torch imported first, this library binds to torch's copy (same SONAME)
    and the process has one runtime.  So when torch is installed it is imported before the
    library is loaded -- the order bench.py and the GPU tests run in.  MINBPE_AMD_NO_TORCH=1
    skips this (for processes that will never import torch)."""
    if "torch" not in sys.modules and not os.environ.get("MINBPE_AMD_NO_TORCH"):
        try:
            import importlib.util
            if importlib.util.find_spec("torch") is not None:
                import torch  # noqa: F401
        except Exception:
            pass
    return C.CDLL(LIB_PATH)


_lib = _load_library()
_p = C.c_void_p
# bpe_allreduce_fn (include/bpe_hip.h): (user, device_buffer, count, dtype, op, hip_stream) -> 0 on success
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_void_p)
DT_INT32, DT_INT64, OP_SUM, OP_MIN = 0, 1, 0, 1
_u64 = C.c_uint64
_i32 = C.c_int32

_SIGS = {
    "bpe_create": (C.c_int, [C.c_int, C.POINTER(_p)]),
    "bpe_destroy": (None, [_p]),
    "bpe_last_error": (C.c_char_p, [_p]),
    "bpe_set_stream": (C.c_int, [_p, _p]),
    "bpe_set_option": (C.c_int, [_p, C.c_char_p, C.c_int64]),
    "bpe_load_bytes": (C.c_int, [_p, _p, _u64, _p, _u64]),
    "bpe_load_bytes_weighted": (C.c_int, [_p, _p, _u64, _p, _u64, _p]),
    "bpe_load_ids": (C.c_int, [_p, _p, _u64, _p, _u64]),
    "bpe_get_stats": (C.c_int, [_p, C.POINTER(_u64)]),
    "bpe_read_stats": (C.c_int, [_p, _p, _p, _p, _p, _u64, C.POINTER(_u64)]),
    "bpe_argmax": (C.c_int, [_p, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_u64)]),
    "bpe_merge": (C.c_int, [_p, _i32, _i32, _i32, C.POINTER(_u64)]),
    "bpe_len": (C.c_int, [_p, C.POINTER(_u64)]),
    "bpe_read_ids": (C.c_int, [_p, _p, _u64]),
    "bpe_read_chunk_starts": (C.c_int, [_p, _p, _u64, C.POINTER(_u64)]),
    "bpe_train": (C.c_int, [_p, _i32, _p, _p, _p, _p, C.POINTER(_i32)]),
    "bpe_dp_begin": (C.c_int, [_p, _i32, _i32, _i32]),
    "bpe_dp_buffers": (C.c_int, [_p, C.POINTER(_p), C.POINTER(_u64), C.POINTER(_p), C.POINTER(_u64),
                                 C.POINTER(_p)]),
    "bpe_dp_table_ready": (C.c_int, [_p]),
    "bpe_dp_select": (C.c_int, [_p, _i32]),
    "bpe_dp_merge": (C.c_int, [_p, _i32]),
    "bpe_dp_apply": (C.c_int, [_p, _i32]),
    "bpe_dp_poll": (C.c_int, [_p, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_u64),
                              C.POINTER(_u64), C.POINTER(_i32)]),
    "bpe_dp_end": (C.c_int, [_p]),
    "bpe_comm_available": (C.c_int, []),
    "bpe_comm_unique_id": (C.c_int, [_p]),
    "bpe_comm_init": (C.c_int, [_p, _i32, _i32, _p]),
    "bpe_comm_destroy": (C.c_int, [_p]),
    "bpe_dp_train": (C.c_int, [_p, _i32, _p, _p, _p, C.POINTER(_i32)]),
    "bpe_dp_train_cb": (C.c_int, [_p, _i32, _i32, _i32, C.c_void_p, _p, _p, _p, _p, C.POINTER(_i32)]),
    "bpe_encode_batch": (C.c_int, [_p, _p, _p, _i32, _p, _u64, _p, _u64, _p, _p, C.POINTER(_u64)]),
    "bpe_encode_batch_resident": (C.c_int, [_p, _p, _p, _i32, _p, _u64, _p, _u64, _p, _p, C.POINTER(_u64)]),
    "bpe_decode_set_vocab": (C.c_int, [_p, _p, _p, _i32]),
    "bpe_decode_batch": (C.c_int, [_p, _p, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "bpe_decode_read": (C.c_int, [_p, _p, _u64, _p, _u64, _p]),
    "bpe_decode_set_sparse": (C.c_int, [_p, _p, _i32, _i32]),
    "bpe_decode_batch_resident": (C.c_int, [_p, _p, _i32, _u64, _p, _u64, _p, _u64, _p, C.POINTER(_u64),
                                            C.POINTER(_u64)]),
    "bpe_rows_resident": (C.c_int, [_p, _p, _u64, _p, _u64, _i32, C.c_uint32, _u64, _u64, _i32, _i32, _p, _i32, _u64,
                                    _p, _p, _p, C.POINTER(_u64), C.POINTER(_u64)]),
    "bpe_token_spans_resident": (C.c_int, [_p, _p, _i32, _u64, _p, _u64, _p, _p, C.POINTER(_u64), C.POINTER(_u64),
                                           C.POINTER(_u64), C.POINTER(_u64)]),
    "bpe_project_set_merges": (C.c_int, [_p, _p, _i32, _p, _i32]),
    "bpe_project_resident": (C.c_int, [_p, _p, _i32, _u64, _i32, _p, _u64, _p, _u64, _p, C.POINTER(_u64),
                                       C.POINTER(_u64)]),
    "bpe_count_resident": (C.c_int, [_p, _p, _i32, _u64, _p, _u64, _i32, C.POINTER(_u64)]),
    "bpe_count_fold": (C.c_int, [_p, _i32, _p, _u64, _i32, _p, _p]),
    "bpe_select_docs_resident": (C.c_int, [_p, _p, _i32, _u64, _p, _u64, _p, _u64, _u64, C.c_uint32, _p, _u64, _p,
                                           C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "bpe_dup_docs_resident": (C.c_int, [_p, _p, _i32, _u64, _p, _u64, _u64, C.c_uint32, _p, _p, C.POINTER(_u64),
                                        C.POINTER(_u64)]),
    "bpe_minhash_resident": (C.c_int, [_p, _p, _i32, _u64, _p, _u64, _u64, C.c_uint32, C.c_uint32, C.c_uint32, _u64, _p,
                                       _u64, C.POINTER(_u64)]),
    "bpe_minhash_agree_resident": (C.c_int, [_p, _p, _u64, C.c_uint32, _p, _p, _u64, _p, C.POINTER(_u64)]),
    "bpe_ngram_index_resident": (C.c_int, [_p, _p, _i32, _u64, _p, _u64, C.c_uint32, C.POINTER(_u64), C.POINTER(_u64),
                                           C.POINTER(_u64), C.POINTER(_u64)]),
    "bpe_ngram_overlap_resident": (C.c_int, [_p, _u64, _p, _i32, _u64, _p, _u64, _u64, C.c_uint32, _p, _p, _p, _p,
                                             C.POINTER(_u64), C.POINTER(_u64)]),
    "bpe_repeat_stats_resident": (C.c_int, [_p, _p, _i32, _u64, _p, _u64, C.c_uint32, _u64, C.c_uint32, _p, _p, _p, _p,
                                            _p, _p, _p, C.POINTER(_u64), C.POINTER(_u64)]),
    "bpe_dup_spans_resident": (C.c_int, [_p, _p, _i32, _u64, _p, _u64, C.c_uint32, _u64, C.c_uint32, _p, _p, _p, _p,
                                         _p, _p, _p, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "bpe_keep_ids_resident": (C.c_int, [_p, _p, _i32, _u64, _p, _u64, _p, C.c_uint32, C.c_uint32, _p, _u64, _p,
                                        C.POINTER(_u64), C.POINTER(_u64)]),
    "bpe_segment_docs_resident": (C.c_int, [_p, _p, _i32, _u64, _p, _u64, _p, _u64, C.c_uint32, _p, _u64, _p, _u64,
                                            _p, _p, _p, _p, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "bpe_segment_marks_resident": (C.c_int, [_p, _p, _p, _u64, _p, _u64, _p, C.POINTER(_u64)]),
    "bpe_prof_reset": (C.c_int, [_p]),
    "bpe_prof_read": (C.c_int, [_p, _p, _p, _p]),
    "bpe_encode_uses_16bit": (C.c_int, [_p, C.c_int32]),
    "bpe_train_stats": (C.c_int, [_p, _p]),
    "bpe_train_stats_ex": (C.c_int, [_p, _p, C.c_int]),
    "bpe_utf8_encode": (C.c_int, [C.c_int, _p, _u64, _p, _u64, C.POINTER(_u64), C.c_int]),
    "bpe_split": (C.c_int, [C.c_int, _p, _u64, _p, _u64, C.POINTER(_u64), C.c_int]),
    "bpe_dedup_chunks": (C.c_int, [_p, _u64, _p, _u64, _p, _p, _p, C.POINTER(_u64), C.POINTER(_u64),
                                  C.POINTER(_u64), C.c_int]),
    "bpe_split_docs": (C.c_int, [C.c_int, _p, _u64, _p, _u64, _p, _u64, C.POINTER(_u64), _p, C.c_int]),
    "bpe_synth_text": (C.c_int, [_p, _u64, _u64]),
    "bpe_version": (C.c_char_p, []),
}
for _name, (_res, _args) in _SIGS.items():
    _fn = getattr(_lib, _name)
    _fn.restype = _res
    _fn.argtypes = _args


def exported_symbols():
    """Names bound above (tests check them against include/bpe_hip.h)."""
    return sorted(_SIGS)


def version():
    return _lib.bpe_version().decode()


def synth_text(n: int, seed: int) -> bytes:
    """Deterministic synthetic UTF-8 text (host only, no GPU needed)."""
    buf = np.empty(n, dtype=np.uint8)
    rc = _lib.bpe_synth_text(buf.ctypes.data_as(_p), n, seed)
    if rc != BPE_OK:
        raise RuntimeError(f"bpe_synth_text failed: {rc}")
    return buf.tobytes()


def utf8_encode(text: str, threads: int = 0):
    """text.encode("utf-8") (basic.py:25, regex.py:44) -- by all host threads for a long text: CPython encodes with one
    thread, 0.7 s per GB of a str with characters beyond the BMP, more than the device side of a whole train().  A
    compact CPython str is a header followed by its code points, 1, 2 or 4 bytes each; the library transcodes them in
    place (bpe_utf8_encode).  The layout is checked, not assumed: interpreter and version, the object's state bits, its
    size, and the first and last code points read through the pointer against the str itself -- anything that does not
    fit (another interpreter, a non-compact or short or ASCII str, a lone surrogate) goes to str.encode.  Returns bytes
    or a uint8 array (both are buffers: what every consumer here takes)."""
    n = len(text)
    if n < (1 << 22) or sys.implementation.name != "cpython" or sys.version_info[:2] != (3, 10) or type(text) is not str:
        return text.encode("utf-8")
    state = C.c_uint8.from_address(id(text) + 32).value  # PyASCIIObject.state: interned:2 kind:3 compact:1 ascii:1 ready:1
    kind, compact, ascii_, ready = (state >> 2) & 7, (state >> 5) & 1, (state >> 6) & 1, (state >> 7) & 1
    if not (compact and ready) or ascii_ or kind not in (1, 2, 4) or sys.getsizeof(text) != 72 + (n + 1) * kind:
        return text.encode("utf-8")  # (an ASCII str encodes by memcpy; a cached utf-8 copy changes the size: both rare here)
    ptr = id(text) + 72  # sizeof(PyCompactUnicodeObject)
    ctype = {1: C.c_uint8, 2: C.c_uint16, 4: C.c_uint32}[kind]
    probe = (ctype * 8).from_address(ptr), (ctype * 8).from_address(ptr + (n - 8) * kind)
    if [ord(c) for c in text[:8]] != list(probe[0]) or [ord(c) for c in text[-8:]] != list(probe[1]):
        return text.encode("utf-8")
    nb = _u64(0)
    if _lib.bpe_utf8_encode(kind, C.c_void_p(ptr), n, None, 0, C.byref(nb), threads) != BPE_OK:
        return text.encode("utf-8")  # (a lone surrogate: str.encode raises the reference's own exception)
    out = np.empty(nb.value, np.uint8)
    if _lib.bpe_utf8_encode(kind, C.c_void_p(ptr), n, _ptr(out), len(out), C.byref(nb), threads) != BPE_OK:
        return text.encode("utf-8")
    return out


def split_offsets(data: bytes, which: int, threads: int = 0):
    """Chunk start offsets of regex.findall(GPT-2 | GPT-4 split pattern) over UTF-8 `data`
    (host only).  which: 2 or 4."""
    buf = np.frombuffer(data, dtype=np.uint8)
    n = _u64(0)
    out = np.empty(len(buf) // 3 + 16, np.uint64)  # GPT-style chunks average > 4 bytes
    rc = _lib.bpe_split(which, _ptr(buf) if len(buf) else None, len(buf), _ptr(out), len(out), C.byref(n), threads)
    if rc == BPE_E_CAP:  # unusually short chunks: now we know the count
        out = np.empty(n.value, np.uint64)
        rc = _lib.bpe_split(which, _ptr(buf), len(buf), _ptr(out), len(out), C.byref(n), threads)
    if rc != BPE_OK:
        raise RuntimeError(f"bpe_split failed: {rc}")
    return out[:n.value].copy() if n.value * 2 < len(out) else out[:n.value]


def split_docs(data: bytes, doc_offsets, which: int, threads: int = 0):
    """split_offsets for documents laid out back to back: every document is split on its own.
    Returns (chunk start offsets, index of each document's first chunk [n_docs + 1])."""
    buf = np.frombuffer(data, dtype=np.uint8)
    doff = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
    first = np.zeros(len(doff) + 1, np.uint64)
    n = _u64(0)
    out = np.empty(len(buf) // 3 + len(doff) + 16, np.uint64)
    args = (which, _ptr(buf) if len(buf) else None, len(buf), _ptr(doff) if len(doff) else None, len(doff))
    rc = _lib.bpe_split_docs(*args, _ptr(out), len(out), C.byref(n), _ptr(first), threads)
    if rc == BPE_E_CAP:
        out = np.empty(n.value, np.uint64)
        rc = _lib.bpe_split_docs(*args, _ptr(out), len(out), C.byref(n), _ptr(first), threads)
    if rc != BPE_OK:
        raise RuntimeError(f"bpe_split_docs failed: {rc}")
    return out[:n.value].copy(), first


def dedup_chunks(data: bytes, offsets, threads: int = 0):
    """Distinct chunks of (data, chunk start offsets) in order of first appearance, one copy
    per set bit of the multiplicity (host only).  Returns (data2, offsets2, weight_exp uint8,
    n_distinct)."""
    buf = np.frombuffer(data, dtype=np.uint8)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    out = np.empty(max(len(buf), 1), np.uint8)
    ooff = np.empty(max(len(off), 1), np.uint64)
    wexp = np.empty(max(len(off), 1), np.uint8)
    nb, nc, nd = _u64(0), _u64(0), _u64(0)
    rc = _lib.bpe_dedup_chunks(_ptr(buf) if len(buf) else None, len(buf), _ptr(off) if len(off) else None,
                               len(off), _ptr(out), _ptr(ooff), _ptr(wexp), C.byref(nb), C.byref(nc),
                               C.byref(nd), threads)
    if rc != BPE_OK:
        raise RuntimeError(f"bpe_dedup_chunks failed: {rc}")
    return out[:nb.value].tobytes(), ooff[:nc.value].copy(), wexp[:nc.value].copy(), int(nd.value)


def count_fold(pairs, counts, vocab_size=None, want_curve=True):
    """bpe_count_fold (host only): pairs [M, 2] int32 in merge order, counts a histogram of at least 256 + M bins in the
    layout of Engine.count_resident (non-negative integers).  Returns (folded, curve): the histogram at vocab_size as
    uint64 [len(counts)] (None without a vocab_size), and the tokens at every size 256 .. 256 + M as int64 [M + 1] (None
    with want_curve=False).  ValueError for a list of another shape than training makes, a vocab_size outside
    [256, 256 + M], too few bins or a negative count; OverflowError when a sum does not fit (the curve: int64)."""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    arr = np.asarray(counts)
    if arr.ndim != 1 or (arr.size and arr.dtype.kind not in "iu"):
        raise TypeError("counts must be a 1-D array of integers")
    if arr.dtype.kind == "i" and arr.size and int(arr.min()) < 0:
        raise ValueError("counts must not be negative")
    cnt = np.ascontiguousarray(arr, dtype=np.uint64)
    M = len(pairs)
    folded = None if vocab_size is None else np.empty(len(cnt), np.uint64)
    curve = np.empty(M + 1, np.uint64) if want_curve else None
    rc = _lib.bpe_count_fold(_ptr(pairs) if M else None, M, _ptr(cnt) if len(cnt) else None, len(cnt),
                             256 + M if vocab_size is None else int(vocab_size), _ptr(folded), _ptr(curve))
    if rc == BPE_E_LIMIT:
        raise OverflowError("the folded counts pass 2^64")
    if rc == BPE_E_ARG:
        raise ValueError("bpe_count_fold: a merge list that does not have the shape training makes, a vocab_size outside "
                         "[256, 256 + M], or fewer than 256 + M bins")
    if rc != BPE_OK:
        raise RuntimeError(f"bpe_count_fold failed: {rc}")
    if curve is not None:
        if int(curve[0]) >= 2**63:  # (the curve descends with k: its first entry is the largest)
            raise OverflowError("the token counts pass 2^63")
        curve = curve.astype(np.int64)
    return folded, curve


class InvalidToken(Exception):
    """bpe_decode_batch met an id outside the vocab table; args[0] = its position."""


class OutputTooSmall(ValueError):
    """bpe_decode_batch_resident was given fewer bytes of room than the batch decodes to; needed = that number."""

    def __init__(self, needed, msg):
        super().__init__(msg)
        self.needed = needed


class BadDocOffsets(ValueError):
    """bpe_rows_resident met document offsets that descend or lie beyond the ids; index = the first such entry."""

    def __init__(self, index, msg):
        super().__init__(msg)
        self.index = index


class RowsTooSmall(ValueError):
    """bpe_rows_resident was given room for fewer rows than the batch makes; needed = that number."""

    def __init__(self, needed, msg):
        super().__init__(msg)
        self.needed = needed


class BadSelection(IndexError):
    """bpe_select_docs_resident met an index outside [0, n_docs); index = the lowest such position of the selection."""

    def __init__(self, index, msg):
        super().__init__(msg)
        self.index = index


class BadPair(IndexError):
    """bpe_minhash_agree_resident met a pair that names no document; index = the lowest such position of the pairs."""

    def __init__(self, index, msg):
        super().__init__(msg)
        self.index = index


ROWS_PACK, ROWS_PER_DOC = 0, 1
ROWS_HAS_SEP, ROWS_TRUNC_LEFT, ROWS_PAD_LEFT = 1, 2, 4
SELECT_TAIL = 1
SPANS_ANYWHERE = 2
KEEP_DROP = 1
SEG_BREAK, SEG_SKIP = 1, 2
SEG_TAG_DOC = 1


class BadSegment(IndexError):
    """bpe_segment_marks_resident met a range that descends, overlaps the one before or leaves [0, n]; index = the
    lowest such range."""

    def __init__(self, index, msg):
        super().__init__(msg)
        self.index = index


class SegmentsTooSmall(OutputTooSmall):
    """bpe_segment_docs_resident was given too little room; needed, needed_segments = the ids and the segments of the
    stream."""

    def __init__(self, needed, needed_segments, msg):
        super().__init__(needed, msg)
        self.needed_segments = needed_segments


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_p)


class Engine:
    """One ctx = one GPU.  Thin, typed wrapper; all compute is in the library."""

    def __init__(self, device: int = 0):
        h = _p()
        rc = _lib.bpe_create(device, C.byref(h))
        if rc != BPE_OK:
            raise RuntimeError(
                "minbpe_amd needs an AMD GPU (gfx950): "
                + (_lib.bpe_last_error(None) or b"").decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.bpe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- errors ------------------------------------------------------------
    def _check(self, rc):
        if rc == BPE_OK:
            return
        msg = (_lib.bpe_last_error(self._h) or b"").decode()
        if rc == BPE_E_EMPTY_STATS:
            # the reference's failure mode: max() over an empty dict (basic.py:35)
            raise ValueError("max() arg is an empty sequence")
        if rc == BPE_E_ARG:
            raise ValueError(msg)
        raise RuntimeError(f"libbpe_hip error {rc}: {msg}")

    # -- options -------------------------------------------------------------
    def set_option(self, name: str, value: int):
        self._check(_lib.bpe_set_option(self._h, name.encode(), int(value)))

    def set_stream(self, stream_handle: int):
        self._check(_lib.bpe_set_stream(self._h, _p(stream_handle)))

    # -- input -----------------------------------------------------------------
    @staticmethod
    def _offsets(offsets):
        if offsets is None:
            return None, 0
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        return off, len(off)

    def load_bytes(self, data, offsets=None, weight_exp=None):
        """weight_exp (uint8 per chunk): pairs inside chunk c count 2**weight_exp[c] times."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        off, n_off = self._offsets(offsets)
        self._keep = (buf, off)
        if weight_exp is None:
            self._check(_lib.bpe_load_bytes(self._h, _ptr(buf) if len(buf) else None, len(buf),
                                            _ptr(off), n_off))
            return
        w = np.ascontiguousarray(weight_exp, dtype=np.uint8)
        if off is None or len(w) != n_off:
            raise ValueError("weight_exp needs one entry per chunk offset")
        self._check(_lib.bpe_load_bytes_weighted(self._h, _ptr(buf) if len(buf) else None, len(buf),
                                                 _ptr(off), n_off, _ptr(w)))

    def load_ids(self, ids, offsets=None):
        arr = np.ascontiguousarray(ids, dtype=np.int32)
        off, n_off = self._offsets(offsets)
        self._check(_lib.bpe_load_ids(self._h, _ptr(arr) if len(arr) else None, len(arr),
                                      _ptr(off), n_off))

    # -- single steps ---------------------------------------------------------------
    def get_stats(self):
        """[( (a,b), count, first_pos )] in the reference's dict order."""
        n = _u64(0)
        self._check(_lib.bpe_get_stats(self._h, C.byref(n)))
        cap = max(int(n.value), 1)
        a = np.empty(cap, np.int32)
        b = np.empty(cap, np.int32)
        cnt = np.empty(cap, np.uint64)
        first = np.empty(cap, np.uint64)
        got = _u64(0)
        self._check(_lib.bpe_read_stats(self._h, _ptr(a), _ptr(b), _ptr(cnt), _ptr(first), cap,
                                        C.byref(got)))
        k = int(got.value)
        order = np.argsort(first[:k], kind="stable")
        return [((int(a[i]), int(b[i])), int(cnt[i]), int(first[i])) for i in order]

    def argmax(self):
        a, b, cnt = _i32(0), _i32(0), _u64(0)
        self._check(_lib.bpe_argmax(self._h, C.byref(a), C.byref(b), C.byref(cnt)))
        return (a.value, b.value), cnt.value

    def merge(self, pair, idx):
        n = _u64(0)
        self._check(_lib.bpe_merge(self._h, int(pair[0]), int(pair[1]), int(idx), C.byref(n)))
        return n.value

    def __len__(self):
        n = _u64(0)
        self._check(_lib.bpe_len(self._h, C.byref(n)))
        return n.value

    def read_ids(self):
        n = len(self)
        out = np.empty(max(n, 1), np.int32)
        self._check(_lib.bpe_read_ids(self._h, _ptr(out), len(out)))
        return out[:n]

    def read_chunk_starts(self):
        n = len(self)
        out = np.empty(max(n, 1), np.uint64)
        got = _u64(0)
        self._check(_lib.bpe_read_chunk_starts(self._h, _ptr(out), len(out), C.byref(got)))
        return out[:got.value]

    # -- training ---------------------------------------------------------------------
    def train(self, num_merges: int, want_iter_ms: bool = False):
        """Returns dict(pairs, counts, lens, iter_ms, n_done); raises ValueError
        like the reference when the pair table runs empty (basic.py:35)."""
        nm = max(num_merges, 1)
        pairs = np.zeros(2 * nm, np.int32)
        counts = np.zeros(nm, np.uint64)
        lens = np.zeros(nm, np.uint64)
        ms = np.zeros(nm, np.float64) if want_iter_ms else None
        done = _i32(0)
        rc = _lib.bpe_train(self._h, num_merges, _ptr(pairs), _ptr(counts), _ptr(ms), _ptr(lens),
                            C.byref(done))
        d = done.value
        self.last_train = dict(
            pairs=list(map(tuple, pairs[:2 * d].reshape(d, 2).tolist())),
            counts=counts[:d].tolist(), lens=lens[:d].tolist(),
            iter_ms=None if ms is None else ms[:d].copy(), n_done=d)
        self._check(rc)
        return self.last_train

    # -- data-parallel stepping (minbpe_amd/dist.py drives these) ------------------------
    def dp_begin(self, num_merges, rank, nranks):
        self._check(_lib.bpe_dp_begin(self._h, num_merges, rank, nranks))

    def dp_buffers(self):
        """(table_ptr, table_count, delta_ptr, delta_count, tiekey_ptr): raw device
        pointers of the three all-reduce payloads (int32, int32, int64 x 2)."""
        t, d, k = _p(), _p(), _p()
        tc, dc = _u64(0), _u64(0)
        self._check(_lib.bpe_dp_buffers(self._h, C.byref(t), C.byref(tc), C.byref(d), C.byref(dc),
                                        C.byref(k)))
        return t.value, tc.value, d.value, dc.value, k.value

    def dp_table_ready(self):
        self._check(_lib.bpe_dp_table_ready(self._h))

    def dp_select(self, i):
        self._check(_lib.bpe_dp_select(self._h, i))

    def dp_merge(self, i):
        self._check(_lib.bpe_dp_merge(self._h, i))

    def dp_apply(self, i):
        self._check(_lib.bpe_dp_apply(self._h, i))

    def dp_poll(self, i):
        """(pair, count, local_len, status) of iteration i; blocks until reported."""
        a, b, st = _i32(0), _i32(0), _i32(0)
        cnt, ln = _u64(0), _u64(0)
        self._check(_lib.bpe_dp_poll(self._h, i, C.byref(a), C.byref(b), C.byref(cnt), C.byref(ln),
                                     C.byref(st)))
        return (a.value, b.value), cnt.value, ln.value, st.value

    def dp_end(self):
        self._check(_lib.bpe_dp_end(self._h))

    # -- RCCL called from inside the library ---------------------------------------------
    @staticmethod
    def comm_available() -> bool:
        """librccl can be loaded in this process (bpe_comm_available)."""
        return bool(_lib.bpe_comm_available())

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = np.zeros(128, np.uint8)
        rc = _lib.bpe_comm_unique_id(_ptr(buf))
        if rc != BPE_OK:
            raise RuntimeError("bpe_comm_unique_id failed: " + (_lib.bpe_last_error(None) or b"").decode())
        return buf.tobytes()

    def comm_init(self, rank: int, nranks: int, uid: bytes):
        buf = np.frombuffer(uid, np.uint8)
        self._check(_lib.bpe_comm_init(self._h, rank, nranks, _ptr(buf)))

    def comm_destroy(self):
        self._check(_lib.bpe_comm_destroy(self._h))

    def dp_train(self, num_merges: int):
        """Sharded training with the collectives issued by the library (after comm_init).
        Same result dict as train(); lens are global."""
        nm = max(num_merges, 1)
        pairs = np.zeros(2 * nm, np.int32)
        counts = np.zeros(nm, np.uint64)
        lens = np.zeros(nm, np.uint64)
        done = _i32(0)
        rc = _lib.bpe_dp_train(self._h, num_merges, _ptr(pairs), _ptr(counts), _ptr(lens), C.byref(done))
        d = done.value
        self.last_train = dict(
            pairs=list(map(tuple, pairs[:2 * d].reshape(d, 2).tolist())),
            counts=counts[:d].tolist(), lens=lens[:d].tolist(), iter_ms=None, n_done=d)
        self._check(rc)
        return self.last_train

    def dp_train_cb(self, num_merges: int, rank: int, nranks: int, allreduce):
        """Sharded training (the same loop as dp_train) with the collectives handed to `allreduce(ptr, count, dtype,
        op, stream)`: all-reduce `count` elements at device address `ptr` in place across the ranks (dtype DT_INT32 /
        DT_INT64, op OP_SUM / OP_MIN), ordered after the work already on HIP stream `stream`; raise to fail.
        Same result dict as train(); lens are global."""
        nm = max(num_merges, 1)
        pairs = np.zeros(2 * nm, np.int32)
        counts = np.zeros(nm, np.uint64)
        lens = np.zeros(nm, np.uint64)
        done = _i32(0)
        raised = []

        def _cb(_user, buf, count, dtype, op, stream):
            try:
                allreduce(buf, count, dtype, op, stream)
                return 0
            except BaseException as e:  # (must not propagate through the C frames)
                raised.append(e)
                return 1

        cb = ALLREDUCE_FN(_cb)
        rc = _lib.bpe_dp_train_cb(self._h, num_merges, rank, nranks, C.cast(cb, C.c_void_p), None, _ptr(pairs),
                                  _ptr(counts), _ptr(lens), C.byref(done))
        d = done.value
        self.last_train = dict(
            pairs=list(map(tuple, pairs[:2 * d].reshape(d, 2).tolist())),
            counts=counts[:d].tolist(), lens=lens[:d].tolist(), iter_ms=None, n_done=d)
        if raised:
            raise raised[0]
        self._check(rc)
        return self.last_train

    # -- encoding ----------------------------------------------------------------------
    def encode_batch(self, pairs, merge_ids, data, offsets=None):
        """pairs: (M,2) int32 in priority order; merge_ids: (M,) int32 or None.
        Returns (ids ndarray int32, out_offsets ndarray uint64 of n_chunks+1)."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        off, n_off = self._offsets(offsets)
        n_chunks = n_off if off is not None else 1
        pm = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1)
        M = len(pm) // 2
        mi = None if merge_ids is None else np.ascontiguousarray(merge_ids, dtype=np.int32)
        out = np.empty(max(len(buf), 1), np.int32)
        oo = np.zeros(n_chunks + 1, np.uint64)
        n_out = _u64(0)
        self._check(_lib.bpe_encode_batch(self._h, _ptr(pm) if M else None, _ptr(mi), M,
                                          _ptr(buf) if len(buf) else None, len(buf), _ptr(off),
                                          n_off, _ptr(out), _ptr(oo), C.byref(n_out)))
        return out[:n_out.value], oo

    # -- decoding ----------------------------------------------------------------------
    def encode_batch_resident(self, pairs, merge_ids, d_bytes: int, n: int, d_offsets: int, n_chunks: int,
                              d_ids_out: int, d_out_offsets: int) -> int:
        """encode_batch with the batch and its outputs in HBM: d_bytes (n bytes), d_offsets (n_chunks uint64),
        d_ids_out (room for n int32), d_out_offsets (n_chunks + 1 uint64) are device addresses (e.g. torch
        tensor.data_ptr()).  Returns the number of tokens written."""
        p = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1)
        mids = None if merge_ids is None else np.ascontiguousarray(merge_ids, dtype=np.int32)
        total = _u64(0)
        self._check(_lib.bpe_encode_batch_resident(
            self._h, _ptr(p) if len(p) else None, None if mids is None else _ptr(mids), len(p) // 2,
            C.c_void_p(d_bytes), n, C.c_void_p(d_offsets), n_chunks, C.c_void_p(d_ids_out), C.c_void_p(d_out_offsets),
            C.byref(total)))
        return int(total.value)

    def decode_set_vocab(self, blob: bytes, offsets):
        """Vocab table: entry i = blob[offsets[i]:offsets[i+1]]; stays resident in HBM."""
        buf = np.frombuffer(blob, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._check(_lib.bpe_decode_set_vocab(self._h, _ptr(buf) if len(buf) else None, _ptr(off),
                                              len(off) - 1))

    def decode_batch(self, ids, doc_offsets=None):
        """ids: int32 table indices.  Returns the concatenated bytes, or (bytes, byte offset of
        each token position in doc_offsets).  An index outside the table raises
        InvalidToken(position)."""
        arr = np.ascontiguousarray(ids, dtype=np.int32)
        nb, bad = _u64(0), _u64(0)
        rc = _lib.bpe_decode_batch(self._h, _ptr(arr) if len(arr) else None, len(arr), C.byref(nb),
                                   C.byref(bad))
        if rc == BPE_E_ARG and bad.value != 0xFFFFFFFFFFFFFFFF:
            raise InvalidToken(int(bad.value))
        self._check(rc)
        out = np.empty(max(nb.value, 1), np.uint8)
        if doc_offsets is None:
            self._check(_lib.bpe_decode_read(self._h, _ptr(out), len(out), None, 0, None))
            return out[:nb.value].tobytes()
        doff = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        boff = np.zeros(len(doff), np.uint64)
        self._check(_lib.bpe_decode_read(self._h, _ptr(out), len(out), _ptr(doff), len(doff), _ptr(boff)))
        return out[:nb.value].tobytes(), boff

    def decode_set_sparse(self, sparse_ids, v_dense: int):
        """Ids outside [0, v_dense) that decode_batch_resident accepts: sparse_ids[j] (int32, strictly ascending) is
        entry v_dense + j of the table given to decode_set_vocab, which resets the list."""
        arr = np.ascontiguousarray(sparse_ids, dtype=np.int32)
        self._check(_lib.bpe_decode_set_sparse(self._h, _ptr(arr) if len(arr) else None, len(arr), int(v_dense)))

    def decode_batch_resident(self, d_ids: int, id_width: int, n: int, d_doc_off: int, k: int, d_out: int, out_cap: int,
                              d_boff: int) -> int:
        """decode_batch with the ids and the results in HBM: d_ids (n ids of id_width = 4 or 8 bytes), d_doc_off
        (k uint64 token positions), d_out (room for out_cap bytes; 0 = only count), d_boff (k uint64) are device
        addresses (e.g. torch tensor.data_ptr()).  Returns the number of bytes the batch decodes to.  An id that does
        not decode raises InvalidToken(position); too little room raises OutputTooSmall."""
        nb, bad = _u64(0), _u64(0)
        rc = _lib.bpe_decode_batch_resident(self._h, C.c_void_p(d_ids), id_width, n, C.c_void_p(d_doc_off), k,
                                            C.c_void_p(d_out), out_cap, C.c_void_p(d_boff), C.byref(nb), C.byref(bad))
        if rc == BPE_E_ARG and bad.value != 0xFFFFFFFFFFFFFFFF:
            raise InvalidToken(int(bad.value))
        if rc == BPE_E_CAP:
            raise OutputTooSmall(int(nb.value), (_lib.bpe_last_error(self._h) or b"").decode())
        self._check(rc)
        return int(nb.value)

    # -- resident training rows ------------------------------------------------------
    def rows_resident(self, d_ids: int, n: int, d_doc_off: int, n_docs: int, mode: int, flags: int, row_len: int,
                      stride: int, sep: int, pad: int, d_rows: int, row_width: int, rows_cap: int, d_doc_index: int = 0,
                      d_pos: int = 0, d_lengths: int = 0) -> int:
        """bpe_rows_resident: d_ids (n int32), d_doc_off (n_docs + 1 uint64), d_rows (rows_cap rows of row_len elements
        of row_width = 4 or 8 bytes; 0 = only count) and the int32 companions (0 = none) are device addresses (e.g.
        torch tensor.data_ptr()).  mode ROWS_PACK / ROWS_PER_DOC, flags ROWS_HAS_SEP | ROWS_TRUNC_LEFT | ROWS_PAD_LEFT.
        Returns the number of rows.  Offsets that descend or pass n raise BadDocOffsets(entry); too little room raises
        RowsTooSmall."""
        nr, bad = _u64(0), _u64(0)
        rc = _lib.bpe_rows_resident(self._h, C.c_void_p(d_ids), n, C.c_void_p(d_doc_off), n_docs, mode, flags, row_len,
                                    stride, sep, pad, C.c_void_p(d_rows), row_width, rows_cap, C.c_void_p(d_doc_index),
                                    C.c_void_p(d_pos), C.c_void_p(d_lengths), C.byref(nr), C.byref(bad))
        if rc == BPE_E_ARG and bad.value != 0xFFFFFFFFFFFFFFFF:
            raise BadDocOffsets(int(bad.value), (_lib.bpe_last_error(self._h) or b"").decode())
        if rc == BPE_E_CAP:
            raise RowsTooSmall(int(nr.value), (_lib.bpe_last_error(self._h) or b"").decode())
        self._check(rc)
        return int(nr.value)

    # -- resident token spans --------------------------------------------------------
    def token_spans_resident(self, d_ids: int, id_width: int, n: int, d_doc_off: int = 0, n_docs: int = 0,
                             d_byte_spans: int = 0, d_char_spans: int = 0):
        """bpe_token_spans_resident: d_ids (n ids of id_width = 4 or 8 bytes), d_doc_off (n_docs + 1 uint64; 0 = the batch
        is one document) and the two int64 [n, 2] span arrays (0 = not wanted) are device addresses (e.g. torch
        tensor.data_ptr()).  Returns (total bytes, total characters) of the batch.  An id that does not decode raises
        InvalidToken(position); offsets that descend or pass n raise BadDocOffsets(entry)."""
        nb, nc, bad, bad_doc = _u64(0), _u64(0), _u64(0), _u64(0)
        rc = _lib.bpe_token_spans_resident(self._h, C.c_void_p(d_ids), id_width, n, C.c_void_p(d_doc_off), n_docs,
                                           C.c_void_p(d_byte_spans), C.c_void_p(d_char_spans), C.byref(nb), C.byref(nc),
                                           C.byref(bad), C.byref(bad_doc))
        if rc == BPE_E_ARG and bad.value != 0xFFFFFFFFFFFFFFFF:
            raise InvalidToken(int(bad.value))
        if rc == BPE_E_ARG and bad_doc.value != 0xFFFFFFFFFFFFFFFF:
            raise BadDocOffsets(int(bad_doc.value), (_lib.bpe_last_error(self._h) or b"").decode())
        self._check(rc)
        return int(nb.value), int(nc.value)

    # -- projection onto a smaller vocabulary ------------------------------------------
    def project_set_merges(self, pairs, pass_ids=()):
        """bpe_project_set_merges: pairs [M, 2] int32 in merge order (merge r makes id 256 + r), pass_ids the ids outside
        [0, 256 + M) that pass through unchanged (int32, strictly ascending).  A list that does not have the shape
        training makes raises ValueError."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        pas = np.ascontiguousarray(pass_ids, dtype=np.int32).reshape(-1)
        self._check(_lib.bpe_project_set_merges(self._h, _ptr(pairs) if len(pairs) else None, len(pairs),
                                                _ptr(pas) if len(pas) else None, len(pas)))

    def project_resident(self, d_ids: int, id_width: int, n: int, vocab_size: int, d_doc_off: int = 0, k: int = 0,
                         d_out: int = 0, out_cap: int = 0, d_ooff: int = 0) -> int:
        """bpe_project_resident: d_ids (n ids of id_width = 4 or 8 bytes), d_doc_off (k uint64 token positions), d_out
        (room for out_cap ids of the same width; 0 = only count), d_ooff (k uint64) are device addresses (e.g. torch
        tensor.data_ptr()).  Returns the number of ids the batch projects to.  An id that does not project raises
        InvalidToken(position); too little room raises OutputTooSmall."""
        no, bad = _u64(0), _u64(0)
        rc = _lib.bpe_project_resident(self._h, C.c_void_p(d_ids), id_width, n, int(vocab_size), C.c_void_p(d_doc_off), k,
                                       C.c_void_p(d_out), out_cap, C.c_void_p(d_ooff), C.byref(no), C.byref(bad))
        if rc == BPE_E_ARG and bad.value != 0xFFFFFFFFFFFFFFFF:
            raise InvalidToken(int(bad.value))
        if rc == BPE_E_CAP:
            raise OutputTooSmall(int(no.value), (_lib.bpe_last_error(self._h) or b"").decode())
        self._check(rc)
        return int(no.value)

    # -- token counts ------------------------------------------------------------------
    def count_resident(self, d_ids: int, id_width: int, n: int, d_counts: int, n_bins: int, accumulate: bool = False):
        """bpe_count_resident: d_ids (n ids of id_width = 4 or 8 bytes) and d_counts (n_bins uint64) are device addresses
        (e.g. torch tensor.data_ptr()); the bins are those of the list given to project_set_merges, n_bins = 256 + M +
        the number of pass ids.  accumulate: add to what d_counts holds.  An id that has no bin raises
        InvalidToken(position), and d_counts is then unchanged."""
        bad = _u64(0)
        rc = _lib.bpe_count_resident(self._h, C.c_void_p(d_ids), id_width, n, C.c_void_p(d_counts), n_bins,
                                     1 if accumulate else 0, C.byref(bad))
        if rc == BPE_E_ARG and bad.value != 0xFFFFFFFFFFFFFFFF:
            raise InvalidToken(int(bad.value))
        self._check(rc)

    # -- document selection ------------------------------------------------------------
    def select_docs_resident(self, d_ids: int, id_width: int, n: int, d_doc_off: int, n_docs: int, d_index: int, m: int,
                             max_len: int = 0, flags: int = 0, d_out: int = 0, out_cap: int = 0, d_ooff: int = 0) -> int:
        """bpe_select_docs_resident: d_ids (n ids of id_width = 4 or 8 bytes), d_doc_off (n_docs + 1 uint64), d_index
        (m int64 document numbers), d_out (room for out_cap ids of the same width; 0 = only count) and d_ooff (m + 1
        uint64, always written when the call counts) are device addresses (e.g. torch tensor.data_ptr()).  max_len 0 =
        whole documents, flags SELECT_TAIL = the last max_len ids of each.  Returns the number of ids selected.  Offsets
        that descend or pass n raise BadDocOffsets(entry), an index outside [0, n_docs) BadSelection(position); too
        little room raises OutputTooSmall."""
        no, bad_doc, bad_sel = _u64(0), _u64(0), _u64(0)
        rc = _lib.bpe_select_docs_resident(self._h, C.c_void_p(d_ids), id_width, n, C.c_void_p(d_doc_off), n_docs,
                                           C.c_void_p(d_index), m, int(max_len), flags, C.c_void_p(d_out), out_cap,
                                           C.c_void_p(d_ooff), C.byref(no), C.byref(bad_doc), C.byref(bad_sel))
        if rc == BPE_E_ARG and bad_doc.value != 0xFFFFFFFFFFFFFFFF:
            raise BadDocOffsets(int(bad_doc.value), (_lib.bpe_last_error(self._h) or b"").decode())
        if rc == BPE_E_ARG and bad_sel.value != 0xFFFFFFFFFFFFFFFF:
            raise BadSelection(int(bad_sel.value), (_lib.bpe_last_error(self._h) or b"").decode())
        if rc == BPE_E_CAP:
            raise OutputTooSmall(int(no.value), (_lib.bpe_last_error(self._h) or b"").decode())
        self._check(rc)
        return int(no.value)

    # -- document de-duplication -------------------------------------------------------
    def dup_docs_resident(self, d_ids: int, id_width: int, n: int, d_doc_off: int, n_docs: int, max_len: int = 0,
                          flags: int = 0, d_first: int = 0, d_counts: int = 0) -> int:
        """bpe_dup_docs_resident: d_ids (n ids of id_width = 4 or 8 bytes), d_doc_off (n_docs + 1 uint64), d_first
        (n_docs int64) and d_counts (n_docs uint64; 0 = not wanted) are device addresses (e.g. torch tensor.data_ptr()).
        Documents are compared by the slices select_docs_resident emits for the same max_len and flags.  Returns the
        number of distinct documents.  Offsets that descend or pass n raise BadDocOffsets(entry), and nothing is
        written then."""
        nd, bad_doc = _u64(0), _u64(0)
        rc = _lib.bpe_dup_docs_resident(self._h, C.c_void_p(d_ids), id_width, n, C.c_void_p(d_doc_off), n_docs,
                                        int(max_len), flags, C.c_void_p(d_first), C.c_void_p(d_counts), C.byref(nd),
                                        C.byref(bad_doc))
        if rc == BPE_E_ARG and bad_doc.value != 0xFFFFFFFFFFFFFFFF:
            raise BadDocOffsets(int(bad_doc.value), (_lib.bpe_last_error(self._h) or b"").decode())
        self._check(rc)
        return int(nd.value)

    # -- near-duplicate documents ------------------------------------------------------
    def minhash_resident(self, d_ids: int, id_width: int, n: int, d_doc_off: int, n_docs: int, max_len: int = 0,
                         flags: int = 0, ngram: int = 5, n_perm: int = 128, seed: int = 0, d_sig: int = 0,
                         sig_cap: int = 0):
        """bpe_minhash_resident: d_ids (n ids of id_width = 4 or 8 bytes), d_doc_off (n_docs + 1 uint64) and d_sig (room
        for sig_cap >= n_docs * n_perm int32 words) are device addresses (e.g. torch tensor.data_ptr()).  Documents are
        cut as select_docs_resident cuts them for the same max_len and flags.  Offsets that descend or pass n raise
        BadDocOffsets(entry), too little room raises OutputTooSmall; nothing is written then."""
        bad_doc = _u64(0)
        rc = _lib.bpe_minhash_resident(self._h, C.c_void_p(d_ids), id_width, n, C.c_void_p(d_doc_off), n_docs, int(max_len),
                                       flags, ngram, n_perm, int(seed) & 0xFFFFFFFFFFFFFFFF, C.c_void_p(d_sig), sig_cap,
                                       C.byref(bad_doc))
        if rc == BPE_E_ARG and bad_doc.value != 0xFFFFFFFFFFFFFFFF:
            raise BadDocOffsets(int(bad_doc.value), (_lib.bpe_last_error(self._h) or b"").decode())
        if rc == BPE_E_CAP:
            raise OutputTooSmall(n_docs * n_perm, (_lib.bpe_last_error(self._h) or b"").decode())
        self._check(rc)

    def minhash_agree_resident(self, d_sig: int, n_docs: int, n_perm: int, d_a: int, d_b: int, m: int, d_agree: int):
        """bpe_minhash_agree_resident: d_sig (int32 [n_docs][n_perm]), d_a and d_b (m int64 document numbers each) and
        d_agree (m int32) are device addresses.  A pair outside [0, n_docs) raises BadPair(position), and nothing is
        written then."""
        bad = _u64(0)
        rc = _lib.bpe_minhash_agree_resident(self._h, C.c_void_p(d_sig), n_docs, n_perm, C.c_void_p(d_a), C.c_void_p(d_b),
                                             m, C.c_void_p(d_agree), C.byref(bad))
        if rc == BPE_E_ARG and bad.value != 0xFFFFFFFFFFFFFFFF:
            raise BadPair(int(bad.value), (_lib.bpe_last_error(self._h) or b"").decode())
        self._check(rc)

    # -- n-gram overlap with a reference set -------------------------------------------
    def ngram_index_resident(self, d_ref_ids: int, id_width: int, n_ref: int, d_ref_off: int, n_ref_docs: int,
                             ngram: int = 13):
        """bpe_ngram_index_resident: d_ref_ids (n_ref ids of id_width = 4 or 8 bytes) and d_ref_off (n_ref_docs + 1
        uint64) are device addresses (e.g. torch tensor.data_ptr()); the engine keeps its own copy, and ONE index: this
        one replaces any earlier one.  Returns (index_id, n_windows, n_distinct).  Offsets that descend or pass n_ref
        raise BadDocOffsets(entry); a call that fails leaves the engine without an index."""
        iid, nw, nd, bad_doc = _u64(0), _u64(0), _u64(0), _u64(0)
        rc = _lib.bpe_ngram_index_resident(self._h, C.c_void_p(d_ref_ids), id_width, n_ref, C.c_void_p(d_ref_off),
                                           n_ref_docs, ngram, C.byref(iid), C.byref(nw), C.byref(nd), C.byref(bad_doc))
        if rc == BPE_E_ARG and bad_doc.value != 0xFFFFFFFFFFFFFFFF:
            raise BadDocOffsets(int(bad_doc.value), (_lib.bpe_last_error(self._h) or b"").decode())
        self._check(rc)
        return int(iid.value), int(nw.value), int(nd.value)

    def ngram_overlap_resident(self, index_id: int, d_ids: int, id_width: int, n: int, d_doc_off: int, n_docs: int,
                               max_len: int = 0, flags: int = 0, d_hits: int = 0, d_first: int = 0, d_ref_pos: int = 0,
                               d_starts: int = 0) -> int:
        """bpe_ngram_overlap_resident: d_ids (n ids of id_width = 4 or 8 bytes), d_doc_off (n_docs + 1 uint64), d_hits
        and, where wanted (0 = not), d_first and d_ref_pos (n_docs int64 each) and d_starts (n uint8) are device
        addresses.  Documents are cut as select_docs_resident cuts them for the same max_len and flags.  Returns the
        number of documents with a hit.  Offsets that descend or pass n raise BadDocOffsets(entry), an index_id that is
        not the engine's current index raises RuntimeError; nothing is written then."""
        nh, bad_doc = _u64(0), _u64(0)
        rc = _lib.bpe_ngram_overlap_resident(self._h, index_id, C.c_void_p(d_ids), id_width, n, C.c_void_p(d_doc_off),
                                             n_docs, int(max_len), flags, C.c_void_p(d_hits), C.c_void_p(d_first),
                                             C.c_void_p(d_ref_pos), C.c_void_p(d_starts), C.byref(nh), C.byref(bad_doc))
        if rc == BPE_E_ARG and bad_doc.value != 0xFFFFFFFFFFFFFFFF:
            raise BadDocOffsets(int(bad_doc.value), (_lib.bpe_last_error(self._h) or b"").decode())
        self._check(rc)
        return int(nh.value)

    # -- repetition statistics ---------------------------------------------------------
    def repeat_stats_resident(self, d_ids: int, id_width: int, n: int, d_doc_off: int, n_docs: int, ngram: int = 5,
                              max_len: int = 0, flags: int = 0, d_length: int = 0, d_windows: int = 0, d_distinct: int = 0,
                              d_covered: int = 0, d_top_count: int = 0, d_top_pos: int = 0, d_marks: int = 0) -> int:
        """bpe_repeat_stats_resident: d_ids (n ids of id_width = 4 or 8 bytes), d_doc_off (n_docs + 1 uint64) and, where
        wanted (0 = not), the six columns (n_docs int64 each) and d_marks (n uint8) are device addresses.  Documents are
        cut as select_docs_resident cuts them for the same max_len and flags.  Returns the number of documents that
        hold a repeated window of `ngram` ids.  Offsets that descend or pass n raise BadDocOffsets(entry); nothing is
        written then."""
        nr, bad_doc = _u64(0), _u64(0)
        rc = _lib.bpe_repeat_stats_resident(self._h, C.c_void_p(d_ids), id_width, n, C.c_void_p(d_doc_off), n_docs, ngram,
                                            int(max_len), flags, C.c_void_p(d_length), C.c_void_p(d_windows),
                                            C.c_void_p(d_distinct), C.c_void_p(d_covered), C.c_void_p(d_top_count),
                                            C.c_void_p(d_top_pos), C.c_void_p(d_marks), C.byref(nr), C.byref(bad_doc))
        if rc == BPE_E_ARG and bad_doc.value != 0xFFFFFFFFFFFFFFFF:
            raise BadDocOffsets(int(bad_doc.value), (_lib.bpe_last_error(self._h) or b"").decode())
        self._check(rc)
        return int(nr.value)

    # -- span de-duplication -----------------------------------------------------------
    def dup_spans_resident(self, d_ids: int, id_width: int, n: int, d_doc_off: int, n_docs: int, ngram: int = 50,
                           max_len: int = 0, flags: int = 0, d_length: int = 0, d_windows: int = 0, d_seen: int = 0,
                           d_covered: int = 0, d_first: int = 0, d_src_pos: int = 0, d_marks: int = 0):
        """bpe_dup_spans_resident: d_ids (n ids of id_width = 4 or 8 bytes), d_doc_off (n_docs + 1 uint64) and, where
        wanted (0 = not), the six columns (n_docs int64 each) and d_marks (n uint8) are device addresses.  Documents are
        cut as select_docs_resident cuts them for the same max_len and flags; flags SPANS_ANYWHERE = a window is seen
        if it starts anywhere earlier in the stream, not only in an earlier document.  Returns (documents with a seen
        window, windows, distinct windows).  Offsets that descend or pass n raise BadDocOffsets(entry); nothing is
        written then."""
        ns, nw, nd, bad_doc = _u64(0), _u64(0), _u64(0), _u64(0)
        rc = _lib.bpe_dup_spans_resident(self._h, C.c_void_p(d_ids), id_width, n, C.c_void_p(d_doc_off), n_docs, ngram,
                                         int(max_len), flags, C.c_void_p(d_length), C.c_void_p(d_windows),
                                         C.c_void_p(d_seen), C.c_void_p(d_covered), C.c_void_p(d_first),
                                         C.c_void_p(d_src_pos), C.c_void_p(d_marks), C.byref(ns), C.byref(nw),
                                         C.byref(nd), C.byref(bad_doc))
        if rc == BPE_E_ARG and bad_doc.value != 0xFFFFFFFFFFFFFFFF:
            raise BadDocOffsets(int(bad_doc.value), (_lib.bpe_last_error(self._h) or b"").decode())
        self._check(rc)
        return int(ns.value), int(nw.value), int(nd.value)

    def keep_ids_resident(self, d_ids: int, id_width: int, n: int, d_doc_off: int, n_docs: int, d_mask: int,
                          bits: int = 0xFF, flags: int = 0, d_out: int = 0, out_cap: int = 0, d_ooff: int = 0) -> int:
        """bpe_keep_ids_resident: d_ids (n ids of id_width = 4 or 8 bytes), d_doc_off (n_docs + 1 uint64), d_mask (n
        uint8), d_out (room for out_cap ids of the same width; 0 = only count) and d_ooff (n_docs + 1 uint64, always
        written when the call counts) are device addresses.  A position inside the documents is kept iff mask & bits is
        not 0, with flags KEEP_DROP iff it is 0.  Returns the number of ids kept.  Offsets that descend or pass n raise
        BadDocOffsets(entry); too little room raises OutputTooSmall."""
        no, bad_doc = _u64(0), _u64(0)
        rc = _lib.bpe_keep_ids_resident(self._h, C.c_void_p(d_ids), id_width, n, C.c_void_p(d_doc_off), n_docs,
                                        C.c_void_p(d_mask), bits, flags, C.c_void_p(d_out), out_cap, C.c_void_p(d_ooff),
                                        C.byref(no), C.byref(bad_doc))
        if rc == BPE_E_ARG and bad_doc.value != 0xFFFFFFFFFFFFFFFF:
            raise BadDocOffsets(int(bad_doc.value), (_lib.bpe_last_error(self._h) or b"").decode())
        if rc == BPE_E_CAP:
            raise OutputTooSmall(int(no.value), (_lib.bpe_last_error(self._h) or b"").decode())
        self._check(rc)
        return int(no.value)

    # -- segments of documents ---------------------------------------------------------
    def segment_docs_resident(self, d_ids: int, id_width: int, n: int, d_doc_off: int, n_docs: int, d_class: int = 0,
                              n_class: int = 0, flags: int = 0, d_out: int = 0, out_cap: int = 0, d_seg_off: int = 0,
                              seg_cap: int = 0, d_seg_doc: int = 0, d_src_start: int = 0, d_src_end: int = 0,
                              d_doc_seg_off: int = 0):
        """bpe_segment_docs_resident: d_ids (n ids of id_width = 4 or 8 bytes), d_doc_off (n_docs + 1 uint64), d_class
        (n_class uint8: SEG_BREAK | SEG_SKIP per id), d_out (room for out_cap ids of the same width; 0 = only count),
        d_seg_off (seg_cap + 1 uint64), the columns d_seg_doc, d_src_start, d_src_end (seg_cap int64 each, 0 = not
        wanted) and d_doc_seg_off (n_docs + 1 uint64, 0 = not wanted) are device addresses.  flags SEG_TAG_DOC = every
        segment is preceded by an id holding its document's number.  Returns (ids of the segment stream, segments).
        Offsets that descend or pass n raise BadDocOffsets(entry); too little room raises SegmentsTooSmall."""
        no, ns, bad_doc = _u64(0), _u64(0), _u64(0)
        rc = _lib.bpe_segment_docs_resident(self._h, C.c_void_p(d_ids), id_width, n, C.c_void_p(d_doc_off), n_docs,
                                            C.c_void_p(d_class), n_class, flags, C.c_void_p(d_out), out_cap,
                                            C.c_void_p(d_seg_off), seg_cap, C.c_void_p(d_seg_doc), C.c_void_p(d_src_start),
                                            C.c_void_p(d_src_end), C.c_void_p(d_doc_seg_off), C.byref(no), C.byref(ns),
                                            C.byref(bad_doc))
        if rc == BPE_E_ARG and bad_doc.value != 0xFFFFFFFFFFFFFFFF:
            raise BadDocOffsets(int(bad_doc.value), (_lib.bpe_last_error(self._h) or b"").decode())
        if rc == BPE_E_CAP:
            raise SegmentsTooSmall(int(no.value), int(ns.value), (_lib.bpe_last_error(self._h) or b"").decode())
        self._check(rc)
        return int(no.value), int(ns.value)

    def segment_marks_resident(self, d_src_start: int, d_src_end: int, n_seg: int, d_seg_val: int, n: int, d_marks: int):
        """bpe_segment_marks_resident: d_src_start, d_src_end (n_seg int64 each), d_seg_val (n_seg uint8) and d_marks (n
        uint8, all written) are device addresses: marks[p] = val[s] inside range s, 0 elsewhere.  Ranges that descend,
        overlap or leave [0, n] raise BadSegment(entry); nothing is written then."""
        bad = _u64(0)
        rc = _lib.bpe_segment_marks_resident(self._h, C.c_void_p(d_src_start), C.c_void_p(d_src_end), n_seg,
                                             C.c_void_p(d_seg_val), n, C.c_void_p(d_marks), C.byref(bad))
        if rc == BPE_E_ARG and bad.value != 0xFFFFFFFFFFFFFFFF:
            raise BadSegment(int(bad.value), (_lib.bpe_last_error(self._h) or b"").decode())
        self._check(rc)

    # -- measurement ----------------------------------------------------------------
    def prof_reset(self):
        self._check(_lib.bpe_prof_reset(self._h))

    def train_stats(self):
        """dict(dense, sparse, index_builds, slots, lean, deferred, chained, steps, selections) of the last train()
        (bpe_train_stats_ex): passes by kind, merges done by lean iterations / chain steps, merges handed back to the
        general path, merges that needed no selection of their own, chain steps, chain steps that selected; slot_ids = ids per
        slot the stream ended in (1024, or 256 once it was re-packed for sparse passes); fused_steps = chain steps that were
        one launch (k_step.hip); aa_in_chain = merges of a pair with a == b that chain steps did themselves (option
        "chain_aa") instead of handing them back; shared_first = chain steps whose batch held a first token twice (option
        "chain_share_first")."""
        out = np.zeros(13, np.uint64)
        self._check(_lib.bpe_train_stats_ex(self._h, _ptr(out), 13))
        return dict(dense=int(out[0]), sparse=int(out[1]), index_builds=int(out[2]), slots=int(out[3]),
                    lean=int(out[4]), deferred=int(out[5]), chained=int(out[6]), steps=int(out[7]),
                    selections=int(out[8]), slot_ids=int(out[9]), fused_steps=int(out[10]), aa_in_chain=int(out[11]),
                    shared_first=int(out[12]))

    def prof_read(self):
        k = len(PROF_KINDS)
        ms = np.zeros(k, np.float64)
        launches = np.zeros(k, np.uint64)
        nbytes = np.zeros(k, np.uint64)
        self._check(_lib.bpe_prof_read(self._h, _ptr(ms), _ptr(launches), _ptr(nbytes)))
        return {name: dict(ms=float(ms[i]), launches=int(launches[i]), alg_bytes=int(nbytes[i]))
                for i, name in enumerate(PROF_KINDS)}
