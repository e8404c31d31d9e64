#!/usr/bin/env python3
"""The lifecycle of tests/test_gpu_ctx_lifecycle.py once, with nothing else in the process that talks to the HIP
runtime (no torch: the few device buffers of the resident calls come from hipMalloc through ctypes and are freed
again) -- to be run under HIP-API tracing, so that the call counts of two builds of the library can be compared and the
allocations of one balanced against its frees:

    rocprofv3 --hip-runtime-trace --stats --output-format csv -d OUT -- python3 tools/ctx_lifecycle_trace.py
    MINBPE_AMD_LIB=other/libbpe_hip.so rocprofv3 --hip-runtime-trace --stats --output-format csv -d OUT2 -- python3 tools/ctx_lifecycle_trace.py

Three engines: the work at the base sizes; at the base sizes, twice the sizes and the base sizes again; at the base
sizes.  The work: train 64 merges on 64 KiB of synth_text, encode a batch of a few hundred short chunks, then the
resident decode, spans, rows and projection of a few thousand ids.  Prints a digest of everything the engines returned
(equal for equal libraries)."""
import ctypes as C
import hashlib
import os
import sys

os.environ.setdefault("MINBPE_AMD_NO_TORCH", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import minbpe_amd  # noqa: E402
from minbpe_amd import _native as native  # noqa: E402

hip = C.CDLL("libamdhip64.so")
H2D, D2H = 1, 2


class Dev:
    """a device buffer holding a copy of a numpy array (or `nbytes` undefined bytes)"""

    def __init__(self, arr=None, nbytes=0):
        self.nbytes = max(arr.nbytes if arr is not None else nbytes, 16)
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(self.nbytes)) == 0
        self.ptr = p.value
        if arr is not None and arr.nbytes:
            assert hip.hipMemcpy(C.c_void_p(self.ptr), arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes), H2D) == 0

    def read(self, dtype, count):
        out = np.empty(count, dtype)
        if count:
            assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), C.c_size_t(out.nbytes), D2H) == 0
        return out

    def free(self):
        assert hip.hipFree(C.c_void_p(self.ptr)) == 0


MERGES = [(97, 98), (256, 99), (257, 257), (258, 100)]      # a merge list of the shape training makes, for the projection
TABLE = [bytes([i]) * (1 + i % 5) for i in range(256)] + [b"\xc3\xa9", b"\xf0\x9f\x98\x89", b"", b"xyz" * 40]


def work(e, scale, digest):
    data = minbpe_amd.synth_text(65536 * scale, 3)
    e.load_bytes(data)
    res = e.train(64)
    digest.update(repr((res["pairs"], res["counts"], res["lens"])).encode())
    rng = np.random.default_rng(11)
    offs = np.concatenate([[0], np.cumsum(rng.integers(1, 40, size=300 * scale - 1))]).astype(np.uint64)
    ids, out_off = e.encode_batch(np.array(res["pairs"], np.int32), None, data[:int(offs[-1]) + 17], offs)
    digest.update(ids.tobytes() + out_off.tobytes())
    n = 3000 * scale
    doc = np.array([0, n // 3, n // 3, n], np.uint64)
    bufs = [Dev(rng.integers(0, len(TABLE), size=n).astype(np.int32)), Dev(doc), Dev(nbytes=32)]
    d_ids, d_doc, d_off = bufs
    total = e.decode_batch_resident(d_ids.ptr, 4, n, 0, 0, 0, 0, 0)
    bufs.append(Dev(nbytes=total))
    assert e.decode_batch_resident(d_ids.ptr, 4, n, d_doc.ptr, 4, bufs[-1].ptr, total, d_off.ptr) == total
    digest.update(bufs[-1].read(np.uint8, total).tobytes() + d_off.read(np.uint64, 4).tobytes())
    bufs += [Dev(nbytes=16 * n), Dev(nbytes=16 * n)]
    digest.update(repr(e.token_spans_resident(d_ids.ptr, 4, n, d_doc.ptr, 3, bufs[-2].ptr, bufs[-1].ptr)).encode())
    digest.update(bufs[-2].read(np.int64, 2 * n).tobytes() + bufs[-1].read(np.int64, 2 * n).tobytes())
    rows = e.rows_resident(d_ids.ptr, n, d_doc.ptr, 3, 0, 1, 96, 64, 7, -1, 0, 8, 0)
    bufs.append(Dev(nbytes=8 * 96 * rows))
    assert e.rows_resident(d_ids.ptr, n, d_doc.ptr, 3, 0, 1, 96, 64, 7, -1, bufs[-1].ptr, 8, rows) == rows
    digest.update(bufs[-1].read(np.int64, 96 * rows).tobytes())
    bufs.append(Dev(rng.integers(0, 256 + len(MERGES), size=n).astype(np.int32)))
    d_pids = bufs[-1]
    n_out = e.project_resident(d_pids.ptr, 4, n, 256)
    bufs.append(Dev(nbytes=4 * n_out))
    assert e.project_resident(d_pids.ptr, 4, n, 256, d_doc.ptr, 4, bufs[-1].ptr, n_out, d_off.ptr) == n_out
    digest.update(bufs[-1].read(np.int32, n_out).tobytes() + d_off.read(np.uint64, 4).tobytes())
    for b in bufs:
        b.free()


def main():
    digest = hashlib.sha256()
    offs = np.zeros(len(TABLE) + 1, np.uint64)
    np.cumsum([len(t) for t in TABLE], out=offs[1:])
    for sizes in ([1], [1, 2, 1], [1]):
        with native.Engine(0) as e:
            e.decode_set_vocab(b"".join(TABLE), offs)
            e.project_set_merges(np.array(MERGES, np.int32))
            for scale in sizes:
                work(e, scale, digest)
    print("ctx_lifecycle_trace:", os.path.basename(os.path.dirname(native.LIB_PATH)) or ".", digest.hexdigest())


if __name__ == "__main__":
    main()
