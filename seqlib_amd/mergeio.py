"""ctypes binding of include/seqlib_amd_merge.h (the merge of coordinate-sorted BAM files, part of libseqlib_amd.so) for tests and tools.

Plumbing only: the product is the C-ABI and SeqLib::BamMerger of include/SeqLib/BamMerger.h.  No CPU fallback: without the library it raises, without a GPU
slx_merge_create and slx_merge_files return SLX_ENODEVICE; slx_merge_header_text is host only.
"""
import ctypes as C
import os

import numpy as np

from . import _ffi, bamio

# every symbol include/seqlib_amd_merge.h declares (checked by tests/test_merge_host.py against the header text)
EXPORTS = ["slx_merge_create", "slx_merge_free", "slx_merge_add_file", "slx_merge_header", "slx_merge_next", "slx_merge_batch_to_host", "slx_merge_run", "slx_merge_files",
           "slx_merge_header_text", "slx_merge_set", "slx_merge_counter"]
COUNTERS = ("inputs", "records", "bytes", "rounds", "refills", "us_key", "us_rank", "us_gather", "held_records", "held_bytes")
KNOBS = ("batch_bytes", "slab_bytes", "max_bytes", "by_sort")


class Batch(C.Structure):
    _fields_ = [("n_records", C.c_int64), ("n_bytes", C.c_int64), ("d_stream", C.c_void_p), ("d_rec_off", C.c_void_p), ("d_input", C.c_void_p)]


_READY = False


def lib():
    global _READY
    L = bamio.lib()
    if not _READY:
        L.slx_merge_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.slx_merge_free.argtypes = [C.c_void_p]
        L.slx_merge_free.restype = None
        L.slx_merge_add_file.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_merge_header.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        L.slx_merge_next.argtypes = [C.c_void_p, C.POINTER(Batch)]
        L.slx_merge_batch_to_host.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_void_p]
        L.slx_merge_run.argtypes = [C.c_void_p, C.c_void_p]
        L.slx_merge_files.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_char_p, C.c_int]
        L.slx_merge_header_text.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int, C.c_char_p, C.c_int64]
        L.slx_merge_header_text.restype = C.c_int64
        L.slx_merge_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_merge_counter.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_merge_counter.restype = C.c_int64
        _READY = True
    return L


def header_text(texts):
    """host only: the header text of the merge of files with these header texts, in add order ([str] -> str); raises SlxError on an ID clash"""
    raw = [t.encode() for t in texts]
    arr = (C.c_char_p * max(len(raw), 1))(*raw)
    lens = (C.c_int64 * max(len(raw), 1))(*[len(r) for r in raw])
    n = lib().slx_merge_header_text(arr, lens, len(raw), None, 0)
    if n < 0:
        _ffi.check(int(n))
    buf = C.create_string_buffer(max(n, 1))
    lib().slx_merge_header_text(arr, lens, len(raw), buf, n)
    return buf.raw[:n].decode()


class Merger:
    """slx_merge handle"""

    def __init__(self, device=-1):
        self.h = C.c_void_p()
        _ffi.check(lib().slx_merge_create(device, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            lib().slx_merge_free(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set(self, key, value):
        _ffi.check(lib().slx_merge_set(self.h, key.encode(), value))

    def counter(self, name):
        return int(lib().slx_merge_counter(self.h, name.encode()))

    def add_file(self, path):
        _ffi.check(lib().slx_merge_add_file(self.h, str(path).encode()))

    def header(self):
        """the header block of the output as bytes"""
        p, n = C.c_void_p(), C.c_int64(0)
        _ffi.check(lib().slx_merge_header(self.h, C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value)

    def next_device(self):
        """one round: a Batch whose pointers are in HBM, valid until the next call"""
        b = Batch()
        _ffi.check(lib().slx_merge_next(self.h, C.byref(b)))
        return b

    def next(self):
        """one round copied down -> (stream as bytes, [rec_off], [input of every record]); (b"", [0], []) at the end"""
        b = self.next_device()
        stream = np.zeros(max(b.n_bytes, 1), dtype=np.uint8)
        off = np.zeros(b.n_records + 1, dtype=np.uint64)
        inp = np.zeros(max(b.n_records, 1), dtype=np.uint8)
        _ffi.check(lib().slx_merge_batch_to_host(self.h, C.byref(b), stream.ctypes.data, off.ctypes.data, inp.ctypes.data))
        return stream[:b.n_bytes].tobytes(), off.tolist(), inp[:b.n_records].tolist()

    def all(self):
        """every round -> (stream, [rec_off] over the whole stream, [input])"""
        stream, off, inp = [], [0], []
        while True:
            s, o, i = self.next()
            if not i:
                return b"".join(stream), off, inp
            off += [off[-1] + x for x in o[1:]]
            stream.append(s)
            inp += i

    def run(self, writer):
        """writer: an open bamio.Writer"""
        _ffi.check(lib().slx_merge_run(self.h, writer.h))


def merge_files(in_paths, out_path, device=-1, **knobs):
    """the sorted files in_paths merged into out_path on the GPU.  knobs: batch_bytes, slab_bytes, max_bytes, by_sort (None or absent: the default).
    -> the merger's counters"""
    knobs = {k: v for k, v in knobs.items() if v is not None}
    raw = [str(p).encode() for p in in_paths]
    if not knobs:
        _ffi.check(lib().slx_merge_files((C.c_char_p * max(len(raw), 1))(*raw), len(raw), str(out_path).encode(), device))
        return {}
    m = Merger(device)
    w = None
    try:
        for k, v in knobs.items():
            m.set(k, v)
        if str(out_path) in [str(p) for p in in_paths]:
            raise _ffi.SlxError(_ffi.SLX_EINVAL, "merge_files: '%s' is an input and the output" % out_path)
        for p in in_paths:
            m.add_file(p)
        w = bamio.Writer(out_path, device)
        w.write(m.header())
        w.flush()
        m.run(w)
        w.close()
        w = None
        return {name: m.counter(name) for name in COUNTERS}
    except Exception:
        if w is not None:
            try:
                w.close()
            except _ffi.SlxError:
                pass
            if os.path.exists(str(out_path)):
                os.unlink(str(out_path))
        raise
    finally:
        m.close()
