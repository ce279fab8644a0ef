"""ctypes binding of include/seqlib_amd_sort.h (the coordinate sort of libseqlib_amd.so) for tests and tools.

Plumbing only: the product is the C-ABI and BamWriter::SortByCoordinate of include/SeqLib/BamWriter.h.  No CPU fallback: without the library it raises,
without a GPU slx_sort_create and slx_sort_file return SLX_ENODEVICE.
"""
import ctypes as C

import numpy as np

from . import _ffi, bamio

# every symbol include/seqlib_amd_sort.h declares (checked by tests/test_sort_host.py against the header text)
SORT_EXPORTS = ["slx_sort_create", "slx_sort_free", "slx_sort_add_device", "slx_sort_add_host", "slx_sort_finish", "slx_sort_to_host", "slx_sort_file", "slx_sort_file_ex",
                "slx_sort_header", "slx_sort_set", "slx_sort_counter", "slx_sort_spill", "slx_sort_file_spill"]
COUNTERS = ("records", "bytes", "segments", "slabs", "us_key", "us_sort", "us_gather", "held_records", "held_bytes", "runs", "run_bytes", "us_merge")

_READY = False


def lib():
    global _READY
    L = bamio.lib()
    if not _READY:
        L.slx_sort_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.slx_sort_free.argtypes = [C.c_void_p]
        L.slx_sort_free.restype = None
        L.slx_sort_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        L.slx_sort_add_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        L.slx_sort_finish.argtypes = [C.c_void_p, C.c_void_p]
        L.slx_sort_to_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.slx_sort_file.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
        L.slx_sort_file_ex.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        L.slx_sort_spill.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int64]
        L.slx_sort_file_spill.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p]
        L.slx_sort_header.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_int64]
        L.slx_sort_header.restype = C.c_int64
        L.slx_sort_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_sort_counter.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_sort_counter.restype = C.c_int64
        _READY = True
    return L


def header_so(text):
    """host only: the header text of a coordinate-sorted file made from text (str -> str)"""
    raw = text.encode()
    n = lib().slx_sort_header(raw, len(raw), None, 0)
    if n < 0:
        _ffi.check(int(n))
    buf = C.create_string_buffer(max(n, 1))
    lib().slx_sort_header(raw, len(raw), buf, n)
    return buf.raw[:n].decode()


class Sorter:
    """slx_sort handle"""

    def __init__(self, device=-1):
        self.h = C.c_void_p()
        _ffi.check(lib().slx_sort_create(device, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().slx_sort_free(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set(self, key, value):
        _ffi.check(lib().slx_sort_set(self.h, key.encode(), value))

    def counter(self, name):
        return int(lib().slx_sort_counter(self.h, name.encode()))

    def add_host(self, records, offsets=None):
        """records: list of whole records as bytes (block_size word included); offsets: an offset table to use instead of the records' own"""
        stream = np.frombuffer(b"".join(records), dtype=np.uint8).copy() if records else np.zeros(1, dtype=np.uint8)
        off = np.zeros(len(records) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in records], dtype=np.uint64)
        if offsets is not None:
            off = np.asarray(offsets, dtype=np.uint64)
        _ffi.check(lib().slx_sort_add_host(self.h, stream.ctypes.data, sum(len(r) for r in records), off.ctypes.data, len(records)))

    def add_device(self, d_stream, n_bytes, d_rec_off, n_records):
        """device pointers as ints, e.g. the fields of a bamio.Batch"""
        _ffi.check(lib().slx_sort_add_device(self.h, d_stream, n_bytes, d_rec_off, n_records))

    def finish(self, writer):
        """writer: an open bamio.Writer"""
        _ffi.check(lib().slx_sort_finish(self.h, writer.h))

    def to_host(self):
        """-> (sorted stream as bytes, [rec_off], [input ordinal of every output record]); empties the sorter"""
        nb, n = self.counter("held_bytes"), self.counter("held_records")
        buf = np.zeros(max(nb, 1), dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uint64)
        perm = np.zeros(max(n, 1), dtype=np.uint32)
        _ffi.check(lib().slx_sort_to_host(self.h, buf.ctypes.data, nb, off.ctypes.data, perm.ctypes.data))
        return buf[:nb].tobytes(), off.tolist(), perm[:n].tolist()

    def spill(self, prefix, bam_header=b""):
        """run files "<prefix>.run%04d.bam" for what passes max_bytes, each with the header block bam_header; None: off"""
        _ffi.check(lib().slx_sort_spill(self.h, None if prefix is None else str(prefix).encode(), bam_header, len(bam_header)))

    def sort_file(self, in_path, out_path, spill_prefix=None):
        """file to file with this sorter's device, knobs and counters; spill_prefix: sorted runs go to disk where max_bytes is passed, and are merged"""
        if spill_prefix is None:
            _ffi.check(lib().slx_sort_file_ex(self.h, str(in_path).encode(), str(out_path).encode()))
        else:
            _ffi.check(lib().slx_sort_file_spill(self.h, str(in_path).encode(), str(out_path).encode(), str(spill_prefix).encode()))


def sort_file(in_path, out_path, device=-1, spill_prefix=None, **knobs):
    """in_path coordinate-sorted into out_path on the GPU.  knobs: max_bytes, slab_bytes, batch_bytes (None or absent: the default).  spill_prefix: where the
    run files of an input beyond max_bytes go (None: such an input is refused).  -> the sorter's counters"""
    knobs = {k: v for k, v in knobs.items() if v is not None}
    if not knobs and spill_prefix is None:
        _ffi.check(lib().slx_sort_file(str(in_path).encode(), str(out_path).encode(), device))
        return {}
    s = Sorter(device)
    try:
        for k, v in knobs.items():
            s.set(k, v)
        s.sort_file(in_path, out_path, spill_prefix)
        return {name: s.counter(name) for name in COUNTERS}
    finally:
        s.close()
