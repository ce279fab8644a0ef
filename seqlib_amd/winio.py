"""ctypes binding of include/seqlib_amd_win.h (the assembly-window collector, part of libseqlib_amd.so) for tests and tools.

Plumbing only: the product is the C-ABI.  No CPU fallback: without the library it raises, on a host-only handle every batch entry returns SLX_ENODEVICE;
set(), counter() and quality_trim() are host only.
"""
import ctypes as C

import numpy as np

from . import _ffi, bamio

# every symbol include/seqlib_amd_win.h declares (checked by tests/test_win_host.py against the header text)
WIN_EXPORTS = ["slx_win_create", "slx_win_free", "slx_win_set", "slx_win_add_device", "slx_win_add_host", "slx_win_finish", "slx_win_view", "slx_win_download", "slx_win_clear",
               "slx_win_quality_trim", "slx_win_counter"]
COUNTERS = ("device", "windows", "skip_flags", "qual_trim", "original_strand", "wave_len", "arena_bytes", "records", "pairs", "reads", "drop_flags", "drop_no_seq", "drop_no_name",
            "drop_trimmed", "long_reads", "arena_bytes_used", "us_measure", "us_join", "us_extract", "us_entries", "us_sort", "us_gather")
HOST, AUTO = -1, -2


class Iv(C.Structure):
    _fields_ = [("chr", C.c_int32), ("pos1", C.c_int32), ("pos2", C.c_int32), ("strand", C.c_char)]


class Result(C.Structure):
    _fields_ = [("n_win", C.c_int64), ("n_reads", C.c_int64), ("total", C.c_int64), ("max_len", C.c_int64), ("d_bases", C.c_void_p), ("d_quals", C.c_void_p), ("d_offs", C.c_void_p),
                ("d_win_off", C.c_void_p), ("d_rec_of_read", C.c_void_p)]


_READY = False


def lib():
    global _READY
    L = bamio.lib()
    if not _READY:
        L.slx_win_create.argtypes = [C.c_int, C.POINTER(Iv), C.c_int64, C.POINTER(C.c_void_p)]
        L.slx_win_free.argtypes = [C.c_void_p]
        L.slx_win_free.restype = None
        L.slx_win_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_win_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        L.slx_win_add_host.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.POINTER(C.c_uint64), C.c_int64]
        L.slx_win_finish.argtypes = [C.c_void_p]
        L.slx_win_view.argtypes = [C.c_void_p, C.POINTER(Result)]
        L.slx_win_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.slx_win_clear.argtypes = [C.c_void_p]
        L.slx_win_quality_trim.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.slx_win_quality_trim.restype = None
        L.slx_win_counter.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_win_counter.restype = C.c_int64
        _READY = True
    return L


def quality_trim(qual, t):
    """BamRecord::QualityTrimmedSequence on the phred bytes -> (startpoint, endpoint)"""
    a, b = C.c_int32(), C.c_int32()
    lib().slx_win_quality_trim(bytes(qual), len(qual), t, C.byref(a), C.byref(b))
    return a.value, b.value


class Collector:
    """slx_win handle; windows: [(chr, pos1, pos2)] closed, in the caller's order"""

    def __init__(self, windows, device=AUTO, **knobs):
        self.h = C.c_void_p()
        arr = (Iv * max(len(windows), 1))(*[Iv(c, a, b, b"*") for c, a, b in windows])
        _ffi.check(lib().slx_win_create(device, arr, len(windows), C.byref(self.h)))
        for k, v in knobs.items():
            self.set(k, v)

    def set(self, key, value):
        _ffi.check(lib().slx_win_set(self.h, key.encode(), value))

    def counter(self, name):
        return int(lib().slx_win_counter(self.h, name.encode()))

    def add_device(self, d_stream, n_bytes, d_rec_off, n_records):
        """device pointers as ints"""
        _ffi.check(lib().slx_win_add_device(self.h, d_stream, n_bytes, d_rec_off, n_records))

    def add_host(self, stream, rec_off):
        arr = (C.c_uint64 * len(rec_off))(*rec_off)
        _ffi.check(lib().slx_win_add_host(self.h, bytes(stream), len(stream), arr, len(rec_off) - 1))

    def finish(self):
        _ffi.check(lib().slx_win_finish(self.h))

    def view(self):
        r = Result()
        _ffi.check(lib().slx_win_view(self.h, C.byref(r)))
        return r

    def download(self):
        """-> (bases bytes, quals bytes, offs, win_off, rec_of_read) of the finished collector"""
        r = self.view()
        bases, quals = np.zeros(max(r.total, 1), np.uint8), np.zeros(max(r.total, 1), np.uint8)
        offs, win_off, ror = np.zeros(r.n_reads + 1, np.uint64), np.zeros(r.n_win + 1, np.int64), np.zeros(max(r.n_reads, 1), np.int64)
        _ffi.check(lib().slx_win_download(self.h, bases.ctypes.data, quals.ctypes.data, offs.ctypes.data, win_off.ctypes.data, ror.ctypes.data))
        return bases[:r.total].tobytes(), quals[:r.total].tobytes(), [int(x) for x in offs], [int(x) for x in win_off], [int(x) for x in ror[:r.n_reads]]

    def clear(self):
        _ffi.check(lib().slx_win_clear(self.h))

    def close(self):
        if self.h:
            lib().slx_win_free(self.h)
            self.h = None

    def __del__(self):
        if getattr(self, "h", None):
            self.close()
