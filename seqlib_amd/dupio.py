"""ctypes binding of include/seqlib_amd_dup.h (the duplicate marker, part of libseqlib_amd.so) for tests and tools.

Plumbing only: the product is the C-ABI.  No CPU fallback: without the library it raises, without a GPU Marker() raises SLX_ENODEVICE;
library_of() and signature_host() are host only.
"""
import ctypes as C

import numpy as np

from . import _ffi, bamio

# every symbol include/seqlib_amd_dup.h declares (checked by tests/test_dup_host.py against the header text)
DUP_EXPORTS = ["slx_dup_create", "slx_dup_free", "slx_dup_set", "slx_dup_set_header", "slx_dup_add_device", "slx_dup_add_host", "slx_dup_finish", "slx_dup_apply_device",
               "slx_dup_flags_to_host", "slx_dup_clear", "slx_dup_mark_sorter", "slx_dup_file", "slx_dup_file_ex", "slx_dup_library_of", "slx_dup_signature_host", "slx_dup_counter"]
COUNTERS = ("device", "max_bytes", "wave_len", "hash_bits", "run_max", "libraries", "read_groups", "records", "ignored", "paired", "fragments", "long_records", "held_bytes", "finished",
            "pairs", "orphans", "duplicate_pairs", "duplicate_fragments", "duplicates", "hash_runs_mixed", "us_sig", "us_place", "us_commit", "us_join", "us_pairs", "us_group", "us_apply")
IGNORED, FRAGMENT, PAIRED = 0, 1, 2


class Sig(C.Structure):
    _fields_ = [("cls", C.c_int32), ("library", C.c_int32), ("refid", C.c_int32), ("reverse", C.c_int32), ("upos", C.c_int64), ("score", C.c_int64), ("hash", C.c_uint64)]


_READY = False


def lib():
    global _READY
    L = bamio.lib()
    if not _READY:
        L.slx_dup_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.slx_dup_free.argtypes = [C.c_void_p]
        L.slx_dup_free.restype = None
        L.slx_dup_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_dup_set_header.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_dup_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        L.slx_dup_add_host.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.POINTER(C.c_uint64), C.c_int64]
        L.slx_dup_finish.argtypes = [C.c_void_p]
        L.slx_dup_apply_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        L.slx_dup_flags_to_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.slx_dup_clear.argtypes = [C.c_void_p]
        L.slx_dup_mark_sorter.argtypes = [C.c_void_p, C.c_void_p]
        L.slx_dup_file.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
        L.slx_dup_file_ex.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int64]
        L.slx_dup_library_of.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_int64]
        L.slx_dup_signature_host.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, C.POINTER(C.c_uint64), C.c_int64, C.POINTER(Sig)]
        L.slx_dup_counter.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_dup_counter.restype = C.c_int64
        _READY = True
    return L


def _text(header_text):
    return header_text.encode() if isinstance(header_text, str) else bytes(header_text or b"")


def library_of(header_text, rg):
    """the library number of read group rg (bytes) under the header text"""
    t, rg = _text(header_text), bytes(rg)
    rc = lib().slx_dup_library_of(t, len(t), rg, len(rg))
    if rc < 0:
        _ffi.check(rc)
    return rc


def signature_host(stream, rec_off, header_text=None):
    """-> [(cls, library, refid, upos, reverse, score)] of the records of a host batch, by the kernels' body on the CPU"""
    t = _text(header_text)
    n = len(rec_off) - 1
    arr = (C.c_uint64 * len(rec_off))(*rec_off)
    out = (Sig * max(n, 1))()
    _ffi.check(lib().slx_dup_signature_host(t, len(t), bytes(stream), len(stream), arr, n, out))
    return [(s.cls, s.library, s.refid, s.upos, s.reverse, s.score) for s in out[:n]]


class Marker:
    """slx_dup handle"""

    def __init__(self, device=-1, header_text=None, **knobs):
        self.h = C.c_void_p()
        _ffi.check(lib().slx_dup_create(device, C.byref(self.h)))
        for k, v in knobs.items():
            self.set(k, v)
        if header_text is not None:
            self.set_header(header_text)

    def set(self, key, value):
        _ffi.check(lib().slx_dup_set(self.h, key.encode(), value))

    def set_header(self, header_text):
        t = _text(header_text)
        _ffi.check(lib().slx_dup_set_header(self.h, t, len(t)))

    def counter(self, name):
        return int(lib().slx_dup_counter(self.h, name.encode()))

    def add_device(self, d_stream, n_bytes, d_rec_off, n_records):
        """device pointers as ints"""
        _ffi.check(lib().slx_dup_add_device(self.h, d_stream, n_bytes, d_rec_off, n_records))

    def add_host(self, stream, rec_off):
        arr = (C.c_uint64 * len(rec_off))(*rec_off)
        _ffi.check(lib().slx_dup_add_host(self.h, bytes(stream), len(stream), arr, len(rec_off) - 1))

    def finish(self):
        _ffi.check(lib().slx_dup_finish(self.h))

    def apply_device(self, d_stream, n_bytes, d_rec_off, n_records, first_ordinal=0, d_ordinals=None):
        _ffi.check(lib().slx_dup_apply_device(self.h, d_stream, n_bytes, d_rec_off, n_records, first_ordinal, d_ordinals))

    def flags(self):
        """one byte per ordinal: 0 no duplicate, 1 duplicate, 2 ignored"""
        n = self.counter("records")
        out = np.zeros(max(n, 1), np.uint8)
        _ffi.check(lib().slx_dup_flags_to_host(self.h, out.ctypes.data, n))
        return [int(x) for x in out[:n]]

    def mark_sorter(self, sorter_handle):
        _ffi.check(lib().slx_dup_mark_sorter(self.h, sorter_handle))

    def mark_file(self, in_path, out_path, batch_bytes=64 << 20):
        """file to file with this marker's device, knobs and counters"""
        _ffi.check(lib().slx_dup_file_ex(self.h, str(in_path).encode(), str(out_path).encode(), batch_bytes))

    def clear(self):
        _ffi.check(lib().slx_dup_clear(self.h))

    def close(self):
        if self.h:
            lib().slx_dup_free(self.h)
            self.h = None

    def __del__(self):
        if getattr(self, "h", None):
            self.close()


def mark_file(in_path, out_path, device=-1):
    """in_path with its duplicates marked into out_path on the GPU"""
    _ffi.check(lib().slx_dup_file(str(in_path).encode(), str(out_path).encode(), device))
