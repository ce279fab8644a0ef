"""ctypes binding of include/seqlib_amd_grc.h (interval queries, part of libseqlib_amd.so) for tests and tools.

Plumbing only: the product is the C-ABI and SeqLib::GenomicRegionCollection of include/SeqLib/GenomicRegionCollection.h.  No CPU fallback for batches: without the
library it raises, SLX_GRC_HOST (and SLX_GRC_AUTO without a GPU) gives a host-only object on which sorted, merged and query_host work and every batch entry returns SLX_ENODEVICE.
"""
import ctypes as C

import numpy as np

from . import _ffi, bamio

# every symbol include/seqlib_amd_grc.h declares (checked by tests/test_grc_host.py against the header text)
GRC_EXPORTS = ["slx_grc_create", "slx_grc_free", "slx_grc_set", "slx_grc_sorted", "slx_grc_merged", "slx_grc_query_host", "slx_grc_overlaps", "slx_grc_count",
               "slx_grc_overlaps_device", "slx_grc_overlaps_host", "slx_grc_subject_counts", "slx_grc_clear_counts", "slx_grc_result_free", "slx_grc_counter"]
COUNTERS = ("device", "subjects", "chrs", "queries", "queries_lane", "queries_wave", "pairs", "records", "long_records", "merged", "us_build", "us_count", "us_fill", "us_records", "us_merge")
KNOBS = ("wave_range", "slice_queries", "long_cigar")
SLX_GRC_HOST, SLX_GRC_AUTO = -1, -2


class Iv(C.Structure):
    _fields_ = [("chr", C.c_int32), ("pos1", C.c_int32), ("pos2", C.c_int32), ("strand", C.c_char)]


class Result(C.Structure):
    _fields_ = [("n_queries", C.c_int64), ("n_pairs", C.c_int64), ("count", C.POINTER(C.c_uint32)), ("width", C.POINTER(C.c_int64)), ("offset", C.POINTER(C.c_int64)),
                ("query_id", C.POINTER(C.c_int32)), ("subject_id", C.POINTER(C.c_int32)), ("pos1", C.POINTER(C.c_int32)), ("pos2", C.POINTER(C.c_int32)),
                ("d_count", C.c_void_p), ("d_width", C.c_void_p), ("d_offset", C.c_void_p), ("d_query_id", C.c_void_p), ("d_subject_id", C.c_void_p), ("d_pos1", C.c_void_p),
                ("d_pos2", C.c_void_p)]


_READY = False


def lib():
    global _READY
    L = bamio.lib()
    if not _READY:
        L.slx_grc_create.argtypes = [C.c_int, C.POINTER(Iv), C.c_int64, C.POINTER(C.c_void_p)]
        L.slx_grc_free.argtypes = [C.c_void_p]
        L.slx_grc_free.restype = None
        L.slx_grc_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_grc_sorted.argtypes = [C.c_void_p, C.POINTER(Iv), C.c_void_p, C.c_void_p, C.c_void_p]
        L.slx_grc_merged.argtypes = [C.c_void_p, C.POINTER(Iv), C.c_int64, C.POINTER(C.c_int64)]
        L.slx_grc_query_host.argtypes = [C.c_void_p, C.POINTER(Iv), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.slx_grc_overlaps.argtypes = [C.c_void_p, C.POINTER(Iv), C.c_int64, C.c_int, C.POINTER(Result)]
        L.slx_grc_count.argtypes = [C.c_void_p, C.POINTER(Iv), C.c_int64, C.c_int, C.c_int, C.c_void_p]
        L.slx_grc_overlaps_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.POINTER(Result)]
        L.slx_grc_overlaps_host.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.POINTER(C.c_uint64), C.c_int64, C.c_int, C.POINTER(Result)]
        L.slx_grc_subject_counts.argtypes = [C.c_void_p, C.c_void_p]
        L.slx_grc_clear_counts.argtypes = [C.c_void_p]
        L.slx_grc_result_free.argtypes = [C.POINTER(Result)]
        L.slx_grc_result_free.restype = None
        L.slx_grc_counter.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_grc_counter.restype = C.c_int64
        _READY = True
    return L


def ivs(intervals):
    """[(chr, pos1, pos2[, strand])] -> a ctypes array of Iv (one spare entry, so that an empty list has an address)"""
    arr = (Iv * (len(intervals) + 1))()
    for i, t in enumerate(intervals):
        arr[i].chr, arr[i].pos1, arr[i].pos2 = t[0], t[1], t[2]
        arr[i].strand = (t[3] if len(t) > 3 else "*").encode()
    return arr


def _tuples(arr, n):
    return [(arr[i].chr, arr[i].pos1, arr[i].pos2, arr[i].strand.decode()) for i in range(n)]


def _take(res, pairs=True):
    """a Result's host arrays as Python lists, then freed"""
    nq, npairs = res.n_queries, res.n_pairs
    out = {"n_pairs": npairs, "count": [res.count[i] for i in range(nq)], "offset": [res.offset[i] for i in range(nq + 1)]}
    if pairs:
        out["width"] = [res.width[i] for i in range(nq)]
        out["pairs"] = [(res.query_id[k], res.subject_id[k], res.pos1[k], res.pos2[k]) for k in range(npairs)]
    lib().slx_grc_result_free(C.byref(res))
    return out


class Collection:
    """slx_grc handle over [(chr, pos1, pos2[, strand])]; device: a GPU's number, SLX_GRC_HOST or SLX_GRC_AUTO"""

    def __init__(self, intervals, device=SLX_GRC_AUTO):
        self.h = C.c_void_p()
        self.n = len(intervals)
        _ffi.check(lib().slx_grc_create(device, ivs(intervals), self.n, C.byref(self.h)))

    def set(self, key, value):
        _ffi.check(lib().slx_grc_set(self.h, key.encode(), value))

    def counter(self, name):
        return int(lib().slx_grc_counter(self.h, name.encode()))

    def sorted(self):
        """-> (sorted intervals, perm, run_p2, ends)"""
        out = (Iv * (self.n + 1))()
        a = [np.zeros(self.n + 1, dtype=np.int32) for _ in range(3)]
        _ffi.check(lib().slx_grc_sorted(self.h, out, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data))
        return (_tuples(out, self.n),) + tuple(x[:self.n].tolist() for x in a)

    def merged(self):
        out, n = (Iv * (self.n + 1))(), C.c_int64(0)
        _ffi.check(lib().slx_grc_merged(self.h, out, self.n, C.byref(n)))
        return _tuples(out, n.value)

    def query_host(self, q, ignore_strand=True, contained=False):
        """-> ([(subject id, clipped pos1, clipped pos2)], width)"""
        cap = self.n + 1
        a = [np.zeros(cap, dtype=np.int32) for _ in range(3)]
        n, w = C.c_int64(0), C.c_int64(0)
        _ffi.check(lib().slx_grc_query_host(self.h, ivs([q]), int(ignore_strand), int(contained), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, cap, C.byref(n), C.byref(w)))
        return [(int(a[0][k]), int(a[1][k]), int(a[2][k])) for k in range(n.value)], w.value

    def overlaps(self, queries, ignore_strand=True):
        """-> {"count", "width", "offset", "pairs": [(query id, subject id, clipped pos1, clipped pos2)], "n_pairs"}"""
        res = Result()
        _ffi.check(lib().slx_grc_overlaps(self.h, ivs(queries), len(queries), int(ignore_strand), C.byref(res)))
        return _take(res)

    def count(self, queries, ignore_strand=True, contained=False):
        out = np.zeros(len(queries) + 1, dtype=np.uint32)
        _ffi.check(lib().slx_grc_count(self.h, ivs(queries), len(queries), int(ignore_strand), int(contained), out.ctypes.data))
        return out[:len(queries)].tolist()

    def overlaps_host(self, stream, rec_off, want_pairs=True, want_result=True):
        arr = (C.c_uint64 * len(rec_off))(*rec_off)
        res = Result()
        _ffi.check(lib().slx_grc_overlaps_host(self.h, bytes(stream), len(stream), arr, len(rec_off) - 1, int(want_pairs), C.byref(res) if want_result else None))
        return _take(res, want_pairs) if want_result else None

    def overlaps_device(self, d_stream, n_bytes, d_rec_off, n_records, want_pairs=True, want_result=True):
        """device pointers as ints"""
        res = Result()
        _ffi.check(lib().slx_grc_overlaps_device(self.h, d_stream, n_bytes, d_rec_off, n_records, int(want_pairs), C.byref(res) if want_result else None))
        return _take(res, want_pairs) if want_result else None

    def subject_counts(self):
        out = np.zeros(self.n + 1, dtype=np.int64)
        _ffi.check(lib().slx_grc_subject_counts(self.h, out.ctypes.data))
        return out[:self.n].tolist()

    def clear_counts(self):
        _ffi.check(lib().slx_grc_clear_counts(self.h))

    def close(self):
        if self.h:
            lib().slx_grc_free(self.h)
            self.h = None

    def __del__(self):
        if getattr(self, "h", None):
            self.close()
