"""ctypes binding of include/seqlib_amd_cov.h (depth of coverage, part of libseqlib_amd.so) for tests and tools.

Plumbing only: the product is the C-ABI and SeqLib::STCoverage of include/SeqLib/STCoverage.h.  No CPU fallback: without the library it raises, without a GPU
slx_cov_create gives a host-only object whose every kernel entry returns SLX_ENODEVICE; slx_cov_record_intervals is host only.
"""
import ctypes as C

import numpy as np

from . import _ffi, bamio

# every symbol include/seqlib_amd_cov.h declares (checked by tests/test_cov_host.py against the header text)
COV_EXPORTS = ["slx_cov_create", "slx_cov_free", "slx_cov_set", "slx_cov_add_device", "slx_cov_add_host", "slx_cov_record_intervals", "slx_cov_depth", "slx_cov_depth_device",
               "slx_cov_at", "slx_cov_max", "slx_cov_regions", "slx_cov_bedgraph", "slx_cov_clear", "slx_cov_counter"]
COUNTERS = ("records_seen", "records_counted", "long_records", "events_lds", "events_global", "runs", "us_add", "us_settle")
KNOBS = ("mode", "buff", "min_mapq", "exclude_flags", "count_del", "long_cigar", "lds_window", "slice_records", "scan_chunk")
SLX_COV_SPAN, SLX_COV_FULL, SLX_COV_ALIGNED = 0, 1, 2

_READY = False


def lib():
    global _READY
    L = bamio.lib()
    if not _READY:
        L.slx_cov_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_char_p), C.POINTER(bamio.Region), C.POINTER(C.c_void_p)]
        L.slx_cov_free.argtypes = [C.c_void_p]
        L.slx_cov_free.restype = None
        L.slx_cov_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_cov_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        L.slx_cov_add_host.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.POINTER(C.c_uint64), C.c_int64]
        L.slx_cov_record_intervals.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64,
                                               C.POINTER(C.c_int64)]
        L.slx_cov_depth.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p]
        L.slx_cov_depth_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        L.slx_cov_at.argtypes = [C.c_void_p, C.c_int, C.c_int64]
        L.slx_cov_at.restype = C.c_int64
        L.slx_cov_max.argtypes = [C.c_void_p, C.c_int]
        L.slx_cov_max.restype = C.c_int64
        L.slx_cov_regions.argtypes = [C.c_void_p, C.POINTER(bamio.Region), C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.slx_cov_bedgraph.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p]
        L.slx_cov_clear.argtypes = [C.c_void_p]
        L.slx_cov_counter.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_cov_counter.restype = C.c_int64
        _READY = True
    return L


def record_intervals(rec, mode, buff=0, count_del=0, clip=(0, 1 << 40)):
    """host only: the [lo, hi) intervals one block_size-prefixed record contributes to a contig kept as clip; raises SlxError (SLX_EIO) for a broken record"""
    cap = max(16, (len(rec) - 36) // 4 + 1)
    lo, hi, n = (C.c_int64 * cap)(), (C.c_int64 * cap)(), C.c_int64(0)
    _ffi.check(lib().slx_cov_record_intervals(bytes(rec), len(rec), mode, buff, count_del, clip[0], clip[1], lo, hi, cap, C.byref(n)))
    return [(lo[i], hi[i]) for i in range(n.value)]


class Coverage:
    """slx_cov handle.  refs: [(name, length)]; window: (tid, beg, end) or None"""

    def __init__(self, refs, window=None, device=-1):
        self.h = C.c_void_p()
        self.refs = list(refs)
        lens = (C.c_int64 * max(len(refs), 1))(*[l for _, l in refs])
        names = (C.c_char_p * max(len(refs), 1))(*[n.encode() for n, _ in refs])
        win = None if window is None else C.byref(bamio.Region(*window))
        _ffi.check(lib().slx_cov_create(device, len(refs), lens, names, win, C.byref(self.h)))

    def set(self, key, value):
        _ffi.check(lib().slx_cov_set(self.h, key.encode(), value))

    def counter(self, name):
        return int(lib().slx_cov_counter(self.h, name.encode()))

    def add_host(self, stream, rec_off):
        arr = (C.c_uint64 * len(rec_off))(*rec_off)
        _ffi.check(lib().slx_cov_add_host(self.h, bytes(stream), len(stream), arr, len(rec_off) - 1))

    def add_device(self, d_stream, n_bytes, d_rec_off, n_records):
        """device pointers as ints"""
        _ffi.check(lib().slx_cov_add_device(self.h, d_stream, n_bytes, d_rec_off, n_records))

    def depth(self, tid, beg=0, end=None):
        """-> numpy int32 of positions [beg, end) (end None: the contig's length)"""
        end = self.refs[tid][1] if end is None else end
        out = np.zeros(max(end - beg, 1), dtype=np.int32)
        _ffi.check(lib().slx_cov_depth(self.h, tid, beg, end, out.ctypes.data))
        return out[:end - beg]

    def depth_device(self, tid):
        """-> (device pointer, number of int32)"""
        p, n = C.c_void_p(), C.c_int64(0)
        _ffi.check(lib().slx_cov_depth_device(self.h, tid, C.byref(p), C.byref(n)))
        return p.value, n.value

    def _value(self, v):
        if v < 0:
            _ffi.check(int(v))
        return int(v)

    def at(self, tid, pos):
        return self._value(lib().slx_cov_at(self.h, tid, pos))

    def max(self, tid=-1):
        return self._value(lib().slx_cov_max(self.h, tid))

    def regions(self, regs, min_depth=1):
        """regs: [(tid, beg, end)] -> ([sum], [positions with depth >= min_depth])"""
        n = len(regs)
        arr = (bamio.Region * max(n, 1))(*[bamio.Region(*r) for r in regs])
        s, c = (C.c_int64 * max(n, 1))(), (C.c_int64 * max(n, 1))()
        _ffi.check(lib().slx_cov_regions(self.h, arr, n, min_depth, s, c))
        return list(s[:n]), list(c[:n])

    def bedgraph(self, path, tid=-1, include_zero=False):
        _ffi.check(lib().slx_cov_bedgraph(self.h, tid, 1 if include_zero else 0, str(path).encode()))

    def clear(self):
        _ffi.check(lib().slx_cov_clear(self.h))

    def close(self):
        if self.h:
            lib().slx_cov_free(self.h)
            self.h = None

    def __del__(self):
        if getattr(self, "h", None):
            self.close()
