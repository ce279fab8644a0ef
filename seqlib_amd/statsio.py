"""ctypes binding of include/seqlib_amd_stats.h (per-read-group statistics, part of libseqlib_amd.so) for tests and tools.

Plumbing only: the product is the C-ABI and SeqLib::BamStats of include/SeqLib/BamStats.h.  No CPU fallback: without the library it raises, without a GPU
slx_stats_create gives a host-only object whose batch entries return SLX_ENODEVICE; slx_stats_record is host only.
"""
import ctypes as C

from . import _ffi, bamio

# every symbol include/seqlib_amd_stats.h declares (checked by tests/test_stats_host.py against the header text)
STATS_EXPORTS = ["slx_stats_create", "slx_stats_free", "slx_stats_set", "slx_stats_add_device", "slx_stats_add_host", "slx_stats_record", "slx_stats_n_groups",
                 "slx_stats_group_name", "slx_stats_counter_of", "slx_stats_hist", "slx_stats_bins", "slx_stats_text", "slx_stats_text_free", "slx_stats_merge", "slx_stats_clear",
                 "slx_stats_counter"]
HISTS = ("mapq", "nm", "isize", "clip", "phred", "len")
GROUP_COUNTERS = ("reads", "supp", "qcfail", "duplicate", "unmap", "mate_unmap", "supplementary", "paired", "proper_pair", "read1", "read2", "reverse", "bases", "nm_missing")
COUNTERS = ("records_seen", "records_counted", "long_records", "adds_lds", "adds_global", "group_misses", "us_add")
KNOBS = ("len_max", "isize_max", "exclude_flags", "min_mapq", "max_groups", "lds_groups", "window_bytes", "group_slots", "long_record")


class Rec(C.Structure):
    _fields_ = [("value", C.c_int64 * 6), ("flag", C.c_uint32), ("has_nm", C.c_int32), ("group_len", C.c_int32), ("pad", C.c_int32), ("group", C.c_char * 256)]


_READY = False


def lib():
    global _READY
    L = bamio.lib()
    if not _READY:
        L.slx_stats_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.slx_stats_free.argtypes = [C.c_void_p]
        L.slx_stats_free.restype = None
        L.slx_stats_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_stats_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        L.slx_stats_add_host.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.POINTER(C.c_uint64), C.c_int64]
        L.slx_stats_record.argtypes = [C.c_char_p, C.c_int64, C.POINTER(Rec)]
        L.slx_stats_n_groups.argtypes = [C.c_void_p]
        L.slx_stats_n_groups.restype = C.c_int64
        L.slx_stats_group_name.argtypes = [C.c_void_p, C.c_int64]
        L.slx_stats_group_name.restype = C.c_char_p
        L.slx_stats_counter_of.argtypes = [C.c_void_p, C.c_int64, C.c_char_p]
        L.slx_stats_counter_of.restype = C.c_int64
        L.slx_stats_hist.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_uint64), C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.slx_stats_bins.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64)]
        L.slx_stats_text.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        L.slx_stats_text_free.argtypes = [C.c_void_p]
        L.slx_stats_text_free.restype = None
        L.slx_stats_merge.argtypes = [C.c_void_p, C.c_void_p]
        L.slx_stats_clear.argtypes = [C.c_void_p]
        L.slx_stats_counter.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_stats_counter.restype = C.c_int64
        _READY = True
    return L


def record(rec):
    """host only: (group bytes, {histogram name: value}, has_nm, flag) of one block_size-prefixed record; raises SlxError (SLX_EIO, SLX_EUNSUPPORTED)"""
    out = Rec()
    _ffi.check(lib().slx_stats_record(bytes(rec), len(rec), C.byref(out)))
    return C.string_at(C.addressof(out) + Rec.group.offset, out.group_len), dict(zip(HISTS, out.value)), bool(out.has_nm), out.flag


class Stats:
    """slx_stats handle"""

    def __init__(self, device=-1, **knobs):
        self.h = C.c_void_p()
        _ffi.check(lib().slx_stats_create(device, C.byref(self.h)))
        for k, v in knobs.items():
            self.set(k, v)

    def set(self, key, value):
        _ffi.check(lib().slx_stats_set(self.h, key.encode(), value))

    def counter(self, name):
        return int(lib().slx_stats_counter(self.h, name.encode()))

    def add_host(self, stream, rec_off):
        arr = (C.c_uint64 * len(rec_off))(*rec_off)
        _ffi.check(lib().slx_stats_add_host(self.h, bytes(stream), len(stream), arr, len(rec_off) - 1))

    def add_device(self, d_stream, n_bytes, d_rec_off, n_records):
        """device pointers as ints"""
        _ffi.check(lib().slx_stats_add_device(self.h, d_stream, n_bytes, d_rec_off, n_records))

    def _value(self, v):
        if v < 0:
            _ffi.check(int(v))
        return int(v)

    def n_groups(self):
        return self._value(lib().slx_stats_n_groups(self.h))

    def group_name(self, i):
        return lib().slx_stats_group_name(self.h, i)

    def counter_of(self, i, name):
        return self._value(lib().slx_stats_counter_of(self.h, i, name.encode()))

    def bins(self, which):
        """-> [(lo, hi)] of histogram `which` (an index or a name of HISTS)"""
        which = HISTS.index(which) if isinstance(which, str) else which
        n = C.c_int64(0)
        _ffi.check(lib().slx_stats_bins(self.h, which, None, None, 0, C.byref(n)))
        lo, hi = (C.c_int32 * n.value)(), (C.c_int32 * n.value)()
        _ffi.check(lib().slx_stats_bins(self.h, which, lo, hi, n.value, C.byref(n)))
        return list(zip(lo, hi))

    def hist(self, i, which):
        """-> ([bin counts], below, above)"""
        which = HISTS.index(which) if isinstance(which, str) else which
        n = len(self.bins(which))
        b, lo, hi = (C.c_uint64 * n)(), C.c_uint64(0), C.c_uint64(0)
        _ffi.check(lib().slx_stats_hist(self.h, i, which, b, n, C.byref(lo), C.byref(hi)))
        return list(b), lo.value, hi.value

    def group(self, i):
        """-> (name bytes, {counter: value}, {histogram: (bins, below, above)})"""
        return self.group_name(i), {c: self.counter_of(i, c) for c in GROUP_COUNTERS}, {h: self.hist(i, h) for h in HISTS}

    def groups(self):
        """-> [group(i)] in order of first appearance"""
        return [self.group(i) for i in range(self.n_groups())]

    def text(self):
        p, n = C.c_void_p(), C.c_int64(0)
        _ffi.check(lib().slx_stats_text(self.h, C.byref(p), C.byref(n)))
        try:
            return C.string_at(p.value, n.value)
        finally:
            lib().slx_stats_text_free(p)

    def merge(self, other):
        _ffi.check(lib().slx_stats_merge(self.h, other.h))

    def clear(self):
        _ffi.check(lib().slx_stats_clear(self.h))

    def close(self):
        if self.h:
            lib().slx_stats_free(self.h)
            self.h = None

    def __del__(self):
        if getattr(self, "h", None):
            self.close()
