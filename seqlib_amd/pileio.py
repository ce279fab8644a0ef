"""ctypes binding of include/seqlib_amd_pile.h (per-base pileup, part of libseqlib_amd.so) for tests and tools.

Plumbing only: the product is the C-ABI and SeqLib::Pileup of include/SeqLib/Pileup.h.  No CPU fallback: without the library it raises, without a GPU
slx_pile_create gives a host-only object whose every other entry returns SLX_ENODEVICE; slx_pile_record_events is host only.
"""
import ctypes as C

import numpy as np

from . import _ffi, bamio

# every symbol include/seqlib_amd_pile.h declares (checked by tests/test_pile_host.py against the header text)
EXPORTS = ["slx_pile_create", "slx_pile_free", "slx_pile_set", "slx_pile_add_device", "slx_pile_add_host", "slx_pile_record_events", "slx_pile_counts",
           "slx_pile_counts_device", "slx_pile_at", "slx_pile_sites", "slx_pile_sites_to_host", "slx_pile_sites_tsv", "slx_pile_clear", "slx_pile_counter"]
COUNTERS = ("records_seen", "records_counted", "long_records", "events_lds", "events_global", "sites", "us_add", "us_sites")
KNOBS = ("min_mapq", "min_baseq", "exclude_flags", "long_cigar", "long_read", "lds_window", "slice_records", "group_lanes")
PLANES = 15
A, C_, G, T, N, DEL, INS, REV, LOWQ = 0, 1, 2, 3, 4, 5, 6, 7, 14


class Site(C.Structure):
    _fields_ = [("pos", C.c_int64), ("ref", C.c_int32), ("depth", C.c_int32), ("alt", C.c_int32), ("ins", C.c_int32), ("plane", C.c_int32 * PLANES), ("pad", C.c_int32)]


_READY = False


def lib():
    global _READY
    L = bamio.lib()
    if not _READY:
        L.slx_pile_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_char_p), C.POINTER(bamio.Region), C.POINTER(C.c_void_p)]
        L.slx_pile_free.argtypes = [C.c_void_p]
        L.slx_pile_free.restype = None
        L.slx_pile_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_pile_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        L.slx_pile_add_host.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.POINTER(C.c_uint64), C.c_int64]
        L.slx_pile_record_events.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64)]
        L.slx_pile_counts.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p]
        L.slx_pile_counts_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        L.slx_pile_at.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
        L.slx_pile_sites.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
        L.slx_pile_sites_to_host.argtypes = [C.c_void_p, C.POINTER(Site)]
        L.slx_pile_sites_tsv.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_pile_clear.argtypes = [C.c_void_p]
        L.slx_pile_counter.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_pile_counter.restype = C.c_int64
        _READY = True
    return L


def record_events(rec, min_baseq=0, clip=(0, 1 << 40), cap=None):
    """host only: the (plane, position) events one block_size-prefixed record contributes to a window kept as clip, in the walk's order; raises SlxError (SLX_EIO
    for a broken record, SLX_EINVAL when cap is given and too small)"""
    n = C.c_int64(0)
    if cap is None:          # ask first
        rc = lib().slx_pile_record_events(bytes(rec), len(rec), min_baseq, clip[0], clip[1], None, None, 0, C.byref(n))
        if rc != _ffi.SLX_EINVAL or n.value == 0:
            _ffi.check(rc)
            return []
        cap = n.value
    plane, pos = (C.c_int32 * max(cap, 1))(), (C.c_int64 * max(cap, 1))()
    _ffi.check(lib().slx_pile_record_events(bytes(rec), len(rec), min_baseq, clip[0], clip[1], plane, pos, cap, C.byref(n)))
    return [(plane[i], pos[i]) for i in range(n.value)]


class Pile:
    """slx_pile handle.  refs: [(name, length)]; window: (tid, beg, end)"""

    def __init__(self, refs, window, device=-1):
        self.h = C.c_void_p()
        self.refs = list(refs)
        lens = (C.c_int64 * max(len(refs), 1))(*[l for _, l in refs])
        names = (C.c_char_p * max(len(refs), 1))(*[n.encode() for n, _ in refs])
        win = None if window is None else C.byref(bamio.Region(*window))
        _ffi.check(lib().slx_pile_create(device, len(refs), lens, names, win, C.byref(self.h)))
        tid, beg, end = window
        self.beg = min(max(beg, 0), refs[tid][1])
        self.end = min(max(end, self.beg), refs[tid][1])

    def set(self, key, value):
        _ffi.check(lib().slx_pile_set(self.h, key.encode(), value))

    def counter(self, name):
        return int(lib().slx_pile_counter(self.h, name.encode()))

    def add_host(self, stream, rec_off):
        arr = (C.c_uint64 * len(rec_off))(*rec_off)
        _ffi.check(lib().slx_pile_add_host(self.h, bytes(stream), len(stream), arr, len(rec_off) - 1))

    def add_device(self, d_stream, n_bytes, d_rec_off, n_records):
        """device pointers as ints"""
        _ffi.check(lib().slx_pile_add_device(self.h, d_stream, n_bytes, d_rec_off, n_records))

    def counts(self, plane, beg=None, end=None):
        """-> numpy int32 of one plane at positions [beg, end) (None: the window's)"""
        beg = self.beg if beg is None else beg
        end = self.end if end is None else end
        out = np.zeros(max(end - beg, 1), dtype=np.int32)
        _ffi.check(lib().slx_pile_counts(self.h, plane, beg, end, out.ctypes.data))
        return out[:end - beg]

    def planes(self, beg=None, end=None):
        """-> numpy int32 [15, end - beg]"""
        return np.stack([self.counts(p, beg, end) for p in range(PLANES)])

    def counts_device(self, plane):
        """-> (device pointer, number of int32)"""
        p, n = C.c_void_p(), C.c_int64(0)
        _ffi.check(lib().slx_pile_counts_device(self.h, plane, C.byref(p), C.byref(n)))
        return p.value, n.value

    def at(self, pos):
        out = (C.c_int32 * PLANES)()
        _ffi.check(lib().slx_pile_at(self.h, pos, out))
        return list(out)

    def sites(self, ref, ref_tid, min_depth, min_alt, frac_num, frac_den):
        """ref: a refio.Ref -> [(pos, ref byte, depth, alt, ins, [15 counts])]"""
        n = C.c_int64(0)
        _ffi.check(lib().slx_pile_sites(self.h, ref.h, ref_tid, min_depth, min_alt, frac_num, frac_den, C.byref(n)))
        out = (Site * max(n.value, 1))()
        _ffi.check(lib().slx_pile_sites_to_host(self.h, out))
        return [(s.pos, s.ref, s.depth, s.alt, s.ins, list(s.plane)) for s in out[:n.value]]

    def sites_tsv(self, path):
        _ffi.check(lib().slx_pile_sites_tsv(self.h, str(path).encode()))

    def clear(self):
        _ffi.check(lib().slx_pile_clear(self.h))

    def close(self):
        if self.h:
            lib().slx_pile_free(self.h)
            self.h = None

    def __del__(self):
        if getattr(self, "h", None):
            self.close()
