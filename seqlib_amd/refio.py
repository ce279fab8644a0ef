"""ctypes binding of include/seqlib_amd_ref.h (the reference genome, part of libseqlib_amd.so) for tests and tools.

Plumbing only: the product is the C-ABI and SeqLib::RefGenome of include/SeqLib/RefGenome.h.  No CPU fallback: without the library it raises, without a GPU
slx_ref_open returns SLX_ENODEVICE; fai_of_text and record_nm_md are host only.
"""
import ctypes as C

from . import _ffi, bamio

# every symbol include/seqlib_amd_ref.h declares (checked by tests/test_ref_host.py against the header text)
REF_EXPORTS = ["slx_ref_open", "slx_ref_open_ex", "slx_ref_close", "slx_ref_set", "slx_ref_counter", "slx_ref_nseq", "slx_ref_name", "slx_ref_len", "slx_ref_tid",
               "slx_ref_fai_text", "slx_ref_write_fai", "slx_ref_device", "slx_ref_fetch_device", "slx_ref_fetch_host", "slx_ref_nm_md_device", "slx_ref_nm_md_host",
               "slx_ref_md_to_host", "slx_ref_record_nm_md", "slx_ref_fai_of_text", "slx_ref_text_free"]
COUNTERS = ("contigs", "bases", "text_bytes", "windows", "source", "hbm_bytes", "long_records", "long_record", "us_lines", "us_class", "us_gather", "us_inflate", "us_fetch", "us_md_size", "us_md_text")


class Region(C.Structure):
    _fields_ = [("tid", C.c_int32), ("beg", C.c_int64), ("end", C.c_int64)]


class Dev(C.Structure):
    _fields_ = [("n_contigs", C.c_int64), ("n_bytes", C.c_int64), ("d_bases", C.c_void_p), ("d_contig_off", C.c_void_p), ("d_contig_len", C.c_void_p)]


class Md(C.Structure):
    _fields_ = [("n_records", C.c_int64), ("md_bytes", C.c_int64), ("d_nm", C.c_void_p), ("d_md", C.c_void_p), ("d_md_off", C.c_void_p)]


_READY = False


def lib():
    global _READY
    L = bamio.lib()
    if not _READY:
        L.slx_ref_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        L.slx_ref_open_ex.argtypes = [C.c_char_p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]
        L.slx_ref_close.argtypes = [C.c_void_p]
        L.slx_ref_close.restype = None
        L.slx_ref_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_ref_counter.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_ref_counter.restype = C.c_int64
        L.slx_ref_nseq.argtypes = [C.c_void_p]
        L.slx_ref_nseq.restype = C.c_int64
        L.slx_ref_name.argtypes = [C.c_void_p, C.c_int64]
        L.slx_ref_name.restype = C.c_char_p
        L.slx_ref_len.argtypes = [C.c_void_p, C.c_int64]
        L.slx_ref_len.restype = C.c_int64
        L.slx_ref_tid.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_ref_tid.restype = C.c_int64
        L.slx_ref_fai_text.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.slx_ref_fai_text.restype = C.c_void_p
        L.slx_ref_write_fai.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_ref_device.argtypes = [C.c_void_p, C.POINTER(Dev)]
        L.slx_ref_fetch_device.argtypes = [C.c_void_p, C.POINTER(Region), C.c_int64, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        L.slx_ref_fetch_host.argtypes = [C.c_void_p, C.POINTER(Region), C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_uint64)]
        L.slx_ref_nm_md_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.POINTER(Md)]
        L.slx_ref_nm_md_host.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.POINTER(C.c_uint64), C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.POINTER(Md)]
        L.slx_ref_md_to_host.argtypes = [C.c_void_p, C.POINTER(Md), C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_uint64)]
        L.slx_ref_record_nm_md.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, C.POINTER(C.c_int32), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.slx_ref_fai_of_text.argtypes = [C.c_char_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        L.slx_ref_text_free.argtypes = [C.c_void_p]
        L.slx_ref_text_free.restype = None
        _READY = True
    return L


def fai_of_text(text):
    """host only: the .fai text (bytes) of FASTA text; raises SlxError (SLX_EIO) with the rule's sentence"""
    p, n = C.c_void_p(), C.c_int64(0)
    _ffi.check(lib().slx_ref_fai_of_text(bytes(text), len(text), C.byref(p), C.byref(n)))
    try:
        return C.string_at(p.value, n.value)
    finally:
        lib().slx_ref_text_free(p)


def record_nm_md(rec, contig):
    """host only: (nm, md bytes) of one block_size-prefixed record against the contig's bytes; raises SlxError (SLX_EIO)"""
    nm, n = C.c_int32(0), C.c_int64(0)
    _ffi.check(lib().slx_ref_record_nm_md(bytes(rec), len(rec), bytes(contig), len(contig), C.byref(nm), None, 0, C.byref(n)))
    buf = C.create_string_buffer(max(n.value, 1))
    _ffi.check(lib().slx_ref_record_nm_md(bytes(rec), len(rec), bytes(contig), len(contig), C.byref(nm), buf, n.value, C.byref(n)))
    return nm.value, buf.raw[:n.value]


def _regions(regions):
    arr = (Region * max(len(regions), 1))()
    for i, (tid, beg, end) in enumerate(regions):
        arr[i].tid, arr[i].beg, arr[i].end = tid, beg, end
    return arr


def _map(tid_map):
    if tid_map is None:
        return None, 0
    return (C.c_int32 * max(len(tid_map), 1))(*tid_map), len(tid_map)


class Ref:
    """slx_ref handle"""

    def __init__(self, path, device=-1, window_bytes=0, tile_bytes=0, gather_tile_bytes=0, **knobs):
        self.h = C.c_void_p()
        _ffi.check(lib().slx_ref_open_ex(str(path).encode(), device, window_bytes, tile_bytes, gather_tile_bytes, C.byref(self.h)))
        for k, v in knobs.items():
            self.set(k, v)

    def set(self, key, value):
        _ffi.check(lib().slx_ref_set(self.h, key.encode(), value))

    def counter(self, name):
        return int(lib().slx_ref_counter(self.h, name.encode()))

    def nseq(self):
        return int(lib().slx_ref_nseq(self.h))

    def name(self, tid):
        return lib().slx_ref_name(self.h, tid)

    def length(self, tid):
        return int(lib().slx_ref_len(self.h, tid))

    def tid(self, name):
        return int(lib().slx_ref_tid(self.h, name))

    def fai_text(self):
        n = C.c_int64(0)
        p = lib().slx_ref_fai_text(self.h, C.byref(n))
        return C.string_at(p, n.value)

    def write_fai(self, path=None):
        _ffi.check(lib().slx_ref_write_fai(self.h, None if path is None else str(path).encode()))

    def device(self):
        d = Dev()
        _ffi.check(lib().slx_ref_device(self.h, C.byref(d)))
        return d

    def fetch_host(self, regions, upper=0):
        """regions: [(tid, beg, end)] -> (bytes, [offsets])"""
        arr, n = _regions(regions), len(regions)
        offs = (C.c_uint64 * (n + 1))()
        _ffi.check(lib().slx_ref_fetch_host(self.h, arr, n, upper, None, 0, offs))
        buf = C.create_string_buffer(max(int(offs[n]), 1))
        _ffi.check(lib().slx_ref_fetch_host(self.h, arr, n, upper, buf, int(offs[n]), offs))
        return buf.raw[:int(offs[n])], list(offs)

    def fetch_device(self, regions, upper=0):
        """-> (d_bases, d_offs, n_bytes), device pointers as ints, valid until the next fetch"""
        arr, n = _regions(regions), len(regions)
        db, do, nb = C.c_void_p(), C.c_void_p(), C.c_int64(0)
        _ffi.check(lib().slx_ref_fetch_device(self.h, arr, n, upper, C.byref(db), C.byref(do), C.byref(nb)))
        return db.value, do.value, nb.value

    def contig(self, tid):
        """the contig's resident bytes"""
        return self.fetch_host([(tid, 0, self.length(tid))])[0]

    def _down(self, m):
        n = m.n_records
        nm, off = (C.c_int32 * max(n, 1))(), (C.c_uint64 * (n + 1))()
        md = C.create_string_buffer(max(m.md_bytes, 1))
        _ffi.check(lib().slx_ref_md_to_host(self.h, C.byref(m), nm, md, off))
        raw = md.raw
        return list(nm)[:n], [raw[off[i]:off[i + 1]] for i in range(n)]

    def nm_md_host(self, stream, rec_off, tid_map=None):
        """-> ([nm], [md bytes]) of the records of a host stream"""
        arr = (C.c_uint64 * len(rec_off))(*rec_off)
        mp, n_map = _map(tid_map)
        m = Md()
        _ffi.check(lib().slx_ref_nm_md_host(self.h, bytes(stream), len(stream), arr, len(rec_off) - 1, mp, n_map, C.byref(m)))
        return self._down(m)

    def nm_md_device(self, d_stream, n_bytes, d_rec_off, n_records, tid_map=None):
        """device pointers as ints -> ([nm], [md bytes])"""
        mp, n_map = _map(tid_map)
        m = Md()
        _ffi.check(lib().slx_ref_nm_md_device(self.h, d_stream, n_bytes, d_rec_off, n_records, mp, n_map, C.byref(m)))
        return self._down(m)

    def close(self):
        if self.h:
            lib().slx_ref_close(self.h)
            self.h = None

    def __del__(self):
        if getattr(self, "h", None):
            self.close()
