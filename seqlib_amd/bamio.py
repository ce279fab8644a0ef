"""ctypes binding of include/seqlib_amd_bam.h (the BamReader path of libseqlib_amd.so) for tests and tools.

Plumbing only: the product is the C-ABI and the C++ mirror include/SeqLib/BamReader.h.  No CPU fallback: without the library it raises, without a GPU
slx_bam_open and slx_bam_inflate_file return SLX_ENODEVICE.
"""
import ctypes as C

import numpy as np

from . import _ffi

# every symbol include/seqlib_amd_bam.h declares (checked by tests/test_bam_reader.py against the header text)
EXPORTS = [
    "slx_bam_open", "slx_bam_close", "slx_bam_header", "slx_bam_ref_name", "slx_bam_ref_len", "slx_bam_next", "slx_bam_reads_device", "slx_bam_hits_to_host", "slx_bam_rewind",
    "slx_bam_set", "slx_bam_counter", "slx_bam_scan_members", "slx_bam_members_free", "slx_bam_inflate_file",
    "slx_bam_index_load", "slx_bam_has_index", "slx_bam_set_regions", "slx_bam_index_build", "slx_bam_index_build_ex",
]
# the host-only BAI helpers of the same header
BAI_EXPORTS = ["slx_bai_query", "slx_bai_stats", "slx_bai_free"]
# the BGZF writer of the same header (checked by tests/test_bgzf_writer.py)
BGZF_EXPORTS = ["slx_bgzf_open", "slx_bgzf_write", "slx_bgzf_write_device", "slx_bgzf_flush", "slx_bgzf_close", "slx_bgzf_set", "slx_bgzf_counter"]


class Member(C.Structure):
    _fields_ = [("file_off", C.c_uint64), ("data_off", C.c_uint32), ("data_len", C.c_uint32), ("isize", C.c_uint32), ("crc32", C.c_uint32)]


class Region(C.Structure):
    _fields_ = [("tid", C.c_int32), ("beg", C.c_int64), ("end", C.c_int64)]


class Batch(C.Structure):
    _fields_ = [("n_records", C.c_int64), ("n_bytes", C.c_int64), ("stream", C.c_void_p), ("rec_off", C.c_void_p), ("d_stream", C.c_void_p), ("d_rec_off", C.c_void_p),
                ("n_members", C.c_int64), ("n_repaired_chunks", C.c_int64)]


_READY = False


def lib():
    global _READY
    L = _ffi.lib()
    if not _READY:
        L.slx_bam_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        L.slx_bam_close.argtypes = [C.c_void_p]
        L.slx_bam_close.restype = None
        L.slx_bam_header.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        L.slx_bam_ref_name.argtypes = [C.c_void_p, C.c_int]
        L.slx_bam_ref_name.restype = C.c_char_p
        L.slx_bam_ref_len.argtypes = [C.c_void_p, C.c_int]
        L.slx_bam_ref_len.restype = C.c_int64
        L.slx_bam_next.argtypes = [C.c_void_p, C.c_int64, C.POINTER(Batch)]
        L.slx_bam_reads_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                           C.POINTER(C.POINTER(C.c_int64))]
        L.slx_bam_hits_to_host.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_ffi.Hits), C.POINTER(_ffi.Hits)]
        L.slx_bam_rewind.argtypes = [C.c_void_p]
        L.slx_bam_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_bam_counter.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_bam_counter.restype = C.c_int64
        L.slx_bam_scan_members.argtypes = [C.c_char_p, C.POINTER(C.POINTER(Member)), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        L.slx_bam_members_free.argtypes = [C.POINTER(Member)]
        L.slx_bam_members_free.restype = None
        L.slx_bam_inflate_file.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.slx_bam_index_load.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_bam_has_index.argtypes = [C.c_void_p]
        L.slx_bam_set_regions.argtypes = [C.c_void_p, C.POINTER(Region), C.c_int64]
        L.slx_bam_index_build.argtypes = [C.c_char_p, C.c_int, C.c_char_p]
        L.slx_bam_index_build_ex.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int64, C.c_int64]
        L.slx_bai_query.argtypes = [C.c_char_p, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_int64)]
        L.slx_bai_stats.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.slx_bai_free.argtypes = [C.c_void_p]
        L.slx_bai_free.restype = None
        L.slx_bgzf_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        L.slx_bgzf_write.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_bgzf_write_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.slx_bgzf_flush.argtypes = [C.c_void_p]
        L.slx_bgzf_close.argtypes = [C.c_void_p]
        L.slx_bgzf_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_bgzf_counter.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_bgzf_counter.restype = C.c_int64
        _READY = True
    return L


def index_build(path, bai_path=None, device=-1, batch_bytes=0, chunk_bytes=0):
    """the BAI of a coordinate-sorted BAM, built on the GPU (bai_path None: path + ".bai")"""
    _ffi.check(lib().slx_bam_index_build_ex(str(path).encode(), device, None if bai_path is None else str(bai_path).encode(), batch_bytes, chunk_bytes))


def bai_query(bai_path, tid, beg, end):
    """host only -> [(u, v)]: the merged chunk list of a region"""
    p, n = C.POINTER(C.c_uint64)(), C.c_int64(0)
    _ffi.check(lib().slx_bai_query(str(bai_path).encode(), tid, beg, end, C.byref(p), C.byref(n)))
    out = [(p[2 * i], p[2 * i + 1]) for i in range(n.value)]
    lib().slx_bai_free(p)
    return out


def bai_stats(bai_path, tid=-1):
    """host only -> dict(n_ref, n_no_coor[, n_mapped, n_unmapped, n_bin, n_intv])"""
    nr, nc, nm, nu, nb, ni = C.c_int(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int(0), C.c_int(0)
    _ffi.check(lib().slx_bai_stats(str(bai_path).encode(), C.byref(nr), C.byref(nc), tid, C.byref(nm), C.byref(nu), C.byref(nb), C.byref(ni)))
    d = dict(n_ref=nr.value, n_no_coor=nc.value)
    if tid >= 0:
        d.update(n_mapped=nm.value, n_unmapped=nu.value, n_bin=nb.value, n_intv=ni.value)
    return d


def scan_members(path):
    """-> ([(file_off, data_off, data_len, isize, crc32)], has_eof)"""
    p, n, eof = C.POINTER(Member)(), C.c_int64(0), C.c_int(0)
    _ffi.check(lib().slx_bam_scan_members(str(path).encode(), C.byref(p), C.byref(n), C.byref(eof)))
    out = [(p[i].file_off, p[i].data_off, p[i].data_len, p[i].isize, p[i].crc32) for i in range(n.value)]
    lib().slx_bam_members_free(p)
    return out, bool(eof.value)


def inflate_file(path, device=-1):
    """every member of a BGZF file through the GPU kernels -> bytes"""
    n = C.c_uint64(0)
    total = sum(m[3] for m in scan_members(path)[0])
    buf = np.zeros(max(total, 1), dtype=np.uint8)
    _ffi.check(lib().slx_bam_inflate_file(str(path).encode(), device, buf.ctypes.data, total, C.byref(n)))
    return buf[:n.value].tobytes()


class Reader:
    """slx_bam handle"""

    def __init__(self, path, device=-1):
        self.h = C.c_void_p()
        _ffi.check(lib().slx_bam_open(str(path).encode(), device, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().slx_bam_close(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def header(self):
        t, l, n = C.c_char_p(), C.c_int64(0), C.c_int(0)
        _ffi.check(lib().slx_bam_header(self.h, C.byref(t), C.byref(l), C.byref(n)))
        return t.value.decode(), [(lib().slx_bam_ref_name(self.h, i).decode(), lib().slx_bam_ref_len(self.h, i)) for i in range(n.value)]

    def set(self, key, value):
        _ffi.check(lib().slx_bam_set(self.h, key.encode(), value))

    def counter(self, name):
        return int(lib().slx_bam_counter(self.h, name.encode()))

    def rewind(self):
        _ffi.check(lib().slx_bam_rewind(self.h))

    def index_load(self, bai_path=None):
        _ffi.check(lib().slx_bam_index_load(self.h, None if bai_path is None else str(bai_path).encode()))

    def has_index(self):
        return bool(lib().slx_bam_has_index(self.h))

    def set_regions(self, regions):
        """regions: [(tid, beg, end)], 0-based half open; [] = the whole file again"""
        arr = (Region * max(len(regions), 1))(*[Region(*r) for r in regions])
        _ffi.check(lib().slx_bam_set_regions(self.h, arr, len(regions)))

    def next(self, max_bytes=64 << 20):
        """-> (list of whole records as bytes, block_size word included; Batch) -- an empty list at the end of the file"""
        b = Batch()
        _ffi.check(lib().slx_bam_next(self.h, max_bytes, C.byref(b)))
        self.batch = b
        if b.n_records == 0:
            return [], b
        raw = C.string_at(b.stream, b.n_bytes)
        off = np.ctypeslib.as_array(C.cast(b.rec_off, C.POINTER(C.c_uint64)), shape=(b.n_records + 1,)).tolist()
        return [raw[off[i]:off[i + 1]] for i in range(b.n_records)], b

    def reads_device(self, skip_flags=0x900, original_strand=False):
        """-> (device pointer of the bases, device pointer of the offsets, n_reads, record index per read)"""
        db, do, n, m = C.c_void_p(), C.c_void_p(), C.c_int64(0), C.POINTER(C.c_int64)()
        _ffi.check(lib().slx_bam_reads_device(self.h, C.byref(self.batch), skip_flags, 1 if original_strand else 0, C.byref(db), C.byref(do), C.byref(n), C.byref(m)))
        return db.value, do.value, n.value, [m[i] for i in range(n.value)]


class Writer:
    """slx_bgzf handle: a BGZF file compressed on the GPU.  close() frees the handle; the object is not usable afterwards."""

    def __init__(self, path, device=-1):
        self.h = C.c_void_p()
        _ffi.check(lib().slx_bgzf_open(str(path).encode(), device, C.byref(self.h)))

    def write(self, data):
        _ffi.check(lib().slx_bgzf_write(self.h, bytes(data), len(data)))

    def write_device(self, ptr, n):
        """n bytes at the device pointer ptr (an int, e.g. Batch.d_stream)"""
        _ffi.check(lib().slx_bgzf_write_device(self.h, ptr, n))

    def flush(self):
        _ffi.check(lib().slx_bgzf_flush(self.h))

    def set(self, key, value):
        _ffi.check(lib().slx_bgzf_set(self.h, key.encode(), value))

    def counter(self, name):
        return int(lib().slx_bgzf_counter(self.h, name.encode()))

    def close(self):
        if self.h:
            h, self.h = self.h, None
            _ffi.check(lib().slx_bgzf_close(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
