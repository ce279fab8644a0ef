"""ctypes binding of include/seqlib_amd_rec.h (the record builder of libseqlib_amd.so) for tests and tools.

Plumbing only: the product is the C-ABI and BWAAligner::alignToBam of include/SeqLib/BWAAligner.h.  No CPU fallback: without the library it raises,
without a GPU slx_rec_create returns SLX_ENODEVICE.
"""
import ctypes as C

import numpy as np

from . import _ffi, bamio

# every symbol include/seqlib_amd_rec.h declares (checked by tests/test_rec_builder.py against the header text)
REC_EXPORTS = ["slx_rec_create", "slx_rec_free", "slx_rec_upload", "slx_rec_build", "slx_rec_build_from_bam", "slx_rec_to_host", "slx_rec_counter"]


class RecBatch(C.Structure):
    _fields_ = [("n_records", C.c_int64), ("n_bytes", C.c_int64), ("d_stream", C.c_void_p), ("d_rec_off", C.c_void_p)]


_READY = False


def lib():
    global _READY
    L = bamio.lib()
    if not _READY:
        L.slx_rec_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.slx_rec_free.argtypes = [C.c_void_p]
        L.slx_rec_free.restype = None
        L.slx_rec_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.POINTER(C.c_void_p)] * 4
        L.slx_rec_build.argtypes = [C.c_void_p, C.POINTER(_ffi.Hits), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(RecBatch)]
        L.slx_rec_build_from_bam.argtypes = [C.c_void_p, C.POINTER(_ffi.Hits), C.c_void_p, C.POINTER(bamio.Batch), C.c_int, C.POINTER(RecBatch)]
        L.slx_rec_to_host.argtypes = [C.c_void_p, C.POINTER(RecBatch), C.c_void_p, C.c_uint64, C.c_void_p]
        L.slx_rec_counter.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_rec_counter.restype = C.c_int64
        _READY = True
    return L


def flatten(items):
    """list of bytes -> (uint8 array, uint64 offsets of len + 1): the layout of reads and names"""
    offs = np.zeros(len(items) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in items], dtype=np.uint64)
    flat = np.frombuffer(b"".join(items), dtype=np.uint8).copy() if len(items) and offs[-1] else np.zeros(1, dtype=np.uint8)
    return flat, offs


class Builder:
    """slx_rec handle bound to an aligner handle (a c_void_p of slx_aligner_create with one device)"""

    def __init__(self, aligner_handle):
        self.h = C.c_void_p()
        _ffi.check(lib().slx_rec_create(aligner_handle, C.byref(self.h)))
        self.batch = None

    def close(self):
        if self.h:
            lib().slx_rec_free(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def upload(self, seqs, names):
        """seqs, names: lists of bytes -> device pointers (bases, offs, names, name_offs), valid until the next upload"""
        b, bo = flatten(seqs)
        n, no = flatten(names)
        out = [C.c_void_p() for _ in range(4)]
        _ffi.check(lib().slx_rec_upload(self.h, b.ctypes.data, bo.ctypes.data, n.ctypes.data, no.ctypes.data, len(seqs), *[C.byref(o) for o in out]))
        return tuple(o.value for o in out)

    def build(self, hits, d_bases, d_offs, d_names, d_name_offs, hardclip=False):
        """hits: an _ffi.Hits -> RecBatch"""
        b = RecBatch()
        _ffi.check(lib().slx_rec_build(self.h, C.byref(hits), d_bases, d_offs, d_names, d_name_offs, 1 if hardclip else 0, C.byref(b)))
        self.batch = b
        return b

    def build_from_bam(self, hits, reader, hardclip=False):
        """reader: a bamio.Reader whose current batch went through reads_device"""
        b = RecBatch()
        _ffi.check(lib().slx_rec_build_from_bam(self.h, C.byref(hits), reader.h, C.byref(reader.batch), 1 if hardclip else 0, C.byref(b)))
        self.batch = b
        return b

    def to_host(self, batch=None):
        """-> (stream bytes, [rec_off])"""
        b = batch or self.batch
        buf = np.zeros(max(b.n_bytes, 1), dtype=np.uint8)
        off = np.zeros(b.n_records + 1, dtype=np.uint64)
        _ffi.check(lib().slx_rec_to_host(self.h, C.byref(b), buf.ctypes.data, b.n_bytes, off.ctypes.data))
        return buf[:b.n_bytes].tobytes(), off.tolist()

    def counter(self, name):
        return int(lib().slx_rec_counter(self.h, name.encode()))
