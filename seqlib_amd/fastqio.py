"""ctypes binding of include/seqlib_amd_fastq.h (the FASTA / FASTQ reader of libseqlib_amd.so) for tests and tools.

Plumbing only: the product is the C-ABI and SeqLib::FastqReader::NextBatch of include/SeqLib/FastqReader.h.  No CPU fallback: without the library it
raises, without a GPU slx_fastq_open returns SLX_ENODEVICE.
"""
import ctypes as C

import numpy as np

from . import _ffi

# every symbol include/seqlib_amd_fastq.h declares
FASTQ_EXPORTS = ["slx_fastq_open", "slx_fastq_close", "slx_fastq_next", "slx_fastq_to_host", "slx_fastq_rewind", "slx_fastq_set", "slx_fastq_counter"]
COUNTERS = ("reads", "fast_reads", "slow_reads", "batches", "bad_tail", "source", "us_lines", "us_check", "us_gather", "us_inflate")


class Batch(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("d_bases", C.c_void_p), ("d_offs", C.c_void_p), ("d_quals", C.c_void_p), ("d_names", C.c_void_p), ("d_name_offs", C.c_void_p),
                ("d_coms", C.c_void_p), ("d_com_offs", C.c_void_p), ("d_flags", C.c_void_p), ("n_text_bytes", C.c_int64), ("n_slow_reads", C.c_int64)]


_READY = False


def lib():
    global _READY
    L = _ffi.lib()
    if not _READY:
        L.slx_fastq_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        L.slx_fastq_close.argtypes = [C.c_void_p]
        L.slx_fastq_close.restype = None
        L.slx_fastq_next.argtypes = [C.c_void_p, C.c_int64, C.POINTER(Batch)]
        L.slx_fastq_to_host.argtypes = [C.c_void_p, C.POINTER(Batch)] + [C.c_void_p] * 8
        L.slx_fastq_rewind.argtypes = [C.c_void_p]
        L.slx_fastq_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_fastq_counter.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_fastq_counter.restype = C.c_int64
        _READY = True
    return L


class Reader:
    """slx_fastq handle"""

    def __init__(self, path, device=-1):
        self.h = C.c_void_p()
        _ffi.check(lib().slx_fastq_open(str(path).encode(), device, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().slx_fastq_close(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set(self, key, value):
        _ffi.check(lib().slx_fastq_set(self.h, key.encode(), value))

    def counter(self, name):
        return int(lib().slx_fastq_counter(self.h, name.encode()))

    def rewind(self):
        _ffi.check(lib().slx_fastq_rewind(self.h))

    def next(self, max_bytes=0):
        """the next batch (a Batch of device pointers), or None at the end of the input"""
        b = Batch()
        _ffi.check(lib().slx_fastq_next(self.h, max_bytes, C.byref(b)))
        return b if b.n_reads else None

    def to_host(self, b):
        """all eight arrays of the reader's last batch -> dict of numpy arrays (bases, offs, quals, names, name_offs, coms, com_offs, flags)"""
        n = b.n_reads
        o = {k: np.zeros(n + 1, dtype=np.uint64) for k in ("offs", "name_offs", "com_offs")}
        o["flags"] = np.zeros(n, dtype=np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _ffi.check(lib().slx_fastq_to_host(self.h, C.byref(b), None, p(o["offs"]), None, None, p(o["name_offs"]), None, p(o["com_offs"]), p(o["flags"])))
        o["bases"] = np.zeros(int(o["offs"][n]), dtype=np.uint8)
        o["quals"] = np.zeros(int(o["offs"][n]), dtype=np.uint8)
        o["names"] = np.zeros(int(o["name_offs"][n]), dtype=np.uint8)
        o["coms"] = np.zeros(int(o["com_offs"][n]), dtype=np.uint8)
        _ffi.check(lib().slx_fastq_to_host(self.h, C.byref(b), p(o["bases"]), None, p(o["quals"]), p(o["names"]), None, p(o["coms"]), None, None))
        return o

    def read_all(self, max_bytes=0):
        """every batch copied down -> (list of per-read tuples (name, com, seq, qual, flag), list of Batch-like dicts with n_reads / n_slow_reads / n_text_bytes)"""
        reads, info = [], []
        while True:
            b = self.next(max_bytes)
            if b is None:
                return reads, info
            h = self.to_host(b)
            info.append(dict(n_reads=b.n_reads, n_slow_reads=b.n_slow_reads, n_text_bytes=b.n_text_bytes, host=h))
            bs, qs, ns, cs = (h[k].tobytes() for k in ("bases", "quals", "names", "coms"))
            ob, on, oc = ([int(x) for x in h[k]] for k in ("offs", "name_offs", "com_offs"))
            for i in range(b.n_reads):
                reads.append((ns[on[i]:on[i + 1]], cs[oc[i]:oc[i + 1]], bs[ob[i]:ob[i + 1]], qs[ob[i]:ob[i + 1]], int(h["flags"][i])))
