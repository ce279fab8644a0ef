"""ctypes binding of include/seqlib_amd_sam.h (the SAM text reader of libseqlib_amd.so) for tests and tools.

Plumbing only: the product is the C-ABI and SeqLib::BamReader of include/SeqLib/BamReader.h, whose Open takes SAM text.  A SAM reader's handle is an slx_bam, so
Reader is bamio.Reader opened through slx_sam_open.  No CPU fallback: without the library it raises, without a GPU slx_sam_open returns SLX_ENODEVICE;
slx_sam_sniff and slx_sam_parse_line are host only.
"""
import ctypes as C

from . import _ffi, bamio

# every symbol include/seqlib_amd_sam.h declares
SAM_EXPORTS = ["slx_sam_sniff", "slx_sam_open", "slx_sam_parse_line"]
COUNTERS = ("sam", "source", "lines", "fast_records", "slow_records", "us_lines", "us_fields", "us_size", "us_fill", "us_inflate")

_READY = False


def lib():
    global _READY
    L = bamio.lib()
    if not _READY:
        L.slx_sam_sniff.argtypes = [C.c_char_p]
        L.slx_sam_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        L.slx_sam_parse_line.argtypes = [C.c_char_p, C.c_int64, C.POINTER(C.c_char_p), C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        _READY = True
    return L


def sniff(path):
    """0: BAM, 1: SAM text; raises SlxError (SLX_EIO) when the file is unreadable or neither"""
    rc = lib().slx_sam_sniff(str(path).encode())
    if rc < 0:
        _ffi.check(rc)
    return rc


def parse_line(line, ref_names):
    """host only: one SAM line (bytes, no line feed) -> its block_size-prefixed BAM record; raises SlxError (SLX_EIO) when the line breaks a rule"""
    names = [n.encode() if isinstance(n, str) else n for n in ref_names]
    arr = (C.c_char_p * max(len(names), 1))(*names)
    n = C.c_int64(0)
    cap = 2 * len(line) + 64
    buf = C.create_string_buffer(cap)
    _ffi.check(lib().slx_sam_parse_line(line, len(line), arr, len(names), buf, cap, C.byref(n)))
    return buf.raw[:n.value]


class Reader(bamio.Reader):
    """slx_bam handle over SAM text"""

    def __init__(self, path, device=-1):
        self.h = C.c_void_p()
        _ffi.check(lib().slx_sam_open(str(path).encode(), device, C.byref(self.h)))
