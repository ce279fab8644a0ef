"""ctypes binding of include/seqlib_amd_samw.h (the SAM text writer of libseqlib_amd.so) for tests and tools.

Plumbing only: the product is the C-ABI and SeqLib::BamWriter::UseGpuSam of include/SeqLib/BamWriter.h.  No CPU fallback: without the library it raises, without a
GPU slx_samw_open returns SLX_ENODEVICE; slx_samw_format_record is host only.
"""
import ctypes as C

from . import _ffi, bamio

# every symbol include/seqlib_amd_samw.h declares (checked by tests/test_samw_host.py against the header text)
SAMW_EXPORTS = ["slx_samw_open", "slx_samw_header", "slx_samw_write_device", "slx_samw_write_host", "slx_samw_format_device", "slx_samw_format_record", "slx_samw_set",
                "slx_samw_counter", "slx_samw_close"]
COUNTERS = ("records", "bytes", "batches", "fast_records", "slow_records", "wide_records", "extra_waves", "us_size", "us_fill")
SLX_SAMW_BGZF = 1


class Text(C.Structure):
    _fields_ = [("d_text", C.c_void_p), ("d_line_off", C.c_void_p), ("n_bytes", C.c_uint64), ("n_records", C.c_uint64)]


_READY = False


def lib():
    global _READY
    L = bamio.lib()
    if not _READY:
        L.slx_samw_open.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.slx_samw_header.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.POINTER(C.c_char_p), C.c_int]
        L.slx_samw_write_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        L.slx_samw_write_host.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.POINTER(C.c_uint64), C.c_int64]
        L.slx_samw_format_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(Text)]
        L.slx_samw_format_record.argtypes = [C.c_char_p, C.c_int64, C.POINTER(C.c_char_p), C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.slx_samw_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_samw_counter.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_samw_counter.restype = C.c_int64
        L.slx_samw_close.argtypes = [C.c_void_p]
        _READY = True
    return L


def _names(ref_names):
    names = [n.encode() if isinstance(n, str) else n for n in ref_names]
    return (C.c_char_p * max(len(names), 1))(*names), len(names)


def format_record(rec, ref_names):
    """host only: one block_size-prefixed record -> its SAM line (bytes, line feed included); raises SlxError (SLX_EIO) when the record is refused"""
    arr, n_ref = _names(ref_names)
    n = C.c_int64(0)
    cap = 12 * len(rec) + 256
    buf = C.create_string_buffer(cap)
    _ffi.check(lib().slx_samw_format_record(bytes(rec), len(rec), arr, n_ref, buf, cap, C.byref(n)))
    return buf.raw[:n.value]


class Writer:
    """slx_samw handle"""

    def __init__(self, path, device=-1, bgzf=False):
        self.h = C.c_void_p()
        _ffi.check(lib().slx_samw_open(str(path).encode(), device, SLX_SAMW_BGZF if bgzf else 0, C.byref(self.h)))

    def header(self, text, ref_names):
        text = text.encode() if isinstance(text, str) else text
        arr, n_ref = _names(ref_names)
        _ffi.check(lib().slx_samw_header(self.h, text, len(text), arr, n_ref))

    def set(self, key, value):
        _ffi.check(lib().slx_samw_set(self.h, key.encode(), value))

    def counter(self, name):
        return int(lib().slx_samw_counter(self.h, name.encode()))

    def write_host(self, stream, rec_off):
        arr = (C.c_uint64 * len(rec_off))(*rec_off)
        _ffi.check(lib().slx_samw_write_host(self.h, bytes(stream), len(stream), arr, len(rec_off) - 1))

    def write_device(self, d_stream, n_bytes, d_rec_off, n_records):
        """device pointers as ints"""
        _ffi.check(lib().slx_samw_write_device(self.h, d_stream, n_bytes, d_rec_off, n_records))

    def format_device(self, d_stream, n_bytes, d_rec_off, n_records):
        """-> Text: d_text / d_line_off stay valid until the next call on the writer"""
        t = Text()
        _ffi.check(lib().slx_samw_format_device(self.h, d_stream, n_bytes, d_rec_off, n_records, C.byref(t)))
        return t

    def close(self):
        if self.h:
            h, self.h = self.h, None
            _ffi.check(lib().slx_samw_close(h))

    def __del__(self):
        if getattr(self, "h", None):
            lib().slx_samw_close(self.h)
            self.h = None
