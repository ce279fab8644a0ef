"""ctypes binding of include/seqlib_amd_edit.h (the record editor, part of libseqlib_amd.so) for tests and tools.

Plumbing only: the product is the C-ABI.  No CPU fallback: without the library it raises, on a host-only handle the apply calls return SLX_ENODEVICE; the plan
calls and record() are host only.
"""
import ctypes as C

from . import _ffi, bamio

# every symbol include/seqlib_amd_edit.h declares (checked by tests/test_edit_host.py against the header text)
EDIT_EXPORTS = ["slx_edit_create", "slx_edit_free", "slx_edit_plan_clear", "slx_edit_drop_tag", "slx_edit_drop_all_tags", "slx_edit_clear_seq_qual", "slx_edit_add_int", "slx_edit_add_z",
                "slx_edit_add_int_column", "slx_edit_add_z_column", "slx_edit_drop_column", "slx_edit_apply_device", "slx_edit_apply_host", "slx_edit_to_host", "slx_edit_record", "slx_edit_set", "slx_edit_counter"]
COUNTERS = ("device", "long_aux", "records", "long_records", "bytes_in", "bytes_out", "us_size", "us_scan", "us_gather")
HOST, AUTO = -1, -2


class Batch(C.Structure):
    _fields_ = [("n_records", C.c_int64), ("n_bytes", C.c_int64), ("d_stream", C.c_void_p), ("d_rec_off", C.c_void_p)]


_READY = False


def lib():
    global _READY
    L = bamio.lib()
    if not _READY:
        L.slx_edit_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.slx_edit_free.argtypes = [C.c_void_p]
        L.slx_edit_free.restype = None
        L.slx_edit_plan_clear.argtypes = [C.c_void_p]
        L.slx_edit_drop_tag.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_edit_drop_all_tags.argtypes = [C.c_void_p]
        L.slx_edit_clear_seq_qual.argtypes = [C.c_void_p]
        L.slx_edit_add_int.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int]
        L.slx_edit_add_z.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int64]
        L.slx_edit_add_int_column.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int32, C.c_int]
        L.slx_edit_add_z_column.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.slx_edit_drop_column.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_edit_apply_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(Batch)]
        L.slx_edit_apply_host.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.POINTER(C.c_uint64), C.c_int64, C.POINTER(Batch)]
        L.slx_edit_to_host.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(C.c_uint64)]
        L.slx_edit_record.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.slx_edit_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_edit_counter.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_edit_counter.restype = C.c_int64
        _READY = True
    return L


class Editor:
    """slx_edit handle"""

    def __init__(self, device=AUTO, **knobs):
        self.h = C.c_void_p()
        _ffi.check(lib().slx_edit_create(device, C.byref(self.h)))
        for k, v in knobs.items():
            self.set(k, v)

    def set(self, key, value):
        _ffi.check(lib().slx_edit_set(self.h, key.encode(), value))

    def counter(self, name):
        return int(lib().slx_edit_counter(self.h, name.encode()))

    # ---- the plan
    def plan_clear(self):
        _ffi.check(lib().slx_edit_plan_clear(self.h))

    def drop_tag(self, tag):
        _ffi.check(lib().slx_edit_drop_tag(self.h, bytes(tag)))

    def drop_all_tags(self):
        _ffi.check(lib().slx_edit_drop_all_tags(self.h))

    def clear_seq_qual(self):
        _ffi.check(lib().slx_edit_clear_seq_qual(self.h))

    def add_int(self, tag, value, replace=False):
        _ffi.check(lib().slx_edit_add_int(self.h, bytes(tag), value, int(replace)))

    def add_z(self, tag, value):
        _ffi.check(lib().slx_edit_add_z(self.h, bytes(tag), bytes(value), len(value)))

    def add_int_column(self, tag, d_vals, absent, replace=False):
        """d_vals: a device pointer as int (None on a host-only handle)"""
        _ffi.check(lib().slx_edit_add_int_column(self.h, bytes(tag), d_vals, absent, int(replace)))

    def add_z_column(self, tag, d_text, n_text, d_off):
        _ffi.check(lib().slx_edit_add_z_column(self.h, bytes(tag), d_text, n_text, d_off))

    def drop_column(self, tag):
        _ffi.check(lib().slx_edit_drop_column(self.h, bytes(tag)))

    # ---- batches
    def apply_device(self, d_stream, n_bytes, d_rec_off, n_records):
        """device pointers as ints -> Batch (valid until the next apply)"""
        b = Batch()
        _ffi.check(lib().slx_edit_apply_device(self.h, d_stream, n_bytes, d_rec_off, n_records, C.byref(b)))
        return b

    def apply_host(self, stream, rec_off):
        arr = (C.c_uint64 * len(rec_off))(*rec_off)
        b = Batch()
        _ffi.check(lib().slx_edit_apply_host(self.h, bytes(stream), len(stream), arr, len(rec_off) - 1, C.byref(b)))
        return b

    def to_host(self, b):
        """-> (bytes, [offsets])"""
        buf = C.create_string_buffer(max(b.n_bytes, 1))
        off = (C.c_uint64 * (b.n_records + 1))()
        _ffi.check(lib().slx_edit_to_host(self.h, C.byref(b), buf, off))
        return buf.raw[:b.n_bytes], list(off)

    def record(self, rec, col_int=None, col_z=None):
        """host only: one record under the plan; col_int / col_z: {add index: value} for the plan's columns"""
        ci = (C.c_int32 * 8)()
        cz = (C.c_char_p * 8)()
        cl = (C.c_int64 * 8)()
        for k, v in (col_int or {}).items():
            ci[k] = v
        for k, v in (col_z or {}).items():
            cz[k], cl[k] = bytes(v), len(v)
        n = C.c_int64(0)
        _ffi.check(lib().slx_edit_record(self.h, bytes(rec), len(rec), ci, cz, cl, None, 0, C.byref(n)))
        buf = C.create_string_buffer(max(n.value, 1))
        _ffi.check(lib().slx_edit_record(self.h, bytes(rec), len(rec), ci, cz, cl, buf, n.value, C.byref(n)))
        return buf.raw[:n.value]

    def close(self):
        if self.h:
            lib().slx_edit_free(self.h)
            self.h = None

    def __del__(self):
        if getattr(self, "h", None):
            self.close()
