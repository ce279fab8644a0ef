"""ctypes binding of include/seqlib_amd_filter.h (the read filter of libseqlib_amd.so) for tests and tools.

Plumbing only: the product is the C-ABI and SeqLib::Filter of include/SeqLib/ReadFilter.h.  No CPU fallback: without the library it raises, without a GPU
slx_filter_apply_device returns SLX_ENODEVICE; building a filter and testing one record on the host need none.
"""
import ctypes as C

from . import _ffi, bamio

# every symbol include/seqlib_amd_filter.h declares (checked by tests/test_filter_host.py against the header text)
FILTER_EXPORTS = ["slx_filter_create", "slx_filter_free", "slx_filter_add_filter", "slx_filter_add_rule", "slx_filter_apply_device", "slx_filter_attach",
                  "slx_filter_test_record", "slx_filter_features", "slx_filter_set", "slx_filter_counter"]
COUNTERS = ("seen", "passed", "us_filter", "long_records", "dfa_states", "dfa_in_lds")
RANGES = ("isize", "mapq", "len", "clip", "nm", "nbases", "ins", "del")
TRIS = ("dup", "supp", "qcfail", "hardclip", "mapped", "mate_mapped", "ff", "fr", "rf", "rr", "ic")


class Range(C.Structure):
    _fields_ = [("min", C.c_int32), ("max", C.c_int32), ("inverted", C.c_uint8), ("every", C.c_uint8), ("pad", C.c_uint8 * 2)]


class Rule(C.Structure):
    _fields_ = [("r", Range * 8), ("all_on", C.c_uint32), ("all_off", C.c_uint32), ("any_on", C.c_uint32), ("any_off", C.c_uint32), ("tri", C.c_uint32),
                ("subsample_seed", C.c_uint32), ("subsample_frac", C.c_double), ("motifs_inverted", C.c_uint32), ("pad", C.c_uint32)]


class Features(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("full_insert_size", "pair_orientation", "interchromosomal", "pair_mapped", "num_clip", "num_hard_clip", "max_ins", "max_del",
                                         "n_bases_n", "nm", "has_nm", "end")] + [("read_group", C.c_char * 256)]


_READY = False


def lib():
    global _READY
    L = bamio.lib()
    if not _READY:
        L.slx_filter_create.argtypes = [C.POINTER(C.c_void_p)]
        L.slx_filter_free.argtypes = [C.c_void_p]
        L.slx_filter_free.restype = None
        L.slx_filter_add_filter.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(bamio.Region), C.c_int64]
        L.slx_filter_add_rule.argtypes = [C.c_void_p, C.c_int, C.POINTER(Rule), C.c_char_p, C.POINTER(C.c_char_p), C.c_int64]
        L.slx_filter_apply_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]
        L.slx_filter_attach.argtypes = [C.c_void_p, C.c_void_p]
        L.slx_filter_test_record.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_filter_features.argtypes = [C.c_char_p, C.c_int64, C.POINTER(Features)]
        L.slx_filter_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.slx_filter_counter.argtypes = [C.c_void_p, C.c_char_p]
        L.slx_filter_counter.restype = C.c_int64
        _READY = True
    return L


def make_rule(spec):
    """spec: dict -- a range name -> (min, max, inverted); a tri-state name -> "on" | "off"; all_on / all_off / any_on / any_off -> mask;
    subsample -> (frac, seed).  (read_group and motifs travel beside the POD: see Filter.add_rule)"""
    r = Rule()
    for i, name in enumerate(RANGES):
        if name in spec:
            mn, mx, inv = spec[name]
            r.r[i] = Range(mn, mx, 1 if inv else 0, 0)
        else:
            r.r[i] = Range(0, 0, 0, 1)
    for i, name in enumerate(TRIS):
        if name in spec:
            r.tri |= {"on": 1, "off": 2}[spec[name]] << (2 * i)
    for name in ("all_on", "all_off", "any_on", "any_off"):
        setattr(r, name, spec.get(name, 0))
    r.subsample_frac, r.subsample_seed = spec.get("subsample", (1.0, 999))
    return r


def features(rec):
    """host only: the features of one block_size-prefixed record -> dict"""
    f = Features()
    _ffi.check(lib().slx_filter_features(bytes(rec), len(rec), C.byref(f)))
    d = {n: getattr(f, n) for n, _ in Features._fields_}
    d["read_group"] = f.read_group.decode(errors="replace")
    return d


class Filter:
    """slx_filter handle.  filters: [dict(excluder=, mate_linked=, regions=[(tid, p1, p2)] closed, rules=[spec])], spec as make_rule's with read_group / motifs"""

    def __init__(self, filters=()):
        self.h = C.c_void_p()
        _ffi.check(lib().slx_filter_create(C.byref(self.h)))
        for f in filters:
            fid = self.add_filter(f.get("excluder", False), f.get("mate_linked", False), f.get("regions", []))
            for spec in f.get("rules", []):
                self.add_rule(fid, spec)

    def close(self):
        if self.h:
            lib().slx_filter_free(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def add_filter(self, excluder=False, mate_linked=False, regions=()):
        arr = (bamio.Region * max(len(regions), 1))(*[bamio.Region(*g) for g in regions])
        rc = lib().slx_filter_add_filter(self.h, int(excluder), int(mate_linked), arr, len(regions))
        if rc < 0:
            _ffi.check(rc)
        return rc

    def add_rule(self, filter_id, spec):
        motifs = spec.get("motifs", [])
        arr = (C.c_char_p * max(len(motifs), 1))(*[m.encode() for m in motifs])
        rg = spec.get("read_group")
        _ffi.check(lib().slx_filter_add_rule(self.h, filter_id, C.byref(make_rule(spec)), rg.encode() if rg else None, arr, len(motifs)))

    def set(self, key, value):
        _ffi.check(lib().slx_filter_set(self.h, key.encode(), value))

    def counter(self, name):
        return int(lib().slx_filter_counter(self.h, name.encode()))

    def test_record(self, rec):
        rc = lib().slx_filter_test_record(self.h, bytes(rec), len(rec))
        if rc < 0:
            _ffi.check(rc)
        return bool(rc)

    def apply_device(self, d_stream, d_rec_off, n_records, d_keep, device=-1):
        """device pointers as ints -> the number kept"""
        k = C.c_int64(0)
        _ffi.check(lib().slx_filter_apply_device(self.h, device, d_stream, d_rec_off, n_records, d_keep, C.byref(k)))
        return k.value

    def attach(self, reader):
        _ffi.check(lib().slx_filter_attach(self.h, reader.h))

    @staticmethod
    def detach(reader):
        _ffi.check(lib().slx_filter_attach(None, reader.h))
