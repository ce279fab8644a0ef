"""The rules of include/seqlib_amd_edit.h, stated in Python: a strict aux parser, the plan, one record in and one record out; the record cases the host and the
GPU tests share.  Nothing here knows the C++ bodies: it follows the host sequence of the header (ClearSeqQualAndTags / RemoveAllTags / RemoveTag per name, then
AddZTag / AddIntTag per add) on a list of aux fields.
"""
import random
import struct

from tests import ref_util as ru

MAX_DROPS = MAX_ADDS = 8
MAX_CONST = 4096
FIXED = {ord("A"): 1, ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4, ord("d"): 8}
B_ELEM = {ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4}


class BadRecord(Exception):
    pass


class Plan:
    """drops: names in order; adds: (tag, kind, value, replace) with kind 'i' (value an int), 'Z' (bytes), 'ic' (value the absent int: column) or 'Zc' (column)"""

    def __init__(self, drops=(), drop_all=False, clear=False, adds=()):
        self.drops, self.drop_all, self.clear, self.adds = list(drops), drop_all, clear, list(adds)

    def columns(self):
        return [k for k, a in enumerate(self.adds) if a[1] in ("ic", "Zc")]


def tag_ok(t):
    return len(t) == 2 and chr(t[0]).isascii() and chr(t[0]).isalpha() and chr(t[1]).isascii() and chr(t[1]).isalnum()


def plan_error(plan):
    """the SLX_EINVAL of the plan calls, or None"""
    if len(plan.drops) > MAX_DROPS or len(plan.adds) > MAX_ADDS:
        return "too many"
    names = [a[0] for a in plan.adds]
    if any(not tag_ok(t) for t in plan.drops + names):
        return "tag"
    if len(set(names)) != len(names):
        return "twice"
    consts = [a[2] for a in plan.adds if a[1] == "Z"]
    if any(not v or b"\0" in v for v in consts):
        return "value"
    if sum(len(v) + 1 for v in consts) > MAX_CONST:
        return "constants"
    return None


def layout(rec):
    """(offset of the aux area, offset of seq) of a block_size-prefixed record; BadRecord when the fixed fields pass block_size"""
    if len(rec) < 36:
        raise BadRecord("short")
    bs, _tid, _pos, l_name, _mapq, _bin, n_cig, _flag, l_seq = struct.unpack_from("<IiiBBHHHi", rec)
    if bs + 4 != len(rec) or l_seq < 0:
        raise BadRecord("block_size")
    seq = 36 + l_name + 4 * n_cig
    aux = seq + (l_seq + 1) // 2 + l_seq
    if aux > len(rec):
        raise BadRecord("fields")
    return aux, seq


def aux_fields(aux):
    """[bytes] of the fields of an aux area; BadRecord unless it parses exactly to its end"""
    out, at, n = [], 0, len(aux)
    while at < n:
        if at + 3 > n:
            raise BadRecord("aux header")
        t = aux[at + 2]
        if t in FIXED:
            e = at + 3 + FIXED[t]
        elif t in (ord("Z"), ord("H")):
            z = aux.find(b"\0", at + 3)
            if z < 0:
                raise BadRecord("no NUL")
            e = z + 1
        elif t == ord("B"):
            if at + 8 > n or aux[at + 3] not in B_ELEM:
                raise BadRecord("B")
            e = at + 8 + B_ELEM[aux[at + 3]] * struct.unpack_from("<I", aux, at + 4)[0]
        else:
            raise BadRecord("type")
        if e > n:
            raise BadRecord("past the end")
        out.append(bytes(aux[at:e]))
        at = e
    return out


def _remove_first(fields, tag):
    for k, f in enumerate(fields):
        if f[:2] == tag:
            del fields[k]
            return


def apply(rec, plan, cols=()):
    """the edited record; cols[k]: the column value of add k (an int or bytes) where add k is a column"""
    aux_at, seq_at = layout(rec)
    fields = aux_fields(rec[aux_at:])          # (the aux area is validated whatever the plan does with it)
    head = bytearray(rec[:aux_at])
    if plan.clear:
        head = bytearray(rec[:seq_at])
        struct.pack_into("<i", head, 20, 0)
        fields = []
    elif plan.drop_all:
        fields = []
    else:
        for t in plan.drops:
            _remove_first(fields, t)
    for k, (tag, kind, value, replace) in enumerate(plan.adds):
        if kind in ("Z", "Zc"):
            v = value if kind == "Z" else cols[k]
            if not v:
                continue
            _remove_first(fields, tag)
            fields.append(tag + b"Z" + v + b"\0")
        else:
            v = value if kind == "i" else cols[k]
            if kind == "ic" and v == value:
                continue
            if replace:
                _remove_first(fields, tag)
            fields.append(tag + b"i" + struct.pack("<i", v))
    out = head + b"".join(fields)
    struct.pack_into("<I", out, 0, len(out) - 4)
    return bytes(out)


def apply_batch(recs, plan, cols=None):
    """cols: {add index: [value per record]}"""
    cols = cols or {}
    return [apply(r, plan, {k: v[i] for k, v in cols.items()}) for i, r in enumerate(recs)]


def first_bad(stream, off):
    """the record a batch is refused for (None: none): the offset table against the block_size words as rs_key (dev_recsort.h) tests it, then each record's own
    fields and aux area"""
    n, nb = len(off) - 1, len(stream)
    raw, off = off, [o - off[0] for o in off]          # (the offsets count from off[0])
    span_ok = lambda a, b: a < b <= nb and 36 <= b - a <= 0xffffffff
    bs = lambda a: struct.unpack_from("<I", stream, a)[0]
    for i in range(n):
        a, b = off[i], off[i + 1]
        if raw[i] < raw[0] or raw[i + 1] < raw[0]:
            return i
        if i > 0 and span_ok(off[i - 1], a) and bs(off[i - 1]) + 4 != a - off[i - 1]:
            return i
        if not span_ok(a, b) or (i + 1 == n and (b != nb or bs(a) + 4 != b - a)):
            return i
        if bs(a) + 4 != b - a:
            continue          # (record i + 1 is the one named)
        try:
            aux_at, _ = layout(stream[a:b])
            aux_fields(stream[a + aux_at:b])
        except BadRecord:
            return i
    return None


# ---------------------------------------------------------------- record cases
def aux_of(tag, typ, payload):
    return tag + typ + payload


EVERY_TYPE = b"".join([
    aux_of(b"XA", b"A", b"q"), aux_of(b"Xc", b"c", struct.pack("<b", -3)), aux_of(b"XC", b"C", b"\xfe"), aux_of(b"Xs", b"s", struct.pack("<h", -300)),
    aux_of(b"XS", b"S", struct.pack("<H", 60000)), aux_of(b"Xi", b"i", struct.pack("<i", -70000)), aux_of(b"XI", b"I", struct.pack("<I", 4000000000)),
    aux_of(b"Xf", b"f", struct.pack("<f", 1.5)), aux_of(b"Xd", b"d", struct.pack("<d", -2.25)), aux_of(b"XZ", b"Z", b"text with spaces\0"), aux_of(b"XH", b"H", b"1AE301\0"),
    aux_of(b"Bc", b"B", b"c" + struct.pack("<I", 3) + b"\x01\x02\xff"), aux_of(b"BC", b"B", b"C" + struct.pack("<I", 1) + b"\x09"),
    aux_of(b"Bs", b"B", b"s" + struct.pack("<Ihh", 2, -1, 2)), aux_of(b"BS", b"B", b"S" + struct.pack("<IHHH", 3, 1, 2, 3)),
    aux_of(b"Bi", b"B", b"i" + struct.pack("<Ii", 1, -5)), aux_of(b"BI", b"B", b"I" + struct.pack("<III", 2, 7, 8)), aux_of(b"Bf", b"B", b"f" + struct.pack("<Iff", 2, 0.5, 2.0)),
    aux_of(b"B0", b"B", b"S" + struct.pack("<I", 0)), aux_of(b"Z0", b"Z", b"\0"),
])
DROP8 = [b"D1", b"D2", b"D3", b"D4", b"D5", b"D6", b"D7", b"D8"]


def _cases():
    M = 0
    i4 = lambda tag, v: tag + b"i" + struct.pack("<i", v)
    z = lambda tag, v: tag + b"Z" + v + b"\0"
    out = []
    add = lambda name, aux, seq="ACGTACGTAC", cig=((M, 10),), qname=None: out.append((name, ru.raw_record(name if qname is None else qname, 0, 0, 4, list(cig), seq, aux=aux)))
    add("no_aux", b"")
    add("every_type", EVERY_TYPE)
    add("z_only_nul", z(b"MD", b""))
    add("cut_first", z(b"XA", b"chr1,+5,10M,0;") + i4(b"NM", 1) + z(b"RG", b"grp"))
    add("cut_middle", i4(b"NM", 1) + z(b"XA", b"chr1,+5,10M,0;") + z(b"RG", b"grp"))
    add("cut_last", i4(b"NM", 1) + z(b"RG", b"grp") + z(b"XA", b"chr1,+5,10M,0;"))
    add("cut_absent", i4(b"AS", 40) + z(b"PG", b"bwa"))
    add("cut_twice_present", z(b"XA", b"first;") + i4(b"AS", 3) + z(b"XA", b"second;") + z(b"XA", b"third;"))
    add("all_8_drops", b"".join(z(t, b"v" * (k + 1)) + i4(b"K%d" % k, k) for k, t in enumerate(DROP8)))
    add("adjacent_cuts", z(b"XA", b"a") + z(b"SA", b"b") + z(b"OQ", b"c"))
    add("only_cuts", z(b"XA", b"a"))
    add("l_seq_0", i4(b"NM", 0) + z(b"XA", b"x;"), seq="", cig=((M, 4),))
    add("n_cigar_0", i4(b"NM", 2) + z(b"SA", b"s;"), cig=())
    add("l_seq_0_n_cigar_0", b"", seq="", cig=())
    add("name_1_byte", z(b"XA", b"q"), qname="")
    add("name_254_bytes", i4(b"NM", 9) + z(b"XA", b"q"), qname="n" * 253)
    add("has_rg_and_nm", z(b"RG", b"old") + i4(b"NM", 7) + z(b"MD", b"10"))
    add("nm_twice", i4(b"NM", 1) + i4(b"NM", 2) + z(b"MD", b"3A6") + z(b"MD", b"10"))
    add("odd_l_seq", z(b"XA", b"odd"), seq="ACGTA", cig=((M, 5),))
    add("long_z", z(b"XA", b"chr2,-100,50M,1;" * 40) + i4(b"NM", 0) + z(b"SA", b"y" * 300))
    add("big_b", aux_of(b"BB", b"B", b"S" + struct.pack("<I", 500) + bytes(1000)) + z(b"XA", b"after the array"))
    return out


REC_CASES = _cases()
Z_VALUES = [b"", b"7", b"10A5^AC6", b"x" * 15, b"y" * 16, b"z" * 17]

# one plan of each kind; columns get their values from column_values
PLANS = {
    "identity": Plan(),
    "drop_names": Plan(drops=[b"XA", b"SA", b"OQ"]),
    "drop_xa_twice": Plan(drops=[b"XA", b"XA"]),
    "drop_8": Plan(drops=DROP8),
    "drop_all": Plan(drop_all=True),
    "clear": Plan(clear=True),
    "add_consts": Plan(adds=[(b"RG", "Z", b"group.1", False), (b"XN", "i", -17, False)]),
    "add_dropped_name": Plan(drops=[b"XA", b"RG"], adds=[(b"XA", "Z", b"new", False), (b"NM", "i", 5, False)]),
    "int_no_replace": Plan(adds=[(b"NM", "i", 42, False)]),
    "int_replace": Plan(adds=[(b"NM", "i", 42, True)]),
    "columns": Plan(adds=[(b"NM", "ic", -1, True), (b"MD", "Zc", None, False)]),
    "columns_no_replace": Plan(drops=[b"MD"], adds=[(b"XX", "ic", 0, False), (b"XY", "Zc", None, False), (b"RG", "Z", b"g", False)]),
    "clear_then_add": Plan(clear=True, adds=[(b"RG", "Z", b"cleared", False), (b"NM", "ic", -1, True)]),
    "drop_all_then_add": Plan(drop_all=True, drops=[], adds=[(b"MD", "Zc", None, False), (b"XN", "i", 1, True)]),
    "adds_8": Plan(drops=[b"XA"], adds=[(b"A%d" % k, "i", k, bool(k & 1)) for k in range(4)] + [(b"Z%d" % k, "Z", b"v" * (k + 1), False) for k in range(1, 5)]),
}


def column_values(plan, n, seed=1):
    """{add index: [value per record]}: ints that hit `absent` now and then, Z values of the lengths in Z_VALUES (the empty one among them)"""
    rng = random.Random(seed)
    cols = {}
    for k in plan.columns():
        tag, kind, value, _ = plan.adds[k]
        if kind == "ic":
            cols[k] = [value if (i % 5 == 2) else rng.randint(-1000, 1000) + (value == 0) * 2000 for i in range(n)]
        else:
            cols[k] = [Z_VALUES[(i + k) % len(Z_VALUES)] for i in range(n)]
    return cols


def z_column(values):
    """(text, offsets) in the layout of slx_ref_md: no terminators"""
    off = [0]
    for v in values:
        off.append(off[-1] + len(v))
    return b"".join(values), off


def rand_aux(rng, n_fields):
    out = []
    for _ in range(n_fields):
        tag = rng.choice([b"XA", b"SA", b"OQ", b"NM", b"MD", b"RG", b"AS", b"XS", b"D1", b"D2", b"BB", b"Xf"])
        k = rng.randrange(8)
        if k == 0:
            out.append(tag + b"Z" + bytes(rng.choice(b"ACGT;,+-0123456789") for _ in range(rng.choice((0, 1, 5, 14, 15, 16, 17, 40, 70, 200)))) + b"\0")
        elif k == 1:
            out.append(tag + b"i" + struct.pack("<i", rng.randint(-5, 500)))
        elif k == 2:
            out.append(tag + b"C" + bytes([rng.randrange(256)]))
        elif k == 3:
            cnt = rng.randrange(6)
            out.append(tag + b"Bs" + struct.pack("<I", cnt) + bytes(rng.randrange(256) for _ in range(2 * cnt)))
        elif k == 4:
            out.append(tag + b"H" + b"0AF1" * rng.randrange(4) + b"\0")
        elif k == 5:
            out.append(tag + b"A" + b"x")
        elif k == 6:
            out.append(tag + b"f" + struct.pack("<f", rng.random()))
        else:
            out.append(tag + b"S" + struct.pack("<H", rng.randrange(65536)))
    return b"".join(out)


def bulk_records(n=2000, seed=29):
    """the generated records of ref_util.bulk_records (read lengths 1..20 000), each with a generated aux area of 0..12 fields"""
    rng = random.Random(seed)
    out = []
    for r in ru.bulk_records(ru.bulk_contigs(), n=n):
        aux = rand_aux(rng, rng.choice((0, 1, 2, 3, 5, 8, 12)))
        body = r[4:] + aux
        out.append(struct.pack("<I", len(body)) + body)
    return out


def malformed_aux():
    """(name, record) whose aux area does not parse exactly to the record's end"""
    mk = lambda aux: ru.raw_record("bad", 0, 0, 4, [(0, 4)], "ACGT", aux=aux)
    return [
        ("unknown_type", mk(b"XAQ\x01")), ("z_without_nul", mk(b"NMi\0\0\0\0XAZabc")), ("h_without_nul", mk(b"XHH1A")), ("b_unknown_elem", mk(b"BBBd" + struct.pack("<I", 0))),
        ("b_past_the_end", mk(b"BBBi" + struct.pack("<I", 3) + bytes(11))), ("b_count_cut", mk(b"BBBi\x01\0")), ("header_cut", mk(b"NMi\0\0\0\0XA")), ("int_cut", mk(b"NMi\0\0")),
        ("b_huge_count", mk(b"BBBi" + struct.pack("<I", 0xffffffff) + bytes(4))),
    ]


def configure(ed, plan, bind=None):
    """the plan calls on a seqlib_amd.editio.Editor; bind: {add index: (d_vals,) or (d_text, n_text, d_off)} device pointers as ints (None: unbound columns)"""
    ed.plan_clear()
    for t in plan.drops:
        ed.drop_tag(t)
    if plan.drop_all:
        ed.drop_all_tags()
    if plan.clear:
        ed.clear_seq_qual()
    for k, (tag, kind, value, replace) in enumerate(plan.adds):
        if kind == "i":
            ed.add_int(tag, value, replace)
        elif kind == "Z":
            ed.add_z(tag, value)
        elif kind == "ic":
            ed.add_int_column(tag, bind[k][0] if bind else None, value, replace)
        else:
            ed.add_z_column(tag, *(bind[k] if bind else (None, 0, None)))
    return ed
