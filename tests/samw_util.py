"""BAM records -> SAM text in Python only: the independent statement of the rules that include/seqlib_amd_samw.h lists and dev_samw.h / samw_host.h restate in C
(the definition is BamWriter::format_sam).  It is sam_util.record_to_line with printf's %g for floating-point values and with the writer's refusals.  Nothing here
touches the library.  record_to_line is the expectation of every SAM writer test; CASES are the smallest records at which the kernels can go wrong."""
import struct

from tests import bam_util as bu

INT_FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}
OPCHR = "MIDNSHP=XB??????"
WIDE = 256          # CIGAR ops or B elements above which the size kernel takes a whole wave (SAMW_WIDE of slx_samw.hip)


class SamwError(ValueError):
    pass


def record_to_line(rec, refs):
    """a block_size-prefixed BAM record (bytes, its whole extent) -> its SAM line with the line feed, or SamwError; refs: [(name, len)] or [name]"""
    names = [(r[0] if isinstance(r, tuple) else r) for r in refs]
    names = [x.encode() if isinstance(x, str) else x for x in names]
    n = len(rec)
    if n < 36 or struct.unpack_from("<I", rec, 0)[0] + 4 != n:
        raise SamwError("extent is not block_size + 4")
    tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq, mtid, mpos, tlen = struct.unpack_from("<iiBBHHHIiii", rec, 4)
    o_cig = 36 + l_name
    o_seq = o_cig + 4 * n_cig
    o_qual = o_seq + (l_seq + 1) // 2
    o_aux = o_qual + l_seq
    if l_seq > 2 ** 31 - 1 or o_aux > n:
        raise SamwError("fields pass block_size")
    if tid >= len(names):
        raise SamwError("tid is not a reference")
    if mtid >= len(names):
        raise SamwError("mtid is not a reference")
    qname = rec[36:36 + l_name]
    if b"\0" not in qname:
        raise SamwError("no NUL inside l_read_name")
    qname = qname[:qname.index(b"\0")]
    cig = b"".join(b"%d%s" % (w >> 4, OPCHR[w & 15].encode()) for w in struct.unpack_from("<%dI" % n_cig, rec, o_cig)) or b"*"
    if l_seq:
        seq = "".join(bu.SEQ_CODES[(rec[o_seq + (i >> 1)] >> (4 if i % 2 == 0 else 0)) & 15] for i in range(l_seq)).encode()
        q = rec[o_qual:o_aux]
        qual = b"*" if q[0] == 0xff else bytes((c + 33) & 0xff for c in q)
    else:
        seq = qual = b"*"
    rn = lambda t: names[t] if t >= 0 else b"*"
    f = [qname, b"%d" % flag, rn(tid), b"%d" % (pos + 1), b"%d" % mapq, cig, b"=" if mtid >= 0 and mtid == tid else rn(mtid), b"%d" % (mpos + 1), b"%d" % tlen, seq, qual]
    p = o_aux
    while n - p >= 4:          # fewer than four trailing bytes are not a field
        tag, t = rec[p:p + 2], chr(rec[p + 2])
        p += 3
        if t == "A":
            f.append(tag + b":A:" + rec[p:p + 1])
            p += 1
        elif t in INT_FMT:
            w = struct.calcsize(INT_FMT[t])
            if n - p < w:
                raise SamwError("an optional field passes the record's end")
            f.append(tag + b":i:%d" % struct.unpack_from("<" + INT_FMT[t], rec, p)[0])
            p += w
        elif t in "fd":
            w = 4 if t == "f" else 8
            if n - p < w:
                raise SamwError("an optional field passes the record's end")
            f.append(tag + b":" + t.encode() + b":%g" % struct.unpack_from("<" + t, rec, p)[0])
            p += w
        elif t in "ZH":
            e = rec.find(b"\0", p)
            if e < 0:
                raise SamwError("a Z or H field has no NUL")
            f.append(tag + b":" + t.encode() + b":" + rec[p:e])
            p = e + 1
        elif t == "B":
            if n - p < 5:
                raise SamwError("an optional field passes the record's end")
            sub, cnt = chr(rec[p]), struct.unpack_from("<I", rec, p + 1)[0]
            if sub not in INT_FMT and sub != "f":
                raise SamwError("unknown B subtype")
            fmt = INT_FMT.get(sub, "f")
            if cnt * struct.calcsize(fmt) > n - p - 5:
                raise SamwError("an optional field passes the record's end")
            vals = struct.unpack_from("<%d%s" % (cnt, fmt), rec, p + 5)
            p += 5 + cnt * struct.calcsize(fmt)
            f.append(tag + b":B:" + sub.encode() + b"".join((b",%g" if sub == "f" else b",%d") % v for v in vals))
        else:
            raise SamwError("unknown optional field type")
    return b"\t".join(f) + b"\n"


def is_slow(rec):
    """does the record carry an f, d or B:f field (what the GPU hands to the host formatter)?  For records that record_to_line takes."""
    line = record_to_line(rec, [b"x"] * 64)
    return any(x[2:5] in (b":f:", b":d:") or x[2:6] == b":B:f" for x in line[:-1].split(b"\t")[11:])


def is_wide(rec):
    """is the record sized by a whole wave: more than WIDE CIGAR ops, or a B field of more than WIDE elements?  For records that record_to_line takes."""
    f = record_to_line(rec, [b"x"] * 64)[:-1].split(b"\t")
    return struct.unpack_from("<H", rec, 16)[0] > WIDE or any(x[2:5] == b":B:" and x.count(b",") > WIDE for x in f[11:])


def make(name=b"r", flag=0, tid=0, pos=99, mapq=60, cigar=(("M", 4),), seq="ACGT", qual=b"\x28" * 4, aux=b"", mtid=-1, mpos=-1, tlen=0):
    """a record from its fields; cigar: [(op char, len)]; qual: phred bytes, or None for the 0xff fill.  bin is left 0 (it is not printed)."""
    qn = name + b"\0"
    cig = b"".join(struct.pack("<I", (ln << 4) | bu.CIGAR_OPS.index(op)) for op, ln in cigar)
    packed = bytearray((len(seq) + 1) // 2)
    for i, c in enumerate(seq):
        packed[i >> 1] |= bu.SEQ_CODES.index(c) << (4 if i % 2 == 0 else 0)
    q = bytes(qual) if qual is not None else b"\xff" * len(seq)
    assert len(q) == len(seq)
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(qn), mapq, 0, len(cigar), flag, len(seq), mtid, mpos, tlen) + qn + cig + bytes(packed) + q + aux
    return struct.pack("<I", len(body)) + body


def _patch(rec, at, fmt, v):
    b = bytearray(rec)
    struct.pack_into(fmt, b, at, v)
    return bytes(b)


def _seq(n):
    return "".join(bu.SEQ_CODES[(7 * i + 3) % 16] for i in range(n))


def _ms(n, ln=1):
    return tuple((bu.CIGAR_OPS[i % 9], ln) for i in range(n))


def _b(sub, vals):
    return b"XBB" + sub.encode() + struct.pack("<I%d%s" % (len(vals), INT_FMT.get(sub, "f")), len(vals), *vals)


INT_RANGE = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2 ** 31, 2 ** 31 - 1), "I": (0, 2 ** 32 - 1)}
FLOATS = (0.0, -0.0, 1e-3, 3.4e38, float("inf"), float("nan"))
N_REF = len(bu.REFS)

# (name, record, True = a line / False = refused)
CASES = []
for _n in (0, 1, 2, 63, 64, 65, 127, 128, 129):
    CASES.append(("l_seq_%d" % _n, make(cigar=(("M", _n),) if _n else (), seq=_seq(_n), qual=bytes((i * 5) % 94 for i in range(_n))), True))
    if _n:
        CASES.append(("l_seq_%d_no_qual" % _n, make(cigar=(("M", _n),), seq=_seq(_n), qual=None), True))
CASES += [("n_cigar_%d" % _n, make(cigar=_ms(_n, 1 + _n % 7), seq="ACGTA", qual=b"\x00\x01\x02\x5d\x5e"), True) for _n in (0, 1, 63, 64, 65, WIDE, WIDE + 1, 65535)]
CASES += [
    ("cigar_lengths", make(cigar=(("M", 0), ("I", 9), ("D", 10), ("N", 2 ** 28 - 1), ("S", 99), ("H", 100), ("P", 999999), ("=", 1000000), ("X", 123456789))), True),
    ("cigar_op_codes_9_to_15", _patch(_patch(make(cigar=(("M", 5), ("M", 6), ("M", 7))), 36 + 2, "<I", 5 << 4 | 9), 36 + 2 + 4, "<I", 6 << 4 | 15), True),
    ("unmapped", make(flag=4, tid=-1, pos=-1, mapq=0, cigar=(), mtid=-1, mpos=-1), True),
    ("mate_same", make(tid=1, mtid=1, mpos=2 ** 31 - 2, tlen=-1), True),
    ("mate_other", make(tid=0, mtid=N_REF - 1, mpos=0, tlen=2 ** 31 - 1), True),
    ("mate_mapped_read_not", make(tid=-1, pos=-1, mtid=N_REF - 1, mpos=7, tlen=-2 ** 31), True),
    ("both_unmapped_equal", make(tid=-1, mtid=-1), True),
    ("last_reference", make(tid=N_REF - 1, pos=2 ** 31 - 2), True),
    ("pos_min", make(pos=-2 ** 31, mpos=-2 ** 31), True),
    ("flag_0_mapq_0", make(flag=0, mapq=0), True),
    ("flag_max_mapq_max", make(flag=65535, mapq=255), True),
    ("name_1", make(name=b"q"), True),
    ("name_254", make(name=b"n" * 254), True),
    ("name_with_inner_nul", make(name=b"ab\0cd"), True),
    ("qual_wraps", make(qual=bytes([0, 93, 222, 254])), True),
    ("aux_none", make(), True),
    ("aux_A", make(aux=b"XAAq" + b"YAA\t"), True),
    ("aux_Z", make(aux=b"XZZ\0" + b"YZZ" + bytes(33 + i % 90 for i in range(1000)) + b"\0" + b"ZZZone\0"), True),
    ("aux_H", make(aux=b"XHH1AE301ff\0YHH\0"), True),
    ("aux_float_between_ints", make(aux=b"NMC\x07XFf" + struct.pack("<f", 1.5) + b"ASi" + struct.pack("<i", -77) + b"XDd" + struct.pack("<d", 2.718281828459045) + b"XSs" + struct.pack("<h", -3)), True),
    ("aux_B_f_between", make(aux=b"NMC\x01" + _b("f", (1.5, -2e3)) + b"XSS" + struct.pack("<H", 65535)), True),
]
for _t, (_lo, _hi) in INT_RANGE.items():
    CASES.append(("aux_%s_ends" % _t, make(aux=b"".join(b"X" + bytes([65 + k]) + _t.encode() + struct.pack("<" + INT_FMT[_t], v) for k, v in enumerate((_lo, _hi, 0 if _lo else 10)))), True))
    for _n in (0, 1, 64, 65, 1000):
        CASES.append(("aux_B_%s_%d" % (_t, _n), make(aux=b"NMC\x02" + _b(_t, [(_lo, _hi, 0, 9, 10, 99, 100)[i % 7] for i in range(_n)]) + b"ZZZend\0"), True))
for _n in (0, 1, 64, 65, 1000):
    CASES.append(("aux_B_f_%d" % _n, make(aux=_b("f", [FLOATS[i % 6] * (1 if i < 6 else 0.5) for i in range(_n)]) + b"ZZZend\0"), True))
CASES += [("aux_f_%d" % k, make(aux=b"XFf" + struct.pack("<f", v)), True) for k, v in enumerate(FLOATS)]
CASES += [("aux_d_%d" % k, make(aux=b"XDd" + struct.pack("<d", v)), True) for k, v in enumerate(FLOATS + (1e300, -1.25e-300, 123456789.0))]
CASES += [("stray_%d" % k, make(aux=b"NMC\x05" + b"XYi"[:k]), True) for k in (1, 2, 3)]
CASES += [("stray_only_%d" % k, make(aux=b"\0\xff\0"[:k]), True) for k in (1, 2, 3)]
_ok = make(aux=b"NMC\x05")
CASES += [
    ("refuse_tid", make(tid=N_REF), False),
    ("refuse_mtid", make(mtid=N_REF), False),
    ("refuse_tid_far", make(tid=2 ** 31 - 1), False),
    ("refuse_name_no_nul", _patch(make(name=b"abc"), 36 + 3, "<B", 65), False),
    ("refuse_l_name_0", _patch(make(), 12, "<B", 0), False),
    ("refuse_fields_pass_l_seq", _patch(_ok, 20, "<i", 100), False),
    ("refuse_fields_pass_n_cigar", _patch(_ok, 16, "<H", 60000), False),
    ("refuse_l_seq_negative", _patch(_ok, 20, "<i", -1), False),
    ("refuse_block_size_short", _patch(_ok, 0, "<I", len(_ok) - 5), False),
    ("refuse_block_size_long", _patch(_ok, 0, "<I", len(_ok) - 3), False),
    ("refuse_block_size_small", struct.pack("<I", 20) + bytes(20), False),
    ("refuse_aux_i_cut", make(aux=b"XIi\x01\x02\x03"), False),
    ("refuse_aux_s_cut", make(aux=b"NMC\x01XSs\x01"), False),
    ("refuse_aux_f_cut", make(aux=b"NMC\x01XFf\x01\x02\x03"), False),
    ("refuse_aux_d_cut", make(aux=b"XDd" + bytes(7)), False),
    ("refuse_aux_B_head_cut", make(aux=b"XBBC\x01\x00\x00"), False),
    ("refuse_aux_B_array_cut", make(aux=b"XBBS" + struct.pack("<I", 3) + bytes(5)), False),
    ("refuse_aux_B_count_huge", make(aux=b"XBBI" + struct.pack("<I", 2 ** 32 - 1) + bytes(8)), False),
    ("refuse_aux_Z_no_nul", make(aux=b"XZZabc"), False),
    ("refuse_aux_H_no_nul", make(aux=b"NMC\x01XHH1A"), False),
    ("refuse_aux_type", make(aux=b"XXq\x01\x02"), False),
    ("refuse_aux_B_sub", make(aux=b"XBBd" + struct.pack("<I", 0) + b"\0"), False),
    ("refuse_after_float", make(aux=b"XFf" + struct.pack("<f", 1.0) + b"XXq\x01"), False),
]


def dump_expectations(path, case_list=None, refs=None):
    """the cases and what record_to_line makes of them, for tests/cpp/samw_host_test.cpp: u32 n_ref, per reference u32 + name; u32 n; per case u32 + name,
    u32 + record, u32 ok, u32 slow, u32 + line (empty when refused)"""
    case_list = CASES if case_list is None else case_list
    refs = bu.REFS if refs is None else refs
    blob = lambda b: struct.pack("<I", len(b)) + b
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(refs)) + b"".join(blob(n.encode()) for n, _ in refs))
        f.write(struct.pack("<I", len(case_list)))
        for name, rec, ok in case_list:
            try:
                line = record_to_line(rec, refs)
            except SamwError:
                line = None
            assert (line is not None) == ok, name
            f.write(blob(name.encode()) + blob(rec) + struct.pack("<II", int(ok), int(ok and is_slow(rec))) + blob(line or b""))


def stream_of(recs):
    """(the records one behind the other, their offsets as a list of len(recs) + 1)"""
    off = [0]
    for r in recs:
        off.append(off[-1] + len(r))
    return b"".join(recs), off
