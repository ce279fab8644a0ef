"""SAM text <-> BAM records in Python only (SAMv1 sections 1.4, 1.5, 4.2): the independent statement of the grammar that include/seqlib_amd_sam.h lists and
sam_host.h / dev_sam.h restate in C.  Nothing here touches the library.  line_to_record is the expectation of every SAM test; record_to_line writes a line
from a BAM record so that the fixtures of bam_util serve here too."""
import re
import struct

import numpy as np

from tests import bam_util as bu

CIG_Q = "MIS=X"          # ops that consume the query
CIG_R = "MDN=X"          # ops that consume the reference
_INT = re.compile(rb"[-+]?[0-9]+\Z")
_UINT = re.compile(rb"[0-9]+\Z")
_FLOAT = re.compile(rb"[-+]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][-+]?[0-9]+)?\Z")
_HEX = re.compile(rb"([0-9A-Fa-f][0-9A-Fa-f])*\Z")
_CIG = re.compile(rb"([0-9]+)([MIDNSHP=X])")
B_RANGE = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2 ** 31, 2 ** 31 - 1), "I": (0, 2 ** 32 - 1)}
B_FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}


class SamError(ValueError):
    pass


def _uint(b, hi, what):
    if not _UINT.match(b) or int(b) > hi:
        raise SamError("%s is not a decimal number in [0, %d]" % (what, hi))
    return int(b)


def _f32(b, what):
    if not _FLOAT.match(b):
        raise SamError("%s is not a decimal floating-point number" % what)
    with np.errstate(over="ignore"):
        return np.float32(float(b)).tobytes()


def _aux(f):
    if len(f) < 5 or f[2:3] != b":" or f[4:5] != b":" or not re.match(rb"[A-Za-z][A-Za-z0-9]", f[:2]):
        raise SamError("an optional field is not TAG:TYPE:VALUE")
    tag, t, v = f[:2], chr(f[3]), f[5:]
    if t == "A":
        if len(v) != 1 or not 33 <= v[0] <= 126:
            raise SamError("an A field is not one printable byte")
        return tag + b"A" + v
    if t == "i":
        if not _INT.match(v) or not -2 ** 31 <= int(v) <= 2 ** 32 - 1:
            raise SamError("an i field is not an integer in [-2^31, 2^32)")
        x = int(v)
        if x >= 0:
            return tag + (b"C" + struct.pack("<B", x) if x <= 255 else b"S" + struct.pack("<H", x) if x <= 65535 else b"I" + struct.pack("<I", x))
        return tag + (b"c" + struct.pack("<b", x) if x >= -128 else b"s" + struct.pack("<h", x) if x >= -32768 else b"i" + struct.pack("<i", x))
    if t == "Z":
        return tag + b"Z" + v + b"\0"
    if t == "H":
        if not _HEX.match(v):
            raise SamError("an H field is not an even number of hex digits")
        return tag + b"H" + v + b"\0"
    if t == "f":
        return tag + b"f" + _f32(v, "an f field")
    if t == "d":
        if not _FLOAT.match(v):
            raise SamError("a d field is not a decimal floating-point number")
        return tag + b"d" + struct.pack("<d", float(v))
    if t == "B":
        if not v or chr(v[0]) not in B_FMT:
            raise SamError("a B field has no subtype from cCsSiIf")
        sub, el = chr(v[0]), v[1:].split(b",")
        if el[0] != b"":
            raise SamError("a B field's subtype is not followed by a comma")
        out = tag + b"B" + v[:1] + struct.pack("<I", len(el) - 1)
        for e in el[1:]:
            if sub == "f":
                out += _f32(e, "a B:f element")
            else:
                lo, hi = B_RANGE[sub]
                if not _INT.match(e) or not lo <= int(e) <= hi:
                    raise SamError("a B:%s element is outside the subtype's range" % sub)
                out += struct.pack("<" + B_FMT[sub], int(e))
        return out
    raise SamError("unknown optional field type '%s'" % t)


def line_to_record(line, refs):
    """line: bytes without the line feed (one trailing CR is dropped); refs: [(name, len)] -> the block_size-prefixed BAM record, or SamError"""
    if line.endswith(b"\r"):
        line = line[:-1]
    if not line:
        raise SamError("empty line")
    if line[:1] == b"@":
        raise SamError("header line after the first record")
    f = line.split(b"\t")
    if len(f) < 11:
        raise SamError("fewer than 11 fields")
    if any(len(x) == 0 for x in f[:11]):
        raise SamError("an empty mandatory field")
    names = {}
    for i, (nm, _) in enumerate(refs):
        names.setdefault(nm.encode() if isinstance(nm, str) else nm, i)
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    if len(qname) > 254:
        raise SamError("QNAME longer than 254 bytes")
    flag = _uint(flag, 65535, "FLAG")
    if rname == b"*":
        tid = -1
    elif rname in names:
        tid = names[rname]
    else:
        raise SamError("RNAME is not in the header")
    pos = _uint(pos, 2 ** 31 - 1, "POS") - 1
    mapq = _uint(mapq, 255, "MAPQ")
    ops = []
    if cigar != b"*":
        at = 0
        for m in _CIG.finditer(cigar):
            if m.start() != at:
                break
            at = m.end()
            if int(m.group(1)) > 2 ** 28 - 1:
                raise SamError("CIGAR op longer than 2^28 - 1")
            ops.append((m.group(2).decode(), int(m.group(1))))
        if at != len(cigar):
            raise SamError("CIGAR is not a list of <length><op> over MIDNSHP=X")
        if len(ops) > 65535:
            raise SamError("more than 65535 CIGAR ops: the CG:B form is not written")
    mtid = tid if rnext == b"=" else -1 if rnext == b"*" else names.get(rnext)
    if mtid is None:
        raise SamError("RNEXT is not in the header")
    pnext = _uint(pnext, 2 ** 31 - 1, "PNEXT") - 1
    if not _INT.match(tlen) or not -2 ** 31 <= int(tlen) <= 2 ** 31 - 1:
        raise SamError("TLEN does not fit int32")
    tlen = int(tlen)
    l_seq = 0 if seq == b"*" else len(seq)
    if ops and seq != b"*" and sum(n for op, n in ops if op in CIG_Q) != l_seq:
        raise SamError("CIGAR and SEQ differ in length")
    packed = bytearray((l_seq + 1) // 2)
    if seq != b"*":
        for i, c in enumerate(seq.upper()):
            k = bu.SEQ_CODES.find(chr(c)) if c < 128 else -1
            packed[i >> 1] |= (k if k >= 0 else 15) << (4 if i % 2 == 0 else 0)
    if qual == b"*":
        q = b"\xff" * l_seq
    else:
        if len(qual) != l_seq:
            raise SamError("SEQ and QUAL differ in length")
        if any(not 33 <= c <= 126 for c in qual):
            raise SamError("QUAL byte outside [33, 126]")
        q = bytes(c - 33 for c in qual)
    reflen = sum(n for op, n in ops if op in CIG_R)
    end = pos + (reflen if reflen and not flag & 4 else 1)
    bin_ = bu.reg2bin(pos, end) & 0xffff if pos >= 0 else 4680          # (the field holds 16 bits)
    aux = b"".join(_aux(x) for x in f[11:])
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(qname) + 1, mapq, bin_, len(ops), flag, l_seq, mtid, pnext, tlen) + qname + b"\0" + \
        b"".join(struct.pack("<I", n << 4 | bu.CIGAR_OPS.index(op)) for op, n in ops) + bytes(packed) + q + aux
    return struct.pack("<I", len(body)) + body


def _fmt_float(x):
    return repr(float(x)).encode()


def record_to_line(rec, refs):
    """a block_size-prefixed BAM record -> its SAM line (bytes, no line feed)"""
    tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq, mtid, mpos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 4)
    p = 36
    qname = rec[p:p + l_name - 1]
    p += l_name
    cig = b"".join(b"%d%s" % (w >> 4, bu.CIGAR_OPS[w & 15].encode()) for w in struct.unpack_from("<%dI" % n_cig, rec, p)) or b"*"
    p += 4 * n_cig
    seq = "".join(bu.SEQ_CODES[(rec[p + (i >> 1)] >> (4 if i % 2 == 0 else 0)) & 15] for i in range(l_seq)).encode() or b"*"
    p += (l_seq + 1) // 2
    q = rec[p:p + l_seq]
    qual = b"*" if not l_seq or q[0] == 0xff else bytes(c + 33 for c in q)
    p += l_seq
    rn = lambda t: refs[t][0].encode() if t >= 0 else b"*"
    f = [qname, b"%d" % flag, rn(tid), b"%d" % (pos + 1), b"%d" % mapq, cig, b"=" if mtid >= 0 and mtid == tid else rn(mtid), b"%d" % (mpos + 1), b"%d" % tlen, seq, qual]
    while p < len(rec):
        tag, t = rec[p:p + 2], chr(rec[p + 2])
        p += 3
        if t in "cCsSiI":
            v = struct.unpack_from("<" + B_FMT[t], rec, p)[0]
            p += struct.calcsize(B_FMT[t])
            f.append(tag + b":i:%d" % v)
        elif t == "A":
            f.append(tag + b":A:" + rec[p:p + 1])
            p += 1
        elif t in "ZH":
            e = rec.index(b"\0", p)
            f.append(tag + b":" + t.encode() + b":" + rec[p:e])
            p = e + 1
        elif t == "f":
            f.append(tag + b":f:" + _fmt_float(struct.unpack_from("<f", rec, p)[0]))
            p += 4
        elif t == "d":
            f.append(tag + b":d:" + _fmt_float(struct.unpack_from("<d", rec, p)[0]))
            p += 8
        elif t == "B":
            sub, n = chr(rec[p]), struct.unpack_from("<I", rec, p + 1)[0]
            vals = struct.unpack_from("<%d%s" % (n, B_FMT[sub]), rec, p + 5)
            p += 5 + n * struct.calcsize(B_FMT[sub])
            f.append(tag + b":B:" + sub.encode() + b"".join(b"," + (_fmt_float(v) if sub == "f" else b"%d" % v) for v in vals))
        else:
            raise ValueError("aux type %r" % t)
    return b"\t".join(f)


def split_lines(body):
    """(line without LF and without the one CR before it, 1-based line number) of a text; a last line without LF counts, and keeps a trailing CR"""
    out, p, no = [], 0, 1
    while p < len(body):
        e = body.find(b"\n", p)
        if e < 0:
            out.append((body[p:], no))
            break
        out.append((body[p:e - 1] if e > p and body[e - 1:e] == b"\r" else body[p:e], no))
        p, no = e + 1, no + 1
    return out


def parse_text(data):
    """a whole SAM file -> (header text, refs, records, bad): records up to the first bad line, bad = None or (1-based line number, message)"""
    lines = split_lines(data)
    text, refs, k = b"", [], 0
    while k < len(lines) and lines[k][0][:1] == b"@":
        ln = lines[k][0]
        text += ln + b"\n"
        if ln[:4] == b"@SQ\t" or ln == b"@SQ":
            kv = dict((x[:2], x[3:]) for x in ln.split(b"\t")[1:] if x[2:3] == b":")
            if b"SN" not in kv or b"LN" not in kv:
                raise SamError("@SQ line without SN or LN")
            refs.append((kv[b"SN"].decode(), int(kv[b"LN"])))
        k += 1
    recs = []
    for ln, no in lines[k:]:
        try:
            if ln.endswith(b"\r"):          # (only the last line without LF can: the CR is then part of its last field)
                raise SamError("CR at the end of the input without a line feed")
            recs.append(line_to_record(ln, refs))
        except SamError as e:
            return text, refs, recs, (no, str(e))
    return text, refs, recs, None


def sam_text(header, lines, eol=b"\n", last_eol=True):
    body = eol.join(lines) + (eol if last_eol and lines else b"")
    return (header.encode() if isinstance(header, str) else header) + body


def canonical(n=400):
    """(lines, expected records) of bam_util.sample_records(n): the expectation is the Python parser's, since integer aux come back in the smallest type"""
    lines = [record_to_line(r, bu.REFS) for r in bu.sample_records(n)]
    return lines, [line_to_record(l, bu.REFS) for l in lines]


def _l(qname=b"r", flag=b"0", rname=b"chrA", pos=b"100", mapq=b"60", cigar=b"4M", rnext=b"*", pnext=b"0", tlen=b"0", seq=b"ACGT", qual=b"IIII", aux=()):
    return b"\t".join([qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual] + list(aux))


# single-line cases: (name, line, True = parses / False = an error)
CASES = [
    ("plain", _l(), True),
    ("odd_l_seq", _l(cigar=b"5M", seq=b"ACGTA", qual=b"IIIII"), True),
    ("l_seq_1", _l(cigar=b"1M", seq=b"A", qual=b"I"), True),
    ("l_seq_1_qual_star", _l(cigar=b"1M", seq=b"A", qual=b"*"), True),
    ("seq_star_qual_star", _l(seq=b"*", qual=b"*"), True),
    ("qual_star_with_seq", _l(qual=b"*"), True),
    ("seq_star_with_qual", _l(seq=b"*", qual=b"II"), False),
    ("cigar_star", _l(cigar=b"*"), True),
    ("cigar_clips", _l(cigar=b"2H1S2M1I1D1N1=1X0P", seq=b"ACGTAC", qual=b"IIIIII"), True),
    ("cigar_bad_op", _l(cigar=b"4Q"), False),
    ("cigar_no_len", _l(cigar=b"M"), False),
    ("cigar_too_long_op", _l(cigar=b"268435456M", seq=b"*", qual=b"*"), False),
    ("cigar_max_op", _l(cigar=b"268435455N4M"), True),
    ("name_254", _l(qname=b"q" * 254), True),
    ("name_255", _l(qname=b"q" * 255), False),
    ("flag_max", _l(flag=b"65535"), True),
    ("flag_over", _l(flag=b"65536"), False),
    ("flag_hex", _l(flag=b"0x10"), False),
    ("flag_signed", _l(flag=b"+4"), False),
    ("unmapped_flag_with_cigar", _l(flag=b"4"), True),
    ("mapq_256", _l(mapq=b"256"), False),
    ("pos_0", _l(pos=b"0"), True),
    ("pos_max", _l(pos=b"2147483647"), True),
    ("pos_over", _l(pos=b"2147483648"), False),
    ("pos_neg", _l(pos=b"-1"), False),
    ("pos_bins", _l(pos=b"16384", cigar=b"2M100000N2M"), True),
    ("rnext_eq", _l(rnext=b"=", pnext=b"500", tlen=b"-404"), True),
    ("rnext_eq_unmapped", _l(rname=b"*", pos=b"0", rnext=b"="), True),
    ("rnext_other", _l(rnext=b"chrC", pnext=b"7", tlen=b"+12"), True),
    ("rnext_unknown", _l(rnext=b"chrZ"), False),
    ("rname_unknown", _l(rname=b"chrZ"), False),
    ("rname_prefix", _l(rname=b"chr"), False),
    ("tlen_min", _l(tlen=b"-2147483648"), True),
    ("tlen_over", _l(tlen=b"2147483648"), False),
    ("cigar_seq_mismatch", _l(cigar=b"5M"), False),
    ("qual_len_mismatch", _l(qual=b"III"), False),
    ("qual_low_byte", _l(qual=b"II I"), False),
    ("qual_high_byte", _l(qual=b"II\x7fI"), False),
    ("qual_edges", _l(qual=b"!~!~"), True),
    ("lower_iupac", _l(cigar=b"18M", seq=b"acgtnNmrswyhkvdb=.", qual=b"I" * 18), True),
    ("ten_fields", b"\t".join(_l().split(b"\t")[:10]), False),
    ("empty_field", _l(mapq=b""), False),
    ("empty_line", b"", False),
    ("at_line", b"@CO\tlate", False),
    ("crlf", _l() + b"\r", True),
    ("no_aux_trailing_tab", _l() + b"\t", False),
    ("aux_A", _l(aux=[b"XA:A:q"]), True),
    ("aux_A_two", _l(aux=[b"XA:A:qq"]), False),
    ("aux_A_space", _l(aux=[b"XA:A: "]), False),
    ("aux_Z", _l(aux=[b"XZ:Z:some text with spaces", b"YZ:Z:"]), True),
    ("aux_H", _l(aux=[b"XH:H:1AE301ff", b"YH:H:"]), True),
    ("aux_H_odd", _l(aux=[b"XH:H:1AE"]), False),
    ("aux_H_nonhex", _l(aux=[b"XH:H:1G"]), False),
    ("aux_f", _l(aux=[b"XF:f:1e-3", b"YF:f:-3.25", b"ZF:f:.5", b"WF:f:7."]), True),
    ("aux_f_bad", _l(aux=[b"XF:f:1e"]), False),
    ("aux_f_hex", _l(aux=[b"XF:f:0x1p3"]), False),
    ("aux_d", _l(aux=[b"XD:d:2.718281828459045", b"YD:d:-1e300"]), True),
    ("aux_d_empty", _l(aux=[b"XD:d:"]), False),
    ("aux_bad_type", _l(aux=[b"XX:q:1"]), False),
    ("aux_bad_tag", _l(aux=[b"1X:i:1"]), False),
    ("aux_short", _l(aux=[b"XX:i"]), False),
    ("aux_B_c_empty", _l(aux=[b"XB:B:c"]), True),
    ("aux_B_C_256", _l(aux=[b"XB:B:C,1,256"]), False),
    ("aux_B_empty_elem", _l(aux=[b"XB:B:C,1,,2"]), False),
    ("aux_B_no_comma", _l(aux=[b"XB:B:C1"]), False),
    ("aux_B_f", _l(aux=[b"XB:B:f,1.5,-2e3,0"]), True),
    ("aux_B_f_bad", _l(aux=[b"XB:B:f,1.5,x"]), False),
    ("aux_B_bad_sub", _l(aux=[b"XB:B:d,1"]), False),
    ("aux_after_float", _l(aux=[b"XF:f:1.0", b"XI:i:4294967296"]), False),
] + [("aux_i_%d" % v, _l(aux=[b"XI:i:%d" % v]), True) for v in (-2 ** 31, -32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1)] + \
    [("aux_i_over", _l(aux=[b"XI:i:4294967296"]), False), ("aux_i_under", _l(aux=[b"XI:i:-2147483649"]), False), ("aux_i_plus", _l(aux=[b"XI:i:+77"]), True),
     ("aux_i_long", _l(aux=[b"XI:i:" + b"9" * 40]), False), ("aux_i_zeros", _l(aux=[b"XI:i:" + b"0" * 40 + b"7"]), True), ("aux_i_empty", _l(aux=[b"XI:i:"]), False),
     ("aux_i_sign_only", _l(aux=[b"XI:i:-"]), False)] + \
    [("aux_B_%s" % s, _l(aux=[b"XB:B:" + s.encode() + b"".join(b",%d" % v for v in (lo, hi, 0))]), True) for s, (lo, hi) in B_RANGE.items()] + \
    [("aux_B_%s_over" % s, _l(aux=[b"XB:B:" + s.encode() + b",%d" % (hi + 1)]), False) for s, (lo, hi) in B_RANGE.items()] + \
    [("aux_B_%s_under" % s, _l(aux=[b"XB:B:" + s.encode() + b",%d" % (lo - 1)]), False) for s, (lo, hi) in B_RANGE.items()]


def is_slow(line):
    """does the line carry an f, d or B:f field (the fields the GPU fast path hands to the host parser)?"""
    return any(x[2:5] in (b":f:", b":d:") or x[2:6] == b":B:f" for x in line.split(b"\t")[11:])


def dump_expectations(path, case_list=None, refs=None):
    """the cases and what line_to_record makes of them, for tests/cpp/sam_host_test.cpp: u32 n_ref, per reference u32 + name; u32 n; per case u32 + name, u32 + line,
    u32 ok, u32 slow, u32 + record (empty when not ok)"""
    case_list = CASES if case_list is None else case_list
    refs = bu.REFS if refs is None else refs
    blob = lambda b: struct.pack("<I", len(b)) + b
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(refs)) + b"".join(blob(n.encode()) for n, _ in refs))
        f.write(struct.pack("<I", len(case_list)))
        for name, line, ok in case_list:
            try:
                rec = line_to_record(line, refs)
            except SamError:
                rec = None
            assert (rec is not None) == ok, name
            f.write(blob(name.encode()) + blob(line) + struct.pack("<II", int(ok), int(is_slow(line))) + blob(rec or b""))
