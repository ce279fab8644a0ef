"""What the FASTQ reader tests share: an independent Python statement of the record grammar, the generators of the case list, and small BGZF / gzip writers.

The grammar is the one written at the top of include/SeqLib/FastqReader.h, stated here over whole lines with bytes.find -- not a port of the byte-at-a-time
parser, and not of seqlib_amd/csrc/fq_host.h.  tests/test_fastq_host.py holds it against the dump of the GetNextSequence loop (seqlib_api_test fastq).
"""
import random
import struct
import zlib

SPACE = b" \t\n\v\f\r"          # isspace() of the C locale


def _line(text, pos, dst):
    """One line of text from pos appended to dst (the line feed is not), then the CR rule on dst as a whole: a trailing CR goes when dst is longer than one
    byte.  -> (position behind the line, False when the input had already ended at pos)"""
    if pos >= len(text):
        return pos, False
    e = text.find(b"\n", pos)
    end, nxt = (len(text), len(text)) if e < 0 else (e, e + 1)
    dst += text[pos:end]
    if len(dst) > 1 and dst[-1] == 13:
        del dst[-1]
    return nxt, True


def parse(text):
    """-> (records, bad): records = [(name, com, seq, qual, flag)] as bytes and the flag byte of slx_fastq_batch.d_flags (bit 0: the header went on after the
    name, bit 1: a '+' block was read; a read without one has zero bytes as its quality); bad = the stream ended at a truncated or inconsistent quality."""
    recs, pos, n = [], 0, len(text)
    while True:
        cand = [i for i in (text.find(b">", pos), text.find(b"@", pos)) if i >= 0]
        if not cand:
            return recs, False
        pos = min(cand) + 1
        if pos >= n:
            return recs, False                      # a header byte and nothing after it: no record
        e = pos
        while e < n and text[e] not in SPACE:
            e += 1
        name, flag, com = text[pos:e], 0, bytearray()
        pos = e + 1                                  # behind the byte that ended the name (or the end of the input)
        if e < n and text[e] != 10:
            pos, went_on = _line(text, pos, com)
            flag |= 1 if went_on else 0
        seq = bytearray()
        while pos < n and text[pos] not in b">@+":
            if text[pos] == 10:
                pos += 1
                continue
            seq.append(text[pos])
            pos, _ = _line(text, pos + 1, seq)
        if pos >= n or text[pos] != 43:
            recs.append((bytes(name), bytes(com), bytes(seq), bytes(len(seq)), flag))
            continue                                # FASTA: the header byte at pos (if any) starts the next record
        e = text.find(b"\n", pos)
        if e < 0:
            return recs, True
        pos, qual = e + 1, bytearray()
        while True:
            pos, any_ = _line(text, pos, qual)
            if not any_ or len(qual) >= len(seq):
                break
        if len(qual) != len(seq):
            return recs, True
        recs.append((bytes(name), bytes(com), bytes(seq), bytes(qual), flag | 2))


# ---------------------------------------------------------------- generators
def _seq(rng, n):
    return bytes(rng.choice(b"ACGTNacgt") for _ in range(n))


def _qual(rng, n, first=None):
    q = bytes(rng.randrange(35, 74) for _ in range(n)).replace(b"@", b"A").replace(b"+", b",")          # '#' .. 'I'; '@' and '+' only where a case asks for them
    return (first + q[1:]) if first and n else q


def strict(records, final_newline=True):
    """records: [(header line without '@', seq, qual)] -> strict 4-line text"""
    t = b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in records)
    return t if final_newline else t[:-1]


def _reads(rng, lens, name=lambda i: b"r%d c%d x" % (i, i), first=None):
    return [(name(i), _seq(rng, n), _qual(rng, n, first)) for i, n in enumerate(lens)]


def sized(rng, size, first_line_end=None):
    """a strict file of exactly `size` bytes; first_line_end: position of the first line feed"""
    recs = _reads(rng, [rng.randrange(20, 60) for _ in range(6)], name=lambda i: b"s%d" % i)
    if first_line_end is not None:
        recs[0] = (b"n" * (first_line_end - 1), recs[0][1], recs[0][2])
    rest = size - len(strict(recs))          # one more record: '@' + name + '\n' + s + "\n+\n" + q + '\n' = 6 + len(name) + 2 len(s)
    assert rest >= 9, "size too small for the generator"
    ln = (rest - 7) // 2
    nm = rest - 6 - 2 * ln
    recs.append((b"z" * nm, _seq(rng, ln), _qual(rng, ln)))
    t = strict(recs)
    assert len(t) == size, (len(t), size)
    return t


def cases(tile=64):
    """-> [(name, text, is_strict)]: the case list of the FASTQ reader tests, each case also with CR LF line ends.  tile: the tile_bytes the size cases aim at."""
    rng = random.Random(20260)
    out = []
    out.append(("strict", strict(_reads(rng, [rng.randrange(30, 151) for _ in range(50)])), True))
    out.append(("qual_at", strict(_reads(rng, [5, 1, 40, 33, 2], first=b"@")), True))
    out.append(("qual_plus", strict(_reads(rng, [5, 1, 40, 33, 2], first=b"+")), True))
    names = [b"sp rest of it", b"tab\tafter tab", b"eol", b"", b"nocom", b"two  spaces", b"trail ", b"x\x0bvt", b"a b\tc"]
    out.append(("names", strict([(h, _seq(rng, 20 + i), _qual(rng, 20 + i)) for i, h in enumerate(names)]), True))
    out.append(("at_alone", strict([(b"", _seq(rng, 9), _qual(rng, 9))] * 3), True))
    out.append(("lengths", strict(_reads(rng, [1, 15, 16, 17, 2047, 2048, 2049, 5000, 1, 16])), True))
    for d in (-1, 0, 1):
        out.append(("size%+d" % d, sized(rng, 10 * tile + d), True))
        out.append(("line_end%+d" % d, sized(rng, 11 * tile + 3, first_line_end=tile + d), True))
    out.append(("no_final_newline", strict(_reads(rng, [31, 7, 64]), final_newline=False), True))
    out.append(("empty", b"", True))
    body = strict(_reads(rng, [30, 31, 32, 33]))
    out.append(("junk_first", b"some junk\nmore of it\n" + body, False))
    ml = b""
    for i, n in enumerate([70, 10, 130, 61]):
        s, q = _seq(rng, n), _qual(rng, n)
        ml += b"@m%d multi\n" % i + b"".join(s[j:j + 30] + b"\n" for j in range(0, n, 30)) + b"+m%d\n" % i + b"".join(q[j:j + 25] + b"\n" for j in range(0, n, 25))
    out.append(("multiline_fastq", ml, False))
    out.append(("fasta2", b"".join(b">f%d desc %d\n" % (i, i) + _seq(rng, 20 + i) + b"\n" for i in range(7)), False))
    out.append(("fasta_multi", b"".join(b">g%d\n" % i + b"".join(_seq(rng, 25) + b"\n" for _ in range(i + 1)) for i in range(5)) + b">last\nACGT", False))
    a, b_ = _reads(rng, [20, 21, 22]), _reads(rng, [23, 24])
    out.append(("blank_and_junk", strict(a[:1]) + b"\n\n" + strict(a[1:2]) + b"junk here\n" + strict(a[2:]) + b"\n" + strict(b_) + b"\n\n", False))
    pre, post = _reads(rng, [40] * 12, name=lambda i: b"p%d" % i), _reads(rng, [40] * 5, name=lambda i: b"q%d" % i)
    s, q = _seq(rng, 50), _qual(rng, 50)
    out.append(("one_multiline_mid", strict(pre) + b"@mid\n" + s[:25] + b"\n" + s[25:] + b"\n+\n" + q[:25] + b"\n" + q[25:] + b"\n" + strict(post), False))
    t = strict(_reads(rng, [30, 31, 32]))
    out.append(("truncated_qual", t[:-12], False))
    recs = _reads(rng, [20, 21, 22, 23, 24])
    recs[2] = (recs[2][0], recs[2][1], recs[2][2] + b"II")
    out.append(("long_qual_mid", strict(recs), False))
    return out + [(nm + "_crlf", tx.replace(b"\n", b"\r\n"), st) for nm, tx, st in out if tx]


ONE_MULTILINE_MID_BEFORE = 12          # records of "one_multiline_mid" before the multi-line one


# ---------------------------------------------------------------- compressed forms
def bgzf(text, member=0x1800, level=6):
    """text as a BGZF file: members of `member` inflated bytes, then the EOF block"""
    out = bytearray()
    for i in list(range(0, len(text), member)) + [None]:
        chunk = b"" if i is None else text[i:i + member]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        data = c.compress(chunk) + c.flush()
        out += struct.pack("<4BI2BH2BHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(data) + 25) + data + struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return bytes(out)


def gzip_(text, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(text) + c.flush()


def dump_expectations(path, case_list):
    """the cases and what parse() makes of them, for tests/cpp/fastq_host_test.cpp: u32 n; per case u32 + name, u32 + text, u32 strict, u32 bad, u32 n_rec, per record
    four (u32 + bytes) name, com, seq, qual and u32 flag"""
    blob = lambda b: struct.pack("<I", len(b)) + b
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(case_list)))
        for name, text, is_strict in case_list:
            recs, bad = parse(text)
            f.write(blob(name.encode()) + blob(text) + struct.pack("<III", int(is_strict), int(bad), len(recs)))
            for r in recs:
                f.write(b"".join(blob(x) for x in r[:4]) + struct.pack("<I", r[4]))
