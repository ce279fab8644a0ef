"""BGZF and BAM written and parsed with Python's zlib and struct only (SAMv1 sections 4.1, 4.2; RFC 1952): the independent statement of the
format the BamReader tests hold the GPU path against.  Nothing here touches the library."""
import random
import struct
import zlib

EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
MEMBER_MAX = 0xff00

# compression settings -> which deflate block types zlib 1.2.11 emits for them
SETTINGS = {
    "stored": dict(level=0),
    "fixed_memlevel1": dict(level=6, memLevel=1),
    "fixed": dict(level=6, strategy=zlib.Z_FIXED),
    "dyn1": dict(level=1),
    "dyn6": dict(level=6),
    "dyn9": dict(level=9),
    "rle": dict(level=6, strategy=zlib.Z_RLE),
    "huffman_only": dict(level=6, strategy=zlib.Z_HUFFMAN_ONLY),
    "full_flush": dict(level=6, flush_at=0.4),
}


def deflate_raw(payload, level=6, memLevel=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, memLevel, strategy)
    if flush_at is None:
        return c.compress(payload) + c.flush()
    cut = int(len(payload) * flush_at)
    return c.compress(payload[:cut]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(payload[cut:]) + c.flush()


def member_from_deflate(comp, payload):
    total = 18 + len(comp) + 8
    assert total <= 0x10000, total
    return (bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", total - 1) + comp +
            struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload)))


def bgzf_member(payload, **opts):
    return member_from_deflate(deflate_raw(payload, **opts), payload)


def bgzf_bytes(data, member_size=MEMBER_MAX, eof=True, **opts):
    out = [bgzf_member(data[i:i + member_size], **opts) for i in range(0, len(data), member_size)]
    return b"".join(out) + (EOF_BLOCK if eof else b"")


def scan_members(raw):
    """[(file_off, data_off, data_len, isize, crc32)], has_eof"""
    out, o = [], 0
    while o < len(raw):
        assert raw[o:o + 4] == b"\x1f\x8b\x08\x04", o
        xlen = struct.unpack_from("<H", raw, o + 10)[0]
        x, bsize = o + 12, None
        while x < o + 12 + xlen:
            si1, si2, slen = raw[x], raw[x + 1], struct.unpack_from("<H", raw, x + 2)[0]
            if (si1, si2, slen) == (0x42, 0x43, 2):
                bsize = struct.unpack_from("<H", raw, x + 4)[0]
            x += 4 + slen
        total = bsize + 1
        crc, isize = struct.unpack_from("<II", raw, o + total - 8)
        out.append((o, 12 + xlen, total - 12 - xlen - 8, isize, crc))
        o += total
    return out, bool(out) and raw[out[-1][0]:] == EOF_BLOCK


def inflate_all(raw):
    res = []
    for off, doff, dlen, isize, crc in scan_members(raw)[0]:
        d = zlib.decompress(raw[off + doff:off + doff + dlen], -15)
        assert len(d) == isize and (zlib.crc32(d) & 0xffffffff) == crc
        res.append(d)
    return b"".join(res)


# ---------------------------------------------------------------- BAM
SEQ_CODES = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "M": "K", "K": "M", "R": "Y", "Y": "R", "W": "W", "S": "S", "V": "B", "B": "V", "H": "D", "D": "H", "N": "N", "=": "="}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def reg2bin(beg, end):
    end -= 1
    for sh, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> sh == end >> sh:
            return base + (beg >> sh)
    return 0


def bam_record(name, flag=4, refid=-1, pos=-1, mapq=0, cigar=(), seq="", qual=None, aux=b"", next_refid=-1, next_pos=-1, tlen=0):
    """cigar: [(op_char, len)]; qual: bytes of phred values or None (0xff-filled)"""
    qn = name.encode() + b"\0"
    cig = b"".join(struct.pack("<I", (n << 4) | CIGAR_OPS.index(op)) for op, n in cigar)
    packed = bytearray((len(seq) + 1) // 2)
    for i, c in enumerate(seq):
        packed[i >> 1] |= SEQ_CODES.index(c) << (4 if i % 2 == 0 else 0)
    q = bytes(qual) if qual is not None else b"\xff" * len(seq)
    assert len(q) == len(seq)
    reflen = sum(n for op, n in cigar if op in "MDN=X")
    end = pos + (reflen if reflen else 1)
    core = struct.pack("<iiBBHHHiiii", refid, pos, len(qn), mapq, reg2bin(max(pos, 0), max(end, 1)) if pos >= 0 else 4680, len(cigar), flag, len(seq), next_refid, next_pos, tlen)
    body = core + qn + cig + bytes(packed) + q + aux
    return struct.pack("<I", len(body)) + body


def bam_header(text, refs):
    h = b"BAM\1" + struct.pack("<I", len(text)) + text.encode() + struct.pack("<I", len(refs))
    for name, ln in refs:
        h += struct.pack("<I", len(name) + 1) + name.encode() + b"\0" + struct.pack("<I", ln)
    return h


def bam_bytes(text, refs, records, member_size=MEMBER_MAX, header_own_members=True, **opts):
    """records: list of bam_record() byte strings"""
    h, body = bam_header(text, refs), b"".join(records)
    if header_own_members:
        return bgzf_bytes(h, member_size, eof=False, **opts) + bgzf_bytes(body, member_size, eof=True, **opts)
    return bgzf_bytes(h + body, member_size, eof=True, **opts)


def parse_bam(raw):
    """-> (text, [(name, len)], [dict(core fields..., data=blob after the 32 fixed bytes, raw=whole record with block_size)])"""
    s = inflate_all(raw)
    assert s[:4] == b"BAM\1"
    l_text = struct.unpack_from("<I", s, 4)[0]
    text = s[8:8 + l_text].rstrip(b"\0").decode()
    n_ref = struct.unpack_from("<I", s, 8 + l_text)[0]
    p, refs = 12 + l_text, []
    for _ in range(n_ref):
        l = struct.unpack_from("<I", s, p)[0]
        refs.append((s[p + 4:p + 4 + l - 1].decode(), struct.unpack_from("<I", s, p + 4 + l)[0]))
        p += 8 + l
    recs = []
    while p < len(s):
        bs = struct.unpack_from("<I", s, p)[0]
        refid, pos, l_name, mapq, bin_, n_cig, flag, l_seq, nrefid, npos, tlen = struct.unpack_from("<iiBBHHHiiii", s, p + 4)
        data = s[p + 36:p + 4 + bs]
        so = l_name + 4 * n_cig
        seq = "".join(SEQ_CODES[(data[so + (i >> 1)] >> (4 if i % 2 == 0 else 0)) & 15] for i in range(l_seq))
        recs.append(dict(refid=refid, pos=pos, l_name=l_name, mapq=mapq, bin=bin_, n_cigar=n_cig, flag=flag, l_seq=l_seq, next_refid=nrefid, next_pos=npos, tlen=tlen,
                         name=data[:l_name - 1].decode(), seq=seq, data=data, raw=s[p:p + 4 + bs]))
        p += 4 + bs
    return text, refs, recs


# ---------------------------------------------------------------- fixtures shared by the CPU and GPU tests
def sample_records(n=400, seed=5, n_ref=3):
    """mapped, reverse-strand, unmapped, secondary, long-name, aux-laden and zero-length-sequence records"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        kind = i % 7
        L = rng.randrange(30, 260)
        seq = "".join(rng.choice("ACGT") for _ in range(L))
        qual = bytes(rng.randrange(2, 41) for _ in range(L))
        name = "read%05d" % i
        aux = b"NMC" + bytes([rng.randrange(6)]) + b"ASi" + struct.pack("<i", rng.randrange(200))
        if kind == 0:
            out.append(bam_record(name, 0, rng.randrange(n_ref), rng.randrange(100000), 60, [("M", L)], seq, qual, aux))
        elif kind == 1:
            out.append(bam_record(name, 0x10, rng.randrange(n_ref), rng.randrange(100000), 30, [("S", 5), ("M", L - 10), ("S", 5)], seq, qual, aux))
        elif kind == 2:
            out.append(bam_record(name, 4, -1, -1, 0, [], seq, qual))
        elif kind == 3:
            out.append(bam_record(name, 0x100, rng.randrange(n_ref), rng.randrange(100000), 0, [("M", 10), ("D", 3), ("M", L - 10)], seq, None, aux))
        elif kind == 4:
            out.append(bam_record("n" * 200 + name, 0x41, rng.randrange(n_ref), rng.randrange(100000), 17, [("M", L)], seq, qual, aux, rng.randrange(n_ref), rng.randrange(100000), 311))
        elif kind == 5:
            big = b"XBBS" + struct.pack("<I", 300) + bytes(rng.randrange(256) for _ in range(600)) + b"XZZ" + b"some text" * 20 + b"\0"
            out.append(bam_record(name, 0x800, rng.randrange(n_ref), rng.randrange(100000), 3, [("H", 7), ("M", L)], "".join(rng.choice("ACGTNRY") for _ in range(L)), qual, aux + big))
        else:
            out.append(bam_record(name, 4, -1, -1, 0, [], "", b"", b"COZ" + b"no sequence\0"))
    return out


REFS = [("chrA", 200000), ("chrB", 150000), ("chrC", 100001)]
TEXT = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS) + "@PG\tID:bam_util\n"


def decoy_records(chunk=65536):
    """a record whose B:C aux array holds four chained plausible record headers, placed so that chunk 1 begins inside the array, just before them: the
    guess of that chunk takes the decoy, the resolution pass has to repair it"""
    first = bam_record("lead", 4, -1, -1, 0, [], "ACGT" * 25, bytes([30]) * 100)
    fake = bam_record("fk", 4, -1, -1, 0, [], "AC", bytes([1, 2]))            # a whole small record: chains to the next copy of itself
    pre = 36 + 6 + 0 + 0 + 0 + 3 + 1 + 4            # block_size, core, name "decoy\0", aux tag XB + 'B' + 'C' + count: bytes of the host record before the array
    pad = chunk - len(first) - pre + 40               # array bytes before the fakes: the fakes start 40 bytes into chunk 1
    arr = bytes([0xfe]) * pad + fake * 6 + bytes([0xfe]) * 50
    host = bam_record("decoy", 4, -1, -1, 0, [], "", b"", b"XBBC" + struct.pack("<I", len(arr)) + arr)
    tail = [bam_record("t%03d" % i, 4, -1, -1, 0, [], "ACGTACGTAC" * 10, bytes([20]) * 100) for i in range(1500)]
    return [first, host] + tail
