"""The BAI index (SAMv1 section 5.2) written, parsed and queried with Python's struct only, on top of tests/bam_util.py: the independent statement the
GPU index build (slx_bam_index_build), the host parser (slx_bai_query / slx_bai_stats) and the region iteration (slx_bam_set_regions) are held against.
Nothing here touches the library.  The rules, where the specification leaves a choice, are the ones include/seqlib_amd_bam.h states:
  end of a record     pos + reference length of the CIGAR (M D N = X); pos + 1 when that is 0 or the record carries 0x4
  bin                 reg2bin(pos, end), computed, the stored field is not trusted
  virtual offset      of whole-file inflated offset x: the first member m with start[m] + isize[m] > x gives file_off[m] << 16 | (x - start[m]); when x is
                      the end of the data, the file offset behind the last non-empty member << 16
  chunk               a maximal run of file-consecutive records with one (tid, bin), tid >= 0: (begin voff of the first, end voff of the last)
  linear index        per 16 KiB window the lowest begin voff of the records that touch it; an untouched window takes the next touched one above it
  pseudo-bin 37450    per reference with records (first begin voff, last end voff), (n_mapped, n_unmapped); n_no_coor counts the records with tid < 0
No merging of chunks inside one BGZF block and no lifting of sparse bins (htslib's post-pass): the index is valid without it."""
import bisect
import random
import struct

from tests import bam_util as bu

META_BIN = 37450
REF_OPS = (0, 2, 3, 7, 8)          # M D N = X


def rec_end(r):
    """r: a parse_bam() record"""
    cig = struct.unpack_from("<%dI" % r["n_cigar"], r["data"], r["l_name"])
    reflen = sum(c >> 4 for c in cig if (c & 15) in REF_OPS)
    return r["pos"] + (1 if reflen == 0 or r["flag"] & 4 else reflen)


class VoffMap:
    """whole-file inflated offset -> virtual offset"""

    def __init__(self, members):
        self.mem = [m for m in members if m[3] > 0]
        all_starts, run = [], 0
        for m in members:
            all_starts.append(run)
            run += m[3]
        self.starts = [s for s, m in zip(all_starts, members) if m[3] > 0]
        self.total = run
        last = self.mem[-1]
        self.behind = last[0] + last[1] + last[2] + 8

    def __call__(self, x):
        if x >= self.total:
            return self.behind << 16
        i = bisect.bisect_right(self.starts, x) - 1
        return self.mem[i][0] << 16 | (x - self.starts[i])


def record_offsets(raw, recs):
    """whole-file inflated offset of every record of parse_bam(raw), plus the end of the data"""
    total = sum(m[3] for m in bu.scan_members(raw)[0])
    off = [total - sum(len(r["raw"]) for r in recs)]
    for r in recs:
        off.append(off[-1] + len(r["raw"]))
    return off


class Unsorted(ValueError):
    def __init__(self, ordinal):
        ValueError.__init__(self, "record %d is out of order" % ordinal)
        self.ordinal = ordinal


def build_bai(raw):
    """the BAI of a coordinate-sorted BAM, as bytes; Unsorted names the first record that sorts before its predecessor"""
    _, refs, recs = bu.parse_bam(raw)
    vmap = VoffMap(bu.scan_members(raw)[0])
    off = record_offsets(raw, recs)
    for i in range(1, len(recs)):
        a, b = recs[i - 1], recs[i]
        if (b["refid"] & 0xffffffff, b["pos"]) < (a["refid"] & 0xffffffff, a["pos"]):
            raise Unsorted(i)
    n_ref = len(refs)
    chunks = [dict() for _ in range(n_ref)]          # bin -> [[beg, end]]
    lin = [dict() for _ in range(n_ref)]             # window -> min begin voff
    meta = [None] * n_ref
    n_no_coor = 0
    prev = None
    for i, r in enumerate(recs):
        tid = r["refid"]
        if tid < 0:
            n_no_coor += 1
            prev = None
            continue
        pos = max(r["pos"], 0)
        end = max(rec_end(r), pos + 1)
        b = bu.reg2bin(pos, end)
        vb, ve = vmap(off[i]), vmap(off[i + 1])
        if prev == (tid, b):
            chunks[tid][b][-1][1] = ve
        else:
            chunks[tid].setdefault(b, []).append([vb, ve])
        prev = (tid, b)
        for w in range(pos >> 14, ((end - 1) >> 14) + 1):
            lin[tid][w] = min(lin[tid].get(w, vb), vb)
        if meta[tid] is None:
            meta[tid] = [vb, ve, 0, 0]
        meta[tid][1] = ve
        meta[tid][3 if r["flag"] & 4 else 2] += 1
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    for t in range(n_ref):
        if meta[t] is None:
            out.append(struct.pack("<ii", 0, 0))
            continue
        out.append(struct.pack("<i", len(chunks[t]) + 1))
        for b in sorted(chunks[t]):
            out.append(struct.pack("<Ii", b, len(chunks[t][b])))
            for c in sorted(chunks[t][b]):
                out.append(struct.pack("<QQ", *c))
        out.append(struct.pack("<IiQQQQ", META_BIN, 2, *meta[t]))
        n_intv = max(lin[t]) + 1
        io, nxt = [0] * n_intv, 0
        for w in range(n_intv - 1, -1, -1):
            nxt = lin[t].get(w, nxt)
            io[w] = nxt
        out.append(struct.pack("<i%dQ" % n_intv, n_intv, *io))
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def parse_bai(b):
    """-> dict(refs=[dict(bins={bin: [(beg, end)]}, meta=(first, last, n_mapped, n_unmapped) or None, ioffset=[...])], n_no_coor=int or None)"""
    assert b[:4] == b"BAI\1"
    n_ref = struct.unpack_from("<i", b, 4)[0]
    p, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", b, p)[0]
        p += 4
        bins, meta = {}, None
        for _ in range(n_bin):
            bn, n_chunk = struct.unpack_from("<Ii", b, p)
            p += 8
            ch = [struct.unpack_from("<QQ", b, p + 16 * k) for k in range(n_chunk)]
            p += 16 * n_chunk
            if bn == META_BIN:
                meta = ch[0] + ch[1]
            else:
                bins[bn] = ch
        n_intv = struct.unpack_from("<i", b, p)[0]
        io = list(struct.unpack_from("<%dQ" % n_intv, b, p + 4))
        p += 4 + 8 * n_intv
        refs.append(dict(bins=bins, meta=meta, ioffset=io, n_bin=n_bin))
    n_no_coor = struct.unpack_from("<Q", b, p)[0] if p + 8 <= len(b) else None
    return dict(refs=refs, n_no_coor=n_no_coor)


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for sh, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += list(range(base + (beg >> sh), base + (end >> sh) + 1))
    return out


def query(bai, tid, beg, end):
    """the merged chunk list [(u, v)] that holds every record of tid overlapping [beg, end)"""
    beg, end = max(beg, 0), min(end, 1 << 29)
    if beg >= end:
        return []
    ref = bai["refs"][tid]
    io = ref["ioffset"]
    min_off = io[min(beg >> 14, len(io) - 1)] if io else 0
    ch = sorted(c for b in reg2bins(beg, end) for c in ref["bins"].get(b, []) if c[1] > min_off)
    out = []
    for u, v in ch:
        if out and u <= out[-1][1]:
            out[-1][1] = max(out[-1][1], v)
        else:
            out.append([u, v])
    return [tuple(c) for c in out]


def plan_members(members, chunks):
    """how many BGZF members the chunk list makes a reader inflate: per chunk from the member at u >> 16 through the one that holds the byte before v"""
    offs = [m[0] for m in members]
    n = 0
    for u, v in chunks:
        a = offs.index(u >> 16)
        b = offs.index(v >> 16) if (v >> 16) in offs else len(offs)
        n += b - a + (1 if v & 0xffff else 0)
    return n


def region_filter(recs, tid, beg, end):
    """brute force over parse_bam()'s records: the raw bytes of those a region serves, in file order"""
    return [r["raw"] for r in recs if r["refid"] == tid and r["pos"] < end and rec_end(r) > beg]


# ---------------------------------------------------------------- the sorted fixture
REFS = [("chrA", 200000), ("chrB", 150000), ("chrEmpty", 50000), ("chrC", 100001)]
TEXT = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS) + "@PG\tID:bai_util\n"
MEMBER_SIZE = 0x2000
N_POS = 20000              # the long-N record: 30M 100000N 30M from here
CIG300_POS = 40000


def sorted_specs(n=2600, seed=9):
    """keyword arguments of bu.bam_record, sorted by (tid as unsigned, pos); the edge cases of the index on purpose (see the module text of the tests)"""
    rng = random.Random(seed)
    specs = []

    def add(name, flag, tid, pos, cigar, L, **kw):
        seq = "".join(rng.choice("ACGT") for _ in range(L))
        specs.append(dict(name=name, flag=flag, refid=tid, pos=pos, mapq=kw.pop("mapq", 40), cigar=cigar, seq=seq, qual=bytes(rng.randrange(2, 41) for _ in range(L)), **kw))

    for i in range(n):
        kind, L = i % 8, rng.randrange(30, 200)
        tid = rng.choice((0, 0, 1, 3))
        pos = rng.randrange(REFS[tid][1] - 400)
        name = "r%05d" % i
        aux = b"NMC" + bytes([rng.randrange(6)])
        if kind in (0, 1, 2):
            add(name, 0, tid, pos, [("M", L)], L, aux=aux)
        elif kind == 3:
            add(name, 0x10, tid, pos, [("S", 5), ("M", L - 10), ("S", 5)], L, aux=aux)
        elif kind == 4:
            add(name, 0x100, tid, pos, [("M", 10), ("D", 3), ("M", L - 10)], L)
        elif kind == 5:
            add("n" * 180 + name, 0x41, tid, pos, [("=", L - 4), ("X", 1), ("I", 2), ("M", 1)], L, next_refid=tid, next_pos=pos + 300, tlen=311)
        elif kind == 6:
            add(name, 0x800, tid, pos, [("H", 7), ("M", L)], L, aux=aux + b"XZZ" + b"some text " * rng.randrange(1, 40) + b"\0")
        else:
            add(name, 4, -1, -1, [], L)                                                 # the unplaced tail
    add("at_zero", 0, 0, 0, [("M", 50)], 50)
    add("ends_16384", 0, 0, 16384 - 50, [("M", 50)], 50)
    add("starts_16384", 0, 1, 16384, [("M", 50)], 50)
    add("long_n", 0, 0, N_POS, [("M", 30), ("N", 100000), ("M", 30)], 60)
    add("no_cigar", 0, 1, 70000, [], 40)
    add("unmapped_placed", 0x4 | 0x1 | 0x8, 1, 70010, [("M", 40)], 40)
    add("cig300", 0, 0, CIG300_POS, [("M", 1), ("I", 1)] * 150, 300)
    add("pad", 0, 1, 50000, [("M", 80)], 80)
    specs.sort(key=lambda s: (s["refid"] & 0xffffffff, s["pos"]))
    return specs


def sorted_records(n=2600, seed=9, member_size=MEMBER_SIZE):
    """the records as bytes; the record "pad" carries an aux string sized so that it ends exactly where a member of member_size bytes ends"""
    specs = sorted_specs(n, seed)
    recs = [bu.bam_record(**s) for s in specs]
    k = [s["name"] for s in specs].index("pad")
    cum = sum(len(r) for r in recs[:k + 1])
    fill = (-cum) % member_size
    if fill < 4:
        fill += member_size
    recs[k] = bu.bam_record(aux=b"XPZ" + b"p" * (fill - 4) + b"\0", **specs[k])
    assert sum(len(r) for r in recs[:k + 1]) % member_size == 0
    return recs


def sorted_bam(n=2600, seed=9, member_size=MEMBER_SIZE):
    return bu.bam_bytes(TEXT, REFS, sorted_records(n, seed, member_size), member_size=member_size)
