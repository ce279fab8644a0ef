"""The read statistics' rules in plain Python -- the second derivation the library (include/seqlib_amd_stats.h, seqlib_amd/csrc/dev_stats.h) is held against --
with the records the tests share.  Written from the rules at the top of the header and the reference's text (src/non_api/BamStats.cpp:21-109,
src/non_api/Histogram.cpp:14-73), not from the kernels.  Records are the dicts of tests/bam_util.parse_bam; the accessors are tests/filter_util's.  Nothing
here touches the library."""
import struct

from tests import bam_util as bu
from tests import filter_util as fu

HISTS = ("mapq", "nm", "isize", "clip", "phred", "len")
TEXT_COUNTERS = ("reads", "supp", "unmap", "mate_unmap", "qcfail", "duplicate")          # the order of the text
FLAG_COUNTERS = dict(supp=0x100, qcfail=0x200, duplicate=0x400, unmap=0x4, mate_unmap=0x8, supplementary=0x800, paired=0x1, proper_pair=0x2, read1=0x40, read2=0x80, reverse=0x10)
COUNTERS = ("reads", "supp", "qcfail", "duplicate", "unmap", "mate_unmap", "supplementary", "paired", "proper_pair", "read1", "read2", "reverse", "bases", "nm_missing")
HEADER = "ReadGroup\tReadCount\tSupplementary\tUnmapped\tMateUnmapped\tQCFailed\tDuplicate\tMappingQuality\tNM\tInsertSize\tClippedBases\tMeanPhredScore\tReadLength\n"
MAX_KEY = 255


def parse(rec):
    """one record's bytes -> the dict of bam_util.parse_bam"""
    refid, pos, l_name, mapq, bin_, n_cig, flag, l_seq, nrefid, npos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 4)
    data = bytes(rec[36:])
    return dict(refid=refid, pos=pos, l_name=l_name, mapq=mapq, bin=bin_, n_cigar=n_cig, flag=flag, l_seq=l_seq, next_refid=nrefid, next_pos=npos, tlen=tlen,
                name=data[:l_name].split(b"\0")[0].decode("latin-1"), data=data, raw=bytes(rec))


def group(r):
    """the group key, bytes"""
    for tag, ty, v in fu.aux_fields(r):
        if tag == "RG":
            if ty == "Z" and v:
                return bytes(v)
            break          # the first RG decides
    name = r["data"][:r["l_name"]].split(b"\0")[0]
    return b"QNAMED_" + (name[:name.index(b":")] if b":" in name else b"NA")


def qual(r):
    o = r["l_name"] + 4 * r["n_cigar"] + (r["l_seq"] + 1) // 2
    return r["data"][o:o + r["l_seq"]]


def values(r):
    """-> ({histogram: value}, has_nm); nm is 0 without an integer NM"""
    nm, has_nm = 0, False
    for tag, ty, v in fu.aux_fields(r):
        if tag == "NM":
            if ty in "cCsSiI":
                nm, has_nm = v, True
            break          # the first NM decides
    if not fu.pair_mapped(r):
        isize = -2
    elif r["refid"] != r["next_refid"]:
        isize = -1
    else:
        isize = abs(r["tlen"])
    phred = sum(qual(r)) // r["l_seq"] if r["l_seq"] > 0 else -1
    return dict(mapq=r["mapq"], nm=nm, isize=isize, clip=fu.num_clip(r), phred=phred, len=r["l_seq"]), has_nm


def bins(which, len_max=250, isize_max=2000):
    """[(first, second)] of Histogram(start, end, width), both included"""
    start, end, width = dict(mapq=(0, 100, 1), nm=(0, 100, 1), isize=(-2, isize_max, 10), clip=(0, 100, 5), phred=(0, 100, 1), len=(0, len_max, 1))[which]
    out, first, nxt = [], start, start + width - 1
    while nxt < end:
        out.append((first, nxt))
        first, nxt = nxt + 1, nxt + width
    out.append((first, end))
    return out


def accumulate(recs, exclude_flags=0, min_mapq=0, len_max=250, isize_max=2000):
    """recs: dicts.  -> [(name, {counter: n}, {histogram: ([bin counts], below, above)})] in order of first appearance: what Stats.groups() gives"""
    B = {h: bins(h, len_max, isize_max) for h in HISTS}
    order, by = [], {}
    for r in recs:
        if (r["flag"] & exclude_flags) or r["mapq"] < min_mapq:
            continue
        k = group(r)
        assert len(k) <= MAX_KEY
        if k not in by:
            by[k] = ({c: 0 for c in COUNTERS}, {h: [[0] * len(B[h]), 0, 0] for h in HISTS})
            order.append(k)
        cnt, hist = by[k]
        v, has_nm = values(r)
        cnt["reads"] += 1
        for c, bit in FLAG_COUNTERS.items():
            cnt[c] += bool(r["flag"] & bit)
        cnt["bases"] += r["l_seq"]
        cnt["nm_missing"] += not has_nm
        for h in HISTS:
            if h == "nm" and not has_nm:
                continue
            x = v[h]
            if x < B[h][0][0]:
                hist[h][1] += 1
            elif x > B[h][-1][1]:
                hist[h][2] += 1
            else:
                hist[h][0][[i for i, (lo, hi) in enumerate(B[h]) if lo <= x <= hi][0]] += 1
    return [(k, by[k][0], {h: tuple(by[k][1][h]) for h in HISTS}) for k in order]


def text(groups, len_max=250, isize_max=2000):
    """the text of accumulate()'s (or Stats.groups()'s) result, bytes"""
    out = [HEADER.encode()]
    for name, cnt, hist in groups:
        f = [name] + [b"%d" % cnt[c] for c in TEXT_COUNTERS]
        for h in HISTS:
            f.append(b",".join(b"%d_%d_%d" % (lo, hi, n) for (lo, hi), n in zip(bins(h, len_max, isize_max), hist[h][0]) if n))
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


# ---------------------------------------------------------------- the cases: the smallest inputs at which the body can go wrong
def _rec(name, flag=0, mapq=60, cigar=(("M", 10),), seq="ACGTACGTAC", q=None, aux=b"NMC\0RGZg1\0", tid=0, pos=100, mtid=-1, mpos=-1, tlen=0):
    if q is None:
        q = bytes(20 + (i * 7) % 21 for i in range(len(seq)))
    return bu.bam_record(name, flag, tid, pos, mapq, list(cigar), seq, q, aux, mtid, mpos, tlen)


def _pair(name, tlen, flag=0x1, mtid=0):
    return _rec(name, flag, tid=0, mtid=mtid, mpos=300, tlen=tlen)


def _ops(n):
    return [("SMIH"[i % 4], 1 + i % 3) for i in range(n)]


def _cases():
    C = []
    add = lambda n, r: C.append((n, r))
    add("rg_z", _rec("a:1"))
    add("rg_z_empty", _rec("lane7:1", aux=b"RGZ\0NMC\1"))
    add("rg_type_a", _rec("lane8:1", aux=b"RGAx"))
    add("rg_second_of_two", _rec("r", aux=b"RGZfirst\0RGZsecond\0"))
    add("rg_i_then_z", _rec("nocolon", aux=b"RGi" + struct.pack("<i", 3) + b"RGZlater\0"))
    add("name_colon", _rec("flow:cell:7", aux=b""))
    add("name_no_colon", _rec("readname", aux=b""))
    add("name_colon_first", _rec(":x", aux=b""))
    for ty, fmt, v in (("c", "<b", 7), ("C", "<B", 200), ("s", "<h", 30), ("S", "<H", 99), ("i", "<i", 5), ("I", "<I", 6)):
        add("nm_" + ty, _rec("r", aux=b"NM" + ty.encode() + struct.pack(fmt, v) + b"RGZg1\0"))
    add("nm_z", _rec("r", aux=b"NMZ7\0RGZg1\0"))
    add("nm_z_then_int", _rec("r", aux=b"NMZ7\0NMC\3RGZg1\0"))
    add("nm_absent", _rec("r", aux=b"RGZg1\0"))
    add("nm_negative", _rec("r", aux=b"NMc" + struct.pack("<b", -3) + b"RGZg1\0"))
    add("nm_100", _rec("r", aux=b"NMC\x64RGZg1\0"))
    add("nm_101", _rec("r", aux=b"NMC\x65RGZg1\0"))
    for q in (0, 100, 101, 255):
        add("mapq_%d" % q, _rec("r", mapq=q))
    add("isize_not_paired", _rec("r", 0, tid=0, mtid=0, mpos=300, tlen=50))
    add("isize_mate_unmapped", _pair("r", 50, 0x9))
    add("isize_read_unmapped", _pair("r", 50, 0x5))
    add("isize_other_contig", _pair("r", 50, 0x1, 1))
    for t in (0, 7, 8, 1997, 1998, 2000, 2001, -150, -2001, -2 ** 31, 2 ** 31 - 1):
        add("isize_%d" % t, _pair("r", t))
    for n in (0, 4, 5, 99, 100, 101):
        add("clip_%d" % n, _rec("r", cigar=[("M", 10)] + ([("S", n)] if n else [])))
    add("clip_hs_both_ends", _rec("r", cigar=[("H", 3), ("S", 4), ("M", 10), ("S", 6), ("H", 2)]))
    add("no_cigar", _rec("r", 4, cigar=[]))
    for n in (0, 1, 3, 4, 5, 250, 251):
        add("l_seq_%d" % n, _rec("r", seq=("ACGT" * 70)[:n]))
    add("qual_all_0", _rec("r", seq="ACGT" * 5, q=bytes(20)))
    add("qual_all_ff", _rec("r", seq="ACGT" * 5, q=b"\xff" * 20))
    add("qual_101", _rec("r", seq="ACGT" * 5, q=bytes([101]) * 20))
    add("qual_mixed_floor", _rec("r", seq="ACGTACG", q=bytes([40, 40, 40, 40, 40, 40, 39])))          # 279 / 7 = 39.86: the floor
    for k in range(4):          # the QUAL's start at each of the four byte alignments
        for n in (1, 2, 3, 6, 7, 9, 13):
            add("qual_align_%d_len_%d" % (k, n), _rec("q:" + "x" * k, seq=("ACGT" * 4)[:n], q=bytes(1 + (3 * i + k) % 90 for i in range(n))))
    add("key_255", _rec("r", aux=b"RGZ" + b"k" * 255 + b"\0"))
    add("key_256", _rec("r", aux=b"RGZ" + b"k" * 256 + b"\0"))
    add("qnamed_255", _rec("n" * 248 + ":", aux=b""))
    add("qnamed_256", _rec("n" * 249 + ":", aux=b""))
    add("name_254_no_colon", _rec("n" * 254, aux=b""))
    for n in (64, 65, 200):
        add("ops_%d" % n, _rec("r", cigar=_ops(n)))
    for k, fl in enumerate((0x100, 0x200, 0x400, 0x800, 0x4, 0x8, 0x1, 0x3, 0x41, 0x81, 0x10, 0xfff)):
        add("flag_%03x" % fl, _rec("fl:%d" % k, fl))
    add("other_group", _rec("r", aux=b"NMC\2RGZg2\0"))
    add("prefix_of_group", _rec("r", aux=b"NMC\2RGZg\0"))
    add("qnamed_looks_like_rg", _rec("r", aux=b"RGZQNAMED_NA\0"))
    return C


CASES = _cases()
FAILING = ("key_256", "qnamed_256")          # SLX_EUNSUPPORTED
GOOD = [r for n, r in CASES if n not in FAILING]


def bulk(n=780, seed=11):
    """filter_util's records (two of them longer than any stage, one that starts on the last byte of a 16384-byte window)"""
    return fu.records(n, seed)


def stream_of(recs):
    return fu.stream_of(recs)
