"""The duplicate marker's rules (include/seqlib_amd_dup.h) stated again in Python, record by record with dictionaries, and the case lists the CPU and the GPU
tests share.  Nothing here touches the library."""
import random
import struct

from tests import bam_util as bu

IGNORED, FRAGMENT, PAIRED = 0, 1, 2
NOT_DUP, DUP, UNTOUCHED = 0, 1, 2
MAX_SCORE = 2 ** 31 - 1
WAVE_LEN = 512


class BadRecord(Exception):
    pass


def stream_of(recs):
    off = [0]
    for r in recs:
        off.append(off[-1] + len(r))
    return b"".join(recs), off


def fields(rec):
    """a whole record (block_size word included) -> dict; BadRecord when a field passes the block or the name has no NUL"""
    if len(rec) < 36 or struct.unpack_from("<I", rec, 0)[0] + 4 != len(rec):
        raise BadRecord("extent")
    refid, pos, l_name, mapq, bin_, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 4)
    if l_seq < 0:
        raise BadRecord("l_seq")
    seq_at = 36 + l_name + 4 * n_cig
    aux_at = seq_at + (l_seq + 1) // 2 + l_seq
    if aux_at > len(rec) or l_name < 1 or rec[36 + l_name - 1] != 0:
        raise BadRecord("fields")
    cigar = [(w & 15, w >> 4) for w in struct.unpack_from("<%dI" % n_cig, rec, 36 + l_name)]
    return dict(refid=refid, pos=pos, flag=flag, name=bytes(rec[36:36 + l_name - 1]), cigar=cigar, qual=bytes(rec[seq_at + (l_seq + 1) // 2:aux_at]), aux=bytes(rec[aux_at:]))


def first_rg(aux):
    """the value of the first RG field when it has type Z and is not empty, else None; None too where the area cannot be walked that far"""
    at, n = 0, len(aux)
    fixed = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}
    while at < n:
        if n - at < 3:
            return None
        tag, t = aux[at:at + 2], chr(aux[at + 2])
        if t in fixed:
            end = at + 3 + fixed[t]
        elif t in "ZH":
            z = aux.find(b"\0", at + 3)
            if z < 0:
                return None
            if tag == b"RG" and t == "Z":
                return aux[at + 3:z] or None
            end = z + 1
        elif t == "B":
            if n - at < 8 or chr(aux[at + 3]) not in fixed or chr(aux[at + 3]) in "Ad":
                return None
            end = at + 8 + fixed[chr(aux[at + 3])] * struct.unpack_from("<I", aux, at + 4)[0]
        else:
            return None
        if end > n or tag == b"RG":
            return None
        at = end
    return None


def libraries(header_text):
    """{read group id (bytes): library number} of a header text"""
    text = header_text.encode() if isinstance(header_text, str) else bytes(header_text or b"")
    text = text.split(b"\0")[0]
    by_lb, by_id = {}, {}
    n = 0
    for line in text.split(b"\n"):
        if not line.startswith(b"@RG\t"):
            continue
        fs = line.split(b"\t")[1:]
        ids = [f[3:] for f in fs if f.startswith(b"ID:")]
        lbs = [f[3:] for f in fs if f.startswith(b"LB:")]
        if not ids or not ids[0] or ids[0] in by_id:
            continue
        if lbs and lbs[0] in by_lb:
            lib = by_lb[lbs[0]]
        else:
            n += 1
            lib = n
            if lbs:
                by_lb[lbs[0]] = lib
        by_id[ids[0]] = lib
    return by_id


def library_of(header_text, rg):
    return libraries(header_text).get(bytes(rg), 0) if rg else 0


def signature(rec, header_text=None):
    """-> (class, library, refID, upos, reverse, score); (IGNORED, 0, 0, 0, 0, 0) for an ignored record"""
    f = fields(rec)
    if f["flag"] & (0x4 | 0x100 | 0x800) or f["refid"] < 0:
        return (IGNORED, 0, 0, 0, 0, 0)
    ops = f["cigar"]
    ref_len = sum(n for op, n in ops if op in (0, 2, 3, 7, 8))
    lead = trail = 0
    for op, n in ops:
        if op not in (4, 5):
            break
        lead += n
    for op, n in reversed(ops):
        if op not in (4, 5):
            break
        trail += n
    rev = 1 if f["flag"] & 0x10 else 0
    upos = f["pos"] + ref_len - 1 + trail if rev else f["pos"] - lead
    score = min(sum(q for q in f["qual"] if 15 <= q <= 0xfe), MAX_SCORE)
    paired = bool(f["flag"] & 0x1) and not f["flag"] & 0x8
    return (PAIRED if paired else FRAGMENT, library_of(header_text, first_rg(f["aux"])), f["refid"], upos, rev, score)


def mark(batches, header_text=None):
    """batches: lists of whole records -> ([verdict per ordinal: NOT_DUP, DUP or UNTOUCHED], counters)"""
    recs = [r for b in batches for r in b]
    sig = [signature(r, header_text) for r in recs]
    flds = [fields(r) for r in recs]
    ver = [UNTOUCHED if s[0] == IGNORED else NOT_DUP for s in sig]
    E = lambda o: sig[o][1:5]
    by_name = {}
    for o, s in enumerate(sig):
        if s[0] == PAIRED:
            by_name.setdefault((s[1], flds[o]["name"]), []).append(o)
    pairs = []
    for group in by_name.values():
        if len(group) == 2:
            a, b = (flds[o]["flag"] for o in group)
            if (a & 0x40 and b & 0x80) or (a & 0x80 and b & 0x40):
                pairs.append(tuple(group))
    by_ends = {}
    for a, b in pairs:
        by_ends.setdefault(tuple(sorted((E(a), E(b)))), []).append((a, b))
    dup_pairs = 0
    for group in by_ends.values():
        best = min(group, key=lambda p: (-(sig[p[0]][5] + sig[p[1]][5]), min(p)))
        for p in group:
            if p != best:
                ver[p[0]] = ver[p[1]] = DUP
                dup_pairs += 1
    by_e = {}
    for o, s in enumerate(sig):
        if s[0] != IGNORED:
            by_e.setdefault(E(o), []).append(o)
    dup_frags = 0
    for group in by_e.values():
        frags = [o for o in group if sig[o][0] == FRAGMENT]
        if not frags:
            continue
        keep = None if len(frags) < len(group) else min(frags, key=lambda o: (-sig[o][5], o))
        for o in frags:
            if o != keep:
                ver[o] = DUP
                dup_frags += 1
    n_paired = sum(s[0] == PAIRED for s in sig)
    counters = dict(records=len(recs), ignored=sum(s[0] == IGNORED for s in sig), paired=n_paired, fragments=sum(s[0] == FRAGMENT for s in sig), pairs=len(pairs),
                    orphans=n_paired - 2 * len(pairs), duplicate_pairs=dup_pairs, duplicate_fragments=dup_frags, duplicates=2 * dup_pairs + dup_frags)
    return ver, counters


def marked(rec, verdict):
    """the record as apply leaves it"""
    if verdict == UNTOUCHED:
        return bytes(rec)
    out = bytearray(rec)
    flag = struct.unpack_from("<H", rec, 18)[0]
    struct.pack_into("<H", out, 18, flag | 0x400 if verdict == DUP else flag & ~0x400)
    return bytes(out)


# ---------------------------------------------------------------- records
def rg_aux(rg):
    return b"RGZ" + rg + b"\0"


def record(name, refid, pos, cigar=None, qual=None, flag=0, aux=b"", l_seq=None):
    """cigar: [(op_char, len)] or None for <l_seq>M; qual: bytes, or None for phred 30 throughout"""
    if l_seq is None:
        l_seq = len(qual) if qual is not None else (sum(n for op, n in cigar if op in "MIS=X") if cigar is not None else 50)
    if cigar is None:
        cigar = [("M", l_seq)] if l_seq else []
    if qual is None:
        qual = bytes([30]) * l_seq
    return bu.bam_record(name, flag, refid, pos, 60, cigar, "A" * l_seq, qual, aux)


def pair(name, refid, pos1, pos2, qual=None, refid2=None, flag1=0, flag2=0, aux=b"", cigar1=None, cigar2=None, l_seq=50):
    """a forward first read at pos1 and a reverse second read at pos2 (flag1 / flag2 are or-ed in)"""
    return [record(name, refid, pos1, cigar1, qual, 0x1 | 0x40 | 0x20 | flag1, aux, l_seq), record(name, refid if refid2 is None else refid2, pos2, cigar2, qual, 0x1 | 0x80 | 0x10 | flag2, aux, l_seq)]


HEADER = ("@HD\tVN:1.6\n@SQ\tSN:chrA\tLN:200000\n@RG\tID:a1\tLB:libA\tSM:s\n@RG\tID:a2\tSM:s\tLB:libA\n@RG\tID:b\tLB:libB\n@RG\tID:solo\tSM:s\n@RG\tID:a\tLB:libC\n"
          "@RG\tSM:noid\tLB:libD\n@RG\tID:a1\tLB:libE\n@CO\t@RG\tID:comment\n")
HEADERS = {
    "no_rg": "@HD\tVN:1.6\n@SQ\tSN:chrA\tLN:200000\n",
    "shared_lb": "@RG\tID:x\tLB:one\n@RG\tID:y\tLB:two\n@RG\tID:z\tLB:one\n",
    "without_lb": "@RG\tID:x\n@RG\tID:y\tLB:one\n@RG\tID:z\n",
    "prefix_id": "@RG\tID:grp\tLB:one\n@RG\tID:grp1\tLB:two\n@RG\tID:g\tLB:three\n",
    "mixed": HEADER,
    "nul_padded": "@RG\tID:x\tLB:one\n\0@RG\tID:y\tLB:two\n",
    "empty": "",
}
RG_PROBES = [b"", b"x", b"y", b"z", b"grp", b"grp1", b"grp12", b"gr", b"g", b"a", b"a1", b"a2", b"b", b"solo", b"comment", b"noid", b"X"]


def long_cigar(n_ops, lead_clip=True, trail_clip=True):
    """n_ops operations: clips at the ends where asked, M and I / D / N / = / X / P alternating between them"""
    ops = []
    if lead_clip and n_ops >= 3:
        ops += [("H", 3), ("S", 2)]
    tail = [("S", 4), ("H", 1)] if trail_clip and n_ops >= len(ops) + 3 else []
    mid = "IDN=XP"
    k = 0
    while len(ops) + len(tail) < n_ops:
        ops.append(("M", 2) if k % 2 == 0 else (mid[(k // 2) % 6], 1 + k % 3))
        k += 1
    return (ops + tail)[:n_ops]


def edge_records():
    """[(label, record)]: the CIGAR shapes, the lane / wave edges of the CIGAR and of the qualities, the counted and the uncounted quality bytes, the classes and
    the library cases under HEADER"""
    out = []
    add = lambda label, *a, **k: out.append((label, record(label, *a, **k)))
    for strand, fl in (("f", 0), ("r", 0x10)):
        add("noclip_" + strand, 0, 1000, [("M", 50)], flag=fl)
        add("s_lead_" + strand, 0, 1000, [("S", 5), ("M", 45)], flag=fl)
        add("hs_lead_" + strand, 0, 1000, [("H", 7), ("S", 5), ("M", 45)], flag=fl)
        add("s_trail_" + strand, 0, 1000, [("M", 45), ("S", 5)], flag=fl)
        add("sh_trail_" + strand, 0, 1000, [("M", 45), ("S", 5), ("H", 9)], flag=fl)
        add("both_" + strand, 0, 1000, [("H", 2), ("S", 3), ("M", 40), ("S", 7), ("H", 4)], flag=fl)
        add("clips_only_" + strand, 0, 1000, [("S", 20), ("H", 3)], flag=fl)
        add("empty_cigar_" + strand, 0, 1000, [], flag=fl, l_seq=10)
        add("inner_clip_" + strand, 0, 1000, [("S", 2), ("M", 10), ("S", 3), ("M", 10), ("S", 4)], flag=fl)
        for op in "IDNP=X":
            add("op_%s_%s" % (op, strand), 0, 1000, [("M", 20), (op, 3), ("M", 20)], flag=fl)
        for n_ops in (1, 64, 65, 200):
            add("ops%d_%s" % (n_ops, strand), 0, 5000, long_cigar(n_ops), flag=fl)
        add("ops130_noclip_" + strand, 0, 5000, long_cigar(130, False, False), flag=fl)
        add("ops70_clips_only_" + strand, 0, 5000, [("S", 1 + k % 3) for k in range(70)], flag=fl)
        add("ops129_lead_run_66_" + strand, 0, 5000, [("S", 1)] * 66 + [("M", 2)] * 60 + [("H", 2)] * 3, flag=fl)
    rng = random.Random(11)
    for n in (0, 1, 3, 4, 5, 63, 64, 65, WAVE_LEN - 1, WAVE_LEN, WAVE_LEN + 1, 2051):
        add("lseq%d" % n, 1, 300, qual=bytes(rng.choice((3, 14, 15, 16, 40, 93, 0xfe, 0xff)) for _ in range(n)))
        add("lseq%d_odd_name" % n, 1, 300, qual=bytes(rng.randrange(256) for _ in range(n)), flag=0x10)
    for q in (14, 15, 0xfe, 0xff):
        add("q%d" % q, 1, 300, qual=bytes([q]) * 9)
    add("no_qual", 1, 300, qual=b"\xff" * 30)
    for fl in (0x4, 0x100, 0x800, 0x1, 0x1 | 0x8, 0x1 | 0x40, 0x1 | 0x80 | 0x10, 0x400, 0x200):
        add("flag%x" % fl, 0, 100, flag=fl)
    add("no_ref", -1, 100)
    add("neg_pos", 0, -1, [("S", 5), ("M", 5)])
    for label, aux in (("rg_a1", rg_aux(b"a1")), ("rg_a2", rg_aux(b"a2")), ("rg_b", rg_aux(b"b")), ("rg_solo", rg_aux(b"solo")), ("rg_a", rg_aux(b"a")), ("rg_unknown", rg_aux(b"a12")),
                       ("rg_empty", rg_aux(b"")), ("rg_type_A", b"RGAx"), ("rg_type_A_then_Z", b"RGAx" + rg_aux(b"b")), ("rg_behind_others", b"NMC\3XSs\1\0XBBS\2\0\0\0\1\0\2\0XZZtext\0" + rg_aux(b"b")),
                       ("rg_twice", rg_aux(b"b") + rg_aux(b"a1")), ("rg_noid", rg_aux(b"noid")), ("rg_comment", rg_aux(b"comment")), ("aux_broken_before_rg", b"XQ?\1" + rg_aux(b"b")),
                       ("aux_cut_short", b"NMi\1\0")):
        add(label, 0, 700, aux=aux)
    return out


def bulk(n=5000, seed=7, positions=40):
    """a seeded mix over a few positions: half of the records in pairs, fragments, orphans, ignored records, two libraries"""
    rng = random.Random(seed)
    out = []
    k = 0
    while len(out) < n:
        k += 1
        aux = rg_aux(rng.choice((b"a1", b"a2", b"b")))
        p1, p2 = 1000 + 10 * rng.randrange(positions), 3000 + 10 * rng.randrange(positions)
        q = bytes([rng.choice((20, 30, 40))]) * 50
        kind = rng.random()
        if kind < 0.5:
            out += pair("p%d" % k, rng.randrange(2), p1, p2, q, aux=aux)
        elif kind < 0.55:
            out.append(pair("o%d" % k, 0, p1, p2, q, aux=aux)[rng.randrange(2)])
        elif kind < 0.6:
            out.append(record("i%d" % k, 0, p1, qual=q, flag=rng.choice((0x4, 0x100, 0x800)), aux=aux))
        else:
            out.append(record("f%d" % k, rng.randrange(2), p1, qual=q, flag=rng.choice((0, 0x10, 0x400)), aux=aux))
    rng.shuffle(out)
    return out[:n]
