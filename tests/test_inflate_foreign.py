"""dev_inflate.h against DEFLATE that zlib never writes.  Every compressed byte the decoder met before this file came out of one encoder (Python's zlib:
tests/test_bam_reader.corpus()); htslib's libdeflate, the Intel deflater and older tools emit other valid shapes.  tests/deflate_craft.py writes them bit by
bit: valid_set() (runs across the literal/length | distance boundary, a single one-bit distance code, codes of 15 bits, every length and distance symbol,
hundreds of tiny blocks ...) and refused_set() (what zlib refuses or leaves unfinished).  zlib.decompressobj(-15) alone decides which set a stream is in.

No test here needs a GPU, and the refused set never goes to one: a hostile stream meets the host sanitizers first.  The host build runs as one lane
(tests/cpp/inflate_host_test.cpp, ASan + UBSan) and as 7 and 64 lanes, a thread each with INF_SYNC() a real barrier (tests/cpp/inflate_lanes_test.cpp,
once under ASan + UBSan and once under ThreadSanitizer: the check that ties every INF_SYNC() to the accesses it orders).  The GPU takes the valid set in
tests/test_gpu_inflate_foreign.py."""
import functools
import os
import random
import re
import struct
import subprocess
import zlib

from tests import bam_util as bu
from tests import deflate_craft as dc
from tests.test_bam_reader import corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = {k: int(v) for k, v in re.findall(r"\b(INF_E?_?[A-Z]+) = (\d+)", open(os.path.join(ROOT, "seqlib_amd", "csrc", "dev_inflate.h")).read())}
ANY = 0          # a refused entry that the header names no single code for: any non-zero return


def rand(n, seed):
    rng = random.Random(seed)
    return bytes(rng.randrange(256) for _ in range(n))


def lens_of(n, pairs):
    out = [0] * n
    for s, l in pairs.items():
        out[s] = l
    return out


def member_with_extra(comp, payload, before=b"", after=b""):
    """a BGZF member whose gzip extra field carries other subfields around BC"""
    sub = lambda ident, data: ident + struct.pack("<H", len(data)) + data
    xlen = len(before) + 6 + len(after)
    total = 12 + xlen + len(comp) + 8
    assert total <= 0x10000
    extra = before + sub(b"BC", struct.pack("<H", total - 1)) + after
    return (bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff]) + struct.pack("<H", xlen) + extra + comp + struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload)))


# ---------------------------------------------------------------- the valid set
LL_A = {65: 1, 66: 2}                                   # the two literals of the section-a members
LONG_LL = dict([(97 + i, i + 1) for i in range(9)] + [(257, 10), (258, 11), (106, 12), (107, 13), (108, 14), (109, 15), (256, 15)])     # lengths 1, 2, ... 14, 15, 15
LONG_D = [i + 1 for i in range(14)] + [15, 15]


def filler(s, upto, seed):
    """a stored block of 1 KiB, then a fixed block of long matches at changing distances: s.out grows to exactly `upto` bytes"""
    s.stored(rand(1024, seed))
    toks, n, k = [], 1024, 0
    while n < upto:
        ln = min(258, upto - n)
        if 0 < upto - n - ln < 3:
            ln -= 3
        toks.append(dc.match(300 + (k * 37) % 700, ln))
        n += ln
        k += 1
    return s.fixed(toks)


def many_blocks_deflate(data, back, rng):
    """`data` as one deflate stream in the block style of item g: an empty stored block, a stored block of a few bytes, an empty fixed block and a fixed block
    in turn, closed by an empty stored block.  No match finder: back[i] is the one distance tried at byte i (0: none) -- the caller's knowledge of where the
    record before put the same field"""
    s, i, k, n = dc.Stream(), 0, 0, len(data)
    while i < n:
        kind, k = k % 4, k + 1
        if kind == 0:
            s.stored(b"")
        elif kind == 1:
            m = min(n - i, rng.randrange(1, 30))
            s.stored(data[i:i + m])
            i += m
        elif kind == 2:
            s.fixed([])
        else:
            toks, budget = [], rng.randrange(1, 120)
            while i < n and len(toks) < budget:
                d, ln = back[i], 0
                if 0 < d <= i:
                    while ln < 258 and i + ln < n and data[i + ln] == data[i + ln - d]:
                        ln += 1
                if ln >= 3:
                    toks.append(dc.match(d, ln))
                    i += ln
                else:
                    toks.append(data[i])
                    i += 1
            s.fixed(toks)
    s.stored(b"", True)
    assert bytes(s.out) == data
    return s.getvalue()


def many_blocks_bgzf(data, starts, member_size, seed):
    """a BGZF file of `data` cut every member_size bytes, every member by many_blocks_deflate; starts: the offsets at which the records of data begin -- a byte is
    tried against the byte as far into the record before"""
    back, rng = [0] * len(data), random.Random(seed)
    for a, b, c in zip(starts, starts[1:], starts[2:] + [len(data)]):
        back[b:c] = [b - a] * (c - b)
    out = b""
    for o in range(0, len(data), member_size):
        piece = data[o:o + member_size]
        out += bu.member_from_deflate(many_blocks_deflate(piece, back[o:o + member_size], rng), piece)
    return out + bu.EOF_BLOCK


@functools.lru_cache(maxsize=None)
def valid_set():
    """[dict(name, comp, payload[, member])]: crafted here, admitted by zlib alone (test_crafted_members_are_zlib_valid_and_carry_their_feature)"""
    out = []

    def add(name, s, member=None, tail=b""):
        s = s if isinstance(s, bytes) else s.getvalue()
        out.append(dict(name=name, comp=s + tail, payload=bytes(add.payload), member=member))

    def done(name, s, **kw):
        add.payload = s.out
        add(name, s, **kw)

    # a. runs across, up to and from the boundary between the literal/length and the distance lengths
    ll = lens_of(260, {**LL_A, 256: 4, 257: 4, 258: 4, 259: 4})
    toks_a = [65, 66, 65, 65, 66, 66, 65, (257, 0, 0, 0), (258, 0, 3, 0), 66, (259, 0, 5, 1), (257, 0, 4, 1)]
    done("a_run16_across", dc.Stream().dynamic(ll, [4] * 16, toks_a + [(259, 0, 7, 3), 65], True, spelling=dc.rle(ll + [4] * 16)))
    ll17 = lens_of(262, {**LL_A, 256: 3, 257: 4, 258: 4})
    done("a_run17_across", dc.Stream().dynamic(ll17, [0, 0, 1, 1], [65, 66, 65, 65, (257, 0, 2, 0), 66, (258, 0, 3, 0)], True, spelling=dc.rle(ll17 + [0, 0, 1, 1])))
    ll18 = lens_of(280, {**LL_A, 256: 3, 257: 3})
    done("a_run18_across", dc.Stream().dynamic(ll18, [0, 0, 0, 0, 1, 1], [65, 66, 66, 65, 65, 66, (257, 0, 4, 0), 65, (257, 0, 5, 1)], True, spelling=dc.rle(ll18 + [0, 0, 0, 0, 1, 1])))
    done("a_run17_ends_at_boundary", dc.Stream().dynamic(ll17, [1, 1], [65, 66, 65, (257, 0, 0, 0), (258, 0, 1, 0)], True, spelling=dc.rle(ll17 + [1, 1], breaks=[262])))
    ll_s = lens_of(259, {**LL_A, 256: 3, 257: 4, 258: 4})
    done("a_run17_starts_at_boundary", dc.Stream().dynamic(ll_s, [0, 0, 0, 1, 1], [66, 65, 65, 66, (257, 0, 3, 0), (258, 0, 4, 0)], True, spelling=dc.rle(ll_s + [0, 0, 0, 1, 1], breaks=[259])))
    # a 16 on the boundary itself: the distance lengths begin by repeating the last literal/length length
    done("a_run16_starts_at_boundary", dc.Stream().dynamic(ll, [4] * 16, toks_a, True, spelling=dc.rle(ll) + [(16, 3), (16, 3), (16, 1)]))

    # b. distance codes zlib never sends
    done("b_one_bit_distance_code", dc.Stream().dynamic(lens_of(285, {65: 1, 256: 2, 257: 3, 284: 3}), [1], [65, (257, 0, 0, 0), dc.match(1, 258, alt258=True), 65], True))
    done("b_no_distance_code", dc.Stream().dynamic(dc.complete_lengths({97, 98, 99, 100, 256}, 257), [0], [97, 98, 99, 100, 100, 99, 97], True))
    done("b_empty_dynamic", dc.Stream().dynamic(lens_of(257, {256: 1}), [0], [], True))

    # c. long codes, and codes on either side of the first-level tables
    ll = lens_of(259, LONG_LL)
    toks = [97] * 200 + list(range(98, 110)) + [(257, 0, ds, 0) for ds in range(16)] + [(258, 0, ds, (1 << dc.DEXT[ds]) - 1) for ds in range(16)] + [109, 108]
    done("c_codes_of_1_to_15_bits", dc.Stream().dynamic(ll, LONG_D, toks, True))
    ll = lens_of(258, dict([(0, 1), (1, 2), (2, 3)] + [(s, 10) for s in range(3, 103)] + [(s, 11) for s in list(range(200, 254)) + [256, 257]]))
    d = [1, 2, 3, 4, 5] + [8] * 6 + [9] * 4
    toks = [0, 1, 2] + list(range(3, 103)) + list(range(200, 254)) + [(257, 0, ds, 0) for ds in range(15)] + [7, (257, 0, 14, 20), 250]
    done("c_many_codes_of_10_and_11_bits", dc.Stream().dynamic(ll, d, toks, True))

    # d. code-length codes
    syms = list(range(32, 64)) + list(range(65, 127)) + [256, 257]
    ll = lens_of(258, dict(zip(syms, [5] * 16 + [6] * 16 + [7] * 16 + [8] * 16 + [9] * 32)))
    cl = lens_of(19, {0: 1, 8: 2, 7: 3, 9: 4, 6: 5, 18: 6, 1: 7, 5: 7})
    done("d_code_length_codes_of_7_bits", dc.Stream().dynamic(ll, [1], list(b"Seven bits, 1 to 6 and 7, 7") + [(257, 0, 0, 0)], True, cl_lens=cl, spelling=dc.rle(ll + [1], use16=False)))
    ll = [0] + [8] * 256 + [0] * 29
    done("d_fewest_code_length_codes", dc.Stream().dynamic(ll, [0], list(b"five of nineteen") + [255, 1, 128], True, cl_lens=lens_of(19, {8: 1, 0: 2, 18: 2}), spelling=dc.rle(ll + [0], use16=False)))
    ll = lens_of(261, LONG_LL)
    s = dc.Stream().dynamic(ll, [2, 2, 2, 2], [97] * 9 + list(range(98, 110)) + [(257, 0, 3, 0), (258, 0, 1, 0)], True, cl_lens=dc.complete_lengths(range(19), 19), spelling=dc.rle(ll + [2, 2, 2, 2]), hclen=19)
    done("d_all_19_code_length_codes", s)

    # e. table limits: every length symbol and every distance symbol, extra bits all 0 and all 1
    ll = lens_of(286, dict([(s, 5) for s in range(256, 286)] + [(65, 5), (66, 5)]))
    d = [4, 4] + [5] * 28
    s = filler(dc.Stream(), 32768 + 700, 21)
    done("e_every_symbol_extra_bits_0", s.dynamic(ll, d, [65, 66] + [(257 + k % 29, 0, k, 0) for k in range(30)] + [66], True))
    s = filler(dc.Stream(), 32768, 22)
    toks = [(285, 0, 29, 8191)] + [t for k in range(30) for t in (65 + k % 2, (257 + k % 29, (1 << dc.LEXT[k % 29]) - 1, k, (1 << dc.DEXT[k]) - 1))]
    done("e_every_symbol_extra_bits_1", s.dynamic(ll, d, toks, True))

    # f. overlapping copies at the lane-count edges
    rng = random.Random(31)
    s = dc.Stream().stored(rand(128, 30))
    toks = []
    for dist in range(1, 71):
        for ln in sorted({3, dist - 1, dist, dist + 1, 63, 64, 65, 258}):
            if ln >= 3:
                toks += [rng.randrange(256), rng.randrange(256), dc.match(dist, ln)]
    done("f_overlapping_copies", s.fixed(toks, True))

    # g. about 300 tiny blocks of all kinds
    rng = random.Random(41)
    s = dc.Stream().stored(rand(40, 40))
    for r in range(60):
        s.stored(b"")                                                                       # behind the dynamic block of the round before: any bit offset
        s.stored(bytes([rng.randrange(256)]))
        s.fixed([])
        n = r % 8 + 1
        s.fixed([rng.randrange(256) for _ in range(n)] + [dc.match(n + 1, 3 + r % 5)] + ([dc.match(len(s.out) + n + 3 + r % 5, 4)] if r % 7 == 0 else []))   # back into the stored byte
        a, b = rng.sample(range(256), 2)
        s.dynamic(lens_of(258, {a: 1, b: 2, 256: 3, 257: 3}), [1, 1], [a] * (r % 8 + 1) + [b, (257, 0, 1, 0)])
    done("g_many_blocks", s.stored(b"", True))

    # h. ISIZE at the format's limit, and unused bytes behind the final block
    s = dc.Stream().stored(rand(256, 50))
    n, k, toks = 256, 0, []
    while n < 0x10000:
        ln = min(258, 0x10000 - n)
        if 0 < 0x10000 - n - ln < 3:
            ln -= 3
        toks.append(dc.match(1 + (k * 29) % 255, ln))
        n += ln
        k += 1
    done("h_isize_0x10000", s.fixed(toks, True))
    small = out[6]
    add.payload = small["payload"]
    add("h_1_unused_byte", small["comp"], tail=b"\xff")
    add("h_9_unused_bytes", small["comp"], tail=b"\x00\xff\x1f\x8b\x08\x04\x00\x01\xff")

    # i. other subfields in the gzip extra field (the members carry their own headers)
    c0, p0 = out[0]["comp"], out[0]["payload"]
    add.payload = p0
    add("i_subfield_before_BC", c0, member=member_with_extra(c0, p0, before=b"RA\x03\x00abc"))
    add("i_subfield_behind_BC", c0, member=member_with_extra(c0, p0, after=b"XY\x00\x00"))
    add("i_subfields_around_BC", c0, member=member_with_extra(c0, p0, before=b"BC\x03\x00xyz" + b"Q1\x01\x00\x00", after=b"ZZ\x05\x00" + b"BCBC\x02"))
    return out


def member_of(e):
    return e["member"] or bu.member_from_deflate(e["comp"], e["payload"])


# ---------------------------------------------------------------- the refused set
def prefix_streams():
    """two short valid streams whose every proper prefix is refused: [(name, Stream)]"""
    ll = lens_of(259, {**LL_A, 256: 3, 257: 4, 258: 4})
    toks = [65, 66, 65, 65, 66, (257, 0, 0, 0), 66, 65, (258, 0, 2, 0), 66, (257, 0, 1, 0), 65, 65, 66]
    dyn = dc.Stream().dynamic(ll, [1, 2, 2], toks + [66, 66] + toks[5:] * 3, True, spelling=dc.rle(ll + [1, 2, 2]))
    fs = dc.Stream().fixed(list(b"a fixed block, and then") + [dc.match(7, 5), 200, 255, dc.match(1, 9)] + list(b" one that is ")).stored(b"stored", True)
    return [("dynamic", dyn), ("fixed_stored", fs)]


@functools.lru_cache(maxsize=None)
def refused_set():
    """[(name, comp, isize, code)]: streams zlib refuses or does not end; code is the one INF_E_* the header names for the case, or ANY"""
    E = CODES
    out = []
    ok_ll = lens_of(258, {65: 1, 256: 2, 257: 2})
    body = [65, 65, (257, 0, 0, 0)]

    def dyn(name, code, ll=ok_ll, d=(1,), toks=body, isize=16, **kw):
        out.append((name, dc.Stream().dynamic(list(ll), list(d), toks, True, **kw).getvalue(), isize, code))

    plain = [(l, 0) for l in ok_ll + [1]]
    dyn("oversubscribed_code_length_code", E["INF_E_CODE"], cl_lens=lens_of(19, {0: 1, 1: 1, 2: 1}))
    dyn("oversubscribed_literal_code", E["INF_E_CODE"], ll=lens_of(258, {65: 1, 256: 1, 257: 1}))
    dyn("oversubscribed_distance_code", E["INF_E_CODE"], d=(1, 1, 1))
    dyn("incomplete_literal_code", E["INF_E_CODE"], ll=lens_of(258, {65: 2, 256: 2, 257: 2}))
    dyn("incomplete_distance_code", E["INF_E_CODE"], d=(2, 2))
    dyn("incomplete_code_length_code", E["INF_E_CODE"], cl_lens=lens_of(19, {0: 2, 1: 2, 2: 2}))
    dyn("single_code_length_code", ANY, ll=[8] * 257, d=(8,), toks=[65], cl_lens=lens_of(19, {8: 1}))
    dyn("repeat_at_index_0", E["INF_E_CODE"], spelling=[(16, 0)] + plain[3:], cl_lens=dc.complete_lengths({0, 1, 2, 16}, 19))
    dyn("run_past_the_code_lengths", E["INF_E_CODE"], spelling=plain[:250] + [(18, 0)], cl_lens=dc.complete_lengths({0, 1, 2, 18}, 19))
    dyn("no_end_of_block_code", E["INF_E_CODE"], ll=lens_of(258, {65: 1, 66: 2, 257: 2}), toks=[65, 66], eob=False)
    for h in (30, 31):
        dyn("hlit_%d" % h, E["INF_E_CODE"], hlit=h)
        dyn("hdist_%d" % h, E["INF_E_CODE"], hdist=h)
    dyn("distance_with_no_distance_code", E["INF_E_CODE"], d=(0,), toks=[65, 65, (257, 0, None, 0), ("bits", 0, 8)])
    dyn("pattern_outside_the_one_bit_distance_code", E["INF_E_CODE"], toks=[65, 65, (257, 0, None, 0), ("bits", 1, 1)])
    for ds in (30, 31):
        out.append(("fixed_distance_symbol_%d" % ds, dc.Stream().fixed([65] * 40 + [(257, 0, ds, 0), ("bits", 0, 16)], True).getvalue(), 64, E["INF_E_SYM"]))
    for ls in (286, 287):
        out.append(("fixed_length_symbol_%d" % ls, dc.Stream().fixed([65] * 4 + [("sym", ls), ("bits", 0, 16)], True).getvalue(), 64, E["INF_E_SYM"]))
    out.append(("distance_past_the_start_at_0", dc.Stream().fixed([(257, 0, 0, 0)], True).getvalue(), 16, E["INF_E_DIST"]))
    out.append(("distance_past_the_start_in_mid_member", dc.Stream().stored(rand(60, 3)).fixed([65] * 40 + [dc.match(101, 4)], True).getvalue(), 200, E["INF_E_DIST"]))
    out.append(("literal_past_isize", dc.Stream().fixed([65] * 5, True).getvalue(), 4, E["INF_E_OUT"]))
    out.append(("match_past_isize", dc.Stream().fixed([65, dc.match(1, 10)], True).getvalue(), 10, E["INF_E_OUT"]))
    out.append(("stored_past_isize", dc.Stream().stored(b"12345", True).getvalue(), 4, E["INF_E_OUT"]))
    out.append(("stored_len_nlen", dc.Stream().stored(b"AAAAA", True, nlen=0).getvalue(), 5, E["INF_E_STORED"]))
    out.append(("stored_past_the_input", dc.Stream().stored(b"A" * 50, True, body=b"A" * 10).getvalue(), 50, E["INF_E_STORED"]))
    w = dc.BitWriter()
    w.bits(1, 1), w.bits(3, 2), w.bits(0, 13)
    out.append(("block_type_3", w.getvalue(), 10, E["INF_E_BTYPE"]))
    for name, s in prefix_streams():
        comp = s.getvalue()
        stored_from = None
        if name == "fixed_stored":
            stored_from = len(comp) - 6
        for k in range(len(comp)):
            code = ANY
            if 8 * k in s.marks:
                code = E["INF_E_EOF"]                    # ends between two symbols: the next one is read off bits that are not there
            if stored_from is not None and k >= stored_from:
                code = E["INF_E_STORED"]                 # LEN and NLEN are in, the bytes are not
            out.append(("prefix_%s_%d" % (name, k), comp[:k], len(s.out), code))
    return out


def write_valid(path):
    with open(path, "wb") as f:
        for e in valid_set():
            f.write(struct.pack("<II", len(e["comp"]), len(e["payload"])) + e["comp"])


def write_refused(path):
    """{u32 size, u32 ISIZE, u32 expected code (0: any non-zero), bytes}"""
    with open(path, "wb") as f:
        for _, comp, isize, code in refused_set():
            f.write(struct.pack("<III", len(comp), isize, code) + comp)


# ---------------------------------------------------------------- tests
def summary(c):
    return ("blocks s/f/d %s  max code ll %d d %d cl %d  runs across %s to %s from %s  dist codes %s  len syms %d dist syms %d  dist %s..%s len %s..%s  overlaps %d  "
            "HLIT %s HDIST %s HCLEN %s  trailing %d" % (c["blocks"], c["max_ll_len"], c["max_d_len"], c["max_cl_len"], sorted(c["runs_across"]), sorted(c["runs_end_at_boundary"]),
                                                       sorted(c["runs_start_at_boundary"]), sorted(c["n_dist_codes"]), len(c["lsyms"]), len(c["dsyms"]), c["min_dist"], c["max_dist"], c["min_len"],
                                                       c["max_len"], len(c["overlaps"]), sorted(c["hlit"]), sorted(c["hdist"]), sorted(c["hclen"]), c["trailing"]))


def behind(c, p0):
    """the matches (dist, len, length symbol, extra, distance symbol, extra) at output positions from p0 on"""
    return [v for p, v in c["match_at"].items() if p >= p0]


def lengths_of(decoded):
    return {l for _, l in decoded}


FEATURES = {
    "a_run16_across": lambda c: 16 in c["runs_across"],
    "a_run17_across": lambda c: 17 in c["runs_across"],
    "a_run18_across": lambda c: 18 in c["runs_across"],
    "a_run17_ends_at_boundary": lambda c: 17 in c["runs_end_at_boundary"] and not c["runs_across"],
    "a_run17_starts_at_boundary": lambda c: 17 in c["runs_start_at_boundary"] and not c["runs_across"],
    "a_run16_starts_at_boundary": lambda c: 16 in c["runs_start_at_boundary"] and 16 in c["runs_end_at_boundary"] and not c["runs_across"],
    "b_one_bit_distance_code": lambda c: c["n_dist_codes"] == {1} and c["d_decoded"] == {(0, 1)} and c["hdist"] == {0} and c["match_at"][4] == (1, 258, 284, 31, 0, 0),
    "b_no_distance_code": lambda c: c["n_dist_codes"] == {0} and c["hdist"] == {0} and not c["lsyms"] and c["hlit"] == {0},
    "b_empty_dynamic": lambda c: c["ll_code_sizes"] == {1} and c["ll_decoded"] == {(256, 1)} and c["n_dist_codes"] == {0},
    "c_codes_of_1_to_15_bits": lambda c: (c["ll_decoded"] == set(LONG_LL.items()) and c["d_decoded"] == set(enumerate(LONG_D)) and lengths_of(c["ll_decoded"]) == set(range(1, 16))
                                          and lengths_of(c["d_decoded"]) == set(range(1, 16))),
    "c_many_codes_of_10_and_11_bits": lambda c: (sum(1 for _, l in c["ll_decoded"] if l == 10) == 100 and sum(1 for _, l in c["ll_decoded"] if l == 11) == 56
                                                 and sum(1 for _, l in c["d_decoded"] if l == 8) == 6 and sum(1 for _, l in c["d_decoded"] if l == 9) == 4),
    "d_code_length_codes_of_7_bits": lambda c: sorted(l for _, l in c["cl_decoded"]) == [1, 2, 3, 4, 5, 6, 7, 7] and c["max_cl_len"] == 7,
    "d_fewest_code_length_codes": lambda c: c["hclen"] == {1} and c["hlit"] == {29} and 18 in c["runs_across"],
    "d_all_19_code_length_codes": lambda c: c["hclen"] == {15} and {s for s, _ in c["cl_decoded"]} == set(range(19)),
    "e_every_symbol_extra_bits_0": lambda c: (c["hlit"] == {29} and c["hdist"] == {29} and {v[2:4] for v in behind(c, 32768 + 700)} == {(s, 0) for s in range(257, 286)}
                                              and {v[4:] for v in behind(c, 32768 + 700)} == {(s, 0) for s in range(30)}),
    "e_every_symbol_extra_bits_1": lambda c: (c["hlit"] == {29} and c["hdist"] == {29} and {v[2:4] for v in behind(c, 32768)} == {(s, (1 << dc.LEXT[s - 257]) - 1) for s in range(257, 286)}
                                              and {v[4:] for v in behind(c, 32768)} == {(s, (1 << dc.DEXT[s]) - 1) for s in range(30)}
                                              and c["match_at"][32768] == (32768, 258, 285, 0, 29, 8191) and (258, 284, 31) in {v[1:4] for v in behind(c, 32768)} and c["max_dist"] == 32768),
    "f_overlapping_copies": lambda c: {(d, l) for d in range(1, 71) for l in (3, d - 1, d, d + 1, 63, 64, 65, 258) if l >= 3} <= {(v[0], v[1]) for v in c["match_at"].values()},
    "g_many_blocks": lambda c: (sum(c["blocks"]) >= 300 and min(c["blocks"]) >= 60 and c["stored_after_bit"] == set(range(8)) and c["back_into_stored"] >= 60 and c["final_block"] == 0
                                and c["stored_sizes"] >= {0, 1}),
    "h_isize_0x10000": lambda c: True,
    "h_1_unused_byte": lambda c: c["trailing"] == 1,
    "h_9_unused_bytes": lambda c: c["trailing"] == 9,
}


def test_crafted_members_are_zlib_valid_and_carry_their_feature(capsys):
    """every member of the valid set: zlib ends it with the intended payload, and the census finds in it the shape it is named for"""
    names = [e["name"] for e in valid_set()]
    assert len(set(names)) == len(names) and set(FEATURES) <= set(names)
    with capsys.disabled():
        print()
        for e in valid_set():
            ok, got, unused = dc.accepted(e["comp"], len(e["payload"]))
            assert ok and got == e["payload"], e["name"]
            mine, c = dc.census(e["comp"])
            assert mine == e["payload"] and len(unused) == c["trailing"], e["name"]
            print("%-32s %6d -> %6d  %s" % (e["name"], len(e["comp"]), len(e["payload"]), summary(c)))
            if e["member"] is None:
                assert FEATURES[e["name"]](c), (e["name"], summary(c))
                assert 18 + len(e["comp"]) + 8 <= 0x10000
            else:
                m = e["member"]
                assert zlib.decompress(m, 31) == e["payload"] and struct.unpack_from("<H", m, 10)[0] > 6 and len(m) <= 0x10000
                (off, doff, dlen, isize, crc), = bu.scan_members(m)[0]
                assert (off, doff + dlen + 8, isize, crc) == (0, len(m), len(e["payload"]), zlib.crc32(e["payload"]) & 0xffffffff) and m[doff:doff + dlen] == e["comp"]
    by = {e["name"]: e for e in valid_set()}
    assert len(by["h_isize_0x10000"]["payload"]) == 0x10000 and len(by["b_empty_dynamic"]["payload"]) == 0
    assert by["i_subfield_before_BC"]["member"][12:14] != b"BC" and by["i_subfield_behind_BC"]["member"][12:14] == b"BC"


def test_census_of_the_zlib_corpus_is_printed(capsys):
    """what the one encoder the decoder had met so far writes, for comparison with the above: printed, nothing asserted about it (the system's zlib may differ)"""
    total = dc.new_census()
    for name, comp, payload in corpus():
        if name.endswith("/random") and not name.startswith(("dyn6", "fixed/")):
            continue                                     # 64 KiB of literals each: two of them say what nine would
        got, _ = dc.census(comp, total)
        assert got == payload, name
    with capsys.disabled():
        print("\nzlib corpus: " + summary(total))


def test_refused_set_is_refused_by_zlib():
    names = [r[0] for r in refused_set()]
    assert len(set(names)) == len(names) and sum(1 for n in names if n.startswith("prefix_")) > 60
    for name, comp, isize, code in refused_set():
        assert not dc.accepted(comp, isize)[0], name
        assert code in (ANY, CODES["INF_E_EOF"], CODES["INF_E_BTYPE"], CODES["INF_E_STORED"], CODES["INF_E_CODE"], CODES["INF_E_SYM"], CODES["INF_E_DIST"], CODES["INF_E_OUT"])
    for name, s in prefix_streams():                     # the whole streams are valid
        assert dc.accepted(s.getvalue(), len(s.out)) == (True, bytes(s.out), b""), name
    assert sum(1 for r in refused_set() if r[0].startswith("prefix_") and r[3] == CODES["INF_E_EOF"]) >= 4


def build(tmp_path, src, san, extra=()):
    exe = str(tmp_path / (os.path.splitext(src)[0] + "_" + san.replace(",", "_")))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=" + san, "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", src), "-lz"] + list(extra))
    return exe


def test_one_lane_under_asan_and_ubsan(tmp_path):
    """tests/cpp/inflate_host_test.cpp over the crafted sets: bytes equal to zlib's, the sliced CRC32, ISIZE +- 1 and 80 damaged variants of every valid member end
    cleanly; every refused stream gets zlib's verdict, and the code the header names for it"""
    write_valid(tmp_path / "valid.bin")
    write_refused(tmp_path / "refused.bin")
    exe = build(tmp_path, "inflate_host_test.cpp", "address,undefined")
    r = subprocess.run([exe, str(tmp_path / "valid.bin"), "80", str(tmp_path / "refused.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    last = lines[-1].split()
    n_valid = len(valid_set())
    assert int(last[0]) == n_valid and int(last[2]) == 80 * sum(1 for e in valid_set() if e["comp"]) and int(last[4]) == 0, r.stdout[-2000:]
    assert lines[-2].split() == [str(len(refused_set())), "refused", "0", "bad"], r.stdout[-2000:]


def run_lanes(tmp_path, san):
    write_valid(tmp_path / "valid.bin")
    write_refused(tmp_path / "refused.bin")
    exe = build(tmp_path, "inflate_lanes_test.cpp", san)
    r = subprocess.run([exe, str(tmp_path / "valid.bin"), str(tmp_path / "refused.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-3000:] + r.stderr[-6000:]
    want = ["%d lanes %d valid %d refused 0 bad" % (n, len(valid_set()), len(refused_set())) for n in (7, 64)]
    assert r.stdout.strip().splitlines()[-2:] == want, r.stdout[-2000:]


def test_lanes_on_threads_under_asan_and_ubsan(tmp_path):
    """inf_member as 7 and as 64 lanes, a thread each, one shared inf_tables and one shared output, INF_SYNC() a barrier: the valid set gives zlib's bytes, the
    refused set the same code in every lane -- and every thread returns (a lane that left a barrier early would hang the group: the program's watchdog)"""
    run_lanes(tmp_path, "address,undefined")


def test_lanes_on_threads_under_tsan(tmp_path):
    """the same under ThreadSanitizer: a report is a failure.  With the barrier as the only ordering between the lanes, an access that no INF_SYNC() orders
    against another lane's write is a data race by the letter -- on the GPU the same slip passes by luck, a wave running in step"""
    run_lanes(tmp_path, "thread")
