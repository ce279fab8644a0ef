"""The row exit of the extension's row loop (seqlib_amd/csrc/dev_lane_rows.h: ext_row_bound / ext_row_done, derived in dev_ext_wave.h) on the host, under
ASan + UBSan (tests/cpp/ext_row_exit_test.cpp): lane_rows_extend with the exit off, strict and relaxed against the checker's ksw_extend2, band trials as
mem_chain2aln runs them.  Strict: all six results and the band.  Relaxed: score, max_off, the band, the branch dev_extend_core / lane_extend_core take
(`gscore <= 0 || gscore <= score - pen_clip`) and the fields that branch reads.  Every case is compared under every rule."""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF, STRICT, RELAXED = 0, 1, 2
KINDS = {"junk": (0.0, 0.0), "third": (1 / 3, 0.10), "twothirds": (2 / 3, 0.10), "homol": (1.0, 0.02)}       # homologous share of the flank, its error rate
N_RANDOM = 500          # per kind


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ext_row_exit") / "ext_row_exit_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "ext_row_exit_test.cpp")])
    return out


def mutate(q, rate, rng):
    """q as the reference holds it: substitutions (80 %), a base the query lacks (10 %), a base of the query missing (10 %)"""
    t = []
    for b in q:
        if rng.random() < rate:
            x = rng.random()
            if x < 0.8:
                t.append((b + 1 + rng.randrange(3)) % 4)
            elif x < 0.9:
                t += [rng.randrange(4), b]
        else:
            t.append(b)
    return t


def flank(rng, qlen, kind, extra=None):
    share, rate = KINDS[kind]
    q = [rng.randrange(4) for _ in range(qlen)]
    k = int(round(qlen * share))
    t = mutate(q[:k], rate, rng) + [rng.randrange(4) for _ in range(qlen - k)]
    t += [rng.randrange(4) for _ in range(rng.randrange(8, 40) if extra is None else extra)]
    return q, t


def oracle_side(orc, q, t, w, end_bonus, h0, before, zdrop):
    L = orc.lib()
    mat = orc.default_opt().mat
    prev = before
    for i in range(2):
        aw = w << i
        o = [C.c_int() for _ in range(5)]
        sc = L.orc_ksw_extend2(len(q), bytes(q), len(t), bytes(t), 5, mat, 6, 1, 6, 1, aw, end_bonus, zdrop, h0, *[C.byref(x) for x in o])
        res = (sc, o[0].value, o[1].value, o[2].value, o[3].value, o[4].value, aw)
        if sc == prev or o[4].value < (aw >> 1) + (aw >> 2):
            break
        prev = sc
    return res


def expected(orc, case):
    exp, score = [], case["h0"]
    for s, (q, t) in enumerate(case["sides"]):
        if not q:
            continue
        r = oracle_side(orc, q, t, case["w"], case["pen3"] if s else case["pen5"], score, score if s else -1, case["zdrop"])
        exp.append((s,) + r)
        score = r[0]
    return exp


def make_cases():
    rng = random.Random(1019)
    cases = []

    def add(kind, sides, w=100, h0=None, zdrop=100, pen5=5, pen3=5):
        cases.append(dict(kind=kind, sides=sides, w=w, h0=h0 if h0 is not None else rng.randrange(19, 120), zdrop=zdrop, pen5=pen5, pen3=pen3))

    none = ([], [])
    for kind in KINDS:
        for n in range(N_RANDOM):
            qt = flank(rng, rng.randrange(5, 131), kind)
            if n % 5 == 4:          # both sides of a seed on one row
                add(kind, [flank(rng, rng.randrange(5, 131), kind), qt])
            else:
                add(kind, [qt, none] if n & 1 else [none, qt])
    # ---- crafted.  With the default scores the effective band is min(w, qlen): the band never clips a row up to qlen = w + 1
    for kind in KINDS:
        for qlen in (1, 63, 64, 65, 128, 130, 100, 101, 102):          # 101 = w + 1 (the band never clips), 102 = w + 2 (allowed only for a small h0: c_clip below)
            for h0 in (19, qlen + 5 - 1, qlen + 5 + 1, 131):            # below / above qlen + pen_clip
                for pen in (5, 0):
                    add("c_" + kind, [none, flank(rng, qlen, kind)], h0=h0, pen5=pen, pen3=pen)
                add("c_" + kind, [flank(rng, qlen, kind), none], h0=h0, zdrop=0)
                for extra in (0, 1, 3):                                 # tlen binds the min(): no, one, three rows beyond the query
                    add("c_" + kind, [none, flank(rng, qlen, kind, extra)], h0=h0)
        for w, qlen in ((20, 21), (20, 22), (4, 5), (4, 6), (4, 8), (4, 9), (4, 10), (1, 2), (1, 3)):   # qlen = w + 1, w + 2, and what the second band (2 w) allows
            for _ in range(6):
                add("c_band_" + kind, [none, flank(rng, qlen, kind)], w=w)
                add("c_band_" + kind, [flank(rng, qlen, kind), flank(rng, qlen, kind)], w=w)
    # queries longer than the band + 1: the exit is allowed where row -1's ramp is zero from column w + 2 on -- h0 <= oe_ins + (w + 1) e_ins = w + 8 -- and
    # barred above that, where the ramp re-enters the band (h0 on both sides of the edge; band 100, and bands 4 and 8 whose cells re-enter within a few rows)
    for kind in KINDS:
        for w, qlens in ((100, (102, 120, 130)), (4, (7, 12, 40)), (8, (11, 20, 40))):
            for qlen in qlens:
                for h0 in (w + 6, w + 7, w + 8, w + 9, w + 10, w + 30):
                    for pen in (5, 0):
                        add("c_clip", [none, flank(rng, qlen, kind)], w=w, h0=h0, pen3=pen)
                        add("c_clip", [flank(rng, qlen, kind), none], w=w, h0=h0, pen5=pen)
                    add("c_clip", [flank(rng, qlen, kind), flank(rng, qlen, kind)], w=w, h0=h0)
    # the second band trial: a gap wider than the first band, then a flank of each kind
    for kind in KINDS:
        for w in (4, 8):
            for gap in (w, w + 2):
                for qlen in (w + 1, 2 * w + 1, 2 * w + 2, 40):
                    for _ in range(4):
                        q, t = flank(rng, qlen, kind)
                        k = qlen // 2
                        add("c_band2", [none, (q, t[:k] + [rng.randrange(4) for _ in range(gap)] + t[k:])], w=w, h0=60)          # bases the query lacks
                        add("c_band2", [none, (q[:k] + [rng.randrange(4) for _ in range(gap)] + q[k:], t)], w=w, h0=60)          # bases the reference lacks
    # the query's end reached before, at and after the best row
    for qlen in (12, 40, 64, 101):
        for h0 in (19, 60):
            for pen in (5, 0):
                q = [rng.randrange(4) for _ in range(qlen)]
                junk = [rng.randrange(4) for _ in range(30)]
                bad = lambda v: [(b + 2) % 4 for b in v]
                add("c_end", [none, (q, q + junk)], h0=h0, pen3=pen)                                          # at: a perfect flank
                add("c_end", [none, (q, q[:-6] + bad(q[-6:]) + junk)], h0=h0, pen3=pen)                       # the best row lies before the query's end
                add("c_end", [none, (q, q[:-3] + bad(q[-3:-1]) + q[-1:] + junk)], h0=h0, pen3=pen)
                add("c_end", [none, (q + q[:8], q + junk[:3] + q[:8] + junk)], h0=h0, pen3=pen)               # the end first reached through the insertion ramp, better rows later
                add("c_end", [none, (q[:3] + bad(q[3:]), q + junk)], h0=max(h0, qlen + 12), pen3=pen)         # only h0 carries the path to the query's end
    # rows that match nothing, then the whole query: the best path enters from column -1 (the deletion ramp), where the bound must count the
    # ramp as the NEXT row reads it -- h0 - o_del - e_del * (i + 1) -- for the relaxed rule to hold exactly at equality
    for d in range(1, 9):
        for qlen in range(1, 13):
            for h0 in (19, 50):
                for pen in (5, 0):
                    add("c_ramp", [none, ([0] * qlen, [1] * d + [0] * qlen + [2] * 5)], h0=h0, pen3=pen)
                    add("c_ramp", [([0] * qlen, [1] * d + [0] * qlen), none], h0=h0, pen5=pen)
    # What the precondition (ext_row_exit_ok) is for: rows that match nothing, then a match that comes back into the band through columns a clipped
    # `end` never wrote -- row -1's insertion ramp, alive there when h0 > oe_ins + (w + 1) e_ins = w + 8 -- in a target that ends some twenty to
    # forty-five rows short of the query, so that the bound without those columns is already below max - pen_clip.  A homopolymer or periodic
    # query lets the match start at any column: the best path is the one through the ramp whenever there is one.  h0 on both sides of that edge,
    # qlen at w + 1 (the band never clips) and from w + 2 on, the target's end scanned; bands 1 .. 8 and 100.  With ext_row_exit_ok's body replaced
    # by `return true` this test fails on cases of this family (h0 = w + 45 and a query of 65, e.g. band 1 behind ten rows of junk: a score of 46
    # where the checker has 50) and on no other; test_guard_edges below holds the two edges themselves, which no result can see one step away (at h0 = w + 9 the ramp
    # is 1 in one column, and a path from it that beats max - pen_clip needs more rows than the bound leaves).
    junk = lambda n, k: [2 + (k + x * x) % 2 for x in range(n)]
    for w in (1, 2, 4, 8, 100):
        for qlen in ((w + 1, w + 2, 2 * w + 10, 65) if w < 100 else (101, 102, 250)):
            for h0 in (w + 7, w + 8, w + 9, w + 10, w + 20, w + 45):
                for d in (2, 10, 18):
                    for q in ([0] * qlen, ([0, 1] * qlen)[:qlen]):
                        for k in sorted(set(max(1, qlen - x) for x in (0, 3, 21, 24, 27, 30, 34, 39, 44))):
                            for pen in (0, 5):
                                add("c_guard", [none, (q, junk(d, h0) + q[:k])], w=w, h0=h0, pen3=pen)
                                if (d + k) % 4 == 0:
                                    add("c_guard", [(q, junk(d, h0) + q[:k]), none], w=w, h0=h0, pen5=pen)
    add("c_guard", [none, ([0] * 65, [3, 2, 3, 2, 3, 3, 3, 2, 3, 2, 3, 3, 2, 3, 2, 3, 3, 2] + [0] * 44)], w=8, h0=53, pen3=0)
    add("c_guard", [none, ([0] * 65, [3, 2, 3, 2, 3, 3, 3, 2, 3, 2, 3, 3, 2, 3, 2, 3, 3, 2] + [0] * 44)], w=8, h0=53, pen3=5)
    return cases


def branch(r, pen):          # (side, score, qle, tle, gtle, gscore, max_off, band): True = the local end (qle, tle), False = to the query's end (gtle, gscore)
    return r[5] <= 0 or r[5] <= r[1] - pen


def test_row_exit_against_the_checker(orc, exe, tmp_path):
    opt = orc.default_opt()
    assert (opt.o_del, opt.e_del, opt.o_ins, opt.e_ins, opt.a, opt.b) == (6, 1, 6, 1, 1, 4)
    cases = make_cases()
    dig = lambda v: "".join(map(str, v)) if v else "-"
    lines = []
    for c in cases:
        cols = max(len(q) for q, _ in c["sides"]) + 2
        lines.append("%s %d %d %d %d %d %d %s %s %s %s" % (c["kind"], cols, c["h0"], c["w"], c["zdrop"], c["pen5"], c["pen3"], dig(c["sides"][0][0]), dig(c["sides"][0][1]),
                                                            dig(c["sides"][1][0]), dig(c["sides"][1][1])))
    exp = [expected(orc, c) for c in cases]
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    tallies = {}
    for mode in (OFF, STRICT, RELAXED):
        p = subprocess.run([exe, "run", str(path), str(mode)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        got = [[] for _ in cases]
        tally = tallies[mode] = {}
        for ln in p.stdout.split("\n"):
            if ln.startswith("#"):
                f = ln.split()
                tally[f[1]] = dict(cases=int(f[2]), trials=int(f[3]), rows=int(f[4]), exits=int(f[5]))
            elif ln:
                v = tuple(int(x) for x in ln.split())
                got[v[0]].append(v[1:])
        assert sum(t["cases"] for t in tally.values()) == len(cases)          # every case ran: none is skipped
        for i, (g, e, c) in enumerate(zip(got, exp, cases)):
            what = "mode %d case %d (%s): (side, score, qle, tle, gtle, gscore, max_off, band) %r, the checker %r" % (mode, i, lines[i], g, e)
            if mode != RELAXED:
                assert g == e, what
                continue
            assert len(g) == len(e), what
            for rg, re_ in zip(g, e):
                pen = c["pen3"] if re_[0] else c["pen5"]
                assert (rg[0], rg[1], rg[6], rg[7]) == (re_[0], re_[1], re_[6], re_[7]), what          # side, score, max_off, band
                assert branch(rg, pen) == branch(re_, pen), what
                if branch(re_, pen):
                    assert rg[2:4] == re_[2:4], what          # qle, tle
                else:
                    assert rg[4:6] == re_[4:6], what          # gtle, gscore
        for kind in sorted(tally):
            t = tally[kind]
            print("mode %d %-18s %5d cases %6d trials %8d rows (%.1f per trial) %5d exits" % (mode, kind, t["cases"], t["trials"], t["rows"], t["rows"] / max(t["trials"], 1), t["exits"]))
    assert all(t["exits"] == 0 for t in tallies[OFF].values())
    for mode in (STRICT, RELAXED):
        assert tallies[mode]["junk"]["exits"] >= 1, mode
        assert tallies[mode]["third"]["exits"] >= 1 and tallies[mode]["twothirds"]["exits"] >= 1, mode
        assert sum(t["rows"] for t in tallies[mode].values()) < sum(t["rows"] for t in tallies[OFF].values())


def test_guard_edges(exe):
    """ext_row_exit_ok itself, at its edges: allowed iff the band never clips the row (qlen <= w + 1) or row -1's ramp is dead from column w + 2 on
    (h0 <= oe_ins + (w + 1) e_ins, with bwa's defaults w + 8) -- the two conditions dev_ext_wave.h proves; never with a negative gap penalty"""
    asked = [(qlen, w, h0, 0) for w in (1, 4, 8, 100) for qlen in (w, w + 1, w + 2, w + 3, 4 * w + 50) for h0 in (1, w + 7, w + 8, w + 9, w + 10, 5 * w + 60)]
    asked += [(5, 100, 19, 1), (200, 100, 19, 1)]
    p = subprocess.run([exe, "guard"], input="".join("%d %d %d %d\n" % a for a in asked), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = [int(x) for x in p.stdout.split()]
    assert got == [int(not neg and (qlen <= w + 1 or h0 <= w + 8)) for qlen, w, h0, neg in asked]
    assert 0 < sum(got) < len(got)

