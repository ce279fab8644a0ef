"""The narrow band of the extension's row loop (seqlib_amd/csrc/dev_lane_rows.h: ext_narrow_band, LaneSide::wband, LaneRing; derived in dev_ext_wave.h,
"the narrow band") on the host, under ASan + UBSan (tests/cpp/ext_narrow_band_test.cpp).  A flank whose main diagonal loses L against a perfect match
and starts above L needs no band beyond floor((L - o) / e): lane_rows_extend clamped to it reports what the unclamped run and the checker's ksw_extend2
report -- all six results and the band with the row exit off and strict; with the relaxed exit what that rule keeps (the two runs may end at different
rows, and gscore / gtle are then free in the branch that does not read them).  The ring layout runs on a heap block of exactly 32 columns per lane."""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF, STRICT, RELAXED = 0, 1, 2
NONE, CLAMP, RING, ONE_LESS = 0, 1, 2, 3
OE, CAP = 7, 14          # bwa's default o + e; EXT_NARROW_CAP
N_RANDOM = 400           # per kind
GOLDEN = os.path.join(ROOT, "tests", "golden", "ext_narrow_tight.txt")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ext_narrow") / "ext_narrow_band_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "ext_narrow_band_test.cpp")])
    return out


def base_seq(rng, n, kind):
    if kind == "random":
        return [rng.randrange(4) for _ in range(n)]
    unit = [rng.randrange(4) for _ in range(rng.randrange(1, 7))]          # period 1 .. 6
    q = (unit * (n // len(unit) + 1))[:n]
    if kind == "noisy":
        for _ in range(max(1, n // 12)):
            q[rng.randrange(n)] = rng.randrange(4)
    return q


def subst(rng, q, at):
    t = list(q)
    for p in at:
        t[p] = (t[p] + 1 + rng.randrange(3)) % 4
    return t


def loss_of(q, t):
    """what the main diagonal loses: 5 per mismatch, 2 per N (a = 1, b = 4, N scores -1)"""
    return sum(0 if (a == b and a < 4) else (2 if a == 4 or b == 4 else 5) for a, b in zip(q, t))


def flank(rng, kind, qlen=None, n_sub=None, extra=None, with_n=False):
    qlen = qlen if qlen is not None else rng.randrange(2, 131)
    q = base_seq(rng, qlen, kind)
    k = min(qlen, n_sub if n_sub is not None else rng.randrange(2, 26))
    t = subst(rng, q, rng.sample(range(qlen), k))
    if with_n:
        (q if rng.random() < 0.5 else t)[rng.randrange(qlen)] = 4
    tail = base_seq(rng, 40, kind) if kind != "random" and rng.random() < 0.5 else [rng.randrange(4) for _ in range(40)]
    t += tail[:rng.randrange(0, 41) if extra is None else extra]
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


none = ([], [])


def make_cases():
    """every case carries `elig`: per side None (no such side / not asserted), True or False"""
    rng = random.Random(2061)
    cases = []

    def add(kind, sides, w=100, h0=None, zdrop=100, pen5=5, pen3=5, elig=(None, None)):
        if h0 is None:          # from L + 1 upwards (L = the larger loss of the job's sides)
            h0 = max(loss_of(q, t) for q, t in sides if q) + 1 + (0 if rng.random() < 0.2 else rng.randrange(0, 100))
        cases.append(dict(kind=kind, sides=sides, w=w, h0=h0, zdrop=zdrop, pen5=pen5, pen3=pen3, elig=elig))

    for kind in ("random", "periodic", "noisy"):
        for n in range(N_RANDOM):
            qt = flank(rng, kind, with_n=n % 8 == 7, n_sub=rng.randrange(2, 5) if n % 2 else None)
            if n % 5 == 4:
                add(kind, [flank(rng, kind, n_sub=rng.randrange(2, 5)), qt])
            else:
                add(kind, [qt, none] if n & 1 else [none, qt])
    # ---- crafted (a mismatch loses 5, an N loses 2: L = 5 m + 2 n)
    def exact(qlen, m, n, kind="random", first=False, last=False, extra=20):
        q = base_seq(rng, qlen, kind)
        pos = set()
        if first:
            pos.add(0)
        if last:
            pos.add(qlen - 1)
        while len(pos) < m + n:
            pos.add(rng.randrange(qlen))
        pos = sorted(pos)
        rng.shuffle(pos)
        t = subst(rng, q, pos[:m])
        for p in pos[m:]:
            t[p] = 4
        t += [rng.randrange(4) for _ in range(extra)]
        assert loss_of(q, t) == 5 * m + 2 * n
        return q, t

    for qlen in (2, 3, 17, 31, 32, 33, 64, 65, 130):
        for kind in ("random", "periodic"):
            ok = qlen > 4          # (the effective band of a query that short is its length: 4 is not below it)
            add("c_ends", [none, exact(qlen, 2, 0, kind, first=True, last=True)], elig=(None, ok))          # mismatches at the first and at the last base
            add("c_ends", [exact(qlen, 2, 0, kind, first=True), exact(qlen, 2, 0, kind, last=True)], elig=(ok, ok))
    for qlen in (20, 64, 130):
        for m, n, ok in ((2, 0, True), (0, 3, False), (1, 1, True), (4, 0, True), (2, 5, True), (3, 3, False), (5, 0, False)):          # L = 10, 6 (= oe - 1), 7 (= oe), 20 (the cap), 20, 21, 25
            L = 5 * m + 2 * n
            assert ok == (OE <= L and L - 6 <= CAP)
            if m + n > qlen:
                continue
            f = exact(qlen, m, n)
            add("c_loss", [none, f], h0=L + 30, elig=(None, ok))
            add("c_loss", [f, none], h0=L + 30, elig=(ok, None))
            add("c_h0", [none, f], h0=L + 1, elig=(None, ok))                                  # h0 = L + 1; h0 = L bars it
            add("c_h0", [none, f], h0=L, elig=(None, False))
            add("c_zdrop", [none, f], h0=L + 30, zdrop=2 * L, elig=(None, ok))               # 2 L = zdrop; one above bars it
            add("c_zdrop", [none, f], h0=L + 30, zdrop=2 * L - 1, elig=(None, False))
            add("c_zdrop", [f, none], h0=L + 30, zdrop=0, elig=(ok, None))                   # no z-drop at all
            add("c_tlen", [none, exact(qlen, m, n, extra=0)], h0=L + 30, elig=(None, ok))     # tlen = qlen; tlen = qlen - 1 bars it
            q, t = exact(qlen, m, n, extra=0)
            add("c_tlen", [none, (q, t[:-1])], h0=L + 30, elig=(None, False))
            add("c_band", [none, f], w=max(1, L - 6), h0=L + 30, elig=(None, False if L - 6 >= 1 else None))          # not below the trial's band: nothing to clamp
            add("c_band", [none, f], w=L - 6 + 1, h0=L + 30, elig=(None, ok))
    # a flank with an insertion or a deletion: the diagonal behind it is junk, its loss far beyond the cap
    for qlen in (40, 90, 130):
        for _ in range(6):
            q = base_seq(rng, qlen, "random")
            k = rng.randrange(5, qlen // 2)
            g = rng.randrange(1, 4)
            tail = [rng.randrange(4) for _ in range(30)]
            add("c_indel", [none, (q, q[:k] + [rng.randrange(4) for _ in range(g)] + q[k:] + tail)], h0=140, elig=(None, False))
            add("c_indel", [(q, q[:k] + q[k + g:] + tail), none], h0=140, elig=(False, None))
    # one side narrow, the other not
    for _ in range(20):
        a, b = exact(rng.randrange(10, 100), 2, 0), flank(rng, "random", qlen=rng.randrange(30, 100), n_sub=12)
        add("c_mixed", [a, b], h0=135, elig=(True, False))
        add("c_mixed", [b, a], h0=135, elig=(False, True))
    return cases


def write_cases(cases, path):
    dig = lambda v: "".join(map(str, v)) if v else "-"
    lines = []
    for c in cases:
        cols = max(len(q) for q, _ in c["sides"]) + 2
        lines.append("%s %d %d %d %d %d %d %s %s %s %s" % (c["kind"], cols, c["h0"], c["w"], c["zdrop"], c["pen5"], c["pen3"], dig(c["sides"][0][0]), dig(c["sides"][0][1]),
                                                            dig(c["sides"][1][0]), dig(c["sides"][1][1])))
    path.write_text("\n".join(lines) + "\n")
    return lines


def run_exe(exe, path, mode, clamp, n):
    p = subprocess.run([exe, "run", str(path), str(mode), str(clamp)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    got, cells = [[] for _ in range(n)], None
    for ln in p.stdout.split("\n"):
        if ln.startswith("# cells"):
            cells = int(ln.split()[2])
        elif ln:
            v = tuple(int(x) for x in ln.split())
            got[v[0]].append(v[1:])          # (side, score, qle, tle, gtle, gscore, max_off, band, wband, loss, ring)
    assert cells is not None
    return got, cells


def branch(r, pen):
    return r[5] <= 0 or r[5] <= r[1] - pen


def relaxed_same(g, e, c, what):
    assert len(g) == len(e), what
    for rg, re_ in zip(g, e):
        pen = c["pen3"] if re_[0] else c["pen5"]
        assert (rg[0], rg[1], rg[6], rg[7]) == (re_[0], re_[1], re_[6], re_[7]), what          # side, score, max_off, band
        assert branch(rg, pen) == branch(re_, pen), what
        if branch(re_, pen):
            assert rg[2:4] == re_[2:4], what          # qle, tle
        else:
            assert rg[4:6] == re_[4:6], what          # gtle, gscore


def test_clamped_equals_unclamped_and_the_checker(orc, exe, tmp_path):
    opt = orc.default_opt()
    assert (opt.o_del, opt.e_del, opt.o_ins, opt.e_ins, opt.a, opt.b) == (6, 1, 6, 1, 1, 4)
    cases = make_cases()
    path = tmp_path / "cases.txt"
    lines = write_cases(cases, path)
    exp = [expected(orc, c) for c in cases]
    n_narrow = n_ring = 0
    for mode in (OFF, STRICT, RELAXED):
        plain, cells0 = run_exe(exe, path, mode, NONE, len(cases))
        for clamp in (CLAMP, RING):
            got, cells = run_exe(exe, path, mode, clamp, len(cases))
            for i, (g, p, e, c) in enumerate(zip(got, plain, exp, cases)):
                what = "mode %d clamp %d case %d (%s): (side, score, qle, tle, gtle, gscore, max_off, band | wband, loss, ring) %r, unclamped %r, the checker %r" % (mode, clamp, i, lines[i], g, p, e)
                assert len(g) == len(p) == len(e) == sum(1 for q, _ in c["sides"] if q), what          # every side ran
                if mode == RELAXED:
                    relaxed_same([r[:8] for r in g], [r[:8] for r in p], c, what)
                    relaxed_same([r[:8] for r in g], e, c, what)
                else:
                    assert [r[:8] for r in g] == [r[:8] for r in p] == e, what
                for r in g:
                    q, t = c["sides"][r[0]]
                    if len(t) >= len(q):
                        assert r[9] == loss_of(q, t), what
                    want = c["elig"][r[0]]
                    if want is not None:
                        assert (r[8] >= 0) == want, what
                    if r[8] >= 0:
                        assert r[8] == r[9] - 6 and OE <= r[9] <= CAP + 6 and c["h0"] > r[9], what          # floor((L - o) / e) with o = 6, e = 1
                        n_narrow += 1
                    if clamp == RING:
                        fits = c["h0"] + sum(len(q) for q, _ in c["sides"]) < 256          # the ring's cells are 8-bit, as LaneNarrow's
                        assert r[10] == int(fits and all(x[8] >= 0 for x in g)), what
                        n_ring += r[10]
            print("mode %d clamp %d: %d cells, %.2f of the unclamped %d" % (mode, clamp, cells, cells / cells0, cells0))
            assert cells < cells0
    assert n_narrow > 1000 and n_ring > 500          # the narrow band and the ring have been run, not only passed by


def test_truth_table(exe):
    """ext_narrow_band's conditions one by one: each line breaks one of them (or none)"""
    #        o_del e_del o_ins e_ins zdrop amax  L  h0 qlen tlen w_eff   band
    rows = [((6, 1, 6, 1, 100, 1, 10, 11, 50, 50, 50), 4),          # all hold: floor((10 - 6) / 1)
            ((6, 1, 6, 1, 100, 1, 7, 8, 1, 1, 2), 1),               # L = oe, qlen = 1
            ((6, 1, 6, 1, 100, 1, 6, 30, 50, 50, 50), -1),          # L = oe - 1: the diagonal answers it
            ((6, 1, 6, 1, 100, 1, 20, 30, 50, 50, 50), 14),         # the cap
            ((6, 1, 6, 1, 100, 1, 21, 30, 50, 50, 50), -1),         # one above
            ((6, 1, 6, 1, 100, 1, 10, 10, 50, 50, 50), -1),         # h0 = L
            ((6, 1, 6, 1, 100, 1, 10, 11, 50, 49, 50), -1),         # tlen < qlen
            ((6, 1, 6, 1, 100, 1, 10, 11, 0, 49, 50), -1),          # no query
            ((6, 1, 6, 1, 20, 1, 10, 11, 50, 50, 50), 4),           # 2 L = zdrop
            ((6, 1, 6, 1, 19, 1, 10, 11, 50, 50, 50), -1),          # 2 L = zdrop + 1
            ((6, 1, 6, 1, 0, 1, 10, 11, 50, 50, 50), 4),            # no z-drop
            ((6, 1, 6, 1, 100, 1, 10, 11, 50, 50, 4), -1),          # not below the effective band
            ((6, 1, 6, 1, 100, 1, 10, 11, 50, 50, 5), 4),
            ((6, 1, 6, 1, 100, 0, 10, 11, 50, 50, 50), -1),         # amax = 0
            ((-1, 1, 6, 1, 100, 1, 10, 11, 50, 50, 50), -1),        # a negative penalty
            ((6, 1, 6, -1, 100, 1, 10, 11, 50, 50, 50), -1),
            ((6, 0, 6, 1, 100, 1, 10, 11, 50, 50, 50), -1),         # a gap extension of 0
            ((6, 1, 6, 0, 100, 1, 10, 11, 50, 50, 50), -1),
            ((6, 2, 6, 1, 100, 1, 12, 13, 50, 50, 50), 6),          # the larger of floor((12 - 6) / 2) and floor((12 - 6) / 1)
            ((4, 1, 9, 3, 100, 1, 11, 12, 50, 50, 50), 7),          # ... of floor((11 - 4) / 1) and floor((11 - 9) / 3)
            ((4, 1, 9, 3, 100, 1, 5, 12, 50, 50, 50), 1),           # L >= the smaller o + e; the other pair allows no excursion at all
            ((4, 1, 9, 3, 100, 1, 4, 12, 50, 50, 50), -1)]
    p = subprocess.run([exe, "band"], input="".join(" ".join(map(str, a)) + "\n" for a, _ in rows), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert [int(x) for x in p.stdout.split()] == [b for _, b in rows]


def test_the_bound_is_tight(exe):
    """tests/golden/ext_narrow_tight.txt: flanks, found by search, where a band ONE narrower than ext_narrow_band's changes a result.  With the bound built one
    too small the clamped run is that narrower run, and differs from the unclamped one here"""
    with open(GOLDEN) as f:
        n = sum(1 for ln in f if ln.strip() and not ln.startswith("#"))
    assert n >= 5
    plain, _ = run_exe(exe, GOLDEN, OFF, NONE, n)
    got, _ = run_exe(exe, GOLDEN, OFF, CLAMP, n)
    less, _ = run_exe(exe, GOLDEN, OFF, ONE_LESS, n)
    for i in range(n):
        assert all(r[8] >= 1 for r in got[i]), i          # every side of these cases has a band, and one that can be narrowed
        assert [r[:8] for r in got[i]] == [r[:8] for r in plain[i]], i
        assert [r[:8] for r in less[i]] != [r[:8] for r in plain[i]], i
