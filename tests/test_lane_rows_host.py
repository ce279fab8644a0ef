"""The lane kernels' row loop (seqlib_amd/csrc/dev_lane_rows.h: both sides of a seed and both band trials in one loop) compiled for the host,
under ASan + UBSan, on rows of exactly the columns the kernel gives a job (tests/cpp/lane_rows_test.cpp): all six results of every extension
against the checker's ksw_extend2, band trials as mem_chain2aln runs them."""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QLENS = (1, 2, 63, 64, 65, 131)
H0S = (19, 131)
WS = (1, 4, 100)
ZDROP, PEN5, PEN3 = 100, 5, 5


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lane_rows") / "lane_rows_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "lane_rows_test.cpp")])
    return out


def edits():
    """(name, function query -> target): 0 / 1 / 2 / 10 mismatches; insertions and deletions (in the query, against the target) of 1 .. 8 bases"""
    def subst(n):
        def f(q, rng):
            t = list(q)
            for k in rng.sample(range(len(q)), min(n, len(q))):
                t[k] = (t[k] + 1 + rng.randrange(3)) % 4
            return t
        return f

    def ins(n):         # the query holds n bases the target lacks
        def f(q, rng):
            k = rng.randrange(len(q))
            return list(q[:k]) + list(q[k + n:])
        return f

    def dele(n):        # the target holds n bases the query lacks
        def f(q, rng):
            k = rng.randrange(len(q) + 1)
            return list(q[:k]) + [rng.randrange(4) for _ in range(n)] + list(q[k:])
        return f
    return [("mm%d" % n, subst(n)) for n in (0, 1, 2, 10)] + [("ins%d" % n, ins(n)) for n in range(1, 9)] + [("del%d" % n, dele(n)) for n in range(1, 9)]


def make_side(rng, qlen, edit, longer):
    """a query of qlen bases and its target: the edited query, cut below the query's length or run on past it"""
    q = [rng.randrange(4) for _ in range(qlen)]
    t = edit(q, rng)
    if longer:
        t = t + [rng.randrange(4) for _ in range(max(qlen + 12 - len(t), 7))]
    else:
        t = t[:max(min(len(t), qlen - 1 - rng.randrange(3)), 0)]
    return q, t


def oracle_side(orc, q, t, w, end_bonus, h0, before):
    """mem_chain2aln's two band trials around the checker's ksw_extend2: the six results and the band of the trial that stands"""
    L = orc.lib()
    mat = orc.default_opt().mat
    prev = before
    for i in range(2):
        aw = w << i
        o = [C.c_int() for _ in range(5)]
        sc = L.orc_ksw_extend2(len(q), bytes(q), len(t), bytes(t), 5, mat, 6, 1, 6, 1, aw, end_bonus, ZDROP, h0, *[C.byref(x) for x in o])
        res = (sc, o[0].value, o[1].value, o[2].value, o[3].value, o[4].value, aw)
        if sc == prev or o[4].value < (aw >> 1) + (aw >> 2):
            break
        prev = sc
    return res


def expected(orc, sides, w, h0):
    exp = []
    score = h0
    for s, (q, t) in enumerate(sides):
        if not q:
            continue
        r = oracle_side(orc, q, t, w, PEN3 if s else PEN5, score, score if s else -1)
        exp.append((s,) + r)
        score = r[0]
    return exp


def test_rows_against_the_checker(orc, exe, tmp_path):
    opt = orc.default_opt()
    assert (opt.o_del, opt.e_del, opt.o_ins, opt.e_ins, opt.a, opt.b) == (6, 1, 6, 1, 1, 4)
    rng = random.Random(20)
    cases = []          # (sides, w, h0)
    for qlen in QLENS:
        for longer in (0, 1):
            for h0 in H0S:
                for name, edit in edits():
                    for w in WS:
                        for side in (0, 1):          # dir = -1, +1
                            qt = make_side(rng, qlen, edit, longer)
                            cases.append(([qt, ([], [])] if side == 0 else [([], []), qt], w, h0))
    # two sides back to back on one row: the second meets the cells the first left (a longer first side, a shorter, the same)
    ed = dict(edits())
    for ql, qr in ((131, 5), (5, 131), (65, 63), (63, 65), (64, 64), (2, 1), (131, 131)):
        for h0 in H0S:
            for name in ("mm0", "mm2", "mm10", "ins3", "del5", "del8"):
                for w in WS:
                    for longer in (0, 1):
                        cases.append(([make_side(rng, ql, ed[name], longer), make_side(rng, qr, ed[name], 1 - longer if ql == qr else longer)], w, h0))
    lines, exp, lanes = [], [], (0, 37, 63)
    dig = lambda v: "".join(map(str, v)) if v else "-"
    n_narrow = 0
    for sides, w, h0 in cases:
        e = expected(orc, sides, w, h0)
        cols = max(len(q) for q, _ in sides) + 2          # columns 0 .. the longer query, and the one the kernels' rows keep beyond it
        # the 8-bit cells take a job only where no score can reach 256 (the kernel: read length x max(mat) < 256)
        layouts = "wn" if h0 + sum(len(q) for q, _ in sides) < 256 else "w"
        for lay in layouts:
            n_narrow += lay == "n"
            lines.append("%s %d %d %d %d %d %d %d %s %s %s %s" % (lay, lanes[len(lines) % 3], cols, h0, w, ZDROP, PEN5, PEN3, dig(sides[0][0]), dig(sides[0][1]),
                                                                     dig(sides[1][0]), dig(sides[1][1])))
            exp.append(e)
    assert n_narrow > 1000 and len(lines) - n_narrow > 2000
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    p = subprocess.run([exe, "run", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    got = [[] for _ in lines]
    for ln in p.stdout.split("\n"):
        if ln:
            v = tuple(int(x) for x in ln.split())
            got[v[0]].append(v[1:])
    second_band = 0
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g == e, "case %d (%s): (side, score, qle, tle, gtle, gscore, max_off, band) %r, the checker %r" % (i, lines[i], g, e)
        second_band += any(r[7] != int(lines[i].split()[4]) for r in e)
    assert second_band > 50          # the second band trial ran (w = 1 and 4 against indels)

