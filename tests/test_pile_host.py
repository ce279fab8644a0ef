"""The host side of the pileup unit, without a GPU: the exports, slx_pile_record_events against the Python statement of the rules (tests/pile_util.py), what a
host-only object answers, and pile_host.h's per-record and per-position bodies under sanitizers in a stand-alone program (tests/cpp/pile_host_test.cpp) with 1, 16
and 64 simulated lanes."""
import os
import random
import re
import subprocess

import pytest

import seqlib_amd  # noqa: F401  (the package must import)
from seqlib_amd import _ffi, pileio
from tests import pile_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """tests/cpp/pile_host_test.cpp under ASan and UBSan: a program of its own, nothing is loaded into Python"""
    out = str(tmp_path_factory.mktemp("pile") / "pile_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Werror", "-pthread",
                           "-I" + os.path.join(ROOT, "seqlib_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pile_host_test.cpp"), "-o", out])
    return out


def test_header_declares_exactly_the_exports():
    text = open(os.path.join(ROOT, "include", "seqlib_amd_pile.h")).read()
    body = text[text.index("#ifndef SEQLIB_AMD_PILE_H"):]
    declared = re.findall(r"^\s*(?:int|void|int64_t|const char \*)\s+\*?(slx_\w+)\s*\(", body, re.M)
    assert sorted(declared) == sorted(pileio.EXPORTS)
    assert all(n.startswith("slx_pile_") for n in declared)
    L = pileio.lib()
    for n in pileio.EXPORTS:
        assert hasattr(L, n), n
    assert "#define SLX_PILE_PLANES 15" in body and "bit-identical whatever the order of records, batches, kernels and knobs" in text
    assert "seqlib_amd_pile.h" in open(os.path.join(ROOT, "include", "seqlib_amd_cov.h")).read()


def test_the_case_list_covers_what_it_claims():
    names = [n for n, _ in pu.CASES]
    assert len(set(names)) == len(names)
    by = dict(pu.CASES)
    ev = pu.events
    assert ev(by["one_base"]) == [(pu.G, 250)] and ev(by["odd_length"]) == [(pu.A, 230), (pu.C, 231), (pu.G, 232), (pu.T, 233), (pu.N, 234), (pu.A, 235), (pu.C, 236)]
    assert [p for p, _ in ev(by["all_codes"])] == [pu.N, pu.A, pu.C, pu.N, pu.G, pu.N, pu.N, pu.N, pu.T, pu.N, pu.N, pu.N, pu.N, pu.N, pu.N, pu.N]
    assert all(7 <= p < 14 for p, _ in ev(by["plain_rev"])) and all(p < 7 for p, _ in ev(by["plain"])) and len(ev(by["plain"])) == 50
    assert ev(by["leading_I"])[0] == (pu.INS, 99) and ev(by["leading_I_at_0"])[0] == (pu.INS, -1) and ev(by["trailing_I"])[-1] == (pu.INS, 299)
    assert pu.clipped(ev(by["leading_I"]), 100, 300)[0][1] == 100 and len(pu.clipped(ev(by["leading_I_at_0"]), 0, 5000)) == 10
    assert ev(by["trailing_I_at_window_end"])[-1] == (pu.INS, 299) and ev(by["I_anchored_on_last_base"])[5] == (pu.INS, 4999)
    assert len(ev(by["short_seq_in_M"])) == 12 and len(ev(by["short_seq_second_M"])) == 5 + 3 + 3 and ev(by["short_seq_S_passes_it"]) == []
    assert [p for p, _ in ev(by["short_seq_I_D_then_M"])][5:] == [pu.INS, pu.DEL, pu.DEL] and [p for p, _ in ev(by["short_seq_ends_with_op"])][8:] == [pu.DEL] * 4
    assert ev(by["0M"]) == [] and [p for p, _ in ev(by["0M_past_short_seq"])][2:] == [pu.DEL] * 3
    assert {p for p, _ in ev(by["with_quals"], 20)} >= {pu.LOWQ} and pu.LOWQ not in {p for p, _ in ev(by["plain"], 99)} and pu.LOWQ not in {p for p, _ in ev(by["quals_ff_then_zeros"], 99)}
    assert {p for p, _ in ev(by["with_quals_rev"], 20)} >= {pu.LOWQ, pu.REV + pu.INS} and [p for p, _ in ev(by["quals_ff_inside"], 1)].count(pu.LOWQ) == 19
    for k in range(16):
        got = ev(by["op_code_%d" % k])
        assert len(got) == (7 if k in (0, 2, 7, 8) else 1 if k == 1 else 0), k
    assert [len(pu.parse(by["ops_%d" % n])[4]) for n in (64, 65, 200)] == [64, 65, 200] and len(pu.parse(by["read_5000"])[5]) == 5000
    assert not any(pu.eligible(by[n], 2) for n in ("tid_elsewhere", "tid_-1", "pos_-1", "unmapped_placed", "dup", "secondary", "qcfail", "n_cigar_0", "l_seq_0", "big_contig"))
    assert pu.eligible(by["supplementary"], 2) and pu.eligible(by["low_mapq"], 2) and not pu.eligible(by["low_mapq"], 2, min_mapq=4) and pu.eligible(by["dup"], 2, exclude_flags=0)
    pl = pu.planes([r for _, r in pu.CASES])
    assert pl.shape == (15, 5000) and pl[pu.DEL, 4999] == 2 and pl[pu.INS, 4999] == 1 and pl[:, 0].sum() == 3 and pl[pu.REV + pu.DEL].sum() == 28
    w = pu.planes([r for _, r in pu.CASES], (2, 100, 300))
    assert (w == pl[:, 100:300]).all() and w[pu.INS, 199] == 2 and pu.planes([], (2, 4900, 6000)).shape == (15, 100)


@pytest.mark.parametrize("name,r", pu.CASES, ids=[n for n, _ in pu.CASES])
def test_record_events_equal_python(name, r):
    for min_baseq in (0, 20, 41):
        for clip in pu.CLIPS:
            assert pileio.record_events(r, min_baseq, clip) == pu.clipped(pu.events(r, min_baseq), *clip), (min_baseq, clip)


def test_record_events_clip_at_both_ends():
    r = dict(pu.CASES)["M_over_window_begin_and_end"]          # 300M from 95
    got = pileio.record_events(r, 0, (100, 300))
    assert [x for _, x in got] == list(range(100, 300)) and got == pu.events(r)[5:205]
    assert pileio.record_events(r, 0, (395, 5000)) == [] and len(pileio.record_events(r, 0, (394, 5000))) == 1 and len(pileio.record_events(r, 0, (0, 96))) == 1
    d = dict(pu.CASES)["D_over_window_begin"]                  # 5M20D5M from 90
    assert pileio.record_events(d, 0, (100, 300)) == [(pu.DEL, x) for x in range(100, 115)] + pu.events(d)[25:]


def test_record_events_refuse_a_small_cap_and_a_broken_record():
    r = dict(pu.CASES)["10M3D10M2I5M"]
    n = len(pu.events(r))
    assert pileio.record_events(r, cap=n) == pu.events(r)
    with pytest.raises(_ffi.SlxError) as e:
        pileio.record_events(r, cap=n - 1)
    assert e.value.code == _ffi.SLX_EINVAL
    b = bytearray(r)
    for bad in (bytes(b[:-1]), bytes(b[:20]), bytes(b[:16] + b"\xff\xff" + b[18:]), bytes(b[:20] + b"\xff\xff\xff\x7f" + b[24:])):          # cut, cut inside the fixed part, n_cigar and l_seq past block_size
        with pytest.raises(_ffi.SlxError) as e:
            pileio.record_events(bad)
        assert e.value.code == _ffi.SLX_EIO


def test_create_and_knobs_refuse_bad_arguments():
    with pytest.raises(_ffi.SlxError) as e:
        pileio.Pile(pu.REFS, None)
    assert e.value.code == _ffi.SLX_EINVAL and "window" in str(e.value)
    for win in ((4, 0, 10), (-1, 0, 10), (2, 10, 5)):
        with pytest.raises(_ffi.SlxError) as e:
            pileio.Pile(pu.REFS, win)
        assert e.value.code == _ffi.SLX_EINVAL
    with pytest.raises(_ffi.SlxError) as e:
        pileio.Pile([("neg", -1)], (0, 0, 1))
    assert e.value.code == _ffi.SLX_EINVAL
    p = pileio.Pile(pu.REFS, pu.WHOLE)          # host only without a GPU: the arguments are checked first either way
    for key, v in (("min_mapq", 256), ("min_mapq", -1), ("min_baseq", 256), ("exclude_flags", 0x10000), ("long_cigar", (1 << 20) + 1), ("long_read", -1), ("lds_window", 1025),
                   ("lds_window", -1), ("slice_records", 63), ("slice_records", (1 << 20) + 1), ("group_lanes", 8), ("group_lanes", 48), ("no_such_knob", 1)):
        with pytest.raises(_ffi.SlxError) as e:
            p.set(key, v)
        assert e.value.code == _ffi.SLX_EINVAL, (key, v)
    assert p.counter("records_seen") == 0 and p.counter("sites") == 0 and p.counter("nonsense") == -1
    p.close()


def test_without_a_gpu_everything_else_is_enodevice():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_pile.py adds records")
    p = pileio.Pile(pu.REFS, pu.WHOLE)          # host only
    stream, off = pu.stream_of([r for _, r in pu.CASES])

    class NoRef:
        h = None
    for call in (lambda: p.add_host(stream, off), lambda: p.add_device(None, 0, None, 0), lambda: p.counts(0), lambda: p.counts_device(0), lambda: p.at(3), lambda: p.clear(),
                 lambda: p.sites(NoRef, 0, 1, 1, 0, 1), lambda: p.sites_tsv("/dev/null"), lambda: _ffi.check(pileio.lib().slx_pile_sites_to_host(p.h, None)),
                 lambda: p.set("min_mapq", 3), lambda: p.set("lds_window", 0)):
        with pytest.raises(_ffi.SlxError) as e:
            call()
        assert e.value.code == _ffi.SLX_ENODEVICE
    assert p.counter("records_seen") == 0
    p.close()
    with pytest.raises(_ffi.SlxError) as e:
        pileio.Pile(pu.REFS, pu.WHOLE, device=0)
    assert e.value.code == _ffi.SLX_ENODEVICE


def test_bodies_under_sanitizers(exe, tmp_path):
    """pile_host.h over the case list, every record in a heap block of exactly its size, through 1, 16 and 64 lanes: pile_head's verdict and pile_record's events for
    every clip (and, where the record has qualities, for two floors), and pile_site on random and on edge positions -- Python's, with no sanitizer report"""
    lines, n = [], 0
    for name, r in pu.CASES:
        has_q = len(pu.parse(r)[6]) > 0 and pu.parse(r)[6][0] != 0xff
        for min_baseq, clips in [(0, pu.CLIPS)] + ([(20, pu.CLIPS[:1]), (41, pu.CLIPS[2:3])] if has_q else []):
            for clip in clips:
                ev = pu.clipped(pu.events(r, min_baseq), *clip)
                many = clip in (pu.CLIPS[0], pu.CLIPS[2])          # every case through 1, 16 and 64 lanes unclipped and clipped at both ends; the other clips through one lane
                lines.append("C %s %s %d %d %d %d %d %d %s" % (name, r.hex(), pu.eligible(r, 2), min_baseq, many, clip[0], clip[1], len(ev), " ".join("%d %d" % x for x in ev)))
                n += 1
    rng = random.Random(11)
    n_pos = 0
    import numpy as np
    for k in range(400):
        c = [rng.choice((0, 0, 1, 2, 5, 30)) for _ in range(15)]
        if k == 0:
            c = [0] * 15
        if k == 1:
            c = [2 ** 31 - 1] * 4 + [0] * 11          # the sums are 64-bit before they are compared
        ref = rng.choice(b"ACGTacgtNnRyX*")
        q = rng.choice([(1, 1, 0, 1), (10, 2, 1, 5), (1, 1, 1, 1), (100, 1, 0, 1), (3, 3, 1, 3)])
        pl = np.array(c, dtype=np.int64).reshape(15, 1)
        got = pu.sites(pl, 0, bytes([ref]), *q)
        depth = sum(c[i] + c[7 + i] for i in range(6))
        up = ref - 32 if 97 <= ref <= 122 else ref
        r4 = {65: 0, 67: 1, 71: 2, 84: 3}.get(up)
        alt = 0 if r4 is None else depth - c[r4] - c[7 + r4]
        if k == 1:          # (depth does not fit the int32 the site carries: only the verdict is compared on the GPU; here the truncated values)
            wrap = lambda v: (v + 2 ** 31) % 2 ** 32 - 2 ** 31
            depth_s, alt_s = wrap(depth), wrap(alt)
        else:
            depth_s, alt_s = depth, alt
        lines.append("S %d %d %d %d %d %s %d %d %d %d %d" % (q + (ref, " ".join(map(str, c)), len(got), up, depth_s, alt_s, c[6] + c[13])))
        n_pos += 1
    p = tmp_path / "expect.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "cases", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "pile_host_test OK: %d cases, %d positions" % (n, n_pos) in r.stdout
