"""Wave reductions and prefix sums of the record-batch units go through seqlib_amd/csrc/dev_lanes.h only.

The butterfly `for (o = 32; o; o >>= 1) v op= __shfl_xor(v, o, 64)` and the `__shfl_up` ladder stood in some twenty places, copied from unit to unit with
a different cast each time; so did the per-unit lane policy structs and the "sum, then one atomic from lane 0" wrappers.  dev_lanes.h has them once
(DESIGN.md section 9).  What stays hand-written is listed here by file, with the number of lines that name a shuffle.  The aligner, the FML units, the index
builders and the inflate / deflate kernels are out of scope: their shuffles sit inside tuned loops.  This is plain text matching over the sources: no
compiler, no GPU."""
import fnmatch
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "seqlib_amd", "csrc")

SHUFFLE = re.compile(r"\b__shfl_(?:xor|up|down)\b")
OUT_OF_SCOPE = ("dev_seed4.h", "dev_ext_*.h", "dev_chain*.h", "dev_fin*.h", "dev_cig_*.h", "dev_long.h", "slx_align*.hip", "slx_chunk.inc",
                "dev_fml*.h", "slx_fml*", "slx_index_gpu*.hip", "dev_inflate.h", "dev_deflate.h")
# lines that name a shuffle, per file
ALLOWED = {
    "slx_filter.hip": 3,    # k_flt_eval_long: a reduction over a whole struct (rf_part_join)
    "slx_rec.hip": 1,       # a reduction over a whole struct
    "slx_bam.hip": 3,       # an xor reduction, the fused min / max of a tile's offsets, a __shfl_down hand-over
    "slx_bgzf.hip": 1,      # an xor reduction
    "slx_sort.hip": 1,      # k_sort_key: max and min in one loop; as two helper calls the kernel took 18 VGPRs for 14
    "slx_ref.hip": 1,       # md_wave_walk: the scan of the MD pieces; through wave_scan_excl k_md_long<true> took 54 VGPRs for 53
}
GONE = ("cov_one", "pile_one", "samw_one", "cov_wave", "pile_group", "samw_wave", "cov_count", "pile_count", "st_count", "dp_count", "dp_report", "wn_report",
        "st_wave_sum", "dp_wave_sum32")
GONE_RX = re.compile(r"\b(?:" + "|".join(GONE) + r")\b")


def _in_scope():
    files = []
    for pat in ("*.h", "*.hip", "*.inc"):
        files += glob.glob(os.path.join(CSRC, pat))
    assert len(files) > 30 and os.path.join(CSRC, "dev_lanes.h") in files
    skip = ("dev_lanes.h",) + OUT_OF_SCOPE
    return sorted(f for f in files if not any(fnmatch.fnmatch(os.path.basename(f), p) for p in skip))


def _hits(rx, files):
    out = []
    for f in files:
        with open(f, errors="replace") as fh:
            for n, line in enumerate(fh, 1):
                if rx.search(line):
                    out.append((os.path.basename(f), "%s:%d: %s" % (os.path.relpath(f, ROOT), n, line.strip()[:160])))
    return out


def test_the_patterns_match_what_they_are_meant_to():
    for bad in ("for (int o = 32; o; o >>= 1) v += (uint64_t)__shfl_xor((cov_ull)v, o, 64);", "const uint32_t t = __shfl_up(incl, s, 64);",
                "const unsigned long long up = __shfl_down(v, o, 64);", "m = x < m ? x : __shfl_xor(m, o);"):
        assert SHUFFLE.search(bad), bad
    for good in ("const uint64_t bj = (uint64_t)__shfl((ull)b, j, 64);", "c = wave_sum(c);", "uint64_t w = at + wave_scan_excl(c, &total);",
                 "const int v = my__shfl_xor_like(m);"):
        assert not SHUFFLE.search(good), good
    for bad in ("cov_record(F, P, G, 0u, 1u, cov_one(), S);", "template <int G> struct pile_group {", "st_count(cnt, ST_K_LDS, S.n_lds);",
                "dp_count(&st->mixed, mixed);", "Q.qsum = st_wave_sum(Q.qsum);"):
        assert GONE_RX.search(bad), bad
    for good in ("const int k = name ? st_counter_index(name) : -1;", "struct dp_counts { int64_t ignored = 0; };", "def test_counts(io, data):",
                 "pile_record(F, P, 0u, 1u, lanes_one(), S);", "wave_count(&st->mixed, mixed);"):
        assert not GONE_RX.search(good), good
    assert any(fnmatch.fnmatch("dev_ext_reg.h", p) for p in OUT_OF_SCOPE) and not any(fnmatch.fnmatch("dev_edit.h", p) for p in OUT_OF_SCOPE)


def test_no_hand_written_collective_outside_dev_lanes_h():
    per_file = {}
    for name, where in _hits(SHUFFLE, _in_scope()):
        per_file.setdefault(name, []).append(where)
    wrong = {f: w for f, w in per_file.items() if len(w) != ALLOWED.get(f, 0)}
    wrong.update({f: [] for f in ALLOWED if f not in per_file})
    assert not wrong, "reduce and scan through dev_lanes.h (wave_sum, wave_min, wave_max, wave_scan_excl, lanes_group), or correct the allow-list:\n" + "\n".join(
        "%s: %d lines, %d allowed\n  %s" % (f, len(w), ALLOWED.get(f, 0), "\n  ".join(w)) for f, w in sorted(wrong.items()))


def test_the_per_unit_copies_are_gone():
    files = []
    for top in ("seqlib_amd", "tests", "tools"):
        for d, _, names in os.walk(os.path.join(ROOT, top)):
            files += [os.path.join(d, n) for n in names if n.endswith((".h", ".hip", ".inc", ".cpp", ".py", ".md"))]
    me = os.path.abspath(__file__)
    found = [w for _, w in _hits(GONE_RX, sorted(f for f in files if os.path.abspath(f) != me))]
    assert len(files) > 100 and not found, "dev_lanes.h has lanes_one, lanes_group, wave_count and wave_report_min for these:\n" + "\n".join(found)
