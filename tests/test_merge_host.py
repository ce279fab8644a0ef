"""CPU tests of the merge of sorted BAM files (include/seqlib_amd_merge.h, seqlib_amd/csrc/slx_merge.hip, dev_merge.h, merge_host.h): the exports, the refusal
without a GPU, the header rule against the Python rule of tests/merge_util.py, and a whole merge on the host -- the planner over the host-compiled key, bound,
rank and place bodies -- under ASan + UBSan against std::stable_sort (tests/cpp/merge_host_test.cpp, a program of its own).  No test here needs a GPU."""
import os
import re
import subprocess

import pytest

from tests import merge_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "seqlib_amd", "libseqlib_amd.so")):
        g.build()
    from seqlib_amd import _ffi
    _ffi.lib()
    return _ffi


def test_merge_exports_match_header(ffi):
    from seqlib_amd import mergeio, sortio
    hdr = open(os.path.join(ROOT, "include", "seqlib_amd_merge.h")).read()
    body = hdr[hdr.index("extern \"C\""):]
    declared = set(re.findall(r"\b(slx_[a-z0-9_]+)\s*\(", body))
    assert declared == set(mergeio.EXPORTS), declared ^ set(mergeio.EXPORTS)
    assert all(name.startswith("slx_merge_") for name in declared)
    L = mergeio.lib()
    for name in declared:
        assert hasattr(L, name), name
    head = hdr[:hdr.index("#ifndef")]
    for name in mergeio.EXPORTS:
        assert name in head, name
    for words in ("Not carried", "No CPU fallback", "key < B", "never edited", "at most 64") + mergeio.KNOBS + mergeio.COUNTERS:
        assert words in hdr, words
    # the sorter's two new entry points are declared, bound and exported too
    sort_hdr = open(os.path.join(ROOT, "include", "seqlib_amd_sort.h")).read()
    for name in ("slx_sort_spill", "slx_sort_file_spill"):
        assert name in sort_hdr and name in sortio.SORT_EXPORTS and hasattr(sortio.lib(), name), name
    assert {"runs", "run_bytes", "us_merge"} <= set(sortio.COUNTERS)


def test_merge_no_gpu_fails_loudly(ffi, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from seqlib_amd import mergeio
    from tests import bam_util as bu
    with pytest.raises(ffi.SlxError) as e:
        mergeio.Merger()
    assert e.value.code == ffi.SLX_ENODEVICE and "no CPU fallback" in str(e.value)
    src, out = tmp_path / "in.bam", tmp_path / "out.bam"
    src.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, sorted(bu.sample_records(20), key=mu.key)))
    with pytest.raises(ffi.SlxError) as e:
        mergeio.merge_files([src, src], out)
    assert e.value.code == ffi.SLX_ENODEVICE and "no CPU fallback" in str(e.value)
    assert not out.exists()


@pytest.mark.parametrize("name", list(mu.HEADER_CASES))
def test_merge_header_rule(ffi, name):
    from seqlib_amd import mergeio
    texts, want = mu.HEADER_CASES[name]
    if want is mu.IdClash:
        with pytest.raises(mu.IdClash) as clash:
            mu.header_rule(texts)
        with pytest.raises(ffi.SlxError) as e:
            mergeio.header_text(texts)
        assert e.value.code == ffi.SLX_EUNSUPPORTED and "ID:" + str(clash.value) in str(e.value), str(e.value)
        return
    assert mu.header_rule(texts) == want                       # the Python rule gives what the case was written down to give
    assert mergeio.header_text(texts) == want
    assert mergeio.header_text([want]) == want                 # and a merged text is a fixed point as the only input


def test_merge_header_is_one_copy():
    """the C-ABI and the C++ class share the rule: BamMerger.h takes the header from slx_merge_header, and the rule's lines are told apart in merge_host.h only"""
    hits = []
    for base, exts in (("include", (".h",)), (os.path.join("seqlib_amd", "csrc"), (".h", ".hip", ".cpp"))):
        for dp, _, fns in os.walk(os.path.join(ROOT, base)):
            for fn in fns:
                if fn.endswith(exts):
                    code = [ln.split("//")[0] for ln in open(os.path.join(dp, fn), errors="replace") if not ln.lstrip().startswith(("*", "/*", "//"))]
                    if any('"@CO"' in ln for ln in code):
                        hits.append(fn)
    assert hits == ["merge_host.h"], hits
    assert "slx_merge_header(" in open(os.path.join(ROOT, "include", "SeqLib", "BamMerger.h")).read()


def test_merge_util_is_consistent():
    """the helper the GPU tests take their expectation from: stable, ties by input; the builder deals by (7 * j) % k and keeps every input sorted"""
    inputs = mu.build_inputs(3, block_in=1)
    want, frm = mu.expected_merge(inputs)
    assert sorted(want, key=mu.key) == want and len(want) == sum(len(v) for v in inputs)
    ties = [(r, i) for r, i in zip(want, frm) if mu.key(r) == mu.TIE_AT]
    assert len(ties) == mu.N_TIES and [i for _, i in ties] == sorted(i for _, i in ties) and {i for _, i in ties} == {0, 1, 2}
    blk = [i for r, i in zip(want, frm) if mu.key(r) == mu.BLOCK_AT]
    assert blk == [1] * mu.N_BLOCK and sum(len(r) for r in mu.block_records()) > 2 * 0x2000
    assert sum(1 for v in inputs if mu.key(v[-1])[0] == 0xffffffff) == 3 and want[0][36:45] == b"minus_one"
    assert mu.expected_runs([5, 5, 5, 5], 10) == 2 and mu.expected_runs([5, 5], 10) == 0 and mu.expected_runs([5, 6, 5], 10) == 3 and mu.expected_runs([11], 10) is None


def test_merge_host_program_under_asan_ubsan(tmp_path):
    """the planner of merge_host.h over the bodies of dev_merge.h on the host, waves of 1 and of 64 lanes, in a stand-alone program: batches of 1, 2 and 3
    records, k = 1, 2, 3 and 64, every table allocated exactly, against std::stable_sort; the program asserts the edges its inputs are built for"""
    exe = str(tmp_path / "merge_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Werror",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "cpp", "merge_host_test.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    # cases, rounds, rounds that emitted nothing (the tie block's), waves that straddled two inputs
    assert words[:2] == ["merge_host", "OK"] and int(words[2]) >= 40 and int(words[3]) > 1000 and int(words[4]) > 50 and int(words[5]) > 100, r.stdout
