"""SeqLib::STCoverage through the headers only (tests/cpp/cov_api_test.cpp): the program compiles and links without a GPU and its error cases run there; on the GPU
an addRead loop, addReads(BamReader&), the window constructor, SetMode(ALIGNED) and RegionSums are held against tests/cov_util.py, and the bedGraph files of both
ToBedgraph forms against its text."""
import os
import subprocess

import numpy as np
import pytest

from tests import bam_util as bu
from tests import cov_util as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import __graft_entry__ as g
    lib = os.path.join(ROOT, "seqlib_amd")
    if not os.path.exists(os.path.join(lib, "libseqlib_amd.so")):
        g.build()
    out = str(tmp_path_factory.mktemp("covapi") / "cov_api_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cov_api_test.cpp"), "-o", out,
                           "-L" + lib, "-lseqlib_amd", "-Wl,-rpath," + lib, "-lz", "-lpthread"])
    return out


def test_cpp_mirror_links_and_throws_without_a_gpu(exe):
    r = subprocess.run([exe, "errors"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("cov api errors OK"), r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_cpp_mirror_on_the_gpu(exe, tmp_path):
    recs = sorted((r for n, r in cu.CASES if n not in ("tid_n_ref", "tid_-1", "pos_-1")), key=lambda r: cu.parse(r)[:2]) + [dict(cu.CASES)["tid_-1"]]
    bam = tmp_path / "cases.bam"
    bam.write_bytes(bu.bam_bytes(cu.TEXT, cu.REFS, recs, member_size=700))
    E = {"n_records": [len(recs)]}
    for name, mode, buff in (("span0", cu.SPAN, 0), ("span3", cu.SPAN, 3), ("full", cu.FULL, 0)):
        d = cu.depth(recs, mode, buff, exclude_flags=0)          # addRead tests no flag
        E[name + "_depth2"] = d[2].tolist()
        E[name + "_max"] = [max(int(v.max()) for v in d)]
        E[name + "_win_290_310"] = d[2][290:300].tolist() + [0] * 10
    E["aligned_depth2"] = cu.depth(recs, cu.ALIGNED, min_mapq=4)[2].tolist()
    dd = cu.depth(recs, cu.ALIGNED, 0, 1, min_mapq=4)
    E["aligned_del_depth2"] = dd[2].tolist()
    E["region_sum"], E["region_cnt"] = cu.region_sums(dd, [(2, 0, 5000), (2, 700, 730), (1, 10, 10), (3, 9999000, 10000001)], 2)
    assert E["span0_depth2"] != E["span3_depth2"] != E["full_depth2"] != E["aligned_depth2"] != E["aligned_del_depth2"] and E["region_cnt"][0] > 0
    exp = tmp_path / "expect.txt"
    exp.write_text("".join("%s %d %s\n" % (k, len(v), " ".join(map(str, v))) for k, v in E.items()))
    r = subprocess.run([exe, "run", str(bam), str(exp), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.endswith("cov api OK\n"), r.stdout[-2000:] + r.stderr[-3000:]
    for name, mode, buff in (("span0", cu.SPAN, 0), ("span3", cu.SPAN, 3), ("full", cu.FULL, 0)):
        d = cu.depth(recs, mode, buff, exclude_flags=0)
        want = cu.bedgraph(d, 0)
        assert want.count(b"\n") > 10 and np.count_nonzero(d[3]) > 0
        assert (tmp_path / (name + "_stream.bg")).read_bytes() == want, name
        assert (tmp_path / (name + "_path.bg")).read_bytes() == want, name
        assert (tmp_path / (name + "_zero.bg")).read_bytes() == cu.bedgraph(d, 1), name
