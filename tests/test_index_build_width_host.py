"""Which suffix sorter builds a text (seqlib_amd/csrc/index_build_width.h), compiled for the host under ASan + UBSan (tests/cpp/index_build_width_test.cpp): the
32-bit builder hands hipCUB its 2 * total + 1 elements as an int, so references from 2^30 bases on -- a chicken or zebrafish genome, chr1 of GRCh38 with its
neighbours -- belong to the 64-bit builder.  The predicate at INT_MAX / 2 - 1, INT_MAX / 2, INT_MAX / 2 + 1, around 2^31 and 2^32 and where 2 * total wraps."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_builder_choice_at_the_int_boundary(tmp_path):
    exe = str(tmp_path / "index_build_width_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "seqlib_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "index_build_width_test.cpp")])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(p.stdout)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "failures 0" in p.stdout
