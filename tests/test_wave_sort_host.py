"""The wave sort of the many-region and many-hit reads (seqlib_amd/csrc/dev_wave_sort.h) compiled for the host under ASan + UBSan
(tests/cpp/wave_sort_test.cpp): lists of 2 to 2 048 slots in the four orders the kernels use -- region end; (score, rb, qb); (score, alt, hash);
(mapq, rid, pos) -- against std::sort on distinct keys, guard slots behind the list, and one equal pair at the first, a middle and the last
sorted position for the tie flag."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wave_sort_against_std_sort(tmp_path):
    exe = str(tmp_path / "wave_sort_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "wave_sort_test.cpp")])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(p.stdout)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "failures 0" in p.stdout
