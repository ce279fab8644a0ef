"""The extension walk's lane-made chain header (seqlib_amd/csrc/dev_chain_hdr.h) compiled for the host under ASan + UBSan
(tests/cpp/chain_hdr_test.cpp): chains of 1, 2, 8, 9 and 65 seeds at the ends of three contigs, on both strands and across l_pac, reads of
40 and 150 bases -- the window, the top seed and the one-seed seedcov against a restatement of the checker's mem_chain2aln."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_header_against_the_checker(tmp_path):
    exe = str(tmp_path / "chain_hdr_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "chain_hdr_test.cpp")])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(p.stdout)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "failures 0" in p.stdout
