"""CPU tests of the BamReader path (include/seqlib_amd_bam.h, seqlib_amd/csrc/slx_bam.hip): the exports, the host-side member scan against the Python
statement of BGZF (tests/bam_util.py), the refusal without a GPU, the host-compiled DEFLATE / CRC32 bodies against zlib under ASan + UBSan, and the
record index's algorithm restated in scalar C against the plain chain walk.  No test here needs a GPU.
DEFLATE that zlib never writes, streams it refuses and the 64-lane host run are in tests/test_inflate_foreign.py."""
import json
import os
import random
import re
import struct
import subprocess

import pytest

from tests import bam_util as bu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "seqlib_amd", "libseqlib_amd.so")):
        g.build()
    from seqlib_amd import _ffi
    _ffi.lib()
    return _ffi


def payloads():
    rng = random.Random(11)
    bam = bu.bam_header(bu.TEXT, bu.REFS) + b"".join(bu.sample_records(120))
    return {"bam": bam[:bu.MEMBER_MAX], "one_byte": b"\x07" * bu.MEMBER_MAX, "random": bytes(rng.randrange(256) for _ in range(bu.MEMBER_MAX)),
            "text": b"the quick brown fox jumps over the lazy dog, and the quick brown fox does it again"}


def corpus():
    """[(name, deflate bytes, payload)]: every compression setting x every payload, plus empty members"""
    out = []
    for sname, opts in bu.SETTINGS.items():
        for pname, p in payloads().items():
            if 18 + len(bu.deflate_raw(p, **opts)) + 8 > 0x10000:          # fixed codes spend nine bits on most random bytes: a writer fills such a member less
                p = p[:0xd000]
            out.append((sname + "/" + pname, bu.deflate_raw(p, **opts), p))
    out.append(("empty/dyn6", bu.deflate_raw(b""), b""))
    out.append(("empty/stored", bu.deflate_raw(b"", level=0), b""))
    out.append(("eof", bu.EOF_BLOCK[18:20], b""))
    return out


def test_corpus_has_all_three_block_types():
    """the settings give what the tests rely on: stored, fixed and dynamic first blocks, and several blocks in one member"""
    kinds = {}
    for name, comp, _ in corpus():
        kinds.setdefault((comp[0] >> 1) & 3, []).append(name)
    assert set(kinds) == {0, 1, 2}, kinds
    assert any(n.startswith("stored/") for n in kinds[0]) and any(n.startswith("fixed/") for n in kinds[1]) and any(n.startswith("dyn6/") for n in kinds[2])
    p = payloads()["bam"]
    assert len(bu.deflate_raw(p, **bu.SETTINGS["full_flush"])) > len(bu.deflate_raw(p)) and all(18 + len(c) + 8 <= 0x10000 for _, c, _ in corpus())


def test_bam_exports_match_header(ffi):
    from seqlib_amd import bamio
    hdr = open(os.path.join(ROOT, "include", "seqlib_amd_bam.h")).read()
    body = hdr[hdr.index("extern \"C\""):]
    declared = set(re.findall(r"\b(slx_bam_[a-z0-9_]+)\s*\(", body))
    assert declared == set(bamio.EXPORTS), declared ^ set(bamio.EXPORTS)
    L = bamio.lib()
    for name in declared:
        assert hasattr(L, name), name
    head = hdr[:hdr.index("#ifndef")]
    for name in ("slx_bam_open", "slx_bam_next", "slx_bam_rewind", "slx_bam_close", "slx_bam_reads_device", "slx_bam_scan_members", "slx_bam_inflate_file"):
        assert name in head
    assert "SeqLib/BamReader.h:16-76" in hdr and "src/BamReader.cpp" in hdr
    # the aligner's header and binding stay as they were: the new entry points live in a header and a module of their own
    assert "slx_bam_" not in open(os.path.join(ROOT, "include", "seqlib_amd.h")).read() and not any(e.startswith("slx_bam_") for e in ffi.EXPORTS)


def test_scan_members_equals_python(ffi, tmp_path):
    from seqlib_amd import bamio
    raw = bu.bam_bytes(bu.TEXT, bu.REFS, bu.sample_records(300), member_size=0x3000)
    raw = raw[:-28] + bu.EOF_BLOCK + bu.bgzf_member(b"after the eof block in mid-file", level=0) + bu.EOF_BLOCK
    p = tmp_path / "a.bam"
    p.write_bytes(raw)
    got, eof = bamio.scan_members(p)
    want, weof = bu.scan_members(raw)
    assert got == want and eof and weof and len(got) > 10
    p.write_bytes(raw[:-28])
    assert bamio.scan_members(p) == (want[:-1], False)
    members = bu.scan_members(raw)[0]
    cases = {"truncated": raw[:members[3][0] + 100], "truncated_header": raw[:members[3][0] + 7], "bad_magic": b"\x1f\x8c" + raw[2:],
             "bad_magic_mid": raw[:members[2][0]] + b"BAM\1" + raw[members[2][0] + 4:],
             "wrong_bsize": raw[:members[1][0] + 16] + struct.pack("<H", struct.unpack_from("<H", raw, members[1][0] + 16)[0] - 9) + raw[members[1][0] + 18:],
             "tiny_bsize": raw[:16] + struct.pack("<H", 5) + raw[18:], "empty": b""}
    for name, data in cases.items():
        p.write_bytes(data)
        with pytest.raises(ffi.SlxError) as e:
            bamio.scan_members(p)
        assert e.value.code == ffi.SLX_EIO and "a.bam" in str(e.value), name
    with pytest.raises(ffi.SlxError) as e:
        bamio.scan_members(tmp_path / "missing.bam")
    assert e.value.code == ffi.SLX_EIO and "cannot open" in str(e.value)


def test_bam_no_gpu_fails_loudly(ffi, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from seqlib_amd import bamio
    p = tmp_path / "a.bam"
    p.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, bu.sample_records(20)))
    with pytest.raises(ffi.SlxError) as e:
        bamio.Reader(p)
    assert e.value.code == ffi.SLX_ENODEVICE
    with pytest.raises(ffi.SlxError) as e:
        bamio.inflate_file(p)
    assert e.value.code == ffi.SLX_ENODEVICE


def test_inflate_host_build_against_zlib(tmp_path):
    """dev_inflate.h on the host, one lane: the whole corpus byte for byte against zlib, a few thousand damaged members and the hand-made malformed streams,
    under ASan + UBSan with exactly sized buffers"""
    cfile = tmp_path / "corpus.bin"
    with open(cfile, "wb") as f:
        for _, comp, p in corpus():
            f.write(struct.pack("<II", len(comp), len(p)) + comp)
    n = len(corpus())
    exe = str(tmp_path / "inflate_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "inflate_host_test.cpp"), "-lz"])
    r = subprocess.run([exe, str(cfile), "80"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert int(last[0]) == n and int(last[2]) >= 2500 and int(last[4]) == 0, r.stdout[-2000:]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bamidx") / "bam_index_model")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-o", out, os.path.join(ROOT, "tests", "second", "bam_index_model.c")])
    return out


def run_model(model, tmp_path, stream, chunk, fail=0):
    p = tmp_path / "stream.bin"
    p.write_bytes(stream)
    r = subprocess.run([model, str(p), str(chunk), str(len(bu.REFS)), str(fail)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_index_model_equals_the_chain_walk(model, tmp_path):
    recs = bu.sample_records(3000)
    stream = b"".join(recs)
    for chunk in (65536, 4096, 1000):
        d = run_model(model, tmp_path, stream, chunk)
        assert d["same"] == 1 and d["records"] == len(recs) and d["repaired"] == 0 and d["cut"] == 0, (chunk, d)
        d = run_model(model, tmp_path, stream[:-57], chunk)                                  # the end of the batch cuts a record
        assert d["same"] == 1 and d["records"] == len(recs) - 1 and d["repaired"] == 0 and d["cut"] == 1 and d["end"] == len(stream) - len(recs[-1]), (chunk, d)
        d = run_model(model, tmp_path, stream, chunk, fail=1)                                # every guess forced wrong
        assert d["same"] == 1 and d["records"] == len(recs) and d["repaired"] == d["chunks"] - 1 > 0, (chunk, d)
    # records longer than a chunk: chunks wholly inside one guess "none"
    long_recs = [bu.bam_record("long%d" % i, 4, -1, -1, 0, [], "ACGT" * 60000, bytes([9]) * 240000) for i in range(3)]
    mixed = b"".join(recs[:50] + long_recs[:1] + recs[50:90] + long_recs[1:] + recs[90:200])
    d = run_model(model, tmp_path, mixed, 65536)
    assert d["same"] == 1 and d["records"] == 203 and d["repaired"] == 0, d
    d = run_model(model, tmp_path, mixed, 65536, fail=1)
    assert d["same"] == 1 and d["records"] == 203 and d["repaired"] > 0, d
    # the decoy: chunk 1 begins inside a B:C array that holds a chain of plausible headers
    dec = bu.decoy_records()
    d = run_model(model, tmp_path, b"".join(dec), 65536)
    assert d["same"] == 1 and d["records"] == len(dec) and d["repaired"] >= 1, d
