"""k_bgzf_inflate + k_bgzf_crc on DEFLATE that zlib never writes: the valid set of tests/test_inflate_foreign.py (crafted bit by bit with tests/deflate_craft.py,
admitted by zlib, and through the host build under the sanitizers at 1, 7 and 64 lanes there) -- every member alone, all of them side by side with members
of the zlib corpus so that the four waves of a block decode different shapes and rebuild their tables at different times, and BAM records and FASTQ reads
whose members are hundreds of tiny stored and fixed blocks.  The refused set stays on the CPU."""
import os

import pytest

from tests import bam_util as bu
from tests import fastq_util
from tests.test_bam_reader import corpus
from tests.test_inflate_foreign import many_blocks_bgzf, member_of, valid_set

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bamio(sl):
    from seqlib_amd import bamio as b
    b.lib()
    return b


def test_each_crafted_member_alone(bamio, tmp_path):
    for i, e in enumerate(valid_set()):
        p = tmp_path / ("m%d.gz" % i)
        p.write_bytes(member_of(e) + bu.EOF_BLOCK)
        assert bamio.inflate_file(p) == e["payload"], e["name"]


def test_crafted_and_zlib_members_side_by_side(bamio, tmp_path):
    """crafted, zlib's and empty members interleaved in one file, one launch: forwards, then in reverse order"""
    keep = ("dyn6/bam", "fixed/bam", "huffman_only/bam", "dyn9/one_byte", "stored/text", "empty/dyn6", "empty/stored")
    zl = [(bu.member_from_deflate(c, p), p) for n, c, p in corpus() if n in keep or (n.endswith("/text") and not n.startswith("stored"))]
    assert len(zl) >= 12
    members = []
    for i, e in enumerate(valid_set()):
        members.append((member_of(e), e["payload"]))
        members.append(zl[i % len(zl)])
        if i % 3 == 1:
            members.append((bu.EOF_BLOCK, b""))
    for k, order in enumerate((members, members[::-1])):
        raw = b"".join(m for m, _ in order) + bu.EOF_BLOCK
        p = tmp_path / ("all%d.gz" % k)
        p.write_bytes(raw)
        assert bamio.scan_members(p) == bu.scan_members(raw)
        assert bamio.inflate_file(p) == bu.inflate_all(raw) == b"".join(pl for _, pl in order)


def test_records_through_members_of_many_blocks(bamio, tmp_path):
    """a BAM whose every member is some hundred stored and fixed blocks with hand-placed matches, read as records at two batch sizes"""
    recs = bu.sample_records(400)
    head = bu.bam_header(bu.TEXT, bu.REFS)
    starts = [0]
    for r in [head] + recs[:-1]:
        starts.append(starts[-1] + len(r))
    raw = many_blocks_bgzf(head + b"".join(recs), starts, 0x3000, seed=7)
    text, refs, want = bu.parse_bam(raw)
    assert (text, refs) == (bu.TEXT, bu.REFS) and [w["raw"] for w in want] == recs and len(bu.scan_members(raw)[0]) > 8
    p = tmp_path / "blocks.bam"
    p.write_bytes(raw)
    rd = bamio.Reader(p)
    assert rd.header() == (text, refs)
    for mb in (64 << 20, 5000):
        rd.rewind()
        got = []
        while True:
            batch, _ = rd.next(mb)
            if not batch:
                break
            got += batch
        assert got == [w["raw"] for w in want], mb
    rd.close()


def test_fastq_through_members_of_many_blocks(sl, golden_dir, tmp_path):
    from seqlib_amd import fastqio
    fastqio.lib()
    lines = open(os.path.join(golden_dir, "sim1_bcr.head3000.fq"), "rb").read().split(b"\n")[:800]
    text = b"\n".join(lines) + b"\n"
    starts = [0]
    for i in range(0, 796, 4):
        starts.append(starts[-1] + sum(len(l) + 1 for l in lines[i:i + 4]))
    raw = many_blocks_bgzf(text, starts, 0x3000, seed=8)
    assert bu.inflate_all(raw) == text
    want, bad = fastq_util.parse(text)
    assert len(want) == 200 and not bad
    p = tmp_path / "blocks.fq.gz"
    p.write_bytes(raw)
    with fastqio.Reader(p) as r:
        reads, _ = r.read_all(0)
        assert reads == want and r.counter("source") == 1 and r.counter("reads") == 200
