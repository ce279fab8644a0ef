"""Create and free of every unit built on the shared device context (csrc/slx_hip.h SlxGpu), on a machine without a GPU: cov, stats and grc give a host-only handle whose
kernel entry points answer SLX_ENODEVICE with the unit's own sentence, every other unit's create or open answers SLX_ENODEVICE, and after every free the two tallies of
slx_hip_live_bytes are what they were before.  With a GPU tests/test_gpu_handle_life.py runs the same handles over batches."""
import os

import pytest

from seqlib_amd import _ffi
from tests import bam_util as bu
from tests import cov_util as cu
from tests import sam_util as su
from tests import stats_util as tu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def tallies_return():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_handle_life.py creates and frees on it")
    L = _ffi.lib()
    before = (L.slx_hip_live_bytes(0), L.slx_hip_live_bytes(1))
    yield
    assert (L.slx_hip_live_bytes(0), L.slx_hip_live_bytes(1)) == before


def enodevice(call, sentence):
    with pytest.raises(_ffi.SlxError) as e:
        call()
    assert e.value.code == _ffi.SLX_ENODEVICE and sentence in str(e.value), str(e.value)


def test_cov_host_only_handle():
    from seqlib_amd import covio
    c = covio.Coverage(cu.REFS)
    stream, off = cu.stream_of([r for _, r in cu.CASES][:8])
    for who, call in (("slx_cov_add_host", lambda: c.add_host(stream, off)), ("slx_cov_add_device", lambda: c.add_device(None, 0, None, 0)),
                      ("slx_cov_depth", lambda: c.depth(1)), ("slx_cov_regions", lambda: c.regions([(1, 0, 5)])), ("slx_cov_bedgraph", lambda: c.bedgraph("/dev/null")),
                      ("slx_cov_max", lambda: c.max()), ("slx_cov_clear", lambda: c.clear())):
        enodevice(call, who + ": no HIP device: coverage is computed on MI355X only (no CPU fallback)")
    c.close()
    enodevice(lambda: covio.Coverage(cu.REFS, device=0), "no HIP device: coverage is computed on MI355X only (no CPU fallback)")


def test_stats_host_only_handle():
    from seqlib_amd import statsio
    s = statsio.Stats()
    stream, off = tu.stream_of(tu.GOOD[:8])
    for who, call in (("slx_stats_add_host", lambda: s.add_host(stream, off)), ("slx_stats_add_device", lambda: s.add_device(None, 0, None, 0))):
        enodevice(call, who + ": no HIP device: batches are counted on MI355X only (no CPU fallback)")
    s.close()
    enodevice(lambda: statsio.Stats(device=0), "no HIP device: batches are counted on MI355X only (no CPU fallback)")


@pytest.mark.parametrize("device", ["SLX_GRC_HOST", "SLX_GRC_AUTO"])
def test_grc_host_only_handle(device):
    from seqlib_amd import grcio
    g = grcio.Collection([(0, 1, 20), (0, 10, 30), (1, 5, 6)], device=getattr(grcio, device))
    stream, off = cu.stream_of([r for _, r in cu.CASES][:8])
    for who, call in (("slx_grc_overlaps", lambda: g.overlaps([(0, 1, 2)])), ("slx_grc_count", lambda: g.count([(0, 1, 2)])), ("slx_grc_overlaps_host", lambda: g.overlaps_host(stream, off)),
                      ("slx_grc_overlaps_device", lambda: g.overlaps_device(None, 0, None, 0)), ("slx_grc_subject_counts", lambda: g.subject_counts()),
                      ("slx_grc_clear_counts", lambda: g.clear_counts())):
        enodevice(call, who + ": no HIP device: interval batches are joined on MI355X only (no CPU fallback)")
    assert len(g.merged()) == 2          # the host mirror answers
    g.close()
    enodevice(lambda: grcio.Collection([(0, 1, 2)], device=0), "no HIP device: interval batches are joined on MI355X only (no CPU fallback)")


def test_every_other_unit_refuses_to_open(tmp_path):
    from seqlib_amd import bamio, fastqio, recio, refio, samio, samwio, sortio
    bam, sam, fq, out = tmp_path / "a.bam", tmp_path / "a.sam", tmp_path / "a.fq", tmp_path / "out"
    bam.write_bytes(bu.bam_bytes(bu.TEXT, bu.REFS, bu.sample_records(8)))
    sam.write_bytes(su.sam_text(bu.TEXT, su.canonical(3)[0]))
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    for call, sentence in ((lambda: samwio.Writer(out), "the SAM writer formats on MI355X only"), (lambda: samwio.Writer(out, bgzf=True), "the SAM writer formats on MI355X only"),
                           (lambda: sortio.Sorter(), "BAM records are sorted on MI355X only"), (lambda: recio.Builder(None), "BAM records are built on MI355X only"),
                           (lambda: bamio.Writer(out), "the BGZF writer compresses on MI355X only"), (lambda: bamio.Reader(bam), "the BAM reader inflates and indexes on MI355X only"),
                           (lambda: samio.Reader(sam), "the SAM reader parses on MI355X only"), (lambda: fastqio.Reader(fq), "the FASTQ reader parses on MI355X only"),
                           (lambda: refio.Ref(os.path.join(GOLDEN, "tiny.fa")), "the reference genome parses on MI355X only")):
        enodevice(call, "no HIP device: " + sentence)
    assert not out.exists()
