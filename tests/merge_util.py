"""What a merge of coordinate-sorted BAM files must give, in plain Python, written from the rules of include/seqlib_amd_merge.h: the expected order, the header rule,
the inputs the tests merge and the run count of a spilling sort.  No GPU, no library."""
import struct

from tests import bam_util as bu

N_TIES = 130
TIE_AT = (1, 4242)          # a block of 130 records at one key, dealt over the inputs: more than a wave
N_BLOCK = 400
BLOCK_AT = (2, 5000)        # a block of 400 records at one key inside ONE input: more than a batch of 0x2000 bytes, so a round emits nothing and refills


def key(rec):
    refid, pos = struct.unpack_from("<ii", rec, 4)
    return (refid & 0xffffffff, pos)


def expected_merge(inputs):
    """inputs: [[record bytes]] in add order -> ([records in merged order], [the input each came from]).  Python's sort is stable: ties go by input, then by
    position inside the input."""
    flat = [(r, i) for i, recs in enumerate(inputs) for r in recs]
    flat.sort(key=lambda x: key(x[0]))
    return [r for r, _ in flat], [i for _, i in flat]


# ---------------------------------------------------------------- the header rule
def header_so(text):
    """the sorter's rule: SO:coordinate in the @HD line, which is made when there is none"""
    if not (text.startswith("@HD") and (len(text) == 3 or text[3] in "\t\n")):
        return "@HD\tVN:1.6\tSO:coordinate\n" + text
    eol = text.find("\n")
    eol = len(text) if eol < 0 else eol
    fields = text[:eol].split("\t")
    for i in range(1, len(fields)):
        if fields[i].startswith("SO:"):
            fields[i] = "SO:coordinate"
            return "\t".join(fields) + text[eol:]
    return text[:eol] + "\tSO:coordinate" + text[eol:]


class IdClash(Exception):
    pass


def _lines(text):
    v = text.split("\n")
    return v[:-1] if text.endswith("\n") or not text else v


def _line_id(line):
    for f in line.split("\t")[1:]:
        if f.startswith("ID:"):
            return f[3:]
    return ""


def header_rule(texts):
    """input 0's text with SO:coordinate; then from inputs 1.., in order, every @RG, @PG or @CO line not byte-identical to a line already present; an @RG or @PG
    whose ID: a different line of its kind already carries raises IdClash(ID); @HD, @SQ and anything else of a later input is dropped"""
    if not texts:
        return ""
    text = header_so(texts[0])
    have = _lines(text)
    for t in texts[1:]:
        for ln in _lines(t):
            kind = ln[:3]
            if kind not in ("@RG", "@PG", "@CO") or (len(ln) > 3 and ln[3] != "\t") or ln in have:
                continue
            if kind != "@CO" and any(h[:3] == kind and _line_id(h) == _line_id(ln) for h in have):
                raise IdClash(_line_id(ln))
            if text and not text.endswith("\n"):
                text += "\n"
            text += ln + "\n"
            have.append(ln)
    return text


SQ = "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in bu.REFS)
HD = "@HD\tVN:1.6\tSO:unsorted\n"
# name -> (texts, expected text or IdClash)
HEADER_CASES = {
    "identical inputs": ([bu.TEXT, bu.TEXT, bu.TEXT], bu.TEXT.replace("SO:unsorted", "SO:coordinate")),
    "a new @RG": ([HD + SQ + "@RG\tID:a\tSM:s\n", HD + SQ + "@RG\tID:b\tSM:s\n@PG\tID:p\tPN:x\n"],
                  "@HD\tVN:1.6\tSO:coordinate\n" + SQ + "@RG\tID:a\tSM:s\n@RG\tID:b\tSM:s\n@PG\tID:p\tPN:x\n"),
    "the same line twice": ([HD + SQ + "@CO\tone\n", HD + SQ + "@CO\ttwo\n@CO\tone\n", SQ + "@CO\ttwo\n@RG\tID:r\n", SQ + "@RG\tID:r\n"],
                            "@HD\tVN:1.6\tSO:coordinate\n" + SQ + "@CO\tone\n@CO\ttwo\n@RG\tID:r\n"),
    "an ID clash": ([HD + SQ + "@RG\tID:a\tSM:one\n", HD + SQ + "@RG\tID:a\tSM:two\n"], IdClash),
    "a @PG clash": ([SQ + "@PG\tID:bwa\tVN:1\n", SQ + "@RG\tID:bwa\n@PG\tID:bwa\tVN:2\n"], IdClash),
    "no @HD": ([SQ + "@RG\tID:a\n", "@HD\tVN:1.0\tSO:queryname\n@SQ\tSN:other\tLN:9\n@CO\tlater\n"], "@HD\tVN:1.6\tSO:coordinate\n" + SQ + "@RG\tID:a\n@CO\tlater\n"),
    "no newline at the end": (["@HD\tVN:1.4", "@CO\tc"], "@HD\tVN:1.4\tSO:coordinate\n@CO\tc\n"),
    "one input": ([HD + SQ], "@HD\tVN:1.6\tSO:coordinate\n" + SQ),
}


# ---------------------------------------------------------------- the inputs
def base_records():
    """the records of tests/test_gpu_sort.py: bu.sample_records(400) with, scattered through it, 130 records at one (tid, pos) with alternating strand flags; a
    record at pos -1 on tid 0, one of 10 000 bytes and the 38-byte one.  Unsorted."""
    recs = list(bu.sample_records(400))
    ties = [bu.bam_record("tie%03d" % i, 0x10 if i % 2 else 0, TIE_AT[0], TIE_AT[1], 30, [("M", 20)], "ACGTA" * 4, bytes([30]) * 20) for i in range(N_TIES)]
    for i, t in enumerate(ties):
        recs.insert(5 + 4 * i, t)
    recs.insert(17, bu.bam_record("minus_one", 0, 0, -1, 11, [("M", 20)], "ACGTA" * 4, bytes([30]) * 20))
    bare = len(bu.bam_record("big", 0, 2, 77, 9, [("M", 100)], "ACGT" * 25, bytes([33]) * 100))
    big = bu.bam_record("big", 0, 2, 77, 9, [("M", 100)], "ACGT" * 25, bytes([33]) * 100, b"XZZ" + b"x" * (10000 - bare - 4) + b"\0")
    assert len(big) == 10000
    recs.insert(301, big)
    tiny = bu.bam_record("a", 4, -1, -1, 0, [], "", b"")
    assert len(tiny) == 38
    recs.insert(99, tiny)
    return recs


def block_records():
    return [bu.bam_record("blk%03d" % i, 0, BLOCK_AT[0], BLOCK_AT[1], 40, [("M", 20)], "TTGCA" * 4, bytes([20 + i % 20]) * 20) for i in range(N_BLOCK)]


def build_inputs(k, records=None, block_in=None):
    """the records sorted, then dealt to k inputs: record j of the sorted list goes to input (7 * j) % k.  block_in: the 400-record block goes into that one
    input, at its place.  Every input is sorted."""
    recs = sorted(base_records() if records is None else records, key=key)
    inputs = [[] for _ in range(k)]
    for j, r in enumerate(recs):
        inputs[(7 * j) % k].append(r)
    if block_in is not None:
        inputs[block_in] = sorted(inputs[block_in] + block_records(), key=key)
    for v in inputs:
        assert v == sorted(v, key=key)
    return inputs


def expected_runs(add_sizes, max_bytes):
    """how many run files a spilling sorter writes for adds of these byte sizes: an add that would pass max_bytes while something is held spills what is held
    first; what is held at the end is the last run, if any run was spilled before.  None: an add alone is beyond max_bytes (refused)."""
    held, runs = 0, 0
    for n in add_sizes:
        if n > max_bytes:
            return None
        if held and held + n > max_bytes:
            runs += 1
            held = 0
        held += n
    return runs + 1 if runs and held else runs
