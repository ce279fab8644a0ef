"""Work is taken from a device counter through seqlib_amd/csrc/dev_wave.h only.

`if (lane == 0) slot = atomicAdd(queue, 1u); slot = readfirstlane(slot);` at the head of a persistent loop has a loop-invariant
predicate: the compiler unswitched k_hits_wave's loop on it and the wave took item 0 for ever (dev_wave.h).
wave_take / wave_take_u64 / block_take compare a lane number made opaque at the call.  This is plain text matching over the
sources: no compiler, no GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "seqlib_amd", "csrc")

# if (<lane | l0 | tid | threadIdx.x | threadIdx.x & 63> == 0) [{] <lvalue> = [cast] atomicAdd(
PRED = r"\(?\s*(?:lane|l0|tid|threadIdx\.x(?:\s*&\s*63)?)\s*\)?"
TAKE = re.compile(r"if\s*\(\s*(?:\(int\))?" + PRED + r"\s*==\s*0\s*\)\s*\{?\s*[\w\.\->\[\]\*&]+\s*=\s*(?:\([\w\s\*]+\)\s*)?atomicAdd\s*\(")
HALVES = re.compile(r"readfirstlane\s*\(\s*\(int\)\s*\(.*>>\s*32\s*\)\s*\)")
RFL_DEF = re.compile(r"^[\w\s]*\brfl_u64\s*\(\s*uint64_t\s+\w+\s*\)\s*(?:\{|$)", re.M)


def _sources(with_helper):
    files = []
    for pat in ("*.h", "*.hip", "*.inc"):
        files += glob.glob(os.path.join(CSRC, pat))
    files += glob.glob(os.path.join(ROOT, "scripts", "ubench", "*.hip"))
    assert len(files) > 30 and os.path.join(CSRC, "dev_wave.h") in files
    return sorted(f for f in files if with_helper or os.path.basename(f) != "dev_wave.h")


def _hits(rx, files):
    out = []
    for f in files:
        with open(f, errors="replace") as fh:
            for n, line in enumerate(fh, 1):
                if rx.search(line):
                    out.append("%s:%d: %s" % (os.path.relpath(f, ROOT), n, line.strip()[:160]))
    return out


def test_the_patterns_match_what_they_are_meant_to():
    for bad in ("if (lane == 0) slot = (int)atomicAdd(queue, 1u);", "if (l0 == 0) slot = (int)atomicAdd(queue, 1u);",
                "if ((threadIdx.x & 63) == 0) wbase = atomicAdd(n_items, total);", "if (threadIdx.x == 0) s_job = atomicAdd(&P.cnt[3], 1u);",
                "if (tid == 0) at_s = atomicAdd(out_n, (unsigned long long)tot);", "if (threadIdx.x == 0) SB->off = atomicAdd(ck.zused, need);",
                "if (lane == 0) { at = atomicAdd(out_n, (unsigned long long)keep); n_irr[u] = (unsigned int)keep; }"):
        assert TAKE.search(bad), bad
    for good in ("if (wave_lane() == 0) pend_base = atomicAdd(queue, (unsigned int)pool);", "if (lane == 0) atomicAdd(&g_ext_stats[5], 1ull);",
                 "if (lane == 0) big_list[atomicAdd(n_big, 1u)] = (int)u;", "if (rank == 0) base = atomicAdd(ctr, (uint32_t)__popcll(m));",
                 "if (lane == (int)__ffsll((long long)m) - 1) base = atomicAdd(cursor, (u64)__popcll(m));"):
        assert not TAKE.search(good), good
    assert HALVES.search("off = ((unsigned long long)(unsigned int)__builtin_amdgcn_readfirstlane((int)(off >> 32)) << 32) |")
    assert HALVES.search("return (qp_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32 | x;")
    assert not HALVES.search("const int w = __builtin_amdgcn_readfirstlane((int)*n_slots);")


def test_no_hand_written_take_outside_dev_wave_h():
    found = _hits(TAKE, _sources(False))
    assert not found, "take work through wave_take / wave_take_u64 / block_take (dev_wave.h):\n" + "\n".join(found)


def test_rfl_u64_is_defined_once_and_the_two_halves_are_spelled_out_in_dev_wave_h_only():
    found = _hits(HALVES, _sources(False))
    assert not found, "use rfl_u64 (dev_wave.h):\n" + "\n".join(found)
    defs = []
    for f in _sources(True):
        with open(f, errors="replace") as fh:
            defs += [os.path.basename(f)] * len(RFL_DEF.findall(fh.read()))
    assert defs == ["dev_wave.h"], defs
