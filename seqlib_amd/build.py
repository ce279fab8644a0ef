"""Builds libseqlib_amd.so (HIP kernels + C-ABI) in-tree for gfx950 with hipcc."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
SO = os.path.join(HERE, "libseqlib_amd.so")
SOURCES = ["slx_index.cpp", "slx_index_gpu.hip", "slx_index_gpu64.hip", "slx_align.hip", "slx_align_wide.hip", "slx_fml.hip", "slx_fml_asm.hip", "slx_bam.hip", "slx_bai.cpp", "slx_bgzf.hip", "slx_rec.hip", "slx_sort.hip", "slx_filter.hip", "slx_fastq.hip", "slx_sam.hip", "slx_samw.hip", "slx_cov.hip", "slx_stats.hip", "slx_ref.hip", "slx_grc.hip", "slx_edit.hip", "slx_win.hip", "slx_dup.hip", "slx_pile.hip", "slx_merge.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-value",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(not os.path.exists(d) or os.path.getmtime(d) > t for d in deps)


def parse_depfile(text):
    """The files a compiler's -MMD output (Makefile format) names as prerequisites: a backslash at a line's end continues the rule, what stands before the
    rule's ':' is the target and is left out, and a backslash before a space keeps the space inside a name."""
    deps = []
    for rule in text.replace("\\\n", " ").splitlines():
        _, colon, tail = rule.partition(":")
        if colon:
            deps += [name.replace("\0", " ") for name in tail.replace("\\ ", "\0").split()]
    return deps


def stale(target, depfile):
    """True when target must be made again: it or its depfile is missing, or a file the depfile names is newer (or gone)."""
    if not os.path.exists(target) or not os.path.exists(depfile):
        return True
    with open(depfile) as f:
        return _stale(target, parse_depfile(f.read()))


def build(force=False, verbose=False):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs, procs = [], []
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    for s in SOURCES:                      # the translation units compile side by side
        src = os.path.join(CSRC, s)
        obj = os.path.join(HERE, "build", s + ".o")
        if force or stale(obj, obj + ".d"):          # the compiler writes what the object was made from beside it
            cmd = [hipcc] + FLAGS + ["-MMD", "-MF", obj + ".d", "-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            procs.append((cmd, subprocess.Popen(cmd)))
        objs.append(obj)
    for cmd, p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    if force or _stale(SO, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", SO]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    # tools/*: the C++ drop-in class timed end to end (bench.py's value_bamrecords, value_per_call); host-only code over the C-ABI (csrc is on the include path
    # for the tools whose host loops run a *_host.h themselves)
    for name in ("bamrec_bench", "percall_bench", "bamread_bench", "bamregion_bench", "bamwrite_bench", "alignbam_bench", "bamsort_bench", "bamfilter_bench", "fastq_bench", "samread_bench", "samwrite_bench", "bamcov_bench", "bamstats_bench", "refgenome_bench", "grc_bench", "bamedit_bench", "bamasm_bench", "bammarkdup_bench", "bampile_bench", "bammerge_bench"):
        tool_src = os.path.join(ROOT, "tools", name + ".cpp")
        tool = os.path.join(HERE, name)
        dep = os.path.join(HERE, "build", name + ".d")
        if force or stale(tool, dep) or _stale(tool, [SO]):
            cmd = ["g++", "-std=c++17", "-O2", "-MMD", "-MF", dep, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, tool_src, "-o", tool, "-L" + HERE, "-lseqlib_amd",
                   "-Wl,-rpath," + HERE, "-Wl,-rpath,/opt/rocm/lib", "-lz", "-lpthread"]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            subprocess.check_call(cmd)
    return SO


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
