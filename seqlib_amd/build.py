"""Builds libseqlib_amd.so (HIP kernels + C-ABI) in-tree for gfx950 with hipcc."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
SO = os.path.join(HERE, "libseqlib_amd.so")
SOURCES = ["slx_index.cpp", "slx_index_gpu.hip", "slx_index_gpu64.hip", "slx_align.hip", "slx_align_wide.hip", "slx_fml.hip", "slx_fml_asm.hip", "slx_bam.hip", "slx_bai.cpp", "slx_bgzf.hip", "slx_rec.hip", "slx_sort.hip", "slx_filter.hip", "slx_fastq.hip", "slx_sam.hip", "slx_samw.hip", "slx_cov.hip", "slx_stats.hip", "slx_ref.hip", "slx_grc.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-value",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # two groups of translation units with their own headers: the BWAAligner path, and the FermiAssembler / BFC path (slx_fml*)
    is_fml = lambda f: "fml" in f
    is_bam = lambda f: f in ("slx_bam.hip", "slx_bai.cpp", "slx_bgzf.hip", "slx_rec.hip", "slx_sort.hip", "slx_filter.hip", "slx_fastq.hip", "slx_sam.hip", "slx_samw.hip", "slx_cov.hip", "slx_stats.hip", "slx_ref.hip", "slx_grc.hip", "dev_grc.h", "grc_host.h", "dev_ref.h", "ref_host.h", "dev_stats.h", "stats_host.h", "dev_cov.h", "cov_host.h", "dev_fastq.h", "fq_host.h", "fq_text.h", "dev_sam.h", "sam_host.h", "sam_reader.h", "dev_samw.h", "samw_host.h", "dev_rfilter.h", "rfilter_host.h", "dev_inflate.h", "dev_deflate.h", "dev_bamidx.h", "dev_bai.h", "bai_host.h", "dev_rec.h", "dev_recsort.h", "recsort_host.h")          # the BamReader / BamWriter path (slx_bam.hip, slx_bgzf.hip, slx_rec.hip, slx_sort.hip, slx_filter.hip, slx_fastq.hip, slx_sam.hip, slx_samw.hip, slx_cov.hip, slx_stats.hip, slx_ref.hip, slx_grc.hip), a third group
    hdr_align = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc")) and not is_fml(f) and not is_bam(f)] + [os.path.join(ROOT, "include", "seqlib_amd.h")]
    hdr_bam = [os.path.join(CSRC, f) for f in ("dev_inflate.h", "dev_deflate.h", "dev_bamidx.h", "dev_bai.h", "bai_host.h", "dev_rec.h", "dev_recsort.h", "recsort_host.h", "dev_rfilter.h", "rfilter_host.h", "dev_fastq.h", "fq_host.h", "fq_text.h", "dev_sam.h", "sam_host.h", "sam_reader.h", "dev_samw.h", "samw_host.h", "dev_cov.h", "cov_host.h", "dev_stats.h", "stats_host.h", "dev_ref.h", "ref_host.h", "dev_grc.h", "grc_host.h", "dev_wave.h", "slx_internal.h", "slx_hip.h")] + [os.path.join(ROOT, "include", f) for f in ("seqlib_amd.h", "seqlib_amd_bam.h", "seqlib_amd_rec.h", "seqlib_amd_sort.h", "seqlib_amd_filter.h", "seqlib_amd_fastq.h", "seqlib_amd_sam.h", "seqlib_amd_samw.h", "seqlib_amd_cov.h", "seqlib_amd_stats.h", "seqlib_amd_ref.h", "seqlib_amd_grc.h")]
    hdr_fml = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h") and is_fml(f)] + \
              [os.path.join(CSRC, "slx_internal.h"), os.path.join(CSRC, "slx_hip.h"), os.path.join(CSRC, "dev_wave.h"), os.path.join(ROOT, "include", "seqlib_amd.h"), os.path.join(ROOT, "include", "seqlib_amd_fml.h")]
    objs, procs = [], []
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    for s in SOURCES:                      # the translation units compile side by side
        src = os.path.join(CSRC, s)
        obj = os.path.join(HERE, "build", s + ".o")
        if force or _stale(obj, [src] + (hdr_fml if is_fml(s) else hdr_bam if is_bam(s) else hdr_align)):
            cmd = [hipcc] + FLAGS + ["-c", src, "-o", obj]
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
    # tools/*: the C++ drop-in class timed end to end (bench.py's value_bamrecords, value_per_call); host-only code over the C-ABI (csrc is on the include path for
    # samread_bench, which times sam_host.h, the host parser, itself, refgenome_bench, whose host loops run ref_host.h, and grc_bench, whose host loops run grc_host.h)
    hdrs = [os.path.join(ROOT, "include", "SeqLib", f) for f in os.listdir(os.path.join(ROOT, "include", "SeqLib"))]
    for name in ("bamrec_bench", "percall_bench", "bamread_bench", "bamregion_bench", "bamwrite_bench", "alignbam_bench", "bamsort_bench", "bamfilter_bench", "fastq_bench", "samread_bench", "samwrite_bench", "bamcov_bench", "bamstats_bench", "refgenome_bench", "grc_bench"):
        tool_src = os.path.join(ROOT, "tools", name + ".cpp")
        tool = os.path.join(HERE, name)
        if force or _stale(tool, [tool_src, SO] + hdrs + ([os.path.join(CSRC, "sam_host.h"), os.path.join(CSRC, "dev_sam.h")] if name == "samread_bench" else [os.path.join(CSRC, "ref_host.h"), os.path.join(CSRC, "dev_ref.h")] if name == "refgenome_bench" else [os.path.join(CSRC, "grc_host.h"), os.path.join(CSRC, "dev_rfilter.h")] if name == "grc_bench" else [])):
            cmd = ["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, tool_src, "-o", tool, "-L" + HERE, "-lseqlib_amd",
                   "-Wl,-rpath," + HERE, "-Wl,-rpath,/opt/rocm/lib", "-lz", "-lpthread"]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            subprocess.check_call(cmd)
    return SO


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
