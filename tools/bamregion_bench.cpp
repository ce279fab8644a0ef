// bamregion_bench -- what the BAI index costs to build and what a region query saves, from one process and one coordinate-sorted file:
//   (a) slx_bam_index_build (the reader's pass plus the index kernels)   against a plain slx_bam_next pass over the same file: inflated GB/s of both
//   (b) one region through SetRegion + NextBatch                          against the only way to answer it without an index: NextBatch over the whole
//       file with the overlap test on the host; both times, the records found (equal, or the run fails) and the BGZF members each inflated
//   bamregion_bench <sorted.bam> [tid beg end] [reps]        (default region: reference 0, [0, 1 000 000); reps 3: median and range of every time)
// Prints one JSON line.  Built by seqlib_amd/build.py with g++ against libseqlib_amd.so.  scripts/make_bench_bam.py --sorted writes the input.  The share
// of the index kernels in (a) comes from a profiler's kernel trace of a run of this tool, not from here.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "SeqLib/BamReader.h"

using namespace SeqLib;
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct Stat { double med, lo, hi; };
static Stat stat(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return Stat{v[v.size() / 2], v.front(), v.back()};
}
// pos + reference length of the CIGAR (M D N = X), pos + 1 when that is 0 or the record is unmapped: the end the index and the region filter use
static int64_t end_of(const bam1_t *b)
{
    int64_t len = 0;
    const uint32_t *c = bam_get_cigar(b);
    for (uint32_t i = 0; i < b->core.n_cigar; ++i) if ((0x18du >> (c[i] & 15u)) & 1u) len += c[i] >> 4;
    return b->core.pos + ((b->core.flag & 4) || !len ? 1 : len);
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: bamregion_bench <sorted.bam> [tid beg end] [reps]\n"); return 2; }
    const std::string path = argv[1], bai = path + ".bai";
    const int tid = argc > 4 ? std::atoi(argv[2]) : 0;
    const int64_t beg = argc > 4 ? std::atoll(argv[3]) : 0, end = argc > 4 ? std::atoll(argv[4]) : 1000000;
    const int reps = std::max(1, argc > 5 ? std::atoi(argv[5]) : argc == 3 ? std::atoi(argv[2]) : 3);
    try {
        slx_bam_member *mem = nullptr; int64_t nm = 0;
        if (slx_bam_scan_members(path.c_str(), &mem, &nm, nullptr) != SLX_OK) { std::fprintf(stderr, "bamregion_bench: %s\n", slx_last_error()); return 1; }
        uint64_t total = 0;
        for (int64_t i = 0; i < nm; ++i) total += mem[i].isize;
        slx_bam_members_free(mem);
        // ---- (a) the plain pass, then the index build; one unmeasured pass of each first
        std::vector<double> t_plain, t_build;
        slx_bam *rd = nullptr;
        if (slx_bam_open(path.c_str(), -1, &rd) != SLX_OK) { std::fprintf(stderr, "bamregion_bench: %s\n", slx_last_error()); return 1; }
        int64_t records = 0;
        for (int rep = 0; rep < reps + 1; ++rep) {
            slx_bam_rewind(rd);
            records = 0;
            const double t0 = now();
            for (;;) {
                slx_bam_batch bt;
                if (slx_bam_next(rd, (int64_t)64 << 20, &bt) != SLX_OK) { std::fprintf(stderr, "bamregion_bench: %s\n", slx_last_error()); return 1; }
                if (!bt.n_records) break;
                records += bt.n_records;
            }
            if (rep) t_plain.push_back(now() - t0);
        }
        slx_bam_close(rd);
        for (int rep = 0; rep < reps + 1; ++rep) {
            const double t0 = now();
            if (slx_bam_index_build(path.c_str(), -1, bai.c_str()) != SLX_OK) { std::fprintf(stderr, "bamregion_bench: %s\n", slx_last_error()); return 1; }
            if (rep) t_build.push_back(now() - t0);
        }
        // ---- (b) the region: through the index, and by reading everything
        std::vector<double> t_region, t_whole;
        int64_t n_region = 0, n_whole = 0, m_region = 0, m_whole = 0;
        BamReader r;
        if (!r.Open(path) || !r.HasIndex()) { std::fprintf(stderr, "bamregion_bench: no index after the build\n"); return 1; }
        for (int rep = 0; rep < reps + 1; ++rep) {
            const int64_t m0 = r.Counter("members_done");
            const double t0 = now();
            if (!r.SetRegion(GenomicRegion(tid, (int32_t)beg, (int32_t)end))) return 1;
            n_region = 0;
            for (;;) {
                BamRecordPtrVector v;
                const size_t got = r.NextBatch(v, (size_t)1 << 20);
                if (!got) break;
                n_region += (int64_t)got;
            }
            if (rep) t_region.push_back(now() - t0);
            m_region = r.Counter("members_done") - m0;
        }
        for (int rep = 0; rep < reps + 1; ++rep) {
            r.Reset();
            const int64_t m0 = r.Counter("members_done");
            const double t0 = now();
            n_whole = 0;
            for (;;) {
                BamRecordPtrVector v;
                const size_t got = r.NextBatch(v, (size_t)1 << 20);
                if (!got) break;
                for (const BamRecordPtr &p : v) { const bam1_t *b = p->raw(); n_whole += b->core.tid == tid && b->core.pos < end && end_of(b) > beg; }
            }
            if (rep) t_whole.push_back(now() - t0);
            m_whole = r.Counter("members_done") - m0;
        }
        if (n_region != n_whole) { std::fprintf(stderr, "bamregion_bench: the region gives %lld records, the whole-file pass %lld\n", (long long)n_region, (long long)n_whole); return 1; }
        const Stat p = stat(t_plain), b = stat(t_build), q = stat(t_region), w = stat(t_whole);
        std::printf("{\"inflated_bytes\": %llu, \"members\": %lld, \"records\": %lld, \"reps\": %d, "
                    "\"plain_pass_s\": [%.4f, %.4f, %.4f], \"plain_pass_GBps\": %.3f, \"index_build_s\": [%.4f, %.4f, %.4f], \"index_build_GBps\": %.3f, \"build_over_plain\": %.3f, "
                    "\"region\": [%d, %lld, %lld], \"region_records\": %lld, \"region_s\": [%.5f, %.5f, %.5f], \"whole_file_s\": [%.5f, %.5f, %.5f], "
                    "\"region_members\": %lld, \"whole_file_members\": %lld, \"members_ratio\": %.5f, \"time_ratio\": %.4f}\n",
                    (unsigned long long)total, (long long)nm, (long long)records, reps, p.med, p.lo, p.hi, total / p.med / 1e9, b.med, b.lo, b.hi, total / b.med / 1e9, b.med / p.med,
                    tid, (long long)beg, (long long)end, (long long)n_region, q.med, q.lo, q.hi, w.med, w.lo, w.hi, (long long)m_region, (long long)m_whole,
                    m_whole ? (double)m_region / (double)m_whole : 0.0, w.med > 0 ? q.med / w.med : 0.0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bamregion_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
