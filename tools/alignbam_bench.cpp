// alignbam_bench -- what building the records on the GPU buys a caller who wants a BAM file, from one process and one input.  The input is aligned to BAM by
// three routes, `reps` times each, alternating, median and range:
//     (a) alignSequences + SeqLib::BamWriter, WriteRecords          records on the host, zlib level 6 on the calling thread
//     (b) alignSequences + BamWriter with UseGpu(), WriteRecords    records on the host, serialised and copied up, BGZF on the GPU: the path as it stood
//     (c) alignToBam through a UseGpu() writer                      records built in HBM (slx_rec_build), nothing comes down but the file
// Per route: reads/s, the process's CPU seconds (user + system, all threads), and for (c) the builder's us_size / us_fill next to the writer's us_deflate.
//   alignbam_bench <index prefix> <reads.fq | reads.bam> <scratch prefix> [reps] [max reads] [skip_a]
// A BAM input (scripts/make_bench_bam.py) goes through the BamReader forms, a FASTQ through the vector forms.  skip_a = 1 leaves route (a) out (zlib on one
// thread takes minutes on millions of reads).  Prints one JSON line.  Built by seqlib_amd/build.py with g++ against libseqlib_amd.so.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <sys/resource.h>
#include <sys/stat.h>
#include "SeqLib/BWAAligner.h"
#include "SeqLib/BamReader.h"
#include "SeqLib/BamWriter.h"
#include "SeqLib/FastqReader.h"

using namespace SeqLib;
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static double cpu_now()
{
    struct rusage ru;
    getrusage(RUSAGE_SELF, &ru);
    return (double)ru.ru_utime.tv_sec + ru.ru_utime.tv_usec * 1e-6 + (double)ru.ru_stime.tv_sec + ru.ru_stime.tv_usec * 1e-6;
}
static long long file_size(const std::string &p) { struct stat sb; return stat(p.c_str(), &sb) == 0 ? (long long)sb.st_size : -1; }
struct Runs {
    std::vector<double> s, cpu;
    double med(const std::vector<double> &x) const { if (x.empty()) return 0; std::vector<double> v = x; std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
    double lo() const { return s.empty() ? 0 : *std::min_element(s.begin(), s.end()); }
    double hi() const { return s.empty() ? 0 : *std::max_element(s.begin(), s.end()); }
};

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: alignbam_bench <index prefix> <reads.fq | reads.bam> <scratch prefix> [reps] [max reads] [skip_a]\n"); return 2; }
    const std::string input = argv[2], scratch = argv[3];
    const int reps = argc > 4 ? std::atoi(argv[4]) : 3;
    const size_t max_reads = argc > 5 && std::atoll(argv[5]) > 0 ? (size_t)std::atoll(argv[5]) : (size_t)-1;
    const bool skip_a = argc > 6 && std::atoi(argv[6]) != 0;
    const bool from_bam = input.size() > 4 && input.compare(input.size() - 4, 4, ".bam") == 0;
    try {
        BWAIndexPtr idx = std::make_shared<BWAIndex>();
        idx->LoadIndex(argv[1]);
        BWAAligner al(idx);
        const BamHeader hdr = idx->HeaderFromIndex();
        UnalignedSequenceVector reads;
        if (!from_bam) {
            FastqReader fr(input);
            UnalignedSequence s;
            while (reads.size() < max_reads && fr.GetNextSequence(s)) reads.push_back(s);
        }
        size_t n_reads = reads.size(), n_records[3] = {0, 0, 0};
        const std::string out[3] = {scratch + ".a.bam", scratch + ".b.bam", scratch + ".c.bam"};
        Runs run[3];
        long long size[3] = {0, 0, 0};
        double us_deflate[3] = {0, 0, 0}, us_size = 0, us_fill = 0;
        // routes (a) and (b): the records on the host, written vector by vector in pieces of 2^18 records
        auto host_route = [&](int route) {
            BamWriter w; w.SetHeader(hdr);
            if (route == 1 && !w.UseGpu()) throw std::runtime_error("UseGpu failed");
            if (!w.Open(out[route]) || !w.WriteHeader()) throw std::runtime_error("cannot open " + out[route]);
            std::vector<BamRecordPtrVector> res;
            if (from_bam) {
                BamReader r;
                if (!r.Open(input)) throw std::runtime_error("cannot open " + input);
                al.alignSequences(r, res, false, 0.9, 10);
                n_reads = res.size();
            } else al.alignSequences(reads, res, false, 0.9, 10);
            BamRecordPtrVector piece;
            size_t n = 0;
            for (auto &v : res) {
                piece.insert(piece.end(), v.begin(), v.end());
                if (piece.size() >= ((size_t)1 << 18)) { if (!w.WriteRecords(piece)) throw std::runtime_error("WriteRecords failed"); n += piece.size(); piece.clear(); }
            }
            if (!w.WriteRecords(piece)) throw std::runtime_error("WriteRecords failed");
            n += piece.size();
            if (route == 1) us_deflate[1] = (double)w.GpuCounter("us_deflate");
            if (!w.Close()) throw std::runtime_error("Close failed");
            n_records[route] = n;
        };
        auto gpu_route = [&]() {
            BamWriter w; w.SetHeader(hdr);
            if (!w.UseGpu() || !w.Open(out[2]) || !w.WriteHeader()) throw std::runtime_error("cannot open " + out[2]);
            const double s0 = (double)al.RecordBuilderCounter("us_size"), f0 = (double)al.RecordBuilderCounter("us_fill");
            if (from_bam) {
                BamReader r;
                if (!r.Open(input)) throw std::runtime_error("cannot open " + input);
                n_records[2] = al.alignToBam(r, w, false, 0.9, 10);
            } else n_records[2] = al.alignToBam(reads, w, false, 0.9, 10);
            us_size = (double)al.RecordBuilderCounter("us_size") - std::max(0.0, s0); us_fill = (double)al.RecordBuilderCounter("us_fill") - std::max(0.0, f0);
            us_deflate[2] = (double)w.GpuCounter("us_deflate");
            if (!w.Close()) throw std::runtime_error("Close failed");
        };
        srand48(11);
        gpu_route();                                          // (the first pass sizes the buffers and loads the kernels: not timed)
        for (int rep = 0; rep < reps; ++rep)
            for (int route = skip_a ? 1 : 0; route < 3; ++route) {
                srand48(11);
                const double t0 = now(), c0 = cpu_now();
                if (route < 2) host_route(route); else gpu_route();
                run[route].s.push_back(now() - t0); run[route].cpu.push_back(cpu_now() - c0);
                size[route] = file_size(out[route]);
            }
        for (const std::string &f : out) std::remove(f.c_str());
        const double R = (double)n_reads;
        auto rate = [&](const Runs &r) { return r.s.empty() ? 0.0 : R / r.med(r.s) / 1e6; };
        const double M = (double)n_records[2] / 1e6;
        std::printf("{\"input\": \"%s\", \"reads\": %zu, \"records\": [%zu, %zu, %zu], \"cpus\": %u, \"reps\": %d, "
                    "\"a_host_zlib_s\": [%.3f, %.3f, %.3f], \"a_Mreads_s\": %.3f, \"a_cpu_s\": %.2f, \"a_bytes\": %lld, "
                    "\"b_host_records_gpu_bgzf_s\": [%.3f, %.3f, %.3f], \"b_Mreads_s\": %.3f, \"b_cpu_s\": %.2f, \"b_bytes\": %lld, \"b_us_deflate\": %.0f, "
                    "\"c_align_to_bam_s\": [%.3f, %.3f, %.3f], \"c_Mreads_s\": %.3f, \"c_cpu_s\": %.2f, \"c_bytes\": %lld, \"c_us_deflate\": %.0f, "
                    "\"c_us_size\": %.0f, \"c_us_fill\": %.0f, \"c_us_size_fill_per_M_records\": %.0f, \"c_over_b\": %.3f, \"b_cpu_over_c_cpu\": %.2f, \"files_identical_size\": %s}\n",
                    from_bam ? "bam" : "fastq", n_reads, n_records[0], n_records[1], n_records[2], detail::effective_cpus(), reps,
                    run[0].lo(), run[0].med(run[0].s), run[0].hi(), rate(run[0]), run[0].med(run[0].cpu), size[0],
                    run[1].lo(), run[1].med(run[1].s), run[1].hi(), rate(run[1]), run[1].med(run[1].cpu), size[1], us_deflate[1],
                    run[2].lo(), run[2].med(run[2].s), run[2].hi(), rate(run[2]), run[2].med(run[2].cpu), size[2], us_deflate[2],
                    us_size, us_fill, M > 0 ? (us_size + us_fill) / M : 0.0, run[1].med(run[1].s) / run[2].med(run[2].s),
                    run[2].med(run[2].cpu) > 0 ? run[1].med(run[1].cpu) / run[2].med(run[2].cpu) : 0.0, size[1] == size[2] ? "true" : "false");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "alignbam_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
