// fastq_bench -- what parsing FASTQ on the GPU buys, from one process and one input file (plain, bgzip'd or gzip'd; scripts/make_bench_fastq.py writes all three):
//     (a) the `while (r.GetNextSequence(s))` loop of SeqLib::FastqReader: one host thread, zlib, a byte at a time
//     (b) slx_fastq_next over the file: batches left in HBM, with the kernel times of the reader's counters
// and, with an index, FASTQ -> BAM through a UseGpu() writer:
//     (c) GetNextSequence into a vector, then alignToBam(vector)
//     (d) alignToBam(FastqReader&): nothing per read on the host
// Each route `reps` times, alternating, median and range.  (c) and (d) must write files of the same size.
//   fastq_bench <reads.fq[.gz]> [reps] [batch_bytes] [index prefix] [scratch prefix]
// Prints one JSON line.  Built by seqlib_amd/build.py with g++ against libseqlib_amd.so.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include <sys/stat.h>
#include "SeqLib/BWAAligner.h"
#include "SeqLib/BamWriter.h"
#include "SeqLib/FastqReader.h"

using namespace SeqLib;
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static long long file_size(const std::string &p) { struct stat sb; return stat(p.c_str(), &sb) == 0 ? (long long)sb.st_size : -1; }
struct Runs {
    std::vector<double> s;
    double med() const { if (s.empty()) return 0; std::vector<double> v = s; std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
    double lo() const { return s.empty() ? 0 : *std::min_element(s.begin(), s.end()); }
    double hi() const { return s.empty() ? 0 : *std::max_element(s.begin(), s.end()); }
};

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: fastq_bench <reads.fq[.gz]> [reps] [batch_bytes] [index prefix] [scratch prefix]\n"); return 2; }
    const std::string input = argv[1];
    const int reps = argc > 2 ? std::max(1, std::atoi(argv[2])) : 3;
    const int64_t batch_bytes = argc > 3 ? std::atoll(argv[3]) : 0;
    const bool align = argc > 5;
    try {
        Runs run[4];
        size_t n_host = 0, n_dev = 0, rec_c = 0, rec_d = 0;
        int64_t text_bytes = 0, c[8] = {0};
        long long size_c = 0, size_d = 0;
        slx_fastq *fq = nullptr;
        if (slx_fastq_open(input.c_str(), -1, &fq) != 0) throw std::runtime_error(slx_last_error());
        auto host_loop = [&]() {
            FastqReader r;
            if (!r.Open(input)) throw std::runtime_error("cannot open " + input);
            UnalignedSequence s;
            size_t n = 0;
            while (r.GetNextSequence(s)) ++n;
            n_host = n;
        };
        auto dev_loop = [&]() {
            if (slx_fastq_rewind(fq) != 0) throw std::runtime_error(slx_last_error());
            slx_fastq_batch b;
            size_t n = 0;
            int64_t t = 0;
            for (;;) {
                if (slx_fastq_next(fq, batch_bytes, &b) != 0) throw std::runtime_error(slx_last_error());
                if (b.n_reads == 0) break;
                n += (size_t)b.n_reads; t += b.n_text_bytes;
            }
            n_dev = n; text_bytes = t;
            const char *names[8] = {"fast_reads", "slow_reads", "batches", "source", "us_lines", "us_check", "us_gather", "us_inflate"};
            for (int i = 0; i < 8; ++i) c[i] = slx_fastq_counter(fq, names[i]);
        };
        dev_loop();                                           // (the first pass sizes the buffers and loads the kernels: not timed)
        for (int rep = 0; rep < reps; ++rep) {
            double t0 = now(); host_loop(); run[0].s.push_back(now() - t0);
            t0 = now(); dev_loop(); run[1].s.push_back(now() - t0);
        }
        slx_fastq_close(fq);
        if (align) {
            BWAIndexPtr idx = std::make_shared<BWAIndex>();
            idx->LoadIndex(argv[4]);
            BWAAligner al(idx);
            const BamHeader hdr = idx->HeaderFromIndex();
            const std::string out_c = std::string(argv[5]) + ".c.bam", out_d = std::string(argv[5]) + ".d.bam";
            auto route = [&](bool dev) {
                BamWriter w; w.SetHeader(hdr);
                const std::string &out = dev ? out_d : out_c;
                if (!w.UseGpu() || !w.Open(out) || !w.WriteHeader()) throw std::runtime_error("cannot open " + out);
                FastqReader r;
                if (!r.Open(input)) throw std::runtime_error("cannot open " + input);
                if (dev) rec_d = al.alignToBam(r, w, false, 0.9, 10, batch_bytes > 0 ? (size_t)batch_bytes : (size_t)64 << 20);
                else {
                    UnalignedSequenceVector reads;
                    UnalignedSequence s;
                    while (r.GetNextSequence(s)) reads.push_back(s);
                    rec_c = al.alignToBam(reads, w, false, 0.9, 10);
                }
                if (!w.Close()) throw std::runtime_error("Close failed");
            };
            srand48(11);
            route(true);                                      // warm-up, not timed
            for (int rep = 0; rep < reps; ++rep)
                for (int d = 0; d < 2; ++d) {
                    srand48(11);
                    const double t0 = now();
                    route(d != 0);
                    run[2 + d].s.push_back(now() - t0);
                }
            size_c = file_size(out_c); size_d = file_size(out_d);
            std::remove(out_c.c_str()); std::remove(out_d.c_str());
        }
        auto rate = [&](const Runs &r, size_t n) { return r.s.empty() || r.med() <= 0 ? 0.0 : (double)n / r.med() / 1e6; };
        std::printf("{\"input\": \"%s\", \"file_bytes\": %lld, \"text_bytes\": %lld, \"source\": %lld, \"reads\": %zu, \"reads_host_loop\": %zu, \"reps\": %d, \"batch_bytes\": %lld, "
                    "\"a_get_next_sequence_s\": [%.4f, %.4f, %.4f], \"a_Mreads_s\": %.3f, "
                    "\"b_slx_fastq_next_s\": [%.4f, %.4f, %.4f], \"b_Mreads_s\": %.3f, \"b_text_GB_s\": %.3f, \"b_over_a\": %.2f, "
                    "\"fast_reads\": %lld, \"slow_reads\": %lld, \"batches\": %lld, \"us_lines\": %lld, \"us_check\": %lld, \"us_gather\": %lld, \"us_inflate\": %lld",
                    input.c_str(), file_size(input), (long long)text_bytes, (long long)c[3], n_dev, n_host, reps, (long long)batch_bytes,
                    run[0].lo(), run[0].med(), run[0].hi(), rate(run[0], n_host), run[1].lo(), run[1].med(), run[1].hi(), rate(run[1], n_dev),
                    run[1].med() > 0 ? (double)text_bytes / run[1].med() / 1e9 : 0.0, run[1].med() > 0 ? run[0].med() / run[1].med() : 0.0,
                    (long long)c[0], (long long)c[1], (long long)c[2], (long long)c[4], (long long)c[5], (long long)c[6], (long long)c[7]);
        if (align)
            std::printf(", \"c_per_read_then_align_to_bam_s\": [%.3f, %.3f, %.3f], \"c_Mreads_s\": %.3f, \"d_align_to_bam_fastq_reader_s\": [%.3f, %.3f, %.3f], \"d_Mreads_s\": %.3f, "
                        "\"d_over_c\": %.2f, \"records\": [%zu, %zu], \"files_identical_size\": %s",
                        run[2].lo(), run[2].med(), run[2].hi(), rate(run[2], n_host), run[3].lo(), run[3].med(), run[3].hi(), rate(run[3], n_dev),
                        run[3].med() > 0 ? run[2].med() / run[3].med() : 0.0, rec_c, rec_d, size_c == size_d ? "true" : "false");
        std::printf("}\n");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "fastq_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
