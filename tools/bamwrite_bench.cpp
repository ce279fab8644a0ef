// bamwrite_bench -- what the GPU BGZF writer buys, from one process and one file.  The records of <file.bam> are read into host memory once; then, three
// runs each, alternating, median and range:
//     (a) SeqLib::BamWriter, WriteRecord per record                 zlib level 6 on the calling thread: the path UseGpu() replaces
//     (b) zlib level 1 and level 6 of the same 0xff00 blocks on the granted CPUs, one block per task (bamread_bench's yardstick, the other direction)
//     (c) SeqLib::BamWriter with UseGpu(), WriteRecords              end to end to a file
//     (d) slx_bgzf_write of the inflated stream                      the kernels alone by HIP events: us_deflate, us_crc, us_gather
// and the compressed size of each.
//   bamwrite_bench <file.bam> <scratch prefix> [reps] [max records]
// Prints one JSON line.  Built by seqlib_amd/build.py with g++ against libseqlib_amd.so.  scripts/make_bench_bam.py writes the input.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include <sys/stat.h>
#include <zlib.h>
#include "SeqLib/BWAAligner.h"
#include "SeqLib/BamReader.h"
#include "SeqLib/BamWriter.h"

using namespace SeqLib;
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static long long file_size(const std::string &p) { struct stat sb; return stat(p.c_str(), &sb) == 0 ? (long long)sb.st_size : -1; }
struct Runs {
    std::vector<double> s;
    double med() const { std::vector<double> v = s; std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
    double lo() const { return *std::min_element(s.begin(), s.end()); }
    double hi() const { return *std::max_element(s.begin(), s.end()); }
};

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: bamwrite_bench <file.bam> <scratch prefix> [reps] [max records]\n"); return 2; }
    const std::string path = argv[1], scratch = argv[2];
    const int reps = argc > 3 ? std::atoi(argv[3]) : 3;
    const size_t max_rec = argc > 4 ? (size_t)std::atoll(argv[4]) : (size_t)-1;
    try {
        // ---- the records, once
        BamReader rd;
        if (!rd.Open(path)) return 1;
        const BamHeader hdr = rd.Header();
        BamRecordPtrVector recs;
        for (;;) {
            BamRecordPtrVector v;
            const size_t got = rd.NextBatch(v, std::min<size_t>((size_t)1 << 20, max_rec - recs.size()));
            if (!got) break;
            recs.insert(recs.end(), v.begin(), v.end());
            if (recs.size() >= max_rec) break;
        }
        rd.Close();
        const std::string f_host = scratch + ".host.bam", f_gpu = scratch + ".gpu.bam", f_raw = scratch + ".raw.bam";
        Runs a, c, z1, z6, d;
        long long size_a = 0, size_c = 0, size_z1 = 0, size_z6 = 0, size_d = 0;
        double us_def = 0, us_crc = 0, us_gat = 0;
        std::vector<unsigned char> stream;
        const unsigned cpus = detail::effective_cpus();
        const size_t piece = (size_t)1 << 18;               // records per WriteRecords call
        {                                                    // (the first GPU pass sizes the buffers and loads the kernels: not timed)
            BamWriter w; w.SetHeader(hdr);
            if (!w.UseGpu() || !w.Open(f_gpu) || !w.WriteHeader()) return 1;
            BamRecordPtrVector v(recs.begin(), recs.begin() + (ptrdiff_t)std::min(recs.size(), piece));
            if (!w.WriteRecords(v) || !w.Close()) return 1;
        }
        for (int rep = 0; rep < reps; ++rep) {
            {   // (a)
                BamWriter w; w.SetHeader(hdr);
                const double t0 = now();
                if (!w.Open(f_host) || !w.WriteHeader()) return 1;
                for (const BamRecordPtr &r : recs) if (!w.WriteRecord(*r)) return 1;
                if (!w.Close()) return 1;
                a.s.push_back(now() - t0);
                size_a = file_size(f_host);
            }
            {   // (c)
                BamWriter w; w.SetHeader(hdr);
                const double t0 = now();
                if (!w.UseGpu() || !w.Open(f_gpu) || !w.WriteHeader()) return 1;
                BamRecordPtrVector v;
                for (size_t i = 0; i < recs.size(); i += piece) {
                    v.assign(recs.begin() + (ptrdiff_t)i, recs.begin() + (ptrdiff_t)std::min(recs.size(), i + piece));
                    if (!w.WriteRecords(v)) return 1;
                }
                if (!w.Close()) return 1;
                c.s.push_back(now() - t0);
                size_c = file_size(f_gpu);
            }
            if (stream.empty()) {                            // the inflated stream of the file just written, for (b) and (d)
                uint64_t n = 0;
                slx_bam_member *mem = nullptr; int64_t nm = 0; int eof = 0;
                if (slx_bam_scan_members(f_gpu.c_str(), &mem, &nm, &eof) != SLX_OK) { std::fprintf(stderr, "bamwrite_bench: %s\n", slx_last_error()); return 1; }
                uint64_t total = 0;
                for (int64_t i = 0; i < nm; ++i) total += mem[i].isize;
                slx_bam_members_free(mem);
                stream.resize(total);
                if (slx_bam_inflate_file(f_gpu.c_str(), -1, stream.data(), total, &n) != SLX_OK || n != total) { std::fprintf(stderr, "bamwrite_bench: %s\n", slx_last_error()); return 1; }
            }
            const int64_t nblk = (int64_t)((stream.size() + 0xff00 - 1) / 0xff00);
            for (int level : {1, 6}) {   // (b)
                std::atomic<int64_t> next{0};
                std::atomic<long long> bytes{0};
                const double t0 = now();
                std::vector<std::thread> th;
                for (unsigned t = 0; t < cpus; ++t)
                    th.emplace_back([&]() {
                        std::vector<unsigned char> out(0x10000);
                        z_stream zs;
                        for (;;) {
                            const int64_t i = next.fetch_add(1);
                            if (i >= nblk) break;
                            const size_t off = (size_t)i * 0xff00, len = std::min<size_t>(0xff00, stream.size() - off);
                            std::memset(&zs, 0, sizeof zs);
                            deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
                            zs.next_in = stream.data() + off; zs.avail_in = (uInt)len; zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
                            deflate(&zs, Z_FINISH);
                            bytes += (long long)zs.total_out + 26;
                            (void)crc32(crc32(0L, Z_NULL, 0), stream.data() + off, (uInt)len);
                            deflateEnd(&zs);
                        }
                    });
                for (auto &t : th) t.join();
                (level == 1 ? z1 : z6).s.push_back(now() - t0);
                (level == 1 ? size_z1 : size_z6) = bytes + 28;
            }
            {   // (d)
                slx_bgzf *w = nullptr;
                if (slx_bgzf_open(f_raw.c_str(), -1, &w) != SLX_OK) { std::fprintf(stderr, "bamwrite_bench: %s\n", slx_last_error()); return 1; }
                const double t0 = now();
                if (slx_bgzf_write(w, stream.data(), (int64_t)stream.size()) != SLX_OK || slx_bgzf_flush(w) != SLX_OK) { std::fprintf(stderr, "bamwrite_bench: %s\n", slx_last_error()); return 1; }
                us_def = (double)slx_bgzf_counter(w, "us_deflate"); us_crc = (double)slx_bgzf_counter(w, "us_crc"); us_gat = (double)slx_bgzf_counter(w, "us_gather");
                if (slx_bgzf_close(w) != SLX_OK) { std::fprintf(stderr, "bamwrite_bench: %s\n", slx_last_error()); return 1; }
                d.s.push_back(now() - t0);
                size_d = file_size(f_raw);
            }
        }
        std::remove(f_host.c_str()); std::remove(f_gpu.c_str()); std::remove(f_raw.c_str());
        const double B = (double)stream.size();
        std::printf("{\"records\": %zu, \"stream_bytes\": %zu, \"cpus\": %u, \"reps\": %d, "
                    "\"host_writer_s\": [%.3f, %.3f, %.3f], \"host_writer_GBps\": %.4f, \"host_writer_bytes\": %lld, "
                    "\"zlib1_s\": [%.3f, %.3f, %.3f], \"zlib1_GBps\": %.3f, \"zlib1_bytes\": %lld, "
                    "\"zlib6_s\": [%.3f, %.3f, %.3f], \"zlib6_GBps\": %.3f, \"zlib6_bytes\": %lld, "
                    "\"gpu_writer_s\": [%.3f, %.3f, %.3f], \"gpu_writer_GBps\": %.3f, \"gpu_writer_bytes\": %lld, "
                    "\"gpu_stream_s\": [%.3f, %.3f, %.3f], \"gpu_stream_GBps\": %.3f, \"gpu_stream_bytes\": %lld, "
                    "\"us_deflate\": %.0f, \"us_crc\": %.0f, \"us_gather\": %.0f, \"deflate_kernel_GBps\": %.3f, \"kernels_GBps\": %.3f, "
                    "\"gpu_vs_host_writer\": %.2f, \"gpu_vs_zlib1\": %.2f, \"gpu_vs_zlib6\": %.2f, \"gpu_size_over_zlib1\": %.4f, \"gpu_size_over_zlib6\": %.4f, \"gate_c_beats_a\": %s}\n",
                    recs.size(), stream.size(), cpus, reps,
                    a.lo(), a.med(), a.hi(), B / a.med() / 1e9, size_a,
                    z1.lo(), z1.med(), z1.hi(), B / z1.med() / 1e9, size_z1,
                    z6.lo(), z6.med(), z6.hi(), B / z6.med() / 1e9, size_z6,
                    c.lo(), c.med(), c.hi(), B / c.med() / 1e9, size_c,
                    d.lo(), d.med(), d.hi(), B / d.med() / 1e9, size_d,
                    us_def, us_crc, us_gat, us_def > 0 ? B / (us_def * 1e-6) / 1e9 : 0.0, us_def + us_crc + us_gat > 0 ? B / ((us_def + us_crc + us_gat) * 1e-6) / 1e9 : 0.0,
                    a.med() / c.med(), z1.med() / c.med(), z6.med() / c.med(), (double)size_c / (double)size_z1, (double)size_c / (double)size_z6,
                    c.hi() < a.lo() ? "true" : "false");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bamwrite_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
