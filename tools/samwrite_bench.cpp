// samwrite_bench -- what the GPU SAM writer buys, against the host writer on one thread of the same machine, from one process and one file:
//     (a) in.bam -> BamReader::GetNextRecord -> BamWriter(SAM)::WriteRecord -> <work dir>/host.sam, and the same to /dev/null        format_sam, one record at a time
//     (b) in.bam -> slx_bam_next batches in HBM -> BamWriter(SAM) + UseGpuSam()::WriteDevice -> <work dir>/gpu.sam, and to /dev/null  slx_samw_*: formatted on the GPU
//   samwrite_bench <in.bam> <work dir> [reps]
// The two files are compared byte for byte first.  In (a) the clock runs over reading and writing, and the reading alone (the same loop without the writer) is
// timed beside it, so that the writer's own share is visible; in (b) the kernel time comes from the writer's counters (HIP events).  Prints one JSON line per
// batch size.  Built by seqlib_amd/build.py with g++ against libseqlib_amd.so.  scripts/make_bench_bam.py writes in.bam.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/BamWriter.h"
#include "seqlib_amd_samw.h"

using namespace SeqLib;
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static std::string slurp(const std::string &p) { std::ifstream f(p, std::ios::binary); return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()); }

#define OK(x) do { if ((x) != SLX_OK) { std::fprintf(stderr, "samwrite_bench: %s\n", slx_last_error()); return 1; } } while (0)

// route (a); out empty: the reading alone
static int host_route(const std::string &in, const std::string &out, double *secs, int64_t *records)
{
    BamReader r;
    if (!r.Open(in)) return 1;
    BamWriter w(SAM);
    w.SetHeader(r.Header());
    const double t0 = now();
    if (!out.empty() && (!w.Open(out) || !w.WriteHeader())) return 1;
    BamRecord rec;
    int64_t n = 0;
    while (r.GetNextRecord(rec)) {
        if (!out.empty() && !w.WriteRecord(rec)) return 1;
        ++n;
    }
    if (!out.empty() && !w.Close()) return 1;
    *secs = now() - t0; *records = n;
    return 0;
}

// route (b); out empty: the reading alone
static int gpu_route(const std::string &in, const std::string &out, int64_t batch, double *secs, int64_t *records, int64_t *text_bytes, double *us_size, double *us_fill, int64_t *slow)
{
    BamHeader hdr;
    { BamReader r; if (!r.Open(in)) return 1; hdr = r.Header(); }
    slx_bam *rd = nullptr;
    OK(slx_bam_open(in.c_str(), -1, &rd));
    BamWriter w(SAM);
    w.SetHeader(hdr);
    const double t0 = now();
    const bool wr = !out.empty();
    if (wr && (!w.UseGpuSam() || !w.Open(out) || !w.WriteHeader())) return 1;
    int64_t n = 0;
    for (;;) {
        slx_bam_batch bt;
        OK(slx_bam_next(rd, batch, &bt));
        if (!bt.n_records) break;
        if (wr && !w.WriteDevice(bt.d_stream, bt.n_bytes, bt.d_rec_off, bt.n_records)) return 1;
        n += bt.n_records;
    }
    *text_bytes = w.GpuSamCounter("bytes"); *us_size = (double)w.GpuSamCounter("us_size"); *us_fill = (double)w.GpuSamCounter("us_fill"); *slow = w.GpuSamCounter("slow_records");
    if (wr && !w.Close()) return 1;
    *secs = now() - t0; *records = n;
    slx_bam_close(rd);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: samwrite_bench <in.bam> <work dir> [reps]\n"); return 2; }
    const std::string in = argv[1], dir = argv[2], host_sam = dir + "/host.sam", gpu_sam = dir + "/gpu.sam";
    const int reps = argc > 3 ? std::atoi(argv[3]) : 3;
    try {
        double s = 0, us_size = 0, us_fill = 0;
        int64_t n_host = 0, n_gpu = 0, text = 0, slow = 0;
        // ---- the two outputs are the same bytes (this pass also sizes the GPU writer's first buffers and warms the page cache)
        if (host_route(in, host_sam, &s, &n_host) || gpu_route(in, gpu_sam, (int64_t)64 << 20, &s, &n_gpu, &text, &us_size, &us_fill, &slow)) return 1;
        const std::string a = slurp(host_sam), b = slurp(gpu_sam);
        if (a != b || n_host != n_gpu) { std::fprintf(stderr, "samwrite_bench: the two files differ (%zu against %zu bytes, %lld against %lld records)\n", a.size(), b.size(), (long long)n_host, (long long)n_gpu); return 1; }
        const double file_bytes = (double)a.size();
        // ---- (a)
        double read_s = 1e30, host_file_s = 1e30, host_null_s = 1e30;
        for (int rep = 0; rep < reps; ++rep) {
            if (host_route(in, "", &s, &n_host)) return 1;
            read_s = s < read_s ? s : read_s;
            if (host_route(in, host_sam, &s, &n_host)) return 1;
            host_file_s = s < host_file_s ? s : host_file_s;
            if (host_route(in, "/dev/null", &s, &n_host)) return 1;
            host_null_s = s < host_null_s ? s : host_null_s;
        }
        // ---- (b), per batch size
        for (const int64_t batch : {(int64_t)4 << 20, (int64_t)16 << 20, (int64_t)64 << 20, (int64_t)256 << 20}) {
            double gpu_file_s = 1e30, gpu_null_s = 1e30, gpu_read_s = 1e30, k_size = 0, k_fill = 0;
            for (int rep = 0; rep < reps; ++rep) {
                if (gpu_route(in, "", batch, &s, &n_gpu, &text, &us_size, &us_fill, &slow)) return 1;
                gpu_read_s = s < gpu_read_s ? s : gpu_read_s;
                if (gpu_route(in, gpu_sam, batch, &s, &n_gpu, &text, &us_size, &us_fill, &slow)) return 1;
                gpu_file_s = s < gpu_file_s ? s : gpu_file_s;
                if (gpu_route(in, "/dev/null", batch, &s, &n_gpu, &text, &us_size, &us_fill, &slow)) return 1;
                if (s < gpu_null_s) { gpu_null_s = s; k_size = us_size; k_fill = us_fill; }
            }
            const double kern = k_size + k_fill;
            std::printf("{\"file_bytes\": %.0f, \"records\": %lld, \"batch_bytes\": %lld, \"slow_records\": %lld, \"host_read_only_s\": %.4f, \"host_file_s\": %.4f, \"host_null_s\": %.4f, "
                        "\"host_file_MBps\": %.1f, \"host_null_MBps\": %.1f, \"host_writer_alone_MBps\": %.1f, \"gpu_read_only_s\": %.4f, \"gpu_file_s\": %.4f, \"gpu_null_s\": %.4f, \"gpu_writer_alone_MBps\": %.1f, \"gpu_file_MBps\": %.1f, "
                        "\"gpu_null_MBps\": %.1f, \"gpu_vs_host_file\": %.2f, \"gpu_vs_host_null\": %.2f, \"host_records_per_s\": %.0f, \"gpu_records_per_s\": %.0f, \"us_size\": %.0f, "
                        "\"us_fill\": %.0f, \"kernels_MBps\": %.1f, \"fill_MBps\": %.1f}\n",
                        file_bytes, (long long)n_gpu, (long long)batch, (long long)slow, read_s, host_file_s, host_null_s, file_bytes / host_file_s / 1e6, file_bytes / host_null_s / 1e6,
                        host_null_s > read_s ? file_bytes / (host_null_s - read_s) / 1e6 : 0.0, gpu_read_s, gpu_file_s, gpu_null_s, gpu_null_s > gpu_read_s ? file_bytes / (gpu_null_s - gpu_read_s) / 1e6 : 0.0, file_bytes / gpu_file_s / 1e6, file_bytes / gpu_null_s / 1e6,
                        host_file_s / gpu_file_s, host_null_s / gpu_null_s, (double)n_host / host_file_s, (double)n_gpu / gpu_file_s, k_size, k_fill,
                        kern > 0 ? (double)text / (kern * 1e-6) / 1e6 : 0.0, k_fill > 0 ? (double)text / (k_fill * 1e-6) / 1e6 : 0.0);
            std::fflush(stdout);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "samwrite_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
