// samread_bench -- what the GPU SAM reader buys, against the serial host parser on one thread of the same machine (what a sam_read1 loop is), from one process
// and one file:
//     in.bam -> SeqLib::BamReader -> SeqLib::BamWriter(SAM) -> <work dir>/bench.sam          the input: SAM text as this project's own writer emits it (not timed)
//     bench.sam -> slx_sam_open + slx_bam_next to the end of the file                          GPU kernels (HIP events, from the counters) and end to end, per batch size
//     bench.sam -> sam_host.h's samh_parse_line line by line, one thread                       the baseline
//     bench.sam -> slx_sam_open + slx_bgzf_write_device -> <work dir>/bench.out.bam            SAM to BAM, file to file, no host round trip of the records
//   samread_bench <in.bam> <work dir> [reps]
// Prints one JSON line per batch size.  Built by seqlib_amd/build.py with g++ against libseqlib_amd.so.  scripts/make_bench_bam.py writes in.bam.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/BamWriter.h"
#include "seqlib_amd_sam.h"
#include "sam_host.h"

using namespace SeqLib;
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static void put32(std::string &s, uint32_t v) { s.append(reinterpret_cast<const char *>(&v), 4); }

#define OK(x) do { if ((x) != SLX_OK) { std::fprintf(stderr, "samread_bench: %s\n", slx_last_error()); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: samread_bench <in.bam> <work dir> [reps]\n"); return 2; }
    const std::string in = argv[1], dir = argv[2], sam = dir + "/bench.sam", out_bam = dir + "/bench.out.bam";
    const int reps = argc > 3 ? std::atoi(argv[3]) : 3;
    try {
        {   // ---- the input
            BamReader r;
            if (!r.Open(in)) return 1;
            BamWriter w(SAM);
            w.SetHeader(r.Header());
            if (!w.Open(sam) || !w.WriteHeader()) return 1;
            for (;;) {
                BamRecordPtrVector v;
                if (!r.NextBatch(v, (size_t)1 << 20)) break;
                if (!w.WriteRecords(v)) return 1;
            }
            if (!w.Close()) return 1;
        }
        std::vector<unsigned char> file;
        {
            FILE *fp = std::fopen(sam.c_str(), "rb");
            if (!fp) return 1;
            std::fseek(fp, 0, SEEK_END); file.resize((size_t)std::ftell(fp)); std::fseek(fp, 0, SEEK_SET);
            if (std::fread(file.data(), 1, file.size(), fp) != file.size()) return 1;
            std::fclose(fp);
        }
        const double text_bytes = (double)file.size();
        // ---- the baseline: the serial host parser, one thread
        std::string text, msg;
        std::vector<std::string> names;
        std::vector<int64_t> lens;
        uint64_t body = 0, hdr_lines = 0;
        if (samh_header(file.data(), file.size(), true, text, names, lens, &body, &hdr_lines, msg) != 1) { std::fprintf(stderr, "samread_bench: %s\n", msg.c_str()); return 1; }
        SamRefTable tab;
        tab.build(names);
        double host_s = 1e30;
        uint64_t host_records = 0, host_bytes = 0;
        for (int rep = 0; rep < reps; ++rep) {
            const sam_refs R = tab.view();
            std::vector<uint8_t> rec;
            host_records = host_bytes = 0;
            const double t0 = now();
            for (uint64_t p = body; p < file.size();) {
                const unsigned char *nl = (const unsigned char *)std::memchr(file.data() + p, '\n', file.size() - p);
                const uint64_t e = nl ? (uint64_t)(nl - file.data()) : file.size();
                int err = 0;
                if (samh_parse_line(file.data() + p, e - p, R, rec, &err) != SAM_FAST) { std::fprintf(stderr, "samread_bench: host parser: %s\n", samh_errtext(err)); return 1; }
                ++host_records; host_bytes += rec.size();
                p = e + 1;
            }
            const double s = now() - t0;
            host_s = s < host_s ? s : host_s;
        }
        // ---- the reader, per batch size
        for (const int64_t batch : {(int64_t)1 << 20, (int64_t)16 << 20, (int64_t)64 << 20, (int64_t)256 << 20}) {
            slx_bam *rd = nullptr;
            OK(slx_sam_open(sam.c_str(), -1, &rd));
            double gpu_s = 1e30, us[5] = {0, 0, 0, 0, 0};
            int64_t records = 0, bytes = 0, batches = 0, slow = 0;
            for (int rep = 0; rep < reps + 1; ++rep) {           // (the first pass sizes the buffers)
                OK(slx_bam_rewind(rd));
                records = bytes = batches = 0;
                const double t0 = now();
                for (;;) {
                    slx_bam_batch bt;
                    OK(slx_bam_next(rd, batch, &bt));
                    if (!bt.n_records) break;
                    records += bt.n_records; bytes += bt.n_bytes; ++batches;
                }
                const double s = now() - t0;
                if (rep && s < gpu_s) {
                    gpu_s = s;
                    const char *nm[5] = {"us_lines", "us_fields", "us_size", "us_fill", "us_inflate"};
                    for (int i = 0; i < 5; ++i) us[i] = (double)slx_bam_counter(rd, nm[i]);
                    slow = slx_bam_counter(rd, "slow_records");
                }
            }
            const int source = (int)slx_bam_counter(rd, "source");
            slx_bam_close(rd);
            if ((uint64_t)records != host_records || (uint64_t)bytes != host_bytes) { std::fprintf(stderr, "samread_bench: the reader gives %lld records, the host parser %llu\n", (long long)records, (unsigned long long)host_records); return 1; }
            // ---- SAM to BAM, file to file
            double conv_s = 1e30;
            for (int rep = 0; rep < 2; ++rep) {
                const double t0 = now();
                slx_bam *r2 = nullptr;
                OK(slx_sam_open(sam.c_str(), -1, &r2));
                slx_bgzf *w = nullptr;
                OK(slx_bgzf_open(out_bam.c_str(), -1, &w));
                std::string h("BAM\1", 4);
                put32(h, (uint32_t)text.size()); h += text; put32(h, (uint32_t)names.size());
                for (size_t i = 0; i < names.size(); ++i) { put32(h, (uint32_t)names[i].size() + 1); h += names[i]; h += '\0'; put32(h, (uint32_t)lens[i]); }
                OK(slx_bgzf_write(w, h.data(), (int64_t)h.size()));
                OK(slx_bgzf_flush(w));
                for (;;) {
                    slx_bam_batch bt;
                    OK(slx_bam_next(r2, batch, &bt));
                    if (!bt.n_records) break;
                    OK(slx_bgzf_write_device(w, bt.d_stream, bt.n_bytes));
                }
                OK(slx_bgzf_close(w));
                slx_bam_close(r2);
                const double s = now() - t0;
                conv_s = s < conv_s ? s : conv_s;
            }
            const double kern = us[0] + us[1] + us[2] + us[3];
            std::printf("{\"text_bytes\": %.0f, \"records\": %lld, \"source\": %d, \"batch_bytes\": %lld, \"batches\": %lld, \"slow_records\": %lld, \"host_parser_s\": %.4f, "
                        "\"host_parser_MBps\": %.1f, \"reader_s\": %.4f, \"reader_MBps\": %.1f, \"reader_vs_host\": %.2f, \"records_per_s\": %.0f, \"us_lines\": %.0f, \"us_fields\": %.0f, "
                        "\"us_size\": %.0f, \"us_fill\": %.0f, \"kernels_MBps\": %.1f, \"sam_to_bam_s\": %.4f, \"sam_to_bam_MBps\": %.1f}\n",
                        text_bytes, (long long)records, source, (long long)batch, (long long)batches, (long long)slow, host_s, text_bytes / host_s / 1e6, gpu_s, text_bytes / gpu_s / 1e6,
                        host_s / gpu_s, (double)records / gpu_s, us[0], us[1], us[2], us[3], kern > 0 ? text_bytes / (kern * 1e-6) / 1e6 : 0.0, conv_s, text_bytes / conv_s / 1e6);
            std::fflush(stdout);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "samread_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
