// bamread_bench -- what the GPU BAM reader buys, against zlib on the CPUs the process may use, from one process and one file:
//     file -> slx_bam_next (pinned inflated stream + record offsets)            GPU kernels (HIP events) and end to end
//     file -> SeqLib::BamReader::NextBatch -> BamRecordPtrVector                end to end records/s
//     file -> SeqLib::BWAAligner::alignSequences(BamReader&)                    end to end reads/s (only with an index prefix)
//     file -> zlib inflate + crc32 of the same members, one member per task     the baseline
//   bamread_bench <file.bam> [index prefix] [reps]
// Prints one JSON line.  Built by seqlib_amd/build.py with g++ against libseqlib_amd.so.  scripts/make_bench_bam.py writes the input.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include <zlib.h>
#include "SeqLib/BWAAligner.h"
#include "SeqLib/BamReader.h"

using namespace SeqLib;
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: bamread_bench <file.bam> [index prefix | -] [reps]\n"); return 2; }
    const std::string path = argv[1], prefix = argc > 2 && std::strcmp(argv[2], "-") ? argv[2] : "";
    const int reps = argc > 3 ? std::atoi(argv[3]) : 3;
    try {
        // ---- the baseline: zlib on the granted CPUs, one member per task
        slx_bam_member *mem = nullptr; int64_t nm = 0; int eof = 0;
        if (slx_bam_scan_members(path.c_str(), &mem, &nm, &eof) != SLX_OK) { std::fprintf(stderr, "bamread_bench: %s\n", slx_last_error()); return 1; }
        std::vector<unsigned char> file;
        {
            FILE *fp = std::fopen(path.c_str(), "rb");
            std::fseek(fp, 0, SEEK_END); file.resize((size_t)std::ftell(fp)); std::fseek(fp, 0, SEEK_SET);
            if (std::fread(file.data(), 1, file.size(), fp) != file.size()) return 1;
            std::fclose(fp);
        }
        std::vector<uint64_t> out_off((size_t)nm + 1, 0);
        for (int64_t i = 0; i < nm; ++i) out_off[(size_t)i + 1] = out_off[(size_t)i] + mem[i].isize;
        const uint64_t total = out_off[(size_t)nm];
        const unsigned cpus = detail::effective_cpus();
        std::vector<unsigned char> inflated(total + 1);
        double zlib_s = 1e30;
        for (int rep = 0; rep < reps; ++rep) {
            std::atomic<int64_t> next{0};
            std::atomic<int> bad{0};
            const double t0 = now();
            std::vector<std::thread> th;
            for (unsigned t = 0; t < cpus; ++t)
                th.emplace_back([&]() {
                    z_stream zs;
                    for (;;) {
                        const int64_t i = next.fetch_add(1);
                        if (i >= nm) break;
                        std::memset(&zs, 0, sizeof zs);
                        inflateInit2(&zs, -15);
                        zs.next_in = file.data() + mem[i].file_off + mem[i].data_off; zs.avail_in = mem[i].data_len;
                        zs.next_out = inflated.data() + out_off[(size_t)i]; zs.avail_out = mem[i].isize;
                        const int rc = inflate(&zs, Z_FINISH);
                        inflateEnd(&zs);
                        if (rc != Z_STREAM_END || (uint32_t)crc32(crc32(0L, Z_NULL, 0), inflated.data() + out_off[(size_t)i], mem[i].isize) != mem[i].crc32) ++bad;
                    }
                });
            for (auto &t : th) t.join();
            const double s = now() - t0;
            if (bad) { std::fprintf(stderr, "bamread_bench: zlib rejects %d members\n", bad.load()); return 1; }
            zlib_s = s < zlib_s ? s : zlib_s;
        }
        // ---- the C-ABI: file -> pinned stream + offsets
        slx_bam *rd = nullptr;
        if (slx_bam_open(path.c_str(), -1, &rd) != SLX_OK) { std::fprintf(stderr, "bamread_bench: %s\n", slx_last_error()); return 1; }
        double gpu_s = 1e30, us_inf = 0, us_crc = 0, us_idx = 0;
        int64_t records = 0, bytes = 0, repaired = 0;
        for (int rep = 0; rep < reps + 1; ++rep) {           // (the first pass sizes the buffers)
            slx_bam_rewind(rd);
            double a = 0, b = 0, c = 0;
            records = bytes = 0;
            const double t0 = now();
            for (;;) {
                slx_bam_batch bt;
                if (slx_bam_next(rd, (int64_t)256 << 20, &bt) != SLX_OK) { std::fprintf(stderr, "bamread_bench: %s\n", slx_last_error()); return 1; }
                if (!bt.n_records) break;
                records += bt.n_records; bytes += bt.n_bytes; repaired += bt.n_repaired_chunks;
                a += (double)slx_bam_counter(rd, "us_inflate"); b += (double)slx_bam_counter(rd, "us_crc"); c += (double)slx_bam_counter(rd, "us_index");
            }
            const double s = now() - t0;
            if (rep && s < gpu_s) { gpu_s = s; us_inf = a; us_crc = b; us_idx = c; }
        }
        slx_bam_close(rd);
        // ---- the class: file -> BamRecords
        double rec_s = 1e30;
        size_t n_rec = 0;
        for (int rep = 0; rep < reps; ++rep) {
            BamReader r;
            if (!r.Open(path)) return 1;
            const double t0 = now();
            n_rec = 0;
            for (;;) {
                BamRecordPtrVector v;
                const size_t got = r.NextBatch(v, (size_t)1 << 20);
                n_rec += got;
                if (!got) break;
            }
            const double s = now() - t0;
            rec_s = s < rec_s ? s : rec_s;
        }
        // ---- realignment: file -> alignSequences(BamReader&)
        double aln_s = 0; size_t n_reads = 0, n_hits = 0;
        if (!prefix.empty()) {
            BWAIndexPtr idx = std::make_shared<BWAIndex>();
            idx->LoadIndex(prefix);
            BWAAligner al(idx);
            aln_s = 1e30;
            for (int rep = 0; rep < 2; ++rep) {
                BamReader r;
                if (!r.Open(path)) return 1;
                std::vector<BamRecordPtrVector> out;
                const double t0 = now();
                al.alignSequences(r, out, false, 0.9, 10, 0x900, true);
                const double s = now() - t0;
                aln_s = s < aln_s ? s : aln_s;
                n_reads = out.size(); n_hits = 0;
                for (auto &v : out) n_hits += v.size();
            }
        }
        std::printf("{\"inflated_bytes\": %llu, \"members\": %lld, \"records\": %lld, \"cpus\": %u, \"zlib_GBps\": %.3f, \"gpu_inflate_GBps\": %.3f, \"gpu_kernels_GBps\": %.3f, "
                    "\"reader_GBps\": %.3f, \"reader_vs_zlib\": %.2f, \"us_inflate\": %.0f, \"us_crc\": %.0f, \"us_index\": %.0f, \"repaired_chunks\": %lld, "
                    "\"records_per_s\": %.0f, \"realign_reads_per_s\": %.0f, \"realign_reads\": %zu, \"realign_records\": %zu}\n",
                    (unsigned long long)total, (long long)nm, (long long)records, cpus, total / zlib_s / 1e9, us_inf > 0 ? total / (us_inf * 1e-6) / 1e9 : 0.0,
                    us_inf + us_crc + us_idx > 0 ? total / ((us_inf + us_crc + us_idx) * 1e-6) / 1e9 : 0.0, total / gpu_s / 1e9, zlib_s / gpu_s, us_inf, us_crc, us_idx,
                    (long long)repaired, (double)n_rec / rec_s, aln_s > 0 ? (double)n_reads / aln_s : 0.0, n_reads, n_hits);
        slx_bam_members_free(mem);
        (void)bytes;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bamread_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
