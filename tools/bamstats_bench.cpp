// bamstats_bench -- what per-read-group statistics on the GPU buy, against the only alternative a user has today, from one process and one file:
//     host      file -> BamReader::Next() -> BamStats::addRead, one thread
//     route     file -> BamStats::addReads(BamReader&), the records never leave HBM
//     add       slx_stats_add_device over the file's records as one device-resident batch (slx_bam_next with no size limit), per lds_groups / window_bytes /
//               long_record setting: kernel time from the unit's HIP events ("us_add"), as GB/s of the batch's bytes.  The groups are known after the warm-up
//               call, so this is the steady state of one launch per batch.
//     add_64    the same records with 64 group keys (the names rewritten to "xy:..." on the host, slx_stats_add_host; the upload is outside "us_add")
//   bamstats_bench <in.bam> [reps]
// The two texts are compared first.  Every figure is the median of reps runs (at least 5) after one warm-up, with the fastest and the slowest beside it.
// Prints one JSON line per measurement.  Built by seqlib_amd/build.py with g++ against libseqlib_amd.so; scripts/make_bench_bam.py writes in.bam (its records
// carry no RG and no ':' in their names: one group, the worst case for same-address atomics).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/BamStats.h"
#include "seqlib_amd_stats.h"

using namespace SeqLib;
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#define OK(x) do { if ((x) != SLX_OK) { std::fprintf(stderr, "bamstats_bench: %s\n", slx_last_error()); return 1; } } while (0)

struct Stat { double med, lo, hi; };
static Stat stat(std::vector<double> v) { std::sort(v.begin(), v.end()); return Stat{v[v.size() / 2], v.front(), v.back()}; }
static void put(const char *what, const char *unit, const Stat &s, const std::string &extra = "")
{
    std::printf("{\"what\": \"%s\", \"unit\": \"%s\", \"median\": %.3f, \"min\": %.3f, \"max\": %.3f%s%s}\n", what, unit, s.med, s.lo, s.hi, extra.empty() ? "" : ", ", extra.c_str());
    std::fflush(stdout);
}

// kernel time of reps adds of the same batch into st (the counts grow; the time does not depend on them)
template <class Add> static int time_adds(slx_stats *st, int reps, Add add, std::vector<double> &ms)
{
    for (int rep = 0; rep <= reps; ++rep) {
        const int64_t u0 = slx_stats_counter(st, "us_add");
        if (add() != SLX_OK) return 1;
        if (rep) ms.push_back((double)(slx_stats_counter(st, "us_add") - u0) / 1e3);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: bamstats_bench <in.bam> [reps]\n"); return 2; }
    const std::string in = argv[1];
    const int reps = std::max(5, argc > 2 ? std::atoi(argv[2]) : 5);
    try {
        // ---- the host loop and the route, and the check
        std::vector<double> th, tg, kg;
        std::string text_host, text_gpu;
        size_t n_host = 0, n_gpu = 0;
        for (int rep = 0; rep <= reps; ++rep) {
            BamReader r;
            if (!r.Open(in)) return 1;
            const double t0 = now();
            BamStats s;
            n_host = 0;
            while (std::optional<BamRecord> rec = r.Next()) { s.addRead(*rec); ++n_host; }
            std::ostringstream o;
            o << s;
            if (rep) th.push_back(now() - t0);
            text_host = o.str();
        }
        for (int rep = 0; rep <= reps; ++rep) {
            BamReader r;
            if (!r.Open(in)) return 1;
            const double t0 = now();
            BamStats s;
            n_gpu = s.addReads(r);
            std::ostringstream o;
            o << s;
            if (rep) { tg.push_back(now() - t0); kg.push_back((double)s.Counter("us_add") / 1e3); }
            text_gpu = o.str();
        }
        if (n_host != n_gpu || text_host != text_gpu) { std::fprintf(stderr, "bamstats_bench: addReads' text is not the host loop's (%zu and %zu records)\n", n_gpu, n_host); return 1; }
        const std::string recs = "\"records\": " + std::to_string(n_host);
        put("host_next_addread_1_thread", "s", stat(th), recs + ", \"records_per_s\": " + std::to_string((double)n_host / stat(th).med));
        put("route_addreads", "s", stat(tg), recs + ", \"records_per_s\": " + std::to_string((double)n_host / stat(tg).med) + ", \"vs_host\": " + std::to_string(stat(th).med / stat(tg).med));
        put("route_add_kernels", "ms", stat(kg));
        // ---- the kernels alone: the file as one device-resident batch
        slx_bam *rd = nullptr;
        OK(slx_bam_open(in.c_str(), -1, &rd));
        slx_bam_batch bt;
        OK(slx_bam_next(rd, (int64_t)1 << 40, &bt));
        const std::string common = "\"records\": " + std::to_string(bt.n_records) + ", \"record_bytes\": " + std::to_string(bt.n_bytes);
        auto gbs = [&](const Stat &s) { return ", \"GB_per_s\": " + std::to_string((double)bt.n_bytes / (s.med * 1e-3) / 1e9); };
        const struct { int64_t lds, win, lng; } cfg[] = {{0, 16384, 4096}, {1, 16384, 4096}, {4, 16384, 4096}, {4, 4096, 4096}, {4, 8192, 4096}, {4, 32768, 4096}, {0, 32768, 4096},
                                                         {4, 16384, 256}, {4, 16384, 1024}};
        for (const auto &c : cfg) {
            slx_stats *st = nullptr;
            OK(slx_stats_create(-1, &st));
            OK(slx_stats_set(st, "lds_groups", c.lds)); OK(slx_stats_set(st, "window_bytes", c.win)); OK(slx_stats_set(st, "long_record", c.lng));
            std::vector<double> ms;
            if (time_adds(st, reps, [&] { return slx_stats_add_device(st, bt.d_stream, bt.n_bytes, bt.d_rec_off, bt.n_records); }, ms)) { std::fprintf(stderr, "bamstats_bench: %s\n", slx_last_error()); return 1; }
            const Stat s = stat(ms);
            put("add_kernels", "ms", s, common + ", \"groups\": " + std::to_string(slx_stats_n_groups(st)) + ", \"lds_groups\": " + std::to_string(c.lds) + ", \"window_bytes\": " + std::to_string(c.win) +
                                            ", \"long_record\": " + std::to_string(c.lng) + ", \"long_records\": " + std::to_string(slx_stats_counter(st, "long_records")) + gbs(s));
            slx_stats_free(st);
        }
        // ---- 64 groups: the names become "xy:...", x and y from the record's index
        std::vector<uint8_t> host(bt.stream, bt.stream + bt.n_bytes);
        for (int64_t i = 0; i < bt.n_records; ++i) {
            uint8_t *h = host.data() + bt.rec_off[i];
            if (h[12] < 5) continue;          // l_read_name
            h[36] = (uint8_t)('a' + (i & 7)); h[37] = (uint8_t)('a' + ((i >> 3) & 7)); h[38] = ':';
        }
        for (const int64_t lds : {0, 4, 16}) {
            slx_stats *st = nullptr;
            OK(slx_stats_create(-1, &st));
            OK(slx_stats_set(st, "lds_groups", lds));
            std::vector<double> ms;
            if (time_adds(st, reps, [&] { return slx_stats_add_host(st, host.data(), bt.n_bytes, bt.rec_off, bt.n_records); }, ms)) { std::fprintf(stderr, "bamstats_bench: %s\n", slx_last_error()); return 1; }
            const Stat s = stat(ms);
            put("add_kernels_64_groups", "ms", s, common + ", \"groups\": " + std::to_string(slx_stats_n_groups(st)) + ", \"lds_groups\": " + std::to_string(lds) + gbs(s));
            slx_stats_free(st);
        }
        slx_bam_close(rd);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bamstats_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
