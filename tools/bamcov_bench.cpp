// bamcov_bench -- what depth of coverage on the GPU buys, against a host loop on 1 and on 16 threads of the same machine, from one process and one file:
//     add       slx_cov_add_device over the file's records as one device-resident batch (slx_bam_next with no size limit), per lds_window / slice_records setting:
//               kernel time from the unit's HIP events ("us_add") and wall clock
//     settle    the in-place scan ("us_settle") ; regions: slx_cov_regions on 10 000 windows of 1 kbp; bedgraph: slx_cov_bedgraph to <work dir>/cov.bg
//     route     file -> STCoverage::addReads(BamReader&) -> settled depth, wall clock
//     host      file -> BamReader::NextBatch -> CIGAR walk -> difference array -> prefix sum, on one thread and with the walk spread over 16 threads
//   bamcov_bench <in.bam> <work dir> [reps]
// The host loop's depth is compared with the GPU's first (SLX_COV_ALIGNED, samtools' flags).  Every figure is the median of reps runs (at least 5) after one
// warm-up, with the fastest and the slowest beside it.  Prints one JSON line per measurement.  Built by seqlib_amd/build.py with g++ against libseqlib_amd.so;
// scripts/make_bench_bam.py --sorted / --shuffled writes in.bam.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/STCoverage.h"
#include "seqlib_amd_cov.h"

using namespace SeqLib;
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#define OK(x) do { if ((x) != SLX_OK) { std::fprintf(stderr, "bamcov_bench: %s\n", slx_last_error()); return 1; } } while (0)

struct Stat { double med, lo, hi; };
static Stat stat(std::vector<double> v) { std::sort(v.begin(), v.end()); return Stat{v[v.size() / 2], v.front(), v.back()}; }
static void put(const char *what, const char *unit, const Stat &s, const std::string &extra = "")
{
    std::printf("{\"what\": \"%s\", \"unit\": \"%s\", \"median\": %.3f, \"min\": %.3f, \"max\": %.3f%s%s}\n", what, unit, s.med, s.lo, s.hi, extra.empty() ? "" : ", ", extra.c_str());
    std::fflush(stdout);
}

// the host loop: what a SeqLib user writes today.  threads > 1: the walk of a batch is spread over the threads, the adds are atomic
static void host_walk(const BamRecordPtrVector &recs, size_t from, size_t step, std::vector<std::vector<int32_t>> &diff)
{
    for (size_t i = from; i < recs.size(); i += step) {
        const bam1_t *b = recs[i]->raw();
        const bam1_core_t &c = b->core;
        if (c.tid < 0 || c.tid >= (int)diff.size() || c.pos < 0 || (c.flag & 0x704)) continue;
        const uint32_t *cig = bam_get_cigar(b);
        int64_t x = c.pos;
        const int64_t L = (int64_t)diff[(size_t)c.tid].size() - 1;
        for (uint32_t k = 0; k < c.n_cigar; ++k) {
            const uint32_t op = cig[k] & 15u, len = cig[k] >> 4;
            if (op == 0 || op == 7 || op == 8) {
                const int64_t lo = std::min(x, L), hi = std::min(x + (int64_t)len, L);
                if (lo < hi) { __atomic_fetch_add(&diff[(size_t)c.tid][(size_t)lo], 1, __ATOMIC_RELAXED); __atomic_fetch_add(&diff[(size_t)c.tid][(size_t)hi], -1, __ATOMIC_RELAXED); }
            }
            if ((0x18du >> op) & 1u) x += len;
        }
    }
}
static int host_route(const std::string &in, int threads, std::vector<std::vector<int32_t>> &depth, double *secs, int64_t *n_out)
{
    BamReader r;
    if (!r.Open(in)) return 1;
    const double t0 = now();
    depth.clear();
    for (int t = 0; t < r.Header().NumSequences(); ++t) depth.emplace_back((size_t)r.Header().GetSequenceLength(t) + 1, 0);
    int64_t n = 0;
    for (;;) {
        BamRecordPtrVector recs;
        if (!r.NextBatch(recs, 1 << 18)) break;
        n += (int64_t)recs.size();
        if (threads == 1) host_walk(recs, 0, 1, depth);
        else {
            std::vector<std::thread> th;
            for (int t = 0; t < threads; ++t) th.emplace_back(host_walk, std::cref(recs), (size_t)t, (size_t)threads, std::ref(depth));
            for (auto &t : th) t.join();
        }
    }
    for (auto &d : depth) for (size_t i = 1; i < d.size(); ++i) d[i] += d[i - 1];
    *secs = now() - t0; *n_out = n;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: bamcov_bench <in.bam> <work dir> [reps]\n"); return 2; }
    const std::string in = argv[1], dir = argv[2];
    const int reps = std::max(5, argc > 3 ? std::atoi(argv[3]) : 5);
    try {
        BamHeader hdr;
        { BamReader r; if (!r.Open(in)) return 1; hdr = r.Header(); }
        const int n_ref = hdr.NumSequences();
        std::vector<int64_t> len;
        std::vector<std::string> names;
        std::vector<const char *> nm;
        for (int t = 0; t < n_ref; ++t) { len.push_back(hdr.GetSequenceLength(t)); names.push_back(hdr.IDtoName(t)); }
        for (auto &s : names) nm.push_back(s.c_str());
        // ---- the host loop, and the check
        std::vector<std::vector<int32_t>> hd;
        std::vector<double> h1, h16;
        double s = 0; int64_t n_host = 0;
        for (int rep = 0; rep <= reps; ++rep) { if (host_route(in, 1, hd, &s, &n_host)) return 1; if (rep) h1.push_back(s); }
        for (int rep = 0; rep <= reps; ++rep) { if (host_route(in, 16, hd, &s, &n_host)) return 1; if (rep) h16.push_back(s); }
        // ---- the file as one device-resident batch
        slx_bam *rd = nullptr;
        OK(slx_bam_open(in.c_str(), -1, &rd));
        slx_bam_batch bt;
        OK(slx_bam_next(rd, (int64_t)1 << 40, &bt));
        slx_cov *cov = nullptr;
        OK(slx_cov_create(-1, n_ref, len.data(), nm.data(), nullptr, &cov));
        OK(slx_cov_add_device(cov, bt.d_stream, bt.n_bytes, bt.d_rec_off, bt.n_records));
        for (int t = 0; t < n_ref; ++t) {
            std::vector<int32_t> g((size_t)len[(size_t)t]);
            OK(slx_cov_depth(cov, t, 0, len[(size_t)t], g.data()));
            if (bt.n_records != n_host || !std::equal(g.begin(), g.end(), hd[(size_t)t].begin())) { std::fprintf(stderr, "bamcov_bench: the GPU's depth of contig %d is not the host loop's\n", t); return 1; }
        }
        const std::string common = "\"records\": " + std::to_string(bt.n_records) + ", \"record_bytes\": " + std::to_string(bt.n_bytes);
        put("host_1_thread", "s", stat(h1), common);
        put("host_16_threads", "s", stat(h16), common);
        // ---- add: the A/B of the window
        for (const int64_t w : {0, 2048, 8192, 15360}) for (const int64_t slice : {256, 1024, 4096}) {
            OK(slx_cov_set(cov, "lds_window", w)); OK(slx_cov_set(cov, "slice_records", slice));
            std::vector<double> k, wall;
            int64_t lds = 0, glob = 0;
            for (int rep = 0; rep <= reps; ++rep) {
                OK(slx_cov_clear(cov));
                const int64_t u0 = slx_cov_counter(cov, "us_add"), l0 = slx_cov_counter(cov, "events_lds"), g0 = slx_cov_counter(cov, "events_global");
                const double t0 = now();
                OK(slx_cov_add_device(cov, bt.d_stream, bt.n_bytes, bt.d_rec_off, bt.n_records));
                if (rep) { wall.push_back((now() - t0) * 1e3); k.push_back((double)(slx_cov_counter(cov, "us_add") - u0) / 1e3); }
                lds = slx_cov_counter(cov, "events_lds") - l0; glob = slx_cov_counter(cov, "events_global") - g0;
            }
            const std::string x = "\"lds_window\": " + std::to_string(w) + ", \"slice_records\": " + std::to_string(slice) + ", \"events_lds\": " + std::to_string(lds) + ", \"events_global\": " + std::to_string(glob);
            put("add_kernels", "ms", stat(k), x);
            put("add_wall", "ms", stat(wall), x);
        }
        OK(slx_cov_set(cov, "lds_window", 8192)); OK(slx_cov_set(cov, "slice_records", 1024));
        // ---- settle, regions, bedGraph
        std::vector<double> ks, ws, wr, wb;
        std::vector<slx_bam_region> regs;
        uint64_t x = 88172645463325252ull;
        for (int i = 0; i < 10000; ++i) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            const int t = (int)(x % (uint64_t)n_ref);
            const int64_t b = (int64_t)((x >> 20) % (uint64_t)std::max<int64_t>(len[(size_t)t], 1));
            regs.push_back(slx_bam_region{t, b, b + 1000});
        }
        std::vector<int64_t> sum(regs.size()), cnt(regs.size());
        const std::string bg = dir + "/cov.bg";
        for (int rep = 0; rep <= reps; ++rep) {
            OK(slx_cov_clear(cov));
            OK(slx_cov_add_device(cov, bt.d_stream, bt.n_bytes, bt.d_rec_off, bt.n_records));
            const int64_t u0 = slx_cov_counter(cov, "us_settle");
            double t0 = now();
            OK(slx_cov_depth(cov, 0, 0, 0, nullptr));
            if (rep) { ws.push_back((now() - t0) * 1e3); ks.push_back((double)(slx_cov_counter(cov, "us_settle") - u0) / 1e3); }
            t0 = now();
            OK(slx_cov_regions(cov, regs.data(), (int64_t)regs.size(), 1, sum.data(), cnt.data()));
            if (rep) wr.push_back((now() - t0) * 1e3);
            t0 = now();
            OK(slx_cov_bedgraph(cov, -1, 0, bg.c_str()));
            if (rep) wb.push_back((now() - t0) * 1e3);
        }
        int64_t positions = 0;
        for (int64_t l : len) positions += l;
        put("settle_kernels", "ms", stat(ks), "\"positions\": " + std::to_string(positions));
        put("settle_wall", "ms", stat(ws));
        put("regions_10000_wall", "ms", stat(wr));
        put("bedgraph_wall", "ms", stat(wb), "\"runs\": " + std::to_string(slx_cov_counter(cov, "runs")));
        slx_cov_free(cov);
        slx_bam_close(rd);
        // ---- the whole route from the file
        // ---- the whole route from the file (the reader's default batches of 64 MiB), and the add kernels' share of it per setting
        for (const int64_t w : {8192, 0}) for (const int64_t slice : {256, 1024, 4096}) {
            std::vector<double> route, k;
            for (int rep = 0; rep <= reps; ++rep) {
                BamReader r;
                if (!r.Open(in)) return 1;
                const double t0 = now();
                STCoverage c;
                c.SetHeader(r.Header());
                c.SetMode(SLX_COV_ALIGNED); c.SetExcludeFlags(0x704);
                c.SetKnob("lds_window", w); c.SetKnob("slice_records", slice);
                const size_t n = c.addReads(r, 0, false);
                c.settleCoverage();
                if (rep) { route.push_back(now() - t0); k.push_back((double)c.Counter("us_add") / 1e3); }
                if ((int64_t)n != n_host) { std::fprintf(stderr, "bamcov_bench: addReads handed over %zu of %lld records\n", n, (long long)n_host); return 1; }
            }
            const std::string x = "\"lds_window\": " + std::to_string(w) + ", \"slice_records\": " + std::to_string(slice);
            put("route_add_kernels", "ms", stat(k), x);
            put("route_file_to_depth", "s", stat(route), x + ", \"vs_host_16_threads\": " + std::to_string(stat(h16).med / stat(route).med) + ", \"vs_host_1_thread\": " + std::to_string(stat(h1).med / stat(route).med));
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bamcov_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
