// bamsort_bench -- what the coordinate sort in HBM costs and buys, from one process and one file.  [reps] runs each, alternating, median and range:
//     (a) slx_sort_file_ex                       <file.bam> sorted into a scratch file end to end: inflate, keys, radix sort, tile gather, DEFLATE, the file;
//                                                and its stages from the sorter's counters (HIP events): us_key, us_sort, us_gather
//     (b) a host route on the granted CPUs       over the inflated record stream, already in memory (so WITHOUT the inflate, the deflate and the file that (a)
//                                                pays for): one walk for key / index pairs, std::stable_sort on them, a memcpy gather by as many threads as CPUs
// The gather's rate is bytes read plus bytes written over its time: every byte of the stream moves twice.
//   bamsort_bench <file.bam> <scratch prefix> [reps]
// Prints one JSON line.  Built by seqlib_amd/build.py with g++ against libseqlib_amd.so.  scripts/make_bench_bam.py --shuffled writes an input worth sorting
// (without the option its records are all unplaced: one key, and the sort leaves the file as it is).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "SeqLib/BWAAligner.h"
#include "seqlib_amd_bam.h"
#include "seqlib_amd_sort.h"

using namespace SeqLib;
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct Runs {
    std::vector<double> s;
    double med() const { std::vector<double> v = s; std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
    double lo() const { return *std::min_element(s.begin(), s.end()); }
    double hi() const { return *std::max_element(s.begin(), s.end()); }
};
static uint32_t ld32(const unsigned char *p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
#define DIE() do { std::fprintf(stderr, "bamsort_bench: %s\n", slx_last_error()); return 1; } while (0)

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: bamsort_bench <file.bam> <scratch prefix> [reps]\n"); return 2; }
    const std::string path = argv[1], out = std::string(argv[2]) + ".sorted.bam";
    const int reps = argc > 3 ? std::max(1, std::atoi(argv[3])) : 3;
    // ---- the inflated stream and where its records start, once
    slx_bam_member *mem = nullptr; int64_t nm = 0; int eof = 0;
    if (slx_bam_scan_members(path.c_str(), &mem, &nm, &eof) != SLX_OK) DIE();
    uint64_t total = 0, got = 0;
    for (int64_t i = 0; i < nm; ++i) total += mem[i].isize;
    slx_bam_members_free(mem);
    std::vector<unsigned char> stream(total);
    if (slx_bam_inflate_file(path.c_str(), -1, stream.data(), total, &got) != SLX_OK || got != total) DIE();
    if (total < 12 || std::memcmp(stream.data(), "BAM\1", 4) != 0) { std::fprintf(stderr, "bamsort_bench: not a BAM stream\n"); return 1; }
    uint64_t first = 12 + ld32(&stream[4]);
    for (uint32_t r = ld32(&stream[first - 4]); r; --r) first += 8 + ld32(&stream[first]);
    const uint64_t B = total - first;
    const unsigned cpus = detail::effective_cpus();
    slx_sort *s = nullptr;
    if (slx_sort_create(-1, &s) != SLX_OK) DIE();
    if (slx_sort_file_ex(s, path.c_str(), out.c_str()) != SLX_OK) DIE();          // (the first pass sizes the buffers and loads the kernels: not timed)
    Runs g, hk, hs, hg, ht, uk, us, ug;
    int64_t records = 0, segments = 0, slabs = 0;
    std::vector<unsigned char> sorted(B);
    for (int rep = 0; rep < reps; ++rep) {
        {   // (a)
            const int64_t k0 = slx_sort_counter(s, "us_key"), s0 = slx_sort_counter(s, "us_sort"), g0 = slx_sort_counter(s, "us_gather");
            const int64_t r0 = slx_sort_counter(s, "records"), e0 = slx_sort_counter(s, "segments"), l0 = slx_sort_counter(s, "slabs");
            const double t0 = now();
            if (slx_sort_file_ex(s, path.c_str(), out.c_str()) != SLX_OK) DIE();
            g.s.push_back(now() - t0);
            uk.s.push_back((double)(slx_sort_counter(s, "us_key") - k0)); us.s.push_back((double)(slx_sort_counter(s, "us_sort") - s0)); ug.s.push_back((double)(slx_sort_counter(s, "us_gather") - g0));
            records = slx_sort_counter(s, "records") - r0; segments = slx_sort_counter(s, "segments") - e0; slabs = slx_sort_counter(s, "slabs") - l0;
        }
        {   // (b)
            const unsigned char *p = stream.data() + first;
            const double t0 = now();
            std::vector<std::pair<uint64_t, uint32_t>> ki;
            std::vector<uint64_t> off;
            for (uint64_t o = 0; o + 36 <= B; o += 4 + (uint64_t)ld32(p + o)) {
                ki.emplace_back((uint64_t)ld32(p + o + 4) << 32 | (uint64_t)(ld32(p + o + 8) ^ 0x80000000u), (uint32_t)off.size());
                off.push_back(o);
            }
            off.push_back(B);
            const double t1 = now();
            std::stable_sort(ki.begin(), ki.end(), [](const std::pair<uint64_t, uint32_t> &a, const std::pair<uint64_t, uint32_t> &b) { return a.first < b.first; });
            const double t2 = now();
            const size_t n = ki.size();
            std::vector<uint64_t> dst(n + 1, 0);
            for (size_t j = 0; j < n; ++j) dst[j + 1] = dst[j] + (off[ki[j].second + 1] - off[ki[j].second]);
            std::vector<std::thread> th;
            for (unsigned t = 0; t < cpus; ++t)
                th.emplace_back([&, t]() {
                    for (size_t j = n * t / cpus; j < n * (t + 1) / cpus; ++j) std::memcpy(&sorted[dst[j]], p + off[ki[j].second], off[ki[j].second + 1] - off[ki[j].second]);
                });
            for (auto &t : th) t.join();
            const double t3 = now();
            hk.s.push_back(t1 - t0); hs.s.push_back(t2 - t1); hg.s.push_back(t3 - t2); ht.s.push_back(t3 - t0);
            if ((int64_t)n != records) { std::fprintf(stderr, "bamsort_bench: the host walk found %zu records, the sorter %lld\n", n, (long long)records); return 1; }
        }
    }
    // the two routes agree: the file (a) wrote inflates to the header (with SO:coordinate) and the stream (b) gathered
    {
        uint64_t n2 = 0, t2 = 0;
        if (slx_bam_scan_members(out.c_str(), &mem, &nm, &eof) != SLX_OK) DIE();
        for (int64_t i = 0; i < nm; ++i) t2 += mem[i].isize;
        slx_bam_members_free(mem);
        std::vector<unsigned char> back(t2);
        if (slx_bam_inflate_file(out.c_str(), -1, back.data(), t2, &n2) != SLX_OK || n2 != t2) DIE();
        if (t2 < B || std::memcmp(back.data() + (t2 - B), sorted.data(), B) != 0) { std::fprintf(stderr, "bamsort_bench: the sorted file differs from the host route's stream\n"); return 1; }
    }
    slx_sort_free(s);
    std::remove(out.c_str());
    const double gather_rate = ug.med() > 0 ? 2.0 * (double)B / (ug.med() * 1e-6) / 1e12 : 0.0;
    std::printf("{\"records\": %lld, \"record_bytes\": %llu, \"cpus\": %u, \"reps\": %d, \"segments\": %lld, \"slabs\": %lld, "
                "\"gpu_file_s\": [%.3f, %.3f, %.3f], \"gpu_file_GBps\": %.3f, "
                "\"us_key\": [%.0f, %.0f, %.0f], \"us_sort\": [%.0f, %.0f, %.0f], \"us_gather\": [%.0f, %.0f, %.0f], "
                "\"gather_TBps_read_plus_written\": %.3f, \"gather_fraction_of_6.29_TBps\": %.3f, "
                "\"host_keys_s\": [%.3f, %.3f, %.3f], \"host_stable_sort_s\": [%.3f, %.3f, %.3f], \"host_gather_s\": [%.3f, %.3f, %.3f], \"host_route_s\": [%.3f, %.3f, %.3f], "
                "\"host_route_over_gpu_file\": %.2f, \"host_route_over_gpu_stages\": %.1f}\n",
                (long long)records, (unsigned long long)B, cpus, reps, (long long)segments, (long long)slabs,
                g.lo(), g.med(), g.hi(), (double)B / g.med() / 1e9,
                uk.lo(), uk.med(), uk.hi(), us.lo(), us.med(), us.hi(), ug.lo(), ug.med(), ug.hi(),
                gather_rate, gather_rate / 6.29,
                hk.lo(), hk.med(), hk.hi(), hs.lo(), hs.med(), hs.hi(), hg.lo(), hg.med(), hg.hi(), ht.lo(), ht.med(), ht.hi(),
                ht.med() / g.med(), ht.med() / ((uk.med() + us.med() + ug.med()) * 1e-6));
    return 0;
}
