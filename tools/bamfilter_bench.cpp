// bamfilter_bench -- what the read filter costs on the GPU and what it replaces on the host, from one process and one file, for three rule sets:
//   flags    mapq >= 20, duplicates, QC failures and secondary alignments off            (fixed fields only)
//   cigar    the largest insertion <= 5, NM <= 4, clipped bases <= 20                     (CIGAR and aux walks)
//   motifs   1 000 random 20-mers                                                         (the automaton read from HBM)
//   gpu      slx_filter_attach + slx_bam_next over the whole file: the batches come out filtered and compacted
//   host     the way without it: NextBatch of every record, then slx_filter_test_record per record on 16 threads
//   plain    slx_bam_next over the same file with no filter attached
//   bamfilter_bench <file.bam> [reps]        (reps 3: the median of every time; one unmeasured pass first)
// Prints one JSON line; the kept counts of gpu and host are equal, or the run fails.  Built by seqlib_amd/build.py.  scripts/make_bench_bam.py writes the input.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <thread>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/ReadFilter.h"

using namespace SeqLib;
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

static slx_filter *make(int which)
{
    slx_filter *f = nullptr;
    if (slx_filter_create(&f) != SLX_OK) return nullptr;
    const int id = slx_filter_add_filter(f, 0, 0, nullptr, 0);
    slx_filter_rule r;
    std::memset(&r, 0, sizeof r);
    for (auto &g : r.r) g.every = 1;
    r.subsample_frac = 1; r.subsample_seed = 999;
    auto range = [&](int i, int mn, int mx) { r.r[i].min = mn; r.r[i].max = mx; r.r[i].every = 0; };
    std::vector<std::string> motifs;
    if (which == 0) { range(SLX_FR_MAPQ, 20, 255); r.any_off = 0x700; }
    else if (which == 1) { range(SLX_FR_INS, 0, 5); range(SLX_FR_NM, 0, 4); range(SLX_FR_CLIP, 0, 20); }
    else {
        std::mt19937 rng(7);
        for (int i = 0; i < 1000; ++i) { std::string m; for (int j = 0; j < 20; ++j) m += "ACGT"[rng() & 3]; motifs.push_back(m); }
    }
    std::vector<const char *> mp;
    for (const std::string &m : motifs) mp.push_back(m.c_str());
    if (id < 0 || slx_filter_add_rule(f, id, &r, nullptr, mp.data(), (int64_t)mp.size()) != SLX_OK) { slx_filter_free(f); return nullptr; }
    return f;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: bamfilter_bench <file.bam> [reps]\n"); return 2; }
    const std::string path = argv[1];
    const int reps = std::max(1, argc > 2 ? std::atoi(argv[2]) : 3);
    const char *names[3] = {"flags", "cigar", "motifs"};
    try {
        slx_bam *rd = nullptr;
        if (slx_bam_open(path.c_str(), -1, &rd) != SLX_OK) { std::fprintf(stderr, "bamfilter_bench: %s\n", slx_last_error()); return 1; }
        auto pass = [&](int64_t *records) -> double {
            slx_bam_rewind(rd);
            *records = 0;
            const double t0 = now();
            for (;;) {
                slx_bam_batch bt;
                if (slx_bam_next(rd, (int64_t)64 << 20, &bt) != SLX_OK) { std::fprintf(stderr, "bamfilter_bench: %s\n", slx_last_error()); std::exit(1); }
                if (!bt.n_records) break;
                *records += bt.n_records;
            }
            return now() - t0;
        };
        int64_t records = 0;
        std::vector<double> t_plain;
        for (int rep = 0; rep < reps + 1; ++rep) { const double t = pass(&records); if (rep) t_plain.push_back(t); }
        std::string out = "{\"records\": " + std::to_string(records) + ", \"reps\": " + std::to_string(reps);
        char buf[512];
        std::snprintf(buf, sizeof buf, ", \"plain_s\": %.4f, \"plain_Mrec_s\": %.3f", median(t_plain), records / median(t_plain) / 1e6);
        out += buf;
        BamReader hr;
        if (!hr.Open(path)) return 1;
        for (int w = 0; w < 3; ++w) {
            slx_filter *f = make(w);
            if (!f) { std::fprintf(stderr, "bamfilter_bench: %s\n", slx_last_error()); return 1; }
            slx_filter_attach(f, rd);
            std::vector<double> t_gpu, t_host;
            int64_t kept_gpu = 0, kept_host = 0;
            const int64_t us0 = slx_filter_counter(f, "us_filter");
            for (int rep = 0; rep < reps + 1; ++rep) { const double t = pass(&kept_gpu); if (rep) t_gpu.push_back(t); }
            const double us_pass = (double)(slx_filter_counter(f, "us_filter") - us0) / (reps + 1);
            slx_filter_attach(nullptr, rd);
            // the host way: every record out as a BamRecord, then the per-record body on 16 threads (one filter each: the counters are not shared)
            std::vector<slx_filter *> tf;
            for (int t = 0; t < 16; ++t) tf.push_back(make(w));
            for (int rep = 0; rep < reps + 1; ++rep) {
                hr.Reset();
                std::atomic<int64_t> kept{0};
                const double t0 = now();
                for (;;) {
                    BamRecordPtrVector v;
                    if (!hr.NextBatch(v, (size_t)1 << 20)) break;
                    std::vector<std::thread> th;
                    for (int t = 0; t < 16; ++t)
                        th.emplace_back([&, t] {
                            int64_t k = 0;
                            for (size_t i = (size_t)t; i < v.size(); i += 16) {
                                const std::vector<uint8_t> p = SeqLib::detail::packed_record(v[i]->raw());
                                k += slx_filter_test_record(tf[t], p.data(), (int64_t)p.size()) == 1;
                            }
                            kept += k;
                        });
                    for (auto &x : th) x.join();
                }
                if (rep) t_host.push_back(now() - t0);
                kept_host = kept;
            }
            for (slx_filter *x : tf) slx_filter_free(x);
            if (kept_gpu != kept_host) { std::fprintf(stderr, "bamfilter_bench: %s: the GPU keeps %lld records, the host %lld\n", names[w], (long long)kept_gpu, (long long)kept_host); return 1; }
            std::snprintf(buf, sizeof buf, ", \"%s\": {\"kept\": %lld, \"gpu_s\": %.4f, \"gpu_Mrec_s\": %.3f, \"filter_kernels_us\": %.0f, \"host_s\": %.4f, \"host_Mrec_s\": %.3f, \"dfa_states\": %lld, \"dfa_in_lds\": %lld}",
                          names[w], (long long)kept_gpu, median(t_gpu), records / median(t_gpu) / 1e6, us_pass, median(t_host), records / median(t_host) / 1e6,
                          (long long)slx_filter_counter(f, "dfa_states"), (long long)slx_filter_counter(f, "dfa_in_lds"));
            out += buf;
            slx_filter_free(f);
        }
        slx_bam_close(rd);
        std::printf("%s}\n", out.c_str());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bamfilter_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
