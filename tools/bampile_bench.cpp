// bampile_bench -- what the per-base pileup on the GPU buys against a one-thread host loop of the same machine, from one process and one file.  A pileup object
// holds one window of one contig, so for a whole file the tool keeps one object per contig of the header and hands every batch to each of them.
//     host      file -> BamReader::NextBatch -> CIGAR walk -> increments into the same 15 planes, on one thread: once for the one window a pileup object holds (the
//               contig with the most bases) and once for every contig; its planes are compared with the GPU's first
//     route     file -> Pileup::addReads(BamReader&) -> the 15 planes on the host, wall clock: the one window in one pass, and every contig in a pass each
//     add       slx_pile_add_device over the file's records as one device-resident batch (slx_bam_next with no size limit), per lds_window / group_lanes /
//               slice_records setting: kernel time from the unit's HIP events ("us_add"), beside slx_cov_add_device on the same batch ("us_add" of that unit)
//     sites     slx_pile_sites of every contig against the FASTA (min_depth 10, min_alt 3, 1/50), kernel time ("us_sites") and wall clock
//   bampile_bench <in.bam> <ref.fa> [reps]
// Every figure is the median of reps runs (at least 5) after one warm-up, with the fastest and the slowest beside it.  Prints one JSON line per measurement.
// Built by seqlib_amd/build.py with g++ against libseqlib_amd.so; scripts/make_bench_bam.py --sorted / --shuffled writes in.bam.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/Pileup.h"
#include "SeqLib/RefGenome.h"
#include "seqlib_amd_cov.h"
#include "seqlib_amd_pile.h"

using namespace SeqLib;
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#define OK(x) do { if ((x) != SLX_OK) { std::fprintf(stderr, "bampile_bench: %s\n", slx_last_error()); return 1; } } while (0)

struct Stat { double med, lo, hi; };
static Stat stat(std::vector<double> v) { std::sort(v.begin(), v.end()); return Stat{v[v.size() / 2], v.front(), v.back()}; }
static void put(const char *what, const char *unit, const Stat &s, const std::string &extra = "")
{
    std::printf("{\"what\": \"%s\", \"unit\": \"%s\", \"median\": %.3f, \"min\": %.3f, \"max\": %.3f%s%s}\n", what, unit, s.med, s.lo, s.hi, extra.empty() ? "" : ", ", extra.c_str());
    std::fflush(stdout);
}

// the host loop: what a SeqLib user writes today, by the rules of seqlib_amd_pile.h with the default knobs
typedef std::vector<std::vector<int32_t>> Planes;          // per contig: 15 planes of len entries
static void host_walk(const BamRecordPtrVector &recs, const std::vector<int64_t> &len, Planes &pl, int only)
{
    static const uint8_t base_of[16] = {4, 0, 1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4};
    for (const BamRecordPtr &rp : recs) {
        const bam1_t *b = rp->raw();
        const bam1_core_t &c = b->core;
        if (c.tid < 0 || c.tid >= (int)len.size() || (only >= 0 && c.tid != only) || c.pos < 0 || (c.flag & 0x704) || c.n_cigar == 0 || c.l_qseq == 0) continue;
        const int64_t L = len[(size_t)c.tid];
        int32_t *p = pl[(size_t)c.tid].data();
        const uint32_t *cig = bam_get_cigar(b);
        const uint8_t *seq = bam_get_seq(b);
        const int64_t s = (c.flag & 0x10) ? 7 : 0, ls = c.l_qseq;
        int64_t x = c.pos, y = 0;
        bool stop = false;
        for (uint32_t k = 0; k < c.n_cigar && !stop; ++k) {
            const uint32_t op = cig[k] & 15u, n = cig[k] >> 4;
            if (op == 0 || op == 7 || op == 8) {
                for (uint32_t i = 0; i < n; ++i, ++x, ++y) {
                    if (y >= ls) { stop = true; break; }
                    if (x < L) ++p[(s + base_of[(seq[y >> 1] >> ((~y & 1) << 2)) & 15]) * L + x];          // (min_baseq 0: every base passes)
                }
            } else if (op == 2) { for (uint32_t i = 0; i < n; ++i, ++x) if (x < L) ++p[(s + 5) * L + x]; }
            else if (op == 1) { if (x - 1 >= 0 && x - 1 < L) ++p[(s + 6) * L + x - 1]; y += n; }
            else if (op == 4) y += n;
            else if (op == 3) x += n;
        }
    }
}
static int host_route(const std::string &in, const std::vector<int64_t> &len, Planes &pl, int only, double *secs, int64_t *n_out)
{
    BamReader r;
    if (!r.Open(in)) return 1;
    const double t0 = now();
    pl.clear();
    for (size_t t = 0; t < len.size(); ++t) pl.emplace_back(only < 0 || (int)t == only ? (size_t)(15 * len[t]) : (size_t)0, 0);
    int64_t n = 0;
    for (;;) {
        BamRecordPtrVector recs;
        if (!r.NextBatch(recs, 1 << 18)) break;
        n += (int64_t)recs.size();
        host_walk(recs, len, pl, only);
    }
    *secs = now() - t0; *n_out = n;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: bampile_bench <in.bam> <ref.fa> [reps]\n"); return 2; }
    const std::string in = argv[1], fa = argv[2];
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
        // ---- the host loop
        Planes hp;
        std::vector<double> h1;
        double s = 0; int64_t n_host = 0;
        // one window, as one pileup object holds it: the contig with the most bases, whole
        int big = 0;
        for (int t = 1; t < n_ref; ++t) if (len[(size_t)t] > len[(size_t)big]) big = t;
        std::vector<double> hw;
        for (int rep = 0; rep <= reps; ++rep) { if (host_route(in, len, hp, big, &s, &n_host)) return 1; if (rep) hw.push_back(s); }
        const Planes hp_window = hp;
        for (int rep = 0; rep <= reps; ++rep) { if (host_route(in, len, hp, -1, &s, &n_host)) return 1; if (rep) h1.push_back(s); }
        // ---- the file as one device-resident batch, and the check
        slx_bam *rd = nullptr;
        OK(slx_bam_open(in.c_str(), -1, &rd));
        slx_bam_batch bt;
        OK(slx_bam_next(rd, (int64_t)1 << 40, &bt));
        std::vector<slx_pile *> pile((size_t)n_ref, nullptr);
        for (int t = 0; t < n_ref; ++t) {
            const slx_bam_region w = {t, 0, len[(size_t)t]};
            OK(slx_pile_create(-1, n_ref, len.data(), nm.data(), &w, &pile[(size_t)t]));
            OK(slx_pile_add_device(pile[(size_t)t], bt.d_stream, bt.n_bytes, bt.d_rec_off, bt.n_records));
            std::vector<int32_t> g((size_t)len[(size_t)t]);
            for (int p = 0; p < SLX_PILE_PLANES; ++p) {
                OK(slx_pile_counts(pile[(size_t)t], p, 0, len[(size_t)t], g.data()));
                if (bt.n_records != n_host || !std::equal(g.begin(), g.end(), hp[(size_t)t].begin() + (size_t)p * g.size())) { std::fprintf(stderr, "bampile_bench: the GPU's plane %d of contig %d is not the host loop's\n", p, t); return 1; }
            }
        }
        const std::string common = "\"records\": " + std::to_string(bt.n_records) + ", \"record_bytes\": " + std::to_string(bt.n_bytes) + ", \"planes_equal_host\": true";
        put("host_1_thread_all_contigs", "s", stat(h1), common);
        // ---- add: the plain form against the window, at each group width, beside the coverage unit's add on the same batch
        auto add_all = [&](double *kernel_ms, int64_t *lds, int64_t *glob) -> int {
            *kernel_ms = 0; *lds = *glob = 0;
            for (slx_pile *p : pile) {
                OK(slx_pile_clear(p));
                const int64_t u0 = slx_pile_counter(p, "us_add"), l0 = slx_pile_counter(p, "events_lds"), g0 = slx_pile_counter(p, "events_global");
                OK(slx_pile_add_device(p, bt.d_stream, bt.n_bytes, bt.d_rec_off, bt.n_records));
                *kernel_ms += (double)(slx_pile_counter(p, "us_add") - u0) / 1e3; *lds += slx_pile_counter(p, "events_lds") - l0; *glob += slx_pile_counter(p, "events_global") - g0;
            }
            return 0;
        };
        for (const int64_t slice : {256, 1024}) for (const int64_t w : {0, 256, 512, 1024}) for (const int64_t g : {16, 32, 64}) {
            for (slx_pile *p : pile) { OK(slx_pile_set(p, "lds_window", w)); OK(slx_pile_set(p, "group_lanes", g)); OK(slx_pile_set(p, "slice_records", slice)); }
            std::vector<double> k, wall;
            int64_t lds = 0, glob = 0;
            for (int rep = 0; rep <= reps; ++rep) {
                double ms = 0;
                const double t0 = now();
                if (add_all(&ms, &lds, &glob)) return 1;
                if (rep) { wall.push_back((now() - t0) * 1e3); k.push_back(ms); }
            }
            const std::string x = "\"lds_window\": " + std::to_string(w) + ", \"group_lanes\": " + std::to_string(g) + ", \"slice_records\": " + std::to_string(slice) + ", \"events_lds\": " + std::to_string(lds) +
                                  ", \"events_global\": " + std::to_string(glob);
            put("add_kernels", "ms", stat(k), x);
            put("add_wall", "ms", stat(wall), x);
        }
        {
            slx_cov *cov = nullptr;
            OK(slx_cov_create(-1, n_ref, len.data(), nm.data(), nullptr, &cov));
            std::vector<double> k;
            for (int rep = 0; rep <= reps; ++rep) {
                OK(slx_cov_clear(cov));
                const int64_t u0 = slx_cov_counter(cov, "us_add");
                OK(slx_cov_add_device(cov, bt.d_stream, bt.n_bytes, bt.d_rec_off, bt.n_records));
                if (rep) k.push_back((double)(slx_cov_counter(cov, "us_add") - u0) / 1e3);
            }
            put("cov_add_kernels", "ms", stat(k));
            slx_cov_free(cov);
        }
        for (slx_pile *p : pile) slx_pile_free(p);
        slx_bam_close(rd);
        // ---- the whole route from the file with the default knobs: one window, one pass, against the host loop over the same window
        {
            std::vector<double> route;
            for (int rep = 0; rep <= reps; ++rep) {
                BamReader r;
                if (!r.Open(in)) return 1;
                const double t0 = now();
                Pileup P(GenomicRegion(big, 0, (int32_t)len[(size_t)big]));
                const size_t n = P.addReads(r);
                std::vector<std::vector<int32_t>> g;
                for (int p = 0; p < SLX_PILE_PLANES; ++p) g.push_back(P.Counts(p));
                if (rep) route.push_back(now() - t0);
                if ((int64_t)n != n_host) { std::fprintf(stderr, "bampile_bench: addReads handed over %zu of %lld records\n", n, (long long)n_host); return 1; }
                for (int p = 0; p < SLX_PILE_PLANES; ++p)
                    if (!std::equal(g[(size_t)p].begin(), g[(size_t)p].end(), hp_window[(size_t)big].begin() + (size_t)p * g[(size_t)p].size())) { std::fprintf(stderr, "bampile_bench: the route's plane %d is not the host loop's\n", p); return 1; }
            }
            const std::string w = "\"contig\": " + std::to_string(big) + ", \"positions\": " + std::to_string(len[(size_t)big]);
            put("host_1_thread_window", "s", stat(hw), w);
            put("route_file_to_planes_window", "s", stat(route), w + ", \"vs_host_1_thread_window\": " + std::to_string(stat(hw).med / stat(route).med));
        }
        // ---- every contig, a pass over the file each (there is no all-contigs object), and the sites
        std::vector<double> route, sites_k, sites_wall;
        int64_t n_sites = 0;
        RefGenome ref;
        if (!ref.LoadIndex(fa)) return 1;
        for (int rep = 0; rep <= reps; ++rep) {
            const double t0 = now();
            std::vector<std::unique_ptr<Pileup>> P;
            size_t n = 0;
            int64_t acc = 0;
            for (int t = 0; t < n_ref; ++t) {
                BamReader r;
                if (!r.Open(in)) return 1;
                P.emplace_back(new Pileup(GenomicRegion(t, 0, (int32_t)len[(size_t)t])));
                n = P.back()->addReads(r);
                const std::vector<int32_t> a = P.back()->Counts(SLX_PILE_A);
                acc += a.empty() ? 0 : a[a.size() / 2];
            }
            if (rep) route.push_back(now() - t0);
            if ((int64_t)n != n_host) { std::fprintf(stderr, "bampile_bench: addReads handed over %zu of %lld records (%lld)\n", n, (long long)n_host, (long long)acc); return 1; }
            const double t1 = now();
            double us = 0;
            n_sites = 0;
            for (auto &p : P) { const int64_t u0 = p->Counter("us_sites"); n_sites += (int64_t)p->Sites(ref, 10, 3, 1, 50).size(); us += (double)(p->Counter("us_sites") - u0); }
            if (rep) { sites_wall.push_back((now() - t1) * 1e3); sites_k.push_back(us / 1e3); }
        }
        put("route_file_to_planes_all_contigs", "s", stat(route), "\"vs_host_1_thread_all_contigs\": " + std::to_string(stat(h1).med / stat(route).med) + ", \"passes_over_the_file\": " + std::to_string(n_ref));
        put("sites_kernels", "ms", stat(sites_k), "\"sites\": " + std::to_string(n_sites));
        put("sites_wall", "ms", stat(sites_wall));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bampile_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
