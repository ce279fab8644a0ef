// bammarkdup_bench -- what marking duplicates in HBM buys, against the host loop a user would write through BamRecords, from one process:
//     gpu        DuplicateMarker::MarkFile: reader -> marker (pass 1), reader -> apply in HBM -> GPU BGZF writer (pass 2); no record on the host
//     host_loop  one thread: Next() into hash maps keyed by name and by 5' end (the same rules, the per-record body of dup_host.h on the CPU), then Next()
//                again, the flag set, WriteRecord through the host (zlib) BamWriter
//   bammarkdup_bench <in.bam> <out_prefix> [reps]
// <in.bam>: scripts/make_bench_bam.py --shuffled --pairs.  Every figure is the median of reps runs (at least 3) after one warm-up, with the fastest and the
// slowest beside it.  The stage times are the marker's counters of the LAST repetition.  The two jobs must agree on the number of duplicates.  Prints one JSON
// line per measurement.  Built by seqlib_amd/build.py with g++ against libseqlib_amd.so.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <optional>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/BamWriter.h"
#include "SeqLib/DuplicateMarker.h"
#include "dup_host.h"

using namespace SeqLib;

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct Stat { double med, lo, hi; };
static Stat stat(std::vector<double> v) { std::sort(v.begin(), v.end()); return Stat{v[v.size() / 2], v.front(), v.back()}; }
struct Run {
    double pass1 = 0, total = 0;
    long long records = 0, duplicates = 0, pairs = 0;
    long long us_sig = 0, us_commit = 0, us_join = 0, us_pairs = 0, us_group = 0, us_apply = 0, held = 0;
};

static bool gpu_job(const std::string &in, const std::string &out, Run &r)
{
    const double t0 = now();
    DuplicateMarker m;
    m.MarkFile(in, out);
    r.total = now() - t0;
    r.pass1 = (double)(m.Counter("us_sig") + m.Counter("us_place") + m.Counter("us_commit") + m.Counter("us_join") + m.Counter("us_pairs") + m.Counter("us_group")) * 1e-6;          // (kernel time only)
    r.records = m.Counter("records"); r.duplicates = m.Counter("duplicates"); r.pairs = m.Counter("pairs");
    r.us_sig = m.Counter("us_sig"); r.us_commit = m.Counter("us_commit"); r.us_join = m.Counter("us_join"); r.us_pairs = m.Counter("us_pairs"); r.us_group = m.Counter("us_group");
    r.us_apply = m.Counter("us_apply"); r.held = m.Counter("held_bytes");
    return true;
}

typedef std::tuple<uint64_t, uint64_t> End;          // E(r): the two words of dup_host.h
struct HostRec { End e; uint32_t cls, score; };

static bool host_job(const std::string &in, const std::string &out, Run &r)
{
    const double t0 = now();
    BamReader rd;
    if (!rd.Open(in)) return false;
    const BamHeader hdr = rd.Header();
    dp_header H;
    const std::string text = hdr.AsString();
    if (!H.parse(text.data(), (int64_t)text.size())) return false;
    const dp_libtab T = H.view();
    std::vector<HostRec> recs;
    std::unordered_map<std::string, std::vector<uint32_t> > by_name;
    while (std::optional<BamRecord> rec = rd.Next()) {
        const std::vector<uint8_t> p = detail::packed_record(rec->raw());
        uint32_t seq_at = 0, aux_at = 0;
        dp_sig s;
        if (!dp_head(p.data(), (uint32_t)p.size(), &seq_at, &aux_at)) return false;
        dp_signature<false>(T, p.data(), (uint32_t)p.size(), seq_at, aux_at, 0, 1, &s);
        if ((s.cls & DP_CLASS) == DP_PAIRED) by_name[std::string(1, (char)s.library) + std::string(1, (char)(s.library >> 8)) + rec->Qname()].push_back((uint32_t)recs.size());
        recs.push_back(HostRec{End(s.hi, s.lo), s.cls, s.score});
    }
    std::vector<uint8_t> dup(recs.size(), 0);
    std::map<std::tuple<End, End>, std::vector<std::pair<uint32_t, uint32_t> > > by_ends;
    for (const auto &kv : by_name) {
        const std::vector<uint32_t> &g = kv.second;
        if (g.size() != 2) continue;
        const uint32_t a = recs[g[0]].cls, b = recs[g[1]].cls;
        if (!(((a & DP_FIRST) && (b & DP_SECOND)) || ((a & DP_SECOND) && (b & DP_FIRST)))) continue;
        const End ea = recs[g[0]].e, eb = recs[g[1]].e;
        by_ends[std::make_tuple(std::min(ea, eb), std::max(ea, eb))].push_back(std::make_pair(g[0], g[1]));
        ++r.pairs;
    }
    for (const auto &kv : by_ends) {
        size_t best = 0;
        auto score = [&](const std::pair<uint32_t, uint32_t> &p) { return (uint64_t)recs[p.first].score + recs[p.second].score; };
        for (size_t i = 1; i < kv.second.size(); ++i)
            if (score(kv.second[i]) > score(kv.second[best]) || (score(kv.second[i]) == score(kv.second[best]) && kv.second[i].first < kv.second[best].first)) best = i;
        for (size_t i = 0; i < kv.second.size(); ++i) if (i != best) dup[kv.second[i].first] = dup[kv.second[i].second] = 1;
    }
    std::map<End, std::vector<uint32_t> > by_e;
    for (uint32_t o = 0; o < recs.size(); ++o) if ((recs[o].cls & DP_CLASS) != DP_IGNORED) by_e[recs[o].e].push_back(o);
    for (const auto &kv : by_e) {
        bool any_paired = false;
        int64_t best = -1;
        for (uint32_t o : kv.second) {
            if ((recs[o].cls & DP_CLASS) == DP_PAIRED) any_paired = true;
            else if (best < 0 || recs[o].score > recs[(size_t)best].score) best = o;
        }
        for (uint32_t o : kv.second) if ((recs[o].cls & DP_CLASS) == DP_FRAGMENT && (any_paired || (int64_t)o != best)) dup[o] = 1;
    }
    r.pass1 = now() - t0;
    BamReader rd2;
    if (!rd2.Open(in)) return false;
    BamWriter w(BAM);
    w.SetHeader(hdr);
    if (!w.Open(out) || !w.WriteHeader()) return false;
    size_t o = 0;
    while (std::optional<BamRecord> rec = rd2.Next()) {
        if (o >= recs.size()) return false;
        bam1_t *b = const_cast<bam1_t *>(rec->raw());
        if ((recs[o].cls & DP_CLASS) != DP_IGNORED) b->core.flag = (uint16_t)(dup[o] ? b->core.flag | 0x400 : b->core.flag & ~0x400);
        r.duplicates += dup[o];
        if (!w.WriteRecord(*rec)) return false;
        ++o;
    }
    if (!w.Close()) return false;
    r.total = now() - t0;
    r.records = (long long)recs.size();
    return true;
}

static void put(const char *what, const std::vector<Run> &runs)
{
    std::vector<double> p, t;
    for (const Run &r : runs) { p.push_back(r.pass1); t.push_back(r.total); }
    const Stat sp = stat(p), st = stat(t);
    const Run &r = runs.back();
    std::printf("{\"what\": \"%s\", \"unit\": \"s\", \"total_median\": %.4f, \"total_min\": %.4f, \"total_max\": %.4f, \"pass1_median\": %.4f, \"records\": %lld, \"pairs\": %lld, "
                "\"duplicates\": %lld, \"records_per_s\": %.0f, \"us_sig\": %lld, \"us_commit\": %lld, \"us_join\": %lld, \"us_pairs\": %lld, \"us_group\": %lld, \"us_apply\": %lld, "
                "\"held_bytes\": %lld}\n",
                what, st.med, st.lo, st.hi, sp.med, r.records, r.pairs, r.duplicates, (double)r.records / st.med, r.us_sig, r.us_commit, r.us_join, r.us_pairs, r.us_group, r.us_apply, r.held);
    std::fflush(stdout);
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: bammarkdup_bench <in.bam> <out_prefix> [reps]\n"); return 2; }
    const std::string in = argv[1], prefix = argv[2];
    const int reps = std::max(3, argc > 3 ? std::atoi(argv[3]) : 3);
    try {
        const char *names[2] = {"gpu", "host_loop"};
        long long dups[2] = {0, 0};
        for (int job = 0; job < 2; ++job) {
            std::vector<Run> runs;
            for (int k = 0; k <= reps; ++k) {
                Run r;
                const bool ok = job == 0 ? gpu_job(in, prefix + ".gpu.bam", r) : host_job(in, prefix + ".host.bam", r);
                if (!ok) { std::fprintf(stderr, "bammarkdup_bench: %s failed: %s\n", names[job], slx_last_error()); return 1; }
                if (k) runs.push_back(r);          // (the first run warms up)
            }
            dups[job] = runs.back().duplicates;
            put(names[job], runs);
        }
        if (dups[0] != dups[1]) { std::fprintf(stderr, "bammarkdup_bench: the gpu marks %lld duplicates, the host loop %lld\n", dups[0], dups[1]); return 1; }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bammarkdup_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
