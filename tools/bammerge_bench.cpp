// bammerge_bench -- what the k-way merge in HBM costs and buys, and what a sort that spills runs costs next to one that fits, from one process and one file.
//   merge   <sorted.bam> (scripts/make_bench_bam.py --sorted) is dealt into k = 2, 8 and 32 sorted files by record ordinal (record j to file j % k).  Per k,
//           [reps] runs each, alternating, median and range:
//     (a) slx_merge_files' route with by_sort 0  the rank kernel: readers, keys, ranks, tile gather, DEFLATE, the file; and its stages from the merger's counters
//     (b) the same with by_sort 1                hipCUB's radix sort in place of the rank kernel
//     (c) a one-thread host loop                 k BamReaders (GPU inflate), a heap on (key, input), BamWriter::WriteRecord into a UseGpu() writer (GPU DEFLATE):
//                                                both sides of it are the GPU's, the merge itself is the host's
//           (a) and (b) must write identical files, and (c)'s records must be theirs.
//   spill   slx_sort_file_spill of <file to sort> (default: the same file) with max_bytes at a quarter of its inflated size, against slx_sort_file_ex with
//           everything in HBM; the two files must be identical.
//   bammerge_bench <sorted.bam> <scratch prefix> [reps] [file to sort]
// Prints one JSON line per k and one for the spill.  Built by seqlib_amd/build.py with g++ against libseqlib_amd.so.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <queue>
#include <string>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/BamWriter.h"
#include "seqlib_amd_bam.h"
#include "seqlib_amd_merge.h"
#include "seqlib_amd_sort.h"

using namespace SeqLib;
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct Runs {
    std::vector<double> s;
    double med() const { std::vector<double> v = s; std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
    double lo() const { return *std::min_element(s.begin(), s.end()); }
    double hi() const { return *std::max_element(s.begin(), s.end()); }
};
#define DIE() do { std::fprintf(stderr, "bammerge_bench: line %d: %s\n", __LINE__, slx_last_error()); return 1; } while (0)

static std::string slurp(const std::string &p) { std::ifstream f(p, std::ios::binary); return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>()); }

// the inflated bytes of a BGZF file
static int inflate(const std::string &path, std::vector<unsigned char> &out)
{
    slx_bam_member *mem = nullptr; int64_t nm = 0; int eof = 0;
    if (slx_bam_scan_members(path.c_str(), &mem, &nm, &eof) != SLX_OK) return 1;
    uint64_t total = 0, got = 0;
    for (int64_t i = 0; i < nm; ++i) total += mem[i].isize;
    slx_bam_members_free(mem);
    out.resize(total);
    return slx_bam_inflate_file(path.c_str(), -1, out.data(), total, &got) != SLX_OK || got != total;
}
static uint32_t ld32(const unsigned char *p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
static uint64_t first_record(const std::vector<unsigned char> &s)
{
    uint64_t first = 12 + ld32(&s[4]);
    for (uint32_t r = ld32(&s[first - 4]); r; --r) first += 8 + ld32(&s[first]);
    return first;
}

struct Stage { int64_t key, rank, gather, rounds, refills; };
static int gpu_merge(const std::vector<std::string> &in, const std::string &out, int by_sort, double *secs, Stage *st)
{
    const double t0 = now();
    slx_merge *m = nullptr;
    if (slx_merge_create(-1, &m) != SLX_OK) return 1;
    int rc = slx_merge_set(m, "by_sort", by_sort);
    for (size_t i = 0; rc == SLX_OK && i < in.size(); ++i) rc = slx_merge_add_file(m, in[i].c_str());
    const char *h = nullptr; int64_t l = 0;
    if (rc == SLX_OK) rc = slx_merge_header(m, &h, &l);
    slx_bgzf *w = nullptr;
    if (rc == SLX_OK) rc = slx_bgzf_open(out.c_str(), -1, &w);
    if (rc == SLX_OK) rc = slx_bgzf_write(w, h, l);
    if (rc == SLX_OK) rc = slx_bgzf_flush(w);
    if (rc == SLX_OK) rc = slx_merge_run(m, w);
    if (w && slx_bgzf_close(w) != SLX_OK && rc == SLX_OK) rc = SLX_EIO;
    *secs = now() - t0;
    if (rc == SLX_OK) *st = Stage{slx_merge_counter(m, "us_key"), slx_merge_counter(m, "us_rank"), slx_merge_counter(m, "us_gather"), slx_merge_counter(m, "rounds"), slx_merge_counter(m, "refills")};
    slx_merge_free(m);
    return rc != SLX_OK;
}

// (c): one record per reader in a heap on (key, input)
static int host_merge(const std::vector<std::string> &in, const std::string &out, double *secs, int64_t *n_out)
{
    const double t0 = now();
    std::vector<std::unique_ptr<BamReader>> rd;
    for (const std::string &p : in) { rd.emplace_back(new BamReader()); if (!rd.back()->Open(p)) return 1; }
    BamWriter w;
    w.SetHeader(rd[0]->Header());
    if (!w.UseGpu() || !w.Open(out) || !w.WriteHeader()) return 1;
    typedef std::pair<uint64_t, size_t> Item;
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    std::vector<BamRecord> cur(in.size());
    auto key = [](const BamRecord &r) { return (uint64_t)(uint32_t)r.ChrID() << 32 | (uint64_t)((uint32_t)r.Position() ^ 0x80000000u); };
    for (size_t i = 0; i < in.size(); ++i) if (rd[i]->GetNextRecord(cur[i])) heap.push(Item(key(cur[i]), i));
    int64_t n = 0;
    while (!heap.empty()) {
        const size_t i = heap.top().second;
        heap.pop();
        if (!w.WriteRecord(cur[i])) return 1;
        ++n;
        if (rd[i]->GetNextRecord(cur[i])) heap.push(Item(key(cur[i]), i));
    }
    if (!w.Close()) return 1;
    *secs = now() - t0; *n_out = n;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: bammerge_bench <sorted.bam> <scratch prefix> [reps] [file to sort]\n"); return 2; }
    const std::string path = argv[1], pre = argv[2], to_sort = argc > 4 ? argv[4] : argv[1];
    const int reps = argc > 3 ? std::max(1, std::atoi(argv[3])) : 3;
    for (int k : {2, 8, 32}) {
        // ---- the deal
        std::vector<std::string> in;
        int64_t records = 0;
        {
            BamReader r;
            if (!r.Open(path)) return 1;
            std::vector<std::unique_ptr<BamWriter>> w;
            for (int i = 0; i < k; ++i) {
                in.push_back(pre + ".in" + std::to_string(k) + "_" + std::to_string(i) + ".bam");
                w.emplace_back(new BamWriter());
                w.back()->SetHeader(r.Header());
                if (!w.back()->UseGpu() || !w.back()->Open(in.back()) || !w.back()->WriteHeader()) return 1;
            }
            BamRecord rec;
            while (r.GetNextRecord(rec)) { if (!w[(size_t)(records % k)]->WriteRecord(rec)) return 1; ++records; }
            for (auto &x : w) if (!x->Close()) return 1;
        }
        const std::string out0 = pre + ".merged0.bam", out1 = pre + ".merged1.bam", outh = pre + ".mergedh.bam";
        double s = 0; Stage st = {};
        if (gpu_merge(in, out0, 0, &s, &st) || gpu_merge(in, out1, 1, &s, &st)) DIE();          // (the first passes load the kernels: not timed)
        Runs a, b, c, ak, ar, ag, bk, br, bg;
        Stage sa = {}, sb = {};
        int64_t n_host = 0;
        for (int rep = 0; rep < reps; ++rep) {
            if (gpu_merge(in, out0, 0, &s, &sa)) DIE();
            a.s.push_back(s); ak.s.push_back((double)sa.key); ar.s.push_back((double)sa.rank); ag.s.push_back((double)sa.gather);
            if (gpu_merge(in, out1, 1, &s, &sb)) DIE();
            b.s.push_back(s); bk.s.push_back((double)sb.key); br.s.push_back((double)sb.rank); bg.s.push_back((double)sb.gather);
            if (rep == 0 || reps > 2) { if (host_merge(in, outh, &s, &n_host)) DIE(); c.s.push_back(s); }
        }
        if (slurp(out0) != slurp(out1)) { std::fprintf(stderr, "bammerge_bench: by_sort 0 and 1 wrote different files at k = %d\n", k); return 1; }
        std::vector<unsigned char> g, h;
        if (inflate(out0, g) || inflate(outh, h)) DIE();
        const uint64_t fg = first_record(g), fh = first_record(h);
        if (n_host != records || g.size() - fg != h.size() - fh || std::memcmp(g.data() + fg, h.data() + fh, g.size() - fg) != 0) {
            std::fprintf(stderr, "bammerge_bench: the merged records differ from the host loop's at k = %d\n", k);
            return 1;
        }
        const double B = (double)(g.size() - fg);
        std::printf("{\"what\": \"merge\", \"k\": %d, \"records\": %lld, \"record_bytes\": %.0f, \"reps\": %d, \"rounds\": %lld, \"refills\": %lld, "
                    "\"rank_file_s\": [%.3f, %.3f, %.3f], \"rank_GBps\": %.3f, \"rank_us_key\": %.0f, \"rank_us_rank\": [%.0f, %.0f, %.0f], \"rank_us_gather\": %.0f, "
                    "\"sort_file_s\": [%.3f, %.3f, %.3f], \"sort_us_key\": %.0f, \"sort_us_rank\": [%.0f, %.0f, %.0f], \"sort_us_gather\": %.0f, "
                    "\"host_heap_s\": [%.3f, %.3f, %.3f], \"host_over_rank\": %.2f}\n",
                    k, (long long)records, B, reps, (long long)sa.rounds, (long long)sa.refills,
                    a.lo(), a.med(), a.hi(), B / a.med() / 1e9, ak.med(), ar.lo(), ar.med(), ar.hi(), ag.med(),
                    b.lo(), b.med(), b.hi(), bk.med(), br.lo(), br.med(), br.hi(), bg.med(),
                    c.lo(), c.med(), c.hi(), c.med() / a.med());
        std::fflush(stdout);
        for (const std::string &p : in) std::remove(p.c_str());
        std::remove(out0.c_str()); std::remove(out1.c_str()); std::remove(outh.c_str());
    }
    // ---- the spill
    {
        std::vector<unsigned char> g;
        if (inflate(to_sort, g)) DIE();
        const int64_t B = (int64_t)(g.size() - first_record(g));
        g.clear(); g.shrink_to_fit();
        const std::string fit = pre + ".fit.bam", spl = pre + ".spill.bam";
        slx_sort *s_fit = nullptr, *s_spl = nullptr;
        if (slx_sort_create(-1, &s_fit) != SLX_OK || slx_sort_create(-1, &s_spl) != SLX_OK) DIE();
        if (slx_sort_set(s_spl, "max_bytes", std::max<int64_t>(B / 4, 1)) != SLX_OK) DIE();
        if (slx_sort_file_ex(s_fit, to_sort.c_str(), fit.c_str()) != SLX_OK || slx_sort_file_spill(s_spl, to_sort.c_str(), spl.c_str(), nullptr) != SLX_OK) DIE();          // not timed
        Runs a, b, um;
        int64_t runs = 0;
        for (int rep = 0; rep < reps; ++rep) {
            double t0 = now();
            if (slx_sort_file_ex(s_fit, to_sort.c_str(), fit.c_str()) != SLX_OK) DIE();
            a.s.push_back(now() - t0);
            const int64_t r0 = slx_sort_counter(s_spl, "runs"), m0 = slx_sort_counter(s_spl, "us_merge");
            t0 = now();
            if (slx_sort_file_spill(s_spl, to_sort.c_str(), spl.c_str(), nullptr) != SLX_OK) DIE();
            b.s.push_back(now() - t0);
            runs = slx_sort_counter(s_spl, "runs") - r0; um.s.push_back((double)(slx_sort_counter(s_spl, "us_merge") - m0));
        }
        if (slurp(fit) != slurp(spl)) { std::fprintf(stderr, "bammerge_bench: the spilling sort wrote another file than the sort in HBM\n"); return 1; }
        std::printf("{\"what\": \"spill\", \"record_bytes\": %lld, \"max_bytes\": %lld, \"runs\": %lld, \"reps\": %d, \"in_hbm_s\": [%.3f, %.3f, %.3f], \"spill_s\": [%.3f, %.3f, %.3f], "
                    "\"us_merge\": [%.0f, %.0f, %.0f], \"spill_over_in_hbm\": %.2f}\n",
                    (long long)B, (long long)(B / 4), (long long)runs, reps, a.lo(), a.med(), a.hi(), b.lo(), b.med(), b.hi(), um.lo(), um.med(), um.hi(), b.med() / a.med());
        slx_sort_free(s_fit); slx_sort_free(s_spl);
        std::remove(fit.c_str()); std::remove(spl.c_str());
    }
    return 0;
}
