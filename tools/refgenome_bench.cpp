// refgenome_bench -- what the reference genome on the GPU buys, against the host loops a user would write, from one process:
//     load      the whole of slx_ref_open (read, line pass, index, compaction into HBM) against one host thread that reads the file, builds the .fai by the same
//               rules (ref_host.h) and strips the line ends into one buffer per contig; the kernels' own times from the unit's HIP events beside it
//     fetch     a batch of regions through slx_ref_fetch_device (the bytes stay in HBM) against a host memcpy loop over the host copy of the contigs; per
//               gather_tile_bytes, kernel time from "us_fetch"
//     nm_md     slx_ref_nm_md_device over the records of <mapped.bam> as one device-resident batch against a host loop that runs the kernels' body per record
//               (rg_record_nm_md), per long_record; kernel times from "us_md_size" and "us_md_text"
//   refgenome_bench <big.fa> <small.fa> <mapped.bam> [reps]
// <big.fa>: scripts/make_bench_fasta.py; <mapped.bam>: scripts/make_bench_bam.py --sorted --ref <small.fa>, whose records are placed on <small.fa>'s contigs.
// Results are compared before anything is timed.  Every figure is the median of reps runs (at least 5) after one warm-up, with the fastest and the slowest beside
// it.  GB/s count the bytes the step must move (named per line); "hbm_share" is that rate over 8 TB/s.  Prints one JSON line per measurement.  Built by
// seqlib_amd/build.py with g++ against libseqlib_amd.so.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <string>
#include <vector>
#include "seqlib_amd_bam.h"
#include "seqlib_amd_ref.h"
#include "ref_host.h"

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#define OK(x) do { if ((x) != SLX_OK) { std::fprintf(stderr, "refgenome_bench: %s\n", slx_last_error()); return 1; } } while (0)
static const double HBM_PEAK = 8e12;

struct Stat { double med, lo, hi; };
static Stat stat(std::vector<double> v) { std::sort(v.begin(), v.end()); return Stat{v[v.size() / 2], v.front(), v.back()}; }
static void put(const char *what, const char *unit, const Stat &s, const std::string &extra = "")
{
    std::printf("{\"what\": \"%s\", \"unit\": \"%s\", \"median\": %.3f, \"min\": %.3f, \"max\": %.3f%s%s}\n", what, unit, s.med, s.lo, s.hi, extra.empty() ? "" : ", ", extra.c_str());
    std::fflush(stdout);
}
static std::string rate(double bytes, double seconds) { return ", \"bytes\": " + std::to_string((long long)bytes) + ", \"GB_per_s\": " + std::to_string(bytes / seconds / 1e9) + ", \"hbm_share\": " + std::to_string(bytes / seconds / HBM_PEAK); }

// the host loop of the load: the file into memory, the index by the rules, the bases of every contig without their line ends
static bool host_load(const std::string &path, std::string *fai, std::vector<std::string> *bases)
{
    std::ifstream f(path, std::ios::binary);
    std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<rg_contig> C;
    std::string msg;
    if (!rg_fai_of_text((const uint8_t *)text.data(), text.size(), &C, &msg)) { std::fprintf(stderr, "refgenome_bench: %s\n", msg.c_str()); return false; }
    *fai = rg_fai_text(C);
    bases->assign(C.size(), std::string());
    for (size_t i = 0; i < C.size(); ++i) {
        std::string &b = (*bases)[i];
        b.resize((size_t)C[i].len);
        for (int64_t done = 0; done < C[i].len; done += C[i].lb) {
            const int64_t k = std::min<int64_t>(C[i].lb, C[i].len - done);
            std::memcpy(&b[(size_t)done], text.data() + C[i].off + (uint64_t)(done / C[i].lb) * C[i].lw, (size_t)k);
        }
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: refgenome_bench <big.fa> <small.fa> <mapped.bam> [reps]\n"); return 2; }
    const std::string big = argv[1], small = argv[2], bam = argv[3];
    const int reps = std::max(5, argc > 4 ? std::atoi(argv[4]) : 5);
    // ---- (a) the load
    std::string fai;
    std::vector<std::string> bases;
    std::vector<double> th, tg, k_lines, k_class, k_gather, k_inflate;
    for (int rep = 0; rep <= reps; ++rep) {
        const double t0 = now();
        if (!host_load(big, &fai, &bases)) return 1;
        if (rep) th.push_back(now() - t0);
    }
    slx_ref *r = nullptr;
    int64_t text_bytes = 0, n_bases = 0;
    for (int rep = 0; rep <= reps; ++rep) {
        if (r) slx_ref_close(r);
        const double t0 = now();
        OK(slx_ref_open(big.c_str(), -1, &r));
        if (rep) {
            tg.push_back(now() - t0);
            k_lines.push_back((double)slx_ref_counter(r, "us_lines") / 1e3); k_class.push_back((double)slx_ref_counter(r, "us_class") / 1e3);
            k_gather.push_back((double)slx_ref_counter(r, "us_gather") / 1e3); k_inflate.push_back((double)slx_ref_counter(r, "us_inflate") / 1e3);
        }
        text_bytes = slx_ref_counter(r, "text_bytes"); n_bases = slx_ref_counter(r, "bases");
    }
    {
        int64_t n = 0;
        const char *t = slx_ref_fai_text(r, &n);
        if (std::string(t, (size_t)n) != fai || slx_ref_nseq(r) != (int64_t)bases.size()) { std::fprintf(stderr, "refgenome_bench: the index differs from the host loop's\n"); return 1; }
        for (int64_t i = 0; i < slx_ref_nseq(r); ++i) {
            const slx_bam_region g = {(int32_t)i, 0, slx_ref_len(r, i)};
            uint64_t offs[2];
            std::string got((size_t)slx_ref_len(r, i), '\0');
            OK(slx_ref_fetch_host(r, &g, 1, 0, got.empty() ? nullptr : &got[0], (int64_t)got.size(), offs));
            if (got != bases[(size_t)i]) { std::fprintf(stderr, "refgenome_bench: contig %lld differs from the host loop's\n", (long long)i); return 1; }
        }
    }
    const std::string common = "\"text_bytes\": " + std::to_string(text_bytes) + ", \"bases\": " + std::to_string(n_bases) + ", \"contigs\": " + std::to_string(slx_ref_nseq(r)) +
                               ", \"source\": " + std::to_string(slx_ref_counter(r, "source")) + ", \"windows\": " + std::to_string(slx_ref_counter(r, "windows"));
    put("load_host_1_thread", "s", stat(th), common + ", \"text_GB_per_s\": " + std::to_string((double)text_bytes / stat(th).med / 1e9));
    put("load_slx_ref_open", "s", stat(tg), common + ", \"text_GB_per_s\": " + std::to_string((double)text_bytes / stat(tg).med / 1e9) + ", \"vs_host\": " + std::to_string(stat(th).med / stat(tg).med));
    put("load_kernels_lines", "ms", stat(k_lines), "\"moves\": \"the text, read twice\"" + rate(2.0 * (double)text_bytes, stat(k_lines).med * 1e-3));
    put("load_kernels_class_scan_check", "ms", stat(k_class), "\"moves\": \"the text, read once\"" + rate((double)text_bytes, stat(k_class).med * 1e-3));
    put("load_kernels_gather", "ms", stat(k_gather), "\"moves\": \"the bases, read and written\"" + rate(2.0 * (double)n_bases, stat(k_gather).med * 1e-3));
    if (stat(k_inflate).med > 0) put("load_kernels_inflate", "ms", stat(k_inflate));
    // ---- (b) the fetch
    {
        std::mt19937_64 rng(7);
        const int64_t nreg = 200000;
        std::vector<slx_bam_region> reg((size_t)nreg);
        for (slx_bam_region &g : reg) {
            g.tid = (int32_t)(rng() % bases.size());
            const int64_t len = (int64_t)bases[(size_t)g.tid].size(), w = 150 + (int64_t)(rng() % 1851);
            g.beg = (int64_t)(rng() % (uint64_t)std::max<int64_t>(1, len - w));
            g.end = std::min(len, g.beg + w);
        }
        std::vector<double> hm;
        std::string out;
        std::vector<uint64_t> offs((size_t)nreg + 1, 0);
        for (int rep = 0; rep <= reps; ++rep) {
            const double t0 = now();
            uint64_t total = 0;
            for (int64_t i = 0; i < nreg; ++i) { offs[(size_t)i] = total; total += (uint64_t)(reg[(size_t)i].end - reg[(size_t)i].beg); }
            offs[(size_t)nreg] = total;
            out.resize((size_t)total);
            for (int64_t i = 0; i < nreg; ++i) std::memcpy(&out[(size_t)offs[(size_t)i]], bases[(size_t)reg[(size_t)i].tid].data() + reg[(size_t)i].beg, (size_t)(reg[(size_t)i].end - reg[(size_t)i].beg));
            if (rep) hm.push_back(now() - t0);
        }
        {
            std::string got(out.size(), '\0');
            std::vector<uint64_t> go((size_t)nreg + 1);
            OK(slx_ref_fetch_host(r, reg.data(), nreg, 0, &got[0], (int64_t)got.size(), go.data()));
            if (got != out || go != offs) { std::fprintf(stderr, "refgenome_bench: the fetch differs from the host loop's\n"); return 1; }
        }
        const std::string fc = "\"regions\": " + std::to_string(nreg) + ", \"fetched_bytes\": " + std::to_string(out.size());
        put("fetch_host_memcpy_1_thread", "ms", Stat{stat(hm).med * 1e3, stat(hm).lo * 1e3, stat(hm).hi * 1e3}, fc);
        for (const int64_t tile : {256, 1024, 2048, 4096}) {
            OK(slx_ref_set(r, "gather_tile_bytes", tile));
            std::vector<double> wall, kern;
            for (int rep = 0; rep <= reps; ++rep) {
                const void *db = nullptr, *dof = nullptr;
                int64_t nb = 0;
                const double t0 = now();
                OK(slx_ref_fetch_device(r, reg.data(), nreg, 1, &db, &dof, &nb));
                if (rep) { wall.push_back((now() - t0) * 1e3); kern.push_back((double)slx_ref_counter(r, "us_fetch") / 1e3); }
            }
            put("fetch_device_call", "ms", stat(wall), fc + ", \"gather_tile_bytes\": " + std::to_string(tile) + ", \"vs_host\": " + std::to_string(stat(hm).med * 1e3 / stat(wall).med));
            put("fetch_kernels", "ms", stat(kern), fc + ", \"gather_tile_bytes\": " + std::to_string(tile) + ", \"moves\": \"the fetched bytes, read and written\"" + rate(2.0 * (double)out.size(), stat(kern).med * 1e-3));
        }
        OK(slx_ref_set(r, "gather_tile_bytes", 2048));
    }
    slx_ref_close(r);
    // ---- (c) NM and MD
    {
        std::string sfai;
        std::vector<std::string> sb;
        if (!host_load(small, &sfai, &sb)) return 1;
        OK(slx_ref_open(small.c_str(), -1, &r));
        slx_bam *rd = nullptr;
        OK(slx_bam_open(bam.c_str(), -1, &rd));
        slx_bam_batch bt;
        OK(slx_bam_next(rd, (int64_t)1 << 40, &bt));
        const int64_t n = bt.n_records;
        std::vector<int32_t> h_nm((size_t)n);
        std::vector<uint64_t> h_off((size_t)n + 1, 0);
        std::string h_md;
        std::vector<double> hm;
        for (int rep = 0; rep <= reps; ++rep) {
            const double t0 = now();
            h_md.clear();
            char buf[4096];
            for (int64_t i = 0; i < n; ++i) {
                const uint8_t *rec = bt.stream + bt.rec_off[i];
                const int32_t tid = (int32_t)((uint32_t)rec[4] | (uint32_t)rec[5] << 8 | (uint32_t)rec[6] << 16 | (uint32_t)rec[7] << 24);
                const std::string *c = tid >= 0 && tid < (int32_t)sb.size() ? &sb[(size_t)tid] : nullptr;
                uint64_t len = 0;
                int32_t nm = -1;
                if (c && !rg_record_nm_md(rec, bt.rec_off[i + 1] - bt.rec_off[i], (const uint8_t *)c->data(), (int64_t)c->size(), &nm, (uint8_t *)buf, sizeof buf, &len)) return 1;
                if (len > sizeof buf) { std::fprintf(stderr, "refgenome_bench: an MD of %llu bytes\n", (unsigned long long)len); return 1; }
                h_nm[(size_t)i] = nm; h_off[(size_t)i] = h_md.size(); h_md.append(buf, (size_t)len);
            }
            h_off[(size_t)n] = h_md.size();
            if (rep) hm.push_back(now() - t0);
        }
        const std::string mc = "\"records\": " + std::to_string(n) + ", \"record_bytes\": " + std::to_string(bt.n_bytes) + ", \"md_bytes\": " + std::to_string(h_md.size());
        put("nm_md_host_1_thread", "s", stat(hm), mc + ", \"records_per_s\": " + std::to_string((double)n / stat(hm).med));
        for (const int64_t lng : {(int64_t)1, (int64_t)64, (int64_t)128, (int64_t)256, (int64_t)512, (int64_t)1 << 30}) {
            OK(slx_ref_set(r, "long_record", lng));
            std::vector<double> wall, ks, kt;
            slx_ref_md m;
            for (int rep = 0; rep <= reps; ++rep) {
                const double t0 = now();
                OK(slx_ref_nm_md_device(r, bt.d_stream, bt.n_bytes, bt.d_rec_off, n, nullptr, 0, &m));
                if (rep) { wall.push_back((now() - t0) * 1e3); ks.push_back((double)slx_ref_counter(r, "us_md_size") / 1e3); kt.push_back((double)slx_ref_counter(r, "us_md_text") / 1e3); }
            }
            std::vector<int32_t> g_nm((size_t)n);
            std::vector<uint64_t> g_off((size_t)n + 1);
            std::string g_md((size_t)m.md_bytes, '\0');
            OK(slx_ref_md_to_host(r, &m, g_nm.data(), g_md.empty() ? nullptr : &g_md[0], g_off.data()));
            if (g_nm != h_nm || g_off != h_off || g_md != h_md) { std::fprintf(stderr, "refgenome_bench: NM / MD differ from the host loop's (long_record %lld)\n", (long long)lng); return 1; }
            const std::string lc = mc + ", \"long_record\": " + std::to_string(lng) + ", \"long_records\": " + std::to_string(slx_ref_counter(r, "long_records"));
            put("nm_md_device_call", "ms", stat(wall), lc + ", \"records_per_s\": " + std::to_string((double)n / (stat(wall).med * 1e-3)) + ", \"vs_host\": " + std::to_string(stat(hm).med * 1e3 / stat(wall).med));
            put("nm_md_kernels_size", "ms", stat(ks), lc + ", \"moves\": \"the records, read once\"" + rate((double)bt.n_bytes, stat(ks).med * 1e-3));
            put("nm_md_kernels_text", "ms", stat(kt), lc + ", \"moves\": \"the records, read once, and the MD bytes\"" + rate((double)bt.n_bytes + (double)h_md.size(), stat(kt).med * 1e-3));
        }
        slx_bam_close(rd);
        slx_ref_close(r);
    }
    return 0;
}
