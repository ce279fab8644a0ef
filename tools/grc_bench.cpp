// grc_bench -- what the interval unit on the GPU buys, against a host loop over the same bodies (csrc/grc_host.h) on 1 and on 16 threads of the same machine, from
// one process and generated data:
//     build     slx_grc_create over the subjects (hipCUB sorts, scan, mirror): kernel time from the unit's HIP events ("us_build") and wall clock, against
//               grc_build_host (std::stable_sort)
//     merge     slx_grc_merged ("us_merge", wall clock), against the host sweep over grc_run_starts
//     join      slx_grc_overlaps of the queries ("us_count", "us_fill", wall clock with the copies of the pairs down), per wave_range setting, against
//               grc_range + grc_count + grc_fill per query on 1 and 16 threads (each thread fills its own vectors)
//     records   slx_grc_overlaps_host of generated 100M records, counts only ("us_records" + "us_count", wall clock with the upload)
//   grc_bench [subjects (200000)] [queries (2000000)] [reps (5)]
// Subjects: "exons" -- random intervals of 50 .. 2000 bp on 24 chr of 100 Mbp; "long" -- the same plus one interval over the whole of every chr, the known weak
// case (every query's candidate range then starts at the chr's first entry: the count stays two binary searches, the fill scans).  The long case runs a
// hundredth of the queries.  The pairs of the GPU and of the host loop are compared first.  Every figure is the median of reps runs after one warm-up, with the
// fastest and the slowest beside it.  Prints one JSON line per measurement.  Built by seqlib_amd/build.py with g++ against libseqlib_amd.so.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>
#include "seqlib_amd_grc.h"
#include "grc_host.h"

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#define OK(x) do { if ((x) != SLX_OK) { std::fprintf(stderr, "grc_bench: %s\n", slx_last_error()); return 1; } } while (0)

struct Stat { double med, lo, hi; };
static Stat stat(std::vector<double> v) { std::sort(v.begin(), v.end()); return Stat{v[v.size() / 2], v.front(), v.back()}; }
static void put(const std::string &what, const char *unit, const Stat &s, const std::string &extra = "")
{
    std::printf("{\"what\": \"%s\", \"unit\": \"%s\", \"median\": %.3f, \"min\": %.3f, \"max\": %.3f%s%s}\n", what.c_str(), unit, s.med, s.lo, s.hi, extra.empty() ? "" : ", ", extra.c_str());
    std::fflush(stdout);
}

static const int N_CHR = 24;
static const int32_t CHR_LEN = 100000000;

static std::vector<slx_grc_iv> intervals(size_t n, unsigned seed, int min_len, int max_len)
{
    std::mt19937 rng(seed);
    std::vector<slx_grc_iv> v(n);
    for (size_t i = 0; i < n; ++i) {
        std::memset(&v[i], 0, sizeof v[i]);
        v[i].chr = (int32_t)(rng() % N_CHR);
        v[i].pos1 = (int32_t)(rng() % (uint32_t)(CHR_LEN - max_len));
        v[i].pos2 = v[i].pos1 + min_len + (int32_t)(rng() % (uint32_t)(max_len - min_len + 1));
        v[i].strand = "+-*"[rng() % 3];
    }
    return v;
}

// a block_size-prefixed record "r" at (tid, pos) with the CIGAR 100M and no sequence
static void put_record(std::vector<uint8_t> &s, std::vector<uint64_t> &off, int32_t tid, int32_t pos)
{
    uint8_t r[42];
    std::memset(r, 0, sizeof r);
    const uint32_t bs = 38, cig = 100u << 4;
    std::memcpy(r, &bs, 4); std::memcpy(r + 4, &tid, 4); std::memcpy(r + 8, &pos, 4);
    r[12] = 2; r[13] = 60; r[16] = 1;          // l_read_name, mapq, n_cigar_op
    r[36] = 'r';
    std::memcpy(r + 38, &cig, 4);
    s.insert(s.end(), r, r + sizeof r);
    off.push_back(s.size());
}

struct HostPairs { std::vector<int32_t> sid, c1, c2; uint64_t n = 0; };
static void host_join(const grc_idx &X, const grc_iv *q, size_t q0, size_t q1, HostPairs &P)
{
    for (size_t i = q0; i < q1; ++i) {
        const grc_cand C = grc_range(X, q[i]);
        const uint32_t k = grc_count(X, q[i], GRC_IGNORE_STRAND, C);
        if (!k) continue;
        const size_t at = P.sid.size();
        P.sid.resize(at + k); P.c1.resize(at + k); P.c2.resize(at + k);
        P.n += grc_fill(X, q[i], GRC_IGNORE_STRAND, C.lo, C.hi, P.sid.data() + at, P.c1.data() + at, P.c2.data() + at, k);
    }
}

static int run_case(const char *name, const std::vector<slx_grc_iv> &subj, const std::vector<slx_grc_iv> &qry, int reps)
{
    const std::string tag = std::string("\"case\": \"") + name + "\", \"subjects\": " + std::to_string(subj.size()) + ", \"queries\": " + std::to_string(qry.size());
    const grc_iv *sv = (const grc_iv *)subj.data(), *qv = (const grc_iv *)qry.data();
    // ---- build
    std::vector<double> wall, kern;
    slx_grc *g = nullptr;
    for (int r = 0; r <= reps; ++r) {
        if (g) slx_grc_free(g);
        const double t0 = now();
        OK(slx_grc_create(SLX_GRC_AUTO, subj.data(), (int64_t)subj.size(), &g));
        if (r) { wall.push_back((now() - t0) * 1e3); kern.push_back(slx_grc_counter(g, "us_build") / 1e3); }
    }
    put("build_gpu_wall", "ms", stat(wall), tag); put("build_gpu_kernels", "ms", stat(kern), tag);
    grc_host_arrays H;
    wall.clear();
    for (int r = 0; r <= reps; ++r) { const double t0 = now(); grc_build_host(sv, (uint32_t)subj.size(), H); if (r) wall.push_back((now() - t0) * 1e3); }
    put("build_host_1_thread", "ms", stat(wall), tag);
    const grc_idx X = H.idx();
    // ---- merge
    std::vector<slx_grc_iv> merged(subj.size());
    int64_t n_merged = 0;
    wall.clear(); kern.clear();
    for (int r = 0; r <= reps; ++r) {
        const int64_t us0 = slx_grc_counter(g, "us_merge");
        const double t0 = now();
        OK(slx_grc_merged(g, merged.data(), (int64_t)merged.size(), &n_merged));
        if (r) { wall.push_back((now() - t0) * 1e3); kern.push_back((slx_grc_counter(g, "us_merge") - us0) / 1e3); }
    }
    put("merge_gpu_wall", "ms", stat(wall), tag + ", \"merged\": " + std::to_string(n_merged)); put("merge_gpu_kernels", "ms", stat(kern), tag);
    wall.clear();
    int64_t n_host = 0;
    for (int r = 0; r <= reps; ++r) {
        const double t0 = now();
        std::vector<grc_iv> m;
        for (uint32_t i = 0; i < X.n; ++i) {
            if (grc_run_starts(X, i)) { grc_iv v; std::memset(&v, 0, sizeof v); v.chr = X.chr[i]; v.pos1 = X.p1[i]; v.strand = (char)X.strand[i]; m.push_back(v); }
            m.back().pos2 = X.run_p2[i];
        }
        n_host = (int64_t)m.size();
        if (r) wall.push_back((now() - t0) * 1e3);
    }
    if (n_host != n_merged) { std::fprintf(stderr, "grc_bench: merge: the GPU has %lld intervals, the host %lld\n", (long long)n_merged, (long long)n_host); return 1; }
    put("merge_host_1_thread", "ms", stat(wall), tag);
    // ---- join: the host loop first, its pairs are what the GPU's are compared with
    HostPairs ref;
    for (int threads : {1, 16}) {
        wall.clear();
        for (int r = 0; r <= reps; ++r) {
            std::vector<HostPairs> part((size_t)threads);
            const double t0 = now();
            std::vector<std::thread> th;
            const size_t step = (qry.size() + (size_t)threads - 1) / (size_t)threads;
            for (int t = 0; t < threads; ++t) th.emplace_back(host_join, std::cref(X), qv, std::min(qry.size(), (size_t)t * step), std::min(qry.size(), (size_t)(t + 1) * step), std::ref(part[(size_t)t]));
            for (std::thread &x : th) x.join();
            if (r) wall.push_back((now() - t0) * 1e3);
            if (threads == 1) ref = std::move(part[0]);
        }
        put(threads == 1 ? "join_host_1_thread" : "join_host_16_threads", "ms", stat(wall), tag + ", \"pairs\": " + std::to_string(ref.n));
    }
    for (int64_t wave_range : {64ll, 0ll, 1ll << 20}) {
        OK(slx_grc_set(g, "wave_range", wave_range));
        wall.clear(); kern.clear();
        std::vector<double> kcount, kfill;
        int64_t lane = 0, wave = 0;
        for (int r = 0; r <= reps; ++r) {
            slx_grc_result res;
            const int64_t c0 = slx_grc_counter(g, "us_count"), f0 = slx_grc_counter(g, "us_fill");
            const double t0 = now();
            OK(slx_grc_overlaps(g, qry.data(), (int64_t)qry.size(), 1, &res));
            if (r) { wall.push_back((now() - t0) * 1e3); kcount.push_back((slx_grc_counter(g, "us_count") - c0) / 1e3); kfill.push_back((slx_grc_counter(g, "us_fill") - f0) / 1e3); }
            if (r == 0 && ((uint64_t)res.n_pairs != ref.n || std::memcmp(res.subject_id, ref.sid.data(), 4 * ref.n) || std::memcmp(res.pos1, ref.c1.data(), 4 * ref.n) ||
                           std::memcmp(res.pos2, ref.c2.data(), 4 * ref.n))) {
                std::fprintf(stderr, "grc_bench: join: the GPU's pairs differ from the host loop's (%lld against %llu)\n", (long long)res.n_pairs, (unsigned long long)ref.n);
                return 1;
            }
            lane = slx_grc_counter(g, "queries_lane"); wave = slx_grc_counter(g, "queries_wave");
            slx_grc_result_free(&res);
        }
        const std::string t2 = tag + ", \"wave_range\": " + std::to_string(wave_range) + ", \"queries_lane\": " + std::to_string(lane) + ", \"queries_wave\": " + std::to_string(wave);
        put("join_gpu_wall", "ms", stat(wall), t2); put("join_gpu_count_kernels", "ms", stat(kcount), t2); put("join_gpu_fill_kernels", "ms", stat(kfill), t2);
    }
    OK(slx_grc_set(g, "wave_range", 64));
    // ---- records: one 100M record per query's start
    std::vector<uint8_t> stream;
    std::vector<uint64_t> off(1, 0);
    for (const slx_grc_iv &q : qry) put_record(stream, off, q.chr, q.pos1);
    wall.clear(); kern.clear();
    uint64_t hits = 0;
    for (int r = 0; r <= reps; ++r) {
        slx_grc_result res;
        const int64_t k0 = slx_grc_counter(g, "us_records") + slx_grc_counter(g, "us_count");
        const double t0 = now();
        OK(slx_grc_overlaps_host(g, stream.data(), (int64_t)stream.size(), off.data(), (int64_t)qry.size(), 0, &res));
        if (r) { wall.push_back((now() - t0) * 1e3); kern.push_back((slx_grc_counter(g, "us_records") + slx_grc_counter(g, "us_count") - k0) / 1e3); }
        hits = (uint64_t)res.n_pairs;
        slx_grc_result_free(&res);
    }
    const std::string t3 = tag + ", \"records\": " + std::to_string(qry.size()) + ", \"stream_bytes\": " + std::to_string(stream.size()) + ", \"hits\": " + std::to_string(hits);
    put("records_gpu_wall_with_upload", "ms", stat(wall), t3); put("records_gpu_kernels", "ms", stat(kern), t3);
    slx_grc_free(g);
    return 0;
}

int main(int argc, char **argv)
{
    const size_t n_subj = argc > 1 ? (size_t)std::atoll(argv[1]) : 200000, n_qry = argc > 2 ? (size_t)std::atoll(argv[2]) : 2000000;
    const int reps = std::max(argc > 3 ? std::atoi(argv[3]) : 5, 3);
    if (slx_device_count() <= 0) { std::fprintf(stderr, "grc_bench: no HIP device (there is no CPU fallback for batches)\n"); return 1; }
    const std::vector<slx_grc_iv> subj = intervals(n_subj, 1, 50, 2000), qry = intervals(n_qry, 2, 30, 300);
    if (run_case("exons", subj, qry, reps)) return 1;
    std::vector<slx_grc_iv> with_long = subj;
    for (int c = 0; c < N_CHR; ++c) { slx_grc_iv v; std::memset(&v, 0, sizeof v); v.chr = c; v.pos1 = 0; v.pos2 = CHR_LEN; v.strand = '*'; with_long.push_back(v); }
    return run_case("long", with_long, std::vector<slx_grc_iv>(qry.begin(), qry.begin() + (long)(n_qry / 100)), reps);
}
