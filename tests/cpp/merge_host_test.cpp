// merge_host_test.cpp -- a whole k-way merge on the host: the planner of seqlib_amd/csrc/merge_host.h over the key, bound, rank and place bodies of dev_merge.h
// (compiled for the host: one call plays all lanes of a wave, 1 or 64 of them), run under ASan + UBSan by tests/test_merge_host.py.  Its own main, no input.
// The model is plain: std::stable_sort of the concatenation of the inputs in add order.  Every batch, table and output is an allocation of exactly its size: a
// load or a store outside is the sanitizer's to report.  The cases: batches of 1, 2, 3 records (and one batch per input), k = 1, 2, 3, 64; a block of 12 equal
// keys in one input -- longer than three batches -- with the same key at the end of a batch of another input; empty inputs; an input wholly below the others;
// unplaced tails (tid -1) in three inputs; pos -1; waves that straddle inputs; the max_bytes refusal; an unsorted input inside a batch and at a batch join.
// Prints "merge_host OK <cases> <rounds> <rounds that emitted nothing> <waves that straddled inputs>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>
#include "../../seqlib_amd/csrc/dev_merge.h"
#include "../../seqlib_amd/csrc/merge_host.h"

typedef unsigned long long ull;

static int fails = 0;
static long n_cases = 0, n_rounds = 0, n_empty_rounds = 0, n_straddle = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static void put32(std::string &s, uint32_t v) { const char b[4] = {(char)v, (char)(v >> 8), (char)(v >> 16), (char)(v >> 24)}; s.append(b, 4); }

// a record of exactly `total` bytes (>= 36 + name + 1) whose filler depends on the tag, so that no two records look alike
static std::string record(int32_t tid, int32_t pos, const std::string &name, size_t total, uint32_t tag)
{
    std::string r;
    put32(r, (uint32_t)total - 4);
    put32(r, (uint32_t)tid); put32(r, (uint32_t)pos);
    put32(r, (uint32_t)(4680u << 16 | (name.size() + 1)));
    put32(r, (tag & 1 ? 16u : 0u) << 16); put32(r, 0);
    put32(r, 0xffffffffu); put32(r, 0xffffffffu); put32(r, 0);
    r += name; r.push_back('\0');
    if (r.size() > total) { fprintf(stderr, "record too small\n"); exit(2); }
    uint32_t x = tag * 2654435761u + 12345u;
    while (r.size() < total) { x = x * 1664525u + 1013904223u; r.push_back((char)(x >> 24)); }
    return r;
}
static ull key_of(int32_t tid, int32_t pos) { return (ull)(uint32_t)tid << 32 | (ull)((uint32_t)pos ^ 0x80000000u); }
static ull key_of(const std::string &r) { int32_t t, p; memcpy(&t, r.data() + 4, 4); memcpy(&p, r.data() + 8, 4); return key_of(t, p); }

typedef std::vector<std::vector<std::string>> Inputs;

struct Batch { uint8_t *base; uint64_t n_bytes, n; uint64_t *off; ull *key, *src; uint32_t *len; };
static void drop(Batch &b) { free(b.base); free(b.off); free(b.key); free(b.src); free(b.len); }

struct Result { int rc = 0; int input = -1; uint64_t ordinal = 0; ull at_key = 0; std::string out; std::vector<uint8_t> from; };          // rc 1: unsorted, 2: budget, 3: a broken record

// the merge of slx_merge.hip with host memory for HBM: the same planner calls in the same order, the same bodies
static Result merge(const Inputs &in, size_t batch, int nlanes, int64_t max_bytes)
{
    const int k = (int)in.size();
    Result R;
    std::vector<merge_in> mi((size_t)k);
    std::vector<std::deque<Batch>> win((size_t)k);
    std::vector<uint64_t> consumed((size_t)k, 0), n_read((size_t)k, 0);
    std::vector<bool> has_last((size_t)k, false);
    std::vector<ull> last_read((size_t)k, 0);
    uint64_t held_bytes = 0;
    bool had_bound = false; ull prev_bound = 0;
    auto cleanup = [&]() { for (auto &w : win) { for (Batch &b : w) drop(b); w.clear(); } };
    for (;;) {
        ++n_rounds;
        for (int i = 0; i < k && R.rc == 0; ++i) {
            if (!merge_wants_refill(mi[(size_t)i], had_bound, prev_bound)) continue;
            const size_t a = (size_t)n_read[(size_t)i], e = std::min(in[(size_t)i].size(), a + batch);
            if (a == e) { mi[(size_t)i].at_end = true; continue; }
            Batch b;
            b.n = e - a; b.n_bytes = 0;
            for (size_t r = a; r < e; ++r) b.n_bytes += in[(size_t)i][r].size();
            b.base = (uint8_t *)malloc(b.n_bytes); b.off = (uint64_t *)malloc(8 * (b.n + 1));
            b.key = (ull *)malloc(8 * b.n); b.src = (ull *)malloc(8 * b.n); b.len = (uint32_t *)malloc(4 * b.n);
            uint64_t o = 0;
            for (size_t r = a; r < e; ++r) { b.off[r - a] = o; memcpy(b.base + o, in[(size_t)i][r].data(), in[(size_t)i][r].size()); o += in[(size_t)i][r].size(); }
            b.off[b.n] = o;
            ull bad = RS_NO_BAD, uns = RS_NO_BAD, last = 0;
            for (uint64_t r = 0; r < b.n; ++r) {          // k_merge_key, a lane per record
                uint64_t kk = 0; uint32_t l = 0; bool u = false;
                if (mg_key(b.base, b.n_bytes, b.off, r, b.n, has_last[(size_t)i], last_read[(size_t)i], &kk, &l, &u)) {
                    b.key[r] = kk; b.len[r] = l; b.src[r] = (ull)(uintptr_t)(b.base + b.off[r]);
                    if (u && uns == RS_NO_BAD) uns = r;
                    if (r + 1 == b.n) last = kk;
                } else { if (bad == RS_NO_BAD) bad = r; b.key[r] = 0; b.len[r] = 0; b.src[r] = 0; }
            }
            if (bad != RS_NO_BAD) { R.rc = 3; R.input = i; R.ordinal = n_read[(size_t)i] + bad; drop(b); break; }
            if (uns != RS_NO_BAD) { R.rc = 1; R.input = i; R.ordinal = n_read[(size_t)i] + uns; drop(b); break; }
            if (!merge_fits(held_bytes + b.n_bytes, max_bytes)) { R.rc = 2; R.input = i; R.at_key = last; drop(b); break; }
            win[(size_t)i].push_back(b);
            has_last[(size_t)i] = true; last_read[(size_t)i] = last; n_read[(size_t)i] += b.n;
            mi[(size_t)i].held += b.n; mi[(size_t)i].last_key = last;
            held_bytes += b.n_bytes;
        }
        if (R.rc) { cleanup(); return R; }
        uint64_t bound = 0;
        const bool finite = merge_bound(mi.data(), k, &bound);
        had_bound = finite; prev_bound = bound;
        uint64_t N = 0;
        for (int i = 0; i < k; ++i) N += mi[(size_t)i].held;
        if (N == 0) { if (!finite) break; ++n_empty_rounds; continue; }
        // the table, exactly sized
        ull *keys = (ull *)malloc(8 * N), *src = (ull *)malloc(8 * N);
        uint32_t *len = (uint32_t *)malloc(4 * N), *beg = (uint32_t *)malloc(4 * (size_t)(k + 1)), *ebeg = (uint32_t *)malloc(4 * (size_t)(k + 1));
        size_t at = 0;
        for (int i = 0; i < k; ++i) {
            beg[i] = (uint32_t)at;
            for (size_t s = 0; s < win[(size_t)i].size(); ++s) {
                const Batch &b = win[(size_t)i][s];
                const size_t c = s == 0 ? (size_t)consumed[(size_t)i] : 0, n = (size_t)b.n - c;
                memcpy(keys + at, b.key + c, 8 * n); memcpy(src + at, b.src + c, 8 * n); memcpy(len + at, b.len + c, 4 * n);
                at += n;
            }
        }
        beg[k] = (uint32_t)at;
        CHECK(at == N);
        std::vector<uint32_t> elig((size_t)k);
        uint64_t E = 0;
        for (int i = 0; i < k; ++i) {          // k_merge_elig, a wave per input
            elig[(size_t)i] = mg_elig(keys + beg[i], (uint64_t)(beg[i + 1] - beg[i]), finite, bound, 0, nlanes);
            uint32_t want = 0;
            for (uint32_t x = beg[i]; x < beg[i + 1]; ++x) want += !finite || keys[x] < bound;
            CHECK(elig[(size_t)i] == want);
            ebeg[i] = (uint32_t)E; E += elig[(size_t)i];
        }
        ebeg[k] = (uint32_t)E;
        if (E) {
            uint32_t *rank = (uint32_t *)malloc(4 * E);
            ull *slen = (ull *)malloc(8 * (E + 1)), *ssrc = (ull *)malloc(8 * E);
            uint8_t *from = (uint8_t *)malloc(E);
            memset(rank, 0xff, 4 * E);
            for (uint64_t g0 = 0; g0 < E + (uint64_t)nlanes; g0 += (uint64_t)nlanes) {          // k_merge_rank, a wave per nlanes eligible records, and one wave past the end
                mg_rank_wave(keys, beg, ebeg, k, g0, rank, 0, nlanes);
                if (g0 < E && mg_input_of(ebeg, k, g0) != mg_input_of(ebeg, k, std::min(E, g0 + (uint64_t)nlanes) - 1)) ++n_straddle;
            }
            std::vector<bool> seen((size_t)E, false);
            for (uint64_t g = 0; g < E; ++g) { CHECK(rank[g] < E && !seen[rank[g]]); if (rank[g] < E) seen[rank[g]] = true; }
            if (!fails) {
                for (uint64_t g = 0; g < E; ++g) mg_place(beg, ebeg, k, g, rank, len, src, slen, ssrc, from);          // k_merge_place
                slen[E] = 0;
                for (uint64_t j = 0; j < E; ++j) { R.out.append((const char *)(uintptr_t)ssrc[j], (size_t)slen[j]); R.from.push_back(from[j]); }
            }
            free(rank); free(slen); free(ssrc); free(from);
            for (int i = 0; i < k; ++i) {          // the round's records leave their windows
                uint64_t c = elig[(size_t)i];
                mi[(size_t)i].held -= c;
                while (c) {
                    Batch &b = win[(size_t)i].front();
                    const uint64_t left = b.n - consumed[(size_t)i];
                    if (c < left) { consumed[(size_t)i] += c; break; }
                    c -= left; held_bytes -= b.n_bytes;
                    drop(b); win[(size_t)i].pop_front(); consumed[(size_t)i] = 0;
                }
            }
        } else ++n_empty_rounds;
        free(keys); free(src); free(len); free(beg); free(ebeg);
        if (fails) break;
    }
    CHECK(held_bytes == 0 || fails);
    cleanup();
    return R;
}

static void expect_merged(const Inputs &in, size_t batch, int nlanes, const char *what)
{
    ++n_cases;
    std::vector<std::pair<ull, std::pair<int, const std::string *>>> all;
    for (size_t i = 0; i < in.size(); ++i) {
        for (size_t r = 0; r < in[i].size(); ++r) {
            if (r) CHECK(key_of(in[i][r - 1]) <= key_of(in[i][r]));          // the case itself is sorted
            all.push_back({key_of(in[i][r]), {(int)i, &in[i][r]}});
        }
    }
    std::stable_sort(all.begin(), all.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    std::string want; std::vector<uint8_t> from;
    for (const auto &x : all) { want += *x.second.second; from.push_back((uint8_t)x.second.first); }
    const int before = fails;
    const Result R = merge(in, batch, nlanes, (int64_t)1 << 40);
    CHECK(R.rc == 0);
    CHECK(R.out == want);
    CHECK(R.from == from);
    if (fails != before) fprintf(stderr, "  in case %s, k = %zu, batches of %zu, %d lanes\n", what, in.size(), batch, nlanes);
}

// the general case for k inputs (see the top of the file); *tie_input: where the block of equal keys lies
static Inputs general(int k, int *tie_input)
{
    Inputs in((size_t)k);
    uint32_t x = 77u + (uint32_t)k, tag = 0;
    auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    auto rec = [&](int32_t tid, int32_t pos) { ++tag; return record(tid, pos, "r" + std::to_string(tag), 44 + rnd() % 90, tag); };
    const int T = k - 1;
    *tie_input = T;
    for (int i = 0; i < k; ++i) {
        std::vector<std::pair<int32_t, int32_t>> at;
        if (k >= 3 && (i == 1 || i == 5)) continue;          // empty inputs
        if (k >= 4 && i == 2) {                                // wholly below the others, pos -1 first
            in[(size_t)i].push_back(rec(0, -1));
            for (int p = 0; p < 7; ++p) in[(size_t)i].push_back(rec(0, p / 2));
            continue;
        }
        if (k >= 2 && i == 0) {                                // (1, 130) at the end of a batch of 1, of 2 and of 3
            for (auto tp : {std::pair<int32_t, int32_t>{0, 100}, {1, 130}, {1, 130}, {1, 130}}) in[0].push_back(rec(tp.first, tp.second));
            for (int n = 0; n < 6; ++n) at.push_back({2, 150 + (int32_t)(rnd() % 20)});
        } else {
            if (k < 4 && i == T) in[(size_t)i].push_back(rec(0, -1));
            const int n = 5 + (i * 7) % 11;
            for (int r = 0; r < n; ++r) at.push_back({(int32_t)(rnd() % 3), 100 + (int32_t)(rnd() % 41)});
            if (i == T) for (int r = 0; r < 12; ++r) at.push_back({1, 130});
        }
        std::stable_sort(at.begin(), at.end());
        for (auto tp : at) in[(size_t)i].push_back(rec(tp.first, tp.second));
        if (i == 0 || i == T || i == k / 2) for (int r = 0; r < 2; ++r) in[(size_t)i].push_back(rec(-1, -1));          // the unplaced tail
    }
    return in;
}

int main()
{
    for (int k : {1, 2, 3, 64}) {
        int T = 0;
        const Inputs in = general(k, &T);
        size_t ties = 0, unplaced_inputs = 0, empty = 0;
        for (const std::string &r : in[(size_t)T]) ties += key_of(r) == key_of(1, 130);
        for (const auto &v : in) { unplaced_inputs += !v.empty() && key_of(v.back()) == key_of(-1, -1); empty += v.empty(); }
        CHECK(ties >= 12);                                                  // longer than three batches of 3
        CHECK(unplaced_inputs == (size_t)(k >= 4 ? 3 : std::min(k, 2)));          // three of them at k = 64
        CHECK(empty == (k >= 64 ? 2u : k >= 3 ? 1u : 0u));
        if (k >= 2) CHECK(key_of(in[0][1]) == key_of(1, 130) && key_of(in[0][2]) == key_of(1, 130) && key_of(in[0][3]) == key_of(1, 130));
        if (k >= 4) for (size_t i = 0; i < in.size(); ++i) if (i != 2 && !in[i].empty()) CHECK(key_of(in[2].back()) < key_of(in[i][0]) && key_of(in[2][0]) == key_of(0, -1));
        for (size_t batch : {(size_t)1, (size_t)2, (size_t)3, (size_t)1000})
            for (int nlanes : {1, 64}) {
                const long empty_before = n_empty_rounds;
                expect_merged(in, batch, nlanes, "general");
                if (k >= 2 && batch <= 3) CHECK(n_empty_rounds > empty_before);          // the tie block made rounds that emit nothing and refill
            }
    }
    CHECK(n_straddle > 0);
    // a wave of 64 over inputs of 40 records each, all keys equal: every wave straddles, every tie goes by input
    {
        Inputs in(5);
        uint32_t tag = 1000;
        for (auto &v : in) for (int r = 0; r < 40; ++r) { ++tag; v.push_back(record(1, 7, "t" + std::to_string(tag), 44 + tag % 30, tag)); }
        for (int nlanes : {1, 64}) expect_merged(in, 1000, nlanes, "all equal");
        expect_merged(in, 3, 64, "all equal");
    }
    // one input, nothing at all, and only empty inputs
    expect_merged(Inputs(1), 2, 64, "one empty");
    expect_merged(Inputs(3), 2, 64, "three empty");
    // the budget: batches of 1 and a block of 12 equal keys of at least 44 bytes each need the block held at once
    {
        int T = 0;
        const Inputs in = general(2, &T);
        ++n_cases;
        Result R = merge(in, 1, 64, 450);          // (three records of the largest size fit: only the block passes it)
        CHECK(R.rc == 2 && R.input == T && R.at_key == key_of(1, 130) && merge_key_tid(R.at_key) == 1 && merge_key_pos(R.at_key) == 130);
        R = merge(in, 1, 64, 0);
        CHECK(R.rc == 2);
        CHECK(merge_key_tid(key_of(-1, -1)) == -1 && merge_key_pos(key_of(-1, -1)) == -1 && merge_key_pos(key_of(0, 0x7fffffff)) == 0x7fffffff);
    }
    // unsorted: inside a batch, and at a batch join (the predecessor is the batch before's last record)
    {
        Inputs in(2);
        in[0] = {record(0, 5, "a", 40, 1), record(0, 9, "b", 41, 2)};
        in[1] = {record(0, 5, "c", 40, 3), record(0, 9, "d", 44, 4), record(0, 8, "e", 42, 5), record(0, 20, "f", 42, 6)};
        n_cases += 3;
        Result R = merge(in, 2, 64, 1 << 20);                 // record 2 is the first of the second batch
        CHECK(R.rc == 1 && R.input == 1 && R.ordinal == 2);
        R = merge(in, 3, 1, 1 << 20);                          // ... the last of the first batch
        CHECK(R.rc == 1 && R.input == 1 && R.ordinal == 2);
        R = merge(in, 1, 64, 1 << 20);
        CHECK(R.rc == 1 && R.input == 1 && R.ordinal == 2);
        in[1][2] = record(-1, 0, "g", 42, 7);                  // tid -1 is the highest: what follows it is out of order
        R = merge(in, 2, 64, 1 << 20);
        CHECK(R.rc == 1 && R.input == 1 && R.ordinal == 3);
        in[1].pop_back();
        expect_merged(in, 2, 64, "tid -1 last");
    }
    // the planner alone
    {
        merge_in a; a.held = 3; a.last_key = 10;
        CHECK(!merge_wants_refill(a, false, 0) && !merge_wants_refill(a, true, 9) && merge_wants_refill(a, true, 10));
        a.at_end = true;
        CHECK(!merge_wants_refill(a, true, 10));
        merge_in e;
        CHECK(merge_wants_refill(e, false, 0));
        merge_in v[3]; v[0] = a; v[1].held = 2; v[1].last_key = 7; v[2].held = 1; v[2].last_key = 8;
        uint64_t B = 0;
        CHECK(merge_bound(v, 3, &B) && B == 7);              // input 0 is at its end: its last key bounds nothing
        v[1].at_end = v[2].at_end = true;
        CHECK(!merge_bound(v, 3, &B));
    }
    // the header rule
    {
        const std::string sq = "@SQ\tSN:a\tLN:5\n", hd = "@HD\tVN:1.6\tSO:unsorted\n";
        std::string out, what;
        CHECK(merge_header_rule({hd + sq + "@RG\tID:x\n", hd + sq + "@RG\tID:x\n"}, &out, &what) == 0 && out == "@HD\tVN:1.6\tSO:coordinate\n" + sq + "@RG\tID:x\n");
        CHECK(merge_header_rule({hd + sq + "@RG\tID:x\n", "@HD\tVN:1.0\n@SQ\tSN:zzz\tLN:9\n@RG\tID:y\tSM:s\n@CO\thello\n@PG\tID:x\n"}, &out, &what) == 0 &&
              out == "@HD\tVN:1.6\tSO:coordinate\n" + sq + "@RG\tID:x\n@RG\tID:y\tSM:s\n@CO\thello\n@PG\tID:x\n");
        CHECK(merge_header_rule({hd + sq + "@RG\tID:x\tSM:one\n", sq + "@RG\tID:x\tSM:two\n"}, &out, &what) == 2 && what == "@RG ID:x");
        CHECK(merge_header_rule({sq, sq + "@CO\tc\n", sq + "@CO\tc\n"}, &out, &what) == 0 && out == "@HD\tVN:1.6\tSO:coordinate\n" + sq + "@CO\tc\n");
        CHECK(merge_header_rule({"@HD\tVN:1.4", "@CO\tc"}, &out, &what) == 0 && out == "@HD\tVN:1.4\tSO:coordinate\n@CO\tc\n");
    }
    if (fails) { printf("merge_host FAILED %d\n", fails); return 1; }
    printf("merge_host OK %ld %ld %ld %ld\n", n_cases, n_rounds, n_empty_rounds, n_straddle);
    return 0;
}
