// sort_host_test.cpp -- seqlib_amd/csrc/dev_recsort.h compiled for the host (lane 0 of 1), run under ASan + UBSan by tests/test_sort_host.py.  Its own main, no input.
// The model is plain: std::stable_sort of the input ordinals by key, then one memcpy per record.  Every segment, table, slab and the LDS tile is an
// allocation of exactly its size: a load or a store outside is the sanitizer's to report.  The record list is built for the edges of the tile gather (each
// is asserted below, so the list cannot drift away from them): a 38-byte record, one that ends exactly on a tile boundary, one that starts 1 byte before a
// boundary, one of 10 000 bytes over five tiles, sources at every alignment mod 16 -- among them a record that is first and one that is last in its segment --
// a tie block for stability, pos = -1, the unplaced tail, and a stream whose size is no multiple of 16.  Prints "sort_host OK <records> <bytes> <tiles>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>
#include "../../seqlib_amd/csrc/dev_recsort.h"
#include "../../seqlib_amd/csrc/recsort_host.h"

typedef unsigned long long ull;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static void put32(std::string &s, uint32_t v) { const char b[4] = {(char)v, (char)(v >> 8), (char)(v >> 16), (char)(v >> 24)}; s.append(b, 4); }

// a record of exactly `total` bytes (>= 36 + name + 1): fixed fields, name, then a filler that depends on the tag so that no two records look alike
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

struct Seg { uint8_t *base; uint64_t n_bytes, n; uint64_t *off; };

// the records (in input order, cut into segments at `cuts`) through rs_key, the model, and rs_gather_tile for every tile under the given slab sizes
static void run_case(const std::vector<std::string> &recs, const std::vector<size_t> &cuts, const std::vector<ull> &want_keys, const char *what,
                     std::vector<ull> *doff_out, std::vector<uint32_t> *perm_out, std::vector<uint64_t> *srcs_out)
{
    const size_t N = recs.size();
    std::vector<Seg> segs;
    std::vector<ull> key(N), src(N);
    std::vector<uint32_t> len(N);
    size_t at = 0;
    for (size_t c = 0; c + 1 < cuts.size(); ++c) {
        Seg g;
        g.n = cuts[c + 1] - cuts[c];
        g.n_bytes = 0;
        for (size_t i = cuts[c]; i < cuts[c + 1]; ++i) g.n_bytes += recs[i].size();
        g.base = (uint8_t *)malloc(g.n_bytes ? g.n_bytes : 1);
        g.off = (uint64_t *)malloc(8 * (g.n + 1));
        uint64_t o = 0;
        for (size_t i = cuts[c]; i < cuts[c + 1]; ++i) { g.off[i - cuts[c]] = o; memcpy(g.base + o, recs[i].data(), recs[i].size()); o += recs[i].size(); }
        g.off[g.n] = o;
        for (uint64_t i = 0; i < g.n; ++i, ++at) {
            uint64_t k = 0; uint32_t l = 0;
            const bool ok = rs_key(g.base, g.n_bytes, g.off, i, g.n, &k, &l);
            CHECK(ok);
            key[at] = k; len[at] = l; src[at] = (ull)(uintptr_t)(g.base + g.off[i]);
            CHECK(k == want_keys[at] && l == recs[at].size());
        }
        segs.push_back(g);
    }
    std::vector<uint32_t> perm(N);
    for (size_t i = 0; i < N; ++i) perm[i] = (uint32_t)i;
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    // exactly sized tables, as the kernel gets them
    ull *doff = (ull *)malloc(8 * (N + 1)), *ssrc = (ull *)malloc(N ? 8 * N : 1);
    ull total = 0;
    for (size_t j = 0; j < N; ++j) { doff[j] = total; total += len[perm[j]]; ssrc[j] = src[perm[j]]; }
    doff[N] = total;
    uint8_t *expect = (uint8_t *)malloc(total ? total : 1);
    for (size_t j = 0; j < N; ++j) memcpy(expect + doff[j], recs[perm[j]].data(), recs[perm[j]].size());
    const ull n_tiles = (total + RS_TILE - 1) / RS_TILE;
    uint8_t *lds = (uint8_t *)aligned_alloc(16, RS_TILE);
    rs_desc *D = (rs_desc *)malloc(sizeof(rs_desc));
    for (ull slab_tiles : {1ull, 3ull, n_tiles ? n_tiles : 1ull}) {
        for (ull t = 0; t < n_tiles; t += slab_tiles) {
            const ull te = std::min(n_tiles, t + slab_tiles), bytes = std::min(total, te * RS_TILE) - t * RS_TILE;
            uint8_t *slab = (uint8_t *)malloc(bytes);          // (16-byte aligned by malloc, and exactly the slab's bytes)
            memset(slab, 0xa5, bytes);
            for (ull x = t; x < te; ++x) {
                memset(lds, 0x5a, RS_TILE);
                memset(D, 0x5a, sizeof(rs_desc));
                rs_gather_tile(doff, ssrc, (int64_t)N, total, x, lds, D, slab, t * RS_TILE, 0, 1);
            }
            if (memcmp(slab, expect + t * RS_TILE, bytes) != 0) { fprintf(stderr, "%s: slab of %llu tiles at tile %llu differs from the model\n", what, slab_tiles, t); ++fails; }
            free(slab);
        }
        // a tile past the end and a call with no records store nothing
        uint8_t *past = (uint8_t *)malloc(RS_TILE);
        memset(past, 0x77, RS_TILE);
        rs_gather_tile(doff, ssrc, (int64_t)N, total, n_tiles, lds, D, past, n_tiles * RS_TILE, 0, 1);
        CHECK(std::count(past, past + RS_TILE, (uint8_t)0x77) == (long)RS_TILE);
        free(past);
    }
    if (doff_out) doff_out->assign(doff, doff + N + 1);
    if (perm_out) *perm_out = perm;
    if (srcs_out) { srcs_out->clear(); for (const Seg &g : segs) { srcs_out->push_back((uint64_t)(uintptr_t)g.base); srcs_out->push_back(g.n_bytes); } }
    free(lds); free(D); free(expect); free(doff); free(ssrc);
    for (Seg &g : segs) { free(g.base); free(g.off); }
}

static void bad_tables()
{
    std::vector<std::string> r = {record(0, 5, "x", 40, 1), record(0, 6, "y", 50, 2), record(1, 7, "z", 36 + 2, 3)};
    std::string s = r[0] + r[1] + r[2];
    auto bad_at = [&](std::vector<uint64_t> off, const std::string &bytes) -> long {
        uint8_t *b = (uint8_t *)malloc(bytes.size());
        memcpy(b, bytes.data(), bytes.size());
        uint64_t *o = (uint64_t *)malloc(8 * off.size());
        memcpy(o, off.data(), 8 * off.size());
        long first = -1;
        for (uint64_t i = 0; i + 1 < off.size(); ++i) { uint64_t k; uint32_t l; if (!rs_key(b, bytes.size(), o, i, off.size() - 1, &k, &l) && first < 0) first = (long)i; }
        free(b); free(o);
        return first;
    };
    CHECK(bad_at({0, 40, 90, 128}, s) == -1);
    CHECK(bad_at({0, 40, 91, 128}, s) == 2);                 // the third entry disagrees with record 1's block_size: record 2 does not start where record 1 ends
    CHECK(bad_at({0, 41, 90, 128}, s) == 1);
    CHECK(bad_at({0, 40, 40, 128}, s) == 1);                 // not rising: record 1 has no span
    CHECK(bad_at({0, 40, 60, 128}, s) == 1);                 // 20 bytes cannot be a record: its fields are not read
    CHECK(bad_at({0, 40, 90, 127}, s) == 2);                 // the last offset is not n_bytes
    CHECK(bad_at({0, 40, 90, 4000}, s) == 2);                // past the stream: not read
    CHECK(bad_at({4, 40, 90, 128}, s) == 0);                 // does not start at 0
    std::string small = s;
    small[90] = 31;                                          // block_size below 32 in the last record
    CHECK(bad_at({0, 40, 90, 128}, small) == 2);
    CHECK(bad_at({0, 40, 90, 125}, small.substr(0, 125)) == 2);          // and with offsets to match: 35 bytes cannot be a record
    small = s;
    small[0] = 30;                                           // block_size below 32 in the first: no span of 36 bytes agrees with it, record 1 cannot start there
    CHECK(bad_at({0, 34, 90, 128}, small) == 0);
    CHECK(bad_at({0, 40, 90, 128}, small) == 1);
}

static void header_rule()
{
    CHECK(recsort_header_so("@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:a\tLN:5\n") == "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:a\tLN:5\n");
    CHECK(recsort_header_so("@HD\tVN:1.6\tGO:query\n@SQ\tSN:a\tLN:5\n") == "@HD\tVN:1.6\tGO:query\tSO:coordinate\n@SQ\tSN:a\tLN:5\n");
    CHECK(recsort_header_so("@HD\tSO:queryname\tVN:1.6\tGO:query\n") == "@HD\tSO:coordinate\tVN:1.6\tGO:query\n");
    CHECK(recsort_header_so("@SQ\tSN:a\tLN:5\n") == "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:a\tLN:5\n");
    CHECK(recsort_header_so("") == "@HD\tVN:1.6\tSO:coordinate\n");
    CHECK(recsort_header_so("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:a\tLN:5\n") == "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:a\tLN:5\n");
    CHECK(recsort_header_so("@HD\tVN:1.4") == "@HD\tVN:1.4\tSO:coordinate");
    CHECK(recsort_header_so("@HD\tVN:1.4\n@CO\tSO:unsorted\n") == "@HD\tVN:1.4\tSO:coordinate\n@CO\tSO:unsorted\n");
}

int main()
{
    // ---- the list, written down in SORTED order (keys rise with the index, but for the tie block), then dealt out to the input
    struct Spec { int32_t tid, pos; std::string name; size_t total; };
    std::vector<Spec> sorted;
    sorted.push_back({0, -1, "a", 38, });                        // [0, 38): the smallest record there is with a name, at pos -1
    sorted.push_back({0, 0, "to_the_boundary", RS_TILE - 38});   // [38, 2048): ends exactly on a tile boundary
    sorted.push_back({0, 7, "fills_a_tile_but_one", RS_TILE - 1});   // [2048, 4095)
    sorted.push_back({0, 9, "one_before", 100});                 // [4095, 4195): starts 1 byte before a boundary
    sorted.push_back({0, 11, "ten_thousand", 10000});            // [4195, 14195): 99 + 10000 bytes from its tile's start: tiles 2 .. 6, five of them
    for (int i = 0; i < 48; ++i) sorted.push_back({1, 100 + i, "al" + std::to_string(i), (size_t)(41 + i)});          // lengths 41 .. 88: the sources walk through every alignment
    for (int i = 0; i < 7; ++i) sorted.push_back({2, 500, "tie" + std::to_string(i), 60});                             // one (tid, pos): input order must survive
    sorted.push_back({2, 501, "after_ties", 333});
    for (int i = 0; i < 5; ++i) sorted.push_back({-1, -1, "unplaced" + std::to_string(i), (size_t)(70 + 3 * i)});      // tid -1 sorts last, as unsigned
    const size_t N = sorted.size();
    // input order: a fixed scramble that keeps the relative order inside the two blocks of equal keys (j -> (j * 29) % N is a bijection for these N records; checked)
    std::vector<size_t> order;
    { std::vector<bool> seen(N, false); for (size_t j = 0; j < N; ++j) { const size_t i = (j * 29 + 11) % N; CHECK(!seen[i]); seen[i] = true; order.push_back(i); } }
    for (const char *block : {"tie", "unplaced"}) {          // records of one key: their input order is their order in the list
        std::vector<size_t> at, ids;
        for (size_t j = 0; j < N; ++j) if (sorted[order[j]].name.rfind(block, 0) == 0) { at.push_back(j); ids.push_back(order[j]); }
        std::sort(ids.begin(), ids.end());
        for (size_t t = 0; t < at.size(); ++t) order[at[t]] = ids[t];
    }
    std::vector<std::string> recs;
    std::vector<ull> keys;
    for (size_t j = 0; j < N; ++j) { const Spec &s = sorted[order[j]]; recs.push_back(record(s.tid, s.pos, s.name, s.total, (uint32_t)order[j])); keys.push_back(key_of(s.tid, s.pos)); }
    std::vector<ull> doff; std::vector<uint32_t> perm; std::vector<uint64_t> segs;
    const std::vector<size_t> cuts = {0, 1, 24, 25, 50, N};          // five segments, two of them of one record
    run_case(recs, cuts, keys, "list", &doff, &perm, &segs);
    // the model put the list back into the order it was written down in, ties in input order
    for (size_t j = 0; j < N; ++j) CHECK(order[perm[j]] == j);
    // ---- the edges the list is there for
    CHECK(doff[1] == 38 && recs[perm[0]].size() == 38);
    CHECK(doff[2] == RS_TILE);                                            // a record ends exactly on a boundary
    CHECK(doff[3] % RS_TILE == RS_TILE - 1);                              // one starts 1 byte before one
    CHECK(doff[5] - doff[4] == 10000 && (doff[5] - 1) / RS_TILE - doff[4] / RS_TILE + 1 == 5);
    CHECK(doff[N] % 16 != 0);                                             // the last tile's tail goes out narrower
    {   // sources at every alignment mod 16; a first and a last record of a segment among the unaligned ones
        std::set<unsigned> al; bool first_unal = false, last_unal = false;
        size_t at = 0;
        for (size_t c = 0; c + 1 < cuts.size(); ++c) {
            uint64_t o = 0;
            for (size_t i = cuts[c]; i < cuts[c + 1]; ++i, ++at) {
                const uint64_t a = segs[2 * c] + o, e = a + recs[i].size();
                al.insert((unsigned)(a & 15));
                if (i == cuts[c] && (e & 15)) first_unal = true;          // (a segment's first byte is where malloc puts it: the record's END is unaligned, the last word guarded)
                if (i + 1 == cuts[c + 1] && (a & 15) && (e & 15)) last_unal = true;
                o += recs[i].size();
            }
            CHECK(o == segs[2 * c + 1]);
        }
        CHECK(al.size() == 16 && first_unal && last_unal);
    }
    // ---- zero records, one record
    run_case({}, {0, 0}, {}, "empty", nullptr, nullptr, nullptr);
    run_case({record(3, 77, "only", 61, 9)}, {0, 1}, {key_of(3, 77)}, "one", nullptr, nullptr, nullptr);
    run_case({record(3, 77, "only_long", 5000, 9)}, {0, 1}, {key_of(3, 77)}, "one long", nullptr, nullptr, nullptr);
    bad_tables();
    header_rule();
    if (fails) { printf("sort_host FAILED %d\n", fails); return 1; }
    printf("sort_host OK %zu %llu %llu\n", N, doff[N], (doff[N] + RS_TILE - 1) / RS_TILE);
    return 0;
}
