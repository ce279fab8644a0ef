// The bodies of seqlib_amd/csrc/dev_stats.h and stats_host.h on the host, under ASan + UBSan, as a program of its own (tests/test_stats_host.py builds and runs it).
//   stats_host_test cases <expect>     <expect>, written by Python from tests/stats_util.py:
//       "B which n lo0 hi0 lo1 hi1 ..."                                the bins of a histogram
//       "C name hex err group_hex has_nm flag v0 v1 v2 v3 v4 v5"       a record, what it gives (err: 0, 1 SLX_EIO, 2 key too long)
//       "T hex"                                                        the text of all records with err 0, in order
//   Every record lies in a heap block of exactly its size.  It goes through st_record, through the lane-of-nlanes split for 1, 2, 7 and 64 lanes, and -- for what
//   must not be read -- through every truncated copy of itself, once as it is and once with block_size set to the copy's size.  The good ones are then added
//   into rows through st_adds and a group registry of two slots, and the text is compared.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "stats_host.h"

#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static std::vector<uint8_t> unhex(const std::string &s)
{
    std::vector<uint8_t> o;
    if (s == "-") return o;
    for (size_t i = 0; i + 1 < s.size(); i += 2) o.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
    return o;
}
// a heap block of exactly the bytes: one byte more is a sanitizer report
struct Block {
    uint8_t *p; size_t n;
    explicit Block(const uint8_t *src, size_t len) : p((uint8_t *)std::malloc(len ? len : 1)), n(len) { if (len) std::memcpy(p, src, len); }
    ~Block() { std::free(p); }
    Block(const Block &) = delete;
};
static int err_class(uint32_t er) { return er & (RF_E_FIELDS | RF_E_AUX) ? 1 : er & ST_E_KEY ? 2 : 0; }

// the record through `nlanes` lanes that share the CIGAR and the QUAL
static uint32_t by_lanes(const uint8_t *h, uint64_t span, uint32_t nlanes, rf_feat *F, st_rec *R)
{
    if (!rf_fixed(h, span, F)) return RF_E_FIELDS;
    st_part sum = {0, 0, 0};
    for (uint32_t lane = 0; lane < nlanes; ++lane) { st_part P; st_part_of(F, lane, nlanes, &P); st_part_join(&sum, &P); }
    return st_finish(h, F, &sum, R);
}
static bool same_rec(const st_rec &a, const st_rec &b)
{
    if (a.key_len != b.key_len || a.flag != b.flag || a.has_nm != b.has_nm) return false;
    for (int h = 0; h < ST_N_HIST; ++h) if (a.v[h] != b.v[h]) return false;
    for (uint32_t i = 0; i < a.key_len; ++i) if (st_key_byte(&a, i) != st_key_byte(&b, i)) return false;
    return true;
}

static int cases(const char *path)
{
    st_lay L;
    st_layout_default(&L, 250, 2000);
    CHECK(L.row == ST_C_N + 2 * ST_N_HIST + 776);
    st_groups G;
    G.reset(2);
    std::vector<uint64_t> rows;
    std::ifstream f(path);
    std::string line;
    int n_cases = 0, n_bins = 0, n_text = 0, n_trunc = 0;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string tag;
        in >> tag;
        if (tag == "B") {
            int which; uint32_t n;
            in >> which >> n;
            CHECK(which >= 0 && which < ST_N_HIST && L.nb[which] == n);
            for (uint32_t k = 0; k < n; ++k) {
                int32_t lo, hi;
                in >> lo >> hi;
                CHECK(st_bin_lo(&L, which, k) == lo && st_bin_hi(&L, which, k) == hi);
                for (int64_t v = lo; v <= hi; v += (hi - lo > 4 ? hi - lo : 1)) CHECK(st_slot(&L, which, v) == L.base[which] + 2 + k);
            }
            CHECK(st_slot(&L, which, (int64_t)L.start[which] - 1) == L.base[which] && st_slot(&L, which, (int64_t)L.end[which] + 1) == L.base[which] + 1);
            CHECK(st_slot(&L, which, INT64_MIN / 2) == L.base[which] && st_slot(&L, which, 1ll << 31) == L.base[which] + 1);
            ++n_bins;
        } else if (tag == "C") {
            std::string name, hex, ghex;
            int err, has_nm; uint32_t flag; int64_t v[ST_N_HIST];
            in >> name >> hex >> err >> ghex >> has_nm >> flag;
            for (auto &x : v) in >> x;
            const std::vector<uint8_t> rec = unhex(hex), key = unhex(ghex);
            Block B(rec.data(), rec.size());
            rf_feat F;
            st_rec R;
            std::memset(&R, 0, sizeof R);
            const uint32_t er = st_record(B.p, B.n, &F, &R);
            if (err_class(er) != err) { std::printf("FAILED %s: error class %d, expected %d\n", name.c_str(), err_class(er), err); return 1; }
            if (!err) {
                bool ok = R.key_len == key.size() && R.flag == flag && (int)R.has_nm == has_nm;
                for (int h = 0; ok && h < ST_N_HIST; ++h) ok = R.v[h] == v[h];
                for (uint32_t i = 0; ok && i < R.key_len; ++i) ok = st_key_byte(&R, i) == key[i];
                if (!ok) { std::printf("FAILED %s: the values or the key differ\n", name.c_str()); return 1; }
                CHECK(st_hash(&R) == st_hash_bytes(key.data(), (uint32_t)key.size()));
                for (uint32_t nl : {1u, 2u, 7u, 64u}) {
                    rf_feat F2;
                    st_rec R2;
                    std::memset(&R2, 0, sizeof R2);
                    if (by_lanes(B.p, B.n, nl, &F2, &R2) != 0 || !same_rec(R, R2)) { std::printf("FAILED %s: %u lanes differ from one\n", name.c_str(), nl); return 1; }
                }
                // into its group's row, and a look-up through the table the kernels probe
                const uint32_t g = G.intern(key.data(), (uint32_t)key.size());
                rows.resize((size_t)G.size() * L.row, 0);
                const st_tab T = {G.slots.data(), G.koff.data(), (const uint8_t *)G.pool.data(), (uint32_t)G.slots.size() - 1, 0};
                CHECK(st_lookup(&T, &R) == g);
                st_sink_host S = {rows.data() + (size_t)g * L.row};
                st_adds(&L, &R, true, S);
            }
            // truncated copies: nothing behind the copy is read, and a copy as it is never passes
            const size_t step = rec.size() > 600 ? 7 : 1;
            for (size_t n = 0; n < rec.size(); n += step) {
                Block C(rec.data(), n);
                rf_feat F3;
                st_rec R3;
                std::memset(&R3, 0, sizeof R3);
                CHECK(st_record(C.p, C.n, &F3, &R3) == RF_E_FIELDS);
                if (n >= 4) {
                    const uint32_t bs = (uint32_t)n - 4;
                    std::memcpy(C.p, &bs, 4);
                    (void)st_record(C.p, C.n, &F3, &R3);          // whatever it says, it says it from inside the block
                    for (uint32_t nl : {2u, 64u}) (void)by_lanes(C.p, C.n, nl, &F3, &R3);
                }
                ++n_trunc;
            }
            ++n_cases;
        } else if (tag == "T") {
            std::string hex;
            in >> hex;
            const std::vector<uint8_t> want = unhex(hex);
            const std::string got = st_text(L, G, rows.data());
            if (got != std::string(want.begin(), want.end())) { std::printf("FAILED: the text differs:\n%s", got.c_str()); return 1; }
            CHECK(G.n_grown >= 2);          // two slots to begin with
            for (uint32_t g = 0; g < G.size(); ++g) { const std::string nm = G.name(g); CHECK(G.find((const uint8_t *)nm.data(), (uint32_t)nm.size()) == g); }
            CHECK(G.find((const uint8_t *)"no such group", 13) == ST_NO_GROUP);
            ++n_text;
        }
    }
    std::printf("stats_host_test OK: %d cases, %d histograms, %d texts, %d truncated copies\n", n_cases, n_bins, n_text, n_trunc);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "cases")) return cases(argv[2]);
    return 2;
}
