// The bodies of seqlib_amd/csrc/win_host.h and dev_win.h on the host, under ASan + UBSan, as a program of its own (tests/test_win_host.py builds and runs it):
// the measure step, the extract and the tile gather, lane 0 of 1, the way the kernels call them.
//   win_host_test cases <expect>     <expect>, written by Python from tests/win_util.py:
//       "R skip_flags qual_trim original_strand"          the rules for what follows
//       "T t qual_hex start end"                          wn_trim, the lane form and the wave form, against the reference's pair
//       "B n stream_hex off,off,... err bad statuses bases_hex quals_hex"
//            a batch: err 1 and the record named, or err 0, the status of every record, and the kept reads' text in record order -- what the extract writes
//            into an arena segment and the gather then brings together
//   Every stream, offset table, segment and output lies in a heap block of exactly its size: one byte more is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "dev_win.h"

static std::vector<uint8_t> unhex(const std::string &s)
{
    std::vector<uint8_t> o;
    if (s == "-") return o;
    for (size_t i = 0; i + 1 < s.size(); i += 2) o.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
    return o;
}
template <class T> static std::vector<T> numbers(const std::string &s)
{
    std::vector<T> o;
    if (s == "-") return o;
    std::istringstream in(s);
    std::string tok;
    while (std::getline(in, tok, ',')) o.push_back((T)std::stoll(tok));
    return o;
}
struct Block {
    uint8_t *p; size_t n;
    Block(const void *src, size_t len) : p((uint8_t *)std::malloc(len ? len : 1)), n(len) { if (len && src) std::memcpy(p, src, len); }
    ~Block() { std::free(p); }
    Block(const Block &) = delete;
};

static int cases(const char *path)
{
    std::ifstream f(path);
    std::string line;
    wn_rules R = {0u, -1, 0u, WN_WAVE_LEN};
    int n_batches = 0, n_trims = 0;
    long n_records = 0;
    const char lut[] = WN_SEQ_FWD WN_SEQ_REV;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "R") { long a, b, c; in >> a >> b >> c; R.skip_flags = (uint32_t)a; R.qual_trim = (int32_t)b; R.original_strand = (uint32_t)c; }
        else if (cmd == "T") {
            int t, ws, we;
            std::string qh;
            in >> t >> qh >> ws >> we;
            const std::vector<uint8_t> q = unhex(qh);
            Block Q(q.data(), q.size());
            int32_t a = 7, b = 7, c = 7, d = 7;
            wn_trim<false>(Q.p, (int32_t)Q.n, t, &a, &b, 0, 1);
            wn_trim<true>(Q.p, (int32_t)Q.n, t, &c, &d, 0, 1);
            if (a != ws || b != we || c != ws || d != we) { std::printf("FAILED trim %d: (%d, %d) and (%d, %d), expected (%d, %d)\n", n_trims, a, b, c, d, ws, we); return 1; }
            ++n_trims;
        } else if (cmd == "B") {
            uint64_t n; int want_err; long long want_bad;
            std::string shex, offs, sts, bhex, qhex;
            in >> n >> shex >> offs >> want_err >> want_bad >> sts >> bhex >> qhex;
            const std::vector<uint8_t> s = unhex(shex), want_b = unhex(bhex), want_q = unhex(qhex);
            const std::vector<uint64_t> off = numbers<uint64_t>(offs);
            const std::vector<uint32_t> want_st = numbers<uint32_t>(sts);
            Block S(s.data(), s.size()), O(off.data(), 8 * off.size());
            std::vector<wn_rec> M;
            uint64_t bad = ED_NONE;
            const bool ok = wn_measure_on_host(R, S.p, S.n, (const uint64_t *)O.p, n, &M, &bad);
            if (ok == (want_err != 0) || (want_err && (long long)bad != want_bad)) {
                std::printf("FAILED batch %d: %s naming %lld, expected error %d naming %lld\n", n_batches, ok ? "accepted" : "refused", (long long)bad, want_err, want_bad);
                return 1;
            }
            if (!want_err) {
                std::vector<unsigned long long> aoff(n + 1, 0), roff(1, 0);
                std::vector<uint32_t> kept;
                for (uint64_t i = 0; i < n; ++i) {
                    if (M[i].status != want_st[i]) { std::printf("FAILED batch %d: record %llu has status %u, expected %u\n", n_batches, (unsigned long long)i, M[i].status, want_st[i]); return 1; }
                    aoff[i + 1] = aoff[i] + (M[i].status == WN_KEEP ? wn_padded(M[i].klen) : 0);
                    if (M[i].status == WN_KEEP) { kept.push_back((uint32_t)i); roff.push_back(roff.back() + M[i].klen); }
                }
                const uint64_t seg = aoff[n], total = roff.back();
                Block AB(nullptr, seg), AQ(nullptr, seg), MB(M.data(), sizeof(wn_rec) * M.size()), AO(aoff.data(), 8 * aoff.size());
                for (uint64_t w = 0; w < seg / 16; ++w) wn_extract_word(S.p, (const uint64_t *)O.p, (const unsigned long long *)AO.p, (const wn_rec *)MB.p, n, w, lut, AB.p, AQ.p);
                std::vector<wn_entry> ent;
                std::vector<uint32_t> idx;
                for (size_t k = 0; k < kept.size(); ++k) {          // the entries in reverse, the index puts them right: the gather goes through idx
                    const uint32_t i = kept[kept.size() - 1 - k];
                    ent.push_back(wn_entry{(unsigned long long)(uintptr_t)(AB.p + aoff[i]), (unsigned long long)(uintptr_t)(AQ.p + aoff[i]), (long long)i, 0u, M[i].klen});
                }
                for (size_t k = 0; k < kept.size(); ++k) idx.push_back((uint32_t)(kept.size() - 1 - k));
                Block E(ent.data(), sizeof(wn_entry) * ent.size()), I(idx.data(), 4 * idx.size()), RO(roff.data(), 8 * roff.size()), OB(nullptr, total), OQ(nullptr, total);
                std::vector<uint8_t> img(WN_TILE + 16);
                uint8_t *lds = img.data() + ((16 - ((uintptr_t)img.data() & 15)) & 15);
                for (uint64_t t = 0; t * WN_TILE < total; ++t) {
                    wn_gather_tile((const unsigned long long *)RO.p, (const wn_entry *)E.p, (const uint32_t *)I.p, kept.size(), total, t, 0, lds, OB.p, 0, 1);
                    wn_gather_tile((const unsigned long long *)RO.p, (const wn_entry *)E.p, (const uint32_t *)I.p, kept.size(), total, t, 1, lds, OQ.p, 0, 1);
                }
                if (total != want_b.size() || total != want_q.size() || (total && (std::memcmp(OB.p, want_b.data(), total) || std::memcmp(OQ.p, want_q.data(), total)))) {
                    std::printf("FAILED batch %d: %llu bytes of reads, expected %zu, or they differ\n", n_batches, (unsigned long long)total, want_b.size());
                    return 1;
                }
                n_records += (long)n;
            }
            ++n_batches;
        }
    }
    std::printf("win_host_test OK: %d trims, %d batches, %ld records\n", n_trims, n_batches, n_records);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "cases")) return cases(argv[2]);
    return 2;
}
