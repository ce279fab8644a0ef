// The bodies of seqlib_amd/csrc/dev_ref.h and ref_host.h on the host, under ASan + UBSan, as a program of its own (tests/test_ref_host.py builds and runs it): what
// slx_ref_fai_of_text and slx_ref_record_nm_md run (rg_fai_of_text, rg_fai_text, rg_record_nm_md), called the way those entries call them.
//   ref_host_test cases <expect>     <expect>, written by Python from tests/ref_util.py:
//       "F name text_hex ok out_hex"             a FASTA text: ok 1 and its .fai text, or ok 0 and the error's sentence
//       "G index bytes_hex"                      a contig the records are walked against
//       "R name rec_hex contig err nm md_hex"    a record against contig `contig` (err 1: SLX_EIO)
//   Every text and every record lies in a heap block of exactly its size: one byte more is a sanitizer report.  A good record also goes through every truncated
//   copy of itself, once as it is (which must fail) and once with block_size set to the copy's size (whatever it says, it says it from inside the block), and
//   through a cap one byte short of its MD, which must leave the buffer alone.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "ref_host.h"

#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static std::vector<uint8_t> unhex(const std::string &s)
{
    std::vector<uint8_t> o;
    if (s == "-") return o;
    for (size_t i = 0; i + 1 < s.size(); i += 2) o.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
    return o;
}
struct Block {
    uint8_t *p; size_t n;
    explicit Block(const uint8_t *src, size_t len) : p((uint8_t *)std::malloc(len ? len : 1)), n(len) { if (len && src) std::memcpy(p, src, len); }
    ~Block() { std::free(p); }
    Block(const Block &) = delete;
};

static int cases(const char *path)
{
    std::map<int, std::vector<uint8_t>> contigs;
    std::ifstream f(path);
    std::string line;
    int n_fa = 0, n_rec = 0, n_trunc = 0;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string tag;
        in >> tag;
        if (tag == "F") {
            std::string name, hex, out;
            int ok;
            in >> name >> hex >> ok >> out;
            const std::vector<uint8_t> text = unhex(hex), want = unhex(out);
            Block B(text.data(), text.size());
            std::vector<rg_contig> C;
            std::string msg;
            const bool got = rg_fai_of_text(B.p, B.n, &C, &msg);
            const std::string have = got ? rg_fai_text(C) : msg;
            if ((int)got != ok || have != std::string(want.begin(), want.end())) { std::printf("FAILED %s: ok %d, expected %d:\n%s\n", name.c_str(), (int)got, ok, have.c_str()); return 1; }
            ++n_fa;
        } else if (tag == "G") {
            int idx; std::string hex;
            in >> idx >> hex;
            contigs[idx] = unhex(hex);
        } else if (tag == "R") {
            std::string name, hex, mdhex;
            int contig, err, nm;
            in >> name >> hex >> contig >> err >> nm >> mdhex;
            const std::vector<uint8_t> rec = unhex(hex), want = unhex(mdhex);
            const std::vector<uint8_t> &cb = contigs[contig];
            Block B(rec.data(), rec.size()), G(cb.data(), cb.size());
            int32_t got_nm = 0;
            uint64_t len = 0;
            bool ok = rg_record_nm_md(B.p, B.n, G.p, (int64_t)G.n, &got_nm, nullptr, 0, &len);
            if ((int)!ok != err) { std::printf("FAILED %s: error %d, expected %d\n", name.c_str(), (int)!ok, err); return 1; }
            if (err) { ++n_rec; continue; }
            Block M(nullptr, (size_t)len);
            ok = rg_record_nm_md(B.p, B.n, G.p, (int64_t)G.n, &got_nm, M.p, len, &len);
            if (!ok || got_nm != nm || len != want.size() || (len && std::memcmp(M.p, want.data(), len))) {
                std::printf("FAILED %s: nm %d md %.*s, expected nm %d md %.*s\n", name.c_str(), got_nm, (int)len, (const char *)M.p, nm, (int)want.size(), (const char *)want.data());
                return 1;
            }
            if (len) {          // one byte short: nothing is written
                Block S(nullptr, (size_t)len - 1);
                if (len > 1) std::memset(S.p, 0x5a, len - 1);
                uint64_t l2 = 0;
                CHECK(rg_record_nm_md(B.p, B.n, G.p, (int64_t)G.n, &got_nm, S.p, len - 1, &l2) && l2 == len);
                for (uint64_t i = 0; i + 1 < len; ++i) CHECK(S.p[i] == 0x5a);
            }
            const size_t step = rec.size() > 600 ? 97 : 1;
            for (size_t n = 0; n < rec.size(); n += step) {
                Block C(rec.data(), n);
                uint64_t l3 = 0;
                CHECK(!rg_record_nm_md(C.p, C.n, G.p, (int64_t)G.n, &got_nm, nullptr, 0, &l3));
                if (n >= 4) {
                    const uint32_t bs = (uint32_t)n - 4;
                    std::memcpy(C.p, &bs, 4);
                    (void)rg_record_nm_md(C.p, C.n, G.p, (int64_t)G.n, &got_nm, nullptr, 0, &l3);
                }
                ++n_trunc;
            }
            ++n_rec;
        }
    }
    std::printf("ref_host_test OK: %d texts, %d records, %d truncated copies\n", n_fa, n_rec, n_trunc);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "cases")) return cases(argv[2]);
    return 2;
}
