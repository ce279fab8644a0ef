// The bodies of seqlib_amd/csrc/dev_edit.h through edit_host.h on the host, under ASan + UBSan, as a program of its own (tests/test_edit_host.py builds and runs
// it): the size step and the tile gather, lane 0 of 1, the way slx_edit_record and the kernels call them.
//   edit_host_test cases <expect>     <expect>, written by Python from tests/edit_util.py; a plan, then the batches it is applied to:
//       "P"                                        a new, empty plan
//       "D tag" | "DA" | "CL"                      drop a name | drop all tags | clear_seq_qual
//       "AI tag value replace" | "AZ tag hex"      constant adds
//       "CI tag absent replace" | "CZ tag"         column adds
//       "B n stream_hex off,off,... err bad out_hex noff,noff,..."     a batch: err 0 and the edited stream and offsets, or err 1 and the record named
//       "V k v,v,..." | "T k text_hex off,off,..."                    in front of a B: the int column / the Z column of add k for that batch
//   Every stream, offset table and column lies in a heap block of exactly its size: one byte more is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "edit_host.h"

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
    ed_host_plan H;
    std::map<int, std::vector<int32_t>> vcol;
    std::map<int, std::pair<std::vector<uint8_t>, std::vector<uint64_t>>> zcol;
    int n_plans = 0, n_batches = 0;
    long n_records = 0;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string cmd, tag, a, b;
        in >> cmd;
        std::string err;
        if (cmd == "P") { H = ed_host_plan(); ++n_plans; }
        else if (cmd == "D") { in >> tag; err = ed_plan_drop(H, tag.c_str()); }
        else if (cmd == "DA") H.P.drop_all = 1;
        else if (cmd == "CL") H.P.clear = 1;
        else if (cmd == "AI") { long v; int r; in >> tag >> v >> r; err = ed_plan_add(H, tag.c_str(), ED_INT, (int32_t)v, r != 0, nullptr, 0, nullptr, nullptr, nullptr, 0); }
        else if (cmd == "AZ") { in >> tag >> a; const auto v = unhex(a); err = ed_plan_add(H, tag.c_str(), ED_Z, 0, true, v.data(), (int64_t)v.size(), nullptr, nullptr, nullptr, 0); }
        else if (cmd == "CI") { long v; int r; in >> tag >> v >> r; err = ed_plan_add(H, tag.c_str(), ED_INT_COL, (int32_t)v, r != 0, nullptr, 0, nullptr, nullptr, nullptr, 0); }
        else if (cmd == "CZ") { in >> tag; err = ed_plan_add(H, tag.c_str(), ED_Z_COL, 0, true, nullptr, 0, nullptr, nullptr, nullptr, 0); }
        else if (cmd == "V") { int k; in >> k >> a; vcol[k] = numbers<int32_t>(a); }
        else if (cmd == "T") { int k; in >> k >> a >> b; zcol[k] = {unhex(a), numbers<uint64_t>(b)}; }
        else if (cmd == "B") {
            uint64_t n; int want_err; long long want_bad;
            std::string shex, offs, ohex, noffs;
            in >> n >> shex >> offs >> want_err >> want_bad >> ohex >> noffs;
            const std::vector<uint8_t> s = unhex(shex), want = unhex(ohex);
            const std::vector<uint64_t> off = numbers<uint64_t>(offs), want_off = numbers<uint64_t>(noffs);
            Block S(s.data(), s.size()), O(off.data(), 8 * off.size());
            std::vector<Block *> keep;
            ed_plan P = H.P;
            Block C(H.consts.data(), H.consts.size());
            P.consts = C.p;
            for (uint32_t k = 0; k < P.n_add; ++k) {
                if (P.add[k].kind == ED_INT_COL) { keep.push_back(new Block(vcol[k].data(), 4 * vcol[k].size())); P.add[k].vals = (const int32_t *)keep.back()->p; }
                if (P.add[k].kind == ED_Z_COL) {
                    keep.push_back(new Block(zcol[k].first.data(), zcol[k].first.size())); P.add[k].text = keep.back()->p; P.add[k].n_text = zcol[k].first.size();
                    keep.push_back(new Block(zcol[k].second.data(), 8 * zcol[k].second.size())); P.add[k].toff = (const uint64_t *)keep.back()->p;
                }
            }
            std::vector<uint8_t> out;
            std::vector<unsigned long long> noff;
            uint64_t bad = ED_NONE;
            const uint32_t rc = ed_apply_on_host(P, S.p, S.n, (const uint64_t *)O.p, n, &out, &noff, &bad);
            for (Block *k : keep) delete k;
            if ((rc != ED_OK) != (want_err != 0) || (want_err && (rc != ED_E_RECORD || (long long)bad != want_bad))) {
                std::printf("FAILED batch %d: refusal %u naming %lld, expected error %d naming %lld\n", n_batches, rc, (long long)bad, want_err, want_bad);
                return 1;
            }
            if (!want_err) {
                bool same = out == want && noff.size() == want_off.size();
                for (size_t i = 0; same && i < noff.size(); ++i) same = noff[i] == want_off[i];
                if (!same) {
                    size_t at = 0;
                    while (at < out.size() && at < want.size() && out[at] == want[at]) ++at;
                    std::printf("FAILED batch %d: %zu bytes, expected %zu, first difference at byte %zu\n", n_batches, out.size(), want.size(), at);
                    return 1;
                }
                n_records += (long)n;
            }
            ++n_batches;
            vcol.clear(); zcol.clear();
        }
        if (!err.empty()) { std::printf("FAILED plan line '%s': %s\n", line.c_str(), err.c_str()); return 1; }
    }
    std::printf("edit_host_test OK: %d plans, %d batches, %ld records\n", n_plans, n_batches, n_records);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "cases")) return cases(argv[2]);
    return 2;
}
