// dup_host_test -- the duplicate marker's per-record body (seqlib_amd/csrc/dup_host.h) on the CPU under ASan + UBSan, every stream and offset table in a heap
// block of exactly its size (tests/test_dup_host.py builds it and writes the cases).  Input lines:
//   H <hex of the header text or ->                                       the header for the batches that follow
//   B <n> <hex of the stream or -> <offsets, comma separated>             -> prints "S" and per record "cls lib refid upos rev score", or "E <lowest bad index>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "dup_host.h"

static std::vector<uint8_t> unhex(const std::string &h)
{
    std::vector<uint8_t> out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)std::stoul(h.substr(i, 2), nullptr, 16));
    return out;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    dp_header H;
    size_t batches = 0, records = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string kind;
        ss >> kind;
        if (kind == "H") {
            std::string hex;
            ss >> hex;
            const std::vector<uint8_t> t = unhex(hex);
            char *text = (char *)std::malloc(t.size() ? t.size() : 1);          // exactly sized: the parser must not read past l_text
            if (!t.empty()) std::memcpy(text, t.data(), t.size());
            if (!H.parse(text, (int64_t)t.size())) return 1;
            std::free(text);
        } else if (kind == "B") {
            size_t n;
            std::string hex, offs;
            ss >> n >> hex >> offs;
            const std::vector<uint8_t> s = unhex(hex);
            uint8_t *stream = (uint8_t *)std::malloc(s.size() ? s.size() : 1);
            if (!s.empty()) std::memcpy(stream, s.data(), s.size());
            uint64_t *off = (uint64_t *)std::malloc(8 * (n + 1));
            std::istringstream os(offs);
            std::string tok;
            for (size_t i = 0; i <= n && std::getline(os, tok, ','); ++i) off[i] = std::stoull(tok);
            std::vector<dp_sig> S;
            uint64_t bad = ED_NONE;
            if (!dp_signatures_on_host(H.view(), stream, s.size(), off, n, &S, &bad)) std::printf("E %llu\n", (unsigned long long)bad);
            else {
                std::printf("S\n");
                for (const dp_sig &g : S) {
                    const uint32_t cls = g.cls & DP_CLASS;
                    if (cls == DP_IGNORED) std::printf("0 0 0 0 0 0\n");
                    else std::printf("%u %u %d %lld %u %u\n", cls, g.library, (int32_t)(uint32_t)g.hi, (long long)(g.lo >> 1) - (1ll << 62), (unsigned)(g.lo & 1), g.score);
                    ++records;
                }
            }
            std::free(stream); std::free(off);
            ++batches;
        }
    }
    std::printf("dup_host_test OK: %zu batches, %zu records\n", batches, records);
    return 0;
}
