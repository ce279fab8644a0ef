// The host side of the BAI index (seqlib_amd/csrc/slx_bai.cpp) under ASan + UBSan (tests/test_bai_host.py): the file given is parsed from an exactly
// sized heap copy at every length from 0 to its own, so a read past the bytes left is a heap overflow the sanitizer sees; every cut must be refused with
// SLX_EIO or, where only the optional trailer is missing, load cleanly.  Then the whole file is queried over a sweep of regions.
//   san_bai_test <file.bai>     stdout: "cuts <n> eio <n> clean <n> chunks <n>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>
#include "slx_internal.h"
#include "bai_host.h"

// slx_index.cpp is linked for slx_set_error; its device builds are not part of a host build
int slx_gpu_build_fm(slx_index *, const uint8_t *, uint64_t) { slx_set_error("no device in the sanitizer build"); return SLX_ENODEVICE; }
int slx_gpu_build_fm64(slx_index *, const uint8_t *, uint64_t) { slx_set_error("no device in the sanitizer build"); return SLX_ENODEVICE; }

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (all.empty()) return 2;
    size_t eio = 0, clean = 0;
    for (size_t n = 0; n <= all.size(); ++n) {
        uint8_t *copy = (uint8_t *)malloc(n ? n : 1);
        memcpy(copy, all.data(), n);
        Bai b;
        const int rc = bai_parse(copy, n, "cut", b);
        free(copy);
        if (rc == SLX_EIO) ++eio;
        else if (rc == SLX_OK) ++clean;
        else { std::printf("length %zu: code %d\n", n, rc); return 1; }
    }
    Bai b;
    if (bai_parse(all.data(), all.size(), argv[1], b) != SLX_OK) return 1;
    size_t chunks = 0;
    std::vector<std::pair<uint64_t, uint64_t>> ch;
    for (int tid = -1; tid <= (int)b.refs.size(); ++tid)
        for (int64_t beg = -20000; beg < 400000; beg += 4093)
            for (int64_t len : {0ll, 1ll, 16384ll, 1ll << 40}) { bai_plan(b, tid, beg, beg + len, ch); chunks += ch.size(); }
    std::printf("cuts %zu eio %zu clean %zu chunks %zu\n", all.size() + 1, eio, clean, chunks);
    return 0;
}
