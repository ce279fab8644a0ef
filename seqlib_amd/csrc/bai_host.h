// bai_host.h -- the BAI index (SAMv1 section 5.2) on the host: the parsed form, its loader and the query plan (slx_bai.cpp).  Plain C++, no GPU: the
// reader (slx_bam.hip) plans its region spans with it, slx_bai_query / slx_bai_stats expose it, tests/cpp/san_bai_test.cpp runs it under the sanitizers.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#define BAI_META_BIN 37450u

struct BaiBin { uint32_t bin; uint32_t first, n; };          // chunks[first, first + n) of the reference
struct BaiRef {
    std::vector<BaiBin> bins;                                // as they stand in the file, the pseudo-bin left out
    std::vector<std::pair<uint64_t, uint64_t>> chunks;
    std::vector<uint64_t> ioffset;
    int32_t n_bin = 0;                                       // the file's count, the pseudo-bin included
    bool has_meta = false;
    uint64_t meta[4] = {0, 0, 0, 0};                         // first begin voff, last end voff, n_mapped, n_unmapped
};
struct Bai {
    std::vector<BaiRef> refs;
    bool has_no_coor = false;
    uint64_t n_no_coor = 0;
};

// SLX_EIO for a file that is missing, short, truncated or whose counts pass the bytes left; never reads outside [p, p + n)
int bai_parse(const uint8_t *p, uint64_t n, const char *name, Bai &out);
int bai_load_file(const char *path, Bai &out);
// the merged chunk list (u, v) holding every record of tid that overlaps [beg, end): reg2bins, the linear index's lower bound, sort, merge
void bai_plan(const Bai &b, int tid, int64_t beg, int64_t end, std::vector<std::pair<uint64_t, uint64_t>> &out);
