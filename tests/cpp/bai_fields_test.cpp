// The per-record bodies of the BAI build and the region filter (seqlib_amd/csrc/dev_bai.h) compiled for the host (tests/test_bai_host.py): for every record of
// an inflated record stream one line "tid pos end bin ok", with the reference length summed in one piece and, as the wave-cooperative path does, in 64 strided
// parts.  Every record is read from an exactly sized copy, so a record whose n_cigar_op passes its block_size must come back not-ok without a read past it.
//   bai_fields_test <records.bin>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>
#include "dev_bai.h"

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> s((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    for (uint64_t o = 0; o + 4 <= s.size();) {
        const uint64_t bs = bidx_u32(s.data() + o);
        if (bs < 32 || o + 4 + bs > s.size()) return 1;
        // an exactly sized copy, so that the sanitizer sees a read past the record
        uint8_t *h = (uint8_t *)malloc(4 + bs);
        memcpy(h, s.data() + o, 4 + bs);
        const bai_fields f = bai_read(h);
        const uint64_t whole = bai_reflen_part(f.cig, 0, f.n_cig, 1);
        uint64_t parts = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) parts += bai_reflen_part(f.cig, lane, f.n_cig, 64);
        if (whole != parts) { free(h); return 1; }
        const int64_t pos = f.pos < 0 ? 0 : f.pos;
        int64_t end = bai_end(f.pos, f.flag, whole);
        std::printf("%d %d %lld %u %d\n", f.tid, f.pos, (long long)end, bai_reg2bin(pos, end <= pos ? pos + 1 : end), f.ok ? 1 : 0);
        free(h);
        o += 4 + bs;
    }
    return 0;
}
