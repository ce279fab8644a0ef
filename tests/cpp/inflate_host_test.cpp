// The per-member bodies of k_bgzf_inflate and k_bgzf_crc (seqlib_amd/csrc/dev_inflate.h) compiled for the host, one lane of one, against zlib, under
// ASan + UBSan with every buffer sized exactly (tests/test_bam_reader.py builds and runs this):
//   1. every member of the corpus file (argv[1]: repeated {u32 compressed size, u32 ISIZE, deflate bytes}) inflates to zlib's bytes, and the sliced CRC32
//      (1, 7 and 64 slices) equals zlib's crc32;
//   2. seeded single-byte and single-bit damage of every member (argv[2] variants each): the decoder returns an error, or INF_OK with exactly ISIZE bytes --
//      and the sanitizers see no access outside the member's compressed bytes and its ISIZE bytes of output;
//   3. hand-made malformed streams end with the error code that names them;
//   4. with argv[3] (tests/test_inflate_foreign.py: repeated {u32 size, u32 ISIZE, u32 expected code or 0, deflate bytes}), streams that zlib refuses or does not
//      end: inf_member returns non-zero exactly when zlib does not end the stream with ISIZE bytes, and the expected code where one is given.
// Prints "<members> members <damaged> damaged <bad> bad", and before it "<refused> refused <bad> bad" when there is an argv[3].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <zlib.h>
#include "../../seqlib_amd/csrc/dev_inflate.h"

static int run(const uint8_t *in, uint32_t n, uint32_t isize, std::vector<uint8_t> &out)
{
    // exact-size heap copies: one byte past either end is a sanitizer report
    uint8_t *ci = (uint8_t *)malloc(n ? n : 1);
    if (n) memcpy(ci, in, n);
    uint8_t *co = (uint8_t *)malloc(isize ? isize : 1);
    inf_tables *t = (inf_tables *)malloc(sizeof(inf_tables));
    memset(t, 0, sizeof *t);
    const int e = inf_member(ci, n, co, isize, t, 0, 1);
    out.assign(co, co + (e == INF_OK ? isize : 0));
    free(ci); free(co); free(t);
    return e;
}

static uint32_t crc_sliced(const uint8_t *p, uint32_t n, int nlanes)
{
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; ++i) tab[i] = inf_crc_entry(i);
    uint32_t c = 0;
    for (int l = 0; l < nlanes; ++l) c ^= inf_crc_part(tab, p, n, l, nlanes);
    return c;
}

struct BitW {
    std::vector<uint8_t> b; int n = 0;
    void put(uint32_t v, int k) { for (int i = 0; i < k; ++i) { if ((n & 7) == 0) b.push_back(0); b.back() |= (uint8_t)(((v >> i) & 1u) << (n & 7)); ++n; } }
};

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int n_var = atoi(argv[2]);
    long members = 0, damaged = 0, bad = 0;
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    uint32_t hdr[2];
    std::vector<uint8_t> comp, got;
    while (fread(hdr, 4, 2, f) == 2) {
        comp.resize(hdr[0]);
        if (hdr[0] && fread(comp.data(), 1, hdr[0], f) != hdr[0]) return 2;
        const uint32_t isize = hdr[1];
        ++members;
        std::vector<uint8_t> want(isize ? isize : 1);
        z_stream zs; memset(&zs, 0, sizeof zs);
        inflateInit2(&zs, -15);
        zs.next_in = comp.data(); zs.avail_in = hdr[0]; zs.next_out = want.data(); zs.avail_out = isize;
        const int zr = inflate(&zs, Z_FINISH);
        inflateEnd(&zs);
        if (zr != Z_STREAM_END || zs.total_out != isize) { printf("corpus member %ld: zlib rc %d\n", members, zr); ++bad; continue; }
        want.resize(isize);
        const int e = run(comp.data(), hdr[0], isize, got);
        if (e != INF_OK || got != want) { printf("member %ld: rc %d, %s\n", members, e, got == want ? "same" : "differs"); ++bad; }
        const uint32_t zc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), want.data(), isize);
        for (int nl : {1, 7, 64}) if (crc_sliced(want.data(), isize, nl) != zc) { printf("member %ld: crc with %d slices\n", members, nl); ++bad; }
        // ISIZE one off either way
        if (run(comp.data(), hdr[0], isize + 1, got) != INF_E_ISIZE) { printf("member %ld: ISIZE + 1 accepted\n", members); ++bad; }
        if (isize && run(comp.data(), hdr[0], isize - 1, got) != INF_E_OUT) { printf("member %ld: ISIZE - 1 accepted\n", members); ++bad; }
        if (hdr[0] > 2 && run(comp.data(), hdr[0] / 2, isize, got) == INF_OK && isize) { printf("member %ld: half the stream accepted\n", members); ++bad; }
        for (int v = 0; v < n_var && hdr[0]; ++v) {
            std::vector<uint8_t> d = comp;
            const uint64_t r = next();
            const size_t at = (size_t)((r >> 16) % d.size());
            // the damage lands mostly in the first bytes, where the block headers and code lengths are
            const size_t where = (v & 1) ? at : at % (d.size() < 96 ? d.size() : 96);
            if (v & 2) d[where] ^= (uint8_t)(1u << (r & 7)); else d[where] = (uint8_t)(r >> 8);
            const int e2 = run(d.data(), hdr[0], isize, got);
            ++damaged;
            if (e2 == INF_OK && got.size() != isize) { printf("member %ld variant %d: ok with %zu bytes\n", members, v, got.size()); ++bad; }
            if (e2 < 0 || e2 > INF_E_ISIZE) { printf("member %ld variant %d: code %d\n", members, v, e2); ++bad; }
        }
    }
    fclose(f);
    // hand-made malformed streams
    auto expect = [&](const char *what, const std::vector<uint8_t> &s, uint32_t isize, int code) {
        const int e = run(s.data(), (uint32_t)s.size(), isize, got);
        if (e != code) { printf("%s: code %d, expected %d\n", what, e, code); ++bad; }
    };
    { BitW w; w.put(1, 1); w.put(3, 2); w.put(0, 13); expect("block type 3", w.b, 10, INF_E_BTYPE); }
    { BitW w; w.put(1, 1); w.put(0, 2); w.put(0, 5); w.put(5, 16); w.put(0, 16); w.put(0x4141, 16); w.put(0x4141, 16); w.put(0x41, 8); expect("stored LEN/NLEN", w.b, 5, INF_E_STORED); }
    { BitW w; w.put(1, 1); w.put(0, 2); w.put(0, 5); w.put(5, 16); w.put(0xfffa, 16); w.put(0x4141, 16); expect("stored past the input", w.b, 5, INF_E_STORED); }
    { BitW w; w.put(1, 1); w.put(1, 2); w.put(0x40, 7); w.put(0, 5); w.put(0, 16); expect("distance before the output", w.b, 10, INF_E_DIST); }      // fixed: length 3 (code 0000001), distance 1 at p = 0
    { BitW w; w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(0, 4); for (int i = 0; i < 4; ++i) w.put(1, 3); w.put(0, 32); expect("over-subscribed code", w.b, 10, INF_E_CODE); }
    { BitW w; w.put(1, 1); w.put(2, 2); w.put(30, 5); w.put(0, 5); w.put(0, 4); w.put(0, 32); expect("HLIT above 286", w.b, 10, INF_E_CODE); }
    { BitW w; w.put(1, 1); w.put(1, 2); w.put(0x63, 8); w.put(0, 16); expect("length symbol 286", w.b, 10, INF_E_SYM); }          // fixed 11000110 -> symbol 286, sent MSB first
    { std::vector<uint8_t> e; expect("empty input", e, 0, INF_E_EOF); }
    // the refused set (argv[3]: repeated {u32 size, u32 ISIZE, u32 expected code or 0 for any non-zero, bytes}): zlib does not end the stream with ISIZE bytes exactly
    // when inf_member returns non-zero, and with the code named where one is
    if (argc > 3) {
        FILE *g = fopen(argv[3], "rb");
        if (!g) return 2;
        long refused = 0, rbad = 0;
        uint32_t h3[3];
        while (fread(h3, 4, 3, g) == 3) {
            comp.resize(h3[0]);
            if (h3[0] && fread(comp.data(), 1, h3[0], g) != h3[0]) return 2;
            ++refused;
            std::vector<uint8_t> want(h3[1] + 1);
            z_stream zs; memset(&zs, 0, sizeof zs);
            inflateInit2(&zs, -15);
            zs.next_in = comp.data(); zs.avail_in = h3[0]; zs.next_out = want.data(); zs.avail_out = h3[1];
            const int zr = inflate(&zs, Z_FINISH);
            const bool zok = zr == Z_STREAM_END && zs.total_out == h3[1];
            inflateEnd(&zs);
            const int e = run(comp.data(), h3[0], h3[1], got);
            if (zok) { printf("refused %ld: zlib accepts it\n", refused); ++rbad; }
            if (zok != (e == INF_OK)) { printf("refused %ld: zlib %s, inf_member %d\n", refused, zok ? "accepts" : "refuses", e); ++rbad; }
            if (h3[2] && e != (int)h3[2]) { printf("refused %ld: code %d, expected %u\n", refused, e, h3[2]); ++rbad; }
        }
        fclose(g);
        printf("%ld refused %ld bad\n", refused, rbad);
        bad += rbad;
    }
    printf("%ld members %ld damaged %ld bad\n", members, damaged, bad);
    return bad ? 1 : 0;
}
