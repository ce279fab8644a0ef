// The per-member body of k_bgzf_deflate (seqlib_amd/csrc/dev_deflate.h) compiled for the host, one lane of one, against zlib, under ASan + UBSan with
// every buffer sized exactly (tests/test_bgzf_writer.py builds and runs this):
//   members <file>   the file holds repeated {u32 n, n bytes}, n <= 0xff00: each payload goes through def_member (input n bytes, output 5 + n bytes, the
//                    encoder's own bound, tokens n words), zlib inflates the stream and the bytes are compared; the member's header and trailer are framed
//                    with def_bgzf_header / def_bgzf_trailer and the sliced CRC32, and checked.  One line per payload:
//                    "<n> <stream bytes> <stored> <tokens> <matches> <longest match> <largest distance>"
//   sweep <count>    seeded payloads of 0..70 000 bytes (cut into members as the writer cuts them), alphabets of 1, 2, 4, 16 and 256 symbols, planted repeats
//   lengths          def_code_lengths alone on Fibonacci frequencies: 286 and 30 symbols with limit 15, 19 symbols with limit 7; zero frequencies; one used symbol
// Each mode ends with "<checked> checked <bad> bad".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <zlib.h>
#include "../../seqlib_amd/csrc/dev_deflate.h"

static long g_bad = 0, g_checked = 0;

struct Stats { uint32_t out_len, stored, ntok, nmatch, maxlen, maxdist; };

// one member through the encoder with exactly sized heap buffers: one byte past either end is a sanitizer report
static bool member(const uint8_t *p, uint32_t n, Stats &st, bool print)
{
    uint8_t *in = (uint8_t *)malloc(n ? n : 1);
    if (n) memcpy(in, p, n);
    const uint32_t cap = 5 + n;
    uint8_t *out = (uint8_t *)malloc(cap);
    uint32_t *tok = (uint32_t *)malloc(n ? 4 * (size_t)n : 4);
    def_state *t = (def_state *)malloc(sizeof(def_state));
    memset(t, 0xa5, sizeof *t);
    uint32_t out_len = 0, stored = 0;
    const int e = def_member(in, n, out, cap, tok, t, 0, 1, &out_len, &stored);
    bool ok = e == DEF_OK && out_len <= cap;
    st = Stats{out_len, stored, 0, 0, 0, 0};
    if (ok && !stored) {                    // the tokens cover the input exactly
        uint32_t pos = 0, k = 0;
        while (pos < n) {
            const uint32_t tk = tok[k++];
            if (tk & 0x80000000u) {
                const uint32_t len = ((tk >> 16) & 0xffu) + 3, dist = (tk & 0xffffu) + 1;
                ++st.nmatch; if (len > st.maxlen) st.maxlen = len; if (dist > st.maxdist) st.maxdist = dist;
                if (dist > pos || dist > DEF_MAX_DIST) { printf("token %u: distance %u at position %u\n", k - 1, dist, pos); ok = false; break; }
                pos += len;
            } else ++pos;
        }
        st.ntok = k;
        if (pos != n) { printf("tokens cover %u of %u bytes\n", pos, n); ok = false; }
    }
    if (ok) {
        std::vector<uint8_t> back(n ? n : 1);
        z_stream zs; memset(&zs, 0, sizeof zs);
        inflateInit2(&zs, -15);
        zs.next_in = out; zs.avail_in = out_len; zs.next_out = back.data(); zs.avail_out = n;
        const int zr = inflate(&zs, Z_FINISH);
        const bool all_in = zs.avail_in == 0;
        inflateEnd(&zs);
        if (zr != Z_STREAM_END || zs.total_out != n || !all_in || (n && memcmp(back.data(), in, n) != 0)) {
            printf("zlib: rc %d, %lu of %u bytes, %s\n", zr, (unsigned long)zs.total_out, n, zs.msg ? zs.msg : "");
            ok = false;
        }
        if (stored != (uint32_t)(((out[0] >> 1) & 3) == 0) || !(out[0] & 1)) { printf("stored flag %u, first byte %02x\n", stored, out[0]); ok = false; }
        if (!stored && out_len >= 5 + n) { printf("a coded block of %u bytes for %u\n", out_len, n); ok = false; }
        // the frame: header, sliced CRC32, trailer
        uint8_t head[18], tail[8];
        def_bgzf_header(head, 18 + out_len + 8);
        uint32_t tab[256];
        for (uint32_t i = 0; i < 256; ++i) tab[i] = inf_crc_entry(i);
        uint32_t c = 0;
        for (int l = 0; l < 64; ++l) c ^= inf_crc_part(tab, in, n, l, 64);
        def_bgzf_trailer(tail, c, n);
        const uint32_t zc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), in, n);
        uint8_t want[8];
        for (int i = 0; i < 4; ++i) { want[i] = (uint8_t)(zc >> (8 * i)); want[4 + i] = (uint8_t)(n >> (8 * i)); }
        const uint32_t bsize = 18 + out_len + 8 - 1;
        if (memcmp(tail, want, 8) != 0 || head[0] != 0x1f || head[1] != 0x8b || head[3] != 4 || head[12] != 'B' || head[13] != 'C' || head[16] != (bsize & 0xff) || head[17] != bsize >> 8 ||
            18 + out_len + 8 > 65536) { printf("frame\n"); ok = false; }
    } else if (e != DEF_OK) printf("def_member: code %d\n", e);
    // twice the same bytes
    if (ok) {
        uint8_t *out2 = (uint8_t *)malloc(cap);
        uint32_t l2 = 0, s2 = 0;
        memset(t, 0x5a, sizeof *t);
        const int e2 = def_member(in, n, out2, cap, tok, t, 0, 1, &l2, &s2);
        if (e2 != DEF_OK || l2 != out_len || memcmp(out, out2, out_len) != 0) { printf("second run differs\n"); ok = false; }
        free(out2);
    }
    if (print) printf("%u %u %u %u %u %u %u\n", n, st.out_len, st.stored, st.ntok, st.nmatch, st.maxlen, st.maxdist);
    ++g_checked;
    if (!ok) { printf("payload of %u bytes: bad\n", n); ++g_bad; }
    free(in); free(out); free(tok); free(t);
    return ok;
}

static int lengths_case(const char *what, const std::vector<uint32_t> &f, int limit)
{
    const int n = (int)f.size();
    def_huff *h = (def_huff *)malloc(sizeof(def_huff));
    memset(h, 0xa5, sizeof *h);
    uint32_t *freq = (uint32_t *)malloc(4 * (size_t)n);
    memcpy(freq, f.data(), 4 * (size_t)n);
    uint8_t *len = (uint8_t *)malloc((size_t)n);
    def_code_lengths(freq, n, limit, len, h, 0, 1);
    int used = 0, coded = 0, bad = 0;
    uint64_t kraft = 0;
    for (int s = 0; s < n; ++s) {
        used += f[s] != 0;
        if (len[s] > limit) { printf("%s: symbol %d has %d bits\n", what, s, len[s]); bad = 1; }
        if (len[s]) { ++coded; kraft += 1ull << (limit - len[s]); }
        if (f[s] && !len[s]) { printf("%s: used symbol %d has no code\n", what, s); bad = 1; }
    }
    if (kraft != 1ull << limit) { printf("%s: Kraft sum %llu / %llu\n", what, (unsigned long long)kraft, 1ull << limit); bad = 1; }
    if (coded != (used < 2 ? 2 : used)) { printf("%s: %d codes for %d used symbols\n", what, coded, used); bad = 1; }
    // a heavier symbol never has the longer code
    for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) if (f[a] > f[b] && f[b] && len[a] > len[b]) { printf("%s: %d (x%u) longer than %d (x%u)\n", what, a, f[a], b, f[b]); bad = 1; a = n; break; }
    free(h); free(freq); free(len);
    ++g_checked; g_bad += bad;
    return bad;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    Stats st;
    if (mode == "members" && argc >= 3) {
        FILE *f = fopen(argv[2], "rb");
        if (!f) return 2;
        uint32_t n;
        std::vector<uint8_t> p;
        while (fread(&n, 4, 1, f) == 1) {
            if (n > DEF_MEMBER) return 2;
            p.resize(n);
            if (n && fread(p.data(), 1, n, f) != n) return 2;
            member(p.data(), n, st, true);
        }
        fclose(f);
    } else if (mode == "sweep" && argc >= 3) {
        uint64_t rng = 0x2545f4914f6cdd1dull;
        auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
        const int alpha[5] = {1, 2, 4, 16, 256};
        uint64_t in_bytes = 0, out_bytes = 0;
        for (int it = 0; it < atoi(argv[2]); ++it) {
            const uint32_t len = it < 8 ? (uint32_t)it : (uint32_t)(next() % 70001);
            const int a = alpha[it % 5];
            std::vector<uint8_t> p(len);
            for (auto &b : p) b = (uint8_t)(next() % (uint64_t)a * (a == 256 ? 1 : 37));
            for (int r = 0; len > 16 && r < (int)(next() % 12); ++r) {            // planted repeats: a piece copied further on, near and far
                const uint32_t l = 3 + (uint32_t)(next() % 600), from = (uint32_t)(next() % len), to = (uint32_t)(next() % len);
                for (uint32_t i = 0; i < l && from + i < len && to + i < len; ++i) p[to + i] = p[from + i];
            }
            for (uint32_t o = 0; o < len || o == 0; o += DEF_MEMBER) {
                const uint32_t n = len - o < DEF_MEMBER ? len - o : DEF_MEMBER;
                member(p.data() + o, n, st, false);
                in_bytes += n; out_bytes += st.out_len;
                if (len == 0) break;
            }
        }
        printf("sweep: %llu bytes in, %llu out\n", (unsigned long long)in_bytes, (unsigned long long)out_bytes);
    } else if (mode == "lengths") {
        auto fib = [](int n, int zero_every) {
            std::vector<uint32_t> f((size_t)n);
            uint32_t a = 1, b = 1;
            for (int i = 0; i < n; ++i) {
                f[i] = zero_every && i % zero_every == 0 ? 0 : a;
                const uint32_t c = a + b > 0x3fffffffu / (uint32_t)n ? a : a + b;      // (286 Fibonacci numbers do not fit: the sum of all weights stays below 2^30)
                a = b; b = c;
            }
            return f;
        };
        lengths_case("286 symbols, limit 15", fib(286, 0), 15);
        lengths_case("286 symbols with zeros, limit 15", fib(286, 3), 15);
        lengths_case("30 symbols, limit 15", fib(30, 0), 15);
        lengths_case("30 symbols with zeros, limit 15", fib(30, 4), 15);
        lengths_case("19 symbols, limit 7", fib(19, 0), 7);
        lengths_case("19 symbols with zeros, limit 7", fib(19, 5), 7);
        for (int n : {286, 30, 19}) {
            std::vector<uint32_t> one((size_t)n, 0), none((size_t)n, 0), two((size_t)n, 0), flat((size_t)n, 7);
            one[(size_t)n / 2] = 9; two[0] = 1; two[(size_t)n - 1] = 100000;
            lengths_case("one used symbol", one, n == 19 ? 7 : 15);
            lengths_case("no used symbol", none, n == 19 ? 7 : 15);
            lengths_case("two used symbols", two, n == 19 ? 7 : 15);
            lengths_case("equal weights", flat, n == 19 ? 7 : 15);
            one.assign((size_t)n, 0); one[0] = 5;
            lengths_case("symbol 0 alone", one, n == 19 ? 7 : 15);
        }
    } else return 2;
    printf("%ld checked %ld bad\n", g_checked, g_bad);
    return g_bad ? 1 : 0;
}
