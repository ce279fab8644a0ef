// samw_host_test.cpp -- the host-compilable parts of the SAM writer (seqlib_amd/csrc/samw_host.h, dev_samw.h) against the expectations that the Python statement of
// the rules wrote (tests/samw_util.py: dump_expectations).  Stand-alone: no library, no GPU; tests/test_samw_host.py builds it with -fsanitize=address,undefined and
// runs it.
//   1. samwh_format over each case: the line byte for byte, or a refusal where Python raises;
//   2. the kernel's per-record body (samw_line with samw_no_float as k_samw_size and k_samw_fill call it on one lane, then samw_bulk): SLOW exactly on the records
//      with f, d or B:f fields, ERROR exactly where the host formatter refuses, DEFER (with the kernel's threshold) only above the threshold, and a FAST record's
//      line equal to the expectation, written into a heap block of exactly its size;
//   3. both over every case truncated at every byte, block_size adjusted to the truncation: every run ends in FAST, SLOW or ERROR, a FAST line is the expected
//      line cut in front of one of its fields, and the two bodies agree.  A record of up to 4 KiB lies in a heap block of exactly its size, so that a byte read
//      past it is a sanitizer report; behind a longer one the bytes past the cut are poisoned by hand.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "samw_host.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#else
#define POISON(p, n) ((void)(p), (void)(n))
#define UNPOISON(p, n) ((void)(p), (void)(n))
#endif

struct Case { std::string name, rec, line; uint32_t ok, slow; };

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); if (++g_fail > 20) return; } } while (0)

static bool rd_u32(FILE *f, uint32_t &v) { return std::fread(&v, 4, 1, f) == 1; }
static bool rd_blob(FILE *f, std::string &s)
{
    uint32_t n;
    if (!rd_u32(f, n)) return false;
    s.resize(n);
    return n == 0 || std::fread(&s[0], 1, n, f) == n;
}

// the kernel's body on one record: verdict, and for FAST the line
static int dev_line(const uint8_t *r, uint64_t n, const samw_refs &R, std::string &line, uint32_t defer, int *err)
{
    samw_fld F;
    memset(&F, 0, sizeof F);
    uint64_t size = 0, size2 = 0;
    int v = samw_line(r, n, R, &F, (uint8_t *)nullptr, &size, err, 0u, 1u, lanes_one(), samw_no_float(), defer);
    line.clear();
    if (v != SAMW_FAST) return v;
    uint8_t *out = (uint8_t *)malloc(size);          // exactly the size: a byte written past it is a sanitizer report
    memset(out, 0xa5, size);
    v = samw_line(r, n, R, &F, out, &size2, err, 0u, 1u, lanes_one(), samw_no_float(), SAMW_NO_DEFER);
    if (v == SAMW_FAST && size2 == size) samw_bulk(r, F, out, 0, 1); else v = -1;
    line.assign((const char *)out, size);
    free(out);
    return v;
}

static void one_cut(const Case &c, const uint8_t *s, size_t cut, const samw_refs &R, long *n_fast, long *n_slow, long *n_err)
{
    std::vector<uint8_t> hline;
    std::string dline;
    int herr = 0, derr = 0;
    const int hv = samwh_format(s, cut, R, hline, &herr);
    const int dv = dev_line(s, cut, R, dline, SAMW_NO_DEFER, &derr);
    CHECK(hv == SAMW_FAST || hv == SAMW_ERROR, "%s cut at %zu: host verdict %d", c.name.c_str(), cut, hv);
    CHECK(dv == SAMW_FAST || dv == SAMW_SLOW || dv == SAMW_ERROR, "%s cut at %zu: kernel-body verdict %d", c.name.c_str(), cut, dv);
    CHECK((hv == SAMW_ERROR) == (dv == SAMW_ERROR) && (hv != SAMW_ERROR || herr == derr), "%s cut at %zu: host %d (%d), kernel body %d (%d)", c.name.c_str(), cut, hv, herr, dv, derr);
    if (hv == SAMW_FAST) {
        const std::string h(hline.begin(), hline.end());
        const size_t k = h.size() - 1;
        if (c.ok)          // (a refused record has no expected line; what is left of it may well be a record)
            CHECK(k < c.line.size() && h[k] == '\n' && c.line.compare(0, k, h, 0, k) == 0 && (c.line[k] == '\t' || c.line[k] == '\n'),
                  "%s cut at %zu: the line is not the expected one cut in front of a field", c.name.c_str(), cut);
        if (dv == SAMW_FAST) CHECK(dline == h, "%s cut at %zu: the two bodies differ", c.name.c_str(), cut);
    }
    ++*(dv == SAMW_FAST ? n_fast : dv == SAMW_SLOW ? n_slow : n_err);
}

static void run(const std::vector<Case> &cases, const samw_refs &R)
{
    long n_fast = 0, n_slow = 0, n_err = 0;
    for (const Case &c : cases) {
        const uint8_t *p = (const uint8_t *)c.rec.data();
        const size_t n = c.rec.size();
        std::vector<uint8_t> hline;
        std::string dline;
        int herr = 0, derr = 0;
        const int hv = samwh_format(p, n, R, hline, &herr);
        CHECK((hv == SAMW_FAST) == (c.ok != 0), "%s: host formatter %s, Python %s", c.name.c_str(), hv == SAMW_FAST ? "takes the record" : samwh_errtext(herr), c.ok ? "takes it" : "raises");
        if (c.ok) CHECK(std::string(hline.begin(), hline.end()) == c.line, "%s: the host formatter's line differs from Python's (%zu against %zu bytes)", c.name.c_str(), hline.size(), c.line.size());
        int dv = dev_line(p, n, R, dline, 256u, &derr);
        if (dv == SAMW_DEFER) {
            CHECK(c.name.find("65535") != std::string::npos || c.name.find("1000") != std::string::npos || c.name.find("257") != std::string::npos, "%s: deferred below the threshold", c.name.c_str());
            dv = dev_line(p, n, R, dline, SAMW_NO_DEFER, &derr);
        }
        if (!c.ok) CHECK(dv == SAMW_ERROR && derr == herr, "%s: the kernel's body gives %d (%d) on a refused record, the host %d", c.name.c_str(), dv, derr, herr);
        else if (c.slow) CHECK(dv == SAMW_SLOW, "%s: a record with floating-point fields is %d", c.name.c_str(), dv);
        else CHECK(dv == SAMW_FAST && dline == c.line, "%s: the kernel's body gives %d or other bytes", c.name.c_str(), dv);
        // truncations, block_size adjusted
        if (n <= 4096) {
            for (size_t cut = 0; cut < n; ++cut) {
                uint8_t *s = (uint8_t *)malloc(cut ? cut : 1);
                if (cut) memcpy(s, p, cut);
                if (cut >= 4) { const uint32_t bs = (uint32_t)cut - 4; memcpy(s, &bs, 4); }
                one_cut(c, s, cut, R, &n_fast, &n_slow, &n_err);
                free(s);
                if (g_fail) return;
            }
        } else {
            uint8_t *s = (uint8_t *)malloc(n);
            memcpy(s, p, n);
            for (size_t cut = n; cut-- > 0;) {
                POISON(s + cut, n - cut);
                if (cut >= 4) { const uint32_t bs = (uint32_t)cut - 4; memcpy(s, &bs, 4); }
                one_cut(c, s, cut, R, &n_fast, &n_slow, &n_err);
                if (g_fail) break;
            }
            UNPOISON(s, n);
            free(s);
        }
        if (g_fail) return;
    }
    std::printf("truncations: %ld FAST, %ld SLOW, %ld ERROR\n", n_fast, n_slow, n_err);
}

static void small_parts()
{
    uint8_t b[16];
    const int64_t v[] = {0, 9, 10, 99, 100, 4294967295ll, -1, -9, -10, -2147483648ll, 2147483648ll, 65535, 1000000000, 999999999};
    for (int64_t x : v) {
        char want[32];
        const int w = std::snprintf(want, sizeof want, "%lld", (long long)x);
        CHECK((int)samw_wi(x) == w && (int)samw_put_i(b, x) == w && memcmp(b, want, (size_t)w) == 0, "decimal %lld", (long long)x);
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s expectations.bin\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t n_ref = 0, n = 0;
    std::vector<std::string> refs;
    bool ok = rd_u32(f, n_ref);
    for (uint32_t i = 0; ok && i < n_ref; ++i) { std::string s; ok = rd_blob(f, s); refs.push_back(s); }
    ok = ok && rd_u32(f, n);
    std::vector<Case> cases(ok ? n : 0);
    for (Case &c : cases) ok = ok && rd_blob(f, c.name) && rd_blob(f, c.rec) && rd_u32(f, c.ok) && rd_u32(f, c.slow) && rd_blob(f, c.line);
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "%s is cut short\n", argv[1]); return 2; }
    SamwRefTable tab;
    tab.build(refs);
    run(cases, tab.view());
    if (!g_fail) small_parts();
    if (g_fail) return 1;
    std::printf("samw_host_test OK: %zu cases\n", cases.size());
    return 0;
}
