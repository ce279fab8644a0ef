// sam_host_test.cpp -- the host-compilable parts of the SAM reader (seqlib_amd/csrc/sam_host.h, dev_sam.h) against the expectations that the Python statement of the
// grammar wrote (tests/sam_util.py: dump_expectations).  Stand-alone: no library, no GPU; tests/test_sam_host.py builds it with -fsanitize=address,undefined and runs it.
//   1. samh_parse_line over each case: the record byte for byte, or an error where Python raises;
//   2. the kernel's per-line body (sam_fields + sam_record with sam_no_float, as k_sam_size and k_sam_fill call it) over each case: SLOW exactly on the lines with
//      f, d or B:f fields, ERROR exactly where the host parser errs, and a FAST line's record equal to the host parser's -- also when 64 lanes fill it in turn;
//   3. both over every case truncated at every byte position and with every single byte replaced by tab, LF, NUL and 0xff: every run ends in FAST, SLOW or ERROR
//      (the line lies in a heap block of exactly its size: a byte read past it is a sanitizer report), and whenever the kernel's body says FAST its record is the
//      host parser's; when it says ERROR the host parser errs too;
//   4. sam_line_span, samh_header and the reference-name table on small inputs.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "sam_host.h"

struct Case { std::string name, line, rec; uint32_t ok, slow; };

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

// the kernel's body on one line (the reader has already dropped the CR): verdict, and for FAST the record, filled by `nl` lanes in turn
static int dev_line(const uint8_t *s, uint32_t n, const sam_refs &R, std::vector<uint8_t> &rec, uint32_t nl)
{
    sam_fld F;
    memset(&F, 0, sizeof F);
    sam_fields(s, n, &F);
    uint32_t size = 0;
    int err = 0;
    const int v = sam_record(s, n, F, R, (uint8_t *)nullptr, &size, &err, 0u, 1u, sam_no_float());
    rec.clear();
    if (v != SAM_FAST) return v;
    uint8_t *out = (uint8_t *)malloc(size);          // exactly the size: a byte written past it is a sanitizer report
    memset(out, 0xa5, size);
    for (uint32_t lane = 0; lane < nl; ++lane) {
        uint32_t sz2 = 0;
        if (sam_record(s, n, F, R, out, &sz2, &err, lane, nl, sam_no_float()) != SAM_FAST || sz2 != size) { free(out); return -1; }
    }
    rec.assign(out, out + size);
    free(out);
    return v;
}

static void one(const std::string &what, const uint8_t *line, size_t n, const sam_refs &R, long *n_fast, long *n_slow, long *n_err)
{
    uint8_t *s = (uint8_t *)malloc(n ? n : 1);
    if (n) memcpy(s, line, n);
    std::vector<uint8_t> hrec, drec;
    int herr = 0;
    const int hv = samh_parse_line(s, n, R, hrec, &herr);
    size_t m = n;
    if (m && s[m - 1] == '\r') --m;
    const int dv = dev_line(s, (uint32_t)m, R, drec, 1);
    free(s);
    CHECK(hv == SAM_FAST || hv == SAM_ERROR, "%s: host verdict %d", what.c_str(), hv);
    CHECK(dv == SAM_FAST || dv == SAM_SLOW || dv == SAM_ERROR, "%s: kernel-body verdict %d", what.c_str(), dv);
    if (dv == SAM_FAST) { CHECK(hv == SAM_FAST && hrec == drec, "%s: the kernel's body says FAST, the host parser %s", what.c_str(), hv == SAM_FAST ? "gives other bytes" : samh_errtext(herr)); ++*n_fast; }
    else if (dv == SAM_ERROR) { CHECK(hv == SAM_ERROR, "%s: the kernel's body says ERROR, the host parser takes the line", what.c_str()); ++*n_err; }
    else ++*n_slow;
}

static void run(const std::vector<Case> &cases, const sam_refs &R)
{
    long n_fast = 0, n_slow = 0, n_err = 0;
    for (const Case &c : cases) {
        const uint8_t *p = (const uint8_t *)c.line.data();
        const size_t n = c.line.size();
        std::vector<uint8_t> hrec, drec;
        int herr = 0;
        const int hv = samh_parse_line(p, n, R, hrec, &herr);
        CHECK((hv == SAM_FAST) == (c.ok != 0), "%s: host parser %s, Python %s", c.name.c_str(), hv == SAM_FAST ? "takes the line" : samh_errtext(herr), c.ok ? "takes it" : "raises");
        if (c.ok) CHECK(std::string(hrec.begin(), hrec.end()) == c.rec, "%s: the host parser's record differs from Python's (%zu against %zu bytes)", c.name.c_str(), hrec.size(), c.rec.size());
        size_t m = n;
        if (m && p[m - 1] == '\r') --m;
        for (uint32_t nl : {1u, 64u}) {
            const int dv = dev_line(p, (uint32_t)m, R, drec, nl);
            if (c.slow) CHECK(dv == SAM_SLOW || (!c.ok && dv == SAM_ERROR), "%s: a line with floating-point fields is %d", c.name.c_str(), dv);
            else if (!c.ok) CHECK(dv == SAM_ERROR, "%s: the kernel's body gives %d on a bad line", c.name.c_str(), dv);
            else CHECK(dv == SAM_FAST && std::string(drec.begin(), drec.end()) == c.rec, "%s: the kernel's body (%u lanes) gives %d or other bytes", c.name.c_str(), nl, dv);
        }
        // mutations
        for (size_t cut = 0; cut <= n; ++cut) one(c.name + " cut at " + std::to_string(cut), p, cut, R, &n_fast, &n_slow, &n_err);
        static const uint8_t repl[4] = {'\t', '\n', 0, 0xff};
        std::string mline = c.line;
        for (size_t i = 0; i < n; ++i)
            for (uint8_t r : repl) {
                if ((uint8_t)c.line[i] == r) continue;
                mline[i] = (char)r;
                one(c.name + " byte " + std::to_string(i) + " = " + std::to_string(r), (const uint8_t *)mline.data(), n, R, &n_fast, &n_slow, &n_err);
                mline[i] = c.line[i];
            }
        if (g_fail) return;
    }
    std::printf("mutations: %ld FAST, %ld SLOW, %ld ERROR\n", n_fast, n_slow, n_err);
}

static void small_parts()
{
    // line spans: LF, CRLF, an empty line, a last line without LF, and one that ends in CR
    const std::string t = "ab\ncd\r\n\nef\r";
    const unsigned long long off[5] = {0, 3, 7, 8, 12};          // the last entry: end of the input + 1
    const uint32_t want_n[4] = {2, 2, 0, 3};
    for (uint64_t k = 0; k < 4; ++k) {
        uint64_t beg; uint32_t n; bool cr;
        sam_line_span((const uint8_t *)t.data(), off, k, 4, 1, &beg, &n, &cr);
        CHECK(beg == off[k] && n == want_n[k] && cr == (k == 3), "line span %llu: %llu + %u cr %d", (unsigned long long)k, (unsigned long long)beg, n, (int)cr);
    }
    // the header
    const std::string h = "@HD\tVN:1.6\r\n@SQ\tSN:b\tLN:7\n@SQ\tLN:9\tXX:y\tSN:a\n@CO\tx\nr1\t";
    std::string text, msg;
    std::vector<std::string> names;
    std::vector<int64_t> lens;
    uint64_t body = 0, lines = 0;
    CHECK(samh_header((const uint8_t *)h.data(), h.size(), false, text, names, lens, &body, &lines, msg) == 1, "header: not complete");
    CHECK(text == "@HD\tVN:1.6\n@SQ\tSN:b\tLN:7\n@SQ\tLN:9\tXX:y\tSN:a\n@CO\tx\n" && lines == 4 && h.compare(body, 2, "r1") == 0, "header: text or body");
    CHECK(names.size() == 2 && names[0] == "b" && names[1] == "a" && lens[0] == 7 && lens[1] == 9, "header: references");
    CHECK(samh_header((const uint8_t *)h.data(), 20, false, text, names, lens, &body, &lines, msg) == 0, "header: a cut header is not 'more bytes'");
    CHECK(samh_header((const uint8_t *)h.data(), 11, true, text, names, lens, &body, &lines, msg) == 1 && text == "@HD\tVN:1.6\r\n" && body == 11, "header: a last line without LF");
    const std::string nosn = "@SQ\tLN:5\n";
    CHECK(samh_header((const uint8_t *)nosn.data(), nosn.size(), true, text, names, lens, &body, &lines, msg) == -1, "header: @SQ without SN passes");
    const std::string noln = "@SQ\tSN:x\tLN:abc\n";
    CHECK(samh_header((const uint8_t *)noln.data(), noln.size(), true, text, names, lens, &body, &lines, msg) == -1, "header: @SQ without a decimal LN passes");
    CHECK(samh_header((const uint8_t *)"", 0, true, text, names, lens, &body, &lines, msg) == 1 && text.empty() && names.empty() && body == 0, "header: an empty input");
    // the name table: prefixes, a duplicate, bytes above 127
    SamRefTable tab;
    tab.build({"chr10", "chr1", "chr", "chr1", "\xff" "x", "a"});
    const sam_refs R = tab.view();
    const char *q[] = {"chr10", "chr1", "chr", "\xff" "x", "a", "chr2", "ch", "chr100", ""};
    const int want[] = {0, 1, 2, 4, 5, -2, -2, -2, -2};
    for (int i = 0; i < 9; ++i) CHECK(sam_ref_find(R, (const uint8_t *)q[i], (uint32_t)strlen(q[i])) == want[i], "name table: '%s'", q[i]);
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
    for (Case &c : cases) ok = ok && rd_blob(f, c.name) && rd_blob(f, c.line) && rd_u32(f, c.ok) && rd_u32(f, c.slow) && rd_blob(f, c.rec);
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "%s is cut short\n", argv[1]); return 2; }
    SamRefTable tab;
    tab.build(refs);
    run(cases, tab.view());
    if (!g_fail) small_parts();
    if (g_fail) return 1;
    std::printf("sam_host_test OK: %zu cases\n", cases.size());
    return 0;
}
