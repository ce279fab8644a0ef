// fastq_host_test.cpp -- the host-compilable parts of the FASTQ reader (seqlib_amd/csrc/fq_host.h, dev_fastq.h) against the expectations that the Python
// statement of the grammar wrote (tests/fastq_util.py: dump_expectations).  Stand-alone: no library, no GPU; tests/test_fastq_host.py builds it with
// -fsanitize=address,undefined and runs it.
//   1. fqh_parse over each whole case (final): the records, and where the stream ends (end of input / damaged tail);
//   2. fqh_parse fed chunks cut at EVERY byte position of each small case: a prefix first (not final) until it asks for more, then the whole text from where
//      it stood -- the same records must come out;
//   3. fq_check, the fast path's per-record test, over the line table of the whole text and of every prefix: the records it accepts must be the expected
//      ones field by field, and on a strict 4-line case it must accept all of them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "fq_host.h"
#include "dev_fastq.h"

struct Rec { std::string name, com, seq, qual; uint32_t flag; };
struct Case { std::string name, text; uint32_t strict, bad; std::vector<Rec> recs; };

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

static bool same(const fqh_rec &r, const Rec &e)
{
    const std::string q = r.has_qual ? r.qual : std::string(r.seq.size(), '\0');
    const uint32_t flag = (r.has_com ? 1u : 0u) | (r.has_qual ? 2u : 0u);
    return r.name == e.name && r.com == e.com && r.seq == e.seq && q == e.qual && flag == e.flag;
}

// records of text from byte `from` on, appended to out; returns the status that ended the walk and where it stood
static int walk(const std::string &text, size_t len, bool final, size_t &pos, std::vector<fqh_rec> &out)
{
    const uint8_t *p = reinterpret_cast<const uint8_t *>(text.data());
    for (;;) {
        fqh_rec r;
        size_t used = 0;
        const int rc = fqh_parse(p + pos, len - pos, final, r, &used);
        pos += used;
        if (rc != FQH_REC) return rc;
        out.push_back(r);
    }
}

static void check_records(const Case &c, const std::vector<fqh_rec> &got, int rc, const char *what, size_t cut)
{
    CHECK(rc == (c.bad ? FQH_BAD : FQH_END), "%s (%s, cut %zu): the stream ended with status %d", c.name.c_str(), what, cut, rc);
    CHECK(got.size() == c.recs.size(), "%s (%s, cut %zu): %zu records, expected %zu", c.name.c_str(), what, cut, got.size(), c.recs.size());
    for (size_t i = 0; i < got.size(); ++i) CHECK(same(got[i], c.recs[i]), "%s (%s, cut %zu): record %zu differs", c.name.c_str(), what, cut, i);
}

static void line_table(const std::string &text, size_t n, bool eof, std::vector<uint64_t> &off)
{
    off.assign(1, 0);
    for (size_t i = 0; i < n; ++i) if (text[i] == '\n') off.push_back(i + 1);
    if (eof && n > 0 && text[n - 1] != '\n') off.push_back(n + 1);          // the end of the input counts as a line end
}

// the records fq_check accepts from the start of text[0, n)
static void check_fast(const Case &c, size_t n, bool eof)
{
    std::vector<uint64_t> off;
    line_table(c.text, n, eof, off);
    const uint64_t L = off.size() - 1;
    // an exact copy of the n bytes: a read behind them is a heap overflow that ASan reports
    std::vector<uint8_t> t(c.text.begin(), c.text.begin() + n);
    uint64_t k = 0;
    int s = FQ_NONE;
    for (; k <= L / 4; ++k) {
        fq_rec_out o;
        s = fq_check(t.data(), n, off.data(), L, eof, k, &o);
        if (s != FQ_OK) break;
        CHECK(k < c.recs.size(), "%s (n %zu): fq_check accepts record %llu, the file has %zu", c.name.c_str(), n, (unsigned long long)k, c.recs.size());
        const Rec &e = c.recs[k];
        const std::string text(t.begin(), t.end());
        CHECK(text.substr(o.name, o.len_name) == e.name && text.substr(o.com, o.len_com) == e.com && text.substr(o.seq, o.len_seq) == e.seq &&
              text.substr(o.qual, o.len_seq) == e.qual && o.flag == e.flag, "%s (n %zu): the fields fq_check gives for record %llu differ", c.name.c_str(), n, (unsigned long long)k);
    }
    CHECK(s != FQ_OK, "%s (n %zu): the last candidate was accepted", c.name.c_str(), n);
    if (eof && c.strict) CHECK(k == c.recs.size() && s == FQ_NONE, "%s: a strict file, but fq_check stops at record %llu of %zu with status %d", c.name.c_str(), (unsigned long long)k, c.recs.size(), s);
    if (eof) CHECK(s != FQ_MORE, "%s: FQ_MORE at the end of the input", c.name.c_str());
}

static void run_case(const Case &c)
{
    {
        std::vector<fqh_rec> got;
        size_t pos = 0;
        const int rc = walk(c.text, c.text.size(), true, pos, got);
        check_records(c, got, rc, "whole", 0);
        if (!c.bad) CHECK(pos == c.text.size(), "%s: %zu of %zu bytes consumed at the end", c.name.c_str(), pos, c.text.size());
    }
    check_fast(c, c.text.size(), true);
    if (c.text.size() > 800) return;
    for (size_t cut = 0; cut <= c.text.size(); ++cut) {
        std::vector<fqh_rec> got;
        size_t pos = 0;
        int rc = walk(c.text, cut, false, pos, got);
        CHECK(rc == FQH_MORE || rc == FQH_BAD, "%s (cut %zu): a prefix ended with status %d", c.name.c_str(), cut, rc);
        CHECK(pos <= cut, "%s (cut %zu): consumed %zu", c.name.c_str(), cut, pos);
        if (rc == FQH_MORE) rc = walk(c.text, c.text.size(), true, pos, got);
        check_records(c, got, rc, "prefix then rest", cut);
        check_fast(c, cut, false);
        if (g_fail) return;
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s expectations.bin\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t n_cases = 0;
    if (!rd_u32(f, n_cases)) return 2;
    size_t n_rec = 0;
    for (uint32_t i = 0; i < n_cases; ++i) {
        Case c;
        uint32_t nr = 0;
        if (!rd_blob(f, c.name) || !rd_blob(f, c.text) || !rd_u32(f, c.strict) || !rd_u32(f, c.bad) || !rd_u32(f, nr)) { std::fprintf(stderr, "short file\n"); return 2; }
        c.recs.resize(nr);
        for (Rec &r : c.recs)
            if (!rd_blob(f, r.name) || !rd_blob(f, r.com) || !rd_blob(f, r.seq) || !rd_blob(f, r.qual) || !rd_u32(f, r.flag)) { std::fprintf(stderr, "short file\n"); return 2; }
        run_case(c);
        n_rec += nr;
    }
    std::fclose(f);
    if (g_fail) { std::fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    std::printf("fastq_host_test OK: %u cases, %zu records\n", n_cases, n_rec);
    return 0;
}
