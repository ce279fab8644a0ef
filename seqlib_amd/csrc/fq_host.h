// fq_host.h -- the serial FASTA / FASTQ parser of the FASTQ reader's slow path (slx_fastq.hip): parse_record() of include/SeqLib/FastqReader.h restated over
// a chunk of text in memory.  Host only, no HIP, no library: tests/cpp/fastq_host_test.cpp drives it under ASan + UBSan.
//
// One call parses one record that starts at p (the place where parse_record() would skip junk to the next '>' or '@').  The chunk p[0, n) is either the rest
// of the input (final) or a prefix of it.  With a prefix, every read past the end of the chunk gives up with FQH_MORE instead of being taken as the end of the
// input: the caller comes back with a longer chunk from the same place, so every decision is taken on the bytes the streaming parser would have seen.
//   FQH_REC   a record; *consumed is where the next call starts (a header byte that ended a FASTA record is left for that call: parse_record's pending_)
//   FQH_MORE  the chunk ends inside the record (or inside the junk before it); *consumed = junk that may be dropped (never part of a record)
//   FQH_END   the input ends before another record (kseq's -1); *consumed = n
//   FQH_BAD   truncated or inconsistent quality (kseq's -2): the stream ends here
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

enum { FQH_REC = 1, FQH_MORE = 2, FQH_END = 3, FQH_BAD = 4 };

struct fqh_rec {
    std::string name, com, seq, qual;
    bool has_com = false, has_qual = false;          // the flag bits of slx_fastq_batch.d_flags
};

// isspace() of the C locale
static inline bool fqh_space(unsigned c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

struct fqh_cur {
    const uint8_t *p; size_t n, i; bool final, starved;
    // -1 at the end of the chunk; `starved` says that it was not the end of the input
    int get() { if (i < n) return p[i++]; if (!final) starved = true; return -1; }
};

// FastqReader::until_: appends up to the next delimiter (line: '\n', else any whitespace); the delimiter, 0 at the end after some byte, -1 at the end at once
static inline int fqh_until(fqh_cur &c, bool line, std::string &dst)
{
    bool any = false;
    int ch;
    while ((ch = c.get()) != -1) {
        any = true;
        if (line ? ch == '\n' : fqh_space((unsigned)ch)) break;
        dst.push_back((char)ch);
    }
    if (!any) return -1;
    if (line && dst.size() > 1 && dst.back() == '\r') dst.pop_back();
    return ch == -1 ? 0 : ch;
}

static inline int fqh_parse(const uint8_t *p, size_t n, bool final, fqh_rec &r, size_t *consumed)
{
    fqh_cur c{p, n, 0, final, false};
    int ch;
    while ((ch = c.get()) != -1 && ch != '>' && ch != '@') {}
    if (ch == -1) { *consumed = n; return final ? FQH_END : FQH_MORE; }
    const size_t head = c.i - 1;
    *consumed = head;
    r.name.clear(); r.com.clear(); r.seq.clear(); r.qual.clear();
    r.has_com = r.has_qual = false;
    const int d = fqh_until(c, false, r.name);
    if (c.starved) return FQH_MORE;
    if (d == -1) { *consumed = n; return FQH_END; }
    if (d != '\n' && fqh_until(c, true, r.com) != -1) r.has_com = true;
    if (c.starved) return FQH_MORE;
    size_t at = c.i;
    while ((ch = c.get()) != -1 && ch != '>' && ch != '+' && ch != '@') {
        if (ch != '\n') { r.seq.push_back((char)ch); fqh_until(c, true, r.seq); }
        at = c.i;
    }
    if (c.starved) return FQH_MORE;
    if (ch != '+') { *consumed = ch == -1 ? n : at; return FQH_REC; }          // FASTA: the next header byte stays
    r.has_qual = true;
    while ((ch = c.get()) != -1 && ch != '\n') {}
    if (c.starved) return FQH_MORE;
    if (ch == -1) { *consumed = n; return FQH_BAD; }
    while (fqh_until(c, true, r.qual) >= 0 && r.qual.size() < r.seq.size()) {}
    if (c.starved) return FQH_MORE;
    *consumed = c.i;
    return r.qual.size() == r.seq.size() ? FQH_REC : FQH_BAD;
}
