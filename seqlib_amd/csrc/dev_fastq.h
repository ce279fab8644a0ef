// dev_fastq.h -- the per-record test of the FASTQ reader's fast path (k_fq_check, slx_fastq.hip), host-compilable so that tests/cpp/fastq_host_test.cpp
// runs the very same code under ASan + UBSan before it runs on a GPU.
//
// The text is text[0, n); line i is text[line_off[i], line_off[i + 1] - 1), its line feed (or the end of the input, which counts as one) at
// line_off[i + 1] - 1; line_off has n_lines + 1 entries.  A batch begins at a record start, record k is TAKEN to be lines 4k .. 4k+3, and fq_check says
// whether kseq's loop (the grammar at the top of include/SeqLib/FastqReader.h) yields exactly these four fields:
//   FQ_OK    it does: *o holds where the fields lie and how long they are
//   FQ_FAIL  it does not, or this code cannot tell: the serial parser (fq_host.h) decides from this record on
//   FQ_MORE  the text ends before the record's four lines and the first byte behind them are known, and the input goes on
//   FQ_NONE  no byte is left at the record's place: the text is used up
// Memory safety: every byte read lies inside a line, every line inside [0, n) (line_off rises, its entries are at most n + 1 and the byte at
// line_off[i + 1] - 1 is never read as content); line_off itself is read at 4k .. 4k+4 only after 4k + 4 <= n_lines.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FQ_FN __host__ __device__ __forceinline__
#else
#define FQ_FN static inline
#endif

enum { FQ_OK = 0, FQ_FAIL = 1, FQ_MORE = 2, FQ_NONE = 3 };

struct fq_rec_out {
    uint64_t seq, qual, name, com;          // offsets of the fields in the text
    uint32_t len_seq, len_name, len_com;    // the quality has len_seq bytes
    uint32_t flag;                          // bit 0: the header went on after the name; bit 1: a '+' block was read
};

FQ_FN bool fq_space(uint32_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }          // isspace() of the C locale

// length of the line [a, b) after the CR rule: a trailing CR goes from a line longer than one byte
FQ_FN uint64_t fq_cr_len(const uint8_t *text, uint64_t a, uint64_t b) { return b - a > 1 && text[b - 1] == '\r' ? b - a - 1 : b - a; }

FQ_FN int fq_check(const uint8_t *text, uint64_t n, const uint64_t *line_off, uint64_t n_lines, bool eof, uint64_t k, fq_rec_out *o)
{
    const uint64_t l0 = 4 * k;
    if (l0 + 4 > n_lines) {
        const uint64_t at = line_off[l0 < n_lines ? l0 : n_lines];
        if (at >= n) return FQ_NONE;
        return eof ? FQ_FAIL : FQ_MORE;
    }
    const uint64_t a0 = line_off[l0], a1 = line_off[l0 + 1], a2 = line_off[l0 + 2], a3 = line_off[l0 + 3], a4 = line_off[l0 + 4];
    const uint64_t e0 = a1 - 1, e1 = a2 - 1, e2 = a3 - 1, e3 = a4 - 1;          // the ends of the four lines
    if (e0 == a0 || text[a0] != '@') return FQ_FAIL;
    if (e1 == a1) return FQ_FAIL;
    const uint8_t s0 = text[a1];
    if (s0 == '>' || s0 == '@' || s0 == '+') return FQ_FAIL;
    if (e2 == a2 || text[a2] != '+') return FQ_FAIL;
    if (e3 == a3) return FQ_FAIL;
    const uint64_t ls = fq_cr_len(text, a1, e1), lq = fq_cr_len(text, a3, e3);
    if (ls != lq || ls < 1 || ls > 0xffffffffull) return FQ_FAIL;
    if (a4 < n) { if (text[a4] != '@') return FQ_FAIL; }
    else if (!eof) return FQ_MORE;
    uint64_t d = a0 + 1;
    while (d < e0 && !fq_space(text[d])) ++d;
    o->name = a0 + 1; o->len_name = (uint32_t)(d - (a0 + 1));
    o->seq = a1; o->qual = a3; o->len_seq = (uint32_t)ls;
    o->flag = 2;
    o->com = d; o->len_com = 0;
    if (d < e0) {                                  // the name ended at a whitespace byte of the line, not at its line feed: the rest is the comment
        o->flag |= 1;
        o->com = d + 1;
        o->len_com = (uint32_t)fq_cr_len(text, d + 1, e0);
    }
    if (e0 - a0 > 0xffffffffull) return FQ_FAIL;
    return FQ_OK;
}
