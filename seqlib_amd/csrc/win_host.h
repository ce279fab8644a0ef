// win_host.h -- the per-record body of the assembly-window collector (include/seqlib_amd_win.h): validate, select, trim.  Compiles for host and device, like
// edit_host.h and stats_host.h: k_win_measure and k_win_measure_long (slx_win.hip) run it a lane or a wave per record, slx_win_quality_trim and
// BamRecord::QualityTrimmedSequence run it on the CPU, tests/cpp/win_host_test.cpp runs it under ASan + UBSan (`lane` of `nlanes`, the host build runs lane 0 of 1).
// The rules are the header comment of include/seqlib_amd_win.h; DESIGN.md 9.14.
//
// Memory safety.  Nothing of record i is read before ed_span (dev_edit.h) has placed [off[i], off[i + 1]) inside the stream with 36 bytes at least; ed_fixed checks
// name, CIGAR, sequence and qualities against the span before any of them is read; the name's last byte is read at 36 + l_read_name - 1 < span; the trim reads
// qual[0, l_seq) only.
#pragma once
#include <stdint.h>
#include "dev_edit.h"

// what becomes of a record.  WN_KEEP: bases [k0, k0 + klen) of it are a read of every window it overlaps
enum { WN_KEEP = 0, WN_SKIP_FLAG = 1, WN_NO_SEQ = 2, WN_NO_NAME = 3, WN_TRIMMED = 4, WN_BROKEN = 5, WN_N_STATUS = 6 };
#define WN_WAVE_LEN 512u        // the default of "wave_len"
#define WN_MAX_TRIM 93

// the selection rules, a kernel argument: whole 32-bit words (dev_edit.h says why)
struct wn_rules {
    uint32_t skip_flags;
    int32_t qual_trim;          // -1: off
    uint32_t original_strand, wave_len;
};
// what the measure step leaves of a record
struct wn_rec {
    uint32_t status, seq_at, l_seq, k0, klen, flip;
};

// BamRecord::QualityTrimmedSequence (reference src/BamRecord.cpp:591-624) on qual[0, len): (0, -1) for no bases or qual[0] == 0xff -- the whole read;
// (len, -1) when no base reaches t; otherwise [first base >= t, one past the last base >= t).  WAVE: every lane of a wave with the same arguments, 64 bytes per
// ballot from both ends; all lanes return the same.
template <bool WAVE> ED_FN void wn_trim(const uint8_t *qual, int32_t len, int32_t t, int32_t *start, int32_t *end, int lane, int nlanes)
{
    *start = 0; *end = -1;
    if (len <= 0 || qual[0] == 0xff) return;
    int32_t first = len, last = -1;
    if (!WAVE) {
        for (int32_t i = 0; i < len; ++i) if ((int32_t)qual[i] >= t) { first = i; break; }
        if (first < len) for (int32_t i = len - 1; i >= 0; --i) if ((int32_t)qual[i] >= t) { last = i; break; }
    } else {
        for (int32_t base = 0; base < len; base += nlanes) {
            const int32_t p = base + lane;
            const uint64_t m = ED_BALLOT(p < len && (int32_t)qual[p < len ? p : 0] >= t);
            if (m) { first = base + (int32_t)ed_ctz64(m); break; }
        }
        if (first < len) for (int32_t hi = len; hi > 0; hi -= nlanes) {
            const int32_t p = hi - 1 - lane;
            const uint64_t m = ED_BALLOT(p >= 0 && (int32_t)qual[p >= 0 ? p : 0] >= t);
            if (m) { last = hi - 1 - (int32_t)ed_ctz64(m); break; }
        }
    }
    if (first >= len) { *start = len; return; }
    *start = first; *end = last + 1;
}

// The fixed part of a record of `span` bytes whose block_size fills it, and the selection: WN_BROKEN, a drop cause, or WN_KEEP with seq_at and l_seq (the trim
// is still to come).  Broken before anything else: fields that pass the span, or a name of one byte or more that does not end in NUL.
ED_FN uint32_t wn_select(const wn_rules &R, const uint8_t *rec, uint32_t span, wn_rec *M)
{
    uint32_t seq_at = 0, aux_at = 0;
    M->status = WN_BROKEN; M->seq_at = 0; M->l_seq = 0; M->k0 = 0; M->klen = 0; M->flip = 0;
    if (!ed_fixed(rec, span, &seq_at, &aux_at)) return WN_BROKEN;
    const uint32_t l_name = rec[12], flag = (uint32_t)rec[18] | (uint32_t)rec[19] << 8, l_seq = ed_ld32(rec + 20);
    if (l_name >= 1 && rec[36 + l_name - 1] != 0) return WN_BROKEN;
    M->seq_at = seq_at; M->l_seq = l_seq;
    M->flip = (R.original_strand && (flag & 0x10u)) ? 1u : 0u;
    if (flag & R.skip_flags) return M->status = WN_SKIP_FLAG;
    if (l_seq == 0) return M->status = WN_NO_SEQ;
    if (l_name <= 1) return M->status = WN_NO_NAME;
    return M->status = WN_KEEP;
}

// the trim of a selected record (status WN_KEEP): the kept stretch, or WN_TRIMMED.  WAVE as wn_trim; lane 0 writes.
template <bool WAVE> ED_FN uint32_t wn_keep(const wn_rules &R, const uint8_t *rec, wn_rec *M, int lane, int nlanes)
{
    const uint32_t seq_at = M->seq_at, l_seq = M->l_seq;
    uint32_t k0 = 0, klen = l_seq, status = WN_KEEP;
    if (R.qual_trim >= 0) {
        int32_t a, b;
        wn_trim<WAVE>(rec + seq_at + ((l_seq + 1) >> 1), (int32_t)l_seq, R.qual_trim, &a, &b, lane, nlanes);
        if (b < 0 && a != 0) { status = WN_TRIMMED; klen = 0; }
        else if (b >= 0) { k0 = (uint32_t)a; klen = (uint32_t)(b - a); }
    }
    if (!WAVE || lane == 0) { M->status = status; M->k0 = k0; M->klen = klen; }
    return status;
}

// the arena bytes of a kept stretch: every read starts on a 16-byte word, so that k_win_extract stores and k_win_gather loads whole aligned words
ED_FN uint64_t wn_padded(uint32_t klen) { return ((uint64_t)klen + 15u) & ~15ull; }

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
// A batch in host memory through the measure step, lane 0 of 1: true with one wn_rec per record, or false and in *bad the first broken record
static inline bool wn_measure_on_host(const wn_rules &R, const uint8_t *stream, uint64_t n_bytes, const uint64_t *off, uint64_t n, std::vector<wn_rec> *out, uint64_t *bad)
{
    out->assign(n, wn_rec{WN_BROKEN, 0, 0, 0, 0, 0});
    *bad = ED_NONE;
    if (n == 0 && n_bytes) { *bad = 0; return false; }
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t span = 0;
        bool own = false;
        if (!ed_span(stream, n_bytes, off, i, n, &span, &own)) { *bad = i; return false; }
        if (!own) continue;          // (record i + 1 is the one named)
        const uint8_t *rec = stream + (off[i] - off[0]);
        wn_rec *M = &(*out)[i];
        const uint32_t s = wn_select(R, rec, span, M);
        if (s == WN_BROKEN) { *bad = i; return false; }
        if (s == WN_KEEP) (void)wn_keep<false>(R, rec, M, 0, 1);
    }
    return true;
}
#endif
