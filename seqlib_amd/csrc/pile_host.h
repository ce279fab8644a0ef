// pile_host.h -- what the pileup unit (include/seqlib_amd_pile.h) computes per record and per position, compilable for host and device like cov_host.h
// (`lane` of `nlanes` lanes call together; W is dev_lanes.h's lanes_one or lanes_group): the eligibility test, the walk of one record that gives its (plane, position) events, and the candidate-site rule
// of one position.  dev_pile.h's kernels (a group of lanes per record, a wave per long record), slx_pile_record_events and tests/cpp/pile_host_test.cpp (under
// ASan + UBSan, with 1, 16 and 64 simulated lanes) all go over these bodies.  The fixed fields are the read filter's (dev_rfilter.h: rf_fixed).
// Memory safety: rf_fixed has placed the name, the CIGAR, the packed sequence and the l_seq quality bytes inside the record before pile_record reads any of
// them; the walk reads the sequence and the qualities at y < l_seq only.  The sink is called for positions inside [P.beg, P.end) only.
#pragma once
#include <stdint.h>
#include "dev_lanes.h"
#include "dev_rfilter.h"

#define PILE_PLANES 15
#define PILE_N 4
#define PILE_DEL 5
#define PILE_INS 6
#define PILE_REV 7
#define PILE_LOWQ 14

#define PILE_R_BAD (-1)         // the record's fields pass its block_size, or its extent is not block_size + 4
#define PILE_R_SKIP 0           // not eligible: contributes nothing
#define PILE_R_COUNTED 1
#define PILE_R_LONG 2           // eligible, with more than long_cigar ops or more than long_read bases: the wave's

// the window [beg, end) of contig tid and the knobs a record is judged by
struct pile_par { int64_t beg, end; int32_t tid, min_mapq, min_baseq; uint32_t exclude_flags, long_cigar, long_read; };

// planes of `stride` entries each, one behind the other
RF_HD uint64_t pile_stride(int64_t L) { return ((uint64_t)L + 3u) & ~3ull; }

// the fixed fields and the verdict; F is the filter's feature block
RF_HD int pile_head(const uint8_t *h, uint64_t span, const pile_par &P, rf_feat *F)
{
    if (!rf_fixed(h, span, F)) return PILE_R_BAD;
    if (F->tid != P.tid || F->pos < 0 || (F->flag & P.exclude_flags) || (int32_t)F->mapq < P.min_mapq || F->n_cig == 0 || F->l_seq == 0) return PILE_R_SKIP;
    return F->n_cig > P.long_cigar || (uint32_t)F->l_seq > P.long_read ? PILE_R_LONG : PILE_R_COUNTED;
}

// the plane offset of a 4-bit base code: 1 A, 2 C, 4 G, 8 T, everything else N
RF_HD uint32_t pile_base(uint32_t code) { return code == 1u ? 0u : code == 2u ? 1u : code == 4u ? 2u : code == 8u ? 3u : (uint32_t)PILE_N; }

// The events of an eligible record (pile_head said COUNTED or LONG; n_cig > 0 and l_seq > 0), by `nlanes` lanes that call together.  The ops are taken nlanes at
// a time: lane `lane` reads op base + lane, W.scan gives every op its start on the reference and in the read from the lengths of the ops before it, then the
// ops of the chunk are walked one after the other, W.bcast handing an op and its starts to all lanes, and lane `lane` takes bases lane, lane + nlanes, ... of
// an M or D block: neighbouring lanes read neighbouring bases and add to neighbouring positions.  The trip counts of every loop that holds a scan or a bcast
// are the same for all lanes of the group.  nlanes == 1 with lanes_one is the plain walk.  S(plane, x) is called for P.beg <= x < P.end only.
template <class Wave, class Sink> RF_HD void pile_record(const rf_feat &F, const pile_par &P, uint32_t lane, uint32_t nlanes, const Wave &W, Sink &S)
{
    const uint64_t ls = (uint64_t)F.l_seq;
    const uint8_t *seq = F.seq, *qual = F.seq + ((ls + 1) >> 1);
    const bool has_q = qual[0] != 0xffu;
    const uint32_t sb = (F.flag & 0x10u) ? (uint32_t)PILE_REV : 0u;
    int64_t x = F.pos;
    uint64_t y = 0;
    for (uint32_t base = 0; base < F.n_cig; base += nlanes) {
        const uint32_t i = base + lane;
        const uint32_t w = i < F.n_cig ? rf_u32(F.cig + 4ull * i) : 0u;
        uint64_t rt = 0, qt = 0;
        const uint64_t xb = W.scan(((0x18du >> (w & 15u)) & 1u) ? (uint64_t)(w >> 4) : 0ull, &rt);          // M D N = X
        const uint64_t yb = W.scan(((0x193u >> (w & 15u)) & 1u) ? (uint64_t)(w >> 4) : 0ull, &qt);          // M I S = X
        const uint32_t cnt = F.n_cig - base < nlanes ? F.n_cig - base : nlanes;
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t wj = (uint32_t)W.bcast(w, j), op = wj & 15u;
            const int64_t len = (int64_t)(wj >> 4), xs = x + (int64_t)W.bcast(xb, j);
            const uint64_t ys = y + W.bcast(yb, j);
            if ((0x181u >> op) & 1u) {                                        // M = X
                const bool stop = len > 0 && ys + (uint64_t)len > ls;          // a base with y >= l_seq is met: the whole walk ends there
                const int64_t n = !stop ? len : ys < ls ? (int64_t)(ls - ys) : 0;
                int64_t b0 = P.beg > xs ? P.beg - xs : 0, b1 = P.end - xs < n ? P.end - xs : n;
                for (int64_t b = b0 + lane; b < b1; b += nlanes) {
                    const uint64_t yy = ys + (uint64_t)b;
                    const uint32_t code = (seq[yy >> 1] >> ((~yy & 1u) << 2)) & 15u;
                    const bool pass = !has_q || (int32_t)qual[yy] >= P.min_baseq;
                    S(pass ? sb + pile_base(code) : (uint32_t)PILE_LOWQ, xs + b);
                }
                if (stop) return;
            } else if (op == 2u) {                                            // D
                int64_t b0 = P.beg > xs ? P.beg - xs : 0, b1 = P.end - xs < len ? P.end - xs : len;
                for (int64_t b = b0 + lane; b < b1; b += nlanes) S(sb + (uint32_t)PILE_DEL, xs + b);
            } else if (op == 1u) {                                            // I: the anchor is the base in front of it
                if (lane == 0 && xs - 1 >= P.beg && xs - 1 < P.end) S(sb + (uint32_t)PILE_INS, xs - 1);
            }
        }
        x += (int64_t)rt; y += qt;
    }
}

// ---- candidate sites: one position's 15 counts c[] and its reference byte
struct pile_site_par { int32_t min_depth, min_alt, frac_num, frac_den; };
struct pile_site_val { int32_t ref, depth, alt, ins; };
RF_HD bool pile_qualifies(int64_t c, int64_t depth, const pile_site_par &Q) { return c >= Q.min_alt && c * Q.frac_den >= (int64_t)Q.frac_num * depth; }
RF_HD bool pile_site(const int32_t *c, uint32_t ref_byte, const pile_site_par &Q, pile_site_val *V)
{
    int64_t depth = 0;
    for (int k = 0; k <= PILE_DEL; ++k) depth += (int64_t)c[k] + (int64_t)c[PILE_REV + k];
    const uint32_t u = ref_byte >= 'a' && ref_byte <= 'z' ? ref_byte - 32u : ref_byte;
    // (no index computed from the byte: on the GPU the counts are registers)
    const int64_t of_ref = u == 'A' ? (int64_t)c[0] + c[PILE_REV] : u == 'C' ? (int64_t)c[1] + c[PILE_REV + 1] : u == 'G' ? (int64_t)c[2] + c[PILE_REV + 2] : u == 'T' ? (int64_t)c[3] + c[PILE_REV + 3] : depth;
    const int64_t alt = depth - of_ref;
    const int64_t ins = (int64_t)c[PILE_INS] + (int64_t)c[PILE_REV + PILE_INS];
    V->ref = (int32_t)u; V->depth = (int32_t)depth; V->alt = (int32_t)alt; V->ins = (int32_t)ins;
    return depth >= Q.min_depth && (pile_qualifies(alt, depth, Q) || pile_qualifies(ins, depth, Q));
}
