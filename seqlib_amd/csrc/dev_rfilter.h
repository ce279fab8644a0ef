// dev_rfilter.h -- the per-record bodies of the read filter (k_flt_eval, k_flt_eval_long in slx_filter.hip; slx_filter_test_record on the host): the rules of
// SeqLib::Filter::ReadFilterCollection (src/ReadFilter.cpp:22-136, 457-658 of the reference, restated in include/seqlib_amd_filter.h) over one
// block_size-prefixed BAM record.  Host-compilable like dev_recsort.h and dev_rec.h (`lane` of `nlanes`; the host build runs lane 0 of 1) so that
// tests/cpp/filter_host_test.cpp can hold every body against a naive evaluator under ASan + UBSan before it runs on a GPU.
//
// Three steps per record:
//   features  the fixed fields, then only the walks the compiled rule set needs (T.need): the CIGAR (reference length, query length, clips, largest I and D),
//             the aux fields (NM, RG), the 4-bit sequence (N count; one DFA pass per motif set), the name (X31 hash).  Every one of them is written once, here,
//             and the BamRecord accessors of the C++ mirror go over the same functions (slx_filter_features).
//   evaluate  rf_eval: collection -> filters (regions by binary search, then rules) -> rule clauses, pure integer work on the features.
//   long      a record that does not fit the stage of k_flt_eval is taken by a whole wave: rf_long_part gives lane `lane` its share of the CIGAR ops, of the
//             sequence bytes and of the motif search (chunks of the sequence, each scanned from lmax - 1 bases before its start out of the root state: every
//             occurrence lies inside one extended chunk, so "does any motif occur" is exact); the shares are summed / maxed / or-ed (rf_part_join).
// Memory safety: rf_fixed checks block_size + 4 against the span the offset table gives and the name, CIGAR, sequence and qualities against block_size before
// anything variable is read; the aux walk checks every field against the record's end and stops at an unknown type.  Nothing outside [h, h + span) is read.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define RF_FN __device__ __forceinline__
#define RF_HD __host__ __device__ __forceinline__
#define RF_BLOCK_SYNC() __syncthreads()
#if defined(__HIP_DEVICE_COMPILE__)
#define RF_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#define RF_ATOMIC_OR(p, v) atomicOr((p), (v))
#else
#define RF_ATOMIC_ADD(p, v) (*(p) += (v), *(p) - (v))
#define RF_ATOMIC_OR(p, v) (*(p) |= (v))
#endif
#else
#define RF_FN static inline
#define RF_HD static inline
#define RF_BLOCK_SYNC() do { } while (0)
#define RF_ATOMIC_ADD(p, v) (*(p) += (v), *(p) - (v))
#define RF_ATOMIC_OR(p, v) (*(p) |= (v))
#endif

#define RF_NEED_CIGAR 1u
#define RF_NEED_AUX   2u
#define RF_NEED_NCOUNT 4u
#define RF_NEED_MOTIF 8u
#define RF_NEED_HASH  16u

#define RF_E_FIELDS 1u          // a record's fields pass its block_size, or the offset table does not hold a record there
#define RF_E_AUX    2u          // an aux field of unknown type, or one that passes the record's end

#define RF_MAX_DFA 64           // motif sets (rules with motifs) of one collection: a bit each in the hit mask
#define RF_ROOT_NONE 0xffffffffu

// orientation codes of SeqLib/BamRecord.h
#define RF_FR 0
#define RF_FF 1
#define RF_RF 2
#define RF_RR 3
#define RF_UD 4

// range indices and tri-state indices: the order of include/seqlib_amd_filter.h
enum { RF_R_ISIZE = 0, RF_R_MAPQ, RF_R_LEN, RF_R_CLIP, RF_R_NM, RF_R_NBASES, RF_R_INS, RF_R_DEL, RF_R_N };
enum { RF_T_DUP = 0, RF_T_SUPP, RF_T_QCFAIL, RF_T_HARDCLIP, RF_T_MAPPED, RF_T_MATE_MAPPED, RF_T_FF, RF_T_FR, RF_T_RF, RF_T_RR, RF_T_IC };

struct rf_rule {
    int32_t mn[RF_R_N], mx[RF_R_N];
    uint8_t inv[RF_R_N], every[RF_R_N];
    uint32_t all_on, all_off, any_on, any_off, tri;
    uint32_t sub_on, sub_thresh, seed;          // sub_on: frac < 1; the record fails when (hash & 0xffffff) >= sub_thresh
    uint32_t rg_off, rg_len;                    // the read group in T.strs; rg_len 0: none
    int32_t  motif_bit;                         // its motif set's bit in the hit mask; -1: no motifs
};
struct rf_filter { uint32_t rule0, n_rules, reg0, n_regs, excluder, mate; };
struct rf_reg { int32_t chr, p1, run_p2; };    // sorted by (chr, p1); run_p2: the largest p2 of the regions of chr up to and including this one
struct rf_tab {
    const rf_filter *flt; const rf_rule *rules; const rf_reg *regs; const uint8_t *strs; const uint32_t *dfa;
    uint32_t n_flt, need, n_dfa, pad;
    uint32_t root[RF_MAX_DFA], lmax[RF_MAX_DFA];          // per motif set: its root state in dfa, its longest motif
};

struct rf_feat {
    const uint8_t *name, *cig, *seq, *aux, *rg;
    uint64_t reflen, qlen, hits;                // hits: bit d = a motif of set d occurs
    uint32_t flag, mapq, n_cig, l_name, aux_len, rg_len, rg_na;
    uint32_t clip, hclip, max_ins, max_del, n_n, has_nm, hash;
    int32_t tid, pos, mtid, mpos, l_seq, nm;
};

// what a lane of a wave brings of a long record
struct rf_part { uint64_t reflen, qlen, hits; uint32_t clip, hclip, max_ins, max_del, n_n; };

RF_HD uint32_t rf_u32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
RF_HD uint32_t rf_u16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

// The fixed fields of the record at h whose offset-table span is `span` bytes; false when the span cannot hold a record, block_size + 4 is not the span, or the
// name, CIGAR, sequence and qualities pass block_size.
RF_HD bool rf_fixed(const uint8_t *h, uint64_t span, rf_feat *F)
{
    memset(F, 0, sizeof *F);
    if (span < 36 || span > 0xffffffffull + 4) return false;
    const uint64_t bs = rf_u32(h);
    if (bs + 4 != span) return false;
    F->tid = (int32_t)rf_u32(h + 4); F->pos = (int32_t)rf_u32(h + 8);
    F->l_name = h[12]; F->mapq = h[13];
    F->n_cig = rf_u16(h + 16); F->flag = rf_u16(h + 18);
    F->l_seq = (int32_t)rf_u32(h + 20);
    F->mtid = (int32_t)rf_u32(h + 24); F->mpos = (int32_t)rf_u32(h + 28);
    if (F->l_seq < 0) return false;
    const uint64_t ls = (uint64_t)F->l_seq, fixed = 32ull + F->l_name + 4ull * F->n_cig + ((ls + 1) >> 1) + ls;
    if (fixed > bs) return false;
    F->name = h + 36; F->cig = F->name + F->l_name; F->seq = F->cig + 4ull * F->n_cig; F->aux = F->seq + ((ls + 1) >> 1) + ls;
    F->aux_len = (uint32_t)(bs - fixed);
    return true;
}

// ops first, first + stride, ... of the CIGAR (src/BamRecord.cpp:1139-1158: NumClip, NumHardClip; :1012-1028: MaxInsertionBases, MaxDeletionBases; reference
// length M D N = X as bam_endpos; query length M I S = X as Cigar::NumQueryConsumed)
RF_HD void rf_cigar_part(const uint8_t *cig, uint32_t first, uint32_t n, uint32_t stride, rf_part *P)
{
    for (uint32_t i = first; i < n; i += stride) {
        const uint32_t w = rf_u32(cig + 4ull * i), op = w & 15u, len = w >> 4;
        if ((0x18du >> op) & 1u) P->reflen += len;          // M D N = X
        if ((0x193u >> op) & 1u) P->qlen += len;            // M I S = X
        if (op == 4 || op == 5) P->clip += len;
        if (op == 5) P->hclip += len;
        if (op == 1 && len > P->max_ins) P->max_ins = len;
        if (op == 2 && len > P->max_del) P->max_del = len;
    }
}

// code 15 among bases [2 * b0, min(2 * b1, l_seq)) : whole bytes b0 .. b1 of the packed sequence (src/BamRecord.cpp:580-589)
RF_HD uint32_t rf_ncount_part(const uint8_t *seq, uint64_t b0, uint64_t b1, uint64_t l_seq)
{
    uint32_t n = 0;
    for (uint64_t j = b0; j < b1; ++j) {
        const uint32_t v = seq[j];
        n += (v >> 4) == 15u;
        n += (2 * j + 1 < l_seq) && (v & 15u) == 15u;
    }
    return n;
}

// does a motif of the set with root `root` end in bases [from, to), scanning from `start` (<= from) out of the root state.  An entry of the dense table is
// next state << 1 | (the next state, or one on its failure chain, ends a motif).
RF_HD bool rf_dfa_scan(const uint32_t *dfa, uint32_t root, const uint8_t *seq, uint64_t start, uint64_t from, uint64_t to)
{
    uint32_t st = root;
    for (uint64_t i = start; i < to; ++i) {
        const uint32_t c = (seq[i >> 1] >> ((~i & 1u) << 2)) & 15u;
        const uint32_t e = dfa[(uint64_t)st * 16 + c];
        st = e >> 1;
        if ((e & 1u) && i >= from) return true;
    }
    return false;
}

// X31 of the name up to its NUL (khash's __ac_X31_hash_string) -- the subsample clause xors the seed in and runs Wang's hash over it (rf_wang)
RF_HD uint32_t rf_x31(const uint8_t *name, uint32_t l_name)
{
    if (l_name == 0 || name[0] == 0) return 0;
    uint32_t h = name[0];
    for (uint32_t i = 1; i < l_name && name[i]; ++i) h = (h << 5) - h + name[i];
    return h;
}
RF_HD uint32_t rf_wang(uint32_t k)
{
    k += ~(k << 15); k ^= (k >> 10); k += (k << 3); k ^= (k >> 6); k += ~(k << 11); k ^= (k >> 16);
    return k;
}

// The aux fields: NM of an integer type (src/BamRecord.cpp:861-874: the FIRST field named NM decides, of another type it counts as absent) and RG of type Z
// (ParseReadGroup, :983-996).  Returns 0 or RF_E_AUX; nothing at or beyond aux + n is read.
RF_HD uint32_t rf_aux(const uint8_t *aux, uint32_t n, rf_feat *F)
{
    uint32_t p = 0;
    bool seen_nm = false, seen_rg = false;
    while (p < n) {
        if (n - p < 3) return RF_E_AUX;
        const uint8_t t0 = aux[p], t1 = aux[p + 1], ty = aux[p + 2];
        const uint32_t v = p + 3;
        uint32_t sz;
        switch (ty) {
        case 'A': case 'c': case 'C': sz = 1; break;
        case 's': case 'S': sz = 2; break;
        case 'i': case 'I': case 'f': sz = 4; break;
        case 'd': sz = 8; break;
        case 'Z': case 'H': {
            uint32_t q = v;
            while (q < n && aux[q]) ++q;
            if (q >= n) return RF_E_AUX;
            sz = q - v + 1;
            break;
        }
        case 'B': {
            if (n - v < 5) return RF_E_AUX;
            const uint8_t sub = aux[v];
            uint32_t es;
            switch (sub) {
            case 'c': case 'C': es = 1; break;
            case 's': case 'S': es = 2; break;
            case 'i': case 'I': case 'f': es = 4; break;
            default: return RF_E_AUX;
            }
            const uint64_t bytes = 5ull + (uint64_t)es * rf_u32(aux + v + 1);
            if (bytes > n - v) return RF_E_AUX;
            sz = (uint32_t)bytes;
            break;
        }
        default: return RF_E_AUX;
        }
        if (sz > n - v) return RF_E_AUX;
        if (t0 == 'N' && t1 == 'M' && !seen_nm) {
            seen_nm = true;
            const uint8_t *q = aux + v;
            switch (ty) {
            case 'c': F->nm = (int8_t)q[0]; F->has_nm = 1; break;
            case 'C': F->nm = q[0]; F->has_nm = 1; break;
            case 's': F->nm = (int16_t)rf_u16(q); F->has_nm = 1; break;
            case 'S': F->nm = (int32_t)rf_u16(q); F->has_nm = 1; break;
            case 'i': case 'I': F->nm = (int32_t)rf_u32(q); F->has_nm = 1; break;
            default: break;
            }
        }
        if (t0 == 'R' && t1 == 'G' && !seen_rg) {
            seen_rg = true;
            if (ty == 'Z') { F->rg = aux + v; F->rg_len = sz - 1; F->rg_na = 0; }
        }
        p = v + sz;
    }
    return 0;
}

// ParseReadGroup without an RG:Z field: the name up to its first ':', else "NA"
RF_HD void rf_rg_from_name(rf_feat *F)
{
    if (F->rg) return;
    F->rg_na = 1; F->rg_len = 2;
    for (uint32_t i = 0; i < F->l_name && F->name[i]; ++i)
        if (F->name[i] == ':') { F->rg = F->name; F->rg_len = i; F->rg_na = 0; return; }
}

RF_HD void rf_take_part(rf_feat *F, const rf_part *P)
{
    F->reflen = P->reflen; F->qlen = P->qlen; F->hits = P->hits;
    F->clip = P->clip; F->hclip = P->hclip; F->max_ins = P->max_ins; F->max_del = P->max_del; F->n_n = P->n_n;
}
RF_HD void rf_part_join(rf_part *a, const rf_part *b)
{
    a->reflen += b->reflen; a->qlen += b->qlen; a->hits |= b->hits; a->clip += b->clip; a->hclip += b->hclip; a->n_n += b->n_n;
    if (b->max_ins > a->max_ins) a->max_ins = b->max_ins;
    if (b->max_del > a->max_del) a->max_del = b->max_del;
}

// lane `lane` of `nlanes`: its share of the CIGAR ops, of the packed sequence bytes, and of the motif search in chunks of chunk_bases (0: l_seq split evenly)
RF_HD void rf_long_part(const rf_tab *T, const rf_feat *F, uint32_t chunk_bases, uint32_t lane, uint32_t nlanes, rf_part *P)
{
    memset(P, 0, sizeof *P);
    const uint64_t ls = (uint64_t)F->l_seq;
    if (T->need & RF_NEED_CIGAR) rf_cigar_part(F->cig, lane, F->n_cig, nlanes, P);
    if (T->need & RF_NEED_NCOUNT) {
        const uint64_t nb = (ls + 1) >> 1, per = (nb + nlanes - 1) / nlanes, b0 = (uint64_t)lane * per < nb ? (uint64_t)lane * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
        P->n_n = rf_ncount_part(F->seq, b0, b1, ls);
    }
    if ((T->need & RF_NEED_MOTIF) && ls) {
        const uint64_t cb = chunk_bases ? chunk_bases : (ls + nlanes - 1) / nlanes;
        for (uint64_t c0 = (uint64_t)lane * cb; c0 < ls; c0 += (uint64_t)nlanes * cb) {
            const uint64_t c1 = c0 + cb < ls ? c0 + cb : ls;
            for (uint32_t d = 0; d < T->n_dfa; ++d) {
                if ((P->hits >> d) & 1ull) continue;
                const uint64_t back = T->lmax[d] ? T->lmax[d] - 1 : 0, start = c0 > back ? c0 - back : 0;
                if (rf_dfa_scan(T->dfa, T->root[d], F->seq, start, c0, c1)) P->hits |= 1ull << d;
            }
        }
    }
}

// what one lane does alone for a record (the short path, and the host): every needed walk.  Returns 0 or error bits; F is whole when 0.
RF_HD uint32_t rf_features(const uint8_t *h, uint64_t span, const rf_tab *T, rf_feat *F)
{
    if (!rf_fixed(h, span, F)) return RF_E_FIELDS;
    rf_part P;
    rf_long_part(T, F, 0, 0, 1, &P);
    rf_take_part(F, &P);
    if (T->need & RF_NEED_AUX) {
        const uint32_t e = rf_aux(F->aux, F->aux_len, F);
        if (e) return e;
        rf_rg_from_name(F);
    }
    if (T->need & RF_NEED_HASH) F->hash = rf_x31(F->name, F->l_name);
    return 0;
}

// ---------------------------------------------------------------- evaluation
RF_HD bool rf_pair_mapped(uint32_t flag) { return !(flag & 8u) && !(flag & 4u) && (flag & 1u); }          // SeqLib/BamRecord.h:298
RF_HD int32_t rf_full_isize(const rf_feat *F)                                                               // SeqLib/BamRecord.h:408-415
{
    if (F->tid != F->mtid || !rf_pair_mapped(F->flag)) return 0;
    const int64_t d = (int64_t)F->pos - (int64_t)F->mpos;
    return (int32_t)((d < 0 ? -d : d) + (int64_t)F->qlen);
}
RF_HD int rf_orientation(const rf_feat *F)                                                                  // src/BamRecord.cpp:1185-1213
{
    if ((F->flag & 4u) || (F->flag & 8u)) return RF_UD;
    const bool rev = (F->flag & 0x10u) != 0, mrev = (F->flag & 0x20u) != 0;
    const bool left_is_this = F->tid < F->mtid || (F->tid == F->mtid && F->pos <= F->mpos);
    const bool lrev = left_is_this ? rev : mrev, rrev = left_is_this ? mrev : rev;
    if (!lrev && rrev) return RF_FR;
    if (!lrev && !rrev) return RF_FF;
    if (lrev && rrev) return RF_RR;
    return RF_RF;
}
RF_HD int64_t rf_end(const rf_feat *F) { return (int64_t)F->pos + (int64_t)((F->flag & 4u) || F->reflen == 0 ? 1 : F->reflen); }

RF_HD bool rf_range(const rf_rule *R, int i, int32_t v)                                                     // SeqLib/ReadFilter.h:147-154
{
    if (R->every[i]) return true;
    return R->inv[i] ? (v < R->mn[i] || v > R->mx[i]) : (v >= R->mn[i] && v <= R->mx[i]);
}
// a tri-state against a bit of the record: fails when (off and set) or (on and not set)
RF_HD bool rf_tri_fails(uint32_t tri, int i, bool set) { const uint32_t t = (tri >> (2 * i)) & 3u; return (t == 2 && set) || (t == 1 && !set); }

RF_HD bool rf_flag_rule(const rf_rule *R, const rf_feat *F)                                                 // src/ReadFilter.cpp:565-658
{
    const uint32_t fl = F->flag, tri = R->tri;
    if (R->all_on && (fl & R->all_on) != R->all_on) return false;
    if (R->all_off && (fl & R->all_off) == R->all_off) return false;
    if (R->any_on && !(fl & R->any_on)) return false;
    if (R->any_off && (fl & R->any_off)) return false;
    if (rf_tri_fails(tri, RF_T_DUP, (fl & 0x400u) != 0)) return false;
    if (rf_tri_fails(tri, RF_T_SUPP, (fl & 0x100u) != 0)) return false;          // SecondaryFlag, as the reference tests it
    if (rf_tri_fails(tri, RF_T_QCFAIL, (fl & 0x200u) != 0)) return false;
    if (rf_tri_fails(tri, RF_T_MAPPED, !(fl & 4u))) return false;
    if (rf_tri_fails(tri, RF_T_MATE_MAPPED, !(fl & 8u))) return false;
    if (((tri >> (2 * RF_T_HARDCLIP)) & 3u) && F->n_cig > 1 && rf_tri_fails(tri, RF_T_HARDCLIP, F->hclip > 0)) return false;
    const bool ocheck = ((tri >> (2 * RF_T_FF)) & 0x3ffu) != 0;                   // ff fr rf rr ic
    if (!ocheck) return true;
    if (!rf_pair_mapped(fl)) return false;
    const bool bic = F->tid != F->mtid;                                           // Interchromosomal: pair-mapped holds here
    if (!bic) {
        const int po = rf_orientation(F);
        if (rf_tri_fails(tri, RF_T_FR, po == RF_FR)) return false;
        if (rf_tri_fails(tri, RF_T_RR, po == RF_RR)) return false;
        if (rf_tri_fails(tri, RF_T_RF, po == RF_RF)) return false;
        if (rf_tri_fails(tri, RF_T_FF, po == RF_FF)) return false;
    }
    return !rf_tri_fails(tri, RF_T_IC, bic);
}

RF_HD bool rf_rule_valid(const rf_tab *T, const rf_rule *R, const rf_feat *F)                               // src/ReadFilter.cpp:457-563
{
    if (R->sub_on && (rf_wang(F->hash ^ R->seed) & 0xffffffu) >= R->sub_thresh) return false;
    if (!rf_range(R, RF_R_ISIZE, rf_full_isize(F))) return false;
    if (R->rg_len) {
        const uint8_t *want = T->strs + R->rg_off;
        bool same = F->rg_len == R->rg_len;
        if (F->rg_na) same = same && want[0] == 'N' && want[1] == 'A';
        else for (uint32_t i = 0; same && i < R->rg_len; ++i) same = F->rg[i] == want[i];
        if (F->rg_len && !same) return false;                                      // an empty read group passes, as in the reference
    }
    if (!rf_range(R, RF_R_MAPQ, (int32_t)F->mapq)) return false;
    if (!rf_flag_rule(R, F)) return false;
    if (!R->every[RF_R_INS] || !R->every[RF_R_DEL]) {
        if (!rf_range(R, RF_R_INS, (int32_t)F->max_ins)) return false;
        if (!rf_range(R, RF_R_DEL, (int32_t)F->max_del)) return false;
    }
    if (R->motif_bit >= 0 && !((F->hits >> R->motif_bit) & 1ull)) return false;
    if (!rf_range(R, RF_R_NM, F->has_nm ? F->nm : 0)) return false;
    if (!rf_range(R, RF_R_NBASES, (int32_t)F->n_n)) return false;
    if (!rf_range(R, RF_R_LEN, F->l_seq)) return false;
    return rf_range(R, RF_R_CLIP, (int32_t)F->clip);
}

// some region [p1, p2] of the filter on chr with p2 >= pos and p1 <= end (SeqLib/IntervalTree.h:198): the last region with (chr, p1) <= (chr, end) by binary
// search; its running maximum of p2 answers for all before it on the chromosome
RF_HD bool rf_regions_hit(const rf_reg *g, uint32_t n, int32_t chr, int64_t pos, int64_t end)
{
    if (chr < 0) return false;
    uint32_t lo = 0, hi = n;          // the first region after (chr, end)
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (g[mid].chr < chr || (g[mid].chr == chr && (int64_t)g[mid].p1 <= end)) lo = mid + 1; else hi = mid;
    }
    return lo > 0 && g[lo - 1].chr == chr && (int64_t)g[lo - 1].run_p2 >= pos;
}

RF_HD bool rf_eval(const rf_tab *T, const rf_feat *F)                                                       // src/ReadFilter.cpp:33-49, 77-136
{
    if (T->n_flt == 0) return true;
    bool valid = false, excluded = false;
    for (uint32_t i = 0; i < T->n_flt; ++i) {
        const rf_filter *f = T->flt + i;
        if (f->n_regs) {
            bool in = rf_regions_hit(T->regs + f->reg0, f->n_regs, F->tid, F->pos, rf_end(F));
            if (!in && f->mate) in = rf_regions_hit(T->regs + f->reg0, f->n_regs, F->mtid, F->mpos, (int64_t)F->mpos + F->l_seq);
            if (!in) continue;
        }
        bool pass = f->n_rules == 0;
        for (uint32_t r = 0; !pass && r < f->n_rules; ++r) pass = rf_rule_valid(T, T->rules + f->rule0 + r, F);
        if (pass) { valid = true; if (f->excluder) excluded = true; }
    }
    return valid && !excluded;
}

// the end of the long path, one lane: the joined shares, then the aux fields, the read group and the name hash, then the verdict.  *er: 0 or error bits
RF_HD bool rf_long_finish(const rf_tab *T, rf_feat *F, const rf_part *P, uint32_t *er)
{
    rf_take_part(F, P);
    *er = 0;
    if (T->need & RF_NEED_AUX) {
        *er = rf_aux(F->aux, F->aux_len, F);
        if (*er) return false;
        rf_rg_from_name(F);
    }
    if (T->need & RF_NEED_HASH) F->hash = rf_x31(F->name, F->l_name);
    return rf_eval(T, F);
}

// ---------------------------------------------------------------- the window of k_flt_eval
// the first of the n offsets that is >= x
RF_HD uint64_t rf_lower(const uint64_t *off, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (off[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}

#if defined(__HIPCC__)
typedef uint32_t rf_v4 __attribute__((ext_vector_type(4)));
#endif

// Window `win` of the stream: the records that START in [win * W, win * W + W) are this block's.  The window and V bytes behind it (cut to the stream) are
// staged in lds -- W + V + 16 bytes, 16-byte aligned -- at the source's own alignment: the aligned 16-byte words that lie wholly inside the range as words,
// the up to 15 bytes before the first and after the last byte by byte, so nothing outside the stream is loaded.  Then thread `tid` of `nthreads` evaluates
// records first + tid, first + tid + nthreads, ... out of lds; one that ends behind the stage goes to the long list.  Returns this thread's kept records.
RF_FN uint32_t rf_window(const uint8_t *s, uint64_t n_bytes, const uint64_t *rec_off, uint64_t n_rec, uint64_t win, uint32_t W, uint32_t V, uint8_t *lds, const rf_tab *T,
                         uint8_t *keep, uint32_t *long_list, uint32_t *n_long, uint32_t *err, uint32_t tid, uint32_t nthreads)
{
    const uint64_t w0 = win * W;
    if (w0 >= n_bytes || n_rec == 0) return 0;
    const uint64_t w1 = w0 + W < n_bytes ? w0 + W : n_bytes, e = w1 + V < n_bytes ? w1 + V : n_bytes;
    const uint64_t first = rf_lower(rec_off, n_rec, w0), last = rf_lower(rec_off, n_rec, w1);
    if (first >= last) return 0;
    const uint8_t *g = s + w0;
    const uint32_t len = (uint32_t)(e - w0), lead = (uint32_t)((uintptr_t)g & 15u);
    uint32_t head = (16u - lead) & 15u;
    if (head > len) head = len;
    const uint32_t nw = (len - head) >> 4, tail0 = head + (nw << 4);
    for (uint32_t i = tid; i < head; i += nthreads) lds[lead + i] = g[i];
    for (uint32_t i = tid; i < nw; i += nthreads) {
        const uint32_t o = head + (i << 4);
#if defined(__HIPCC__)
        *reinterpret_cast<rf_v4 *>(lds + lead + o) = *reinterpret_cast<const rf_v4 *>(g + o);
#else
        memcpy(lds + lead + o, g + o, 16);
#endif
    }
    for (uint32_t i = tail0 + tid; i < len; i += nthreads) lds[lead + i] = g[i];
    RF_BLOCK_SYNC();
    uint32_t kept = 0;
    for (uint64_t r = first + tid; r < last; r += nthreads) {
        const uint64_t a = rec_off[r], b = rec_off[r + 1];
        if (a < w0 || a >= w1 || b <= a || b > n_bytes || b - a < 36) { RF_ATOMIC_OR(err, RF_E_FIELDS); keep[r] = 0; continue; }
        if (b > e) { long_list[RF_ATOMIC_ADD(n_long, 1u)] = (uint32_t)r; continue; }
        rf_feat F;
        const uint32_t er = rf_features(lds + lead + (uint32_t)(a - w0), b - a, T, &F);
        if (er) { RF_ATOMIC_OR(err, er); keep[r] = 0; continue; }
        const bool k = rf_eval(T, &F);
        keep[r] = k ? 1 : 0;
        kept += k;
    }
    return kept;
}
