/*
 * seqlib_amd_filter.h -- C-ABI of the MI355X-native read filter, part of libseqlib_amd.so: the rules of SeqLib::Filter::ReadFilterCollection evaluated on
 * block_size-prefixed BAM records that lie in HBM (slx_bam_batch.d_stream of seqlib_amd_bam.h), one keep byte per record, and -- attached to a reader --
 * every batch of slx_bam_next compacted to the kept records on the GPU.  Plain pointers and sizes, never throws; every function returns 0 or a negative
 * SLX_E* code (seqlib_amd.h), slx_last_error() gives the text.  include/SeqLib/ReadFilter.h is the header-only mirror of the reference classes.
 *
 * Reference interface each entry point replaces (paths relative to /root/reference; the reference hands records to htslib, which is not part of this
 * image, so parity is by restatement of the lines named here):
 *   slx_filter_create, slx_filter_free   ReadFilterCollection()                                        SeqLib/ReadFilter.h:493-500
 *   slx_filter_add_filter    ReadFilterCollection::AddReadFilter, ReadFilter::setRegions, SetExcluder, SetMateLinked   SeqLib/ReadFilter.h:398-484, src/ReadFilter.cpp:289-298
 *   slx_filter_add_rule      ReadFilter::AddRule of an AbstractRule (Range, FlagRule, read group, motifs, subsample)    SeqLib/ReadFilter.h:129-388, src/ReadFilter.cpp:138-140, 832-854
 *   slx_filter_apply_device  ReadFilterCollection::isValid over a batch in HBM                          src/ReadFilter.cpp:33-49, 77-136, 457-658
 *   slx_filter_attach        (new) the same inside slx_bam_next; no reference counterpart
 *   slx_filter_test_record   ReadFilterCollection::isValid(const BamRecord&), one record on the host     src/ReadFilter.cpp:96-136
 *   slx_filter_features      the BamRecord accessors the rules call: FullInsertSize, PairOrientation, NumClip, NumHardClip, MaxInsertionBases,
 *                            MaxDeletionBases, CountNBases, GetIntTag("NM"), ParseReadGroup              src/BamRecord.cpp:580-589, 861-874, 983-996, 1012-1028, 1139-1158, 1185-1213; SeqLib/BamRecord.h:264, 298, 408-415
 *   slx_filter_set, slx_filter_counter   (new) knobs and diagnostics
 *
 * The rules (src/ReadFilter.cpp:22-136, 457-658), quirks kept:
 *   collection  no filters: keep.  Otherwise every filter whose region test and whose rules pass makes the record valid, and an excluder among them
 *               excludes it; keep iff valid and not excluded.
 *   filter      no rules: pass; otherwise any rule.  Regions: none: pass; otherwise some region [p1, p2] (CLOSED, SeqLib/IntervalTree.h:198) on chr == tid
 *               with p2 >= pos and p1 <= end, end = pos + reference length of the CIGAR (pos + 1 when that is 0 or the record carries 0x4); a mate-linked
 *               filter also passes on (mtid, mpos, mpos + l_seq).  tid < 0 overlaps nothing.
 *   rule        subsample (X31 hash of the name, xor seed, Wang hash, low 24 bits against the fraction); isize on FullInsertSize; the read group (a record
 *               fails when ParseReadGroup() is not empty and differs); mapq; the flag rule (four masks, dup, supp AGAINST 0x100, qcfail, mapped, mate_mapped,
 *               hardclip only when n_cigar > 1, the orientation block); ins / del (both tested when either is set); motifs (fail when the rule has
 *               motifs and none occurs in the sequence over =ACMGRSVTWYHKDBN; a motif with another character, or an empty one, never matches; the
 *               inverted bit is stored and, as in the reference, not consulted); nm; nbases; len; clip.  A Range passes min <= v <= max, or its complement
 *               when inverted.
 *
 * Not carried: the JSON constructor, addGlobalRule and every parseJson (jsoncpp is third-party and not in the tree); the phred and xp ranges and the
 * fwd_strand / rev_strand / mate_*_strand / paired flags, which the reference stores and never evaluates; per-rule and per-filter pass counts.
 *
 * No CPU fallback: without a GPU slx_filter_apply_device and slx_bam_next on a reader with a filter attached return SLX_ENODEVICE.  Building a filter
 * needs no GPU, and slx_filter_test_record is the per-record body compiled for the host: what isValid(const BamRecord&) calls, not a path for batches.
 */
#ifndef SEQLIB_AMD_FILTER_H
#define SEQLIB_AMD_FILTER_H
#include <stdint.h>
#include <stddef.h>
#include "seqlib_amd.h"
#include "seqlib_amd_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slx_filter slx_filter;

typedef struct { int32_t min, max; uint8_t inverted, every; uint8_t pad[2]; } slx_filter_range;      /* every != 0: passes all values (Range()) */

/* the eight evaluated ranges, in this order in r[] */
enum { SLX_FR_ISIZE = 0, SLX_FR_MAPQ, SLX_FR_LEN, SLX_FR_CLIP, SLX_FR_NM, SLX_FR_NBASES, SLX_FR_INS, SLX_FR_DEL, SLX_FR_N };
/* the evaluated tri-state flags: two bits each in `tri` at 2 * index; 0 = NA, 1 = must be on, 2 = must be off */
enum { SLX_FT_DUP = 0, SLX_FT_SUPP, SLX_FT_QCFAIL, SLX_FT_HARDCLIP, SLX_FT_MAPPED, SLX_FT_MATE_MAPPED, SLX_FT_FF, SLX_FT_FR, SLX_FT_RF, SLX_FT_RR, SLX_FT_IC, SLX_FT_N };

typedef struct {
    slx_filter_range r[SLX_FR_N];
    uint32_t all_on, all_off, any_on, any_off;      /* FlagRule's four masks; 0 = unset */
    uint32_t tri;
    uint32_t subsample_seed;                         /* 999 in the reference */
    double   subsample_frac;                         /* >= 1: no subsampling */
    uint32_t motifs_inverted;                        /* stored, not consulted */
    uint32_t pad;
} slx_filter_rule;

/* what the rules read of one record (slx_filter_features) */
typedef struct {
    int32_t full_insert_size, pair_orientation, interchromosomal, pair_mapped;      /* orientation: 0 FR, 1 FF, 2 RF, 3 RR, 4 undefined (SeqLib/BamRecord.h) */
    int32_t num_clip, num_hard_clip, max_ins, max_del, n_bases_n, nm, has_nm;
    int32_t end;                                     /* PositionEnd as the region test takes it */
    char    read_group[256];                         /* ParseReadGroup, NUL-terminated (cut at 255 bytes) */
} slx_filter_feat;

int  slx_filter_create(slx_filter **f);
void slx_filter_free(slx_filter *f);                 /* detach it from every reader first */
/* a filter of the collection.  regs: n CLOSED intervals [beg, end] on tid (n = 0: the whole genome).  Returns the filter's id (>= 0) or SLX_E*. */
int  slx_filter_add_filter(slx_filter *f, int excluder, int mate_linked, const slx_bam_region *regs, int64_t n);
/* a rule of filter filter_id.  r NULL: a rule that passes every record.  read_group NULL or "": none.  motifs: n_motifs NUL-terminated strings. */
int  slx_filter_add_rule(slx_filter *f, int filter_id, const slx_filter_rule *r, const char *read_group, const char *const *motifs, int64_t n_motifs);
/* d_keep[i] = 1 when record i is kept, else 0: n_records bytes in HBM; *n_kept (may be NULL) their sum.  d_stream / d_rec_off as in slx_bam_batch.  The
 * first use compiles the rule table, the sorted regions and the motif automata and uploads them.  SLX_EIO: a record's fields pass its block_size, or an
 * aux field of unknown type (nothing beyond a record is read).  SLX_ENODEVICE without a GPU. */
int  slx_filter_apply_device(slx_filter *f, int device, const void *d_stream, const void *d_rec_off, int64_t n_records, void *d_keep, int64_t *n_kept);
/* after the call every batch of slx_bam_next on rd holds exactly the kept records, bytes unchanged, in file order -- for the whole file and for regions
 * (keep = region test AND filter).  n_records == 0 still means the end only.  f == NULL detaches: the reader is what it was. */
int  slx_filter_attach(slx_filter *f, slx_bam *rd);
/* host only: one block_size-prefixed record of n bytes.  1 = kept, 0 = dropped, SLX_EIO / SLX_EINVAL as above */
int  slx_filter_test_record(slx_filter *f, const uint8_t *rec, int64_t n);
/* host only, no filter needed: the features of one record */
int  slx_filter_features(const uint8_t *rec, int64_t n, slx_filter_feat *out);
/* "window_bytes" (16384; a multiple of 16, 64 ..), "overhang_bytes" (2048; a multiple of 16, 48 ..): the stage of k_flt_eval, their sum at most 49152;
 * "chunk_bases" (0 = the sequence split evenly over the 64 lanes; otherwise bases per lane-chunk of k_flt_eval_long's motif search) */
int  slx_filter_set(slx_filter *f, const char *key, int64_t value);
/* "seen", "passed" (records over the filter's life, test_record included), "us_filter" (kernel time from HIP events, microseconds, over its life),
 * "long_records" (records that went to k_flt_eval_long), "dfa_states", "dfa_in_lds" (0 | 1, of the last launch); -1 = unknown name */
int64_t slx_filter_counter(const slx_filter *f, const char *name);

#ifdef __cplusplus
}
#endif
#endif
