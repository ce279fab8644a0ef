/*
 * seqlib_amd_pile.h -- C-ABI of the MI355X-native per-base pileup, part of libseqlib_amd.so: block_size-prefixed BAM records that lie in HBM (slx_bam_batch,
 * slx_rec_batch, a sorter's output: d_stream with d_rec_off) are turned there into a per-position table of allele counts over one window of one contig, and the
 * table is read back as planes, as the 15 counts of one position, or as the compacted list of the positions where the reads disagree with a reference that lies
 * in HBM too (slx_ref, seqlib_amd_ref.h).  Plain pointers and sizes, never throws; every function returns 0 or a negative SLX_E* code (seqlib_amd.h),
 * slx_last_error() gives the text.  SeqLib::Pileup (include/SeqLib/Pileup.h) is the header-only caller.  There is no reference counterpart: the reference
 * library leaves the table to its user (Next() + GetCigar() + Sequence() + Qualities()).
 *
 * The rules.
 *   object     one window [beg, end) of one contig, clipped to the contig; L = end - beg.  A whole contig is the window [0, len); there is no all-contigs object.
 *              Storage is SLX_PILE_PLANES = 15 planes of int32, each of L entries rounded up to 4 (the stride), plane-major: the count of plane p at position
 *              pos is entry p * stride + (pos - beg).  60 bytes per reference base: 14.9 GB of HBM for chr1 of GRCh38; SLX_ENOMEM when it does not fit.
 *   planes     for strand s (0 forward, 1 when flag 0x10 is set): 7 * s + {0 A, 1 C, 2 G, 3 T, 4 N, 5 DEL, 6 INS}; plane 14, LOWQ, counts both strands.
 *   eligible   tid is the window's tid, pos >= 0, (flag & exclude_flags) == 0, mapq >= min_mapq, n_cigar > 0, l_seq > 0.  Defaults: exclude_flags 0x704,
 *              min_mapq 0.
 *   qualities  a record whose first quality byte is 0xff has none ("0xff then zeros", seqlib_amd_rec.h: what alignToBam and the host builder write): the
 *              base-quality test is then not applied and every base passes.  Otherwise the base at y passes when qual[y] >= min_baseq (default 0).
 *   walk       x = pos, y = 0, then op by op:
 *                M, =, X   per base: the whole walk stops when y has reached l_seq (the answer seqlib_amd_ref.h gives for NM and MD).  The 4-bit code at y maps
 *                          1 -> A, 2 -> C, 4 -> G, 8 -> T and every other code, 0 included, to N.  A passing base adds 1 to plane 7 * s + base at x, a failing
 *                          one adds 1 to LOWQ at x.  Then x += 1, y += 1.
 *                D         1 to plane 7 * s + DEL at each of the len positions from x, with no quality test; x += len.
 *                I         1 to plane 7 * s + INS at the anchor x - 1 (pos - 1 for a leading insertion: clipping then drops it at a window's or the contig's
 *                          start); y += len.
 *                S         y += len.        N   x += len.        H, P and the op codes 9..15: nothing.
 *   clipping   an event outside [beg, end) is dropped silently.
 *   counts     int32, no saturation.  Integer adds commute: the result is bit-identical whatever the order of records, batches, kernels and knobs.
 *   failure    a record whose fields pass its block_size (or whose extent in the offsets is not block_size + 4 inside the stream) fails the call with SLX_EIO;
 *              slx_last_error names the lowest such index of the batch; nothing beyond a record is read.  The object then holds the contributions of an
 *              unspecified part of that batch: slx_pile_clear it.  This is the coverage unit's contract (seqlib_amd_cov.h).
 *   regions    a reader with SetRegions serves a record once per region it overlaps; such a record is counted once per time it is served.
 *   sites      per position: depth = A + C + G + T + N + DEL over both strands (LOWQ and INS are not in it); r = the reference byte, case-insensitive, A C G T
 *              -> 0..3, anything else -> none; alt = depth - (the count of r on both strands), 0 when r is none; ins = INS on both strands.  A count c
 *              qualifies when c >= min_alt and (int64)c * frac_den >= (int64)frac_num * depth.  A position is a site when depth >= min_depth and alt or ins
 *              qualifies.  Integer arithmetic throughout.
 *
 * No CPU fallback for batches: without a GPU slx_pile_create succeeds with device = -1 (for slx_pile_free and the host-only slx_pile_record_events) and every
 * other entry returns SLX_ENODEVICE (slx_pile_set after it has checked its arguments; slx_pile_counter returns counts, 0 on such an object).  Not carried:
 * base-alignment quality, overlap-aware counting of mates, per-base quality sums, the inserted sequences themselves, genotype likelihoods or VCF, an
 * all-contigs object, several GPUs, CRAM, the CG:B long-CIGAR form.
 */
#ifndef SEQLIB_AMD_PILE_H
#define SEQLIB_AMD_PILE_H
#include <stdint.h>
#include <stddef.h>
#include "seqlib_amd.h"
#include "seqlib_amd_bam.h"
#include "seqlib_amd_ref.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slx_pile slx_pile;

#define SLX_PILE_PLANES 15
#define SLX_PILE_A 0
#define SLX_PILE_C 1
#define SLX_PILE_G 2
#define SLX_PILE_T 3
#define SLX_PILE_N 4
#define SLX_PILE_DEL 5
#define SLX_PILE_INS 6
#define SLX_PILE_REV 7          /* added to the seven above for a record with flag 0x10 */
#define SLX_PILE_LOWQ 14

/* one candidate site; ref is the reference byte in upper case, plane[] the position's 15 counts */
typedef struct {
    int64_t pos;
    int32_t ref, depth, alt, ins;
    int32_t plane[SLX_PILE_PLANES];
    int32_t pad;
} slx_pile_site;

/* n_ref contigs of ref_len[i] bases (0 .. 2^31 - 1) named ref_names[i] (NULL: no names, the TSV then prints the tid).  window is mandatory (SLX_EINVAL for NULL,
 * for a tid outside [0, n_ref) and for beg > end): [window->beg, window->end) of contig window->tid is kept, clipped to the contig; records elsewhere contribute
 * nothing.  device < 0: the current one, or with no GPU at all a host-only object.  SLX_ENOMEM when the planes do not fit in HBM. */
int slx_pile_create(int device, int n_ref, const int64_t *ref_len, const char *const *ref_names, const slx_bam_region *window, slx_pile **out);
void slx_pile_free(slx_pile *p);

/* Result knobs: "min_mapq" (0; 0 .. 255), "min_baseq" (0; 0 .. 255), "exclude_flags" (0x704; 0 .. 0xffff).  Layout knobs, which never change a result:
 * "long_cigar" (64; 0 .. 2^20) and "long_read" (1024; 0 .. 2^31 - 1): records with more ops or more bases are taken by a whole wave; "lds_window" (0 .. 1024
 * positions; the default is the measured one, profiles/NOTES_pile.md): 0 is the plain form with global atomics only; "slice_records" (1024; 64 .. 2^20):
 * records per block; "group_lanes" (16, 32 or 64): the lanes that walk one record together.  SLX_EINVAL for an unknown key or a value outside its range. */
int slx_pile_set(slx_pile *p, const char *key, int64_t value);

/* n_records records in n_bytes of HBM on the object's device, d_rec_off their n_records + 1 uint64 offsets.  The caller's buffers are free again on return. */
int slx_pile_add_device(slx_pile *p, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records);
/* The same for records in host memory: they are uploaded and take the same kernels. */
int slx_pile_add_host(slx_pile *p, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records);
/* Host only, no GPU: the events (plane, position) the record rec[0, n) contributes to a window [clip_beg, clip_end), through the body the kernels compile, in
 * the walk's order; flags and mapq are not looked at, pos < 0, n_cigar == 0 or l_seq == 0 gives none.  *n_out events; SLX_EINVAL when cap is too small (the
 * first cap are written), SLX_EIO for a record as above. */
int slx_pile_record_events(const uint8_t *rec, int64_t n, int min_baseq, int64_t clip_beg, int64_t clip_end, int32_t *plane, int64_t *pos, int64_t cap, int64_t *n_out);

/* out[0, end - beg) = the counts of one plane at positions [beg, end); 0 outside the window */
int slx_pile_counts(slx_pile *p, int plane, int64_t beg, int64_t end, int32_t *out);
/* the plane in HBM: *n = L int32 from the window's first position, valid until the object is freed */
int slx_pile_counts_device(slx_pile *p, int plane, const void **d_counts, int64_t *n);
/* the 15 counts of one position; all 0 outside the window */
int slx_pile_at(slx_pile *p, int64_t pos, int32_t out[SLX_PILE_PLANES]);

/* The candidate sites of the window against contig ref_tid of ref (which must have the length given for the window's contig at create: SLX_EINVAL otherwise), by
 * the rule above; min_depth >= 1, min_alt >= 1, 0 <= frac_num <= frac_den, frac_den >= 1 (SLX_EINVAL otherwise).  *n_sites of them, in ascending position, stay
 * in HBM until the next call on the handle. */
int slx_pile_sites(slx_pile *p, slx_ref *ref, int64_t ref_tid, int32_t min_depth, int32_t min_alt, int32_t frac_num, int32_t frac_den, int64_t *n_sites);
/* the last result copied down: out holds the n_sites of that call */
int slx_pile_sites_to_host(slx_pile *p, slx_pile_site *out);
/* the last result as text to path ("-": stdout), formatted on the host (the list is small):
 * name \t pos + 1 \t ref \t depth \t A \t C \t G \t T \t N \t DEL \t INS \t LOWQ \n, every allele column as fwd,rev; name is the contig's of ref_names */
int slx_pile_sites_tsv(slx_pile *p, const char *path);

/* all counts 0 again; the knobs stay */
int slx_pile_clear(slx_pile *p);
/* "records_seen", "records_counted", "long_records", "events_lds", "events_global" (the adds by where they went), "sites" (of the last slx_pile_sites), and
 * kernel times from HIP events in microseconds "us_add", "us_sites"; -1 for an unknown name */
int64_t slx_pile_counter(const slx_pile *p, const char *name);

#ifdef __cplusplus
}
#endif
#endif
