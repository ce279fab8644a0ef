/*
 * seqlib_amd_grc.h -- C-ABI of the MI355X-native interval queries, part of libseqlib_amd.so: a collection of genomic intervals becomes a sorted index in HBM (no
 * pointer tree), and whole batches of queries -- another collection's intervals, or block_size-prefixed BAM records that lie in HBM (slx_bam_batch,
 * slx_rec_batch: d_stream with d_rec_off) -- are joined against it there.  Plain pointers and sizes, never throws; calls that report a status return 0 or a
 * negative SLX_E* code (seqlib_amd.h), slx_last_error() gives the text.  slx_grc_free and slx_grc_result_free return nothing, slx_grc_counter a value.
 *
 * Reference interface (paths relative to the SeqLib sources); SeqLib::GenomicRegionCollection of include/SeqLib/GenomicRegionCollection.h is served by it:
 *   slx_grc_create, slx_grc_sorted       CoordinateSort, CreateTreeMap                          SeqLib/GenomicRegionCollection.cpp:69-75, 317-345
 *   slx_grc_merged                       MergeOverlappingIntervals                              SeqLib/GenomicRegionCollection.cpp:267-306
 *   slx_grc_query_host                   FindOverlappedIntervals, FindOverlaps(gr), CountOverlaps, CountContained   SeqLib/GenomicRegionCollection.cpp:400-415, 528-614
 *   slx_grc_overlaps, slx_grc_count      FindOverlaps(subject, query_id, subject_id), Intersection, FindOverlapWidth   SeqLib/GenomicRegionCollection.cpp:556-570, 619-701
 *   the overlap and containment tests    TIntervalTree::findOverlapping, findContained          SeqLib/IntervalTree.h:198, 224
 *   slx_grc_overlaps_device / _host, slx_grc_subject_counts, slx_grc_clear_counts   (new) no reference counterpart: records against a collection
 *
 * The rules.
 *   interval   (chr, pos1, pos2, strand), closed on both ends, as GenomicRegion has it.  chr is compared as a signed number; negative values are ordinary values.
 *              An interval with pos2 < pos1 fails the call with SLX_EINVAL.  Positions cover the full int32 range; whatever adds or subtracts 1 is done in 64 bits.
 *   overlap    subject s overlaps query q iff s.chr == q.chr && s.pos2 >= q.pos1 && s.pos1 <= q.pos2 (IntervalTree.h:198); with ignore_strand == 0 also
 *              s.strand == q.strand (GenomicRegionCollection.cpp:604).  Contained: s.pos1 >= q.pos1 && s.pos2 <= q.pos2 (IntervalTree.h:224).
 *   ids        the object is built from the caller's intervals in any order and keeps a permutation: every subject id is an index into the caller's array as given.
 *   order      queries in ascending query index; inside a query the hits by ascending (pos1, pos2, subject id).  The reference's order is its tree's traversal
 *              order (unspecified for equal starts, std::sort not being stable): a stated difference.  The contract is the set of (query, subject) pairs and this order.
 *   clipped    the interval of a hit is (q.chr, max(s.pos1, q.pos1), min(s.pos2, q.pos2)), strand '*' (GenomicRegionCollection.cpp:608).
 *   width      of a query: the number of its positions covered by at least one hit -- FindOverlapWidth without a collection being materialised and merged.
 *   merge      sort by (chr, pos1, pos2), stable; a run continues while run_max_pos2 >= next.pos1 on the same chr, so touching intervals merge ([4,6] and [6,8]) and
 *              adjacent ones do not ([4,5] and [6,7]); the merged interval takes its first member's pos1 and strand and the run's largest pos2.
 *   records    a record's interval is (tid, pos, end) with end = pos + reference length of the CIGAR (pos + 1 when that is 0 or the record carries 0x4): the read
 *              filter's end, compared closed against the subject's numbers as they stand -- the interval the read filter's region test uses and
 *              GenomicRegionCollection(const BamRecordVector&) builds.  The strand is ignored for records.  A record whose fields pass its block_size (or whose
 *              extent is not block_size + 4 inside the stream) fails the call with SLX_EIO, as in the filter and coverage units.
 *   counts     per-subject record counts are int64 and accumulate over calls; integer adds commute, so they are identical for any split into batches and any knob.
 *
 * No CPU fallback for batches: SLX_GRC_HOST (and SLX_GRC_AUTO on a machine without a GPU) gives a host-only object on which slx_grc_sorted,
 * slx_grc_merged, slx_grc_query_host, slx_grc_set and slx_grc_counter work and every batch entry returns SLX_ENODEVICE.  Not carried: a decomposition for one very
 * long subject at the start of a chr (every later query's candidates then start there: the count stays two binary searches, the fill scans), several GPUs.
 */
#ifndef SEQLIB_AMD_GRC_H
#define SEQLIB_AMD_GRC_H
#include <stdint.h>
#include <stddef.h>
#include "seqlib_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slx_grc slx_grc;

#define SLX_GRC_HOST (-1)          /* slx_grc_create: a host-only object, GPU or not */
#define SLX_GRC_AUTO (-2)          /* the current device, or a host-only object when there is no GPU at all */
typedef struct { int32_t chr, pos1, pos2; char strand; } slx_grc_iv;

/* What a batch join returns.  The host arrays belong to the result (slx_grc_result_free); the d_ pointers are the same arrays in HBM, valid until the next call
 * on the object.  Pairs k in [offset[i], offset[i + 1]) are query i's; offset has n_queries + 1 entries.  Without pairs (want_pairs == 0) n_pairs is still the
 * total and the four pair arrays and width are NULL. */
typedef struct {
    int64_t n_queries, n_pairs;
    uint32_t *count;            /* per query: its hits */
    int64_t *width;             /* per query: its positions covered by a hit */
    int64_t *offset;
    int32_t *query_id, *subject_id, *pos1, *pos2;          /* per pair; pos1 / pos2: the clipped interval (its chr is the query's) */
    const void *d_count, *d_width, *d_offset, *d_query_id, *d_subject_id, *d_pos1, *d_pos2;
} slx_grc_result;

/* The index over iv[0, n).  n == 0 is valid: every query answers 0.  device >= 0: that GPU (SLX_ENODEVICE without one); SLX_GRC_HOST: a host-only object, built
 * with std::stable_sort; SLX_GRC_AUTO: the current device, or a host-only object when there is no GPU.  On a GPU the sort, the running maximum and the end-sorted
 * array are made there and mirrored on the host; the two builds give identical arrays.  SLX_EINVAL for pos2 < pos1, n >= 2^31 or a device below SLX_GRC_AUTO. */
int slx_grc_create(int device, const slx_grc_iv *iv, int64_t n, slx_grc **g);
void slx_grc_free(slx_grc *g);

/* "wave_range" (64; 0 .. 2^20): a query whose candidate range is longer is filled by a whole wave, 0 sends every query with a hit there, 2^20 none;
 * "slice_queries" (2^20; 64 .. 2^24): queries per launch of the count pass; "long_cigar" (64; 0 .. 2^20): records with more ops are measured by a whole wave.
 * None changes a result.  SLX_EINVAL otherwise. */
int slx_grc_set(slx_grc *g, const char *key, int64_t value);

/* the n intervals in sorted order and the caller's index of each (either may be NULL); run_p2 / ends (may be NULL): the index's two search arrays */
int slx_grc_sorted(const slx_grc *g, slx_grc_iv *out, int32_t *perm, int32_t *run_p2, int32_t *ends);
/* the merged collection; *n_out is its size even when cap is smaller (SLX_EINVAL then, nothing past cap written) */
int slx_grc_merged(slx_grc *g, slx_grc_iv *out, int64_t cap, int64_t *n_out);

/* One query on the host, no GPU needed: the subject ids of its hits in order (contained != 0: of the subjects it contains), clipped into pos1 / pos2 when those
 * are not NULL, *width (may be NULL) its covered positions.  *n_out is the number of hits even when cap is smaller (SLX_EINVAL then). */
int slx_grc_query_host(const slx_grc *g, const slx_grc_iv *q, int ignore_strand, int contained, int32_t *subject_id, int32_t *pos1, int32_t *pos2, int64_t cap,
                       int64_t *n_out, int64_t *width);

/* nq queries against the index on the GPU: pairs, clipped intervals, per-query count and width */
int slx_grc_overlaps(slx_grc *g, const slx_grc_iv *q, int64_t nq, int ignore_strand, slx_grc_result *res);
/* counts only (contained != 0: of the subjects the query contains) */
int slx_grc_count(slx_grc *g, const slx_grc_iv *q, int64_t nq, int ignore_strand, int contained, uint32_t *count);

/* The records of a batch in HBM as queries.  res may be NULL (per-subject counts only); want_pairs == 0 leaves the pair arrays out.  Every call adds the batch to
 * the per-subject record counts. */
int slx_grc_overlaps_device(slx_grc *g, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records, int want_pairs, slx_grc_result *res);
/* the same for records in host memory (rec_off: n_records + 1 offsets): uploaded, same kernels */
int slx_grc_overlaps_host(slx_grc *g, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records, int want_pairs, slx_grc_result *res);
/* out[i]: the records so far that overlap the caller's interval i */
int slx_grc_subject_counts(slx_grc *g, int64_t *out);
int slx_grc_clear_counts(slx_grc *g);
void slx_grc_result_free(slx_grc_result *res);

/* "device" (-1: host only), "subjects", "chrs" (distinct chr values of the index), "queries", "queries_lane", "queries_wave", "pairs", "records", "long_records", "merged", "us_build", "us_count", "us_fill", "us_records", "us_merge";
 * -1 for an unknown name.  queries_lane / queries_wave / pairs are the last join's, the rest accumulate. */
int64_t slx_grc_counter(const slx_grc *g, const char *name);

#ifdef __cplusplus
}
#endif
#endif
