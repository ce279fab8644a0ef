/*
 * seqlib_amd_cov.h -- C-ABI of the MI355X-native depth of coverage, part of libseqlib_amd.so: block_size-prefixed BAM records that lie in HBM (slx_bam_batch,
 * slx_rec_batch, a sorter's output: d_stream with d_rec_off) are turned into per-base depth there, and the depth is read back as arrays, region sums or bedGraph
 * text.  Plain pointers and sizes, never throws; every function returns 0 or a negative SLX_E* code (seqlib_amd.h), slx_last_error() gives the text.
 *
 * Reference interface (paths relative to the SeqLib sources).  The class is src/non_api/STCoverage.{h,cpp}; it is orphaned there (it includes headers that no
 * longer exist, and ToBedgraph prints a vector addRead never fills), so only its interface and addRead's interval arithmetic are taken:
 *   slx_cov_add_host, SLX_COV_SPAN / SLX_COV_FULL     STCoverage::addRead                      src/non_api/STCoverage.cpp:44-109
 *   slx_cov_bedgraph, slx_cov_at                      STCoverage::ToBedgraph, getCoverageAtPosition   src/non_api/STCoverage.cpp:116-176
 *   everything else                                   (new) no reference counterpart; SLX_COV_ALIGNED counts what `samtools depth` counts
 *
 * The rules.
 *   object     all contigs of a header (n_ref, ref_len, names), or one window [beg, end) of one contig.  Storage is one dense int32 array: len + 1 entries per
 *              contig or window (rounded up to 4), 4 bytes per reference base -- 12.4 GB of HBM for GRCh38.  A covered interval [lo, hi) adds +1 at lo and -1 at hi;
 *              reading settles the array into depths by an in-place inclusive scan, adding afterwards turns it back by an in-place adjacent difference.
 *   eligible   0 <= tid < n_ref, pos >= 0, (flag & exclude_flags) == 0, mapq >= min_mapq.  Defaults: exclude_flags 0x704, min_mapq 0 (samtools depth's).
 *   end        pos + reference length of the CIGAR by htslib's table (M D N = X consume, op codes 9..15 do not); pos + 1 when that is 0 or the record carries 0x4:
 *              the read filter's and the BAI builder's end.
 *   SLX_COV_SPAN     addRead(r, buff, false): p = pos + buff, e = end - buff; nothing when p < 0, e < 0 or p > e; else positions p..e INCLUSIVE of e.  Kept quirk 1: e is
 *                    one past the last aligned base, so a read covers one position more than it aligns to.  buff may be negative.
 *   SLX_COV_FULL     addRead(r, *, true): p = max(0, pos - len(first op)) when the first op is S, else pos; e = end + len(last op) when the last op is S, else end.
 *                    Kept quirk 2: only the first and the last op are looked at, so H S M gets no extension.  Inclusive of e as above.
 *   SLX_COV_ALIGNED  (default) every M, = and X block covers [x, x + len); D blocks too when count_del is 1 (default 0); N advances without covering; I, S, H, P
 *                    and op codes 9..15 do nothing.
 *   clipping   every interval is clipped to the contig or window; what lies outside is dropped silently.  In SLX_COV_SPAN a read that ends at the contig's last base
 *              therefore loses its extra position.
 *   counts     int32, no saturation.  Integer adds commute: the result is bit-identical whatever the order of records, batches, kernels and knobs.
 *   failure    a record whose fields pass its block_size (or whose extent is not block_size + 4 inside the stream) fails the call with SLX_EIO, as the read filter
 *              does; nothing beyond a record is read.  The object then holds the contributions of an unspecified part of that batch: slx_cov_clear it.
 *   regions    a reader with SetRegions serves a record once per region it overlaps; such a record is counted once per time it is served.
 *
 * No CPU fallback for batches: without a GPU slx_cov_create succeeds with device = -1 (for slx_cov_free and the host-only slx_cov_record_intervals) and
 * every other entry returns SLX_ENODEVICE.  Not carried: the reference's unordered-map storage and its uint16 vector, CRAM, several GPUs.  The bases
 * of the reads at a position (per-base pileup) are the pileup unit's: seqlib_amd_pile.h.
 */
#ifndef SEQLIB_AMD_COV_H
#define SEQLIB_AMD_COV_H
#include <stdint.h>
#include <stddef.h>
#include "seqlib_amd.h"
#include "seqlib_amd_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slx_cov slx_cov;

#define SLX_COV_SPAN 0
#define SLX_COV_FULL 1
#define SLX_COV_ALIGNED 2

/* n_ref contigs of ref_len[i] bases (0 .. 2^31 - 1) named ref_names[i] (NULL: no names, bedGraph then prints the tid).  window NULL: all contigs; else only
 * [window->beg, window->end) of contig window->tid is kept (clipped to the contig), records elsewhere contribute nothing.  device < 0: the current one, or with
 * no GPU at all a host-only object.  SLX_ENOMEM when the array does not fit in HBM. */
int slx_cov_create(int device, int n_ref, const int64_t *ref_len, const char *const *ref_names, const slx_bam_region *window, slx_cov **cov);
void slx_cov_free(slx_cov *cov);

/* "mode" SLX_COV_*; "buff" (SPAN; may be negative); "min_mapq"; "exclude_flags"; "count_del" 0|1; "long_cigar" (64; 0 .. 2^20): records with more ops are taken
 * by a whole wave; "lds_window" (8192; 0 .. 15360 entries): 0 is the plain form with global atomics only; "slice_records" (1024; 64 .. 2^20): records per block;
 * "scan_chunk" (2^30; 64 .. 2^30, a multiple of 4): entries per hipCUB call when settling.  The last four never change a result.  SLX_EINVAL otherwise. */
int slx_cov_set(slx_cov *cov, const char *key, int64_t value);

/* n_records records in n_bytes of HBM on the object's device, d_rec_off their n_records + 1 uint64 offsets.  The caller's buffers are free again on return. */
int slx_cov_add_device(slx_cov *cov, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records);
/* The same for records in host memory: they are uploaded and take the same kernels. */
int slx_cov_add_host(slx_cov *cov, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records);
/* Host only, no GPU: the [lo, hi) intervals the record rec[0, n) contributes to a contig kept as [clip_beg, clip_end), through the body the kernels compile;
 * flags and mapq are not looked at, tid < 0 or pos < 0 gives none.  *n_out intervals; SLX_EINVAL when cap is too small, SLX_EIO for a record as above. */
int slx_cov_record_intervals(const uint8_t *rec, int64_t n, int mode, int buff, int count_del, int64_t clip_beg, int64_t clip_end, int64_t *out_lo, int64_t *out_hi,
                             int64_t cap, int64_t *n_out);

/* out[0, end - beg) = depth of positions [beg, end) of contig tid; 0 outside the contig or window */
int slx_cov_depth(slx_cov *cov, int tid, int64_t beg, int64_t end, int32_t *out);
/* the settled depths of contig tid (or of the window) in HBM: *n int32, valid until the next add or clear */
int slx_cov_depth_device(slx_cov *cov, int tid, const void **d_depth, int64_t *n);
/* depth at one position, 0 outside (getCoverageAtPosition); a negative SLX_E* code on failure */
int64_t slx_cov_at(slx_cov *cov, int tid, int64_t pos);
/* the largest depth of contig tid, or of all for tid = -1; a negative SLX_E* code on failure */
int64_t slx_cov_max(slx_cov *cov, int tid);
/* per region, clipped to the contig or window: sum[i] = the sum of depth, n_at_least[i] = positions with depth >= min_depth; beg == end gives 0, 0 */
int slx_cov_regions(slx_cov *cov, const slx_bam_region *regs, int64_t n, int32_t min_depth, int64_t *sum, int64_t *n_at_least);
/* bedGraph to path ("-": stdout): name \t start \t end \t depth \n, 0-based half open, maximal runs of equal depth, contigs in header order (tid >= 0: that one
 * only); runs of depth 0 only when include_zero.  The text is made on the GPU and comes down through two pinned buffers. */
int slx_cov_bedgraph(slx_cov *cov, int tid, int include_zero, const char *path);

/* all depths 0 again; the knobs stay */
int slx_cov_clear(slx_cov *cov);
/* "records_seen", "records_counted", "long_records", "events_lds", "events_global" (the +-1 adds by where they went), "runs" (bedGraph lines of the last call),
 * and kernel times from HIP events in microseconds "us_add", "us_settle"; -1 for an unknown name */
int64_t slx_cov_counter(const slx_cov *cov, const char *name);

#ifdef __cplusplus
}
#endif
#endif
