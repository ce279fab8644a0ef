/*
 * seqlib_amd_stats.h -- C-ABI of the MI355X-native per-read-group statistics, part of libseqlib_amd.so: block_size-prefixed BAM records that lie in HBM
 * (slx_bam_batch, slx_rec_batch, a sorter's output: d_stream with d_rec_off) are counted there, per read group: six flag counters and six histograms as the
 * reference's BamStats keeps them, and eight counters more.  Plain pointers and sizes, never throws; every function returns 0 or a negative SLX_E* code
 * (seqlib_amd.h), slx_last_error() gives the text.
 *
 * Reference interface (paths relative to the SeqLib sources).  The classes are src/non_api/BamStats.{h,cpp} and src/non_api/Histogram.{h,cpp}; they are orphaned
 * there: BamStats calls BamRecord::MeanPhred() and an int GetIntTag(tag) that no longer exist, Histogram's constructor throws for every valid argument
 * (`end >= start`), retrieveBinID returns one past the last bin for the last bin and calls exit(1) for a value outside the bins (a 300 bp read).  So the
 * interface, the bin layout, the output format and addRead's arithmetic are taken and restated here, and the broken parts are named:
 *   slx_stats_add_*, slx_stats_record     BamStats::addRead, BamReadGroup::addRead      src/non_api/BamStats.cpp:45-109
 *   slx_stats_bins                        Histogram::Histogram(start, end, width)       src/non_api/Histogram.cpp:14-48
 *   slx_stats_text                        operator<<, Histogram::toFileString           src/non_api/BamStats.cpp:21-43, src/non_api/Histogram.cpp:64-73
 *   everything else                       (new) no reference counterpart
 *
 * The rules.
 *   group      the value of the first aux field named RG if it has type Z and is not empty; otherwise "QNAMED_" + the read filter's ParseReadGroup for a record
 *              without RG:Z: the name up to its first ':', else "NA" (BamStats.cpp:89-92).  Keys are compared byte for byte and in full, never by hash alone.
 *              A key longer than 255 bytes fails the call with SLX_EUNSUPPORTED and names the record.  Groups are numbered in order of first appearance: batch
 *              order, then record order within a batch; every listing and the text use that order (the reference iterates an unordered_map: unspecified).
 *   counters   the reference's six (BamStats.cpp:48-58): "reads" every record, "supp" flag & 0x100, "qcfail" 0x200, "duplicate" 0x400, "unmap" 0x4,
 *              "mate_unmap" 0x8.  Kept quirk: "supp" counts 0x100, SecondaryFlag() under that name, as the read filter's `supp` does.  New, not part of the
 *              text: "supplementary" 0x800, "paired" 0x1, "proper_pair" 0x2, "read1" 0x40, "read2" 0x80, "reverse" 0x10, "bases" the sum of l_seq,
 *              "nm_missing" (below).
 *   histograms bounds inclusive, the layout of Histogram(start, end, width): bins [start + k * width, start + (k + 1) * width - 1] while the upper bound is
 *              below end, then one last bin up to end.
 *                SLX_STATS_MAPQ (0, 100, 1) 101 bins    SLX_STATS_NM (0, 100, 1) 101     SLX_STATS_ISIZE (-2, 2000, 10) 201: 200 bins of ten, then [1998, 2000]
 *                SLX_STATS_CLIP (0, 100, 5) 21          SLX_STATS_PHRED (0, 100, 1) 101  SLX_STATS_LEN (0, 250, 1) 251
 *              776 bins.  The end of LEN and of ISIZE is settable before the first add ("len_max", "isize_max"); the defaults are the reference's.
 *   values     mapq   the MAPQ field
 *              nm     the first aux field named NM if it has an integer type (the read filter's rule); absent or of another type nothing is added and
 *                     "nm_missing" counts it.  The reference's guard this_nm <= 100 is subsumed by the out-of-range rule.
 *              isize  -2 unless PairMappedFlag(); else -1 when tid != mtid; else |isize| computed in 64 bits
 *              clip   NumClip(): the sum of S and H operation lengths
 *              len    l_seq
 *              phred  sum(QUAL) / l_seq in integer division -- what (int)MeanPhred() gave: the double quotient of two integers below 2^53 is below the next
 *                     integer whenever the exact one is, by at least 1 / l_seq > 2^-31, far more than a rounding of 2^-52 relative -- and -1 when l_seq <= 0.
 *                     The bytes are summed as they are: 0xff "no qualities" gives 255.
 *   outside    a value below a histogram's first bound adds to its `below` count, one above its last bound to its `above` count; no bin is touched, nothing
 *              exits, nothing is clamped.  below and above are readable, not part of the text.
 *   counts     uint64, no saturation.  Integer adds commute: every result is bit-identical whatever the order of records, batches and kernels and the knobs.
 *   eligible   every record counts (addRead tests nothing).  "exclude_flags" and "min_mapq" (defaults 0 and 0) drop records with (flag & exclude_flags) != 0 or
 *              mapq < min_mapq from the batch entries.  A reader with SetRegions serves a record once per region it overlaps; it counts once per time served.
 *   failure    a record whose fields pass its block_size, or an aux field of unknown type or past the record's end, fails the call with SLX_EIO (the checks are
 *              the read filter's rf_fixed and aux walk).  The object then holds an unspecified part of that batch: slx_stats_clear it.  Nothing outside a
 *              record's span is read.  The aux fields of a record the two knobs above drop are not walked.
 *   limits     a group costs 8 copies of its row in HBM (51 KB with the default layouts) and new groups are registered 4096 per pass over the batch, so the unit is
 *              for files with few groups.  A file whose names are unique up to their first ':' and that carries no RG:Z makes a group per read; "max_groups"
 *              (default 65536: 3.4 GB, at most 16 extra passes) stops that with SLX_EUNSUPPORTED and names the record.  Clear the object then.
 *   text       the reference's header line, then one line per group: name, reads, supp, unmap, mate_unmap, qcfail, duplicate, then the histograms mapq, nm,
 *              isize, clip, phred, len, separated by tabs.  A histogram is its non-empty bins as first_second_count joined by ','; an empty histogram is
 *              an empty field (the reference's pop_back() on an empty string is undefined).
 *
 * No CPU fallback for batches: without a GPU slx_stats_create succeeds with device = -1 and the batch entries return SLX_ENODEVICE; slx_stats_record is host
 * only and works everywhere.  Not carried: Histogram::initialize (quantile bins), toCSV, Fractions, the snowtools CLI, several GPUs in one object (use
 * slx_stats_merge), CRAM.
 */
#ifndef SEQLIB_AMD_STATS_H
#define SEQLIB_AMD_STATS_H
#include <stdint.h>
#include <stddef.h>
#include "seqlib_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slx_stats slx_stats;

#define SLX_STATS_MAPQ 0
#define SLX_STATS_NM 1
#define SLX_STATS_ISIZE 2
#define SLX_STATS_CLIP 3
#define SLX_STATS_PHRED 4
#define SLX_STATS_LEN 5
#define SLX_STATS_N_HIST 6

/* what slx_stats_record says of one record: value[which] as above (value[SLX_STATS_NM] is 0 when has_nm is 0) */
typedef struct slx_stats_rec {
    int64_t value[SLX_STATS_N_HIST];
    uint32_t flag;
    int32_t has_nm, group_len, pad;
    char group[256];          /* group_len bytes, then a NUL */
} slx_stats_rec;

/* device < 0: the current one, or with no GPU at all a host-only object */
int slx_stats_create(int device, slx_stats **st);
void slx_stats_free(slx_stats *st);

/* "len_max" (250) and "isize_max" (2000), 1 .. 2^20, before the first add only; "exclude_flags" (0; 0 .. 0xffff); "min_mapq" (0; 0 .. 255); "max_groups" (65536; 1 .. 2^20):
 * the call that opens one group more fails with SLX_EUNSUPPORTED.  Knobs that never
 * change a result: "lds_groups" (1; 0 .. 16): the first groups whose rows a block keeps in LDS, fewer when LDS does not hold them, 0 is the plain form with
 * global atomics only; "window_bytes" (16384; 64 .. 32768, a multiple of 16): the stage window; "group_slots" (64; 2 .. 2^24, rounded up to a power of two): the
 * initial size of the group table, which grows; "long_record" (4096; 1 .. 2^31 - 1): a record of more bytes, or one that does not fit the stage, is taken by a
 * whole wave.  SLX_EINVAL otherwise. */
int slx_stats_set(slx_stats *st, const char *key, int64_t value);

/* n_records records in n_bytes of HBM on the object's device, d_rec_off their n_records + 1 uint64 offsets.  The caller's buffers are free again on return. */
int slx_stats_add_device(slx_stats *st, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records);
/* The same for records in host memory: they are uploaded and take the same kernels. */
int slx_stats_add_host(slx_stats *st, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records);
/* Host only, no GPU: the group key, the six values, has_nm and the flag word of the record rec[0, n), through the body the kernels compile.  SLX_EIO and
 * SLX_EUNSUPPORTED as above. */
int slx_stats_record(const uint8_t *rec, int64_t n, slx_stats_rec *out);

/* groups so far, in order of first appearance; a negative SLX_E* code on failure */
int64_t slx_stats_n_groups(slx_stats *st);
/* the name of group i (valid until the next add, merge or clear); NULL for an i that is not a group */
const char *slx_stats_group_name(slx_stats *st, int64_t i);
/* a counter of group i by its name above; a negative SLX_E* code on failure */
int64_t slx_stats_counter_of(slx_stats *st, int64_t i, const char *name);
/* the bins of histogram `which` of group i into bins[0, cap) (SLX_EINVAL when cap is below the number of bins), its below and above counts */
int slx_stats_hist(slx_stats *st, int64_t i, int which, uint64_t *bins, int64_t cap, uint64_t *below, uint64_t *above);
/* the inclusive bounds of the bins of histogram `which`: *n bins, the first min(*n, cap) into lo and hi */
int slx_stats_bins(slx_stats *st, int which, int32_t *lo, int32_t *hi, int64_t cap, int64_t *n);
/* the text above: *n bytes at *text and a NUL behind them, to be given back to slx_stats_text_free */
int slx_stats_text(slx_stats *st, char **text, int64_t *n);
void slx_stats_text_free(char *text);

/* dst += src.  Groups are matched by name; new ones are appended in src's order.  SLX_EINVAL when the bin layouts differ. */
int slx_stats_merge(slx_stats *dst, slx_stats *src);
/* no groups and no counts; the knobs stay */
int slx_stats_clear(slx_stats *st);
/* "records_seen", "records_counted", "long_records" (taken by a wave), "adds_lds" and "adds_global" (atomic adds by where they went), "group_misses" (records
 * that met a key the table did not have and were counted by a second launch), and kernel time from HIP events in microseconds "us_add"; -1 for an unknown name */
int64_t slx_stats_counter(const slx_stats *st, const char *name);

#ifdef __cplusplus
}
#endif
#endif
