/*
 * seqlib_amd_win.h -- C-ABI of the MI355X-native assembly-window collector, part of libseqlib_amd.so: batches of BAM records in HBM and a collection of
 * windows go in, the assembler's staged read arrays (bases, quals, offs of slx_fml_stage, and win_off) come out in HBM, for slx_fml_stage_device and
 * slx_fml_assemble_staged.  Nothing but offsets and counters is copied to the host.  The batch is the four values every unit here shares, (d_stream, n_bytes,
 * d_rec_off, n_records).  Plain pointers and sizes, never throws; every function that reports a status returns 0 or a negative SLX_E* code (seqlib_amd.h),
 * slx_last_error() gives the text.
 *
 * Reference interface the result restates (paths relative to the reference tree): the loop
 *     while (reader.GetNextRecord(r)) for each window the record overlaps: assembler[window].AddRead(r);
 *   FermiAssembler::AddRead(const BamRecord&), AddRead(const UnalignedSequence&)          src/FermiAssembler.cpp:41-67
 *   BamRecord::Sequence, Qualities, QualityTrimmedSequence                                src/BamRecord.cpp:591-624
 * The read order and the bytes are exactly those of that loop; equality is exact.
 *
 * ---- the rules.
 *   membership  record r is a read of window i iff slx_grc_overlaps_device pairs them: the "records" rule of seqlib_amd_grc.h -- the record's interval is
 *               (tid, pos, end), end = pos + reference length of the CIGAR, pos + 1 when that is 0 or the record carries 0x4, compared closed against the
 *               window; the strand is ignored.  The collector owns an slx_grc over its windows and joins with that entry: there is one overlap test.
 *               A record in k windows is a read of each of them.
 *   selection   in this order: "skip_flags" (default 0, the reference's AddReads tests nothing): a record that carries any of these bits is left out; a
 *               record with l_seq == 0 is left out; a record with an empty name (l_read_name <= 1) is left out -- the two tests of
 *               AddRead(const UnalignedSequence&).  Each cause has a counter.
 *   bases       the record's sequence as BamRecord::Sequence() gives it, one of "=ACMGRSVTWYHKDBN" per base, as stored.  With "original_strand" = 1 a record
 *               with 0x10 comes out reverse-complemented (IUPAC complement: "=TGKCYSBAWRDMHVN") and its qualities reversed.
 *   qualities   byte j is (uint8_t)(qual[j] + 33), what BamRecord::Qualities() returns.  This holds for the 0xff filler of a record without qualities too,
 *               which wraps to 0x20 (a space): a QUIRK of the reference's AddRead(const BamRecord&), kept.  The collector always produces a quality array.
 *   trim        "qual_trim" (default -1 = off; 0 .. 93): the stretch BamRecord::QualityTrimmedSequence names is kept.  qual[0] == 0xff: the whole read.  No
 *               base at or above the threshold: the read is dropped (counter).  Otherwise [first base >= t, one past the last base >= t).  The trim happens
 *               before the strand flip.
 *   order       inside a window the reads are in ascending global record ordinal; the ordinal counts records over all adds, in the order of the adds and of
 *               the records inside a batch.  Windows are in the caller's order.  A record served twice by a reader in region mode is two records.
 *   broken      a record whose fields pass its block_size, whose name of one byte or more does not end in NUL, or whose extent does not match the offsets
 *               (the editor's test: every record starts where the block_size of the one before it ends, the last ends at n_bytes, no span below 36 bytes)
 *               fails the add with SLX_EIO; slx_last_error names the LOWEST such record index.  A failed add leaves the collector as it was before the call.
 *
 * ---- refusals.
 *   SLX_EIO          above.
 *   SLX_EUNSUPPORTED an add that would take the arena past "arena_bytes" (both figures are in the message), or the entry list to 2^32 entries or more; the
 *                    collector is unchanged and takes a smaller add afterwards.
 *   SLX_EINVAL       null or negative arguments, a window with pos2 < pos1, an unknown knob or a value out of range, slx_win_view / slx_win_download
 *                    before slx_win_finish.
 * The arena holds every read once per add on 16-byte words: bases and qualities, each rounded up to 16 bytes per read.
 *
 * Knob that never changes a result: "wave_len" (0 .. 2^20, default 512): with a trim, a record longer than this is measured by a whole wave, 64 qualities
 * per ballot from both ends.
 * No CPU fallback for batches: SLX_WIN_HOST (and SLX_WIN_AUTO on a machine without a GPU) gives a host-only object on which slx_win_set and slx_win_counter
 * work and every batch entry (add, finish, view, download, clear) returns SLX_ENODEVICE.  Not carried: read names, a per-window read cap, mate lookup, several
 * GPUs, an out-of-core arena.
 */
#ifndef SEQLIB_AMD_WIN_H
#define SEQLIB_AMD_WIN_H
#include <stdint.h>
#include <stddef.h>
#include "seqlib_amd.h"
#include "seqlib_amd_grc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slx_win slx_win;

#define SLX_WIN_HOST (-1)          /* slx_win_create: a host-only object, GPU or not (SLX_GRC_HOST) */
#define SLX_WIN_AUTO (-2)          /* the current device, or a host-only object when there is no GPU at all */

/* the result of slx_win_finish, in HBM of the collector's device; valid until the next slx_win_finish, slx_win_clear or slx_win_free on the handle */
typedef struct {
    int64_t n_win, n_reads, total, max_len;
    const void *d_bases, *d_quals;      /* total bytes each, ASCII */
    const void *d_offs;                 /* n_reads + 1 uint64: read r is [offs[r], offs[r + 1]), the layout slx_fml_stage takes */
    const void *d_win_off;              /* n_win + 1 int64: window i holds reads [win_off[i], win_off[i + 1]) */
    const void *d_rec_of_read;          /* n_reads int64: the global ordinal of the record a read came from */
} slx_win_result;

/* n_win windows, closed intervals, in the caller's order (n_win == 0 is valid).  device >= 0: that GPU (SLX_ENODEVICE without one). */
int  slx_win_create(int device, const slx_grc_iv *windows, int64_t n_win, slx_win **w);
void slx_win_free(slx_win *w);

/* "skip_flags" (0 .. 0xffff), "qual_trim" (-1 .. 93), "original_strand" (0, 1): the rules, for the adds that follow; "arena_bytes" (>= 0, default 2^34);
 * "wave_len" (0 .. 2^20) */
int  slx_win_set(slx_win *w, const char *key, int64_t value);

/* d_stream: n_bytes of block_size-prefixed BAM records in HBM of the collector's device, d_rec_off: n_records + 1 uint64 offsets, counted from d_rec_off[0]
 * (which stands for d_stream's first byte, as in seqlib_amd_edit.h).  Everything the collector needs is in its own arena when the call returns: the batch's
 * memory may be recycled. */
int  slx_win_add_device(slx_win *w, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records);
/* the same for records in host memory: uploaded, then the same kernels */
int  slx_win_add_host(slx_win *w, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records);

/* orders the reads added so far by window; more adds may follow, and another finish */
int  slx_win_finish(slx_win *w);
int  slx_win_view(slx_win *w, slx_win_result *out);
/* the same copied down; any pointer may be NULL.  bases, quals: total bytes; offs: n_reads + 1; win_off: n_win + 1; rec_of_read: n_reads */
int  slx_win_download(slx_win *w, void *bases, void *quals, uint64_t *offs, int64_t *win_off, int64_t *rec_of_read);
/* empties the collector (reads, ordinal, counters) and keeps its windows, its rules and its memory */
int  slx_win_clear(slx_win *w);

/* host only, the kernels' body: BamRecord::QualityTrimmedSequence on qual[0, len) */
void slx_win_quality_trim(const uint8_t *qual, int32_t len, int32_t qual_trim, int32_t *startpoint, int32_t *endpoint);

/* "device" (-1: host only), "windows", the knobs by name, and since the last clear: "records", "pairs" (of the join), "reads" (entries kept),
 * "drop_flags", "drop_no_seq", "drop_no_name", "drop_trimmed" (records), "long_reads" (measured by a wave), "arena_bytes_used", and kernel times from HIP
 * events in microseconds "us_measure", "us_join", "us_extract", "us_entries", "us_sort", "us_gather"; -1 = unknown name */
int64_t slx_win_counter(const slx_win *w, const char *name);

#ifdef __cplusplus
}
#endif
#endif
