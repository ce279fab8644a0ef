/*
 * seqlib_amd_merge.h -- C-ABI of the MI355X-native merge of coordinate-sorted BAM files, part of libseqlib_amd.so: up to 64 inputs are read by the GPU reader
 * (seqlib_amd_bam.h) batch by batch, their records are merged in HBM into one stream in the sorter's order (seqlib_amd_sort.h) and handed to the GPU BGZF writer
 * or to the caller, a round at a time.  The host merges nothing and moves no record.  Plain pointers and sizes, never throws; every function returns 0 or a
 * negative SLX_E* code (seqlib_amd.h), slx_last_error() gives the text.  SeqLib::BamMerger (include/SeqLib/BamMerger.h) is the header-only caller, and the
 * sorter uses a merger for inputs beyond HBM (slx_sort_spill).
 *
 * Reference interface each entry point replaces (paths relative to /root/reference; the reference has no file merge of its own -- its older multi-file reader
 * iterated several BAMs in coordinate order, and its users leave the library for `samtools merge`):
 *   slx_merge_create, slx_merge_free     (new) a merger bound to one device
 *   slx_merge_add_file                   one more file of the multi-file reader
 *   slx_merge_header                     the header of the merged stream
 *   slx_merge_next, slx_merge_batch_to_host   the next records of the merged iteration, a round at a time, in HBM and copied down
 *   slx_merge_run, slx_merge_files       `samtools merge`: the merged stream into a writer, file to file
 *   slx_merge_header_text                the header rule alone (host only)
 *   slx_merge_set, slx_merge_counter     (new) knobs and diagnostics
 *
 * The rules.
 *   The order    is the sorter's: key = (uint32)tid << 32 | (uint32)pos ^ 0x80000000, ties by input index (the order of the slx_merge_add_file calls), then by
 *                position inside the input.  In Python, sorted(concatenation of the inputs in add order, key=lambda r: (r.refid & 0xffffffff, r.pos)) IS the
 *                result.  Every record is validated as the sorter validates it, and every input must be in that order itself.
 *   The bytes    are never edited.
 *   The rounds   every input has a window of records read and not yet emitted; L_i is the last key of a non-empty window.  Before a round every input that is
 *                not at its end and whose window is empty, or whose L_i equalled the previous round's bound, reads its next batch ("batch_bytes") into the
 *                window.  The bound is B = min L_i over the inputs not at their end (infinite when all are), and the round emits exactly the held records with
 *                key < B: every record not yet read has key >= L_i >= B.  An input at the bound is refilled every round, so a round that emits nothing has
 *                read something or ended an input.  A block of equal keys longer than a batch makes a window grow; the windows together hold "max_bytes".
 *   The header   every input has the same references: count, names and lengths, in order.  The text is input 0's with SO:coordinate by the sorter's rule
 *                (slx_sort_header); then, from inputs 1.. in order, every @RG, @PG or @CO line that is not byte-identical to a line already present.  @HD and
 *                @SQ lines of later inputs are dropped.
 *   Refusals     SLX_EUNSUPPORTED: more than 64 inputs; an @RG or @PG whose ID: is that of a different line already present (the message names the ID:
 *                samtools would rename it and edit the records); windows past max_bytes (the message names tid, pos and both figures); 2^32 held records.
 *                SLX_EINVAL: references that differ (the message names the input and the reference index); an input that is not sorted (the message names the
 *                path and the record's 0-based ordinal in the file) or whose records are broken; "-" as a path; an input equal to the output; a writer on
 *                another device (nothing is written); slx_merge_add_file after the first round.
 *
 * Not carried: regions and read filters on the inputs, a multi-pass merge for more than 64 inputs, CRAM, name order.
 *
 * No CPU fallback: without a GPU slx_merge_create and slx_merge_files return SLX_ENODEVICE.
 */
#ifndef SEQLIB_AMD_MERGE_H
#define SEQLIB_AMD_MERGE_H
#include <stdint.h>
#include <stddef.h>
#include "seqlib_amd.h"
#include "seqlib_amd_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slx_merge slx_merge;
typedef struct {
    int64_t n_records, n_bytes;     /* 0 records = all inputs at their end */
    const void *d_stream;           /* block_size-prefixed records in merged order, HBM, valid until the next call */
    const void *d_rec_off;          /* n_records + 1 uint64 */
    const void *d_input;            /* uint8 per record: the input it came from */
} slx_merge_batch;

/* device < 0: the current device.  SLX_ENODEVICE without a GPU */
int  slx_merge_create(int device, slx_merge **m);
void slx_merge_free(slx_merge *m);
/* whatever slx_bam_open opens; the order of the calls is the tie order; at most 64.  A refused file is not added, and the merger stays as it was */
int  slx_merge_add_file(slx_merge *m, const char *path);
/* the whole header block of the output, "BAM\1" .. last l_ref; owned by the merger, valid until the next slx_merge_add_file */
int  slx_merge_header(const slx_merge *m, const char **bam_header, int64_t *l_header);
/* one round that emits something (rounds that emit nothing are run through), or n_records = 0.  After an error of slx_merge_next or slx_merge_run the merge cannot go
 * on (an input has been read past what was emitted): the windows are dropped, and the next call reports the end */
int  slx_merge_next(slx_merge *m, slx_merge_batch *b);
/* a batch's three arrays copied down; any of the destinations may be NULL */
int  slx_merge_batch_to_host(slx_merge *m, const slx_merge_batch *b, void *stream, uint64_t *rec_off, uint8_t *input);
/* rounds until the end, each handed to the open GPU writer w in slabs of "slab_bytes" through slx_bgzf_write_device; no flush, no close */
int  slx_merge_run(slx_merge *m, slx_bgzf *w);
/* the n inputs merged into out_path: the header in a member of its own, the records, the EOF block; no file is left on error */
int  slx_merge_files(const char *const *in_paths, int n, const char *out_path, int device);
/* host only, no GPU: the header rule over n texts.  Returns the length of the merged text; it is written to dst when cap holds it (no terminator is added) */
int64_t slx_merge_header_text(const char *const *texts, const int64_t *l_texts, int n, char *dst, int64_t cap);
/* "batch_bytes" (64 MiB; >= 1): per read of an input;  "slab_bytes" (64 MiB; a multiple of the 2048-byte tile, at least one, at most 2^40): bytes per hand-over
 * to the writer;  "max_bytes" (half of the free HBM at create; >= 1): bounds all windows together;  "by_sort" (0): 1 = the ranks come from hipCUB's stable
 * radix sort over the eligible keys laid side by side in add order (the sorter's own route) instead of from the rank kernel; the bytes are the same */
int  slx_merge_set(slx_merge *m, const char *key, int64_t value);
/* over the merger's life: "inputs", "records", "bytes" (emitted), "rounds", "refills" (reads of an input, the one that finds its end included), and kernel times
 * from HIP events in microseconds "us_key", "us_rank" (table, bound, ranks, placement, prefix sum), "us_gather"; what the windows hold now: "held_records",
 * "held_bytes" (of whole batches: a batch leaves when its last record has); "device": the merger's; -1 = unknown name */
int64_t slx_merge_counter(const slx_merge *m, const char *name);

#ifdef __cplusplus
}
#endif
#endif
