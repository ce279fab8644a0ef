/*
 * seqlib_amd_dup.h -- C-ABI of the MI355X-native duplicate marker, part of libseqlib_amd.so: batches of BAM records in HBM go in, one signature per record
 * is kept (a few tens of bytes, and the read names of paired records), a verdict per input ordinal comes out, and bit 0x400 of the records of a batch is
 * rewritten in place in HBM.  The marker keeps no record, so a file far larger than HBM is marked in two passes: add everything, finish, read it again and
 * apply.  The batch is the four values every unit here shares, (d_stream, n_bytes, d_rec_off, n_records).  Plain pointers and sizes, never throws; every
 * function that reports a status returns 0 or a negative SLX_E* code (seqlib_amd.h), slx_last_error() gives the text.
 *
 * The reference has no duplicate marker: its users leave the library for `samtools markdup` or Picard between the sort and the index.  This unit is new
 * beside it, like the sorter and the coverage unit; its rules are stated here and restated in Python, record by record, in tests/dup_util.py.
 *
 * ---- the rules.
 *   ignored     a record with flag & (0x4 | 0x100 | 0x800) or refID < 0 takes no part and is never changed by apply.  Every other record is ELIGIBLE, and
 *               apply sets its bit 0x400 to the verdict: a bit that was set before on a record that is no duplicate is cleared.
 *   library     slx_dup_set_header reads the @RG lines (lines cut at '\n', fields at '\t', the text ends at l_text or its first NUL).  An @RG line takes part
 *               when it has an ID that is not empty and that no earlier line names.  Libraries are numbered from 1: distinct LB values by first appearance,
 *               an @RG without LB is a library of its own.  Library 0 holds every record that is not resolved to a library of the header: no RG field, a
 *               first RG field of another type than Z, an empty value, an id the header does not name, an aux area that cannot be walked as far as RG.
 *               Without a header everything is library 0.  Ids are compared byte for byte, in full.
 *   5' end      ref_len = the summed lengths of M, D, N, = and X; lead, trail = the summed lengths of the leading and the trailing run of S and H
 *               operations (a CIGAR of clips only has both).  Forward: upos = pos - lead.  Reverse (0x10): upos = pos + ref_len - 1 + trail; an EMPTY CIGAR
 *               on the reverse strand gives pos - 1, which is kept.  E(r) = (library, refID, upos, reverse).
 *   score       the sum of the quality bytes q with 15 <= q <= 0xfe, summed in 64 bits and saturated at 2^31 - 1.  A pair's score is the sum of its two
 *               records' scores.
 *   classes     paired = eligible, 0x1 set and 0x8 clear; fragment = eligible and not paired.  Paired records are grouped by (library, read name); the name
 *               is the l_read_name - 1 bytes before the NUL, compared in full.  A group of exactly two records, one with 0x40 and the other with 0x80, is
 *               a PAIR; the records of every other group are ORPHANS.
 *   verdict     1. pairs are grouped by (E(a), E(b)) ordered so that E(a) <= E(b).  Every pair but the best is a duplicate, and both of its records are.
 *                  The best pair has the highest score; a tie goes to the pair whose lower ordinal is lowest.
 *               2. eligible records are grouped by E.  Where a group holds any paired record, of a pair or an orphan, every fragment in it is a duplicate.
 *                  Otherwise every fragment but the best is; the best has the highest score, a tie goes to the lowest ordinal.
 *               3. a paired record is a duplicate only by rule 1.  An orphan never is.
 *   ordinal     every record takes the next input ordinal, counted over all adds in the order of the adds and of the records inside a batch.
 *   broken      a record whose fields pass its block_size, whose name does not end in NUL (l_read_name 0 included), or whose extent does not match the
 *               offsets (the editor's test: every record starts where the block_size of the one before it ends, the last ends at n_bytes, no span below 36
 *               bytes) fails the add with SLX_EIO; slx_last_error names the LOWEST such record index.  A refused add leaves the marker as it was.
 *
 * ---- refusals.
 *   SLX_EIO          above; for apply, a record whose fixed part does not lie inside the stream (nothing is written).
 *   SLX_EUNSUPPORTED an add past "max_bytes" (default: a quarter of the HBM that is free at create; both figures are in the message), past 2^31 - 1 records
 *                    (hipCUB counts in int), a header with more than 65 535 libraries, a run of equal hash longer than "run_max" at finish.
 *   SLX_EINVAL       null or negative arguments, an unknown knob or a value out of range, apply or flags_to_host before finish, add or set_header after
 *                    finish without slx_dup_clear, set_header after the first add, an ordinal beyond those added.
 *
 * Knobs that never change a result: "wave_len" (0 .. 2^20, default 512): a record longer than this, or with more than 64 CIGAR operations, is read by a whole
 * wave (counter "long_records"); "hash_bits" (0 .. 64, default 64): the join sorts the paired records by this many low bits of the hash of (library, name)
 * and every record compares names in full inside its run of equal bits (counter "hash_runs_mixed": runs that held more than one name); "run_max" (default
 * 4096): the longest run finish walks.
 *
 * No CPU fallback: without a GPU slx_dup_create and slx_dup_file return SLX_ENODEVICE.  slx_dup_library_of and slx_dup_signature_host are host only and run the kernels'
 * own body.  Not carried: optical duplicates, secondary and supplementary records following their primary, Picard's distinction of first and second read
 * within FF and RR pairs, UMIs, the CG:B long-CIGAR form, removing duplicates (that is ReadFilter on the flag afterwards).
 */
#ifndef SEQLIB_AMD_DUP_H
#define SEQLIB_AMD_DUP_H
#include <stdint.h>
#include <stddef.h>
#include "seqlib_amd.h"
#include "seqlib_amd_sort.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slx_dup slx_dup;

/* what slx_dup_signature_host says of a record.  cls: 0 ignored (every other field is 0), 1 fragment, 2 paired.  hash: of (library, name), paired only */
typedef struct {
    int32_t cls, library, refid, reverse;
    int64_t upos, score;
    uint64_t hash;
} slx_dup_sig;

/* device < 0: the current device.  SLX_ENODEVICE without a GPU */
int  slx_dup_create(int device, slx_dup **d);
void slx_dup_free(slx_dup *d);
/* "max_bytes" (>= 1), "wave_len" (0 .. 2^20), "hash_bits" (0 .. 64), "run_max" (1 .. 2^31 - 1) */
int  slx_dup_set(slx_dup *d, const char *key, int64_t value);
/* the header text whose @RG lines name the libraries; before the first add.  A second call replaces the first */
int  slx_dup_set_header(slx_dup *d, const char *text, int64_t l_text);

/* the arguments of slx_sort_add_device: n_records block_size-prefixed records in HBM of the marker's device with their n_records + 1 uint64 offsets, counted
 * from d_rec_off[0] (which stands for d_stream's first byte).  Everything the marker needs is in its own memory when the call returns. */
int  slx_dup_add_device(slx_dup *d, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records);
/* the same for records in host memory: uploaded, then the same kernels */
int  slx_dup_add_host(slx_dup *d, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records);
/* decides every ordinal added so far; a second call changes nothing */
int  slx_dup_finish(slx_dup *d);
/* rewrites bit 0x400 of the eligible records of the batch in place in HBM; no other byte of the stream changes.  Record i has ordinal first_ordinal + i, or
 * d_ordinals[i] where that column (n_records uint32 in HBM) is given.  The whole batch is checked before a byte is written. */
int  slx_dup_apply_device(slx_dup *d, void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records, int64_t first_ordinal, const uint32_t *d_ordinals);
/* one byte per ordinal into dst (cap >= counter "records"): 0 eligible and no duplicate, 1 duplicate, 2 ignored */
int  slx_dup_flags_to_host(slx_dup *d, uint8_t *dst, int64_t cap);
/* empties the marker (signatures, names, ordinal, counters) and keeps its header, its knobs and its memory */
int  slx_dup_clear(slx_dup *d);

/* adds the records the sorter holds, segment by segment in input order, finishes, and applies the verdicts to the segments where they lie: what
 * slx_sort_finish or slx_sort_to_host hands out afterwards carries the marks.  The marker must be empty and on the sorter's device.  SLX_EUNSUPPORTED for a sorter that has spilled runs to disk
 * (slx_sort_spill): the marker works among held records only, and slx_dup_file is the route for files beyond HBM. */
int  slx_dup_mark_sorter(slx_dup *d, slx_sort *s);

/* in_path marked into out_path.  Pass 1 reads the file into a marker, taking the header's @RG lines; pass 2 reads it again, applies batch by batch in HBM and
 * hands each batch to slx_bgzf_write_device.  The header and the record order are unchanged (the header in a member of its own), an EOF block ends the file.
 * On any error no output file is left behind.  SLX_EINVAL: in_path == out_path, or "-" for either (the input is read twice).  SLX_ENODEVICE without a GPU.
 * _ex: with the caller's marker -- its device, its knobs, its counters; it must be empty, and holds the file's verdicts afterwards -- and the reader's batch
 * size in bytes (slx_dup_file takes 64 MiB). */
int  slx_dup_file(const char *in_path, const char *out_path, int device);
int  slx_dup_file_ex(slx_dup *d, const char *in_path, const char *out_path, int64_t batch_bytes);

/* host only.  The library (0 .. 65 535) of read group rg[0, l_rg) under the header text, or a negative SLX_E* code */
int  slx_dup_library_of(const char *text, int64_t l_text, const char *rg, int64_t l_rg);
/* host only, the kernels' body: the signatures of a batch in host memory under the header text (NULL, 0: none).  SLX_EIO names the lowest broken record */
int  slx_dup_signature_host(const char *text, int64_t l_text, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records, slx_dup_sig *out);

/* "device", the knobs by name, "libraries", "read_groups" (of the header), and since the last clear: "records", "ignored", "paired", "fragments",
 * "long_records", "held_bytes", "finished"; after finish "pairs", "orphans" (records), "duplicate_pairs", "duplicate_fragments", "duplicates" (records),
 * "hash_runs_mixed"; kernel times from HIP events in microseconds "us_sig" (k_dup_sig alone), "us_place" (long records, sizes, sums), "us_commit", "us_join", "us_pairs", "us_group", "us_apply"; -1 = unknown name */
int64_t slx_dup_counter(const slx_dup *d, const char *name);

#ifdef __cplusplus
}
#endif
#endif
