/*
 * seqlib_amd_sort.h -- C-ABI of the MI355X-native coordinate sort of BAM records, part of libseqlib_amd.so: block_size-prefixed records that lie in HBM
 * (slx_bam_batch.d_stream of seqlib_amd_bam.h, slx_rec_batch.d_stream of seqlib_amd_rec.h) or come from the host are kept in an arena in HBM, sorted there
 * and handed to the GPU BGZF writer (slx_bgzf_write_device) as one sorted stream.  The host sorts nothing and moves no record.  Plain pointers and sizes,
 * never throws; every function returns 0 or a negative SLX_E* code (seqlib_amd.h), slx_last_error() gives the text.  SeqLib::BamWriter::SortByCoordinate
 * (include/SeqLib/BamWriter.h) is the header-only caller.
 *
 * Reference interface each entry point replaces (paths relative to /root/reference; the reference has no file sort of its own -- its users sort a
 * BamRecordVector with the functors below, or leave the library for `samtools sort`):
 *   slx_sort_create, slx_sort_free      (new) a sorter bound to one device; no reference counterpart
 *   slx_sort_add_device, slx_sort_add_host   the push_back into the BamRecordVector that is sorted later            SeqLib/BamRecord.h:677
 *   slx_sort_finish        std::sort(v.begin(), v.end(), BamRecordSort::ByReadPosition()) followed by the        SeqLib/BamRecord.h:681-699
 *                          BamWriter::WriteRecord loop over the sorted vector                                      src/BamWriter.cpp:103-113
 *   slx_sort_to_host       (new) the sorted stream, its offsets and the permutation copied down, for tests and tools
 *   slx_sort_file, slx_sort_file_ex     (new) file to file, what `samtools sort` is called for between BamWriter::Close and BamWriter::BuildIndex
 *   slx_sort_header        the SO: field of the @HD line that sam_hdr_write emits for a sorted file (host only)
 *   slx_sort_spill, slx_sort_file_spill (new) the sort of an input beyond HBM: sorted runs on disk, merged by a slx_merge (seqlib_amd_merge.h) -- the
 *                          temporary files and the merge of `samtools sort`
 *   slx_sort_set, slx_sort_counter      (new) knobs and diagnostics
 *
 * The rules.
 *   The order    key = (uint32)tid << 32 | (uint32)pos ^ 0x80000000: tid ascending AS UNSIGNED (so -1, the unplaced tail, comes last), inside a tid pos
 *                ascending as signed.  Ties keep input order: the sort is stable over the order of the add calls and of the records inside them.  In Python,
 *                sorted(records, key=lambda r: (r.refid & 0xffffffff, r.pos)) IS the result.  It is the order slx_bam_index_build demands, and
 *                BamRecordSort::ByReadPosition's but for where the unplaced records go.  A sorted input comes out unchanged byte for byte.
 *   The bytes    are never edited, the stored bin included.
 *   The arena    one segment of HBM per add call, filled by one device-to-device (or host-to-device) copy and never moved again.  The budget "max_bytes"
 *                is, by default, HALF of the HBM that is free when slx_sort_create runs (the rest is for the sort's tables -- 60 bytes per record -- one
 *                slab, and the writer's staging).  What does not fit is refused -- unless slx_sort_spill has named a place for run files: then the add
 *                that would pass the budget first writes the held records, sorted, as a run file and empties the arena, and slx_sort_finish merges the runs
 *                (at most 64) with a slx_merge.  Runs are consecutive stretches of the input, each sorted stably, and the merge breaks ties by run index,
 *                then by position: the result is the stable sort of the whole, byte for byte the file an arena that held everything would have given.
 *   The header   (slx_sort_header) an @HD line with an SO: field gets its value replaced, every other field and the field order kept; an @HD line without
 *                SO: gets "\tSO:coordinate" appended; a text without @HD gets "@HD\tVN:1.6\tSO:coordinate\n" in front.
 *   Refusals     SLX_EUNSUPPORTED: more bytes than max_bytes (the message gives both figures), 2^32 records or more.  SLX_EINVAL: offsets that do not rise
 *                from 0 to n_bytes, a block_size that disagrees with its offsets or is below 32 -- slx_last_error() names the 0-based ordinal, inside the
 *                call, of the first record that does not start where its predecessor's block_size ends, whose span cannot hold a record, or (the last)
 *                that does not end at n_bytes; it is found by the key kernel before any byte is gathered, and nothing of the call is added.
 *
 * Not carried: samtools' further tie-break on the strand flag (ties keep input order instead, which is what makes a sorted input come out unchanged),
 * sorting by name or by tag, a second merge pass for more than 64 runs, merging the last run from HBM instead of through a file, CRAM, SAM text.  NUL padding behind the header text is not kept by slx_sort_file.
 *
 * No CPU fallback: without a GPU slx_sort_create, slx_sort_file and slx_sort_file_ex return SLX_ENODEVICE.
 */
#ifndef SEQLIB_AMD_SORT_H
#define SEQLIB_AMD_SORT_H
#include <stdint.h>
#include <stddef.h>
#include "seqlib_amd.h"
#include "seqlib_amd_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slx_sort slx_sort;

/* device < 0: the current device.  SLX_ENODEVICE without a GPU */
int  slx_sort_create(int device, slx_sort **s);
void slx_sort_free(slx_sort *s);
/* n_records whole block_size-prefixed records, n_bytes in all, in the HBM of the sorter's device, with their n_records + 1 uint64 offsets (d_rec_off[0] = 0,
 * d_rec_off[n_records] = n_bytes): what slx_bam_batch and slx_rec_batch carry.  The bytes are copied into a new segment of the arena and the keys are
 * extracted there; the caller's buffers are free again when the call returns.  n_records = 0 adds nothing. */
int  slx_sort_add_device(slx_sort *s, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records);
/* the same for host bytes with host offsets */
int  slx_sort_add_host(slx_sort *s, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records);
/* sorts what was added and hands the sorted stream to the open GPU writer w in slabs of "slab_bytes" through slx_bgzf_write_device; no flush, no close.
 * w is on the sorter's device: a writer on another one is SLX_EINVAL, and nothing is written.  Empties the sorter, which stays usable -- also after
 * an error, of the writer's too. */
int  slx_sort_finish(slx_sort *s, slx_bgzf *w);
/* without a writer: the sorted stream into dst (cap bytes; counter "held_bytes" says how many), and, where not NULL, its "held_records" + 1 offsets into
 * rec_off_dst and the input ordinal of every output record into perm_dst.  SLX_EINVAL when cap is too small, and then the sorter keeps what it holds;
 * otherwise it is emptied. */
int  slx_sort_to_host(slx_sort *s, void *dst, uint64_t cap, uint64_t *rec_off_dst, uint32_t *perm_dst);
/* in_path through the reader batch by batch into a sorter, the header with SO:coordinate (a member of its own, as BamWriter writes it), the sorted records
 * through a GPU BGZF writer into out_path, the EOF block.  On any error no output file is left behind.  SLX_EINVAL: in_path == out_path, or "-" for either.
 * _ex: with the caller's sorter -- its device, its knobs, its counters; it must be empty, and is empty afterwards. */
int  slx_sort_file(const char *in_path, const char *out_path, int device);
int  slx_sort_file_ex(slx_sort *s, const char *in_path, const char *out_path);
/* prefix != NULL: an add that would pass max_bytes first writes the held records, sorted, as the run file "<prefix>.run%04d.bam" -- bam_header[0, l_header)
 * (a BAM header block) in a member of its own, the records, the EOF block, through the GPU BGZF writer -- and empties the sorter; slx_sort_finish then
 * writes what is still held as a last run and merges all runs into w with a slx_merge.  NULL: off, the default, behaviour as before.  With no run spilled
 * slx_sort_finish does what it does without the call.  Run files are removed by slx_sort_finish, by an error of a spill or of the merge, and by slx_sort_free;
 * a refused add (a single call's records beyond max_bytes stay refused) leaves the sorter and its runs as they were.  More than 64 runs: SLX_EUNSUPPORTED with the
 * count, and the runs are removed.  While runs are pending slx_sort_to_host returns SLX_EUNSUPPORTED, and so does the duplicate marker's route through the sorter
 * (seqlib_amd_dup.h: the marker works among held records only, and its file-to-file route is the one for large files); slx_sort_spill itself SLX_EINVAL. */
int  slx_sort_spill(slx_sort *s, const char *prefix, const void *bam_header, int64_t l_header);
/* slx_sort_file_ex with spilling for the length of the call; prefix NULL = out_path */
int  slx_sort_file_spill(slx_sort *s, const char *in_path, const char *out_path, const char *prefix);
/* host only, no GPU: the header text of a coordinate-sorted file made from text[0, l_text) (the rule above).  Returns its length; it is written to dst when
 * cap holds it (no terminator is added).  SLX_EINVAL: a null text or a negative length.  The rule itself is one host function (recsort_host.h beside the
 * kernels); it is exported because the header-only BamWriter reaches the library through this ABI alone, so that the class and slx_sort_file share the
 * one copy.  Like slx_sort_file_ex and the "held_*" counters it is more than a file sort needs: they are what the class, the tests and the tool call. */
int64_t slx_sort_header(const char *text, int64_t l_text, char *dst, int64_t cap);
/* "max_bytes" (half of the free HBM at create; >= 1): the arena's budget;  "slab_bytes" (64 MiB; a multiple of the 2048-byte tile, at least one, at most 2^40): bytes per
 * hand-over to the writer;  "batch_bytes" (64 MiB; >= 1): the reader's batch size in slx_sort_file_ex */
int  slx_sort_set(slx_sort *s, const char *key, int64_t value);
/* over the sorter's life: "records", "bytes", "segments", "slabs", and kernel times from HIP events in microseconds "us_key", "us_sort" (tables, radix sort,
 * prefix sum), "us_gather"; of the spill "runs", "run_bytes" (record bytes written to run files) and "us_merge" (wall time of the merge of the runs); what it
 * holds now: "held_records", "held_bytes"; -1 = unknown name */
int64_t slx_sort_counter(const slx_sort *s, const char *name);

#ifdef __cplusplus
}
#endif
#endif
