/*
 * seqlib_amd_fastq.h -- C-ABI of the MI355X-native FASTA / FASTQ reader, part of libseqlib_amd.so: the text of a plain, bgzip'd or gzip'd file parsed into
 * batches that lie in HBM in the layouts slx_align_batch_device (d_bases, d_offs) and slx_rec_build (d_names, d_name_offs) take.  Plain pointers and sizes,
 * never throws; every function returns 0 or a negative SLX_E* code (seqlib_amd.h), slx_last_error() gives the text.  include/SeqLib/FastqReader.h carries
 * the C++ entry (FastqReader::NextBatch) beside the per-read parser of the reference class.
 *
 * Reference interface each entry point replaces (paths relative to the reference tree; the reference delegates the grammar to bwa's kseq.h, an un-vendored
 * submodule, so parity is by restatement of the grammar written at the top of include/SeqLib/FastqReader.h):
 *   slx_fastq_open        FastqReader::Open (gzopen + kseq_init)              SeqLib/FastqReader.h:26-41, src/FastqReader.cpp:8-31
 *   slx_fastq_next        FastqReader::GetNextSequence (kseq_read), a batch at a time          SeqLib/FastqReader.h:43-46, src/FastqReader.cpp:37-59
 *   slx_fastq_close       ~FastqReader (kseq_destroy + gzclose)               SeqLib/FastqReader.h:48-53
 *   slx_fastq_rewind, slx_fastq_to_host, slx_fastq_set, slx_fastq_counter   (new) no reference counterpart
 *
 * Where the bytes come from (counter "source"):
 *   0 plain   the file is read in chunks into pinned memory by a producer thread and uploaded;
 *   1 BGZF    the member chain is scanned on the host (slx_bam_scan_members); the members are inflated and CRC-checked on the GPU (dev_inflate.h) straight
 *             into the text buffer in HBM.  The host inflates nothing;
 *   2 gzip    one DEFLATE stream is serial: zlib inflates it on the producer thread into the same pinned chunks.  This source is bounded by zlib.
 *
 * How a batch is parsed.  The grammar is not regular (the end of the quality block depends on the sequence length), so the batch is
 * guessed, verified and walked again where the guess fails:
 *   fast path  k_fq_count / k_fq_lines find the line starts; k_fq_check takes record k to be lines 4k .. 4k+3 and accepts it only when line 4k starts
 *              with '@', line 4k+1 is non-empty and starts with none of '>' '@' '+', line 4k+2 starts with '+', lines 4k+1 and 4k+3 have the same
 *              length >= 1 (each after dropping a trailing CR from a line longer than one byte), and the next line starts with '@' or the input ends;
 *   slow path  from the first record that is not accepted, the rest of the batch's text comes down and goes through the serial chunk-mode parser
 *              (csrc/fq_host.h) on the host; its reads go up into the same arrays and are counted in n_slow_reads.  FASTA, multi-line records, blank lines,
 *              junk between records and every error case take this path.
 * A damaged tail (truncated or inconsistent quality, kseq's -2) ends the stream: the records before it are delivered, the next call returns n_reads == 0,
 * and counter "bad_tail" = 1.
 *
 * No CPU fallback: without a GPU slx_fastq_open returns SLX_ENODEVICE.  Not carried: reading from stdin ("-").
 */
#ifndef SEQLIB_AMD_FASTQ_H
#define SEQLIB_AMD_FASTQ_H
#include <stdint.h>
#include <stddef.h>
#include "seqlib_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slx_fastq slx_fastq;

typedef struct {
    int64_t n_reads;                 /* 0 = end of input */
    const void *d_bases, *d_offs;    /* slx_align_batch_device's layout: n_reads + 1 uint64 offsets */
    const void *d_quals;             /* same offsets as the bases; a read without a '+' block has its bytes zero */
    const void *d_names, *d_name_offs;   /* slx_rec_build's layout, no terminators */
    const void *d_coms,  *d_com_offs;
    const void *d_flags;             /* one byte per read: bit 0 the header went on after the name (kseq's comment buffer was touched), bit 1 a '+' block was read */
    int64_t n_text_bytes;            /* text consumed by this batch */
    int64_t n_slow_reads;            /* reads of this batch that came from the serial parser */
} slx_fastq_batch;                   /* valid until the next call on the reader */

/* device < 0: the current device.  SLX_EIO: missing / unreadable, or a BGZF member chain that breaks; SLX_ENODEVICE without a GPU */
int  slx_fastq_open(const char *path, int device, slx_fastq **fq);
void slx_fastq_close(slx_fastq *fq);
/* About max_bytes of text (grown until the batch holds one whole record), parsed: every complete record of it is delivered, the cut tail is carried to the
 * next call, so the concatenation of the batches does not depend on max_bytes.  Bytes are copied as they stand (no case folding).  max_bytes <= 0: 64 MiB.
 * SLX_EIO: a BGZF member that does not inflate or whose CRC differs, a gzip stream zlib refuses. */
int  slx_fastq_next(slx_fastq *fq, int64_t max_bytes, slx_fastq_batch *b);
/* Everything of the reader's current batch copied down; a NULL destination is skipped.  offs / name_offs / com_offs take n_reads + 1 uint64 each, flags
 * n_reads bytes, bases and quals offs[n_reads] bytes, names name_offs[n_reads], coms com_offs[n_reads]: fetch the offsets first.  SLX_EINVAL: b is not the
 * reader's last batch. */
int  slx_fastq_to_host(slx_fastq *fq, const slx_fastq_batch *b, void *bases, uint64_t *offs, void *quals, void *names, uint64_t *name_offs, void *coms,
                       uint64_t *com_offs, uint8_t *flags);
int  slx_fastq_rewind(slx_fastq *fq);
/* "tile_bytes" (4096; a multiple of 16, 16 ..): text per wave of k_fq_count / k_fq_lines; "gather_tile_bytes" (2048; a multiple of 16, 16 .. 4096): output
 * bytes per wave of k_fq_gather; "fast_fail" 0|1: test knob, every record fails the fast path's test (as the BAM reader's "idx_fail") */
int  slx_fastq_set(slx_fastq *fq, const char *key, int64_t value);
/* over the reader's pass: "reads", "fast_reads", "slow_reads", "batches", "bad_tail" (0 | 1), "source" (0 plain, 1 BGZF, 2 gzip), and kernel times from HIP
 * events in microseconds "us_lines", "us_check" (the offset scans included), "us_gather", "us_inflate" (the CRC included); -1 = unknown name */
int64_t slx_fastq_counter(const slx_fastq *fq, const char *name);

#ifdef __cplusplus
}
#endif
#endif
