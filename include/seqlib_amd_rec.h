/*
 * seqlib_amd_rec.h -- C-ABI of the MI355X-native BAM record builder, part of libseqlib_amd.so: a device-resident slx_hits, the reads and their names
 * turned into the block_size-prefixed BAM record stream in HBM, ready for slx_bgzf_write_device (seqlib_amd_bam.h).  The host builds no record and
 * serialises nothing.  Plain pointers and sizes, never throws; every function returns 0 or a negative SLX_E* code (seqlib_amd.h), slx_last_error()
 * gives the text.  BWAAligner::alignToBam (include/SeqLib/BWAAligner.h) is the header-only caller.
 *
 * Reference interface each entry point replaces (paths relative to /root/reference):
 *   slx_rec_create, slx_rec_free   (new) a builder bound to one single-device aligner; no reference counterpart
 *   slx_rec_build          the record construction of BWAAligner::alignSequence, once per hit     src/BWAAligner.cpp:151-248
 *                          and what BamWriter::WriteRecord hands to sam_write1 for each            src/BamWriter.cpp:103-113
 *                          (block_size, the fixed fields with bin = reg2bin(pos, bam_endpos), the bam1_t::data image)
 *   slx_rec_build_from_bam the same for reads that came from slx_bam_reads_device: the names are read from the batch's records in HBM
 *   slx_rec_upload         (new) reads and names from (pinned) host memory into HBM the builder owns, as slx_align_batch_device and slx_rec_build take them
 *   slx_rec_to_host        (new) the stream and its offsets copied down, for tests and tools
 *   slx_rec_counter        (new) diagnostics
 * A record's bytes are those of SeqLib::BWAAligner::make_record followed by SeqLib::BamWriter::put_record of this tree, which restate the lines above:
 * tid = rid, pos as 32 bits, bin << 16 | mapq << 8 | l_name + 1, flag << 16 | n_cigar, l_seq = the hard-clip window, mtid = mpos = -1, isize = 0, name + NUL,
 * the CIGAR words of slx_hits.cigar, the 4-bit sequence (A C G T = 1 2 4 8, anything else 15; on 0x10 the window backwards with only A and T swapped, the
 * reference's own map), qualities 0xff then zeros, NA:i NM:i AS:i.  Reads without hits produce nothing.
 *
 * Not carried: records of a SLX_F_REG2SAM result (XA / SA / MD / XS are built on the host: SLX_EUNSUPPORTED), the BC:Z comment tag, real quality values
 * (the reference's glue drops them too), SAM text, multi-device aligners.  Where the host path truncates silently -- a name beyond 254 bytes, more than
 * 65 535 CIGAR operations -- this one refuses the batch (SLX_EUNSUPPORTED), and where it asserts -- an empty hard-clip window or one that passes the
 * read -- it returns SLX_EINVAL.  A refusal builds nothing of the batch, and slx_last_error() names the first read concerned.
 *
 * No CPU fallback: without a GPU slx_rec_create returns SLX_ENODEVICE.
 */
#ifndef SEQLIB_AMD_REC_H
#define SEQLIB_AMD_REC_H
#include <stdint.h>
#include <stddef.h>
#include "seqlib_amd.h"
#include "seqlib_amd_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slx_rec slx_rec;         /* a record builder bound to one single-device aligner */

typedef struct {
    int64_t n_records, n_bytes;
    const void *d_stream;               /* n_bytes of block_size-prefixed records, in hit order; HBM of the aligner's device, valid until the builder's next call */
    const void *d_rec_off;              /* n_records + 1 uint64 offsets into d_stream */
} slx_rec_batch;

/* SLX_EINVAL: a multi-device aligner; SLX_ENODEVICE without a GPU */
int  slx_rec_create(slx_aligner *al, slx_rec **out);
void slx_rec_free(slx_rec *rb);
/* n_reads reads and names (offs[0] = name_offs[0] = 0; n_reads + 1 offsets each) copied into the builder's HBM: *d_bases, *d_offs, *d_names, *d_name_offs are valid
 * until the builder's next slx_rec_upload.  Pinned host memory (slx_host_alloc) goes up at the full rate. */
int  slx_rec_upload(slx_rec *rb, const void *bases, const uint64_t *offs, const void *names, const uint64_t *name_offs, int64_t n_reads,
                    void **d_bases, void **d_offs, void **d_names, void **d_name_offs);
/* dev: an on_device result of slx_align_batch_device on that aligner, not yet invalidated by the aligner's next call.  d_bases / d_offs: what that call was
 * given.  d_names / d_name_offs: the names laid out the same way (n_reads + 1 uint64 offsets, no terminators).  hardclip: as given to the alignment.
 * Returns when the stream is complete in HBM.  SLX_EINVAL: a host-resident result, a hard-clip window outside its read; SLX_EUNSUPPORTED: a
 * SLX_F_REG2SAM result, a name beyond 254 bytes, a hit with more than 65 535 CIGAR operations. */
int  slx_rec_build(slx_rec *rb, const slx_hits *dev, const void *d_bases, const void *d_offs, const void *d_names, const void *d_name_offs, int hardclip,
                   slx_rec_batch *out);
/* the same for the reads slx_bam_reads_device(rd, batch, ...) last produced (dev is their alignment): the bases and the names are taken from the reader's
 * HBM (the unpacked reads; read_name of record rec_of_read[i] in the batch's d_stream), nothing is uploaded */
int  slx_rec_build_from_bam(slx_rec *rb, const slx_hits *dev, slx_bam *rd, const slx_bam_batch *batch, int hardclip, slx_rec_batch *out);
/* b->n_bytes bytes into dst (cap bytes) and, when rec_off_dst is not NULL, b->n_records + 1 offsets; SLX_EINVAL when cap is too small or b is not the builder's last batch */
int  slx_rec_to_host(slx_rec *rb, const slx_rec_batch *b, void *dst, uint64_t cap, uint64_t *rec_off_dst);
/* over the builder's life: "records", "bytes", "batches", "wide_hits" (hits sized by a wave), and kernel times from HIP events in microseconds "us_size" (owner map, sizes,
 * prefix sum), "us_fill"; -1 = unknown name */
int64_t slx_rec_counter(const slx_rec *rb, const char *name);

#ifdef __cplusplus
}
#endif
#endif
