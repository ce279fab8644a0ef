/*
 * seqlib_amd_bam.h -- C-ABI of the MI355X-native BAM reader, part of libseqlib_amd.so: BGZF members inflated, CRC-checked and cut
 * into records on the GPU.  Plain pointers and sizes, never throws; every function returns 0 or a negative SLX_E* code (seqlib_amd.h),
 * slx_last_error() gives the text.  include/SeqLib/BamReader.h is the thin header-only mirror of the reference class over these entry points.
 *
 * Reference interface each entry point replaces (paths relative to /root/reference; the reference hands the bytes to htslib, which is not part of
 * this image: BGZF, DEFLATE and the BAM layout are restated from RFC 1951 / 1952 and SAMv1 sections 4.1, 4.2):
 *   slx_bam_open          BamReader::Open (hts_open + sam_hdr_read)         SeqLib/BamReader.h:16-76, src/BamReader.cpp:10-42
 *   slx_bam_header, slx_bam_ref_name, slx_bam_ref_len      BamReader::Header            SeqLib/BamReader.h:52, src/BamReader.cpp:153-157
 *   slx_bam_next          BamReader::Next (sam_read1), a batch at a time    src/BamReader.cpp:104-151
 *   slx_bam_reads_device  (new) the batch's sequences as slx_align_batch_device takes them, unpacked in HBM; no reference counterpart
 *   slx_bam_hits_to_host  (new) a device-resident slx_hits of slx_align_batch_device copied to the host in one piece; no reference counterpart
 *   slx_bam_rewind        BamReader::Reset                   src/BamReader.cpp:56-62
 *   slx_bam_close         BamReader::Close                   src/BamReader.cpp:44-54
 *   slx_bam_set, slx_bam_counter   (new) knobs and diagnostics
 *   slx_bam_scan_members, slx_bam_members_free, slx_bam_inflate_file   (new) helpers for tests and tools
 *
 * No CPU fallback: without a GPU slx_bam_open and slx_bam_inflate_file return SLX_ENODEVICE.  Not carried: region iteration (BAI), CRAM, SAM text.
 */
#ifndef SEQLIB_AMD_BAM_H
#define SEQLIB_AMD_BAM_H
#include <stdint.h>
#include <stddef.h>
#include "seqlib_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slx_bam slx_bam;

typedef struct {            /* one BGZF member (a gzip member with the "BC" extra field) */
    uint64_t file_off;      /* of the member's first byte */
    uint32_t data_off;      /* of the deflate stream, from file_off */
    uint32_t data_len;      /* compressed bytes */
    uint32_t isize;         /* inflated bytes, from the trailer (<= 65536) */
    uint32_t crc32;         /* of the inflated bytes, from the trailer */
} slx_bam_member;

typedef struct {
    int64_t n_records;          /* 0 = end of file */
    int64_t n_bytes;            /* bytes of the n_records whole records: stream[0, n_bytes) */
    const uint8_t  *stream;     /* block_size-prefixed records as they stand in the file; pinned host memory, recycled by the next call */
    const uint64_t *rec_off;    /* n_records + 1 offsets into stream (record i at rec_off[i], its block_size word first); pinned, recycled */
    const void *d_stream;       /* the same two arrays in HBM, valid until the next call on the reader */
    const void *d_rec_off;
    int64_t n_members;          /* BGZF members inflated for this batch */
    int64_t n_repaired_chunks;  /* chunks of the record index whose guessed first record start was wrong and were walked again */
} slx_bam_batch;

/* device < 0: the current device.  SLX_EIO: missing file, bad magic, broken member chain, a header that does not parse.  A file without the EOF
 * block opens with a warning on stderr (as htslib's) and counter "missing_eof" = 1. */
int  slx_bam_open(const char *path, int device, slx_bam **rd);
void slx_bam_close(slx_bam *rd);
int  slx_bam_header(const slx_bam *rd, const char **text, int64_t *l_text, int *n_ref);
const char *slx_bam_ref_name(const slx_bam *rd, int i);
int64_t slx_bam_ref_len(const slx_bam *rd, int i);

/* The next span of members whose inflated size is about max_bytes (at least one member; grown until it holds one whole record), inflated, CRC-checked
 * and indexed.  A record cut by the end of the span is carried to the next batch.  SLX_EIO names the file offset of a member that fails to inflate
 * or whose CRC differs. */
int  slx_bam_next(slx_bam *rd, int64_t max_bytes, slx_bam_batch *batch);
/* The sequences of the batch's records that carry none of skip_flags, as ASCII (=ACMGRSVTWYHKDBN) in HBM in slx_align_batch_device's layout
 * (*d_bases, *d_offs with *n_reads + 1 uint64 entries; valid until the next call on the reader).  original_strand = 1: records with 0x10 come out reverse-complemented
 * (IUPAC complement), the read as sequenced; 0: as stored.  *rec_of_read: record index of read i, host memory owned by the reader. */
int  slx_bam_reads_device(slx_bam *rd, const slx_bam_batch *batch, int skip_flags, int original_strand, void **d_bases, void **d_offs,
                          int64_t *n_reads, const int64_t **rec_of_read);
/* *host = the device-resident result *dev (of slx_align_batch_device on the single-device aligner al) as a host result: freed with slx_hits_free */
int  slx_bam_hits_to_host(slx_bam *rd, slx_aligner *al, const slx_hits *dev, slx_hits *host);
int  slx_bam_rewind(slx_bam *rd);
/* "chunk_bytes" (65536; >= 64): chunk of the record index;  "idx_fail" 0|1: test knob, every guess of the index is made wrong */
int  slx_bam_set(slx_bam *rd, const char *key, int64_t value);
/* "members", "members_done", "repaired_chunks", "index_rounds", "missing_eof", "records", and kernel times of the last batch from HIP events in
 * microseconds: "us_inflate", "us_crc", "us_index", "us_unpack"; -1 = unknown name */
int64_t slx_bam_counter(const slx_bam *rd, const char *name);

/* host only: the member table of a BGZF file (*members is owned by the caller until slx_bam_members_free); *has_eof = the last member is the empty EOF block */
int  slx_bam_scan_members(const char *path, slx_bam_member **members, int64_t *n_members, int *has_eof);
void slx_bam_members_free(slx_bam_member *members);
/* every member of any BGZF file through k_bgzf_inflate + k_bgzf_crc into the host buffer dst (cap bytes); no BAM parsing.  *n = inflated size (also
 * when cap is too small: SLX_EINVAL) */
int  slx_bam_inflate_file(const char *path, int device, void *dst, uint64_t cap, uint64_t *n);

#ifdef __cplusplus
}
#endif
#endif
