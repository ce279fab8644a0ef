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
 *   slx_bam_index_load, slx_bam_has_index   the sam_index_load of BamReader::Open          src/BamReader.cpp:33
 *   slx_bam_set_regions   BamReader::SetRegion / SetRegions (sam_itr_queryi per region)    src/BamReader.cpp:64-102, 104-137
 *   slx_bam_index_build   BamWriter::BuildIndex (sam_index_build)                          src/BamWriter.cpp
 *   slx_bai_query, slx_bai_stats, slx_bai_free   (new) the index on the host, for tests and tools
 * and of the BGZF writer (slx_bgzf_*: DEFLATE, CRC32 and framing on the GPU; the host compresses nothing):
 *   slx_bgzf_open         BamWriter::Open (hts_open "wb")                    SeqLib/BamWriter.h:10-136, src/BamWriter.cpp:69-89
 *   slx_bgzf_write        BamWriter::WriteHeader / WriteRecord (sam_hdr_write, sam_write1: the bytes they hand to bgzf_write)   src/BamWriter.cpp:14-33, 103-113
 *   slx_bgzf_write_device (new) the same for bytes that already lie in HBM, e.g. slx_bam_batch.d_stream; no reference counterpart
 *   slx_bgzf_flush        the bgzf_flush behind sam_hdr_write: the records start in a member of their own       src/BamWriter.cpp:26
 *   slx_bgzf_close        BamWriter::Close (sam_close: the last member and the EOF block)                       src/BamWriter.cpp:35-44
 *   slx_bgzf_set, slx_bgzf_counter   (new) knobs and diagnostics
 *
 * The BAI index is restated from SAMv1 section 5.2; where it leaves a choice the rule is htslib's:
 *   end of a record   pos + reference length of the CIGAR (M D N = X); pos + 1 when that is 0 or the record carries 0x4
 *   bin               reg2bin(pos, end), computed: the record's stored bin is not trusted
 *   virtual offset    of whole-file inflated offset x: the first member m with start[m] + isize[m] > x (never an empty one) gives
 *                     file_off[m] << 16 | (x - start[m]); the end of the data gives the file offset behind the last non-empty member << 16
 *   chunk             a maximal run of file-consecutive records with one (tid, bin), tid >= 0: (begin of the first, end of the last)
 *   linear index      per 16 KiB window the lowest begin of the records touching it; an untouched window takes the next touched one above it
 *   pseudo-bin 37450  per reference with records: (begin of its first record, end of its last), (n_mapped, n_unmapped: 0x4); n_no_coor: tid < 0
 * Not done: htslib's post-pass that merges chunks lying in one BGZF block and lifts sparse bins into their parents (the index is valid without it,
 * byte parity with `samtools index` is not claimed), and CSI.
 *
 * No CPU fallback: without a GPU slx_bam_open, slx_bam_inflate_file, slx_bam_index_build and slx_bgzf_open return SLX_ENODEVICE.  Not carried: CRAM, CSI.
 * SAM text is read by slx_sam_open (seqlib_amd_sam.h), whose handle is an slx_bam; slx_bam_open itself takes BAM only.
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
 * microseconds: "us_inflate", "us_crc", "us_index", "us_unpack"; of the region iteration "regions_done", "region_candidates" (records walked),
 * "region_kept" and "us_region"; "sam" 0|1: the reader is over SAM text (seqlib_amd_sam.h lists that reader's further names); -1 = unknown name */
int64_t slx_bam_counter(const slx_bam *rd, const char *name);

/* The index of the reader's file: bai_path, or when NULL <path>.bai, then <path> with ".bam" replaced by ".bai".  slx_bam_open tries the same two names
 * silently (a missing index is no error).  SLX_EIO: missing, short or damaged; SLX_EINVAL: its reference count is not the header's. */
int  slx_bam_index_load(slx_bam *rd, const char *bai_path);
int  slx_bam_has_index(const slx_bam *rd);

typedef struct { int32_t tid; int64_t beg, end; } slx_bam_region;      /* 0-based, half open */
/* After the call slx_bam_next serves the regions in the order given, inside a region in file order: every record with tid == region.tid,
 * pos < region.end and end > region.beg (end as above), once per region it overlaps.  Per region the index's merged chunk list is planned on the host; only
 * the members it names are inflated and indexed, k_bam_region_keep tests their records and k_bam_gather compacts the kept ones, bytes unchanged, so a batch
 * is what it is for the whole file: stream[0, n_bytes) holds exactly the n_records whole records, and slx_bam_reads_device works on it as it stands.  One call
 * takes as many of the next regions as fit max_bytes, a larger region is cut at member boundaries; n_records == 0 is the end of the last region.
 * n = 0: back to the whole file, from its start (slx_bam_rewind drops the regions too).  SLX_EINVAL: no index loaded, or a tid outside the header. */
int  slx_bam_set_regions(slx_bam *rd, const slx_bam_region *regs, int64_t n);

/* The BAI of a coordinate-sorted BAM (tid ascending as unsigned, pos non-decreasing inside a tid), built on the GPU: the file goes through the reader's
 * inflate, CRC and record-index kernels batch by batch, and per batch k_bai_rec / k_bai_heads / k_bai_chunks compute ends, bins, virtual offsets, chunks, the
 * linear index and the pseudo-bin's figures; hipCUB sorts the chunks; the host lays the bytes out.  bai_path NULL: bam_path + ".bai".  SLX_EINVAL: the
 * first record out of order (slx_last_error names its 0-based ordinal) or a record past its reference's end; no file is written then.
 * _ex: batch_bytes / chunk_bytes of the pass (0: 64 MiB / 65536), for tests and tools. */
int  slx_bam_index_build(const char *bam_path, int device, const char *bai_path);
int  slx_bam_index_build_ex(const char *bam_path, int device, const char *bai_path, int64_t batch_bytes, int64_t chunk_bytes);

/* host only, no GPU: the merged chunk list that holds every record of tid overlapping [beg, end): the bins of reg2bins(beg, end), chunks that end at or
 * below the linear index's offset of beg's window dropped, the rest sorted by begin and merged where they touch or overlap.  *chunks: 2 * *n virtual
 * offsets, freed with slx_bai_free.  SLX_EIO: a missing, short, truncated or damaged file (every count is checked against the bytes left). */
int  slx_bai_query(const char *bai_path, int tid, int64_t beg, int64_t end, uint64_t **chunks, int64_t *n);
/* host only: n_ref and the trailing n_no_coor (0 when absent); for tid >= 0 also the pseudo-bin's two counts, n_bin (the pseudo-bin counted) and n_intv */
int  slx_bai_stats(const char *bai_path, int *n_ref, uint64_t *n_no_coor, int tid, uint64_t *n_mapped, uint64_t *n_unmapped, int *n_bin, int *n_intv);
void slx_bai_free(void *p);

/* host only: the member table of a BGZF file (*members is owned by the caller until slx_bam_members_free); *has_eof = the last member is the empty EOF block */
int  slx_bam_scan_members(const char *path, slx_bam_member **members, int64_t *n_members, int *has_eof);
void slx_bam_members_free(slx_bam_member *members);
/* every member of any BGZF file through k_bgzf_inflate + k_bgzf_crc into the host buffer dst (cap bytes); no BAM parsing.  *n = inflated size (also
 * when cap is too small: SLX_EINVAL) */
int  slx_bam_inflate_file(const char *path, int device, void *dst, uint64_t cap, uint64_t *n);

/* ---- the BGZF writer.  The file is the concatenation of the writes in call order, cut into members of 0xff00 bytes from the start of the stream and from
 * every flush (SeqLib::BamWriter's cutting), each member deflated (one dynamic-code block, or a stored one where that is not smaller), CRC-summed and
 * framed on the GPU by k_bgzf_deflate / k_bgzf_trailer / k_bgzf_pack; one device-to-host copy of exactly the file bytes and one fwrite per batch.
 * The bytes of the file depend only on the byte stream and the flush points: not on how the stream was split over calls, not on host or device origin,
 * not on batch_bytes, and they are the same on every run.  Errors are sticky: after the first one every call returns it, and slx_bgzf_close returns it.
 * A handle is not usable after slx_bgzf_close, which frees it (there is no "write to a closed writer": the handle is gone). */
typedef struct slx_bgzf slx_bgzf;
/* "-" = stdout; device < 0: the current device.  SLX_ENODEVICE without a GPU, and then no file is created; SLX_EIO: the file cannot be created */
int  slx_bgzf_open(const char *path, int device, slx_bgzf **w);
/* n host bytes; returns once they are staged in HBM (p may be reused).  Whole batches are compressed and written while later calls stage.  SLX_EINVAL: n < 0 */
int  slx_bgzf_write(slx_bgzf *w, const void *p, int64_t n);
/* the same for n bytes in the writer's device's HBM */
int  slx_bgzf_write_device(slx_bgzf *w, const void *d_p, int64_t n);
/* ends the member being filled: the next byte written starts a new one.  Nothing pending: no member */
int  slx_bgzf_flush(slx_bgzf *w);
/* flush, the 28-byte EOF block, close the file, free the handle.  Returns the first error of the writer's life (SLX_EIO: a failed fwrite; SLX_ENODEVICE: HIP) */
int  slx_bgzf_close(slx_bgzf *w);
/* "batch_bytes" (64 MiB; >= 0xff00): staged bytes that make a batch */
int  slx_bgzf_set(slx_bgzf *w, const char *key, int64_t value);
/* over the writer's life, of the batches handed over so far (the call waits for the one in flight): "members", "stored_members", "bytes_in", "bytes_out", and
 * kernel times from HIP events in microseconds "us_deflate", "us_crc", "us_gather"; -1 = unknown name */
int64_t slx_bgzf_counter(const slx_bgzf *w, const char *name);

#ifdef __cplusplus
}
#endif
#endif
