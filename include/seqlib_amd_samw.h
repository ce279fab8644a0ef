/*
 * seqlib_amd_samw.h -- C-ABI of the MI355X-native SAM text writer, part of libseqlib_amd.so: block_size-prefixed BAM records that lie in HBM (slx_rec_batch,
 * slx_bam_batch: d_stream with d_rec_off) are formatted into SAM lines on the GPU and leave as plain text or, bgzip'd, through the GPU BGZF writer (slx_bgzf_*).
 * Plain pointers and sizes, never throws; every function returns 0 or a negative SLX_E* code (seqlib_amd.h), slx_last_error() gives the text.
 *
 * Reference interface each entry point replaces (paths relative to the SeqLib sources; the reference hands the records to htslib, which is not part of this
 * image: parity with htslib is by restatement of SAMv1 section 1.4, not by comparison):
 *   slx_samw_open           BamWriter::Open on a "w" writer (hts_open)                          SeqLib/BamWriter.h:10-136, src/BamWriter.cpp:69-89
 *   slx_samw_header         BamWriter::WriteHeader on a "w" writer (sam_hdr_write)              src/BamWriter.cpp:14-33
 *   slx_samw_write_host     BamWriter::WriteRecord on a "w" writer (sam_write1 per record)      src/BamWriter.cpp:103-113
 *   slx_samw_write_device   (new) the same for records that already lie in HBM; no reference counterpart
 *   slx_samw_format_device  (new) the text kept in HBM; no reference counterpart
 *   slx_samw_format_record  sam_write1 on one record (sam_format1)                              src/BamWriter.cpp:103-113
 *   slx_samw_close          BamWriter::Close (sam_close)                                        src/BamWriter.cpp:35-44
 *   slx_samw_set, slx_samw_counter   (new) knobs and diagnostics
 *
 * The text.  The definition is BamWriter::format_sam of include/SeqLib/BamWriter.h: a line is byte for byte what BamWriter(SAM)::WriteRecord writes for the
 * record (csrc/dev_samw.h and csrc/samw_host.h state the rules in C, tests/samw_util.py in Python):
 *   QNAME      the bytes up to the first NUL inside l_read_name
 *   FLAG POS+1 MAPQ PNEXT+1 TLEN   decimal
 *   RNAME      '*' for tid < 0, else the header's name;  RNEXT  '*' for mtid < 0, '=' for mtid == tid, else the name
 *   CIGAR      '*' for no ops, else <len><op> over MIDNSHP=X (op codes 9 and above print as the host writer prints them: 'B', then '?')
 *   SEQ QUAL   "*\t*" for l_seq == 0; SEQ over =ACMGRSVTWYHKDBN; QUAL '*' when qual[0] == 0xff, else qual + 33
 *   optional   while at least 4 bytes remain (fewer than four trailing bytes are not a field): c C s S i I print as 'i'; A, Z, H; B:<sub> with ",value" per
 *              element, sub from cCsSiIf; f, d and the elements of B:f as printf's %g -- formatted on the host (the slow path), the line lands among the others
 *   refusals   SLX_EIO, the message names the record's index in the batch and the rule: the record's extent is not block_size + 4 (or lies outside the stream);
 *              32 + l_read_name + 4 n_cigar + (l_seq + 1) / 2 + l_seq > block_size; tid or mtid >= n_ref; no NUL inside l_read_name; an aux field that passes the
 *              record's end; a Z / H field without NUL; an unknown aux type or B subtype.  Where a record breaks several rules the first of this list is named (the optional
 *              fields' rules field by field).
 *              A batch is all or nothing: nothing of a refused batch reaches the file, the writer stays usable, earlier batches stand.
 * Nothing beyond a record's block_size is read: the size pass checks every rule before the fill pass touches a byte.
 *
 * No CPU fallback: without a GPU slx_samw_open returns SLX_ENODEVICE.  Not carried: CRAM, the CG:B long-CIGAR form, %g on the device.
 */
#ifndef SEQLIB_AMD_SAMW_H
#define SEQLIB_AMD_SAMW_H
#include <stdint.h>
#include <stddef.h>
#include "seqlib_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slx_samw slx_samw;

#define SLX_SAMW_BGZF 1          /* slx_samw_open: the text, header included, leaves as a bgzip'd SAM through the GPU BGZF writer; no plain text comes down */

typedef struct {
    const void *d_text;          /* n_bytes of SAM lines in HBM, each ended by a line feed */
    const void *d_line_off;      /* n_records + 1 uint64 offsets into d_text */
    uint64_t n_bytes, n_records;
} slx_samw_text;

/* path "-": stdout.  device < 0: the current one.  SLX_ENODEVICE without a GPU (the file is not created), SLX_EIO when the file cannot be created. */
int slx_samw_open(const char *path, int device, int flags, slx_samw **w);

/* The header text byte for byte (l_text bytes; may be 0), and the reference names in tid order: the RNAME / RNEXT table, kept in HBM.  Once, before the records. */
int slx_samw_header(slx_samw *w, const char *text, int64_t l_text, const char *const *ref_names, int n_ref);

/* n_records records in n_bytes of HBM on the writer's device, d_rec_off their n_records + 1 uint64 offsets (slx_rec_batch, slx_bam_batch).  The caller's buffers are
 * free again when the call returns; the file write (plain text: from pinned memory, double-buffered; SLX_SAMW_BGZF: the compression) may still be in flight.
 * SLX_EIO for a refused record (see the top of the file): nothing of the batch is written. */
int slx_samw_write_device(slx_samw *w, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records);

/* The same for records in host memory: they are uploaded and take the same kernels. */
int slx_samw_write_host(slx_samw *w, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records);

/* Formats without writing: *out stays valid until the next call on w.  For callers who keep the text in HBM. */
int slx_samw_format_device(slx_samw *w, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records, slx_samw_text *out);

/* Host only, no GPU: one block_size-prefixed record rec[0, n) -> its line in out[0, *n_out), line feed included.  SLX_EIO: the record is refused (slx_last_error
 * says why); SLX_EINVAL: cap is too small (*n_out = the size needed).  The body of the slow path, and what the CPU tests hold against Python. */
int slx_samw_format_record(const uint8_t *rec, int64_t n, const char *const *ref_names, int n_ref, char *out, int64_t cap, int64_t *n_out);

/* "fast_fail" 0|1: test knob, every record takes the slow path (formatted on the host).  "stage_bytes" (16 MiB; 4096 to 2^30): plain text comes down and goes to
 * the file in pieces of this size, two pinned buffers taking turns.  SLX_EINVAL for an unknown key or a value out of range. */
int slx_samw_set(slx_samw *w, const char *key, int64_t value);

/* "records", "bytes" (of text, the header not counted), "batches", "fast_records", "slow_records", "wide_records" (sized by a whole wave: more than 256 CIGAR ops
 * or B elements), "extra_waves" (waves beyond the first that filled the SEQ / QUAL of long records), and kernel times from HIP events in microseconds "us_size",
 * "us_fill"; -1 for an unknown name. */
int64_t slx_samw_counter(const slx_samw *w, const char *name);

/* Waits for what is in flight, closes the file (SLX_SAMW_BGZF: the last member and the EOF block) and frees the handle.  Returns the first write error, if any. */
int slx_samw_close(slx_samw *w);

#ifdef __cplusplus
}
#endif
#endif
