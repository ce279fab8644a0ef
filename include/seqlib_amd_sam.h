/*
 * seqlib_amd_sam.h -- C-ABI of the MI355X-native SAM text reader, part of libseqlib_amd.so: SAM lines (plain, gzip'd or bgzip'd) parsed on the GPU into
 * block_size-prefixed BAM records in HBM, delivered as the BAM reader's batches (seqlib_amd_bam.h), so that everything that takes an slx_bam_batch takes SAM:
 * slx_bam_reads_device, slx_filter_attach, slx_bgzf_write_device (SAM to BAM with no host round trip), slx_sort_add_device, SeqLib::BamReader.
 * Plain pointers and sizes, never throws; every function returns 0 or a negative SLX_E* code (seqlib_amd.h), slx_last_error() gives the text.
 *
 * Reference interface each entry point replaces (paths relative to /root/reference; the reference hands the text to htslib, which is not part of this
 * image: parity with htslib is by restatement of SAMv1 sections 1.3 - 1.5 and 4.2, not by comparison):
 *   slx_sam_sniff        the format detection inside hts_open                      SeqLib/BamReader.h:22-26 ("BAM/SAM/CRAM"), src/BamReader.cpp:10-42
 *   slx_sam_open         BamReader::Open (hts_open + sam_hdr_read) on SAM text     src/BamReader.cpp:10-42
 *   slx_sam_parse_line   sam_read1 on one line (sam_parse1)                        src/BamReader.cpp:104-151
 *
 * The grammar.  Where SAMv1 leaves a choice, these rules are the definition (csrc/dev_sam.h and csrc/sam_host.h state them in C, tests/sam_util.py in Python):
 *   header     the leading lines that start with '@', byte for byte, a CR before the LF dropped; references = SN and LN of the @SQ lines in order of appearance
 *              (a name carried twice keeps its first line); an @SQ line without SN or LN is SLX_EIO at open; no '@' lines: empty text, no references
 *   lines      end at LF or at the end of the input; one CR before the LF is dropped (an input that ends in CR without LF is an error); at least 11 tab-separated
 *              fields, none of the 11 empty; an empty line and an '@' line after the first record are errors
 *   QNAME      1 to 254 bytes; l_read_name = length + 1
 *   FLAG       decimal, 0 to 65535 (no sign, no hex, no symbolic form)
 *   RNAME      '*' -> -1, else a header name, else an error (htslib warns and treats the record as unmapped: a deviation, nothing is silently approximated here)
 *   RNEXT      '=' -> the record's tid, '*' -> -1, else a header name, else an error
 *   POS PNEXT  decimal, 0 to 2^31 - 1; stored minus 1
 *   MAPQ       decimal, 0 to 255
 *   TLEN       [-+]?digits, fits int32
 *   CIGAR      '*' -> no ops; else <length><op>... over MIDNSHP=X, each length 0 to 2^28 - 1; more than 65535 ops is an error (the CG:B form is not written); with both
 *              CIGAR and SEQ present the lengths of M I S = X sum to l_seq
 *   SEQ        '*' -> l_seq 0; else 4-bit codes over =ACMGRSVTWYHKDBN, case folded, any other byte 15
 *   QUAL       '*' -> l_seq bytes 0xff; else l_seq bytes in [33, 126], stored minus 33
 *   bin        reg2bin(pos, end) in 16 bits, end = pos + the CIGAR's reference length (M D N = X), pos + 1 when that is 0 or the record carries 0x4; 4680 when pos < 0
 *   optional   TAG:TYPE:VALUE, TAG [A-Za-z][A-Za-z0-9].  A one byte in [33, 126].  i [-+]?digits in [-2^31, 2^32 - 1], stored in the smallest type: >= 0 as C S I
 *              (up to 255, 65535), < 0 as c s i (down to -128, -32768).  Z the bytes up to the tab, NUL.  H an even number of hex digits, laid out as Z.
 *              B a subtype from cCsSiIf, then ",element" per element (count = the number of commas), every element inside the subtype's range.
 *              f and the elements of B:f: (float)strtod(text); d: strtod(text) in 8 bytes; the text must be [-+]?(digits[.digits]|.digits)([eE][-+]?digits)? (no inf, nan
 *              or hex floats: a deviation from strtod's full grammar).  Any other type is an error.
 *   errors     the records before the first bad line are delivered, from whichever batch they came; the call after that returns SLX_EIO, and its message names the
 *              1-based line number of the file and what was wrong.  What is delivered does not depend on max_bytes.
 *
 * No CPU fallback: without a GPU slx_sam_open returns SLX_ENODEVICE.  Not carried: stdin, CRAM, the CG:B long-CIGAR form, FLAG in hex or symbolic form.
 */
#ifndef SEQLIB_AMD_SAM_H
#define SEQLIB_AMD_SAM_H
#include <stdint.h>
#include <stddef.h>
#include "seqlib_amd.h"
#include "seqlib_amd_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 0: BGZF (or gzip) that holds BAM\1.  1: SAM text (plain, gzip'd or bgzip'd).  SLX_EIO: unreadable, or neither.  Host only. */
int slx_sam_sniff(const char *path);

/* A reader over SAM text.  The handle is an slx_bam: slx_bam_header / _ref_name / _ref_len / _next / _rewind / _reads_device / _hits_to_host / _set / _counter /
 * _close and slx_filter_attach work on it as on a BAM reader.  slx_bam_index_load and slx_bam_set_regions return SLX_EINVAL ("SAM text has no index");
 * slx_bam_has_index returns 0.  SLX_ENODEVICE without a GPU.
 * A batch is an slx_bam_batch like any other; n_members = BGZF members inflated (0 for plain and gzip sources), n_repaired_chunks = 0.  max_bytes counts text
 * bytes and is grown until the batch holds one whole line; the cut tail is carried to the next call.
 * slx_bam_counter: "sam" 0|1, "source" 0 plain 1 BGZF 2 gzip, "lines" (of the file, consumed so far), "fast_records", "slow_records", and kernel times from HIP
 * events in microseconds "us_lines", "us_fields", "us_size", "us_fill", "us_inflate" (all summed since the open or the last rewind).
 * slx_bam_set: "sam_tile_bytes" (4096; >= 16, a multiple of 16): tile of the line pass;  "sam_fast_fail" 0|1: test knob, every line takes the slow path. */
int slx_sam_open(const char *path, int device, slx_bam **rd);

/* Host only, no GPU: one line (no line feed; one trailing CR is dropped) -> one block_size-prefixed BAM record in out[0, *n_out).  SLX_EIO: the line breaks a rule
 * (slx_last_error says which); SLX_EINVAL: cap is too small (*n_out = the size needed).  The body of the slow path, and what the CPU tests hold against Python. */
int slx_sam_parse_line(const char *line, int64_t n, const char *const *ref_names, int n_ref, uint8_t *out, int64_t cap, int64_t *n_out);

#ifdef __cplusplus
}
#endif
#endif
