/*
 * seqlib_amd_ref.h -- C-ABI of the MI355X-native reference genome, part of libseqlib_amd.so: a FASTA (plain, BGZF or gzip) indexed on the GPU into the text of
 * its .fai, its bases resident in HBM one byte each, regions fetched in batches in the layout slx_align_batch_device takes, and NM and MD:Z of every record of
 * a device-resident batch of BAM records computed against it.  Plain pointers and sizes, never throws; every function returns 0 or a negative SLX_E* code
 * (seqlib_amd.h), slx_last_error() gives the text.  SeqLib::RefGenome (include/SeqLib/RefGenome.h) is the header-only caller.
 *
 * Reference interface each entry point replaces (paths relative to the reference tree):
 *   slx_ref_open / slx_ref_close        RefGenome::LoadIndex -> fai_load, ~RefGenome -> fai_destroy                       src/RefGenome.cpp
 *   slx_ref_fetch_host                  RefGenome::QueryRegion -> faidx_fetch_seq, many regions a call                   src/RefGenome.cpp
 *   slx_ref_fetch_device, slx_ref_nm_md_*, slx_ref_device, slx_ref_fai_text, slx_ref_write_fai, the rest        (new) no reference counterpart
 *
 * ---- the .fai index.  htslib and samtools are not part of this tree: what follows restates the format as samtools documents it (faidx(5)), and the answers
 * to what that text leaves open are this library's own.  One line per contig, in file order: NAME \t LENGTH \t OFFSET \t LINEBASES \t LINEWIDTH \n.
 *   - The text is cut into lines at LF; a last line need not have one.  In front of the LF a CR belongs to the terminator (so does a CR at the very end of an
 *     unterminated last line).  The bytes in front of the terminator are the line's content.
 *   - A line of no content is blank.  A line whose first byte is '>' is a header; NAME is what follows '>' up to the first space or tab (or the terminator);
 *     what follows the name is a description and is ignored.  Every other line is a sequence line, and its whole content is bases.
 *   - A base is any byte 33..126.  LENGTH is the sum of the contents of the contig's sequence lines; OFFSET the 64-bit offset, in the uncompressed text, of its
 *     first sequence line (of the byte behind the header line for a contig without one); LINEBASES and LINEWIDTH the content and the whole of that first line
 *     (0 and 0 without one).  A contig without bases is legal.
 *   - Every sequence line of a contig except its last has LINEBASES bases and LINEWIDTH bytes.  The last may be shorter (not longer), and its terminator
 *     is not compared: base i lies at OFFSET + (i / LINEBASES) * LINEWIDTH + i % LINEBASES either way.
 *   - A blank line may be followed only by another blank line, a header or the end of the text.
 *   - SLX_EIO, with the contig's name and the byte offset of the line in the message ("... (contig 'NAME', byte N)"), for: an empty name; a name seen before;
 *     a text that does not begin with '>' ("bytes before the first '>'", or "a '@' record" when it begins with '@': FASTQ); a sequence line that holds a
 *     space, a tab or any other byte outside 33..126; a sequence line that is not the contig's last and differs from its first in bases or width, or is the
 *     last and longer ("a ragged line"); a sequence line directly behind a blank line; a contig of more than 2^31 - 1 bases; a text without any contig.
 *     The first such line in file order is the one reported.
 *   - A line longer than 2^32 - 1 bytes is refused as a sequence line with a bad byte.
 * An existing <path>.fai is never trusted: the index is always built, and a file that is present and differs from the built text by a byte fails the open
 * with SLX_EIO ("stale index") -- a stale index that is believed returns wrong bases silently.  Nothing is written unless slx_ref_write_fai is called.
 *
 * ---- residency.  One byte per base exactly as in the file (case kept), contigs back to back, each starting at a multiple of 16 bytes (the bytes between are 0).
 *
 * ---- regions.  slx_bam_region (seqlib_amd_bam.h): tid over the FASTA's own contig order, [beg, end) half open and 0-based.  A region is clipped to [0, len);
 * one that is empty after clipping yields no bytes and is not an error; a tid outside [0, nseq) is SLX_EINVAL and nothing is fetched.
 *
 * ---- NM and MD.  The core of samtools calmd, restated from memory: samtools is not part of this tree, so parity with it is NOT pinned by any test here; the
 * tests pin the statement below (tests/ref_util.py) and, independently, the aligner's own NM and the host-built MD:Z of BWAAligner.
 *   A record gets nm = -1 and an empty MD when: flag 0x4 is set; its tid is outside the map (or the FASTA, with the identity) or maps to -1; pos < 0; it has no
 *   CIGAR; l_seq == 0.  Otherwise walk the CIGAR with x = pos, y = 0, u = 0, nm = 0:
 *     M, =, X   per base: stop the whole walk when x has passed the contig's end (and -- this library's answer where the rule is silent -- when y has reached
 *               l_seq).  c1 = the read's 4-bit code at y; c2 = the nt16 code of the reference byte at x, case-insensitive: the letters of "ACMGRSVTWYHKDBN"
 *               take their codes 1..15, every other byte 15.  A match is (c1 == c2 and c1 != 15) or c1 == 0: u += 1.  A mismatch emits u in decimal, then
 *               the reference byte in upper case; nm += 1; u = 0.
 *     D         emit u, then '^', then the deleted reference bytes in upper case, stopping the walk at the contig's end; nm grows by the bytes emitted; u = 0.
 *     I         nm += len, y += len.      S   y += len.      N   x += len.      H, P and the op codes 9..15: nothing.
 *   At the end emit u.  A record whose fields pass its block_size, or whose extent in the offsets is not block_size + 4 inside the stream, fails the call with
 *   SLX_EIO; slx_last_error names the first such record.
 *
 * Knobs that never change a result: "tile_bytes" (the line pass), "gather_tile_bytes" (the compaction and the fetch), "window_bytes" (text in HBM at a time),
 * "long_record" (l_seq from which a wave, not a lane, walks a record).
 *
 * No CPU fallback: without a GPU slx_ref_open returns SLX_ENODEVICE.  slx_ref_fai_of_text and slx_ref_record_nm_md are host only and need none; they run the
 * bodies the kernels run.
 */
#ifndef SEQLIB_AMD_REF_H
#define SEQLIB_AMD_REF_H
#include <stdint.h>
#include <stddef.h>
#include "seqlib_amd.h"
#include "seqlib_amd_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slx_ref slx_ref;

/* what device consumers take: contig i is d_bases[d_contig_off[i], d_contig_off[i] + d_contig_len[i]); valid until slx_ref_close */
typedef struct {
    int64_t n_contigs, n_bytes;         /* n_bytes: the extent of d_bases */
    const void *d_bases;                /* uint8 */
    const void *d_contig_off;           /* n_contigs + 1 uint64, multiples of 16 */
    const void *d_contig_len;           /* n_contigs int64 */
} slx_ref_dev;

/* NM and MD of a batch, in HBM of the reference's device; valid until the next slx_ref_nm_md_* on the same handle */
typedef struct {
    int64_t n_records, md_bytes;
    const void *d_nm;                   /* n_records int32; -1: not eligible */
    const void *d_md;                   /* md_bytes bytes, no terminators */
    const void *d_md_off;               /* n_records + 1 uint64 */
} slx_ref_md;

/* Loads the whole FASTA: index built, bases resident.  SLX_EIO: unreadable, malformed (rules above) or beside a stale .fai.  _ex: the knobs of the load, for tests
 * and tools; 0 takes the default (window_bytes 64 MiB, at least 64; tile_bytes 4096 and gather_tile_bytes 2048, multiples of 16, the latter at most 4096). */
int  slx_ref_open(const char *path, int device, slx_ref **out);
int  slx_ref_open_ex(const char *path, int device, int64_t window_bytes, int64_t tile_bytes, int64_t gather_tile_bytes, slx_ref **out);
void slx_ref_close(slx_ref *r);
/* "gather_tile_bytes" (the fetch; 2048), "long_record" 1..2^31 - 1 (64: from one full chunk of lanes on a wave walks a record; profiles/NOTES_ref.md) */
int  slx_ref_set(slx_ref *r, const char *key, int64_t value);
/* "contigs", "bases", "text_bytes", "windows", "source" (0 plain, 1 BGZF, 2 gzip), "hbm_bytes", "long_records" (of the last NM/MD call), "long_record" (the knob), and kernel times from HIP
 * events in microseconds: "us_lines", "us_class" (class, scans, headers, check), "us_gather" (the compaction), "us_inflate", "us_fetch", "us_md_size", "us_md_text" (the last
 * three of the last call); -1 = unknown name */
int64_t slx_ref_counter(const slx_ref *r, const char *name);

int64_t slx_ref_nseq(const slx_ref *r);
const char *slx_ref_name(const slx_ref *r, int64_t tid);          /* NULL outside [0, nseq) */
int64_t slx_ref_len(const slx_ref *r, int64_t tid);               /* -1 outside [0, nseq) */
int64_t slx_ref_tid(const slx_ref *r, const char *name);          /* -1: no such contig */
/* the .fai text (owned by the handle) */
const char *slx_ref_fai_text(const slx_ref *r, int64_t *n);
/* writes it; fai_path NULL: the FASTA's path + ".fai" */
int  slx_ref_write_fai(const slx_ref *r, const char *fai_path);
int  slx_ref_device(const slx_ref *r, slx_ref_dev *out);

/* n regions, clipped, back to back in *d_bases with n + 1 uint64 offsets in *d_offs: what slx_align_batch_device takes.  upper = 1 folds a-z to upper case.  Both
 * blocks belong to the handle and are valid until its next fetch.  *n_bytes (may be NULL): the total. */
int  slx_ref_fetch_device(slx_ref *r, const slx_bam_region *regions, int64_t n, int upper, const void **d_bases, const void **d_offs, int64_t *n_bytes);
/* the same into caller memory: offs holds n + 1; bases may be NULL to learn offs[n] first, otherwise cap bytes of it must hold offs[n] (SLX_EINVAL) */
int  slx_ref_fetch_host(slx_ref *r, const slx_bam_region *regions, int64_t n, int upper, void *bases, int64_t cap, uint64_t *offs);

/* d_stream: n_bytes of block_size-prefixed BAM records in HBM of the reference's device, d_rec_off: n_records + 1 uint64 offsets (as slx_cov_add_device takes
 * them).  tid_map[batch tid], n_map entries of host memory, gives the FASTA contig or -1; NULL is the identity over the FASTA's contigs. */
int  slx_ref_nm_md_device(slx_ref *r, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records, const int32_t *tid_map, int64_t n_map, slx_ref_md *out);
/* the same for records in host memory: uploaded, then the same kernels */
int  slx_ref_nm_md_host(slx_ref *r, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records, const int32_t *tid_map, int64_t n_map, slx_ref_md *out);
/* the handle's last result copied down: nm holds n_records, md_off n_records + 1, md (may be NULL) md_bytes */
int  slx_ref_md_to_host(slx_ref *r, const slx_ref_md *m, int32_t *nm, void *md, uint64_t *md_off);

/* ---- host only, the kernels' bodies */
/* one block_size-prefixed record of n bytes against the contig contig[0, contig_len) its tid is taken to name: *nm (-1: not eligible) and *md_len bytes of MD;
 * at most cap of them are written to md (the text is complete only when *md_len <= cap).  SLX_EIO as above. */
int  slx_ref_record_nm_md(const uint8_t *rec, int64_t n, const uint8_t *contig_bytes, int64_t contig_len, int32_t *nm, char *md, int64_t cap, int64_t *md_len);
/* the .fai text of n bytes of FASTA text: *fai (slx_ref_text_free) and *fai_len.  SLX_EIO with the message of the rules above. */
int  slx_ref_fai_of_text(const void *text, int64_t n, char **fai, int64_t *fai_len);
void slx_ref_text_free(char *p);

#ifdef __cplusplus
}
#endif
#endif
