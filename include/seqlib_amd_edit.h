/*
 * seqlib_amd_edit.h -- C-ABI of the MI355X-native record editor, part of libseqlib_amd.so: a batch of BAM records in HBM goes in, a batch of edited records in
 * HBM comes out -- tags dropped, tags added (constants, or one value per record out of a column in HBM such as the NM and MD of slx_ref_nm_md_device), sequence
 * and qualities cleared.  The batch is the four values every unit here shares, (d_stream, n_bytes, d_rec_off, n_records); the result is what the sorter, the
 * BGZF and SAM writers, coverage, statistics, intervals and the reference take.  Plain pointers and sizes, never throws; every function returns 0 or a negative
 * SLX_E* code (seqlib_amd.h), slx_last_error() gives the text.
 *
 * Reference interface the result restates, record by record (paths relative to the reference tree):
 *   drop            BamRecord::RemoveTag, RemoveAllTags                                  SeqLib/BamRecord.h
 *   clear_seq_qual  BamRecord::ClearSeqQualAndTags                                      src/BamRecord.cpp
 *   add             BamRecord::AddZTag, AddIntTag                                       src/BamRecord.cpp
 *
 * ---- the rules.  A plan is fixed per handle, then applied to batches.  Its normal form has three parts:
 *   drop   nothing, up to 8 tag names, or all tags; and a flag clear_seq_qual.
 *   add    up to 8 tags, appended behind the kept aux bytes in plan order.  An add is an INT constant (always type 'i' and 4 bytes, what AddIntTag appends), a Z
 *          constant (the value, then NUL), an INT column (one int32 per record in HBM, and a value `absent`) or a Z column (text plus n_records + 1 uint64
 *          offsets, no terminators: the layout of slx_ref_md).  An INT add carries a flag `replace`; a Z add always replaces.
 *   The result for every record is exactly what this host sequence gives on a BamRecord that holds it:
 *     1. with clear_seq_qual, ClearSeqQualAndTags(): sequence, qualities and all aux bytes go and l_seq = 0;
 *     2. otherwise, with all tags dropped, RemoveAllTags();
 *     3. otherwise RemoveTag(name) per dropped name, in plan order: each removes the FIRST occurrence only, as bam_aux_get + bam_aux_del do (a name given twice
 *        removes the first two);
 *     4. for each add in order -- Z: AddZTag: the first occurrence is removed, then the tag is appended; an EMPTY value does nothing at all, no removal and no
 *        append (the reference's rule, and what leaves an unmapped read's old MD alone).  INT without replace: AddIntTag, a plain append, so a second tag of the
 *        same name can result, as in the reference.  INT with replace: the first occurrence is removed, then the tag is appended.  An INT column whose value
 *        equals `absent`: nothing at all;
 *     5. block_size is rewritten.  No other fixed field changes, except l_seq under clear_seq_qual.
 *
 * ---- refusals.
 *   SLX_EINVAL when the plan is built: a tag that is not two bytes in [A-Za-z][A-Za-z0-9]; a name twice among the adds; more than 8 drops or more than 8 adds; a
 *     constant Z value that is empty or holds a NUL; constants above 4096 bytes in total (a Z constant counts its NUL).
 *   SLX_EIO, slx_last_error names the FIRST such record: a record whose offsets and block_size disagree (the sorter's test, with the offsets counted from
 *     d_rec_off[0]: every record starts where the block_size of the one before it ends, the last ends at n_bytes, no span below 36 bytes); fixed fields that pass its block_size; an aux area that does
 *     not parse exactly to the record's end -- an unknown type byte, a Z or H without NUL, a B with an unknown element type or running past the end, a header
 *     or a value cut short.  This is STRICTER than bam_aux_skip of include/SeqLib/hts_compat.h, which clamps a field that passes the end to the end and goes on:
 *     a batch the host accessors walk without complaint can be refused here.  The aux area is parsed whatever the plan does with it.
 *   SLX_EUNSUPPORTED for a record whose new size no longer fits block_size (2^32 + 3 bytes); no test reaches it.
 *   SLX_EINVAL for a Z column whose offsets fall or pass n_text, a column add that is not bound when the plan is applied, and for editing the handle's own last
 *     result: a result is valid until the next apply on the handle.
 *
 * Knob that never changes a result: "long_aux" (aux bytes from which a wave, not a lane, walks a record).
 * No CPU fallback for batches: SLX_EDIT_HOST (and SLX_EDIT_AUTO on a machine without a GPU) gives a host-only object on which the plan calls, slx_edit_record,
 * slx_edit_set and slx_edit_counter work and the apply calls return SLX_ENODEVICE.  slx_edit_record runs the bodies the kernels run.
 */
#ifndef SEQLIB_AMD_EDIT_H
#define SEQLIB_AMD_EDIT_H
#include <stdint.h>
#include <stddef.h>
#include "seqlib_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slx_edit slx_edit;

#define SLX_EDIT_HOST (-1)          /* slx_edit_create: a host-only object, GPU or not */
#define SLX_EDIT_AUTO (-2)          /* the current device, or a host-only object when there is no GPU at all */

/* an edited batch, in HBM of the editor's device; valid until the next slx_edit_apply_* on the same handle */
typedef struct {
    int64_t n_records, n_bytes;
    const void *d_stream;               /* n_bytes of block_size-prefixed records */
    const void *d_rec_off;              /* n_records + 1 uint64 */
} slx_edit_batch;

/* device >= 0: that GPU (SLX_ENODEVICE without one); SLX_EDIT_HOST, SLX_EDIT_AUTO: above.  The plan starts empty: the identity. */
int  slx_edit_create(int device, slx_edit **e);
void slx_edit_free(slx_edit *e);

/* ---- the plan.  tag: two bytes and a NUL. */
int  slx_edit_plan_clear(slx_edit *e);
int  slx_edit_drop_tag(slx_edit *e, const char *tag);
int  slx_edit_drop_all_tags(slx_edit *e);
int  slx_edit_clear_seq_qual(slx_edit *e);
int  slx_edit_add_int(slx_edit *e, const char *tag, int32_t value, int replace);
int  slx_edit_add_z(slx_edit *e, const char *tag, const void *value, int64_t n);
/* Columns: d_vals holds one int32 per record of the next batch; d_text holds n_text bytes and d_off n_records + 1 uint64 offsets into it.  The first call for a
 * tag appends the add to the plan; a later call for the same tag (and kind) binds new pointers in place.  The pointers are bound for the NEXT apply only: every
 * apply, failed or not, unbinds them.  They may be NULL on a handle that only serves slx_edit_record. */
int  slx_edit_add_int_column(slx_edit *e, const char *tag, const void *d_vals, int32_t absent, int replace);
int  slx_edit_add_z_column(slx_edit *e, const char *tag, const void *d_text, int64_t n_text, const void *d_off);
/* takes the column add of that tag out of the plan again (the adds behind it move up); SLX_EINVAL when the plan has no column add of that tag */
int  slx_edit_drop_column(slx_edit *e, const char *tag);

/* d_stream: n_bytes of block_size-prefixed BAM records in HBM of the editor's device, d_rec_off: n_records + 1 uint64 offsets.  The offsets count from
 * d_rec_off[0], which stands for d_stream's first byte: the tail of a larger batch is its stream pointer moved up to record k, the bytes from there on and the
 * table from entry k on.  The result's own offsets start at 0.  The result is complete when the call returns. */
int  slx_edit_apply_device(slx_edit *e, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records, slx_edit_batch *out);
/* the same for records in host memory: uploaded, then the same kernels (column pointers are device pointers all the same) */
int  slx_edit_apply_host(slx_edit *e, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records, slx_edit_batch *out);
/* the handle's last result copied down: stream (may be NULL) holds n_bytes, rec_off (may be NULL) n_records + 1 */
int  slx_edit_to_host(slx_edit *e, const slx_edit_batch *b, void *stream, uint64_t *rec_off);

/* ---- host only, the kernels' bodies: one block_size-prefixed record of n bytes under the handle's plan.  Add k of the plan, when it is a column, takes its
 * value for this record from col_int[k], or from col_z[k] with col_z_len[k] bytes (arrays of 8; NULL where the plan has no such column).  *out_len bytes result;
 * they are written to out only when they fit cap.  SLX_EIO as above. */
int  slx_edit_record(const slx_edit *e, const uint8_t *rec, int64_t n, const int32_t *col_int, const void *const *col_z, const int64_t *col_z_len, uint8_t *out, int64_t cap, int64_t *out_len);

/* "long_aux" 1..2^31 - 1 (256: four ballots of the NUL search) */
int  slx_edit_set(slx_edit *e, const char *key, int64_t value);
/* "device" (-1: host only), "long_aux", and of the last apply: "records", "long_records", "bytes_in", "bytes_out", and kernel times from HIP events in
 * microseconds "us_size", "us_scan", "us_gather"; -1 = unknown name */
int64_t slx_edit_counter(const slx_edit *e, const char *name);

#ifdef __cplusplus
}
#endif
#endif
