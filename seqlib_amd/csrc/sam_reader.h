// sam_reader.h -- what the BAM reader (slx_bam.hip) needs of the SAM text source (slx_sam.hip): an slx_bam whose `sam` is set takes its batches from here
// instead of from BGZF members, and hands them on unchanged (read filter, slx_bam_reads_device, the host copies).  Not part of the C-ABI.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

struct slx_samsrc;
// the source opened, its header read (SLX_EIO: an @SQ line without SN or LN), the reference-name table on the device.  SLX_ENODEVICE without a GPU
int  slx_samsrc_open(const char *path, int device, slx_samsrc **out);
void slx_samsrc_close(slx_samsrc *s);
void slx_samsrc_header(const slx_samsrc *s, std::string *text, std::vector<std::string> *names, std::vector<int64_t> *lens);
int  slx_samsrc_device(const slx_samsrc *s);
int  slx_samsrc_rewind(slx_samsrc *s);
// The records of the next max_bytes of text (grown until they hold one whole line): *n_rec records in (*d_stream)[0, *n_bytes), *d_rec their n_rec + 1 offsets, both in
// HBM and valid until the next call; the source's stream has drained.  *n_rec == 0: the end of the input.  The records before a bad line are delivered; the call
// after that returns SLX_EIO and names the line.
int  slx_samsrc_next(slx_samsrc *s, int64_t max_bytes, const void **d_stream, const void **d_rec, uint64_t *n_rec, uint64_t *n_bytes, int64_t *n_members);
// false: not one of the source's names
bool slx_samsrc_set(slx_samsrc *s, const char *key, int64_t value, int *rc);
bool slx_samsrc_counter(const slx_samsrc *s, const char *name, int64_t *v);
