// slx_internal.h -- internal declarations shared by the host and device translation units of
// libseqlib_amd.so.  Nothing here is part of the C-ABI (include/seqlib_amd.h).
#pragma once
#include <atomic>
#include <cstdint>
#include <cstddef>
#include <string>
#include <vector>
#include "seqlib_amd.h"

struct slx_ann {
    int64_t offset;
    int32_t len;
    int32_t n_ambs;
    uint32_t gi;
    int32_t is_alt;
    std::string name, anno;
};
struct slx_amb {
    int64_t offset;
    int32_t len;
    char amb;
};

// Host copy of the index in bwa's own layout (what LoadIndex reads and WriteIndex dumps).
struct slx_index {
    uint64_t primary = 0;
    uint64_t L2[5] = {0, 0, 0, 0, 0};
    uint64_t seq_len = 0;               // 2 * l_pac
    std::vector<uint32_t> bwt;          // interleaved: per 128 bases 4 x u64 counts + 8 x u32
    int sa_intv = 32;
    std::vector<uint64_t> sa;           // sa[0] = -1
    int64_t l_pac = 0;
    uint32_t seed = 11;
    std::vector<slx_ann> anns;
    std::vector<slx_amb> ambs;
    std::vector<uint8_t> pac;           // forward strand, 2 bit/base
    // optional: full suffix array kept from a device build (sentinel-inclusive order, n+1 entries)
    std::vector<uint32_t> dense_sa32;
    // is the pac the forward half of the text the FM-index is over?  1: built here from sequences without N.  0: built here and N were drawn -- twice, as the
    // reference does, once for the pac and once for the BWT text.  -1: loaded from files, which do not say: the aligner finds out (slx_align.hip, k_text_is_pac)
    int text_is_pac = -1;
};

void slx_set_error(const char *fmt, ...);
// Bytes of HBM and of pinned memory this process holds through SlxDevBuf / SlxPinBuf (slx_hip.h keeps them, slx_hip_live_bytes reads them)
inline std::atomic<int64_t> slx_live_dev{0}, slx_live_pin{0};

// How a host thread waits for a stream: hipStreamSynchronize, or -- SEQLIB_AMD_WAIT=sleep -- polling the stream every 40 us.  Measured with the whole bench confined to two
// CPUs (taskset, round 6): the default wait is NOT what a starved rank loses to -- BamRecords 15.5 M reads/s (default) against 14.8 M (sleep), C5 4.6 against 4.4 M, and one
// per-read call 439 against 1 069 us -- so the default stays; the switch is kept for hosts whose runtime does spin.
bool slx_wait_sleeps();
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include <time.h>
static inline hipError_t slx_wait_stream(hipStream_t st)
{
    static const bool sleeps = slx_wait_sleeps();
    if (!sleeps) return hipStreamSynchronize(st);
    for (;;) {
        const hipError_t e = hipStreamQuery(st);
        if (e != hipErrorNotReady) return e == hipSuccess ? hipStreamSynchronize(st) : e;          // (idle: the call returns at once and leaves the usual guarantees)
        struct timespec ts = {0, 40000};
        nanosleep(&ts, nullptr);
    }
}
#endif

// device-side index construction (slx_index_gpu.hip): text T[0..n) over {0..3} -> fills bwt/sa/primary/L2
int slx_gpu_build_fm(slx_index *idx, const uint8_t *text, uint64_t n);
// the same for texts the 32-bit builder cannot count in an int (index_build_width.h: 2^31 - 1 symbols and more; slx_index_gpu64.hip); also taken for small texts when SLX_BUILD64 is set (test hook)
int slx_gpu_build_fm64(slx_index *idx, const uint8_t *text, uint64_t n);

// what the record builder (slx_rec.hip) needs of the other handles
struct slx_aligner;
struct slx_bam;
int slx_aligner_device_of(const slx_aligner *al);          // the device of a single-device aligner; -1 for a group handle
// the reads slx_bam_reads_device last unpacked for the batch whose d_stream is batch_d_stream: bases, offsets, record of read (all in HBM) and their number; false when there are none
bool slx_reader_device_reads(const slx_bam *rd, const void *batch_d_stream, const void **d_bases, const void **d_offs, const int64_t **d_rec_of_read, int64_t *n_reads, int *device);

// what the read filter (slx_filter.hip) and the reader (slx_bam.hip) need of each other
struct slx_filter;
void slx_reader_set_filter(slx_bam *rd, slx_filter *f);          // nullptr detaches
// keep bytes of the n_rec records of s[0, n_bytes) (offsets rec, n_rec + 1 of them) into d_keep, all in the HBM of `device`, on `stream` (a hipStream_t), which has
// drained when the call returns; *n_kept where not null.  SLX_EIO: a record's fields pass its block_size
int slx_filter_eval_device(slx_filter *f, int device, void *stream, const uint8_t *s, const uint64_t *rec, uint64_t n_rec, uint64_t n_bytes, uint8_t *d_keep, uint64_t *n_kept);
