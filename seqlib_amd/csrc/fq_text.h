// fq_text.h -- where the bytes of a text file come from, for the readers that parse text on the GPU (slx_fastq.hip, slx_sam.hip): plain text read and gzip inflated
// (zlib, one DEFLATE stream is serial) by a producer thread into pinned slots, BGZF members inflated and CRC-checked on the GPU (slx_bgzf_inflate_members), the window
// of text in HBM, and its line starts (k_fq_count / k_fq_lines).  DESIGN.md section 9.6.  The functions are defined in slx_fastq.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>
#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "slx_internal.h"
#include "seqlib_amd_bam.h"
#include "slx_hip.h"
#include "dev_inflate.h"

typedef unsigned long long fq_u64;
// ------------------------------------------------------------------ host: buffers
// the text readers' buffers in HBM and pinned: a margin of 1/4 + 256 bytes on every growth, kept as found
typedef SlxDevBuf<SlxMargin<4, 256>> FqDBuf;
typedef SlxPinBuf<SlxMargin<4, 256>> FqHBuf;

// ------------------------------------------------------------------ host: the producer of a plain or gzip file's bytes
// A thread of its own reads (plain) or inflates (gzip: one DEFLATE stream is serial) the next chunks into pinned slots while the batch before is on the GPU.
struct FqProducer {
    static constexpr int NSLOT = 3;
    struct Slot { uint8_t *p = nullptr; size_t n = 0; bool eof = false, err = false; };
    Slot slot[NSLOT];
    size_t chunk = 8u << 20;
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    int head = 0, tail = 0, count = 0;
    bool stop = false, running = false;
    int fd = -1;
    gzFile gz = nullptr;
    size_t tail_pos = 0;          // bytes of slot[tail] already taken

    void run()
    {
        for (;;) {
            {
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&] { return stop || count < NSLOT; });
                if (stop) return;
            }
            Slot &s = slot[head];
            s.n = 0; s.eof = false; s.err = false;
            while (s.n < chunk) {
                long r;
                if (gz) r = gzread(gz, s.p + s.n, (unsigned)std::min<size_t>(chunk - s.n, 1u << 30));
                else r = (long)::read(fd, s.p + s.n, chunk - s.n);
                if (r < 0) { s.err = true; break; }
                if (r == 0) { s.eof = true; break; }
                s.n += (size_t)r;
            }
            const bool last = s.eof || s.err;
            {
                std::lock_guard<std::mutex> g(mu);
                head = (head + 1) % NSLOT; ++count;
            }
            cv.notify_all();
            if (last) return;
        }
    }
    void halt()
    {
        if (running) {
            { std::lock_guard<std::mutex> g(mu); stop = true; }
            cv.notify_all();
            th.join();
            running = false;
        }
        if (gz) { gzclose(gz); gz = nullptr; fd = -1; }
        if (fd >= 0) { ::close(fd); fd = -1; }
        head = tail = count = 0; stop = false; tail_pos = 0;
    }
    int start(const std::string &path, bool gzip)
    {
        halt();
        fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) { slx_set_error("text reader: cannot open '%s'", path.c_str()); return SLX_EIO; }
        if (gzip) {
            gz = gzdopen(fd, "r");
            if (!gz) { ::close(fd); fd = -1; slx_set_error("text reader: zlib cannot open '%s'", path.c_str()); return SLX_EIO; }
            gzbuffer(gz, 1u << 20);
        }
        for (Slot &s : slot)
            if (!s.p && hipHostMalloc((void **)&s.p, chunk, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); s.p = nullptr; slx_set_error("text reader: cannot pin %zu bytes", chunk); return SLX_ENOMEM; }
        th = std::thread([this] { run(); });
        running = true;
        return SLX_OK;
    }
    // the slot to take bytes from (blocks until the producer has one)
    Slot &front()
    {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return count > 0; });
        return slot[tail];
    }
    void pop()
    {
        { std::lock_guard<std::mutex> g(mu); tail = (tail + 1) % NSLOT; --count; tail_pos = 0; }
        cv.notify_all();
    }
    void release() { halt(); for (Slot &s : slot) { if (s.p) (void)hipHostFree(s.p); s.p = nullptr; } }
};

// ------------------------------------------------------------------ the source and the text window
struct FqText : SlxGpu<10> {          // the device, the stream and the events; a reader built on it hangs its own buffers on it too
    const char *who = "FASTQ reader";          // the reader's name in messages
    std::string path;
    int source = 0;                            // 0 plain, 1 BGZF, 2 gzip
    // BGZF: the file mapped, its members
    int fd = -1; const uint8_t *map = nullptr; uint64_t fsize = 0;
    std::vector<slx_bam_member> mem; int64_t next_member = 0;
    FqProducer prod;
    // the text window: d_text[cur][used, have) is text not yet delivered, [0, used) has been
    FqDBuf d_text[2] = {*this, *this}; int cur = 0; uint64_t have = 0, used = 0; bool src_eof = false;
    uint32_t tile_bytes = 4096;
    bgzf_stage stage;                    // slx_bgzf_inflate_members' buffers
    FqDBuf d_count{*this}, d_base{*this}, d_tmp{*this}, d_line{*this};
    FqHBuf h_small{*this};
    float us[4] = {0, 0, 0, 0};          // lines, check, gather, inflate
    int64_t c_members = 0;               // BGZF members inflated since the last fq_text_start
    std::vector<FqDBuf *> text_dbufs() { return {&d_text[0], &d_text[1], &d_count, &d_base, &d_tmp, &d_line}; }          // for a reader that gives the window back early (slx_ref.hip)
};

// the kind of source from the file's first bytes, the BGZF member table, the device, the stream and the events.  SLX_ENODEVICE without a GPU
int fq_text_open(FqText *t, const char *path, int device);
// everything fq_text_open and the calls after it took (not t itself)
void fq_text_free(FqText *t);
// (again) at the start of the source
int fq_text_start(FqText *t);
// at least `want` more bytes of text (fewer only at the end of the source) behind d_text[cur][have)
int fq_pull(FqText *t, uint64_t want);
// the cut tail d_text[cur][used, have) moves to the front of the other buffer, which is made to hold room bytes behind it
int fq_shift(FqText *t, uint64_t room);
// exclusive sum of n values on the reader's stream
static inline int fq_scan(FqText *t, const fq_u64 *in, fq_u64 *out, uint64_t n) { return slx_exclusive_sum(t->d_tmp, in, out, n, t->st, 16); }
// d_line = the line starts of d_text[cur][0, have): *n_lines + 1 entries, entry 0 = 0, entry 1 + j = the byte behind line feed j; at the end of the source a last line
// without a line feed counts (*virt = 1, its entry have + 1).  Returns after the stream has drained up to the count (the starts themselves may still be in flight).
int fq_line_starts(FqText *t, uint64_t *n_lines, int *virt);
