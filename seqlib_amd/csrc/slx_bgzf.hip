// slx_bgzf.hip -- the BamWriter path of libseqlib_amd.so (include/seqlib_amd_bam.h, slx_bgzf_*): a BGZF writer whose DEFLATE, CRC32 and framing run on the
// GPU.  The host cuts nothing and compresses nothing: it stages bytes into HBM, and what comes down is file bytes.
//   k_bgzf_deflate   one wave per member: bytes [i * 0xff00, ...) of the staged segment into slot i (64 KiB) as header + DEFLATE stream     dev_deflate.h
//   k_bgzf_trailer   one wave per member: CRC32 of the member's input by slices (the body of k_bgzf_crc), CRC32 + ISIZE behind the stream   dev_inflate.h
//   k_bgzf_pack      one block per member: slot i to its place in the file (hipCUB's exclusive sum of the sizes), as k_bam_gather moves records
// Members map to waves statically (wave i owns member i), as in k_bgzf_inflate: no work queue.
// Two input segments: while one is compressed, copied down and written by the writer's worker thread, the caller stages into the other.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include "slx_internal.h"
#include "seqlib_amd_bam.h"
#include "dev_deflate.h"
#include "slx_hip.h"

#define BGZF_SLOT 65536u

typedef unsigned long long ull;

// ------------------------------------------------------------------ kernels
// size[i] = bytes of member i in its slot (0 on an error); flag[i] = stored | error code << 8
__global__ __launch_bounds__(64) void k_bgzf_deflate(const uint8_t *in, uint64_t in_bytes, int n, uint8_t *slots, uint32_t *tok, ull *size, uint32_t *flag)
{
    __shared__ def_state st;
    const int idx = blockIdx.x, lane = threadIdx.x;
    if (idx >= n) return;
    const uint64_t off = (uint64_t)idx * DEF_MEMBER;
    const uint32_t len = in_bytes - off < DEF_MEMBER ? (uint32_t)(in_bytes - off) : DEF_MEMBER;
    uint8_t *slot = slots + (uint64_t)idx * BGZF_SLOT;
    uint32_t out_len = 0, stored = 0;
    const int e = def_member(in + off, len, slot + 18, BGZF_SLOT - 18 - 8, tok + off, &st, lane, 64, &out_len, &stored);
    if (lane == 0) {
        if (e == DEF_OK) def_bgzf_header(slot, 18 + out_len + 8);
        size[idx] = e == DEF_OK ? 18 + out_len + 8 : 0;
        flag[idx] = stored | (uint32_t)e << 8;
        if (idx == 0) size[n] = 0;
    }
}

__global__ __launch_bounds__(256) void k_bgzf_trailer(const uint8_t *in, uint64_t in_bytes, int n, uint8_t *slots, const ull *size)
{
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = inf_crc_entry(threadIdx.x);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int idx = blockIdx.x * 4 + wave;
    if (idx >= n) return;
    const uint32_t sz = (uint32_t)size[idx];
    if (sz < 26 || sz > BGZF_SLOT) return;
    const uint64_t off = (uint64_t)idx * DEF_MEMBER;
    const uint32_t len = in_bytes - off < DEF_MEMBER ? (uint32_t)(in_bytes - off) : DEF_MEMBER;
    uint32_t c = inf_crc_part(tab, in + off, len, lane, 64);
    for (int o = 32; o; o >>= 1) c ^= __shfl_xor(c, o, 64);
    if (lane == 0) def_bgzf_trailer(slots + (uint64_t)idx * BGZF_SLOT + sz - 8, c, len);
}

__global__ __launch_bounds__(256) void k_bgzf_pack(const uint8_t *slots, int n, const ull *size, const ull *off, uint8_t *dst, uint64_t dst_bytes)
{
    const int idx = blockIdx.x;
    if (idx >= n) return;
    const uint64_t sz = size[idx], o = off[idx];
    if (sz > BGZF_SLOT || o + sz > dst_bytes) return;
    const uint8_t *s = slots + (uint64_t)idx * BGZF_SLOT;
    for (uint64_t i = threadIdx.x; i < sz; i += 256) dst[o + i] = s[i];
}

// ------------------------------------------------------------------ host
// no margin: the writer's buffers are computed from batch_bytes (the token arena is four bytes per input byte), so a batch never asks for more than the first did
typedef SlxDevBuf<SlxExact> DBuf;
typedef SlxPinBuf<SlxExact> HBuf;

static const unsigned char BGZF_EOF[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

struct slx_bgzf : SlxGpu<4> {          // st is the worker's stream
    FILE *fp = nullptr;
    bool is_stdout = false;
    std::string path;
    hipStream_t st_stage = nullptr;          // the caller's copies into d_in: the unit's own, beside the context's
    int64_t batch_bytes = 64ll << 20;
    DBuf d_in[2] = {*this, *this};                  // the two input segments
    int cur = 0;                    // the one being filled
    uint64_t fill = 0;
    // the worker's buffers: one batch is compressed at a time
    DBuf d_slots{*this}, d_tok{*this}, d_size{*this}, d_off{*this}, d_flag{*this}, d_tmp{*this}, d_pack{*this};
    HBuf h_pack{*this}, h_flag{*this}, h_total{*this};
    std::thread worker;
    bool worker_on = false;
    int worker_rc = SLX_OK;         // of the batch in flight; read after join
    std::string worker_msg;
    int err = SLX_OK;               // the first error of the writer's life
    std::string err_msg;
    int64_t c_members = 0, c_stored = 0, c_in = 0, c_out = 0;
    double us[3] = {0, 0, 0};
};

static int bgzf_fail(slx_bgzf *w, int rc)         // keeps the first error and its text (slx_last_error() is per thread: the text travels with the writer)
{
    if (w->err == SLX_OK) { w->err = rc; w->err_msg = slx_last_error(); }
    return rc;
}
static int bgzf_sticky(slx_bgzf *w) { slx_set_error("%s", w->err_msg.c_str()); return w->err; }

// the worker: d_in[set][0, bytes) -> members -> file
static int bgzf_compress(slx_bgzf *w, int set, uint64_t bytes)
{
    SLX_HIPCHK(hipSetDevice(w->device));
    const int n = (int)((bytes + DEF_MEMBER - 1) / DEF_MEMBER);
    hipStream_t st = w->st;
    SLX_CHK(w->d_slots.ensure((size_t)n * BGZF_SLOT));
    SLX_CHK(w->d_tok.ensure((size_t)n * DEF_MEMBER * 4));          // the token arena, computed from the batch: one token per input byte at most
    SLX_CHK(w->d_size.ensure(sizeof(ull) * ((size_t)n + 1)));
    SLX_CHK(w->d_off.ensure(sizeof(ull) * ((size_t)n + 1)));
    SLX_CHK(w->d_flag.ensure(4 * (size_t)n));
    SLX_CHK(w->d_pack.ensure((size_t)n * BGZF_SLOT));
    SLX_CHK(w->h_pack.ensure((size_t)n * BGZF_SLOT));
    SLX_CHK(w->h_flag.ensure(4 * (size_t)n));
    SLX_CHK(w->h_total.ensure(sizeof(ull)));
    const uint8_t *in = w->d_in[set].as<uint8_t>();
    SLX_HIPCHK(hipEventRecord(w->ev[0], st));
    k_bgzf_deflate<<<n, 64, 0, st>>>(in, bytes, n, w->d_slots.as<uint8_t>(), w->d_tok.as<uint32_t>(), w->d_size.as<ull>(), w->d_flag.as<uint32_t>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(w->ev[1], st));
    k_bgzf_trailer<<<(n + 3) / 4, 256, 0, st>>>(in, bytes, n, w->d_slots.as<uint8_t>(), w->d_size.as<ull>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(w->ev[2], st));
    SLX_CHK(slx_exclusive_sum(w->d_tmp, w->d_size.as<ull>(), w->d_off.as<ull>(), (size_t)n + 1, st));
    k_bgzf_pack<<<n, 256, 0, st>>>(w->d_slots.as<uint8_t>(), n, w->d_size.as<ull>(), w->d_off.as<ull>(), w->d_pack.as<uint8_t>(), (uint64_t)n * BGZF_SLOT);
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(w->ev[3], st));
    SLX_HIPCHK(hipMemcpyAsync(w->h_total.p, w->d_off.as<ull>() + n, sizeof(ull), hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync(w->h_flag.p, w->d_flag.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipStreamSynchronize(st));
    const uint32_t *flag = w->h_flag.as<uint32_t>();
    int64_t stored = 0;
    for (int i = 0; i < n; ++i) {
        if (flag[i] >> 8) { slx_set_error("BGZF writer: internal: member %d of the batch did not encode (code %u)", i, flag[i] >> 8); return SLX_EINTERNAL; }
        stored += flag[i] & 1u;
    }
    const ull total = *w->h_total.as<ull>();
    if (total < 26ull * (ull)n || total > (ull)n * BGZF_SLOT) { slx_set_error("BGZF writer: internal: %llu bytes for %d members", total, n); return SLX_EINTERNAL; }
    SLX_HIPCHK(hipMemcpyAsync(w->h_pack.p, w->d_pack.p, total, hipMemcpyDeviceToHost, st));        // one copy of exactly the file bytes
    SLX_HIPCHK(hipStreamSynchronize(st));
    w->us[0] += slx_ev_us(w->ev[0], w->ev[1]); w->us[1] += slx_ev_us(w->ev[1], w->ev[2]); w->us[2] += slx_ev_us(w->ev[2], w->ev[3]);
    w->c_members += n; w->c_stored += stored; w->c_in += (int64_t)bytes; w->c_out += (int64_t)total;
    if (std::fwrite(w->h_pack.p, 1, total, w->fp) != total) { slx_set_error("BGZF writer: cannot write to '%s': %s", w->path.c_str(), strerror(errno)); return SLX_EIO; }
    return SLX_OK;
}

// waits for the batch in flight and takes its outcome
static int bgzf_join(slx_bgzf *w)
{
    if (!w->worker_on) return SLX_OK;
    w->worker.join();
    w->worker_on = false;
    if (w->worker_rc != SLX_OK) { slx_set_error("%s", w->worker_msg.c_str()); return bgzf_fail(w, w->worker_rc); }
    return SLX_OK;
}

// Hands the filled segment to the worker.  final: all of it, the last member short (a flush); otherwise its whole 0xff00 blocks, and the bytes behind them
// open the other segment.
static int bgzf_submit(slx_bgzf *w, bool final)
{
    const uint64_t take = final ? w->fill : w->fill / DEF_MEMBER * DEF_MEMBER, rest = w->fill - take;
    if (take == 0) return SLX_OK;
    SLX_CHK(bgzf_join(w));                  // the other segment is free once the batch before this one is in the file
    const int set = w->cur, other = set ^ 1;
    if (rest) {
        SLX_CHK(w->d_in[other].ensure(std::max<size_t>((size_t)w->batch_bytes, rest)));
        SLX_HIPCHK(hipMemcpyAsync(w->d_in[other].p, w->d_in[set].as<uint8_t>() + take, rest, hipMemcpyDeviceToDevice, w->st_stage));
        SLX_HIPCHK(hipStreamSynchronize(w->st_stage));
    }
    w->cur = other; w->fill = rest;
    w->worker_rc = SLX_OK;
    w->worker_on = true;
    w->worker = std::thread([w, set, take]() {
        w->worker_rc = bgzf_compress(w, set, take);
        if (w->worker_rc != SLX_OK) w->worker_msg = slx_last_error();
    });
    return SLX_OK;
}

static void bgzf_free(slx_bgzf *w)
{
    if (w->worker_on) { w->worker.join(); w->worker_on = false; }
    if (w->st_stage) {
        (void)hipSetDevice(w->device);
        if (w->st) (void)hipStreamSynchronize(w->st);
        (void)hipStreamSynchronize(w->st_stage);
    }
    w->close();
    if (w->st_stage) (void)hipStreamDestroy(w->st_stage);
    if (w->fp && !w->is_stdout) std::fclose(w->fp);
    delete w;
}

static int bgzf_open_impl(slx_bgzf *w, const char *path, int device)
{
    const std::string no_device = std::string("no HIP device: the BGZF writer compresses on MI355X only (no CPU fallback); '") + path + "' is not created";
    SLX_CHK(w->open(device, "BGZF writer", no_device.c_str()));
    w->path = path;
    w->is_stdout = w->path == "-";
    w->fp = w->is_stdout ? stdout : std::fopen(path, "wb");
    if (!w->fp) { slx_set_error("BGZF writer: cannot create '%s': %s", path, strerror(errno)); return SLX_EIO; }
    SLX_HIPCHK(hipStreamCreateWithFlags(&w->st_stage, hipStreamNonBlocking));
    return SLX_OK;
}

extern "C" int slx_bgzf_open(const char *path, int device, slx_bgzf **out)
{
    if (!path || !out) { slx_set_error("slx_bgzf_open: null argument"); return SLX_EINVAL; }
    return slx_create(out, bgzf_free, [&](slx_bgzf *w) { return bgzf_open_impl(w, path, device); });
}

static int bgzf_write_impl(slx_bgzf *w, const void *p, int64_t n, bool from_device)
{
    if (!w) { slx_set_error("slx_bgzf_write: null writer"); return SLX_EINVAL; }
    if (n < 0 || (n > 0 && !p)) { slx_set_error("slx_bgzf_write: %lld bytes from %p", (long long)n, p); return SLX_EINVAL; }
    if (w->err != SLX_OK) return bgzf_sticky(w);
    if (hipSetDevice(w->device) != hipSuccess) { slx_set_error("BGZF writer: cannot select device %d", w->device); return bgzf_fail(w, SLX_ENODEVICE); }
    const uint8_t *src = (const uint8_t *)p;
    while (n > 0) {
        const uint64_t cap = (uint64_t)w->batch_bytes;
        if (w->fill >= cap) { const int rc = bgzf_submit(w, false); if (rc != SLX_OK) return bgzf_fail(w, rc); continue; }
        const uint64_t take = std::min<uint64_t>((uint64_t)n, cap - w->fill);
        DBuf &d = w->d_in[w->cur];
        int rc = d.ensure((size_t)cap, w->st_stage, (size_t)w->fill);
        if (rc == SLX_OK && hipMemcpyAsync(d.as<uint8_t>() + w->fill, src, take, from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, w->st_stage) != hipSuccess) rc = SLX_ENODEVICE;
        if (rc == SLX_OK && hipStreamSynchronize(w->st_stage) != hipSuccess) rc = SLX_ENODEVICE;         // the caller's buffer is free when the call returns
        if (rc == SLX_ENODEVICE) slx_set_error("BGZF writer: HIP error %s while staging %llu bytes", hipGetErrorString(hipGetLastError()), (unsigned long long)take);
        if (rc != SLX_OK) return bgzf_fail(w, rc);
        w->fill += take; src += take; n -= (int64_t)take;
    }
    if (w->fill >= (uint64_t)w->batch_bytes) { const int rc = bgzf_submit(w, false); if (rc != SLX_OK) return bgzf_fail(w, rc); }
    return SLX_OK;
}

extern "C" int slx_bgzf_write(slx_bgzf *w, const void *p, int64_t n) { return bgzf_write_impl(w, p, n, false); }
extern "C" int slx_bgzf_write_device(slx_bgzf *w, const void *d_p, int64_t n) { return bgzf_write_impl(w, d_p, n, true); }

extern "C" int slx_bgzf_flush(slx_bgzf *w)
{
    if (!w) { slx_set_error("slx_bgzf_flush: null writer"); return SLX_EINVAL; }
    if (w->err != SLX_OK) return bgzf_sticky(w);
    if (hipSetDevice(w->device) != hipSuccess) { slx_set_error("BGZF writer: cannot select device %d", w->device); return bgzf_fail(w, SLX_ENODEVICE); }
    const int rc = bgzf_submit(w, true);
    return rc == SLX_OK ? SLX_OK : bgzf_fail(w, rc);
}

extern "C" int slx_bgzf_close(slx_bgzf *w)
{
    if (!w) { slx_set_error("slx_bgzf_close: null writer"); return SLX_EINVAL; }
    if (w->err == SLX_OK) (void)slx_bgzf_flush(w);
    const int jr = bgzf_join(w);
    (void)jr;
    if (w->err == SLX_OK) {
        bool ok = std::fwrite(BGZF_EOF, 1, 28, w->fp) == 28;
        if (w->is_stdout) ok = std::fflush(stdout) == 0 && ok; else { ok = std::fclose(w->fp) == 0 && ok; w->fp = nullptr; }
        if (!ok) { slx_set_error("BGZF writer: cannot write to '%s': %s", w->path.c_str(), strerror(errno)); bgzf_fail(w, SLX_EIO); }
    }
    const int rc = w->err;
    if (rc != SLX_OK) slx_set_error("%s", w->err_msg.c_str());
    bgzf_free(w);
    return rc;
}

extern "C" int slx_bgzf_set(slx_bgzf *w, const char *key, int64_t value)
{
    if (!w || !key) { slx_set_error("slx_bgzf_set: null argument"); return SLX_EINVAL; }
    if (!strcmp(key, "batch_bytes")) {
        if (value < (int64_t)DEF_MEMBER || value > (1ll << 31)) { slx_set_error("slx_bgzf_set: batch_bytes %lld outside [0xff00, 2^31]", (long long)value); return SLX_EINVAL; }
        w->batch_bytes = value;
        return SLX_OK;
    }
    slx_set_error("slx_bgzf_set: unknown key '%s'", key);
    return SLX_EINVAL;
}

extern "C" int64_t slx_bgzf_counter(const slx_bgzf *cw, const char *name)
{
    if (!cw || !name) return -1;
    slx_bgzf *w = const_cast<slx_bgzf *>(cw);
    (void)bgzf_join(w);                      // the figures of every batch handed over so far
    if (!strcmp(name, "members")) return w->c_members;
    if (!strcmp(name, "stored_members")) return w->c_stored;
    if (!strcmp(name, "bytes_in")) return w->c_in;
    if (!strcmp(name, "bytes_out")) return w->c_out;
    if (!strcmp(name, "us_deflate")) return (int64_t)w->us[0];
    if (!strcmp(name, "us_crc")) return (int64_t)w->us[1];
    if (!strcmp(name, "us_gather")) return (int64_t)w->us[2];
    return -1;
}
