// slx_hip.h -- the host-side HIP plumbing the translation units of libseqlib_amd.so share: the error macros, the grow-only device and pinned buffers and
// their tally, the event timer, one runner for hipCUB calls with their temporary storage, the device context of a handle (device, stream, events, owned buffers:
// SlxGpu), the intake of a batch of records and the two-pass add of the units that list their long records.  Host code only; included from .hip files and their internal
// headers.  Nothing here is part of the C-ABI.  DESIGN.md section 9.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "slx_internal.h"

// A HIP call that failed ends the function: out of memory is SLX_ENOMEM, anything else SLX_ENODEVICE; the message carries the expression.
#define SLX_HIPCHK(x)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) {                                                                     \
            slx_set_error("HIP error %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__, __LINE__, #x); \
            return e_ == hipErrorOutOfMemory ? SLX_ENOMEM : SLX_ENODEVICE;                          \
        }                                                                                           \
    } while (0)
#define SLX_CHK(x) do { const int rc_ = (x); if (rc_ != SLX_OK) return rc_; } while (0)

// ------------------------------------------------------------------ buffers
// The tallies of slx_internal.h: bytes held through SlxDevBuf / SlxPinBuf right now, what a test of create and free reads (slx_hip_live_bytes).
static inline void slx_live(std::atomic<int64_t> &t, size_t taken, size_t given_back) { t.fetch_add((int64_t)taken - (int64_t)given_back, std::memory_order_relaxed); }
// How much a buffer asks for when n bytes no longer fit.  The policy belongs to the buffer's type: every owner names its own once, by alias.
struct SlxExact { static size_t want(size_t n) { return n; } };
template <size_t DIV, size_t PAD> struct SlxMargin { static size_t want(size_t n) { return n + n / DIV + PAD; } };
// *p becomes a block of `want` bytes of HBM.  keep: the leading bytes of the old block that survive (copied on st, which has drained on return); without any the
// old block goes first -- deliberately: the two never stand side by side in HBM, and a growth that fails leaves the buffer empty (p null, cap 0), not as it was.
// The new block is freed on every failure path; with keep the old one then stands as it was.  A failed allocation is SLX_ENOMEM whatever the runtime calls it.
static inline int slx_dev_realloc(void **p, size_t *cap, size_t want, hipStream_t st, size_t keep)
{
    if (!*p) keep = 0;
    if (!keep) {
        if (*p) { (void)hipFree(*p); slx_live(slx_live_dev, 0, *cap); }
        *p = nullptr; *cap = 0;
    }
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, want);
    if (e != hipSuccess) { (void)hipGetLastError(); slx_set_error("cannot allocate %zu bytes of HBM (%s)", want, hipGetErrorString(e)); return SLX_ENOMEM; }
    if (keep) {
        e = hipMemcpyAsync(q, *p, keep, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { (void)hipFree(q); SLX_HIPCHK(e); }
        (void)hipFree(*p);
        slx_live(slx_live_dev, 0, *cap);
    }
    *p = q; *cap = want;
    slx_live(slx_live_dev, want, 0);
    return SLX_OK;
}

// *p becomes `want` bytes of pinned host memory; the contents go.  Pinned: what a copy to or from the device reads or writes without a staging copy, and what a
// kernel's results can come down into while the host waits on the stream only.
static inline int slx_pin_realloc(void **p, size_t *cap, size_t want)
{
    if (*p) { (void)hipHostFree(*p); slx_live(slx_live_pin, 0, *cap); }
    *p = nullptr; *cap = 0;
    const hipError_t e = hipHostMalloc(p, want, hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); *p = nullptr; slx_set_error("cannot pin %zu bytes (%s)", want, hipGetErrorString(e)); return SLX_ENOMEM; }
    *cap = want;
    slx_live(slx_live_pin, want, 0);
    return SLX_OK;
}

// ------------------------------------------------------------------ owned buffers
struct SlxBuf;
// What the buffers of one handle (or of one call's scratch) hang on: a buffer constructed with its owner links itself in, and release_bufs releases them all.
struct SlxBufOwner {
    SlxBuf *bufs = nullptr;
    inline void release_bufs();
};
// A grow-only block.  No destructor: the owner releases it, after the stream that uses it has drained.  Not copied: the owner's list holds its address.
struct SlxBuf {
    void *p = nullptr; size_t cap = 0;
    SlxBuf *next = nullptr;
    const bool pinned;
    SlxBuf(bool pin, SlxBufOwner *o) : pinned(pin) { if (o) { next = o->bufs; o->bufs = this; } }
    SlxBuf(const SlxBuf &) = delete;
    SlxBuf &operator=(const SlxBuf &) = delete;
    void release()
    {
        if (p) { (void)(pinned ? hipHostFree(p) : hipFree(p)); slx_live(pinned ? slx_live_pin : slx_live_dev, 0, cap); }
        p = nullptr; cap = 0;
    }
    template <typename T> T *as() const { return (T *)p; }
};
inline void SlxBufOwner::release_bufs() { for (SlxBuf *b = bufs; b; b = b->next) b->release(); }
// ... of HBM: `SlxDevBuf<G> d_x{gpu}` belongs to gpu, `SlxDevBuf<G> d_x` to whoever releases it by name
template <class Grow> struct SlxDevBuf : SlxBuf {
    SlxDevBuf() : SlxBuf(false, nullptr) {}
    SlxDevBuf(SlxBufOwner &o) : SlxBuf(false, &o) {}
    int ensure(size_t n) { return n <= cap ? SLX_OK : slx_dev_realloc(&p, &cap, Grow::want(n), nullptr, 0); }          // the contents may go
    int ensure(size_t n, hipStream_t st, size_t keep) { return n <= cap ? SLX_OK : slx_dev_realloc(&p, &cap, Grow::want(n), st, keep); }          // keep: leading bytes that survive a growth
};
// ... and of pinned host memory
template <class Grow> struct SlxPinBuf : SlxBuf {
    SlxPinBuf() : SlxBuf(true, nullptr) {}
    SlxPinBuf(SlxBufOwner &o) : SlxBuf(true, &o) {}
    int ensure(size_t n) { return n <= cap ? SLX_OK : slx_pin_realloc(&p, &cap, Grow::want(n)); }
};

// ------------------------------------------------------------------ events
// between two recorded events whose stream has drained; 0 when the runtime cannot say
static inline float slx_ev_ms(hipEvent_t a, hipEvent_t b) { float ms = 0; return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f; }
static inline float slx_ev_us(hipEvent_t a, hipEvent_t b) { return slx_ev_ms(a, b) * 1000.f; }

// ------------------------------------------------------------------ hipCUB
// One hipCUB call with its temporary storage: run(nullptr, bytes) asks for the size, tmp is made to hold it and `slack` bytes more (what the caller's unit has
// always added to the figure: kept as found), run(tmp.p, bytes) enqueues the work.  run binds the stream and every other argument; what names the call in the
// message of a failure (the lambda hides the expression from SLX_HIPCHK).
template <class Buf, class Run> static inline int slx_cub(const char *what, Buf &tmp, size_t slack, Run run)
{
    size_t bytes = 0;
    hipError_t e = run((void *)nullptr, bytes);
    if (e == hipSuccess) {
        SLX_CHK(tmp.ensure(bytes + slack));
        e = run(tmp.p, bytes);
    }
    if (e == hipSuccess) return SLX_OK;
    slx_set_error("HIP error %s in %s", hipGetErrorString(e), what);
    return e == hipErrorOutOfMemory ? SLX_ENOMEM : SLX_ENODEVICE;
}
// out[i] = in[0] + ... + in[i - 1] for i < n, enqueued on st (hipCUB's rocPRIM backend forwards the count as a size_t whatever type it is given)
template <class Buf, class In, class Out> static inline int slx_exclusive_sum(Buf &tmp, In in, Out out, size_t n, hipStream_t st, size_t slack = 0)
{
    return slx_cub("hipcub::DeviceScan::ExclusiveSum", tmp, slack, [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, in, out, n, st); });
}

// ------------------------------------------------------------------ the device of a handle
// SLX_OK and the number of visible devices; without one the caller's sentence (there is no CPU fallback anywhere) and SLX_ENODEVICE
static inline int slx_count_devices(const char *no_device_msg, int *ndev)
{
    *ndev = 0;
    if (hipGetDeviceCount(ndev) != hipSuccess || *ndev <= 0) {
        (void)hipGetLastError();
        slx_set_error("%s", no_device_msg);
        return SLX_ENODEVICE;
    }
    return SLX_OK;
}
// the device a handle is created on: device < 0 is the current one; SLX_EINVAL for one that is not there.  It is the calling thread's device on return.
static inline int slx_pick_device(int device, const char *no_device_msg, const char *who, int *device_out)
{
    int ndev = 0;
    SLX_CHK(slx_count_devices(no_device_msg, &ndev));
    if (device < 0) SLX_HIPCHK(hipGetDevice(&device));
    if (device >= ndev) { slx_set_error("%s: device %d is not one of the %d visible", who, device, ndev); return SLX_EINVAL; }
    SLX_HIPCHK(hipSetDevice(device));
    *device_out = device;
    return SLX_OK;
}

// ------------------------------------------------------------------ the device context of a handle
// The device, the stream, the events and the owned buffers of one handle.  open's sentence is the message of a create without a device (it may name the file that is
// not created); the constructor's is need()'s.  N events: most units time one span (2), the SAM writer two overlapping ones (4).
template <int N = 2> struct SlxGpu : SlxBufOwner {
    int device = -1;          // -1: host only, or not opened
    hipStream_t st = nullptr;
    hipEvent_t ev[N] = {};
    const char *const no_device;          // what need() says on a host-only handle: the unit's sentence, a constant; units without host-only handles give none
    explicit SlxGpu(const char *no_device_sentence = "no HIP device") : no_device(no_device_sentence) {}

    // device < 0 is the current one.  host_only_ok: with device < 0 and no visible device the handle stays host only (SLX_OK, device -1); otherwise no device is
    // SLX_ENODEVICE with the sentence, and a device that is not there SLX_EINVAL
    int open(int dev, const char *who, const char *no_device_sentence, bool host_only_ok = false)
    {
        int ndev = 0;
        if (host_only_ok && dev < 0 && (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)) { (void)hipGetLastError(); device = -1; return SLX_OK; }
        SLX_CHK(slx_pick_device(dev, no_device_sentence, who, &device));
        SLX_HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        for (auto &e : ev) SLX_HIPCHK(hipEventCreate(&e));
        return SLX_OK;
    }
    // before a kernel entry point does anything: the handle's device is the calling thread's, or SLX_ENODEVICE with the unit's sentence
    int need(const char *who)
    {
        if (device < 0) { slx_set_error("%s: %s", who, no_device); return SLX_ENODEVICE; }
        SLX_HIPCHK(hipSetDevice(device));
        return SLX_OK;
    }
    // the stream drains, then the buffers, the events and the stream go; safe on a context that open left half made, and a second time
    void close()
    {
        if (device >= 0) {
            (void)hipSetDevice(device);
            if (st) (void)hipStreamSynchronize(st);
        }
        release_bufs();
        for (auto &e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
        if (st) (void)hipStreamDestroy(st);
        st = nullptr;
    }
};
// need() for a handle the caller may have passed as null
template <class H> static inline int slx_need(H *h, const char *who)
{
    if (!h) { slx_set_error("%s: null object", who); return SLX_EINVAL; }
    return h->need(who);
}
// The body of a create entry point: a new H, impl(h) fills it, a failure frees it with the unit's own free, *out is the handle or null
template <class H, class Impl> static inline int slx_create(H **out, void (*free_fn)(H *), Impl impl)
{
    *out = nullptr;
    H *h = new H();
    const int rc = impl(h);
    if (rc != SLX_OK) { free_fn(h); return rc; }
    *out = h;
    return SLX_OK;
}

// ------------------------------------------------------------------ a batch of records
// block_size-prefixed BAM records and their offset table (n + 1 entries), on the host or already in HBM: the argument check every unit's add entry points share ...
static inline int slx_batch_args(const char *who, const void *s, int64_t n_bytes, const void *off, int64_t n)
{
    if (n_bytes < 0 || n < 0 || (n_bytes && !s) || (n && !off)) { slx_set_error("%s: null or negative argument", who); return SLX_EINVAL; }
    return SLX_OK;
}
// ... and a host batch (n > 0) on its way into the handle's d_in / d_off on st; pad: the bytes a unit's kernels may read behind the stream's end
template <class Buf> static inline int slx_batch_stage(Buf &d_in, Buf &d_off, size_t pad, const void *s, int64_t n_bytes, const uint64_t *off, int64_t n, hipStream_t st)
{
    SLX_CHK(d_in.ensure((size_t)n_bytes + pad)); SLX_CHK(d_off.ensure(8 * ((size_t)n + 1)));
    if (n_bytes) SLX_HIPCHK(hipMemcpyAsync(d_in.p, s, (size_t)n_bytes, hipMemcpyHostToDevice, st));
    SLX_HIPCHK(hipMemcpyAsync(d_off.p, off, 8 * ((size_t)n + 1), hipMemcpyHostToDevice, st));
    return SLX_OK;
}

// ------------------------------------------------------------------ a two-pass add
// What the units that add a batch in two passes share (coverage, pileup): a lane kernel over all the records, which lists the long ones, then a wave kernel over
// that list.  The device counters of one add stand in this order (a unit's own come behind SLX_ADD_N), and the members below are the part of the handle the
// add works on.
enum { SLX_ADD_ERR = 0, SLX_ADD_NLONG, SLX_ADD_COUNTED, SLX_ADD_LDS, SLX_ADD_GLOBAL, SLX_ADD_N };
struct SlxTwoPass : SlxGpu<> {
    explicit SlxTwoPass(const char *no_device_sentence) : SlxGpu(no_device_sentence) {}
    SlxDevBuf<SlxMargin<4, 256>> d_long{*this}, d_cnt{*this};          // the long list; the counters (the unit's create makes d_cnt and h_cnt)
    SlxPinBuf<SlxMargin<4, 256>> h_cnt{*this};
    int64_t c_seen = 0, c_counted = 0, c_long = 0, c_lds = 0, c_global = 0;
    double us_add = 0;
};
// The n > 0 records of a batch: the n_cnt counters are reset, lane_pass() launches the lane kernel (a record it refuses ends the call), long_pass(n_long) the wave
// kernel when anything was listed; the span is timed and tallied.  unit: what the sentences begin with.  The stream has drained on return.
template <class LanePass, class LongPass> static inline int slx_two_pass_add(SlxTwoPass &h, const char *unit, uint64_t n, int n_cnt, LanePass lane_pass, LongPass long_pass)
{
    typedef unsigned long long ull;
    if (n >= 0x7fffffffull) { slx_set_error("%s: 2^31 records or more in one batch", unit); return SLX_EUNSUPPORTED; }
    hipStream_t st = h.st;
    SLX_CHK(h.d_long.ensure(8 * n));
    ull *hc = h.h_cnt.template as<ull>(), *dc = h.d_cnt.template as<ull>();
    memset(hc, 0, 8 * (size_t)n_cnt);
    hc[SLX_ADD_ERR] = ~0ull;
    SLX_HIPCHK(hipMemcpyAsync(dc, hc, 8 * (size_t)n_cnt, hipMemcpyHostToDevice, st));
    SLX_HIPCHK(hipEventRecord(h.ev[0], st));
    lane_pass();
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipMemcpyAsync(hc, dc, 8 * (size_t)n_cnt, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    if (hc[SLX_ADD_ERR] != ~0ull) {
        slx_set_error("%s: record %llu of the batch: its fields pass its block_size, or its extent is not block_size + 4 inside the stream", unit, hc[SLX_ADD_ERR]);
        return SLX_EIO;
    }
    const uint64_t n_long = hc[SLX_ADD_NLONG];
    if (n_long) {
        long_pass(n_long);
        SLX_HIPCHK(hipGetLastError());
        SLX_HIPCHK(hipMemcpyAsync(hc, dc, 8 * (size_t)n_cnt, hipMemcpyDeviceToHost, st));
    }
    SLX_HIPCHK(hipEventRecord(h.ev[1], st));
    SLX_HIPCHK(slx_wait_stream(st));
    h.us_add += slx_ev_us(h.ev[0], h.ev[1]);
    h.c_seen += (int64_t)n; h.c_counted += (int64_t)hc[SLX_ADD_COUNTED]; h.c_long += (int64_t)n_long; h.c_lds += (int64_t)hc[SLX_ADD_LDS]; h.c_global += (int64_t)hc[SLX_ADD_GLOBAL];
    return SLX_OK;
}
