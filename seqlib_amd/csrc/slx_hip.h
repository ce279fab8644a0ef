// slx_hip.h -- the host-side HIP plumbing the translation units of libseqlib_amd.so share: the error macros, the grow-only device and pinned buffers, the event
// timer, hipCUB's exclusive sum with its temporary storage, and the device preamble of the handles.  Host code only; included from .hip files and their internal
// headers.  Nothing here is part of the C-ABI.  DESIGN.md section 9.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <cstddef>
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
        if (*p) (void)hipFree(*p);
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
    }
    *p = q; *cap = want;
    return SLX_OK;
}

// *p becomes `want` bytes of pinned host memory; the contents go.  Pinned: what a copy to or from the device reads or writes without a staging copy, and what a
// kernel's results can come down into while the host waits on the stream only.
static inline int slx_pin_realloc(void **p, size_t *cap, size_t want)
{
    if (*p) (void)hipHostFree(*p);
    *p = nullptr; *cap = 0;
    const hipError_t e = hipHostMalloc(p, want, hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); *p = nullptr; slx_set_error("cannot pin %zu bytes (%s)", want, hipGetErrorString(e)); return SLX_ENOMEM; }
    *cap = want;
    return SLX_OK;
}

// A grow-only block of HBM.  No destructor: the owner releases it, after the stream that uses it has drained.
template <class Grow> struct SlxDevBuf {
    void *p = nullptr; size_t cap = 0;
    int ensure(size_t n) { return n <= cap ? SLX_OK : slx_dev_realloc(&p, &cap, Grow::want(n), nullptr, 0); }          // the contents may go
    int ensure(size_t n, hipStream_t st, size_t keep) { return n <= cap ? SLX_OK : slx_dev_realloc(&p, &cap, Grow::want(n), st, keep); }          // keep: leading bytes that survive a growth
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <typename T> T *as() const { return (T *)p; }
};
// ... and one of pinned host memory
template <class Grow> struct SlxPinBuf {
    void *p = nullptr; size_t cap = 0;
    int ensure(size_t n) { return n <= cap ? SLX_OK : slx_pin_realloc(&p, &cap, Grow::want(n)); }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    template <typename T> T *as() const { return (T *)p; }
};

// ------------------------------------------------------------------ events
// between two recorded events whose stream has drained; 0 when the runtime cannot say
static inline float slx_ev_ms(hipEvent_t a, hipEvent_t b) { float ms = 0; return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f; }
static inline float slx_ev_us(hipEvent_t a, hipEvent_t b) { return slx_ev_ms(a, b) * 1000.f; }

// ------------------------------------------------------------------ hipCUB's exclusive sum
// bytes of temporary storage the sum of n items asks for (hipCUB's rocPRIM backend forwards the count as a size_t whatever type it is given)
template <class In, class Out> static inline int slx_exclusive_sum_bytes(In in, Out out, size_t n, hipStream_t st, size_t *bytes)
{
    *bytes = 0;
    SLX_HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, in, out, n, st));
    return SLX_OK;
}
// out[i] = in[0] + ... + in[i - 1] for i < n, enqueued on st; tmp is made to hold hipCUB's temporary storage and `slack` bytes more (what the caller's unit has
// always added to the figure: kept as found)
template <class Buf, class In, class Out> static inline int slx_exclusive_sum(Buf &tmp, In in, Out out, size_t n, hipStream_t st, size_t slack = 0)
{
    size_t tb = 0;
    SLX_CHK(slx_exclusive_sum_bytes(in, out, n, st, &tb));
    SLX_CHK(tmp.ensure(tb + slack));
    SLX_HIPCHK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, in, out, n, st));
    return SLX_OK;
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
