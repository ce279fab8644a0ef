// slx_samw.hip -- SAM text written on the GPU (include/seqlib_amd_samw.h): block_size-prefixed BAM records in HBM -> SAM lines in HBM, then down as plain text or
// through the GPU BGZF writer.  DESIGN.md section 9.8 has the argument.  It is the SAM reader (slx_sam.hip) turned around; every record is independent of its
// neighbours:
//   k_samw_size       one lane per record: every refusal rule, the line's length, the field table, the verdict                      dev_samw.h samw_line, out == nullptr
//                     a record with more than SAMW_WIDE CIGAR ops or B elements is sized again by its whole wave, in the same kernel (the wave walks the lanes
//                     that hold one)
//   hipCUB            exclusive sum of the lengths: the line offsets; and of the extra waves that long records get
//   k_samw_fill       one wave per record: the short fields by lane 0, QNAME, CIGAR (64 ops at a time, places from the wave's scan), Z / H strings and B elements
//                     over the lanes, SEQ and QUAL over the lanes; a record of the slow path is copied from its staging place    dev_samw.h samw_line, out != nullptr
//   k_samw_fill_more  one wave per SAMW_PART bases beyond the first of a long record: SEQ and QUAL only                               dev_samw.h samw_bulk
// SLOW records (f, d, B:f fields: no floating-point text is printed on the GPU) come down, compacted by k_samw_gather, and go through samw_host.h one by one; their
// lengths go up into the size array before the scan and their text into a staging buffer.  The first ERROR record ends the call with its index and the rule.
// Waves and lanes take records by a static map: there is no work queue, and the only atomic is one atomicAdd per wave that holds a record which is not FAST or
// which was sized by the wave.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <fcntl.h>
#include <unistd.h>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "slx_internal.h"
#include "slx_hip.h"
#include "seqlib_amd_bam.h"
#include "seqlib_amd_samw.h"
#include "dev_samw.h"
#include "samw_host.h"

typedef unsigned long long ull;
#define SAMW_WIDE 256u            // CIGAR ops or B elements above which a record is sized by its wave
#define SAMW_PART 8192u           // bases per extra wave of a long record
#define SAMW_MAX_EXTRA 4095u
#define SAMW_STAGE (16ull << 20)  // bytes of text one pinned staging buffer holds (knob "stage_bytes")

// ------------------------------------------------------------------ kernels
// size[k] = bytes of record k's line when it is FAST, else 0; size[n] = 0; verdict[k] = verdict | error << 2; fld[k]; extra[k] = waves beyond the first that fill it;
// *cnt += records that are not FAST | records sized by the wave << 32
__global__ __launch_bounds__(256) void k_samw_size(const uint8_t *s, uint64_t n_bytes, const ull *rec_off, uint64_t n, samw_refs R, int fast_fail, ull *size, uint8_t *verdict, samw_fld *fld,
                                                   ull *extra, ull *cnt)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    int v = SAMW_FAST, err = SAMW_E_NONE;
    uint64_t sz = 0, b = 0, e = 0;
    samw_fld F = {};
    if (k < n) {
        b = rec_off[k]; e = rec_off[k + 1];
        if (b > e || e > n_bytes) { v = SAMW_ERROR; err = SAMW_E_SPAN; }
        else v = samw_line(s + b, e - b, R, &F, (uint8_t *)nullptr, &sz, &err, 0u, 1u, lanes_one(), samw_no_float(), SAMW_WIDE);
    }
    const ull wide = __ballot(v == SAMW_DEFER);
    for (ull m = wide; m; m &= m - 1ull) {          // (wave-uniform: all 64 lanes size the record of lane j together)
        const int j = __ffsll(m) - 1;
        const uint64_t bj = (uint64_t)__shfl((ull)b, j, 64), ej = (uint64_t)__shfl((ull)e, j, 64);
        samw_fld Fj = {};
        uint64_t szj = 0;
        int errj = SAMW_E_NONE;
        const int vj = samw_line(s + bj, ej - bj, R, &Fj, (uint8_t *)nullptr, &szj, &errj, lane, 64u, lanes_group<>(), samw_no_float(), SAMW_NO_DEFER);
        if ((int)lane == j) { v = vj; F = Fj; sz = szj; err = errj; }
    }
    if (k < n) {
        if (v == SAMW_FAST && fast_fail) v = SAMW_SLOW;
        const uint64_t x = F.l_seq / SAMW_PART;
        size[k] = v == SAMW_FAST ? sz : 0;
        extra[k] = v == SAMW_FAST ? (x < SAMW_MAX_EXTRA ? x : SAMW_MAX_EXTRA) : 0;
        verdict[k] = (uint8_t)(v | err << 2);
        fld[k] = F;
    } else if (k == n) { size[k] = 0; extra[k] = 0; }
    const ull other = __ballot(v != SAMW_FAST);
    if (lane == 0 && (other | wide)) atomicAdd(cnt, (ull)__popcll(other) | (ull)__popcll(wide) << 32);
}

// dst[to[j], to[j] + len[j]) = s[from[j], ...): the slow records one behind the other, one wave each.  g: from, len, to per record
__global__ __launch_bounds__(256) void k_samw_gather(const uint8_t *s, const ull *g, uint64_t m, uint8_t *dst)
{
    const uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= m) return;
    const uint8_t *p = s + g[3 * j];
    uint8_t *o = dst + g[3 * j + 2];
    for (uint64_t i = threadIdx.x & 63, nb = g[3 * j + 1]; i < nb; i += 64) o[i] = p[i];
}

// size[idx[j]] = len[j], src[idx[j]] = at[j]: the host's lines take their places.  g: idx, len, at per record
__global__ __launch_bounds__(256) void k_samw_slow_put(const ull *g, uint64_t m, ull *size, ull *src)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    size[g[3 * j]] = g[3 * j + 1]; src[g[3 * j]] = g[3 * j + 2];
}

// text[line[k], line[k + 1]) = the line of record k < n: built from the record, or copied from slow[src[k]] when the record is not FAST
__global__ __launch_bounds__(256) void k_samw_fill(const uint8_t *s, const ull *rec_off, uint64_t n, samw_refs R, const uint8_t *verdict, const samw_fld *fld, const ull *extra,
                                                   const uint8_t *slow, const ull *src, const ull *line, uint8_t *text)
{
    const uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (k >= n) return;
    uint8_t *o = text + line[k];
    if ((verdict[k] & 3) != SAMW_FAST) {
        const uint8_t *p = slow + src[k];
        const uint64_t nb = line[k + 1] - line[k];
        for (uint64_t i = lane; i < nb; i += 64) o[i] = p[i];
        return;
    }
    samw_fld F = fld[k];
    const uint8_t *r = s + rec_off[k];
    uint64_t sz = 0;
    int err;
    (void)samw_line(r, rec_off[k + 1] - rec_off[k], R, &F, o, &sz, &err, lane, 64u, lanes_group<>(), samw_no_float(), SAMW_NO_DEFER);
    samw_bulk(r, F, o, lane, 64u * (extra[k] + 1));
}

// wave w < xoff[n] fills SEQ and QUAL of the record k with xoff[k] <= w < xoff[k + 1], as its part w - xoff[k] + 1
__global__ __launch_bounds__(256) void k_samw_fill_more(const uint8_t *s, const ull *rec_off, uint64_t n, const samw_fld *fld, const ull *xoff, uint64_t n_waves, const ull *line, uint8_t *text)
{
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_waves) return;
    uint64_t lo = 0, hi = n;          // xoff[lo] <= w < xoff[hi]
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (xoff[mid] <= w) lo = mid; else hi = mid; }
    const uint64_t parts = xoff[lo + 1] - xoff[lo] + 1, part = w - xoff[lo] + 1;
    samw_bulk(s + rec_off[lo], fld[lo], text + line[lo], part * 64 + (threadIdx.x & 63), 64 * parts);
}

// ------------------------------------------------------------------ host: the writer
typedef SlxDevBuf<SlxMargin<4, 256>> WDBuf;
typedef SlxPinBuf<SlxMargin<4, 256>> WHBuf;

struct slx_samw : SlxGpu<4> {
    int fd = -1;
    bool is_stdout = false;
    std::string path;
    int flags = 0, fast_fail = 0;
    uint64_t stage_bytes = SAMW_STAGE;
    slx_bgzf *gz = nullptr;                        // SLX_SAMW_BGZF: the file is the BGZF writer's
    SamwRefTable tab;
    bool have_header = false;
    WDBuf d_names{*this}, d_noff{*this}, d_in{*this}, d_off{*this}, d_size{*this}, d_verdict{*this}, d_fld{*this}, d_extra{*this}, d_xoff{*this}, d_line{*this}, d_text{*this}, d_cnt{*this},
          d_tmp{*this}, d_g{*this}, d_slow_in{*this}, d_slow{*this}, d_src{*this};
    WHBuf h_small{*this}, h_verdict{*this}, h_off{*this}, h_g{*this}, h_slow_in{*this}, h_slow{*this}, h_text[2] = {*this, *this};
    int cur = 0;                                   // the pinned buffer the next SAMW_STAGE bytes come down into; the other one may be on its way to the file
    std::thread worker;
    bool worker_on = false;
    int worker_rc = SLX_OK;
    std::string worker_msg;
    int err = SLX_OK;                              // the first write error of the writer's life: sticky
    std::string err_msg;
    int64_t c_records = 0, c_bytes = 0, c_batches = 0, c_fast = 0, c_slow = 0, c_wide = 0, c_extra = 0;
    double us[2] = {0, 0};
    samw_refs dev_refs() const { return samw_refs{d_names.as<uint8_t>(), d_noff.as<uint32_t>(), (int32_t)tab.off.size() - 1}; }
};

static int samw_fail(slx_samw *w, int rc)
{
    if (w->err == SLX_OK) { w->err = rc; w->err_msg = slx_last_error(); }
    return rc;
}
static int samw_sticky(slx_samw *w) { slx_set_error("%s", w->err_msg.c_str()); return w->err; }

// waits for the text on its way to the file and takes the outcome
static int samw_join(slx_samw *w)
{
    if (!w->worker_on) return SLX_OK;
    w->worker.join();
    w->worker_on = false;
    if (w->worker_rc != SLX_OK) { slx_set_error("%s", w->worker_msg.c_str()); return samw_fail(w, w->worker_rc); }
    return SLX_OK;
}

static int samw_write_all(slx_samw *w, const uint8_t *p, uint64_t n)
{
    while (n) {
        const ssize_t got = ::write(w->fd, p, n);
        if (got < 0) { if (errno == EINTR) continue; slx_set_error("SAM writer: cannot write to '%s': %s", w->path.c_str(), strerror(errno)); return SLX_EIO; }
        p += got; n -= (uint64_t)got;
    }
    return SLX_OK;
}

static void samw_free(slx_samw *w)
{
    if (w->worker_on) { w->worker.join(); w->worker_on = false; }
    w->close();
    if (w->fd >= 0 && !w->is_stdout) ::close(w->fd);
    delete w;
}

static int samw_open_impl(slx_samw *w, const char *path, int device, int flags)
{
    const std::string no_device = std::string("no HIP device: the SAM writer formats on MI355X only (no CPU fallback); '") + path + "' is not created";
    SLX_CHK(w->open(device, "SAM writer", no_device.c_str()));
    w->path = path; w->flags = flags;
    w->is_stdout = w->path == "-";
    if (flags & SLX_SAMW_BGZF) SLX_CHK(slx_bgzf_open(path, w->device, &w->gz));
    else {
        w->fd = w->is_stdout ? STDOUT_FILENO : ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (w->fd < 0) { slx_set_error("SAM writer: cannot create '%s': %s", path, strerror(errno)); return SLX_EIO; }
    }
    SLX_CHK(w->h_small.ensure(64));
    w->tab.build({});
    return SLX_OK;
}

extern "C" int slx_samw_open(const char *path, int device, int flags, slx_samw **out)
{
    if (!path || !out || (flags & ~SLX_SAMW_BGZF)) { slx_set_error("slx_samw_open: null argument or unknown flag"); return SLX_EINVAL; }
    *out = nullptr;
    slx_samw *w = new slx_samw();
    const int rc = samw_open_impl(w, path, device, flags);
    if (rc != SLX_OK) {
        if (w->gz) { (void)slx_bgzf_close(w->gz); w->gz = nullptr; }
        samw_free(w);
        return rc;
    }
    *out = w;
    return SLX_OK;
}

extern "C" int slx_samw_header(slx_samw *w, const char *text, int64_t l_text, const char *const *ref_names, int n_ref)
{
    if (!w || l_text < 0 || (l_text && !text) || n_ref < 0 || (n_ref && !ref_names)) { slx_set_error("slx_samw_header: null or negative argument"); return SLX_EINVAL; }
    if (w->err != SLX_OK) return samw_sticky(w);
    if (w->have_header) { slx_set_error("slx_samw_header: the header is already written"); return SLX_EINVAL; }
    SLX_HIPCHK(hipSetDevice(w->device));
    std::vector<std::string> names;
    for (int i = 0; i < n_ref; ++i) names.push_back(ref_names[i] ? ref_names[i] : "");
    w->tab.build(names);
    SLX_CHK(w->d_names.ensure(w->tab.names.size())); SLX_CHK(w->d_noff.ensure(4 * w->tab.off.size()));
    SLX_HIPCHK(hipMemcpy(w->d_names.p, w->tab.names.data(), w->tab.names.size(), hipMemcpyHostToDevice));
    SLX_HIPCHK(hipMemcpy(w->d_noff.p, w->tab.off.data(), 4 * w->tab.off.size(), hipMemcpyHostToDevice));
    w->have_header = true;
    if (!l_text) return SLX_OK;
    if (w->gz) { const int rc = slx_bgzf_write(w->gz, text, l_text); return rc == SLX_OK ? SLX_OK : samw_fail(w, rc); }
    SLX_CHK(samw_join(w));
    const int rc = samw_write_all(w, (const uint8_t *)text, (uint64_t)l_text);
    return rc == SLX_OK ? SLX_OK : samw_fail(w, rc);
}

// The lines of n records (n_bytes of HBM at d_s, offsets d_off) into d_text / d_line.  h_s, h_off: the same records on the host when the caller has them (the slow
// path then reads them there); nullptr: the slow records are gathered and come down.  The stream has drained on return.
static int samw_format(slx_samw *w, const uint8_t *d_s, uint64_t n_bytes, const ull *d_off, uint64_t n, const uint8_t *h_s, const uint64_t *h_off, uint64_t *total_out)
{
    hipStream_t st = w->st;
    *total_out = 0;
    SLX_CHK(w->d_line.ensure(8 * (n + 1)));
    if (n == 0) { SLX_HIPCHK(hipMemsetAsync(w->d_line.p, 0, 8, st)); SLX_HIPCHK(slx_wait_stream(st)); ++w->c_batches; return SLX_OK; }
    if (n >= 0x7fffffffull) { slx_set_error("SAM writer: 2^31 records or more in one batch"); return SLX_EUNSUPPORTED; }
    SLX_CHK(w->d_size.ensure(8 * (n + 1))); SLX_CHK(w->d_extra.ensure(8 * (n + 1))); SLX_CHK(w->d_xoff.ensure(8 * (n + 1))); SLX_CHK(w->d_verdict.ensure(n + 8));
    SLX_CHK(w->d_fld.ensure(sizeof(samw_fld) * n)); SLX_CHK(w->d_cnt.ensure(8)); SLX_CHK(w->d_src.ensure(8 * (n + 1)));
    ull *hs = w->h_small.as<ull>();
    const samw_refs R = w->dev_refs();
    SLX_HIPCHK(hipMemsetAsync(w->d_cnt.p, 0, 8, st));
    SLX_HIPCHK(hipEventRecord(w->ev[0], st));
    k_samw_size<<<(unsigned)((n + 1 + 255) / 256), 256, 0, st>>>(d_s, n_bytes, d_off, n, R, w->fast_fail, w->d_size.as<ull>(), w->d_verdict.as<uint8_t>(), w->d_fld.as<samw_fld>(),
                                                                w->d_extra.as<ull>(), w->d_cnt.as<ull>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(w->ev[1], st));
    SLX_HIPCHK(hipMemcpyAsync(hs, w->d_cnt.p, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    w->us[0] += slx_ev_us(w->ev[0], w->ev[1]);
    const uint64_t n_other = hs[0] & 0xffffffffull, n_wide = hs[0] >> 32;
    // ---- the records that are not FAST: the first ERROR ends the call; the SLOW ones through the host formatter
    uint64_t n_slow = 0;
    if (n_other) {
        SLX_CHK(w->h_verdict.ensure(n + 8));
        SLX_HIPCHK(hipMemcpyAsync(w->h_verdict.p, w->d_verdict.p, n, hipMemcpyDeviceToHost, st));
        if (!h_off) { SLX_CHK(w->h_off.ensure(8 * (n + 1))); SLX_HIPCHK(hipMemcpyAsync(w->h_off.p, d_off, 8 * (n + 1), hipMemcpyDeviceToHost, st)); h_off = w->h_off.as<uint64_t>(); }
        SLX_HIPCHK(slx_wait_stream(st));
        const uint8_t *hv = w->h_verdict.as<uint8_t>();
        for (uint64_t k = 0; k < n; ++k)
            if ((hv[k] & 3) == SAMW_ERROR) { slx_set_error("SAM writer: record %llu of the batch: %s; nothing of the batch is written", (ull)k, samwh_errtext(hv[k] >> 2)); return SLX_EIO; }
        for (uint64_t k = 0; k < n; ++k) n_slow += (hv[k] & 3) == SAMW_SLOW;
        SLX_CHK(w->h_g.ensure(24 * n_slow + 8)); SLX_CHK(w->d_g.ensure(24 * n_slow + 8));
        ull *g = w->h_g.as<ull>();
        uint64_t j = 0, in_bytes = 0;
        for (uint64_t k = 0; k < n; ++k)
            if ((hv[k] & 3) == SAMW_SLOW) { g[3 * j] = h_off[k]; g[3 * j + 1] = h_off[k + 1] - h_off[k]; g[3 * j + 2] = in_bytes; in_bytes += g[3 * j + 1]; ++j; }
        if (!h_s) {          // (the verdicts are the size kernel's: every extent lies inside the stream)
            SLX_CHK(w->d_slow_in.ensure(in_bytes + 8)); SLX_CHK(w->h_slow_in.ensure(in_bytes + 8));
            SLX_HIPCHK(hipMemcpyAsync(w->d_g.p, g, 24 * n_slow, hipMemcpyHostToDevice, st));
            k_samw_gather<<<(unsigned)((n_slow + 3) / 4), 256, 0, st>>>(d_s, w->d_g.as<ull>(), n_slow, w->d_slow_in.as<uint8_t>());
            SLX_HIPCHK(hipGetLastError());
            SLX_HIPCHK(hipMemcpyAsync(w->h_slow_in.p, w->d_slow_in.p, in_bytes, hipMemcpyDeviceToHost, st));
            SLX_HIPCHK(slx_wait_stream(st));
        }
        const samw_refs HR = w->tab.view();
        std::vector<uint8_t> stage;
        j = 0;
        for (uint64_t k = 0; k < n; ++k) {
            if ((hv[k] & 3) != SAMW_SLOW) continue;
            const uint8_t *rec = h_s ? h_s + g[3 * j] : w->h_slow_in.as<uint8_t>() + g[3 * j + 2];
            const uint64_t len = g[3 * j + 1], at = stage.size();
            int e = SAMW_E_NONE;
            if (samwh_format(rec, len, HR, stage, &e) != SAMW_FAST) { slx_set_error("SAM writer: internal: the kernel takes record %llu, the host formatter refuses it (%s)", (ull)k, samwh_errtext(e)); return SLX_EINTERNAL; }
            g[3 * j] = k; g[3 * j + 1] = stage.size() - at; g[3 * j + 2] = at;
            ++j;
        }
        SLX_CHK(w->d_slow.ensure(stage.size() + 8)); SLX_CHK(w->h_slow.ensure(stage.size() + 8));
        memcpy(w->h_slow.p, stage.data(), stage.size());
        SLX_HIPCHK(hipMemcpyAsync(w->d_slow.p, w->h_slow.p, stage.size(), hipMemcpyHostToDevice, st));
        SLX_HIPCHK(hipMemcpyAsync(w->d_g.p, g, 24 * n_slow, hipMemcpyHostToDevice, st));
        if (n_slow) { k_samw_slow_put<<<(unsigned)((n_slow + 255) / 256), 256, 0, st>>>(w->d_g.as<ull>(), n_slow, w->d_size.as<ull>(), w->d_src.as<ull>()); SLX_HIPCHK(hipGetLastError()); }
    }
    // ---- offsets, then the text
    SLX_CHK(slx_exclusive_sum(w->d_tmp, w->d_size.as<ull>(), w->d_line.as<ull>(), (size_t)n + 1, st));
    SLX_CHK(slx_exclusive_sum(w->d_tmp, w->d_extra.as<ull>(), w->d_xoff.as<ull>(), (size_t)n + 1, st));
    SLX_HIPCHK(hipMemcpyAsync(hs, w->d_line.as<ull>() + n, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync(hs + 1, w->d_xoff.as<ull>() + n, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    const uint64_t total = hs[0], n_extra = hs[1];
    SLX_CHK(w->d_text.ensure(total + 64));
    SLX_HIPCHK(hipEventRecord(w->ev[2], st));
    k_samw_fill<<<(unsigned)((n + 3) / 4), 256, 0, st>>>(d_s, d_off, n, R, w->d_verdict.as<uint8_t>(), w->d_fld.as<samw_fld>(), w->d_extra.as<ull>(), w->d_slow.as<uint8_t>(), w->d_src.as<ull>(),
                                                        w->d_line.as<ull>(), w->d_text.as<uint8_t>());
    SLX_HIPCHK(hipGetLastError());
    if (n_extra) {
        k_samw_fill_more<<<(unsigned)((n_extra + 3) / 4), 256, 0, st>>>(d_s, d_off, n, w->d_fld.as<samw_fld>(), w->d_xoff.as<ull>(), n_extra, w->d_line.as<ull>(), w->d_text.as<uint8_t>());
        SLX_HIPCHK(hipGetLastError());
    }
    SLX_HIPCHK(hipEventRecord(w->ev[3], st));
    SLX_HIPCHK(slx_wait_stream(st));
    w->us[1] += slx_ev_us(w->ev[2], w->ev[3]);
    w->c_records += (int64_t)n; w->c_bytes += (int64_t)total; ++w->c_batches; w->c_slow += (int64_t)n_slow; w->c_fast += (int64_t)(n - n_slow); w->c_wide += (int64_t)n_wide;
    w->c_extra += (int64_t)n_extra;
    *total_out = total;
    return SLX_OK;
}

// d_text[0, total) to the file
static int samw_emit(slx_samw *w, uint64_t total)
{
    if (!total) return SLX_OK;
    if (w->gz) { const int rc = slx_bgzf_write_device(w->gz, w->d_text.p, (int64_t)total); return rc == SLX_OK ? SLX_OK : samw_fail(w, rc); }
    for (uint64_t at = 0; at < total; at += w->stage_bytes) {          // a stage at a time: the copy down of one runs beside the file write of the one before
        const uint64_t len = total - at < w->stage_bytes ? total - at : w->stage_bytes;
        WHBuf &h = w->h_text[w->cur];          // (not the one on its way to the file)
        SLX_CHK(h.ensure(len));
        SLX_HIPCHK(hipMemcpyAsync(h.p, w->d_text.as<uint8_t>() + at, len, hipMemcpyDeviceToHost, w->st));
        SLX_HIPCHK(slx_wait_stream(w->st));
        SLX_CHK(samw_join(w));
        const uint8_t *p = h.as<uint8_t>();
        w->cur ^= 1;
        w->worker_rc = SLX_OK;
        w->worker_on = true;
        w->worker = std::thread([w, p, len]() {
            w->worker_rc = samw_write_all(w, p, len);
            if (w->worker_rc != SLX_OK) w->worker_msg = slx_last_error();
        });
    }
    return SLX_OK;
}

static int samw_args(const char *who, slx_samw *w, const void *s, int64_t n_bytes, const void *off, int64_t n)
{
    if (!w) { slx_set_error("%s: null writer", who); return SLX_EINVAL; }
    SLX_CHK(slx_batch_args(who, s, n_bytes, off, n));
    if (w->err != SLX_OK) return samw_sticky(w);
    SLX_HIPCHK(hipSetDevice(w->device));
    return SLX_OK;
}

extern "C" int slx_samw_format_device(slx_samw *w, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records, slx_samw_text *out)
{
    if (!out) { slx_set_error("slx_samw_format_device: out is null"); return SLX_EINVAL; }
    memset(out, 0, sizeof *out);
    SLX_CHK(samw_args("slx_samw_format_device", w, d_stream, n_bytes, d_rec_off, n_records));
    uint64_t total = 0;
    SLX_CHK(samw_format(w, (const uint8_t *)d_stream, (uint64_t)n_bytes, (const ull *)d_rec_off, (uint64_t)n_records, nullptr, nullptr, &total));
    out->d_text = w->d_text.p; out->d_line_off = w->d_line.p; out->n_bytes = total; out->n_records = (uint64_t)n_records;
    return SLX_OK;
}

extern "C" int slx_samw_write_device(slx_samw *w, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records)
{
    SLX_CHK(samw_args("slx_samw_write_device", w, d_stream, n_bytes, d_rec_off, n_records));
    uint64_t total = 0;
    SLX_CHK(samw_format(w, (const uint8_t *)d_stream, (uint64_t)n_bytes, (const ull *)d_rec_off, (uint64_t)n_records, nullptr, nullptr, &total));
    return samw_emit(w, total);
}

extern "C" int slx_samw_write_host(slx_samw *w, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records)
{
    SLX_CHK(samw_args("slx_samw_write_host", w, stream, n_bytes, rec_off, n_records));
    if (n_records == 0) return SLX_OK;
    SLX_CHK(slx_batch_stage(w->d_in, w->d_off, 8, stream, n_bytes, rec_off, n_records, w->st));
    uint64_t total = 0;
    SLX_CHK(samw_format(w, w->d_in.as<uint8_t>(), (uint64_t)n_bytes, w->d_off.as<ull>(), (uint64_t)n_records, (const uint8_t *)stream, rec_off, &total));
    return samw_emit(w, total);
}

extern "C" int slx_samw_format_record(const uint8_t *rec, int64_t n, const char *const *ref_names, int n_ref, char *out, int64_t cap, int64_t *n_out)
{
    if (!rec || n < 0 || n_ref < 0 || (n_ref && !ref_names) || !n_out || (cap > 0 && !out)) { slx_set_error("slx_samw_format_record: null or negative argument"); return SLX_EINVAL; }
    *n_out = 0;
    std::vector<std::string> names;
    for (int i = 0; i < n_ref; ++i) names.push_back(ref_names[i] ? ref_names[i] : "");
    SamwRefTable tab;
    tab.build(names);
    std::vector<uint8_t> text;
    int err = SAMW_E_NONE;
    if (samwh_format(rec, (uint64_t)n, tab.view(), text, &err) != SAMW_FAST) { slx_set_error("SAM writer: %s", samwh_errtext(err)); return SLX_EIO; }
    *n_out = (int64_t)text.size();
    if ((int64_t)text.size() > cap) { slx_set_error("slx_samw_format_record: the line takes %zu bytes, out holds %lld", text.size(), (long long)cap); return SLX_EINVAL; }
    memcpy(out, text.data(), text.size());
    return SLX_OK;
}

extern "C" int slx_samw_set(slx_samw *w, const char *key, int64_t value)
{
    if (!w || !key) { slx_set_error("slx_samw_set: null argument"); return SLX_EINVAL; }
    if (!strcmp(key, "fast_fail")) {
        if (value != 0 && value != 1) { slx_set_error("slx_samw_set: fast_fail is 0 or 1"); return SLX_EINVAL; }
        w->fast_fail = (int)value;
        return SLX_OK;
    }
    if (!strcmp(key, "stage_bytes")) {
        if (value < 4096 || value > (1ll << 30)) { slx_set_error("slx_samw_set: stage_bytes %lld outside [4096, 2^30]", (long long)value); return SLX_EINVAL; }
        w->stage_bytes = (uint64_t)value;
        return SLX_OK;
    }
    slx_set_error("slx_samw_set: unknown key '%s'", key);
    return SLX_EINVAL;
}

extern "C" int64_t slx_samw_counter(const slx_samw *w, const char *name)
{
    if (!w || !name) return -1;
    if (!strcmp(name, "records")) return w->c_records;
    if (!strcmp(name, "bytes")) return w->c_bytes;
    if (!strcmp(name, "batches")) return w->c_batches;
    if (!strcmp(name, "fast_records")) return w->c_fast;
    if (!strcmp(name, "slow_records")) return w->c_slow;
    if (!strcmp(name, "wide_records")) return w->c_wide;
    if (!strcmp(name, "extra_waves")) return w->c_extra;
    if (!strcmp(name, "us_size")) return (int64_t)w->us[0];
    if (!strcmp(name, "us_fill")) return (int64_t)w->us[1];
    return -1;
}

extern "C" int slx_samw_close(slx_samw *w)
{
    if (!w) { slx_set_error("slx_samw_close: null writer"); return SLX_EINVAL; }
    (void)samw_join(w);
    if (w->gz) {
        const int rc = slx_bgzf_close(w->gz);          // the last member, the EOF block; its handle is freed
        w->gz = nullptr;
        if (rc != SLX_OK) samw_fail(w, rc);
    } else if (!w->is_stdout && w->fd >= 0) {
        if (::close(w->fd) != 0) { slx_set_error("SAM writer: cannot close '%s': %s", w->path.c_str(), strerror(errno)); samw_fail(w, SLX_EIO); }
        w->fd = -1;
    }
    const int rc = w->err;
    if (rc != SLX_OK) slx_set_error("%s", w->err_msg.c_str());
    samw_free(w);
    return rc;
}
