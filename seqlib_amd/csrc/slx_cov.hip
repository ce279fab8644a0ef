// slx_cov.hip -- depth of coverage on the GPU (include/seqlib_amd_cov.h): block_size-prefixed BAM records in HBM -> one int32 array over all contigs, read back as
// depths, region sums or bedGraph text.  DESIGN.md section 9.9 has the argument.
//   k_cov_events       one lane per record, a block per slice of records: eligibility, the CIGAR walk, the +-1 adds -- into an LDS window anchored at the slice's
//                      first eligible record where they fall inside it, into HBM otherwise; the window is flushed at the block's end        cov_host.h cov_record
//   k_cov_events_long  one wave per record with more than long_cigar ops (a compacted list k_cov_events fills)                            cov_host.h cov_record
//   settle             hipCUB's inclusive sum in place, scan_chunk entries at a time, the carry added to a chunk's first entry (k_cov_carry).  A contig's
//                      differences sum to 0 at its last entry, so one scan over the whole array is the scan of every contig
//   unsettle           k_cov_tails + k_cov_diff: the adjacent difference in place, before records are added to a settled array
//   k_cov_regions      one wave per region tile, 16-byte loads, partial sums by atomics
//   k_cov_bg_len / hipCUB / k_cov_bg_fill   bedGraph: one lane per entry gives the piece of text its position starts or ends (cov_host.h cov_bg_piece), the
//                      exclusive sum places the pieces; a chunk of entries at a time, down through two pinned buffers while the file is written
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <fcntl.h>
#include <unistd.h>
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "slx_internal.h"
#include "slx_hip.h"
#include "seqlib_amd_cov.h"
#include "dev_cov.h"

typedef unsigned long long ull;
#define COV_BG_CHUNK (1ull << 22)          // entries per bedGraph pass (and never more than scan_chunk)
#define COV_STAGE (16ull << 20)            // bytes of text one pinned buffer holds

typedef SlxDevBuf<SlxMargin<4, 256>> CDBuf;
typedef SlxPinBuf<SlxMargin<4, 256>> CHBuf;

static const char COV_NO_DEVICE[] = "no HIP device: coverage is computed on MI355X only (no CPU fallback)";

struct slx_cov : SlxTwoPass {
    slx_cov() : SlxTwoPass(COV_NO_DEVICE) {}
    std::vector<int64_t> len, beg, end, off;
    std::vector<std::string> names;
    uint64_t total = 0;
    cov_par par = {COV_ALIGNED, 0, 0, 0, 0x704u, 64u};
    uint32_t lds_window = 8192, slice = 1024;
    uint64_t scan_chunk = 1ull << 30;
    bool settled = false;          // the array holds depths, not differences
    SlxDevBuf<SlxExact> d_arr{*this};
    CDBuf d_geo{*this}, d_names{*this}, d_noff{*this}, d_in{*this}, d_off{*this}, d_tmp{*this}, d_bound{*this}, d_items{*this}, d_sums{*this}, d_len{*this},
          d_at{*this}, d_text{*this}, d_max{*this};
    CHBuf h_items{*this}, h_sums{*this}, h_text[2] = {*this, *this};
    int64_t c_runs = 0;
    double us_settle = 0;
    cov_geo geo() const { const int64_t *g = d_geo.as<int64_t>(); const size_t n = len.size(); return cov_geo{g, g + n, g + 2 * n, (int32_t)n, 0, (int64_t)total}; }
    int32_t *arr() const { return d_arr.as<int32_t>(); }
};

extern "C" void slx_cov_free(slx_cov *c)
{
    if (!c) return;
    c->close();
    delete c;
}

static int cov_create_impl(slx_cov *c, int device, int n_ref, const int64_t *ref_len, const char *const *ref_names, const slx_bam_region *win)
{
    for (int i = 0; i < n_ref; ++i) {
        if (ref_len[i] < 0 || ref_len[i] > 0x7fffffffll) { slx_set_error("slx_cov_create: contig %d has length %lld, outside [0, 2^31 - 1]", i, (long long)ref_len[i]); return SLX_EINVAL; }
        c->len.push_back(ref_len[i]);
        c->names.push_back(ref_names && ref_names[i] ? ref_names[i] : std::to_string(i));
    }
    c->beg.assign((size_t)n_ref, 0); c->end = c->len;
    if (win) {
        if (win->tid < 0 || win->tid >= n_ref || win->beg > win->end) { slx_set_error("slx_cov_create: the window names contig %d of %d, or ends before it begins", win->tid, n_ref); return SLX_EINVAL; }
        for (int i = 0; i < n_ref; ++i) c->end[i] = 0;
        const int64_t L = c->len[win->tid];
        c->beg[win->tid] = std::min(std::max<int64_t>(win->beg, 0), L); c->end[win->tid] = std::min(std::max<int64_t>(win->end, c->beg[win->tid]), L);
    }
    std::vector<int64_t> kept((size_t)n_ref);
    for (int i = 0; i < n_ref; ++i) kept[i] = c->end[i] - c->beg[i];
    c->off.assign((size_t)n_ref, 0);
    c->total = cov_layout(kept.data(), n_ref, c->off.data());
    SLX_CHK(c->open(device, "slx_cov_create", COV_NO_DEVICE, true));
    if (c->device < 0) return SLX_OK;          // host only
    SLX_CHK(c->d_arr.ensure(4 * c->total + 16));
    SLX_HIPCHK(hipMemsetAsync(c->d_arr.p, 0, 4 * c->total + 16, c->st));
    std::vector<int64_t> g;
    g.insert(g.end(), c->beg.begin(), c->beg.end()); g.insert(g.end(), c->end.begin(), c->end.end()); g.insert(g.end(), c->off.begin(), c->off.end());
    std::vector<uint8_t> nm;
    std::vector<uint32_t> noff(1, 0);
    for (const std::string &s : c->names) { nm.insert(nm.end(), s.begin(), s.end()); noff.push_back((uint32_t)nm.size()); }
    nm.push_back(0);
    SLX_CHK(c->d_geo.ensure(8 * g.size() + 8)); SLX_CHK(c->d_names.ensure(nm.size())); SLX_CHK(c->d_noff.ensure(4 * noff.size()));
    SLX_CHK(c->d_cnt.ensure(8 * COV_C_N)); SLX_CHK(c->h_cnt.ensure(8 * (COV_C_N + 1))); SLX_CHK(c->d_max.ensure(8));
    if (!g.empty()) SLX_HIPCHK(hipMemcpyAsync(c->d_geo.p, g.data(), 8 * g.size(), hipMemcpyHostToDevice, c->st));
    SLX_HIPCHK(hipMemcpyAsync(c->d_names.p, nm.data(), nm.size(), hipMemcpyHostToDevice, c->st));
    SLX_HIPCHK(hipMemcpyAsync(c->d_noff.p, noff.data(), 4 * noff.size(), hipMemcpyHostToDevice, c->st));
    SLX_HIPCHK(slx_wait_stream(c->st));
    return SLX_OK;
}

extern "C" int slx_cov_create(int device, int n_ref, const int64_t *ref_len, const char *const *ref_names, const slx_bam_region *window, slx_cov **out)
{
    if (!out || n_ref < 0 || (n_ref && !ref_len)) { slx_set_error("slx_cov_create: null or negative argument"); return SLX_EINVAL; }
    return slx_create(out, slx_cov_free, [&](slx_cov *c) { return cov_create_impl(c, device, n_ref, ref_len, ref_names, window); });
}

extern "C" int slx_cov_set(slx_cov *c, const char *key, int64_t v)
{
    if (!c || !key) { slx_set_error("slx_cov_set: null argument"); return SLX_EINVAL; }
    auto in = [&](int64_t lo, int64_t hi) { if (v >= lo && v <= hi) return true; slx_set_error("slx_cov_set: %s %lld outside [%lld, %lld]", key, (long long)v, (long long)lo, (long long)hi); return false; };
    if (!strcmp(key, "mode")) { if (!in(0, 2)) return SLX_EINVAL; c->par.mode = (int32_t)v; return SLX_OK; }
    if (!strcmp(key, "buff")) { if (!in(-(1ll << 30), 1ll << 30)) return SLX_EINVAL; c->par.buff = (int32_t)v; return SLX_OK; }
    if (!strcmp(key, "min_mapq")) { if (!in(0, 255)) return SLX_EINVAL; c->par.min_mapq = (int32_t)v; return SLX_OK; }
    if (!strcmp(key, "exclude_flags")) { if (!in(0, 0xffff)) return SLX_EINVAL; c->par.exclude_flags = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "count_del")) { if (!in(0, 1)) return SLX_EINVAL; c->par.count_del = (int32_t)v; return SLX_OK; }
    if (!strcmp(key, "long_cigar")) { if (!in(0, 1 << 20)) return SLX_EINVAL; c->par.long_cigar = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "lds_window")) { if (!in(0, 15360)) return SLX_EINVAL; c->lds_window = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "slice_records")) { if (!in(64, 1 << 20)) return SLX_EINVAL; c->slice = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "scan_chunk")) {
        if (!in(64, 1ll << 30)) return SLX_EINVAL;
        if (v & 3) { slx_set_error("slx_cov_set: scan_chunk %lld is not a multiple of 4", (long long)v); return SLX_EINVAL; }
        c->scan_chunk = (uint64_t)v;
        return SLX_OK;
    }
    slx_set_error("slx_cov_set: unknown key '%s'", key);
    return SLX_EINVAL;
}

// depths -> differences, in place
static int cov_unsettle(slx_cov *c)
{
    if (!c->settled) return SLX_OK;
    if (c->total) {
        const uint64_t tiles = (c->total + 1023) / 1024;
        SLX_CHK(c->d_bound.ensure(4 * tiles + 4));
        k_cov_tails<<<(unsigned)((tiles + 255) / 256), 256, 0, c->st>>>(c->arr(), c->total, c->d_bound.as<int32_t>());
        SLX_HIPCHK(hipGetLastError());
        k_cov_diff<<<(unsigned)tiles, 256, 0, c->st>>>(c->arr(), c->total, c->d_bound.as<int32_t>());
        SLX_HIPCHK(hipGetLastError());
        SLX_HIPCHK(slx_wait_stream(c->st));
    }
    c->settled = false;
    return SLX_OK;
}

// differences -> depths, in place: hipCUB never sees more than scan_chunk (<= 2^30) items
static int cov_settle(slx_cov *c)
{
    if (c->settled) return SLX_OK;
    SLX_HIPCHK(hipEventRecord(c->ev[0], c->st));
    for (uint64_t at = 0; at < c->total; at += c->scan_chunk) {
        const uint64_t n = std::min(c->scan_chunk, c->total - at);
        if (at) { k_cov_carry<<<1, 1, 0, c->st>>>(c->arr(), at); SLX_HIPCHK(hipGetLastError()); }
        SLX_CHK(slx_cub("hipcub::DeviceScan::InclusiveSum (coverage, settle)", c->d_tmp, 8, [&](void *t, size_t &b) { return hipcub::DeviceScan::InclusiveSum(t, b, c->arr() + at, c->arr() + at, (int)n, c->st); }));
    }
    SLX_HIPCHK(hipEventRecord(c->ev[1], c->st));
    SLX_HIPCHK(slx_wait_stream(c->st));
    c->us_settle += slx_ev_us(c->ev[0], c->ev[1]);
    c->settled = true;
    return SLX_OK;
}

// the records of d_s (n_bytes, offsets d_off) into the array; the stream has drained on return
static int cov_add(slx_cov *c, const uint8_t *d_s, uint64_t n_bytes, const ull *d_off, uint64_t n)
{
    if (n == 0) return SLX_OK;
    if (n < 0x7fffffffull) SLX_CHK(cov_unsettle(c));          // (a batch that is refused for its size leaves the array as it stands)
    hipStream_t st = c->st;
    ull *dc = c->d_cnt.as<ull>();
    return slx_two_pass_add(*c, "coverage", n, COV_C_N,
        [&]() { k_cov_events<<<(unsigned)((n + c->slice - 1) / c->slice), 256, 4 * (size_t)c->lds_window, st>>>(d_s, n_bytes, d_off, n, c->par, c->geo(), c->arr(), c->slice, c->lds_window, c->d_long.as<ull>(), dc); },
        [&](uint64_t n_long) { k_cov_events_long<<<(unsigned)((n_long + 3) / 4), 256, 0, st>>>(d_s, d_off, c->d_long.as<ull>(), n_long, c->par, c->geo(), c->arr(), dc); });
}

extern "C" int slx_cov_add_device(slx_cov *c, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records)
{
    SLX_CHK(slx_need(c, "slx_cov_add_device"));
    SLX_CHK(slx_batch_args("slx_cov_add_device", d_stream, n_bytes, d_rec_off, n_records));
    return cov_add(c, (const uint8_t *)d_stream, (uint64_t)n_bytes, (const ull *)d_rec_off, (uint64_t)n_records);
}

extern "C" int slx_cov_add_host(slx_cov *c, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records)
{
    SLX_CHK(slx_need(c, "slx_cov_add_host"));
    SLX_CHK(slx_batch_args("slx_cov_add_host", stream, n_bytes, rec_off, n_records));
    if (n_records == 0) return SLX_OK;
    SLX_CHK(slx_batch_stage(c->d_in, c->d_off, 8, stream, n_bytes, rec_off, n_records, c->st));
    return cov_add(c, c->d_in.as<uint8_t>(), (uint64_t)n_bytes, c->d_off.as<ull>(), (uint64_t)n_records);
}

struct CovHostSink {
    int64_t *lo, *hi, cap, n;
    void operator()(int32_t, int64_t a, int64_t b) { if (n < cap) { lo[n] = a; hi[n] = b; } ++n; }
};

extern "C" int slx_cov_record_intervals(const uint8_t *rec, int64_t n, int mode, int buff, int count_del, int64_t clip_beg, int64_t clip_end, int64_t *out_lo, int64_t *out_hi,
                                        int64_t cap, int64_t *n_out)
{
    if (!rec || n < 0 || !n_out || cap < 0 || (cap && (!out_lo || !out_hi)) || mode < 0 || mode > 2) { slx_set_error("slx_cov_record_intervals: null, negative or unknown argument"); return SLX_EINVAL; }
    *n_out = 0;
    const cov_par P = {mode, buff, count_del ? 1 : 0, 0, 0u, 1u << 20};
    rf_feat F;
    const int v = cov_head(rec, (uint64_t)n, P, 0x7fffffff, &F);
    if (v == COV_R_BAD) { slx_set_error("coverage: the record's fields pass its block_size, or its extent is not block_size + 4"); return SLX_EIO; }
    if (v == COV_R_SKIP) return SLX_OK;
    // (one contig stands for the record's: the geometry is indexed by tid 0)
    const int64_t beg = clip_beg, end = clip_end, off = 0;
    const cov_geo G = {&beg, &end, &off, 1, 0, 0};
    F.tid = 0;
    CovHostSink S = {out_lo, out_hi, cap, 0};
    cov_record(F, P, G, 0u, 1u, lanes_one(), S);
    *n_out = S.n;
    if (S.n > cap) { slx_set_error("slx_cov_record_intervals: %lld intervals, out holds %lld", (long long)S.n, (long long)cap); return SLX_EINVAL; }
    return SLX_OK;
}

static int cov_tid(const char *who, const slx_cov *c, int tid)
{
    if (tid < 0 || tid >= (int)c->len.size()) { slx_set_error("%s: contig %d is not one of the %zu", who, tid, c->len.size()); return SLX_EINVAL; }
    return SLX_OK;
}

extern "C" int slx_cov_depth(slx_cov *c, int tid, int64_t beg, int64_t end, int32_t *out)
{
    SLX_CHK(slx_need(c, "slx_cov_depth"));
    SLX_CHK(cov_tid("slx_cov_depth", c, tid));
    if (beg > end || (beg < end && !out)) { slx_set_error("slx_cov_depth: null output or an interval that ends before it begins"); return SLX_EINVAL; }
    SLX_CHK(cov_settle(c));
    if (beg == end) return SLX_OK;
    memset(out, 0, 4 * (size_t)(end - beg));
    const int64_t lo = std::max(beg, c->beg[tid]), hi = std::min(end, c->end[tid]);
    if (lo < hi) SLX_HIPCHK(hipMemcpy(out + (lo - beg), c->arr() + c->off[tid] + (lo - c->beg[tid]), 4 * (size_t)(hi - lo), hipMemcpyDeviceToHost));
    return SLX_OK;
}

extern "C" int slx_cov_depth_device(slx_cov *c, int tid, const void **d_depth, int64_t *n)
{
    SLX_CHK(slx_need(c, "slx_cov_depth_device"));
    SLX_CHK(cov_tid("slx_cov_depth_device", c, tid));
    if (!d_depth || !n) { slx_set_error("slx_cov_depth_device: null argument"); return SLX_EINVAL; }
    SLX_CHK(cov_settle(c));
    *d_depth = c->arr() + c->off[tid]; *n = c->end[tid] - c->beg[tid];
    return SLX_OK;
}

extern "C" int64_t slx_cov_at(slx_cov *c, int tid, int64_t pos)
{
    SLX_CHK(slx_need(c, "slx_cov_at"));
    if (tid < 0 || tid >= (int)c->len.size() || pos < c->beg[tid] || pos >= c->end[tid]) return 0;
    SLX_CHK(cov_settle(c));
    int32_t v = 0;
    SLX_HIPCHK(hipMemcpy(&v, c->arr() + c->off[tid] + (pos - c->beg[tid]), 4, hipMemcpyDeviceToHost));
    return v;
}

extern "C" int64_t slx_cov_max(slx_cov *c, int tid)
{
    SLX_CHK(slx_need(c, "slx_cov_max"));
    if (tid != -1) SLX_CHK(cov_tid("slx_cov_max", c, tid));
    SLX_CHK(cov_settle(c));
    const uint64_t g0 = tid < 0 ? 0 : (uint64_t)c->off[tid], g1 = tid < 0 ? c->total : g0 + (uint64_t)(c->end[tid] - c->beg[tid]);
    SLX_HIPCHK(hipMemsetAsync(c->d_max.p, 0, 4, c->st));
    if (g1 > g0) {
        const uint64_t blocks = std::min<uint64_t>((g1 - g0 + 255) / 256, 4096);
        k_cov_max<<<(unsigned)blocks, 256, 0, c->st>>>(c->arr(), g0, g1, c->d_max.as<int32_t>());
        SLX_HIPCHK(hipGetLastError());
    }
    int32_t *h = c->h_cnt.as<int32_t>();
    SLX_HIPCHK(hipMemcpyAsync(h, c->d_max.p, 4, hipMemcpyDeviceToHost, c->st));
    SLX_HIPCHK(slx_wait_stream(c->st));
    return h[0];
}

extern "C" int slx_cov_regions(slx_cov *c, const slx_bam_region *regs, int64_t n, int32_t min_depth, int64_t *sum, int64_t *n_at_least)
{
    SLX_CHK(slx_need(c, "slx_cov_regions"));
    if (n < 0 || (n && (!regs || !sum || !n_at_least))) { slx_set_error("slx_cov_regions: null or negative argument"); return SLX_EINVAL; }
    for (int64_t i = 0; i < n; ++i) SLX_CHK(cov_tid("slx_cov_regions", c, regs[i].tid));
    SLX_CHK(cov_settle(c));
    if (n == 0) return SLX_OK;
    std::vector<cov_item> items;
    for (int64_t i = 0; i < n; ++i) {
        const slx_bam_region &r = regs[i];
        const int64_t lo = std::max(r.beg, c->beg[r.tid]), hi = std::min(r.end, c->end[r.tid]);
        if (lo >= hi) continue;
        const uint64_t g0 = (uint64_t)(c->off[r.tid] + lo - c->beg[r.tid]), g1 = g0 + (uint64_t)(hi - lo);
        for (uint64_t g = g0; g < g1; g += COV_REG_TILE) items.push_back(cov_item{g, std::min<uint64_t>(g + COV_REG_TILE, g1), (uint64_t)i});
    }
    SLX_CHK(c->d_sums.ensure(16 * (size_t)n)); SLX_CHK(c->h_sums.ensure(16 * (size_t)n));
    SLX_HIPCHK(hipMemsetAsync(c->d_sums.p, 0, 16 * (size_t)n, c->st));
    if (!items.empty()) {
        const size_t ib = sizeof(cov_item) * items.size();
        SLX_CHK(c->d_items.ensure(ib)); SLX_CHK(c->h_items.ensure(ib));
        memcpy(c->h_items.p, items.data(), ib);
        SLX_HIPCHK(hipMemcpyAsync(c->d_items.p, c->h_items.p, ib, hipMemcpyHostToDevice, c->st));
        k_cov_regions<<<(unsigned)((items.size() + 3) / 4), 256, 0, c->st>>>(c->arr(), c->d_items.as<cov_item>(), items.size(), min_depth, c->d_sums.as<ull>(), c->d_sums.as<ull>() + n);
        SLX_HIPCHK(hipGetLastError());
    }
    SLX_HIPCHK(hipMemcpyAsync(c->h_sums.p, c->d_sums.p, 16 * (size_t)n, hipMemcpyDeviceToHost, c->st));
    SLX_HIPCHK(slx_wait_stream(c->st));
    const int64_t *h = c->h_sums.as<int64_t>();
    for (int64_t i = 0; i < n; ++i) { sum[i] = h[i]; n_at_least[i] = h[n + i]; }
    return SLX_OK;
}

static int cov_write_all(int fd, const char *path, const uint8_t *p, uint64_t n)
{
    while (n) {
        const ssize_t got = ::write(fd, p, n);
        if (got < 0) { if (errno == EINTR) continue; slx_set_error("coverage: cannot write to '%s': %s", path, strerror(errno)); return SLX_EIO; }
        p += got; n -= (uint64_t)got;
    }
    return SLX_OK;
}

// the file write of one pinned buffer, beside the kernels and the copy of the next
struct CovWriter {
    int fd; const char *path;
    std::thread th; bool on = false; int rc = SLX_OK; std::string msg;
    int join() { if (on) { th.join(); on = false; } if (rc != SLX_OK) slx_set_error("%s", msg.c_str()); return rc; }
    void start(const uint8_t *p, uint64_t n) { on = true; th = std::thread([this, p, n]() { rc = cov_write_all(fd, path, p, n); if (rc != SLX_OK) msg = slx_last_error(); }); }
};

static int cov_bedgraph_impl(slx_cov *c, int tid, int include_zero, CovWriter &W)
{
    const cov_geo G = c->geo();
    const cov_names N = {c->d_names.as<uint8_t>(), c->d_noff.as<uint32_t>()};
    const uint64_t g_beg = tid < 0 ? 0 : (uint64_t)c->off[tid], g_end = tid < 0 ? c->total : g_beg + (uint64_t)(c->end[tid] - c->beg[tid]);
    const uint64_t chunk = std::min<uint64_t>(COV_BG_CHUNK, c->scan_chunk);
    ull *dc = c->d_cnt.as<ull>(), *hc = c->h_cnt.as<ull>();
    SLX_HIPCHK(hipMemsetAsync(dc, 0, 8 * COV_C_N, c->st));
    int cur = 0;
    for (uint64_t c0 = g_beg; c0 < g_end; c0 += chunk) {
        const uint64_t m = std::min(chunk, g_end - c0);
        SLX_CHK(c->d_len.ensure(8 * (m + 1))); SLX_CHK(c->d_at.ensure(8 * (m + 1)));
        k_cov_bg_len<<<(unsigned)((m + 1 + 255) / 256), 256, 0, c->st>>>(c->arr(), G, N, c0, m, include_zero, c->d_len.as<ull>(), dc);
        SLX_HIPCHK(hipGetLastError());
        SLX_CHK(slx_exclusive_sum(c->d_tmp, c->d_len.as<ull>(), c->d_at.as<ull>(), (size_t)m + 1, c->st));
        SLX_HIPCHK(hipMemcpyAsync(hc + COV_C_N, c->d_at.as<ull>() + m, 8, hipMemcpyDeviceToHost, c->st));
        SLX_HIPCHK(slx_wait_stream(c->st));
        const uint64_t bytes = hc[COV_C_N];
        if (!bytes) continue;
        SLX_CHK(c->d_text.ensure(bytes + 64));
        k_cov_bg_fill<<<(unsigned)((m + 255) / 256), 256, 0, c->st>>>(c->arr(), G, N, c0, m, include_zero, c->d_at.as<ull>(), c->d_text.as<uint8_t>());
        SLX_HIPCHK(hipGetLastError());
        for (uint64_t at = 0; at < bytes; at += COV_STAGE) {
            const uint64_t len = std::min<uint64_t>(COV_STAGE, bytes - at);
            CHBuf &h = c->h_text[cur];          // (not the one on its way to the file)
            SLX_CHK(h.ensure(len));
            SLX_HIPCHK(hipMemcpyAsync(h.p, c->d_text.as<uint8_t>() + at, len, hipMemcpyDeviceToHost, c->st));
            SLX_HIPCHK(slx_wait_stream(c->st));
            SLX_CHK(W.join());
            W.start(h.as<uint8_t>(), len);
            cur ^= 1;
        }
    }
    SLX_HIPCHK(hipMemcpyAsync(hc, dc, 8 * COV_C_N, hipMemcpyDeviceToHost, c->st));
    SLX_HIPCHK(slx_wait_stream(c->st));
    c->c_runs = (int64_t)hc[COV_C_RUNS];
    return W.join();
}

extern "C" int slx_cov_bedgraph(slx_cov *c, int tid, int include_zero, const char *path)
{
    SLX_CHK(slx_need(c, "slx_cov_bedgraph"));
    if (!path) { slx_set_error("slx_cov_bedgraph: null path"); return SLX_EINVAL; }
    if (tid != -1) SLX_CHK(cov_tid("slx_cov_bedgraph", c, tid));
    SLX_CHK(cov_settle(c));
    const bool is_stdout = !strcmp(path, "-");
    const int fd = is_stdout ? STDOUT_FILENO : ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) { slx_set_error("coverage: cannot create '%s': %s", path, strerror(errno)); return SLX_EIO; }
    CovWriter W{fd, path};
    int rc = cov_bedgraph_impl(c, tid, include_zero ? 1 : 0, W);
    if (W.on) { W.th.join(); W.on = false; }
    if (!is_stdout && ::close(fd) != 0 && rc == SLX_OK) { slx_set_error("coverage: cannot close '%s': %s", path, strerror(errno)); rc = SLX_EIO; }
    return rc;
}

extern "C" int slx_cov_clear(slx_cov *c)
{
    SLX_CHK(slx_need(c, "slx_cov_clear"));
    SLX_HIPCHK(hipMemsetAsync(c->d_arr.p, 0, 4 * c->total + 16, c->st));
    SLX_HIPCHK(slx_wait_stream(c->st));
    c->settled = false;
    return SLX_OK;
}

extern "C" int64_t slx_cov_counter(const slx_cov *c, const char *name)
{
    if (!c || !name) return -1;
    if (!strcmp(name, "records_seen")) return c->c_seen;
    if (!strcmp(name, "records_counted")) return c->c_counted;
    if (!strcmp(name, "long_records")) return c->c_long;
    if (!strcmp(name, "events_lds")) return c->c_lds;
    if (!strcmp(name, "events_global")) return c->c_global;
    if (!strcmp(name, "runs")) return c->c_runs;
    if (!strcmp(name, "us_add")) return (int64_t)c->us_add;
    if (!strcmp(name, "us_settle")) return (int64_t)c->us_settle;
    return -1;
}
