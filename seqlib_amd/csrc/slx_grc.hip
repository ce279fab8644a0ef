// slx_grc.hip -- interval queries on the GPU (include/seqlib_amd_grc.h): a collection's intervals -> a sorted index in HBM, mirrored on the host; batches of queries
// (intervals, or BAM records in HBM) -> pairs, clipped intervals, counts, widths; merge.  DESIGN.md section 9.12 has the argument.
//   build          hipCUB's stable radix sort twice (by pos2, then by (chr, pos1)), k_grc_gather, a max-scan and a sort of (chr, pos2) keys  dev_grc.h
//   k_grc_count    one lane per query: candidate range, exact count, the job lists of the two fill forms                                  grc_host.h grc_range, grc_count
//   k_grc_fill_*   one lane or one wave per query writes its hits at the offset the exclusive sum gave                                    grc_host.h grc_hit, grc_put
//   k_grc_records  a record's (tid, pos, end) as a query; per-subject counts from the batch's sorted starts and ends, no atomics          grc_host.h grc_record_iv
//   merge          k_grc_merge_flag, the exclusive sum, k_grc_merge_fill                                                                  grc_host.h grc_run_starts
// A host-only object (no GPU) is built with std::stable_sort and answers slx_grc_sorted, slx_grc_merged and slx_grc_query_host through the same bodies.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>
#include "slx_internal.h"
#include "slx_hip.h"
#include "seqlib_amd_grc.h"
#include "dev_grc.h"

typedef unsigned long long ull;
typedef SlxDevBuf<SlxMargin<4, 256>> GDBuf;
typedef SlxPinBuf<SlxMargin<4, 256>> GHBuf;

static_assert(sizeof(slx_grc_iv) == sizeof(grc_iv) && sizeof(grc_iv) == 16, "slx_grc_iv and grc_iv are one layout");

static const char GRC_NO_DEVICE[] = "no HIP device: interval batches are joined on MI355X only (no CPU fallback)";

struct slx_grc : SlxGpu<> {
    slx_grc() : SlxGpu(GRC_NO_DEVICE) {}
    uint32_t n = 0;
    grc_host_arrays H;          // the host mirror of the index
    uint32_t wave_range = 64, long_cigar = 64;
    uint64_t slice = 1ull << 20;
    GDBuf d_chr{*this}, d_p1{*this}, d_p2{*this}, d_perm{*this}, d_run{*this}, d_ends{*this}, d_strand{*this}, d_segchr{*this}, d_segbeg{*this};          // the index
    GDBuf d_q{*this}, d_cand{*this}, d_cnt32{*this}, d_cnt{*this}, d_at{*this}, d_lane{*this}, d_wave{*this}, d_ctr{*this}, d_tmp{*this}, d_qid{*this}, d_sid{*this}, d_c1{*this}, d_c2{*this}, d_width{*this};          // a join
    GDBuf d_in{*this}, d_off{*this}, d_ks{*this}, d_ke{*this}, d_ks2{*this}, d_ke2{*this}, d_long{*this}, d_subj{*this};          // records
    GDBuf d_a{*this}, d_b{*this}, d_c{*this}, d_d{*this}, d_iv{*this};          // build and merge scratch
    GHBuf h_ctr{*this};
    int64_t c_queries = 0, c_lane = 0, c_wave = 0, c_pairs = 0, c_records = 0, c_long = 0, c_merged = 0;
    double us_build = 0, us_count = 0, us_fill = 0, us_records = 0, us_merge = 0;
    grc_idx host_idx() const { return H.idx(); }
    grc_idx dev_idx() const
    {
        return grc_idx{d_chr.as<int32_t>(), d_p1.as<int32_t>(), d_p2.as<int32_t>(), d_perm.as<int32_t>(), d_run.as<int32_t>(), d_ends.as<int32_t>(), d_segchr.as<int32_t>(), d_strand.as<uint8_t>(),
                       d_segbeg.as<uint32_t>(), n, (uint32_t)H.seg_chr.size()};
    }
};

static inline unsigned grc_blocks(uint64_t n, unsigned per = 256) { return (unsigned)((n + per - 1) / per); }

extern "C" void slx_grc_free(slx_grc *g)
{
    if (!g) return;
    g->close();
    delete g;
}

// a radix sort over all bits of the key (hipCUB takes the count as an int)
template <class K, class V> static int grc_sort_pairs(slx_grc *g, const K *kin, K *kout, const V *vin, V *vout, uint32_t n)
{
    return slx_cub("hipcub::DeviceRadixSort::SortPairs (intervals)", g->d_tmp, 8, [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, kin, kout, vin, vout, (int)n, 0, (int)(8 * sizeof(K)), g->st); });
}
static int grc_sort_keys(slx_grc *g, const ull *kin, ull *kout, uint64_t n)
{
    return slx_cub("hipcub::DeviceRadixSort::SortKeys (intervals)", g->d_tmp, 8, [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortKeys(t, b, kin, kout, (int)n, 0, 64, g->st); });
}

static int grc_build_device(slx_grc *g, const slx_grc_iv *iv)
{
    const uint32_t n = g->n;
    const size_t n4 = 4 * (size_t)n + 16, n8 = 8 * (size_t)n + 16;
    hipStream_t st = g->st;
    SLX_CHK(g->d_chr.ensure(n4)); SLX_CHK(g->d_p1.ensure(n4)); SLX_CHK(g->d_p2.ensure(n4)); SLX_CHK(g->d_perm.ensure(n4)); SLX_CHK(g->d_run.ensure(n4)); SLX_CHK(g->d_ends.ensure(n4));
    SLX_CHK(g->d_strand.ensure((size_t)n + 16)); SLX_CHK(g->d_subj.ensure(n8));
    SLX_HIPCHK(hipMemsetAsync(g->d_subj.p, 0, n8, st));
    if (n) {
        SLX_CHK(g->d_iv.ensure(16 * (size_t)n)); SLX_CHK(g->d_a.ensure(n8)); SLX_CHK(g->d_b.ensure(n8)); SLX_CHK(g->d_c.ensure(n4)); SLX_CHK(g->d_d.ensure(n4));
        SLX_HIPCHK(hipMemcpyAsync(g->d_iv.p, iv, 16 * (size_t)n, hipMemcpyHostToDevice, st));
        SLX_HIPCHK(hipEventRecord(g->ev[0], st));
        const grc_iv *d_iv = g->d_iv.as<grc_iv>();
        uint32_t *k32 = g->d_a.as<uint32_t>(), *k32o = g->d_b.as<uint32_t>(), *idx = g->d_c.as<uint32_t>(), *by_p2 = g->d_d.as<uint32_t>();
        k_grc_key_p2<<<grc_blocks(n), 256, 0, st>>>(d_iv, n, k32, idx);
        SLX_HIPCHK(hipGetLastError());
        SLX_CHK(grc_sort_pairs(g, k32, k32o, idx, by_p2, n));
        ull *k64 = g->d_a.as<ull>(), *k64o = g->d_b.as<ull>();
        k_grc_key_chr_p1<<<grc_blocks(n), 256, 0, st>>>(d_iv, by_p2, n, k64);
        SLX_HIPCHK(hipGetLastError());
        SLX_CHK(grc_sort_pairs(g, k64, k64o, by_p2, idx, n));          // idx: the permutation
        k_grc_gather<<<grc_blocks(n), 256, 0, st>>>(d_iv, idx, n, g->d_chr.as<int32_t>(), g->d_p1.as<int32_t>(), g->d_p2.as<int32_t>(), g->d_strand.as<uint8_t>(), g->d_perm.as<int32_t>(), k64);
        SLX_HIPCHK(hipGetLastError());
        // (chr, p2) keys in k64: their max-scan into k64o, their sort into the query scratch
        SLX_CHK(slx_cub("hipcub::DeviceScan::InclusiveScan (intervals, build)", g->d_tmp, 8, [&](void *t, size_t &b) { return hipcub::DeviceScan::InclusiveScan(t, b, k64, k64o, hipcub::Max(), (int)n, st); }));
        SLX_CHK(g->d_ks.ensure(n8));
        SLX_CHK(grc_sort_keys(g, k64, g->d_ks.as<ull>(), n));
        k_grc_low_halves<<<grc_blocks(n), 256, 0, st>>>(k64o, g->d_ks.as<ull>(), n, g->d_run.as<int32_t>(), g->d_ends.as<int32_t>());
        SLX_HIPCHK(hipGetLastError());
        SLX_HIPCHK(hipEventRecord(g->ev[1], st));
        SLX_HIPCHK(hipMemcpyAsync(g->H.chr.data(), g->d_chr.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(hipMemcpyAsync(g->H.p1.data(), g->d_p1.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(hipMemcpyAsync(g->H.p2.data(), g->d_p2.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(hipMemcpyAsync(g->H.perm.data(), g->d_perm.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(hipMemcpyAsync(g->H.run_p2.data(), g->d_run.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(hipMemcpyAsync(g->H.ends.data(), g->d_ends.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(hipMemcpyAsync(g->H.strand.data(), g->d_strand.p, (size_t)n, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(slx_wait_stream(st));
        g->us_build += slx_ev_us(g->ev[0], g->ev[1]);
    }
    grc_segments(g->H);
    const size_t ns = g->H.seg_chr.size();
    SLX_CHK(g->d_segchr.ensure(4 * ns + 16)); SLX_CHK(g->d_segbeg.ensure(4 * (ns + 1) + 16));
    if (ns) SLX_HIPCHK(hipMemcpyAsync(g->d_segchr.p, g->H.seg_chr.data(), 4 * ns, hipMemcpyHostToDevice, st));
    SLX_HIPCHK(hipMemcpyAsync(g->d_segbeg.p, g->H.seg_beg.data(), 4 * (ns + 1), hipMemcpyHostToDevice, st));
    SLX_CHK(g->d_ctr.ensure(8 * GRC_C_N)); SLX_CHK(g->h_ctr.ensure(8 * (GRC_C_N + 2)));
    SLX_HIPCHK(slx_wait_stream(st));
    return SLX_OK;
}

static int grc_create_impl(slx_grc *g, int device, const slx_grc_iv *iv, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        if (iv[i].pos2 < iv[i].pos1) { slx_set_error("slx_grc_create: interval %lld ends (%d) before it starts (%d)", (long long)i, iv[i].pos2, iv[i].pos1); return SLX_EINVAL; }
    g->n = (uint32_t)n;
    g->H.resize((uint32_t)n);
    // SLX_GRC_HOST never asks the runtime; SLX_GRC_AUTO is the current device, or host only without one
    if (device != SLX_GRC_HOST) SLX_CHK(g->open(device == SLX_GRC_AUTO ? -1 : device, "slx_grc_create", GRC_NO_DEVICE, device == SLX_GRC_AUTO));
    if (g->device < 0) { grc_build_host((const grc_iv *)iv, g->n, g->H); return SLX_OK; }          // host only
    return grc_build_device(g, iv);
}

extern "C" int slx_grc_create(int device, const slx_grc_iv *iv, int64_t n, slx_grc **out)
{
    if (!out || n < 0 || (n && !iv)) { slx_set_error("slx_grc_create: null or negative argument"); return SLX_EINVAL; }
    *out = nullptr;
    if (n >= 0x7fffffffll) { slx_set_error("slx_grc_create: 2^31 intervals or more"); return SLX_EINVAL; }
    if (device < SLX_GRC_AUTO) { slx_set_error("slx_grc_create: device %d", device); return SLX_EINVAL; }
    return slx_create(out, slx_grc_free, [&](slx_grc *g) { return grc_create_impl(g, device, iv, n); });
}

extern "C" int slx_grc_set(slx_grc *g, const char *key, int64_t v)
{
    if (!g || !key) { slx_set_error("slx_grc_set: null argument"); return SLX_EINVAL; }
    auto in = [&](int64_t lo, int64_t hi) { if (v >= lo && v <= hi) return true; slx_set_error("slx_grc_set: %s %lld outside [%lld, %lld]", key, (long long)v, (long long)lo, (long long)hi); return false; };
    if (!strcmp(key, "wave_range")) { if (!in(0, 1 << 20)) return SLX_EINVAL; g->wave_range = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "slice_queries")) { if (!in(64, 1 << 24)) return SLX_EINVAL; g->slice = (uint64_t)v; return SLX_OK; }
    if (!strcmp(key, "long_cigar")) { if (!in(0, 1 << 20)) return SLX_EINVAL; g->long_cigar = (uint32_t)v; return SLX_OK; }
    slx_set_error("slx_grc_set: unknown key '%s'", key);
    return SLX_EINVAL;
}

extern "C" int slx_grc_sorted(const slx_grc *g, slx_grc_iv *out, int32_t *perm, int32_t *run_p2, int32_t *ends)
{
    if (!g) { slx_set_error("slx_grc_sorted: null object"); return SLX_EINVAL; }
    for (uint32_t i = 0; i < g->n; ++i) {
        if (out) { memset(&out[i], 0, sizeof out[i]); out[i].chr = g->H.chr[i]; out[i].pos1 = g->H.p1[i]; out[i].pos2 = g->H.p2[i]; out[i].strand = (char)g->H.strand[i]; }
        if (perm) perm[i] = g->H.perm[i];
        if (run_p2) run_p2[i] = g->H.run_p2[i];
        if (ends) ends[i] = g->H.ends[i];
    }
    return SLX_OK;
}

static int grc_merge_device(slx_grc *g, std::vector<grc_iv> &m)
{
    const uint32_t n = g->n;
    hipStream_t st = g->st;
    SLX_CHK(g->d_a.ensure(8 * ((size_t)n + 1))); SLX_CHK(g->d_b.ensure(8 * ((size_t)n + 1))); SLX_CHK(g->d_iv.ensure(16 * (size_t)n));
    SLX_HIPCHK(hipEventRecord(g->ev[0], st));
    SLX_HIPCHK(hipMemsetAsync(g->d_iv.p, 0, 16 * (size_t)n, st));
    k_grc_merge_flag<<<grc_blocks((uint64_t)n + 1), 256, 0, st>>>(g->dev_idx(), g->d_a.as<ull>());
    SLX_HIPCHK(hipGetLastError());
    SLX_CHK(slx_exclusive_sum(g->d_tmp, g->d_a.as<ull>(), g->d_b.as<ull>(), (size_t)n + 1, st));
    k_grc_merge_fill<<<grc_blocks(n), 256, 0, st>>>(g->dev_idx(), g->d_a.as<ull>(), g->d_b.as<ull>(), g->d_iv.as<grc_iv>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(g->ev[1], st));
    ull *h = g->h_ctr.as<ull>();
    SLX_HIPCHK(hipMemcpyAsync(h + GRC_C_N, g->d_b.as<ull>() + n, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    m.resize((size_t)h[GRC_C_N]);
    if (!m.empty()) SLX_HIPCHK(hipMemcpy(m.data(), g->d_iv.p, 16 * m.size(), hipMemcpyDeviceToHost));
    g->us_merge += slx_ev_us(g->ev[0], g->ev[1]);
    return SLX_OK;
}

extern "C" int slx_grc_merged(slx_grc *g, slx_grc_iv *out, int64_t cap, int64_t *n_out)
{
    if (!g || !n_out || cap < 0 || (cap && !out)) { slx_set_error("slx_grc_merged: null or negative argument"); return SLX_EINVAL; }
    *n_out = 0;
    std::vector<grc_iv> m;
    if (g->device >= 0 && g->n) {
        SLX_HIPCHK(hipSetDevice(g->device));
        SLX_CHK(grc_merge_device(g, m));
    } else {
        const grc_idx X = g->host_idx();
        for (uint32_t i = 0; i < g->n; ++i) {
            if (grc_run_starts(X, i)) { grc_iv v; memset(&v, 0, sizeof v); v.chr = X.chr[i]; v.pos1 = X.p1[i]; v.strand = (char)X.strand[i]; m.push_back(v); }
            m.back().pos2 = X.run_p2[i];
        }
    }
    g->c_merged = (int64_t)m.size();
    *n_out = (int64_t)m.size();
    if ((int64_t)m.size() > cap) { slx_set_error("slx_grc_merged: %zu intervals, out holds %lld", m.size(), (long long)cap); return SLX_EINVAL; }
    if (!m.empty()) memcpy(out, m.data(), 16 * m.size());
    return SLX_OK;
}

static int grc_check_queries(const char *who, const slx_grc_iv *q, int64_t nq)
{
    for (int64_t i = 0; i < nq; ++i)
        if (q[i].pos2 < q[i].pos1) { slx_set_error("%s: query %lld ends (%d) before it starts (%d)", who, (long long)i, q[i].pos2, q[i].pos1); return SLX_EINVAL; }
    return SLX_OK;
}

extern "C" int slx_grc_query_host(const slx_grc *g, const slx_grc_iv *q, int ignore_strand, int contained, int32_t *subject_id, int32_t *pos1, int32_t *pos2, int64_t cap, int64_t *n_out,
                                  int64_t *width)
{
    if (!g || !q || !n_out || cap < 0) { slx_set_error("slx_grc_query_host: null or negative argument"); return SLX_EINVAL; }
    *n_out = 0;
    if (width) *width = 0;
    SLX_CHK(grc_check_queries("slx_grc_query_host", q, 1));
    const grc_idx X = g->host_idx();
    grc_iv v;
    memcpy(&v, q, sizeof v);
    const uint32_t flags = (ignore_strand ? GRC_IGNORE_STRAND : 0u) | (contained ? GRC_CONTAINED : 0u);
    const grc_cand C = grc_range(X, v);
    const uint64_t k = grc_count(X, v, flags, C);
    *n_out = (int64_t)k;
    if (width && k) {          // the clipped hits, whether or not the caller takes them
        std::vector<int32_t> a(k), b(k);
        (void)grc_fill(X, v, flags, C.lo, C.hi, nullptr, a.data(), b.data(), k);
        *width = (int64_t)grc_width(a.data(), b.data(), k);
    }
    if (cap && k) (void)grc_fill(X, v, flags, C.lo, C.hi, subject_id, pos1, pos2, (uint64_t)cap);
    if ((int64_t)k > cap && (subject_id || pos1 || pos2)) { slx_set_error("slx_grc_query_host: %llu hits, the arrays hold %lld", (ull)k, (long long)cap); return SLX_EINVAL; }
    return SLX_OK;
}

// ---- a join of the nq queries in d_q.  pairs: fill the pair arrays and the widths; the stream has drained on return and h_ctr holds the counters
static int grc_join(slx_grc *g, uint64_t nq, uint32_t flags, bool pairs, uint64_t *n_pairs)
{
    hipStream_t st = g->st;
    *n_pairs = 0;
    g->c_lane = g->c_wave = g->c_pairs = 0;
    g->c_queries += (int64_t)nq;
    SLX_CHK(g->d_cand.ensure(8 * nq + 8)); SLX_CHK(g->d_cnt32.ensure(4 * nq + 4)); SLX_CHK(g->d_cnt.ensure(8 * (nq + 1))); SLX_CHK(g->d_at.ensure(8 * (nq + 1)));
    SLX_CHK(g->d_lane.ensure(4 * nq + 4)); SLX_CHK(g->d_wave.ensure(4 * nq + 4)); SLX_CHK(g->d_width.ensure(8 * nq + 8));
    ull *hc = g->h_ctr.as<ull>(), *dc = g->d_ctr.as<ull>();
    const grc_idx X = g->dev_idx();
    const grc_iv *q = g->d_q.as<grc_iv>();
    SLX_HIPCHK(hipMemsetAsync(dc + GRC_C_NLANE, 0, 16, st));
    SLX_HIPCHK(hipMemsetAsync(g->d_cnt.as<ull>() + nq, 0, 8, st));
    SLX_HIPCHK(hipEventRecord(g->ev[0], st));
    for (uint64_t q0 = 0; q0 < nq; q0 += g->slice) {
        const uint64_t q1 = std::min(nq, q0 + g->slice);
        k_grc_count<<<grc_blocks(q1 - q0), 256, 0, st>>>(X, q, q0, q1, flags, g->wave_range, pairs ? 1 : 0, g->d_cand.as<uint2>(), g->d_cnt32.as<uint32_t>(), g->d_cnt.as<ull>(),
                                                         g->d_lane.as<uint32_t>(), g->d_wave.as<uint32_t>(), dc);
        SLX_HIPCHK(hipGetLastError());
    }
    SLX_CHK(slx_exclusive_sum(g->d_tmp, g->d_cnt.as<ull>(), g->d_at.as<ull>(), (size_t)nq + 1, st));
    SLX_HIPCHK(hipEventRecord(g->ev[1], st));
    SLX_HIPCHK(hipMemcpyAsync(hc, dc, 8 * GRC_C_N, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync(hc + GRC_C_N, g->d_at.as<ull>() + nq, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    g->us_count += slx_ev_us(g->ev[0], g->ev[1]);
    const uint64_t total = hc[GRC_C_N], n_lane = hc[GRC_C_NLANE], n_wave = hc[GRC_C_NWAVE];
    *n_pairs = total; g->c_pairs = (int64_t)total;
    if (!pairs) return SLX_OK;
    g->c_lane = (int64_t)n_lane; g->c_wave = (int64_t)n_wave;
    SLX_CHK(g->d_qid.ensure(4 * total + 4)); SLX_CHK(g->d_sid.ensure(4 * total + 4)); SLX_CHK(g->d_c1.ensure(4 * total + 4)); SLX_CHK(g->d_c2.ensure(4 * total + 4));
    const grc_out O = {g->d_qid.as<int32_t>(), g->d_sid.as<int32_t>(), g->d_c1.as<int32_t>(), g->d_c2.as<int32_t>()};
    SLX_HIPCHK(hipEventRecord(g->ev[0], st));
    if (n_lane) {
        k_grc_fill_lane<<<grc_blocks(n_lane), 256, 0, st>>>(X, q, g->d_lane.as<uint32_t>(), n_lane, flags, g->d_cand.as<uint2>(), g->d_at.as<ull>(), g->d_cnt32.as<uint32_t>(), O);
        SLX_HIPCHK(hipGetLastError());
    }
    if (n_wave) {
        k_grc_fill_wave<<<grc_blocks(n_wave, 4), 256, 0, st>>>(X, q, g->d_wave.as<uint32_t>(), n_wave, flags, g->d_cand.as<uint2>(), g->d_at.as<ull>(), g->d_cnt32.as<uint32_t>(), O);
        SLX_HIPCHK(hipGetLastError());
    }
    if (nq) {
        k_grc_width<<<grc_blocks(nq), 256, 0, st>>>(nq, g->d_at.as<ull>(), g->d_cnt32.as<uint32_t>(), O.c1, O.c2, g->d_width.as<ull>());
        SLX_HIPCHK(hipGetLastError());
    }
    SLX_HIPCHK(hipEventRecord(g->ev[1], st));
    SLX_HIPCHK(slx_wait_stream(st));
    g->us_fill += slx_ev_us(g->ev[0], g->ev[1]);
    return SLX_OK;
}

extern "C" void slx_grc_result_free(slx_grc_result *r)
{
    if (!r) return;
    free(r->count); free(r->width); free(r->offset); free(r->query_id); free(r->subject_id); free(r->pos1); free(r->pos2);
    memset(r, 0, sizeof *r);
}

template <class T> static int grc_down(T **dst, const void *src, uint64_t n)
{
    *dst = (T *)malloc(sizeof(T) * (n ? n : 1));
    if (!*dst) { slx_set_error("cannot allocate %llu bytes for a result", (ull)(sizeof(T) * n)); return SLX_ENOMEM; }
    if (n) SLX_HIPCHK(hipMemcpy(*dst, src, sizeof(T) * n, hipMemcpyDeviceToHost));
    return SLX_OK;
}

static int grc_result_impl(slx_grc *g, uint64_t nq, uint64_t total, bool pairs, slx_grc_result *r)
{
    r->n_queries = (int64_t)nq; r->n_pairs = (int64_t)total;
    SLX_CHK(grc_down(&r->count, g->d_cnt32.p, nq)); SLX_CHK(grc_down(&r->offset, g->d_at.p, nq + 1));
    r->d_count = g->d_cnt32.p; r->d_offset = g->d_at.p;
    if (!pairs) return SLX_OK;
    SLX_CHK(grc_down(&r->width, g->d_width.p, nq)); SLX_CHK(grc_down(&r->query_id, g->d_qid.p, total)); SLX_CHK(grc_down(&r->subject_id, g->d_sid.p, total));
    SLX_CHK(grc_down(&r->pos1, g->d_c1.p, total)); SLX_CHK(grc_down(&r->pos2, g->d_c2.p, total));
    r->d_width = g->d_width.p; r->d_query_id = g->d_qid.p; r->d_subject_id = g->d_sid.p; r->d_pos1 = g->d_c1.p; r->d_pos2 = g->d_c2.p;
    return SLX_OK;
}
static int grc_result(slx_grc *g, uint64_t nq, uint64_t total, bool pairs, slx_grc_result *r)
{
    memset(r, 0, sizeof *r);
    const int rc = grc_result_impl(g, nq, total, pairs, r);
    if (rc != SLX_OK) slx_grc_result_free(r);
    return rc;
}

static int grc_upload_queries(const char *who, slx_grc *g, const slx_grc_iv *q, int64_t nq)
{
    if (nq < 0 || (nq && !q)) { slx_set_error("%s: null or negative argument", who); return SLX_EINVAL; }
    if (nq >= 0x7fffffffll) { slx_set_error("%s: 2^31 queries or more in one call", who); return SLX_EUNSUPPORTED; }
    SLX_CHK(grc_check_queries(who, q, nq));
    SLX_CHK(g->d_q.ensure(16 * (size_t)nq + 16));
    if (nq) SLX_HIPCHK(hipMemcpyAsync(g->d_q.p, q, 16 * (size_t)nq, hipMemcpyHostToDevice, g->st));
    return SLX_OK;
}

extern "C" int slx_grc_overlaps(slx_grc *g, const slx_grc_iv *q, int64_t nq, int ignore_strand, slx_grc_result *res)
{
    SLX_CHK(slx_need(g, "slx_grc_overlaps"));
    if (!res) { slx_set_error("slx_grc_overlaps: null result"); return SLX_EINVAL; }
    memset(res, 0, sizeof *res);
    SLX_CHK(grc_upload_queries("slx_grc_overlaps", g, q, nq));
    uint64_t total = 0;
    SLX_CHK(grc_join(g, (uint64_t)nq, ignore_strand ? GRC_IGNORE_STRAND : 0u, true, &total));
    return grc_result(g, (uint64_t)nq, total, true, res);
}

extern "C" int slx_grc_count(slx_grc *g, const slx_grc_iv *q, int64_t nq, int ignore_strand, int contained, uint32_t *count)
{
    SLX_CHK(slx_need(g, "slx_grc_count"));
    if (nq > 0 && !count) { slx_set_error("slx_grc_count: null output"); return SLX_EINVAL; }
    SLX_CHK(grc_upload_queries("slx_grc_count", g, q, nq));
    uint64_t total = 0;
    SLX_CHK(grc_join(g, (uint64_t)nq, (ignore_strand ? GRC_IGNORE_STRAND : 0u) | (contained ? GRC_CONTAINED : 0u), false, &total));
    if (nq) SLX_HIPCHK(hipMemcpy(count, g->d_cnt32.p, 4 * (size_t)nq, hipMemcpyDeviceToHost));
    return SLX_OK;
}

// the records of d_s as queries, the per-subject counts, the join
static int grc_records(slx_grc *g, const uint8_t *d_s, uint64_t n_bytes, const ull *d_off, uint64_t n, bool pairs, slx_grc_result *res)
{
    if (res) memset(res, 0, sizeof *res);
    if (n >= 0x7fffffffull) { slx_set_error("intervals: 2^31 records or more in one batch"); return SLX_EUNSUPPORTED; }
    hipStream_t st = g->st;
    uint64_t total = 0;
    if (n) {
        SLX_CHK(g->d_q.ensure(16 * n + 16)); SLX_CHK(g->d_ks.ensure(8 * n + 8)); SLX_CHK(g->d_ke.ensure(8 * n + 8)); SLX_CHK(g->d_ks2.ensure(8 * n + 8)); SLX_CHK(g->d_ke2.ensure(8 * n + 8));
        SLX_CHK(g->d_long.ensure(4 * n + 4));
        ull *hc = g->h_ctr.as<ull>(), *dc = g->d_ctr.as<ull>();
        memset(hc, 0, 8 * GRC_C_N);
        hc[GRC_C_ERR] = ~0ull;
        SLX_HIPCHK(hipMemcpyAsync(dc, hc, 8 * GRC_C_N, hipMemcpyHostToDevice, st));
        SLX_HIPCHK(hipEventRecord(g->ev[0], st));
        k_grc_records<<<grc_blocks(n), 256, 0, st>>>(d_s, n_bytes, d_off, n, g->long_cigar, g->d_q.as<grc_iv>(), g->d_ks.as<ull>(), g->d_ke.as<ull>(), g->d_long.as<uint32_t>(), dc);
        SLX_HIPCHK(hipGetLastError());
        SLX_HIPCHK(hipMemcpyAsync(hc, dc, 8 * GRC_C_N, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(slx_wait_stream(st));
        if (hc[GRC_C_ERR] != ~0ull) {
            slx_set_error("intervals: record %llu of the batch: its fields pass its block_size, or its extent is not block_size + 4 inside the stream", hc[GRC_C_ERR]);
            return SLX_EIO;
        }
        const uint64_t n_long = hc[GRC_C_NLONG];
        if (n_long) {
            k_grc_records_long<<<grc_blocks(n_long, 4), 256, 0, st>>>(d_s, d_off, g->d_long.as<uint32_t>(), n_long, g->d_q.as<grc_iv>(), g->d_ks.as<ull>(), g->d_ke.as<ull>());
            SLX_HIPCHK(hipGetLastError());
        }
        if (g->n) {
            SLX_CHK(grc_sort_keys(g, g->d_ks.as<ull>(), g->d_ks2.as<ull>(), n));
            SLX_CHK(grc_sort_keys(g, g->d_ke.as<ull>(), g->d_ke2.as<ull>(), n));
            k_grc_subject_counts<<<grc_blocks(g->n), 256, 0, st>>>(g->dev_idx(), g->d_ks2.as<ull>(), g->d_ke2.as<ull>(), n, g->d_subj.as<long long>());
            SLX_HIPCHK(hipGetLastError());
        }
        SLX_HIPCHK(hipEventRecord(g->ev[1], st));
        SLX_HIPCHK(slx_wait_stream(st));
        g->us_records += slx_ev_us(g->ev[0], g->ev[1]);
        g->c_records += (int64_t)n; g->c_long += (int64_t)n_long;
    }
    if (!res) return SLX_OK;
    SLX_CHK(grc_join(g, n, GRC_IGNORE_STRAND, pairs, &total));
    return grc_result(g, n, total, pairs, res);
}

extern "C" int slx_grc_overlaps_device(slx_grc *g, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records, int want_pairs, slx_grc_result *res)
{
    SLX_CHK(slx_need(g, "slx_grc_overlaps_device"));
    SLX_CHK(slx_batch_args("slx_grc_overlaps_device", d_stream, n_bytes, d_rec_off, n_records));
    return grc_records(g, (const uint8_t *)d_stream, (uint64_t)n_bytes, (const ull *)d_rec_off, (uint64_t)n_records, want_pairs != 0, res);
}

extern "C" int slx_grc_overlaps_host(slx_grc *g, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records, int want_pairs, slx_grc_result *res)
{
    SLX_CHK(slx_need(g, "slx_grc_overlaps_host"));
    SLX_CHK(slx_batch_args("slx_grc_overlaps_host", stream, n_bytes, rec_off, n_records));
    if (n_records) SLX_CHK(slx_batch_stage(g->d_in, g->d_off, 8, stream, n_bytes, rec_off, n_records, g->st));
    return grc_records(g, g->d_in.as<uint8_t>(), (uint64_t)n_bytes, g->d_off.as<ull>(), (uint64_t)n_records, want_pairs != 0, res);
}

extern "C" int slx_grc_subject_counts(slx_grc *g, int64_t *out)
{
    SLX_CHK(slx_need(g, "slx_grc_subject_counts"));
    if (g->n && !out) { slx_set_error("slx_grc_subject_counts: null output"); return SLX_EINVAL; }
    if (g->n) SLX_HIPCHK(hipMemcpy(out, g->d_subj.p, 8 * (size_t)g->n, hipMemcpyDeviceToHost));
    return SLX_OK;
}

extern "C" int slx_grc_clear_counts(slx_grc *g)
{
    SLX_CHK(slx_need(g, "slx_grc_clear_counts"));
    SLX_HIPCHK(hipMemsetAsync(g->d_subj.p, 0, 8 * (size_t)g->n + 16, g->st));
    SLX_HIPCHK(slx_wait_stream(g->st));
    return SLX_OK;
}

extern "C" int64_t slx_grc_counter(const slx_grc *g, const char *name)
{
    if (!g || !name) return -1;
    if (!strcmp(name, "device")) return g->device;
    if (!strcmp(name, "subjects")) return g->n;
    if (!strcmp(name, "chrs")) return (int64_t)g->H.seg_chr.size();
    if (!strcmp(name, "queries")) return g->c_queries;
    if (!strcmp(name, "queries_lane")) return g->c_lane;
    if (!strcmp(name, "queries_wave")) return g->c_wave;
    if (!strcmp(name, "pairs")) return g->c_pairs;
    if (!strcmp(name, "records")) return g->c_records;
    if (!strcmp(name, "long_records")) return g->c_long;
    if (!strcmp(name, "merged")) return g->c_merged;
    if (!strcmp(name, "us_build")) return (int64_t)g->us_build;
    if (!strcmp(name, "us_count")) return (int64_t)g->us_count;
    if (!strcmp(name, "us_fill")) return (int64_t)g->us_fill;
    if (!strcmp(name, "us_records")) return (int64_t)g->us_records;
    if (!strcmp(name, "us_merge")) return (int64_t)g->us_merge;
    return -1;
}
