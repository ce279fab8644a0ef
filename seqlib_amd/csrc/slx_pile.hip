// slx_pile.hip -- per-base pileup on the GPU (include/seqlib_amd_pile.h): block_size-prefixed BAM records in HBM -> 15 planes of int32 over one window of one
// contig, read back as planes, as one position's counts or as the compacted list of candidate sites against a reference in HBM.  DESIGN.md section 9.16 has
// the argument.
//   k_pile_events<G>    a group of G lanes per record, a block per slice of records: eligibility, the walk, one add per base -- into an LDS window anchored at
//                       the slice's first eligible record where it falls inside, into HBM otherwise; the window is flushed at the block's end   pile_host.h pile_record
//   k_pile_events_long  one wave per record with more than long_cigar ops or long_read bases (a compacted list k_pile_events fills)             pile_host.h pile_record
//   k_pile_site_flag / hipCUB exclusive sum / k_pile_site_fill   the candidate sites, a lane per four positions                                 pile_host.h pile_site
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "slx_internal.h"
#include "slx_hip.h"
#include "seqlib_amd_pile.h"
#include "dev_pile.h"

typedef unsigned long long ull;
#define PILE_LDS_MAX 1024u          // positions: 15 planes * 4 bytes make them 60 KiB
#define PILE_LDS_DEFAULT 512u       // profiles/NOTES_pile.md

typedef SlxDevBuf<SlxMargin<4, 256>> PDBuf;
typedef SlxPinBuf<SlxMargin<4, 256>> PHBuf;

static const char PILE_NO_DEVICE[] = "no HIP device: the pileup is computed on MI355X only (no CPU fallback)";

struct slx_pile : SlxTwoPass {
    slx_pile() : SlxTwoPass(PILE_NO_DEVICE) {}
    std::vector<int64_t> len;
    std::vector<std::string> names;
    pile_par par = {0, 0, 0, 0, 0, 0x704u, 64u, 1024u};
    int64_t L = 0;
    uint64_t stride = 0;
    uint32_t lds_window = PILE_LDS_DEFAULT, slice = 1024, group = 16;
    SlxDevBuf<SlxExact> d_arr{*this};
    PDBuf d_in{*this}, d_off{*this}, d_tmp{*this}, d_n4{*this}, d_at{*this}, d_sites{*this};
    int64_t n_sites = -1;          // n_sites -1: no slx_pile_sites yet
    double us_sites = 0;
    int32_t *arr() const { return d_arr.as<int32_t>(); }
    size_t arr_bytes() const { return 4 * (size_t)PILE_PLANES * stride + 16; }
};

extern "C" void slx_pile_free(slx_pile *p)
{
    if (!p) return;
    p->close();
    delete p;
}

static int pile_create_impl(slx_pile *p, int device, int n_ref, const int64_t *ref_len, const char *const *ref_names, const slx_bam_region *win)
{
    for (int i = 0; i < n_ref; ++i) {
        if (ref_len[i] < 0 || ref_len[i] > 0x7fffffffll) { slx_set_error("slx_pile_create: contig %d has length %lld, outside [0, 2^31 - 1]", i, (long long)ref_len[i]); return SLX_EINVAL; }
        p->len.push_back(ref_len[i]);
        p->names.push_back(ref_names && ref_names[i] ? ref_names[i] : std::to_string(i));
    }
    if (win->tid < 0 || win->tid >= n_ref || win->beg > win->end) { slx_set_error("slx_pile_create: the window names contig %d of %d, or ends before it begins", win->tid, n_ref); return SLX_EINVAL; }
    const int64_t len = p->len[(size_t)win->tid];
    p->par.tid = win->tid;
    p->par.beg = std::min(std::max<int64_t>(win->beg, 0), len);
    p->par.end = std::min(std::max<int64_t>(win->end, p->par.beg), len);
    p->L = p->par.end - p->par.beg;
    p->stride = pile_stride(p->L);
    SLX_CHK(p->open(device, "slx_pile_create", PILE_NO_DEVICE, true));
    if (p->device < 0) return SLX_OK;          // host only
    SLX_CHK(p->d_arr.ensure(p->arr_bytes()));
    SLX_HIPCHK(hipMemsetAsync(p->d_arr.p, 0, p->arr_bytes(), p->st));
    SLX_CHK(p->d_cnt.ensure(8 * SLX_ADD_N)); SLX_CHK(p->h_cnt.ensure(8 * (SLX_ADD_N + 1)));
    SLX_HIPCHK(slx_wait_stream(p->st));
    return SLX_OK;
}

extern "C" int slx_pile_create(int device, int n_ref, const int64_t *ref_len, const char *const *ref_names, const slx_bam_region *window, slx_pile **out)
{
    if (!out || n_ref < 0 || (n_ref && !ref_len)) { slx_set_error("slx_pile_create: null or negative argument"); return SLX_EINVAL; }
    *out = nullptr;
    if (!window) { slx_set_error("slx_pile_create: a window is mandatory (a whole contig is [0, its length))"); return SLX_EINVAL; }
    return slx_create(out, slx_pile_free, [&](slx_pile *p) { return pile_create_impl(p, device, n_ref, ref_len, ref_names, window); });
}

extern "C" int slx_pile_set(slx_pile *p, const char *key, int64_t v)
{
    if (!p || !key) { slx_set_error("slx_pile_set: null argument"); return SLX_EINVAL; }
    auto in = [&](int64_t lo, int64_t hi) { if (v >= lo && v <= hi) return true; slx_set_error("slx_pile_set: %s %lld outside [%lld, %lld]", key, (long long)v, (long long)lo, (long long)hi); return false; };
    // (a host-only object checks the arguments, then says what every other entry says)
    auto done = [&]() { if (p->device >= 0) return (int)SLX_OK; slx_set_error("slx_pile_set: %s", PILE_NO_DEVICE); return (int)SLX_ENODEVICE; };
    if (!strcmp(key, "min_mapq")) { if (!in(0, 255)) return SLX_EINVAL; SLX_CHK(done()); p->par.min_mapq = (int32_t)v; return SLX_OK; }
    if (!strcmp(key, "min_baseq")) { if (!in(0, 255)) return SLX_EINVAL; SLX_CHK(done()); p->par.min_baseq = (int32_t)v; return SLX_OK; }
    if (!strcmp(key, "exclude_flags")) { if (!in(0, 0xffff)) return SLX_EINVAL; SLX_CHK(done()); p->par.exclude_flags = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "long_cigar")) { if (!in(0, 1 << 20)) return SLX_EINVAL; SLX_CHK(done()); p->par.long_cigar = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "long_read")) { if (!in(0, 0x7fffffffll)) return SLX_EINVAL; SLX_CHK(done()); p->par.long_read = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "lds_window")) { if (!in(0, PILE_LDS_MAX)) return SLX_EINVAL; SLX_CHK(done()); p->lds_window = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "slice_records")) { if (!in(64, 1 << 20)) return SLX_EINVAL; SLX_CHK(done()); p->slice = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "group_lanes")) {
        if (v != 16 && v != 32 && v != 64) { slx_set_error("slx_pile_set: group_lanes %lld is not 16, 32 or 64", (long long)v); return SLX_EINVAL; }
        SLX_CHK(done());
        p->group = (uint32_t)v;
        return SLX_OK;
    }
    slx_set_error("slx_pile_set: unknown key '%s'", key);
    return SLX_EINVAL;
}

// the records of d_s (n_bytes, offsets d_off) into the planes; the stream has drained on return
static int pile_add(slx_pile *p, const uint8_t *d_s, uint64_t n_bytes, const ull *d_off, uint64_t n)
{
    if (n == 0) return SLX_OK;
    hipStream_t st = p->st;
    ull *dc = p->d_cnt.as<ull>();
    const unsigned blocks = (unsigned)((n + p->slice - 1) / p->slice);
    const uint32_t lstride = (p->lds_window + 31u) & ~31u;
    const size_t lds_bytes = 4 * (size_t)PILE_PLANES * lstride;
    return slx_two_pass_add(*p, "pileup", n, SLX_ADD_N,
        [&]() {
            switch (p->group) {
            case 16: k_pile_events<16><<<blocks, 256, lds_bytes, st>>>(d_s, n_bytes, d_off, n, p->par, p->arr(), p->stride, p->slice, p->lds_window, lstride, p->d_long.as<ull>(), dc); break;
            case 32: k_pile_events<32><<<blocks, 256, lds_bytes, st>>>(d_s, n_bytes, d_off, n, p->par, p->arr(), p->stride, p->slice, p->lds_window, lstride, p->d_long.as<ull>(), dc); break;
            default: k_pile_events<64><<<blocks, 256, lds_bytes, st>>>(d_s, n_bytes, d_off, n, p->par, p->arr(), p->stride, p->slice, p->lds_window, lstride, p->d_long.as<ull>(), dc); break;
            }
        },
        [&](uint64_t n_long) { k_pile_events_long<<<(unsigned)((n_long + 3) / 4), 256, 0, st>>>(d_s, d_off, p->d_long.as<ull>(), n_long, p->par, p->arr(), p->stride, dc); });
}

extern "C" int slx_pile_add_device(slx_pile *p, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records)
{
    SLX_CHK(slx_need(p, "slx_pile_add_device"));
    SLX_CHK(slx_batch_args("slx_pile_add_device", d_stream, n_bytes, d_rec_off, n_records));
    return pile_add(p, (const uint8_t *)d_stream, (uint64_t)n_bytes, (const ull *)d_rec_off, (uint64_t)n_records);
}

extern "C" int slx_pile_add_host(slx_pile *p, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records)
{
    SLX_CHK(slx_need(p, "slx_pile_add_host"));
    SLX_CHK(slx_batch_args("slx_pile_add_host", stream, n_bytes, rec_off, n_records));
    if (n_records == 0) return SLX_OK;
    SLX_CHK(slx_batch_stage(p->d_in, p->d_off, 8, stream, n_bytes, rec_off, n_records, p->st));
    return pile_add(p, p->d_in.as<uint8_t>(), (uint64_t)n_bytes, p->d_off.as<ull>(), (uint64_t)n_records);
}

struct PileHostSink {
    int32_t *plane; int64_t *pos, cap, n;
    void operator()(uint32_t pl, int64_t x) { if (n < cap) { plane[n] = (int32_t)pl; pos[n] = x; } ++n; }
};

extern "C" int slx_pile_record_events(const uint8_t *rec, int64_t n, int min_baseq, int64_t clip_beg, int64_t clip_end, int32_t *plane, int64_t *pos, int64_t cap, int64_t *n_out)
{
    if (!rec || n < 0 || !n_out || cap < 0 || (cap && (!plane || !pos)) || min_baseq < 0 || min_baseq > 255) { slx_set_error("slx_pile_record_events: null, negative or unknown argument"); return SLX_EINVAL; }
    *n_out = 0;
    pile_par P = {clip_beg, clip_end, 0, 0, min_baseq, 0u, 1u << 20, 0x7fffffffu};
    rf_feat F;
    if (!rf_fixed(rec, (uint64_t)n, &F)) { slx_set_error("pileup: the record's fields pass its block_size, or its extent is not block_size + 4"); return SLX_EIO; }
    P.tid = F.tid;          // (whatever contig the record names stands for the window's)
    if (pile_head(rec, (uint64_t)n, P, &F) == PILE_R_SKIP) return SLX_OK;
    PileHostSink S = {plane, pos, cap, 0};
    pile_record(F, P, 0u, 1u, lanes_one(), S);
    *n_out = S.n;
    if (S.n > cap) { slx_set_error("slx_pile_record_events: %lld events, out holds %lld", (long long)S.n, (long long)cap); return SLX_EINVAL; }
    return SLX_OK;
}

static int pile_plane(const char *who, int plane)
{
    if (plane < 0 || plane >= PILE_PLANES) { slx_set_error("%s: plane %d is not one of the %d", who, plane, PILE_PLANES); return SLX_EINVAL; }
    return SLX_OK;
}

extern "C" int slx_pile_counts(slx_pile *p, int plane, int64_t beg, int64_t end, int32_t *out)
{
    SLX_CHK(slx_need(p, "slx_pile_counts"));
    SLX_CHK(pile_plane("slx_pile_counts", plane));
    if (beg > end || (beg < end && !out)) { slx_set_error("slx_pile_counts: null output or an interval that ends before it begins"); return SLX_EINVAL; }
    if (beg == end) return SLX_OK;
    memset(out, 0, 4 * (size_t)(end - beg));
    const int64_t lo = std::max(beg, p->par.beg), hi = std::min(end, p->par.end);
    if (lo < hi) SLX_HIPCHK(hipMemcpy(out + (lo - beg), p->arr() + (uint64_t)plane * p->stride + (uint64_t)(lo - p->par.beg), 4 * (size_t)(hi - lo), hipMemcpyDeviceToHost));
    return SLX_OK;
}

extern "C" int slx_pile_counts_device(slx_pile *p, int plane, const void **d_counts, int64_t *n)
{
    SLX_CHK(slx_need(p, "slx_pile_counts_device"));
    SLX_CHK(pile_plane("slx_pile_counts_device", plane));
    if (!d_counts || !n) { slx_set_error("slx_pile_counts_device: null argument"); return SLX_EINVAL; }
    *d_counts = p->arr() + (uint64_t)plane * p->stride; *n = p->L;
    return SLX_OK;
}

extern "C" int slx_pile_at(slx_pile *p, int64_t pos, int32_t out[SLX_PILE_PLANES])
{
    SLX_CHK(slx_need(p, "slx_pile_at"));
    if (!out) { slx_set_error("slx_pile_at: null output"); return SLX_EINVAL; }
    memset(out, 0, 4 * PILE_PLANES);
    if (pos < p->par.beg || pos >= p->par.end) return SLX_OK;
    SLX_HIPCHK(hipMemcpy2D(out, 4, p->arr() + (uint64_t)(pos - p->par.beg), 4 * (size_t)p->stride, 4, PILE_PLANES, hipMemcpyDeviceToHost));
    return SLX_OK;
}

extern "C" int slx_pile_sites(slx_pile *p, slx_ref *ref, int64_t ref_tid, int32_t min_depth, int32_t min_alt, int32_t frac_num, int32_t frac_den, int64_t *n_sites)
{
    SLX_CHK(slx_need(p, "slx_pile_sites"));
    if (!ref || !n_sites) { slx_set_error("slx_pile_sites: null argument"); return SLX_EINVAL; }
    if (min_depth < 1 || min_alt < 1 || frac_den < 1 || frac_num < 0 || frac_num > frac_den) {
        slx_set_error("slx_pile_sites: min_depth %d, min_alt %d, fraction %d / %d: the first two are at least 1, the fraction lies in [0, 1] with a denominator of at least 1", min_depth, min_alt, frac_num, frac_den);
        return SLX_EINVAL;
    }
    const int64_t have = slx_ref_len(ref, ref_tid), want = p->len[(size_t)p->par.tid];
    if (have != want) { slx_set_error("slx_pile_sites: contig %lld of the reference has %lld bases, the window's contig %lld", (long long)ref_tid, (long long)have, (long long)want); return SLX_EINVAL; }
    slx_ref_dev rd;
    SLX_CHK(slx_ref_device(ref, &rd));
    p->n_sites = -1; *n_sites = 0;
    const uint64_t nq = p->stride / 4;
    const pile_site_par Q = {min_depth, min_alt, frac_num, frac_den};
    uint64_t total = 0;
    SLX_HIPCHK(hipEventRecord(p->ev[0], p->st));
    if (nq) {
        SLX_CHK(p->d_n4.ensure(4 * (nq + 1))); SLX_CHK(p->d_at.ensure(4 * (nq + 1)));
        const unsigned blocks = (unsigned)((nq + 1 + 255) / 256);
        k_pile_site_flag<<<blocks, 256, 0, p->st>>>(p->arr(), p->stride, nq, p->L, p->par.beg, (const uint8_t *)rd.d_bases, (const ull *)rd.d_contig_off, ref_tid, Q, p->d_n4.as<uint32_t>());
        SLX_HIPCHK(hipGetLastError());
        SLX_CHK(slx_exclusive_sum(p->d_tmp, p->d_n4.as<uint32_t>(), p->d_at.as<uint32_t>(), (size_t)nq + 1, p->st));
        uint32_t *h = p->h_cnt.as<uint32_t>();
        SLX_HIPCHK(hipMemcpyAsync(h, p->d_at.as<uint32_t>() + nq, 4, hipMemcpyDeviceToHost, p->st));
        SLX_HIPCHK(slx_wait_stream(p->st));
        total = h[0];
        if (total) {
            SLX_CHK(p->d_sites.ensure(sizeof(slx_pile_site) * total));
            k_pile_site_fill<<<blocks, 256, 0, p->st>>>(p->arr(), p->stride, nq, p->L, p->par.beg, (const uint8_t *)rd.d_bases, (const ull *)rd.d_contig_off, ref_tid, Q, p->d_at.as<uint32_t>(),
                                                        p->d_sites.as<slx_pile_site>());
            SLX_HIPCHK(hipGetLastError());
        }
    }
    SLX_HIPCHK(hipEventRecord(p->ev[1], p->st));
    SLX_HIPCHK(slx_wait_stream(p->st));
    p->us_sites += slx_ev_us(p->ev[0], p->ev[1]);
    p->n_sites = (int64_t)total; *n_sites = (int64_t)total;
    return SLX_OK;
}

static int pile_have_sites(const char *who, const slx_pile *p)
{
    if (p->n_sites < 0) { slx_set_error("%s: no result of slx_pile_sites to read", who); return SLX_EINVAL; }
    return SLX_OK;
}

extern "C" int slx_pile_sites_to_host(slx_pile *p, slx_pile_site *out)
{
    SLX_CHK(slx_need(p, "slx_pile_sites_to_host"));
    SLX_CHK(pile_have_sites("slx_pile_sites_to_host", p));
    if (p->n_sites && !out) { slx_set_error("slx_pile_sites_to_host: null output"); return SLX_EINVAL; }
    if (p->n_sites) SLX_HIPCHK(hipMemcpy(out, p->d_sites.p, sizeof(slx_pile_site) * (size_t)p->n_sites, hipMemcpyDeviceToHost));
    return SLX_OK;
}

extern "C" int slx_pile_sites_tsv(slx_pile *p, const char *path)
{
    SLX_CHK(slx_need(p, "slx_pile_sites_tsv"));
    if (!path) { slx_set_error("slx_pile_sites_tsv: null path"); return SLX_EINVAL; }
    SLX_CHK(pile_have_sites("slx_pile_sites_tsv", p));
    std::vector<slx_pile_site> v((size_t)p->n_sites);
    SLX_CHK(slx_pile_sites_to_host(p, v.data()));
    std::string text;
    const std::string &name = p->names[(size_t)p->par.tid];
    char buf[64];
    for (const slx_pile_site &s : v) {
        text += name;
        snprintf(buf, sizeof buf, "\t%lld\t%c\t%d", (long long)s.pos + 1, (char)s.ref, s.depth);
        text += buf;
        for (int k = 0; k < PILE_REV; ++k) { snprintf(buf, sizeof buf, "\t%d,%d", s.plane[k], s.plane[PILE_REV + k]); text += buf; }
        snprintf(buf, sizeof buf, "\t%d\n", s.plane[PILE_LOWQ]);
        text += buf;
    }
    const bool is_stdout = !strcmp(path, "-");
    FILE *f = is_stdout ? stdout : fopen(path, "wb");
    if (!f) { slx_set_error("pileup: cannot create '%s': %s", path, strerror(errno)); return SLX_EIO; }
    const bool wrote = fwrite(text.data(), 1, text.size(), f) == text.size();
    const bool closed = is_stdout ? fflush(f) == 0 : fclose(f) == 0;
    if (!wrote || !closed) { slx_set_error("pileup: cannot write to '%s': %s", path, strerror(errno)); return SLX_EIO; }
    return SLX_OK;
}

extern "C" int slx_pile_clear(slx_pile *p)
{
    SLX_CHK(slx_need(p, "slx_pile_clear"));
    SLX_HIPCHK(hipMemsetAsync(p->d_arr.p, 0, p->arr_bytes(), p->st));
    SLX_HIPCHK(slx_wait_stream(p->st));
    return SLX_OK;
}

extern "C" int64_t slx_pile_counter(const slx_pile *p, const char *name)
{
    if (!p || !name) return -1;
    if (!strcmp(name, "records_seen")) return p->c_seen;
    if (!strcmp(name, "records_counted")) return p->c_counted;
    if (!strcmp(name, "long_records")) return p->c_long;
    if (!strcmp(name, "events_lds")) return p->c_lds;
    if (!strcmp(name, "events_global")) return p->c_global;
    if (!strcmp(name, "sites")) return p->n_sites < 0 ? 0 : p->n_sites;
    if (!strcmp(name, "us_add")) return (int64_t)p->us_add;
    if (!strcmp(name, "us_sites")) return (int64_t)p->us_sites;
    return -1;
}
