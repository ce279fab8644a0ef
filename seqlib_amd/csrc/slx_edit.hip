// slx_edit.hip -- BAM records edited in HBM (include/seqlib_amd_edit.h): a device-resident batch in, a device-resident batch out.  DESIGN.md section 9.13.
//   k_edit_size        a lane per record: its span, its fixed fields, the aux walk of dev_edit.h ed_size_record -> new length and descriptor; a record whose aux
//                      area reaches long_aux bytes is listed instead
//   k_edit_size_long   a wave per listed record: the same walk, the NUL of a Z / H value found 64 bytes per ballot
//   slx_exclusive_sum  the new lengths -> the new offsets and n_bytes
//   k_edit_gather      one wave per ED_TILE bytes of the OUTPUT, pieces brought together in LDS, stored 16 bytes per lane              dev_edit.h ed_gather_tile
// Records map to lanes and tiles to waves statically: no work queue.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "slx_internal.h"
#include "slx_hip.h"
#include "seqlib_amd_edit.h"
#include "dev_lanes.h"
#include "dev_wave.h"
#include "dev_edit.h"
#include "edit_host.h"

typedef unsigned long long ull;
typedef SlxDevBuf<SlxMargin<8, 256>> EDBuf;
typedef SlxPinBuf<SlxExact> EHBuf;

static const char EDIT_NO_DEVICE[] = "no HIP device: batches of records are edited on MI355X only (no CPU fallback)";

// bad, col, big: the first record refused as broken, for a broken column, for its new size (atomicMin); n_long: records left to k_edit_size_long
struct ed_state { ull bad, col, big; uint32_t n_long, pad; };
struct ed_args { const uint8_t *s; uint64_t n_bytes; const uint64_t *off; uint64_t n; uint32_t long_aux, pad; };

// ------------------------------------------------------------------ kernels
__device__ __forceinline__ void ed_report(uint32_t rc, uint64_t i, ed_state *st)
{
    wave_report_min(&st->bad, rc == ED_E_RECORD, i);
    wave_report_min(&st->col, rc == ED_E_COLUMN, i);
    wave_report_min(&st->big, rc == ED_E_SIZE, i);
}

__global__ __launch_bounds__(256) void k_edit_size(ed_plan P, ed_args A, ull *sz, ed_desc *desc, uint32_t *longlist, ed_state *st)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t rc = ED_OK;
    if (i == A.n) sz[i] = 0;
    if (i < A.n) {
        uint32_t span = 0, seq_at = 0, aux_at = 0;
        bool own = false;
        uint64_t len = 0;
        if (!ed_span(A.s, A.n_bytes, A.off, i, A.n, &span, &own)) rc = ED_E_RECORD;
        else if (own) {          // (when not, record i + 1 is the one named, by its own lane)
            const uint8_t *rec = A.s + (A.off[i] - A.off[0]);
            if (!ed_fixed(rec, span, &seq_at, &aux_at)) rc = ED_E_RECORD;
            else if (span - aux_at >= A.long_aux) longlist[wave_fetch_inc(&st->n_long)] = (uint32_t)i;
            else rc = ed_size_record<false>(P, rec, span, seq_at, aux_at, i, desc + i, &len, 0, 1);
        }
        sz[i] = rc == ED_OK ? len : 0;
    }
    ed_report(rc, i, st);
}

// (only records whose span and fixed fields k_edit_size has accepted are listed)
__global__ __launch_bounds__(256) void k_edit_size_long(ed_plan P, ed_args A, const uint32_t *longlist, uint32_t n_long, ull *sz, ed_desc *desc, ed_state *st)
{
    const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= n_long) return;          // (a whole wave)
    const uint64_t i = longlist[w];
    const uint8_t *rec = A.s + (A.off[i] - A.off[0]);
    const uint32_t span = (uint32_t)(A.off[i + 1] - A.off[i]);
    uint32_t seq_at = 0, aux_at = 0;
    uint64_t len = 0;
    uint32_t rc = ED_E_RECORD;
    if (ed_fixed(rec, span, &seq_at, &aux_at)) rc = ed_size_record<true>(P, rec, span, seq_at, aux_at, i, desc + i, &len, (int)lane, 64);
    if (lane == 0) sz[i] = rc == ED_OK ? len : 0;
    ed_report(lane == 0 ? rc : (uint32_t)ED_OK, i, st);
}

__global__ __launch_bounds__(256) void k_edit_gather(ed_plan P, ed_args A, const ull *new_off, const ed_desc *desc, uint64_t n_bytes, uint64_t n_tiles, uint8_t *out)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[4][ED_TILE];
    __shared__ ed_tile T[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t t = (uint64_t)blockIdx.x * 4 + wave;
    if (t >= n_tiles) return;          // (a whole wave: the ballots and shuffles of ed_gather_tile see all 64 lanes)
    ed_gather_tile(P, A.s, A.off, new_off, desc, (int64_t)A.n, n_bytes, t, (ED_LDS uint8_t *)tile[wave], (ED_LDS ed_tile *)&T[wave], out, (int)lane, 64);
}

// ------------------------------------------------------------------ host
struct slx_edit : SlxGpu<8> {
    slx_edit() : SlxGpu(EDIT_NO_DEVICE) {}
    ed_host_plan H;
    bool consts_stale = true;
    uint32_t long_aux = ED_LONG_AUX;
    EDBuf d_in{*this}, d_off{*this}, d_const{*this}, d_sz{*this}, d_noff{*this}, d_desc{*this}, d_long{*this}, d_state{*this}, d_tmp{*this}, d_out{*this};
    EHBuf h_small{*this};
    slx_edit_batch last = {};
    int64_t c_records = 0, c_long = 0, c_in = 0, c_out = 0;
    double us_size = 0, us_scan = 0, us_gather = 0;
};

extern "C" void slx_edit_free(slx_edit *e)
{
    if (!e) return;
    e->close();
    delete e;
}

extern "C" int slx_edit_create(int device, slx_edit **out)
{
    if (!out) { slx_set_error("slx_edit_create: null argument"); return SLX_EINVAL; }
    *out = nullptr;
    if (device < SLX_EDIT_AUTO) { slx_set_error("slx_edit_create: device %d", device); return SLX_EINVAL; }
    return slx_create(out, slx_edit_free, [&](slx_edit *e) {
        // SLX_EDIT_HOST never asks the runtime; SLX_EDIT_AUTO is the current device, or host only without one
        if (device != SLX_EDIT_HOST) SLX_CHK(e->open(device == SLX_EDIT_AUTO ? -1 : device, "slx_edit_create", EDIT_NO_DEVICE, device == SLX_EDIT_AUTO));
        return (int)SLX_OK;
    });
}

static int edit_plan_done(slx_edit *e, const char *who, const std::string &err)
{
    if (!err.empty()) { slx_set_error("%s: %s", who, err.c_str()); return SLX_EINVAL; }
    e->consts_stale = true;
    return SLX_OK;
}
#define EDIT_HANDLE(who) do { if (!e) { slx_set_error(who ": null object"); return SLX_EINVAL; } } while (0)

extern "C" int slx_edit_plan_clear(slx_edit *e)
{
    EDIT_HANDLE("slx_edit_plan_clear");
    e->H = ed_host_plan();
    return edit_plan_done(e, "slx_edit_plan_clear", "");
}
extern "C" int slx_edit_drop_tag(slx_edit *e, const char *tag)
{
    EDIT_HANDLE("slx_edit_drop_tag");
    return edit_plan_done(e, "slx_edit_drop_tag", ed_plan_drop(e->H, tag));
}
extern "C" int slx_edit_drop_all_tags(slx_edit *e)
{
    EDIT_HANDLE("slx_edit_drop_all_tags");
    e->H.P.drop_all = 1;
    return SLX_OK;
}
extern "C" int slx_edit_clear_seq_qual(slx_edit *e)
{
    EDIT_HANDLE("slx_edit_clear_seq_qual");
    e->H.P.clear = 1;
    return SLX_OK;
}
extern "C" int slx_edit_add_int(slx_edit *e, const char *tag, int32_t value, int replace)
{
    EDIT_HANDLE("slx_edit_add_int");
    return edit_plan_done(e, "slx_edit_add_int", ed_plan_add(e->H, tag, ED_INT, value, replace != 0, nullptr, 0, nullptr, nullptr, nullptr, 0));
}
extern "C" int slx_edit_add_z(slx_edit *e, const char *tag, const void *value, int64_t n)
{
    EDIT_HANDLE("slx_edit_add_z");
    return edit_plan_done(e, "slx_edit_add_z", ed_plan_add(e->H, tag, ED_Z, 0, true, value, n, nullptr, nullptr, nullptr, 0));
}
extern "C" int slx_edit_add_int_column(slx_edit *e, const char *tag, const void *d_vals, int32_t absent, int replace)
{
    EDIT_HANDLE("slx_edit_add_int_column");
    return edit_plan_done(e, "slx_edit_add_int_column", ed_plan_add(e->H, tag, ED_INT_COL, absent, replace != 0, nullptr, 0, d_vals, nullptr, nullptr, 0));
}
extern "C" int slx_edit_add_z_column(slx_edit *e, const char *tag, const void *d_text, int64_t n_text, const void *d_off)
{
    EDIT_HANDLE("slx_edit_add_z_column");
    return edit_plan_done(e, "slx_edit_add_z_column", ed_plan_add(e->H, tag, ED_Z_COL, 0, true, nullptr, 0, nullptr, d_text, d_off, n_text));
}

extern "C" int slx_edit_drop_column(slx_edit *e, const char *tag)
{
    EDIT_HANDLE("slx_edit_drop_column");
    ed_plan &P = e->H.P;
    const int at = ed_tag_ok(tag) ? ed_find_add(P, tag) : -1;
    if (at < 0 || (P.add[at].kind != ED_INT_COL && P.add[at].kind != ED_Z_COL)) { slx_set_error("slx_edit_drop_column: the plan has no column add of that tag"); return SLX_EINVAL; }
    for (uint32_t a = (uint32_t)at; a + 1 < P.n_add; ++a) P.add[a] = P.add[a + 1];
    memset(&P.add[--P.n_add], 0, sizeof(ed_add));
    return SLX_OK;
}

extern "C" int slx_edit_set(slx_edit *e, const char *key, int64_t v)
{
    if (!e || !key) { slx_set_error("slx_edit_set: null argument"); return SLX_EINVAL; }
    if (!strcmp(key, "long_aux") && v >= 1 && v <= 0x7fffffffll) { e->long_aux = (uint32_t)v; return SLX_OK; }
    slx_set_error("slx_edit_set: unknown key '%s' or value %lld out of range", key, (long long)v);
    return SLX_EINVAL;
}

extern "C" int64_t slx_edit_counter(const slx_edit *e, const char *name)
{
    if (!e || !name) return -1;
    const std::string k = name;
    if (k == "device") return e->device;
    if (k == "long_aux") return e->long_aux;
    if (k == "records") return e->c_records;
    if (k == "long_records") return e->c_long;
    if (k == "bytes_in") return e->c_in;
    if (k == "bytes_out") return e->c_out;
    if (k == "us_size") return (int64_t)e->us_size;
    if (k == "us_scan") return (int64_t)e->us_scan;
    if (k == "us_gather") return (int64_t)e->us_gather;
    return -1;
}

static int edit_refusal(const char *who, const ull *hs)
{
    // hs: bad, col, big as ed_state
    if (hs[0] != ED_NONE) {
        slx_set_error("record editor: record %llu of the batch: its fields pass its block_size, its extent is not block_size + 4 inside the stream, or its aux area does not parse to its end", hs[0]);
        return SLX_EIO;
    }
    if (hs[1] != ED_NONE) { slx_set_error("%s: a Z column's offsets fall or pass n_text at record %llu", who, hs[1]); return SLX_EINVAL; }
    if (hs[2] != ED_NONE) { slx_set_error("%s: record %llu of the batch no longer fits block_size", who, hs[2]); return SLX_EUNSUPPORTED; }
    return SLX_OK;
}

static int edit_apply_impl(slx_edit *e, const char *who, const uint8_t *d_s, uint64_t n_bytes, const uint64_t *d_off, uint64_t n, slx_edit_batch *out)
{
    hipStream_t st = e->st;
    ed_plan P = e->H.P;
    for (uint32_t a = 0; a < P.n_add; ++a) {
        const ed_add &A = P.add[a];
        if (n && ((A.kind == ED_INT_COL && !A.vals) || (A.kind == ED_Z_COL && (!A.toff || (A.n_text && !A.text))))) {
            slx_set_error("%s: the column of tag %c%c is not bound: columns are bound for one apply", who, (char)A.tag, (char)(A.tag >> 8));
            return SLX_EINVAL;
        }
    }
    if (n >= 0xffffffffull) { slx_set_error("%s: 2^32 - 1 records or more in one batch", who); return SLX_EUNSUPPORTED; }
    if (e->d_out.p && d_s >= e->d_out.as<uint8_t>() && d_s < e->d_out.as<uint8_t>() + e->d_out.cap) {
        slx_set_error("%s: the batch is the handle's own last result, which this apply would overwrite", who);
        return SLX_EINVAL;
    }
    if (e->consts_stale) {
        SLX_CHK(e->d_const.ensure(ED_MAX_CONST));
        if (!e->H.consts.empty()) SLX_HIPCHK(hipMemcpyAsync(e->d_const.p, e->H.consts.data(), e->H.consts.size(), hipMemcpyHostToDevice, st));
        SLX_HIPCHK(slx_wait_stream(st));
        e->consts_stale = false;
    }
    P.consts = e->d_const.as<uint8_t>();
    SLX_CHK(e->d_sz.ensure(8 * (n + 2))); SLX_CHK(e->d_noff.ensure(8 * (n + 2))); SLX_CHK(e->d_desc.ensure(sizeof(ed_desc) * (n + 1))); SLX_CHK(e->d_long.ensure(4 * (n + 1)));
    SLX_CHK(e->d_state.ensure(sizeof(ed_state))); SLX_CHK(e->h_small.ensure(256));
    e->c_records = (int64_t)n; e->c_in = (int64_t)n_bytes; e->c_long = 0; e->c_out = 0;
    e->us_size = e->us_scan = e->us_gather = 0;
    if (n == 0) {
        if (n_bytes) { slx_set_error("record editor: %llu bytes and no record", (ull)n_bytes); return SLX_EIO; }
        SLX_HIPCHK(hipMemsetAsync(e->d_noff.p, 0, 16, st));
        SLX_CHK(e->d_out.ensure(64));
        SLX_HIPCHK(slx_wait_stream(st));
        *out = slx_edit_batch{0, 0, e->d_out.p, e->d_noff.p};
        e->last = *out;
        return SLX_OK;
    }
    ed_state *hs = e->h_small.as<ed_state>();
    hs[0] = ed_state{ED_NONE, ED_NONE, ED_NONE, 0u, 0u};
    const ed_args A = {d_s, n_bytes, d_off, n, e->long_aux, 0u};
    SLX_HIPCHK(hipMemcpyAsync(e->d_state.p, hs, sizeof(ed_state), hipMemcpyHostToDevice, st));
    SLX_HIPCHK(hipEventRecord(e->ev[0], st));
    k_edit_size<<<(unsigned)((n + 256) / 256), 256, 0, st>>>(P, A, e->d_sz.as<ull>(), e->d_desc.as<ed_desc>(), e->d_long.as<uint32_t>(), e->d_state.as<ed_state>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(e->ev[1], st));
    SLX_HIPCHK(hipMemcpyAsync(hs + 1, e->d_state.p, sizeof(ed_state), hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    e->us_size = slx_ev_us(e->ev[0], e->ev[1]);
    // (no refusal yet: a listed record may be broken too, and earlier than the first the lanes found; only records whose span and fixed fields hold are listed, so
    // the wave walk reads inside validated spans whatever the lanes refused)
    const uint32_t n_long = hs[1].n_long;
    e->c_long = n_long;
    if (n_long) {
        SLX_HIPCHK(hipEventRecord(e->ev[2], st));
        k_edit_size_long<<<(n_long + 3) / 4, 256, 0, st>>>(P, A, e->d_long.as<uint32_t>(), n_long, e->d_sz.as<ull>(), e->d_desc.as<ed_desc>(), e->d_state.as<ed_state>());
        SLX_HIPCHK(hipGetLastError());
        SLX_HIPCHK(hipEventRecord(e->ev[3], st));
        SLX_HIPCHK(hipMemcpyAsync(hs + 1, e->d_state.p, sizeof(ed_state), hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(slx_wait_stream(st));
        e->us_size += slx_ev_us(e->ev[2], e->ev[3]);
    }
    SLX_CHK(edit_refusal(who, &hs[1].bad));
    SLX_HIPCHK(hipEventRecord(e->ev[4], st));
    SLX_CHK(slx_exclusive_sum(e->d_tmp, e->d_sz.as<ull>(), e->d_noff.as<ull>(), n + 1, st, 16));
    SLX_HIPCHK(hipEventRecord(e->ev[5], st));
    ull *total_p = (ull *)(hs + 2);
    SLX_HIPCHK(hipMemcpyAsync(total_p, e->d_noff.as<ull>() + n, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    e->us_scan = slx_ev_us(e->ev[4], e->ev[5]);
    const uint64_t total = *total_p, n_tiles = (total + ED_TILE - 1) / ED_TILE;
    if (n_tiles >= 0x1fffffffull) { slx_set_error("%s: %llu bytes in one batch", who, (ull)total); return SLX_EUNSUPPORTED; }
    SLX_CHK(e->d_out.ensure(total + 64));
    SLX_HIPCHK(hipEventRecord(e->ev[6], st));
    k_edit_gather<<<(unsigned)((n_tiles + 3) / 4), 256, 0, st>>>(P, A, e->d_noff.as<ull>(), e->d_desc.as<ed_desc>(), total, n_tiles, e->d_out.as<uint8_t>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(e->ev[7], st));
    SLX_HIPCHK(slx_wait_stream(st));
    e->us_gather = slx_ev_us(e->ev[6], e->ev[7]);
    e->c_out = (int64_t)total;
    *out = slx_edit_batch{(int64_t)n, (int64_t)total, e->d_out.p, e->d_noff.p};
    e->last = *out;
    return SLX_OK;
}

// the columns are bound for one apply, whatever becomes of it
static int edit_apply(slx_edit *e, const char *who, const uint8_t *d_s, uint64_t n_bytes, const uint64_t *d_off, uint64_t n, slx_edit_batch *out)
{
    *out = slx_edit_batch{};
    e->last = *out;
    const int rc = edit_apply_impl(e, who, d_s, n_bytes, d_off, n, out);
    for (uint32_t a = 0; a < e->H.P.n_add; ++a) { ed_add &A = e->H.P.add[a]; A.vals = nullptr; A.text = nullptr; A.toff = nullptr; A.n_text = 0; }
    return rc;
}

extern "C" int slx_edit_apply_device(slx_edit *e, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records, slx_edit_batch *out)
{
    SLX_CHK(slx_need(e, "slx_edit_apply_device"));
    SLX_CHK(slx_batch_args("slx_edit_apply_device", d_stream, n_bytes, d_rec_off, n_records));
    if (!out) { slx_set_error("slx_edit_apply_device: null result"); return SLX_EINVAL; }
    return edit_apply(e, "slx_edit_apply_device", (const uint8_t *)d_stream, (uint64_t)n_bytes, (const uint64_t *)d_rec_off, (uint64_t)n_records, out);
}

extern "C" int slx_edit_apply_host(slx_edit *e, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records, slx_edit_batch *out)
{
    SLX_CHK(slx_need(e, "slx_edit_apply_host"));
    SLX_CHK(slx_batch_args("slx_edit_apply_host", stream, n_bytes, rec_off, n_records));
    if (!out) { slx_set_error("slx_edit_apply_host: null result"); return SLX_EINVAL; }
    if (n_records) {
        SLX_CHK(slx_batch_stage(e->d_in, e->d_off, 16, stream, n_bytes, rec_off, n_records, e->st));
        SLX_HIPCHK(slx_wait_stream(e->st));
    }
    return edit_apply(e, "slx_edit_apply_host", e->d_in.as<uint8_t>(), (uint64_t)n_bytes, e->d_off.as<uint64_t>(), (uint64_t)n_records, out);
}

extern "C" int slx_edit_to_host(slx_edit *e, const slx_edit_batch *b, void *stream, uint64_t *rec_off)
{
    SLX_CHK(slx_need(e, "slx_edit_to_host"));
    if (!b) { slx_set_error("slx_edit_to_host: null argument"); return SLX_EINVAL; }
    if (!b->d_rec_off || b->d_stream != e->last.d_stream || b->d_rec_off != e->last.d_rec_off || b->n_records != e->last.n_records || b->n_bytes != e->last.n_bytes) {
        slx_set_error("slx_edit_to_host: not the handle's last result");
        return SLX_EINVAL;
    }
    if (stream && b->n_bytes) SLX_HIPCHK(hipMemcpyAsync(stream, b->d_stream, (size_t)b->n_bytes, hipMemcpyDeviceToHost, e->st));
    if (rec_off) SLX_HIPCHK(hipMemcpyAsync(rec_off, b->d_rec_off, 8 * ((size_t)b->n_records + 1), hipMemcpyDeviceToHost, e->st));
    SLX_HIPCHK(slx_wait_stream(e->st));
    return SLX_OK;
}

// ------------------------------------------------------------------ host only
extern "C" int slx_edit_record(const slx_edit *e, const uint8_t *rec, int64_t n, const int32_t *col_int, const void *const *col_z, const int64_t *col_z_len, uint8_t *out, int64_t cap,
                               int64_t *out_len)
{
    if (!e || !rec || n < 0 || !out_len || cap < 0 || (cap && !out)) { slx_set_error("slx_edit_record: null or negative argument"); return SLX_EINVAL; }
    *out_len = 0;
    ed_plan P = e->H.P;
    P.consts = e->H.consts.data();
    uint64_t zoff[ED_MAX_ADD][2];
    for (uint32_t a = 0; a < P.n_add; ++a) {
        ed_add &A = P.add[a];
        if (A.kind == ED_INT_COL) {
            if (!col_int) { slx_set_error("slx_edit_record: the plan has an int column and col_int is null"); return SLX_EINVAL; }
            A.vals = col_int + a;
        } else if (A.kind == ED_Z_COL) {
            if (!col_z || !col_z_len || col_z_len[a] < 0 || (col_z_len[a] && !col_z[a])) { slx_set_error("slx_edit_record: the plan has a Z column and its value is null or negative"); return SLX_EINVAL; }
            zoff[a][0] = 0; zoff[a][1] = (uint64_t)col_z_len[a];
            A.text = (const uint8_t *)col_z[a]; A.toff = zoff[a]; A.n_text = (uint64_t)col_z_len[a];
        }
    }
    // one record is a batch of one: record 0, whose column values lie at index 0
    const uint64_t off[2] = {0, (uint64_t)n};
    std::vector<uint8_t> res;
    std::vector<ull> noff;
    uint64_t bad = ED_NONE;
    const uint32_t rc = ed_apply_on_host(P, rec, (uint64_t)n, off, 1, &res, &noff, &bad);
    if (rc != ED_OK) {
        const ull hs[3] = {rc == ED_E_RECORD ? 0ull : ED_NONE, rc == ED_E_COLUMN ? 0ull : ED_NONE, rc == ED_E_SIZE ? 0ull : ED_NONE};
        return edit_refusal("slx_edit_record", hs);
    }
    *out_len = (int64_t)res.size();
    if ((int64_t)res.size() <= cap && !res.empty()) memcpy(out, res.data(), res.size());
    return SLX_OK;
}
