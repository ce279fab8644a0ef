// slx_stats.hip -- per-read-group statistics on the GPU (include/seqlib_amd_stats.h): block_size-prefixed BAM records in HBM -> one uint64 row of counters and
// histogram bins per read group, read back as numbers or as the reference's text.  DESIGN.md section 9.10 has the argument.
//   k_st_windows   a lane per record: the first and the last record that start in each window of the stream
//   k_st_add       the stream cut into windows, a block per window staged in LDS; a lane per record: fixed fields, CIGAR clips, the aux walk, the QUAL sum, the
//                  group by a probe of the table in HBM; adds into uint32 rows in LDS for the first lds_groups groups (one add per wave where the wave agrees),
//                  flushed with 64-bit adds at the block's end                                                                         dev_stats.h st_record
//   k_st_add_long  a wave per record that does not fit the stage or is larger than long_record                                       dev_stats.h st_part_of
//   k_st_keys      the keys of records whose group the table did not have, for the host
// A record with an unknown key is not counted by the launch that meets it: it is marked.  The host takes the (at most ST_PICK) lowest marked records, fetches
// their keys, registers the new groups in record order -- every group still unknown first appears behind them -- and launches again over the marked records
// only.  In steady state there is one launch per batch.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "slx_internal.h"
#include "slx_hip.h"
#include "seqlib_amd_stats.h"
#include "stats_host.h"

typedef unsigned long long ull;
#define ST_PICK 4096u               // marked records whose keys one round fetches
#define ST_LDS_MAX 65536u           // dynamic LDS of one block

typedef SlxDevBuf<SlxMargin<4, 256>> TDBuf;
typedef SlxPinBuf<SlxMargin<4, 256>> THBuf;

static const char ST_NO_DEVICE[] = "no HIP device: batches are counted on MI355X only (no CPU fallback)";

struct slx_stats : SlxGpu<> {
    st_lay L;
    st_par P = {0u, 0, 4096u, 0u};
    int32_t len_max = 250, isize_max = 2000;
    uint32_t lds_groups = 1, window = 16384, group_slots = 64, max_groups = 65536;
    bool started = false;          // something was added: the layout stands
    st_groups G;
    std::vector<uint64_t> h_counts;          // G.size() rows when synced
    bool synced = true;
    std::vector<std::string> names;          // what slx_stats_group_name hands out
    SlxDevBuf<SlxExact> d_counts{*this};
    size_t rows_cap = 0;
    TDBuf d_slots{*this}, d_koff{*this}, d_pool{*this}, d_in{*this}, d_off{*this}, d_long{*this}, d_misslist{*this}, d_miss[2] = {*this, *this}, d_cnt{*this}, d_pick{*this}, d_keys{*this},
          d_win{*this};
    THBuf h_cnt{*this}, h_list{*this}, h_keys{*this};
    int64_t c_seen = 0, c_counted = 0, c_long = 0, c_lds = 0, c_global = 0, c_miss = 0;
    double us_add = 0;
    slx_stats() : SlxGpu(ST_NO_DEVICE) { st_layout_default(&L, len_max, isize_max); G.reset(group_slots); }
    st_tab tab() const { return st_tab{d_slots.as<uint32_t>(), d_koff.as<uint32_t>(), d_pool.as<uint8_t>(), (uint32_t)G.slots.size() - 1, 0u}; }
};

extern "C" void slx_stats_free(slx_stats *c)
{
    if (!c) return;
    c->close();
    delete c;
}

extern "C" int slx_stats_create(int device, slx_stats **out)
{
    if (!out) { slx_set_error("slx_stats_create: null argument"); return SLX_EINVAL; }
    return slx_create(out, slx_stats_free, [&](slx_stats *c) {
        SLX_CHK(c->open(device, "slx_stats_create", ST_NO_DEVICE, true));
        if (c->device < 0) return (int)SLX_OK;          // host only
        SLX_CHK(c->d_cnt.ensure(8 * ST_K_N)); SLX_CHK(c->h_cnt.ensure(8 * ST_K_N));
        return (int)SLX_OK;
    });
}

extern "C" int slx_stats_set(slx_stats *c, const char *key, int64_t v)
{
    if (!c || !key) { slx_set_error("slx_stats_set: null argument"); return SLX_EINVAL; }
    auto in = [&](int64_t lo, int64_t hi) { if (v >= lo && v <= hi) return true; slx_set_error("slx_stats_set: %s %lld outside [%lld, %lld]", key, (long long)v, (long long)lo, (long long)hi); return false; };
    const bool is_len = !strcmp(key, "len_max");
    if (is_len || !strcmp(key, "isize_max")) {
        if (!in(1, 1 << 20)) return SLX_EINVAL;
        if (c->started) { slx_set_error("slx_stats_set: %s after the first add", key); return SLX_EINVAL; }
        (is_len ? c->len_max : c->isize_max) = (int32_t)v;
        st_layout_default(&c->L, c->len_max, c->isize_max);
        c->rows_cap = 0;          // (rows of another size: all of them are zeroed again before the first add)
        return SLX_OK;
    }
    if (!strcmp(key, "exclude_flags")) { if (!in(0, 0xffff)) return SLX_EINVAL; c->P.exclude_flags = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "min_mapq")) { if (!in(0, 255)) return SLX_EINVAL; c->P.min_mapq = (int32_t)v; return SLX_OK; }
    if (!strcmp(key, "lds_groups")) { if (!in(0, 16)) return SLX_EINVAL; c->lds_groups = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "long_record")) { if (!in(1, 0x7fffffffll)) return SLX_EINVAL; c->P.long_record = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "window_bytes")) {
        if (!in(64, 32768)) return SLX_EINVAL;
        if (v & 15) { slx_set_error("slx_stats_set: window_bytes %lld is not a multiple of 16", (long long)v); return SLX_EINVAL; }
        c->window = (uint32_t)v;
        return SLX_OK;
    }
    if (!strcmp(key, "max_groups")) { if (!in(1, 1 << 20)) return SLX_EINVAL; c->max_groups = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "group_slots")) {
        if (!in(2, 1 << 24)) return SLX_EINVAL;
        c->group_slots = (uint32_t)v;
        if (c->G.size() == 0) c->G.reset(c->group_slots);
        return SLX_OK;
    }
    slx_set_error("slx_stats_set: unknown key '%s'", key);
    return SLX_EINVAL;
}

// rows for every group in HBM (the old ones kept, the new ones zero) and the table the kernels probe
static int st_upload_groups(slx_stats *c)
{
    const size_t need = std::max<size_t>(c->G.size(), 1), rb = 8 * (size_t)c->L.row * ST_REPLICAS;
    if (need > c->rows_cap) {
        const size_t cap = std::max(need, 2 * c->rows_cap);
        SLX_CHK(c->d_counts.ensure(cap * rb, c->st, c->rows_cap * rb));
        SLX_HIPCHK(hipMemsetAsync((uint8_t *)c->d_counts.p + c->rows_cap * rb, 0, (cap - c->rows_cap) * rb, c->st));
        c->rows_cap = cap;
    }
    SLX_CHK(c->d_slots.ensure(4 * c->G.slots.size())); SLX_CHK(c->d_koff.ensure(4 * c->G.koff.size())); SLX_CHK(c->d_pool.ensure(c->G.pool.size() + 1));
    SLX_HIPCHK(hipMemcpyAsync(c->d_slots.p, c->G.slots.data(), 4 * c->G.slots.size(), hipMemcpyHostToDevice, c->st));
    SLX_HIPCHK(hipMemcpyAsync(c->d_koff.p, c->G.koff.data(), 4 * c->G.koff.size(), hipMemcpyHostToDevice, c->st));
    if (!c->G.pool.empty()) SLX_HIPCHK(hipMemcpyAsync(c->d_pool.p, c->G.pool.data(), c->G.pool.size(), hipMemcpyHostToDevice, c->st));
    SLX_HIPCHK(slx_wait_stream(c->st));          // (the vectors may move before the next call)
    return SLX_OK;
}

static int st_errors(const ull *hc)
{
    if (hc[ST_K_ERR_IO] != ~0ull) {
        slx_set_error("read statistics: record %llu of the batch: its fields pass its block_size, its extent is not block_size + 4 inside the stream, or an aux field is of unknown type or passes the record's end", hc[ST_K_ERR_IO]);
        return SLX_EIO;
    }
    if (hc[ST_K_ERR_KEY] != ~0ull) { slx_set_error("read statistics: record %llu of the batch: its group key is longer than %u bytes", hc[ST_K_ERR_KEY], ST_MAX_KEY); return SLX_EUNSUPPORTED; }
    return SLX_OK;
}

// the records of d_s (n_bytes, offsets d_off) into the rows; the stream has drained on return
static int st_add(slx_stats *c, const uint8_t *d_s, uint64_t n_bytes, const ull *d_off, uint64_t n)
{
    if (n == 0) return SLX_OK;
    if (n >= 0xffffffffull) { slx_set_error("read statistics: 2^32 - 1 records or more in one batch"); return SLX_EUNSUPPORTED; }
    if (n_bytes < 36 * n) { slx_set_error("read statistics: %llu records in %llu bytes: record 0 of the batch cannot lie inside the stream", (ull)n, (ull)n_bytes); return SLX_EIO; }
    hipStream_t st = c->st;
    c->started = true; c->synced = false;
    SLX_CHK(c->d_long.ensure(4 * n)); SLX_CHK(c->d_misslist.ensure(4 * n)); SLX_CHK(c->d_miss[0].ensure(n)); SLX_CHK(c->d_miss[1].ensure(n));
    SLX_CHK(st_upload_groups(c));
    const uint32_t W = c->window, stage = W + ST_OVERHANG + 16u;
    const uint32_t lds_groups = std::min<uint32_t>(c->lds_groups, (ST_LDS_MAX - stage) / (4u * c->L.row));
    const uint64_t n_win = (n_bytes + W - 1) / W;
    if (n_win >= 0x7fffffffull) { slx_set_error("read statistics: %llu windows in one batch", (ull)n_win); return SLX_EUNSUPPORTED; }
    ull *hc = c->h_cnt.as<ull>(), *dc = c->d_cnt.as<ull>();
    const uint8_t *only = nullptr;
    int cur = 0;
    SLX_CHK(c->d_win.ensure(8 * n_win));
    uint32_t *wfirst = c->d_win.as<uint32_t>(), *wend = wfirst + n_win;
    SLX_HIPCHK(hipEventRecord(c->ev[0], st));
    SLX_HIPCHK(hipMemsetAsync(wfirst, 0xff, 8 * n_win, st));
    for (;;) {
        uint8_t *miss = c->d_miss[cur].as<uint8_t>();
        memset(hc, 0, 8 * ST_K_N);
        hc[ST_K_ERR_IO] = hc[ST_K_ERR_KEY] = ~0ull;
        SLX_HIPCHK(hipMemcpyAsync(dc, hc, 8 * ST_K_N, hipMemcpyHostToDevice, st));
        SLX_HIPCHK(hipMemsetAsync(miss, 0, n, st));
        if (!only) { k_st_windows<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(d_off, n, n_bytes, W, n_win, wfirst, wend, dc); SLX_HIPCHK(hipGetLastError()); }
        k_st_add<<<(unsigned)n_win, 256, stage + 4 * (size_t)lds_groups * c->L.row, st>>>(d_s, n_bytes, d_off, n, W, wfirst, wend, c->P, c->L, c->tab(), c->d_counts.as<ull>(), lds_groups, only, miss,
                                                                                       c->d_misslist.as<uint32_t>(), c->d_long.as<uint32_t>(), dc);
        SLX_HIPCHK(hipGetLastError());
        SLX_HIPCHK(hipMemcpyAsync(hc, dc, 8 * ST_K_N, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(slx_wait_stream(st));
        SLX_CHK(st_errors(hc));
        const uint64_t n_long = hc[ST_K_NLONG];
        if (n_long) {
            k_st_add_long<<<(unsigned)((n_long + 3) / 4), 256, 0, st>>>(d_s, d_off, c->d_long.as<uint32_t>(), n_long, c->P, c->L, c->tab(), c->d_counts.as<ull>(), miss,
                                                                     c->d_misslist.as<uint32_t>(), dc);
            SLX_HIPCHK(hipGetLastError());
            SLX_HIPCHK(hipMemcpyAsync(hc, dc, 8 * ST_K_N, hipMemcpyDeviceToHost, st));
            SLX_HIPCHK(slx_wait_stream(st));
            SLX_CHK(st_errors(hc));
        }
        c->c_counted += (int64_t)hc[ST_K_COUNTED]; c->c_lds += (int64_t)hc[ST_K_LDS]; c->c_global += (int64_t)hc[ST_K_GLOBAL];
        if (!only) c->c_long += (int64_t)n_long;
        const uint64_t n_miss = hc[ST_K_NMISS];
        if (!n_miss) break;
        if (!only) c->c_miss += (int64_t)n_miss;
        // the lowest marked records, their keys, the new groups in record order
        SLX_CHK(c->h_list.ensure(4 * n_miss));
        uint32_t *list = c->h_list.as<uint32_t>();
        SLX_HIPCHK(hipMemcpyAsync(list, c->d_misslist.p, 4 * n_miss, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(slx_wait_stream(st));
        const uint32_t k = (uint32_t)std::min<uint64_t>(n_miss, ST_PICK);
        std::partial_sort(list, list + k, list + n_miss);
        SLX_CHK(c->d_pick.ensure(4 * (size_t)k)); SLX_CHK(c->d_keys.ensure((size_t)k * ST_KEY_STRIDE)); SLX_CHK(c->h_keys.ensure((size_t)k * ST_KEY_STRIDE));
        SLX_HIPCHK(hipMemcpyAsync(c->d_pick.p, list, 4 * (size_t)k, hipMemcpyHostToDevice, st));
        k_st_keys<<<(k + 255) / 256, 256, 0, st>>>(d_s, d_off, c->d_pick.as<uint32_t>(), k, c->d_keys.as<uint8_t>());
        SLX_HIPCHK(hipGetLastError());
        SLX_HIPCHK(hipMemcpyAsync(c->h_keys.p, c->d_keys.p, (size_t)k * ST_KEY_STRIDE, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(slx_wait_stream(st));
        const uint32_t before = c->G.size();
        for (uint32_t j = 0; j < k; ++j) {
            const uint8_t *e = c->h_keys.as<uint8_t>() + (size_t)j * ST_KEY_STRIDE;
            const uint32_t len = (uint32_t)e[0] | (uint32_t)e[1] << 8;
            if (len == 0 || len > ST_MAX_KEY) { slx_set_error("read statistics: record %u of the batch gave no group key on the second look", list[j]); return SLX_EINTERNAL; }
            if (c->G.find(e + 4, len) == ST_NO_GROUP && c->G.size() >= c->max_groups) {          // (before the group exists; the groups of this round get their rows)
                SLX_CHK(st_upload_groups(c));
                slx_set_error("read statistics: record %u of the batch opens one read group more than max_groups = %u (a group costs %zu bytes of HBM; names that are unique up to their first ':' make a group per read)",
                              list[j], c->max_groups, 8 * (size_t)c->L.row * ST_REPLICAS);
                return SLX_EUNSUPPORTED;
            }
            (void)c->G.intern(e + 4, len);
        }
        if (c->G.size() == before) { slx_set_error("read statistics: %llu records miss a table that holds their groups", (ull)n_miss); return SLX_EINTERNAL; }
        SLX_CHK(st_upload_groups(c));
        only = miss;
        cur ^= 1;
    }
    SLX_HIPCHK(hipEventRecord(c->ev[1], st));
    SLX_HIPCHK(slx_wait_stream(st));
    c->us_add += slx_ev_us(c->ev[0], c->ev[1]);
    c->c_seen += (int64_t)n;
    return SLX_OK;
}

extern "C" int slx_stats_add_device(slx_stats *c, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records)
{
    SLX_CHK(slx_need(c, "slx_stats_add_device"));
    SLX_CHK(slx_batch_args("slx_stats_add_device", d_stream, n_bytes, d_rec_off, n_records));
    return st_add(c, (const uint8_t *)d_stream, (uint64_t)n_bytes, (const ull *)d_rec_off, (uint64_t)n_records);
}

extern "C" int slx_stats_add_host(slx_stats *c, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records)
{
    SLX_CHK(slx_need(c, "slx_stats_add_host"));
    SLX_CHK(slx_batch_args("slx_stats_add_host", stream, n_bytes, rec_off, n_records));
    if (n_records == 0) return SLX_OK;
    SLX_CHK(slx_batch_stage(c->d_in, c->d_off, 16, stream, n_bytes, rec_off, n_records, c->st));
    return st_add(c, c->d_in.as<uint8_t>(), (uint64_t)n_bytes, c->d_off.as<ull>(), (uint64_t)n_records);
}

extern "C" int slx_stats_record(const uint8_t *rec, int64_t n, slx_stats_rec *out)
{
    if (!rec || n < 0 || !out) { slx_set_error("slx_stats_record: null or negative argument"); return SLX_EINVAL; }
    memset(out, 0, sizeof *out);
    rf_feat F;
    st_rec R;
    memset(&R, 0, sizeof R);
    const uint32_t er = st_record(rec, (uint64_t)n, &F, &R);
    if (er & (RF_E_FIELDS | RF_E_AUX)) {
        slx_set_error("read statistics: the record's fields pass its block_size, its extent is not block_size + 4, or an aux field is of unknown type or passes the record's end");
        return SLX_EIO;
    }
    if (er) { slx_set_error("read statistics: the record's group key is longer than %u bytes", ST_MAX_KEY); return SLX_EUNSUPPORTED; }
    for (int h = 0; h < ST_N_HIST; ++h) out->value[h] = R.v[h];
    out->flag = R.flag; out->has_nm = (int32_t)R.has_nm; out->group_len = (int32_t)R.key_len;
    for (uint32_t i = 0; i < R.key_len; ++i) out->group[i] = (char)st_key_byte(&R, i);
    return SLX_OK;
}

// the rows of every group on the host
static int st_sync(const char *who, slx_stats *c)
{
    if (!c) { slx_set_error("%s: null object", who); return SLX_EINVAL; }
    if (c->synced) return SLX_OK;
    SLX_CHK(slx_need(c, who));
    const size_t row = c->L.row;
    c->h_counts.assign((size_t)c->G.size() * row, 0);
    std::vector<uint64_t> all(c->h_counts.size() * ST_REPLICAS);
    if (!all.empty()) SLX_HIPCHK(hipMemcpy(all.data(), c->d_counts.p, 8 * all.size(), hipMemcpyDeviceToHost));
    for (size_t g = 0; g < c->G.size(); ++g)          // the copies of a row, summed
        for (size_t r = 0; r < ST_REPLICAS; ++r)
            for (size_t k = 0; k < row; ++k) c->h_counts[g * row + k] += all[(g * ST_REPLICAS + r) * row + k];
    c->synced = true;
    return SLX_OK;
}
static int st_group(const char *who, slx_stats *c, int64_t i)
{
    SLX_CHK(st_sync(who, c));
    if (i < 0 || i >= (int64_t)c->G.size()) { slx_set_error("%s: group %lld is not one of the %u", who, (long long)i, c->G.size()); return SLX_EINVAL; }
    return SLX_OK;
}

extern "C" int64_t slx_stats_n_groups(slx_stats *c)
{
    if (!c) { slx_set_error("slx_stats_n_groups: null object"); return SLX_EINVAL; }
    return c->G.size();
}

extern "C" const char *slx_stats_group_name(slx_stats *c, int64_t i)
{
    if (!c || i < 0 || i >= (int64_t)c->G.size()) return nullptr;
    if (c->names.size() != c->G.size()) { c->names.clear(); for (uint32_t g = 0; g < c->G.size(); ++g) c->names.push_back(c->G.name(g)); }
    return c->names[(size_t)i].c_str();
}

extern "C" int64_t slx_stats_counter_of(slx_stats *c, int64_t i, const char *name)
{
    SLX_CHK(st_group("slx_stats_counter_of", c, i));
    const int k = name ? st_counter_index(name) : -1;
    if (k < 0) { slx_set_error("slx_stats_counter_of: unknown counter '%s'", name ? name : "(null)"); return SLX_EINVAL; }
    return (int64_t)c->h_counts[(size_t)i * c->L.row + k];
}

extern "C" int slx_stats_hist(slx_stats *c, int64_t i, int which, uint64_t *bins, int64_t cap, uint64_t *below, uint64_t *above)
{
    SLX_CHK(st_group("slx_stats_hist", c, i));
    if (which < 0 || which >= ST_N_HIST || !bins || cap < (int64_t)c->L.nb[which]) { slx_set_error("slx_stats_hist: unknown histogram, null output or fewer than its bins"); return SLX_EINVAL; }
    const uint64_t *row = c->h_counts.data() + (size_t)i * c->L.row + c->L.base[which];
    if (below) *below = row[0];
    if (above) *above = row[1];
    memcpy(bins, row + 2, 8 * (size_t)c->L.nb[which]);
    return SLX_OK;
}

extern "C" int slx_stats_bins(slx_stats *c, int which, int32_t *lo, int32_t *hi, int64_t cap, int64_t *n)
{
    if (!c || !n || which < 0 || which >= ST_N_HIST || cap < 0 || (cap && (!lo || !hi))) { slx_set_error("slx_stats_bins: null, negative or unknown argument"); return SLX_EINVAL; }
    *n = c->L.nb[which];
    for (int64_t k = 0; k < std::min<int64_t>(*n, cap); ++k) { lo[k] = st_bin_lo(&c->L, which, (uint32_t)k); hi[k] = st_bin_hi(&c->L, which, (uint32_t)k); }
    return SLX_OK;
}

extern "C" int slx_stats_text(slx_stats *c, char **text, int64_t *n)
{
    if (!text || !n) { slx_set_error("slx_stats_text: null argument"); return SLX_EINVAL; }
    *text = nullptr; *n = 0;
    SLX_CHK(st_sync("slx_stats_text", c));
    const std::string t = st_text(c->L, c->G, c->h_counts.data());
    char *p = (char *)malloc(t.size() + 1);
    if (!p) { slx_set_error("slx_stats_text: cannot allocate %zu bytes", t.size() + 1); return SLX_ENOMEM; }
    memcpy(p, t.c_str(), t.size() + 1);
    *text = p; *n = (int64_t)t.size();
    return SLX_OK;
}
extern "C" void slx_stats_text_free(char *text) { free(text); }

extern "C" int slx_stats_merge(slx_stats *dst, slx_stats *src)
{
    if (!dst || !src || dst == src) { slx_set_error("slx_stats_merge: null argument, or an object into itself"); return SLX_EINVAL; }
    if (memcmp(dst->L.start, src->L.start, sizeof dst->L.start) || memcmp(dst->L.end, src->L.end, sizeof dst->L.end) || memcmp(dst->L.width, src->L.width, sizeof dst->L.width)) {
        slx_set_error("slx_stats_merge: the bin layouts differ (len_max %d and %d, isize_max %d and %d)", dst->len_max, src->len_max, dst->isize_max, src->isize_max);
        return SLX_EINVAL;
    }
    SLX_CHK(st_sync("slx_stats_merge", src));
    if (src->G.size() == 0) return SLX_OK;
    SLX_CHK(slx_need(dst, "slx_stats_merge"));
    SLX_CHK(st_sync("slx_stats_merge", dst));
    const size_t row = dst->L.row;
    size_t n_new = 0;
    for (uint32_t g = 0; g < src->G.size(); ++g) { const std::string nm = src->G.name(g); n_new += dst->G.find((const uint8_t *)nm.data(), (uint32_t)nm.size()) == ST_NO_GROUP; }
    if (dst->G.size() + n_new > dst->max_groups) { slx_set_error("slx_stats_merge: %zu read groups, more than max_groups = %u; nothing was merged", dst->G.size() + n_new, dst->max_groups); return SLX_EUNSUPPORTED; }
    for (uint32_t g = 0; g < src->G.size(); ++g) {
        const std::string nm = src->G.name(g);
        const uint32_t d = dst->G.intern((const uint8_t *)nm.data(), (uint32_t)nm.size());
        if (dst->h_counts.size() < (size_t)dst->G.size() * row) dst->h_counts.resize((size_t)dst->G.size() * row, 0);
        for (size_t k = 0; k < row; ++k) dst->h_counts[d * row + k] += src->h_counts[g * row + k];
    }
    dst->started = true;
    SLX_CHK(st_upload_groups(dst));
    std::vector<uint64_t> all(dst->h_counts.size() * ST_REPLICAS, 0);          // the sums into copy 0 of every row
    for (size_t g = 0; g < dst->G.size(); ++g) memcpy(&all[g * ST_REPLICAS * row], &dst->h_counts[g * row], 8 * row);
    SLX_HIPCHK(hipMemcpy(dst->d_counts.p, all.data(), 8 * all.size(), hipMemcpyHostToDevice));
    dst->c_seen += src->c_seen; dst->c_counted += src->c_counted;
    return SLX_OK;
}

extern "C" int slx_stats_clear(slx_stats *c)
{
    if (!c) { slx_set_error("slx_stats_clear: null object"); return SLX_EINVAL; }
    c->G.reset(c->group_slots);
    c->h_counts.clear(); c->names.clear(); c->synced = true; c->started = false;
    c->c_seen = c->c_counted = c->c_long = c->c_lds = c->c_global = c->c_miss = 0; c->us_add = 0;
    if (c->device >= 0 && c->rows_cap) {
        SLX_HIPCHK(hipSetDevice(c->device));
        SLX_HIPCHK(hipMemsetAsync(c->d_counts.p, 0, c->rows_cap * 8 * (size_t)c->L.row * ST_REPLICAS, c->st));
        SLX_HIPCHK(slx_wait_stream(c->st));
    }
    return SLX_OK;
}

extern "C" int64_t slx_stats_counter(const slx_stats *c, const char *name)
{
    if (!c || !name) return -1;
    if (!strcmp(name, "records_seen")) return c->c_seen;
    if (!strcmp(name, "records_counted")) return c->c_counted;
    if (!strcmp(name, "long_records")) return c->c_long;
    if (!strcmp(name, "adds_lds")) return c->c_lds;
    if (!strcmp(name, "adds_global")) return c->c_global;
    if (!strcmp(name, "group_misses")) return c->c_miss;
    if (!strcmp(name, "us_add")) return (int64_t)c->us_add;
    return -1;
}
