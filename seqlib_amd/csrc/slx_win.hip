// slx_win.hip -- assembly windows collected from BAM records in HBM (include/seqlib_amd_win.h): batches of records and a collection of windows in, the
// assembler's staged read arrays out.  DESIGN.md section 9.14.
//   add:     k_win_measure        a lane per record: its span, its fixed fields, the selection and the trim of win_host.h; with a trim, a record longer than
//                                 wave_len is listed instead
//            k_win_measure_long   a wave per listed record: the qualities 64 bytes per ballot from both ends
//            slx_exclusive_sum    the padded lengths -> where each kept stretch lies in the arena segment
//            slx_grc_overlaps_device   the join of seqlib_amd_grc.h: which windows a record is a read of
//            k_win_count, slx_exclusive_sum   the entries each record appends
//            k_win_extract        one wave per WN_TILE bytes of the segment: nibbles to ASCII, qualities + 33, the strand flip          dev_win.h wn_extract_word
//            k_win_entries        a lane per record: an entry (window, ordinal, arena address, length) per pair
//   finish:  k_win_keys, hipcub::DeviceRadixSort::SortPairs (stable: entries are appended in ordinal order), k_win_lens, slx_exclusive_sum, k_win_winoff,
//            k_win_gather         one wave per WN_TILE bytes of the output                                                               dev_win.h wn_gather_tile
// Records map to lanes and tiles to waves statically: no work queue.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "slx_internal.h"
#include "slx_hip.h"
#include "seqlib_amd_win.h"
#include "dev_lanes.h"
#include "dev_wave.h"
#include "dev_win.h"

typedef unsigned long long ull;
typedef SlxDevBuf<SlxMargin<8, 256>> WDBuf;
typedef SlxDevBuf<SlxExact> WSeg;
typedef SlxPinBuf<SlxExact> WHBuf;

static const char WIN_NO_DEVICE[] = "no HIP device: assembly windows are collected on MI355X only (no CPU fallback)";
#define WIN_SEG_MIN (8ull << 20)          // an arena segment holds this much at least (or "arena_bytes" when that is less)

// bad: the first broken record (atomicMin); n_long: records left to k_win_measure_long; max_len: of the finished reads
struct wn_state { ull bad; uint32_t n_long, max_len; uint32_t drop[WN_N_STATUS]; };
struct wn_args { const uint8_t *s; uint64_t n_bytes; const uint64_t *off; uint64_t n; };

// ------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void k_win_measure(wn_rules R, wn_args A, wn_rec *M, ull *sz, uint32_t *longlist, wn_state *st)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool broken = false;
    if (i == A.n) sz[i] = 0;
    if (i < A.n) {
        uint32_t span = 0;
        bool own = false;
        wn_rec m = {WN_BROKEN, 0, 0, 0, 0, 0};
        if (!ed_span(A.s, A.n_bytes, A.off, i, A.n, &span, &own)) broken = true;
        else if (own) {          // (when not, record i + 1 is the one named, by its own lane)
            const uint8_t *rec = A.s + (A.off[i] - A.off[0]);
            const uint32_t s = wn_select(R, rec, span, &m);
            if (s == WN_BROKEN) broken = true;
            else if (s == WN_KEEP) {
                if (R.qual_trim >= 0 && m.l_seq > R.wave_len) longlist[wave_fetch_inc(&st->n_long)] = (uint32_t)i;
                else (void)wn_keep<false>(R, rec, &m, 0, 1);
            }
            if (m.status != WN_KEEP && m.status != WN_BROKEN) atomicAdd(&st->drop[m.status], 1u);
        }
        M[i] = m;
        sz[i] = m.status == WN_KEEP ? wn_padded(m.klen) : 0;
    }
    wave_report_min(&st->bad, broken, i);
}

// (only records that k_win_measure has selected are listed: their fields lie inside their spans)
__global__ __launch_bounds__(256) void k_win_measure_long(wn_rules R, wn_args A, const uint32_t *longlist, uint32_t n_long, wn_rec *M, ull *sz, wn_state *st)
{
    const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= n_long) return;          // (a whole wave)
    const uint64_t i = longlist[w];
    const uint8_t *rec = A.s + (A.off[i] - A.off[0]);
    wn_rec m = M[i];          // (every lane keeps its own copy; lane 0's takes the result)
    const uint32_t status = wn_keep<true>(R, rec, &m, (int)lane, 64);
    if (lane == 0) {
        M[i] = m;
        sz[i] = status == WN_KEEP ? wn_padded(m.klen) : 0;
        if (status == WN_TRIMMED) atomicAdd(&st->drop[WN_TRIMMED], 1u);
    }
}

// the entries record i appends: one per pair of the join when it is kept
__global__ __launch_bounds__(256) void k_win_count(const wn_rec *M, const uint32_t *count, uint64_t n, ull *ecnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) ecnt[i] = i < n && M[i].status == WN_KEEP ? count[i] : 0;
}

__global__ __launch_bounds__(256) void k_win_extract(wn_args A, const ull *aoff, const wn_rec *M, uint64_t n_words, uint8_t *ob, uint8_t *oq)
{
    __shared__ uint8_t lut[32];
    if (threadIdx.x < 32) lut[threadIdx.x] = (uint8_t)(threadIdx.x < 16 ? WN_SEQ_FWD[threadIdx.x] : WN_SEQ_REV[threadIdx.x - 16]);
    __syncthreads();
    // a wave's tile: words [128 t, 128 t + 128), two per lane, a lane's two words 64 apart so that a store instruction covers 1 KiB
    const uint64_t t = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (uint32_t h = 0; h < WN_TILE / 1024; ++h) {
        const uint64_t w = t * (WN_TILE / 16) + h * 64 + lane;
        if (w < n_words) wn_extract_word(A.s, A.off, aoff, M, A.n, w, (const ED_LDS uint8_t *)lut, ob, oq);
    }
}

__global__ __launch_bounds__(256) void k_win_entries(const wn_rec *M, const ull *aoff, const ull *eoff, const long long *pair_off, const int32_t *subject_id, uint64_t n, long long ord0,
                                                     ull seg_b, ull seg_q, wn_entry *ent)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || M[i].status != WN_KEEP) return;
    ull e = eoff[i];
    for (long long p = pair_off[i]; p < pair_off[i + 1]; ++p, ++e) ent[e] = wn_entry{seg_b + aoff[i], seg_q + aoff[i], ord0 + (long long)i, (uint32_t)subject_id[p], M[i].klen};
}

__global__ __launch_bounds__(256) void k_win_keys(const wn_entry *ent, uint64_t n, uint32_t *key, uint32_t *idx)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { key[i] = ent[i].win; idx[i] = (uint32_t)i; }
}

__global__ __launch_bounds__(256) void k_win_lens(const wn_entry *ent, const uint32_t *idx, uint64_t n, ull *len, long long *rec_of_read, wn_state *st)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t l = 0;
    if (i == n) len[i] = 0;
    if (i < n) { const wn_entry E = ent[idx[i]]; l = E.len; len[i] = l; rec_of_read[i] = E.ord; }
    l = wave_max(l);
    if ((threadIdx.x & 63) == 0 && l) atomicMax(&st->max_len, l);
}

// win_off[w]: the first sorted entry whose window is w or later
__global__ __launch_bounds__(256) void k_win_winoff(const uint32_t *key, uint64_t n, uint64_t n_win, long long *win_off)
{
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w > n_win) return;
    uint64_t lo = 0, hi = n;          // key[k] < w below lo, >= w from hi on
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (key[mid] < w) lo = mid + 1; else hi = mid; }
    win_off[w] = (long long)lo;
}

__global__ __launch_bounds__(256) void k_win_gather(const ull *offs, const wn_entry *ent, const uint32_t *idx, uint64_t n_reads, uint64_t total, uint64_t n_tiles, uint8_t *ob, uint8_t *oq)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[4][WN_TILE];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t t = (uint64_t)blockIdx.x * 4 + wave;
    if (t >= n_tiles) return;          // (a whole wave)
    wn_gather_tile(offs, ent, idx, n_reads, total, t, (int)blockIdx.y, (ED_LDS uint8_t *)tile[wave], blockIdx.y ? oq : ob, (int)lane, 64);
}

// ------------------------------------------------------------------ host
struct wn_seg { std::unique_ptr<WSeg> buf; uint64_t used = 0; };
struct wn_counts { int64_t records = 0, pairs = 0, reads = 0, drop[WN_N_STATUS] = {}, n_long = 0, arena = 0; };

struct slx_win : SlxGpu<2> {
    slx_win() : SlxGpu(WIN_NO_DEVICE) {}
    slx_grc *g = nullptr;
    int64_t n_win = 0;
    wn_rules R = {0u, -1, 0u, WN_WAVE_LEN};
    int64_t arena_bytes = 1ll << 34;
    std::vector<wn_seg> segs;
    uint64_t n_ent = 0;
    long long ordinal = 0;
    wn_counts c;
    double us_measure = 0, us_join = 0, us_extract = 0, us_entries = 0, us_sort = 0, us_gather = 0;
    bool finished = false;
    slx_win_result res = {};
    WDBuf d_in{*this}, d_off{*this}, d_M{*this}, d_sz{*this}, d_aoff{*this}, d_long{*this}, d_state{*this}, d_tmp{*this}, d_ecnt{*this}, d_eoff{*this}, d_ent{*this};
    WDBuf d_key{*this}, d_key2{*this}, d_idx{*this}, d_idx2{*this}, d_len{*this}, d_offs{*this}, d_winoff{*this}, d_ror{*this}, d_bases{*this}, d_quals{*this};
    WHBuf h_small{*this};
};

static unsigned win_blocks(uint64_t n, unsigned per = 256) { return (unsigned)((n + per - 1) / per); }

extern "C" void slx_win_free(slx_win *w)
{
    if (!w) return;
    w->close();
    slx_grc_free(w->g);
    delete w;
}

extern "C" int slx_win_create(int device, const slx_grc_iv *windows, int64_t n_win, slx_win **out)
{
    if (!out) { slx_set_error("slx_win_create: null argument"); return SLX_EINVAL; }
    *out = nullptr;
    if (device < SLX_WIN_AUTO || n_win < 0 || (n_win && !windows)) { slx_set_error("slx_win_create: device %d, %lld windows", device, (long long)n_win); return SLX_EINVAL; }
    return slx_create(out, slx_win_free, [&](slx_win *w) {
        if (device != SLX_WIN_HOST) SLX_CHK(w->open(device == SLX_WIN_AUTO ? -1 : device, "slx_win_create", WIN_NO_DEVICE, device == SLX_WIN_AUTO));
        SLX_CHK(slx_grc_create(w->device >= 0 ? w->device : SLX_GRC_HOST, windows, n_win, &w->g));
        w->n_win = n_win;
        return (int)SLX_OK;
    });
}

extern "C" int slx_win_set(slx_win *w, const char *key, int64_t v)
{
    if (!w || !key) { slx_set_error("slx_win_set: null argument"); return SLX_EINVAL; }
    if (!strcmp(key, "skip_flags") && v >= 0 && v <= 0xffff) { w->R.skip_flags = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "qual_trim") && v >= -1 && v <= WN_MAX_TRIM) { w->R.qual_trim = (int32_t)v; return SLX_OK; }
    if (!strcmp(key, "original_strand") && (v == 0 || v == 1)) { w->R.original_strand = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "wave_len") && v >= 0 && v <= (1 << 20)) { w->R.wave_len = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "arena_bytes") && v >= 0) { w->arena_bytes = v; return SLX_OK; }
    slx_set_error("slx_win_set: unknown key '%s' or value %lld out of range", key, (long long)v);
    return SLX_EINVAL;
}

extern "C" int64_t slx_win_counter(const slx_win *w, const char *name)
{
    if (!w || !name) return -1;
    const std::string k = name;
    if (k == "device") return w->device;
    if (k == "windows") return w->n_win;
    if (k == "skip_flags") return w->R.skip_flags;
    if (k == "qual_trim") return w->R.qual_trim;
    if (k == "original_strand") return w->R.original_strand;
    if (k == "wave_len") return w->R.wave_len;
    if (k == "arena_bytes") return w->arena_bytes;
    if (k == "records") return w->c.records;
    if (k == "pairs") return w->c.pairs;
    if (k == "reads") return w->c.reads;
    if (k == "drop_flags") return w->c.drop[WN_SKIP_FLAG];
    if (k == "drop_no_seq") return w->c.drop[WN_NO_SEQ];
    if (k == "drop_no_name") return w->c.drop[WN_NO_NAME];
    if (k == "drop_trimmed") return w->c.drop[WN_TRIMMED];
    if (k == "long_reads") return w->c.n_long;
    if (k == "arena_bytes_used") return w->c.arena;
    if (k == "us_measure") return (int64_t)w->us_measure;
    if (k == "us_join") return (int64_t)w->us_join;
    if (k == "us_extract") return (int64_t)w->us_extract;
    if (k == "us_entries") return (int64_t)w->us_entries;
    if (k == "us_sort") return (int64_t)w->us_sort;
    if (k == "us_gather") return (int64_t)w->us_gather;
    return -1;
}

extern "C" void slx_win_quality_trim(const uint8_t *qual, int32_t len, int32_t qual_trim, int32_t *startpoint, int32_t *endpoint)
{
    int32_t a = 0, b = -1;
    if (qual) wn_trim<false>(qual, len, qual_trim, &a, &b, 0, 1);
    if (startpoint) *startpoint = a;
    if (endpoint) *endpoint = b;
}

// between two events of the handle on its drained stream
#define WIN_T0(w) SLX_HIPCHK(hipEventRecord((w)->ev[0], (w)->st))
#define WIN_T1(w, acc) do { SLX_HIPCHK(hipEventRecord((w)->ev[1], (w)->st)); SLX_HIPCHK(slx_wait_stream((w)->st)); acc += slx_ev_us((w)->ev[0], (w)->ev[1]); } while (0)

// the segment that takes `need` more bytes: the last one when it has room, a new one otherwise
static int win_segment(slx_win *w, uint64_t need, size_t *seg_at)
{
    if (!w->segs.empty()) {
        wn_seg &s = w->segs.back();
        if (s.buf->cap - s.used >= need) { *seg_at = w->segs.size() - 1; return SLX_OK; }
    }
    uint64_t cap = std::max<uint64_t>(need, std::min<uint64_t>(WIN_SEG_MIN, (uint64_t)w->arena_bytes));
    for (size_t k = 0; k < w->segs.size(); ++k) {          // (an emptied segment of a cleared collector that is large enough)
        if (w->segs[k].used == 0 && w->segs[k].buf->cap >= need) { std::swap(w->segs[k], w->segs.back()); *seg_at = w->segs.size() - 1; return SLX_OK; }
    }
    wn_seg s;
    s.buf.reset(new WSeg(*w));
    SLX_CHK(s.buf->ensure(cap));
    w->segs.push_back(std::move(s));
    *seg_at = w->segs.size() - 1;
    return SLX_OK;
}

static int win_add(slx_win *w, const char *who, const uint8_t *d_s, uint64_t n_bytes, const uint64_t *d_off, uint64_t n)
{
    hipStream_t st = w->st;
    if (n == 0) {
        if (n_bytes) { slx_set_error("assembly windows: %llu bytes and no record", (ull)n_bytes); return SLX_EIO; }
        return SLX_OK;
    }
    if (n >= 0x7fffffffull) { slx_set_error("%s: 2^31 - 1 records or more in one batch", who); return SLX_EUNSUPPORTED; }
    SLX_CHK(w->d_M.ensure(sizeof(wn_rec) * (n + 1))); SLX_CHK(w->d_sz.ensure(8 * (n + 2))); SLX_CHK(w->d_aoff.ensure(8 * (n + 2))); SLX_CHK(w->d_long.ensure(4 * (n + 1)));
    SLX_CHK(w->d_ecnt.ensure(8 * (n + 2))); SLX_CHK(w->d_eoff.ensure(8 * (n + 2))); SLX_CHK(w->d_state.ensure(sizeof(wn_state))); SLX_CHK(w->h_small.ensure(512));
    wn_state *hs = w->h_small.as<wn_state>();
    memset(hs, 0, sizeof(wn_state));
    hs->bad = ED_NONE;
    const wn_args A = {d_s, n_bytes, d_off, n};
    double us_measure = 0, us_join = 0, us_extract = 0, us_entries = 0;
    SLX_HIPCHK(hipMemcpyAsync(w->d_state.p, hs, sizeof(wn_state), hipMemcpyHostToDevice, st));
    WIN_T0(w);
    k_win_measure<<<win_blocks(n + 1), 256, 0, st>>>(w->R, A, w->d_M.as<wn_rec>(), w->d_sz.as<ull>(), w->d_long.as<uint32_t>(), w->d_state.as<wn_state>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipMemcpyAsync(hs + 1, w->d_state.p, sizeof(wn_state), hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync((ull *)(hs + 2) + 2, d_off, 8, hipMemcpyDeviceToHost, st));          // the first offset: what the join's stream pointer is moved down by
    WIN_T1(w, us_measure);
    if (hs[1].bad != ED_NONE) {
        slx_set_error("assembly windows: record %llu of the batch: its fields pass its block_size, its name does not end in NUL, or its extent is not block_size + 4 inside the stream", hs[1].bad);
        return SLX_EIO;
    }
    const uint32_t n_long = hs[1].n_long;
    if (n_long) {
        WIN_T0(w);
        k_win_measure_long<<<win_blocks(n_long, 4), 256, 0, st>>>(w->R, A, w->d_long.as<uint32_t>(), n_long, w->d_M.as<wn_rec>(), w->d_sz.as<ull>(), w->d_state.as<wn_state>());
        SLX_HIPCHK(hipGetLastError());
        SLX_HIPCHK(hipMemcpyAsync(hs + 1, w->d_state.p, sizeof(wn_state), hipMemcpyDeviceToHost, st));
        WIN_T1(w, us_measure);
    }
    ull *tot = (ull *)(hs + 2);
    SLX_CHK(slx_exclusive_sum(w->d_tmp, w->d_sz.as<ull>(), w->d_aoff.as<ull>(), n + 1, st, 16));
    SLX_HIPCHK(hipMemcpyAsync(tot, w->d_aoff.as<ull>() + n, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    const uint64_t seg_bytes = tot[0], need = 2 * seg_bytes;
    // the join: the records rule of seqlib_amd_grc.h, on the collection's own stream; its device arrays stay valid until the next call on it
    slx_grc_result jr;
    const double j0 = (double)slx_grc_counter(w->g, "us_records") + (double)slx_grc_counter(w->g, "us_count") + (double)slx_grc_counter(w->g, "us_fill");
    // (that unit's offsets count from its stream pointer, this one's from d_rec_off[0]: the pointer moves down by the first offset and is never read below d_s)
    const uint64_t off0 = tot[2];
    SLX_CHK(slx_grc_overlaps_device(w->g, d_s - off0, (int64_t)(n_bytes + off0), d_off, (int64_t)n, 1, &jr));
    us_join = (double)slx_grc_counter(w->g, "us_records") + (double)slx_grc_counter(w->g, "us_count") + (double)slx_grc_counter(w->g, "us_fill") - j0;
    const int64_t n_pairs = jr.n_pairs;
    const uint32_t *d_count = (const uint32_t *)jr.d_count;
    const long long *d_pair_off = (const long long *)jr.d_offset;
    const int32_t *d_subject = (const int32_t *)jr.d_subject_id;
    slx_grc_result_free(&jr);
    k_win_count<<<win_blocks(n + 1), 256, 0, st>>>(w->d_M.as<wn_rec>(), d_count, n, w->d_ecnt.as<ull>());
    SLX_HIPCHK(hipGetLastError());
    SLX_CHK(slx_exclusive_sum(w->d_tmp, w->d_ecnt.as<ull>(), w->d_eoff.as<ull>(), n + 1, st, 16));
    SLX_HIPCHK(hipMemcpyAsync(tot + 1, w->d_eoff.as<ull>() + n, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    const uint64_t n_new = tot[1];
    if (w->n_ent + n_new >= 0x100000000ull) { slx_set_error("%s: %llu entries with this batch: 2^32 entries or more", who, (ull)(w->n_ent + n_new)); return SLX_EUNSUPPORTED; }
    if ((uint64_t)w->c.arena + need > (uint64_t)w->arena_bytes) {
        slx_set_error("%s: the arena would hold %llu bytes with this batch, \"arena_bytes\" is %lld", who, (ull)((uint64_t)w->c.arena + need), (long long)w->arena_bytes);
        return SLX_EUNSUPPORTED;
    }
    if (n_new) {
        size_t seg_at = 0;
        SLX_CHK(win_segment(w, need, &seg_at));
        wn_seg &S = w->segs[seg_at];
        uint8_t *ob = S.buf->as<uint8_t>() + S.used, *oq = ob + seg_bytes;          // (used and seg_bytes are multiples of 16; hipMalloc aligns to 256)
        SLX_CHK(w->d_ent.ensure(sizeof(wn_entry) * (w->n_ent + n_new), st, sizeof(wn_entry) * w->n_ent));
        const uint64_t n_words = seg_bytes >> 4, n_tiles = (seg_bytes + WN_TILE - 1) / WN_TILE;
        WIN_T0(w);
        k_win_extract<<<win_blocks(n_tiles, 4), 256, 0, st>>>(A, w->d_aoff.as<ull>(), w->d_M.as<wn_rec>(), n_words, ob, oq);
        SLX_HIPCHK(hipGetLastError());
        WIN_T1(w, us_extract);
        WIN_T0(w);
        k_win_entries<<<win_blocks(n), 256, 0, st>>>(w->d_M.as<wn_rec>(), w->d_aoff.as<ull>(), w->d_eoff.as<ull>(), d_pair_off, d_subject, n, w->ordinal, (ull)(uintptr_t)ob, (ull)(uintptr_t)oq,
                                                    w->d_ent.as<wn_entry>() + w->n_ent);
        SLX_HIPCHK(hipGetLastError());
        WIN_T1(w, us_entries);
        S.used += need;
        w->c.arena += (int64_t)need;
    }
    // only now does the collector change
    w->n_ent += n_new; w->ordinal += (long long)n; w->finished = false;
    w->c.records += (int64_t)n; w->c.pairs += n_pairs; w->c.reads += (int64_t)n_new; w->c.n_long += n_long;
    for (int k = 0; k < WN_N_STATUS; ++k) w->c.drop[k] += hs[1].drop[k];
    w->us_measure += us_measure; w->us_join += us_join; w->us_extract += us_extract; w->us_entries += us_entries;
    return SLX_OK;
}

extern "C" int slx_win_add_device(slx_win *w, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records)
{
    SLX_CHK(slx_need(w, "slx_win_add_device"));
    SLX_CHK(slx_batch_args("slx_win_add_device", d_stream, n_bytes, d_rec_off, n_records));
    return win_add(w, "slx_win_add_device", (const uint8_t *)d_stream, (uint64_t)n_bytes, (const uint64_t *)d_rec_off, (uint64_t)n_records);
}

extern "C" int slx_win_add_host(slx_win *w, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records)
{
    SLX_CHK(slx_need(w, "slx_win_add_host"));
    SLX_CHK(slx_batch_args("slx_win_add_host", stream, n_bytes, rec_off, n_records));
    if (n_records) {
        SLX_CHK(slx_batch_stage(w->d_in, w->d_off, 16, stream, n_bytes, rec_off, n_records, w->st));
        SLX_HIPCHK(slx_wait_stream(w->st));
    }
    return win_add(w, "slx_win_add_host", w->d_in.as<uint8_t>(), (uint64_t)n_bytes, w->d_off.as<uint64_t>(), (uint64_t)n_records);
}

extern "C" int slx_win_finish(slx_win *w)
{
    SLX_CHK(slx_need(w, "slx_win_finish"));
    hipStream_t st = w->st;
    const uint64_t n = w->n_ent, nw = (uint64_t)w->n_win;
    w->finished = false;
    if (n >= 0x7fffffffull) { slx_set_error("slx_win_finish: %llu entries: hipCUB sorts 2^31 - 1 at most in one call", (ull)n); return SLX_EUNSUPPORTED; }
    SLX_CHK(w->d_key.ensure(4 * n + 4)); SLX_CHK(w->d_key2.ensure(4 * n + 4)); SLX_CHK(w->d_idx.ensure(4 * n + 4)); SLX_CHK(w->d_idx2.ensure(4 * n + 4));
    SLX_CHK(w->d_len.ensure(8 * (n + 2))); SLX_CHK(w->d_offs.ensure(8 * (n + 2))); SLX_CHK(w->d_winoff.ensure(8 * (nw + 2))); SLX_CHK(w->d_ror.ensure(8 * (n + 1)));
    SLX_CHK(w->d_state.ensure(sizeof(wn_state))); SLX_CHK(w->h_small.ensure(512));
    wn_state *hs = w->h_small.as<wn_state>();
    SLX_HIPCHK(hipMemsetAsync(w->d_state.p, 0, sizeof(wn_state), st));
    WIN_T0(w);
    if (n) {
        int bits = 1;
        while (bits < 32 && (1ull << bits) < nw) ++bits;
        k_win_keys<<<win_blocks(n), 256, 0, st>>>(w->d_ent.as<wn_entry>(), n, w->d_key.as<uint32_t>(), w->d_idx.as<uint32_t>());
        SLX_HIPCHK(hipGetLastError());
        SLX_CHK(slx_cub("hipcub::DeviceRadixSort::SortPairs", w->d_tmp, 16, [&](void *t, size_t &b) {
            return hipcub::DeviceRadixSort::SortPairs(t, b, w->d_key.as<uint32_t>(), w->d_key2.as<uint32_t>(), w->d_idx.as<uint32_t>(), w->d_idx2.as<uint32_t>(), (int)n, 0, bits, st);
        }));
    }
    k_win_lens<<<win_blocks(n + 1), 256, 0, st>>>(w->d_ent.as<wn_entry>(), w->d_idx2.as<uint32_t>(), n, w->d_len.as<ull>(), w->d_ror.as<long long>(), w->d_state.as<wn_state>());
    SLX_HIPCHK(hipGetLastError());
    SLX_CHK(slx_exclusive_sum(w->d_tmp, w->d_len.as<ull>(), w->d_offs.as<ull>(), n + 1, st, 16));
    k_win_winoff<<<win_blocks(nw + 1), 256, 0, st>>>(w->d_key2.as<uint32_t>(), n, nw, w->d_winoff.as<long long>());
    SLX_HIPCHK(hipGetLastError());
    ull *tot = (ull *)(hs + 2);
    SLX_HIPCHK(hipMemcpyAsync(tot, w->d_offs.as<ull>() + n, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync(hs + 1, w->d_state.p, sizeof(wn_state), hipMemcpyDeviceToHost, st));
    WIN_T1(w, w->us_sort);
    const uint64_t total = tot[0], n_tiles = (total + WN_TILE - 1) / WN_TILE;
    if (n_tiles >= 0x1fffffffull) { slx_set_error("slx_win_finish: %llu bytes of reads", (ull)total); return SLX_EUNSUPPORTED; }
    SLX_CHK(w->d_bases.ensure(total + 64)); SLX_CHK(w->d_quals.ensure(total + 64));
    if (n_tiles) {
        WIN_T0(w);
        k_win_gather<<<dim3(win_blocks(n_tiles, 4), 2), 256, 0, st>>>(w->d_offs.as<ull>(), w->d_ent.as<wn_entry>(), w->d_idx2.as<uint32_t>(), n, total, n_tiles, w->d_bases.as<uint8_t>(),
                                                                    w->d_quals.as<uint8_t>());
        SLX_HIPCHK(hipGetLastError());
        WIN_T1(w, w->us_gather);
    }
    w->res = slx_win_result{w->n_win, (int64_t)n, (int64_t)total, (int64_t)hs[1].max_len, w->d_bases.p, w->d_quals.p, w->d_offs.p, w->d_winoff.p, w->d_ror.p};
    w->finished = true;
    return SLX_OK;
}

extern "C" int slx_win_view(slx_win *w, slx_win_result *out)
{
    SLX_CHK(slx_need(w, "slx_win_view"));
    if (!out) { slx_set_error("slx_win_view: null argument"); return SLX_EINVAL; }
    memset(out, 0, sizeof *out);
    if (!w->finished) { slx_set_error("slx_win_view: no result (slx_win_finish first, after the last add)"); return SLX_EINVAL; }
    *out = w->res;
    return SLX_OK;
}

extern "C" int slx_win_download(slx_win *w, void *bases, void *quals, uint64_t *offs, int64_t *win_off, int64_t *rec_of_read)
{
    SLX_CHK(slx_need(w, "slx_win_download"));
    if (!w->finished) { slx_set_error("slx_win_download: no result (slx_win_finish first, after the last add)"); return SLX_EINVAL; }
    const slx_win_result &r = w->res;
    hipStream_t st = w->st;
    if (bases && r.total) SLX_HIPCHK(hipMemcpyAsync(bases, r.d_bases, (size_t)r.total, hipMemcpyDeviceToHost, st));
    if (quals && r.total) SLX_HIPCHK(hipMemcpyAsync(quals, r.d_quals, (size_t)r.total, hipMemcpyDeviceToHost, st));
    if (offs) SLX_HIPCHK(hipMemcpyAsync(offs, r.d_offs, 8 * ((size_t)r.n_reads + 1), hipMemcpyDeviceToHost, st));
    if (win_off) SLX_HIPCHK(hipMemcpyAsync(win_off, r.d_win_off, 8 * ((size_t)r.n_win + 1), hipMemcpyDeviceToHost, st));
    if (rec_of_read && r.n_reads) SLX_HIPCHK(hipMemcpyAsync(rec_of_read, r.d_rec_of_read, 8 * (size_t)r.n_reads, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    return SLX_OK;
}

extern "C" int slx_win_clear(slx_win *w)
{
    SLX_CHK(slx_need(w, "slx_win_clear"));
    SLX_HIPCHK(slx_wait_stream(w->st));
    for (wn_seg &s : w->segs) s.used = 0;
    w->n_ent = 0; w->ordinal = 0; w->finished = false;
    w->c = wn_counts();
    w->res = slx_win_result{};
    w->us_measure = w->us_join = w->us_extract = w->us_entries = w->us_sort = w->us_gather = 0;
    return SLX_OK;
}
