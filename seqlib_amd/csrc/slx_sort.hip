// slx_sort.hip -- the coordinate sort of libseqlib_amd.so (include/seqlib_amd_sort.h, slx_sort_*): block_size-prefixed BAM records kept in an arena in HBM, sorted
// there and handed to the GPU BGZF writer.  The bodies are dev_recsort.h's; the reader, the writer and the record builder are used through their C-ABI only.
//   k_sort_key        one lane per record of an add: offsets and block_size checked, key, length and source address written, the first bad ordinal and the
//                     highest key kept (one atomic per wave)
//   k_sort_iota       the input ordinals
//   hipCUB            DeviceRadixSort::SortPairs (stable) on key / ordinal, end_bit from the highest key
//   k_sort_perm       lengths and source addresses in sorted order
//   hipCUB            exclusive sum of the lengths = dst_off
//   k_sort_gather     one wave per RS_TILE bytes of the sorted stream, brought together in LDS, stored 16 bytes per lane; launched per slab (a range of tiles)
// Records map to lanes and tiles to waves statically: no work queue.
// Beyond HBM (slx_sort_spill): the add that would pass max_bytes first writes the held records through the same tables and gather as a sorted run file, and
// slx_sort_finish hands the runs to a slx_merge (slx_merge.hip).  Without a spill prefix no line of that runs.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <chrono>
#include <unistd.h>
#include "slx_internal.h"
#include "seqlib_amd_sort.h"
#include "seqlib_amd_dup.h"
#include "seqlib_amd_merge.h"
#include "dev_wave.h"
#include "dev_recsort.h"
#include "recsort_host.h"
#include "slx_hip.h"

typedef unsigned long long ull;
static const int64_t SORT_MAX_SLAB = 1ll << 40;          // 2^29 tiles, 2^27 blocks of k_sort_gather: well inside a grid

struct sort_state { ull bad, max_key; };          // bad: ordinal (inside the add) of the first refused record, RS_NO_BAD = none

// ------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void k_sort_key(const uint8_t *stream, uint64_t n_bytes, const uint64_t *off, uint64_t n, ull *key, uint32_t *len, ull *src, sort_state *st)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    ull k = 0, bad = RS_NO_BAD;
    if (i < n) {
        uint64_t kk = 0; uint32_t l = 0;
        if (rs_key(stream, n_bytes, off, i, n, &kk, &l)) { k = kk; key[i] = kk; len[i] = l; src[i] = (ull)(uintptr_t)(stream + off[i]); }
        else { bad = i; key[i] = 0; len[i] = 0; src[i] = 0; }
    }
    for (int o = 32; o; o >>= 1) {
        const ull k2 = __shfl_xor(k, o, 64), b2 = __shfl_xor(bad, o, 64);
        k = k2 > k ? k2 : k; bad = b2 < bad ? b2 : bad;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&st->max_key, k);
        if (bad != RS_NO_BAD) atomicMin(&st->bad, bad);
    }
}

__global__ __launch_bounds__(256) void k_sort_iota(uint32_t *ord, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) ord[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void k_sort_perm(const uint32_t *ord, const uint32_t *len, const ull *src, uint64_t n, ull *slen, ull *ssrc)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j == n) slen[n] = 0;
    if (j >= n) return;
    const uint32_t o = ord[j];
    slen[j] = len[o]; ssrc[j] = src[o];
}

__global__ __launch_bounds__(256) void k_sort_gather(const ull *dst_off, const ull *ssrc, int64_t n, uint64_t n_bytes, uint64_t tile0, uint64_t tile_end, uint8_t *out)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[4][RS_TILE];
    __shared__ rs_desc desc[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t t = tile0 + (uint64_t)blockIdx.x * 4 + wave;
    if (t >= tile_end) return;          // (a whole wave: the ballots of rs_gather_tile see all 64 lanes)
    rs_gather_tile(dst_off, ssrc, n, n_bytes, t, tile[wave], &desc[wave], out, tile0 * RS_TILE, (int)lane, 64);
}

// ------------------------------------------------------------------ host
static void sort_put32(std::string &o, uint32_t v) { const char b[4] = {(char)v, (char)(v >> 8), (char)(v >> 16), (char)(v >> 24)}; o.append(b, 4); }

namespace {
// no margin: the tables are sized by the held records, which max_bytes bounds -- HBM a margin took would be HBM the budget cannot give to records
typedef SlxDevBuf<SlxExact> SBuf;
typedef SlxPinBuf<SlxExact> SHBuf;

// one add: the bytes and, behind them in the same allocation, the offsets and the three per-record tables
struct Segment {
    uint8_t *base = nullptr;
    uint64_t n_bytes = 0, n = 0;
    uint64_t *off = nullptr; ull *key = nullptr, *src = nullptr; uint32_t *len = nullptr;
};
static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
}  // namespace

struct slx_sort : SlxGpu<> {
    std::vector<Segment> segs;
    uint64_t held_records = 0, held_bytes = 0;
    ull max_key = 0;
    int64_t max_bytes = 0, slab_bytes = 64ll << 20, batch_bytes = 64ll << 20;
    SBuf d_state{*this}, d_key_in{*this}, d_key_out{*this}, d_ord_in{*this}, d_ord_out{*this}, d_len{*this}, d_src{*this}, d_slen{*this}, d_ssrc{*this}, d_doff{*this}, d_tmp{*this},
         d_slab{*this};
    SHBuf h_state{*this};                          // two sort_state: [0] goes up, [1] comes down
    int64_t c_records = 0, c_bytes = 0, c_segments = 0, c_slabs = 0;
    double us_key = 0, us_sort = 0, us_gather = 0;
    // slx_sort_spill: the run files of the sort in progress, in the order their records were added
    bool spill_on = false;
    std::string spill_prefix, spill_header;
    std::vector<std::string> runs;
    int64_t c_runs = 0, c_run_bytes = 0;
    double us_merge = 0;
};

static const size_t SORT_MAX_RUNS = 64;          // what one merger takes (MG_MAX_IN of dev_merge.h)

static void sort_drop_runs(slx_sort *s)
{
    for (const std::string &r : s->runs) (void)unlink(r.c_str());
    s->runs.clear();
}

static void sort_clear(slx_sort *s)
{
    for (Segment &g : s->segs) if (g.base) (void)hipFree(g.base);
    s->segs.clear();
    s->held_records = s->held_bytes = 0; s->max_key = 0;
}

extern "C" void slx_sort_free(slx_sort *s)
{
    if (!s) return;
    if (s->st) { (void)hipSetDevice(s->device); (void)hipStreamSynchronize(s->st); }
    sort_clear(s);          // (the segments are the sorter's own hipMalloc blocks: they go once the stream has drained, before the context closes)
    sort_drop_runs(s);
    s->close();
    delete s;
}

static std::string sort_no_device(const char *who) { return std::string(who) + ": no HIP device: BAM records are sorted on MI355X only (no CPU fallback)"; }

static int sort_init(slx_sort *s, int device)
{
    SLX_CHK(s->open(device, "slx_sort_create", sort_no_device("slx_sort_create").c_str()));
    size_t free_b = 0, total_b = 0;
    SLX_HIPCHK(hipMemGetInfo(&free_b, &total_b));
    s->max_bytes = std::max<int64_t>((int64_t)(free_b / 2), 1);
    SLX_CHK(s->h_state.ensure(2 * sizeof(sort_state)));
    SLX_CHK(s->d_state.ensure(sizeof(sort_state)));
    return SLX_OK;
}

extern "C" int slx_sort_create(int device, slx_sort **out)
{
    if (!out) { slx_set_error("slx_sort_create: null argument"); return SLX_EINVAL; }
    return slx_create(out, slx_sort_free, [&](slx_sort *s) { return sort_init(s, device); });
}

static int sort_spill_run(slx_sort *s);

static int sort_add(slx_sort *s, const void *stream, int64_t n_bytes, const void *rec_off, int64_t n_records, bool from_device, const char *who)
{
    if (!s || n_bytes < 0 || n_records < 0 || (n_records && (!stream || !rec_off))) { slx_set_error("%s: null argument or negative size", who); return SLX_EINVAL; }
    if (n_records == 0) {
        if (n_bytes) { slx_set_error("%s: %lld bytes in 0 records", who, (long long)n_bytes); return SLX_EINVAL; }
        return SLX_OK;
    }
    if (s->spill_on && s->held_records && n_bytes <= s->max_bytes && s->held_bytes + (uint64_t)n_bytes > (uint64_t)s->max_bytes) SLX_CHK(sort_spill_run(s));
    if (s->held_bytes + (uint64_t)n_bytes > (uint64_t)s->max_bytes) {
        slx_set_error("%s: %llu bytes of records do not fit the sorter's max_bytes of %lld (without slx_sort_spill the sort is in HBM only, and one call's records are never split)", who,
                      (ull)(s->held_bytes + (uint64_t)n_bytes), (long long)s->max_bytes);
        return SLX_EUNSUPPORTED;
    }
    if (s->held_records + (uint64_t)n_records > 0xffffffffull) {
        slx_set_error("%s: %llu records: the sorter's ordinals are 32 bits", who, (ull)(s->held_records + (uint64_t)n_records));
        return SLX_EUNSUPPORTED;
    }
    SLX_HIPCHK(hipSetDevice(s->device));
    const size_t n = (size_t)n_records, nb = (size_t)n_bytes;
    const size_t o_off = up16(nb), o_key = o_off + up16(8 * (n + 1)), o_src = o_key + up16(8 * n), o_len = o_src + up16(8 * n), total = o_len + up16(4 * n);
    Segment g;
    if (hipMalloc((void **)&g.base, total) != hipSuccess) { (void)hipGetLastError(); slx_set_error("%s: cannot allocate a segment of %zu bytes of HBM", who, total); return SLX_ENOMEM; }
    g.n_bytes = nb; g.n = n;
    g.off = (uint64_t *)(g.base + o_off); g.key = (ull *)(g.base + o_key); g.src = (ull *)(g.base + o_src); g.len = (uint32_t *)(g.base + o_len);
    hipStream_t st = s->st;
    sort_state *const h_state = s->h_state.as<sort_state>();
    auto run = [&]() -> int {
        const hipMemcpyKind kind = from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        SLX_HIPCHK(hipMemcpyAsync(g.base, stream, nb, kind, st));
        SLX_HIPCHK(hipMemcpyAsync(g.off, rec_off, 8 * (n + 1), kind, st));
        h_state[0].bad = RS_NO_BAD; h_state[0].max_key = 0;
        SLX_HIPCHK(hipMemcpyAsync(s->d_state.p, &h_state[0], sizeof(sort_state), hipMemcpyHostToDevice, st));
        SLX_HIPCHK(hipEventRecord(s->ev[0], st));
        k_sort_key<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(g.base, nb, g.off, n, g.key, g.len, g.src, s->d_state.as<sort_state>());
        SLX_HIPCHK(hipGetLastError());
        SLX_HIPCHK(hipEventRecord(s->ev[1], st));
        SLX_HIPCHK(hipMemcpyAsync(&h_state[1], s->d_state.p, sizeof(sort_state), hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(slx_wait_stream(st));
        s->us_key += slx_ev_us(s->ev[0], s->ev[1]);
        if (h_state[1].bad != RS_NO_BAD) {
            slx_set_error("%s: record %llu of the call does not start where the block_size before it ends, or its offsets do not rise inside the %lld bytes, or (the last) its block_size does not end there; nothing of the call was added",
                          who, h_state[1].bad, (long long)n_bytes);
            return SLX_EINVAL;
        }
        return SLX_OK;
    };
    const int rc = run();
    if (rc != SLX_OK) { (void)hipStreamSynchronize(st); (void)hipFree(g.base); return rc; }
    s->segs.push_back(g);
    s->held_records += n; s->held_bytes += nb;
    s->max_key = std::max(s->max_key, h_state[1].max_key);
    s->c_records += (int64_t)n; s->c_bytes += (int64_t)nb; ++s->c_segments;
    return SLX_OK;
}

extern "C" int slx_sort_add_device(slx_sort *s, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records)
{
    return sort_add(s, d_stream, n_bytes, d_rec_off, n_records, true, "slx_sort_add_device");
}
extern "C" int slx_sort_add_host(slx_sort *s, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records)
{
    return sort_add(s, stream, n_bytes, rec_off, n_records, false, "slx_sort_add_host");
}

// the tables of the held records in sorted order: d_ord_out (input ordinals), d_ssrc (source addresses), d_doff (held_records + 1 offsets in the sorted stream)
static int sort_tables(slx_sort *s)
{
    const size_t N = (size_t)s->held_records;
    hipStream_t st = s->st;
    SLX_CHK(s->d_key_in.ensure(8 * N)); SLX_CHK(s->d_key_out.ensure(8 * N)); SLX_CHK(s->d_ord_in.ensure(4 * N)); SLX_CHK(s->d_ord_out.ensure(4 * N));
    SLX_CHK(s->d_len.ensure(4 * N)); SLX_CHK(s->d_src.ensure(8 * N)); SLX_CHK(s->d_slen.ensure(8 * (N + 1))); SLX_CHK(s->d_ssrc.ensure(8 * N)); SLX_CHK(s->d_doff.ensure(8 * (N + 1)));
    SLX_HIPCHK(hipEventRecord(s->ev[0], st));
    size_t at = 0;
    for (const Segment &g : s->segs) {          // the per-record tables of the segments side by side (the records themselves stay where they are)
        SLX_HIPCHK(hipMemcpyAsync(s->d_key_in.as<ull>() + at, g.key, 8 * g.n, hipMemcpyDeviceToDevice, st));
        SLX_HIPCHK(hipMemcpyAsync(s->d_src.as<ull>() + at, g.src, 8 * g.n, hipMemcpyDeviceToDevice, st));
        SLX_HIPCHK(hipMemcpyAsync(s->d_len.as<uint32_t>() + at, g.len, 4 * g.n, hipMemcpyDeviceToDevice, st));
        at += (size_t)g.n;
    }
    const unsigned grid = (unsigned)((N + 256) / 256);
    k_sort_iota<<<grid, 256, 0, st>>>(s->d_ord_in.as<uint32_t>(), N);
    SLX_HIPCHK(hipGetLastError());
    int end_bit = 1;          // the bits in use: the highest key of the adds is known
    while (end_bit < 64 && (s->max_key >> end_bit)) ++end_bit;
    size_t tb_sort = 0, tb_scan = 0;          // one block for both: the sum finds it large enough and allocates nothing
    SLX_HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, s->d_key_in.as<ull>(), s->d_key_out.as<ull>(), s->d_ord_in.as<uint32_t>(), s->d_ord_out.as<uint32_t>(), N, 0, end_bit, st));
    SLX_HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan, s->d_slen.as<ull>(), s->d_doff.as<ull>(), N + 1, st));
    SLX_CHK(s->d_tmp.ensure(std::max(tb_sort, tb_scan) + 8));
    SLX_HIPCHK(hipcub::DeviceRadixSort::SortPairs(s->d_tmp.p, tb_sort, s->d_key_in.as<ull>(), s->d_key_out.as<ull>(), s->d_ord_in.as<uint32_t>(), s->d_ord_out.as<uint32_t>(), N, 0, end_bit, st));
    k_sort_perm<<<grid, 256, 0, st>>>(s->d_ord_out.as<uint32_t>(), s->d_len.as<uint32_t>(), s->d_src.as<ull>(), N, s->d_slen.as<ull>(), s->d_ssrc.as<ull>());
    SLX_HIPCHK(hipGetLastError());
    SLX_CHK(slx_exclusive_sum(s->d_tmp, s->d_slen.as<ull>(), s->d_doff.as<ull>(), N + 1, st, 8));
    SLX_HIPCHK(hipEventRecord(s->ev[1], st));
    SLX_HIPCHK(slx_wait_stream(st));
    s->us_sort += slx_ev_us(s->ev[0], s->ev[1]);
    return SLX_OK;
}

// tiles [tile0, tile_end) of the sorted stream into out (the slab: its first byte is the stream's byte tile0 * RS_TILE); returns when they are there
static int sort_gather(slx_sort *s, uint64_t tile0, uint64_t tile_end, uint8_t *out)
{
    hipStream_t st = s->st;
    const uint64_t grid = (tile_end - tile0 + 3) / 4;
    if (grid > 0x7fffffffull) { slx_set_error("sorter: %llu tiles in one gather are more than a grid holds", (ull)(tile_end - tile0)); return SLX_EUNSUPPORTED; }
    SLX_HIPCHK(hipSetDevice(s->device));          // (the writer selects its own device in every call between two gathers)
    SLX_HIPCHK(hipEventRecord(s->ev[0], st));
    k_sort_gather<<<(unsigned)grid, 256, 0, st>>>(s->d_doff.as<ull>(), s->d_ssrc.as<ull>(), (int64_t)s->held_records, s->held_bytes, tile0, tile_end, out);
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(s->ev[1], st));
    SLX_HIPCHK(slx_wait_stream(st));
    s->us_gather += slx_ev_us(s->ev[0], s->ev[1]);
    return SLX_OK;
}

static int sort_finish_impl(slx_sort *s, slx_bgzf *w)
{
    if (s->held_records == 0) return SLX_OK;
    SLX_HIPCHK(hipSetDevice(s->device));
    SLX_CHK(sort_tables(s));
    const uint64_t B = s->held_bytes, n_tiles = (B + RS_TILE - 1) / RS_TILE, slab_tiles = (uint64_t)s->slab_bytes / RS_TILE;
    SLX_CHK(s->d_slab.ensure((size_t)std::min<uint64_t>(n_tiles, slab_tiles) * RS_TILE));
    for (uint64_t t = 0; t < n_tiles; t += slab_tiles) {
        const uint64_t te = std::min(n_tiles, t + slab_tiles), bytes = std::min(B, te * RS_TILE) - t * RS_TILE;
        SLX_CHK(sort_gather(s, t, te, s->d_slab.as<uint8_t>()));
        SLX_CHK(slx_bgzf_write_device(w, s->d_slab.p, (int64_t)bytes));          // staged when it returns: the slab is free for the next range of tiles
        ++s->c_slabs;
    }
    return SLX_OK;
}

// The held records, sorted, as the next run file: the header block in a member of its own, the records, the EOF block.  Empties the sorter.  On an error the
// run files written so far go too, and nothing is held.
static int sort_spill_run(slx_sort *s)
{
    auto run = [&]() -> int {
        if (s->runs.size() >= SORT_MAX_RUNS) {
            slx_set_error("slx_sort: run %zu would be written: more than %zu runs cannot be merged in one pass (raise max_bytes)", s->runs.size() + 1, SORT_MAX_RUNS);
            return SLX_EUNSUPPORTED;
        }
        char num[32];
        snprintf(num, sizeof num, ".run%04d.bam", (int)s->runs.size());
        const std::string path = s->spill_prefix + num;
        slx_bgzf *w = nullptr;
        SLX_CHK(slx_bgzf_open(path.c_str(), s->device, &w));
        s->runs.push_back(path);
        int rc = slx_bgzf_write(w, s->spill_header.data(), (int64_t)s->spill_header.size());
        if (rc == SLX_OK) rc = slx_bgzf_flush(w);
        const int64_t bytes = (int64_t)s->held_bytes;
        if (rc == SLX_OK) rc = sort_finish_impl(s, w);
        const std::string msg = rc != SLX_OK ? slx_last_error() : "";
        const int rc2 = slx_bgzf_close(w);
        if (rc != SLX_OK) { slx_set_error("%s", msg.c_str()); return rc; }
        SLX_CHK(rc2);
        ++s->c_runs; s->c_run_bytes += bytes;
        return SLX_OK;
    };
    const int rc = run();
    const std::string msg = rc != SLX_OK ? slx_last_error() : "";
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->st);
    sort_clear(s);
    if (rc != SLX_OK) { sort_drop_runs(s); slx_set_error("%s", msg.c_str()); }
    return rc;
}

// the run files merged into w; they are removed whatever happens
static int sort_merge_runs(slx_sort *s, slx_bgzf *w)
{
    const auto t0 = std::chrono::steady_clock::now();
    slx_merge *m = nullptr;
    int rc = slx_merge_create(s->device, &m);
    if (rc == SLX_OK) rc = slx_merge_set(m, "slab_bytes", s->slab_bytes);
    if (rc == SLX_OK) rc = slx_merge_set(m, "batch_bytes", std::max<int64_t>(1, std::min<int64_t>(s->batch_bytes, s->max_bytes / (int64_t)std::max<size_t>(s->runs.size(), 1))));
    for (size_t i = 0; rc == SLX_OK && i < s->runs.size(); ++i) rc = slx_merge_add_file(m, s->runs[i].c_str());
    if (rc == SLX_OK) rc = slx_merge_run(m, w);
    const std::string msg = rc != SLX_OK ? slx_last_error() : "";
    if (m) slx_merge_free(m);
    sort_drop_runs(s);
    s->us_merge += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (rc != SLX_OK) slx_set_error("%s", msg.c_str());
    return rc;
}

extern "C" int slx_sort_spill(slx_sort *s, const char *prefix, const void *bam_header, int64_t l_header)
{
    if (!s || (prefix && (!bam_header || l_header < 12))) { slx_set_error("slx_sort_spill: null argument, or a header block that cannot be one"); return SLX_EINVAL; }
    if (!s->runs.empty()) { slx_set_error("slx_sort_spill: %zu runs are pending; slx_sort_finish first", s->runs.size()); return SLX_EINVAL; }
    s->spill_on = prefix != nullptr;
    s->spill_prefix = prefix ? prefix : "";
    s->spill_header = prefix ? std::string((const char *)bam_header, (size_t)l_header) : std::string();
    return SLX_OK;
}

extern "C" int slx_sort_finish(slx_sort *s, slx_bgzf *w)
{
    if (!s || !w) { slx_set_error("slx_sort_finish: null argument"); return SLX_EINVAL; }
    if (!s->runs.empty()) {          // the sort went beyond HBM: what is still held is the last run, and the runs are merged
        int rc = slx_bgzf_write_device(w, nullptr, 0), wdev = -1;
        if (rc == SLX_OK && (hipGetDevice(&wdev) != hipSuccess || wdev != s->device)) {
            slx_set_error("slx_sort_finish: the writer is on device %d, the sorter on device %d: both must be on one", wdev, s->device);
            rc = SLX_EINVAL;
        }
        if (rc == SLX_OK && s->held_records) rc = sort_spill_run(s);
        if (rc == SLX_OK) return sort_merge_runs(s, w);
        const std::string msg = slx_last_error();
        (void)hipSetDevice(s->device);
        (void)hipStreamSynchronize(s->st);
        sort_clear(s);
        sort_drop_runs(s);
        slx_set_error("%s", msg.c_str());
        return rc;
    }
    // the writer takes the slabs by a device-to-device copy inside its own device: an empty write makes it select that device, which must be the sorter's
    int rc = slx_bgzf_write_device(w, nullptr, 0), wdev = -1;
    if (rc == SLX_OK && (hipGetDevice(&wdev) != hipSuccess || wdev != s->device)) {
        slx_set_error("slx_sort_finish: the writer is on device %d, the sorter on device %d: both must be on one", wdev, s->device);
        rc = SLX_EINVAL;
    }
    if (rc == SLX_OK) rc = sort_finish_impl(s, w);
    const std::string msg = rc != SLX_OK ? slx_last_error() : "";
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->st);
    sort_clear(s);
    if (rc != SLX_OK) slx_set_error("%s", msg.c_str());
    return rc;
}

extern "C" int slx_sort_to_host(slx_sort *s, void *dst, uint64_t cap, uint64_t *rec_off_dst, uint32_t *perm_dst)
{
    if (!s) { slx_set_error("slx_sort_to_host: null argument"); return SLX_EINVAL; }
    if (!s->runs.empty()) { slx_set_error("slx_sort_to_host: %zu runs were spilled to disk: only slx_sort_finish brings them together", s->runs.size()); return SLX_EUNSUPPORTED; }
    const uint64_t B = s->held_bytes, N = s->held_records;
    if (B > cap || (B && !dst)) { slx_set_error("slx_sort_to_host: %llu bytes do not fit the %llu given", (ull)B, (ull)cap); return SLX_EINVAL; }
    if (N == 0) { if (rec_off_dst) rec_off_dst[0] = 0; return SLX_OK; }
    SLX_HIPCHK(hipSetDevice(s->device));
    auto run = [&]() -> int {
        SLX_CHK(sort_tables(s));
        const uint64_t n_tiles = (B + RS_TILE - 1) / RS_TILE;
        SLX_CHK(s->d_slab.ensure((size_t)n_tiles * RS_TILE));
        SLX_CHK(sort_gather(s, 0, n_tiles, s->d_slab.as<uint8_t>()));
        ++s->c_slabs;
        SLX_HIPCHK(hipMemcpyAsync(dst, s->d_slab.p, B, hipMemcpyDeviceToHost, s->st));
        if (rec_off_dst) SLX_HIPCHK(hipMemcpyAsync(rec_off_dst, s->d_doff.p, 8 * (N + 1), hipMemcpyDeviceToHost, s->st));
        if (perm_dst) SLX_HIPCHK(hipMemcpyAsync(perm_dst, s->d_ord_out.p, 4 * N, hipMemcpyDeviceToHost, s->st));
        SLX_HIPCHK(hipStreamSynchronize(s->st));
        return SLX_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(s->st);
    s->d_slab.release();          // (sized by the whole stream here, by one slab in slx_sort_finish)
    sort_clear(s);
    return rc;
}

extern "C" int64_t slx_sort_header(const char *text, int64_t l_text, char *dst, int64_t cap)
{
    if (!text || l_text < 0) { slx_set_error("slx_sort_header: null text or negative length"); return SLX_EINVAL; }
    const std::string out = recsort_header_so(std::string(text, (size_t)l_text));
    if (dst && cap >= (int64_t)out.size()) memcpy(dst, out.data(), out.size());
    return (int64_t)out.size();
}

// the header block of the sorted file: SO:coordinate by the rule, the reader's references
static std::string sort_header_block(slx_bam *rd)
{
    const char *text = nullptr; int64_t l_text = 0; int n_ref = 0;
    if (slx_bam_header(rd, &text, &l_text, &n_ref) != SLX_OK) return std::string();
    const std::string so = recsort_header_so(std::string(text, (size_t)l_text));
    std::string h("BAM\1", 4);
    sort_put32(h, (uint32_t)so.size());
    h += so;
    sort_put32(h, (uint32_t)n_ref);
    for (int i = 0; i < n_ref; ++i) {
        const std::string nm = slx_bam_ref_name(rd, i);
        sort_put32(h, (uint32_t)nm.size() + 1);
        h += nm; h.push_back('\0');
        sort_put32(h, (uint32_t)slx_bam_ref_len(rd, i));
    }
    return h;
}

static int sort_file_impl(slx_sort *s, slx_bam *rd, const char *out_path, bool *created, const char *spill_prefix)
{
    if (spill_prefix) {
        const std::string h = sort_header_block(rd);
        SLX_CHK(slx_sort_spill(s, spill_prefix, h.data(), (int64_t)h.size()));
    }
    for (;;) {
        slx_bam_batch b;
        SLX_CHK(slx_bam_next(rd, s->batch_bytes, &b));
        if (b.n_records == 0) break;
        SLX_CHK(slx_sort_add_device(s, b.d_stream, b.n_bytes, b.d_rec_off, b.n_records));
    }
    const std::string h = sort_header_block(rd);
    slx_bgzf *w = nullptr;
    SLX_CHK(slx_bgzf_open(out_path, s->device, &w));
    *created = true;
    int rc = slx_bgzf_write(w, h.data(), (int64_t)h.size());
    if (rc == SLX_OK) rc = slx_bgzf_flush(w);          // the records start in a member of their own, as BamWriter::WriteHeader leaves them
    if (rc == SLX_OK) rc = slx_sort_finish(s, w);
    std::string msg = rc != SLX_OK ? slx_last_error() : "";
    const int rc2 = slx_bgzf_close(w);
    if (rc != SLX_OK) { slx_set_error("%s", msg.c_str()); return rc; }
    return rc2;
}

static int sort_file_with(slx_sort *s, const char *in_path, const char *out_path, const char *spill_prefix)
{
    if (!s || !in_path || !out_path) { slx_set_error("slx_sort_file: null argument"); return SLX_EINVAL; }
    if (!strcmp(in_path, out_path) || !strcmp(in_path, "-") || !strcmp(out_path, "-")) {
        slx_set_error("slx_sort_file: '%s' -> '%s': the output must be another file than the input, and neither is a pipe", in_path, out_path);
        return SLX_EINVAL;
    }
    if (s->held_records || !s->runs.empty()) { slx_set_error("slx_sort_file_ex: the sorter holds %llu records and %zu runs; it must be empty", (ull)s->held_records, s->runs.size()); return SLX_EINVAL; }
    SLX_HIPCHK(hipSetDevice(s->device));
    slx_bam *rd = nullptr;
    SLX_CHK(slx_bam_open(in_path, s->device, &rd));
    bool created = false;
    const int rc = sort_file_impl(s, rd, out_path, &created, spill_prefix);
    std::string msg = rc != SLX_OK ? slx_last_error() : "";
    slx_bam_close(rd);
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->st);
    sort_clear(s);
    sort_drop_runs(s);          // (none are left after a finish; an error on the way leaves none either)
    if (spill_prefix) { s->spill_on = false; s->spill_prefix.clear(); s->spill_header.clear(); }
    if (rc != SLX_OK) {
        if (created) (void)unlink(out_path);          // no output file is left behind
        slx_set_error("%s", msg.c_str());
    }
    return rc;
}

extern "C" int slx_sort_file_ex(slx_sort *s, const char *in_path, const char *out_path) { return sort_file_with(s, in_path, out_path, nullptr); }

extern "C" int slx_sort_file_spill(slx_sort *s, const char *in_path, const char *out_path, const char *prefix)
{
    if (!s || !in_path || !out_path) { slx_set_error("slx_sort_file_spill: null argument"); return SLX_EINVAL; }
    return sort_file_with(s, in_path, out_path, prefix ? prefix : out_path);
}

extern "C" int slx_sort_file(const char *in_path, const char *out_path, int device)
{
    if (!in_path || !out_path) { slx_set_error("slx_sort_file: null argument"); return SLX_EINVAL; }
    if (!strcmp(in_path, out_path) || !strcmp(in_path, "-") || !strcmp(out_path, "-")) {
        slx_set_error("slx_sort_file: '%s' -> '%s': the output must be another file than the input, and neither is a pipe", in_path, out_path);
        return SLX_EINVAL;
    }
    int ndev = 0;
    SLX_CHK(slx_count_devices(sort_no_device("slx_sort_file").c_str(), &ndev));
    slx_sort *s = nullptr;
    SLX_CHK(slx_sort_create(device, &s));
    const int rc = slx_sort_file_ex(s, in_path, out_path);
    std::string msg = rc != SLX_OK ? slx_last_error() : "";
    slx_sort_free(s);
    if (rc != SLX_OK) slx_set_error("%s", msg.c_str());
    return rc;
}

extern "C" int slx_sort_set(slx_sort *s, const char *key, int64_t value)
{
    if (!s || !key) { slx_set_error("slx_sort_set: null argument"); return SLX_EINVAL; }
    if (!strcmp(key, "max_bytes") && value >= 1) { s->max_bytes = value; return SLX_OK; }
    if (!strcmp(key, "slab_bytes") && value >= (int64_t)RS_TILE && value <= SORT_MAX_SLAB && value % (int64_t)RS_TILE == 0) { s->slab_bytes = value; return SLX_OK; }
    if (!strcmp(key, "batch_bytes") && value >= 1) { s->batch_bytes = value; return SLX_OK; }
    slx_set_error("slx_sort_set: unknown key or value out of range: %s = %lld (slab_bytes is a multiple of the %u-byte tile, at least one, at most %lld bytes)", key, (long long)value, RS_TILE, (long long)SORT_MAX_SLAB);
    return SLX_EINVAL;
}

extern "C" int64_t slx_sort_counter(const slx_sort *s, const char *name)
{
    if (!s || !name) return -1;
    if (!strcmp(name, "records")) return s->c_records;
    if (!strcmp(name, "bytes")) return s->c_bytes;
    if (!strcmp(name, "segments")) return s->c_segments;
    if (!strcmp(name, "slabs")) return s->c_slabs;
    if (!strcmp(name, "us_key")) return (int64_t)s->us_key;
    if (!strcmp(name, "us_sort")) return (int64_t)s->us_sort;
    if (!strcmp(name, "us_gather")) return (int64_t)s->us_gather;
    if (!strcmp(name, "held_records")) return (int64_t)s->held_records;
    if (!strcmp(name, "held_bytes")) return (int64_t)s->held_bytes;
    if (!strcmp(name, "runs")) return s->c_runs;
    if (!strcmp(name, "run_bytes")) return s->c_run_bytes;
    if (!strcmp(name, "us_merge")) return (int64_t)s->us_merge;
    return -1;
}

// The duplicate marker's route through the sorter (include/seqlib_amd_dup.h): it lives here because the segments are this unit's.  The order key does not read
// the flag, so the sort is what it would have been.
extern "C" int slx_dup_mark_sorter(slx_dup *d, slx_sort *s)
{
    if (!d || !s) { slx_set_error("slx_dup_mark_sorter: null argument"); return SLX_EINVAL; }
    if (!s->runs.empty()) {
        slx_set_error("slx_dup_mark_sorter: %zu runs were spilled to disk and the marker works among held records only; slx_dup_file is the route for files beyond HBM", s->runs.size());
        return SLX_EUNSUPPORTED;
    }
    if (slx_dup_counter(d, "device") != s->device) {
        slx_set_error("slx_dup_mark_sorter: the marker is on device %lld, the sorter on device %d: both must be on one", (long long)slx_dup_counter(d, "device"), s->device);
        return SLX_EINVAL;
    }
    if (slx_dup_counter(d, "records") != 0 || slx_dup_counter(d, "finished") != 0) { slx_set_error("slx_dup_mark_sorter: the marker is not empty (slx_dup_clear first)"); return SLX_EINVAL; }
    SLX_HIPCHK(hipSetDevice(s->device));
    SLX_HIPCHK(hipStreamSynchronize(s->st));
    for (const Segment &g : s->segs) SLX_CHK(slx_dup_add_device(d, g.base, (int64_t)g.n_bytes, g.off, (int64_t)g.n));
    SLX_CHK(slx_dup_finish(d));
    int64_t first = 0;
    for (const Segment &g : s->segs) {
        SLX_CHK(slx_dup_apply_device(d, g.base, (int64_t)g.n_bytes, g.off, (int64_t)g.n, first, nullptr));
        first += (int64_t)g.n;
    }
    return SLX_OK;
}
