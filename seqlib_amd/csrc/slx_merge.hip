// slx_merge.hip -- the k-way merge of coordinate-sorted BAM files of libseqlib_amd.so (include/seqlib_amd_merge.h, slx_merge_*): the inputs are read by the GPU
// reader batch by batch into windows in HBM, a round's eligible records are ranked where they lie and gathered into the merged stream.  The bodies are
// dev_merge.h's and dev_recsort.h's, the planner and the header rule merge_host.h's; the reader and the writer are used through their C-ABI only.
//   k_merge_key       one lane per record of a batch: rs_key's checks, key, length, source address, the order test against the predecessor; the first broken and the
//                     first unsorted ordinal (one atomic per wave) and the last key come down
//   k_merge_elig      one wave per input: how many of its window's keys lie below the round's bound (cooperative lower bound)
//   k_merge_rank      one lane per eligible record: its rank in the round's output (wave-bracketed searches in the other inputs' keys; beg / ebeg in LDS)
//   hipCUB            by_sort = 1 instead: DeviceRadixSort::SortPairs (stable) over the eligible keys side by side, k_merge_unperm turns the order into ranks
//   k_merge_place     lengths, source addresses and input indices to their ranks
//   hipCUB            exclusive sum of the lengths = dst_off
//   k_merge_gather    rs_gather_tile per RS_TILE bytes of the output, as k_sort_gather
// Records map to lanes and tiles to waves statically: no work queue.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>
#include <unistd.h>
#include "slx_internal.h"
#include "seqlib_amd_merge.h"
#include "dev_lanes.h"
#include "dev_wave.h"
#include "dev_merge.h"
#include "merge_host.h"
#include "slx_hip.h"

typedef unsigned long long ull;
static const int64_t MERGE_MAX_SLAB = 1ll << 40;

struct merge_state { ull bad, unsorted, last_key; };          // ordinals inside the batch, RS_NO_BAD = none

// ------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void k_merge_key(const uint8_t *stream, uint64_t n_bytes, const uint64_t *off, uint64_t n, int has_prev, ull prev_last, ull *key, uint32_t *len, ull *src,
                                                   merge_state *st)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    ull bad = RS_NO_BAD, uns = RS_NO_BAD;
    if (i < n) {
        uint64_t kk = 0; uint32_t l = 0; bool u = false;
        if (mg_key(stream, n_bytes, off, i, n, has_prev != 0, prev_last, &kk, &l, &u)) {
            key[i] = kk; len[i] = l; src[i] = (ull)(uintptr_t)(stream + off[i]);
            if (u) uns = i;
            if (i + 1 == n) st->last_key = kk;
        } else { bad = i; key[i] = 0; len[i] = 0; src[i] = 0; }
    }
    bad = wave_min(bad); uns = wave_min(uns);          // (both before either atomic: the two chains of shuffles run side by side)
    if ((threadIdx.x & 63) == 0) {
        if (bad != RS_NO_BAD) atomicMin(&st->bad, bad);
        if (uns != RS_NO_BAD) atomicMin(&st->unsorted, uns);
    }
}

__global__ __launch_bounds__(64) void k_merge_elig(const ull *keys, const uint32_t *beg, int finite, ull bound, uint32_t *elig)
{
    const uint32_t i = blockIdx.x, b = beg[i], e = beg[i + 1];
    const uint32_t c = mg_elig(keys + b, (uint64_t)(e - b), finite != 0, bound, (int)threadIdx.x, 64);
    if (threadIdx.x == 0) elig[i] = c;
}

__global__ __launch_bounds__(256) void k_merge_rank(const ull *keys, const uint32_t *beg, const uint32_t *ebeg, int k, uint32_t *rank)
{
    __shared__ uint32_t s_beg[MG_MAX_IN + 1], s_ebeg[MG_MAX_IN + 1];
    if ((int)threadIdx.x <= k) { s_beg[threadIdx.x] = beg[threadIdx.x]; s_ebeg[threadIdx.x] = ebeg[threadIdx.x]; }
    __syncthreads();
    const uint64_t g0 = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u);          // (a whole wave goes on or returns: the counts of mg_coop_bound see all 64 lanes)
    mg_rank_wave(keys, (const MG_LDS uint32_t *)s_beg, (const MG_LDS uint32_t *)s_ebeg, k, g0, rank, (int)(threadIdx.x & 63), 64);
}

__global__ __launch_bounds__(256) void k_merge_place(const uint32_t *beg, const uint32_t *ebeg, int k, const uint32_t *rank, const uint32_t *len, const ull *src, ull *slen, ull *ssrc,
                                                     uint8_t *input)
{
    __shared__ uint32_t s_beg[MG_MAX_IN + 1], s_ebeg[MG_MAX_IN + 1];
    if ((int)threadIdx.x <= k) { s_beg[threadIdx.x] = beg[threadIdx.x]; s_ebeg[threadIdx.x] = ebeg[threadIdx.x]; }
    __syncthreads();
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x, E = s_ebeg[k];
    if (g == E) slen[E] = 0;
    if (g < E) mg_place((const MG_LDS uint32_t *)s_beg, (const MG_LDS uint32_t *)s_ebeg, k, g, rank, len, src, slen, ssrc, input);
}

__global__ __launch_bounds__(256) void k_merge_iota(uint32_t *ord, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) ord[i] = (uint32_t)i;
}

// the sorted order (ord[p] = the eligible record that goes to place p) as ranks
__global__ __launch_bounds__(256) void k_merge_unperm(const uint32_t *ord, uint64_t n, uint32_t *rank)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) rank[ord[p]] = (uint32_t)p;
}

__global__ __launch_bounds__(256) void k_merge_gather(const ull *dst_off, const ull *ssrc, int64_t n, uint64_t n_bytes, uint64_t tile0, uint64_t tile_end, uint8_t *out)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[4][RS_TILE];
    __shared__ rs_desc desc[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t t = tile0 + (uint64_t)blockIdx.x * 4 + wave;
    if (t >= tile_end) return;          // (a whole wave)
    rs_gather_tile(dst_off, ssrc, n, n_bytes, t, tile[wave], &desc[wave], out, tile0 * RS_TILE, (int)lane, 64);
}

// ------------------------------------------------------------------ host
namespace {
typedef SlxDevBuf<SlxExact> MBuf;
typedef SlxPinBuf<SlxExact> MHBuf;

// one batch of one input: the bytes and, behind them in the same allocation, the offsets and the three per-record tables (the sorter's segment)
struct Seg {
    uint8_t *base = nullptr;
    uint64_t n_bytes = 0, n = 0;
    uint64_t *off = nullptr; ull *key = nullptr, *src = nullptr; uint32_t *len = nullptr;
};
struct Input {
    std::string path;
    slx_bam *rd = nullptr;
    std::deque<Seg> segs;          // the window: the records of segs.front() from `consumed` on, then the other segments whole
    uint64_t consumed = 0;
    bool has_last = false;         // a batch was read: last_read is the key of the last record read (the window may be empty)
    ull last_read = 0;
    uint64_t n_read = 0;           // records read so far: a batch's ordinals count from here
};
static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
static void put32(std::string &o, uint32_t v) { const char b[4] = {(char)v, (char)(v >> 8), (char)(v >> 16), (char)(v >> 24)}; o.append(b, 4); }
}  // namespace

struct slx_merge : SlxGpu<> {
    std::vector<Input> in;
    std::vector<merge_in> mi;          // the planner's view of the inputs
    std::string header;                // the header block of the output
    bool started = false, had_bound = false;
    ull prev_bound = 0;
    uint64_t held_bytes = 0;
    int64_t max_bytes = 0, slab_bytes = 64ll << 20, batch_bytes = 64ll << 20, by_sort = 0;
    // the round in flight
    std::vector<uint32_t> elig;
    uint64_t E = 0, round_bytes = 0;
    MBuf d_state{*this}, d_key{*this}, d_src{*this}, d_len{*this}, d_beg{*this}, d_ebeg{*this}, d_elig{*this}, d_rank{*this}, d_slen{*this}, d_ssrc{*this}, d_doff{*this}, d_input{*this},
         d_tmp{*this}, d_out{*this}, d_slab{*this}, d_ekey{*this}, d_ekey_out{*this}, d_ord_in{*this}, d_ord_out{*this};
    MHBuf h_state{*this}, h_tab{*this};          // merge_state up and down; beg / ebeg / elig and the round's byte count
    int64_t c_records = 0, c_bytes = 0, c_rounds = 0, c_refills = 0;
    double us_key = 0, us_rank = 0, us_gather = 0;
};

static void merge_drop_windows(slx_merge *m)
{
    for (Input &x : m->in) {
        for (Seg &g : x.segs) if (g.base) (void)hipFree(g.base);
        x.segs.clear(); x.consumed = 0;
    }
    for (merge_in &x : m->mi) x.held = 0;
    m->held_bytes = 0; m->E = 0;
}

extern "C" void slx_merge_free(slx_merge *m)
{
    if (!m) return;
    if (m->st) { (void)hipSetDevice(m->device); (void)hipStreamSynchronize(m->st); }
    merge_drop_windows(m);
    for (Input &x : m->in) if (x.rd) slx_bam_close(x.rd);
    m->close();
    delete m;
}

static std::string merge_no_device(const char *who) { return std::string(who) + ": no HIP device: BAM files are merged on MI355X only (no CPU fallback)"; }

static int merge_init(slx_merge *m, int device)
{
    SLX_CHK(m->open(device, "slx_merge_create", merge_no_device("slx_merge_create").c_str()));
    size_t free_b = 0, total_b = 0;
    SLX_HIPCHK(hipMemGetInfo(&free_b, &total_b));
    m->max_bytes = std::max<int64_t>((int64_t)(free_b / 2), 1);
    SLX_CHK(m->h_state.ensure(2 * sizeof(merge_state)));
    SLX_CHK(m->d_state.ensure(sizeof(merge_state)));
    SLX_CHK(m->h_tab.ensure(4 * 3 * (MG_MAX_IN + 1) + 16));
    SLX_CHK(m->d_beg.ensure(4 * (MG_MAX_IN + 1))); SLX_CHK(m->d_ebeg.ensure(4 * (MG_MAX_IN + 1))); SLX_CHK(m->d_elig.ensure(4 * (MG_MAX_IN + 1)));
    return SLX_OK;
}

extern "C" int slx_merge_create(int device, slx_merge **out)
{
    if (!out) { slx_set_error("slx_merge_create: null argument"); return SLX_EINVAL; }
    return slx_create(out, slx_merge_free, [&](slx_merge *m) { return merge_init(m, device); });
}

// the header block of the inputs so far with one more text; SLX_OK = *block is it
static int merge_header_block(const slx_merge *m, slx_bam *extra, const char *extra_path, std::string *block)
{
    std::vector<std::string> texts;
    std::vector<slx_bam *> rds;
    for (const Input &x : m->in) rds.push_back(x.rd);
    if (extra) rds.push_back(extra);
    int n_ref0 = 0;
    for (size_t i = 0; i < rds.size(); ++i) {
        const char *text = nullptr; int64_t l_text = 0; int n_ref = 0;
        SLX_CHK(slx_bam_header(rds[i], &text, &l_text, &n_ref));
        texts.push_back(std::string(text, (size_t)l_text));
        if (i == 0) { n_ref0 = n_ref; continue; }
        if (i + 1 < rds.size() || !extra) continue;          // (the inputs already added were held against input 0 when they came)
        for (int r = 0; r < std::max(n_ref, n_ref0); ++r) {
            if (r < n_ref && r < n_ref0 && !strcmp(slx_bam_ref_name(rds[0], r), slx_bam_ref_name(extra, r)) && slx_bam_ref_len(rds[0], r) == slx_bam_ref_len(extra, r)) continue;
            slx_set_error("slx_merge_add_file: input %zu ('%s') differs from input 0 at reference %d (%d references against %d): every input must have the same references, in the same order",
                          i, extra_path, r, n_ref, n_ref0);
            return SLX_EINVAL;
        }
    }
    std::string text, what;
    if (merge_header_rule(texts, &text, &what) != 0) {
        slx_set_error("slx_merge_add_file: '%s' has an %s that a different line already present carries; it would have to be renamed and the records edited, and records are never edited here",
                      extra_path ? extra_path : "", what.c_str());
        return SLX_EUNSUPPORTED;
    }
    std::string h("BAM\1", 4);
    put32(h, (uint32_t)text.size());
    h += text;
    put32(h, (uint32_t)n_ref0);
    for (int r = 0; r < n_ref0; ++r) {
        const std::string nm = slx_bam_ref_name(rds[0], r);
        put32(h, (uint32_t)nm.size() + 1);
        h += nm; h.push_back('\0');
        put32(h, (uint32_t)slx_bam_ref_len(rds[0], r));
    }
    block->swap(h);
    return SLX_OK;
}

extern "C" int slx_merge_add_file(slx_merge *m, const char *path)
{
    if (!m || !path) { slx_set_error("slx_merge_add_file: null argument"); return SLX_EINVAL; }
    if (!strcmp(path, "-")) { slx_set_error("slx_merge_add_file: '-': an input is a file, not a pipe"); return SLX_EINVAL; }
    if (m->started) { slx_set_error("slx_merge_add_file: '%s': the merge has begun; inputs are added before the first round", path); return SLX_EINVAL; }
    if (m->in.size() >= MG_MAX_IN) {
        slx_set_error("slx_merge_add_file: '%s' would be input %zu: at most %d inputs are merged in one pass (there is no multi-pass merge)", path, m->in.size() + 1, MG_MAX_IN);
        return SLX_EUNSUPPORTED;
    }
    SLX_HIPCHK(hipSetDevice(m->device));
    slx_bam *rd = nullptr;
    SLX_CHK(slx_bam_open(path, m->device, &rd));
    std::string block;
    const int rc = merge_header_block(m, rd, path, &block);
    if (rc != SLX_OK) {
        const std::string msg = slx_last_error();
        slx_bam_close(rd);
        slx_set_error("%s", msg.c_str());
        return rc;
    }
    Input x;
    x.path = path; x.rd = rd;
    m->in.push_back(x);
    m->mi.push_back(merge_in());
    m->header.swap(block);
    return SLX_OK;
}

extern "C" int slx_merge_header(const slx_merge *m, const char **bam_header, int64_t *l_header)
{
    if (!m || !bam_header || !l_header) { slx_set_error("slx_merge_header: null argument"); return SLX_EINVAL; }
    if (m->in.empty()) { slx_set_error("slx_merge_header: no input was added"); return SLX_EINVAL; }
    *bam_header = m->header.data(); *l_header = (int64_t)m->header.size();
    return SLX_OK;
}

extern "C" int64_t slx_merge_header_text(const char *const *texts, const int64_t *l_texts, int n, char *dst, int64_t cap)
{
    if (n < 0 || (n && (!texts || !l_texts))) { slx_set_error("slx_merge_header_text: null argument or negative count"); return SLX_EINVAL; }
    std::vector<std::string> v;
    for (int i = 0; i < n; ++i) {
        if (!texts[i] || l_texts[i] < 0) { slx_set_error("slx_merge_header_text: text %d is null or has a negative length", i); return SLX_EINVAL; }
        v.push_back(std::string(texts[i], (size_t)l_texts[i]));
    }
    std::string out, what;
    if (merge_header_rule(v, &out, &what) != 0) {
        slx_set_error("slx_merge_header_text: an %s that a different line already present carries; it would have to be renamed and the records edited, and records are never edited here", what.c_str());
        return SLX_EUNSUPPORTED;
    }
    if (dst && cap >= (int64_t)out.size()) memcpy(dst, out.data(), out.size());
    return (int64_t)out.size();
}

// the next batch of input i into its window
static int merge_refill(slx_merge *m, int i)
{
    Input &x = m->in[(size_t)i];
    slx_bam_batch b;
    SLX_CHK(slx_bam_next(x.rd, m->batch_bytes, &b));
    ++m->c_refills;
    if (b.n_records == 0) { m->mi[(size_t)i].at_end = true; return SLX_OK; }
    SLX_HIPCHK(hipSetDevice(m->device));
    const size_t n = (size_t)b.n_records, nb = (size_t)b.n_bytes;
    const size_t o_off = up16(nb), o_key = o_off + up16(8 * (n + 1)), o_src = o_key + up16(8 * n), o_len = o_src + up16(8 * n), total = o_len + up16(4 * n);
    Seg g;
    if (hipMalloc((void **)&g.base, total) != hipSuccess) { (void)hipGetLastError(); slx_set_error("slx_merge: cannot allocate a window segment of %zu bytes of HBM", total); return SLX_ENOMEM; }
    g.n_bytes = nb; g.n = n;
    g.off = (uint64_t *)(g.base + o_off); g.key = (ull *)(g.base + o_key); g.src = (ull *)(g.base + o_src); g.len = (uint32_t *)(g.base + o_len);
    hipStream_t st = m->st;
    merge_state *const h = m->h_state.as<merge_state>();
    auto run = [&]() -> int {
        SLX_HIPCHK(hipMemcpyAsync(g.base, b.d_stream, nb, hipMemcpyDeviceToDevice, st));
        SLX_HIPCHK(hipMemcpyAsync(g.off, b.d_rec_off, 8 * (n + 1), hipMemcpyDeviceToDevice, st));
        h[0].bad = RS_NO_BAD; h[0].unsorted = RS_NO_BAD; h[0].last_key = 0;
        SLX_HIPCHK(hipMemcpyAsync(m->d_state.p, &h[0], sizeof(merge_state), hipMemcpyHostToDevice, st));
        SLX_HIPCHK(hipEventRecord(m->ev[0], st));
        k_merge_key<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(g.base, nb, g.off, n, x.has_last ? 1 : 0, x.last_read, g.key, g.len, g.src, m->d_state.as<merge_state>());
        SLX_HIPCHK(hipGetLastError());
        SLX_HIPCHK(hipEventRecord(m->ev[1], st));
        SLX_HIPCHK(hipMemcpyAsync(&h[1], m->d_state.p, sizeof(merge_state), hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(slx_wait_stream(st));
        m->us_key += slx_ev_us(m->ev[0], m->ev[1]);
        if (h[1].bad != RS_NO_BAD) {
            slx_set_error("slx_merge: '%s': record %llu of the file does not start where the block_size before it ends, or cannot hold a record", x.path.c_str(), (ull)(x.n_read + h[1].bad));
            return SLX_EINVAL;
        }
        if (h[1].unsorted != RS_NO_BAD) {
            slx_set_error("slx_merge: '%s' is not coordinate-sorted: record %llu of the file lies before its predecessor (tid ascending as unsigned, then pos)", x.path.c_str(),
                          (ull)(x.n_read + h[1].unsorted));
            return SLX_EINVAL;
        }
        if (!merge_fits(m->held_bytes + nb, m->max_bytes)) {
            slx_set_error("slx_merge: the windows would hold %llu bytes, more than max_bytes of %lld: '%s' had to read on at tid %d pos %d (a block of equal keys, or more inputs times batch_bytes than the budget)",
                          (ull)(m->held_bytes + nb), (long long)m->max_bytes, x.path.c_str(), (int)merge_key_tid(h[1].last_key), (int)merge_key_pos(h[1].last_key));
            return SLX_EUNSUPPORTED;
        }
        return SLX_OK;
    };
    const int rc = run();
    if (rc != SLX_OK) { (void)hipStreamSynchronize(st); (void)hipFree(g.base); return rc; }
    x.segs.push_back(g);
    x.has_last = true; x.last_read = h[1].last_key; x.n_read += n;
    m->mi[(size_t)i].held += n; m->mi[(size_t)i].last_key = h[1].last_key;
    m->held_bytes += nb;
    return SLX_OK;
}

// One round up to the output tables: refills, the bound, the key table, the eligible counts, the ranks, d_slen / d_ssrc / d_input in output order and d_doff.  m->E records
// and m->round_bytes bytes are ready to be gathered; *done = every input is at its end and nothing is held.
static int merge_round(slx_merge *m, bool *done)
{
    const int k = (int)m->in.size();
    hipStream_t st = m->st;
    *done = false; m->E = 0; m->round_bytes = 0;
    m->started = true;
    for (int i = 0; i < k; ++i) if (merge_wants_refill(m->mi[(size_t)i], m->had_bound, m->prev_bound)) SLX_CHK(merge_refill(m, i));
    uint64_t bound = 0;
    const bool finite = merge_bound(m->mi.data(), k, &bound);
    m->had_bound = finite; m->prev_bound = bound;
    ++m->c_rounds;
    uint64_t N = 0;
    for (int i = 0; i < k; ++i) N += m->mi[(size_t)i].held;
    if (N == 0) { *done = !finite; return SLX_OK; }
    if (N > 0xffffffffull) { slx_set_error("slx_merge: %llu records held: the merger's ordinals are 32 bits", (ull)N); return SLX_EUNSUPPORTED; }
    SLX_HIPCHK(hipSetDevice(m->device));
    SLX_CHK(m->d_key.ensure(8 * N)); SLX_CHK(m->d_src.ensure(8 * N)); SLX_CHK(m->d_len.ensure(4 * N));
    uint32_t *h_beg = m->h_tab.as<uint32_t>(), *h_ebeg = h_beg + (MG_MAX_IN + 1), *h_elig = h_ebeg + (MG_MAX_IN + 1);
    SLX_HIPCHK(hipEventRecord(m->ev[0], st));
    size_t at = 0;
    for (int i = 0; i < k; ++i) {          // the per-record tables of the windows side by side (the records themselves stay where they are)
        h_beg[i] = (uint32_t)at;
        const Input &x = m->in[(size_t)i];
        for (size_t s = 0; s < x.segs.size(); ++s) {
            const Seg &g = x.segs[s];
            const size_t c = s == 0 ? (size_t)x.consumed : 0, n = (size_t)g.n - c;
            SLX_HIPCHK(hipMemcpyAsync(m->d_key.as<ull>() + at, g.key + c, 8 * n, hipMemcpyDeviceToDevice, st));
            SLX_HIPCHK(hipMemcpyAsync(m->d_src.as<ull>() + at, g.src + c, 8 * n, hipMemcpyDeviceToDevice, st));
            SLX_HIPCHK(hipMemcpyAsync(m->d_len.as<uint32_t>() + at, g.len + c, 4 * n, hipMemcpyDeviceToDevice, st));
            at += n;
        }
    }
    h_beg[k] = (uint32_t)at;
    SLX_HIPCHK(hipMemcpyAsync(m->d_beg.p, h_beg, 4 * (size_t)(k + 1), hipMemcpyHostToDevice, st));
    k_merge_elig<<<(unsigned)k, 64, 0, st>>>(m->d_key.as<ull>(), m->d_beg.as<uint32_t>(), finite ? 1 : 0, bound, m->d_elig.as<uint32_t>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipMemcpyAsync(h_elig, m->d_elig.p, 4 * (size_t)k, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    uint64_t E = 0;
    m->elig.assign((size_t)k, 0);
    for (int i = 0; i < k; ++i) {
        if ((uint64_t)h_elig[i] > m->mi[(size_t)i].held) { slx_set_error("slx_merge: internal: %u eligible records of %llu held", h_elig[i], (ull)m->mi[(size_t)i].held); return SLX_EINVAL; }
        h_ebeg[i] = (uint32_t)E; m->elig[(size_t)i] = h_elig[i]; E += h_elig[i];
    }
    h_ebeg[k] = (uint32_t)E;
    if (E == 0) {
        SLX_HIPCHK(hipEventRecord(m->ev[1], st));
        SLX_HIPCHK(slx_wait_stream(st));
        m->us_rank += slx_ev_us(m->ev[0], m->ev[1]);
        return SLX_OK;
    }
    SLX_CHK(m->d_rank.ensure(4 * E)); SLX_CHK(m->d_slen.ensure(8 * (E + 1))); SLX_CHK(m->d_ssrc.ensure(8 * E)); SLX_CHK(m->d_doff.ensure(8 * (E + 1))); SLX_CHK(m->d_input.ensure(E));
    SLX_HIPCHK(hipMemcpyAsync(m->d_ebeg.p, h_ebeg, 4 * (size_t)(k + 1), hipMemcpyHostToDevice, st));
    SLX_HIPCHK(hipMemsetAsync(m->d_slen.p, 0, 8 * (E + 1), st));          // a place no rank names holds an empty record, not what the buffer held before
    SLX_HIPCHK(hipMemsetAsync(m->d_ssrc.p, 0, 8 * E, st));
    const unsigned grid = (unsigned)((E + 256) / 256);          // (one lane past the last record: slen[E])
    if (m->by_sort) {
        SLX_CHK(m->d_ekey.ensure(8 * E)); SLX_CHK(m->d_ekey_out.ensure(8 * E)); SLX_CHK(m->d_ord_in.ensure(4 * E)); SLX_CHK(m->d_ord_out.ensure(4 * E));
        for (int i = 0; i < k; ++i)
            if (h_elig[i]) SLX_HIPCHK(hipMemcpyAsync(m->d_ekey.as<ull>() + h_ebeg[i], m->d_key.as<ull>() + h_beg[i], 8 * (size_t)h_elig[i], hipMemcpyDeviceToDevice, st));
        k_merge_iota<<<grid, 256, 0, st>>>(m->d_ord_in.as<uint32_t>(), E);
        SLX_HIPCHK(hipGetLastError());
        SLX_CHK(slx_cub("hipcub::DeviceRadixSort::SortPairs", m->d_tmp, 8, [&](void *t, size_t &b) {
            return hipcub::DeviceRadixSort::SortPairs(t, b, m->d_ekey.as<ull>(), m->d_ekey_out.as<ull>(), m->d_ord_in.as<uint32_t>(), m->d_ord_out.as<uint32_t>(), E, 0, 64, st);
        }));
        k_merge_unperm<<<grid, 256, 0, st>>>(m->d_ord_out.as<uint32_t>(), E, m->d_rank.as<uint32_t>());
    } else {
        k_merge_rank<<<grid, 256, 0, st>>>(m->d_key.as<ull>(), m->d_beg.as<uint32_t>(), m->d_ebeg.as<uint32_t>(), k, m->d_rank.as<uint32_t>());
    }
    SLX_HIPCHK(hipGetLastError());
    k_merge_place<<<grid, 256, 0, st>>>(m->d_beg.as<uint32_t>(), m->d_ebeg.as<uint32_t>(), k, m->d_rank.as<uint32_t>(), m->d_len.as<uint32_t>(), m->d_src.as<ull>(), m->d_slen.as<ull>(),
                                        m->d_ssrc.as<ull>(), m->d_input.as<uint8_t>());
    SLX_HIPCHK(hipGetLastError());
    SLX_CHK(slx_exclusive_sum(m->d_tmp, m->d_slen.as<ull>(), m->d_doff.as<ull>(), E + 1, st, 8));
    SLX_HIPCHK(hipEventRecord(m->ev[1], st));
    ull *h_bytes = (ull *)(h_elig + (MG_MAX_IN + 1) + 1);          // (8-byte aligned: three tables of 65 words and one more)
    SLX_HIPCHK(hipMemcpyAsync(h_bytes, m->d_doff.as<ull>() + E, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    m->us_rank += slx_ev_us(m->ev[0], m->ev[1]);
    m->E = E; m->round_bytes = *h_bytes;
    if (m->round_bytes > m->held_bytes) { slx_set_error("slx_merge: internal: a round of %llu bytes out of windows of %llu", (ull)m->round_bytes, (ull)m->held_bytes); return SLX_EINVAL; }
    return SLX_OK;
}

// tiles [tile0, tile_end) of the round's stream into out (its first byte is the stream's byte tile0 * RS_TILE); returns when they are there
static int merge_gather(slx_merge *m, uint64_t tile0, uint64_t tile_end, uint8_t *out)
{
    hipStream_t st = m->st;
    const uint64_t grid = (tile_end - tile0 + 3) / 4;
    if (grid > 0x7fffffffull) { slx_set_error("slx_merge: %llu tiles in one gather are more than a grid holds", (ull)(tile_end - tile0)); return SLX_EUNSUPPORTED; }
    SLX_HIPCHK(hipSetDevice(m->device));
    SLX_HIPCHK(hipEventRecord(m->ev[0], st));
    k_merge_gather<<<(unsigned)grid, 256, 0, st>>>(m->d_doff.as<ull>(), m->d_ssrc.as<ull>(), (int64_t)m->E, m->round_bytes, tile0, tile_end, out);
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(m->ev[1], st));
    SLX_HIPCHK(slx_wait_stream(st));
    m->us_gather += slx_ev_us(m->ev[0], m->ev[1]);
    return SLX_OK;
}

// the round's records have left: they go from the front of their windows, and a batch whose last record went is freed
static void merge_consume(slx_merge *m)
{
    for (size_t i = 0; i < m->in.size(); ++i) {
        Input &x = m->in[i];
        uint64_t c = m->elig[i];
        m->mi[i].held -= c;
        while (c) {
            Seg &g = x.segs.front();
            const uint64_t left = g.n - x.consumed;
            if (c < left) { x.consumed += c; break; }
            c -= left;
            (void)hipFree(g.base);
            m->held_bytes -= g.n_bytes;
            x.segs.pop_front(); x.consumed = 0;
        }
    }
    m->c_records += (int64_t)m->E; m->c_bytes += (int64_t)m->round_bytes;
    m->E = 0;
}

// rounds until one emits something (or the end)
static int merge_next_round(slx_merge *m, bool *done)
{
    for (;;) {
        SLX_CHK(merge_round(m, done));
        if (*done || m->E) return SLX_OK;
    }
}

// after an error the merge cannot go on (an input has been read past what was emitted): the windows go, the counters stay
static int merge_fail(slx_merge *m, int rc)
{
    const std::string msg = slx_last_error();
    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->st);
    merge_drop_windows(m);
    for (merge_in &x : m->mi) x.at_end = true;
    m->had_bound = false;
    slx_set_error("%s", msg.c_str());
    return rc;
}

extern "C" int slx_merge_next(slx_merge *m, slx_merge_batch *b)
{
    if (!m || !b) { slx_set_error("slx_merge_next: null argument"); return SLX_EINVAL; }
    memset(b, 0, sizeof *b);
    if (m->in.empty()) { slx_set_error("slx_merge_next: no input was added"); return SLX_EINVAL; }
    auto run = [&]() -> int {
        bool done = false;
        SLX_CHK(merge_next_round(m, &done));
        if (done) return SLX_OK;
        const uint64_t n_tiles = (m->round_bytes + RS_TILE - 1) / RS_TILE;
        SLX_CHK(m->d_out.ensure((size_t)n_tiles * RS_TILE));
        SLX_CHK(merge_gather(m, 0, n_tiles, m->d_out.as<uint8_t>()));
        b->n_records = (int64_t)m->E; b->n_bytes = (int64_t)m->round_bytes;
        b->d_stream = m->d_out.p; b->d_rec_off = m->d_doff.p; b->d_input = m->d_input.p;
        merge_consume(m);
        return SLX_OK;
    };
    const int rc = run();
    return rc == SLX_OK ? rc : merge_fail(m, rc);
}

extern "C" int slx_merge_batch_to_host(slx_merge *m, const slx_merge_batch *b, void *stream, uint64_t *rec_off, uint8_t *input)
{
    if (!m || !b) { slx_set_error("slx_merge_batch_to_host: null argument"); return SLX_EINVAL; }
    SLX_HIPCHK(hipSetDevice(m->device));
    if (stream && b->n_bytes) SLX_HIPCHK(hipMemcpyAsync(stream, b->d_stream, (size_t)b->n_bytes, hipMemcpyDeviceToHost, m->st));
    if (rec_off) {
        if (b->n_records) SLX_HIPCHK(hipMemcpyAsync(rec_off, b->d_rec_off, 8 * ((size_t)b->n_records + 1), hipMemcpyDeviceToHost, m->st));
        else rec_off[0] = 0;
    }
    if (input && b->n_records) SLX_HIPCHK(hipMemcpyAsync(input, b->d_input, (size_t)b->n_records, hipMemcpyDeviceToHost, m->st));
    SLX_HIPCHK(hipStreamSynchronize(m->st));
    return SLX_OK;
}

static int merge_run_impl(slx_merge *m, slx_bgzf *w)
{
    const uint64_t slab_tiles = (uint64_t)m->slab_bytes / RS_TILE;
    for (;;) {
        bool done = false;
        SLX_CHK(merge_next_round(m, &done));
        if (done) return SLX_OK;
        const uint64_t B = m->round_bytes, n_tiles = (B + RS_TILE - 1) / RS_TILE;
        SLX_CHK(m->d_slab.ensure((size_t)std::min<uint64_t>(n_tiles, slab_tiles) * RS_TILE));
        for (uint64_t t = 0; t < n_tiles; t += slab_tiles) {
            const uint64_t te = std::min(n_tiles, t + slab_tiles), bytes = std::min(B, te * RS_TILE) - t * RS_TILE;
            SLX_CHK(merge_gather(m, t, te, m->d_slab.as<uint8_t>()));
            SLX_CHK(slx_bgzf_write_device(w, m->d_slab.p, (int64_t)bytes));          // staged when it returns: the slab is free for the next range of tiles
        }
        merge_consume(m);
    }
}

extern "C" int slx_merge_run(slx_merge *m, slx_bgzf *w)
{
    if (!m || !w) { slx_set_error("slx_merge_run: null argument"); return SLX_EINVAL; }
    if (m->in.empty()) { slx_set_error("slx_merge_run: no input was added"); return SLX_EINVAL; }
    // the writer takes the slabs by a device-to-device copy inside its own device: an empty write makes it select that device, which must be the merger's
    int rc = slx_bgzf_write_device(w, nullptr, 0), wdev = -1;
    if (rc == SLX_OK && (hipGetDevice(&wdev) != hipSuccess || wdev != m->device)) {
        slx_set_error("slx_merge_run: the writer is on device %d, the merger on device %d: both must be on one", wdev, m->device);
        return SLX_EINVAL;          // (nothing was read, nothing is written: the merger is as it was)
    }
    if (rc == SLX_OK) rc = merge_run_impl(m, w);
    return rc == SLX_OK ? rc : merge_fail(m, rc);
}

static int merge_files_impl(slx_merge *m, const char *const *in_paths, int n, const char *out_path, bool *created)
{
    for (int i = 0; i < n; ++i) SLX_CHK(slx_merge_add_file(m, in_paths[i]));
    slx_bgzf *w = nullptr;
    SLX_CHK(slx_bgzf_open(out_path, m->device, &w));
    *created = true;
    int rc = slx_bgzf_write(w, m->header.data(), (int64_t)m->header.size());
    if (rc == SLX_OK) rc = slx_bgzf_flush(w);          // the records start in a member of their own, as BamWriter::WriteHeader leaves them
    if (rc == SLX_OK) rc = slx_merge_run(m, w);
    const std::string msg = rc != SLX_OK ? slx_last_error() : "";
    const int rc2 = slx_bgzf_close(w);
    if (rc != SLX_OK) { slx_set_error("%s", msg.c_str()); return rc; }
    return rc2;
}

// slx_merge_files with a merger that has no inputs yet
static int slx_merge_files_with(slx_merge *m, const char *const *in_paths, int n, const char *out_path)
{
    if (!m || !in_paths || n <= 0 || !out_path) { slx_set_error("slx_merge_files: null argument or no input"); return SLX_EINVAL; }
    if (!strcmp(out_path, "-")) { slx_set_error("slx_merge_files: '-': the output is a file, not a pipe"); return SLX_EINVAL; }
    for (int i = 0; i < n; ++i) {
        if (!in_paths[i]) { slx_set_error("slx_merge_files: input %d is null", i); return SLX_EINVAL; }
        if (!strcmp(in_paths[i], out_path)) { slx_set_error("slx_merge_files: '%s' is input %d and the output: the output must be another file than every input", out_path, i); return SLX_EINVAL; }
    }
    if (n > MG_MAX_IN) { slx_set_error("slx_merge_files: %d inputs: at most %d are merged in one pass (there is no multi-pass merge)", n, MG_MAX_IN); return SLX_EUNSUPPORTED; }
    if (!m->in.empty()) { slx_set_error("slx_merge_files: the merger has %zu inputs already", m->in.size()); return SLX_EINVAL; }
    bool created = false;
    const int rc = merge_files_impl(m, in_paths, n, out_path, &created);
    if (rc != SLX_OK) {
        const std::string msg = slx_last_error();
        if (created) (void)unlink(out_path);          // no output file is left behind
        slx_set_error("%s", msg.c_str());
    }
    return rc;
}

extern "C" int slx_merge_files(const char *const *in_paths, int n, const char *out_path, int device)
{
    if (!in_paths || n <= 0 || !out_path) { slx_set_error("slx_merge_files: null argument or no input"); return SLX_EINVAL; }
    int ndev = 0;
    SLX_CHK(slx_count_devices(merge_no_device("slx_merge_files").c_str(), &ndev));
    slx_merge *m = nullptr;
    SLX_CHK(slx_merge_create(device, &m));
    const int rc = slx_merge_files_with(m, in_paths, n, out_path);
    const std::string msg = rc != SLX_OK ? slx_last_error() : "";
    slx_merge_free(m);
    if (rc != SLX_OK) slx_set_error("%s", msg.c_str());
    return rc;
}

extern "C" int slx_merge_set(slx_merge *m, const char *key, int64_t value)
{
    if (!m || !key) { slx_set_error("slx_merge_set: null argument"); return SLX_EINVAL; }
    if (!strcmp(key, "max_bytes") && value >= 1) { m->max_bytes = value; return SLX_OK; }
    if (!strcmp(key, "slab_bytes") && value >= (int64_t)RS_TILE && value <= MERGE_MAX_SLAB && value % (int64_t)RS_TILE == 0) { m->slab_bytes = value; return SLX_OK; }
    if (!strcmp(key, "batch_bytes") && value >= 1) { m->batch_bytes = value; return SLX_OK; }
    if (!strcmp(key, "by_sort") && (value == 0 || value == 1)) { m->by_sort = value; return SLX_OK; }
    slx_set_error("slx_merge_set: unknown key or value out of range: %s = %lld (slab_bytes is a multiple of the %u-byte tile, at least one, at most %lld bytes; by_sort is 0 or 1)", key,
                  (long long)value, RS_TILE, (long long)MERGE_MAX_SLAB);
    return SLX_EINVAL;
}

extern "C" int64_t slx_merge_counter(const slx_merge *m, const char *name)
{
    if (!m || !name) return -1;
    if (!strcmp(name, "inputs")) return (int64_t)m->in.size();
    if (!strcmp(name, "device")) return m->device;
    if (!strcmp(name, "records")) return m->c_records;
    if (!strcmp(name, "bytes")) return m->c_bytes;
    if (!strcmp(name, "rounds")) return m->c_rounds;
    if (!strcmp(name, "refills")) return m->c_refills;
    if (!strcmp(name, "us_key")) return (int64_t)m->us_key;
    if (!strcmp(name, "us_rank")) return (int64_t)m->us_rank;
    if (!strcmp(name, "us_gather")) return (int64_t)m->us_gather;
    if (!strcmp(name, "held_bytes")) return (int64_t)m->held_bytes;
    if (!strcmp(name, "held_records")) { uint64_t n = 0; for (const merge_in &x : m->mi) n += x.held; return (int64_t)n; }
    return -1;
}
