// slx_fastq.hip -- the FastqReader path of libseqlib_amd.so (include/seqlib_amd_fastq.h): FASTA / FASTQ text parsed on the GPU into the arrays
// slx_align_batch_device and slx_rec_build take.  DESIGN.md section 9.6 has the argument; the pattern is the BAM reader's (section 9): guess, verify, and walk
// again what fails.
//   k_bgzf_inflate / k_bgzf_crc   (slx_bam.hip, through slx_bgzf_inflate_members) BGZF members straight into the text buffer, one wave per member     dev_inflate.h
//   k_fq_count / k_fq_lines   line feeds per tile, then (after hipCUB's scan of the counts) the line starts, by a wave prefix per 1 KiB step
//   k_fq_check                one lane per record taken as four lines: the acceptance test, the fields' places and lengths     dev_fastq.h
//   k_fq_gather               one launch per stream (bases, qualities, names, comments): one wave per tile of the OUTPUT, through LDS, aligned 16-byte stores
// The source side (producer thread, BGZF inflate, the text window, the line starts) is fq_text.h's FqText, which the SAM reader (slx_sam.hip) is built on too; its
// functions are defined here.
// From the first record that fails the test the rest of the batch's text comes down and goes through fq_host.h; its reads go up and are gathered like the others.
// Waves take tiles / members / records by a static map: there is no work queue here (DESIGN.md section 4 does not arise), and the only atomic is one
// atomicMin per wave that holds a failing record.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>
#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "slx_internal.h"
#include "seqlib_amd_bam.h"
#include "seqlib_amd_fastq.h"
#include "dev_inflate.h"
#include "dev_lanes.h"
#include "dev_fastq.h"
#include "fq_host.h"
#include "fq_text.h"

typedef uint32_t fq_v4 __attribute__((ext_vector_type(4)));

#define FQ_GATHER_MAX 4096u          // LDS image of one output tile, per wave

// ------------------------------------------------------------------ kernels
// bit i = byte i of the 16 at text + pos is a line feed and lies below n.  The load is an aligned 16-byte one inside the buffer (its capacity is n rounded up
// to 16 and more); bytes at and behind n are whatever the buffer holds and are masked.
__device__ __forceinline__ uint32_t fq_nl_mask(const uint8_t *text, uint64_t pos, uint64_t n)
{
    const fq_v4 v = *reinterpret_cast<const fq_v4 *>(text + pos);
    uint32_t m = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t x = v[w] ^ 0x0a0a0a0au;
        const uint32_t t = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);          // 0x80 in every byte of x that is zero
        m |= (((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u)) << (4 * w);
    }
    const uint64_t left = n - pos;
    return left >= 16 ? m : m & ((1u << (uint32_t)left) - 1u);
}

// count[t] = line feeds of tile t (tile bytes each, a multiple of 16), one wave per tile
__global__ __launch_bounds__(256) void k_fq_count(const uint8_t *text, uint64_t n, uint32_t tile, uint64_t n_tiles, fq_u64 *count)
{
    const uint64_t t = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (t >= n_tiles) return;
    const uint64_t t0 = t * tile, t1 = t0 + tile < n ? t0 + tile : n;
    uint32_t c = 0;
    for (uint64_t p = t0 + ((uint64_t)lane << 4); p < t1; p += 1024) c += (uint32_t)__popc(fq_nl_mask(text, p, t1));
    c = wave_sum(c);
    if (lane == 0) count[t] = c;
}

// line_off[0] = 0, line_off[1 + j] = the byte behind line feed j; with `virt` the end of the input is one more line end: line_off[total + 1] = n + 1.
// base = the exclusive sum of count, base[n_tiles] the total.
__global__ __launch_bounds__(256) void k_fq_lines(const uint8_t *text, uint64_t n, uint32_t tile, uint64_t n_tiles, const fq_u64 *base, int virt, fq_u64 *line_off)
{
    const uint64_t t = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (t >= n_tiles) return;
    if (t == 0 && lane == 0) {
        line_off[0] = 0;
        if (virt) line_off[base[n_tiles] + 1] = n + 1;
    }
    const uint64_t t0 = t * tile, t1 = t0 + tile < n ? t0 + tile : n;
    uint64_t at = base[t] + 1;
    for (uint64_t s = t0; s < t1; s += 1024) {          // (wave-uniform trip count: the shuffles below see all 64 lanes)
        const uint64_t p = s + ((uint64_t)lane << 4);
        uint32_t m = p < t1 ? fq_nl_mask(text, p, t1) : 0u;
        const uint32_t c = (uint32_t)__popc(m);
        uint32_t total;
        uint64_t w = at + wave_scan_excl(c, &total);
        while (m) { const uint32_t j = (uint32_t)__ffs(m) - 1u; m &= m - 1u; line_off[w++] = p + j + 1; }
        at += total;
    }
}

struct fq_arrays {          // per record; the first three are what the exclusive sums take
    fq_u64 *len_b, *len_n, *len_c;
    fq_u64 *src_b, *src_q, *src_n, *src_c;          // address of the field's first byte
    uint8_t *flags;
};

// first[0] = min over the records that are not FQ_OK of (k << 2 | status)
__global__ __launch_bounds__(256) void k_fq_check(const uint8_t *text, uint64_t n, const fq_u64 *line_off, uint64_t n_lines, int eof, int fast_fail, uint64_t n_cand,
                                                  fq_arrays A, fq_u64 *first)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    fq_u64 key = ~0ull;
    if (k < n_cand) {
        fq_rec_out o;
        int s = fq_check(text, n, (const uint64_t *)line_off, n_lines, eof != 0, k, &o);
        if (s == FQ_OK && fast_fail) s = FQ_FAIL;
        if (s == FQ_OK) {
            A.len_b[k] = o.len_seq; A.len_n[k] = o.len_name; A.len_c[k] = o.len_com;
            A.src_b[k] = (fq_u64)(uintptr_t)(text + o.seq); A.src_q[k] = (fq_u64)(uintptr_t)(text + o.qual);
            A.src_n[k] = (fq_u64)(uintptr_t)(text + o.name); A.src_c[k] = (fq_u64)(uintptr_t)(text + o.com);
            A.flags[k] = (uint8_t)o.flag;
        } else key = (fq_u64)k << 2 | (fq_u64)s;
    }
    wave_report_min(first, key);          // at most one atomic per wave, and only from a wave that holds a failing record
}

// out[0, off[n]) = the fields src[k][0, off[k + 1] - off[k]) one behind the other.  One wave per `tile` output bytes (a multiple of 16, at most FQ_GATHER_MAX):
// the owner of every 16th byte by binary search in off, the owners of the bytes between by walking on from it; bytes come into the tile's image in LDS
// (consecutive lanes read consecutive bytes of a field), the image goes out in aligned 16-byte stores.  out is 16-byte aligned and holds off[n] rounded up to 16.
__global__ __launch_bounds__(256) void k_fq_gather(const fq_u64 *src, const fq_u64 *off, uint64_t n, uint64_t total, uint32_t tile, uint8_t *out)
{
    __shared__ __attribute__((aligned(16))) uint8_t img[4][FQ_GATHER_MAX];
    __shared__ uint32_t own[4][FQ_GATHER_MAX / 16];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t t0 = ((uint64_t)blockIdx.x * 4 + wave) * tile;
    if (t0 >= total || n == 0) return;
    const uint32_t nb = (uint32_t)(t0 + tile < total ? tile : total - t0);
    for (uint32_t w = lane; (w << 4) < nb; w += 64) {
        const uint64_t p = t0 + ((uint64_t)w << 4);
        uint64_t lo = 0, hi = n;          // off[lo] <= p < off[hi]: off[0] = 0 and off[n] = total > p
        while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (off[mid] <= p) lo = mid; else hi = mid; }
        own[wave][w] = (uint32_t)lo;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (uint32_t i = lane; i < nb; i += 64) {
        const uint64_t p = t0 + i;
        uint64_t k = own[wave][i >> 4];
        while (k + 1 < n && off[k + 1] <= p) ++k;          // (fields of no bytes are stepped over; p < off[n] ends the walk below n)
        img[wave][i] = *(const uint8_t *)(uintptr_t)(src[k] + (p - off[k]));
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t n16 = (nb + 15u) & ~15u;                // the last tile's ragged tail goes out as a whole word too: out holds it
    for (uint32_t o = lane << 4; o < n16; o += 64 << 4) *reinterpret_cast<fq_v4 *>(out + t0 + o) = *reinterpret_cast<const fq_v4 *>(&img[wave][o]);
}


// ------------------------------------------------------------------ host: the reader
struct slx_fastq : FqText {          // the source, the text window and its line starts: fq_text.h
    bool done = false;
    uint32_t gather_tile = 2048; int fast_fail = 0;
    FqDBuf d_first{*this}, d_slow{*this};
    FqDBuf d_len_b{*this}, d_len_n{*this}, d_len_c{*this}, d_src_b{*this}, d_src_q{*this}, d_src_n{*this}, d_src_c{*this}, d_flags{*this},
           d_off_b{*this}, d_off_n{*this}, d_off_c{*this}, d_bases{*this}, d_quals{*this}, d_names{*this}, d_coms{*this};
    FqHBuf h_tail{*this}, h_slow{*this};
    int64_t c_reads = 0, c_fast = 0, c_slow = 0, c_batches = 0, c_bad_tail = 0;
    slx_fastq_batch last = {};
    uint64_t tot_b = 0, tot_n = 0, tot_c = 0;
};

void fq_text_free(FqText *t)
{
    t->prod.release();
    if (t->st) { (void)hipSetDevice(t->device); (void)hipStreamSynchronize(t->st); }
    t->stage.release();          // (dev_inflate.h's staging buffers: they have no owner, the stream has drained)
    t->close();                  // the window's buffers and the reader's own
    if (t->map) munmap((void *)t->map, t->fsize);
    if (t->fd >= 0) ::close(t->fd);
    t->map = nullptr; t->fd = -1;
}

static void fq_free(slx_fastq *fq)
{
    fq_text_free(fq);
    delete fq;
}

int fq_text_start(FqText *t)
{
    t->have = t->used = 0; t->src_eof = false; t->next_member = 0; t->c_members = 0;
    for (float &u : t->us) u = 0;
    if (t->source != 1) SLX_CHK(t->prod.start(t->path, t->source == 2));
    return SLX_OK;
}

static int fq_start(slx_fastq *fq)
{
    fq->done = false;
    fq->c_reads = fq->c_fast = fq->c_slow = fq->c_batches = fq->c_bad_tail = 0;
    fq->last = slx_fastq_batch{};
    return fq_text_start(fq);
}

int fq_text_open(FqText *t, const char *path, int device)
{
    const char *who = t->who;
    struct stat sb;
    if (stat(path, &sb) != 0 || !S_ISREG(sb.st_mode)) { slx_set_error("%s: '%s' is missing or not a regular file", who, path); return SLX_EIO; }
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) { slx_set_error("%s: cannot open '%s'", who, path); return SLX_EIO; }
    uint8_t h[18] = {0};
    const ssize_t got = ::pread(fd, h, sizeof h, 0);
    int source = 0;
    if (got >= 2 && h[0] == 0x1f && h[1] == 0x8b) source = (got >= 18 && h[2] == 8 && (h[3] & 4) && h[12] == 'B' && h[13] == 'C') ? 1 : 2;
    const std::string no_device = std::string("no HIP device: the ") + who + " parses on MI355X only (no CPU fallback)";
    const int rc = t->open(device, who, no_device.c_str());
    if (rc != SLX_OK) { ::close(fd); return rc; }
    t->path = path; t->source = source;
    if (source == 1) {
        t->fd = fd; t->fsize = (uint64_t)sb.st_size;
        void *p = mmap(nullptr, t->fsize, PROT_READ, MAP_PRIVATE, fd, 0);
        if (p == MAP_FAILED) { slx_set_error("%s: cannot map '%s'", who, path); return SLX_EIO; }
        t->map = (const uint8_t *)p;
        slx_bam_member *m = nullptr; int64_t nm = 0;
        SLX_CHK(slx_bam_scan_members(path, &m, &nm, nullptr));
        t->mem.assign(m, m + nm);
        slx_bam_members_free(m);
    } else ::close(fd);
    return SLX_OK;
}

extern "C" int slx_fastq_open(const char *path, int device, slx_fastq **out)
{
    if (!path || !out) { slx_set_error("slx_fastq_open: null argument"); return SLX_EINVAL; }
    *out = nullptr;
    slx_fastq *fq = new slx_fastq();
    int rc = fq_text_open(fq, path, device);
    if (rc == SLX_OK) rc = fq_start(fq);
    if (rc != SLX_OK) { fq_free(fq); return rc; }
    *out = fq;
    return SLX_OK;
}

extern "C" void slx_fastq_close(slx_fastq *fq) { if (fq) fq_free(fq); }

extern "C" int slx_fastq_rewind(slx_fastq *fq)
{
    if (!fq) { slx_set_error("slx_fastq_rewind: null reader"); return SLX_EINVAL; }
    SLX_HIPCHK(hipSetDevice(fq->device));
    return fq_start(fq);
}

extern "C" int slx_fastq_set(slx_fastq *fq, const char *key, int64_t value)
{
    if (!fq || !key) { slx_set_error("slx_fastq_set: null argument"); return SLX_EINVAL; }
    const std::string k = key;
    if (k == "tile_bytes" && value >= 16 && value % 16 == 0 && value <= (1 << 30)) { fq->tile_bytes = (uint32_t)value; return SLX_OK; }
    if (k == "gather_tile_bytes" && value >= 16 && value % 16 == 0 && value <= (int64_t)FQ_GATHER_MAX) { fq->gather_tile = (uint32_t)value; return SLX_OK; }
    if (k == "fast_fail" && (value == 0 || value == 1)) { fq->fast_fail = (int)value; return SLX_OK; }
    slx_set_error("slx_fastq_set: unknown key '%s' or value %lld out of range", key, (long long)value);
    return SLX_EINVAL;
}

extern "C" int64_t slx_fastq_counter(const slx_fastq *fq, const char *name)
{
    if (!fq || !name) return -1;
    const std::string k = name;
    if (k == "reads") return fq->c_reads;
    if (k == "fast_reads") return fq->c_fast;
    if (k == "slow_reads") return fq->c_slow;
    if (k == "batches") return fq->c_batches;
    if (k == "bad_tail") return fq->c_bad_tail;
    if (k == "source") return fq->source;
    if (k == "us_lines") return (int64_t)fq->us[0];
    if (k == "us_check") return (int64_t)fq->us[1];
    if (k == "us_gather") return (int64_t)fq->us[2];
    if (k == "us_inflate") return (int64_t)fq->us[3];
    return -1;
}

// at least `want` more bytes of text (fewer only at the end of the source) behind d_text[cur][have)
int fq_pull(FqText *fq, uint64_t want)
{
    hipStream_t st = fq->st;
    FqDBuf &T = fq->d_text[fq->cur];
    if (fq->source == 1) {
        const int64_t a = fq->next_member, nm = (int64_t)fq->mem.size();
        int64_t b = a;
        uint64_t out = 0;
        while (b < nm && (out < want || b == a)) out += fq->mem[b++].isize;
        if (b > a && out > 0) {
            SLX_CHK(T.ensure(fq->have + out + 64, st, fq->have));
            float us[2] = {0, 0};
            SLX_CHK(slx_bgzf_inflate_members(fq->map, fq->path.c_str(), fq->mem.data(), a, b, fq->stage, T.as<uint8_t>(), fq->have, fq->have + out, st, fq->ev[8], nullptr, fq->ev[9], us));
            fq->us[3] += us[0]; fq->c_members += b - a;
            fq->have += out;
        }
        fq->next_member = b;
        if (b >= nm) fq->src_eof = true;
        return SLX_OK;
    }
    uint64_t got = 0;
    while (got < want && !fq->src_eof) {
        FqProducer::Slot &s = fq->prod.front();
        if (s.err) { slx_set_error("%s: reading '%s' failed%s", fq->who, fq->path.c_str(), fq->source == 2 ? " (zlib refuses the stream)" : ""); return SLX_EIO; }
        const uint64_t take = std::min<uint64_t>(want - got, s.n - fq->prod.tail_pos);
        if (take) {
            SLX_CHK(T.ensure(fq->have + take + 64, st, fq->have));
            SLX_HIPCHK(hipMemcpyAsync(T.as<uint8_t>() + fq->have, s.p + fq->prod.tail_pos, take, hipMemcpyHostToDevice, st));
            SLX_HIPCHK(slx_wait_stream(st));          // (the slot goes back to the producer)
            fq->have += take; got += take; fq->prod.tail_pos += take;
        }
        if (fq->prod.tail_pos == s.n) {
            const bool eof = s.eof;
            if (eof) fq->src_eof = true; else fq->prod.pop();
        }
    }
    return SLX_OK;
}

int fq_line_starts(FqText *fq, uint64_t *n_lines, int *virt_out)
{
    hipStream_t st = fq->st;
    const uint8_t *text = fq->d_text[fq->cur].as<uint8_t>();
    const uint64_t n = fq->have;
    const uint32_t tile = fq->tile_bytes;
    const uint64_t n_tiles = (n + tile - 1) / tile;
    SLX_CHK(fq->h_small.ensure(256));
    fq_u64 *hs = fq->h_small.as<fq_u64>();
    SLX_CHK(fq->d_count.ensure(8 * (n_tiles + 1))); SLX_CHK(fq->d_base.ensure(8 * (n_tiles + 1)));
    SLX_HIPCHK(hipMemsetAsync(fq->d_count.p, 0, 8 * (n_tiles + 1), st));
    SLX_HIPCHK(hipEventRecord(fq->ev[0], st));
    k_fq_count<<<(unsigned)((n_tiles + 3) / 4), 256, 0, st>>>(text, n, tile, n_tiles, fq->d_count.as<fq_u64>());
    SLX_HIPCHK(hipGetLastError());
    SLX_CHK(fq_scan(fq, fq->d_count.as<fq_u64>(), fq->d_base.as<fq_u64>(), n_tiles + 1));
    SLX_HIPCHK(hipMemcpyAsync(hs, fq->d_base.as<fq_u64>() + n_tiles, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync(hs + 1, text + n - 1, 1, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    const uint64_t n_nl = hs[0];
    const int virt = fq->src_eof && *(const uint8_t *)(hs + 1) != '\n' ? 1 : 0;
    const uint64_t L = n_nl + (uint64_t)virt;
    SLX_CHK(fq->d_line.ensure(8 * (L + 2)));
    k_fq_lines<<<(unsigned)((n_tiles + 3) / 4), 256, 0, st>>>(text, n, tile, n_tiles, fq->d_base.as<fq_u64>(), virt, fq->d_line.as<fq_u64>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(fq->ev[1], st));
    *n_lines = L; *virt_out = virt;
    return SLX_OK;
}

int fq_shift(FqText *fq, uint64_t room)
{
    const uint64_t left = fq->have - fq->used;
    FqDBuf &O = fq->d_text[fq->cur ^ 1];
    SLX_CHK(O.ensure(left + room + 64));
    if (left) SLX_HIPCHK(hipMemcpyAsync(O.p, fq->d_text[fq->cur].as<uint8_t>() + fq->used, left, hipMemcpyDeviceToDevice, fq->st));
    SLX_HIPCHK(slx_wait_stream(fq->st));
    fq->cur ^= 1; fq->have = left; fq->used = 0;
    return SLX_OK;
}

// one attempt on d_text[cur][0, have): *n_reads reads into the output arrays, *consumed bytes of text used up (also when no read came of it)
static int fq_parse(slx_fastq *fq, int64_t *n_reads, int64_t *n_slow, uint64_t *consumed)
{
    hipStream_t st = fq->st;
    const uint8_t *text = fq->d_text[fq->cur].as<uint8_t>();
    const uint64_t n = fq->have;
    const bool eof = fq->src_eof;
    uint64_t L = 0;
    int virt = 0;
    SLX_CHK(fq_line_starts(fq, &L, &virt));          // ---- line starts
    fq_u64 *hs = fq->h_small.as<fq_u64>();
    // ---- the records taken as four lines each
    const uint64_t n_cand = L / 4 + 1;
    FqDBuf *per8[7] = {&fq->d_len_b, &fq->d_len_n, &fq->d_len_c, &fq->d_src_b, &fq->d_src_q, &fq->d_src_n, &fq->d_src_c};
    for (FqDBuf *b : per8) SLX_CHK(b->ensure(8 * (n_cand + 1)));
    SLX_CHK(fq->d_flags.ensure(n_cand + 1));
    SLX_CHK(fq->d_first.ensure(8));
    SLX_HIPCHK(hipMemsetAsync(fq->d_first.p, 0xff, 8, st));
    fq_arrays A{fq->d_len_b.as<fq_u64>(), fq->d_len_n.as<fq_u64>(), fq->d_len_c.as<fq_u64>(), fq->d_src_b.as<fq_u64>(), fq->d_src_q.as<fq_u64>(), fq->d_src_n.as<fq_u64>(),
                fq->d_src_c.as<fq_u64>(), fq->d_flags.as<uint8_t>()};
    SLX_HIPCHK(hipEventRecord(fq->ev[2], st));
    k_fq_check<<<(unsigned)((n_cand + 255) / 256), 256, 0, st>>>(text, n, fq->d_line.as<fq_u64>(), L, eof ? 1 : 0, fq->fast_fail, n_cand, A, fq->d_first.as<fq_u64>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(fq->ev[3], st));
    SLX_HIPCHK(hipMemcpyAsync(hs, fq->d_first.p, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    fq->us[0] += slx_ev_us(fq->ev[0], fq->ev[1]); fq->us[1] += slx_ev_us(fq->ev[2], fq->ev[3]);
    if (hs[0] == ~0ull) { slx_set_error("FASTQ reader: internal: no record ends the fast path"); return SLX_EINTERNAL; }          // (the last candidate is never FQ_OK)
    const uint64_t F = hs[0] >> 2;
    const int status = (int)(hs[0] & 3);
    SLX_HIPCHK(hipMemcpyAsync(hs, fq->d_line.as<fq_u64>() + 4 * F, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    const uint64_t fast_end = status == FQ_NONE ? n : std::min<uint64_t>(hs[0], n);
    // ---- the serial parser from the first record that failed
    uint64_t S = 0, pos = 0;
    std::vector<uint64_t> sl[3];          // lengths of the slow reads: bases, names, comments
    std::string sb, sq, sn, sc, sf;
    if (status == FQ_FAIL) {
        const uint64_t m = n - fast_end;
        SLX_CHK(fq->h_tail.ensure(m + 1));
        SLX_HIPCHK(hipMemcpyAsync(fq->h_tail.p, text + fast_end, m, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(slx_wait_stream(st));
        const uint8_t *p = fq->h_tail.as<uint8_t>();
        fqh_rec r;
        for (;;) {
            size_t used = 0;
            const int rc = fqh_parse(p + pos, (size_t)(m - pos), eof, r, &used);
            pos += used;
            if (rc == FQH_BAD) { fq->c_bad_tail = 1; fq->done = true; pos = m; }
            if (rc != FQH_REC) break;
            sl[0].push_back(r.seq.size()); sl[1].push_back(r.name.size()); sl[2].push_back(r.com.size());
            sb += r.seq; sn += r.name; sc += r.com;
            if (r.has_qual) sq += r.qual; else sq.append(r.seq.size(), '\0');
            sf.push_back((char)((r.has_com ? 1 : 0) | (r.has_qual ? 2 : 0)));
            ++S;
        }
    }
    *consumed = fast_end + pos;
    const uint64_t N = F + S;
    *n_reads = (int64_t)N; *n_slow = (int64_t)S;
    if (N == 0) return SLX_OK;
    if (N >= 0xffffffffull) { slx_set_error("FASTQ reader: 2^32 reads or more in one batch; ask for fewer bytes"); return SLX_EUNSUPPORTED; }
    // ---- the slow reads' bytes and per-record entries go up behind the fast ones
    for (FqDBuf *b : per8) SLX_CHK(b->ensure(8 * (N + 1), st, 8 * F));
    SLX_CHK(fq->d_flags.ensure(N + 1, st, F));
    {
        const uint64_t nb = sb.size(), nn = sn.size(), nc = sc.size();
        const uint64_t bytes = 2 * nb + nn + nc;
        const uint64_t arr = 8 * (3 * (S + 1) + 4 * S);
        SLX_CHK(fq->h_slow.ensure(bytes + arr + S + 64)); SLX_CHK(fq->d_slow.ensure(bytes + 64));
        uint8_t *h = fq->h_slow.as<uint8_t>();
        memcpy(h, sb.data(), nb); memcpy(h + nb, sq.data(), nb); memcpy(h + 2 * nb, sn.data(), nn); memcpy(h + 2 * nb + nn, sc.data(), nc);
        const uint64_t a0 = (bytes + 15) & ~15ull;
        fq_u64 *len[3], *src[4];
        for (int i = 0; i < 3; ++i) len[i] = (fq_u64 *)(h + a0) + (uint64_t)i * (S + 1);
        for (int i = 0; i < 4; ++i) src[i] = (fq_u64 *)(h + a0) + 3 * (S + 1) + (uint64_t)i * S;
        uint8_t *hf = (uint8_t *)(src[3] + S);
        const fq_u64 d0 = (fq_u64)(uintptr_t)fq->d_slow.p;
        uint64_t ob = 0, on = 0, oc = 0;
        for (uint64_t i = 0; i < S; ++i) {
            len[0][i] = sl[0][i]; len[1][i] = sl[1][i]; len[2][i] = sl[2][i];
            src[0][i] = d0 + ob; src[1][i] = d0 + nb + ob; src[2][i] = d0 + 2 * nb + on; src[3][i] = d0 + 2 * nb + nn + oc;
            ob += sl[0][i]; on += sl[1][i]; oc += sl[2][i];
            hf[i] = (uint8_t)sf[i];
        }
        len[0][S] = len[1][S] = len[2][S] = 0;
        if (bytes) SLX_HIPCHK(hipMemcpyAsync(fq->d_slow.p, h, bytes, hipMemcpyHostToDevice, st));
        for (int i = 0; i < 3; ++i) SLX_HIPCHK(hipMemcpyAsync(per8[i]->as<fq_u64>() + F, len[i], 8 * (S + 1), hipMemcpyHostToDevice, st));
        if (S) {
            for (int i = 0; i < 4; ++i) SLX_HIPCHK(hipMemcpyAsync(per8[3 + i]->as<fq_u64>() + F, src[i], 8 * S, hipMemcpyHostToDevice, st));
            SLX_HIPCHK(hipMemcpyAsync(fq->d_flags.as<uint8_t>() + F, hf, S, hipMemcpyHostToDevice, st));
        }
    }
    // ---- offsets, then the four streams
    FqDBuf *offs[3] = {&fq->d_off_b, &fq->d_off_n, &fq->d_off_c};
    SLX_HIPCHK(hipEventRecord(fq->ev[4], st));
    for (int i = 0; i < 3; ++i) {
        SLX_CHK(offs[i]->ensure(8 * (N + 1)));
        SLX_CHK(fq_scan(fq, per8[i]->as<fq_u64>(), offs[i]->as<fq_u64>(), N + 1));
        SLX_HIPCHK(hipMemcpyAsync(hs + i, offs[i]->as<fq_u64>() + N, 8, hipMemcpyDeviceToHost, st));
    }
    SLX_HIPCHK(hipEventRecord(fq->ev[5], st));
    SLX_HIPCHK(slx_wait_stream(st));
    fq->us[1] += slx_ev_us(fq->ev[4], fq->ev[5]);
    fq->tot_b = hs[0]; fq->tot_n = hs[1]; fq->tot_c = hs[2];
    SLX_CHK(fq->d_bases.ensure(fq->tot_b + 64)); SLX_CHK(fq->d_quals.ensure(fq->tot_b + 64)); SLX_CHK(fq->d_names.ensure(fq->tot_n + 64)); SLX_CHK(fq->d_coms.ensure(fq->tot_c + 64));
    const uint32_t gt = fq->gather_tile;
    auto gather = [&](FqDBuf &src, FqDBuf &off, uint64_t total, FqDBuf &dst) {
        if (!total) return;
        const uint64_t tiles = (total + gt - 1) / gt;
        k_fq_gather<<<(unsigned)((tiles + 3) / 4), 256, 0, st>>>(src.as<fq_u64>(), off.as<fq_u64>(), N, total, gt, dst.as<uint8_t>());
    };
    SLX_HIPCHK(hipEventRecord(fq->ev[6], st));
    gather(fq->d_src_b, fq->d_off_b, fq->tot_b, fq->d_bases);
    gather(fq->d_src_q, fq->d_off_b, fq->tot_b, fq->d_quals);
    gather(fq->d_src_n, fq->d_off_n, fq->tot_n, fq->d_names);
    gather(fq->d_src_c, fq->d_off_c, fq->tot_c, fq->d_coms);
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(fq->ev[7], st));
    SLX_HIPCHK(slx_wait_stream(st));
    fq->us[2] += slx_ev_us(fq->ev[6], fq->ev[7]);
    return SLX_OK;
}

extern "C" int slx_fastq_next(slx_fastq *fq, int64_t max_bytes, slx_fastq_batch *b)
{
    if (!fq || !b) { slx_set_error("slx_fastq_next: null argument"); return SLX_EINVAL; }
    *b = slx_fastq_batch{};
    fq->last = *b;
    if (fq->done) return SLX_OK;
    if (max_bytes <= 0) max_bytes = 64ll << 20;
    SLX_HIPCHK(hipSetDevice(fq->device));
    hipStream_t st = fq->st;
    uint64_t target = (uint64_t)max_bytes, text_bytes = 0;
    for (;;) {
        if (fq->used) SLX_CHK(fq_shift(fq, target));          // the cut tail moves to the front of the other buffer
        if (fq->have < target && !fq->src_eof) SLX_CHK(fq_pull(fq, target - fq->have));
        if (fq->have == 0) {
            if (fq->src_eof) { fq->done = true; return SLX_OK; }
            continue;
        }
        int64_t n = 0, n_slow = 0;
        uint64_t consumed = 0;
        SLX_CHK(fq_parse(fq, &n, &n_slow, &consumed));
        fq->used = consumed; text_bytes += consumed;
        if (n > 0) {
            b->n_reads = n; b->n_slow_reads = n_slow; b->n_text_bytes = (int64_t)text_bytes;
            b->d_bases = fq->d_bases.p; b->d_offs = fq->d_off_b.p; b->d_quals = fq->d_quals.p;
            b->d_names = fq->d_names.p; b->d_name_offs = fq->d_off_n.p; b->d_coms = fq->d_coms.p; b->d_com_offs = fq->d_off_c.p; b->d_flags = fq->d_flags.p;
            fq->c_reads += n; fq->c_slow += n_slow; fq->c_fast += n - n_slow; fq->c_batches += 1;
            fq->last = *b;
            return SLX_OK;
        }
        if (fq->done) return SLX_OK;                                   // a damaged tail with no record before it
        if (fq->src_eof && consumed >= fq->have) { fq->done = true; return SLX_OK; }
        if (fq->src_eof && consumed == 0) { slx_set_error("FASTQ reader: internal: the parser made no progress at the end of '%s'", fq->path.c_str()); return SLX_EINTERNAL; }
        if (!fq->src_eof) target = std::max<uint64_t>(2 * target, 2 * (fq->have - consumed) + 64);          // not one whole record yet: the batch grows
    }
}

extern "C" int slx_fastq_to_host(slx_fastq *fq, const slx_fastq_batch *b, void *bases, uint64_t *offs, void *quals, void *names, uint64_t *name_offs, void *coms,
                                 uint64_t *com_offs, uint8_t *flags)
{
    if (!fq || !b) { slx_set_error("slx_fastq_to_host: null argument"); return SLX_EINVAL; }
    if (b->n_reads <= 0 || b->n_reads != fq->last.n_reads || b->d_bases != fq->last.d_bases || b->d_offs != fq->last.d_offs) { slx_set_error("slx_fastq_to_host: not the reader's last batch"); return SLX_EINVAL; }
    SLX_HIPCHK(hipSetDevice(fq->device));
    hipStream_t st = fq->st;
    const size_t n = (size_t)b->n_reads;
    auto down = [&](void *dst, const void *src, size_t bytes) { return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
    SLX_HIPCHK(down(offs, b->d_offs, 8 * (n + 1))); SLX_HIPCHK(down(name_offs, b->d_name_offs, 8 * (n + 1))); SLX_HIPCHK(down(com_offs, b->d_com_offs, 8 * (n + 1)));
    SLX_HIPCHK(down(flags, b->d_flags, n));
    SLX_HIPCHK(down(bases, b->d_bases, fq->tot_b)); SLX_HIPCHK(down(quals, b->d_quals, fq->tot_b));
    SLX_HIPCHK(down(names, b->d_names, fq->tot_n)); SLX_HIPCHK(down(coms, b->d_coms, fq->tot_c));
    SLX_HIPCHK(slx_wait_stream(st));
    return SLX_OK;
}
