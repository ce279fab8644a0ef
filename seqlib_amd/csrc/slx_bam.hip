// slx_bam.hip -- the BamReader path of libseqlib_amd.so (include/seqlib_amd_bam.h): BGZF members inflated, CRC-checked, cut into records and unpacked
// to the aligner's input on the GPU.  The host parses the member chain (18-byte headers, BSIZE, CRC32 + ISIZE trailers) and the BAM header; everything
// that touches the bulk of the bytes is a kernel:
//   k_bgzf_inflate   one wave per member, straight to the member's place in one contiguous stream (exclusive scan of ISIZE)      dev_inflate.h
//   k_bgzf_crc       one wave per member, a slice per lane, slices combined by x^(8n) mod P                                     dev_inflate.h
//   k_bam_guess / k_bam_round / k_bam_scan / k_bam_fill   record starts by speculate / verify / repair, one lane per chunk      dev_bamidx.h
//   k_bam_keep / k_bam_unpack   flag filter, 4-bit sequence -> ASCII (reverse complement on request), one wave per record
// Waves take members / records by a static map (wave w of the grid owns item w): there is no work queue here, so the queue hazards of DESIGN.md
// section 4 do not arise.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "slx_internal.h"
#include "seqlib_amd_bam.h"
#include "dev_inflate.h"
#include "dev_bamidx.h"

#define BAM_HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { slx_set_error("HIP error %s at %s:%d", hipGetErrorString(e_), __FILE__, __LINE__); return SLX_ENODEVICE; } } while (0)
#define BAM_CHK(x) do { const int rc_ = (x); if (rc_ != SLX_OK) return rc_; } while (0)

struct bam_mdesc { uint64_t in_off, out_off; uint32_t in_len, isize, crc, pad; };

// ------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void k_bgzf_inflate(const uint8_t *comp, uint64_t comp_bytes, const bam_mdesc *m, int n, uint8_t *out, uint64_t out_bytes, uint32_t *err)
{
    __shared__ inf_tables tabs[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int idx = blockIdx.x * 4 + wave;
    if (idx >= n) return;
    const bam_mdesc d = m[idx];
    int e;
    if (d.in_off + d.in_len > comp_bytes || d.out_off + d.isize > out_bytes) e = INF_E_DESC;
    else e = inf_member(comp + d.in_off, d.in_len, out + d.out_off, d.isize, &tabs[wave], lane, 64);
    if (lane == 0) err[idx] = (uint32_t)e;
}

__global__ __launch_bounds__(256) void k_bgzf_crc(const bam_mdesc *m, int n, const uint8_t *out, uint64_t out_bytes, uint32_t *err)
{
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = inf_crc_entry(threadIdx.x);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int idx = blockIdx.x * 4 + wave;
    if (idx >= n) return;
    const bam_mdesc d = m[idx];
    if (err[idx] != INF_OK || d.out_off + d.isize > out_bytes) return;
    uint32_t c = inf_crc_part(tab, out + d.out_off, d.isize, lane, 64);
    for (int o = 32; o; o >>= 1) c ^= __shfl_xor(c, o, 64);
    if (lane == 0 && c != d.crc) err[idx] = INF_E_CRC;
}

// state of the index: [0] records, [1] repaired chunks, [2] lowest start of a record with block_size < 32, [3] end of the last whole record, [4] changed (rounds)
__global__ void k_bam_guess(const uint8_t *s, uint64_t n, uint64_t chunk, uint64_t K, int32_t n_ref, int idx_fail, uint64_t *guess0, uint64_t *used, uint64_t *exit_, uint32_t *count)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const uint64_t cs = k * chunk, ce = cs + chunk < n ? cs + chunk : n;
    uint64_t g = 0;
    if (k) {
        g = bidx_guess(s, n, cs, ce, n_ref);
        if (idx_fail) g = g == BIDX_NONE ? cs : g + 1;
    }
    guess0[k] = g; used[k] = g;
    uint32_t c = 0;
    uint64_t ex = BIDX_NONE;
    if (g != BIDX_NONE) ex = bidx_walk(s, n, g, ce, c, nullptr, nullptr);
    exit_[k] = ex; count[k] = c;
}

__global__ void k_bam_round(const uint8_t *s, uint64_t n, uint64_t chunk, uint64_t K, uint64_t *used, const uint64_t *exit_prev, uint64_t *exit_next, uint32_t *count,
                            unsigned long long *state)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    if (k == 0) { exit_next[0] = exit_prev[0]; return; }
    if (bidx_round(s, n, chunk, k, used, exit_prev, exit_next, count)) state[4] = 1;
}

// exclusive sum of the chunks' record counts: one block (K is the stream's size / 64 KiB)
__global__ __launch_bounds__(1024) void k_bam_scan(const uint32_t *count, uint64_t *base, uint64_t K, unsigned long long *state)
{
    __shared__ uint64_t part[1024];
    const uint64_t per = (K + 1023) / 1024, a = threadIdx.x * per, e = a + per < K ? a + per : K;
    uint64_t sum = 0;
    for (uint64_t i = a; i < e; ++i) sum += count[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint64_t v = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = part[threadIdx.x] - sum;
    for (uint64_t i = a; i < e; ++i) { base[i] = run; run += count[i]; }
    if (threadIdx.x == 1023) state[0] = part[1023];
}

__global__ void k_bam_fill(const uint8_t *s, uint64_t n, uint64_t chunk, uint64_t K, const uint64_t *exit_, const uint64_t *guess0, const uint64_t *base, uint64_t *rec,
                           unsigned long long *state)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const uint64_t cs = k * chunk, ce = cs + chunk < n ? cs + chunk : n;
    const uint64_t entry = k ? exit_[k - 1] : 0;
    uint32_t c;
    uint64_t bad = BIDX_NONE;
    const uint64_t ex = bidx_walk(s, n, entry, ce, c, rec + base[k], &bad);
    if (k && !bidx_guess_right(guess0[k], entry, c)) atomicAdd(&state[1], 1ull);
    if (bad != BIDX_NONE) atomicMin(&state[2], (unsigned long long)bad);
    if (k == K - 1) {
        const uint64_t end = ex & ~BIDX_CUT;
        state[3] = end;
        rec[base[k] + c] = end;
    }
}

// per record: kept (none of skip_flags) and its sequence length; a record whose fields do not fit its block_size is reported through state[2]
__global__ void k_bam_keep(const uint8_t *s, const uint64_t *rec, uint64_t n_rec, uint32_t skip, unsigned long long *keep, unsigned long long *blen, unsigned long long *state)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rec) return;
    if (r == n_rec) { keep[r] = 0; blen[r] = 0; return; }
    const uint8_t *h = s + rec[r];
    const uint64_t bs = bidx_u32(h);
    const uint32_t l_name = h[12], n_cig = (uint32_t)h[16] | (uint32_t)h[17] << 8, flag = (uint32_t)h[18] | (uint32_t)h[19] << 8;
    const int32_t l_seq = (int32_t)bidx_u32(h + 20);
    const bool k = (flag & skip) == 0;
    uint64_t len = 0;
    if (k) {
        if (l_seq < 0 || 32ull + l_name + 4ull * n_cig + (((uint64_t)l_seq + 1) >> 1) > bs) atomicMin(&state[2], (unsigned long long)rec[r]);
        else len = (uint64_t)l_seq;
    }
    keep[r] = k; blen[r] = len;
}

__global__ __launch_bounds__(256) void k_bam_unpack(const uint8_t *s, const uint64_t *rec, uint64_t n_rec, const unsigned long long *kidx, const unsigned long long *boff,
                                                    int original_strand, uint8_t *bases, uint64_t *offs, int64_t *map)
{
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n_rec) return;
    if (r == 0 && lane == 0) offs[kidx[n_rec]] = boff[n_rec];
    if (kidx[r + 1] == kidx[r]) return;                         // dropped
    const uint64_t ri = kidx[r], b0 = boff[r], len = boff[r + 1] - b0;
    const uint8_t *h = s + rec[r];
    const uint32_t l_name = h[12], n_cig = (uint32_t)h[16] | (uint32_t)h[17] << 8, flag = (uint32_t)h[18] | (uint32_t)h[19] << 8;
    const uint8_t *seq = h + 36 + l_name + 4ull * n_cig;
    const bool rev = original_strand && (flag & 0x10);
    if (lane == 0) { offs[ri] = b0; map[ri] = (int64_t)r; }
    for (uint64_t i = lane; i < len; i += 64) {
        const uint64_t j = rev ? len - 1 - i : i;
        uint32_t c = (seq[j >> 1] >> ((~j & 1) << 2)) & 15u;
        if (rev) c = ((c & 1) << 3) | ((c & 2) << 1) | ((c & 4) >> 1) | ((c & 8) >> 3);          // A=1 C=2 G=4 T=8: the IUPAC complement reverses the four bits
        bases[b0 + i] = (uint8_t)"=ACMGRSVTWYHKDBN"[c];
    }
}

// ------------------------------------------------------------------ host: the member chain
struct BamFile {
    int fd = -1;
    const uint8_t *map = nullptr;
    uint64_t size = 0;
    std::vector<slx_bam_member> mem;
    int has_eof = 0;
    std::string path;
    ~BamFile() { close_(); }
    void close_()
    {
        if (map) munmap((void *)map, size);
        if (fd >= 0) ::close(fd);
        map = nullptr; fd = -1;
    }
};

static int bam_scan(const char *path, BamFile &f)
{
    if (!path) { slx_set_error("BAM reader: path is null"); return SLX_EINVAL; }
    f.path = path;
    f.fd = ::open(path, O_RDONLY);
    if (f.fd < 0) { slx_set_error("BAM reader: cannot open '%s'", path); return SLX_EIO; }
    struct stat sb;
    if (fstat(f.fd, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size < 28) { slx_set_error("BAM reader: '%s' is not a BGZF file (shorter than one member, or not a regular file)", path); return SLX_EIO; }
    f.size = (uint64_t)sb.st_size;
    void *p = mmap(nullptr, f.size, PROT_READ, MAP_PRIVATE, f.fd, 0);
    if (p == MAP_FAILED) { slx_set_error("BAM reader: cannot map '%s'", path); return SLX_EIO; }
    f.map = (const uint8_t *)p;
    const uint8_t *b = f.map;
    uint64_t o = 0;
    while (o < f.size) {
        if (o + 18 > f.size) { slx_set_error("BGZF: '%s' is truncated inside the member header at offset %llu", path, (unsigned long long)o); return SLX_EIO; }
        if (b[o] != 0x1f || b[o + 1] != 0x8b || b[o + 2] != 8 || b[o + 3] != 4) {
            slx_set_error(o ? "BGZF: '%s' has no member header at offset %llu (broken chain: bad magic; CRAM and SAM text are not read)" : "BGZF: '%s' does not start with a BGZF member at offset %llu (bad magic; CRAM and SAM text are not read)", path, (unsigned long long)o);
            return SLX_EIO;
        }
        const uint32_t xlen = (uint32_t)b[o + 10] | (uint32_t)b[o + 11] << 8;
        if (o + 12 + xlen > f.size) { slx_set_error("BGZF: '%s' is truncated inside the extra field at offset %llu", path, (unsigned long long)o); return SLX_EIO; }
        int64_t bsize = -1;
        for (uint64_t x = o + 12; x + 4 <= o + 12 + xlen;) {
            const uint32_t slen = (uint32_t)b[x + 2] | (uint32_t)b[x + 3] << 8;
            if (b[x] == 'B' && b[x + 1] == 'C' && slen == 2 && x + 6 <= o + 12 + xlen) { bsize = (int64_t)((uint32_t)b[x + 4] | (uint32_t)b[x + 5] << 8); break; }
            x += 4 + slen;
        }
        if (bsize < 0) { slx_set_error("BGZF: '%s': the member at offset %llu has no BC extra field", path, (unsigned long long)o); return SLX_EIO; }
        const uint64_t total = (uint64_t)bsize + 1, data_off = 12 + xlen;
        if (total < data_off + 8) { slx_set_error("BGZF: '%s': BSIZE of the member at offset %llu is smaller than its header and trailer", path, (unsigned long long)o); return SLX_EIO; }
        if (o + total > f.size) { slx_set_error("BGZF: '%s' is truncated inside the member at offset %llu (BSIZE %llu)", path, (unsigned long long)o, (unsigned long long)bsize); return SLX_EIO; }
        slx_bam_member m;
        m.file_off = o; m.data_off = (uint32_t)data_off; m.data_len = (uint32_t)(total - data_off - 8);
        m.crc32 = bidx_u32(b + o + total - 8); m.isize = bidx_u32(b + o + total - 4);
        if (m.isize > 65536) { slx_set_error("BGZF: '%s': ISIZE %u of the member at offset %llu is above 64 KiB", path, m.isize, (unsigned long long)o); return SLX_EIO; }
        f.mem.push_back(m);
        o += total;
    }
    const slx_bam_member &l = f.mem.back();
    f.has_eof = l.isize == 0 && l.data_off + l.data_len + 8 == 28;
    return SLX_OK;
}

extern "C" int slx_bam_scan_members(const char *path, slx_bam_member **members, int64_t *n_members, int *has_eof)
{
    if (!members || !n_members) { slx_set_error("slx_bam_scan_members: null output"); return SLX_EINVAL; }
    BamFile f;
    BAM_CHK(bam_scan(path, f));
    slx_bam_member *m = (slx_bam_member *)malloc(sizeof(slx_bam_member) * f.mem.size());
    if (!m) { slx_set_error("out of memory"); return SLX_ENOMEM; }
    memcpy(m, f.mem.data(), sizeof(slx_bam_member) * f.mem.size());
    *members = m; *n_members = (int64_t)f.mem.size();
    if (has_eof) *has_eof = f.has_eof;
    return SLX_OK;
}
extern "C" void slx_bam_members_free(slx_bam_member *members) { free(members); }

// ------------------------------------------------------------------ host: the device side
struct BamDBuf {
    void *p = nullptr; size_t cap = 0;
    int ensure(size_t n, hipStream_t st = nullptr, size_t keep = 0)       // keep: leading bytes that survive a growth
    {
        if (n <= cap) return SLX_OK;
        const size_t want = n + n / 4 + 256;
        void *q = nullptr;
        if (hipMalloc(&q, want) != hipSuccess) { (void)hipGetLastError(); slx_set_error("BAM reader: cannot allocate %zu bytes of HBM", want); return SLX_ENOMEM; }
        if (keep && p) { BAM_HIPCHK(hipMemcpyAsync(q, p, keep, hipMemcpyDeviceToDevice, st)); BAM_HIPCHK(hipStreamSynchronize(st)); }
        if (p) (void)hipFree(p);
        p = q; cap = want;
        return SLX_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <typename T> T *as() const { return (T *)p; }
};
struct BamHBuf {
    void *p = nullptr; size_t cap = 0;
    int ensure(size_t n)
    {
        if (n <= cap) return SLX_OK;
        const size_t want = n + n / 4 + 256;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); p = nullptr; slx_set_error("BAM reader: cannot pin %zu bytes", want); return SLX_ENOMEM; }
        cap = want;
        return SLX_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    template <typename T> T *as() const { return (T *)p; }
};

struct slx_bam {
    BamFile f;
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev[8] = {};
    std::string text;
    std::vector<std::string> ref_names;
    std::vector<int64_t> ref_lens;
    int64_t first_member = 0, next_member = 0;
    std::vector<uint8_t> carry0, carry;
    uint64_t chunk_bytes = 65536;
    int idx_fail = 0;
    BamDBuf d_comp, d_desc, d_err, d_out, d_guess, d_used, d_exit_a, d_exit_b, d_count, d_base, d_state, d_rec, d_keep, d_blen, d_kidx, d_boff, d_tmp, d_bases, d_offs, d_map;
    BamHBuf h_comp, h_desc, h_err, h_out, h_rec, h_state, h_map;
    int64_t c_members_done = 0, c_repaired = 0, c_rounds = 0, c_records = 0;
    float us[4] = {0, 0, 0, 0};
    std::vector<BamDBuf *> dbufs() { return {&d_comp, &d_desc, &d_err, &d_out, &d_guess, &d_used, &d_exit_a, &d_exit_b, &d_count, &d_base, &d_state, &d_rec, &d_keep, &d_blen, &d_kidx, &d_boff, &d_tmp, &d_bases, &d_offs, &d_map}; }
    std::vector<BamHBuf *> hbufs() { return {&h_comp, &h_desc, &h_err, &h_out, &h_rec, &h_state, &h_map}; }
};

static const char *inf_errtext(uint32_t e)
{
    switch (e) {
    case INF_E_EOF: return "the deflate stream runs past the member's compressed bytes";
    case INF_E_BTYPE: return "invalid deflate block type";
    case INF_E_STORED: return "stored block with LEN / NLEN mismatch or bytes past the member";
    case INF_E_CODE: return "invalid, incomplete or over-subscribed Huffman code";
    case INF_E_SYM: return "invalid length or distance symbol";
    case INF_E_DIST: return "match distance beyond the output so far";
    case INF_E_OUT: return "output passes ISIZE";
    case INF_E_ISIZE: return "stream ends before ISIZE bytes";
    case INF_E_CRC: return "CRC32 mismatch";
    case INF_E_DESC: return "member descriptor outside the buffers";
    }
    return "unknown error";
}

static int bam_dev_init(slx_bam *rd, int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        slx_set_error("no HIP device: the BAM reader inflates and indexes on MI355X only (no CPU fallback)");
        return SLX_ENODEVICE;
    }
    if (device < 0) { BAM_HIPCHK(hipGetDevice(&device)); }
    if (device >= ndev) { slx_set_error("BAM reader: device %d is not one of the %d visible", device, ndev); return SLX_EINVAL; }
    BAM_HIPCHK(hipSetDevice(device));
    rd->device = device;
    BAM_HIPCHK(hipStreamCreateWithFlags(&rd->st, hipStreamNonBlocking));
    for (auto &e : rd->ev) BAM_HIPCHK(hipEventCreate(&e));
    return SLX_OK;
}

static void bam_dev_free(slx_bam *rd)
{
    if (rd->st) {
        (void)hipSetDevice(rd->device);
        (void)hipStreamSynchronize(rd->st);
    }
    for (BamDBuf *b : rd->dbufs()) b->release();
    for (BamHBuf *b : rd->hbufs()) b->release();
    for (auto &e : rd->ev) if (e) (void)hipEventDestroy(e);
    if (rd->st) (void)hipStreamDestroy(rd->st);
    rd->st = nullptr;
}

static float ev_us(hipEvent_t a, hipEvent_t b) { float ms = 0; return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms * 1000.f : 0.f; }

// members [a, b) inflated to d_out[dst_off ..), CRC-checked; d_out holds out_bytes.  Returns after the stream has drained.
static int bam_inflate_span(slx_bam *rd, int64_t a, int64_t b, uint64_t dst_off, uint64_t out_bytes)
{
    const int n = (int)(b - a);
    if (n <= 0) return SLX_OK;
    uint64_t comp = 0;
    for (int64_t i = a; i < b; ++i) comp += rd->f.mem[i].data_len;
    BAM_CHK(rd->h_comp.ensure(comp + 8)); BAM_CHK(rd->d_comp.ensure(comp + 8));
    BAM_CHK(rd->h_desc.ensure(sizeof(bam_mdesc) * n)); BAM_CHK(rd->d_desc.ensure(sizeof(bam_mdesc) * n));
    BAM_CHK(rd->h_err.ensure(4 * (size_t)n)); BAM_CHK(rd->d_err.ensure(4 * (size_t)n));
    bam_mdesc *d = rd->h_desc.as<bam_mdesc>();
    uint64_t ci = 0, oo = dst_off;
    for (int64_t i = a; i < b; ++i) {
        const slx_bam_member &m = rd->f.mem[i];
        memcpy(rd->h_comp.as<uint8_t>() + ci, rd->f.map + m.file_off + m.data_off, m.data_len);
        d[i - a] = bam_mdesc{ci, oo, m.data_len, m.isize, m.crc32, 0};
        ci += m.data_len; oo += m.isize;
    }
    if (oo > out_bytes) { slx_set_error("BAM reader: internal: span of %llu bytes does not fit %llu", (unsigned long long)oo, (unsigned long long)out_bytes); return SLX_EINTERNAL; }
    hipStream_t st = rd->st;
    BAM_HIPCHK(hipMemcpyAsync(rd->d_comp.p, rd->h_comp.p, comp, hipMemcpyHostToDevice, st));
    BAM_HIPCHK(hipMemcpyAsync(rd->d_desc.p, rd->h_desc.p, sizeof(bam_mdesc) * n, hipMemcpyHostToDevice, st));
    BAM_HIPCHK(hipEventRecord(rd->ev[0], st));
    k_bgzf_inflate<<<(n + 3) / 4, 256, 0, st>>>(rd->d_comp.as<uint8_t>(), comp, rd->d_desc.as<bam_mdesc>(), n, rd->d_out.as<uint8_t>(), out_bytes, rd->d_err.as<uint32_t>());
    BAM_HIPCHK(hipGetLastError());
    BAM_HIPCHK(hipEventRecord(rd->ev[1], st));
    k_bgzf_crc<<<(n + 3) / 4, 256, 0, st>>>(rd->d_desc.as<bam_mdesc>(), n, rd->d_out.as<uint8_t>(), out_bytes, rd->d_err.as<uint32_t>());
    BAM_HIPCHK(hipGetLastError());
    BAM_HIPCHK(hipEventRecord(rd->ev[2], st));
    BAM_HIPCHK(hipMemcpyAsync(rd->h_err.p, rd->d_err.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    BAM_HIPCHK(slx_wait_stream(st));
    rd->us[0] += ev_us(rd->ev[0], rd->ev[1]); rd->us[1] += ev_us(rd->ev[1], rd->ev[2]);
    rd->c_members_done += n;
    const uint32_t *err = rd->h_err.as<uint32_t>();
    for (int i = 0; i < n; ++i)
        if (err[i]) {
            slx_set_error("BGZF: '%s': the member at file offset %llu does not inflate: %s", rd->f.path.c_str(), (unsigned long long)rd->f.mem[a + i].file_off, inf_errtext(err[i]));
            return SLX_EIO;
        }
    return SLX_OK;
}

// record starts of d_out[0, n): d_rec gets n_rec + 1 offsets (the last one = end of the last whole record)
static int bam_index(slx_bam *rd, uint64_t n, int32_t n_ref, uint64_t *n_rec, uint64_t *end, uint64_t *repaired)
{
    hipStream_t st = rd->st;
    const uint64_t chunk = rd->chunk_bytes, K = (n + chunk - 1) / chunk;
    *n_rec = 0; *end = 0; *repaired = 0;
    if (!K) return SLX_OK;
    for (BamDBuf *b : {&rd->d_guess, &rd->d_used, &rd->d_exit_a, &rd->d_exit_b, &rd->d_base}) BAM_CHK(b->ensure(8 * K));
    BAM_CHK(rd->d_count.ensure(4 * K)); BAM_CHK(rd->d_state.ensure(64)); BAM_CHK(rd->h_state.ensure(64));
    unsigned long long *hs = rd->h_state.as<unsigned long long>(), *ds = rd->d_state.as<unsigned long long>();
    hs[0] = 0; hs[1] = 0; hs[2] = ~0ull; hs[3] = 0; hs[4] = 0;
    BAM_HIPCHK(hipMemcpyAsync(ds, hs, 40, hipMemcpyHostToDevice, st));
    BAM_HIPCHK(hipEventRecord(rd->ev[3], st));
    const uint8_t *s = rd->d_out.as<uint8_t>();
    const unsigned grid = (unsigned)((K + 63) / 64);
    uint64_t *ex_a = rd->d_exit_a.as<uint64_t>(), *ex_b = rd->d_exit_b.as<uint64_t>();
    k_bam_guess<<<grid, 64, 0, st>>>(s, n, chunk, K, n_ref, rd->idx_fail, rd->d_guess.as<uint64_t>(), rd->d_used.as<uint64_t>(), ex_a, rd->d_count.as<uint32_t>());
    BAM_HIPCHK(hipGetLastError());
    for (uint64_t round = 0; K > 1; ++round) {
        if (round > K) { slx_set_error("BAM reader: internal: the record index did not settle in %llu rounds", (unsigned long long)K); return SLX_EINTERNAL; }
        if (round) BAM_HIPCHK(hipMemsetAsync(ds + 4, 0, 8, st));
        k_bam_round<<<grid, 64, 0, st>>>(s, n, chunk, K, rd->d_used.as<uint64_t>(), ex_a, ex_b, rd->d_count.as<uint32_t>(), ds);
        BAM_HIPCHK(hipGetLastError());
        BAM_HIPCHK(hipMemcpyAsync(hs + 4, ds + 4, 8, hipMemcpyDeviceToHost, st));
        BAM_HIPCHK(slx_wait_stream(st));
        std::swap(ex_a, ex_b);
        ++rd->c_rounds;
        if (!hs[4]) break;
    }
    k_bam_scan<<<1, 1024, 0, st>>>(rd->d_count.as<uint32_t>(), rd->d_base.as<uint64_t>(), K, ds);
    BAM_HIPCHK(hipGetLastError());
    BAM_HIPCHK(hipMemcpyAsync(hs, ds, 8, hipMemcpyDeviceToHost, st));
    BAM_HIPCHK(slx_wait_stream(st));
    const uint64_t nr = hs[0];
    BAM_CHK(rd->d_rec.ensure(8 * (nr + 1)));
    k_bam_fill<<<grid, 64, 0, st>>>(s, n, chunk, K, ex_a, rd->d_guess.as<uint64_t>(), rd->d_base.as<uint64_t>(), rd->d_rec.as<uint64_t>(), ds);
    BAM_HIPCHK(hipGetLastError());
    BAM_HIPCHK(hipEventRecord(rd->ev[4], st));
    BAM_HIPCHK(hipMemcpyAsync(hs, ds, 32, hipMemcpyDeviceToHost, st));
    BAM_HIPCHK(slx_wait_stream(st));
    rd->us[2] += ev_us(rd->ev[3], rd->ev[4]);
    if (hs[2] != ~0ull) { slx_set_error("BAM: '%s': a record's block_size is below its 32 fixed bytes (inflated offset %llu of the batch)", rd->f.path.c_str(), hs[2]); return SLX_EIO; }
    *n_rec = nr; *end = hs[3]; *repaired = hs[1];
    return SLX_OK;
}

// ------------------------------------------------------------------ C-ABI
static int bam_parse_header(slx_bam *rd)
{
    // members are inflated until the header (magic, text, dictionary) is whole; what follows it in the last of them is the first carry
    const int64_t nm = (int64_t)rd->f.mem.size();
    std::vector<uint8_t> h;
    int64_t b = 0;
    auto need = [&](uint64_t upto) -> int {
        while (h.size() < upto) {
            if (b >= nm) { slx_set_error("BAM: '%s': the file ends inside the BAM header", rd->f.path.c_str()); return SLX_EIO; }
            int64_t e = b; uint64_t bytes = 0;
            while (e < nm && (e == b || bytes < upto - h.size())) bytes += rd->f.mem[e++].isize;
            BAM_CHK(rd->d_out.ensure(bytes + 8));
            BAM_CHK(bam_inflate_span(rd, b, e, 0, bytes));
            const size_t at = h.size();
            h.resize(at + bytes);
            if (bytes) { BAM_HIPCHK(hipMemcpyAsync(h.data() + at, rd->d_out.p, bytes, hipMemcpyDeviceToHost, rd->st)); BAM_HIPCHK(hipStreamSynchronize(rd->st)); }
            b = e;
        }
        return SLX_OK;
    };
    BAM_CHK(need(12));
    if (memcmp(h.data(), "BAM\1", 4) != 0) { slx_set_error("BAM: '%s' is BGZF but does not hold a BAM stream (bad magic; SAM text and CRAM are not read)", rd->f.path.c_str()); return SLX_EIO; }
    const uint64_t l_text = bidx_u32(h.data() + 4);
    if (l_text > (1ull << 31)) { slx_set_error("BAM: '%s': header text length %llu", rd->f.path.c_str(), (unsigned long long)l_text); return SLX_EIO; }
    BAM_CHK(need(12 + l_text));
    rd->text.assign((const char *)h.data() + 8, l_text);
    while (!rd->text.empty() && rd->text.back() == '\0') rd->text.pop_back();
    const int32_t n_ref = (int32_t)bidx_u32(h.data() + 8 + l_text);
    if (n_ref < 0) { slx_set_error("BAM: '%s': negative reference count", rd->f.path.c_str()); return SLX_EIO; }
    uint64_t p = 12 + l_text;
    for (int32_t i = 0; i < n_ref; ++i) {
        BAM_CHK(need(p + 4));
        const uint64_t l_name = bidx_u32(h.data() + p);
        if (l_name < 1 || l_name > (1u << 20)) { slx_set_error("BAM: '%s': reference %d has name length %llu", rd->f.path.c_str(), i, (unsigned long long)l_name); return SLX_EIO; }
        BAM_CHK(need(p + 4 + l_name + 4));
        rd->ref_names.emplace_back((const char *)h.data() + p + 4, strnlen((const char *)h.data() + p + 4, l_name));
        rd->ref_lens.push_back((int64_t)bidx_u32(h.data() + p + 4 + l_name));
        p += 8 + l_name;
    }
    rd->first_member = b;
    rd->carry0.assign(h.begin() + p, h.end());
    return SLX_OK;
}

extern "C" int slx_bam_open(const char *path, int device, slx_bam **out)
{
    if (!out) { slx_set_error("slx_bam_open: rd is null"); return SLX_EINVAL; }
    *out = nullptr;
    slx_bam *rd = new slx_bam();
    int rc = bam_scan(path, rd->f);
    if (rc == SLX_OK) rc = bam_dev_init(rd, device);
    if (rc == SLX_OK) rc = bam_parse_header(rd);
    if (rc != SLX_OK) { bam_dev_free(rd); delete rd; return rc; }
    if (!rd->f.has_eof) fprintf(stderr, "[W::slx_bam_open] EOF marker is absent. The input '%s' is probably truncated\n", path);
    rd->next_member = rd->first_member; rd->carry = rd->carry0;
    rd->us[0] = rd->us[1] = 0;
    *out = rd;
    return SLX_OK;
}

extern "C" void slx_bam_close(slx_bam *rd)
{
    if (!rd) return;
    bam_dev_free(rd);
    delete rd;
}

extern "C" int slx_bam_header(const slx_bam *rd, const char **text, int64_t *l_text, int *n_ref)
{
    if (!rd) { slx_set_error("slx_bam_header: reader is null"); return SLX_EINVAL; }
    if (text) *text = rd->text.c_str();
    if (l_text) *l_text = (int64_t)rd->text.size();
    if (n_ref) *n_ref = (int)rd->ref_names.size();
    return SLX_OK;
}
extern "C" const char *slx_bam_ref_name(const slx_bam *rd, int i) { return rd && i >= 0 && i < (int)rd->ref_names.size() ? rd->ref_names[i].c_str() : nullptr; }
extern "C" int64_t slx_bam_ref_len(const slx_bam *rd, int i) { return rd && i >= 0 && i < (int)rd->ref_lens.size() ? rd->ref_lens[i] : -1; }

extern "C" int slx_bam_rewind(slx_bam *rd)
{
    if (!rd) { slx_set_error("slx_bam_rewind: reader is null"); return SLX_EINVAL; }
    rd->next_member = rd->first_member; rd->carry = rd->carry0;
    return SLX_OK;
}

extern "C" int slx_bam_set(slx_bam *rd, const char *key, int64_t value)
{
    if (!rd || !key) { slx_set_error("slx_bam_set: null argument"); return SLX_EINVAL; }
    const std::string k(key);
    if (k == "chunk_bytes" && value >= 64 && value <= (1ll << 30)) { rd->chunk_bytes = (uint64_t)value; return SLX_OK; }
    if (k == "idx_fail" && (value == 0 || value == 1)) { rd->idx_fail = (int)value; return SLX_OK; }
    slx_set_error("slx_bam_set: unknown key or value out of range: %s = %lld", key, (long long)value);
    return SLX_EINVAL;
}

extern "C" int64_t slx_bam_counter(const slx_bam *rd, const char *name)
{
    if (!rd || !name) return -1;
    const std::string k(name);
    if (k == "members") return (int64_t)rd->f.mem.size();
    if (k == "members_done") return rd->c_members_done;
    if (k == "repaired_chunks") return rd->c_repaired;
    if (k == "index_rounds") return rd->c_rounds;
    if (k == "missing_eof") return rd->f.has_eof ? 0 : 1;
    if (k == "records") return rd->c_records;
    if (k == "us_inflate") return (int64_t)rd->us[0];
    if (k == "us_crc") return (int64_t)rd->us[1];
    if (k == "us_index") return (int64_t)rd->us[2];
    if (k == "us_unpack") return (int64_t)rd->us[3];
    return -1;
}

extern "C" int slx_bam_next(slx_bam *rd, int64_t max_bytes, slx_bam_batch *out)
{
    if (!rd || !out) { slx_set_error("slx_bam_next: null argument"); return SLX_EINVAL; }
    memset(out, 0, sizeof *out);
    BAM_HIPCHK(hipSetDevice(rd->device));
    const int64_t nm = (int64_t)rd->f.mem.size();
    const int64_t a = rd->next_member;
    rd->us[0] = rd->us[1] = rd->us[2] = 0;
    if (a >= nm && rd->carry.empty()) return SLX_OK;
    if (max_bytes < 1) max_bytes = 1;
    hipStream_t st = rd->st;
    uint64_t total = rd->carry.size();
    BAM_CHK(rd->d_out.ensure(total + 8));
    if (total) BAM_HIPCHK(hipMemcpyAsync(rd->d_out.p, rd->carry.data(), total, hipMemcpyHostToDevice, st));
    BAM_HIPCHK(hipStreamSynchronize(st));
    int64_t done = a, b = a;
    uint64_t n_rec = 0, end = 0, repaired = 0;
    for (;;) {
        // the span: at least one member, then while it stays within max_bytes; a span without one whole record doubles
        uint64_t bytes = total;
        if (b == done) { while (b < nm && (b == done || bytes + rd->f.mem[b].isize <= (uint64_t)max_bytes)) bytes += rd->f.mem[b++].isize; }
        else bytes = total;
        uint64_t span = 0;
        for (int64_t i = done; i < b; ++i) span += rd->f.mem[i].isize;
        BAM_CHK(rd->d_out.ensure(total + span + 8, st, total));
        BAM_CHK(bam_inflate_span(rd, done, b, total, total + span));
        total += span; done = b;
        BAM_CHK(bam_index(rd, total, (int32_t)rd->ref_names.size(), &n_rec, &end, &repaired));
        if (n_rec || done >= nm) break;
        b = std::min(nm, done + std::max<int64_t>(1, done - a));
    }
    if (!n_rec && total) {
        slx_set_error("BAM: '%s' ends inside a record (%llu bytes after the last whole record)", rd->f.path.c_str(), (unsigned long long)total);
        return SLX_EIO;
    }
    rd->next_member = done;
    BAM_CHK(rd->h_out.ensure(end + 8)); BAM_CHK(rd->h_rec.ensure(8 * (n_rec + 1)));
    if (end) BAM_HIPCHK(hipMemcpyAsync(rd->h_out.p, rd->d_out.p, end, hipMemcpyDeviceToHost, st));
    if (n_rec) BAM_HIPCHK(hipMemcpyAsync(rd->h_rec.p, rd->d_rec.p, 8 * (n_rec + 1), hipMemcpyDeviceToHost, st));
    rd->carry.resize(total - end);
    if (total > end) BAM_HIPCHK(hipMemcpyAsync(rd->carry.data(), rd->d_out.as<uint8_t>() + end, total - end, hipMemcpyDeviceToHost, st));
    BAM_HIPCHK(slx_wait_stream(st));
    rd->c_repaired += (int64_t)repaired; rd->c_records += (int64_t)n_rec;
    out->n_records = (int64_t)n_rec; out->n_bytes = (int64_t)end;
    out->stream = rd->h_out.as<uint8_t>(); out->rec_off = rd->h_rec.as<uint64_t>();
    out->d_stream = rd->d_out.p; out->d_rec_off = rd->d_rec.p;
    out->n_members = done - a; out->n_repaired_chunks = (int64_t)repaired;
    return SLX_OK;
}

extern "C" int slx_bam_reads_device(slx_bam *rd, const slx_bam_batch *batch, int skip_flags, int original_strand, void **d_bases, void **d_offs, int64_t *n_reads,
                                    const int64_t **rec_of_read)
{
    if (!rd || !batch || !d_bases || !d_offs || !n_reads) { slx_set_error("slx_bam_reads_device: null argument"); return SLX_EINVAL; }
    if (batch->d_stream != rd->d_out.p || batch->d_rec_off != rd->d_rec.p) { slx_set_error("slx_bam_reads_device: the batch is not the reader's current one"); return SLX_EINVAL; }
    BAM_HIPCHK(hipSetDevice(rd->device));
    hipStream_t st = rd->st;
    const uint64_t n = (uint64_t)batch->n_records;
    typedef unsigned long long ull;
    for (BamDBuf *b : {&rd->d_keep, &rd->d_blen, &rd->d_kidx, &rd->d_boff}) BAM_CHK(b->ensure(8 * (n + 1)));
    BAM_CHK(rd->d_state.ensure(64)); BAM_CHK(rd->h_state.ensure(64));
    ull *hs = rd->h_state.as<ull>(), *ds = rd->d_state.as<ull>();
    hs[2] = ~0ull;
    BAM_HIPCHK(hipMemcpyAsync(ds + 2, hs + 2, 8, hipMemcpyHostToDevice, st));
    BAM_HIPCHK(hipEventRecord(rd->ev[5], st));
    const uint8_t *s = rd->d_out.as<uint8_t>();
    const uint64_t *rec = rd->d_rec.as<uint64_t>();
    k_bam_keep<<<(unsigned)((n + 1 + 255) / 256), 256, 0, st>>>(s, rec, n, (uint32_t)skip_flags & 0xffffu, rd->d_keep.as<ull>(), rd->d_blen.as<ull>(), ds);
    BAM_HIPCHK(hipGetLastError());
    size_t tb = 0, tb2 = 0;
    BAM_HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, rd->d_keep.as<ull>(), rd->d_kidx.as<ull>(), (int)(n + 1), st));
    BAM_HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, rd->d_blen.as<ull>(), rd->d_boff.as<ull>(), (int)(n + 1), st));
    tb = std::max(tb, tb2);
    BAM_CHK(rd->d_tmp.ensure(tb + 8));
    BAM_HIPCHK(hipcub::DeviceScan::ExclusiveSum(rd->d_tmp.p, tb, rd->d_keep.as<ull>(), rd->d_kidx.as<ull>(), (int)(n + 1), st));
    BAM_HIPCHK(hipcub::DeviceScan::ExclusiveSum(rd->d_tmp.p, tb, rd->d_blen.as<ull>(), rd->d_boff.as<ull>(), (int)(n + 1), st));
    BAM_HIPCHK(hipMemcpyAsync(hs, rd->d_kidx.as<ull>() + n, 8, hipMemcpyDeviceToHost, st));
    BAM_HIPCHK(hipMemcpyAsync(hs + 1, rd->d_boff.as<ull>() + n, 8, hipMemcpyDeviceToHost, st));
    BAM_HIPCHK(hipMemcpyAsync(hs + 2, ds + 2, 8, hipMemcpyDeviceToHost, st));
    BAM_HIPCHK(slx_wait_stream(st));
    if (hs[2] != ~0ull) { slx_set_error("BAM: '%s': a record's fields pass its block_size (inflated offset %llu of the batch)", rd->f.path.c_str(), hs[2]); return SLX_EIO; }
    const uint64_t nr = hs[0], nb = hs[1];
    BAM_CHK(rd->d_bases.ensure(nb + 8)); BAM_CHK(rd->d_offs.ensure(8 * (nr + 1))); BAM_CHK(rd->d_map.ensure(8 * (nr + 1))); BAM_CHK(rd->h_map.ensure(8 * (nr + 1)));
    if (n) {
        k_bam_unpack<<<(unsigned)((n + 3) / 4), 256, 0, st>>>(s, rec, n, rd->d_kidx.as<ull>(), rd->d_boff.as<ull>(), original_strand, rd->d_bases.as<uint8_t>(), rd->d_offs.as<uint64_t>(),
                                                             rd->d_map.as<int64_t>());
        BAM_HIPCHK(hipGetLastError());
    } else BAM_HIPCHK(hipMemsetAsync(rd->d_offs.p, 0, 8, st));
    BAM_HIPCHK(hipEventRecord(rd->ev[6], st));
    if (nr) BAM_HIPCHK(hipMemcpyAsync(rd->h_map.p, rd->d_map.p, 8 * nr, hipMemcpyDeviceToHost, st));
    BAM_HIPCHK(slx_wait_stream(st));
    rd->us[3] = ev_us(rd->ev[5], rd->ev[6]);
    *d_bases = rd->d_bases.p; *d_offs = rd->d_offs.p; *n_reads = (int64_t)nr;
    if (rec_of_read) *rec_of_read = rd->h_map.as<int64_t>();
    return SLX_OK;
}

// a device-resident result of slx_align_batch_device as a host result: one packed image (slx_hits_pack's layout, seqlib_amd.h) in HBM, one copy down
extern "C" int slx_bam_hits_to_host(slx_bam *rd, slx_aligner *al, const slx_hits *dev, slx_hits *host)
{
    if (!rd || !al || !dev || !host || !dev->on_device) { slx_set_error("slx_bam_hits_to_host: needs a reader, an aligner and a device-resident result"); return SLX_EINVAL; }
    memset(host, 0, sizeof *host);
    BAM_HIPCHK(hipSetDevice(rd->device));
    const uint64_t bytes = slx_hits_packed_size(dev);
    BAM_CHK(rd->d_tmp.ensure(bytes + 8));
    BAM_CHK(slx_hits_pack(al, dev, rd->d_tmp.p, bytes));
    uint8_t *blk = (uint8_t *)malloc(bytes + 8);
    if (!blk) { slx_set_error("out of memory"); return SLX_ENOMEM; }
    if (hipMemcpy(blk, rd->d_tmp.p, bytes, hipMemcpyDeviceToHost) != hipSuccess) { free(blk); slx_set_error("HIP error copying the hits to the host"); return SLX_ENODEVICE; }
    const size_t N = (size_t)dev->n_reads, H = (size_t)dev->n_hits, Cg = (size_t)dev->n_cigar;
    host->n_reads = dev->n_reads; host->n_hits = dev->n_hits; host->n_cigar = dev->n_cigar;
    uint8_t *d = blk + 32;
    host->hit_off = (int64_t *)d; d += 8 * (N + 1);
    host->pos = (int64_t *)d; d += 8 * H;
    host->cig_off = (int64_t *)d; d += 8 * (H + 1);
    host->rid = (int32_t *)d; d += 4 * H;
    host->score = (int32_t *)d; d += 4 * H;
    host->nm = (int32_t *)d; d += 4 * H;
    host->na = (int32_t *)d; d += 4 * H;
    host->n_cigar_ops = (int32_t *)d; d += 4 * H;
    host->cigar = (uint32_t *)d; d += 4 * Cg;
    host->flag = (uint16_t *)d; d += 2 * H;
    host->mapq = (uint8_t *)d; d += H;
    if (dev->xa_parent) {
        d = blk + (((size_t)(d - blk) + 3) & ~(size_t)3);
        host->xa_parent = (int32_t *)d; host->sub = (int32_t *)(d + 4 * H);
    }
    host->block = blk; host->block_pinned = 0; host->block_bytes = bytes;
    return SLX_OK;
}

extern "C" int slx_bam_inflate_file(const char *path, int device, void *dst, uint64_t cap, uint64_t *n_out)
{
    slx_bam rd;
    int rc = bam_scan(path, rd.f);
    if (rc == SLX_OK) rc = bam_dev_init(&rd, device);
    if (rc != SLX_OK) { bam_dev_free(&rd); return rc; }
    uint64_t total = 0;
    for (const slx_bam_member &m : rd.f.mem) total += m.isize;
    if (n_out) *n_out = total;
    if (total > cap || (total && !dst)) { bam_dev_free(&rd); slx_set_error("slx_bam_inflate_file: %llu inflated bytes do not fit the %llu given", (unsigned long long)total, (unsigned long long)cap); return SLX_EINVAL; }
    const int64_t nm = (int64_t)rd.f.mem.size();
    uint64_t pos = 0;
    auto body = [&]() -> int {
        for (int64_t a = 0; a < nm;) {
            int64_t b = a; uint64_t bytes = 0;
            while (b < nm && (b == a || bytes + rd.f.mem[b].isize <= (256ull << 20))) bytes += rd.f.mem[b++].isize;
            BAM_CHK(rd.d_out.ensure(bytes + 8));
            BAM_CHK(bam_inflate_span(&rd, a, b, 0, bytes));
            if (bytes) { BAM_HIPCHK(hipMemcpyAsync((uint8_t *)dst + pos, rd.d_out.p, bytes, hipMemcpyDeviceToHost, rd.st)); BAM_HIPCHK(hipStreamSynchronize(rd.st)); }
            pos += bytes; a = b;
        }
        return SLX_OK;
    };
    rc = body();
    bam_dev_free(&rd);
    return rc;
}
