// slx_ref.hip -- the reference genome on the GPU (include/seqlib_amd_ref.h): a FASTA indexed into its .fai text and compacted into one byte per base in HBM, regions
// fetched in batches, NM and MD of the records of a batch.  DESIGN.md section 9.11 has the argument.
//   k_fq_count / k_fq_lines   (slx_fastq.hip, through fq_line_starts) the line starts of the text window                                   fq_text.h
//   k_ref_class    a lane per line: header, sequence or blank, its bases, its width                                                       dev_ref.h rg_line_of
//   k_ref_hdr      a lane per line, the headers: where the contig's text starts, its first line's bases and width, the bases in front of it (hipCUB scans
//                  number the headers and sum the bases)
//   k_ref_check    a lane per sequence line against its contig's first line; the smallest failing line wins                              dev_ref.h rg_check_line
//   k_ref_tiles    segments (dst, count, src, linebases, linewidth) -> bytes: byte i of a segment is src[(i / linebases) * linewidth + i % linebases].  One wave per
//                  tile of the OUTPUT, through LDS, aligned 16-byte stores.  The compaction of a window, the contig names of a window and the fetch are this
//                  one kernel (a fetched region is a segment without line structure).
//   k_ref_regions  a lane per region: clipped length and source address
//   k_md_size / k_md_text     a lane per record below long_record: the walk of dev_ref.h rg_nm_md, counting, then writing behind hipCUB's scan of the sizes
//   k_md_long<WRITE>          a wave per longer record: lanes take the bases of an M block, a ballot gives the mismatch mask, a mismatch lane gets its run
//                             length from the mask, a wave prefix places what it writes
// The text goes through HBM in windows (fq_text.h).  A window is processed up to its last complete line but one -- the line behind a sequence line decides
// whether it is its contig's last -- and the rest moves to the front of the next window.  What crosses windows is held by the host: the open contig's
// LINEBASES and LINEWIDTH, its length so far, and whether the last line was blank.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "slx_internal.h"
#include "slx_hip.h"
#include "seqlib_amd_ref.h"
#include "fq_text.h"
#include "dev_lanes.h"
#include "dev_wave.h"
#include "ref_host.h"

typedef unsigned long long ull;
typedef uint32_t rg_v4 __attribute__((ext_vector_type(4)));
#define RG_TILE_MAX 4096u          // LDS image of one output tile, per wave

struct rg_hdr { ull off, bpre; uint32_t width, name_len, lb, lw; };

// ------------------------------------------------------------------ kernels: the load
__global__ __launch_bounds__(256) void k_ref_class(const uint8_t *text, uint64_t n, const ull *line_off, uint64_t L, rg_line *li, ull *ish, ull *nb64)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > L) return;
    if (j == L) { ish[L] = 0; nb64[L] = 0; return; }
    rg_line o;
    rg_line_of(text, n, line_off[j], line_off[j + 1], &o);
    li[j] = o;
    ish[j] = o.cls == RG_HEADER ? 1u : 0u;
    nb64[j] = o.cls == RG_SEQ ? o.nb : 0u;
}

// headers among the lines [0, Lc): H[k], hline[k] of header k; li holds L > Lc or L == Lc lines
__global__ __launch_bounds__(256) void k_ref_hdr(const rg_line *li, const ull *line_off, const ull *hidx, const ull *bpre, uint64_t Lc, uint64_t L, rg_hdr *H, ull *hline)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= Lc || li[j].cls != RG_HEADER) return;
    const ull k = hidx[j];
    const bool first = j + 1 < L && li[j + 1].cls == RG_SEQ;
    rg_hdr h;
    h.off = line_off[j]; h.bpre = bpre[j]; h.width = li[j].width; h.name_len = li[j].name_len;
    h.lb = first ? li[j + 1].nb : 0u; h.lw = first ? li[j + 1].width : 0u;
    H[k] = h;
    hline[k] = j;
}

// first[0] = min over the failing sequence lines of [0, Lc) of (j << 3 | code).  c_lb, c_lw, c_prev_blank: the contig open at the window's start.
__global__ __launch_bounds__(256) void k_ref_check(const rg_line *li, const ull *hidx, const ull *hline, uint64_t Lc, uint64_t L, uint32_t c_lb, uint32_t c_lw, int c_prev_blank, ull *first)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    ull key = ~0ull;
    if (j < Lc && li[j].cls == RG_SEQ) {
        const ull k = hidx[j];
        uint32_t lb = c_lb, lw = c_lw;
        if (k) {
            const rg_line f = li[hline[k - 1] + 1];          // (at most line j itself)
            lb = f.cls == RG_SEQ ? f.nb : 0u; lw = f.cls == RG_SEQ ? f.width : 0u;
        }
        const bool prev_blank = j ? li[j - 1].cls == RG_BLANK : c_prev_blank != 0;
        const bool is_last = j + 1 < L ? li[j + 1].cls != RG_SEQ : true;
        const uint32_t er = rg_check_line(li[j].nb, li[j].width, li[j].bad, lb, lw, is_last, prev_blank);
        if (er) key = (ull)j << 3 | er;
    }
    wave_report_min(first, key);
}

// out[o0, o1) from the segments: byte p belongs to the last segment k with dst[k] <= p; it is that segment's byte p - dst[k] when that is below cnt[k], and 0
// otherwise (the bytes between segments).  dst ascends.  lb == nullptr or lb[k] == 0: the segment's bytes lie one behind the other at src[k].  One wave per `tile`
// bytes (a multiple of 16, at most RG_TILE_MAX) counted from o0 rounded down to 16: the owner of every 16th byte by binary search, the bytes between by
// walking on; the tile's image in LDS goes out in aligned 16-byte stores, except a first word that begins below o0, which goes out byte by byte.  out holds o1
// rounded up to 16: the last word is stored whole, zeros behind o1.
__global__ __launch_bounds__(256) void k_ref_tiles(const ull *dst, const ull *cnt, const ull *src, const uint32_t *lb, const uint32_t *lw, uint64_t nseg, uint64_t o0, uint64_t o1,
                                                   uint32_t tile, int upper, uint8_t *out)
{
    __shared__ __attribute__((aligned(16))) uint8_t img[4][RG_TILE_MAX];
    __shared__ uint32_t own[4][RG_TILE_MAX / 16];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t t0 = (o0 & ~15ull) + ((uint64_t)blockIdx.x * 4 + wave) * tile;
    if (t0 >= o1 || nseg == 0) return;
    const uint32_t nb = (uint32_t)(t0 + tile < o1 ? tile : o1 - t0);
    const uint32_t n16 = (nb + 15u) & ~15u;
    for (uint32_t w = lane; (w << 4) < nb; w += 64) {
        const uint64_t p = t0 + ((uint64_t)w << 4);
        uint64_t lo = 0, hi = nseg;
        while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (dst[mid] <= p) lo = mid; else hi = mid; }
        own[wave][w] = (uint32_t)lo;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (uint32_t i = lane; i < n16; i += 64) {
        uint8_t c = 0;
        const uint64_t p = t0 + i;
        if (i < nb && p >= o0) {
            uint64_t k = own[wave][i >> 4];
            while (k + 1 < nseg && dst[k + 1] <= p) ++k;
            if (p >= dst[k]) {
                const uint64_t q = p - dst[k];
                if (q < cnt[k]) {
                    const uint32_t b = lb ? lb[k] : 0u;
                    const uint64_t s = b ? (uint64_t)((uint32_t)q / b) * lw[k] + (uint32_t)q % b : q;          // (a segment with lines has fewer than 2^31 bytes)
                    c = *(const uint8_t *)(uintptr_t)(src[k] + s);
                    if (upper) c = rg_upper(c);
                }
            }
        }
        img[wave][i] = c;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (uint32_t o = lane << 4; o < n16; o += 64 << 4) {
        if (t0 + o >= o0) *reinterpret_cast<rg_v4 *>(out + t0 + o) = *reinterpret_cast<const rg_v4 *>(&img[wave][o]);
        else for (uint32_t b = 0; b < 16; ++b) if (t0 + o + b >= o0 && t0 + o + b < o1) out[t0 + o + b] = img[wave][o + b];
    }
}

// ------------------------------------------------------------------ kernels: the fetch
__global__ __launch_bounds__(256) void k_ref_regions(const slx_bam_region *reg, uint64_t n, const ull *coff, const int64_t *clen, int64_t nc, const uint8_t *bases, ull *len, ull *src)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) { len[n] = 0; src[n] = 0; return; }
    const slx_bam_region g = reg[i];
    ull l = 0, s = 0;
    if (g.tid >= 0 && g.tid < nc) {          // (the host has refused the batch otherwise)
        const int64_t b = g.beg < 0 ? 0 : g.beg, e = g.end > clen[g.tid] ? clen[g.tid] : g.end;
        if (e > b) { l = (ull)(e - b); s = (ull)(uintptr_t)(bases + coff[g.tid] + b); }
    }
    len[i] = l; src[i] = s;
}

// ------------------------------------------------------------------ kernels: NM and MD
struct md_args {
    const uint8_t *s; uint64_t n_bytes; const ull *off; uint64_t n;
    const int32_t *map; int64_t n_map;          // map nullptr: the identity over the nc contigs
    const uint8_t *bases; const ull *coff; const int64_t *clen; int64_t nc;
    uint32_t long_record, pad;
};
// the record's fields and its contig (-1: not eligible); false: the record does not hold
__device__ __forceinline__ bool md_record(const md_args &A, uint64_t i, rf_feat *F, int32_t *contig)
{
    const ull a = A.off[i], b = A.off[i + 1];
    if (a > b || b > A.n_bytes || !rf_fixed(A.s + a, b - a, F)) return false;
    int32_t c = rg_eligible(F, A.map, A.map ? A.n_map : A.nc);
    if (c < -1 || c >= A.nc) c = -1;
    *contig = c;
    return true;
}

// cnt[0]: the first record that does not hold (atomicMin); the uint32 at cnt + 1: records left to k_md_long, listed in longlist
__global__ __launch_bounds__(256) void k_md_size(md_args A, int32_t *nm, ull *sz, uint32_t *longlist, ull *cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    ull bad = ~0ull;
    if (i == A.n) sz[i] = 0;
    if (i < A.n) {
        rf_feat F;
        int32_t c = -1;
        int32_t v = -1;
        ull size = 0;
        if (!md_record(A, i, &F, &c)) bad = i;
        else if (c >= 0) {
            if ((uint32_t)F.l_seq >= A.long_record) { longlist[wave_fetch_inc((uint32_t *)(cnt + 1))] = (uint32_t)i; v = 0; }
            else { rg_md_count S = {0}; v = rg_nm_md(&F, A.bases + A.coff[c], A.clen[c], S); size = S.n; }
        }
        nm[i] = v; sz[i] = size;
    }
    wave_report_min(cnt, bad);
}

__global__ __launch_bounds__(256) void k_md_text(md_args A, const int32_t *nm, const ull *mdoff, uint8_t *md)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n || nm[i] < 0) return;
    rf_feat F;
    int32_t c = -1;
    if (!md_record(A, i, &F, &c) || c < 0 || (uint32_t)F.l_seq >= A.long_record) return;
    rg_md_write S = {md + mdoff[i], 0};
    (void)rg_nm_md(&F, A.bases + A.coff[c], A.clen[c], S);
}

__device__ __forceinline__ void md_put_u(uint8_t *p, uint32_t u, uint32_t d) { for (uint32_t k = d; k; --k) { p[k - 1] = (uint8_t)('0' + u % 10u); u /= 10u; } }

// rg_nm_md by a wave: everything but `lane` is wave-uniform
template <bool WRITE> __device__ __forceinline__ void md_wave_walk(const rf_feat &F, const uint8_t *ref, int64_t rlen, uint32_t lane, uint8_t *out, int32_t *nm_out, ull *sz_out)
{
    int64_t x = F.pos, y = 0;
    const int64_t ls = F.l_seq;
    uint32_t u = 0, nm = 0;
    uint64_t o = 0;
    bool stop = false;
    for (uint32_t k = 0; k < F.n_cig && !stop; ++k) {
        const uint32_t wd = rf_u32(F.cig + 4ull * k), op = wd & 15u, len = wd >> 4;
        if (op == 0 || op == 7 || op == 8) {
            int64_t room = rlen - x < ls - y ? rlen - x : ls - y;
            if (room < 0) room = 0;
            const uint32_t rem = (int64_t)len <= room ? len : (uint32_t)room;
            for (uint32_t c0 = 0; c0 < rem; c0 += 64) {
                const uint32_t i = c0 + lane, nv = rem - c0 < 64u ? rem - c0 : 64u;
                uint8_t rb = 0;
                bool mis = false;
                if (i < rem) { rb = ref[x + i]; mis = !rg_match(rg_read_code(F.seq, (uint64_t)(y + i)), rg_nt16(rb)); }
                const ull mask = __ballot(mis);
                if (!mask) { u += nv; continue; }
                uint32_t mysz = 0, run = 0;
                if (mis) {
                    const ull below = mask & ((1ull << lane) - 1ull);
                    run = below ? lane - 1u - (63u - (uint32_t)__clzll((long long)below)) : u + lane;
                    mysz = rg_digits(run) + 1u;
                }
                uint32_t incl = mysz;
                for (int s = 1; s < 64; s <<= 1) { const uint32_t t = __shfl_up(incl, s, 64); if ((int)lane >= s) incl += t; }
                if (WRITE && mis) { uint8_t *p = out + o + (incl - mysz); md_put_u(p, run, mysz - 1u); p[mysz - 1u] = rg_upper(rb); }
                o += __shfl(incl, 63, 64);
                nm += (uint32_t)__popcll(mask);
                u = nv - 1u - (63u - (uint32_t)__clzll((long long)mask));
            }
            x += rem; y += rem;
            if (rem < len) stop = true;
        } else if (op == 2) {
            const uint32_t d = rg_digits(u);
            if (WRITE && lane == 0) { md_put_u(out + o, u, d); out[o + d] = '^'; }
            o += d + 1u;
            int64_t room = rlen - x;
            if (room < 0) room = 0;
            const uint32_t rem = (int64_t)len <= room ? len : (uint32_t)room;
            if (WRITE) for (uint32_t i = lane; i < rem; i += 64) out[o + i] = rg_upper(ref[x + i]);
            o += rem; nm += rem; x += rem; u = 0;
            if (rem < len) stop = true;
        } else if (op == 1) { nm += len; y += len; }
        else if (op == 4) y += len;
        else if (op == 3) x += len;
    }
    const uint32_t d = rg_digits(u);
    if (WRITE && lane == 0) md_put_u(out + o, u, d);
    o += d;
    if (!WRITE && lane == 0) { *nm_out = (int32_t)nm; *sz_out = o; }
}

template <bool WRITE> __global__ __launch_bounds__(256) void k_md_long(md_args A, const uint32_t *longlist, uint32_t n_long, int32_t *nm, ull *sz, const ull *mdoff, uint8_t *md)
{
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= n_long) return;
    const uint64_t i = longlist[w];
    rf_feat F;
    int32_t c = -1;
    if (!md_record(A, i, &F, &c) || c < 0) return;          // (k_md_size listed it: it holds)
    md_wave_walk<WRITE>(F, A.bases + A.coff[c], A.clen[c], lane, WRITE ? md + mdoff[i] : nullptr, nm + i, sz + i);
}

// ------------------------------------------------------------------ host: the handle
typedef SlxDevBuf<SlxMargin<4, 256>> RDBuf;
typedef SlxPinBuf<SlxMargin<4, 256>> RHBuf;

struct slx_ref {
    FqText T;          // the source and its device context: the handle's buffers hang on it
    uint64_t window = 64ull << 20;
    uint32_t gather_tile = 2048, long_record = 64;          // long_record: profiles/NOTES_ref.md
    std::vector<rg_contig> C;
    std::vector<uint64_t> coff;          // C.size() + 1 once loaded
    rg_names names;
    std::string fai;
    uint64_t text_base = 0, bases_end = 0;
    bool prev_blank = false;
    hipEvent_t ev[6] = {};          // beside T's ten: the handle makes and destroys them itself
    RDBuf d_bases{T}, d_coff{T}, d_clen{T};
    // the load
    RDBuf d_li{T}, d_ish{T}, d_nb64{T}, d_hidx{T}, d_bpre{T}, d_H{T}, d_hline{T}, d_first{T}, d_seg{T}, d_names{T};
    RHBuf h_small{T}, h_H{T}, h_seg{T}, h_names{T};
    // the fetch
    RDBuf d_reg{T}, d_flen{T}, d_fsrc{T}, d_foff{T}, d_fout{T};
    // NM and MD
    RDBuf d_in{T}, d_off{T}, d_map{T}, d_nm{T}, d_sz{T}, d_mdoff{T}, d_md{T}, d_long{T}, d_cnt{T};
    slx_ref_md last_md = {};
    int64_t c_windows = 0, c_text = 0, c_bases = 0, c_long = 0;
    double us_class = 0, us_gather = 0, us_fetch = 0, us_md_size = 0, us_md_text = 0;
    std::vector<RDBuf *> load_dbufs() { return {&d_li, &d_ish, &d_nb64, &d_hidx, &d_bpre, &d_H, &d_hline, &d_first, &d_names}; }
};

struct rg_seg { uint64_t dst, cnt, src; uint32_t lb, lw; };

// the segments into out[o0, o1) on the handle's stream (which has not drained on return; h_seg is free again once it has)
static int ref_tiles(slx_ref *r, const std::vector<rg_seg> &S, uint64_t o0, uint64_t o1, uint32_t tile, uint8_t *out)
{
    const size_t m = S.size();
    if (m == 0 || o1 <= o0) return SLX_OK;
    SLX_CHK(r->h_seg.ensure(32 * m)); SLX_CHK(r->d_seg.ensure(32 * m));
    uint64_t *h = r->h_seg.as<uint64_t>();
    uint32_t *h32 = (uint32_t *)(h + 3 * m);
    for (size_t k = 0; k < m; ++k) { h[k] = S[k].dst; h[m + k] = S[k].cnt; h[2 * m + k] = S[k].src; h32[k] = S[k].lb; h32[m + k] = S[k].lw; }
    SLX_HIPCHK(hipMemcpyAsync(r->d_seg.p, h, 32 * m, hipMemcpyHostToDevice, r->T.st));
    const ull *d = r->d_seg.as<ull>();
    const uint32_t *d32 = (const uint32_t *)(d + 3 * m);
    const uint64_t tiles = (o1 - (o0 & ~15ull) + tile - 1) / tile;
    if (tiles >= 0x1fffffffull) { slx_set_error("reference genome: %llu output tiles in one launch", (ull)tiles); return SLX_EUNSUPPORTED; }
    k_ref_tiles<<<(unsigned)((tiles + 3) / 4), 256, 0, r->T.st>>>(d, d + m, d + 2 * m, d32, d32 + m, m, o0, o1, tile, 0, out);
    SLX_HIPCHK(hipGetLastError());
    return SLX_OK;
}

static int ref_fail(slx_ref *r, uint32_t code, const std::string &contig, uint64_t byte)
{
    slx_set_error("reference genome: '%s': %s", r->T.path.c_str(), rg_message(code, contig, byte).c_str());
    return SLX_EIO;
}

// the open contig takes `add` more bases
static int ref_grow(slx_ref *r, uint64_t add)
{
    rg_contig &c = r->C.back();
    c.len += (int64_t)add;
    if (c.len > RG_MAX_CONTIG) return ref_fail(r, RG_E_TOO_LONG, c.name, c.off);
    return SLX_OK;
}

// one window, d_text[cur][0, have): *consumed bytes of it are done with (0: not two whole lines yet)
static int ref_window(slx_ref *r, uint64_t *consumed)
{
    FqText &T = r->T;
    hipStream_t st = T.st;
    const uint8_t *text = T.d_text[T.cur].as<uint8_t>();
    const uint64_t n = T.have;
    uint64_t L = 0;
    int virt = 0;
    *consumed = 0;
    SLX_CHK(fq_line_starts(&T, &L, &virt));
    const uint64_t Lc = T.src_eof ? L : (L ? L - 1 : 0);
    if (Lc == 0) { SLX_HIPCHK(slx_wait_stream(st)); return SLX_OK; }
    if (L >= 0x1fffffffffull) { slx_set_error("reference genome: %llu lines in one window", (ull)L); return SLX_EUNSUPPORTED; }
    const ull *line_off = T.d_line.as<ull>();
    SLX_CHK(r->d_li.ensure(sizeof(rg_line) * (L + 1)));
    for (RDBuf *b : {&r->d_ish, &r->d_nb64, &r->d_hidx, &r->d_bpre}) SLX_CHK(b->ensure(8 * (L + 2)));
    SLX_CHK(r->d_first.ensure(8)); SLX_CHK(r->h_small.ensure(256));
    rg_line *li = r->d_li.as<rg_line>();
    ull *hs = r->h_small.as<ull>();
    SLX_HIPCHK(hipEventRecord(r->ev[0], st));
    k_ref_class<<<(unsigned)((L + 256) / 256), 256, 0, st>>>(text, n, line_off, L, li, r->d_ish.as<ull>(), r->d_nb64.as<ull>());
    SLX_HIPCHK(hipGetLastError());
    SLX_CHK(fq_scan(&T, r->d_ish.as<ull>(), r->d_hidx.as<ull>(), Lc + 1));
    SLX_CHK(fq_scan(&T, r->d_nb64.as<ull>(), r->d_bpre.as<ull>(), Lc + 1));
    SLX_HIPCHK(hipMemcpyAsync(hs, r->d_hidx.as<ull>() + Lc, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync(hs + 1, r->d_bpre.as<ull>() + Lc, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync(hs + 2, line_off + Lc, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync(hs + 8, li + (Lc - 1), sizeof(rg_line), hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    const uint64_t nh = hs[0], nbases = hs[1], used = std::min<uint64_t>(hs[2], n);
    const bool last_blank = ((const rg_line *)(hs + 8))->cls == RG_BLANK;
    SLX_CHK(r->d_H.ensure(sizeof(rg_hdr) * (nh + 1))); SLX_CHK(r->d_hline.ensure(8 * (nh + 1))); SLX_CHK(r->h_H.ensure(sizeof(rg_hdr) * (nh + 1)));
    SLX_HIPCHK(hipMemsetAsync(r->d_first.p, 0xff, 8, st));
    const unsigned gl = (unsigned)((Lc + 255) / 256);
    if (nh) { k_ref_hdr<<<gl, 256, 0, st>>>(li, line_off, r->d_hidx.as<ull>(), r->d_bpre.as<ull>(), Lc, L, r->d_H.as<rg_hdr>(), r->d_hline.as<ull>()); SLX_HIPCHK(hipGetLastError()); }
    const bool open = !r->C.empty();
    k_ref_check<<<gl, 256, 0, st>>>(li, r->d_hidx.as<ull>(), r->d_hline.as<ull>(), Lc, L, open ? r->C.back().lb : 0u, open ? r->C.back().lw : 0u, r->prev_blank ? 1 : 0, r->d_first.as<ull>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(r->ev[1], st));
    SLX_HIPCHK(hipMemcpyAsync(hs, r->d_first.p, 8, hipMemcpyDeviceToHost, st));
    if (nh) SLX_HIPCHK(hipMemcpyAsync(r->h_H.p, r->d_H.p, sizeof(rg_hdr) * nh, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    r->us_class += slx_ev_us(r->ev[0], r->ev[1]); T.us[0] += slx_ev_us(T.ev[0], T.ev[1]);          // (fq_line_starts records its two events and leaves the sum to its caller)
    const rg_hdr *H = r->h_H.as<rg_hdr>();
    // the first failing sequence line, if any: where it is and how many headers of the window lie in front of it
    bool dev_err = hs[0] != ~0ull;
    uint32_t dev_code = 0;
    uint64_t dev_off = 0, dev_hdrs = 0;
    if (dev_err) {
        const uint64_t j = hs[0] >> 3;
        dev_code = (uint32_t)(hs[0] & 7);
        SLX_HIPCHK(hipMemcpyAsync(hs + 3, line_off + j, 8, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(hipMemcpyAsync(hs + 4, r->d_hidx.as<ull>() + j, 8, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(slx_wait_stream(st));
        dev_off = hs[3]; dev_hdrs = hs[4];
    }
    // the names of the window's headers
    if (nh) {
        std::vector<rg_seg> S(nh);
        uint64_t at = 0;
        for (uint64_t k = 0; k < nh; ++k) { S[k] = rg_seg{at, H[k].name_len, (uint64_t)(uintptr_t)(text + H[k].off + 1), 0u, 0u}; at += H[k].name_len; }
        SLX_CHK(r->d_names.ensure(at + 64)); SLX_CHK(r->h_names.ensure(at + 64));
        SLX_CHK(ref_tiles(r, S, 0, at, r->gather_tile, r->d_names.as<uint8_t>()));
        if (at) SLX_HIPCHK(hipMemcpyAsync(r->h_names.p, r->d_names.p, at, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(slx_wait_stream(st));
    }
    // the contigs, in file order; the bases of each as a segment of the compaction
    std::vector<rg_seg> S;
    if (open) {
        const uint64_t add = nh ? H[0].bpre : nbases;
        if (!(dev_err && dev_hdrs == 0)) {
            const rg_contig &c = r->C.back();
            if (add) S.push_back(rg_seg{r->coff.back() + (uint64_t)c.len, add, (uint64_t)(uintptr_t)text, c.lb, c.lw});
            SLX_CHK(ref_grow(r, add));
        }
    }
    const char *nm = r->h_names.as<char>();
    for (uint64_t k = 0; k < nh; ++k) {
        if (dev_err && dev_hdrs == k) break;
        rg_contig c;
        c.name.assign(nm, H[k].name_len); nm += H[k].name_len;
        c.off = r->text_base + H[k].off + H[k].width; c.lb = H[k].lb; c.lw = H[k].lw;
        const uint32_t er = r->names.add(c.name, (int64_t)r->C.size());
        if (er) return ref_fail(r, er, c.name, r->text_base + H[k].off);
        r->coff.push_back(r->C.empty() ? 0 : (r->coff.back() + (uint64_t)r->C.back().len + 15u) & ~15ull);
        r->C.push_back(c);
        const uint64_t add = (k + 1 < nh ? H[k + 1].bpre : nbases) - H[k].bpre;
        if (add) S.push_back(rg_seg{r->coff.back(), add, (uint64_t)(uintptr_t)(text + H[k].off + H[k].width), c.lb, c.lw});
        if (!(dev_err && dev_hdrs == k + 1)) SLX_CHK(ref_grow(r, add));
    }
    if (dev_err) return ref_fail(r, dev_code, r->C.empty() ? std::string() : r->C.back().name, r->text_base + dev_off);
    if (!S.empty()) {
        const uint64_t o0 = r->bases_end, o1 = S.back().dst + S.back().cnt;
        SLX_CHK(r->d_bases.ensure(o1 + 64, st, r->bases_end));
        SLX_HIPCHK(hipEventRecord(r->ev[2], st));
        SLX_CHK(ref_tiles(r, S, o0, o1, r->gather_tile, r->d_bases.as<uint8_t>()));
        SLX_HIPCHK(hipEventRecord(r->ev[3], st));
        SLX_HIPCHK(slx_wait_stream(st));
        r->us_gather += slx_ev_us(r->ev[2], r->ev[3]);
        r->bases_end = o1; r->c_bases += (int64_t)nbases;
    }
    r->prev_blank = last_blank;
    r->c_windows += 1;
    *consumed = used;
    return SLX_OK;
}

static void ref_free(slx_ref *r)
{
    if (r->T.st) { (void)hipSetDevice(r->T.device); (void)hipStreamSynchronize(r->T.st); }
    for (auto &e : r->ev) if (e) (void)hipEventDestroy(e);
    fq_text_free(&r->T);          // every buffer, T's events, the stream
    delete r;
}

static int ref_load(slx_ref *r)
{
    FqText &T = r->T;
    hipStream_t st = T.st;
    for (auto &e : r->ev) SLX_HIPCHK(hipEventCreate(&e));
    SLX_CHK(fq_text_start(&T));
    uint64_t target = r->window;
    bool first = true;
    for (;;) {
        if (T.used) SLX_CHK(fq_shift(&T, target));
        if (T.have < target && !T.src_eof) SLX_CHK(fq_pull(&T, target - T.have));
        if (T.have == 0) {
            if (T.src_eof) break;
            continue;
        }
        if (first) {
            uint8_t b0 = 0;
            SLX_HIPCHK(hipMemcpyAsync(&b0, T.d_text[T.cur].p, 1, hipMemcpyDeviceToHost, st));
            SLX_HIPCHK(slx_wait_stream(st));
            const uint32_t er = rg_first_byte(&b0, 1);
            if (er) return ref_fail(r, er, "", 0);
            first = false;
        }
        uint64_t consumed = 0;
        SLX_CHK(ref_window(r, &consumed));
        T.used = consumed; r->text_base += consumed;
        if (T.src_eof && consumed >= T.have) break;
        if (consumed == 0) {
            if (T.src_eof) { slx_set_error("reference genome: internal: no progress at the end of '%s'", T.path.c_str()); return SLX_EINTERNAL; }
            target = std::max<uint64_t>(2 * target, 2 * T.have + 64);          // not two whole lines yet: the window grows
        } else target = r->window;
    }
    if (r->C.empty()) return ref_fail(r, RG_E_NONE, "", 0);
    r->c_text = (int64_t)r->text_base;
    // the table for device consumers; the extent of the bases, the last contig's padding zeroed
    const size_t nc = r->C.size();
    r->coff.push_back((r->coff.back() + (uint64_t)r->C.back().len + 15u) & ~15ull);
    const uint64_t extent = r->coff.back();
    SLX_CHK(r->d_bases.ensure(extent + 64, st, r->bases_end));
    if (extent > r->bases_end) SLX_HIPCHK(hipMemsetAsync(r->d_bases.as<uint8_t>() + r->bases_end, 0, extent - r->bases_end, st));
    std::vector<int64_t> len(nc);
    for (size_t i = 0; i < nc; ++i) len[i] = r->C[i].len;
    SLX_CHK(r->d_coff.ensure(8 * (nc + 1))); SLX_CHK(r->d_clen.ensure(8 * nc));
    SLX_HIPCHK(hipMemcpyAsync(r->d_coff.p, r->coff.data(), 8 * (nc + 1), hipMemcpyHostToDevice, st));
    SLX_HIPCHK(hipMemcpyAsync(r->d_clen.p, len.data(), 8 * nc, hipMemcpyHostToDevice, st));
    SLX_HIPCHK(slx_wait_stream(st));
    r->fai = rg_fai_text(r->C);
    // what only the load needed goes back
    T.prod.release();
    for (RDBuf *b : r->load_dbufs()) b->release();
    for (FqDBuf *b : T.text_dbufs()) b->release();
    T.stage.release();
    // an index beside the file is compared, never believed
    const std::string fp = T.path + ".fai";
    if (FILE *f = fopen(fp.c_str(), "rb")) {
        std::string have;
        char buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, f)) > 0) have.append(buf, got);
        fclose(f);
        if (have != r->fai) {
            size_t at = 0;
            while (at < have.size() && at < r->fai.size() && have[at] == r->fai[at]) ++at;
            slx_set_error("reference genome: stale index: '%s' differs from the index built from '%s' at byte %zu; remove it or write it again", fp.c_str(), T.path.c_str(), at);
            return SLX_EIO;
        }
    }
    return SLX_OK;
}

extern "C" int slx_ref_open_ex(const char *path, int device, int64_t window_bytes, int64_t tile_bytes, int64_t gather_tile_bytes, slx_ref **out)
{
    if (!path || !out) { slx_set_error("slx_ref_open: null argument"); return SLX_EINVAL; }
    *out = nullptr;
    if ((window_bytes && window_bytes < 64) || (tile_bytes && (tile_bytes < 16 || tile_bytes % 16 || tile_bytes > (1 << 30))) ||
        (gather_tile_bytes && (gather_tile_bytes < 16 || gather_tile_bytes % 16 || gather_tile_bytes > (int64_t)RG_TILE_MAX))) {
        slx_set_error("slx_ref_open_ex: window_bytes %lld, tile_bytes %lld or gather_tile_bytes %lld out of range", (long long)window_bytes, (long long)tile_bytes, (long long)gather_tile_bytes);
        return SLX_EINVAL;
    }
    slx_ref *r = new slx_ref();
    r->T.who = "reference genome";
    if (window_bytes) r->window = (uint64_t)window_bytes;
    if (tile_bytes) r->T.tile_bytes = (uint32_t)tile_bytes;
    if (gather_tile_bytes) r->gather_tile = (uint32_t)gather_tile_bytes;
    int rc = fq_text_open(&r->T, path, device);
    if (rc == SLX_OK) rc = ref_load(r);
    if (rc != SLX_OK) { ref_free(r); return rc; }
    *out = r;
    return SLX_OK;
}
extern "C" int slx_ref_open(const char *path, int device, slx_ref **out) { return slx_ref_open_ex(path, device, 0, 0, 0, out); }
extern "C" void slx_ref_close(slx_ref *r) { if (r) ref_free(r); }

extern "C" int slx_ref_set(slx_ref *r, const char *key, int64_t v)
{
    if (!r || !key) { slx_set_error("slx_ref_set: null argument"); return SLX_EINVAL; }
    if (!strcmp(key, "gather_tile_bytes") && v >= 16 && v % 16 == 0 && v <= (int64_t)RG_TILE_MAX) { r->gather_tile = (uint32_t)v; return SLX_OK; }
    if (!strcmp(key, "long_record") && v >= 1 && v <= 0x7fffffffll) { r->long_record = (uint32_t)v; return SLX_OK; }
    slx_set_error("slx_ref_set: unknown key '%s' or value %lld out of range", key, (long long)v);
    return SLX_EINVAL;
}

extern "C" int64_t slx_ref_counter(const slx_ref *r, const char *name)
{
    if (!r || !name) return -1;
    const std::string k = name;
    if (k == "contigs") return (int64_t)r->C.size();
    if (k == "bases") return r->c_bases;
    if (k == "text_bytes") return r->c_text;
    if (k == "windows") return r->c_windows;
    if (k == "source") return r->T.source;
    if (k == "hbm_bytes") return (int64_t)r->coff.back();
    if (k == "long_records") return r->c_long;
    if (k == "long_record") return r->long_record;
    if (k == "us_lines") return (int64_t)r->T.us[0];
    if (k == "us_class") return (int64_t)r->us_class;
    if (k == "us_gather") return (int64_t)r->us_gather;
    if (k == "us_inflate") return (int64_t)r->T.us[3];
    if (k == "us_fetch") return (int64_t)r->us_fetch;
    if (k == "us_md_size") return (int64_t)r->us_md_size;
    if (k == "us_md_text") return (int64_t)r->us_md_text;
    return -1;
}

extern "C" int64_t slx_ref_nseq(const slx_ref *r) { return r ? (int64_t)r->C.size() : 0; }
extern "C" const char *slx_ref_name(const slx_ref *r, int64_t tid) { return r && tid >= 0 && tid < (int64_t)r->C.size() ? r->C[(size_t)tid].name.c_str() : nullptr; }
extern "C" int64_t slx_ref_len(const slx_ref *r, int64_t tid) { return r && tid >= 0 && tid < (int64_t)r->C.size() ? r->C[(size_t)tid].len : -1; }
extern "C" int64_t slx_ref_tid(const slx_ref *r, const char *name)
{
    if (!r || !name) return -1;
    const auto it = r->names.tid.find(name);
    return it == r->names.tid.end() ? -1 : it->second;
}
extern "C" const char *slx_ref_fai_text(const slx_ref *r, int64_t *n)
{
    if (n) *n = r ? (int64_t)r->fai.size() : 0;
    return r ? r->fai.c_str() : nullptr;
}
extern "C" int slx_ref_write_fai(const slx_ref *r, const char *fai_path)
{
    if (!r) { slx_set_error("slx_ref_write_fai: null object"); return SLX_EINVAL; }
    const std::string p = fai_path ? std::string(fai_path) : r->T.path + ".fai";
    FILE *f = fopen(p.c_str(), "wb");
    if (!f) { slx_set_error("slx_ref_write_fai: cannot create '%s'", p.c_str()); return SLX_EIO; }
    const bool ok = fwrite(r->fai.data(), 1, r->fai.size(), f) == r->fai.size();
    if (fclose(f) != 0 || !ok) { slx_set_error("slx_ref_write_fai: writing '%s' failed", p.c_str()); return SLX_EIO; }
    return SLX_OK;
}
extern "C" int slx_ref_device(const slx_ref *r, slx_ref_dev *out)
{
    if (!r || !out) { slx_set_error("slx_ref_device: null argument"); return SLX_EINVAL; }
    out->n_contigs = (int64_t)r->C.size(); out->n_bytes = (int64_t)r->coff.back();
    out->d_bases = r->d_bases.p; out->d_contig_off = r->d_coff.p; out->d_contig_len = r->d_clen.p;
    return SLX_OK;
}

// ------------------------------------------------------------------ host: the fetch
static int ref_fetch(slx_ref *r, const char *who, const slx_bam_region *regions, int64_t n, int upper, uint64_t *total)
{
    if (!r || n < 0 || (n && !regions)) { slx_set_error("%s: null or negative argument", who); return SLX_EINVAL; }
    const int64_t nc = (int64_t)r->C.size();
    for (int64_t i = 0; i < n; ++i)
        if (regions[i].tid < 0 || regions[i].tid >= nc) { slx_set_error("%s: region %lld names contig %d, which is not one of the %lld", who, (long long)i, regions[i].tid, (long long)nc); return SLX_EINVAL; }
    SLX_HIPCHK(hipSetDevice(r->T.device));
    hipStream_t st = r->T.st;
    const size_t N = (size_t)n;
    SLX_CHK(r->d_reg.ensure(sizeof(slx_bam_region) * (N + 1)));
    for (RDBuf *b : {&r->d_flen, &r->d_fsrc, &r->d_foff}) SLX_CHK(b->ensure(8 * (N + 2)));
    SLX_CHK(r->h_small.ensure(256));
    if (N) SLX_HIPCHK(hipMemcpyAsync(r->d_reg.p, regions, sizeof(slx_bam_region) * N, hipMemcpyHostToDevice, st));
    SLX_HIPCHK(hipEventRecord(r->ev[4], st));
    k_ref_regions<<<(unsigned)((N + 256) / 256), 256, 0, st>>>(r->d_reg.as<slx_bam_region>(), N, r->d_coff.as<ull>(), r->d_clen.as<int64_t>(), nc, r->d_bases.as<uint8_t>(), r->d_flen.as<ull>(),
                                                             r->d_fsrc.as<ull>());
    SLX_HIPCHK(hipGetLastError());
    SLX_CHK(slx_exclusive_sum(r->T.d_tmp, r->d_flen.as<ull>(), r->d_foff.as<ull>(), N + 1, st, 16));
    ull *hs = r->h_small.as<ull>();
    SLX_HIPCHK(hipMemcpyAsync(hs, r->d_foff.as<ull>() + N, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));          // (the regions may be the caller's stack)
    *total = hs[0];
    SLX_CHK(r->d_fout.ensure(*total + 64));
    if (*total) {
        const uint32_t tile = r->gather_tile;
        const uint64_t tiles = (*total + tile - 1) / tile;
        if (tiles >= 0x1fffffffull) { slx_set_error("%s: %llu bytes in one batch", who, (ull)*total); return SLX_EUNSUPPORTED; }
        k_ref_tiles<<<(unsigned)((tiles + 3) / 4), 256, 0, st>>>(r->d_foff.as<ull>(), r->d_flen.as<ull>(), r->d_fsrc.as<ull>(), nullptr, nullptr, N, 0, *total, tile, upper ? 1 : 0,
                                                               r->d_fout.as<uint8_t>());
        SLX_HIPCHK(hipGetLastError());
    }
    SLX_HIPCHK(hipEventRecord(r->ev[5], st));
    SLX_HIPCHK(slx_wait_stream(st));
    r->us_fetch = slx_ev_us(r->ev[4], r->ev[5]);
    return SLX_OK;
}

extern "C" int slx_ref_fetch_device(slx_ref *r, const slx_bam_region *regions, int64_t n, int upper, const void **d_bases, const void **d_offs, int64_t *n_bytes)
{
    if (!d_bases || !d_offs) { slx_set_error("slx_ref_fetch_device: null argument"); return SLX_EINVAL; }
    uint64_t total = 0;
    SLX_CHK(ref_fetch(r, "slx_ref_fetch_device", regions, n, upper, &total));
    *d_bases = r->d_fout.p; *d_offs = r->d_foff.p;
    if (n_bytes) *n_bytes = (int64_t)total;
    return SLX_OK;
}

extern "C" int slx_ref_fetch_host(slx_ref *r, const slx_bam_region *regions, int64_t n, int upper, void *bases, int64_t cap, uint64_t *offs)
{
    if (!offs) { slx_set_error("slx_ref_fetch_host: null argument"); return SLX_EINVAL; }
    uint64_t total = 0;
    SLX_CHK(ref_fetch(r, "slx_ref_fetch_host", regions, n, upper, &total));
    SLX_HIPCHK(hipMemcpyAsync(offs, r->d_foff.p, 8 * ((size_t)n + 1), hipMemcpyDeviceToHost, r->T.st));
    SLX_HIPCHK(slx_wait_stream(r->T.st));
    if (!bases) return SLX_OK;
    if (cap < 0 || (uint64_t)cap < total) { slx_set_error("slx_ref_fetch_host: %llu bytes do not fit %lld", (ull)total, (long long)cap); return SLX_EINVAL; }
    if (total) SLX_HIPCHK(hipMemcpyAsync(bases, r->d_fout.p, total, hipMemcpyDeviceToHost, r->T.st));
    SLX_HIPCHK(slx_wait_stream(r->T.st));
    return SLX_OK;
}

// ------------------------------------------------------------------ host: NM and MD
static int ref_nm_md(slx_ref *r, const char *who, const uint8_t *d_s, uint64_t n_bytes, const ull *d_off, uint64_t n, const int32_t *tid_map, int64_t n_map, slx_ref_md *out)
{
    hipStream_t st = r->T.st;
    const int64_t nc = (int64_t)r->C.size();
    *out = slx_ref_md{};
    r->last_md = *out;
    if (n >= 0xffffffffull) { slx_set_error("%s: 2^32 - 1 records or more in one batch", who); return SLX_EUNSUPPORTED; }
    if (tid_map) {
        if (n_map < 0) { slx_set_error("%s: negative n_map", who); return SLX_EINVAL; }
        for (int64_t i = 0; i < n_map; ++i)
            if (tid_map[i] < -1 || tid_map[i] >= nc) { slx_set_error("%s: tid_map[%lld] = %d is neither -1 nor one of the %lld contigs", who, (long long)i, tid_map[i], (long long)nc); return SLX_EINVAL; }
        SLX_CHK(r->d_map.ensure(4 * (size_t)n_map + 4));
        if (n_map) SLX_HIPCHK(hipMemcpyAsync(r->d_map.p, tid_map, 4 * (size_t)n_map, hipMemcpyHostToDevice, st));
        SLX_HIPCHK(slx_wait_stream(st));
    }
    SLX_CHK(r->d_nm.ensure(4 * (n + 1))); SLX_CHK(r->d_sz.ensure(8 * (n + 2))); SLX_CHK(r->d_mdoff.ensure(8 * (n + 2))); SLX_CHK(r->d_long.ensure(4 * (n + 1)));
    SLX_CHK(r->d_cnt.ensure(16)); SLX_CHK(r->h_small.ensure(256));
    ull *hs = r->h_small.as<ull>();
    md_args A = {d_s, n_bytes, d_off, n, tid_map ? r->d_map.as<int32_t>() : nullptr, n_map, r->d_bases.as<uint8_t>(), r->d_coff.as<ull>(), r->d_clen.as<int64_t>(), nc, r->long_record, 0u};
    hs[0] = ~0ull; hs[1] = 0;
    SLX_HIPCHK(hipMemcpyAsync(r->d_cnt.p, hs, 16, hipMemcpyHostToDevice, st));
    SLX_HIPCHK(hipEventRecord(r->ev[0], st));
    k_md_size<<<(unsigned)((n + 256) / 256), 256, 0, st>>>(A, r->d_nm.as<int32_t>(), r->d_sz.as<ull>(), r->d_long.as<uint32_t>(), r->d_cnt.as<ull>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipMemcpyAsync(hs + 2, r->d_cnt.p, 16, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    if (hs[2] != ~0ull) {
        slx_set_error("reference genome: record %llu of the batch: its fields pass its block_size, or its extent is not block_size + 4 inside the stream", hs[2]);
        return SLX_EIO;
    }
    const uint32_t n_long = (uint32_t)hs[3];
    r->c_long = n_long;
    if (n_long) { k_md_long<false><<<(n_long + 3) / 4, 256, 0, st>>>(A, r->d_long.as<uint32_t>(), n_long, r->d_nm.as<int32_t>(), r->d_sz.as<ull>(), nullptr, nullptr); SLX_HIPCHK(hipGetLastError()); }
    SLX_CHK(slx_exclusive_sum(r->T.d_tmp, r->d_sz.as<ull>(), r->d_mdoff.as<ull>(), n + 1, st, 16));
    SLX_HIPCHK(hipEventRecord(r->ev[1], st));
    SLX_HIPCHK(hipMemcpyAsync(hs, r->d_mdoff.as<ull>() + n, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    const uint64_t total = hs[0];
    SLX_CHK(r->d_md.ensure(total + 64));
    SLX_HIPCHK(hipEventRecord(r->ev[2], st));
    if (n) { k_md_text<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(A, r->d_nm.as<int32_t>(), r->d_mdoff.as<ull>(), r->d_md.as<uint8_t>()); SLX_HIPCHK(hipGetLastError()); }
    if (n_long) {
        k_md_long<true><<<(n_long + 3) / 4, 256, 0, st>>>(A, r->d_long.as<uint32_t>(), n_long, r->d_nm.as<int32_t>(), r->d_sz.as<ull>(), r->d_mdoff.as<ull>(), r->d_md.as<uint8_t>());
        SLX_HIPCHK(hipGetLastError());
    }
    SLX_HIPCHK(hipEventRecord(r->ev[3], st));
    SLX_HIPCHK(slx_wait_stream(st));
    r->us_md_size = slx_ev_us(r->ev[0], r->ev[1]); r->us_md_text = slx_ev_us(r->ev[2], r->ev[3]);
    out->n_records = (int64_t)n; out->md_bytes = (int64_t)total;
    out->d_nm = r->d_nm.p; out->d_md = r->d_md.p; out->d_md_off = r->d_mdoff.p;
    r->last_md = *out;
    return SLX_OK;
}

static int ref_md_args(const char *who, slx_ref *r, const void *s, int64_t n_bytes, const void *off, int64_t n, slx_ref_md *out)
{
    if (!r || !out || n_bytes < 0 || n < 0 || (n_bytes && !s) || !off) { slx_set_error("%s: null or negative argument", who); return SLX_EINVAL; }
    SLX_HIPCHK(hipSetDevice(r->T.device));
    return SLX_OK;
}

extern "C" int slx_ref_nm_md_device(slx_ref *r, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records, const int32_t *tid_map, int64_t n_map, slx_ref_md *out)
{
    SLX_CHK(ref_md_args("slx_ref_nm_md_device", r, d_stream, n_bytes, d_rec_off, n_records, out));
    return ref_nm_md(r, "slx_ref_nm_md_device", (const uint8_t *)d_stream, (uint64_t)n_bytes, (const ull *)d_rec_off, (uint64_t)n_records, tid_map, n_map, out);
}

extern "C" int slx_ref_nm_md_host(slx_ref *r, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records, const int32_t *tid_map, int64_t n_map, slx_ref_md *out)
{
    SLX_CHK(ref_md_args("slx_ref_nm_md_host", r, stream, n_bytes, rec_off, n_records, out));
    SLX_CHK(slx_batch_stage(r->d_in, r->d_off, 16, stream, n_bytes, rec_off, n_records, r->T.st));
    SLX_HIPCHK(slx_wait_stream(r->T.st));
    return ref_nm_md(r, "slx_ref_nm_md_host", r->d_in.as<uint8_t>(), (uint64_t)n_bytes, r->d_off.as<ull>(), (uint64_t)n_records, tid_map, n_map, out);
}

extern "C" int slx_ref_md_to_host(slx_ref *r, const slx_ref_md *m, int32_t *nm, void *md, uint64_t *md_off)
{
    if (!r || !m) { slx_set_error("slx_ref_md_to_host: null argument"); return SLX_EINVAL; }
    if (m->d_nm != r->last_md.d_nm || m->n_records != r->last_md.n_records || m->md_bytes != r->last_md.md_bytes || !m->d_nm) { slx_set_error("slx_ref_md_to_host: not the handle's last result"); return SLX_EINVAL; }
    SLX_HIPCHK(hipSetDevice(r->T.device));
    hipStream_t st = r->T.st;
    const size_t n = (size_t)m->n_records;
    if (nm && n) SLX_HIPCHK(hipMemcpyAsync(nm, m->d_nm, 4 * n, hipMemcpyDeviceToHost, st));
    if (md_off) SLX_HIPCHK(hipMemcpyAsync(md_off, m->d_md_off, 8 * (n + 1), hipMemcpyDeviceToHost, st));
    if (md && m->md_bytes) SLX_HIPCHK(hipMemcpyAsync(md, m->d_md, (size_t)m->md_bytes, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    return SLX_OK;
}

// ------------------------------------------------------------------ host only
extern "C" int slx_ref_record_nm_md(const uint8_t *rec, int64_t n, const uint8_t *contig_bytes, int64_t contig_len, int32_t *nm, char *md, int64_t cap, int64_t *md_len)
{
    if (!rec || n < 0 || contig_len < 0 || (contig_len && !contig_bytes) || !nm || !md_len || cap < 0 || (cap && !md)) { slx_set_error("slx_ref_record_nm_md: null or negative argument"); return SLX_EINVAL; }
    uint64_t len = 0;
    const bool ok = rg_record_nm_md(rec, (uint64_t)n, contig_bytes, contig_len, nm, (uint8_t *)md, (uint64_t)cap, &len);
    *md_len = (int64_t)len;
    if (!ok) { slx_set_error("reference genome: the record's fields pass its block_size, or its extent is not block_size + 4"); return SLX_EIO; }
    return SLX_OK;
}

extern "C" int slx_ref_fai_of_text(const void *text, int64_t n, char **fai, int64_t *fai_len)
{
    if (n < 0 || (n && !text) || !fai || !fai_len) { slx_set_error("slx_ref_fai_of_text: null or negative argument"); return SLX_EINVAL; }
    *fai = nullptr; *fai_len = 0;
    std::vector<rg_contig> C;
    std::string msg;
    if (!rg_fai_of_text((const uint8_t *)text, (uint64_t)n, &C, &msg)) { slx_set_error("reference genome: %s", msg.c_str()); return SLX_EIO; }
    const std::string t = rg_fai_text(C);
    char *p = (char *)malloc(t.size() + 1);
    if (!p) { slx_set_error("slx_ref_fai_of_text: cannot allocate %zu bytes", t.size() + 1); return SLX_ENOMEM; }
    memcpy(p, t.c_str(), t.size() + 1);
    *fai = p; *fai_len = (int64_t)t.size();
    return SLX_OK;
}
extern "C" void slx_ref_text_free(char *p) { free(p); }
