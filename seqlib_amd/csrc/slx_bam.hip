// slx_bam.hip -- the BamReader path of libseqlib_amd.so (include/seqlib_amd_bam.h): BGZF members inflated, CRC-checked, cut into records and unpacked
// to the aligner's input on the GPU.  The host parses the member chain (18-byte headers, BSIZE, CRC32 + ISIZE trailers) and the BAM header; everything
// that touches the bulk of the bytes is a kernel:
//   k_bgzf_inflate   one wave per member, straight to the member's place in one contiguous stream (exclusive scan of ISIZE)      dev_inflate.h
//   k_bgzf_crc       one wave per member, a slice per lane, slices combined by x^(8n) mod P                                     dev_inflate.h
//   k_bam_guess / k_bam_round / k_bam_scan / k_bam_fill   record starts by speculate / verify / repair, one lane per chunk      dev_bamidx.h
//   k_bam_keep / k_bam_unpack   flag filter, 4-bit sequence -> ASCII (reverse complement on request), one wave per record
//   k_bai_rec / k_bai_heads / k_bai_chunks / k_bai_fill   the BAI index of a sorted file: ends, bins, virtual offsets, chunks, linear index   dev_bai.h
//   k_bam_region_keep / k_bam_gather   region iteration: records tested against the region, the kept ones compacted, one wave per record   dev_bai.h
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
#include "dev_bai.h"
#include "bai_host.h"
#include "sam_reader.h"
#include "slx_hip.h"

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

int slx_bgzf_inflate_members(const uint8_t *map, const char *path, const slx_bam_member *mem, int64_t a, int64_t b, bgzf_stage &S, uint8_t *d_out, uint64_t dst_off,
                             uint64_t out_bytes, hipStream_t st, hipEvent_t ev0, hipEvent_t ev_mid, hipEvent_t ev1, float us[2])
{
    const int n = (int)(b - a);
    if (n <= 0) return SLX_OK;
    uint64_t comp = 0;
    for (int64_t i = a; i < b; ++i) comp += mem[i].data_len;
    SLX_CHK(S.h_comp.ensure(comp + 8)); SLX_CHK(S.d_comp.ensure(comp + 8));
    SLX_CHK(S.h_desc.ensure(sizeof(bam_mdesc) * n)); SLX_CHK(S.d_desc.ensure(sizeof(bam_mdesc) * n));
    SLX_CHK(S.h_err.ensure(4 * (size_t)n)); SLX_CHK(S.d_err.ensure(4 * (size_t)n));
    bam_mdesc *d = S.h_desc.as<bam_mdesc>();
    uint64_t ci = 0, oo = dst_off;
    for (int64_t i = a; i < b; ++i) {
        const slx_bam_member &m = mem[i];
        memcpy(S.h_comp.as<uint8_t>() + ci, map + m.file_off + m.data_off, m.data_len);
        d[i - a] = bam_mdesc{ci, oo, m.data_len, m.isize, m.crc32, 0};
        ci += m.data_len; oo += m.isize;
    }
    if (oo > out_bytes) { slx_set_error("BGZF: internal: span of %llu bytes does not fit %llu", (unsigned long long)oo, (unsigned long long)out_bytes); return SLX_EINTERNAL; }
    SLX_HIPCHK(hipMemcpyAsync(S.d_comp.p, S.h_comp.p, comp, hipMemcpyHostToDevice, st));
    SLX_HIPCHK(hipMemcpyAsync(S.d_desc.p, S.h_desc.p, sizeof(bam_mdesc) * n, hipMemcpyHostToDevice, st));
    SLX_HIPCHK(hipEventRecord(ev0, st));
    k_bgzf_inflate<<<(n + 3) / 4, 256, 0, st>>>(S.d_comp.as<uint8_t>(), comp, S.d_desc.as<bam_mdesc>(), n, d_out, out_bytes, S.d_err.as<uint32_t>());
    SLX_HIPCHK(hipGetLastError());
    if (ev_mid) SLX_HIPCHK(hipEventRecord(ev_mid, st));
    k_bgzf_crc<<<(n + 3) / 4, 256, 0, st>>>(S.d_desc.as<bam_mdesc>(), n, d_out, out_bytes, S.d_err.as<uint32_t>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(ev1, st));
    SLX_HIPCHK(hipMemcpyAsync(S.h_err.p, S.d_err.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    if (ev_mid) { us[0] += slx_ev_us(ev0, ev_mid); us[1] += slx_ev_us(ev_mid, ev1); }
    else us[0] += slx_ev_us(ev0, ev1);
    const uint32_t *err = S.h_err.as<uint32_t>();
    for (int i = 0; i < n; ++i)
        if (err[i]) {
            slx_set_error("BGZF: '%s': the member at file offset %llu does not inflate: %s", path, (unsigned long long)mem[a + i].file_off, inf_errtext(err[i]));
            return SLX_EIO;
        }
    return SLX_OK;
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

// ---- the BAI build (dev_bai.h).  Per batch: k_bai_rec (fields, end, bin, virtual offsets, linear index, per-reference figures), k_bai_heads (run heads and the
// order check against the predecessor, the previous batch's last record included), a hipCUB sum of the heads, k_bai_chunks (one chunk per run; a run that is open
// at the end of a batch is closed provisionally and closed again by the next batch).  Once: hipCUB radix sort of the chunks by (tid, bin), k_bai_fill.
struct bai_dev {
    const uint64_t *ne_start, *ne_file; uint64_t nn, total, behind;      // the non-empty members
    const uint64_t *lin_off;                                             // n_ref + 1: first window of every reference in lin
    unsigned long long *lin, *ref_first, *ref_last, *n_map, *n_unmap;
    uint32_t *n_intv;
    int32_t n_ref;
};

// bst: [0] error bits, [1] ordinal of the first record out of order, [2] records with tid < 0
__global__ __launch_bounds__(256) void k_bai_rec(const uint8_t *s, const uint64_t *rec, uint64_t n_rec, uint64_t base_off, bai_dev d, unsigned long long *key, unsigned long long *tp,
                                                 unsigned long long *vbeg, unsigned long long *vend, unsigned long long *bst)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool active = r < n_rec;
    bai_fields f = {};
    uint64_t o0 = 0, o1 = 0;
    if (active) { o0 = rec[r]; o1 = rec[r + 1]; f = bai_read(s + o0); }
    const uint64_t reflen = bai_reflen_wave(f.cig, f.n_cig, active, lane);
    unsigned long long err = 0;
    if (active && !f.ok) err |= BAI_E_CIGAR;
    if (active && f.tid >= d.n_ref) { err |= BAI_E_TID; f.tid = -1; }
    const bool placed = active && f.tid >= 0;
    const int64_t pos = f.pos < 0 ? 0 : f.pos;
    int64_t end = bai_end(f.pos, f.flag, reflen);
    if (end <= pos) end = pos + 1;
    uint64_t vb = 0, ve = 0;
    uint64_t w0 = 0, w1 = 0, lo = 0;
    if (active) {
        tp[r] = (unsigned long long)(uint32_t)f.tid << 32 | ((uint32_t)f.pos ^ 0x80000000u);
        key[r] = placed ? (unsigned long long)(uint32_t)f.tid << 32 | bai_reg2bin(pos, end) : BAI_NOKEY;
    }
    if (placed) {
        vb = bai_voff(d.ne_start, d.ne_file, d.nn, d.total, d.behind, base_off + o0);
        ve = bai_voff(d.ne_start, d.ne_file, d.nn, d.total, d.behind, base_off + o1);
        vbeg[r] = vb; vend[r] = ve;
        lo = d.lin_off[f.tid];
        const uint64_t cap = d.lin_off[f.tid + 1] - lo;
        w0 = (uint64_t)pos >> 14; w1 = (uint64_t)(end - 1) >> 14;
        if (w1 >= cap) { err |= BAI_E_SPAN; w1 = cap - 1; if (w0 > w1) w0 = w1; }
        atomicMax(&d.n_intv[f.tid], (uint32_t)(w1 + 1));
    }
    if (err) atomicOr(&bst[0], err);
    // the linear index: a record's few windows on its own lane, a long span (an N of megabases) by the whole wave
    const bool wide = placed && w1 - w0 >= BAI_COOP_WINS;
    if (placed && !wide) for (uint64_t w = w0; w <= w1; ++w) atomicMin(&d.lin[lo + w], (unsigned long long)vb);
    for (unsigned long long m = __ballot(wide); m; m &= m - 1) {
        const int src = __ffsll(m) - 1;
        const uint64_t a = __shfl((unsigned long long)(lo + w0), src, 64), b = __shfl((unsigned long long)(lo + w1), src, 64), v = __shfl((unsigned long long)vb, src, 64);
        for (uint64_t w = a + lane; w <= b; w += 64) atomicMin(&d.lin[w], (unsigned long long)v);
    }
    // per-reference figures: a wave's records almost always share one reference, and then one lane speaks for all of them
    const unsigned long long pm = __ballot(placed);
    const unsigned long long nc = __ballot(active && !placed);
    if (lane == 0 && nc) atomicAdd(&bst[2], (unsigned long long)__popcll(nc));
    if (pm) {
        const int first = __ffsll(pm) - 1;
        const int32_t t0 = __shfl(f.tid, first, 64);
        const bool unm = (f.flag & 4u) != 0;
        if (__all(!placed || f.tid == t0)) {
            const unsigned long long mu = __ballot(placed && unm);
            unsigned long long mn = placed ? vb : ~0ull, mx = placed ? ve : 0ull;
            for (int o = 32; o; o >>= 1) {
                const unsigned long long a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64);
                mn = a < mn ? a : mn; mx = b > mx ? b : mx;
            }
            if (lane == first) {
                atomicMin(&d.ref_first[t0], mn); atomicMax(&d.ref_last[t0], mx);
                if (pm & ~mu) atomicAdd(&d.n_map[t0], (unsigned long long)__popcll(pm & ~mu));
                if (mu) atomicAdd(&d.n_unmap[t0], (unsigned long long)__popcll(mu));
            }
        } else if (placed) {
            atomicMin(&d.ref_first[f.tid], (unsigned long long)vb); atomicMax(&d.ref_last[f.tid], (unsigned long long)ve);
            atomicAdd(unm ? &d.n_unmap[f.tid] : &d.n_map[f.tid], 1ull);
        }
    }
}

// head[i] = record i opens a chunk; carry_in / carry_out: (key, tid-pos word) of the previous / this batch's last record
__global__ void k_bai_heads(const unsigned long long *key, const unsigned long long *tp, uint64_t n_rec, uint64_t ord_base, const unsigned long long *carry_in,
                            unsigned long long *carry_out, unsigned long long *head, unsigned long long *bst)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rec) return;
    if (r == n_rec) { head[r] = 0; return; }
    const unsigned long long pk = r ? key[r - 1] : carry_in[0], pt = r ? tp[r - 1] : carry_in[1];
    if (tp[r] < pt) atomicMin(&bst[1], (unsigned long long)(ord_base + r));
    head[r] = key[r] != BAI_NOKEY && key[r] != pk;
    if (r == n_rec - 1) { carry_out[0] = key[r]; carry_out[1] = tp[r]; }
}

__global__ void k_bai_chunks(const unsigned long long *key, const unsigned long long *vbeg, const unsigned long long *vend, const unsigned long long *head, const unsigned long long *hidx,
                             uint64_t n_rec, uint64_t chunk_base, uint64_t cap, unsigned long long *ckey, unsigned long long *cbeg, unsigned long long *cend)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rec || key[r] == BAI_NOKEY) return;
    const uint64_t slot = chunk_base + hidx[r] + head[r] - 1;          // a record that continues the previous batch's open run: chunk_base - 1
    if (slot >= cap) return;
    if (head[r]) { ckey[slot] = key[r]; cbeg[slot] = vbeg[r]; }
    if (r == n_rec - 1 || key[r + 1] != key[r]) cend[slot] = vend[r];
}

__global__ void k_bai_iota(uint32_t *v, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = (uint32_t)i;
}

// one wave per reference: a window no record touched takes the value of the next touched window above it, 64 windows at a time from the top
__global__ __launch_bounds__(64) void k_bai_fill(bai_dev d)
{
    const int t = blockIdx.x, lane = threadIdx.x;
    if (t >= d.n_ref) return;
    const uint64_t lo = d.lin_off[t], n = d.n_intv[t];
    unsigned long long above = 0;
    for (uint64_t top = n; top > 0; top = top > 64 ? top - 64 : 0) {
        const int64_t w = (int64_t)top - 64 + lane;                     // lanes 0..63 hold windows top-64 .. top-1
        unsigned long long v = w >= 0 ? d.lin[lo + w] : ~0ull;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long up = __shfl_down(v, o, 64);
            if (v == ~0ull && lane + o < 64) v = up;
        }
        if (v == ~0ull) v = above;
        if (w >= 0) d.lin[lo + w] = v;
        above = __shfl(v, top >= 64 ? 0 : (int)(64 - top), 64);       // the lowest window of this tile
    }
}

// ---- the region filter: keep[i] = record i of the span overlaps the region (the end as in the index build), klen[i] = its bytes when kept
__global__ __launch_bounds__(256) void k_bam_region_keep(const uint8_t *s, const uint64_t *rec, uint64_t n_rec, int32_t tid, int64_t beg, int64_t end, unsigned long long *keep,
                                                         unsigned long long *klen, unsigned long long *bst)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool active = r < n_rec;
    bai_fields f = {};
    if (active) f = bai_read(s + rec[r]);
    const uint64_t reflen = bai_reflen_wave(f.cig, f.n_cig, active, lane);
    if (r == n_rec) { keep[r] = 0; klen[r] = 0; }
    if (!active) return;
    if (!f.ok) atomicOr(&bst[0], BAI_E_CIGAR);
    const bool k = f.ok && f.tid == tid && (int64_t)f.pos < end && bai_end(f.pos, f.flag, reflen) > beg;
    keep[r] = k; klen[r] = k ? rec[r + 1] - rec[r] : 0;
}

// the kept records, bytes unchanged, one wave per record, to dst at the places the two exclusive sums give
__global__ __launch_bounds__(256) void k_bam_gather(const uint8_t *s, const uint64_t *rec, uint64_t n_rec, const unsigned long long *kidx, const unsigned long long *koff, uint8_t *dst,
                                                    uint64_t *dst_rec, uint64_t rec_base, uint64_t byte_base)
{
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n_rec) return;
    if (r == 0 && lane == 0) dst_rec[rec_base + kidx[n_rec]] = byte_base + koff[n_rec];
    if (kidx[r + 1] == kidx[r]) return;
    const uint64_t len = koff[r + 1] - koff[r];
    const uint8_t *src = s + rec[r];
    uint8_t *o = dst + byte_base + koff[r];
    if (lane == 0) dst_rec[rec_base + kidx[r]] = byte_base + koff[r];
    for (uint64_t i = lane; i < len; i += 64) o[i] = src[i];
}

// a read filter attached to the reader (slx_filter.hip): its keep bytes become the keep / length words the two exclusive sums take; and_mode: on top of the region test
__global__ void k_bam_keep_bytes(const uint8_t *fk, const uint64_t *rec, uint64_t n_rec, int and_mode, unsigned long long *keep, unsigned long long *klen)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rec) return;
    if (r == n_rec) { keep[r] = 0; klen[r] = 0; return; }
    const bool k = fk[r] != 0 && (!and_mode || keep[r] != 0);
    keep[r] = k; klen[r] = k ? rec[r + 1] - rec[r] : 0;
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
    SLX_CHK(bam_scan(path, f));
    slx_bam_member *m = (slx_bam_member *)malloc(sizeof(slx_bam_member) * f.mem.size());
    if (!m) { slx_set_error("out of memory"); return SLX_ENOMEM; }
    memcpy(m, f.mem.data(), sizeof(slx_bam_member) * f.mem.size());
    *members = m; *n_members = (int64_t)f.mem.size();
    if (has_eof) *has_eof = f.has_eof;
    return SLX_OK;
}
extern "C" void slx_bam_members_free(slx_bam_member *members) { free(members); }

// ------------------------------------------------------------------ host: the device side
// the reader's buffers in HBM and pinned: a margin of 1/4 + 256 bytes on every growth, kept as found
typedef SlxDevBuf<SlxMargin<4, 256>> BamDBuf;
typedef SlxPinBuf<SlxMargin<4, 256>> BamHBuf;

struct slx_bam : SlxGpu<10> {
    BamFile f;
    std::string text;
    std::vector<std::string> ref_names;
    std::vector<int64_t> ref_lens;
    int64_t first_member = 0, next_member = 0;
    std::vector<uint8_t> carry0, carry;
    uint64_t chunk_bytes = 65536;
    int idx_fail = 0;
    bgzf_stage stage;                                      // slx_bgzf_inflate_members' buffers
    BamDBuf d_out{*this}, d_guess{*this}, d_used{*this}, d_exit_a{*this}, d_exit_b{*this}, d_count{*this}, d_base{*this}, d_state{*this}, d_rec{*this}, d_keep{*this}, d_blen{*this},
            d_kidx{*this}, d_boff{*this}, d_tmp{*this}, d_bases{*this}, d_offs{*this}, d_map{*this};
    BamDBuf d_cs{*this}, d_cr{*this};                      // region mode: the kept records compacted, and their offsets
    BamHBuf h_out{*this}, h_rec{*this}, h_state{*this}, h_map{*this};
    int64_t c_members_done = 0, c_repaired = 0, c_rounds = 0, c_records = 0, c_region_cand = 0, c_region_kept = 0;
    float us[5] = {0, 0, 0, 0, 0};
    const void *map_stream = nullptr; int64_t map_reads = 0; // the batch slx_bam_reads_device last unpacked (d_bases, d_offs, d_map hold its reads), and how many
    const void *cur_stream = nullptr, *cur_rec = nullptr;  // what the current batch points to: d_out / d_rec, or d_cs / d_cr for a region batch
    // region iteration: the index, the regions in the order given, and their chunks as member spans
    bool has_bai = false;
    Bai bai;
    struct Piece { int64_t region, ma, mb; uint64_t start, tail_cut; };      // members [ma, mb): the first record at start of ma, the last tail_cut bytes of mb - 1 left out
    std::vector<slx_bam_region> regions;
    std::vector<Piece> pieces;
    size_t piece_i = 0;
    int64_t piece_cur = -1;                                // next member of pieces[piece_i]; -1: not begun
    bool region_mode = false;
    slx_filter *flt = nullptr;                             // a read filter attached by slx_filter_attach; nullptr: nothing new is launched
    BamDBuf d_fkeep{*this};                                     // its keep bytes
    slx_samsrc *sam = nullptr;                             // a reader over SAM text (slx_sam_open): the batches come from slx_sam.hip, there are no members
};

static int bam_dev_init(slx_bam *rd, int device)
{
    return rd->open(device, "BAM reader", "no HIP device: the BAM reader inflates and indexes on MI355X only (no CPU fallback)");
}

static void bam_dev_free(slx_bam *rd)
{
    if (rd->st) {
        (void)hipSetDevice(rd->device);
        (void)hipStreamSynchronize(rd->st);
    }
    rd->stage.release();          // (dev_inflate.h's staging buffers: they have no owner, the stream has drained)
    rd->close();
}

// members [a, b) inflated to d_out[dst_off ..), CRC-checked; d_out holds out_bytes.  Returns after the stream has drained.
static int bam_inflate_span(slx_bam *rd, int64_t a, int64_t b, uint64_t dst_off, uint64_t out_bytes)
{
    SLX_CHK(slx_bgzf_inflate_members(rd->f.map, rd->f.path.c_str(), rd->f.mem.data(), a, b, rd->stage, rd->d_out.as<uint8_t>(), dst_off, out_bytes, rd->st, rd->ev[0], rd->ev[1], rd->ev[2], rd->us));
    if (b > a) rd->c_members_done += b - a;
    return SLX_OK;
}

// record starts of d_out[start, start + n), the first record at start: d_rec gets n_rec + 1 offsets from start (the last one = end of the last whole record)
static int bam_index(slx_bam *rd, uint64_t start, uint64_t n, int32_t n_ref, uint64_t *n_rec, uint64_t *end, uint64_t *repaired)
{
    hipStream_t st = rd->st;
    const uint64_t chunk = rd->chunk_bytes, K = (n + chunk - 1) / chunk;
    *n_rec = 0; *end = 0; *repaired = 0;
    if (!K) return SLX_OK;
    for (BamDBuf *b : {&rd->d_guess, &rd->d_used, &rd->d_exit_a, &rd->d_exit_b, &rd->d_base}) SLX_CHK(b->ensure(8 * K));
    SLX_CHK(rd->d_count.ensure(4 * K)); SLX_CHK(rd->d_state.ensure(64)); SLX_CHK(rd->h_state.ensure(64));
    unsigned long long *hs = rd->h_state.as<unsigned long long>(), *ds = rd->d_state.as<unsigned long long>();
    hs[0] = 0; hs[1] = 0; hs[2] = ~0ull; hs[3] = 0; hs[4] = 0;
    SLX_HIPCHK(hipMemcpyAsync(ds, hs, 40, hipMemcpyHostToDevice, st));
    SLX_HIPCHK(hipEventRecord(rd->ev[3], st));
    const uint8_t *s = rd->d_out.as<uint8_t>() + start;
    const unsigned grid = (unsigned)((K + 63) / 64);
    uint64_t *ex_a = rd->d_exit_a.as<uint64_t>(), *ex_b = rd->d_exit_b.as<uint64_t>();
    k_bam_guess<<<grid, 64, 0, st>>>(s, n, chunk, K, n_ref, rd->idx_fail, rd->d_guess.as<uint64_t>(), rd->d_used.as<uint64_t>(), ex_a, rd->d_count.as<uint32_t>());
    SLX_HIPCHK(hipGetLastError());
    for (uint64_t round = 0; K > 1; ++round) {
        if (round > K) { slx_set_error("BAM reader: internal: the record index did not settle in %llu rounds", (unsigned long long)K); return SLX_EINTERNAL; }
        if (round) SLX_HIPCHK(hipMemsetAsync(ds + 4, 0, 8, st));
        k_bam_round<<<grid, 64, 0, st>>>(s, n, chunk, K, rd->d_used.as<uint64_t>(), ex_a, ex_b, rd->d_count.as<uint32_t>(), ds);
        SLX_HIPCHK(hipGetLastError());
        SLX_HIPCHK(hipMemcpyAsync(hs + 4, ds + 4, 8, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(slx_wait_stream(st));
        std::swap(ex_a, ex_b);
        ++rd->c_rounds;
        if (!hs[4]) break;
    }
    k_bam_scan<<<1, 1024, 0, st>>>(rd->d_count.as<uint32_t>(), rd->d_base.as<uint64_t>(), K, ds);
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipMemcpyAsync(hs, ds, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    const uint64_t nr = hs[0];
    SLX_CHK(rd->d_rec.ensure(8 * (nr + 1)));
    k_bam_fill<<<grid, 64, 0, st>>>(s, n, chunk, K, ex_a, rd->d_guess.as<uint64_t>(), rd->d_base.as<uint64_t>(), rd->d_rec.as<uint64_t>(), ds);
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(rd->ev[4], st));
    SLX_HIPCHK(hipMemcpyAsync(hs, ds, 32, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    rd->us[2] += slx_ev_us(rd->ev[3], rd->ev[4]);
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
            SLX_CHK(rd->d_out.ensure(bytes + 8));
            SLX_CHK(bam_inflate_span(rd, b, e, 0, bytes));
            const size_t at = h.size();
            h.resize(at + bytes);
            if (bytes) { SLX_HIPCHK(hipMemcpyAsync(h.data() + at, rd->d_out.p, bytes, hipMemcpyDeviceToHost, rd->st)); SLX_HIPCHK(hipStreamSynchronize(rd->st)); }
            b = e;
        }
        return SLX_OK;
    };
    SLX_CHK(need(12));
    if (memcmp(h.data(), "BAM\1", 4) != 0) { slx_set_error("BAM: '%s' is BGZF but does not hold a BAM stream (bad magic; SAM text and CRAM are not read)", rd->f.path.c_str()); return SLX_EIO; }
    const uint64_t l_text = bidx_u32(h.data() + 4);
    if (l_text > (1ull << 31)) { slx_set_error("BAM: '%s': header text length %llu", rd->f.path.c_str(), (unsigned long long)l_text); return SLX_EIO; }
    SLX_CHK(need(12 + l_text));
    rd->text.assign((const char *)h.data() + 8, l_text);
    while (!rd->text.empty() && rd->text.back() == '\0') rd->text.pop_back();
    const int32_t n_ref = (int32_t)bidx_u32(h.data() + 8 + l_text);
    if (n_ref < 0) { slx_set_error("BAM: '%s': negative reference count", rd->f.path.c_str()); return SLX_EIO; }
    uint64_t p = 12 + l_text;
    for (int32_t i = 0; i < n_ref; ++i) {
        SLX_CHK(need(p + 4));
        const uint64_t l_name = bidx_u32(h.data() + p);
        if (l_name < 1 || l_name > (1u << 20)) { slx_set_error("BAM: '%s': reference %d has name length %llu", rd->f.path.c_str(), i, (unsigned long long)l_name); return SLX_EIO; }
        SLX_CHK(need(p + 4 + l_name + 4));
        rd->ref_names.emplace_back((const char *)h.data() + p + 4, strnlen((const char *)h.data() + p + 4, l_name));
        rd->ref_lens.push_back((int64_t)bidx_u32(h.data() + p + 4 + l_name));
        p += 8 + l_name;
    }
    rd->first_member = b;
    rd->carry0.assign(h.begin() + p, h.end());
    return SLX_OK;
}

static bool file_exists(const std::string &p) { struct stat sb; return stat(p.c_str(), &sb) == 0 && S_ISREG(sb.st_mode); }

// the index next to the file: <path>.bai, then <path> with ".bam" replaced by ".bai"; "" when neither is there
static std::string bai_beside(const std::string &path)
{
    if (file_exists(path + ".bai")) return path + ".bai";
    if (path.size() > 4 && path.compare(path.size() - 4, 4, ".bam") == 0 && file_exists(path.substr(0, path.size() - 4) + ".bai")) return path.substr(0, path.size() - 4) + ".bai";
    return "";
}

static int bam_load_index(slx_bam *rd, const std::string &bai_path)
{
    Bai b;
    SLX_CHK(bai_load_file(bai_path.c_str(), b));
    if (b.refs.size() != rd->ref_names.size()) {
        slx_set_error("BAI: '%s' indexes %zu references, the header of '%s' has %zu: not this file's index", bai_path.c_str(), b.refs.size(), rd->f.path.c_str(), rd->ref_names.size());
        return SLX_EINVAL;
    }
    rd->bai = std::move(b); rd->has_bai = true;
    return SLX_OK;
}

static int bam_open_impl(const char *path, int device, slx_bam **out, bool try_index)
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
    if (try_index) {                     // as sam_index_load in the reference's Open (src/BamReader.cpp:33): a missing index is no error, a wrong one is said and left out
        const std::string bp = bai_beside(rd->f.path);
        if (!bp.empty() && bam_load_index(rd, bp) != SLX_OK) fprintf(stderr, "[W::slx_bam_open] index not loaded: %s\n", slx_last_error());
    }
    *out = rd;
    return SLX_OK;
}

extern "C" int slx_bam_open(const char *path, int device, slx_bam **out) { return bam_open_impl(path, device, out, true); }

extern "C" int slx_bam_index_load(slx_bam *rd, const char *bai_path)
{
    if (!rd) { slx_set_error("slx_bam_index_load: reader is null"); return SLX_EINVAL; }
    if (rd->sam) { slx_set_error("slx_bam_index_load: '%s': SAM text has no index", rd->f.path.c_str()); return SLX_EINVAL; }
    std::string bp = bai_path ? std::string(bai_path) : bai_beside(rd->f.path);
    if (bp.empty()) { slx_set_error("BAI: no index beside '%s' (<path>.bai, or .bai in place of .bam)", rd->f.path.c_str()); return SLX_EIO; }
    return bam_load_index(rd, bp);
}
extern "C" int slx_bam_has_index(const slx_bam *rd) { return rd && rd->has_bai ? 1 : 0; }

static void bam_whole_file(slx_bam *rd)
{
    rd->region_mode = false; rd->regions.clear(); rd->pieces.clear(); rd->piece_i = 0; rd->piece_cur = -1;
    rd->next_member = rd->first_member; rd->carry = rd->carry0;
}

extern "C" int slx_bam_set_regions(slx_bam *rd, const slx_bam_region *regs, int64_t n)
{
    if (!rd || n < 0 || (n && !regs)) { slx_set_error("slx_bam_set_regions: null argument"); return SLX_EINVAL; }
    if (rd->sam) { slx_set_error("slx_bam_set_regions: '%s': SAM text has no index", rd->f.path.c_str()); return SLX_EINVAL; }
    if (n == 0) { bam_whole_file(rd); return SLX_OK; }
    if (!rd->has_bai) { slx_set_error("slx_bam_set_regions: '%s' has no index loaded (slx_bam_index_build writes one, slx_bam_index_load reads it)", rd->f.path.c_str()); return SLX_EINVAL; }
    const int64_t nm = (int64_t)rd->f.mem.size();
    auto member_at = [&](uint64_t file_off) -> int64_t {                 // the member that begins at file_off; nm for the end of the file; -1: none
        if (file_off == rd->f.size) return nm;
        int64_t lo = 0, hi = nm;
        while (lo < hi) { const int64_t mid = (lo + hi) / 2; if (rd->f.mem[mid].file_off < file_off) lo = mid + 1; else hi = mid; }
        return lo < nm && rd->f.mem[lo].file_off == file_off ? lo : -1;
    };
    std::vector<slx_bam::Piece> pieces;
    std::vector<std::pair<uint64_t, uint64_t>> ch;
    for (int64_t i = 0; i < n; ++i) {
        if (regs[i].tid < 0 || regs[i].tid >= (int32_t)rd->ref_names.size()) { slx_set_error("slx_bam_set_regions: region %lld names reference %d, the header has %zu", (long long)i, regs[i].tid, rd->ref_names.size()); return SLX_EINVAL; }
        bai_plan(rd->bai, regs[i].tid, regs[i].beg, regs[i].end, ch);
        for (const auto &c : ch) {
            slx_bam::Piece P;
            P.region = i; P.ma = member_at(c.first >> 16); P.start = c.first & 0xffff;
            const int64_t mv = member_at(c.second >> 16);
            const uint64_t within = c.second & 0xffff;
            bool ok = P.ma >= 0 && P.ma < nm && mv >= 0 && (within == 0 || (mv < nm && within <= rd->f.mem[mv].isize));
            if (ok) {
                P.mb = within ? mv + 1 : mv;
                P.tail_cut = within ? rd->f.mem[mv].isize - within : 0;
                ok = P.mb >= P.ma && P.start <= rd->f.mem[P.ma].isize;
            }
            if (!ok) { slx_set_error("BAI: the index does not fit '%s': chunk %llx - %llx names no member of the file", rd->f.path.c_str(), (unsigned long long)c.first, (unsigned long long)c.second); return SLX_EIO; }
            if (P.mb > P.ma) pieces.push_back(P);
        }
    }
    bam_whole_file(rd);
    rd->regions.assign(regs, regs + n); rd->pieces.swap(pieces);
    rd->region_mode = true; rd->carry.clear();
    return SLX_OK;
}

extern "C" void slx_bam_close(slx_bam *rd)
{
    if (!rd) return;
    if (rd->sam) slx_samsrc_close(rd->sam);
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
    if (rd->sam) SLX_CHK(slx_samsrc_rewind(rd->sam));
    bam_whole_file(rd);                  // the regions go too: the reference's Reset reopens the file (src/BamReader.cpp:56-62)
    return SLX_OK;
}

extern "C" int slx_bam_set(slx_bam *rd, const char *key, int64_t value)
{
    if (!rd || !key) { slx_set_error("slx_bam_set: null argument"); return SLX_EINVAL; }
    const std::string k(key);
    int sam_rc = SLX_OK;
    if (rd->sam && slx_samsrc_set(rd->sam, key, value, &sam_rc)) return sam_rc;
    if (k == "chunk_bytes" && value >= 64 && value <= (1ll << 30)) { rd->chunk_bytes = (uint64_t)value; return SLX_OK; }
    if (k == "idx_fail" && (value == 0 || value == 1)) { rd->idx_fail = (int)value; return SLX_OK; }
    slx_set_error("slx_bam_set: unknown key or value out of range: %s = %lld", key, (long long)value);
    return SLX_EINVAL;
}

extern "C" int64_t slx_bam_counter(const slx_bam *rd, const char *name)
{
    if (!rd || !name) return -1;
    const std::string k(name);
    int64_t sam_v = 0;
    if (rd->sam && slx_samsrc_counter(rd->sam, name, &sam_v)) return sam_v;
    if (k == "sam") return 0;
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
    if (k == "us_region") return (int64_t)rd->us[4];
    if (k == "regions_done") return !rd->region_mode ? 0 : rd->piece_i < rd->pieces.size() ? rd->pieces[rd->piece_i].region : (int64_t)rd->regions.size();
    if (k == "region_candidates") return rd->c_region_cand;
    if (k == "region_kept") return rd->c_region_kept;
    return -1;
}

// One span of members from a towards lim behind rd->carry: at least one member, then members while the span stays within max_bytes; a span without one whole
// record doubles.  The first record stands at start; when the span reaches lim, its last tail_cut bytes are left out.  On return d_out[start, *n) holds the
// span, d_rec the n_rec + 1 record offsets from start, *end the bytes of the whole records (from start).
static int bam_span(slx_bam *rd, int64_t max_bytes, int64_t a, int64_t lim, uint64_t start, uint64_t tail_cut, int64_t *done_out, uint64_t *n_out, uint64_t *n_rec, uint64_t *end,
                    uint64_t *repaired)
{
    hipStream_t st = rd->st;
    if (max_bytes < 1) max_bytes = 1;
    uint64_t total = rd->carry.size();
    SLX_CHK(rd->d_out.ensure(total + 8));
    if (total) SLX_HIPCHK(hipMemcpyAsync(rd->d_out.p, rd->carry.data(), total, hipMemcpyHostToDevice, st));
    SLX_HIPCHK(hipStreamSynchronize(st));
    int64_t done = a, b = a;
    *n_rec = 0; *end = 0; *repaired = 0;
    for (;;) {
        // the span: at least one member, then while it stays within max_bytes; a span without one whole record doubles
        uint64_t bytes = total;
        if (b == done) { while (b < lim && (b == done || bytes + rd->f.mem[b].isize <= (uint64_t)max_bytes)) bytes += rd->f.mem[b++].isize; }
        uint64_t span = 0;
        for (int64_t i = done; i < b; ++i) span += rd->f.mem[i].isize;
        SLX_CHK(rd->d_out.ensure(total + span + 8, st, total));
        SLX_CHK(bam_inflate_span(rd, done, b, total, total + span));
        total += span; done = b;
        const uint64_t cut = done >= lim ? tail_cut : 0;
        if (total < start + cut) { slx_set_error("BAM: '%s': the index does not fit the file (a chunk of %llu bytes begins at %llu and leaves out %llu)", rd->f.path.c_str(), (unsigned long long)total, (unsigned long long)start, (unsigned long long)cut); return SLX_EIO; }
        *n_out = total - cut;
        SLX_CHK(bam_index(rd, start, *n_out - start, (int32_t)rd->ref_names.size(), n_rec, end, repaired));
        if (*n_rec || done >= lim) break;
        b = std::min(lim, done + std::max<int64_t>(1, done - a));
    }
    *done_out = done;
    return SLX_OK;
}

// rd->carry = d_out[from, upto), enqueued
static int bam_take_carry(slx_bam *rd, uint64_t from, uint64_t upto)
{
    rd->carry.resize(upto - from);
    if (upto > from) SLX_HIPCHK(hipMemcpyAsync(rd->carry.data(), rd->d_out.as<uint8_t>() + from, upto - from, hipMemcpyDeviceToHost, rd->st));
    return SLX_OK;
}

// a batch of the regions: spans of the pieces' members, their records tested against the region and the kept ones compacted behind one another in d_cs / d_cr
static int bam_next_regions(slx_bam *rd, int64_t max_bytes, slx_bam_batch *out)
{
    typedef unsigned long long ull;
    hipStream_t st = rd->st;
    if (max_bytes < 1) max_bytes = 1;
    SLX_CHK(rd->d_state.ensure(64)); SLX_CHK(rd->h_state.ensure(64));
    ull *hs = rd->h_state.as<ull>(), *ds = rd->d_state.as<ull>();
    uint64_t kept = 0, bytes = 0, used = 0, repaired = 0;
    int64_t members = 0;
    while (rd->piece_i < rd->pieces.size()) {
        const slx_bam::Piece &P = rd->pieces[rd->piece_i];
        if (rd->piece_cur < 0) { rd->piece_cur = P.ma; rd->carry.clear(); }
        const int64_t a = rd->piece_cur;
        // as many regions as fit max_bytes; a batch without a kept record goes on, since n_records == 0 is the end of the last region
        if (kept && used + rd->carry.size() + rd->f.mem[a].isize > (uint64_t)max_bytes) break;
        const int64_t room = kept && used < (uint64_t)max_bytes ? max_bytes - (int64_t)used : max_bytes;
        const uint64_t start = a == P.ma ? P.start : 0;
        int64_t done = a;
        uint64_t n = 0, n_rec = 0, end = 0, rep = 0;
        SLX_CHK(bam_span(rd, room, a, P.mb, start, P.tail_cut, &done, &n, &n_rec, &end, &rep));
        for (int64_t i = a; i < done; ++i) used += rd->f.mem[i].isize;
        members += done - a; repaired += rep;
        if (done >= P.mb) {
            if (start + end != n) { slx_set_error("BAM: '%s': the index does not fit the file (the chunk that ends in the member at %llu ends inside a record)", rd->f.path.c_str(), (unsigned long long)rd->f.mem[P.mb - 1].file_off); return SLX_EIO; }
            rd->carry.clear();
        } else SLX_CHK(bam_take_carry(rd, start + end, n));
        if (n_rec) {
            const slx_bam_region &g = rd->regions[P.region];
            for (BamDBuf *b : {&rd->d_keep, &rd->d_blen, &rd->d_kidx, &rd->d_boff}) SLX_CHK(b->ensure(8 * (n_rec + 1)));
            SLX_HIPCHK(hipMemsetAsync(ds + 5, 0, 8, st));
            SLX_HIPCHK(hipEventRecord(rd->ev[7], st));
            const uint8_t *s = rd->d_out.as<uint8_t>() + start;
            const uint64_t *rec = rd->d_rec.as<uint64_t>();
            k_bam_region_keep<<<(unsigned)((n_rec + 1 + 255) / 256), 256, 0, st>>>(s, rec, n_rec, g.tid, g.beg, g.end, rd->d_keep.as<ull>(), rd->d_blen.as<ull>(), ds + 5);
            SLX_HIPCHK(hipGetLastError());
            if (rd->flt) {                                 // keep = region test AND filter
                SLX_CHK(rd->d_fkeep.ensure(n_rec + 8));
                SLX_CHK(slx_filter_eval_device(rd->flt, rd->device, st, s, rec, n_rec, end, rd->d_fkeep.as<uint8_t>(), nullptr));
                k_bam_keep_bytes<<<(unsigned)((n_rec + 1 + 255) / 256), 256, 0, st>>>(rd->d_fkeep.as<uint8_t>(), rec, n_rec, 1, rd->d_keep.as<ull>(), rd->d_blen.as<ull>());
                SLX_HIPCHK(hipGetLastError());
            }
            SLX_CHK(slx_exclusive_sum(rd->d_tmp, rd->d_keep.as<ull>(), rd->d_kidx.as<ull>(), n_rec + 1, st, 8));
            SLX_CHK(slx_exclusive_sum(rd->d_tmp, rd->d_blen.as<ull>(), rd->d_boff.as<ull>(), n_rec + 1, st, 8));
            SLX_HIPCHK(hipMemcpyAsync(hs + 5, rd->d_kidx.as<ull>() + n_rec, 8, hipMemcpyDeviceToHost, st));
            SLX_HIPCHK(hipMemcpyAsync(hs + 6, rd->d_boff.as<ull>() + n_rec, 8, hipMemcpyDeviceToHost, st));
            SLX_HIPCHK(hipMemcpyAsync(hs + 7, ds + 5, 8, hipMemcpyDeviceToHost, st));
            SLX_HIPCHK(slx_wait_stream(st));
            if (hs[7]) { slx_set_error("BAM: '%s': a record's name and CIGAR pass its block_size", rd->f.path.c_str()); return SLX_EIO; }
            const uint64_t kn = hs[5], kb = hs[6];
            SLX_CHK(rd->d_cs.ensure(bytes + kb + 8, st, bytes)); SLX_CHK(rd->d_cr.ensure(8 * (kept + kn + 1), st, 8 * kept));
            k_bam_gather<<<(unsigned)((n_rec + 3) / 4), 256, 0, st>>>(s, rec, n_rec, rd->d_kidx.as<ull>(), rd->d_boff.as<ull>(), rd->d_cs.as<uint8_t>(), rd->d_cr.as<uint64_t>(), kept, bytes);
            SLX_HIPCHK(hipGetLastError());
            SLX_HIPCHK(hipEventRecord(rd->ev[8], st));
            SLX_HIPCHK(slx_wait_stream(st));
            rd->us[4] += slx_ev_us(rd->ev[7], rd->ev[8]);
            kept += kn; bytes += kb;
            rd->c_region_cand += (int64_t)n_rec; rd->c_region_kept += (int64_t)kn;
        } else SLX_HIPCHK(slx_wait_stream(st));
        if (done >= P.mb) { ++rd->piece_i; rd->piece_cur = -1; }
        else { rd->piece_cur = done; if (kept) break; used = 0; }
    }
    rd->c_repaired += (int64_t)repaired; rd->c_records += (int64_t)kept;
    if (kept) {
        SLX_CHK(rd->h_out.ensure(bytes + 8)); SLX_CHK(rd->h_rec.ensure(8 * (kept + 1)));
        SLX_HIPCHK(hipMemcpyAsync(rd->h_out.p, rd->d_cs.p, bytes, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(hipMemcpyAsync(rd->h_rec.p, rd->d_cr.p, 8 * (kept + 1), hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(slx_wait_stream(st));
    }
    out->n_records = (int64_t)kept; out->n_bytes = (int64_t)bytes;
    out->stream = rd->h_out.as<uint8_t>(); out->rec_off = rd->h_rec.as<uint64_t>();
    out->d_stream = rd->d_cs.p; out->d_rec_off = rd->d_cr.p;
    out->n_members = members; out->n_repaired_chunks = (int64_t)repaired;
    rd->cur_stream = rd->d_cs.p; rd->cur_rec = rd->d_cr.p; rd->map_stream = nullptr;
    return SLX_OK;
}

// the attached filter's verdicts on the n_rec records of s[0, end) (offsets rec, all in HBM), and the kept ones compacted into d_cs / d_cr, bytes unchanged: *kn of
// them in *kb bytes (the gather is still in flight on return).
static int bam_filter_compact(slx_bam *rd, const uint8_t *s, const uint64_t *rec, uint64_t n_rec, uint64_t end, uint64_t *kn_out, uint64_t *kb_out)
{
    typedef unsigned long long ull;
    hipStream_t st = rd->st;
    SLX_CHK(rd->h_state.ensure(64));
    ull *hs = rd->h_state.as<ull>();
    uint64_t kn = 0, kb = 0;
    *kn_out = *kb_out = 0;
    for (BamDBuf *b : {&rd->d_keep, &rd->d_blen, &rd->d_kidx, &rd->d_boff}) SLX_CHK(b->ensure(8 * (n_rec + 1)));
    SLX_CHK(rd->d_fkeep.ensure(n_rec + 8));
    SLX_CHK(slx_filter_eval_device(rd->flt, rd->device, st, s, rec, n_rec, end, rd->d_fkeep.as<uint8_t>(), nullptr));
    k_bam_keep_bytes<<<(unsigned)((n_rec + 1 + 255) / 256), 256, 0, st>>>(rd->d_fkeep.as<uint8_t>(), rec, n_rec, 0, rd->d_keep.as<ull>(), rd->d_blen.as<ull>());
    SLX_HIPCHK(hipGetLastError());
    SLX_CHK(slx_exclusive_sum(rd->d_tmp, rd->d_keep.as<ull>(), rd->d_kidx.as<ull>(), n_rec + 1, st, 8));
    SLX_CHK(slx_exclusive_sum(rd->d_tmp, rd->d_blen.as<ull>(), rd->d_boff.as<ull>(), n_rec + 1, st, 8));
    SLX_HIPCHK(hipMemcpyAsync(hs + 5, rd->d_kidx.as<ull>() + n_rec, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync(hs + 6, rd->d_boff.as<ull>() + n_rec, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    kn = hs[5]; kb = hs[6];
    if (kn) {
        SLX_CHK(rd->d_cs.ensure(kb + 8)); SLX_CHK(rd->d_cr.ensure(8 * (kn + 1)));
        k_bam_gather<<<(unsigned)((n_rec + 3) / 4), 256, 0, st>>>(s, rec, n_rec, rd->d_kidx.as<ull>(), rd->d_boff.as<ull>(), rd->d_cs.as<uint8_t>(), rd->d_cr.as<uint64_t>(), 0, 0);
        SLX_HIPCHK(hipGetLastError());
    }
    *kn_out = kn; *kb_out = kb;
    return SLX_OK;
}

// the whole file with a read filter attached: spans as without one, the filter's keep bytes, the two exclusive sums and k_bam_gather into d_cs / d_cr as for a
// region; a span whose records are all dropped goes on to the next, since n_records == 0 is the end of the file
static int bam_next_filtered(slx_bam *rd, int64_t max_bytes, slx_bam_batch *out)
{
    hipStream_t st = rd->st;
    const int64_t nm = (int64_t)rd->f.mem.size();
    uint64_t kn = 0, kb = 0, repaired = 0;
    int64_t members = 0;
    while (!kn) {
        const int64_t a = rd->next_member;
        if (a >= nm && rd->carry.empty()) break;
        int64_t done = a;
        uint64_t total = 0, n_rec = 0, end = 0, rep = 0;
        SLX_CHK(bam_span(rd, max_bytes, a, nm, 0, 0, &done, &total, &n_rec, &end, &rep));
        if (!n_rec && total) { slx_set_error("BAM: '%s' ends inside a record (%llu bytes after the last whole record)", rd->f.path.c_str(), (unsigned long long)total); return SLX_EIO; }
        rd->next_member = done; members += done - a; repaired += rep;
        SLX_CHK(bam_take_carry(rd, end, total));
        SLX_HIPCHK(slx_wait_stream(st));
        if (!n_rec) break;
        SLX_CHK(bam_filter_compact(rd, rd->d_out.as<uint8_t>(), rd->d_rec.as<uint64_t>(), n_rec, end, &kn, &kb));
        if (!kn) continue;
        SLX_CHK(rd->h_out.ensure(kb + 8)); SLX_CHK(rd->h_rec.ensure(8 * (kn + 1)));
        SLX_HIPCHK(hipMemcpyAsync(rd->h_out.p, rd->d_cs.p, kb, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(hipMemcpyAsync(rd->h_rec.p, rd->d_cr.p, 8 * (kn + 1), hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(slx_wait_stream(st));
    }
    rd->c_repaired += (int64_t)repaired; rd->c_records += (int64_t)kn;
    out->n_records = (int64_t)kn; out->n_bytes = (int64_t)kb;
    out->stream = rd->h_out.as<uint8_t>(); out->rec_off = rd->h_rec.as<uint64_t>();
    out->d_stream = rd->d_cs.p; out->d_rec_off = rd->d_cr.p;
    out->n_members = members; out->n_repaired_chunks = (int64_t)repaired;
    rd->cur_stream = rd->d_cs.p; rd->cur_rec = rd->d_cr.p; rd->map_stream = nullptr;
    return SLX_OK;
}

// a reader over SAM text: the batch comes from slx_sam.hip as records in HBM; with a read filter attached it is compacted as above
static int bam_next_sam(slx_bam *rd, int64_t max_bytes, slx_bam_batch *out)
{
    hipStream_t st = rd->st;
    uint64_t kn = 0, kb = 0;
    int64_t members = 0;
    const void *ds = nullptr, *dr = nullptr;
    for (;;) {
        uint64_t n_rec = 0, end = 0;
        int64_t nm = 0;
        SLX_CHK(slx_samsrc_next(rd->sam, max_bytes, &ds, &dr, &n_rec, &end, &nm));
        members += nm;
        if (!n_rec) return SLX_OK;
        if (!rd->flt) { kn = n_rec; kb = end; break; }
        SLX_CHK(bam_filter_compact(rd, (const uint8_t *)ds, (const uint64_t *)dr, n_rec, end, &kn, &kb));
        if (kn) { ds = rd->d_cs.p; dr = rd->d_cr.p; break; }
    }
    SLX_CHK(rd->h_out.ensure(kb + 8)); SLX_CHK(rd->h_rec.ensure(8 * (kn + 1)));
    SLX_HIPCHK(hipMemcpyAsync(rd->h_out.p, ds, kb, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync(rd->h_rec.p, dr, 8 * (kn + 1), hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    rd->c_records += (int64_t)kn;
    out->n_records = (int64_t)kn; out->n_bytes = (int64_t)kb;
    out->stream = rd->h_out.as<uint8_t>(); out->rec_off = rd->h_rec.as<uint64_t>();
    out->d_stream = ds; out->d_rec_off = dr;
    out->n_members = members; out->n_repaired_chunks = 0;
    rd->cur_stream = ds; rd->cur_rec = dr; rd->map_stream = nullptr;
    return SLX_OK;
}

extern "C" int slx_sam_open(const char *path, int device, slx_bam **out)
{
    if (!path || !out) { slx_set_error("slx_sam_open: null argument"); return SLX_EINVAL; }
    *out = nullptr;
    slx_samsrc *src = nullptr;
    SLX_CHK(slx_samsrc_open(path, device, &src));
    slx_bam *rd = new slx_bam();
    rd->f.path = path; rd->f.has_eof = 1;
    const int rc = bam_dev_init(rd, slx_samsrc_device(src));
    if (rc != SLX_OK) { slx_samsrc_close(src); bam_dev_free(rd); delete rd; return rc; }
    rd->sam = src;
    slx_samsrc_header(src, &rd->text, &rd->ref_names, &rd->ref_lens);
    *out = rd;
    return SLX_OK;
}

void slx_reader_set_filter(slx_bam *rd, slx_filter *f) { rd->flt = f; }

extern "C" int slx_bam_next(slx_bam *rd, int64_t max_bytes, slx_bam_batch *out)
{
    if (!rd || !out) { slx_set_error("slx_bam_next: null argument"); return SLX_EINVAL; }
    memset(out, 0, sizeof *out);
    SLX_HIPCHK(hipSetDevice(rd->device));
    rd->us[0] = rd->us[1] = rd->us[2] = rd->us[4] = 0;
    if (rd->sam) return bam_next_sam(rd, max_bytes, out);
    if (rd->region_mode) return bam_next_regions(rd, max_bytes, out);
    if (rd->flt) return bam_next_filtered(rd, max_bytes, out);
    const int64_t nm = (int64_t)rd->f.mem.size();
    const int64_t a = rd->next_member;
    if (a >= nm && rd->carry.empty()) return SLX_OK;
    hipStream_t st = rd->st;
    int64_t done = a;
    uint64_t total = 0, n_rec = 0, end = 0, repaired = 0;
    SLX_CHK(bam_span(rd, max_bytes, a, nm, 0, 0, &done, &total, &n_rec, &end, &repaired));
    if (!n_rec && total) {
        slx_set_error("BAM: '%s' ends inside a record (%llu bytes after the last whole record)", rd->f.path.c_str(), (unsigned long long)total);
        return SLX_EIO;
    }
    rd->next_member = done;
    SLX_CHK(rd->h_out.ensure(end + 8)); SLX_CHK(rd->h_rec.ensure(8 * (n_rec + 1)));
    if (end) SLX_HIPCHK(hipMemcpyAsync(rd->h_out.p, rd->d_out.p, end, hipMemcpyDeviceToHost, st));
    if (n_rec) SLX_HIPCHK(hipMemcpyAsync(rd->h_rec.p, rd->d_rec.p, 8 * (n_rec + 1), hipMemcpyDeviceToHost, st));
    SLX_CHK(bam_take_carry(rd, end, total));
    SLX_HIPCHK(slx_wait_stream(st));
    rd->c_repaired += (int64_t)repaired; rd->c_records += (int64_t)n_rec;
    out->n_records = (int64_t)n_rec; out->n_bytes = (int64_t)end;
    out->stream = rd->h_out.as<uint8_t>(); out->rec_off = rd->h_rec.as<uint64_t>();
    out->d_stream = rd->d_out.p; out->d_rec_off = rd->d_rec.p;
    out->n_members = done - a; out->n_repaired_chunks = (int64_t)repaired;
    rd->cur_stream = rd->d_out.p; rd->cur_rec = rd->d_rec.p; rd->map_stream = nullptr;
    return SLX_OK;
}

// ------------------------------------------------------------------ the BAI build
namespace {
struct BaiBuild : SlxBufOwner {          // the scratch of one build: it goes with the call
    BamDBuf ne_start{*this}, ne_file{*this}, lin_off{*this}, lin{*this}, first{*this}, last{*this}, n_map{*this}, n_unmap{*this}, n_intv{*this}, bst{*this}, carry{*this}, key{*this},
            tp{*this}, vbeg{*this}, vend{*this}, head{*this}, hidx{*this}, ckey{*this}, cbeg{*this}, cend{*this}, skey{*this}, sidx_in{*this}, sidx{*this}, tmp{*this};
    ~BaiBuild() { release_bufs(); }
};
void put_u32(std::string &o, uint32_t v) { o.append((const char *)&v, 4); }
void put_u64(std::string &o, uint64_t v) { o.append((const char *)&v, 8); }
}

// the whole file through the reader's inflate, CRC and record-index kernels, batch by batch, and the index kernels behind them; bai: the file's bytes
static int bai_build_body(slx_bam *rd, int64_t batch_bytes, BaiBuild &B, std::string &bai)
{
    typedef unsigned long long ull;
    hipStream_t st = rd->st;
    const int64_t nm = (int64_t)rd->f.mem.size();
    const int32_t n_ref = (int32_t)rd->ref_names.size();
    std::vector<uint64_t> start_all(nm + 1, 0), ne_start, ne_file, lin_off(n_ref + 1, 0);
    uint64_t behind = 0;
    for (int64_t i = 0; i < nm; ++i) {
        const slx_bam_member &m = rd->f.mem[i];
        start_all[i + 1] = start_all[i] + m.isize;
        if (m.isize) { ne_start.push_back(start_all[i]); ne_file.push_back(m.file_off); behind = m.file_off + m.data_off + m.data_len + 8; }
    }
    // windows of a reference: its length's, and one to spare; a record that passes them is refused (BAI_E_SPAN)
    for (int32_t t = 0; t < n_ref; ++t) lin_off[t + 1] = lin_off[t] + ((uint64_t)std::max<int64_t>(rd->ref_lens[t], 0) >> 14) + 2;
    const uint64_t nn = ne_start.size(), n_win = lin_off[n_ref], R = (uint64_t)std::max(n_ref, 1);
    auto up = [&](BamDBuf &b, const void *src, size_t bytes) -> int {
        SLX_CHK(b.ensure(bytes + 8));
        if (bytes) SLX_HIPCHK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st));
        return SLX_OK;
    };
    auto fill = [&](BamDBuf &b, int byte, size_t bytes) -> int {
        SLX_CHK(b.ensure(bytes + 8));
        SLX_HIPCHK(hipMemsetAsync(b.p, byte, bytes + 8, st));
        return SLX_OK;
    };
    auto down = [&](void *dst, const void *src, size_t bytes) -> int {
        if (bytes) SLX_HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
        return SLX_OK;
    };
    SLX_CHK(up(B.ne_start, ne_start.data(), 8 * nn)); SLX_CHK(up(B.ne_file, ne_file.data(), 8 * nn)); SLX_CHK(up(B.lin_off, lin_off.data(), 8 * (size_t)(n_ref + 1)));
    SLX_CHK(fill(B.lin, 0xff, 8 * n_win)); SLX_CHK(fill(B.first, 0xff, 8 * R)); SLX_CHK(fill(B.last, 0, 8 * R)); SLX_CHK(fill(B.n_map, 0, 8 * R)); SLX_CHK(fill(B.n_unmap, 0, 8 * R));
    SLX_CHK(fill(B.n_intv, 0, 4 * R));
    const ull bst0[3] = {0, ~0ull, 0}, carry0[4] = {BAI_NOKEY, 0, BAI_NOKEY, 0};
    SLX_CHK(up(B.bst, bst0, sizeof bst0)); SLX_CHK(up(B.carry, carry0, sizeof carry0));
    SLX_HIPCHK(hipStreamSynchronize(st));                  // (the uploads read this frame's memory)
    bai_dev d;
    d.ne_start = B.ne_start.as<uint64_t>(); d.ne_file = B.ne_file.as<uint64_t>(); d.nn = nn; d.total = start_all[nm]; d.behind = behind;
    d.lin_off = B.lin_off.as<uint64_t>(); d.lin = B.lin.as<ull>(); d.ref_first = B.first.as<ull>(); d.ref_last = B.last.as<ull>(); d.n_map = B.n_map.as<ull>(); d.n_unmap = B.n_unmap.as<ull>();
    d.n_intv = B.n_intv.as<uint32_t>(); d.n_ref = n_ref;
    SLX_CHK(rd->h_state.ensure(64));
    ull *hs = rd->h_state.as<ull>(), *bst = B.bst.as<ull>();
    uint64_t chunk_base = 0, ord_base = 0;
    int flip = 0;
    for (;;) {
        const int64_t a = rd->next_member;
        if (a >= nm && rd->carry.empty()) break;
        const uint64_t base_off = start_all[a] - rd->carry.size();
        int64_t done = a;
        uint64_t total = 0, n = 0, end = 0, rep = 0;
        SLX_CHK(bam_span(rd, batch_bytes, a, nm, 0, 0, &done, &total, &n, &end, &rep));
        if (!n && total) { slx_set_error("BAM: '%s' ends inside a record (%llu bytes after the last whole record)", rd->f.path.c_str(), (unsigned long long)total); return SLX_EIO; }
        rd->next_member = done;
        SLX_CHK(bam_take_carry(rd, end, total));
        SLX_HIPCHK(slx_wait_stream(st));
        if (!n) break;
        for (BamDBuf *b : {&B.key, &B.tp, &B.vbeg, &B.vend, &B.head, &B.hidx}) SLX_CHK(b->ensure(8 * (n + 1)));
        for (BamDBuf *b : {&B.ckey, &B.cbeg, &B.cend}) SLX_CHK(b->ensure(8 * (chunk_base + n + 1), st, 8 * chunk_base));
        const uint64_t cap = chunk_base + n + 1;
        const uint8_t *s = rd->d_out.as<uint8_t>();
        const uint64_t *rec = rd->d_rec.as<uint64_t>();
        SLX_HIPCHK(hipEventRecord(rd->ev[7], st));
        k_bai_rec<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(s, rec, n, base_off, d, B.key.as<ull>(), B.tp.as<ull>(), B.vbeg.as<ull>(), B.vend.as<ull>(), bst);
        SLX_HIPCHK(hipGetLastError());
        k_bai_heads<<<(unsigned)((n + 1 + 255) / 256), 256, 0, st>>>(B.key.as<ull>(), B.tp.as<ull>(), n, ord_base, B.carry.as<ull>() + 2 * flip, B.carry.as<ull>() + 2 * (flip ^ 1), B.head.as<ull>(), bst);
        SLX_HIPCHK(hipGetLastError());
        SLX_CHK(slx_exclusive_sum(B.tmp, B.head.as<ull>(), B.hidx.as<ull>(), n + 1, st, 8));
        k_bai_chunks<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(B.key.as<ull>(), B.vbeg.as<ull>(), B.vend.as<ull>(), B.head.as<ull>(), B.hidx.as<ull>(), n, chunk_base, cap, B.ckey.as<ull>(),
                                                                  B.cbeg.as<ull>(), B.cend.as<ull>());
        SLX_HIPCHK(hipGetLastError());
        SLX_HIPCHK(hipEventRecord(rd->ev[8], st));
        SLX_CHK(down(hs, B.hidx.as<ull>() + n, 8)); SLX_CHK(down(hs + 1, bst, 16));
        SLX_HIPCHK(slx_wait_stream(st));
        rd->us[4] += slx_ev_us(rd->ev[7], rd->ev[8]);
        if (hs[2] != ~0ull) { slx_set_error("BAM: '%s' is not coordinate-sorted: record %llu sorts before its predecessor; no index written", rd->f.path.c_str(), hs[2]); return SLX_EINVAL; }
        if (hs[1] & BAI_E_CIGAR) { slx_set_error("BAM: '%s': a record's name and CIGAR pass its block_size", rd->f.path.c_str()); return SLX_EIO; }
        if (hs[1] & BAI_E_TID) { slx_set_error("BAM: '%s': a record names a reference outside the header's %d", rd->f.path.c_str(), n_ref); return SLX_EIO; }
        if (hs[1] & BAI_E_SPAN) { slx_set_error("BAM: '%s': a record reaches past the end of its reference; no index written", rd->f.path.c_str()); return SLX_EINVAL; }
        chunk_base += hs[0]; ord_base += n; flip ^= 1;
        rd->c_records += (int64_t)n; rd->c_repaired += (int64_t)rep;
    }
    // chunks by (tid, bin); the radix sort is stable, so inside a bin they stay in file order, which is the order of their begins
    const uint64_t nc = chunk_base;
    std::vector<ull> skey(nc), cbeg(nc), cend(nc), lin(n_win), first(R), last(R), n_map(R), n_unmap(R);
    std::vector<uint32_t> sidx(nc), n_intv(R);
    ull n_no_coor = 0;
    if (nc) {
        if (nc >= (1ull << 31)) { slx_set_error("BAI: %llu chunks", (ull)nc); return SLX_EUNSUPPORTED; }
        SLX_CHK(B.skey.ensure(8 * nc)); SLX_CHK(B.sidx_in.ensure(4 * nc)); SLX_CHK(B.sidx.ensure(4 * nc));
        k_bai_iota<<<(unsigned)((nc + 255) / 256), 256, 0, st>>>(B.sidx_in.as<uint32_t>(), nc);
        SLX_HIPCHK(hipGetLastError());
        SLX_CHK(slx_cub("the BAI build's hipcub::DeviceRadixSort::SortPairs", B.tmp, 8, [&](void *t, size_t &b) {
            return hipcub::DeviceRadixSort::SortPairs(t, b, B.ckey.as<ull>(), B.skey.as<ull>(), B.sidx_in.as<uint32_t>(), B.sidx.as<uint32_t>(), (int)nc, 0, 64, st);
        }));
        SLX_CHK(down(skey.data(), B.skey.p, 8 * nc)); SLX_CHK(down(sidx.data(), B.sidx.p, 4 * nc)); SLX_CHK(down(cbeg.data(), B.cbeg.p, 8 * nc)); SLX_CHK(down(cend.data(), B.cend.p, 8 * nc));
    }
    if (n_ref) {
        k_bai_fill<<<(unsigned)n_ref, 64, 0, st>>>(d);
        SLX_HIPCHK(hipGetLastError());
        SLX_CHK(down(lin.data(), B.lin.p, 8 * n_win)); SLX_CHK(down(first.data(), B.first.p, 8 * R)); SLX_CHK(down(last.data(), B.last.p, 8 * R));
        SLX_CHK(down(n_map.data(), B.n_map.p, 8 * R)); SLX_CHK(down(n_unmap.data(), B.n_unmap.p, 8 * R)); SLX_CHK(down(n_intv.data(), B.n_intv.p, 4 * R));
    }
    SLX_CHK(down(&n_no_coor, bst + 2, 8));
    SLX_HIPCHK(slx_wait_stream(st));
    // the host only lays the bytes out: per reference its bins in ascending number, the pseudo-bin last, then the windows
    bai.assign("BAI\1", 4);
    put_u32(bai, (uint32_t)n_ref);
    uint64_t c = 0;
    for (int32_t t = 0; t < n_ref; ++t) {
        if (n_map[t] + n_unmap[t] == 0) { put_u32(bai, 0); put_u32(bai, 0); continue; }
        uint64_t e = c, n_bin = 0;
        while (e < nc && (int32_t)(skey[e] >> 32) == t) { if (e == c || skey[e] != skey[e - 1]) ++n_bin; ++e; }
        put_u32(bai, (uint32_t)n_bin + 1);
        while (c < e) {
            uint64_t f = c;
            while (f < e && skey[f] == skey[c]) ++f;
            put_u32(bai, (uint32_t)skey[c]); put_u32(bai, (uint32_t)(f - c));
            for (; c < f; ++c) { put_u64(bai, cbeg[sidx[c]]); put_u64(bai, cend[sidx[c]]); }
        }
        put_u32(bai, BAI_META_BIN); put_u32(bai, 2);
        put_u64(bai, first[t]); put_u64(bai, last[t]); put_u64(bai, n_map[t]); put_u64(bai, n_unmap[t]);
        put_u32(bai, n_intv[t]);
        for (uint32_t w = 0; w < n_intv[t]; ++w) put_u64(bai, lin[lin_off[t] + w]);
    }
    put_u64(bai, n_no_coor);
    return SLX_OK;
}

extern "C" int slx_bam_index_build_ex(const char *bam_path, int device, const char *bai_path, int64_t batch_bytes, int64_t chunk_bytes)
{
    slx_bam *rd = nullptr;
    SLX_CHK(bam_open_impl(bam_path, device, &rd, false));
    if (chunk_bytes >= 64) rd->chunk_bytes = (uint64_t)chunk_bytes;
    std::string bai;
    int rc;
    {
        BaiBuild B;
        rc = bai_build_body(rd, batch_bytes > 0 ? batch_bytes : (int64_t)64 << 20, B, bai);
        (void)hipStreamSynchronize(rd->st);
    }
    slx_bam_close(rd);
    if (rc != SLX_OK) return rc;
    const std::string out = bai_path ? std::string(bai_path) : std::string(bam_path) + ".bai";
    FILE *f = fopen(out.c_str(), "wb");
    if (!f) { slx_set_error("BAI: cannot write '%s'", out.c_str()); return SLX_EIO; }
    const bool ok = fwrite(bai.data(), 1, bai.size(), f) == bai.size();
    if (fclose(f) != 0 || !ok) { slx_set_error("BAI: cannot write '%s'", out.c_str()); return SLX_EIO; }
    return SLX_OK;
}
extern "C" int slx_bam_index_build(const char *bam_path, int device, const char *bai_path) { return slx_bam_index_build_ex(bam_path, device, bai_path, 0, 0); }

extern "C" int slx_bam_reads_device(slx_bam *rd, const slx_bam_batch *batch, int skip_flags, int original_strand, void **d_bases, void **d_offs, int64_t *n_reads,
                                    const int64_t **rec_of_read)
{
    if (!rd || !batch || !d_bases || !d_offs || !n_reads) { slx_set_error("slx_bam_reads_device: null argument"); return SLX_EINVAL; }
    if (!rd->cur_stream || batch->d_stream != rd->cur_stream || batch->d_rec_off != rd->cur_rec) { slx_set_error("slx_bam_reads_device: the batch is not the reader's current one"); return SLX_EINVAL; }
    SLX_HIPCHK(hipSetDevice(rd->device));
    hipStream_t st = rd->st;
    const uint64_t n = (uint64_t)batch->n_records;
    typedef unsigned long long ull;
    rd->map_stream = nullptr;
    for (BamDBuf *b : {&rd->d_keep, &rd->d_blen, &rd->d_kidx, &rd->d_boff}) SLX_CHK(b->ensure(8 * (n + 1)));
    SLX_CHK(rd->d_state.ensure(64)); SLX_CHK(rd->h_state.ensure(64));
    ull *hs = rd->h_state.as<ull>(), *ds = rd->d_state.as<ull>();
    hs[2] = ~0ull;
    SLX_HIPCHK(hipMemcpyAsync(ds + 2, hs + 2, 8, hipMemcpyHostToDevice, st));
    SLX_HIPCHK(hipEventRecord(rd->ev[5], st));
    const uint8_t *s = (const uint8_t *)rd->cur_stream;
    const uint64_t *rec = (const uint64_t *)rd->cur_rec;
    k_bam_keep<<<(unsigned)((n + 1 + 255) / 256), 256, 0, st>>>(s, rec, n, (uint32_t)skip_flags & 0xffffu, rd->d_keep.as<ull>(), rd->d_blen.as<ull>(), ds);
    SLX_HIPCHK(hipGetLastError());
    SLX_CHK(slx_exclusive_sum(rd->d_tmp, rd->d_keep.as<ull>(), rd->d_kidx.as<ull>(), n + 1, st, 8));
    SLX_CHK(slx_exclusive_sum(rd->d_tmp, rd->d_blen.as<ull>(), rd->d_boff.as<ull>(), n + 1, st, 8));
    SLX_HIPCHK(hipMemcpyAsync(hs, rd->d_kidx.as<ull>() + n, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync(hs + 1, rd->d_boff.as<ull>() + n, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync(hs + 2, ds + 2, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    if (hs[2] != ~0ull) { slx_set_error("BAM: '%s': a record's fields pass its block_size (inflated offset %llu of the batch)", rd->f.path.c_str(), hs[2]); return SLX_EIO; }
    const uint64_t nr = hs[0], nb = hs[1];
    SLX_CHK(rd->d_bases.ensure(nb + 8)); SLX_CHK(rd->d_offs.ensure(8 * (nr + 1))); SLX_CHK(rd->d_map.ensure(8 * (nr + 1))); SLX_CHK(rd->h_map.ensure(8 * (nr + 1)));
    if (n) {
        k_bam_unpack<<<(unsigned)((n + 3) / 4), 256, 0, st>>>(s, rec, n, rd->d_kidx.as<ull>(), rd->d_boff.as<ull>(), original_strand, rd->d_bases.as<uint8_t>(), rd->d_offs.as<uint64_t>(),
                                                             rd->d_map.as<int64_t>());
        SLX_HIPCHK(hipGetLastError());
    } else SLX_HIPCHK(hipMemsetAsync(rd->d_offs.p, 0, 8, st));
    SLX_HIPCHK(hipEventRecord(rd->ev[6], st));
    if (nr) SLX_HIPCHK(hipMemcpyAsync(rd->h_map.p, rd->d_map.p, 8 * nr, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    rd->us[3] = slx_ev_us(rd->ev[5], rd->ev[6]);
    *d_bases = rd->d_bases.p; *d_offs = rd->d_offs.p; *n_reads = (int64_t)nr;
    rd->map_stream = rd->cur_stream; rd->map_reads = (int64_t)nr;
    if (rec_of_read) *rec_of_read = rd->h_map.as<int64_t>();
    return SLX_OK;
}

bool slx_reader_device_reads(const slx_bam *rd, const void *batch_d_stream, const void **d_bases, const void **d_offs, const int64_t **d_rec_of_read, int64_t *n_reads, int *device)
{
    if (!rd || !rd->map_stream || rd->map_stream != batch_d_stream || rd->map_stream != rd->cur_stream) return false;
    *d_bases = rd->d_bases.p; *d_offs = rd->d_offs.p; *d_rec_of_read = rd->d_map.as<int64_t>(); *n_reads = rd->map_reads; *device = rd->device;
    return true;
}

// a device-resident result of slx_align_batch_device as a host result: one packed image (slx_hits_pack's layout, seqlib_amd.h) in HBM, one copy down
extern "C" int slx_bam_hits_to_host(slx_bam *rd, slx_aligner *al, const slx_hits *dev, slx_hits *host)
{
    if (!rd || !al || !dev || !host || !dev->on_device) { slx_set_error("slx_bam_hits_to_host: needs a reader, an aligner and a device-resident result"); return SLX_EINVAL; }
    memset(host, 0, sizeof *host);
    SLX_HIPCHK(hipSetDevice(rd->device));
    const uint64_t bytes = slx_hits_packed_size(dev);
    SLX_CHK(rd->d_tmp.ensure(bytes + 8));
    SLX_CHK(slx_hits_pack(al, dev, rd->d_tmp.p, bytes));
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
            SLX_CHK(rd.d_out.ensure(bytes + 8));
            SLX_CHK(bam_inflate_span(&rd, a, b, 0, bytes));
            if (bytes) { SLX_HIPCHK(hipMemcpyAsync((uint8_t *)dst + pos, rd.d_out.p, bytes, hipMemcpyDeviceToHost, rd.st)); SLX_HIPCHK(hipStreamSynchronize(rd.st)); }
            pos += bytes; a = b;
        }
        return SLX_OK;
    };
    rc = body();
    bam_dev_free(&rd);
    return rc;
}
