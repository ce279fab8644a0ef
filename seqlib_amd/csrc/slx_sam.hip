// slx_sam.hip -- SAM text parsed on the GPU into the BAM reader's batches (include/seqlib_amd_sam.h): block_size-prefixed BAM records in HBM, in file order, so that
// everything that takes an slx_bam_batch takes SAM.  DESIGN.md section 9.7 has the argument.  The bytes come in as the FASTQ reader's do (fq_text.h: producer thread for
// plain and gzip text, k_bgzf_inflate / k_bgzf_crc for bgzip'd text, k_fq_count / k_fq_lines for the line starts); every line is independent of its neighbours:
//   k_sam_fields   one wave per line: the eleven field starts, the start of the optional fields, QUAL's bytes tested                sam_fields_wave (dev_sam.h's sam_fld)
//   k_sam_size     one lane per line: every rule of the grammar over the line's short fields -> the record's size and the verdict   dev_sam.h sam_record, out == nullptr
//   hipCUB         exclusive sum of the sizes: the record offsets, which are the batch's rec_off
//   k_sam_fill     one wave per line: the 32 fixed bytes, CIGAR words and typed optional values by lane 0, QNAME, SEQ (two bases per byte) and QUAL - 33 over the
//                  64 lanes; a record of the slow path is copied from its staging place                                            dev_sam.h sam_record, out != nullptr
// SLOW lines (f, d, B:f fields: no floating-point text is read on the GPU) and ERROR lines come down and go through sam_host.h one by one; the records go up into a
// staging buffer and k_sam_fill places them among the others.  Waves and lanes take lines by a static map: there is no work queue here, and the only atomic is one
// atomicAdd per wave that holds a line which is not FAST.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <zlib.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "slx_internal.h"
#include "seqlib_amd_bam.h"
#include "seqlib_amd_sam.h"
#include "fq_text.h"
#include "dev_sam.h"
#include "sam_host.h"
#include "sam_reader.h"

// ------------------------------------------------------------------ kernels
// sam_fields for one wave: lane i tests byte 64 j + i, the ballot gives the tabs in order.  s[0, n), n <= SAM_MAX_LINE; F is written by lane 0.
__device__ __forceinline__ void sam_fields_wave(const uint8_t *s, uint32_t n, uint32_t lane, sam_fld *F)
{
    uint32_t k = 1, f10 = 0, f11 = n;
    if (lane == 0) F->f[0] = 0;
    for (uint32_t base = 0; base < n && k < 12; base += 64) {          // (wave-uniform trip count: the ballot sees all 64 lanes)
        const uint32_t i = base + lane;
        unsigned long long m = __ballot(i < n && s[i] == '\t');
        while (m && k < 12) {
            const uint32_t j = (uint32_t)__ffsll(m) - 1u;
            m &= m - 1ull;
            if (k <= 10) { if (lane == 0) F->f[k] = base + j + 1; if (k == 10) f10 = base + j + 1; }
            else f11 = base + j;
            ++k;
        }
    }
    bool bad = false;
    if (k >= 11)
        for (uint32_t i = f10 + lane; i < f11; i += 64) bad |= s[i] < 33 || s[i] > 126;
    const bool any = __ballot(bad) != 0ull;
    if (lane == 0) { F->f[11] = f11; F->nf = k; F->flags = any ? 1u : 0u; }
}

__global__ __launch_bounds__(256) void k_sam_fields(const uint8_t *text, const fq_u64 *line_off, uint64_t L, int virt, sam_fld *fld)
{
    const uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= L) return;
    uint64_t beg; uint32_t n; bool cr;
    sam_line_span(text, line_off, k, L, virt, &beg, &n, &cr);
    if (n > SAM_MAX_LINE) return;
    sam_fields_wave(text + beg, n, threadIdx.x & 63, fld + k);
}

// size[k] = bytes of line k's record when it is FAST, else 0; size[L] = 0; verdict[k]; *n_other = lines that are not FAST
__global__ __launch_bounds__(256) void k_sam_size(const uint8_t *text, const fq_u64 *line_off, uint64_t L, int virt, const sam_fld *fld, sam_refs R, int fast_fail, fq_u64 *size,
                                                  uint8_t *verdict, fq_u64 *n_other)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int v = SAM_FAST;
    if (k < L) {
        uint64_t beg; uint32_t n, sz = 0; bool cr;
        int err;
        sam_line_span(text, line_off, k, L, virt, &beg, &n, &cr);
        if (cr) v = SAM_ERROR;
        else v = sam_record(text + beg, n, fld[k], R, (uint8_t *)nullptr, &sz, &err, 0u, 1u, sam_no_float());
        if (v == SAM_FAST && fast_fail) v = SAM_SLOW;
        size[k] = v == SAM_FAST ? sz : 0;
        verdict[k] = (uint8_t)v;
    } else if (k == L) size[k] = 0;
    const unsigned long long m = __ballot(v != SAM_FAST);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_other, (fq_u64)__popcll(m));          // at most one per wave, and only from a wave that holds such a line
}

// out[rec[k], rec[k + 1]) = the record of line k < L: built from the text, or copied from src[k] (the slow path's staging buffer) when the line is not FAST
__global__ __launch_bounds__(256) void k_sam_fill(const uint8_t *text, const fq_u64 *line_off, uint64_t L, uint64_t L_all, int virt, const sam_fld *fld, sam_refs R, const uint8_t *verdict,
                                                  const fq_u64 *src, const fq_u64 *rec, uint8_t *out)
{
    const uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (k >= L) return;
    uint8_t *o = out + rec[k];
    if (verdict[k] != SAM_FAST) {
        const uint8_t *p = (const uint8_t *)(uintptr_t)src[k];
        const uint64_t nb = rec[k + 1] - rec[k];
        for (uint64_t i = lane; i < nb; i += 64) o[i] = p[i];
        return;
    }
    uint64_t beg; uint32_t n, sz = 0; bool cr;
    int err;
    sam_line_span(text, line_off, k, L_all, virt, &beg, &n, &cr);
    (void)sam_record(text + beg, n, fld[k], R, o, &sz, &err, lane, 64u, sam_no_float());
}

// ------------------------------------------------------------------ host: the reader
struct slx_samsrc : FqText {
    std::string text;                              // the header
    std::vector<std::string> ref_names;
    std::vector<int64_t> ref_lens;
    SamRefTable tab;
    uint64_t body_off = 0, header_lines = 0;       // where the first line that is not an '@' line begins, and how many lines stand before it
    uint64_t line_base = 0;                        // lines of the file delivered or skipped so far
    bool done = false, bad = false;
    std::string bad_msg;
    int fast_fail = 0;
    FqDBuf d_ref_names{*this}, d_ref_off{*this}, d_ref_tid{*this}, d_fld{*this}, d_size{*this}, d_verdict{*this}, d_src{*this}, d_rec{*this}, d_out{*this}, d_slow{*this}, d_cnt{*this};
    FqHBuf h_text{*this}, h_verdict{*this}, h_line{*this}, h_size{*this}, h_src{*this}, h_slow{*this};
    int64_t c_fast = 0, c_slow = 0;
    float us_sam[3] = {0, 0, 0};                   // fields, size, fill
    sam_refs dev_refs() const { return sam_refs{d_ref_names.as<uint8_t>(), d_ref_off.as<uint32_t>(), d_ref_tid.as<int32_t>(), (int32_t)tab.tid.size()}; }
};

void slx_samsrc_close(slx_samsrc *S)
{
    if (!S) return;
    fq_text_free(S);
    delete S;
}

// the window's first bytes on the host until the header is whole
static int sam_read_header(slx_samsrc *S)
{
    uint64_t want = 1u << 16;
    std::string msg;
    for (;;) {
        if (!S->src_eof) SLX_CHK(fq_pull(S, want));
        SLX_CHK(S->h_text.ensure(S->have + 1));
        if (S->have) SLX_HIPCHK(hipMemcpyAsync(S->h_text.p, S->d_text[S->cur].p, S->have, hipMemcpyDeviceToHost, S->st));
        SLX_HIPCHK(slx_wait_stream(S->st));
        const int r = samh_header(S->h_text.as<uint8_t>(), S->have, S->src_eof, S->text, S->ref_names, S->ref_lens, &S->body_off, &S->header_lines, msg);
        if (r < 0) { slx_set_error("SAM: '%s': %s", S->path.c_str(), msg.c_str()); return SLX_EIO; }
        if (r == 1) break;
        want *= 2;
    }
    S->used = S->body_off; S->line_base = S->header_lines;
    return SLX_OK;
}

int slx_samsrc_rewind(slx_samsrc *S)
{
    SLX_HIPCHK(hipSetDevice(S->device));
    SLX_CHK(fq_text_start(S));
    S->done = S->bad = false; S->c_fast = S->c_slow = 0;
    for (float &u : S->us_sam) u = 0;
    while (S->have < S->body_off && !S->src_eof) SLX_CHK(fq_pull(S, S->body_off - S->have));
    S->used = S->body_off; S->line_base = S->header_lines;
    return SLX_OK;
}

int slx_samsrc_open(const char *path, int device, slx_samsrc **out)
{
    *out = nullptr;
    slx_samsrc *S = new slx_samsrc();
    S->who = "SAM reader";
    int rc = fq_text_open(S, path, device);
    if (rc == SLX_OK) rc = fq_text_start(S);
    if (rc == SLX_OK) rc = sam_read_header(S);
    if (rc == SLX_OK) {
        S->tab.build(S->ref_names);
        auto up = [&](FqDBuf &d, const void *p, size_t n) {
            const int r = d.ensure(n + 16);
            if (r != SLX_OK) return r;
            if (n && hipMemcpy(d.p, p, n, hipMemcpyHostToDevice) != hipSuccess) { slx_set_error("SAM reader: cannot copy the reference names to the device"); return (int)SLX_ENODEVICE; }
            return (int)SLX_OK;
        };
        rc = up(S->d_ref_names, S->tab.names.data(), S->tab.names.size());
        if (rc == SLX_OK) rc = up(S->d_ref_off, S->tab.off.data(), 4 * S->tab.off.size());
        if (rc == SLX_OK) rc = up(S->d_ref_tid, S->tab.tid.data(), 4 * S->tab.tid.size());
    }
    if (rc != SLX_OK) { slx_samsrc_close(S); return rc; }
    *out = S;
    return SLX_OK;
}

void slx_samsrc_header(const slx_samsrc *S, std::string *text, std::vector<std::string> *names, std::vector<int64_t> *lens) { *text = S->text; *names = S->ref_names; *lens = S->ref_lens; }
int slx_samsrc_device(const slx_samsrc *S) { return S->device; }

bool slx_samsrc_set(slx_samsrc *S, const char *key, int64_t value, int *rc)
{
    const std::string k = key;
    if (k != "sam_tile_bytes" && k != "sam_fast_fail") return false;
    *rc = SLX_OK;
    if (k == "sam_tile_bytes" && value >= 16 && value % 16 == 0 && value <= (1 << 30)) S->tile_bytes = (uint32_t)value;
    else if (k == "sam_fast_fail" && (value == 0 || value == 1)) S->fast_fail = (int)value;
    else { slx_set_error("slx_bam_set: value out of range: %s = %lld", key, (long long)value); *rc = SLX_EINVAL; }
    return true;
}

bool slx_samsrc_counter(const slx_samsrc *S, const char *name, int64_t *v)
{
    const std::string k = name;
    if (k == "sam") *v = 1;
    else if (k == "source") *v = S->source;
    else if (k == "lines") *v = (int64_t)S->line_base;
    else if (k == "fast_records") *v = S->c_fast;
    else if (k == "slow_records") *v = S->c_slow;
    else if (k == "us_lines") *v = (int64_t)S->us[0];
    else if (k == "us_inflate") *v = (int64_t)S->us[3];
    else if (k == "us_fields") *v = (int64_t)S->us_sam[0];
    else if (k == "us_size") *v = (int64_t)S->us_sam[1];
    else if (k == "us_fill") *v = (int64_t)S->us_sam[2];
    else return false;
    return true;
}

// one attempt on d_text[cur][0, have): the records of its whole lines into d_out / d_rec; *consumed bytes of text used up
static int sam_parse(slx_samsrc *S, uint64_t *n_rec, uint64_t *n_bytes, uint64_t *consumed)
{
    hipStream_t st = S->st;
    const uint8_t *text = S->d_text[S->cur].as<uint8_t>();
    const uint64_t n = S->have;
    uint64_t L = 0;
    int virt = 0;
    *n_rec = *n_bytes = *consumed = 0;
    SLX_CHK(fq_line_starts(S, &L, &virt));
    if (L == 0) return SLX_OK;
    if (L >= 0xffffffffull) { slx_set_error("SAM reader: 2^32 lines or more in one batch; ask for fewer bytes"); return SLX_EUNSUPPORTED; }
    const fq_u64 *line_off = S->d_line.as<fq_u64>();
    SLX_CHK(S->d_fld.ensure(sizeof(sam_fld) * L)); SLX_CHK(S->d_size.ensure(8 * (L + 1))); SLX_CHK(S->d_verdict.ensure(L + 8)); SLX_CHK(S->d_rec.ensure(8 * (L + 1)));
    SLX_CHK(S->d_cnt.ensure(8)); SLX_CHK(S->h_size.ensure(8 * (L + 1) + 64));
    fq_u64 *hs = S->h_small.as<fq_u64>();
    SLX_HIPCHK(hipMemsetAsync(S->d_cnt.p, 0, 8, st));
    SLX_HIPCHK(hipMemsetAsync(S->d_fld.p, 0, sizeof(sam_fld) * L, st));
    const sam_refs R = S->dev_refs();
    SLX_HIPCHK(hipEventRecord(S->ev[2], st));
    k_sam_fields<<<(unsigned)((L + 3) / 4), 256, 0, st>>>(text, line_off, L, virt, S->d_fld.as<sam_fld>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(S->ev[3], st));
    k_sam_size<<<(unsigned)((L + 1 + 255) / 256), 256, 0, st>>>(text, line_off, L, virt, S->d_fld.as<sam_fld>(), R, S->fast_fail, S->d_size.as<fq_u64>(), S->d_verdict.as<uint8_t>(), S->d_cnt.as<fq_u64>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(S->ev[4], st));
    SLX_HIPCHK(hipMemcpyAsync(hs, S->d_cnt.p, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync(hs + 1, line_off + L, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    S->us[0] += slx_ev_us(S->ev[0], S->ev[1]); S->us_sam[0] += slx_ev_us(S->ev[2], S->ev[3]); S->us_sam[1] += slx_ev_us(S->ev[3], S->ev[4]);
    const uint64_t n_other = hs[0];
    *consumed = hs[1] < n ? hs[1] : n;
    // ---- the lines that are not FAST, one by one through the host parser
    uint64_t L_eff = L, n_slow = 0;
    const fq_u64 *d_src = nullptr;
    if (n_other) {
        SLX_CHK(S->h_text.ensure(n + 1)); SLX_CHK(S->h_verdict.ensure(L + 8)); SLX_CHK(S->h_line.ensure(8 * (L + 2))); SLX_CHK(S->h_src.ensure(8 * (L + 1)));
        SLX_HIPCHK(hipMemcpyAsync(S->h_text.p, text, n, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(hipMemcpyAsync(S->h_verdict.p, S->d_verdict.p, L, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(hipMemcpyAsync(S->h_line.p, line_off, 8 * (L + 1), hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(hipMemcpyAsync(S->h_size.p, S->d_size.p, 8 * (L + 1), hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(slx_wait_stream(st));
        const uint8_t *ht = S->h_text.as<uint8_t>(), *hv = S->h_verdict.as<uint8_t>();
        const fq_u64 *hl = S->h_line.as<fq_u64>();
        fq_u64 *hsz = S->h_size.as<fq_u64>(), *hsrc = S->h_src.as<fq_u64>();
        const sam_refs HR = S->tab.view();
        std::vector<uint8_t> rec, stage;
        std::vector<uint64_t> at;          // per slow line: its place in stage
        memset(hsrc, 0, 8 * (L + 1));
        for (uint64_t k = 0; k < L; ++k) {
            if (hv[k] == SAM_FAST) continue;
            uint64_t beg; uint32_t ln; bool cr;
            int err = SAM_E_NONE;
            sam_line_span(ht, hl, k, L, virt, &beg, &ln, &cr);
            int v = SAM_ERROR;
            if (cr) err = SAM_E_CR;
            else if (ln > SAM_MAX_LINE) err = SAM_E_LONG;
            else v = samh_parse_line(ht + beg, ln, HR, rec, &err);
            if (v != SAM_FAST) {
                S->bad = true;
                S->bad_msg = "SAM: '" + S->path + "': line " + std::to_string(S->line_base + k + 1) + ": " + samh_errtext(err);
                L_eff = k;
                break;
            }
            if (hv[k] == SAM_ERROR) { slx_set_error("SAM reader: internal: the kernel refuses line %llu, the host parser takes it", (unsigned long long)(S->line_base + k + 1)); return SLX_EINTERNAL; }
            hsz[k] = rec.size(); hsrc[k] = stage.size();
            stage.insert(stage.end(), rec.begin(), rec.end());
            at.push_back(k);
            ++n_slow;
        }
        hsz[L_eff] = 0;
        if (L_eff == 0) return SLX_OK;          // (S->bad: the caller reports it)
        SLX_CHK(S->d_slow.ensure(stage.size() + 16)); SLX_CHK(S->h_slow.ensure(stage.size() + 16)); SLX_CHK(S->d_src.ensure(8 * (L + 1)));
        if (!stage.empty()) memcpy(S->h_slow.p, stage.data(), stage.size());
        for (uint64_t k : at) hsrc[k] += (fq_u64)(uintptr_t)S->d_slow.p;
        if (!stage.empty()) SLX_HIPCHK(hipMemcpyAsync(S->d_slow.p, S->h_slow.p, stage.size(), hipMemcpyHostToDevice, st));
        SLX_HIPCHK(hipMemcpyAsync(S->d_src.p, hsrc, 8 * (L_eff + 1), hipMemcpyHostToDevice, st));
        SLX_HIPCHK(hipMemcpyAsync(S->d_size.p, hsz, 8 * (L_eff + 1), hipMemcpyHostToDevice, st));
        d_src = S->d_src.as<fq_u64>();
    }
    // ---- offsets, then the records
    SLX_CHK(fq_scan(S, S->d_size.as<fq_u64>(), S->d_rec.as<fq_u64>(), L_eff + 1));
    SLX_HIPCHK(hipMemcpyAsync(hs, S->d_rec.as<fq_u64>() + L_eff, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    const uint64_t total = hs[0];
    SLX_CHK(S->d_out.ensure(total + 64));
    SLX_HIPCHK(hipEventRecord(S->ev[5], st));
    k_sam_fill<<<(unsigned)((L_eff + 3) / 4), 256, 0, st>>>(text, line_off, L_eff, L, virt, S->d_fld.as<sam_fld>(), R, S->d_verdict.as<uint8_t>(), d_src, S->d_rec.as<fq_u64>(), S->d_out.as<uint8_t>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(S->ev[6], st));
    SLX_HIPCHK(slx_wait_stream(st));
    S->us_sam[2] += slx_ev_us(S->ev[5], S->ev[6]);
    *n_rec = L_eff; *n_bytes = total;
    S->c_slow += (int64_t)n_slow; S->c_fast += (int64_t)(L_eff - n_slow);
    S->line_base += L_eff;
    return SLX_OK;
}

int slx_samsrc_next(slx_samsrc *S, int64_t max_bytes, const void **d_stream, const void **d_rec, uint64_t *n_rec, uint64_t *n_bytes, int64_t *n_members)
{
    *d_stream = *d_rec = nullptr; *n_rec = *n_bytes = 0; *n_members = 0;
    if (S->bad) { slx_set_error("%s", S->bad_msg.c_str()); return SLX_EIO; }
    if (S->done) return SLX_OK;
    if (max_bytes <= 0) max_bytes = 64ll << 20;
    SLX_HIPCHK(hipSetDevice(S->device));
    const int64_t members0 = S->c_members;
    uint64_t target = (uint64_t)max_bytes;
    for (;;) {
        if (S->used) SLX_CHK(fq_shift(S, target));          // the cut tail moves to the front of the other buffer
        if (S->have < target && !S->src_eof) SLX_CHK(fq_pull(S, target - S->have));
        if (S->have == 0) {
            if (S->src_eof) { S->done = true; return SLX_OK; }
            continue;
        }
        uint64_t consumed = 0;
        SLX_CHK(sam_parse(S, n_rec, n_bytes, &consumed));
        S->used = consumed;
        *n_members = S->c_members - members0;
        if (*n_rec) { *d_stream = S->d_out.p; *d_rec = S->d_rec.p; return SLX_OK; }
        if (S->bad) { slx_set_error("%s", S->bad_msg.c_str()); return SLX_EIO; }
        if (S->src_eof) {
            if (consumed >= S->have) { S->done = true; return SLX_OK; }
            slx_set_error("SAM reader: internal: the parser made no progress at the end of '%s'", S->path.c_str());
            return SLX_EINTERNAL;
        }
        target = std::max<uint64_t>(2 * target, 2 * (S->have - consumed) + 64);          // not one whole line yet: the batch grows
    }
}

// ------------------------------------------------------------------ host only: sniffing, and one line
extern "C" int slx_sam_sniff(const char *path)
{
    if (!path) { slx_set_error("slx_sam_sniff: path is null"); return SLX_EINVAL; }
    gzFile g = gzopen(path, "rb");          // (reads plain bytes as they are, gzip and BGZF inflated)
    if (!g) { slx_set_error("SAM: cannot open '%s'", path); return SLX_EIO; }
    std::vector<uint8_t> b(1u << 16);
    const int got = gzread(g, b.data(), (unsigned)b.size());
    gzclose(g);
    if (got < 0) { slx_set_error("SAM: '%s' cannot be read (zlib refuses the stream)", path); return SLX_EIO; }
    if (got >= 4 && memcmp(b.data(), "BAM\1", 4) == 0) return 0;
    bool sam = got >= 4 && b[0] == '@' && b[1] >= 'A' && b[1] <= 'Z' && b[2] >= 'A' && b[2] <= 'Z' && b[3] == '\t';
    if (!sam && got > 0 && b[0] != '@') {          // no header: a first line of eleven fields or more, text only
        int tabs = 0;
        bool text = true;
        for (int i = 0; i < got && b[i] != '\n'; ++i) { if (b[i] == '\t') ++tabs; else if (b[i] < 32 && b[i] != '\r') text = false; }
        sam = text && tabs >= 10;
    }
    if (sam) return 1;
    slx_set_error("'%s' is neither BAM nor SAM text (CRAM is not read)", path);
    return SLX_EIO;
}

extern "C" int slx_sam_parse_line(const char *line, int64_t n, const char *const *ref_names, int n_ref, uint8_t *out, int64_t cap, int64_t *n_out)
{
    if (!line || n < 0 || n_ref < 0 || (n_ref && !ref_names) || !n_out || (cap > 0 && !out)) { slx_set_error("slx_sam_parse_line: null or negative argument"); return SLX_EINVAL; }
    *n_out = 0;
    std::vector<std::string> names;
    for (int i = 0; i < n_ref; ++i) names.push_back(ref_names[i] ? ref_names[i] : "");
    SamRefTable tab;
    tab.build(names);
    std::vector<uint8_t> rec;
    int err = SAM_E_NONE;
    if (samh_parse_line((const uint8_t *)line, (uint64_t)n, tab.view(), rec, &err) != SAM_FAST) { slx_set_error("SAM: %s", samh_errtext(err)); return SLX_EIO; }
    *n_out = (int64_t)rec.size();
    if ((int64_t)rec.size() > cap) { slx_set_error("slx_sam_parse_line: the record takes %zu bytes, out holds %lld", rec.size(), (long long)cap); return SLX_EINVAL; }
    memcpy(out, rec.data(), rec.size());
    return SLX_OK;
}
