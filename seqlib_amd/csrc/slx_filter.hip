// slx_filter.hip -- the read filter of libseqlib_amd.so (include/seqlib_amd_filter.h): SeqLib::Filter::ReadFilterCollection over BAM records in HBM.
//   k_flt_eval       the stream cut into windows of W bytes, a block per window: the records that START in the window are the block's (two searches in
//                    rec_off); the window and V bytes behind it staged in LDS with aligned 16-byte loads, then a lane per record out of LDS -- a 150 bp
//                    record is some 350 bytes over six cache lines, and a lane walking them in HBM waits for each.  The motif automata are copied beside
//                    the stage when they fit.  A record that ends behind the stage goes to the long list.                            dev_rfilter.h
//   k_flt_eval_long  the long list, a wave per record: lanes stride over the CIGAR ops and the sequence bytes, the motif search runs in chunks that start
//                    lmax - 1 bases early out of the root state; shares joined by shuffles, lane 0 walks the aux fields and evaluates.   dev_rfilter.h
// The keep byte of a record depends on its bytes and the rule set alone: not on the window, the overhang, the chunk, the batch or the run.
// The host builds the tables (rfilter_host.h) and uploads them once per rule set and device.  No work queue: blocks own windows, waves stride the long list.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "slx_internal.h"
#include "seqlib_amd_filter.h"
#include "dev_lanes.h"
#include "rfilter_host.h"
#include "slx_hip.h"

#define FLT_LDS_MAX 65536u

// st: [0] records on the long list, [1] error bits, [2] kept records
__global__ __launch_bounds__(256) void k_flt_eval(const uint8_t *s, const uint64_t *rec_off, uint64_t n_rec, uint64_t n_bytes, uint32_t W, uint32_t V, rf_tab T, uint32_t dfa_words_lds,
                                                  uint8_t *keep, uint32_t *long_list, uint32_t *st)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t flt_lds[];
    if (dfa_words_lds) {          // the automata beside the stage (the barrier inside rf_window stands between this copy and their use)
        uint32_t *d = reinterpret_cast<uint32_t *>(flt_lds + W + V + 16);
        for (uint32_t i = threadIdx.x; i < dfa_words_lds; i += blockDim.x) d[i] = T.dfa[i];
        T.dfa = d;
    }
    uint32_t kept = rf_window(s, n_bytes, rec_off, n_rec, blockIdx.x, W, V, flt_lds, &T, keep, long_list, st, st + 1, threadIdx.x, blockDim.x);
    wave_count(st + 2, kept);
}

__global__ __launch_bounds__(256) void k_flt_eval_long(const uint8_t *s, const uint64_t *rec_off, uint64_t n_rec, rf_tab T, uint32_t chunk_bases, uint8_t *keep, const uint32_t *long_list,
                                                       uint32_t *st)
{
    const uint32_t lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = gridDim.x * 4;
    const uint32_t n_long = st[0];
    for (uint32_t i = wave; i < n_long; i += n_waves) {
        const uint64_t r = long_list[i];
        if (r >= n_rec) continue;
        const uint64_t a = rec_off[r], b = rec_off[r + 1];          // (k_flt_eval has placed [a, b) inside the stream)
        rf_feat F;
        if (!rf_fixed(s + a, b - a, &F)) {
            if (lane == 0) { atomicOr(st + 1, RF_E_FIELDS); keep[r] = 0; }
            continue;
        }
        rf_part P;
        rf_long_part(&T, &F, chunk_bases, lane, 64, &P);
        for (int o = 32; o; o >>= 1) {
            rf_part Q;
            Q.reflen = __shfl_xor((unsigned long long)P.reflen, o, 64); Q.qlen = __shfl_xor((unsigned long long)P.qlen, o, 64); Q.hits = __shfl_xor((unsigned long long)P.hits, o, 64);
            Q.clip = __shfl_xor(P.clip, o, 64); Q.hclip = __shfl_xor(P.hclip, o, 64); Q.max_ins = __shfl_xor(P.max_ins, o, 64); Q.max_del = __shfl_xor(P.max_del, o, 64);
            Q.n_n = __shfl_xor(P.n_n, o, 64);
            rf_part_join(&P, &Q);
        }
        if (lane == 0) {
            uint32_t er;
            const bool k = rf_long_finish(&T, &F, &P, &er);
            if (er) atomicOr(st + 1, er);
            keep[r] = k ? 1 : 0;
            if (k) atomicAdd(st + 2, 1u);
        }
    }
}

// ------------------------------------------------------------------ host
// a margin of 1/4 + 256 bytes on every growth: kept as found
typedef SlxDevBuf<SlxMargin<4, 256>> FltDBuf;

struct slx_filter {
    std::vector<RfHostFilter> filters;
    RfCompiled C;
    bool compiled = false;
    int up_device = -1, buf_device = -1;                 // the device the current tables lie on (-1: not uploaded), and the one the buffers belong to
    FltDBuf d_flt, d_rules, d_regs, d_strs, d_dfa, d_st, d_long;
    rf_tab dtab;                                         // C.tab with device pointers
    hipStream_t own = nullptr; int own_device = -1;      // slx_filter_apply_device's stream
    hipEvent_t ev[2] = {nullptr, nullptr}; int ev_device = -1;
    uint32_t window = 16384, overhang = 2048, chunk_bases = 0;
    int64_t c_seen = 0, c_passed = 0, c_long = 0, c_in_lds = 0;
    double us = 0;
};

static int flt_compile(slx_filter *f)
{
    if (f->compiled) return SLX_OK;
    if (!rf_compile(f->filters, f->C)) { slx_set_error("read filter: more than %d rules with motifs", RF_MAX_DFA); return SLX_EUNSUPPORTED; }
    f->compiled = true; f->up_device = -1;
    return SLX_OK;
}

extern "C" int slx_filter_create(slx_filter **out)
{
    if (!out) { slx_set_error("slx_filter_create: f is null"); return SLX_EINVAL; }
    *out = new slx_filter();
    return SLX_OK;
}

extern "C" void slx_filter_free(slx_filter *f)
{
    if (!f) return;
    if (f->buf_device >= 0 || f->own || f->ev[0]) {
        if (f->buf_device >= 0) (void)hipSetDevice(f->buf_device);
        for (FltDBuf *b : {&f->d_flt, &f->d_rules, &f->d_regs, &f->d_strs, &f->d_dfa, &f->d_st, &f->d_long}) b->release();
        for (auto &e : f->ev) if (e) (void)hipEventDestroy(e);
        if (f->own) (void)hipStreamDestroy(f->own);
    }
    delete f;
}

extern "C" int slx_filter_add_filter(slx_filter *f, int excluder, int mate_linked, const slx_bam_region *regs, int64_t n)
{
    if (!f || n < 0 || (n && !regs)) { slx_set_error("slx_filter_add_filter: null argument"); return SLX_EINVAL; }
    RfHostFilter hf;
    hf.excluder = excluder != 0; hf.mate = mate_linked != 0;
    if (n) hf.regs.assign(regs, regs + n);
    f->filters.push_back(std::move(hf));
    f->compiled = false;
    return (int)f->filters.size() - 1;
}

extern "C" int slx_filter_add_rule(slx_filter *f, int filter_id, const slx_filter_rule *r, const char *read_group, const char *const *motifs, int64_t n_motifs)
{
    if (!f || n_motifs < 0 || (n_motifs && !motifs)) { slx_set_error("slx_filter_add_rule: null argument"); return SLX_EINVAL; }
    if (filter_id < 0 || filter_id >= (int)f->filters.size()) { slx_set_error("slx_filter_add_rule: filter %d of %zu", filter_id, f->filters.size()); return SLX_EINVAL; }
    RfHostRule hr;
    if (r) hr.r = *r;
    else {
        memset(&hr.r, 0, sizeof hr.r);
        for (auto &g : hr.r.r) g.every = 1;
        hr.r.subsample_frac = 1; hr.r.subsample_seed = 999;
    }
    if (read_group) hr.rg = read_group;
    for (int64_t i = 0; i < n_motifs; ++i) {
        if (!motifs[i]) { slx_set_error("slx_filter_add_rule: motif %lld is null", (long long)i); return SLX_EINVAL; }
        hr.motifs.emplace_back(motifs[i]);
    }
    f->filters[filter_id].rules.push_back(std::move(hr));
    f->compiled = false;
    return SLX_OK;
}

extern "C" int slx_filter_set(slx_filter *f, const char *key, int64_t value)
{
    if (!f || !key) { slx_set_error("slx_filter_set: null argument"); return SLX_EINVAL; }
    const std::string k(key);
    if (k == "window_bytes" && value >= 64 && value % 16 == 0 && value + f->overhang <= 49152) { f->window = (uint32_t)value; return SLX_OK; }
    if (k == "overhang_bytes" && value >= 48 && value % 16 == 0 && value + f->window <= 49152) { f->overhang = (uint32_t)value; return SLX_OK; }
    if (k == "chunk_bases" && value >= 0 && value <= (1ll << 30)) { f->chunk_bases = (uint32_t)value; return SLX_OK; }
    slx_set_error("slx_filter_set: unknown key or value out of range: %s = %lld", key, (long long)value);
    return SLX_EINVAL;
}

extern "C" int64_t slx_filter_counter(const slx_filter *f, const char *name)
{
    if (!f || !name) return -1;
    const std::string k(name);
    if (k == "seen") return f->c_seen;
    if (k == "passed") return f->c_passed;
    if (k == "us_filter") return (int64_t)f->us;
    if (k == "long_records") return f->c_long;
    if (k == "dfa_states") return f->compiled ? (int64_t)f->C.n_states : 0;
    if (k == "dfa_in_lds") return f->c_in_lds;
    return -1;
}

static int flt_record_error(uint32_t bits)
{
    if (bits & RF_E_FIELDS) slx_set_error("BAM: a record's fields pass its block_size");
    else slx_set_error("BAM: a record's fields pass its block_size (an aux field of unknown type, or one that passes the record's end)");
    return SLX_EIO;
}

extern "C" int slx_filter_test_record(slx_filter *f, const uint8_t *rec, int64_t n)
{
    if (!f || !rec || n < 0) { slx_set_error("slx_filter_test_record: null argument"); return SLX_EINVAL; }
    SLX_CHK(flt_compile(f));
    rf_feat F;
    const uint32_t er = n < 4 ? RF_E_FIELDS : rf_features(rec, (uint64_t)n, &f->C.tab, &F);
    if (er) return flt_record_error(er);
    const bool k = rf_eval(&f->C.tab, &F);
    ++f->c_seen; f->c_passed += k;
    return k ? 1 : 0;
}

extern "C" int slx_filter_features(const uint8_t *rec, int64_t n, slx_filter_feat *out)
{
    if (!rec || !out || n < 0) { slx_set_error("slx_filter_features: null argument"); return SLX_EINVAL; }
    rf_tab T;
    memset(&T, 0, sizeof T);
    T.need = RF_NEED_CIGAR | RF_NEED_AUX | RF_NEED_NCOUNT;
    rf_feat F;
    const uint32_t er = n < 4 ? RF_E_FIELDS : rf_features(rec, (uint64_t)n, &T, &F);
    if (er) return flt_record_error(er);
    memset(out, 0, sizeof *out);
    out->full_insert_size = rf_full_isize(&F); out->pair_orientation = rf_orientation(&F);
    out->pair_mapped = rf_pair_mapped(F.flag); out->interchromosomal = F.tid != F.mtid && out->pair_mapped;
    out->num_clip = (int32_t)F.clip; out->num_hard_clip = (int32_t)F.hclip; out->max_ins = (int32_t)F.max_ins; out->max_del = (int32_t)F.max_del;
    out->n_bases_n = (int32_t)F.n_n; out->nm = F.has_nm ? F.nm : 0; out->has_nm = (int32_t)F.has_nm; out->end = (int32_t)rf_end(&F);
    const uint32_t l = F.rg_len < 255 ? F.rg_len : 255;
    if (F.rg_na) memcpy(out->read_group, "NA", 2); else if (l) memcpy(out->read_group, F.rg, l);
    return SLX_OK;
}

static int flt_upload(slx_filter *f, int device, hipStream_t st)
{
    SLX_CHK(flt_compile(f));
    if (f->up_device == device) return SLX_OK;
    if (f->buf_device >= 0 && f->buf_device != device) {          // the buffers of another device go
        SLX_HIPCHK(hipSetDevice(f->buf_device));
        for (FltDBuf *b : {&f->d_flt, &f->d_rules, &f->d_regs, &f->d_strs, &f->d_dfa, &f->d_st, &f->d_long}) b->release();
        SLX_HIPCHK(hipSetDevice(device));
    }
    f->up_device = -1; f->buf_device = device;
    const RfCompiled &C = f->C;
    auto up = [&](FltDBuf &b, const void *src, size_t bytes) -> int {
        SLX_CHK(b.ensure(bytes + 16));
        if (bytes) SLX_HIPCHK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st));
        return SLX_OK;
    };
    SLX_CHK(up(f->d_flt, C.flt.data(), sizeof(rf_filter) * C.flt.size())); SLX_CHK(up(f->d_rules, C.rules.data(), sizeof(rf_rule) * C.rules.size()));
    SLX_CHK(up(f->d_regs, C.regs.data(), sizeof(rf_reg) * C.regs.size())); SLX_CHK(up(f->d_strs, C.strs.data(), C.strs.size()));
    SLX_CHK(up(f->d_dfa, C.dfa.data(), 4 * C.dfa.size())); SLX_CHK(f->d_st.ensure(16));
    SLX_HIPCHK(hipStreamSynchronize(st));
    f->dtab = C.tab;
    f->dtab.flt = (const rf_filter *)f->d_flt.p; f->dtab.rules = (const rf_rule *)f->d_rules.p; f->dtab.regs = (const rf_reg *)f->d_regs.p;
    f->dtab.strs = (const uint8_t *)f->d_strs.p; f->dtab.dfa = (const uint32_t *)f->d_dfa.p;
    f->up_device = device;
    return SLX_OK;
}

int slx_filter_eval_device(slx_filter *f, int device, void *stream, const uint8_t *s, const uint64_t *rec, uint64_t n_rec, uint64_t n_bytes, uint8_t *d_keep, uint64_t *n_kept)
{
    hipStream_t st = (hipStream_t)stream;
    if (n_kept) *n_kept = 0;
    if (n_rec >= 0xffffffffull) { slx_set_error("read filter: %llu records in one batch", (unsigned long long)n_rec); return SLX_EUNSUPPORTED; }
    SLX_CHK(flt_upload(f, device, st));
    if (n_rec == 0) return SLX_OK;
    if (n_bytes < 36 * n_rec) return flt_record_error(RF_E_FIELDS);
    if (f->ev_device != device) {
        for (auto &e : f->ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
        for (auto &e : f->ev) SLX_HIPCHK(hipEventCreate(&e));
        f->ev_device = device;
    }
    SLX_CHK(f->d_long.ensure(4 * (size_t)n_rec));
    uint32_t *d_st = (uint32_t *)f->d_st.p;
    const uint32_t W = f->window, V = f->overhang, stage = W + V + 16;
    const size_t dfa_bytes = 4 * f->C.dfa.size();
    const bool in_lds = dfa_bytes && stage + dfa_bytes <= FLT_LDS_MAX;
    const uint64_t n_win = (n_bytes + W - 1) / W;
    if (n_win >= 0x7fffffffull) { slx_set_error("read filter: %llu windows in one batch", (unsigned long long)n_win); return SLX_EUNSUPPORTED; }
    SLX_HIPCHK(hipMemsetAsync(d_st, 0, 16, st));
    SLX_HIPCHK(hipMemsetAsync(d_keep, 0, n_rec, st));
    SLX_HIPCHK(hipEventRecord(f->ev[0], st));
    k_flt_eval<<<(unsigned)n_win, 256, stage + (in_lds ? dfa_bytes : 0), st>>>(s, rec, n_rec, n_bytes, W, V, f->dtab, in_lds ? (uint32_t)f->C.dfa.size() : 0u, d_keep, (uint32_t *)f->d_long.p, d_st);
    SLX_HIPCHK(hipGetLastError());
    const uint64_t long_blocks = std::min<uint64_t>((n_rec + 3) / 4, 1024);
    k_flt_eval_long<<<(unsigned)long_blocks, 256, 0, st>>>(s, rec, n_rec, f->dtab, f->chunk_bases, d_keep, (const uint32_t *)f->d_long.p, d_st);
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(f->ev[1], st));
    uint32_t h[4] = {0, 0, 0, 0};
    SLX_HIPCHK(hipMemcpyAsync(h, d_st, 16, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    f->us += slx_ev_us(f->ev[0], f->ev[1]);
    f->c_in_lds = in_lds; f->c_long += h[0];
    if (h[1]) return flt_record_error(h[1]);
    f->c_seen += (int64_t)n_rec; f->c_passed += h[2];
    if (n_kept) *n_kept = h[2];
    return SLX_OK;
}

extern "C" int slx_filter_apply_device(slx_filter *f, int device, const void *d_stream, const void *d_rec_off, int64_t n_records, void *d_keep, int64_t *n_kept)
{
    if (!f || n_records < 0 || (n_records && (!d_stream || !d_rec_off || !d_keep))) { slx_set_error("slx_filter_apply_device: null argument"); return SLX_EINVAL; }
    if (n_kept) *n_kept = 0;
    SLX_CHK(slx_pick_device(device, "no HIP device: the read filter evaluates batches on MI355X only (no CPU fallback)", "read filter", &device));
    if (f->own_device != device) {
        if (f->own) (void)hipStreamDestroy(f->own);
        f->own = nullptr;
        SLX_HIPCHK(hipStreamCreateWithFlags(&f->own, hipStreamNonBlocking));
        f->own_device = device;
    }
    uint64_t n_bytes = 0;
    if (n_records) {
        SLX_HIPCHK(hipMemcpyAsync(&n_bytes, (const uint64_t *)d_rec_off + n_records, 8, hipMemcpyDeviceToHost, f->own));
        SLX_HIPCHK(hipStreamSynchronize(f->own));
    }
    uint64_t k = 0;
    SLX_CHK(slx_filter_eval_device(f, device, f->own, (const uint8_t *)d_stream, (const uint64_t *)d_rec_off, (uint64_t)n_records, n_bytes, (uint8_t *)d_keep, &k));
    if (n_kept) *n_kept = (int64_t)k;
    return SLX_OK;
}

extern "C" int slx_filter_attach(slx_filter *f, slx_bam *rd)
{
    if (!rd) { slx_set_error("slx_filter_attach: reader is null"); return SLX_EINVAL; }
    if (f) SLX_CHK(flt_compile(f));
    slx_reader_set_filter(rd, f);
    return SLX_OK;
}
