// slx_dup.hip -- duplicate marking of BAM records in HBM (include/seqlib_amd_dup.h): batches of records in, one signature per record kept, a verdict per input
// ordinal out, bit 0x400 rewritten in place.  The kernels are dev_dup.h's, the per-record body dup_host.h's.  DESIGN.md section 9.15.
//   add:     k_dup_sig, k_dup_sig_long, k_dup_sizes, two exclusive sums (paired records; name bytes), k_dup_commit
//   finish:  the name join (radix sort over the low hash_bits of the hash, runs, k_dup_join), one entry per pair, then for pairs and for records the same
//            grouping: a stable radix pass per key word, least significant first, run heads, an inclusive max-scan, the verdict
//   apply:   k_dup_apply, a checking launch and a writing one
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "slx_internal.h"
#include "slx_hip.h"
#include "seqlib_amd_dup.h"
#include "seqlib_amd_bam.h"
#include <unistd.h>
#include "dev_wave.h"
#include "dev_dup.h"

typedef unsigned long long ull;
typedef SlxDevBuf<SlxMargin<8, 256>> DBuf;
typedef SlxDevBuf<SlxMargin<2, 4096>> DCol;          // a column that grows with every add and keeps what it holds: half as much again, so that the copies stay few
typedef SlxDevBuf<SlxExact> DSeg;
typedef SlxPinBuf<SlxExact> DHBuf;

static const char DUP_NO_DEVICE[] = "no HIP device: duplicates are marked on MI355X only (no CPU fallback)";
#define DUP_SEG_MIN (1ull << 20)          // a name segment holds this much at least
#define DUP_REC_BYTES 22ull               // the columns of a record: hi, lo, score, cls, verdict
#define DUP_PAIRED_BYTES 28ull            // ... and of a paired record: ordinal, hash, name address, length, mate
#define DUP_MAX_RECORDS 0x7fffffffull

struct dp_seg { std::unique_ptr<DSeg> buf; uint64_t used = 0; };
struct dp_counts { int64_t ignored = 0, long_records = 0, pairs = 0, orphans = 0, dup_pairs = 0, dup_frags = 0, mixed = 0; };

struct slx_dup : SlxGpu<2> {
    slx_dup() : SlxGpu(DUP_NO_DEVICE) {}
    dp_header hdr;
    dp_libtab T = {nullptr, nullptr, nullptr, nullptr, 0u, 0u};          // the device's copy of hdr
    int64_t max_bytes = 0, wave_len = DP_WAVE_LEN, hash_bits = 64, run_max = 4096;
    uint64_t n = 0, m = 0, name_bytes = 0;
    bool finished = false;
    std::vector<dp_seg> segs;
    dp_counts c;
    double us_sig = 0, us_place = 0, us_commit = 0, us_join = 0, us_pairs = 0, us_group = 0, us_apply = 0;
    DBuf d_slots{*this}, d_koff{*this}, d_lib{*this}, d_pool{*this};
    DBuf d_in{*this}, d_off{*this}, d_S{*this}, d_long{*this}, d_pcnt{*this}, d_poff{*this}, d_nlen{*this}, d_noff{*this}, d_state{*this}, d_tmp{*this};
    DCol d_hi{*this}, d_lo{*this}, d_score{*this}, d_cls{*this}, d_pord{*this}, d_phash{*this}, d_pname{*this}, d_plen{*this};
    DBuf d_ver{*this}, d_key{*this}, d_key2{*this}, d_perm{*this}, d_perm2{*this}, d_pos{*this}, d_head{*this}, d_k0{*this}, d_mate{*this}, d_islo{*this}, d_eoff{*this};
    DBuf d_eahi{*this}, d_ealo{*this}, d_ebhi{*this}, d_eblo{*this}, d_ek0{*this}, d_eoa{*this}, d_eob{*this};
    DHBuf h_small{*this};
    dp_cols cols() const
    {
        return dp_cols{d_hi.as<ull>(), d_lo.as<ull>(), d_score.as<uint32_t>(), d_cls.as<uint8_t>(), d_pord.as<uint32_t>(), d_phash.as<ull>(), d_pname.as<ull>(), d_plen.as<uint32_t>()};
    }
    uint64_t held() const { return DUP_REC_BYTES * n + DUP_PAIRED_BYTES * m + name_bytes; }
};

static unsigned dup_blocks(uint64_t n, unsigned per = 256) { return (unsigned)((n + per - 1) / per); }
#define DUP_T0(d) SLX_HIPCHK(hipEventRecord((d)->ev[0], (d)->st))
#define DUP_T1(d, acc) do { SLX_HIPCHK(hipEventRecord((d)->ev[1], (d)->st)); SLX_HIPCHK(slx_wait_stream((d)->st)); acc += slx_ev_us((d)->ev[0], (d)->ev[1]); } while (0)

extern "C" void slx_dup_free(slx_dup *d)
{
    if (!d) return;
    d->close();
    delete d;
}

extern "C" int slx_dup_create(int device, slx_dup **out)
{
    if (!out) { slx_set_error("slx_dup_create: null argument"); return SLX_EINVAL; }
    return slx_create(out, slx_dup_free, [&](slx_dup *d) {
        SLX_CHK(d->open(device, "slx_dup_create", DUP_NO_DEVICE));
        size_t free_b = 0, total_b = 0;
        SLX_HIPCHK(hipMemGetInfo(&free_b, &total_b));
        d->max_bytes = std::max<int64_t>((int64_t)(free_b / 4), 1);
        SLX_CHK(d->h_small.ensure(512));
        SLX_CHK(d->d_state.ensure(sizeof(dp_state)));
        return (int)SLX_OK;
    });
}

extern "C" int slx_dup_set(slx_dup *d, const char *key, int64_t v)
{
    if (!d || !key) { slx_set_error("slx_dup_set: null argument"); return SLX_EINVAL; }
    if (!strcmp(key, "max_bytes") && v >= 1) { d->max_bytes = v; return SLX_OK; }
    if (!strcmp(key, "wave_len") && v >= 0 && v <= (1 << 20)) { d->wave_len = v; return SLX_OK; }
    if (!strcmp(key, "hash_bits") && v >= 0 && v <= 64) { d->hash_bits = v; return SLX_OK; }
    if (!strcmp(key, "run_max") && v >= 1 && v <= 0x7fffffff) { d->run_max = v; return SLX_OK; }
    slx_set_error("slx_dup_set: unknown key '%s' or value %lld out of range", key, (long long)v);
    return SLX_EINVAL;
}

extern "C" int64_t slx_dup_counter(const slx_dup *d, const char *name)
{
    if (!d || !name) return -1;
    const std::string k = name;
    if (k == "device") return d->device;
    if (k == "max_bytes") return d->max_bytes;
    if (k == "wave_len") return d->wave_len;
    if (k == "hash_bits") return d->hash_bits;
    if (k == "run_max") return d->run_max;
    if (k == "libraries") return d->hdr.n_lib;
    if (k == "read_groups") return (int64_t)d->hdr.ids.size();
    if (k == "records") return (int64_t)d->n;
    if (k == "ignored") return d->c.ignored;
    if (k == "paired") return (int64_t)d->m;
    if (k == "fragments") return (int64_t)d->n - d->c.ignored - (int64_t)d->m;
    if (k == "long_records") return d->c.long_records;
    if (k == "held_bytes") return (int64_t)d->held();
    if (k == "finished") return d->finished ? 1 : 0;
    if (k == "pairs") return d->c.pairs;
    if (k == "orphans") return d->c.orphans;
    if (k == "duplicate_pairs") return d->c.dup_pairs;
    if (k == "duplicate_fragments") return d->c.dup_frags;
    if (k == "duplicates") return 2 * d->c.dup_pairs + d->c.dup_frags;
    if (k == "hash_runs_mixed") return d->c.mixed;
    if (k == "us_sig") return (int64_t)d->us_sig;
    if (k == "us_place") return (int64_t)d->us_place;
    if (k == "us_commit") return (int64_t)d->us_commit;
    if (k == "us_join") return (int64_t)d->us_join;
    if (k == "us_pairs") return (int64_t)d->us_pairs;
    if (k == "us_group") return (int64_t)d->us_group;
    if (k == "us_apply") return (int64_t)d->us_apply;
    return -1;
}

extern "C" int slx_dup_set_header(slx_dup *d, const char *text, int64_t l_text)
{
    SLX_CHK(slx_need(d, "slx_dup_set_header"));
    if (l_text < 0 || (l_text && !text)) { slx_set_error("slx_dup_set_header: null or negative argument"); return SLX_EINVAL; }
    if (d->n || d->finished) { slx_set_error("slx_dup_set_header: the marker holds %llu records (the header comes before the first add, or after slx_dup_clear)", (ull)d->n); return SLX_EINVAL; }
    if (!d->hdr.parse(text, l_text)) {
        slx_set_error("slx_dup_set_header: %u libraries, %u at most", d->hdr.n_lib, DP_MAX_LIB);
        d->hdr.clear();
        d->T = dp_libtab{nullptr, nullptr, nullptr, nullptr, 0u, 0u};
        return SLX_EUNSUPPORTED;
    }
    const dp_libtab H = d->hdr.view();
    d->T = dp_libtab{nullptr, nullptr, nullptr, nullptr, 0u, 0u};
    if (H.n == 0) return SLX_OK;
    const size_t n_slots = (size_t)H.mask + 1, n_pool = d->hdr.pool.size();
    SLX_CHK(d->d_slots.ensure(4 * n_slots)); SLX_CHK(d->d_koff.ensure(4 * ((size_t)H.n + 1))); SLX_CHK(d->d_lib.ensure(4 * (size_t)H.n)); SLX_CHK(d->d_pool.ensure(n_pool + 1));
    SLX_HIPCHK(hipMemcpyAsync(d->d_slots.p, H.slots, 4 * n_slots, hipMemcpyHostToDevice, d->st));
    SLX_HIPCHK(hipMemcpyAsync(d->d_koff.p, H.koff, 4 * ((size_t)H.n + 1), hipMemcpyHostToDevice, d->st));
    SLX_HIPCHK(hipMemcpyAsync(d->d_lib.p, H.lib, 4 * (size_t)H.n, hipMemcpyHostToDevice, d->st));
    SLX_HIPCHK(hipMemcpyAsync(d->d_pool.p, H.pool, n_pool, hipMemcpyHostToDevice, d->st));
    SLX_HIPCHK(slx_wait_stream(d->st));
    d->T = dp_libtab{d->d_slots.as<uint32_t>(), d->d_koff.as<uint32_t>(), d->d_lib.as<uint32_t>(), d->d_pool.as<uint8_t>(), H.mask, H.n};
    return SLX_OK;
}

extern "C" int slx_dup_library_of(const char *text, int64_t l_text, const char *rg, int64_t l_rg)
{
    if (l_text < 0 || l_rg < 0 || (l_text && !text) || (l_rg && !rg) || l_rg > 0x7fffffff) { slx_set_error("slx_dup_library_of: null or negative argument"); return SLX_EINVAL; }
    dp_header h;
    if (!h.parse(text, l_text)) { slx_set_error("slx_dup_library_of: %u libraries, %u at most", h.n_lib, DP_MAX_LIB); return SLX_EUNSUPPORTED; }
    return (int)dp_lookup(h.view(), (const uint8_t *)rg, (uint32_t)l_rg);
}

extern "C" int slx_dup_signature_host(const char *text, int64_t l_text, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records, slx_dup_sig *out)
{
    if (l_text < 0 || (l_text && !text) || (n_records && !out)) { slx_set_error("slx_dup_signature_host: null or negative argument"); return SLX_EINVAL; }
    SLX_CHK(slx_batch_args("slx_dup_signature_host", stream, n_bytes, rec_off, n_records));
    dp_header h;
    if (!h.parse(text, l_text)) { slx_set_error("slx_dup_signature_host: %u libraries, %u at most", h.n_lib, DP_MAX_LIB); return SLX_EUNSUPPORTED; }
    std::vector<dp_sig> S;
    uint64_t bad = ED_NONE;
    if (!dp_signatures_on_host(h.view(), (const uint8_t *)stream, (uint64_t)n_bytes, rec_off, (uint64_t)n_records, &S, &bad)) {
        slx_set_error("duplicate marker: record %llu of the batch: its fields pass its block_size, its name does not end in NUL, or its extent is not block_size + 4 inside the stream", (ull)bad);
        return SLX_EIO;
    }
    for (int64_t i = 0; i < n_records; ++i) {
        const dp_sig &s = S[(size_t)i];
        slx_dup_sig &o = out[i];
        memset(&o, 0, sizeof o);
        o.cls = (int32_t)(s.cls & DP_CLASS);
        if (o.cls == DP_IGNORED) continue;
        o.library = (int32_t)s.library; o.refid = (int32_t)(uint32_t)s.hi; o.reverse = (int32_t)(s.lo & 1u);
        o.upos = (int64_t)(s.lo >> 1) - (1ll << 62); o.score = (int64_t)s.score; o.hash = s.hash;
    }
    return SLX_OK;
}

// the segment that takes `need` more bytes of names: the last one when it has room, an emptied one of a cleared marker that is large enough, or a new one
static int dup_segment(slx_dup *d, uint64_t need, size_t *seg_at)
{
    if (!d->segs.empty()) {
        dp_seg &s = d->segs.back();
        if (s.buf->cap - s.used >= need) { *seg_at = d->segs.size() - 1; return SLX_OK; }
    }
    for (size_t k = 0; k < d->segs.size(); ++k)
        if (d->segs[k].used == 0 && d->segs[k].buf->cap >= need) { std::swap(d->segs[k], d->segs.back()); *seg_at = d->segs.size() - 1; return SLX_OK; }
    dp_seg s;
    s.buf.reset(new DSeg(*d));
    SLX_CHK(s.buf->ensure((size_t)std::max<uint64_t>(need, DUP_SEG_MIN)));
    d->segs.push_back(std::move(s));
    *seg_at = d->segs.size() - 1;
    return SLX_OK;
}

static int dup_add(slx_dup *d, const char *who, const uint8_t *d_s, uint64_t n_bytes, const uint64_t *d_off, uint64_t n)
{
    hipStream_t st = d->st;
    if (d->finished) { slx_set_error("%s: the marker is finished (slx_dup_clear before the next input)", who); return SLX_EINVAL; }
    if (n == 0) {
        if (n_bytes) { slx_set_error("duplicate marker: %llu bytes and no record", (ull)n_bytes); return SLX_EIO; }
        return SLX_OK;
    }
    if (d->n + n > DUP_MAX_RECORDS) { slx_set_error("%s: %llu records with this batch, 2^31 - 1 at most (hipCUB counts in int)", who, (ull)(d->n + n)); return SLX_EUNSUPPORTED; }
    SLX_CHK(d->d_S.ensure(sizeof(dp_sig) * n)); SLX_CHK(d->d_long.ensure(4 * n)); SLX_CHK(d->d_pcnt.ensure(8 * (n + 1))); SLX_CHK(d->d_poff.ensure(8 * (n + 1)));
    SLX_CHK(d->d_nlen.ensure(8 * (n + 1))); SLX_CHK(d->d_noff.ensure(8 * (n + 1)));
    dp_state *hs = d->h_small.as<dp_state>();
    memset(hs, 0, sizeof(dp_state));
    hs->bad = ED_NONE;
    const dp_args A = {d_s, n_bytes, d_off, n};
    double us_sig = 0, us_place = 0, us_commit = 0;
    SLX_HIPCHK(hipMemcpyAsync(d->d_state.p, hs, sizeof(dp_state), hipMemcpyHostToDevice, st));
    DUP_T0(d);
    k_dup_sig<<<dup_blocks(n), 256, 0, st>>>(d->T, A, (uint32_t)d->wave_len, d->d_S.as<dp_sig>(), d->d_long.as<uint32_t>(), d->d_state.as<dp_state>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipMemcpyAsync(hs + 1, d->d_state.p, sizeof(dp_state), hipMemcpyDeviceToHost, st));
    DUP_T1(d, us_sig);
    if (hs[1].bad != ED_NONE) {
        slx_set_error("duplicate marker: record %llu of the batch: its fields pass its block_size, its name does not end in NUL, or its extent is not block_size + 4 inside the stream", hs[1].bad);
        return SLX_EIO;
    }
    const uint32_t n_long = hs[1].n_long;
    DUP_T0(d);
    if (n_long) {
        k_dup_sig_long<<<dup_blocks(n_long, 4), 256, 0, st>>>(d->T, A, d->d_long.as<uint32_t>(), n_long, d->d_S.as<dp_sig>());
        SLX_HIPCHK(hipGetLastError());
    }
    k_dup_sizes<<<dup_blocks(n + 1), 256, 0, st>>>(d->d_S.as<dp_sig>(), n, d->d_pcnt.as<ull>(), d->d_nlen.as<ull>(), d->d_state.as<dp_state>());
    SLX_HIPCHK(hipGetLastError());
    SLX_CHK(slx_exclusive_sum(d->d_tmp, d->d_pcnt.as<ull>(), d->d_poff.as<ull>(), n + 1, st, 16));
    SLX_CHK(slx_exclusive_sum(d->d_tmp, d->d_nlen.as<ull>(), d->d_noff.as<ull>(), n + 1, st, 16));
    ull *tot = (ull *)(hs + 2);
    SLX_HIPCHK(hipMemcpyAsync(tot, d->d_poff.as<ull>() + n, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync(tot + 1, d->d_noff.as<ull>() + n, 8, hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync(hs + 1, d->d_state.p, sizeof(dp_state), hipMemcpyDeviceToHost, st));
    DUP_T1(d, us_place);
    const uint64_t m_new = tot[0], names_new = tot[1], N = d->n + n, M = d->m + m_new;
    const uint64_t after = DUP_REC_BYTES * N + DUP_PAIRED_BYTES * M + d->name_bytes + names_new;
    if (after > (uint64_t)d->max_bytes) {
        slx_set_error("%s: the marker would hold %llu bytes with this batch, \"max_bytes\" is %lld", who, (ull)after, (long long)d->max_bytes);
        return SLX_EUNSUPPORTED;
    }
    // the columns grow and keep what they hold; a growth that fails leaves them as they were
    SLX_CHK(d->d_hi.ensure(8 * N, st, 8 * d->n)); SLX_CHK(d->d_lo.ensure(8 * N, st, 8 * d->n)); SLX_CHK(d->d_score.ensure(4 * N, st, 4 * d->n)); SLX_CHK(d->d_cls.ensure(N, st, d->n));
    SLX_CHK(d->d_pord.ensure(4 * M + 4, st, 4 * d->m)); SLX_CHK(d->d_phash.ensure(8 * M + 8, st, 8 * d->m)); SLX_CHK(d->d_pname.ensure(8 * M + 8, st, 8 * d->m));
    SLX_CHK(d->d_plen.ensure(4 * M + 4, st, 4 * d->m));
    uint8_t *seg = nullptr;
    size_t seg_at = 0;
    if (names_new) {
        SLX_CHK(dup_segment(d, names_new, &seg_at));
        seg = d->segs[seg_at].buf->as<uint8_t>() + d->segs[seg_at].used;
    }
    DUP_T0(d);
    k_dup_commit<<<dup_blocks(n), 256, 0, st>>>(A, d->d_S.as<dp_sig>(), d->d_poff.as<ull>(), d->d_noff.as<ull>(), d->n, d->m, seg, d->cols());
    SLX_HIPCHK(hipGetLastError());
    DUP_T1(d, us_commit);
    // only now does the marker change
    if (names_new) d->segs[seg_at].used += names_new;
    d->n = N; d->m = M; d->name_bytes += names_new;
    d->c.ignored += hs[1].n_ignored; d->c.long_records += n_long;
    d->us_sig += us_sig; d->us_place += us_place; d->us_commit += us_commit;
    return SLX_OK;
}

extern "C" int slx_dup_add_device(slx_dup *d, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records)
{
    SLX_CHK(slx_need(d, "slx_dup_add_device"));
    SLX_CHK(slx_batch_args("slx_dup_add_device", d_stream, n_bytes, d_rec_off, n_records));
    return dup_add(d, "slx_dup_add_device", (const uint8_t *)d_stream, (uint64_t)n_bytes, (const uint64_t *)d_rec_off, (uint64_t)n_records);
}

extern "C" int slx_dup_add_host(slx_dup *d, const void *stream, int64_t n_bytes, const uint64_t *rec_off, int64_t n_records)
{
    SLX_CHK(slx_need(d, "slx_dup_add_host"));
    SLX_CHK(slx_batch_args("slx_dup_add_host", stream, n_bytes, rec_off, n_records));
    if (n_records) {
        SLX_CHK(slx_batch_stage(d->d_in, d->d_off, 16, stream, n_bytes, rec_off, n_records, d->st));
        SLX_HIPCHK(slx_wait_stream(d->st));
    }
    return dup_add(d, "slx_dup_add_host", d->d_in.as<uint8_t>(), (uint64_t)n_bytes, d->d_off.as<uint64_t>(), (uint64_t)n_records);
}

// one stable radix pass: the n elements that *perm lists are reordered by word[element] over its low `bits`; *perm and *perm2 change places
static int dup_pass(slx_dup *d, const ull *word, int bits, uint64_t n, uint32_t **perm, uint32_t **perm2)
{
    hipStream_t st = d->st;
    ull *key = d->d_key.as<ull>(), *key2 = d->d_key2.as<ull>();
    k_dup_take<<<dup_blocks(n), 256, 0, st>>>(word, *perm, n, key);
    SLX_HIPCHK(hipGetLastError());
    uint32_t *in = *perm, *out = *perm2;
    SLX_CHK(slx_cub("hipcub::DeviceRadixSort::SortPairs", d->d_tmp, 16, [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, key, key2, in, out, (int)n, 0, bits, st); }));
    std::swap(*perm, *perm2);
    return SLX_OK;
}
// head[i]: the position of the head of the run that sorted element i lies in (pos: k_dup_heads)
static int dup_max_scan(slx_dup *d, uint64_t n)
{
    hipStream_t st = d->st;
    const uint32_t *in = d->d_pos.as<uint32_t>();
    uint32_t *out = d->d_head.as<uint32_t>();
    return slx_cub("hipcub::DeviceScan::InclusiveScan", d->d_tmp, 16, [&](void *t, size_t &b) { return hipcub::DeviceScan::InclusiveScan(t, b, in, out, hipcub::Max(), (int)n, st); });
}

extern "C" int slx_dup_finish(slx_dup *d)
{
    SLX_CHK(slx_need(d, "slx_dup_finish"));
    if (d->finished) return SLX_OK;
    hipStream_t st = d->st;
    const uint64_t N = d->n, M = d->m;
    const dp_cols C = d->cols();
    SLX_CHK(d->d_ver.ensure(N + 1)); SLX_CHK(d->d_key.ensure(8 * N + 8)); SLX_CHK(d->d_key2.ensure(8 * N + 8)); SLX_CHK(d->d_perm.ensure(4 * N + 4)); SLX_CHK(d->d_perm2.ensure(4 * N + 4));
    SLX_CHK(d->d_pos.ensure(4 * N + 4)); SLX_CHK(d->d_head.ensure(4 * N + 4)); SLX_CHK(d->d_k0.ensure(8 * N + 8));
    SLX_CHK(d->d_mate.ensure(4 * M + 4)); SLX_CHK(d->d_islo.ensure(8 * (M + 1))); SLX_CHK(d->d_eoff.ensure(8 * (M + 1)));
    dp_state *hs = d->h_small.as<dp_state>();
    SLX_HIPCHK(hipMemsetAsync(d->d_state.p, 0, sizeof(dp_state), st));
    dp_state *ds = d->d_state.as<dp_state>();
    uint8_t *ver = d->d_ver.as<uint8_t>();
    uint32_t *perm = d->d_perm.as<uint32_t>(), *perm2 = d->d_perm2.as<uint32_t>(), *pos = d->d_pos.as<uint32_t>(), *head = d->d_head.as<uint32_t>();
    double us_join = 0, us_pairs = 0, us_group = 0;
    uint64_t n_ent = 0;
    if (N) {
        k_dup_init<<<dup_blocks(N), 256, 0, st>>>(C.cls, N, ver, d->d_k0.as<ull>(), C.score);
        SLX_HIPCHK(hipGetLastError());
    }
    if (M) {
        // ---- the join of the paired records by (library, name)
        DUP_T0(d);
        ull *key = d->d_key.as<ull>(), *key2 = d->d_key2.as<ull>();
        const ull mask = d->hash_bits >= 64 ? ~0ull : (1ull << d->hash_bits) - 1ull;
        k_dup_pkeys<<<dup_blocks(M), 256, 0, st>>>(C.phash, M, mask, key, perm);
        SLX_HIPCHK(hipGetLastError());
        const ull *skey = key;
        const uint32_t *sidx = perm;
        if (d->hash_bits > 0) {
            const int bits = (int)d->hash_bits;
            SLX_CHK(slx_cub("hipcub::DeviceRadixSort::SortPairs", d->d_tmp, 16, [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, key, key2, perm, perm2, (int)M, 0, bits, st); }));
            skey = key2; sidx = perm2;
        }
        k_dup_heads<<<dup_blocks(M), 256, 0, st>>>(nullptr, M, skey, nullptr, nullptr, nullptr, pos);
        SLX_HIPCHK(hipGetLastError());
        SLX_CHK(dup_max_scan(d, M));
        k_dup_join<<<dup_blocks(M), 256, 0, st>>>(C, skey, sidx, head, M, (uint32_t)d->run_max, d->d_mate.as<uint32_t>(), ds);
        SLX_HIPCHK(hipGetLastError());
        k_dup_islo<<<dup_blocks(M + 1), 256, 0, st>>>(d->d_mate.as<uint32_t>(), M, d->d_islo.as<ull>());
        SLX_HIPCHK(hipGetLastError());
        SLX_CHK(slx_exclusive_sum(d->d_tmp, d->d_islo.as<ull>(), d->d_eoff.as<ull>(), M + 1, st, 16));
        ull *tot = (ull *)(hs + 2);
        SLX_HIPCHK(hipMemcpyAsync(tot, d->d_eoff.as<ull>() + M, 8, hipMemcpyDeviceToHost, st));
        SLX_HIPCHK(hipMemcpyAsync(hs + 1, ds, sizeof(dp_state), hipMemcpyDeviceToHost, st));
        DUP_T1(d, us_join);
        if (hs[1].too_long) {
            slx_set_error("slx_dup_finish: a run of equal hash holds more than \"run_max\" = %lld paired records (\"hash_bits\" is %lld)", (long long)d->run_max, (long long)d->hash_bits);
            return SLX_EUNSUPPORTED;
        }
        n_ent = tot[0];
    }
    if (n_ent) {
        // ---- one entry per pair, grouped by (E(a), E(b)): the head of every group stays, the others are duplicates
        SLX_CHK(d->d_eahi.ensure(8 * n_ent)); SLX_CHK(d->d_ealo.ensure(8 * n_ent)); SLX_CHK(d->d_ebhi.ensure(8 * n_ent)); SLX_CHK(d->d_eblo.ensure(8 * n_ent));
        SLX_CHK(d->d_ek0.ensure(8 * n_ent)); SLX_CHK(d->d_eoa.ensure(4 * n_ent)); SLX_CHK(d->d_eob.ensure(4 * n_ent));
        const dp_ent E = {d->d_eahi.as<ull>(), d->d_ealo.as<ull>(), d->d_ebhi.as<ull>(), d->d_eblo.as<ull>(), d->d_ek0.as<ull>(), d->d_eoa.as<uint32_t>(), d->d_eob.as<uint32_t>()};
        DUP_T0(d);
        k_dup_entries<<<dup_blocks(M), 256, 0, st>>>(C, d->d_mate.as<uint32_t>(), d->d_eoff.as<ull>(), M, E, perm);
        SLX_HIPCHK(hipGetLastError());
        SLX_CHK(dup_pass(d, E.k0, 32, n_ent, &perm, &perm2));
        SLX_CHK(dup_pass(d, E.blo, 64, n_ent, &perm, &perm2));
        SLX_CHK(dup_pass(d, E.bhi, DP_HI_BITS, n_ent, &perm, &perm2));
        SLX_CHK(dup_pass(d, E.alo, 64, n_ent, &perm, &perm2));
        SLX_CHK(dup_pass(d, E.ahi, DP_HI_BITS, n_ent, &perm, &perm2));
        k_dup_heads<<<dup_blocks(n_ent), 256, 0, st>>>(perm, n_ent, E.ahi, E.alo, E.bhi, E.blo, pos);
        SLX_HIPCHK(hipGetLastError());
        SLX_CHK(dup_max_scan(d, n_ent));
        k_dup_pair_verdict<<<dup_blocks(n_ent), 256, 0, st>>>(perm, head, n_ent, E, ver, ds);
        SLX_HIPCHK(hipGetLastError());
        DUP_T1(d, us_pairs);
    }
    if (N) {
        // ---- the records grouped by E: a group's head is a paired record where it holds one, or else its best fragment
        DUP_T0(d);
        k_dup_iota<<<dup_blocks(N), 256, 0, st>>>(perm, N);
        SLX_HIPCHK(hipGetLastError());
        SLX_CHK(dup_pass(d, d->d_k0.as<ull>(), 32, N, &perm, &perm2));
        SLX_CHK(dup_pass(d, C.lo, 64, N, &perm, &perm2));
        SLX_CHK(dup_pass(d, C.hi, DP_HI_BITS, N, &perm, &perm2));
        k_dup_heads<<<dup_blocks(N), 256, 0, st>>>(perm, N, C.hi, C.lo, nullptr, nullptr, pos);
        SLX_HIPCHK(hipGetLastError());
        SLX_CHK(dup_max_scan(d, N));
        k_dup_frag_verdict<<<dup_blocks(N), 256, 0, st>>>(perm, head, N, C.cls, ver, ds);
        SLX_HIPCHK(hipGetLastError());
        SLX_HIPCHK(hipMemcpyAsync(hs + 1, ds, sizeof(dp_state), hipMemcpyDeviceToHost, st));
        DUP_T1(d, us_group);
    } else memset(hs + 1, 0, sizeof(dp_state));
    d->c.pairs = (int64_t)n_ent; d->c.orphans = (int64_t)M - 2 * (int64_t)n_ent; d->c.dup_pairs = hs[1].dup_pairs; d->c.dup_frags = hs[1].dup_frags; d->c.mixed = hs[1].mixed;
    d->us_join += us_join; d->us_pairs += us_pairs; d->us_group += us_group;
    d->finished = true;
    return SLX_OK;
}

extern "C" int slx_dup_flags_to_host(slx_dup *d, uint8_t *dst, int64_t cap)
{
    SLX_CHK(slx_need(d, "slx_dup_flags_to_host"));
    if (!d->finished) { slx_set_error("slx_dup_flags_to_host: no verdicts (slx_dup_finish first)"); return SLX_EINVAL; }
    if (cap < 0 || (uint64_t)cap < d->n || (d->n && !dst)) { slx_set_error("slx_dup_flags_to_host: room for %lld bytes, %llu records", (long long)cap, (ull)d->n); return SLX_EINVAL; }
    if (d->n) SLX_HIPCHK(hipMemcpyAsync(dst, d->d_ver.p, (size_t)d->n, hipMemcpyDeviceToHost, d->st));
    SLX_HIPCHK(slx_wait_stream(d->st));
    return SLX_OK;
}

extern "C" int slx_dup_apply_device(slx_dup *d, void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records, int64_t first_ordinal, const uint32_t *d_ordinals)
{
    SLX_CHK(slx_need(d, "slx_dup_apply_device"));
    SLX_CHK(slx_batch_args("slx_dup_apply_device", d_stream, n_bytes, d_rec_off, n_records));
    if (!d->finished) { slx_set_error("slx_dup_apply_device: no verdicts (slx_dup_finish first)"); return SLX_EINVAL; }
    if (n_records == 0) return SLX_OK;
    if (!d_ordinals && (first_ordinal < 0 || (uint64_t)first_ordinal + (uint64_t)n_records > d->n)) {
        slx_set_error("slx_dup_apply_device: ordinals [%lld, %lld) and %llu records added", (long long)first_ordinal, (long long)(first_ordinal + n_records), (ull)d->n);
        return SLX_EINVAL;
    }
    hipStream_t st = d->st;
    dp_state *hs = d->h_small.as<dp_state>();
    memset(hs, 0, sizeof(dp_state));
    hs->bad = ED_NONE;
    const uint64_t n = (uint64_t)n_records;
    SLX_HIPCHK(hipMemcpyAsync(d->d_state.p, hs, sizeof(dp_state), hipMemcpyHostToDevice, st));
    DUP_T0(d);
    k_dup_apply<<<dup_blocks(n), 256, 0, st>>>((uint8_t *)d_stream, (uint64_t)n_bytes, (const uint64_t *)d_rec_off, n, (uint64_t)first_ordinal, d_ordinals, d->d_ver.as<uint8_t>(), d->n, 0,
                                               d->d_state.as<dp_state>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipMemcpyAsync(hs + 1, d->d_state.p, sizeof(dp_state), hipMemcpyDeviceToHost, st));
    DUP_T1(d, d->us_apply);
    if (hs[1].bad != ED_NONE) { slx_set_error("slx_dup_apply_device: record %llu of the batch does not lie inside the stream", hs[1].bad); return SLX_EIO; }
    if (hs[1].bad_ord) { slx_set_error("slx_dup_apply_device: %u ordinals of the column are beyond the %llu records added", hs[1].bad_ord, (ull)d->n); return SLX_EINVAL; }
    DUP_T0(d);
    k_dup_apply<<<dup_blocks(n), 256, 0, st>>>((uint8_t *)d_stream, (uint64_t)n_bytes, (const uint64_t *)d_rec_off, n, (uint64_t)first_ordinal, d_ordinals, d->d_ver.as<uint8_t>(), d->n, 1,
                                               d->d_state.as<dp_state>());
    SLX_HIPCHK(hipGetLastError());
    DUP_T1(d, d->us_apply);
    return SLX_OK;
}

extern "C" int slx_dup_clear(slx_dup *d)
{
    SLX_CHK(slx_need(d, "slx_dup_clear"));
    SLX_HIPCHK(slx_wait_stream(d->st));
    for (dp_seg &s : d->segs) s.used = 0;
    d->n = d->m = d->name_bytes = 0; d->finished = false;
    d->c = dp_counts();
    d->us_sig = d->us_place = d->us_commit = d->us_join = d->us_pairs = d->us_group = d->us_apply = 0;
    return SLX_OK;
}

// ------------------------------------------------------------------ file to file
static void dup_put32(std::string &o, uint32_t v) { const char b[4] = {(char)v, (char)(v >> 8), (char)(v >> 16), (char)(v >> 24)}; o.append(b, 4); }

// pass 1: the header's @RG lines and every record into the marker.  pass 2: the file again, batch by batch marked in HBM and handed to the GPU BGZF writer
static int dup_file_impl(slx_dup *d, const char *in_path, const char *out_path, int64_t batch_bytes, bool *created)
{
    slx_bam *rd = nullptr;
    SLX_CHK(slx_bam_open(in_path, d->device, &rd));
    std::string h("BAM\1", 4);
    auto pass1 = [&]() -> int {
        const char *text = nullptr; int64_t l_text = 0; int n_ref = 0;
        SLX_CHK(slx_bam_header(rd, &text, &l_text, &n_ref));
        SLX_CHK(slx_dup_set_header(d, text, l_text));
        dup_put32(h, (uint32_t)l_text);
        h.append(text, (size_t)l_text);
        dup_put32(h, (uint32_t)n_ref);
        for (int i = 0; i < n_ref; ++i) {
            const std::string nm = slx_bam_ref_name(rd, i);
            dup_put32(h, (uint32_t)nm.size() + 1);
            h += nm; h.push_back('\0');
            dup_put32(h, (uint32_t)slx_bam_ref_len(rd, i));
        }
        for (;;) {
            slx_bam_batch b;
            SLX_CHK(slx_bam_next(rd, batch_bytes, &b));
            if (b.n_records == 0) break;
            SLX_CHK(slx_dup_add_device(d, b.d_stream, b.n_bytes, b.d_rec_off, b.n_records));
        }
        return slx_dup_finish(d);
    };
    int rc = pass1();
    std::string msg = rc != SLX_OK ? slx_last_error() : "";
    slx_bam_close(rd);
    if (rc != SLX_OK) { slx_set_error("%s", msg.c_str()); return rc; }
    rd = nullptr;
    SLX_CHK(slx_bam_open(in_path, d->device, &rd));
    slx_bgzf *w = nullptr;
    rc = slx_bgzf_open(out_path, d->device, &w);
    if (rc == SLX_OK) {
        *created = true;
        rc = slx_bgzf_write(w, h.data(), (int64_t)h.size());
        if (rc == SLX_OK) rc = slx_bgzf_flush(w);          // the records start in a member of their own, as BamWriter::WriteHeader leaves them
        int64_t first = 0;
        while (rc == SLX_OK) {
            slx_bam_batch b;
            rc = slx_bam_next(rd, batch_bytes, &b);
            if (rc != SLX_OK || b.n_records == 0) break;
            if (first + b.n_records > (int64_t)d->n) { slx_set_error("slx_dup_file: '%s' holds more records in the second pass than in the first", in_path); rc = SLX_EIO; break; }
            rc = slx_dup_apply_device(d, (void *)b.d_stream, b.n_bytes, b.d_rec_off, b.n_records, first, nullptr);
            if (rc == SLX_OK) rc = slx_bgzf_write_device(w, b.d_stream, b.n_bytes);
            first += b.n_records;
        }
        if (rc == SLX_OK && first != (int64_t)d->n) { slx_set_error("slx_dup_file: '%s' holds %lld records in the second pass, %llu in the first", in_path, (long long)first, (ull)d->n); rc = SLX_EIO; }
        msg = rc != SLX_OK ? slx_last_error() : "";
        const int rc2 = slx_bgzf_close(w);
        if (rc == SLX_OK) { rc = rc2; msg = rc != SLX_OK ? slx_last_error() : ""; }
    } else msg = slx_last_error();
    slx_bam_close(rd);
    if (rc != SLX_OK) slx_set_error("%s", msg.c_str());
    return rc;
}

extern "C" int slx_dup_file_ex(slx_dup *d, const char *in_path, const char *out_path, int64_t batch_bytes)
{
    SLX_CHK(slx_need(d, "slx_dup_file"));
    if (!in_path || !out_path || batch_bytes < 1) { slx_set_error("slx_dup_file: null argument or batch_bytes below 1"); return SLX_EINVAL; }
    if (!strcmp(in_path, out_path) || !strcmp(in_path, "-") || !strcmp(out_path, "-")) {
        slx_set_error("slx_dup_file: '%s' -> '%s': the output must be another file than the input, and neither is a pipe (the input is read twice)", in_path, out_path);
        return SLX_EINVAL;
    }
    if (d->n || d->finished) { slx_set_error("slx_dup_file_ex: the marker is not empty (slx_dup_clear first)"); return SLX_EINVAL; }
    bool created = false;
    const int rc = dup_file_impl(d, in_path, out_path, batch_bytes, &created);
    if (rc != SLX_OK) {
        const std::string msg = slx_last_error();
        if (created) (void)unlink(out_path);          // no output file is left behind
        slx_set_error("%s", msg.c_str());
    }
    return rc;
}

extern "C" int slx_dup_file(const char *in_path, const char *out_path, int device)
{
    if (!in_path || !out_path) { slx_set_error("slx_dup_file: null argument"); return SLX_EINVAL; }
    slx_dup *d = nullptr;
    SLX_CHK(slx_dup_create(device, &d));
    const int rc = slx_dup_file_ex(d, in_path, out_path, 64ll << 20);
    const std::string msg = rc != SLX_OK ? slx_last_error() : "";
    slx_dup_free(d);
    if (rc != SLX_OK) slx_set_error("%s", msg.c_str());
    return rc;
}
