// slx_rec.hip -- the record builder of libseqlib_amd.so (include/seqlib_amd_rec.h, slx_rec_*): a device-resident slx_hits, the reads and their names into the
// block_size-prefixed BAM record stream in HBM.  The bodies are dev_rec.h's.
//   k_rec_owner       one lane per read: the read of every hit
//   k_rec_size        one lane per hit: clip window, end, bin, length, refusal; a hit with more than REC_WIDE_OPS CIGAR operations goes on a list instead
//   k_rec_size_wide   one wave per listed hit: the CIGAR shared by the lanes (a contig's 10^5 operations are not one lane's loop)
//   hipCUB            exclusive sum of the lengths = rec_off; one copy-down of the total and the first refusal: the only synchronisation before the fill
//   k_rec_fill        one wave per REC_TILE bytes of the stream, built in LDS, stored 16 bytes per lane
// Hits map to lanes and tiles to waves statically; the only queue is the list of wide hits, taken through dev_wave.h.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "slx_internal.h"
#include "seqlib_amd_rec.h"
#include "dev_wave.h"
#include "dev_rec.h"
#include "slx_hip.h"

typedef unsigned long long ull;

struct rec_state { ull refusal; uint32_t n_wide, pad; };          // refusal: read << 8 | code of the first refused read; REC_NO_REFUSAL = none

// ------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void k_rec_owner(const int64_t *hit_off, int64_t n_reads, int64_t n_hits, int64_t *owner)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_reads) return;
    int64_t a = hit_off[i], b = hit_off[i + 1];
    if (a < 0) a = 0;
    if (b > n_hits) b = n_hits;
    for (int64_t k = a; k < b; ++k) owner[k] = i;
}

__device__ __forceinline__ void rec_refuse(rec_state *st, int64_t read, uint32_t code)
{
    if (code != REC_OK) atomicMin(&st->refusal, (ull)read << 8 | code);
}

__global__ __launch_bounds__(256) void k_rec_size(rec_in in, const int64_t *owner, rec_meta *meta, ull *len, uint32_t *wide_list, rec_state *st)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k == 0) len[in.n_hits] = 0;
    if (k >= in.n_hits) return;
    if (in.n_cigar_ops[k] > REC_WIDE_OPS) { wide_list[wave_fetch_inc(&st->n_wide)] = (uint32_t)k; return; }
    const rec_part p = rec_cigar_part(in, k, 0, 1);
    const int64_t i = owner[k];
    rec_refuse(st, i, rec_size_finish(in, k, i, p, meta, len));
}

__global__ __launch_bounds__(256) void k_rec_size_wide(rec_in in, const int64_t *owner, rec_meta *meta, ull *len, const uint32_t *wide_list, rec_state *st)
{
    const uint32_t n = st->n_wide, lane = threadIdx.x & 63;
    for (uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6); j < n; j += gridDim.x * 4) {
        const int64_t k = wide_list[j];
        rec_part p = rec_cigar_part(in, k, (int)lane, 64);
        for (int o = 32; o; o >>= 1) {
            rec_part q;
            q.tstart = __shfl_xor(p.tstart, o, 64); q.qlen = __shfl_xor(p.qlen, o, 64); q.rlen = __shfl_xor(p.rlen, o, 64); q.any_ref = __shfl_xor(p.any_ref, o, 64);
            rec_part_add(p, q);
        }
        if (lane == 0) { const int64_t i = owner[k]; rec_refuse(st, i, rec_size_finish(in, k, i, p, meta, len)); }
    }
}

__global__ __launch_bounds__(256) void k_rec_fill(rec_in in, const rec_meta *meta, const int64_t *owner, const ull *rec_off, uint64_t n_bytes, uint8_t *out)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[4][REC_TILE];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    rec_fill_tile(in, meta, owner, rec_off, n_bytes, (uint64_t)blockIdx.x * 4 + wave, tile[wave], out, (int)lane, 64);
}

// ------------------------------------------------------------------ host
// a margin of 1/4 + 256 bytes on every growth: kept as found.  The two pinned words are as large as what they hold
typedef SlxDevBuf<SlxMargin<4, 256>> RDBuf;
typedef SlxPinBuf<SlxExact> RHBuf;

struct slx_rec : SlxGpu<3> {
    slx_aligner *al = nullptr;
    RDBuf d_owner{*this}, d_meta{*this}, d_len{*this}, d_off{*this}, d_wide{*this}, d_state{*this}, d_tmp{*this}, d_stream{*this};
    RDBuf u_bases{*this}, u_offs{*this}, u_names{*this}, u_name_offs{*this};      // slx_rec_upload's copies
    RHBuf h_state{*this};               // two rec_state: [0] goes up, [1] comes down
    RHBuf h_total{*this};               // one ull
    const void *last_stream = nullptr;  // of the batch handed out last
    int64_t last_records = 0, last_bytes = 0;
    int64_t c_records = 0, c_bytes = 0, c_batches = 0, c_wide = 0;
    double us_size = 0, us_fill = 0;
};

extern "C" void slx_rec_free(slx_rec *rb)
{
    if (!rb) return;
    rb->close();
    delete rb;
}

static const char REC_NO_DEVICE[] = "no HIP device: BAM records are built on MI355X only (no CPU fallback)";

static int rec_init(slx_rec *rb, slx_aligner *al)
{
    const int device = slx_aligner_device_of(al);
    if (device < 0) { slx_set_error("slx_rec_create: single-device aligners only (the hits of a multi-device aligner are merged on the host)"); return SLX_EINVAL; }
    rb->al = al;
    SLX_CHK(rb->open(device, "slx_rec_create", REC_NO_DEVICE));
    SLX_CHK(rb->h_state.ensure(2 * sizeof(rec_state))); SLX_CHK(rb->h_total.ensure(sizeof(ull)));
    return SLX_OK;
}

extern "C" int slx_rec_create(slx_aligner *al, slx_rec **out)
{
    if (!out) { slx_set_error("slx_rec_create: null argument"); return SLX_EINVAL; }
    *out = nullptr;
    int ndev = 0;          // (before the aligner is looked at: without a GPU there is none to give)
    SLX_CHK(slx_count_devices(REC_NO_DEVICE, &ndev));
    if (!al) { slx_set_error("slx_rec_create: null aligner"); return SLX_EINVAL; }
    return slx_create(out, slx_rec_free, [&](slx_rec *rb) { return rec_init(rb, al); });
}

static int rec_build_impl(slx_rec *rb, const slx_hits *dev, rec_in in, slx_rec_batch *out)
{
    memset(out, 0, sizeof *out);
    rb->last_stream = nullptr; rb->last_records = rb->last_bytes = 0;
    const int pre = rec_check_result(dev->on_device, dev->xa_parent);
    if (pre == REC_E_HOST) { slx_set_error("slx_rec_build: the result is host-resident; records are built from a result of slx_align_batch_device"); return rec_slx_code(pre); }
    if (pre == REC_E_REG2SAM) { slx_set_error("slx_rec_build: a SLX_F_REG2SAM result (UseBwaMemRecords): its XA / SA / MD strings are built on the host"); return rec_slx_code(pre); }
    if (dev->n_reads < 0 || dev->n_hits < 0 || dev->n_hits > 0xffffffffll) { slx_set_error("slx_rec_build: %lld reads, %lld hits", (long long)dev->n_reads, (long long)dev->n_hits); return SLX_EINVAL; }
    SLX_HIPCHK(hipSetDevice(rb->device));
    const int64_t N = dev->n_reads, H = dev->n_hits;
    SLX_CHK(rb->d_off.ensure(8 * ((size_t)H + 1)));
    if (H == 0) {          // reads without hits produce nothing
        SLX_HIPCHK(hipMemsetAsync(rb->d_off.p, 0, 8, rb->st));
        SLX_HIPCHK(slx_wait_stream(rb->st));
        out->d_rec_off = rb->d_off.p; out->d_stream = rb->d_off.p;
        rb->last_stream = out->d_stream;
        ++rb->c_batches;
        return SLX_OK;
    }
    in.n_reads = N; in.n_hits = H;
    in.hit_off = dev->hit_off; in.rid = dev->rid; in.pos = dev->pos; in.flag = dev->flag; in.mapq = dev->mapq; in.score = dev->score; in.nm = dev->nm; in.na = dev->na;
    in.n_cigar_ops = dev->n_cigar_ops; in.cig_off = dev->cig_off; in.cigar = dev->cigar;
    hipStream_t st = rb->st;
    SLX_CHK(rb->d_owner.ensure(8 * (size_t)H)); SLX_CHK(rb->d_meta.ensure(sizeof(rec_meta) * (size_t)H)); SLX_CHK(rb->d_len.ensure(8 * ((size_t)H + 1)));
    SLX_CHK(rb->d_wide.ensure(4 * (size_t)H)); SLX_CHK(rb->d_state.ensure(sizeof(rec_state)));
    rec_state *const h_state = rb->h_state.as<rec_state>();
    h_state[0].refusal = REC_NO_REFUSAL; h_state[0].n_wide = 0; h_state[0].pad = 0;
    SLX_HIPCHK(hipMemcpyAsync(rb->d_state.p, &h_state[0], sizeof(rec_state), hipMemcpyHostToDevice, st));
    SLX_HIPCHK(hipEventRecord(rb->ev[0], st));
    k_rec_owner<<<(unsigned)((N + 255) / 256), 256, 0, st>>>(in.hit_off, N, H, rb->d_owner.as<int64_t>());
    SLX_HIPCHK(hipGetLastError());
    k_rec_size<<<(unsigned)((H + 255) / 256), 256, 0, st>>>(in, rb->d_owner.as<int64_t>(), rb->d_meta.as<rec_meta>(), rb->d_len.as<ull>(), rb->d_wide.as<uint32_t>(), rb->d_state.as<rec_state>());
    SLX_HIPCHK(hipGetLastError());
    k_rec_size_wide<<<(unsigned)std::min<int64_t>((H + 3) / 4, 2048), 256, 0, st>>>(in, rb->d_owner.as<int64_t>(), rb->d_meta.as<rec_meta>(), rb->d_len.as<ull>(), rb->d_wide.as<uint32_t>(),
                                                                                   rb->d_state.as<rec_state>());
    SLX_HIPCHK(hipGetLastError());
    SLX_CHK(slx_exclusive_sum(rb->d_tmp, rb->d_len.as<ull>(), rb->d_off.as<ull>(), (size_t)H + 1, st, 8));
    SLX_HIPCHK(hipEventRecord(rb->ev[1], st));
    SLX_HIPCHK(hipMemcpyAsync(rb->h_total.p, rb->d_off.as<ull>() + H, sizeof(ull), hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(hipMemcpyAsync(&h_state[1], rb->d_state.p, sizeof(rec_state), hipMemcpyDeviceToHost, st));
    SLX_HIPCHK(slx_wait_stream(st));
    rb->us_size += slx_ev_us(rb->ev[0], rb->ev[1]);
    const rec_state got = h_state[1];
    if (got.refusal != REC_NO_REFUSAL) {
        const long long read = (long long)(got.refusal >> 8);
        const int code = (int)(got.refusal & 0xff);
        if (code == REC_E_NAME) slx_set_error("slx_rec_build: read %lld of the batch has a name longer than %d bytes (a BAM record cannot hold it); nothing of the batch was built", read, REC_MAX_NAME);
        else if (code == REC_E_NCIGAR) slx_set_error("slx_rec_build: read %lld of the batch has a hit with more than %d CIGAR operations (a BAM record cannot hold them); nothing of the batch was built", read, REC_MAX_NCIGAR);
        else slx_set_error("slx_rec_build: read %lld of the batch has a hit whose hard-clip window is empty or passes the read (was the alignment made with the same hardclip?); nothing of the batch was built", read);
        return rec_slx_code(code);
    }
    const ull total = *rb->h_total.as<ull>();
    if (total < 58ull * (ull)H) { slx_set_error("slx_rec_build: internal: %llu bytes for %lld records", total, (long long)H); return SLX_EINTERNAL; }
    SLX_CHK(rb->d_stream.ensure((size_t)total + 16));
    const ull n_tiles = (total + REC_TILE - 1) / REC_TILE;
    k_rec_fill<<<(unsigned)((n_tiles + 3) / 4), 256, 0, st>>>(in, rb->d_meta.as<rec_meta>(), rb->d_owner.as<int64_t>(), rb->d_off.as<ull>(), total, rb->d_stream.as<uint8_t>());
    SLX_HIPCHK(hipGetLastError());
    SLX_HIPCHK(hipEventRecord(rb->ev[2], st));
    SLX_HIPCHK(slx_wait_stream(st));
    rb->us_fill += slx_ev_us(rb->ev[1], rb->ev[2]);
    out->n_records = H; out->n_bytes = (int64_t)total; out->d_stream = rb->d_stream.p; out->d_rec_off = rb->d_off.p;
    rb->last_stream = out->d_stream; rb->last_records = H; rb->last_bytes = (int64_t)total;
    rb->c_records += H; rb->c_bytes += (int64_t)total; ++rb->c_batches; rb->c_wide += got.n_wide;
    return SLX_OK;
}

extern "C" int slx_rec_build(slx_rec *rb, const slx_hits *dev, const void *d_bases, const void *d_offs, const void *d_names, const void *d_name_offs, int hardclip, slx_rec_batch *out)
{
    if (!rb || !dev || !out) { slx_set_error("slx_rec_build: null argument"); return SLX_EINVAL; }
    if (dev->on_device && dev->n_hits > 0 && (!d_bases || !d_offs || !d_names || !d_name_offs)) { slx_set_error("slx_rec_build: null reads or names"); return SLX_EINVAL; }
    rec_in in;
    memset(&in, 0, sizeof in);
    in.bases = (const uint8_t *)d_bases; in.offs = (const uint64_t *)d_offs; in.names = (const uint8_t *)d_names; in.name_offs = (const uint64_t *)d_name_offs;
    in.hardclip = hardclip ? 1 : 0;
    return rec_build_impl(rb, dev, in, out);
}

extern "C" int slx_rec_build_from_bam(slx_rec *rb, const slx_hits *dev, slx_bam *rd, const slx_bam_batch *batch, int hardclip, slx_rec_batch *out)
{
    if (!rb || !dev || !rd || !batch || !out) { slx_set_error("slx_rec_build_from_bam: null argument"); return SLX_EINVAL; }
    rec_in in;
    memset(&in, 0, sizeof in);
    const void *d_bases = nullptr, *d_offs = nullptr;
    const int64_t *d_map = nullptr;
    int64_t n = 0;
    int device = -1;
    if (!slx_reader_device_reads(rd, batch->d_stream, &d_bases, &d_offs, &d_map, &n, &device)) {
        slx_set_error("slx_rec_build_from_bam: the batch is not the one slx_bam_reads_device last unpacked on this reader");
        return SLX_EINVAL;
    }
    if (device != rb->device) { slx_set_error("slx_rec_build_from_bam: the reader is on device %d, the aligner on device %d", device, rb->device); return SLX_EINVAL; }
    if (n != dev->n_reads) { slx_set_error("slx_rec_build_from_bam: the result holds %lld reads, the reader unpacked %lld", (long long)dev->n_reads, (long long)n); return SLX_EINVAL; }
    in.bases = (const uint8_t *)d_bases; in.offs = (const uint64_t *)d_offs;
    in.bam_stream = (const uint8_t *)batch->d_stream; in.bam_rec_off = (const uint64_t *)batch->d_rec_off; in.rec_of_read = d_map;
    in.hardclip = hardclip ? 1 : 0;
    return rec_build_impl(rb, dev, in, out);
}

extern "C" int slx_rec_upload(slx_rec *rb, const void *bases, const uint64_t *offs, const void *names, const uint64_t *name_offs, int64_t n_reads,
                              void **d_bases, void **d_offs, void **d_names, void **d_name_offs)
{
    if (!rb || !offs || !name_offs || n_reads < 0 || !d_bases || !d_offs || !d_names || !d_name_offs) { slx_set_error("slx_rec_upload: null argument"); return SLX_EINVAL; }
    const uint64_t nb = offs[n_reads] - offs[0], nn = name_offs[n_reads] - name_offs[0];
    if (offs[0] != 0 || name_offs[0] != 0 || (nb && !bases) || (nn && !names)) { slx_set_error("slx_rec_upload: offsets start at 0 and the arrays they index are given"); return SLX_EINVAL; }
    SLX_HIPCHK(hipSetDevice(rb->device));
    SLX_CHK(rb->u_bases.ensure(nb + 16)); SLX_CHK(rb->u_names.ensure(nn + 16)); SLX_CHK(rb->u_offs.ensure(8 * ((size_t)n_reads + 1))); SLX_CHK(rb->u_name_offs.ensure(8 * ((size_t)n_reads + 1)));
    if (nb) SLX_HIPCHK(hipMemcpyAsync(rb->u_bases.p, bases, nb, hipMemcpyHostToDevice, rb->st));
    if (nn) SLX_HIPCHK(hipMemcpyAsync(rb->u_names.p, names, nn, hipMemcpyHostToDevice, rb->st));
    SLX_HIPCHK(hipMemcpyAsync(rb->u_offs.p, offs, 8 * ((size_t)n_reads + 1), hipMemcpyHostToDevice, rb->st));
    SLX_HIPCHK(hipMemcpyAsync(rb->u_name_offs.p, name_offs, 8 * ((size_t)n_reads + 1), hipMemcpyHostToDevice, rb->st));
    SLX_HIPCHK(slx_wait_stream(rb->st));
    *d_bases = rb->u_bases.p; *d_offs = rb->u_offs.p; *d_names = rb->u_names.p; *d_name_offs = rb->u_name_offs.p;
    return SLX_OK;
}

extern "C" int slx_rec_to_host(slx_rec *rb, const slx_rec_batch *b, void *dst, uint64_t cap, uint64_t *rec_off_dst)
{
    if (!rb || !b) { slx_set_error("slx_rec_to_host: null argument"); return SLX_EINVAL; }
    if (!rb->last_stream || b->d_stream != rb->last_stream || b->n_records != rb->last_records || b->n_bytes != rb->last_bytes) { slx_set_error("slx_rec_to_host: not the builder's last batch"); return SLX_EINVAL; }
    if ((uint64_t)b->n_bytes > cap || (b->n_bytes && !dst)) { slx_set_error("slx_rec_to_host: %lld bytes do not fit the %llu given", (long long)b->n_bytes, (unsigned long long)cap); return SLX_EINVAL; }
    SLX_HIPCHK(hipSetDevice(rb->device));
    if (b->n_bytes) SLX_HIPCHK(hipMemcpyAsync(dst, b->d_stream, (size_t)b->n_bytes, hipMemcpyDeviceToHost, rb->st));
    if (rec_off_dst) SLX_HIPCHK(hipMemcpyAsync(rec_off_dst, b->d_rec_off, 8 * ((size_t)b->n_records + 1), hipMemcpyDeviceToHost, rb->st));
    SLX_HIPCHK(hipStreamSynchronize(rb->st));
    return SLX_OK;
}

extern "C" int64_t slx_rec_counter(const slx_rec *rb, const char *name)
{
    if (!rb || !name) return -1;
    if (!strcmp(name, "records")) return rb->c_records;
    if (!strcmp(name, "bytes")) return rb->c_bytes;
    if (!strcmp(name, "batches")) return rb->c_batches;
    if (!strcmp(name, "wide_hits")) return rb->c_wide;
    if (!strcmp(name, "us_size")) return (int64_t)rb->us_size;
    if (!strcmp(name, "us_fill")) return (int64_t)rb->us_fill;
    return -1;
}
