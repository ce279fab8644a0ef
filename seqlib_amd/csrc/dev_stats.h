// dev_stats.h -- the per-record bodies and the kernels of the read statistics (include/seqlib_amd_stats.h has the rules; slx_stats.hip launches the kernels,
// slx_stats_record runs the body on the host).  Host-compilable like dev_rfilter.h and cov_host.h (`lane` of `nlanes`; the host build runs lane 0 of 1), so
// tests/cpp/stats_host_test.cpp holds every body against the Python statement of the rules under ASan + UBSan before it runs on a GPU.
//
// One record, three steps:
//   head     rf_fixed (dev_rfilter.h): the fixed fields, checked against block_size and the span of the offset table.
//   part     what lanes can share: the CIGAR ops (rf_cigar_part: NumClip) and the QUAL bytes (st_qual_part: aligned words through the sum of absolute
//            differences against 0, four bytes an instruction; the ragged ends byte by byte by lane 0).  Parts are summed (st_part_join).
//   finish   the aux walk (rf_aux: the first NM of an integer type, the first RG), the group key, the six values.
// A group key is never materialised on the device: it is `pre` * "QNAMED_" followed by bytes of the record (or "NA"), read through st_key_byte.
// Counts live in one uint64 array of rows, ST_REPLICAS copies of a row per group (st_lay): 14 counters, then per histogram `below`, `above` and its bins.
// Memory safety is the read filter's: nothing outside [h, h + span) is read; the QUAL lies inside block_size because rf_fixed said so.
#pragma once
#include <stdint.h>
#include <string.h>
#include "dev_rfilter.h"

enum { ST_H_MAPQ = 0, ST_H_NM, ST_H_ISIZE, ST_H_CLIP, ST_H_PHRED, ST_H_LEN, ST_N_HIST };
enum { ST_C_READS = 0, ST_C_SUPP, ST_C_QCFAIL, ST_C_DUP, ST_C_UNMAP, ST_C_MATE_UNMAP, ST_C_SUPPLEMENTARY, ST_C_PAIRED, ST_C_PROPER, ST_C_READ1, ST_C_READ2, ST_C_REVERSE,
       ST_C_BASES, ST_C_NM_MISSING, ST_C_N };
#define ST_MAX_KEY 255u
#define ST_E_KEY 4u             // a group key longer than ST_MAX_KEY (beside RF_E_FIELDS and RF_E_AUX)
#define ST_NO_GROUP 0xffffffffu
#define ST_OVERHANG 2048u       // bytes staged behind a window, as k_flt_eval's default
#define ST_REPLICAS 8u          // copies of every row in HBM: block b adds to copy b % 8, the host sums them (the flushes of all blocks otherwise meet on a few cache lines)

// Histogram(start, end, width) of the reference (src/non_api/Histogram.cpp:14-48): nfull = (end - start) / width bins of `width`, then one up to `end`
struct st_lay { int32_t start[ST_N_HIST], end[ST_N_HIST], width[ST_N_HIST]; uint32_t nb[ST_N_HIST], base[ST_N_HIST]; uint32_t row, pad; };
struct st_par { uint32_t exclude_flags; int32_t min_mapq; uint32_t long_record, pad; };
// the group table: open addressing, slots[i] = group + 1 or 0; group g's key is pool[koff[g], koff[g + 1])
struct st_tab { const uint32_t *slots, *koff; const uint8_t *pool; uint32_t mask, pad; };

struct st_part { uint64_t qsum; uint32_t clip, pad; };
struct st_rec {
    int64_t v[ST_N_HIST];
    const uint8_t *key;          // the key's bytes behind the prefix; not read when key_na
    uint32_t key_len, key_pre, key_na, flag, has_nm, pad;          // key_len: the whole key, prefix included
};

RF_HD void st_layout(st_lay *L)
{
    uint32_t at = ST_C_N;
    for (int h = 0; h < ST_N_HIST; ++h) {
        L->nb[h] = (uint32_t)(((int64_t)L->end[h] - L->start[h]) / L->width[h]) + 1u;
        L->base[h] = at;
        at += 2u + L->nb[h];
    }
    L->row = at; L->pad = 0;
}
RF_HD void st_layout_default(st_lay *L, int32_t len_max, int32_t isize_max)
{
    const int32_t s[ST_N_HIST] = {0, 0, -2, 0, 0, 0}, e[ST_N_HIST] = {100, 100, isize_max, 100, 100, len_max}, w[ST_N_HIST] = {1, 1, 10, 5, 1, 1};
    for (int h = 0; h < ST_N_HIST; ++h) { L->start[h] = s[h]; L->end[h] = e[h]; L->width[h] = w[h]; }
    st_layout(L);
}
// bounds of bin k
RF_HD int32_t st_bin_lo(const st_lay *L, int h, uint32_t k) { return L->start[h] + (int32_t)k * L->width[h]; }
RF_HD int32_t st_bin_hi(const st_lay *L, int h, uint32_t k) { return k + 1 == L->nb[h] ? L->end[h] : L->start[h] + (int32_t)(k + 1) * L->width[h] - 1; }
// the entry of a row that value v of histogram h adds to: below, above, or its bin (v <= end gives (v - start) / width <= nfull, the last bin)
RF_HD uint32_t st_slot(const st_lay *L, int h, int64_t v)
{
    if (v < L->start[h]) return L->base[h];
    if (v > L->end[h]) return L->base[h] + 1u;
    return L->base[h] + 2u + (uint32_t)((v - L->start[h]) / L->width[h]);
}

// ---------------------------------------------------------------- the QUAL sum
#if defined(__HIP_DEVICE_COMPILE__)
#define ST_LD32(p) (*reinterpret_cast<const uint32_t *>(p))
#define ST_SAD(w, acc) __builtin_amdgcn_sad_u8((w), 0u, (acc))
#else
RF_HD uint32_t st_ld32(const uint8_t *p) { uint32_t w; memcpy(&w, p, 4); return w; }
#define ST_LD32(p) st_ld32(p)
#define ST_SAD(w, acc) ((acc) + ((w) & 255u) + (((w) >> 8) & 255u) + (((w) >> 16) & 255u) + ((w) >> 24))
#endif
// lane's share of the sum of q[0, n): the aligned words lane, lane + nlanes, ...; lane 0 also takes the up to 3 bytes before the first and after the last word
RF_HD uint64_t st_qual_part(const uint8_t *q, uint64_t n, uint32_t lane, uint32_t nlanes)
{
    uint64_t head = (4u - (uint32_t)((uintptr_t)q & 3u)) & 3u;
    if (head > n) head = n;
    const uint64_t nw = (n - head) >> 2, tail0 = head + (nw << 2);
    uint64_t s = 0;
    if (lane == 0) {
        for (uint64_t i = 0; i < head; ++i) s += q[i];
        for (uint64_t i = tail0; i < n; ++i) s += q[i];
    }
    const uint8_t *w = q + head;
    for (uint64_t i = lane; i < nw;) {
        uint32_t acc = 0;          // 65536 words of at most 1020 each
        for (uint32_t k = 0; k < 65536u && i < nw; ++k, i += nlanes) acc = ST_SAD(ST_LD32(w + 4 * i), acc);
        s += acc;
    }
    return s;
}

// ---------------------------------------------------------------- one record
RF_HD void st_part_of(const rf_feat *F, uint32_t lane, uint32_t nlanes, st_part *P)
{
    rf_part c;
    memset(&c, 0, sizeof c);
    rf_cigar_part(F->cig, lane, F->n_cig, nlanes, &c);
    const uint64_t ls = (uint64_t)F->l_seq;
    P->clip = c.clip; P->pad = 0;
    P->qsum = st_qual_part(F->seq + ((ls + 1) >> 1), ls, lane, nlanes);
}
RF_HD void st_part_join(st_part *a, const st_part *b) { a->qsum += b->qsum; a->clip += b->clip; }

// byte i of the key: "QNAMED_" is 0x5f44454d414e51 and "NA" 0x414e, little end first
RF_HD uint8_t st_key_byte(const st_rec *R, uint32_t i)
{
    if (R->key_pre) { if (i < 7u) return (uint8_t)(0x5f44454d414e51ull >> (8u * i)); i -= 7u; }
    return R->key_na ? (uint8_t)(0x414eu >> (8u * i)) : R->key[i];
}
#define ST_HASH_INIT 2166136261u
RF_HD uint32_t st_hash_step(uint32_t h, uint8_t c) { return (h ^ c) * 16777619u; }          // FNV-1a
RF_HD uint32_t st_hash(const st_rec *R)
{
    uint32_t h = ST_HASH_INIT;
    for (uint32_t i = 0; i < R->key_len; ++i) h = st_hash_step(h, st_key_byte(R, i));
    return h;
}
RF_HD uint32_t st_hash_bytes(const uint8_t *p, uint32_t n)
{
    uint32_t h = ST_HASH_INIT;
    for (uint32_t i = 0; i < n; ++i) h = st_hash_step(h, p[i]);
    return h;
}

// the group key of a record whose aux fields were walked: RG:Z when the first RG has that type and is not empty (src/non_api/BamStats.cpp:89-92), else
// "QNAMED_" + ParseReadGroup's name rule.  0 or ST_E_KEY.
RF_HD uint32_t st_key(rf_feat *F, st_rec *R)
{
    if (F->rg && F->rg_len) { R->key = F->rg; R->key_len = F->rg_len; R->key_pre = 0; R->key_na = 0; }
    else {
        F->rg = nullptr;
        rf_rg_from_name(F);
        R->key = F->rg; R->key_len = 7u + F->rg_len; R->key_pre = 1; R->key_na = F->rg_na;
    }
    return R->key_len > ST_MAX_KEY ? ST_E_KEY : 0u;
}

// the end of a record, one lane: the joined parts, the aux walk, the key and the six values (BamReadGroup::addRead, src/non_api/BamStats.cpp:45-84)
RF_HD uint32_t st_finish(const uint8_t *h, rf_feat *F, const st_part *P, st_rec *R)
{
    const uint32_t er = rf_aux(F->aux, F->aux_len, F);
    if (er) return er;
    R->flag = F->flag; R->has_nm = F->has_nm; R->pad = 0;
    R->v[ST_H_MAPQ] = (int64_t)F->mapq;
    R->v[ST_H_NM] = F->has_nm ? (int64_t)F->nm : 0;
    const int64_t isz = (int64_t)(int32_t)rf_u32(h + 32);
    R->v[ST_H_ISIZE] = !rf_pair_mapped(F->flag) ? -2 : F->tid != F->mtid ? -1 : (isz < 0 ? -isz : isz);
    R->v[ST_H_CLIP] = (int64_t)P->clip;
    R->v[ST_H_LEN] = (int64_t)F->l_seq;
    R->v[ST_H_PHRED] = F->l_seq <= 0 ? -1 : (int64_t)(P->qsum / (uint64_t)F->l_seq);
    return st_key(F, R);
}

// what one lane does alone for a record (the short path, and the host).  0 or error bits; R is whole when 0 and points into the record.
RF_HD uint32_t st_record(const uint8_t *h, uint64_t span, rf_feat *F, st_rec *R)
{
    if (!rf_fixed(h, span, F)) return RF_E_FIELDS;
    st_part P;
    st_part_of(F, 0, 1, &P);
    return st_finish(h, F, &P, R);
}
RF_HD bool st_eligible(const st_par *P, const rf_feat *F) { return !(F->flag & P->exclude_flags) && (int32_t)F->mapq >= P->min_mapq; }

// the group of a record, or ST_NO_GROUP
RF_HD uint32_t st_lookup(const st_tab *T, const st_rec *R)
{
    uint32_t i = st_hash(R) & T->mask;
    for (uint32_t v; (v = T->slots[i]) != 0; i = (i + 1) & T->mask) {
        const uint32_t g = v - 1, o = T->koff[g];
        if (T->koff[g + 1] - o != R->key_len) continue;
        uint32_t k = 0;
        while (k < R->key_len && T->pool[o + k] == st_key_byte(R, k)) ++k;
        if (k == R->key_len) return g;
    }
    return ST_NO_GROUP;
}

// the adds of one record to its row through S.add(entry, amount, on).  On the GPU all lanes of a wave call this together (on: this lane has a record).
template <class Sink> RF_HD void st_adds(const st_lay *L, const st_rec *R, bool on, Sink &S)
{
    const uint32_t fl = R->flag;
    S.add(ST_C_READS, 1u, on);
    S.add(ST_C_SUPP, 1u, on && (fl & 0x100u));          // SecondaryFlag under that name: the reference's, kept
    S.add(ST_C_QCFAIL, 1u, on && (fl & 0x200u));
    S.add(ST_C_DUP, 1u, on && (fl & 0x400u));
    S.add(ST_C_UNMAP, 1u, on && (fl & 0x4u));
    S.add(ST_C_MATE_UNMAP, 1u, on && (fl & 0x8u));
    S.add(ST_C_SUPPLEMENTARY, 1u, on && (fl & 0x800u));
    S.add(ST_C_PAIRED, 1u, on && (fl & 0x1u));
    S.add(ST_C_PROPER, 1u, on && (fl & 0x2u));
    S.add(ST_C_READ1, 1u, on && (fl & 0x40u));
    S.add(ST_C_READ2, 1u, on && (fl & 0x80u));
    S.add(ST_C_REVERSE, 1u, on && (fl & 0x10u));
    S.add(ST_C_BASES, (uint32_t)R->v[ST_H_LEN], on && R->v[ST_H_LEN] > 0);
    S.add(ST_C_NM_MISSING, 1u, on && !R->has_nm);
    for (int h = 0; h < ST_N_HIST; ++h) S.add(st_slot(L, h, R->v[h]), 1u, on && (h != ST_H_NM || R->has_nm));
}

// ---------------------------------------------------------------- the kernels
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "dev_lanes.h"
// (no work is TAKEN from a device counter here -- blocks own windows, waves stride the long list -- so dev_wave.h is not needed: the appends to the long and the
// miss list use the counter's old value in the lane that added, and nowhere else)

typedef unsigned long long st_ull;
// device counters of one add: the lowest record with broken fields or aux, the lowest with too long a key, list lengths, and what was done
enum { ST_K_ERR_IO = 0, ST_K_ERR_KEY, ST_K_NLONG, ST_K_NMISS, ST_K_COUNTED, ST_K_LDS, ST_K_GLOBAL, ST_K_N };

// The adds of a wave's 64 records.  Where every lane that adds goes to the same entry of the same group (one read group, MAPQ 60, NM 0: the common case) one
// lane adds the wave's total; otherwise every lane adds its own.  Groups below lds_groups have their row in LDS (uint32: a block's records are bounded by its
// stage), the others go to HBM.  Every lane of the wave calls add().
struct st_sink {
    uint32_t *lds; st_ull *glob;          // glob: this block's copy of the rows (group g at g * ST_REPLICAS * row)
    uint32_t row, lds_groups, g, n_lds, n_glob;
    __device__ __forceinline__ void put(uint32_t entry, uint32_t amount)
    {
        if (g < lds_groups) { atomicAdd(&lds[g * row + entry], amount); ++n_lds; }
        else { atomicAdd(&glob[(uint64_t)g * ST_REPLICAS * row + entry], (st_ull)amount); ++n_glob; }
    }
    __device__ __forceinline__ void add(uint32_t entry, uint32_t amount, bool on)
    {
        const st_ull m = __ballot(on);
        if (!m) return;
        const int leader = __ffsll((long long)m) - 1;          // (the same in every lane: readlane, not a trip through LDS)
        const uint32_t lg = (uint32_t)__builtin_amdgcn_readlane((int)g, leader), le = (uint32_t)__builtin_amdgcn_readlane((int)entry, leader);
        if (__ballot(on && (g != lg || entry != le)) == 0) {
            const bool ones = __ballot(on && amount != 1u) == 0;          // (the same in every lane)
            const uint32_t total = ones ? (uint32_t)__popcll(m) : (uint32_t)wave_sum((st_ull)(on ? amount : 0u));
            if ((int)(threadIdx.x & 63) == leader) put(entry, total);
        } else if (on) put(entry, amount);
    }
};
// one lane, HBM only (the wave's records)
struct st_sink_one {
    st_ull *glob; uint64_t base; uint32_t n_glob;
    __device__ __forceinline__ void add(uint32_t entry, uint32_t amount, bool on) { if (on) { atomicAdd(&glob[base + entry], (st_ull)amount); ++n_glob; } }
};

typedef uint32_t st_v4 __attribute__((ext_vector_type(4)));

// The windows of the stream, a lane per record: record r is the first of window off[r] / W when the record before it starts in an earlier window, and the last
// when the one behind it starts in a later one (wfirst / wend, preset to ST_NO_GROUP: a window no record starts in keeps that).  One pass over the offsets in
// place of two binary searches per block, whose 2 x 21 dependent loads out of a 16 MB table were 30 us of every block's life.  Offsets that do not rise, or
// pass the stream, fail the call here, whatever window they would fall in.
__global__ __launch_bounds__(256) void k_st_windows(const st_ull *rec_off, uint64_t n_rec, uint64_t n_bytes, uint32_t W, uint64_t n_win, uint32_t *wfirst, uint32_t *wend, st_ull *cnt)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rec) return;
    const uint64_t a = rec_off[r], b = rec_off[r + 1];
    if (b <= a || b > n_bytes || b - a < 36) { atomicMin(&cnt[ST_K_ERR_IO], (st_ull)r); return; }
    const uint64_t w = a / W;          // (a < n_bytes: below n_win)
    if (r == 0 || rec_off[r - 1] / W != w) wfirst[w] = (uint32_t)r;
    if (r + 1 == n_rec || b / W != w) wend[w] = (uint32_t)(r + 1);
}

// Window blockIdx.x of the stream: the records that START in [win * W, win * W + W) are this block's (wfirst, wend of k_st_windows).  The window and ST_OVERHANG
// bytes behind it, cut to the stream, are staged in LDS at the source's own alignment -- whole aligned 16-byte words as words, the up to 15 bytes on either
// side byte by byte -- so nothing outside the stream is loaded and a QUAL's word alignment is the same in LDS as in HBM.  Then a lane per record out of LDS,
// 256 records a round, all lanes of a wave in step (st_sink needs them together).  A record that ends behind the stage or is larger than P.long_record goes
// to long_list; one whose key is not in the table sets miss[r] and goes to miss_list.  only != nullptr: records with only[r] == 0 are passed over.
// Dynamic LDS: W + ST_OVERHANG + 16 bytes of stage, then lds_groups * L.row uint32.
__global__ __launch_bounds__(256) void k_st_add(const uint8_t *s, uint64_t n_bytes, const st_ull *rec_off, uint64_t n_rec, uint32_t W, const uint32_t *wfirst, const uint32_t *wend, st_par P,
                                                st_lay L, st_tab T, st_ull *glob, uint32_t lds_groups, const uint8_t *only, uint8_t *miss, uint32_t *miss_list, uint32_t *long_list, st_ull *cnt)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t st_lds[];
    const uint32_t tid = threadIdx.x, nthreads = blockDim.x, V = ST_OVERHANG;
    const uint64_t w0 = (uint64_t)blockIdx.x * W;
    if (w0 >= n_bytes || n_rec == 0) return;
    const uint64_t w1 = w0 + W < n_bytes ? w0 + W : n_bytes, e = w1 + V < n_bytes ? w1 + V : n_bytes;
    const uint64_t first = wfirst[blockIdx.x], last = wend[blockIdx.x];
    if (first == ST_NO_GROUP || last == ST_NO_GROUP || first >= last || last > n_rec) return;          // (the whole block leaves; no record starts here)
    uint32_t *hist = reinterpret_cast<uint32_t *>(st_lds + W + V + 16u);
    const uint32_t n_hist = lds_groups * L.row;
    for (uint32_t i = tid; i < n_hist; i += nthreads) hist[i] = 0;
    const uint8_t *g = s + w0;
    const uint32_t len = (uint32_t)(e - w0), lead = (uint32_t)((uintptr_t)g & 15u);
    uint32_t head = (16u - lead) & 15u;
    if (head > len) head = len;
    const uint32_t nw = (len - head) >> 4, tail0 = head + (nw << 4);
    for (uint32_t i = tid; i < head; i += nthreads) st_lds[lead + i] = g[i];
    for (uint32_t i = tid; i < nw; i += nthreads) {
        const uint32_t o = head + (i << 4);
        *reinterpret_cast<st_v4 *>(st_lds + lead + o) = *reinterpret_cast<const st_v4 *>(g + o);
    }
    for (uint32_t i = tail0 + tid; i < len; i += nthreads) st_lds[lead + i] = g[i];
    __syncthreads();
    st_ull *mine = glob + (uint64_t)(blockIdx.x % ST_REPLICAS) * L.row;
    st_sink S = {hist, mine, L.row, lds_groups, 0u, 0u, 0u};
    uint32_t counted = 0;
    for (uint64_t r0 = first; r0 < last; r0 += nthreads) {          // (uniform over the block)
        const uint64_t r = r0 + tid;
        bool on = false;
        st_rec R;
        memset(&R, 0, sizeof R);
        S.g = 0;
        if (r < last && (!only || only[r])) {
            const uint64_t a = rec_off[r], b = rec_off[r + 1];
            if (a < w0 || a >= w1 || b <= a || b > n_bytes || b - a < 36) atomicMin(&cnt[ST_K_ERR_IO], (st_ull)r);
            else if (b > e || b - a > P.long_record) long_list[atomicAdd(&cnt[ST_K_NLONG], 1ull)] = (uint32_t)r;
            else {
                const uint8_t *h = st_lds + lead + (uint32_t)(a - w0);
                rf_feat F;
                if (!rf_fixed(h, b - a, &F)) atomicMin(&cnt[ST_K_ERR_IO], (st_ull)r);
                else if (st_eligible(&P, &F)) {
                    st_part Q;
                    st_part_of(&F, 0, 1, &Q);
                    const uint32_t er = st_finish(h, &F, &Q, &R);
                    if (er) atomicMin(&cnt[er & ST_E_KEY ? ST_K_ERR_KEY : ST_K_ERR_IO], (st_ull)r);
                    else if ((S.g = st_lookup(&T, &R)) == ST_NO_GROUP) { miss[r] = 1; miss_list[atomicAdd(&cnt[ST_K_NMISS], 1ull)] = (uint32_t)r; }
                    else on = true;
                }
            }
        }
        counted += on;
        st_adds(&L, &R, on, S);
    }
    __syncthreads();
    for (uint32_t i = tid; i < n_hist; i += nthreads) {          // coalesced: neighbouring lanes, neighbouring entries
        const uint32_t v = hist[i];
        if (v) { const uint32_t g = i / L.row; atomicAdd(&mine[(uint64_t)g * ST_REPLICAS * L.row + (i - g * L.row)], (st_ull)v); }
    }
    wave_count(&cnt[ST_K_COUNTED], counted);
    wave_count(&cnt[ST_K_LDS], S.n_lds);
    wave_count(&cnt[ST_K_GLOBAL], S.n_glob);
}

// one wave per record of long_list[0, m): the lanes share the CIGAR ops and the QUAL words out of HBM, lane 0 finishes and adds to HBM
__global__ __launch_bounds__(256) void k_st_add_long(const uint8_t *s, const st_ull *rec_off, const uint32_t *long_list, uint64_t m, st_par P, st_lay L, st_tab T, st_ull *glob,
                                                     uint8_t *miss, uint32_t *miss_list, st_ull *cnt)
{
    const uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= m) return;          // (whole waves leave)
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t r = long_list[j], a = rec_off[r], b = rec_off[r + 1];          // (k_st_add has placed [a, b) inside the stream)
    const uint8_t *h = s + a;
    rf_feat F;
    if (!rf_fixed(h, b - a, &F)) { if (lane == 0) atomicMin(&cnt[ST_K_ERR_IO], (st_ull)r); return; }          // (the same verdict in every lane)
    if (!st_eligible(&P, &F)) return;
    st_part Q;
    st_part_of(&F, lane, 64, &Q);
    Q.qsum = wave_sum((st_ull)Q.qsum); Q.clip = (uint32_t)wave_sum((st_ull)Q.clip);
    if (lane != 0) return;
    st_rec R;
    memset(&R, 0, sizeof R);
    const uint32_t er = st_finish(h, &F, &Q, &R);
    if (er) { atomicMin(&cnt[er & ST_E_KEY ? ST_K_ERR_KEY : ST_K_ERR_IO], (st_ull)r); return; }
    const uint32_t g = st_lookup(&T, &R);
    if (g == ST_NO_GROUP) { miss[r] = 1; miss_list[atomicAdd(&cnt[ST_K_NMISS], 1ull)] = (uint32_t)r; return; }
    st_sink_one S = {glob, ((uint64_t)g * ST_REPLICAS + blockIdx.x % ST_REPLICAS) * L.row, 0u};
    st_adds(&L, &R, true, S);
    atomicAdd(&cnt[ST_K_COUNTED], 1ull);
    atomicAdd(&cnt[ST_K_GLOBAL], (st_ull)S.n_glob);
}

// the keys of records list[0, m) for the host: out[j] is 4 bytes of length and ST_MAX_KEY + 1 bytes of key (the records passed k_st_add's checks)
#define ST_KEY_STRIDE (4u + ST_MAX_KEY + 1u)
__global__ __launch_bounds__(256) void k_st_keys(const uint8_t *s, const st_ull *rec_off, const uint32_t *list, uint32_t m, uint8_t *out)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint64_t r = list[j], a = rec_off[r];
    rf_feat F;
    st_rec R;
    memset(&R, 0, sizeof R);
    uint8_t *o = out + (uint64_t)j * ST_KEY_STRIDE;
    uint32_t n = 0;
    if (rf_fixed(s + a, rec_off[r + 1] - a, &F) && rf_aux(F.aux, F.aux_len, &F) == 0 && st_key(&F, &R) == 0) n = R.key_len;
    for (uint32_t i = 0; i < n; ++i) o[4 + i] = st_key_byte(&R, i);
    o[0] = (uint8_t)n; o[1] = (uint8_t)(n >> 8); o[2] = 0; o[3] = 0;
}
#endif
