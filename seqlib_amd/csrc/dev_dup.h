// dev_dup.h -- the kernels of the duplicate marker (include/seqlib_amd_dup.h; slx_dup.hip launches them, dup_host.h holds the per-record body).  DESIGN.md 9.15.
//
//   add      k_dup_sig        a lane per record: its span, its head, then dp_signature; a record with more than 64 CIGAR operations or longer than wave_len is
//                             listed instead
//            k_dup_sig_long   a wave per listed record: the CIGAR 64 operations per ballot from both ends, the qualities a word per lane and round
//            k_dup_sizes      per record: 1 and its name's length when it is paired (two exclusive sums follow)
//            k_dup_commit     a lane per record: the signature into the marker's columns, a paired record's name into the arena segment
//   finish   k_dup_init, k_dup_pkeys, radix sort, k_dup_heads + max-scan (runs of equal hash), k_dup_join (every record looks through its own run),
//            k_dup_islo + exclusive sum, k_dup_entries (one entry per pair), k_dup_iota, k_dup_take + radix sort per key word (least significant first),
//            k_dup_heads + max-scan (every element learns its group's head), k_dup_pair_verdict, k_dup_frag_verdict
//   apply    k_dup_apply      a lane per record: a byte load, or / and-not, a byte store
// Records, entries and paired records map to lanes statically: no work queue.  Counters are summed over the wave before one lane adds.
//
// Memory safety.  add: dup_host.h.  commit reads a name inside a span that k_dup_sig has validated and writes name_len bytes at the offset the exclusive sum
// gave it inside a segment sized by that sum's total.  finish: every index is an ordinal below n, a paired index below m or an entry below n_ent, all produced
// by the marker's own kernels.  apply: a record's flag bytes are touched only when off[i] - off[0] + 36 <= n_bytes and its ordinal is below n; a batch with any
// record that fails either test is refused before a byte is written (two launches: check, then write).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_lanes.h"
#include "dev_wave.h"
#include "dup_host.h"

typedef unsigned long long dp_ull;

// device counters of one call.  bad: the lowest broken record (atomicMin); the rest are sums
struct dp_state { dp_ull bad; uint32_t n_long, too_long, mixed, dup_pairs, dup_frags, n_orphans, bad_ord, n_ignored; };
struct dp_args { const uint8_t *s; uint64_t n_bytes; const uint64_t *off; uint64_t n; };
// the marker's columns: per ordinal hi, lo, score, cls; per paired record (in ordinal order) its ordinal, hash, name address and length, and after finish its mate
struct dp_cols {
    dp_ull *hi, *lo; uint32_t *score; uint8_t *cls;
    uint32_t *pord; dp_ull *phash, *pname; uint32_t *plen;
};

// ------------------------------------------------------------------ add
__global__ __launch_bounds__(256) void k_dup_sig(dp_libtab T, dp_args A, uint32_t wave_len, dp_sig *S, uint32_t *longlist, dp_state *st)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool broken = false, is_long = false;
    if (i < A.n) {
        uint32_t span = 0, seq_at = 0, aux_at = 0;
        bool own = false;
        dp_sig s = {DP_HI_IGNORED, 0, 0, DP_IGNORED, 0, 0, 0};
        if (!ed_span(A.s, A.n_bytes, A.off, i, A.n, &span, &own)) broken = true;
        else if (own) {          // (when not, record i + 1 is the one named, by its own lane)
            const uint8_t *rec = A.s + (A.off[i] - A.off[0]);
            if (!dp_head(rec, span, &seq_at, &aux_at)) broken = true;
            else if (dp_is_long(rec, wave_len)) is_long = true;
            else dp_signature<false>(T, rec, span, seq_at, aux_at, 0, 1, &s);
        }
        S[i] = s;
    }
    if (is_long) longlist[wave_fetch_inc(&st->n_long)] = (uint32_t)i;
    wave_report_min(&st->bad, broken, i);
}

// (only records whose span and head k_dup_sig has passed are listed)
__global__ __launch_bounds__(256) void k_dup_sig_long(dp_libtab T, dp_args A, const uint32_t *longlist, uint32_t n_long, dp_sig *S)
{
    const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= n_long) return;          // (a whole wave)
    const uint64_t i = longlist[w], a = A.off[i] - A.off[0];
    const uint8_t *rec = A.s + a;
    const uint32_t span = (uint32_t)(A.off[i + 1] - A.off[i]);
    uint32_t seq_at = 0, aux_at = 0;
    (void)ed_fixed(rec, span, &seq_at, &aux_at);
    dp_sig s;
    dp_signature<true>(T, rec, span, seq_at, aux_at, (int)lane, 64, &s);
    if (lane == 0) S[i] = s;
}

__global__ __launch_bounds__(256) void k_dup_sizes(const dp_sig *S, uint64_t n, dp_ull *pcnt, dp_ull *nlen, dp_state *st)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t c = i < n ? S[i].cls & DP_CLASS : 0xffu;
    if (i <= n) {
        pcnt[i] = c == DP_PAIRED ? 1 : 0;
        nlen[i] = c == DP_PAIRED ? S[i].name_len : 0;
    }
    wave_count(&st->n_ignored, c == DP_IGNORED);
}

__global__ __launch_bounds__(256) void k_dup_commit(dp_args A, const dp_sig *S, const dp_ull *poff, const dp_ull *noff, uint64_t base, uint64_t m_old, uint8_t *seg, dp_cols C)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const dp_sig s = S[i];
    const uint64_t o = base + i;
    C.hi[o] = s.hi; C.lo[o] = s.lo; C.score[o] = s.score; C.cls[o] = (uint8_t)s.cls;
    if ((s.cls & DP_CLASS) != DP_PAIRED) return;
    const uint64_t p = m_old + poff[i];
    uint8_t *dst = seg + noff[i];
    const uint8_t *src = A.s + (A.off[i] - A.off[0]) + 36;
    for (uint32_t k = 0; k < s.name_len; ++k) dst[k] = src[k];
    C.pord[p] = (uint32_t)o; C.phash[p] = s.hash; C.pname[p] = (dp_ull)(uintptr_t)dst; C.plen[p] = s.name_len;
}

// ------------------------------------------------------------------ finish
__global__ __launch_bounds__(256) void k_dup_iota(uint32_t *perm, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) perm[i] = (uint32_t)i;
}

// the verdict of every ordinal before any rule has spoken: 2 for an ignored record, 0 otherwise
__global__ __launch_bounds__(256) void k_dup_init(const uint8_t *cls, uint64_t n, uint8_t *ver, dp_ull *k0, const uint32_t *score)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = cls[i] & DP_CLASS;
    ver[i] = c == DP_IGNORED ? 2 : 0;
    // the lowest word of a record's key: paired records first, then fragments by falling score; the stable sort keeps ordinal order among equals
    k0[i] = (dp_ull)(c == DP_FRAGMENT ? 1u : 0u) << 31 | (~score[i] & 0x7fffffffu);
}

__global__ __launch_bounds__(256) void k_dup_pkeys(const dp_ull *phash, uint64_t m, dp_ull mask, dp_ull *key, uint32_t *idx)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) { key[i] = phash[i] & mask; idx[i] = (uint32_t)i; }
}

// pos[i] = i where sorted element i differs from its predecessor in any of the given words (read through perm where given), else 0: an inclusive max-scan
// then hands every element the position of its run's head
__global__ __launch_bounds__(256) void k_dup_heads(const uint32_t *perm, uint64_t n, const dp_ull *w0, const dp_ull *w1, const dp_ull *w2, const dp_ull *w3, uint32_t *pos)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool head = i == 0;
    if (!head) {
        const uint32_t a = perm ? perm[i] : (uint32_t)i, b = perm ? perm[i - 1] : (uint32_t)(i - 1);
        head = w0[a] != w0[b] || (w1 && w1[a] != w1[b]) || (w2 && w2[a] != w2[b]) || (w3 && w3[a] != w3[b]);
    }
    pos[i] = head ? (uint32_t)i : 0u;
}

__device__ __forceinline__ bool dp_same_name(const dp_cols &C, uint32_t a, uint32_t b)
{
    if (C.plen[a] != C.plen[b] || (C.hi[C.pord[a]] >> 32) != (C.hi[C.pord[b]] >> 32)) return false;
    const uint8_t *x = (const uint8_t *)(uintptr_t)C.pname[a], *y = (const uint8_t *)(uintptr_t)C.pname[b];
    for (uint32_t k = 0, n = C.plen[a]; k < n; ++k) if (x[k] != y[k]) return false;
    return true;
}

// Sorted paired record i looks through its run [start[i], the next head) for the records of its (library, name): with exactly one other, and 0x40 on one and
// 0x80 on the other, that one is its mate.  A run longer than run_max is counted and not walked.  The run's head also says whether the run holds another name.
__global__ __launch_bounds__(256) void k_dup_join(dp_cols C, const dp_ull *key, const uint32_t *idx, const uint32_t *start, uint64_t m, uint32_t run_max, uint32_t *mate, dp_state *st)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t too_long = 0, mixed = 0, orphan = 0;
    if (i < m) {
        const uint32_t me = idx[i], s = start[i];
        const dp_ull k = key[i];
        uint32_t cnt = 0, other = DP_NO_MATE;
        for (uint64_t j = s; j < m && key[j] == k; ++j) {
            if (j - s >= run_max) { too_long = 1; break; }
            const uint32_t o = idx[j];
            if (o == me) continue;
            if (dp_same_name(C, me, o)) { ++cnt; other = o; }
            else if (i == s) mixed = 1;
        }
        uint32_t res = DP_NO_MATE;
        if (cnt == 1) {
            const uint32_t a = C.cls[C.pord[me]], b = C.cls[C.pord[other]];
            if (((a & DP_FIRST) && (b & DP_SECOND)) || ((a & DP_SECOND) && (b & DP_FIRST))) res = other;
        }
        mate[me] = res;
        orphan = res == DP_NO_MATE;
    }
    wave_count(&st->too_long, too_long);
    wave_count(&st->mixed, mixed);
    wave_count(&st->n_orphans, orphan);
}

// a pair is entered by its member of the lower ordinal (paired indices rise with the ordinal)
__global__ __launch_bounds__(256) void k_dup_islo(const uint32_t *mate, uint64_t m, dp_ull *islo)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p <= m) islo[p] = p < m && mate[p] != DP_NO_MATE && p < mate[p] ? 1 : 0;
}

// entry e of the pair (p, mate[p]): the four words of (E(a), E(b)) with E(a) <= E(b), the inverted score sum, and the two ordinals
struct dp_ent { dp_ull *ahi, *alo, *bhi, *blo, *k0; uint32_t *oa, *ob; };
__global__ __launch_bounds__(256) void k_dup_entries(dp_cols C, const uint32_t *mate, const dp_ull *eoff, uint64_t m, dp_ent E, uint32_t *perm)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m || mate[p] == DP_NO_MATE || p >= mate[p]) return;
    const uint64_t e = eoff[p];
    uint32_t a = C.pord[p], b = C.pord[mate[p]];
    const uint32_t sum = C.score[a] + C.score[b];          // (two values below 2^31)
    if (C.hi[b] < C.hi[a] || (C.hi[b] == C.hi[a] && C.lo[b] < C.lo[a])) { const uint32_t t = a; a = b; b = t; }
    E.ahi[e] = C.hi[a]; E.alo[e] = C.lo[a]; E.bhi[e] = C.hi[b]; E.blo[e] = C.lo[b];
    E.k0[e] = (dp_ull)(uint32_t)~sum;
    E.oa[e] = a; E.ob[e] = b;
    perm[e] = (uint32_t)e;
}

__global__ __launch_bounds__(256) void k_dup_take(const dp_ull *word, const uint32_t *perm, uint64_t n, dp_ull *key)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) key[i] = word[perm[i]];
}

// every pair but its group's head is a duplicate, and both of its records are
__global__ __launch_bounds__(256) void k_dup_pair_verdict(const uint32_t *perm, const uint32_t *head, uint64_t n, dp_ent E, uint8_t *ver, dp_state *st)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t dup = 0;
    if (i < n && head[i] != (uint32_t)i) {
        const uint32_t e = perm[i];
        ver[E.oa[e]] = 1; ver[E.ob[e]] = 1;
        dup = 1;
    }
    wave_count(&st->dup_pairs, dup);
}

// a fragment that is not its group's head is a duplicate: the head is a paired record where the group holds one, or else the best fragment
__global__ __launch_bounds__(256) void k_dup_frag_verdict(const uint32_t *perm, const uint32_t *head, uint64_t n, const uint8_t *cls, uint8_t *ver, dp_state *st)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t dup = 0;
    if (i < n && head[i] != (uint32_t)i) {
        const uint32_t r = perm[i];
        if ((cls[r] & DP_CLASS) == DP_FRAGMENT) { ver[r] = 1; dup = 1; }
    }
    wave_count(&st->dup_frags, dup);
}

// ------------------------------------------------------------------ apply
// commit == 0: only the checks (a record whose flag does not lie inside the stream is named in bad, an ordinal at or past n_ord is counted).  commit == 1: bit
// 0x400 of every record that is not ignored becomes its verdict; the flag's high byte is byte 19 of the prefixed record.
__global__ __launch_bounds__(256) void k_dup_apply(uint8_t *s, uint64_t n_bytes, const uint64_t *off, uint64_t n, uint64_t first, const uint32_t *ords, const uint8_t *ver, uint64_t n_ord, int commit,
                                                   dp_state *st)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool broken = false;
    uint32_t bad_ord = 0;
    if (i < n) {
        const uint64_t a = off[i] - off[0], ord = ords ? (uint64_t)ords[i] : first + i;
        if (off[i] < off[0] || a > n_bytes || n_bytes - a < ED_MIN_REC) broken = true;
        else if (ord >= n_ord) bad_ord = 1;
        else if (commit) {
            const uint8_t v = ver[ord];
            if (v != 2) {
                const uint8_t b = s[a + 19], nb = v ? (uint8_t)(b | 0x04u) : (uint8_t)(b & ~0x04u);
                if (nb != b) s[a + 19] = nb;
            }
        }
    }
    if (!commit) {
        wave_report_min(&st->bad, broken, i);
        wave_count(&st->bad_ord, bad_ord);
    }
}
