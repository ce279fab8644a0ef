// dev_lane_rows.h -- ksw_extend2 on ONE lane, both sides of a seed and both band trials in ONE row loop.
// The lane kernels (dev_ext_lane.h) run 64 of these side by side, so every instruction a lane spends where its neighbours are not costs
// the whole wave: with the left and the right extension as two calls of the scalar loop, a wave took (its longest left side) + (its
// longest right side), and most jobs have nearly all of their bases on one side.  Here the side and the band trial are lane variables
// and the dynamic program's cell loop exists once: lanes extending to the left, lanes extending to the right and lanes on their second
// band share every instruction, and a wave takes as long as its longest job.
// The arithmetic is ksw_extend2's, statement for statement (the row bound of dev_ext_wave.h and the cells a narrower earlier side left
// in the row included).  Written against two small policies -- where the row lives (L) and where the bases come from (F) -- and kept
// host-compilable, so that tests/cpp/lane_rows_test.cpp can run the same source on rows of exactly `cols` columns.
#pragma once
#include <stdint.h>
#include <stddef.h>
#if defined(__HIPCC__)
#define LROW_FN __host__ __device__ __forceinline__
#define LROW_M __host__ __device__ __forceinline__
#else
#define LROW_FN static inline
#define LROW_M inline
#endif
#ifndef WAVE
#define WAVE 64
#endif

// Rows below the query that cannot matter: the bound and its test (derivation: dev_ext_wave.h).  O = slx_opt.
template <typename O>
LROW_FN int ext_tail_bound0(const O &o, int qlen, int h0, int amax)
{   // B_qlen (the value at row i = qlen); INT_MAX when the bound does not hold
    if (o.o_del < 0 || o.e_del < 0 || o.o_ins < 0 || o.e_ins < 0) return 0x7fffffff;
    const long long b = (long long)h0 + (long long)qlen * (amax > 0 ? amax : 0) - o.o_del - o.e_del;
    return b > 0x3fffffff ? 0x7fffffff : (int)b;
}
LROW_FN bool ext_tail_done(int b, int max, int gscore) { return b <= max && (b > 0 ? b : 0) < gscore; }

// Rows that cannot matter, after ANY row (derivation and preconditions: dev_ext_wave.h, "the row exit").  EXT_ROW_EXIT_*: what has to stay as it is.
#define EXT_ROW_EXIT_OFF 0          // no exit: the loop runs to z-drop, an all-zero row, the tail bound or tlen
#define EXT_ROW_EXIT_STRICT 1       // all six results of ksw_extend2
#define EXT_ROW_EXIT_RELAXED 2      // score, qle, tle, max_off, and which branch of `gscore <= 0 || gscore <= score - pen_clip` the caller takes, with the fields that branch reads
template <typename O>
LROW_FN bool ext_row_exit_ok(const O &o, int qlen, int w, int h0)
{   // w = the trial's effective band (after the max_ins / max_del limits).  Either the band never clips `end`, or what a clipped `end` leaves
    // beyond it -- row -1's insertion ramp in the columns from w + 2 on -- is zero there
    if (o.o_del < 0 || o.e_del < 0 || o.o_ins < 0 || o.e_ins < 0) return false;
    return w + 1 >= qlen || (long long)h0 - o.o_ins - o.e_ins - (long long)(w + 1) * o.e_ins <= 0;
}
// U after row i: m = the row's maximum, hb = what the row left in column -1 for the next one (its h1 start if the band begins at column 0, else 0),
// beg = the next row's first column, apos = max(amax, 0)
LROW_FN int ext_row_bound(int m, int hb, int apos, int qlen, int beg, int tlen, int i)
{
    const int a = qlen - beg, b = tlen - 1 - i;
    const int k = a < b ? a : b;
    return (m > hb ? m : hb) + apos * (k > 0 ? k : 0);
}
// end_bonus: the caller's pen_clip for the relaxed rule; < 0 = the strict rule only
LROW_FN bool ext_row_done(int U, int max, int gscore, int end_bonus) { return (end_bonus >= 0 && U <= max - end_bonus) || ext_tail_done(U, max, gscore); }

// A narrow band for flanks that lose little on the diagonal (derivation and conditions: dev_ext_wave.h, "the narrow band").  L = what the flank's
// main diagonal loses against a perfect match, h0_lower = a lower bound of the score the extension starts from, w_eff = the trial's effective band.
// The band that gives ksw_extend2's six results as w_eff does, or -1 where the bound does not hold or buys nothing.
#define EXT_NARROW_CAP 14           // 2 * band + 3 columns fit LaneRing's 32 (with bwa's default penalties: L <= 20)
template <typename O>
LROW_FN int ext_narrow_band(const O &o, int amax, int L, int h0_lower, int qlen, int tlen, int w_eff)
{
    if (o.o_del < 0 || o.o_ins < 0 || o.e_del <= 0 || o.e_ins <= 0 || amax <= 0) return -1;
    if (qlen < 1 || qlen > tlen) return -1;
    const int oe_del = o.o_del + o.e_del, oe_ins = o.o_ins + o.e_ins;
    if (L <= (oe_del < oe_ins ? oe_del : oe_ins) - 1) return -1;          // the diagonal answers it (diag_extend)
    if (h0_lower <= L) return -1;
    if (o.zdrop > 0 && 2ll * L > o.zdrop) return -1;
    const int wd = L >= o.o_del ? (L - o.o_del) / o.e_del : -1, wi = L >= o.o_ins ? (L - o.o_ins) / o.e_ins : -1;
    const int w = wd > wi ? wd : wi;
    return w >= 0 && w < w_eff && w <= EXT_NARROW_CAP ? w : -1;
}
// the effective band of a trial: ksw_extend2's max_ins / max_del limits on w.  ksw_extend2 has (int)((double)x / e + 1.), then at least 1: in integers x / e + 1
// is the same number wherever that is above 1 (x and e of one sign: the quotient's floor is its truncation, and a double holds it exactly enough), and at most
// 1 wherever the other is -- without the two double divisions, which one lane of k_first_diag's 64 would make the whole wave wait for
template <typename O>
LROW_FN int ext_eff_band(const O &o, int qlen, int amax, int end_bonus, int w)
{
    const int xi = qlen * amax + end_bonus - o.o_ins, xd = qlen * amax + end_bonus - o.o_del;
    int max_ins = o.e_ins ? xi / o.e_ins + 1 : (xi > 0 ? 0x7fffffff : 1);          // (e = 0: what the conversion of +-inf and NaN gives on the GPU)
    max_ins = max_ins > 1 ? max_ins : 1;
    w = w < max_ins ? w : max_ins;
    int max_del = o.e_del ? xd / o.e_del + 1 : (xd > 0 ? 0x7fffffff : 1);
    max_del = max_del > 1 ? max_del : 1;
    return w < max_del ? w : max_del;
}

// Where a lane keeps its H/E row.  WIDE: one 32-bit word per column -- 14-bit H, 14-bit E, the column's query code above them.  NARROW: when
// no score can reach 256 (150 bp reads with bwa's default scores: read length x max(mat) < 256) a column is 8-bit H + 8-bit E in a 16-bit
// word and the query codes sit apart, eight 4-bit codes per word: half the LDS per wave, twice the waves per CU -- and the kernel's time
// is inversely proportional to its waves per CU (measured by padding the rows: 4 / 3 / 2 waves per CU -> 30.8 / 40.4 / 60.3 ms).
struct LaneWide {
    static constexpr bool ring = false;
    uint32_t *eh;                                   // this lane's word of column 0; stride WAVE words
    static LROW_M size_t bytes(int cols) { return (size_t)cols * WAVE * 4; }
    LROW_M void init(uint32_t *base, int, int lane) { eh = base + lane; }
    LROW_M void put_all(int j, int h, int e, int q) { eh[j * WAVE] = (uint32_t)h | (uint32_t)e << 14 | (uint32_t)q << 28; }
    LROW_M uint32_t get(int j) const { return eh[j * WAVE]; }
    LROW_M int q_of(uint32_t v, int) const { return (int)(v >> 28); }
    static LROW_M int h_of(uint32_t v) { return (int)(v & 0x3fffu); }
    static LROW_M int e_of(uint32_t v) { return (int)((v >> 14) & 0x3fffu); }
    LROW_M void put(int j, int h, int e, uint32_t old) { eh[j * WAVE] = (uint32_t)h | (uint32_t)e << 14 | (old & 0xf0000000u); }
    static LROW_M bool zero(uint32_t v) { return (v & 0x0fffffffu) == 0; }
};
struct LaneNarrow {
    static constexpr bool ring = false;
    uint16_t *eh;                                   // 16-bit cells, stride WAVE
    uint32_t *qa;                                   // eight 4-bit query codes per word, stride WAVE words
    static LROW_M size_t bytes(int cols) { return (size_t)cols * WAVE * 2 + (size_t)((cols + 7) / 8) * WAVE * 4; }
    LROW_M void init(uint32_t *base, int cols, int lane) { eh = (uint16_t *)base + lane; qa = base + (size_t)cols * WAVE / 2 + lane; }
    LROW_M void put_all(int j, int h, int e, int q)
    {
        eh[j * WAVE] = (uint16_t)(h | e << 8);
        uint32_t w = (j & 7) ? qa[(j >> 3) * WAVE] : 0u;        // (columns are written in ascending order: a word starts at its column 0)
        w |= (uint32_t)q << ((j & 7) * 4);
        qa[(j >> 3) * WAVE] = w;
    }
    LROW_M uint32_t get(int j) const { return eh[j * WAVE]; }
    LROW_M int q_of(uint32_t, int j) const { return (int)((qa[(j >> 3) * WAVE] >> ((j & 7) * 4)) & 7u); }
    static LROW_M int h_of(uint32_t v) { return (int)(v & 0xffu); }
    static LROW_M int e_of(uint32_t v) { return (int)(v >> 8); }
    LROW_M void put(int j, int h, int e, uint32_t) { eh[j * WAVE] = (uint16_t)(h | e << 8); }
    static LROW_M bool zero(uint32_t v) { return v == 0; }
};

// RING: for jobs whose sides all run in a narrow band (LaneSide::wband <= EXT_NARROW_CAP).  A row of such a side reads and writes the columns
// i - w .. i + w + 1 only -- at most 2 w + 2 <= 30 consecutive columns -- so the cells are a ring of 32, column j at j & 31; the query codes stay as
// LaneNarrow keeps them.  The columns a trial has written so far are 0 .. top without a hole (a row writes beg .. end, and `end` grows by at most two
// over the row before).  A column up to `top` holds its last value: column j + 32 is first written in row j + 31 - w, after the last row that reads
// column j (row j + w).  A column beyond `top` holds row -1's ramp in the other layouts, and a row whose `end` was not clipped by the band in the row
// before it does read one; here the row loop writes the ramp into such a column when `end` first reaches it (ring == true), into the slot column
// j - 32 has left for good by then.
#define LANE_RING_COLS 32
struct LaneRing {
    static constexpr bool ring = true;
    uint16_t *eh;                                   // 16-bit cells, a ring of LANE_RING_COLS, stride WAVE
    uint32_t *qa;                                   // eight 4-bit query codes per word, stride WAVE words
    static LROW_M size_t bytes(int cols) { return (size_t)LANE_RING_COLS * WAVE * 2 + (size_t)((cols + 7) / 8) * WAVE * 4; }
    LROW_M void init(uint32_t *base, int, int lane) { eh = (uint16_t *)base + lane; qa = base + (size_t)LANE_RING_COLS * WAVE / 2 + lane; }
    LROW_M void put_all(int j, int h, int e, int q)
    {
        if (j < LANE_RING_COLS) eh[j * WAVE] = (uint16_t)(h | e << 8);
        uint32_t w = (j & 7) ? qa[(j >> 3) * WAVE] : 0u;
        w |= (uint32_t)q << ((j & 7) * 4);
        qa[(j >> 3) * WAVE] = w;
    }
    LROW_M uint32_t get(int j) const { return eh[(j & (LANE_RING_COLS - 1)) * WAVE]; }
    LROW_M int q_of(uint32_t, int j) const { return (int)((qa[(j >> 3) * WAVE] >> ((j & 7) * 4)) & 7u); }
    static LROW_M int h_of(uint32_t v) { return (int)(v & 0xffu); }
    static LROW_M int e_of(uint32_t v) { return (int)(v >> 8); }
    LROW_M void put(int j, int h, int e, uint32_t) { eh[(j & (LANE_RING_COLS - 1)) * WAVE] = (uint16_t)(h | e << 8); }
    static LROW_M bool zero(uint32_t v) { return v == 0; }
};

// ---------------------------------------------------------------------------------------------- the row loop
// wband: a band both trials are clamped to (ext_narrow_band), < 0 = none
struct LaneSide { int qlen, tlen, q0, end_bonus; int64_t t0; int wband = -1; };          // query base j = F.q(q0 + dir * j), text base t = F.t(t0 + dir * t); dir = -1 for side 0 (left), +1 for side 1
struct LaneRes { int score, qle, tle, gtle, gscore, max_off, aw; };      // ksw_extend2's six results and the band (opt.w << trial) they were found with

// Extends side 0 (where s[0].qlen > 0) from score h0, then side 1 (where s[1].qlen > 0) from the score side 0 ended with, each with the band
// opt.w and -- by mem_chain2aln's rule -- once more with twice the band.  done(side, res) is called once per side that ran, in that order.
// O = slx_opt, MR = MatRows (dev_ext_wave.h), L = the lane's row (not initialised by the caller), F = the bases.
// row_exit (EXT_ROW_EXIT_*): end a trial after a row that rules out any change; *n_exit (optional) counts the trials it ended.
template <typename L, typename F, typename O, typename MR, typename D>
LROW_FN void lane_rows_extend(const LaneSide s[2], int h0, const O &o, const MR &mr, L &row, F &fetch, D done, int row_exit = EXT_ROW_EXIT_STRICT,
                              unsigned int *n_exit = nullptr)
{
    const int o_del = o.o_del, e_del = o.e_del, o_ins = o.o_ins, e_ins = o.e_ins, zdrop = o.zdrop;
    const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
    int amax = 0;
    for (int i = 0; i < 25; ++i) amax = amax > o.mat[i] ? amax : o.mat[i];
    int side = s[0].qlen > 0 ? 0 : (s[1].qlen > 0 ? 1 : 2), trial = 0, prev = -1;
    bool fresh = true;
    int qlen = 0, tlen = 0, q0 = 0, dir = 0, w = 0, aw = 0, tail_top = 0, exit_bonus = -1;
    bool exit_ok = false;
    const int apos = amax > 0 ? amax : 0;
    int64_t t0 = 0;
    int max = 0, max_i = -1, max_j = -1, max_ie = -1, gscore = -1, max_off = 0, beg = 0, end = 0, i = 0;
    int top = 0;                 // LaneRing: the last column that holds this trial's value (row -1's or a later row's)
    while (side < 2) {
        if (fresh) {             // a side's trial begins: its row -1
            fresh = false;
            const int end_bonus = side ? s[1].end_bonus : s[0].end_bonus;
            qlen = side ? s[1].qlen : s[0].qlen; tlen = side ? s[1].tlen : s[0].tlen; q0 = side ? s[1].q0 : s[0].q0; t0 = side ? s[1].t0 : s[0].t0;
            dir = side ? 1 : -1;
            aw = o.w << trial;
            // row -1: eh[0].h = h0, then the insertion ramp while it stays positive; the query code of column j rides along
            for (int j = 0; j <= qlen; ++j) {
                const int v = h0 - oe_ins - (j - 1) * e_ins;
                const int h = j == 0 ? h0 : (v > 0 ? v : 0);
                row.put_all(j, h, 0, j < qlen ? fetch.q(q0 + dir * j) : 0);
            }
            w = ext_eff_band(o, qlen, amax, end_bonus, aw);
            const int wband = side ? s[1].wband : s[0].wband;
            if (wband >= 0) w = w < wband ? w : wband;                  // the narrow band (dev_ext_wave.h): the same six results; aw stays the trial's
            tail_top = ext_tail_bound0(o, qlen, h0, amax);
            exit_ok = row_exit != EXT_ROW_EXIT_OFF && ext_row_exit_ok(o, qlen, w, h0);
            exit_bonus = row_exit == EXT_ROW_EXIT_RELAXED ? end_bonus : -1;
            max = h0;
            max_i = -1; max_j = -1; max_ie = -1; gscore = -1; max_off = 0; beg = 0; end = qlen; i = 0;
            top = qlen < LANE_RING_COLS - 1 ? qlen : LANE_RING_COLS - 1;
        }
        bool stop = i >= tlen || (i >= qlen && ext_tail_done(tail_top - (i - qlen) * e_del, max, gscore));      // dev_ext_wave.h: rows that cannot matter
        if (!stop) {
            const int t = fetch.t(t0 + (int64_t)(dir * i));
            const uint32_t rowp = t == 0 ? mr.packed[0] : t == 1 ? mr.packed[1] : t == 2 ? mr.packed[2] : t == 3 ? mr.packed[3] : mr.packed[4];
            const int row4 = t == 0 ? mr.q4[0] : t == 1 ? mr.q4[1] : t == 2 ? mr.q4[2] : t == 3 ? mr.q4[3] : mr.q4[4];
            int f = 0, m = 0, mj = -1;
            if (beg < i - w) beg = i - w;
            if (end > i + w + 1) end = i + w + 1;
            if (end > qlen) end = qlen;
            if (L::ring) {                                              // columns this trial reaches for the first time: row -1's ramp, as the other layouts hold it
                for (; top < end; ++top) { const int v = h0 - oe_ins - top * e_ins; row.put(top + 1, v > 0 ? v : 0, 0, 0u); }
            }
            int h1 = 0;
            if (beg == 0) { h1 = h0 - (o_del + e_del * (i + 1)); if (h1 < 0) h1 = 0; }
            const int hb = h1;                                          // column -1 as the next row reads it
            uint32_t cur = beg < end ? row.get(beg) : 0u;
            for (int j = beg; j < end; ++j) {
                const uint32_t nxt = row.get(j + 1);                    // (column j + 1 <= qlen exists; read ahead of this cell's arithmetic)
                int M = L::h_of(cur), e = L::e_of(cur);
                const uint32_t q = (uint32_t)row.q_of(cur, j);
#if defined(__HIP_DEVICE_COMPILE__)
                const int sc = q < 4 ? __builtin_amdgcn_sbfe((int)rowp, q << 3, 8u) : row4;
#else
                const int sc = q < 4 ? (int)(int8_t)(rowp >> (q << 3)) : row4;
#endif
                M = M ? M + sc : 0;
                int h = M > e ? M : e;
                h = h > f ? h : f;
                const int hl = h1;                                      // H(i, j-1): what eh[j].h holds for the next row
                h1 = h;
                mj = m > h ? mj : j;
                m = m > h ? m : h;
                int t2 = M - oe_del; t2 = t2 > 0 ? t2 : 0;
                e -= e_del; e = e > t2 ? e : t2;
                row.put(j, hl, e, cur);
                t2 = M - oe_ins; t2 = t2 > 0 ? t2 : 0;
                f -= e_ins; f = f > t2 ? f : t2;
                cur = nxt;
            }
            row.put(end, h1, 0, beg < end ? cur : row.get(end));        // eh[end].h = h1; eh[end].e = 0 (the column keeps its query code)
            if ((end > beg ? end : beg) == qlen) {                       // (the scalar loop's j after its last trip)
                max_ie = gscore > h1 ? max_ie : i;
                gscore = gscore > h1 ? gscore : h1;
            }
            if (m == 0) stop = true;
            else if (m > max) {
                max = m; max_i = i; max_j = mj;
                const int off = mj - i < 0 ? i - mj : mj - i;
                max_off = max_off > off ? max_off : off;
            } else if (zdrop > 0) {
                if (i - max_i > mj - max_j) { if (max - m - ((i - max_i) - (mj - max_j)) * e_del > zdrop) stop = true; }
                else { if (max - m - ((mj - max_j) - (i - max_i)) * e_ins > zdrop) stop = true; }
            }
            if (!stop) {
                int j;
                for (j = beg; j < end && L::zero(row.get(j)); ++j) {}
                beg = j;
                for (j = end; j >= beg && L::zero(row.get(j)); --j) {}
                end = j + 2 < qlen ? j + 2 : qlen;
                if (exit_ok && ext_row_done(ext_row_bound(m, beg == 0 ? hb : 0, apos, qlen, beg, tlen, i), max, gscore, exit_bonus)) {
                    stop = true;                                        // no later row can change what is reported (dev_ext_wave.h)
                    if (n_exit) ++*n_exit;
                }
                ++i;
            }
        }
        if (stop) {              // the trial is over: again with twice the band (mem_chain2aln's rule), or on to the next side
            fresh = true;
            const int before = trial ? prev : (side ? h0 : -1);          // the region's score before this trial
            if (trial == 0 && !(max == before || max_off < (aw >> 1) + (aw >> 2))) { prev = max; trial = 1; }
            else {
                LaneRes r;
                r.score = max; r.qle = max_j + 1; r.tle = max_i + 1; r.gtle = max_ie + 1; r.gscore = gscore; r.max_off = max_off; r.aw = aw;
                done(side, r);
                if (side == 0) h0 = max;
                side = side == 0 && s[1].qlen > 0 ? 1 : 2;
                trial = 0;
            }
        }
    }
}
