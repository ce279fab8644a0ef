// dev_ext_lane.h -- the ahead-of-time extensions of the heavy reads, ONE LANE PER SEED.
//
// A read inside a repeat family keeps ~500 one-seed chains, and mem_chain2aln extends nearly every one of them (they lie at different
// reference positions, so no earlier region covers them): ~1 000 ksw_extend2 calls of ~60 rows per read, which on the wave-per-read
// kernel is a serial walk of 10-40 ms on one wave (the extension stage's tail) and on the wave-per-seed job kernel (k_extend_cand)
// ~10 000 wave instructions per extension.  The extensions of different seeds do not depend on each other, and for these reads there
// are hundreds of them with the same query: here a wave takes 64 seeds and every lane runs ksw_extend2's scalar loops on its own -- the
// H/E row of a lane lives in LDS, column-major across the lanes (cell j * 64 + lane: no bank conflicts; layouts and the row loop: dev_lane_rows.h) -- ~36 instructions
// per cell for 64 extensions at once instead of ~170 per row for one.
// k_extend_reg then replays mem_chain2aln's decisions and takes the regions from the table (cand), as it does after k_extend_cand.
// /root/reference/src/BWAAligner.cpp:104 -> mem_align1 -> mem_chain2aln -> ksw_extend2.
#pragma once
#include "dev_seed4.h"
#include "dev_ext_reg.h"
#include "dev_lane_rows.h"

struct alignas(8) LaneJob {    // one seed extension (k_cand_lane_prep -> k_ext_lanes)
    int64_t s_rbeg, rmax0, rmax1;
    uint64_t q_off;             // the read's codes
    int l_query, s_qbeg, s_len, rid;
    float frac_rep;
    int out;                    // slot of the region in the table (cand_base[r] + seed index)
    int r, c;                   // read and chain (for seedcov)
};

#define LANE_SCORE_LIMIT 16000  // (read length) x max(mat) has to stay below this for the lane kernel to be used (host check)

// (the rows' two layouts, LaneWide and LaneNarrow, and the row loop: dev_lane_rows.h)

struct LaneBases {              // lane_rows_extend's bases: the read's codes, the reference through a 32-base window (one 8-byte read per 32 rows)
    const DevRef &R;
    const uint8_t *query;
    RWin rw;
    __device__ __forceinline__ int q(int j) const { return (int)query[j]; }
    __device__ __forceinline__ int t(int64_t p) { return text_at(R, p, rw); }
};

// the lanes' counts of trials the row exit ended, summed over the wave: one atomic per wave ("ext_row_exits")
__device__ __forceinline__ void lane_exits_add(unsigned int *dst, unsigned int mine, int lane)
{
    const unsigned int sum = (unsigned int)__builtin_amdgcn_readlane(dpp_incl_add_scan((int)mine), WAVE - 1);
    if (dst && sum && lane == 0) atomicAdd(dst, sum);
}

// dev_extend_core, one seed per lane (the same statements; both sides and both band trials run in lane_rows_extend's one row loop)
// row_exit: non-zero = the RELAXED row exit, which is enough here for the reason given at dev_extend_core: `done` below reads gscore / gtle only in
// the branch the rule keeps.  n_exit: this lane's band trials the exit ended.  wband0 / wband1: a narrow band for the left / right side (LaneSide::wband), < 0 = none.
template <typename L>
__device__ DReg lane_extend_core(const DevRef &R, const slx_opt &opt, const MatRows &mr, const uint8_t *query, int l_query, int s_qbeg, int s_len,
                                 int64_t s_rbeg, int64_t rmax0, int64_t rmax1, int rid, float frac_rep, L &eh, int row_exit, unsigned int &n_exit, int wband0 = -1, int wband1 = -1)
{
    DReg a;
    a.rb = a.re = 0; a.qb = a.qe = 0; a.sub = a.csub = a.sub_n = 0; a.seedcov = 0; a.secondary = 0;
    a.n_comp = 0; a.hash = 0;
    int aw0 = opt.w, aw1 = opt.w;
    a.w = opt.w; a.rid = rid;
    a.score = a.truesc = s_len * opt.a; a.qb = 0; a.rb = s_rbeg;          // (what stands where there is nothing to the left of the seed)
    const int qe = s_qbeg + s_len;
    const int64_t re0 = s_rbeg + s_len;
    a.qe = l_query; a.re = re0;                                           // (... and to its right)
    LaneSide sd[2];
    sd[0].qlen = s_qbeg; sd[0].tlen = (int)(s_rbeg - rmax0); sd[0].q0 = s_qbeg - 1; sd[0].t0 = s_rbeg - 1; sd[0].end_bonus = opt.pen_clip5; sd[0].wband = wband0;
    sd[1].qlen = l_query - qe; sd[1].tlen = (int)(rmax1 - re0); sd[1].q0 = qe; sd[1].t0 = re0; sd[1].end_bonus = opt.pen_clip3; sd[1].wband = wband1;
    LaneBases bases{R, query, {0, -1}};
    lane_rows_extend(sd, s_len * opt.a, opt, mr, eh, bases, [&](int side, const LaneRes &er) {
        if (side == 0) {
            aw0 = er.aw;
            a.score = er.score;
            if (er.gscore <= 0 || er.gscore <= a.score - opt.pen_clip5) { a.qb = s_qbeg - er.qle; a.rb = s_rbeg - er.tle; a.truesc = a.score; }
            else { a.qb = 0; a.rb = s_rbeg - er.gtle; a.truesc = er.gscore; }
        } else {
            aw1 = er.aw;
            const int sc0 = a.score;
            a.score = er.score;
            if (er.gscore <= 0 || er.gscore <= a.score - opt.pen_clip3) { a.qe = qe + er.qle; a.re = re0 + er.tle; a.truesc += a.score - sc0; }
            else { a.qe = l_query; a.re = re0 + er.gtle; a.truesc += er.gscore - sc0; }
        }
    }, row_exit ? EXT_ROW_EXIT_RELAXED : EXT_ROW_EXIT_OFF, &n_exit);
    a.w = aw0 > aw1 ? aw0 : aw1;
    a.seedlen0 = s_len;
    a.frac_rep = frac_rep;
    return a;
}

// one wave per selected heavy read: a job for every seed of every kept chain (chains across the lanes: the reference window of a chain
// -- rmax, clipped to its contig -- is computed once and copied into its seeds' jobs)
template <int MAXQ>
__global__ void __launch_bounds__(64) k_cand_lane_prep(DevRef R, Chunk ck, DevOpt dopt, const int *heavy, const unsigned int *n_heavy, const unsigned int *job_off, LaneJob *jobs)
{
    const slx_opt &opt = dopt.o;
    const int lane = threadIdx.x;
    __shared__ int gap_lut[MAXQ + 2];
    for (int q = lane; q < MAXQ + 2; q += WAVE) gap_lut[q] = dev_cal_max_gap(opt, q);
    __syncthreads();
    auto max_gap_of = [&](int q) { return gap_lut[q < 0 ? 0 : (q > MAXQ + 1 ? MAXQ + 1 : q)]; };
    const int64_t l_pac = R.l_pac;
    const unsigned int nh = (unsigned int)__builtin_amdgcn_readfirstlane((int)*n_heavy);
    for (unsigned int s = blockIdx.x; s < nh; s += gridDim.x) {
        const int r = heavy[s];
        const int base = __builtin_amdgcn_readfirstlane(ck.cand_base[r]);
        if (base < 0 || job_off[s + 1] == job_off[s]) continue;
        const unsigned int job0 = job_off[s];
        const ReadWS w = make_ws_uniform(ck, r);
        const uint64_t q_off = ck.offs[r];
        const int l_query = (int)(ck.offs[r + 1] - q_off);
        const int n_chn = ck.n_chain[r];
        const float frac_rep = ck.frac_rep[r];
        unsigned int running = 0;
        for (int cb = 0; cb < n_chn; cb += WAVE) {
            const int ci = cb + lane;
            const int c = ci < n_chn ? w.ia[ci] : -1;
            const int n = c >= 0 ? w.c_n[c] : 0;
            int incl = n;
            for (int d = 1; d < WAVE; d <<= 1) { const int u = __shfl_up(incl, d, WAVE); if (lane >= d) incl += u; }
            const unsigned int my = running + (unsigned int)(incl - n);
            running += (unsigned int)__shfl(incl, WAVE - 1, WAVE);
            if (n <= 0) continue;
            const int *cs = w.c_w + w.c_first[c];
            int64_t rmax0 = l_pac << 1, rmax1 = 0;
            for (int i = 0; i < n; ++i) {
                const int sd = cs[i];
                const int qb = w.s_qbeg(sd), sl = w.s_len(sd);
                const int64_t b = w.s_rbeg[sd] - (qb + max_gap_of(qb));
                const int64_t e = w.s_rbeg[sd] + sl + ((l_query - qb - sl) + max_gap_of(l_query - qb - sl));
                rmax0 = rmax0 < b ? rmax0 : b;
                rmax1 = rmax1 > e ? rmax1 : e;
            }
            rmax0 = rmax0 > 0 ? rmax0 : 0;
            rmax1 = rmax1 < l_pac << 1 ? rmax1 : l_pac << 1;
            const int64_t first_rbeg = w.s_rbeg[cs[0]];
            if (rmax0 < l_pac && l_pac < rmax1) {
                if (first_rbeg < l_pac) rmax1 = l_pac; else rmax0 = l_pac;
            }
            {
                int is_rev;
                const int rid = dev_pos2rid(R, dev_depos(R, first_rbeg, &is_rev));
                int64_t far_beg = R.ann_off[rid], far_end = far_beg + R.ann_len[rid];
                if (is_rev) { const int64_t t = far_beg; far_beg = (l_pac << 1) - far_end; far_end = (l_pac << 1) - t; }
                rmax0 = rmax0 > far_beg ? rmax0 : far_beg;
                rmax1 = rmax1 < far_end ? rmax1 : far_end;
            }
            const int rid_c = w.c_rid[c];
            for (int i = 0; i < n; ++i) {
                const int sd = cs[i];
                LaneJob j;
                j.s_rbeg = w.s_rbeg[sd]; j.rmax0 = rmax0; j.rmax1 = rmax1; j.q_off = q_off; j.l_query = l_query;
                j.s_qbeg = w.s_qbeg(sd); j.s_len = w.s_len(sd); j.rid = rid_c; j.frac_rep = frac_rep; j.out = base + sd; j.r = r; j.c = c;
                jobs[job0 + my + (unsigned int)i] = j;
            }
        }
    }
}

// (dynamic LDS: columns 0 .. longest query of an extension = longest read - min_seed_len: 34 KB per wave for 150 bp reads in the wide layout -- four waves
// per CU -- 21 KB in the narrow one)
template <typename L>
__global__ void __launch_bounds__(64) k_ext_lanes(DevRef R, Chunk ck, DevOpt dopt, const unsigned int *n_heavy, const unsigned int *job_off, unsigned int *queue,
                                                   const LaneJob *jobs, DReg *cand, int cols)
{
    const slx_opt &opt = dopt.o;
    const int lane = threadIdx.x;
    const MatRows mr = make_matrows(opt.mat);
    extern __shared__ uint32_t lane_lds[];
    L row;
    row.init(lane_lds, cols, lane);
    const unsigned int nh = (unsigned int)__builtin_amdgcn_readfirstlane((int)*n_heavy);
    const unsigned int n_jobs = nh ? (unsigned int)__builtin_amdgcn_readfirstlane((int)job_off[nh]) : 0u;
    unsigned int exit_cnt = 0;                       // this lane's band trials the row exit ended
    for (;;) {
        const unsigned int base = wave_take(queue, (unsigned int)WAVE);
        if (base >= n_jobs) break;
        const unsigned int job = base + (unsigned int)lane;
        if (job < n_jobs) {
            const LaneJob j = jobs[job];
            const uint8_t *query = ck.codes + j.q_off;
            DReg a = lane_extend_core<L>(R, opt, mr, query, j.l_query, j.s_qbeg, j.s_len, j.s_rbeg, j.rmax0, j.rmax1, j.rid, j.frac_rep, row, ck.ext_row_exit, exit_cnt);
            // seedcov: the chain's seeds that lie inside the region
            const ReadWS w = make_ws(ck, j.r);
            const int n = w.c_n[j.c];
            const int *cs = w.c_w + w.c_first[j.c];
            int cov = 0;
            for (int i = 0; i < n; ++i) {
                const int t = cs[i];
                const int t_qbeg = w.s_qbeg(t), t_len = w.s_len(t);
                const int64_t t_rbeg = w.s_rbeg[t];
                if (t_qbeg >= a.qb && t_qbeg + t_len <= a.qe && t_rbeg >= a.rb && t_rbeg + t_len <= a.re) cov += t_len;
            }
            a.seedcov = cov;
            cand[j.out] = a;
        }
    }
    lane_exits_add(ck.ext_exits, exit_cnt, lane);
}

// ---------------------------------------------------------------------------------------------- light reads: the top-seed extensions that need the dynamic program, one lane per job
// k_ext_first gives each of them a wave (~11 000 wave instructions per job of which a band of a few dozen columns uses a fraction of the lanes).  The jobs are independent
// and come with everything in one 64-byte descriptor, so they can run as the heavy reads' seeds do above, 64 per wave on lane_extend_core -- but a wave then lasts as long
// as its longest job, and the work of a job goes with the SQUARE of its extension queries (0 .. read length - seed length bases on either side of the seed).  Hence the
// bins: the jobs k_first_diag left are counting-sorted by sqrt(left^2 + right^2) into 64 classes, most work first, so that the 64 jobs of a wave are alike and the long
// ones start early (three small launches, no host round trip; the order inside a class is whatever the atomics give: every job writes its own table entry).
// "ext_narrow": k_first_diag also measures what a job's flanks lose on their main diagonals.  A side that loses little runs in the narrow band that allows
// (dev_ext_wave.h, "the narrow band"; the bands go with the job in FirstJob::pad), and the jobs whose sides ALL do -- 54 % of C3's -- go on a list of their
// own: k_first_lanes<LaneRing>, rows of 32 columns (8.4 KB of LDS a wave instead of 21: 16 waves per CU, what its 99 VGPRs allow), binned by their own
// work, bases x band width.  Mixed into the other jobs' waves the narrow band buys next to nothing: a wave lasts as long as its widest lane.
// (by_band: the jobs of the narrow list, whose work is their bases times the width of their bands, 2 w + 1 columns a row)
// FirstJob::pad as k_first_diag leaves it: the narrow band (ext_narrow_band) of either side + 1, 16 bits each; 0 = none
__device__ __forceinline__ int first_job_band(const FirstJob &j, int side) { return (int)((side ? (unsigned int)j.pad >> 16 : (unsigned int)j.pad) & 0xffffu) - 1; }
__device__ __forceinline__ int first_job_bin(const FirstJob &j, int max_len, int by_band)
{
    const int left = j.s_qbeg, right = j.l_query - j.s_qbeg - j.s_len;
    float w;
    if (by_band) {
        const int b0 = first_job_band(j, 0), b1 = first_job_band(j, 1);
        w = (float)(left * (2 * (b0 > 0 ? b0 : 0) + 1) + right * (2 * (b1 > 0 ? b1 : 0) + 1)) / (float)(2 * EXT_NARROW_CAP + 1);
    } else w = sqrtf((float)(left * left + right * right));
    int b = (int)(w * 64.f / (float)(max_len > 0 ? max_len : 1));
    b = b > 63 ? 63 : (b < 0 ? 0 : b);
    return 63 - b;
}
__global__ void __launch_bounds__(256) k_first_bin_count(const FirstJob *jobs, const unsigned int *dp_list, const unsigned int *n_dp, int max_len, unsigned int *bins, int by_band)
{
    __shared__ unsigned int s[64];
    if (threadIdx.x < 64) s[threadIdx.x] = 0;
    __syncthreads();
    const unsigned int n = *n_dp;
    for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) atomicAdd(&s[first_job_bin(jobs[dp_list[t]], max_len, by_band)], 1u);
    __syncthreads();
    if (threadIdx.x < 64 && s[threadIdx.x]) atomicAdd(&bins[threadIdx.x], s[threadIdx.x]);
}
__global__ void k_first_bin_scan(unsigned int *bins)          // bins[64 + b] = where class b starts (then its cursor)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) { unsigned int acc = 0; for (int b = 0; b < 64; ++b) { bins[64 + b] = acc; acc += bins[b]; } }
}
__global__ void __launch_bounds__(256) k_first_bin_scatter(const FirstJob *jobs, const unsigned int *dp_list, const unsigned int *n_dp, int max_len, unsigned int *bins, unsigned int *out, int by_band)
{
    __shared__ unsigned int s_cnt[64], s_base[64];
    const unsigned int n = *n_dp;
    for (unsigned int t0 = blockIdx.x * blockDim.x; t0 < n; t0 += gridDim.x * blockDim.x) {          // (block-uniform trip count: the barriers below are reached by all)
        if (threadIdx.x < 64) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        const unsigned int t = t0 + threadIdx.x;
        int b = -1;
        unsigned int job = 0, my = 0;
        if (t < n) { job = dp_list[t]; b = first_job_bin(jobs[job], max_len, by_band); my = atomicAdd(&s_cnt[b], 1u); }
        __syncthreads();
        if (threadIdx.x < 64 && s_cnt[threadIdx.x]) s_base[threadIdx.x] = atomicAdd(&bins[64 + threadIdx.x], s_cnt[threadIdx.x]);
        __syncthreads();
        if (b >= 0) out[s_base[b] + my] = job;
        __syncthreads();
    }
}

template <typename L>
__global__ void __launch_bounds__(64) k_first_lanes(DevRef R, Chunk ck, DevOpt dopt, unsigned int *queue, const FirstJob *jobs, DReg *first, const unsigned int *list,
                                                     const unsigned int *n_list, int cols, unsigned int *n_ran)
{
    const slx_opt &opt = dopt.o;
    const int lane = threadIdx.x;
    const MatRows mr = make_matrows(opt.mat);
    extern __shared__ uint32_t lane_lds[];
    L row;
    row.init(lane_lds, cols, lane);
    const unsigned int n_jobs = (unsigned int)__builtin_amdgcn_readfirstlane((int)*n_list);
    unsigned int exit_cnt = 0;                       // this lane's band trials the row exit ended
    for (;;) {
        const unsigned int base = wave_take(queue, (unsigned int)WAVE);
        if (base >= n_jobs) break;
        const unsigned int t = base + (unsigned int)lane;
        if (t < n_jobs) {
            const unsigned int job = list[t];
            const FirstJob j = jobs[job];
            const DReg a = lane_extend_core<L>(R, opt, mr, ck.codes + j.q_off, j.l_query, j.s_qbeg, j.s_len, j.s_rbeg, j.rmax0, j.rmax1, j.rid, j.frac_rep, row, ck.ext_row_exit, exit_cnt,
                                                 first_job_band(j, 0), first_job_band(j, 1));          // (the bands k_first_diag found: none with "ext_narrow" 0)
            first[job] = a;                              // seedcov is filled in by k_ext_replay
        }
        if (lane == 0) atomicAdd(n_ran, n_jobs - base < (unsigned int)WAVE ? n_jobs - base : (unsigned int)WAVE);      // jobs this wave has run ("first_lane_jobs")
    }
    lane_exits_add(ck.ext_exits, exit_cnt, lane);
}

// ---------------------------------------------------------------------------------------------- light reads: the diagonal, one lane per job
// Most top-seed extensions of the light reads are answered by the diagonal alone (diag_extend, dev_ext_reg.h: at most oe - 1 lost against a
// perfect match).  One wave per job that is ~1 000 instructions around two short scans -- 12.8 of k_ext_first's 20 ms per 8.3 M reads;
// one LANE per job it is a loop over the query with both sequences read through register windows.  k_first_diag answers those jobs (the
// region goes straight into the table) and lists the others for k_ext_first, which keeps the dynamic program.
// loss_stop: the largest loss worth measuring -- oe - 1 where only the diagonal's answer is wanted, beyond it what ext_narrow_band's cap allows.  loss_out: what
// the flank's main diagonal loses against a perfect match, -1 where it is not known (no diagonal of qlen bases, or more than loss_stop).
template <typename QF, typename TF>
__device__ __forceinline__ bool lane_diag_extend(int qlen, QF qf, int tlen, TF tf, const slx_opt &o, const MatRows &mr, int amax, int h0, int loss_stop, ExtResult &out, int &loss_out)
{   // the conditions and the result of diag_extend, computed by one lane
    loss_out = -1;
    if (tlen < qlen || qlen > 3 * WAVE || qlen < 1) return false;
    if ((long long)h0 + (long long)qlen * amax >= (1 << 22)) return false;
    const int oe_del = o.o_del + o.e_del, oe_ins = o.o_ins + o.e_ins;
    const int oe = oe_del < oe_ins ? oe_del : oe_ins;
    int loss = 0, run = h0, best = h0, best_p = -1;
    for (int p = 0; p < qlen; ++p) {
        const int t = tf(p), q = qf(p);
        const uint32_t rowp = t == 0 ? mr.packed[0] : t == 1 ? mr.packed[1] : t == 2 ? mr.packed[2] : mr.packed[3];
        const int row4 = t == 0 ? mr.q4[0] : t == 1 ? mr.q4[1] : t == 2 ? mr.q4[2] : mr.q4[3];
        const int sc = q < 4 ? __builtin_amdgcn_sbfe((int)rowp, (uint32_t)q << 3, 8u) : row4;
        loss += amax - sc;
        if (loss > loss_stop) return false;              // (the loss only grows: amax is the largest entry)
        run += sc;
        if (run > best) { best = run; best_p = p; }      // the largest prefix above h0 at its FIRST position
    }
    loss_out = loss;
    if (loss > oe - 1 || h0 <= loss) return false;
    out.score = best; out.qle = best_p + 1; out.tle = best_p + 1; out.gtle = qlen; out.gscore = run; out.max_off = 0;
    return true;
}

// The band of a side of a job that goes to the dynamic program (ext_narrow_band, dev_lane_rows.h), from the loss k_first_diag measured (< 0: not known).
// A side the diagonal would answer runs in the row loop all the same when the job's other side needs it: the bound holds for any L' >= L below the
// start, so it is taken at L' = oe.  A side whose own limits (max_ins / max_del) keep every trial's band within the cap needs no clamp and fits
// LaneRing as it is: it gets the cap, which clamps nothing.  dp_side: the side is one the diagonal does not answer and has a band ("ext_narrow_sides").
__device__ __forceinline__ int first_side_band(const slx_opt &o, int amax, int loss, int h0_lower, int qlen, int tlen, int end_bonus, bool &dp_side)
{
    dp_side = false;
    const int oe_del = o.o_del + o.e_del, oe_ins = o.o_ins + o.e_ins;
    const int oe = oe_del < oe_ins ? oe_del : oe_ins;
    if (o.e_ins <= 0 || o.e_del <= 0) return -1;
    const int lim = ext_eff_band(o, qlen, amax, end_bonus, 0x3fffffff);          // what max_ins / max_del allow: every trial's band is min(its w, lim)
    int band = -1;
    if (loss >= 0) {
        band = ext_narrow_band(o, amax, loss > oe ? loss : oe, h0_lower, qlen, tlen, o.w < lim ? o.w : lim);
        dp_side = band >= 0 && loss > oe - 1;
    }
    if (band < 0 && lim <= EXT_NARROW_CAP) band = EXT_NARROW_CAP;
    return band;
}

// One job of k_first_diag: true = the job needs the dynamic program (else its region is in the table).  narrow (the knob "ext_narrow"): non-zero = such a job
// carries the bands of its sides in FirstJob::pad; all = every side of it has one; n_dp_sides = its sides the diagonal does not answer that have a band.
__device__ __forceinline__ bool first_diag_job(const DevRef &R, const Chunk &ck, const slx_opt &opt, const MatRows &mr, int amax, FirstJob *jobs, unsigned int job, DReg *first, int narrow,
                                               bool &all, unsigned int &n_dp_sides)
{
    const FirstJob j = jobs[job];
    if (j.l_query <= 0) return false;                     // an empty job (a read whose slots pass the table end): k_extend_reg has the read
    const uint8_t *codes = ck.codes;
    QWin qw; qw.bits = 0; qw.chunk = 0xffffffffu;
    RWin rw; rw.bits = 0; rw.chunk = -1;
    DReg a;
    a.rb = a.re = 0; a.qb = a.qe = 0; a.sub = a.csub = a.sub_n = 0; a.seedcov = 0; a.secondary = 0;
    a.n_comp = 0; a.hash = 0;
    a.score = a.truesc = -1; a.rid = j.rid;
    // the diagonal's max_off is 0, so the band-doubling loop of dev_extend_core ends after its first trip (band opt.w) -- unless the band is so
    // narrow that (w >> 1) + (w >> 2) is 0: then it takes the second trip, finds the same score and ends with band 2 w
    const int aw_ext = ((opt.w >> 1) + (opt.w >> 2)) > 0 ? opt.w : opt.w << 1;
    int aw0 = opt.w, aw1 = opt.w;
    const int oe_del = opt.o_del + opt.e_del, oe_ins = opt.o_ins + opt.e_ins;
    const int oe = oe_del < oe_ins ? oe_del : oe_ins;
    int loss_stop = oe - 1;
    if (narrow && opt.o_del >= 0 && opt.o_ins >= 0 && opt.e_del > 0 && opt.e_ins > 0) {          // the largest loss whose band is within the cap
        const long long sd = (long long)opt.o_del + (long long)(EXT_NARROW_CAP + 1) * opt.e_del, si = (long long)opt.o_ins + (long long)(EXT_NARROW_CAP + 1) * opt.e_ins;
        const long long st = (sd < si ? sd : si) - 1;
        loss_stop = st > loss_stop ? (st < (1 << 20) ? (int)st : (1 << 20)) : loss_stop;
    }
    bool ok0 = true, ok1 = true;
    int loss0 = -1, loss1 = -1;
    const int s_qbeg = j.s_qbeg, s_len = j.s_len, l_query = j.l_query;
    const int64_t s_rbeg = j.s_rbeg;
    const int qe = s_qbeg + s_len;
    const int64_t re0 = s_rbeg + s_len;
    if (s_qbeg) {
        aw0 = aw_ext;
        ExtResult er;
        ok0 = lane_diag_extend(s_qbeg, [&](int p) { return q_at(codes, j.q_off + (uint64_t)(s_qbeg - 1 - p), qw); }, (int)(s_rbeg - j.rmax0),
                               [&](int t) { return text_at(R, s_rbeg - 1 - t, rw); }, opt, mr, amax, s_len * opt.a, loss_stop, er, loss0);
        if (ok0) {
            a.score = er.score;
            if (er.gscore <= 0 || er.gscore <= a.score - opt.pen_clip5) { a.qb = s_qbeg - er.qle; a.rb = s_rbeg - er.tle; a.truesc = a.score; }
            else { a.qb = 0; a.rb = s_rbeg - er.gtle; a.truesc = er.gscore; }
        }
    } else { a.score = a.truesc = s_len * opt.a; a.qb = 0; a.rb = s_rbeg; }
    // the right side starts from the left side's score.  Where the left side needs the dynamic program that score is not known here: its lower bound, the
    // seed's own score (an extension never ends below its h0), does for measuring the loss and for the band
    const int h0_right = ok0 ? a.score : s_len * opt.a;
    if (ok0 || narrow) {
        if (qe != l_query) {
            aw1 = aw_ext;
            const int sc0 = a.score;
            ExtResult er;
            ok1 = lane_diag_extend(l_query - qe, [&](int p) { return q_at(codes, j.q_off + (uint64_t)(qe + p), qw); }, (int)(j.rmax1 - re0),
                                   [&](int t) { return text_at(R, re0 + t, rw); }, opt, mr, amax, h0_right, loss_stop, er, loss1);
            if (ok0 && ok1) {
                a.score = er.score;
                if (er.gscore <= 0 || er.gscore <= a.score - opt.pen_clip3) { a.qe = qe + er.qle; a.re = re0 + er.tle; a.truesc += a.score - sc0; }
                else { a.qe = l_query; a.re = re0 + er.gtle; a.truesc += er.gscore - sc0; }
            }
        } else { a.qe = l_query; a.re = s_rbeg + s_len; }
    }
    if (ok0 && ok1) {
        a.w = aw0 > aw1 ? aw0 : aw1;
        a.seedlen0 = s_len;
        a.frac_rep = j.frac_rep;
        first[job] = a;                                   // seedcov is filled in by k_ext_replay
        return false;
    }
    if (narrow) {
        bool dp0 = false, dp1 = false;
        const int b0 = s_qbeg ? first_side_band(opt, amax, loss0, s_len * opt.a, s_qbeg, (int)(s_rbeg - j.rmax0), opt.pen_clip5, dp0) : -1;
        const int b1 = qe != l_query ? first_side_band(opt, amax, loss1, h0_right, l_query - qe, (int)(j.rmax1 - re0), opt.pen_clip3, dp1) : -1;
        jobs[job].pad = (int)((unsigned int)(b0 + 1) | (unsigned int)(b1 + 1) << 16);
        all = (!s_qbeg || b0 >= 0) && (qe == l_query || b1 >= 0);
        n_dp_sides = (unsigned int)dp0 + (unsigned int)dp1;
    }
    return true;
}

// The jobs that need the dynamic program go on dp_list -- with nar_list, those whose sides all have a narrow band go on nar_list (k_first_lanes<LaneRing>).
// nar_stat (8-byte aligned): [0] += the jobs whose sides all have a band (with nar_list: that list's length), [1] += the sides the diagonal does not answer that
// have one.  The lists' counters take every top seed's worth of same-address atomics (one per wave was 1.2 of the kernel's 1.8 ms): the four waves of a block
// add their counts up in LDS and the block takes its places with one atomic per counter, the two of nar_stat in one 64-bit add.
__global__ void __launch_bounds__(256) k_first_diag(DevRef R, Chunk ck, DevOpt dopt, int n, const unsigned int *first_off, unsigned int cap, FirstJob *jobs, DReg *first,
                                                    unsigned int *dp_list, unsigned int *n_dp, int narrow, unsigned int *nar_list, unsigned int *nar_stat)
{
    const slx_opt &opt = dopt.o;
    const MatRows mr = make_matrows(opt.mat);
    int amax = 0;
    for (int i = 0; i < 25; ++i) amax = amax > opt.mat[i] ? amax : opt.mat[i];
    unsigned int n_jobs = first_off[n];
    if (n_jobs > cap) n_jobs = cap;
    const unsigned int job = blockIdx.x * blockDim.x + threadIdx.x;
    bool all = false;
    unsigned int sides = 0;
    const bool dp = job < n_jobs && first_diag_job(R, ck, opt, mr, amax, jobs, job, first, narrow, all, sides);
    __shared__ unsigned int s_cnt[4][3], s_base[2];          // per wave: jobs for dp_list, jobs with every side narrow, narrow sides -- then where the wave's jobs go
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & (WAVE - 1);
    const bool to_nar = dp && all && nar_list != nullptr, to_dp = dp && !to_nar;
    const unsigned long long m_dp = __ballot(to_dp), m_nar = __ballot(to_nar);
    const unsigned int w_all = (unsigned int)__popcll(__ballot(dp && all));
    const unsigned int w_sides = (unsigned int)__builtin_amdgcn_readlane(dpp_incl_add_scan((int)sides), WAVE - 1);
    if (ln == 0) { s_cnt[wv][0] = (unsigned int)__popcll(m_dp); s_cnt[wv][1] = (unsigned int)__popcll(m_nar); s_cnt[wv][2] = w_all | w_sides << 16; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int d = 0, a = 0, n_all = 0, n_sides = 0;
        for (int w = 0; w < 4; ++w) {
            unsigned int t = s_cnt[w][0]; s_cnt[w][0] = d; d += t;
            t = s_cnt[w][1]; s_cnt[w][1] = a; a += t;
            n_all += s_cnt[w][2] & 0xffffu; n_sides += s_cnt[w][2] >> 16;
        }
        s_base[0] = d ? atomicAdd(n_dp, d) : 0u;
        s_base[1] = (n_all | n_sides) ? (unsigned int)atomicAdd((unsigned long long *)nar_stat, (unsigned long long)n_all | (unsigned long long)n_sides << 32) : 0u;
    }
    __syncthreads();
    // (with nar_list every job counted in n_all goes on it, so the low word of nar_stat before the add is where the block's narrow jobs start)
    if (to_dp) dp_list[s_base[0] + s_cnt[wv][0] + __builtin_amdgcn_mbcnt_hi((uint32_t)(m_dp >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_dp, 0u))] = job;
    if (to_nar) nar_list[s_base[1] + s_cnt[wv][1] + __builtin_amdgcn_mbcnt_hi((uint32_t)(m_nar >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_nar, 0u))] = job;
}
