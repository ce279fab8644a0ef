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
// the branch the rule keeps.  n_exit: this lane's band trials the exit ended.
template <typename L>
__device__ DReg lane_extend_core(const DevRef &R, const slx_opt &opt, const MatRows &mr, const uint8_t *query, int l_query, int s_qbeg, int s_len,
                                 int64_t s_rbeg, int64_t rmax0, int64_t rmax1, int rid, float frac_rep, L &eh, int row_exit, unsigned int &n_exit)
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
    sd[0].qlen = s_qbeg; sd[0].tlen = (int)(s_rbeg - rmax0); sd[0].q0 = s_qbeg - 1; sd[0].t0 = s_rbeg - 1; sd[0].end_bonus = opt.pen_clip5;
    sd[1].qlen = l_query - qe; sd[1].tlen = (int)(rmax1 - re0); sd[1].q0 = qe; sd[1].t0 = re0; sd[1].end_bonus = opt.pen_clip3;
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
__device__ __forceinline__ int first_job_bin(const FirstJob &j, int max_len)
{
    const int left = j.s_qbeg, right = j.l_query - j.s_qbeg - j.s_len;
    const float w = sqrtf((float)(left * left + right * right));
    int b = (int)(w * 64.f / (float)(max_len > 0 ? max_len : 1));
    b = b > 63 ? 63 : (b < 0 ? 0 : b);
    return 63 - b;
}
__global__ void __launch_bounds__(256) k_first_bin_count(const FirstJob *jobs, const unsigned int *dp_list, const unsigned int *n_dp, int max_len, unsigned int *bins)
{
    __shared__ unsigned int s[64];
    if (threadIdx.x < 64) s[threadIdx.x] = 0;
    __syncthreads();
    const unsigned int n = *n_dp;
    for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) atomicAdd(&s[first_job_bin(jobs[dp_list[t]], max_len)], 1u);
    __syncthreads();
    if (threadIdx.x < 64 && s[threadIdx.x]) atomicAdd(&bins[threadIdx.x], s[threadIdx.x]);
}
__global__ void k_first_bin_scan(unsigned int *bins)          // bins[64 + b] = where class b starts (then its cursor)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) { unsigned int acc = 0; for (int b = 0; b < 64; ++b) { bins[64 + b] = acc; acc += bins[b]; } }
}
__global__ void __launch_bounds__(256) k_first_bin_scatter(const FirstJob *jobs, const unsigned int *dp_list, const unsigned int *n_dp, int max_len, unsigned int *bins, unsigned int *out)
{
    __shared__ unsigned int s_cnt[64], s_base[64];
    const unsigned int n = *n_dp;
    for (unsigned int t0 = blockIdx.x * blockDim.x; t0 < n; t0 += gridDim.x * blockDim.x) {          // (block-uniform trip count: the barriers below are reached by all)
        if (threadIdx.x < 64) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        const unsigned int t = t0 + threadIdx.x;
        int b = -1;
        unsigned int job = 0, my = 0;
        if (t < n) { job = dp_list[t]; b = first_job_bin(jobs[job], max_len); my = atomicAdd(&s_cnt[b], 1u); }
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
            const DReg a = lane_extend_core<L>(R, opt, mr, ck.codes + j.q_off, j.l_query, j.s_qbeg, j.s_len, j.s_rbeg, j.rmax0, j.rmax1, j.rid, j.frac_rep, row, ck.ext_row_exit, exit_cnt);
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
template <typename QF, typename TF>
__device__ __forceinline__ bool lane_diag_extend(int qlen, QF qf, int tlen, TF tf, const slx_opt &o, const MatRows &mr, int amax, int h0, ExtResult &out)
{   // the conditions and the result of diag_extend, computed by one lane
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
        if (loss > oe - 1) return false;                 // (the loss only grows: amax is the largest entry)
        run += sc;
        if (run > best) { best = run; best_p = p; }      // the largest prefix above h0 at its FIRST position
    }
    if (h0 <= loss) return false;
    out.score = best; out.qle = best_p + 1; out.tle = best_p + 1; out.gtle = qlen; out.gscore = run; out.max_off = 0;
    return true;
}

__global__ void __launch_bounds__(256) k_first_diag(DevRef R, Chunk ck, DevOpt dopt, int n, const unsigned int *first_off, unsigned int cap, const FirstJob *jobs, DReg *first,
                                                    unsigned int *dp_list, unsigned int *n_dp)
{
    const slx_opt &opt = dopt.o;
    const MatRows mr = make_matrows(opt.mat);
    int amax = 0;
    for (int i = 0; i < 25; ++i) amax = amax > opt.mat[i] ? amax : opt.mat[i];
    unsigned int n_jobs = first_off[n];
    if (n_jobs > cap) n_jobs = cap;
    const unsigned int job = blockIdx.x * blockDim.x + threadIdx.x;
    if (job >= n_jobs) return;
    const FirstJob j = jobs[job];
    if (j.l_query <= 0) return;                           // an empty job (a read whose slots pass the table end): k_extend_reg has the read
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
    bool ok = true;
    const int s_qbeg = j.s_qbeg, s_len = j.s_len, l_query = j.l_query;
    const int64_t s_rbeg = j.s_rbeg;
    if (s_qbeg) {
        aw0 = aw_ext;
        ExtResult er;
        ok = lane_diag_extend(s_qbeg, [&](int p) { return q_at(codes, j.q_off + (uint64_t)(s_qbeg - 1 - p), qw); }, (int)(s_rbeg - j.rmax0),
                              [&](int t) { return text_at(R, s_rbeg - 1 - t, rw); }, opt, mr, amax, s_len * opt.a, er);
        if (ok) {
            a.score = er.score;
            if (er.gscore <= 0 || er.gscore <= a.score - opt.pen_clip5) { a.qb = s_qbeg - er.qle; a.rb = s_rbeg - er.tle; a.truesc = a.score; }
            else { a.qb = 0; a.rb = s_rbeg - er.gtle; a.truesc = er.gscore; }
        }
    } else { a.score = a.truesc = s_len * opt.a; a.qb = 0; a.rb = s_rbeg; }
    if (ok) {
        if (s_qbeg + s_len != l_query) {
            aw1 = aw_ext;
            const int sc0 = a.score, qe = s_qbeg + s_len;
            const int64_t re0 = s_rbeg + s_len;
            ExtResult er;
            ok = lane_diag_extend(l_query - qe, [&](int p) { return q_at(codes, j.q_off + (uint64_t)(qe + p), qw); }, (int)(j.rmax1 - re0),
                                  [&](int t) { return text_at(R, re0 + t, rw); }, opt, mr, amax, sc0, er);
            if (ok) {
                a.score = er.score;
                if (er.gscore <= 0 || er.gscore <= a.score - opt.pen_clip3) { a.qe = qe + er.qle; a.re = re0 + er.tle; a.truesc += a.score - sc0; }
                else { a.qe = l_query; a.re = re0 + er.gtle; a.truesc += er.gscore - sc0; }
            }
        } else { a.qe = l_query; a.re = s_rbeg + s_len; }
    }
    if (ok) {
        a.w = aw0 > aw1 ? aw0 : aw1;
        a.seedlen0 = s_len;
        a.frac_rep = j.frac_rep;
        first[job] = a;                                   // seedcov is filled in by k_ext_replay
    } else dp_list[wave_fetch_inc(n_dp)] = job;
}
