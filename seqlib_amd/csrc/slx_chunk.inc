// slx_chunk.inc -- one chunk of reads through the pipeline: the small kernels, the launch sequence (run_chunk, launch_tail) and its
// routing thresholds.  Included by slx_align.hip (reads below 65 536 bp: 32-bit query-position packings) and, inside namespace slxw, by
// slx_align_wide.hip (the same code with 64-bit packings for longer reads; dev_pack.h).

// ---------------------------------------------------------------- small kernels
__device__ __forceinline__ uint32_t nt4_of(uint32_t b)
{   // nst_nt4_table as mem_align1_core applies it: bytes < 4 are kept, A/C/G/T (either case) -> 0..3, else 4
    const uint32_t u = b & 0xDFu;
    const uint32_t x = (b >> 1) & 3u;                        // A 0, C 1, T 2, G 3
    const bool letter = u == 'A' || u == 'C' || u == 'G' || u == 'T';
    return b < 4u ? b : (letter ? (x ^ (x >> 1)) : 4u);
}

// 16 bases per thread: four aligned 32-bit loads when the source allows it, one 16-byte store (the codes buffer is 16-byte aligned)
__global__ void k_encode(const uint8_t *ascii, uint8_t *codes, size_t n)
{
    const size_t n16 = (n + 15) >> 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const bool aligned = ((uintptr_t)ascii & 3) == 0;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n16; t += stride) {
        const size_t i = t << 4;
        uint32_t w[4];
        if (aligned && i + 16 <= n) {
            const uint32_t *src = (const uint32_t *)(ascii + i);
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = src[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                w[k] = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) { const size_t p = i + 4 * k + b; w[k] |= (uint32_t)(p < n ? ascii[p] : (uint8_t)'N') << (8 * b); }
            }
        }
        uint4 o;
        uint32_t *ov = &o.x;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            ov[k] = nt4_of(w[k] & 0xff) | nt4_of((w[k] >> 8) & 0xff) << 8 | nt4_of((w[k] >> 16) & 0xff) << 16 | nt4_of(w[k] >> 24) << 24;
        *(uint4 *)(codes + i) = o;                           // the buffer is padded: a partial last group writes its 16 bytes
    }
}

__global__ void k_order_keys(const unsigned long long *seed_cnt, int n, unsigned int *key, int *val)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long c = seed_cnt[i];
    key[i] = c > 0xfffffu ? 0xfffffu : (unsigned int)c;   // 20-bit keys are plenty to separate heavy from light
    val[i] = i;
}

// sort keys of the heavy list (heaviest first): the seed count of every read on it
__global__ void k_heavy_keys(const unsigned long long *seed_cnt, const int *heavy, unsigned int n_heavy, unsigned int *key)
{
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_heavy) return;
    const unsigned long long c = seed_cnt[heavy[i]];
    key[i] = c > 0xfffffu ? 0xfffffu : (unsigned int)c;   // 20-bit keys are plenty
}

__global__ void k_rel_offsets(const uint64_t *offs, uint64_t *rel, int n_reads, uint64_t base)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n_reads) rel[i] = offs[i] - base;
}


#define CAND_REP_AUTO_READS (5 << 20)
#ifndef COOP_N1
#define COOP_N1 768      // chains the first LDS table of k_chain_coop holds: 25 KB per wave, six waves per CU (measured on C3: 1536 -> 47.8,
                         // 1024 -> 48.9, 768 -> 49.3, 512 -> 49.0 M reads/s; reads beyond it take the 4 096-chain launch)
#endif

// ---------------------------------------------------------------- one chunk
// light / heavy partition of a chunk by seed count (stable for the light reads: they keep their input order and locality)
__global__ void k_part_flags(const unsigned long long *seed_cnt, int n, unsigned int thr, unsigned int *flag)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = seed_cnt[i] < thr ? 1u : 0u;
}

__global__ void k_part_flags_nreg(const int *n_reg, int n, unsigned int *flag)
{   // 1 = at most one region: nothing to de-duplicate or patch, stays on the lane-per-read kernel
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = n_reg[i] <= 1 ? 1u : 0u;
}

__global__ void k_part_scatter(const unsigned int *flag, const unsigned int *pos, int n, int *light, int *heavy, unsigned int *counts)
{
    // (the heavy reads of a wave reserve their places with ONE atomic: with a read in five on the heavy side -- the multi-region partition -- a 16 M-read chunk sent
    // three million same-address atomics through one L2 channel, 2.7 ms a launch)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < n;
    const bool lt = in && flag[i] != 0;
    const bool hv = in && !lt;
    const unsigned long long m = __ballot(hv);
    unsigned int base = 0;
    if (m) {
        const int leader = __ffsll((long long)m) - 1;
        if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(counts + 1, (unsigned int)__popcll(m));
        base = (unsigned int)__shfl((int)base, leader);
    }
    if (lt) light[pos[i]] = i;
    if (hv) heavy[base + (unsigned int)__popcll(m & ((1ULL << (threadIdx.x & 63)) - 1ULL))] = i;
    if (in && i == n - 1) counts[0] = pos[i] + flag[i];
}

// The multi-region reads by region count, most regions first (64 bins, counts capped at 63) -- an experiment behind the knob "regs_sorted", off by default: the
// lane-per-read kernels that follow (k_regs, k_hits) run a wave for as long as its slowest lane and show one active lane in sixteen to forty, but binning the reads made
// them SLOWER (see slx_align_types.h): the low lane utilisation of these kernels is the price of spreading the heavy reads over many waves, which is what keeps them short.
// Counting sort in three small launches, no host round trip; the order inside a bin is whatever the atomics give.
template <typename K>
__global__ void __launch_bounds__(256) k_nreg_bin_count(const int *list, const unsigned int *n_list, const K *n_reg, unsigned int *bins)
{
    __shared__ unsigned int s[64];
    if (threadIdx.x < 64) s[threadIdx.x] = 0;
    __syncthreads();
    const unsigned int n = *n_list, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) { long long c = (long long)n_reg[list[t]]; c = c > 63 ? 63 : (c < 0 ? 0 : c); atomicAdd(&s[63 - (int)c], 1u); }
    __syncthreads();
    if (threadIdx.x < 64 && s[threadIdx.x]) atomicAdd(&bins[threadIdx.x], s[threadIdx.x]);
}
__global__ void k_nreg_bin_scan(unsigned int *bins)          // bins[64 + b] = where bin b starts (then its cursor)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) { unsigned int acc = 0; for (int b = 0; b < 64; ++b) { bins[64 + b] = acc; acc += bins[b]; } }
}
template <typename K>
__global__ void __launch_bounds__(256) k_nreg_bin_scatter(const int *list, const unsigned int *n_list, const K *n_reg, unsigned int *bins, int *out)
{
    __shared__ unsigned int s_cnt[64], s_base[64];
    if (threadIdx.x < 64) { s_cnt[threadIdx.x] = 0; s_base[threadIdx.x] = 0; }
    __syncthreads();
    const unsigned int n = *n_list, t = blockIdx.x * blockDim.x + threadIdx.x;
    int b = -1, r = 0;
    unsigned int my = 0;
    if (t < n) { r = list[t]; long long c = (long long)n_reg[r]; c = c > 63 ? 63 : (c < 0 ? 0 : c); b = 63 - (int)c; my = atomicAdd(&s_cnt[b], 1u); }
    __syncthreads();
    if (threadIdx.x < 64 && s_cnt[threadIdx.x]) s_base[threadIdx.x] = atomicAdd(&bins[64 + threadIdx.x], s_cnt[threadIdx.x]);
    __syncthreads();
    if (b >= 0) out[s_base[b] + my] = r;
}

__global__ void k_set_u32(unsigned int *p, unsigned int v) { *p = v; }
__global__ void k_or_u32(unsigned int *p, unsigned int v) { atomicOr(p, v); }

// extension jobs longest first: key = the job's read length (what its two extensions can run to), value = the job
__global__ void k_job_keys(const FirstJob *jobs, const unsigned int *list, unsigned int n, unsigned int *key, unsigned int *val)
{
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned int j = list ? list[i] : i;
    key[i] = (unsigned int)jobs[j].l_query; val[i] = j;
}

// runs f(std::integral_constant<int, MAXQ>) for the narrowest compiled MAXQ that holds the chunk's longest read
template <typename F>
static void with_maxq(int max_len, F f)
{
    if (max_len <= 160) f(std::integral_constant<int, 160>());
    else if (max_len <= 320) f(std::integral_constant<int, 320>());
    else f(std::integral_constant<int, 704>());
}
#define HUGE_BLOCKS 2048         // blocks of k_extend_reg on a chunk whose rows live in HBM (ck.huge_rows holds three rows for each)
#define MAXQ_LONG 8004          // columns of the H/E row k_extend_reg keeps in LDS for long reads; longer reads (up to SLX_MAX_READ_LEN) keep it in HBM

#ifdef EXT_STATS
static void ext_stats_print(hipStream_t st, const char *what, int n, const unsigned int *d_jobs)
{   // tuning build (-DEXT_STATS=1): what the extension kernels did since the last print
    unsigned long long a[8], b[8]; unsigned int nj = 0;
    (void)slx_wait_stream(st);
    (void)hipMemcpyFromSymbol(a, HIP_SYMBOL(g_ext_stats), sizeof a);
    if (d_jobs) (void)hipMemcpy(&nj, d_jobs, 4, hipMemcpyDeviceToHost);
    static unsigned long long prev[8];
    for (int i = 0; i < 8; ++i) { b[i] = a[i] - prev[i]; prev[i] = a[i]; }
    const double nd = (double)(b[0] - b[1] ? b[0] - b[1] : 1);
    fprintf(stderr, "[ext %s] %d reads, %u jobs: %llu extensions, %llu diagonal, DP mean qlen %.1f tlen %.1f rows %.1f band %.1f, %llu ended by the tail bound\n", what, n, nj,
            b[0], b[1], (double)b[2] / nd, (double)b[3] / nd, (double)b[4] / nd, b[4] ? (double)b[6] / (double)b[4] : 0., b[5]);
}
#endif

// the reads of a list / the CIGAR jobs of a list by size, for the same reason
__global__ void k_read_len_keys(const uint64_t *offs, const int *list, unsigned int n, unsigned int *key, unsigned int *val)
{
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = list[i];
    key[i] = (unsigned int)(offs[r + 1] - offs[r]); val[i] = (unsigned int)r;
}
// ... the jobs whose first band is wider than two columns per lane of a wave and that run for thousands of rows sort to the front and are counted:
// they take a block each (k_cig_band_block)
__global__ void k_cig_job_keys(const DJob *jobs, const uint32_t *list, unsigned int n, DevOpt dopt, unsigned int *key, unsigned int *val, unsigned int *n_big, int seg)
{
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = list[i];
    const DJob j = jobs[slot];
    const slx_opt &opt = dopt.o;
    const int lq = j.qe - j.qb, rlen = (int)(j.re - j.rb);
    int w2 = j.w2 < opt.w << 2 ? j.w2 : opt.w << 2;
    const int max_ins = (int)((double)(((lq + 1) >> 1) * opt.mat[0] - opt.o_ins) / opt.e_ins + 1.);
    const int max_del = (int)((double)(((lq + 1) >> 1) * opt.mat[0] - opt.o_del) / opt.e_del + 1.);
    int max_gap = max_ins > max_del ? max_ins : max_del;
    max_gap = max_gap > 1 ? max_gap : 1;
    const int dl = rlen - lq < 0 ? lq - rlen : rlen - lq;
    int ww = (max_gap + dl + 1) >> 1;
    ww = ww < w2 ? ww : w2;
    ww = ww > dl + 3 ? ww : dl + 3;
    // (seg: the long jobs' first band try runs in segments on blocks -- dev_cig_seg.h --, narrow bands included: a 300 kb contig's narrow-band CIGAR is as many rows as a wide one)
    const bool big = (2 * ww + 1 > 2 * WAVE || (seg && lq >= 4 * GSEG_LEN)) && lq >= 4096 && opt.e_ins > 0 && opt.e_del > 0;
    if (big) atomicAdd(n_big, 1u);
    key[i] = (big ? 0x80000000u : 0u) | ((unsigned int)lq & 0x7fffffffu); val[i] = slot;
}

static bool sort_keys_largest_first(Worker *wk, hipStream_t st, unsigned int n);

// (key, job) pairs of an extension job list sorted by descending read length into wk->job_val_out; false = no room, the list stays as it is
static bool sort_jobs_longest_first(Worker *wk, hipStream_t st, const FirstJob *jobs, const unsigned int *list, unsigned int n)
{
    if (wk->job_key_in.ensure((size_t)n * 4) != SLX_OK || wk->job_val_in.ensure((size_t)n * 4) != SLX_OK) return false;
    hipLaunchKernelGGL(k_job_keys, dim3((n + 255) / 256), dim3(256), 0, st, jobs, list, n, wk->job_key_in.as<unsigned int>(), wk->job_val_in.as<unsigned int>());
    return sort_keys_largest_first(wk, st, n);
}

// wk->job_key_in / job_val_in [0, n) -> job_val_out in descending key order
static bool sort_keys_largest_first(Worker *wk, hipStream_t st, unsigned int n)
{
    if (wk->job_key_in.ensure((size_t)n * 4) != SLX_OK || wk->job_key_out.ensure((size_t)n * 4) != SLX_OK || wk->job_val_in.ensure((size_t)n * 4) != SLX_OK ||
        wk->job_val_out.ensure((size_t)n * 4) != SLX_OK) return false;
    size_t tb = 0;
    if (hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tb, wk->job_key_in.as<unsigned int>(), wk->job_key_out.as<unsigned int>(), wk->job_val_in.as<unsigned int>(),
                                                     wk->job_val_out.as<unsigned int>(), (int)n, 0, 32, st) != hipSuccess) return false;
    if (wk->job_sort_tmp.ensure(tb + 256) != SLX_OK) return false;
    return hipcub::DeviceRadixSort::SortPairsDescending(wk->job_sort_tmp.p, tb, wk->job_key_in.as<unsigned int>(), wk->job_key_out.as<unsigned int>(), wk->job_val_in.as<unsigned int>(),
                                                        wk->job_val_out.as<unsigned int>(), (int)n, 0, 32, st) == hipSuccess;
}

// The extension jobs of a batch of contigs with their long sides cut into segments (dev_ext_seg.h): plan (segments per side), the segments one block
// each, then the join one block per job.  false = not applicable (nothing long enough, or out of memory): the caller runs k_ext_block.
static bool launch_ext_jobs_seg(slx_aligner *al, Worker *wk, const Chunk &ck, const DevOpt &dopt, hipStream_t st, unsigned int n_jobs, const FirstJob *jobs, DReg *out,
                                const unsigned int *job_list, unsigned first_smem)
{
    if (!al->long_seg || n_jobs == 0) return false;
    if (wk->xseg_jobs.ensure((size_t)n_jobs * sizeof(XJob)) != SLX_OK || wk->xseg_state.ensure((size_t)n_jobs * sizeof(XState)) != SLX_OK || wk->xseg_cnt.ensure(64) != SLX_OK) return false;
    XPlan P;
    P.xjobs = wk->xseg_jobs.as<XJob>(); P.state = wk->xseg_state.as<XState>(); P.cnt = wk->xseg_cnt.as<unsigned int>(); P.fail_mod = al->xseg_fail;
    P.units = nullptr; P.out = nullptr; P.wrec = P.wout = P.scratch = nullptr;
    if (hipMemsetAsync(P.cnt, 0, 64, st) != hipSuccess) return false;
    const int g_join = std::max(1, std::min((int)std::min<unsigned int>(n_jobs, 1u << 30), HUGE_BLOCKS));
    size_t slots_have = 0;
    // once a pass has run, the jobs are half done: whatever goes wrong after that, the chunk fails loudly (the flags are read back after its last kernel)
    auto mid_pass_failure = [&]() { (void)hipGetLastError(); hipLaunchKernelGGL(k_or_u32, dim3(1), dim3(1), 0, st, ck.flags, (unsigned int)ERR_INTERNAL); (void)slx_wait_stream(st); };
    for (int pass = 0; pass < 3; ++pass) {          // first band tries; second tries of the sides that need one; those of right sides whose left side needed one
        P.pass = pass;
        (void)hipMemsetAsync(P.cnt + 1, 0, 12, st);          // units of this pass, the two queues
        (void)hipMemsetAsync(P.cnt + 8, 0, 4, st);
        hipLaunchKernelGGL(k_xseg_plan, dim3((n_jobs + 255) / 256), dim3(256), 0, st, ck, dopt, jobs, job_list, n_jobs, P);
        unsigned int h[2] = {0, 0};
        if (hipMemcpyAsync(h, P.cnt, 8, hipMemcpyDeviceToHost, st) != hipSuccess || slx_wait_stream(st) != hipSuccess) {
            if (pass == 0) return false;
            mid_pass_failure();
            return true;
        }
        if (pass == 0 && h[1] == 0) return false;
        // (later passes keep the segments of the earlier ones: a right side's first try is joined after its left side's second)
        if (wk->xseg_units.ensure((size_t)std::max(h[1], 1u) * sizeof(XUnit)) != SLX_OK || wk->xseg_out.grow((size_t)h[0] * sizeof(XSegOut), slots_have * sizeof(XSegOut), st) != SLX_OK ||
            wk->xseg_wrec.grow((size_t)h[0] * XSEG_WIN * 4, slots_have * XSEG_WIN * 4, st) != SLX_OK || wk->xseg_wout.grow((size_t)h[0] * XSEG_WIN * 4, slots_have * XSEG_WIN * 4, st) != SLX_OK ||
            wk->xseg_scratch.ensure((size_t)g_join * XSEG_WIN * 4) != SLX_OK) {
            (void)hipGetLastError();
            if (pass == 0) return false;
            mid_pass_failure();
            return true;
        }
        slots_have = h[0];
        P.units = wk->xseg_units.as<XUnit>(); P.out = wk->xseg_out.as<XSegOut>(); P.wrec = wk->xseg_wrec.as<int>(); P.wout = wk->xseg_wout.as<int>(); P.scratch = wk->xseg_scratch.as<int>();
        if (h[1]) {
            hipLaunchKernelGGL(k_xseg_units, dim3((n_jobs + 255) / 256), dim3(256), 0, st, n_jobs, P);
            if (al->xseg_wave_min > 0 && h[1] >= (unsigned int)al->xseg_wave_min)          // thousands of segments: one wave each (dev_ext_seg.h)
                hipLaunchKernelGGL(k_xseg_run_w, dim3(std::max(1, std::min((int)std::min<unsigned int>((h[1] + 3) / 4, 1u << 30), al->n_cu * 8))), dim3(XB_THREADS), 0, st, al->ref, ck, dopt, jobs, job_list, P, h[1]);
            else
            hipLaunchKernelGGL(k_xseg_run, dim3(std::max(1, std::min((int)std::min<unsigned int>(h[1], 1u << 30), al->n_cu * 8))), dim3(XB_THREADS), 0, st, al->ref, ck, dopt, jobs, job_list, P, h[1]);
        }
        hipLaunchKernelGGL(k_xseg_join, dim3(g_join), dim3(XB_THREADS), first_smem, st, al->ref, ck, dopt, jobs, out, job_list, n_jobs, P);
        unsigned int waiting = 0;
        if (hipMemcpyAsync(&waiting, P.cnt + 8, 4, hipMemcpyDeviceToHost, st) != hipSuccess || slx_wait_stream(st) != hipSuccess) { mid_pass_failure(); return true; }
        if (waiting == 0) break;
    }
    unsigned int stat[4] = {0, 0, 0, 0};
    if (hipMemcpyAsync(stat, P.cnt + 4, 16, hipMemcpyDeviceToHost, st) == hipSuccess && slx_wait_stream(st) == hipSuccess)
        for (int i = 0; i < 4; ++i) wk->xseg_stat[i] += stat[i];
    return true;
}

// extension -> regions -> CIGAR jobs -> hit sort/filter, over all reads of the chunk on the worker's stream
template <int MAXQ>
static void launch_tail(slx_aligner *al, Worker *wk, const Chunk &ck, const DevOpt &dopt, unsigned int *q, const unsigned int *n_slots, int grid, int bs, int n,
                        const int *ext_light, const int *ext_heavy, const unsigned int *n_heavy, const unsigned int *ext_slots,
                        const unsigned int *top_off = nullptr, unsigned int top_cap = 0, const DReg *top_tab = nullptr, bool predict = false)
{
    hipStream_t st = wk->stream;
    hipEvent_t *dbg = wk->dbg_ev;
    const bool dbg_on = getenv("SLX_DEBUG_SUB") != nullptr;
    if (dbg_on) (void)hipEventRecord(dbg[1], st);
    const int g = std::max(1, std::min(n, ck.huge_rows ? HUGE_BLOCKS : al->n_cu * 32));
    const unsigned ext_smem = (MAXQ > 704 && !ck.huge_rows) ? (unsigned)(3 * ck.long_stride * 4) : 0u;
    if (ext_heavy) hipLaunchKernelGGL(k_extend_reg<MAXQ>, dim3(g), dim3(64), ext_smem, st, al->ref, ck, dopt, ext_light, q + 1, ext_slots ? ext_slots : n_slots, 0,
                                      ext_heavy, n_heavy, top_off, top_cap, top_tab, ExtSpec(), al->walk_stage, q + 55);
    else {
        bool in_rounds = false;
        if constexpr (MAXQ > 704) {
            // contigs: rounds of (walk every unfinished read, collecting the seeds whose regions it lacks) + (those seeds one wave each); a
            // contig that ends in a tandem repeat needs dozens of full-length extensions that are serial only through the covered tests
            const size_t S1 = wk->last_S1;
            if (al->long_budget > 0 && (top_tab || predict) && top_off && S1 > 0 && wk->memo_idx.ensure(S1 * 4) == SLX_OK && wk->memo_jobs.ensure(S1 * sizeof(FirstJob)) == SLX_OK &&
                wk->memo_tab.ensure(S1 * sizeof(DReg)) == SLX_OK && wk->round_list.ensure(S1 * 4) == SLX_OK && wk->todo_a.ensure((size_t)n * 4 + 4) == SLX_OK &&
                wk->todo_b.ensure((size_t)n * 4 + 4) == SLX_OK && wk->spec_cnt.ensure(64) == SLX_OK) {
                in_rounds = true;
                unsigned int *cnt = wk->spec_cnt.as<unsigned int>();          // [0] jobs so far, [1] jobs of this round, [2] reads for the next round, [3] queue, [4] reads of this round
                (void)hipMemsetAsync(wk->memo_idx.p, 0xff, S1 * 4, st);
                (void)hipMemsetAsync(cnt, 0, 64, st);
                ExtSpec sp;
                sp.memo_idx = wk->memo_idx.as<int>(); sp.memo_jobs = wk->memo_jobs.as<FirstJob>(); sp.memo_tab = wk->memo_tab.as<DReg>();
                sp.n_jobs = cnt; sp.round_list = wk->round_list.as<unsigned int>(); sp.n_round = cnt + 1; sp.n_todo_next = cnt + 2; sp.budget = al->long_budget; sp.guess = al->long_guess;
                const int *todo = nullptr;
                int n_todo = n, round = 0;
                unsigned int jobs_total = 0;
                for (;; ++round) {
                    sp.todo_next = (round & 1 ? wk->todo_b : wk->todo_a).as<int>();
                    sp.predict = predict && round == 0;
                    (void)hipMemsetAsync(cnt + 1, 0, 12, st);
                    const int gw = std::max(1, std::min(n_todo, g));
                    hipLaunchKernelGGL(k_extend_reg<MAXQ>, dim3(gw), dim3(64), ext_smem, st, al->ref, ck, dopt, todo, cnt + 3, round ? cnt + 4 : n_slots, 0, (const int *)nullptr,
                                       (const unsigned int *)nullptr, top_off, top_cap, top_tab, sp);
                    unsigned int h[3] = {0, 0, 0};
                    if (hipMemcpyAsync(h, cnt, 12, hipMemcpyDeviceToHost, st) != hipSuccess || slx_wait_stream(st) != hipSuccess) break;   // (the caller's sync reports it)
                    if (h[1]) {
                        (void)hipMemsetAsync(cnt + 3, 0, 4, st);
                        const unsigned first_smem = ck.huge_rows ? 0u : (unsigned)(2 * ck.long_stride * 4);
                        // longest jobs first: the full-length extensions of the longest contig are the launch's critical path, and in the order
                        // the walks emitted them they could start last
                        if (h[1] > 1 && sort_jobs_longest_first(wk, st, wk->memo_jobs.as<FirstJob>(), wk->round_list.as<unsigned int>(), h[1]))
                            (void)hipMemcpyAsync(wk->round_list.p, wk->job_val_out.p, (size_t)h[1] * 4, hipMemcpyDeviceToDevice, st);
                        const int gj = std::max(1, std::min((int)std::min<unsigned int>(h[1], 1u << 30), ck.huge_rows ? HUGE_BLOCKS : al->n_cu * 8));
                        if (al->long_block && h[1] <= (unsigned int)al->long_block && launch_ext_jobs_seg(al, wk, ck, dopt, st, h[1], wk->memo_jobs.as<FirstJob>(), wk->memo_tab.as<DReg>(),
                                                                                                         wk->round_list.as<unsigned int>(), first_smem)) {}
                        else if (al->long_block && h[1] <= (unsigned int)al->long_block)       // few jobs, each tens of thousands of rows: four waves per job
                            hipLaunchKernelGGL(k_ext_block, dim3(std::max(1, std::min((int)h[1], HUGE_BLOCKS))), dim3(XB_THREADS), first_smem, st, al->ref, ck, dopt, top_off + n, top_cap,
                                               cnt + 3, wk->memo_jobs.as<FirstJob>(), wk->memo_tab.as<DReg>(), wk->round_list.as<unsigned int>(), cnt + 1);
                        else
                        hipLaunchKernelGGL(k_ext_first<MAXQ>, dim3(gj), dim3(64), first_smem, st, al->ref, ck, dopt, n, top_off, top_cap, cnt + 3, wk->memo_jobs.as<FirstJob>(),
                                           wk->memo_tab.as<DReg>(), wk->round_list.as<unsigned int>(), cnt + 1);
                    }
                    jobs_total = h[0];
                    if (h[2] == 0) break;
                    (void)hipMemcpyAsync(cnt + 4, cnt + 2, 4, hipMemcpyDeviceToDevice, st);
                    todo = sp.todo_next; n_todo = (int)h[2];
                }
                wk->long_rounds_run = round + 1; wk->long_jobs_run = jobs_total;
            }
        }
        if (!in_rounds)
            hipLaunchKernelGGL(k_extend_reg<MAXQ>, dim3(g), dim3(64), ext_smem, st, al->ref, ck, dopt, (const int *)nullptr, q + 1, n_slots, 0, (const int *)nullptr,
                               (const unsigned int *)nullptr, top_off, top_cap, top_tab, ExtSpec(), al->walk_stage, q + 55);
    }
#ifdef EXT_STATS
    ext_stats_print(st, "extend_reg", n, nullptr);
#endif
    if (al->keep_stages && wk->last_S1) {      // the region stage reuses ia[] and rewrites regs[] in place
        if (wk->snap_ia.ensure(wk->last_S1 * 4) == SLX_OK && wk->snap_regs.ensure(wk->last_S1 * sizeof(DReg)) == SLX_OK && wk->snap_nreg.ensure((size_t)n * 4) == SLX_OK) {
            (void)hipMemcpyAsync(wk->snap_ia.p, ck.ia, wk->last_S1 * 4, hipMemcpyDeviceToDevice, st);
            (void)hipMemcpyAsync(wk->snap_regs.p, ck.regs, wk->last_S1 * sizeof(DReg), hipMemcpyDeviceToDevice, st);
            (void)hipMemcpyAsync(wk->snap_nreg.p, ck.n_reg, (size_t)n * 4, hipMemcpyDeviceToDevice, st);
        }
    }
    (void)hipEventRecord(wk->ev[5], st);
    (void)hipEventRecord(wk->ev_probe[3], st);
    if (dbg_on) (void)hipEventRecord(dbg[2], st);
    FinLists fl;
    fl.jobs = wk->jobs.as<DJob>();
    fl.fast_list = wk->fast_list.as<uint32_t>();
    fl.dp_list = wk->dp_list.as<uint32_t>();
    fl.n_fast = q + 4; fl.n_dp = q + 5; fl.q_dp = q + 6;
    // DP jobs with a narrow band one lane per job (k_cig_lanes): 16-bit rows need small scores
    bool cig_lanes = al->cig_lanes && MAXQ <= 704 && n >= 256;          // (a handful of reads: a lane per job leaves 63 lanes of its wave idle for the whole alignment -- 49 us for one read; the wave form takes 15)
    {
        int pen = std::max(std::max(dopt.o.e_del, dopt.o.e_ins), 1), amax = 0;
        for (int i = 0; i < 25; ++i) { pen = std::max(pen, -(int)dopt.o.mat[i]); amax = std::max(amax, (int)dopt.o.mat[i]); }
        if ((int64_t)(LANE_CIG_MAXQ + LANE_CIG_MAXT) * pen + dopt.o.o_del + dopt.o.o_ins >= LANE_FIN_LIMIT || (int64_t)amax * LANE_CIG_MAXQ >= LANE_FIN_LIMIT ||
            dopt.o.o_del < 0 || dopt.o.o_ins < 0 || dopt.o.e_del < 1 || dopt.o.e_ins < 1) cig_lanes = false;
    }
    fl.lane_list = cig_lanes ? wk->cig_lane_list.as<uint32_t>() : nullptr; fl.n_lane = q + 42;
    // reads with <= 1 region: straight-line kernel; the rest: many regions (low-complexity tracts) first, one wave each with the sorts
    // staged in LDS, the others one per lane.  order_in / order_out are free again after chaining + extension.
    unsigned int *cnt2 = q + 32;
    hipLaunchKernelGGL(k_part_flags_nreg, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ck.n_reg, n, wk->part_flag.as<unsigned int>());
    size_t tb = wk->scan_tmp.cap;
    (void)hipcub::DeviceScan::ExclusiveSum(wk->scan_tmp.p, tb, wk->part_flag.as<unsigned int>(), wk->part_pos.as<unsigned int>(), n, st);
    hipLaunchKernelGGL(k_part_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, wk->part_flag.as<unsigned int>(),
                       wk->part_pos.as<unsigned int>(), n, wk->order_in.as<int>(), wk->order_out.as<int>(), cnt2);
    hipLaunchKernelGGL(k_regs1, dim3(std::max(1, std::min(n / 256 + 1, al->n_cu * 8))), dim3(256), 0, st, ck, dopt, fl, wk->order_in.as<int>(), cnt2);
    int *multi = wk->order_out.as<int>();          // the multi-region reads: in list order, or (short reads) binned by region count, most regions first
    if constexpr (MAXQ <= 704) {
        if (al->regs_sorted && wk->order_bin.ensure((size_t)n * 4) == SLX_OK && wk->bin_cnt.ensure(512) == SLX_OK && hipMemsetAsync(wk->bin_cnt.p, 0, 512, st) == hipSuccess) {
            const dim3 gb((unsigned)((n + 255) / 256));
            unsigned int *bins = wk->bin_cnt.as<unsigned int>();
            hipLaunchKernelGGL(k_nreg_bin_count<int>, gb, dim3(256), 0, st, (const int *)wk->order_out.as<int>(), (const unsigned int *)(cnt2 + 1), (const int *)ck.n_reg, bins);
            hipLaunchKernelGGL(k_nreg_bin_scan, dim3(1), dim3(64), 0, st, bins);
            hipLaunchKernelGGL(k_nreg_bin_scatter<int>, gb, dim3(256), 0, st, (const int *)wk->order_out.as<int>(), (const unsigned int *)(cnt2 + 1), (const int *)ck.n_reg, bins, wk->order_bin.as<int>());
            multi = wk->order_bin.as<int>();
        } else (void)hipGetLastError();
    }
    if constexpr (MAXQ <= 704) {
        if (al->regs_big < (1 << 20)) {   // two launches: a 640-region LDS table at six waves per CU, then the few reads beyond it on the 2 048-region table
            const int mid = std::max(al->regs_big, REGS_MID_N);
            // each launch takes a list of its own reads (k_regs_pick; part_flag / part_pos are free since the scatter above), counts in queue words 64 / 65
            int *list_mid = wk->part_flag.as<int>(), *list_big = wk->part_pos.as<int>();
            hipLaunchKernelGGL(k_regs_pick, dim3(std::max(1, std::min(n / 256 + 1, al->n_cu * 8))), dim3(256), 0, st, (const int *)multi, (const unsigned int *)(cnt2 + 1), (const int *)ck.n_reg,
                               al->regs_big, al->regs_big <= REGS_MID_N ? REGS_MID_N : al->regs_big - 1, list_mid, q + 64, list_big, q + 65);
            if (al->regs_big <= REGS_MID_N)
                hipLaunchKernelGGL((k_regs_wave<MAXQ, REGS_MID_N>), dim3(std::max(1, std::min(n / 64 + 1, al->n_cu * 8))), dim3(64), 0, st, al->ref, ck, dopt, fl,
                                   (const int *)list_mid, q + 11, (const unsigned int *)(q + 64), al->regs_big, REGS_MID_N);
            if (mid < 512 || wk->max_seed_cnt > (unsigned int)mid)       // (regions <= seed occurrences; counts up to 512 are not tracked)
                hipLaunchKernelGGL((k_regs_wave<MAXQ, REGS_BIG_N>), dim3(std::max(1, std::min(n / 4096 + 1, al->n_cu))), dim3(64), 0, st, al->ref, ck, dopt, fl,
                                   (const int *)list_big, q + 15, (const unsigned int *)(q + 65), al->regs_big <= REGS_MID_N ? mid + 1 : al->regs_big, 1 << 30);
        }
        // the lane-per-read kernel hands the reads in which mem_patch_reg would run its alignment on to a wave-per-read launch (queue words 46 / 47)
        int *defer_list = (al->regs_defer && wk->defer_list.ensure((size_t)n * 4) == SLX_OK) ? wk->defer_list.as<int>() : nullptr;
        hipLaunchKernelGGL(k_regs<MAXQ>, dim3(ck.spread > 1 ? std::max(grid, (n + 1) / 2) : grid), dim3(bs), 0, st, al->ref, ck, dopt, fl, multi, q + 9, cnt2 + 1, ck.spread > 1 ? 1 : 0, al->regs_big,
                           defer_list, q + 46);
        if (defer_list)
            hipLaunchKernelGGL((k_regs_wave<MAXQ, REGS_SMALL_N>), dim3(std::max(1, std::min(n / 64 + 1, al->n_cu * 16))), dim3(64), 0, st, al->ref, ck, dopt, fl, (const int *)defer_list, q + 47,
                               (const unsigned int *)(q + 46), 0, 1 << 30);
    } else {   // long reads: every multi-region read one wave each, mem_patch_reg's contig-long alignment in band coordinates (dev_cig_band.h)
        // -- longest read first: the scratch rows bound the launch to a few waves, and the longest contig's patch alignments are its critical path
        unsigned int n_multi = 0;
        if (hipMemcpyAsync(&n_multi, cnt2 + 1, 4, hipMemcpyDeviceToHost, st) == hipSuccess && slx_wait_stream(st) == hipSuccess && n_multi > 1 &&
            wk->job_key_in.ensure((size_t)n_multi * 4) == SLX_OK && wk->job_val_in.ensure((size_t)n_multi * 4) == SLX_OK) {
            hipLaunchKernelGGL(k_read_len_keys, dim3((n_multi + 255) / 256), dim3(256), 0, st, ck.offs, (const int *)wk->order_out.as<int>(), n_multi, wk->job_key_in.as<unsigned int>(),
                               wk->job_val_in.as<unsigned int>());
            if (sort_keys_largest_first(wk, st, n_multi)) (void)hipMemcpyAsync(wk->order_out.p, wk->job_val_out.p, (size_t)n_multi * 4, hipMemcpyDeviceToDevice, st);
        }
        // mem_patch_reg's contig-long alignments ahead of the walk, in segments (dev_cig_seg.h: k_pseg_plan); the walk's scorer looks them up by their arguments
        PMemo pm; pm.jobs = nullptr; pm.off = pm.n = nullptr;
        if (al->long_seg && n_multi > 0) {
            const unsigned int job_cap = n_multi * PSEG_MAX_PAIRS;
            const unsigned int g_pj = (unsigned int)std::max(1, std::min((int)std::min<unsigned int>(job_cap, 1u << 20), al->n_cu * 4));
            if (wk->pseg_jobs.ensure((size_t)job_cap * sizeof(GJob)) == SLX_OK && wk->pseg_idx.ensure((size_t)n * 8 + 64) == SLX_OK && wk->pseg_cnt.ensure(64) == SLX_OK &&
                wk->gseg_scratch.ensure((size_t)g_pj * GSEG_WIN * 4) == SLX_OK && hipMemsetAsync(wk->pseg_cnt.p, 0, 64, st) == hipSuccess &&
                hipMemsetAsync(wk->pseg_idx.p, 0, (size_t)n * 8, st) == hipSuccess) {
                GPlan PP;
                PP.gjobs = wk->pseg_jobs.as<GJob>(); PP.units = nullptr; PP.wrec = PP.wout = nullptr; PP.scratch = wk->gseg_scratch.as<int>(); PP.cnt = wk->pseg_cnt.as<unsigned int>();
                PP.fail_mod = al->xseg_fail;
                int *memo_off = wk->pseg_idx.as<int>(), *memo_n = memo_off + n;
                hipLaunchKernelGGL(k_pseg_plan, dim3((n_multi + 255) / 256), dim3(256), 0, st, al->ref, ck, dopt, (const int *)wk->order_out.as<int>(), n_multi, PP, memo_off, memo_n, job_cap);
                unsigned int hp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                if (hipMemcpyAsync(hp, PP.cnt, 32, hipMemcpyDeviceToHost, st) == hipSuccess && slx_wait_stream(st) == hipSuccess && hp[7] > 0 && hp[7] <= job_cap &&
                    wk->gseg_units.ensure((size_t)std::max(hp[1], 1u) * sizeof(GUnit)) == SLX_OK && wk->gseg_wrec.ensure((size_t)std::max(hp[0], 1u) * GSEG_WIN * 4) == SLX_OK &&
                    wk->gseg_wout.ensure((size_t)std::max(hp[0], 1u) * GSEG_WIN * 4) == SLX_OK) {
                    PP.units = wk->gseg_units.as<GUnit>(); PP.wrec = wk->gseg_wrec.as<int>(); PP.wout = wk->gseg_wout.as<int>();
                    if (hp[1]) {
                        hipLaunchKernelGGL(k_gseg_units, dim3((hp[7] + 255) / 256), dim3(256), 0, st, (const unsigned int *)nullptr, hp[7], PP);
                        hipLaunchKernelGGL(k_gseg_run, dim3(std::max(1u, std::min(hp[1], (unsigned int)(al->n_cu * 8)))), dim3(GB_THREADS), 0, st, al->ref, ck, dopt, PP, hp[1]);
                    }
                    hipLaunchKernelGGL(k_pseg_join, dim3(std::min(g_pj, hp[7])), dim3(GB_THREADS), 0, st, al->ref, ck, dopt, PP, hp[7]);
                    pm.jobs = PP.gjobs; pm.off = memo_off; pm.n = memo_n;
                    wk->pseg_stat += hp[7];
                } else (void)hipGetLastError();
            } else (void)hipGetLastError();
        }
        hipLaunchKernelGGL((k_regs_wave_long<MAXQ, REGS_BIG_N>), dim3(std::max(1, std::min(n, ck.long_threads / 64))), dim3(GB_THREADS), 0, st, al->ref, ck, dopt, fl,
                           wk->order_out.as<int>(), q + 9, cnt2 + 1, pm);
    }
    if (dbg_on) (void)hipEventRecord(dbg[3], st);
    (void)hipEventRecord(wk->ev_probe[4], st);
    if (al->cig_fast_coop) hipLaunchKernelGGL(k_cig_fast_coop, dim3(std::max(1, std::min(n / 256 + 1, al->n_cu * 8))), dim3(256), 0, st, al->ref, ck, fl);
    else hipLaunchKernelGGL(k_cig_fast, dim3(std::max(1, std::min(n / 256 + 1, al->n_cu * 8))), dim3(256), 0, st, al->ref, ck, fl);
    if (cig_lanes) {
        if (al->cig_lane_il) hipLaunchKernelGGL(k_cig_lanes<true>, dim3(al->n_cu * 16), dim3(64), 0, st, al->ref, ck, dopt, fl, wk->cig_lane_list.as<uint32_t>(), q + 42, q + 43);
        else hipLaunchKernelGGL(k_cig_lanes<false>, dim3(al->n_cu * 16), dim3(64), 0, st, al->ref, ck, dopt, fl, wk->cig_lane_list.as<uint32_t>(), q + 42, q + 43);
    }
    if constexpr (MAXQ <= 704) hipLaunchKernelGGL(k_cig_dp<MAXQ>, dim3(g), dim3(64), 0, st, al->ref, ck, dopt, fl, 0);
    else {   // long reads: one wave per job in band coordinates; what it leaves (bands beyond its 832 columns) one lane per job
        FinLists rest = fl;
        rest.dp_list = wk->cig_lane_list.as<uint32_t>(); rest.n_dp = q + 42; rest.q_dp = q + 43;
        unsigned int n_dp_h = 0;                     // largest jobs first (a contig's CIGAR is one alignment of its whole length on one wave)
        if (hipMemcpyAsync(&n_dp_h, fl.n_dp, 4, hipMemcpyDeviceToHost, st) == hipSuccess && slx_wait_stream(st) == hipSuccess && n_dp_h > 1 &&
            wk->job_key_in.ensure((size_t)n_dp_h * 4) == SLX_OK && wk->job_val_in.ensure((size_t)n_dp_h * 4) == SLX_OK) {
            (void)hipMemsetAsync(q + 44, 0, 8, st);                    // [44] jobs for the block kernel, [45] its queue
            hipLaunchKernelGGL(k_cig_job_keys, dim3((n_dp_h + 255) / 256), dim3(256), 0, st, (const DJob *)fl.jobs, (const uint32_t *)fl.dp_list, n_dp_h, dopt, wk->job_key_in.as<unsigned int>(),
                               wk->job_val_in.as<unsigned int>(), q + 44, al->long_seg);
            if (sort_keys_largest_first(wk, st, n_dp_h)) {
                (void)hipMemcpyAsync(fl.dp_list, wk->job_val_out.p, (size_t)n_dp_h * 4, hipMemcpyDeviceToDevice, st);
                unsigned int n_big = 0;
                if (al->long_block && hipMemcpyAsync(&n_big, q + 44, 4, hipMemcpyDeviceToHost, st) == hipSuccess && slx_wait_stream(st) == hipSuccess && n_big) {
                    // wide-band jobs of thousands of rows: four waves per job, then the others on the wave kernel from where these end
                    // (and in the same launch the other jobs one wave each: dev_cig_seg.h)
                    const unsigned int bb = std::min(n_big, (unsigned int)(al->n_cu * 4));
                    const unsigned int wb = std::min((n_dp_h - std::min(n_dp_h, n_big) + 3) / 4, (unsigned int)(al->n_cu * 4));
                    // the first band try of the long jobs in segments that run side by side (dev_cig_seg.h): plan, segments, then the join inside the job's block
                    GPlan GP;
                    GP.gjobs = nullptr; GP.units = nullptr; GP.wrec = GP.wout = GP.scratch = nullptr; GP.cnt = nullptr; GP.fail_mod = al->xseg_fail;
                    if (al->long_seg && wk->gseg_jobs.ensure((size_t)n_big * sizeof(GJob)) == SLX_OK && wk->gseg_cnt.ensure(64) == SLX_OK &&
                        wk->gseg_scratch.ensure((size_t)(bb + wb) * GSEG_WIN * 4) == SLX_OK && hipMemsetAsync(wk->gseg_cnt.p, 0, 64, st) == hipSuccess) {
                        GP.gjobs = wk->gseg_jobs.as<GJob>(); GP.cnt = wk->gseg_cnt.as<unsigned int>(); GP.scratch = wk->gseg_scratch.as<int>();
                        (void)hipMemcpyAsync(GP.cnt + 8, ck.zused, 8, hipMemcpyDeviceToDevice, st);          // (the arena's top before the plan: restored if the cut is dropped)
                        hipLaunchKernelGGL(k_gseg_plan, dim3((n_big + 255) / 256), dim3(256), 0, st, al->ref, ck, dopt, fl, n_big, GP);
                        unsigned int hh[2] = {0, 0};
                        if (hipMemcpyAsync(hh, GP.cnt, 8, hipMemcpyDeviceToHost, st) != hipSuccess || slx_wait_stream(st) != hipSuccess) hh[1] = 0;
                        if (hh[1] && wk->gseg_units.ensure((size_t)hh[1] * sizeof(GUnit)) == SLX_OK && wk->gseg_wrec.ensure((size_t)hh[0] * GSEG_WIN * 4) == SLX_OK &&
                            wk->gseg_wout.ensure((size_t)hh[0] * GSEG_WIN * 4) == SLX_OK) {
                            GP.units = wk->gseg_units.as<GUnit>(); GP.wrec = wk->gseg_wrec.as<int>(); GP.wout = wk->gseg_wout.as<int>();
                            hipLaunchKernelGGL(k_gseg_units, dim3((n_big + 255) / 256), dim3(256), 0, st, (const unsigned int *)fl.n_dp, n_big, GP);
                            hipLaunchKernelGGL(k_gseg_run, dim3(std::max(1u, std::min(hh[1], (unsigned int)(al->n_cu * 8)))), dim3(GB_THREADS), 0, st, al->ref, ck, dopt, GP, hh[1]);
                        } else if (hh[1]) {
                            // no memory for the segments' windows (an allocation failure, not an arena overflow: a re-run with a larger arena would only fail the same way):
                            // the cut is dropped and the plan's traceback stretches -- the last reservations made, nothing ran since -- are handed back; the jobs run uncut
                            (void)hipGetLastError();
                            (void)hipMemcpyAsync(ck.zused, GP.cnt + 8, 8, hipMemcpyDeviceToDevice, st);
                            GP.gjobs = nullptr;
                        } else GP.gjobs = nullptr;
                    } else (void)hipGetLastError();
                    hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, st, fl.q_dp, n_big);
                    hipLaunchKernelGGL(k_cig_band_block, dim3(bb + wb), dim3(GB_THREADS), 0, st, al->ref, ck, dopt, fl, n_big, bb, q + 45,
                                       wk->cig_lane_list.as<uint32_t>(), q + 42, GP);
                    if (GP.gjobs) {
                        unsigned int stat[3] = {0, 0, 0};
                        if (hipMemcpyAsync(stat, GP.cnt + 4, 12, hipMemcpyDeviceToHost, st) == hipSuccess && slx_wait_stream(st) == hipSuccess)
                            for (int i = 0; i < 3; ++i) wk->gseg_stat[i] += stat[i];
                    }
                }
            }
        }
        hipLaunchKernelGGL(k_cig_band, dim3(std::max(1, std::min(n * 4, al->n_cu * 16))), dim3(64), 0, st, al->ref, ck, dopt, fl, wk->cig_lane_list.as<uint32_t>(), q + 42);
        hipLaunchKernelGGL(k_cig_long, dim3(grid), dim3(bs), 0, st, al->ref, ck, dopt, rest);
    }
    (void)hipEventRecord(wk->ev_probe[5], st);
    if (dbg_on) (void)hipEventRecord(dbg[4], st);
    // single-region reads are final already; the others: the glue's std::sort + secondary filters, or (SLX_F_REG2SAM) bwa's own selection
    if (ck.sam_mode) hipLaunchKernelGGL(k_hits_sam, dim3(grid), dim3(bs), 0, st, al->ref, ck, dopt, (const int *)multi, q + 3, q + 33);
    else {   // reads with many hits one wave each (queue words 48 / 49)
        int *big = (al->hits_wave && wk->hits_big.ensure((size_t)n * 4) == SLX_OK) ? wk->hits_big.as<int>() : nullptr;
        hipLaunchKernelGGL(k_hits, dim3(ck.spread > 1 ? std::max(grid, (n + 1) / 2) : grid), dim3(bs), 0, st, ck, (const int *)multi, q + 3, q + 33, ck.spread > 1 ? 1 : 0, big, q + 48);
        if (big) hipLaunchKernelGGL(k_hits_wave, dim3(std::max(1, std::min(n / 256 + 1, al->n_cu * 4))), dim3(64), 0, st, ck, (const int *)big, (const unsigned int *)(q + 48), q + 49);
    }
    if (dbg_on) (void)hipEventRecord(dbg[5], st);
}

struct CvtI32U64 { __host__ __device__ unsigned long long operator()(int v) const { return (unsigned long long)v; } };

// wave-cooperative chaining of the heavy list, then (a few blocks, normally nothing to do) the reads whose chains outgrew the LDS table
// Chaining of the reads on `order` (null: all of them), one lane per read: in LDS where the chunk allows it (dev_chain_lds.h: no per-seed
// scores, i.e. no long reads, and not one read per wave -- a small chunk's 64 slices would serve one lane each), with k_chain behind it
// for the reads the LDS pass leaves; else every read on k_chain.
template <typename I>
static void launch_chain(slx_aligner *al, Worker *wk, const Chunk &ck, const DevOpt &dopt, const DevFM<I> &fm, hipStream_t st, const int *order, unsigned int *q,
                         const unsigned int *n_slots, int n, int grid, int bs)
{
#ifndef SLX_WIDE
    if (al->chain_lds && !ck.s_score && ck.spread <= 1) {
        const size_t slice = LdsWS<I, CHAIN_LDS_SEEDS>::bytes();
        const int waves_cu = std::max(1, (int)((160u << 10) / slice));
        int *left = wk->chain_left.as<int>();        // (n entries: run_chunk)
        hipLaunchKernelGGL(k_chain_lds<I>, dim3(std::max(1, std::min(n / 64 + 1, al->n_cu * waves_cu))), dim3(64), slice, st, fm, al->ref, ck, dopt, order, q + 0, n_slots,
                           left, q + 52, q + 50);
        // (how many reads are left is known on the device only, so this launch has k_chain's usual grid: with nothing on the list every wave makes one fetch-add
        // and leaves.  The list is in the order the reads were given up, not the input order the light list has: results do not depend on the order, and the reads on it are all of the long kind, so a wave's lanes still hold reads of like weight.)
        hipLaunchKernelGGL(k_chain<I>, dim3(grid), dim3(bs), 0, st, fm, al->ref, ck, dopt, (const int *)left, q + 53, (const unsigned int *)(q + 52), 0);
        return;
    }
#endif
    hipLaunchKernelGGL(k_chain<I>, dim3(grid), dim3(bs), 0, st, fm, al->ref, ck, dopt, order, q + 0, n_slots, ck.spread > 1 ? 1 : 0);
}

template <typename I>
static void launch_coop(slx_aligner *al, Worker *wk, const Chunk &ck, const DevOpt &dopt, const DevFM<I> &fm, hipStream_t st, unsigned int *q,
                        unsigned int *counts, int n, bool both_tables = false)
{
    // first table: COOP_N1 chains per wave in LDS (33 bytes each).  The kernel is bound by the serial merge steps of single reads, so what
    // counts is how many reads are in flight: the table size sets the waves per CU (1 536 chains = 50 KB: three; 512 = 17 KB: nine)
    constexpr int N1 = COOP_N1;
    constexpr int WAVES_PER_CU = N1 <= 512 ? 8 : N1 <= 768 ? 6 : N1 <= 1024 ? 4 : 3;
    hipLaunchKernelGGL((k_chain_coop<I, N1, false>), dim3(std::max(1, std::min(n / 8 + 1, al->n_cu * WAVES_PER_CU))), dim3(64), 0, st, fm, al->ref, ck, dopt,
                       wk->order_out.as<int>(), q + 8, counts + 1, al->coop_lim1);
    // the 4 096-chain table only when a read can have more chains than the first table takes (chains <= seed occurrences): in the
    // pipeline an empty launch of it still waited ~20 ms for a CU with that much free LDS
    if (both_tables || std::min(N1, al->coop_lim1) < 512 || wk->max_seed_cnt > (unsigned int)std::min(N1, al->coop_lim1))     // (counts up to 512 are not tracked)
        hipLaunchKernelGGL((k_chain_coop<I, 4096, true>), dim3(std::max(1, std::min(n / 4096 + 1, N1 < 1536 ? al->n_cu : 16))), dim3(64), 0, st, fm, al->ref, ck, dopt,
                           wk->order_out.as<int>(), q + 10, counts + 1, al->coop_lim2);
}


// chunks of the production schedule (large, short reads) are the ones whose seeding launch fills the chip
static bool production_seed(const slx_aligner *al, int n, bool has_long) { return n >= al->split_min && !has_long; }

// runs the pipeline on reads [r0, r0+n) whose ASCII bases are d_ascii + d_offs[r0]...; appends to the outputs.
template <typename I>
static int run_chunk(slx_aligner *al, Worker *wk, const slx_opt *opt, const uint8_t *d_ascii, const uint64_t *d_offs, const uint64_t *h_offs_pair,
                     int64_t r0, int64_t part_lo, int n, int max_len, uint64_t rng_state, uint64_t first_ordinal, int hardclip, double ksf, int maxsec,
                     const ChunkCaps &caps, int64_t *hit_base, int64_t *cig_base, uint32_t *flags_out)
{
    hipStream_t st = wk->stream;
    int rc;
    const uint64_t base0 = h_offs_pair[0], n_bases = h_offs_pair[1] - h_offs_pair[0];
    const int bs = 128;
    // chunks holding a read long enough for bwa's seed filter (mem_flt_chained_seeds, live from ~727 bp) take the long-read path
    const bool has_long = max_len > 704 || flt_live(*opt, max_len, log((double)std::max(max_len, 1)), nullptr);
    int n_threads = (int)std::min<int64_t>(((int64_t)n + bs - 1) / bs * bs, (int64_t)(has_long ? std::min(al->max_threads, 16384) : al->max_threads));
    if (has_long) {   // the per-thread work lists and H/E rows grow with the longest read: at most ~8 GB of them per worker
        const int64_t per_thread = (int64_t)2 * (max_len + 1) * (int64_t)sizeof(IntvE<I>) + (int64_t)2 * (max_len + 8) * 4;
        const int64_t fit = std::max<int64_t>(bs, ((int64_t)8 << 30) / per_thread / bs * bs);
        n_threads = (int)std::min<int64_t>(n_threads, fit);
    }
    const int grid = n_threads / bs;
    // seeding launch: persistent waves fed from the queue, or ("seed_quota" > 0) waves that take a fixed share of the reads and leave
    int seed_grid = grid;
    uint32_t seed_quota = 0;
    if (al->seed_quota > 0 && !has_long && n >= al->split_min) {
        seed_quota = (uint32_t)((al->seed_quota + SEED_POOL - 1) / SEED_POOL * SEED_POOL);
        seed_grid = (int)(((int64_t)n + 2 * (int64_t)seed_quota - 1) / (2 * (int64_t)seed_quota));     // 128 lanes = two waves per block
        n_threads = std::max(n_threads, seed_grid * bs);                                              // (the work-list scratch is per launched thread)
    }
    // A small chunk of short reads (a per-read call, a shared round of concurrent callers): one read per WAVE through the lane-per-read kernels -- sixteen reads on sixteen
    // lanes of one wave walk their divergent paths one after another (seeding 441 us for sixteen reads against 152 us for one), on sixteen waves side by side.
    const int spread = (al->small_spread && n <= SMALL_SPREAD_MAX && n >= 2 && !has_long && n < al->split_min) ? 64 : 1;
    if (spread > 1) {
        seed_grid = std::max(seed_grid, (n + 1) / 2);                    // two waves per block, a read each
        n_threads = std::max(n_threads, seed_grid * bs);
    }
    const int cap_list = max_len + 1;
#define ENS(buf, bytes) if ((rc = wk->buf.ensure((size_t)(bytes))) != SLX_OK) return rc
    ENS(codes, n_bases + 16); ENS(offs_rel, ((size_t)n + 1) * 8);
    ENS(intv_n, (size_t)n * 4); ENS(intv_info, (size_t)n * caps.cap_intv * sizeof(qp_t)); ENS(intv_x0, (size_t)n * caps.cap_intv * sizeof(I));
    ENS(intv_x2, (size_t)n * caps.cap_intv * sizeof(I)); ENS(l_rep, (size_t)n * 4); ENS(seed_cnt, ((size_t)n + 1) * 8); ENS(seed_off, ((size_t)n + 1) * 8);
    ENS(n_chain, (size_t)n * 4); ENS(n_reg, (size_t)n * 4); ENS(n_hit, ((size_t)n + 1) * 4); ENS(na, (size_t)n * 4); ENS(frac_rep, (size_t)n * 4);
    ENS(lists, (size_t)2 * cap_list * n_threads * sizeof(IntvE<I>));
    ENS(zarena, caps.zcap); ENS(cigpool, caps.cigcap * 4);
    ENS(hit_cnt, ((size_t)n + 1) * 8); ENS(cig_cnt, ((size_t)n + 1) * 8); ENS(hit_off_c, ((size_t)n + 1) * 8); ENS(cig_off_c, ((size_t)n + 1) * 8);
    ENS(counters, 64); ENS(p2mask, (size_t)n * 8); ENS(p2list, (size_t)n * 4); ENS(p2items, (size_t)n * 4); ENS(p2long, (size_t)n * 4);
    // counters: [0] zused, [1] cigused, [2] flags(u32), then one u32 of site bits that raise no flag (OVS_Z_DP_WAVE, dev_types.h)
    HIPCHK(hipMemsetAsync(wk->counters.p, 0, 64, st));
    ENS(queues, 320);          // (80 words: 0..63 as numbered at their uses, 64 / 65 the lengths of the two many-region lists of k_regs_pick)
    HIPCHK(hipMemsetAsync(wk->queues.p, 0, 320, st));
    wk->first_lanes_ran = false;
    HIPCHK(hipMemsetAsync(wk->seed_cnt.as<unsigned long long>() + n, 0, 8, st));      // (k_seed_epi writes the count of every read; the scan takes n + 1 entries)

    Chunk ck;
    memset(&ck, 0, sizeof ck);
    ck.n_reads = n;
    ck.spread = spread;
    ck.codes = wk->codes.as<uint8_t>();
    ck.offs = wk->offs_rel.as<uint64_t>();
    ck.first_ordinal = first_ordinal + (uint64_t)r0;
    ck.rng_state = rng_state;
    ck.cap_intv = caps.cap_intv;
    ck.intv_n = wk->intv_n.as<uint32_t>(); ck.intv_info = wk->intv_info.as<uint32_t>();
    ck.intv_x0 = wk->intv_x0.p; ck.intv_x2 = wk->intv_x2.p;
    ck.l_rep = wk->l_rep.as<int32_t>();
    ck.seed_off = wk->seed_off.as<uint64_t>();
    ck.n_chain = wk->n_chain.as<int32_t>(); ck.n_reg = wk->n_reg.as<int32_t>(); ck.n_hit = wk->n_hit.as<int32_t>();
    ck.na = wk->na.as<int32_t>(); ck.frac_rep = wk->frac_rep.as<float>();
    ck.zarena = wk->zarena.as<uint8_t>(); ck.zcap = caps.zcap; ck.zused = wk->counters.as<unsigned long long>();
    ck.cigpool = wk->cigpool.as<uint32_t>(); ck.cigcap = caps.cigcap; ck.cigused = wk->counters.as<unsigned long long>() + 1;
    ck.flags = (uint32_t *)(wk->counters.as<unsigned long long>() + 2);
    ck.log_lut = al->d_loglut.as<double>(); ck.log_lut_n = SLX_LOG_LUT_N;
    ck.lists = wk->lists.p; ck.cap_list = cap_list; ck.n_threads = n_threads;
    ck.hardclip = hardclip; ck.keepSecFrac = ksf; ck.maxSecondary = maxsec;
    ck.sam_mode = (opt->flag & SLX_F_REG2SAM) ? 1 : 0;
    ck.seed_cnt = wk->seed_cnt.as<unsigned long long>();
    ck.ext_row_exit = al->ext_row_exit; ck.ext_exits = wk->queues.as<unsigned int>() + 56;          // [56] DPs the row exit ended (the extension kernels add to it)
    ck.wave_sort = al->wave_sort; ck.sort_cnt = wk->queues.as<unsigned int>() + 61;          // [61] staged region sorts that ended on the wave, [62] that fell back to one lane, [63] of those the sorts by region end; [66] / [67] hit sorts of k_hits_wave on the wave / on one lane (sort_cnt[5], [6])
    const bool production = al->chain_mode == 1 && n >= al->split_min && !has_long;
    const bool use_cand = al->cand_mode == 1 && production;
    if (use_cand) {
        ENS(cand, (size_t)al->cand_cap * sizeof(DReg)); ENS(cand_base, (size_t)n * 4); ENS(cand_cnt, ((size_t)n + 2) * 8); ENS(cand_off, ((size_t)n + 2) * 8);
        HIPCHK(hipMemsetAsync(wk->cand_base.p, 0xff, (size_t)n * 4, st));
        ck.cand = wk->cand.as<DReg>(); ck.cand_base = wk->cand_base.as<int32_t>();
    }
    if (getenv("SLX_DEBUG_CYC")) {
        ENS(dbg_cyc, (size_t)n * 32);
        HIPCHK(hipMemsetAsync(wk->dbg_cyc.p, 0, (size_t)n * 32, st));
        ck.dbg_cyc = wk->dbg_cyc.as<unsigned long long>();
        ck.dbg_stage = atoi(getenv("SLX_DEBUG_CYC"));
    }
    DevOpt dopt; dopt.o = *opt;
    DevFM<I> fm = fm_of<I>(al);
    // (the seeding kernels take "dense SA present" as leave to step through the pac instead of the index: not where the pac is not the indexed text -- that
    // index runs as with dense_sa = 0)
    fm.sa_dense = (al->dense_sa && al->have_dense && al->text_is_pac) ? al->d_sa_dense.as<I>() : nullptr;
    fm.rep = al->rep_mask ? al->d_rep.as<uint32_t>() : nullptr; fm.rep_mask = al->rep_mask; fm.rep_k = al->rep_k;
    // (a text position plus the flag bit must fit the index type: every u64 index, u32 indexes below 2^31 symbols)
    fm.bwd_direct = (al->bwd_direct && fm.sa_dense && (sizeof(I) == 8 || (uint64_t)fm.seq_len < (1ULL << 31))) ? 1 : 0;

    (void)hipEventRecord(wk->ev[0], st);
    {   // encode + relative offsets
        const unsigned g = (unsigned)std::min<uint64_t>((n_bases / 16 + 255) / 256 + 1, 65535u * 4);
        hipLaunchKernelGGL(k_encode, dim3(g), dim3(256), 0, st, d_ascii + base0, wk->codes.as<uint8_t>(), (size_t)n_bases);
        hipLaunchKernelGGL(k_rel_offsets, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, d_offs + r0, wk->offs_rel.as<uint64_t>(), n, base0);
    }
    (void)hipEventRecord(wk->ev[1], st);
    (void)hipEventRecord(wk->ev_probe[0], st);
    {
        hipStream_t ss = st;
        if (wk->seed_stream && production_seed(al, n, has_long)) {   // the CU-masked seeding stream: encode -> [seeding] -> scan
            ss = wk->seed_stream;
            HIPCHK(hipEventRecord(wk->ev_seed_in, st));
            HIPCHK(hipStreamWaitEvent(ss, wk->ev_seed_in, 0));
        }
        // passes 1 + 2 of mem_collect_intv: all SMEMs; then, one lane per read, which re-seeding calls can keep anything (repeat filter);
        // then those calls -- a few per cent of the reads
        unsigned int *qq = wk->queues.as<unsigned int>();
        hipLaunchKernelGGL((k_seed12m<I, 1>), dim3(seed_grid), dim3(bs), 0, ss, fm, al->ref, ck, dopt, qq + 29, seed_quota,
                           (const int *)nullptr, (const unsigned int *)nullptr, (const unsigned long long *)nullptr, (const uint32_t *)nullptr, (const unsigned int *)nullptr, 0u,
                           (uint32_t *)nullptr, (unsigned int *)nullptr, 0u);
        // pass-2 calls as single items (read << 6 | interval): at most one per read on average, else whole reads (k_seed2_select)
        const uint32_t cap_items = (al->p2_items && n < (1 << 26)) ? (uint32_t)(al->p2_items_cap > 0 ? std::min(al->p2_items_cap, n) : n) : 0u;
        const uint32_t cap_long = (cap_items && al->p2_coop) ? cap_items : 0u;
        hipLaunchKernelGGL(k_seed2_select<I>, dim3((unsigned)(((int64_t)n * spread + bs - 1) / bs)), dim3(bs), 0, ss, fm, ck, dopt, wk->p2mask.as<unsigned long long>(), wk->p2list.as<int>(), qq + 35,
                           wk->p2items.as<uint32_t>(), qq + 37, cap_items);
        hipLaunchKernelGGL((k_seed12m<I, 2>), dim3(grid), dim3(bs), 0, ss, fm, al->ref, ck, dopt, qq + 36, 0u, wk->p2list.as<int>(), qq + 35,
                           wk->p2mask.as<unsigned long long>(), wk->p2items.as<uint32_t>(), qq + 37, cap_items, wk->p2long.as<uint32_t>(), qq + 38, cap_long);
        // the calls inside repeats that the lanes put aside: one wave per call
        if (cap_long) hipLaunchKernelGGL(k_seed2_coop<I>, dim3((unsigned)(al->n_cu * 8)), dim3(64), 0, ss, fm, al->ref, ck, dopt, qq + 39, wk->p2long.as<uint32_t>(), qq + 38, cap_long);
        // pass 3: one lane per read -- and for the contigs of a long-read chunk one lane per POSITION, then the chain through the results
        const int seed3_par = (max_len > 8192 && al->long_seed3) ? 4096 : 0x7fffffff;
        hipLaunchKernelGGL(k_seed3m<I>, dim3((unsigned)(((int64_t)n * spread + bs - 1) / bs)), dim3(bs), 0, ss, fm, al->ref, ck, dopt, seed3_par);
        if (seed3_par != 0x7fffffff) {
            ENS(seed3_buf, (size_t)n_bases * sizeof(Seed3Next<I>));
            hipLaunchKernelGGL(k_seed3_next<I>, dim3((unsigned)((n_bases + 255) / 256)), dim3(256), 0, ss, fm, al->ref, ck, dopt, seed3_par, (uint64_t)n_bases, wk->seed3_buf.as<Seed3Next<I>>());
            hipLaunchKernelGGL(k_seed3_chase<I>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ss, ck, dopt, seed3_par, (const Seed3Next<I> *)wk->seed3_buf.as<Seed3Next<I>>());
        }
        hipLaunchKernelGGL(k_seed_epi<I>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ss, ck, dopt, wk->queues.as<unsigned int>() + 31,
                           (unsigned int)al->heavy_seeds, wk->queues.as<unsigned int>() + 34);
        if (ss != st) {
            HIPCHK(hipEventRecord(wk->ev_seed_out, ss));
            HIPCHK(hipStreamWaitEvent(st, wk->ev_seed_out, 0));
        }
    }
    (void)hipEventRecord(wk->ev_probe[1], st);
    (void)hipEventRecord(wk->ev[2], st);
    {   // exclusive scan of the per-read seed counts -> seed-slot regions
        size_t tmp_bytes = 0;
        hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, (unsigned long long *)wk->seed_cnt.p, (unsigned long long *)wk->seed_off.p, n + 1, st);
        ENS(scan_tmp, tmp_bytes + 256);
        HIPCHK(hipcub::DeviceScan::ExclusiveSum(wk->scan_tmp.p, tmp_bytes, (unsigned long long *)wk->seed_cnt.p, (unsigned long long *)wk->seed_off.p, n + 1, st));
    }
    // what the host sizes the next stages by, in one launch (k_mail, slx_align.hip): the number of seed slots, the chunk's flags, the largest seed-occurrence
    // count of a read (0: none above 512; bounds its chains and regions), the reads with at least heavy_seeds seed occurrences, pass 2's counters (queue words
    // 35..38: whole reads, (queue), items, items one wave each)
    {
        MailSpec ms{};
        ms.src[0] = (const unsigned int *)(wk->seed_off.as<uint64_t>() + n); ms.words[0] = 2;
        ms.src[1] = (const unsigned int *)ck.flags; ms.words[1] = 1;
        ms.src[2] = wk->queues.as<unsigned int>() + 31; ms.words[2] = 1;
        ms.src[3] = wk->queues.as<unsigned int>() + 34; ms.words[3] = 1;
        ms.src[4] = wk->queues.as<unsigned int>() + 35; ms.words[4] = 4;
        ms.n = 5;
        hipLaunchKernelGGL(k_mail, dim3(1), dim3(64), 0, st, ms, wk->h_mail);
    }
    HIPCHK(slx_wait_stream(st));
    unsigned long long S = 0;
    memcpy(&S, wk->h_mail, 8);
    const uint32_t fl0 = wk->h_mail[2];
    const unsigned int max_cnt = wk->h_mail[3], n_heavy_h = wk->h_mail[4];
    unsigned int n_p2_h = 0, n_long_h = 0, n_it_h = 0;          // reads whose pass 2 was run (SLX_DEBUG_SEED), those of them handed to k_seed2_coop, single calls on the item list
    unsigned int p2c[4] = {wk->h_mail[5], wk->h_mail[6], wk->h_mail[7], wk->h_mail[8]};
    n_p2_h = p2c[0]; n_it_h = p2c[2]; n_long_h = p2c[3];
    wk->cnt[0] += n_heavy_h; wk->cnt[1] += n_it_h; wk->cnt[2] += n_long_h; wk->cnt[3] += n_p2_h;
    if (getenv("SLX_DEBUG_SEED")) fprintf(stderr, "[seed] worker %d: %d reads, pass 2: %u single calls (%u of them one wave each) + %u whole reads (repeat filter k = %d), %u heavy\n", wk->id, n, n_it_h, n_long_h, n_p2_h, fm.rep ? fm.rep_k : 0, n_heavy_h);
    if (fl0) { *flags_out = fl0; return SLX_OK; }
    wk->max_seed_cnt = max_cnt;
    const size_t S1 = (size_t)S + 1;
    ENS(s_rbeg, S1 * 8); ENS(s_ql, S1 * sizeof(qp_t)); ENS(s_next, S1 * 4); ENS(c_pos, S1 * 8); ENS(c_head, S1 * 4); ENS(c_tail, S1 * 4);
    ENS(c_n, S1 * 4); ENS(c_rid, S1 * 4); ENS(c_w, S1 * 4); ENS(c_first, S1 * 4); ENS(c_kept, S1); ENS(ia, S1 * 4); ENS(ib, S1 * 4);
    ENS(ic, S1 * 4); ENS(srt, S1 * 8); ENS(regs, S1 * sizeof(DReg)); ENS(hits, S1 * sizeof(DHit));
    ENS(jobs, S1 * sizeof(DJob)); ENS(fast_list, S1 * 4); ENS(dp_list, S1 * 4); ENS(cig_lane_list, S1 * 4);
    ck.s_rbeg = wk->s_rbeg.as<int64_t>(); ck.s_ql = wk->s_ql.as<uint32_t>(); ck.s_next = wk->s_next.as<int32_t>();
    ck.c_pos = wk->c_pos.as<int64_t>(); ck.c_head = wk->c_head.as<int32_t>(); ck.c_tail = wk->c_tail.as<int32_t>();
    ck.c_n = wk->c_n.as<int32_t>(); ck.c_rid = wk->c_rid.as<int32_t>(); ck.c_w = wk->c_w.as<int32_t>();
    ck.c_first = wk->c_first.as<int32_t>(); ck.c_kept = wk->c_kept.as<int8_t>();
    ck.ia = wk->ia.as<int32_t>(); ck.ib = wk->ib.as<int32_t>(); ck.ic = wk->ic.as<int32_t>(); ck.srt = wk->srt.as<uint64_t>();
    ck.regs = wk->regs.as<DReg>(); ck.hits = wk->hits.as<DHit>();
    wk->last_S1 = S1;
    if (has_long) {   // per-seed scores (mem_seed_t::score) and the per-thread H/E rows of the lane-per-read alignment kernels
        ENS(s_score, S1 * 4); ENS(long_list, (size_t)n * 4);
        ck.s_score = wk->s_score.as<int32_t>();
        ck.long_stride = max_len + 8; ck.long_threads = n_threads;
        ENS(long_scratch, (size_t)n_threads * 2 * ck.long_stride * 4);
        ck.long_scratch = wk->long_scratch.as<int>();
        if (3 * (max_len + 8) * 4 > 64 * 1024) {          // three rows beyond 64 KB of LDS: in HBM
            ck.huge_stride = max_len + 8;
            ENS(huge_rows, (size_t)HUGE_BLOCKS * 3 * ck.huge_stride * 4);
            ck.huge_rows = wk->huge_rows.as<int>();
        }
    }
    (void)hipEventRecord(wk->ev[3], st);
    {
        unsigned int *q = wk->queues.as<unsigned int>();
        unsigned int *counts = q + 24;          // [0] light (or all) reads, [1] heavy reads
        ENS(part_flag, (size_t)n * 4); ENS(part_pos, (size_t)n * 4); ENS(order_in, (size_t)n * 4); ENS(order_out, (size_t)n * 4);
        if (al->chain_lds) ENS(chain_left, (size_t)n * 4);
        {   // scan_tmp must hold the scans of launch_tail / the partition below
            size_t tb = 0;
            HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, wk->part_flag.as<unsigned int>(), wk->part_pos.as<unsigned int>(), n + 1, st));
            ENS(scan_tmp, tb + 256);
        }
        const bool dbg_on = getenv("SLX_DEBUG_SUB") != nullptr;
        if (dbg_on) (void)hipEventRecord(wk->dbg_ev[0], st);
        const bool hsort = al->heavy_sorted && al->heavy_seeds <= 0xfffff;   // k_order_keys keeps 20 bits of the seed count
        if (!production) {
            // small batch (per-read calls) or a chunk with reads long enough for the seed filter: every read on the lane-per-read
            // chaining kernel, then the seed filter for the long ones, then every read on the wave-per-read extension kernel
            // ... and so does a heavy SHORT read of a small chunk (a per-read call, a shared round of concurrent callers): a read inside a repeat brings thousands of seed
            // occurrences, and on one lane its chaining took 15.7 ms -- one such read in sixty was more than half of the mean per-call time
            if ((max_len > 704 && al->long_coop) || (max_len <= 704 && al->small_coop && n_heavy_h > 0)) {
                // contigs carry thousands of seed occurrences each: on one lane per read (k_chain) the chaining of a hundred contigs kept
                // two waves busy for 200 ms.  They take the heavy reads' route -- one wave per read, the ordered chain set in LDS
                // (k_chain_coop) -- and the short reads of the chunk stay on lanes
                hipLaunchKernelGGL(k_part_flags, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, wk->seed_cnt.as<unsigned long long>(), n,
                                   (unsigned int)al->heavy_seeds, wk->part_flag.as<unsigned int>());
                size_t tb = wk->scan_tmp.cap;
                HIPCHK(hipcub::DeviceScan::ExclusiveSum(wk->scan_tmp.p, tb, wk->part_flag.as<unsigned int>(), wk->part_pos.as<unsigned int>(), n, st));
                hipLaunchKernelGGL(k_part_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, wk->part_flag.as<unsigned int>(),
                                   wk->part_pos.as<unsigned int>(), n, wk->order_in.as<int>(), wk->order_out.as<int>(), counts);
                launch_chain<I>(al, wk, ck, dopt, fm, st, wk->order_in.as<int>(), q, counts, n, spread > 1 ? seed_grid : grid, bs);
                launch_coop<I>(al, wk, ck, dopt, fm, st, q, counts, n, max_len > 704);
                hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, st, counts, (unsigned int)n);      // the stages below take every read in input order
            } else {
            hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, st, counts, (unsigned int)n);
            launch_chain<I>(al, wk, ck, dopt, fm, st, (const int *)nullptr, q, counts, n, spread > 1 ? seed_grid : grid, bs);
            }
            if (has_long) {   // mem_flt_chained_seeds
                hipLaunchKernelGGL(k_long_list, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ck, dopt, wk->long_list.as<int>(), q + 16);
                hipLaunchKernelGGL(k_flt_score, dim3((unsigned)std::min<int64_t>((int64_t)n * FLT_PARTS, 0x7fffffff)), dim3(64), 0, st, al->ref, ck, dopt, wk->long_list.as<int>(), q + 16);
                hipLaunchKernelGGL(k_flt_seeds, dim3(std::max(1, std::min(n, al->n_cu * 8))), dim3(64), 0, st, al->ref, ck, dopt, wk->long_list.as<int>(), q + 16, q + 17);
            }
            (void)hipEventRecord(wk->ev_probe[2], st);
            (void)hipEventRecord(wk->ev[4], st);
            if (max_len > 8192 && al->long_budget > 0 && al->long_predict) {
                // a batch of contigs, extension in rounds: no separate pass for the chains' top seeds -- the first walk takes them as jobs like any
                // other seed, GUESSES their regions (ExtSpec::predict) and so finds the seeds on other diagonals at once: the full-length
                // extensions of a contig that ends in a tandem repeat then all run in ONE launch instead of two (top seeds, then the rest)
                ENS(first_off, ((size_t)n + 2) * 4);
                HIPCHK(hipMemsetAsync(wk->first_off.p, 0, ((size_t)n + 2) * 4, st));
                launch_tail<MAXQ_LONG>(al, wk, ck, dopt, q, counts, grid, bs, n, nullptr, nullptr, nullptr, nullptr, wk->first_off.as<unsigned int>(), 0u, (const DReg *)nullptr, true);
            }
            else if (max_len > 704) {
                // contigs: the top (longest) seed of every kept chain extended ahead of time, one wave per CHAIN (k_ext_first), and taken from the
                // table by the per-read walk (k_extend_reg, top_reuse).  A contig that ends inside a tandem repeat keeps hundreds of chains on
                // shifted diagonals, and bwa extends the top seed of each across the whole contig (a gap of a few repeat units, then tens of
                // thousands of matching rows): on the read's own wave that walk took seconds for one contig
                const unsigned int top_cap = (unsigned int)std::min<uint64_t>((uint64_t)S1, 0x7fffffffu);
                ENS(first_tab, (size_t)top_cap * sizeof(DReg)); ENS(first_cnt, ((size_t)n + 2) * 4); ENS(first_off, ((size_t)n + 2) * 4);
                ENS(first_jobs, (size_t)top_cap * sizeof(FirstJob));
                HIPCHK(hipMemsetAsync(wk->first_cnt.p, 0, ((size_t)n + 2) * 4, st));
                hipLaunchKernelGGL(k_first_count, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ck, n, 0xffffffffu, wk->first_cnt.as<unsigned int>(), 0);
                size_t tb = wk->scan_tmp.cap;
                HIPCHK(hipcub::DeviceScan::ExclusiveSum(wk->scan_tmp.p, tb, wk->first_cnt.as<unsigned int>(), wk->first_off.as<unsigned int>(), n + 1, st));
                hipLaunchKernelGGL(k_first_prep, dim3(std::max(1, std::min(n / 128 + 1, al->n_cu * 12))), dim3(128), 0, st, al->ref, ck, dopt, n, wk->first_off.as<unsigned int>(),
                                   top_cap, wk->first_jobs.as<FirstJob>());
                const unsigned first_smem = ck.huge_rows ? 0u : (unsigned)(2 * ck.long_stride * 4);
                if (al->long_block && n <= al->long_block / 4 && max_len > 8192) {      // a batch of contigs: the top seeds four waves per job (dev_ext_block.h), longest first
                    unsigned int n_top_h = 0;
                    HIPCHK(hipMemcpyAsync(&n_top_h, wk->first_off.as<unsigned int>() + n, 4, hipMemcpyDeviceToHost, st));
                    HIPCHK(slx_wait_stream(st));
                    n_top_h = std::min(n_top_h, top_cap);
                    const bool sorted = n_top_h > 1 && sort_jobs_longest_first(wk, st, wk->first_jobs.as<FirstJob>(), nullptr, n_top_h);
                    if (n_top_h && launch_ext_jobs_seg(al, wk, ck, dopt, st, n_top_h, wk->first_jobs.as<FirstJob>(), wk->first_tab.as<DReg>(),
                                                       sorted ? (const unsigned int *)wk->job_val_out.as<unsigned int>() : (const unsigned int *)nullptr, first_smem)) {}
                    else
                    hipLaunchKernelGGL(k_ext_block, dim3(HUGE_BLOCKS), dim3(XB_THREADS), first_smem, st, al->ref, ck, dopt, wk->first_off.as<unsigned int>() + n, top_cap, q + 22,
                                       wk->first_jobs.as<FirstJob>(), wk->first_tab.as<DReg>(), sorted ? (const unsigned int *)wk->job_val_out.as<unsigned int>() : (const unsigned int *)nullptr,
                                       sorted ? (const unsigned int *)(wk->first_off.as<unsigned int>() + n) : (const unsigned int *)nullptr);
                }
                else
                hipLaunchKernelGGL(k_ext_first<MAXQ_LONG>, dim3(ck.huge_rows ? HUGE_BLOCKS : al->n_cu * 8), dim3(64), first_smem, st, al->ref, ck, dopt, n, wk->first_off.as<unsigned int>(),
                                   top_cap, q + 22, wk->first_jobs.as<FirstJob>(), wk->first_tab.as<DReg>(), (const unsigned int *)nullptr, (const unsigned int *)nullptr);
                launch_tail<MAXQ_LONG>(al, wk, ck, dopt, q, counts, grid, bs, n, nullptr, nullptr, nullptr, nullptr, wk->first_off.as<unsigned int>(), top_cap, wk->first_tab.as<DReg>());
            }
            else with_maxq(max_len, [&](auto mq) {
                launch_tail<decltype(mq)::value>(al, wk, ck, dopt, q, counts, grid, bs, n, nullptr, nullptr, nullptr, nullptr);
            });
        } else {
            // chaining: light reads one per lane, heavy reads one per wave (cooperative); everything after it over all reads in input order
            // partition: light reads (input order) -> order_in, heavy reads -> order_out, counts[0] / counts[1]
            hipLaunchKernelGGL(k_part_flags, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, wk->seed_cnt.as<unsigned long long>(), n,
                               (unsigned int)al->heavy_seeds, wk->part_flag.as<unsigned int>());
            size_t tb = wk->scan_tmp.cap;
            HIPCHK(hipcub::DeviceScan::ExclusiveSum(wk->scan_tmp.p, tb, wk->part_flag.as<unsigned int>(), wk->part_pos.as<unsigned int>(), n, st));
            hipLaunchKernelGGL(k_part_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, wk->part_flag.as<unsigned int>(),
                               wk->part_pos.as<unsigned int>(), n, wk->order_in.as<int>(), wk->order_out.as<int>(), counts);
            if (hsort && n_heavy_h > 1) {
                // heavy list heaviest-first.  Only that list is sorted (its size is known since the seeding sync): a few thousand to a few
                // ten thousand reads, not the chunk -- the radix sort of all 8 M read ids cost five launches of 1-7 ms each in the pipeline
                const unsigned int nh = n_heavy_h;
                ENS(order_key_in, (size_t)nh * 4); ENS(order_key_out, (size_t)nh * 4); ENS(order_tmp, (size_t)nh * 4);
                hipLaunchKernelGGL(k_heavy_keys, dim3((nh + 255) / 256), dim3(256), 0, st, wk->seed_cnt.as<unsigned long long>(), wk->order_out.as<int>(), nh,
                                   wk->order_key_in.as<unsigned int>());
                size_t tb2 = 0;
                HIPCHK(hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tb2, wk->order_key_in.as<unsigned int>(), wk->order_key_out.as<unsigned int>(),
                                                                    wk->order_out.as<int>(), wk->order_tmp.as<int>(), (int)nh, 0, 20, st));
                ENS(sort_tmp, tb2 + 256);
                HIPCHK(hipcub::DeviceRadixSort::SortPairsDescending(wk->sort_tmp.p, tb2, wk->order_key_in.as<unsigned int>(), wk->order_key_out.as<unsigned int>(),
                                                                    wk->order_out.as<int>(), wk->order_tmp.as<int>(), (int)nh, 0, 20, st));
                HIPCHK(hipMemcpyAsync(wk->order_out.p, wk->order_tmp.p, (size_t)nh * 4, hipMemcpyDeviceToDevice, st));
            }
            hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, st, counts + 2, (unsigned int)n);
            const int *light = wk->order_in.as<int>();
            if (al->chain_sorted && wk->order_bin.ensure((size_t)n * 4) == SLX_OK && wk->bin_cnt.ensure(512) == SLX_OK && hipMemsetAsync(wk->bin_cnt.p, 0, 512, st) == hipSuccess) {
                // experiment ("chain_sorted"): the light reads by seed-occurrence count, most first, so that the 64 lanes of a wave of k_chain hold reads of like size
                const dim3 gbn((unsigned)((n + 255) / 256));
                unsigned int *bins = wk->bin_cnt.as<unsigned int>();
                hipLaunchKernelGGL(k_nreg_bin_count<unsigned long long>, gbn, dim3(256), 0, st, light, (const unsigned int *)counts, (const unsigned long long *)wk->seed_cnt.as<unsigned long long>(), bins);
                hipLaunchKernelGGL(k_nreg_bin_scan, dim3(1), dim3(64), 0, st, bins);
                hipLaunchKernelGGL(k_nreg_bin_scatter<unsigned long long>, gbn, dim3(256), 0, st, light, (const unsigned int *)counts, (const unsigned long long *)wk->seed_cnt.as<unsigned long long>(), bins,
                                   wk->order_bin.as<int>());
                light = wk->order_bin.as<int>();
            } else (void)hipGetLastError();
            launch_chain<I>(al, wk, ck, dopt, fm, st, light, q, counts, n, grid, bs);
            launch_coop<I>(al, wk, ck, dopt, fm, st, q, counts, n);
            (void)hipEventRecord(wk->ev_probe[2], st);
            if (use_cand) {
                const int nh = (int)n_heavy_h;                 // slots of these arrays are positions on the heavy list
                const unsigned gb = (unsigned)((nh + 255) / 256) + 1;
                HIPCHK(hipMemsetAsync(wk->cand_cnt.p, 0, ((size_t)nh + 2) * 8, st));
                unsigned int *slot_cnt = wk->cand_cnt.as<unsigned int>(), *job_cnt = slot_cnt + (nh + 2);
                unsigned int *slot_off = wk->cand_off.as<unsigned int>(), *job_off = slot_off + (nh + 2);
                // one lane per seed (k_ext_lanes): every heavy read is worth taking; it needs the H/E row of 64 extensions in LDS and 14-bit scores
                int amax = 0;
                for (int i = 0; i < 25; ++i) amax = std::max(amax, (int)opt->mat[i]);
                amax = std::max(amax, opt->a);                 // (a seed's score is its length x opt->a, whatever the matrix says)
                // -- and pays where the heavy reads' serial walk is a large part of a chunk's time, i.e. for small chunks (like cand_rep)
                const int lane_cols = max_len - std::min(opt->min_seed_len, max_len) + 2 + al->lane_pad;   // columns 0 .. longest extension query
                const bool lane_narrow = al->lane_narrow && amax * max_len < 256;      // 8-bit H / E cells: no score can reach 256
                const bool lanes = (al->cand_lanes > 0 || (al->cand_lanes < 0 && n <= CAND_REP_AUTO_READS)) && max_len <= 704 && (lane_narrow ? LaneNarrow::bytes(lane_cols) : LaneWide::bytes(lane_cols)) <= 64 * 1024 &&
                                   (int64_t)amax * max_len < LANE_SCORE_LIMIT;
                const int cand_rep = lanes ? 0 : (al->cand_rep >= 0 ? al->cand_rep : (n <= CAND_REP_AUTO_READS ? 75 : 0));
                for (int pass = cand_rep > 0 ? 1 : 0; pass >= 0; --pass)      // (first the count of partly repetitive reads, then the selection)
                    hipLaunchKernelGGL(k_cand_count, dim3(gb), dim3(256), 0, st, ck, wk->order_out.as<int>(), counts + 1, slot_cnt, job_cnt,
                                       (unsigned int)(lanes ? al->cand_lane_seeds : al->cand_seeds), (hsort && !lanes) ? (unsigned int)al->cand_top : 0xffffffffu,
                                       (unsigned int)cand_rep, q + 30, (unsigned int)al->cand_rep_max, pass, lanes ? 1 : CAND_PART);
                tb = wk->scan_tmp.cap;
                HIPCHK(hipcub::DeviceScan::ExclusiveSum(wk->scan_tmp.p, tb, slot_cnt, slot_off, nh + 1, st));
                hipLaunchKernelGGL(k_cand_base, dim3(gb), dim3(256), 0, st, wk->order_out.as<int>(), counts + 1, slot_off, (unsigned int)al->cand_cap,
                                   wk->cand_base.as<int32_t>(), job_cnt);
                tb = wk->scan_tmp.cap;
                HIPCHK(hipcub::DeviceScan::ExclusiveSum(wk->scan_tmp.p, tb, job_cnt, job_off, nh + 1, st));
                const int gc = al->n_cu * 32;
                if (lanes) {
                    const size_t max_jobs = std::min<size_t>((size_t)al->cand_cap, S1);      // (a job per seed slot of the selected reads, and those fit the table)
                    ENS(lane_jobs, max_jobs * sizeof(LaneJob));
                    auto go = [&](auto mq) {
                        constexpr int MAXQ = decltype(mq)::value;
                        hipLaunchKernelGGL(k_cand_lane_prep<MAXQ>, dim3(std::max(1, std::min(nh, al->n_cu * 16))), dim3(64), 0, st, al->ref, ck, dopt, wk->order_out.as<int>(), counts + 1,
                                           job_off, wk->lane_jobs.as<LaneJob>());
                        if (lane_narrow) hipLaunchKernelGGL(k_ext_lanes<LaneNarrow>, dim3(al->n_cu * 8), dim3(64), LaneNarrow::bytes(lane_cols), st, al->ref, ck, dopt, counts + 1, job_off,
                                                            q + 14, wk->lane_jobs.as<LaneJob>(), wk->cand.as<DReg>(), lane_cols);
                        else hipLaunchKernelGGL(k_ext_lanes<LaneWide>, dim3(al->n_cu * 4), dim3(64), LaneWide::bytes(lane_cols), st, al->ref, ck, dopt, counts + 1, job_off, q + 14,
                                                wk->lane_jobs.as<LaneJob>(), wk->cand.as<DReg>(), lane_cols);
                    };
                    with_maxq(max_len, go);
                } else
                with_maxq(max_len, [&](auto mq) {
                    hipLaunchKernelGGL(k_extend_cand<decltype(mq)::value>, dim3(gc), dim3(64), 0, st, al->ref, ck, dopt, wk->order_out.as<int>(), counts + 1,
                                       job_off, q + 14, wk->cand.as<DReg>());
                });
            }
            if (hsort && al->ext_split) {
                // light reads: top seed of every chain extended one wave per chain, decision sequence one read per lane; what is left
                // (reads needing another extension) joins the heavy reads in the wave-per-read kernel
                // the table takes one entry per kept chain: ~1.2 per light read, and the chains of the heavy reads (kept chains <= seed slots)
                const unsigned int top_cap = (unsigned int)std::min<uint64_t>((uint64_t)n + std::min<uint64_t>((uint64_t)S1, (uint64_t)n), 0x7fffffffu);
                ENS(first_tab, (size_t)top_cap * sizeof(DReg)); ENS(first_cnt, ((size_t)n + 2) * 4); ENS(first_off, ((size_t)n + 2) * 4); ENS(fb_list, (size_t)n * 4);
                unsigned int *n_fb = q + 20, *ext_tot = q + 21;
                HIPCHK(hipMemsetAsync(wk->first_cnt.p, 0, ((size_t)n + 2) * 4, st));
                hipLaunchKernelGGL(k_first_count, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ck, n, (unsigned int)al->heavy_seeds, wk->first_cnt.as<unsigned int>(),
                                   al->top_heavy);
                tb = wk->scan_tmp.cap;
                HIPCHK(hipcub::DeviceScan::ExclusiveSum(wk->scan_tmp.p, tb, wk->first_cnt.as<unsigned int>(), wk->first_off.as<unsigned int>(), n + 1, st));
                const int gf = al->n_cu * 32;
                ENS(first_jobs, (size_t)top_cap * sizeof(FirstJob));
                if (al->first_diag) ENS(first_dp, (size_t)top_cap * 4);
                // the jobs the diagonal does not answer: one LANE per job, binned by work (k_first_lanes, dev_ext_lane.h) where the rows of 64 extensions fit the LDS
                // and the scores the 14-bit (8-bit) cells, as for k_ext_lanes; else one wave per job (k_ext_first)
                int fl_amax = 0;
                for (int i = 0; i < 25; ++i) fl_amax = std::max(fl_amax, (int)opt->mat[i]);
                fl_amax = std::max(fl_amax, opt->a);
                const int fl_cols = max_len - std::min(opt->min_seed_len, max_len) + 2 + al->lane_pad;
                const bool fl_narrow = al->lane_narrow && fl_amax * max_len < 256;
                const bool first_lanes = al->first_lanes && al->first_diag && max_len <= 704 && (fl_narrow ? LaneNarrow::bytes(fl_cols) : LaneWide::bytes(fl_cols)) <= 64 * 1024 &&
                                         (int64_t)fl_amax * max_len < LANE_SCORE_LIMIT;
                // "ext_narrow": the bands go with the jobs (FirstJob::pad) wherever lanes run them; the jobs whose sides all have one get LaneRing rows and a launch
                // of their own where the 8-bit cells do (ring_cu: waves per CU that launch is sized for -- its 8.4 KB of LDS a wave would allow 19)
                const int narrow = first_lanes ? al->ext_narrow : 0;
                const bool ring = (narrow == 1 || narrow == 3) && fl_narrow;
                const int by_band = narrow == 1;          // (3: the narrow jobs binned by the wide launch's key, to measure the binning by itself)
                const int ring_cu = 16;
                if (first_lanes) {
                    ENS(first_sorted, (size_t)top_cap * 4); ENS(first_bins, 1024);
                    HIPCHK(hipMemsetAsync(wk->first_bins.p, 0, 1024, st));          // [0, 128): the DP jobs' classes and cursors, [128, 256): the narrow jobs'
                    if (ring) { ENS(first_nar, (size_t)top_cap * 4); ENS(first_nar_sorted, (size_t)top_cap * 4); }
                    wk->first_lanes_ran = true;
                }
                hipLaunchKernelGGL(k_first_prep, dim3(std::max(1, std::min(n / 128 + 1, al->n_cu * 12))), dim3(128), 0, st, al->ref, ck, dopt, n, wk->first_off.as<unsigned int>(),
                                   top_cap, wk->first_jobs.as<FirstJob>());
                with_maxq(max_len, [&](auto mq) {
                    constexpr int MAXQ = decltype(mq)::value;
                    if (al->first_diag) {   // what the diagonal answers, one lane per job; k_ext_first keeps the jobs that need the dynamic program
                        hipLaunchKernelGGL(k_first_diag, dim3((top_cap + 255) / 256), dim3(256), 0, st, al->ref, ck, dopt, n, wk->first_off.as<unsigned int>(), top_cap,
                                           wk->first_jobs.as<FirstJob>(), wk->first_tab.as<DReg>(), wk->first_dp.as<unsigned int>(), q + 40, narrow,
                                           ring ? wk->first_nar.as<unsigned int>() : (unsigned int *)nullptr, q + 58);          // [58] narrow jobs (the narrow list's length), [59] narrow sides, [60] the narrow launch's queue
                    }
                    if (first_lanes) {
                        unsigned int *bins = wk->first_bins.as<unsigned int>(), *sorted = wk->first_sorted.as<unsigned int>();
                        const FirstJob *fj = wk->first_jobs.as<FirstJob>();
                        hipLaunchKernelGGL(k_first_bin_count, dim3(al->n_cu * 4), dim3(256), 0, st, fj, (const unsigned int *)wk->first_dp.as<unsigned int>(), (const unsigned int *)(q + 40), max_len, bins, 0);
                        hipLaunchKernelGGL(k_first_bin_scan, dim3(1), dim3(1), 0, st, bins);
                        hipLaunchKernelGGL(k_first_bin_scatter, dim3(al->n_cu * 4), dim3(256), 0, st, fj, (const unsigned int *)wk->first_dp.as<unsigned int>(), (const unsigned int *)(q + 40), max_len, bins, sorted, 0);
                        if (fl_narrow) hipLaunchKernelGGL(k_first_lanes<LaneNarrow>, dim3(al->n_cu * 8), dim3(64), LaneNarrow::bytes(fl_cols), st, al->ref, ck, dopt, q + 22, fj, wk->first_tab.as<DReg>(),
                                                          (const unsigned int *)sorted, (const unsigned int *)(q + 40), fl_cols, q + 54);
                        else hipLaunchKernelGGL(k_first_lanes<LaneWide>, dim3(al->n_cu * 4), dim3(64), LaneWide::bytes(fl_cols), st, al->ref, ck, dopt, q + 22, fj, wk->first_tab.as<DReg>(),
                                                (const unsigned int *)sorted, (const unsigned int *)(q + 40), fl_cols, q + 54);
                        if (ring) {          // the narrow jobs: binned by bases x band width, 32 columns of cells per lane
                            const unsigned int *nar = wk->first_nar.as<unsigned int>();
                            unsigned int *nbins = bins + 128, *nsorted = wk->first_nar_sorted.as<unsigned int>();
                            hipLaunchKernelGGL(k_first_bin_count, dim3(al->n_cu * 4), dim3(256), 0, st, fj, nar, (const unsigned int *)(q + 58), max_len, nbins, by_band);
                            hipLaunchKernelGGL(k_first_bin_scan, dim3(1), dim3(1), 0, st, nbins);
                            hipLaunchKernelGGL(k_first_bin_scatter, dim3(al->n_cu * 4), dim3(256), 0, st, fj, nar, (const unsigned int *)(q + 58), max_len, nbins, nsorted, by_band);
                            hipLaunchKernelGGL(k_first_lanes<LaneRing>, dim3(al->n_cu * ring_cu), dim3(64), LaneRing::bytes(fl_cols), st, al->ref, ck, dopt, q + 60, fj, wk->first_tab.as<DReg>(),
                                               (const unsigned int *)nsorted, (const unsigned int *)(q + 58), fl_cols, q + 54);
                        }
                    } else
                    hipLaunchKernelGGL(k_ext_first<MAXQ>, dim3(gf), dim3(64), 0, st, al->ref, ck, dopt, n, wk->first_off.as<unsigned int>(), top_cap, q + 22,
                                       wk->first_jobs.as<FirstJob>(), wk->first_tab.as<DReg>(), al->first_diag ? wk->first_dp.as<unsigned int>() : (const unsigned int *)nullptr, q + 40);
#ifdef EXT_STATS
                    ext_stats_print(st, "cand + ext_first", n, wk->first_off.as<unsigned int>() + n);
#endif
                    hipLaunchKernelGGL(k_ext_replay<MAXQ>, dim3(grid), dim3(bs), 0, st, al->ref, ck, dopt, n, (unsigned int)al->heavy_seeds, wk->first_off.as<unsigned int>(),
                                       top_cap, wk->first_tab.as<DReg>(), q + 23, wk->fb_list.as<int>(), n_fb);
                });
                hipLaunchKernelGGL(k_add_u32, dim3(1), dim3(1), 0, st, counts + 1, n_fb, ext_tot);
                (void)hipEventRecord(wk->ev[4], st);
                with_maxq(max_len, [&](auto mq) {
                    launch_tail<decltype(mq)::value>(al, wk, ck, dopt, q, counts + 2, grid, bs, n, wk->fb_list.as<int>(), wk->order_out.as<int>(), counts + 1, ext_tot,
                                                     al->top_reuse ? wk->first_off.as<unsigned int>() : nullptr, top_cap, wk->first_tab.as<DReg>());
                });
            } else {
                (void)hipEventRecord(wk->ev[4], st);
                with_maxq(max_len, [&](auto mq) {
                    if (hsort) launch_tail<decltype(mq)::value>(al, wk, ck, dopt, q, counts + 2, grid, bs, n, wk->order_in.as<int>(), wk->order_out.as<int>(), counts + 1, nullptr);
                    else launch_tail<decltype(mq)::value>(al, wk, ck, dopt, q, counts + 2, grid, bs, n, nullptr, nullptr, nullptr, nullptr);
                });
            }
        }
    }
    (void)hipEventRecord(wk->ev[6], st);
    // hit / cigar counts -> offsets
    hipLaunchKernelGGL(k_hit_counts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ck, wk->cig_cnt.as<unsigned long long>());
    {
        hipcub::TransformInputIterator<unsigned long long, CvtI32U64, const int *> it(wk->n_hit.as<int>(), CvtI32U64());
        size_t tb = 0;
        hipcub::DeviceScan::ExclusiveSum(nullptr, tb, it, wk->hit_off_c.as<unsigned long long>(), n + 1, st);
        ENS(scan_tmp, tb + 256);
        HIPCHK(hipcub::DeviceScan::ExclusiveSum(wk->scan_tmp.p, tb, it, wk->hit_off_c.as<unsigned long long>(), n + 1, st));
        size_t tb2 = 0;
        hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, wk->cig_cnt.as<unsigned long long>(), wk->cig_off_c.as<unsigned long long>(), n + 1, st);
        ENS(scan_tmp, tb2 + 256);
        HIPCHK(hipcub::DeviceScan::ExclusiveSum(wk->scan_tmp.p, tb2, wk->cig_cnt.as<unsigned long long>(), wk->cig_off_c.as<unsigned long long>(), n + 1, st));
    }
    unsigned long long Hc = 0, Cc = 0;
    // the counters the host reads after the chunk, in one launch: every part gets its place in h_mail where it is added, so no reader counts words by hand
    int m_hits, m_cig, m_flags, m_defer, m_big, m_chain, m_walk, m_first = -1;
    {
        MailSpec ms{};
        int at = 0;
        auto part = [&](const unsigned int *src, int words) {
            if (ms.n >= SLX_MAIL_PARTS || at + words > 64) return -1;          // (h_mail holds 64 words)
            ms.src[ms.n] = src; ms.words[ms.n] = words; ++ms.n;
            at += words;
            return at - words;
        };
        m_hits = part((const unsigned int *)(wk->hit_off_c.as<unsigned long long>() + n), 2);
        m_cig = part((const unsigned int *)(wk->cig_off_c.as<unsigned long long>() + n), 2);
        m_flags = part((const unsigned int *)ck.flags, 1);
        m_defer = part(wk->queues.as<unsigned int>() + 46, 1);          // reads k_regs deferred to the wave kernel
        m_big = part(wk->queues.as<unsigned int>() + 48, 1);            // reads k_hits left to k_hits_wave
        m_chain = part(wk->queues.as<unsigned int>() + 50, 2);          // reads k_chain_lds started over on the HBM columns, reads it finished in LDS
        m_walk = part(wk->queues.as<unsigned int>() + 55, 13);          // chains k_extend_reg opened from a lane-made header, DPs the row exit ended, -, narrow jobs, narrow sides, (a queue), the region sorts' three counts, (two list lengths), the hit sorts' two counts
        if (wk->first_lanes_ran) m_first = part(wk->queues.as<unsigned int>() + 54, 1);          // jobs k_first_lanes counted as run
        if (m_hits < 0 || m_cig < 0 || m_flags < 0 || m_defer < 0 || m_big < 0 || m_chain < 0 || m_walk < 0 || (wk->first_lanes_ran && m_first < 0)) {
            slx_set_error("run_chunk: more counters than k_mail has parts (SLX_MAIL_PARTS)");
            return SLX_EINTERNAL;
        }
        hipLaunchKernelGGL(k_mail, dim3(1), dim3(64), 0, st, ms, wk->h_mail);
    }
    HIPCHK(slx_wait_stream(st));
    memcpy(&Hc, wk->h_mail + m_hits, 8); memcpy(&Cc, wk->h_mail + m_cig, 8);
    const uint32_t fl = wk->h_mail[m_flags];
    wk->fin_stat[0] += wk->h_mail[m_defer]; wk->fin_stat[1] += wk->h_mail[m_big];
    if (fl) { *flags_out = fl; return SLX_OK; }
    wk->chain_stat[0] += wk->h_mail[m_chain]; wk->chain_stat[1] += wk->h_mail[m_chain + 1];
    wk->walk_stat += wk->h_mail[m_walk];
    wk->exit_stat += wk->h_mail[m_walk + 1];
    wk->narrow_stat[0] += wk->h_mail[m_walk + 4]; wk->narrow_stat[1] += wk->h_mail[m_walk + 3];
    for (int i = 0; i < 3; ++i) wk->sort_stat[i] += wk->h_mail[m_walk + 6 + i];
    wk->sort_stat[3] += wk->h_mail[m_walk + 11]; wk->sort_stat[4] += wk->h_mail[m_walk + 12];
    if (m_first >= 0) wk->first_stat += wk->h_mail[m_first];
    // grow the outputs and compact
    const size_t H = (size_t)*hit_base + Hc, C = (size_t)*cig_base + Cc;
#define GROW(buf, bytes, keep) if ((rc = wk->buf.grow((size_t)(bytes), (size_t)(keep), st)) != SLX_OK) return rc
    GROW(o_rid, (H + 1) * 4, *hit_base * 4); GROW(o_pos, (H + 1) * 8, *hit_base * 8); GROW(o_flag, (H + 1) * 2, *hit_base * 2);
    GROW(o_mapq, (H + 1), *hit_base); GROW(o_score, (H + 1) * 4, *hit_base * 4); GROW(o_nm, (H + 1) * 4, *hit_base * 4);
    GROW(o_na, (H + 1) * 4, *hit_base * 4); GROW(o_ncig, (H + 1) * 4, *hit_base * 4); GROW(o_cig_off, (H + 2) * 8, *hit_base * 8);
    GROW(o_cigar, (C + 1) * 4, *cig_base * 4);
    if (ck.sam_mode) { GROW(o_xa, (H + 1) * 4, *hit_base * 4); GROW(o_sub, (H + 1) * 4, *hit_base * 4); }
    HitsSoA so;
    so.hit_off = wk->o_hit_off.as<int64_t>(); so.rid = wk->o_rid.as<int32_t>(); so.pos = wk->o_pos.as<int64_t>();
    so.flag = wk->o_flag.as<uint16_t>(); so.mapq = wk->o_mapq.as<uint8_t>(); so.score = wk->o_score.as<int32_t>();
    so.nm = wk->o_nm.as<int32_t>(); so.na = wk->o_na.as<int32_t>(); so.n_cigar_ops = wk->o_ncig.as<int32_t>();
    so.cig_off = wk->o_cig_off.as<int64_t>(); so.cigar = wk->o_cigar.as<uint32_t>();
    so.xa_parent = ck.sam_mode ? wk->o_xa.as<int32_t>() : nullptr; so.sub = ck.sam_mode ? wk->o_sub.as<int32_t>() : nullptr;
    hipLaunchKernelGGL(k_compact, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ck, wk->hit_off_c.as<unsigned long long>(),
                       wk->cig_off_c.as<unsigned long long>(), so, r0 - part_lo, *hit_base, *cig_base);
    (void)hipEventRecord(wk->ev[7], st);
    HIPCHK(hipGetLastError());
    HIPCHK(slx_wait_stream(st));
    for (int i = 0; i < 7; ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, wk->ev[i], wk->ev[i + 1]) == hipSuccess) wk->stage_ms[i] += ms;
    }
    for (int i = 0; i < 3; ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, wk->ev_probe[2 * i], wk->ev_probe[2 * i + 1]) == hipSuccess) wk->probe_ms[i] += ms;
    }
    {   // the groups between them, from events that are there already: chaining (start of the chain stage -> start of the extension group), the region
        // kernels (end of the extension group -> start of the CIGAR group), the hit sort + filters (end of the CIGAR group -> end of the finalize stage)
        hipEvent_t a[3] = {wk->ev[3], wk->ev_probe[3], wk->ev_probe[5]}, b[3] = {wk->ev_probe[2], wk->ev_probe[4], wk->ev[6]};
        for (int i = 0; i < 3; ++i) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, a[i], b[i]) == hipSuccess) wk->probe_ms[3 + i] += ms;
        }
    }
    if (ck.dbg_cyc && ck.dbg_stage == 3) {
        unsigned long long c6[32];
        HIPCHK(hipMemcpy(c6, wk->dbg_cyc.p, 256, hipMemcpyDeviceToHost));
        fprintf(stderr, "[seed12m] calls with min_intv <= 2: %llu, %.1f backward steps each; others: %llu, %.1f each; by length < 64 / < 256 / < 1024 / more: %llu (%.3g steps), %llu (%.3g), %llu (%.3g), %llu (%.3g); longest %llu\n",
                c6[16], c6[16] ? (double)c6[17] / (double)c6[16] : 0., c6[18], c6[18] ? (double)c6[19] / (double)c6[18] : 0., c6[20], (double)c6[21], c6[22], (double)c6[23], c6[24], (double)c6[25],
                c6[26], (double)c6[27], c6[30]);
        {
            std::vector<unsigned long long> life((size_t)grid * 2);
            HIPCHK(hipMemcpy(life.data(), wk->dbg_cyc.as<unsigned long long>() + 64, life.size() * 8, hipMemcpyDeviceToHost));
            std::vector<unsigned long long> lv;
            for (unsigned long long v : life) if (v) lv.push_back(v);
            std::sort(lv.begin(), lv.end());
            if (!lv.empty()) {
                fprintf(stderr, "[seed12m] wave lifetimes (cycle-counter ticks), %zu waves: min %.3g  p10 %.3g  p50 %.3g  p90 %.3g  p99 %.3g  max %.3g\n", lv.size(), (double)lv[0],
                        (double)lv[lv.size() / 10], (double)lv[lv.size() / 2], (double)lv[lv.size() * 9 / 10], (double)lv[lv.size() * 99 / 100], (double)lv.back());
            }
        }
        fprintf(stderr, "[seed12m] lanes per round by phase: fetch %.1f init %.1f start %.1f fwd %.1f dir %.1f row %.1f bwd %.1f done %.1f\n", (double)c6[8] / (double)c6[4],
                (double)c6[9] / (double)c6[4], (double)c6[10] / (double)c6[4], (double)c6[11] / (double)c6[4], (double)c6[12] / (double)c6[4], (double)c6[13] / (double)c6[4],
                (double)c6[14] / (double)c6[4], (double)c6[15] / (double)c6[4]);
        fprintf(stderr, "[seed12m] forward loop: %.4g wave-steps, %.1f lanes active; backward loop: %.4g wave-steps, %.1f lanes active; %.4g rounds, %.4g with events; direct loop: %.4g wave-steps (32 bases each), %.1f lanes active; %d reads\n",
                (double)c6[0], (double)c6[1] / (double)(c6[0] ? c6[0] : 1), (double)c6[2], (double)c6[3] / (double)(c6[2] ? c6[2] : 1), (double)c6[4], (double)c6[5], (double)c6[6], (double)c6[7] / (double)(c6[6] ? c6[6] : 1), n);
    } else if (ck.dbg_cyc) {   // the reads the extension kernel spent longest on
        std::vector<unsigned long long> cyc((size_t)n * 4), sc((size_t)n);
        std::vector<int> nch((size_t)n), nrg((size_t)n), lrep((size_t)n);
        HIPCHK(hipMemcpy(lrep.data(), wk->l_rep.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(cyc.data(), wk->dbg_cyc.p, (size_t)n * 32, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(sc.data(), wk->seed_cnt.p, (size_t)n * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(nch.data(), wk->n_chain.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(nrg.data(), wk->n_reg.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        std::vector<int> ord((size_t)n);
        for (int i = 0; i < n; ++i) ord[(size_t)i] = i;
        const int top = std::min(n, 12);
        std::partial_sort(ord.begin(), ord.begin() + top, ord.end(), [&](int a, int b) { return cyc[(size_t)a] > cyc[(size_t)b]; });
        unsigned long long tot = 0, tot_heavy = 0;
        unsigned long long ph[3] = {0, 0, 0};
        for (int i = 0; i < n; ++i) {
            tot += cyc[(size_t)i];
            if (sc[(size_t)i] >= (unsigned long long)al->heavy_seeds) tot_heavy += cyc[(size_t)i];
            for (int k = 0; k < 3; ++k) ph[k] += cyc[(size_t)(k + 1) * (size_t)n + (size_t)i];
        }
        float ext_ms = 0;
        (void)hipEventElapsedTime(&ext_ms, wk->ev[4], wk->ev[5]);
        fprintf(stderr, "[ext phases] sort %.3g  covered tests %.3g  extend+store %.3g ticks; extension stage %.1f ms\n", (double)ph[0], (double)ph[1], (double)ph[2], ext_ms);
        {
            const int lim[6] = {2, 8, 48, 128, 256, 640};
            for (int b = 0; b < 6; ++b) {
                long cnt = 0; unsigned long long cy = 0, a = 0, bb = 0, c = 0;
                for (int i = 0; i < n; ++i)
                    if (nrg[(size_t)i] >= lim[b] && (b == 5 || nrg[(size_t)i] < lim[b + 1])) {
                        ++cnt; cy += cyc[(size_t)i]; a += cyc[(size_t)n + i]; bb += cyc[2 * (size_t)n + i]; c += cyc[3 * (size_t)n + i];
                    }
                fprintf(stderr, "[regions >= %d] reads %ld  ticks %.3g (A %.3g B %.3g C %.3g)\n", lim[b], cnt, (double)cy, (double)a, (double)bb, (double)c);
            }
        }
        {
            const int lb[5] = {0, 1, 50, 100, 140};
            for (int b = 0; b < 5; ++b) {
                long cnt = 0; unsigned long long cy = 0;
                for (int i = 0; i < n; ++i)
                    if (nrg[(size_t)i] >= 256 && lrep[(size_t)i] >= lb[b] && (b == 4 || lrep[(size_t)i] < lb[b + 1])) { ++cnt; cy += cyc[(size_t)i]; }
                fprintf(stderr, "[>= 256 regions, l_rep >= %d] reads %ld  mean ticks %.3g\n", lb[b], cnt, cnt ? (double)cy / (double)cnt : 0.0);
            }
        }
        if (ck.dbg_stage == 2)
            fprintf(stderr, "[region sorts] wave_sort %d: on the wave %llu, one lane %llu (of those by region end %llu)\n", al->wave_sort, (unsigned long long)wk->h_mail[m_walk + 6],
                    (unsigned long long)wk->h_mail[m_walk + 7], (unsigned long long)wk->h_mail[m_walk + 8]);
        fprintf(stderr, "[ext cycles] n=%d total=%.3g (100 MHz ticks) heavy share=%.3f\n", n, (double)tot, tot ? (double)tot_heavy / (double)tot : 0.0);
        for (int i = 0; i < top; ++i) {
            const size_t r = (size_t)ord[(size_t)i];
            fprintf(stderr, "  read %zu: %.3g ticks (A %.3g, B %.3g, C %.3g; stage 1: sort, covered tests, extend+store; stage 2: sort by end, dedup/patch, second sort)  seeds=%llu chains=%d regions=%d l_rep=%d\n", r, (double)cyc[r],
                    (double)cyc[(size_t)n + r], (double)cyc[2 * (size_t)n + r], (double)cyc[3 * (size_t)n + r], sc[r], nch[r], nrg[r], lrep[r]);
        }
    }
    if (getenv("SLX_DEBUG_SUB")) {
        const char *nm[5] = {"chain", "extend", "regs", "cig", "hits"};
        fprintf(stderr, "[worker %d n=%d]", wk->id, n);
        for (int i = 0; i < 5; ++i) { float ms = -1; (void)hipEventElapsedTime(&ms, wk->dbg_ev[i], wk->dbg_ev[i + 1]); fprintf(stderr, " %s=%.1f", nm[i], ms); }
        float tot = -1; (void)hipEventElapsedTime(&tot, wk->dbg_ev[0], wk->dbg_ev[5]);
        fprintf(stderr, " total=%.1f\n", tot);
    }
    wk->last_ck = ck; wk->last_valid = true; wk->last_wide = sizeof(I) == 8;
    *hit_base += (int64_t)Hc;
    *cig_base += (int64_t)Cc;
    *flags_out = 0;
    return SLX_OK;
#undef ENS
#undef GROW
}
