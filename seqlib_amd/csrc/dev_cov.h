// dev_cov.h -- the kernels of the coverage unit (slx_cov.hip launches them; cov_host.h has the per-record and per-position bodies).  The state is one int32 array
// over all contigs (cov_geo): a difference array while records are added (+1 at an interval's start, -1 at its end), depths once it is settled by an inclusive
// scan.  Every store to HBM is a plain store or an atomic from vector lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cov_host.h"
#include "slx_hip.h"

typedef unsigned long long cov_ull;

// device counters: an add's (slx_hip.h: SLX_ADD_*), then the bedGraph's runs
enum { COV_C_RUNS = SLX_ADD_N, COV_C_N };

// where the +-1 of an interval go: entries [A, A + W) of the array stand in LDS, the others in HBM
struct cov_sink {
    int32_t *arr, *lds;
    uint64_t A, W;
    const int64_t *beg, *off;
    uint32_t n_lds, n_global;
    __device__ __forceinline__ void add(uint64_t g, int v)
    {
        if (g - A < W) { atomicAdd(&lds[g - A], v); ++n_lds; }
        else { atomicAdd(&arr[g], v); ++n_global; }
    }
    __device__ __forceinline__ void operator()(int32_t tid, int64_t lo, int64_t hi)          // beg <= lo < hi <= end: both entries are the contig's
    {
        const uint64_t base = (uint64_t)(off[tid] - beg[tid]);
        add(base + (uint64_t)lo, 1);
        add(base + (uint64_t)hi, -1);
    }
};

// Block b takes records [b * slice, (b + 1) * slice), one lane per record.  lds_window > 0: the block keeps the lds_window entries from the first eligible
// record's start in LDS (dynamic shared memory, lds_window ints) and flushes the non-zero ones at its end.  Records with more than P.long_cigar ops go to
// long_list; the lowest index of a record whose fields pass its block_size goes to cnt[SLX_ADD_ERR].
__global__ __launch_bounds__(256) void k_cov_events(const uint8_t *s, uint64_t n_bytes, const cov_ull *rec_off, uint64_t n, cov_par P, cov_geo G, int32_t *arr, uint32_t slice,
                                                    uint32_t lds_window, cov_ull *long_list, cov_ull *cnt)
{
    extern __shared__ int32_t lds[];
    __shared__ cov_ull s_first;
    const uint64_t r0 = (uint64_t)blockIdx.x * slice, r1 = r0 + slice < n ? r0 + slice : n;
    cov_sink S = {arr, lds, 0, 0, G.beg, G.off, 0, 0};
    if (lds_window) {
        for (uint32_t i = threadIdx.x; i < lds_window; i += blockDim.x) lds[i] = 0;
        if (threadIdx.x == 0) s_first = ~0ull;
        __syncthreads();
        for (uint64_t k = r0 + threadIdx.x; k < r1; k += blockDim.x) {          // the first eligible record of the slice
            const uint64_t b = rec_off[k], e = rec_off[k + 1];
            rf_feat F;
            if (b <= e && e <= n_bytes && cov_head(s + b, e - b, P, G.n_ref, &F) > COV_R_SKIP) { atomicMin(&s_first, (cov_ull)k); break; }
        }
        __syncthreads();
        const uint64_t k = s_first;
        if (k != ~0ull) {
            const uint64_t b = rec_off[k];
            rf_feat F;
            (void)cov_head(s + b, rec_off[k + 1] - b, P, G.n_ref, &F);
            int64_t x = F.pos;
            if (x < G.beg[F.tid]) x = G.beg[F.tid];
            if (x > G.end[F.tid]) x = G.end[F.tid];
            S.A = (uint64_t)(G.off[F.tid] + x - G.beg[F.tid]);
            S.W = lds_window;
        }
    }
    uint32_t counted = 0;
    for (uint64_t k = r0 + threadIdx.x; k < r1; k += blockDim.x) {
        const uint64_t b = rec_off[k], e = rec_off[k + 1];
        rf_feat F;
        const int v = b <= e && e <= n_bytes ? cov_head(s + b, e - b, P, G.n_ref, &F) : COV_R_BAD;
        if (v == COV_R_BAD) atomicMin(&cnt[SLX_ADD_ERR], (cov_ull)k);
        else if (v == COV_R_LONG) long_list[atomicAdd(&cnt[SLX_ADD_NLONG], 1ull)] = k;
        else if (v == COV_R_COUNTED) { cov_record(F, P, G, 0u, 1u, lanes_one(), S); ++counted; }
    }
    if (lds_window) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < lds_window; i += blockDim.x) {          // coalesced: neighbouring lanes, neighbouring entries
            const int32_t v = lds[i];
            if (v && S.A + i < (uint64_t)G.total) atomicAdd(&arr[S.A + i], v);
        }
    }
    wave_count(&cnt[SLX_ADD_COUNTED], counted);
    wave_count(&cnt[SLX_ADD_LDS], S.n_lds);
    wave_count(&cnt[SLX_ADD_GLOBAL], S.n_global);
}

// one wave per record of long_list[0, m): ops 64 at a time, a block's start from the wave's prefix sum; global atomics only
__global__ __launch_bounds__(256) void k_cov_events_long(const uint8_t *s, const cov_ull *rec_off, const cov_ull *long_list, uint64_t m, cov_par P, cov_geo G, int32_t *arr, cov_ull *cnt)
{
    const uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= m) return;          // (whole waves leave)
    const uint64_t k = long_list[j], b = rec_off[k];
    rf_feat F;
    (void)cov_head(s + b, rec_off[k + 1] - b, P, G.n_ref, &F);          // (k_cov_events took it: the fields are inside the record)
    cov_sink S = {arr, nullptr, 0, 0, G.beg, G.off, 0, 0};
    cov_record(F, P, G, threadIdx.x & 63u, 64u, lanes_group<>(), S);
    wave_count(&cnt[SLX_ADD_COUNTED], (threadIdx.x & 63) == 0 ? 1u : 0u);
    wave_count(&cnt[SLX_ADD_GLOBAL], S.n_global);
}

// ---- settle (inclusive scan in place, hipCUB, chunk by chunk) and its inverse
__global__ void k_cov_carry(int32_t *arr, uint64_t at) { arr[at] += arr[at - 1]; }

// bound[j] = the last entry of tile j (1024 entries), read before k_cov_diff overwrites it
__global__ __launch_bounds__(256) void k_cov_tails(const int32_t *arr, uint64_t total, int32_t *bound)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, at = (j + 1) * 1024 - 1;
    if (at < total) bound[j] = arr[at];
}
// arr[i] = arr[i] - arr[i - 1] in place: a block reads its tile (and the entry in front of it from bound) before it writes any of it.  total is a multiple of 4.
__global__ __launch_bounds__(256) void k_cov_diff(int32_t *arr, uint64_t total, const int32_t *bound)
{
    const uint64_t at = (uint64_t)blockIdx.x * 1024 + 4ull * threadIdx.x;
    int4 v = {0, 0, 0, 0};
    int32_t prev = 0;
    if (at < total) {
        v = *(const int4 *)(arr + at);
        prev = threadIdx.x ? arr[at - 1] : blockIdx.x ? bound[blockIdx.x - 1] : 0;
    }
    __syncthreads();
    if (at < total) *(int4 *)(arr + at) = make_int4(v.x - prev, v.y - v.x, v.z - v.y, v.w - v.z);
}

// *out = max(*out, arr[g0 .. g1))
__global__ __launch_bounds__(256) void k_cov_max(const int32_t *arr, uint64_t g0, uint64_t g1, int32_t *out)
{
    int32_t m = INT32_MIN;
    for (uint64_t g = g0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < g1; g += (uint64_t)gridDim.x * blockDim.x) { const int32_t v = arr[g]; m = v > m ? v : m; }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0 && m != INT32_MIN) atomicMax(out, m);
}

// ---- region sums: one wave per item, an item is at most COV_REG_TILE entries [g0, g1) of region r; aligned 16-byte loads, the ends masked
#define COV_REG_TILE 65536ull
struct cov_item { uint64_t g0, g1; uint64_t r; };
__global__ __launch_bounds__(256) void k_cov_regions(const int32_t *arr, const cov_item *items, uint64_t n_items, int32_t min_depth, cov_ull *sum, cov_ull *n_at_least)
{
    const uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n_items) return;
    const cov_item it = items[j];
    int64_t s = 0;
    uint64_t c = 0;
    for (uint64_t q = (it.g0 >> 2) + (threadIdx.x & 63); 4 * q < it.g1; q += 64) {          // (the array's size is a multiple of 4: the whole vector is inside)
        const int4 v = *(const int4 *)(arr + 4 * q);
        const int32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint64_t g = 4 * q + i;
            if (g >= it.g0 && g < it.g1) { s += e[i]; c += e[i] >= min_depth; }
        }
    }
    s = (int64_t)wave_sum((uint64_t)s); c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) { if (s) atomicAdd(&sum[it.r], (cov_ull)s); if (c) atomicAdd(&n_at_least[it.r], (cov_ull)c); }
}

// ---- bedGraph: len[i] = bytes entry c0 + i gives (cov_bg_piece), len[m] = 0; then, with at = the exclusive sum of len, the text
__global__ __launch_bounds__(256) void k_cov_bg_len(const int32_t *arr, cov_geo G, cov_names N, uint64_t c0, uint64_t m, int include_zero, cov_ull *len, cov_ull *cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t head = 0;
    if (i < m) len[i] = cov_bg_piece(arr, G, N, c0 + i, include_zero, (uint8_t *)nullptr, &head);
    else if (i == m) len[i] = 0;
    wave_count(&cnt[COV_C_RUNS], head);
}
__global__ __launch_bounds__(256) void k_cov_bg_fill(const int32_t *arr, cov_geo G, cov_names N, uint64_t c0, uint64_t m, int include_zero, const cov_ull *at, uint8_t *text)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t head;
    if (i < m && at[i + 1] > at[i]) (void)cov_bg_piece(arr, G, N, c0 + i, include_zero, text + at[i], &head);
}
