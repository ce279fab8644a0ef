// dev_pile.h -- the kernels of the pileup unit (slx_pile.hip launches them; pile_host.h has the per-record and per-position bodies).  The state is 15 planes of
// int32 over one window, plane-major (entry plane * stride + pos - beg).  Every store to HBM is a plain store or an atomic from vector lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pile_host.h"
#include "slx_hip.h"
#include "seqlib_amd_pile.h"

typedef unsigned long long pile_ull;

// (the device counters of one add are slx_hip.h's SLX_ADD_*; the G lanes -- 16, 32 or 64, aligned in the wave -- that walk one record are a lanes_group<G>)

// where an event goes: positions [A, A + W) of every plane stand in LDS (plane-major, lstride entries a plane: a multiple of 32, so the bank of an entry is
// its position's whatever its plane, and the consecutive positions of a group's lanes fall on consecutive banks), the others in HBM
struct pile_sink {
    int32_t *arr, *lds;
    uint64_t stride;
    int64_t beg, A;
    uint32_t W, lstride, n_lds, n_global;
    __device__ __forceinline__ void operator()(uint32_t plane, int64_t x)          // beg <= x < end
    {
        const uint64_t d = (uint64_t)(x - A);
        if (d < W) { atomicAdd(&lds[plane * lstride + (uint32_t)d], 1); ++n_lds; }
        else { atomicAdd(&arr[plane * stride + (uint64_t)(x - beg)], 1); ++n_global; }
    }
};

// Block b (256 threads) takes records [b * slice, (b + 1) * slice), a group of G lanes per record.  lds_window > 0: the block keeps lds_window positions of all
// 15 planes from the first eligible record's start in LDS (dynamic shared memory, 15 * lstride ints) and flushes the non-zero entries at its end.  Long
// records go to long_list; the lowest index of a record whose fields pass its block_size goes to cnt[SLX_ADD_ERR].
template <int G> __global__ __launch_bounds__(256) void k_pile_events(const uint8_t *s, uint64_t n_bytes, const pile_ull *rec_off, uint64_t n, pile_par P, int32_t *arr, uint64_t stride,
                                                                      uint32_t slice, uint32_t lds_window, uint32_t lstride, pile_ull *long_list, pile_ull *cnt)
{
    extern __shared__ int32_t lds[];
    __shared__ pile_ull s_first;
    const uint64_t r0 = (uint64_t)blockIdx.x * slice, r1 = r0 + slice < n ? r0 + slice : n;
    pile_sink S = {arr, lds, stride, P.beg, 0, 0u, lstride, 0u, 0u};
    if (lds_window) {
        for (uint32_t i = threadIdx.x; i < PILE_PLANES * lstride; i += blockDim.x) lds[i] = 0;
        if (threadIdx.x == 0) s_first = ~0ull;
        __syncthreads();
        for (uint64_t k = r0 + threadIdx.x; k < r1; k += blockDim.x) {          // the first eligible record of the slice
            const uint64_t b = rec_off[k], e = rec_off[k + 1];
            rf_feat F;
            if (b <= e && e <= n_bytes && pile_head(s + b, e - b, P, &F) > PILE_R_SKIP) { atomicMin(&s_first, (pile_ull)k); break; }
        }
        __syncthreads();
        const uint64_t k = s_first;
        if (k != ~0ull) {
            const uint64_t b = rec_off[k];
            rf_feat F;
            (void)pile_head(s + b, rec_off[k + 1] - b, P, &F);
            int64_t x = F.pos;
            if (x < P.beg) x = P.beg;
            if (x > P.end) x = P.end;
            S.A = x;
            S.W = lds_window;
        }
    }
    const uint32_t lane = threadIdx.x & (G - 1);
    uint32_t counted = 0;
    for (uint64_t k = r0 + threadIdx.x / G; k < r1; k += 256 / G) {          // (uniform over the group)
        const uint64_t b = rec_off[k], e = rec_off[k + 1];
        rf_feat F;
        const int v = b <= e && e <= n_bytes ? pile_head(s + b, e - b, P, &F) : PILE_R_BAD;
        if (v == PILE_R_BAD) { if (lane == 0) atomicMin(&cnt[SLX_ADD_ERR], (pile_ull)k); }
        else if (v == PILE_R_LONG) { if (lane == 0) long_list[atomicAdd(&cnt[SLX_ADD_NLONG], 1ull)] = k; }
        else if (v == PILE_R_COUNTED) { pile_record(F, P, lane, (uint32_t)G, lanes_group<G>(), S); counted += lane == 0; }
    }
    if (lds_window) {
        __syncthreads();
        for (uint32_t p = 0; p < PILE_PLANES; ++p)
            for (uint32_t i = threadIdx.x; i < lds_window; i += blockDim.x) {          // coalesced: neighbouring lanes, neighbouring entries of one plane
                const int32_t v = lds[p * lstride + i];
                if (v && S.A + i < P.end) atomicAdd(&arr[p * stride + (uint64_t)(S.A + i - P.beg)], v);
            }
    }
    wave_count(&cnt[SLX_ADD_COUNTED], counted);
    wave_count(&cnt[SLX_ADD_LDS], S.n_lds);
    wave_count(&cnt[SLX_ADD_GLOBAL], S.n_global);
}

// one wave per record of long_list[0, m): ops 64 at a time, the bases of a block over the 64 lanes; global atomics only
__global__ __launch_bounds__(256) void k_pile_events_long(const uint8_t *s, const pile_ull *rec_off, const pile_ull *long_list, uint64_t m, pile_par P, int32_t *arr, uint64_t stride, pile_ull *cnt)
{
    const uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= m) return;          // (whole waves leave)
    const uint64_t k = long_list[j], b = rec_off[k];
    rf_feat F;
    (void)pile_head(s + b, rec_off[k + 1] - b, P, &F);          // (k_pile_events took it: the fields are inside the record)
    pile_sink S = {arr, nullptr, stride, P.beg, 0, 0u, 0u, 0u, 0u};
    pile_record(F, P, threadIdx.x & 63u, 64u, lanes_group<64>(), S);
    wave_count(&cnt[SLX_ADD_COUNTED], (threadIdx.x & 63) == 0 ? 1u : 0u);
    wave_count(&cnt[SLX_ADD_GLOBAL], S.n_global);
}

// ---- candidate sites.  A lane takes the four positions 4q .. 4q + 3 of the window: one 16-byte load per plane (the planes start on 16-byte boundaries and
// the stride is a multiple of 4), the four reference bytes, pile_site per position.  out == nullptr: the number of sites among them only.
__device__ __forceinline__ uint32_t pile_sites_of4(const int32_t *arr, uint64_t stride, uint64_t q, int64_t L, int64_t beg, const uint8_t *ref_at_beg, const pile_site_par &Q, slx_pile_site *out)
{
    int32_t e[PILE_PLANES][4];
#pragma unroll
    for (int k = 0; k < PILE_PLANES; ++k) {
        const int4 v = *(const int4 *)(arr + (uint64_t)k * stride + 4 * q);
        e[k][0] = v.x; e[k][1] = v.y; e[k][2] = v.z; e[k][3] = v.w;
    }
    uint32_t n = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t p = (int64_t)(4 * q) + i;
        if (p >= L) break;
        int32_t c[PILE_PLANES];
#pragma unroll
        for (int k = 0; k < PILE_PLANES; ++k) c[k] = e[k][i];
        pile_site_val V;
        if (!pile_site(c, ref_at_beg[p], Q, &V)) continue;
        if (out) {
            slx_pile_site *o = out + n;
            o->pos = beg + p; o->ref = V.ref; o->depth = V.depth; o->alt = V.alt; o->ins = V.ins; o->pad = 0;
#pragma unroll
            for (int k = 0; k < PILE_PLANES; ++k) o->plane[k] = c[k];
        }
        ++n;
    }
    return n;
}
// n4[q] = the sites among positions 4q .. 4q + 3 for q < nq, n4[nq] = 0
__global__ __launch_bounds__(256) void k_pile_site_flag(const int32_t *arr, uint64_t stride, uint64_t nq, int64_t L, int64_t beg, const uint8_t *bases, const pile_ull *contig_off, int64_t ref_tid,
                                                        pile_site_par Q, uint32_t *n4)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq) n4[q] = pile_sites_of4(arr, stride, q, L, beg, bases + contig_off[ref_tid] + beg, Q, nullptr);
    else if (q == nq) n4[q] = 0;
}
// with at = the exclusive sum of n4: the sites of positions 4q .. 4q + 3 to sites[at[q] ..], in ascending position
__global__ __launch_bounds__(256) void k_pile_site_fill(const int32_t *arr, uint64_t stride, uint64_t nq, int64_t L, int64_t beg, const uint8_t *bases, const pile_ull *contig_off, int64_t ref_tid,
                                                        pile_site_par Q, const uint32_t *at, slx_pile_site *sites)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq && at[q + 1] > at[q]) (void)pile_sites_of4(arr, stride, q, L, beg, bases + contig_off[ref_tid] + beg, Q, sites + at[q]);
}
