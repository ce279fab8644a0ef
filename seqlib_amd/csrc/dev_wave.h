// dev_wave.h -- how a wave (or a block) takes work from a device-wide counter, in one place (what a wave's lanes compute together -- sums, minima, prefix
// sums -- is dev_lanes.h's).
//
// The idiom: ONE lane does the atomicAdd for the wave and the old value comes back to every lane through readfirstlane.
// The hazard: written as `if (lane == 0) slot = atomicAdd(queue, 1u); slot = readfirstlane(slot);` at the head of a persistent loop,
// the condition `lane == 0` is loop-invariant, and the compiler unswitched the loop of k_hits_wave (dev_fin2.h) on it: lanes 1..63 got a
// copy of the loop with no atomic in it, in which slot stays 0 and readfirstlane reads lane 1 -- the wave took item 0 for ever (that
// kernel's first version hung in the library and faulted in scripts/ubench/hits_wave_test.hip; profiles/NOTES_r06.md).  Whether the
// pass fires depends on the size of the loop body, so no site of that shape is safe because it happens to pass today.
// The guard: the lane number goes through an empty volatile asm AT THE TAKE.  A volatile asm is not hoisted out of the loop, so the
// predicate is not loop-invariant and there is nothing to unswitch on.  Every kernel takes its work through the helpers below.
//
// All kernels here run 1-D blocks of a multiple of 64 threads: threadIdx.x & 63 is the lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the lane number, opaque to the optimiser (__forceinline__: the asm has to land inside the caller's loop)
__device__ __forceinline__ unsigned int wave_lane()
{
    unsigned int l = threadIdx.x & 63;
    asm volatile("" : "+v"(l));
    return l;
}

// the first active lane's 64-bit word in every lane, pinned to scalar registers
__device__ __forceinline__ uint64_t rfl_u64(uint64_t v)
{
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32 | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// wave_take*: for a point the whole wave reaches together (lane 0 must be active).  Lane 0 adds n; ONE value, the counter's old one, for the wave.
__device__ __forceinline__ unsigned int wave_take(unsigned int *ctr, unsigned int n)
{
    unsigned int old = 0;
    if (wave_lane() == 0) old = atomicAdd(ctr, n);
    return (unsigned int)__builtin_amdgcn_readfirstlane((int)old);
}
__device__ __forceinline__ unsigned long long wave_take_u64(unsigned long long *ctr, unsigned long long n)
{
    unsigned long long old = 0;
    if (wave_lane() == 0) old = atomicAdd(ctr, n);
    return rfl_u64(old);
}

// block_take: the same for a block whose threads all reach it.  Thread 0 adds n; the old value goes to every thread through *s_slot (LDS), a barrier on either side.
__device__ __forceinline__ unsigned int block_tid()
{
    unsigned int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}
__device__ __forceinline__ unsigned int block_take(unsigned int *ctr, unsigned int n, unsigned int *s_slot)
{
    __syncthreads();
    if (block_tid() == 0) *s_slot = atomicAdd(ctr, n);
    __syncthreads();
    return *s_slot;
}

// wave_fetch_*: for whatever subset of the lanes arrives; ONE value PER LANE.  One atomic per wave instead of one per lane: the lanes that reach the
// call together share a single fetch-add on the wave-uniform counter and take consecutive values (the leader's rank comes from a ballot made at the
// call, so it is not loop-invariant).  3 M same-address atomics in a kernel otherwise serialise in one L2 channel (measured: 35 ms for a 3.3 M-read launch).
__device__ __forceinline__ uint32_t wave_fetch_inc(uint32_t *ctr)
{
    const unsigned long long m = __ballot(1);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    uint32_t base = 0;
    if (rank == 0) base = atomicAdd(ctr, (uint32_t)__popcll(m));
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)base) + rank;
}
__device__ __forceinline__ unsigned long long wave_fetch_add_u64(unsigned long long *ctr, unsigned long long each)
{
    const unsigned long long m = __ballot(1);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    unsigned long long base = 0;
    if (rank == 0) base = atomicAdd(ctr, each * (unsigned long long)__popcll(m));
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
    return (((unsigned long long)hi << 32) | lo) + each * rank;
}
