// dev_lanes.h -- what the lanes that call together share, in one place: sums, minima, maxima, exclusive prefix sums and broadcasts over a wave or an aligned
// group of its lanes, and the two shapes every record-batch unit ends a kernel with (one atomicAdd a wave for a counter, one atomicMin a wave for the lowest
// broken record).  (How a wave TAKES work from a counter is dev_wave.h's.)
//   lanes_one        lane 0 of 1: what the host-and-device bodies (cov_record, pile_record, samw_line) are given by the host and by a lane that walks alone
//   lanes_group<G>   the same members for G = 16, 32 or 64 aligned lanes of a wave; all G lanes call together.  Device only.
//   wave_*           the whole wave; all 64 lanes call together.  Device only.
// A value keeps the width its caller gives it: 32-bit values go through 32-bit shuffles, 64-bit values through two.  The casts the shuffles want are in here.
// All kernels run 1-D blocks of a multiple of 64 threads: threadIdx.x & 63 is the lane.  Compiles without HIP for the stand-alone host tests.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include <type_traits>
#define LANES_MEMBER __host__ __device__ __forceinline__
#else
#define LANES_MEMBER inline
#endif

struct lanes_one {
    LANES_MEMBER uint64_t sum(uint64_t v) const { return v; }
    LANES_MEMBER uint64_t min(uint64_t v) const { return v; }
    LANES_MEMBER uint64_t max(uint64_t v) const { return v; }
    LANES_MEMBER uint32_t scan(uint32_t v, uint32_t *total) const { *total = v; return 0; }          // exclusive
    LANES_MEMBER uint64_t scan(uint64_t v, uint64_t *total) const { *total = v; return 0; }
    LANES_MEMBER uint64_t bcast(uint64_t v, uint32_t) const { return v; }
};

#if defined(__HIPCC__)
// one shuffle of a 32- or 64-bit integer, G lanes wide
#define LANES_INT(T) static_assert(std::is_integral<T>::value && (sizeof(T) == 4 || sizeof(T) == 8), "a 32- or 64-bit integer")
template <class T> __device__ __forceinline__ T lanes_xor(T v, int o)
{
    LANES_INT(T);
    if constexpr (sizeof(T) == 4) return (T)__shfl_xor((int)v, o, 64);
    else return (T)__shfl_xor((unsigned long long)v, o, 64);
}
template <int G, class T> __device__ __forceinline__ T lanes_up(T v, unsigned int o)
{
    LANES_INT(T);
    if constexpr (sizeof(T) == 4) return (T)__shfl_up((int)v, o, G);
    else return (T)__shfl_up((unsigned long long)v, o, G);
}
template <int G, class T> __device__ __forceinline__ T lanes_get(T v, int j)
{
    LANES_INT(T);
    if constexpr (sizeof(T) == 4) return (T)__shfl((int)v, j, G);
    else return (T)__shfl((unsigned long long)v, j, G);
}

template <class T> __device__ __forceinline__ T wave_sum(T v) { for (int o = 32; o; o >>= 1) v += lanes_xor(v, o); return v; }
template <class T> __device__ __forceinline__ T wave_min(T v) { for (int o = 32; o; o >>= 1) { const T u = lanes_xor(v, o); v = u < v ? u : v; } return v; }
template <class T> __device__ __forceinline__ T wave_max(T v) { for (int o = 32; o; o >>= 1) { const T u = lanes_xor(v, o); v = u > v ? u : v; } return v; }

// v summed over the lanes of the group in front of this one; *total: over all of them
template <int G, class T> __device__ __forceinline__ T lanes_scan_excl(T v, T *total)
{
    const uint32_t lane = threadIdx.x & (G - 1);
    T x = v;
#pragma unroll
    for (uint32_t o = 1; o < G; o <<= 1) { const T y = lanes_up<G>(x, o); if (lane >= o) x += y; }
    *total = lanes_get<G>(x, G - 1);
    return x - v;
}
__device__ __forceinline__ uint32_t wave_scan_excl(uint32_t v, uint32_t *total) { return lanes_scan_excl<64>(v, total); }

// *ctr += v summed over the wave: one atomic, from lane 0, and none for a sum of 0.  A 32-bit counter takes a 32-bit sum, a 64-bit one a 64-bit sum.
__device__ __forceinline__ void wave_count(uint32_t *ctr, uint32_t v)
{
    const uint32_t s = wave_sum(v);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(ctr, s);
}
__device__ __forceinline__ void wave_count(unsigned long long *ctr, uint32_t v)
{
    const unsigned long long s = wave_sum((unsigned long long)v);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(ctr, s);
}
// *slot = min(*slot, v over the wave): one atomic, from lane 0, and none when every lane says ~0ull ("none")
__device__ __forceinline__ void wave_report_min(unsigned long long *slot, unsigned long long v)
{
    const unsigned long long m = wave_min(v);
    if ((threadIdx.x & 63) == 0 && m != ~0ull) atomicMin(slot, m);
}
// ... over the lanes that say `on` (the choice between v and "none" is made in here, behind the caller's control flow: a flag costs the caller fewer registers
// than a 64-bit value carried through its branches)
__device__ __forceinline__ void wave_report_min(unsigned long long *slot, bool on, unsigned long long v) { wave_report_min(slot, on ? v : ~0ull); }

template <int G = 64> struct lanes_group {
    static_assert(G == 16 || G == 32 || G == 64, "16, 32 or 64 aligned lanes");
    __device__ __forceinline__ uint64_t sum(uint64_t v) const { static_assert(G == 64, "the whole wave only"); return wave_sum(v); }
    __device__ __forceinline__ uint64_t min(uint64_t v) const { static_assert(G == 64, "the whole wave only"); return wave_min(v); }
    __device__ __forceinline__ uint64_t max(uint64_t v) const { static_assert(G == 64, "the whole wave only"); return wave_max(v); }
    __device__ __forceinline__ uint32_t scan(uint32_t v, uint32_t *total) const { return lanes_scan_excl<G>(v, total); }
    __device__ __forceinline__ uint64_t scan(uint64_t v, uint64_t *total) const { return lanes_scan_excl<G>(v, total); }
    __device__ __forceinline__ uint64_t bcast(uint64_t v, uint32_t j) const { return lanes_get<G>(v, (int)j); }
};
#endif
