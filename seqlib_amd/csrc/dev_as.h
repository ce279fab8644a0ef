// dev_as.h -- pointers that carry their address space.
//
// A __shared__ array that reaches an out-of-line function through a plain `int *` is addressed with flat instructions there: the
// compiler cannot know that it is LDS.  A flat access counts on both the vector-memory and the LDS counter and may return out of
// order, so each one is followed by a full drain of everything in flight, the stores to HBM included.  With the address space in the
// pointer's type an LDS table is read with ds_ instructions that wait on their own counter only, and a column in HBM with global_
// instructions that an LDS read never waits for.  The kernels that keep a wave's tables in LDS and work on them out of line
// (dev_chain_coop.h, dev_fin.h) pass them as lds_ptr, and the HBM columns they touch in their loops as glb_ptr.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_wave.h"

template <typename T> using lds_ptr = __attribute__((address_space(3))) T *;
template <typename T> using glb_ptr = __attribute__((address_space(1))) T *;

// a generic pointer that is known to address HBM / LDS (the caller's claim: a wrong one reads the wrong memory)
template <typename T> __device__ __forceinline__ glb_ptr<T> as_glb(T *p) { return (glb_ptr<T>)p; }
template <typename T> __device__ __forceinline__ lds_ptr<T> as_lds(T *p) { return (lds_ptr<T>)p; }
// ... that is also the same in every lane of the wave: the base goes to scalar registers
template <typename T> __device__ __forceinline__ glb_ptr<T> as_glb_uniform(T *p) { return (glb_ptr<T>)rfl_u64((uint64_t)p); }
// a whole record out of HBM (the language has no copy of a struct across address spaces: eight bytes at a time, which the compiler widens)
template <typename T> __device__ __forceinline__ T glb_load(glb_ptr<const T> p)
{
    static_assert(sizeof(T) % 8 == 0 && alignof(T) >= 8, "glb_load: a record of 8-byte words");
    T v;
    uint64_t *d = (uint64_t *)&v;
    const glb_ptr<const uint64_t> s = (glb_ptr<const uint64_t>)p;
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / 8); ++k) d[k] = s[k];
    return v;
}

template <typename T> __device__ __forceinline__ lds_ptr<T> lds_uniform(lds_ptr<T> p)
{
    return (lds_ptr<T>)(uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)p);
}

// a value that is the same in every lane, pinned to a scalar register
__device__ __forceinline__ int rfl_i32(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float rfl_f32(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ int64_t rfl_i64(int64_t v) { return (int64_t)rfl_u64((uint64_t)v); }
