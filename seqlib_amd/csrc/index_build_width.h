// index_build_width.h -- which of the two suffix sorters builds a text (host code only; tests/cpp/index_build_width_test.cpp compiles it alone).
// The 32-bit builder (slx_index_gpu.hip) hands its element count, the 2 * total symbols of forward ++ reverse complement plus the sentinel,
// to hipCUB's device sort and scan as an int: it is valid while that count fits one.  Everything larger -- from 1 073 741 824 bases of
// reference on -- goes to the 64-bit builder (slx_index_gpu64.hip), which sorts in pieces and is not bound by it.
#pragma once
#include <cstdint>

static inline bool slx_build32_fits(uint64_t total_bases)
{
    return total_bases <= (((uint64_t)INT32_MAX - 1) >> 1);          // 2 * total + 1 <= INT_MAX, without the overflow
}
