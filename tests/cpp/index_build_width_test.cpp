// The choice between the 32-bit and the 64-bit index builder (seqlib_amd/csrc/index_build_width.h) at its boundary: the 32-bit builder counts the 2 * total + 1
// suffixes of forward ++ reverse complement ++ sentinel in an int, so it is valid exactly while that number is <= INT_MAX.  Stated here a second way (128-bit
// arithmetic, no shifts) and checked around INT_MAX / 2, around 2^31 and 2^32, and at the ends of the range.
#include <climits>
#include <cstdint>
#include <cstdio>
#include "index_build_width.h"

static int failures = 0;

static void expect(uint64_t total, bool fits)
{
    const bool model = (unsigned __int128)total * 2 + 1 <= (unsigned __int128)INT_MAX;
    const bool got = slx_build32_fits(total);
    if (got != fits || model != fits) {
        printf("total %llu: predicate %d, model %d, expected %d\n", (unsigned long long)total, (int)got, (int)model, (int)fits);
        ++failures;
    }
    if (got) {          // what the builder then casts: the count as an int is the count
        const uint64_t n1 = total * 2 + 1;
        if ((int)n1 <= 0 || (uint64_t)(int)n1 != n1) { printf("total %llu: (int)n1 = %d\n", (unsigned long long)total, (int)n1); ++failures; }
    }
}

int main()
{
    const uint64_t half = (uint64_t)INT_MAX / 2;          // 1 073 741 823
    expect(0, true);
    expect(1, true);
    expect(half - 1, true);
    expect(half, true);                                    // 2 * total + 1 == INT_MAX
    expect(half + 1, false);                               // 2^30 bases: n1 = 2^31 + 1
    expect(half + 2, false);
    expect((1ULL << 31) - 1, false);
    expect(1ULL << 31, false);
    expect((1ULL << 31) + 1, false);
    expect((1ULL << 32) - 1, false);
    expect(1ULL << 32, false);
    expect(3100000000ULL, false);                          // a human genome
    expect((1ULL << 63) - 1, false);
    expect(1ULL << 63, false);                             // 2 * total wraps to 0 in 64 bits
    expect(UINT64_MAX, false);
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
