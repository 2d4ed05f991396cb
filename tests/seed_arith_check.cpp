// seed_arith_check.cpp -- a stand-alone host program over chroma_amd/csrc/seed_common.h (tests/test_seed_arith.py builds and runs
// it): what the calls' coordinate ranges keep out of reach of the case sets.  The floor square root on (y^2 + 1)^2 - 1 -- the
// squared length of a difference (y^2, y, y), whose root lies just below an integer -- for every y up to the last below 2^53, the
// issue's 5791 and 5792 among them, and on n^2 - 1, n^2, n^2 + 1 and 2^53 - 1; the settling compares on estimates one beside
// the floor, which a correctly rounded square root never produces below 2^51; and how a batch is cut into launches of fewer than
// 2^32 threads.  Prints the first failure and returns 1, or "ok".
#include <stdint.h>
#include <stdio.h>

#include "seed_common.h"

static int failures = 0;

static void check_root(uint64_t D2)
{
    const uint64_t d = seed::isqrt_floor(D2);
    bool ok = d * d <= D2 && (d + 1) * (d + 1) > D2;
    for (int off = -1; off <= 1 && ok; off++)
        if (d + off + 1 >= 1) ok = seed::isqrt_settle(D2, d + off) == d;
    if (!ok && !failures++) printf("isqrt_floor(%llu) = %llu\n", (unsigned long long)D2, (unsigned long long)d);
}

static void check_cut(uint32_t groups, uint32_t limit, uint32_t want)
{
    const uint32_t got = seed::fits_a_launch(groups, limit);
    if ((got != want || (got > 1 && (uint64_t)got * groups > limit)) && !failures++) printf("fits_a_launch(%u, %u) = %u, not %u\n", groups, limit, got, want);
}

int main()
{
    const uint64_t top = (1ull << 53) - 1;
    for (uint64_t y = 0; (y * y + 1) * (y * y + 1) - 1 <= top; y++) check_root((y * y + 1) * (y * y + 1) - 1);
    for (uint64_t n = 1; n * n + 1 <= top; n = n < 4096 ? n + 1 : n + n / 1024 + 1)
        for (uint64_t D2 = n * n - 1; D2 <= n * n + 1; D2++) check_root(D2);
    for (uint64_t n = 94906265 - 2000; n <= 94906265; n++)          // (94906265^2 < 2^53 < 94906266^2)
        for (uint64_t D2 = n * n - 1; D2 <= n * n + 1 && D2 <= top; D2++) check_root(D2);
    check_root(0); check_root(top);
    // 512-thread blocks: 2^23 - 1 to a launch; the default seeder's 264 groups, a fine grid's 17 142, 2^20 candidates' 2^17
    const uint32_t most = seed::launch_blocks(512);
    if ((most != (1u << 23) - 1 || (uint64_t)most * 512 >= (1ull << 32) || (uint64_t)(most + 1) * 512 < (1ull << 32)) && !failures++)
        printf("launch_blocks(512) = %u\n", most);
    check_cut(264, most, 31775); check_cut(17142, most, 489); check_cut(1u << 17, most, 63); check_cut(1, most, most);
    check_cut(9, 8, 1); check_cut(9, 9, 1); check_cut(9, 40, 4); check_cut(1u << 17, 1, 1);
    if (!failures) printf("ok\n");
    return failures ? 1 : 0;
}
