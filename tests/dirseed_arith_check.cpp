// dirseed_arith_check.cpp -- a stand-alone host program over chroma_amd/csrc/dirseed_common.h (tests/test_dirseed_arith.py builds
// and runs it, plainly and under the address and undefined-behaviour sanitizers): the truncating division trunc(x * 16384 / d)
// against plain int64 division -- every d a distance can be for numerators at the ends of their range, every x <= d for small d,
// where the quotient's estimate sits on its rounding boundaries (x * 16384 a multiple of d, one below, one above), and samples
// over the whole range in both signs; the int32 dot product and the clamp at the components' extremes against int64; the
// renormalisation bound |u_k| <= 16384 for every point with components within 40 and for sampled points up to 2^15; the cosine
// bin's range for every profile size.  Prints the first failure and returns 1, or "ok".
#include <stdint.h>
#include <stdio.h>

#include "dirseed_common.h"

static int failures = 0;

static void check_div(int64_t x, uint64_t d)
{
    const int64_t want = x * 16384 / (int64_t)d;
    const int32_t got = dirseed::q14_div(x, d);
    if (got != want && !failures++) printf("q14_div(%lld, %llu) = %d, not %lld\n", (long long)x, (unsigned long long)d, got, (long long)want);
}

static void check_cosine(int32_t nx, int32_t ny, int32_t nz, int32_t ux, int32_t uy, int32_t uz)
{
    int64_t want = ((int64_t)nx * ux + (int64_t)ny * uy + (int64_t)nz * uz) >> 14;
    want = want < -16384 ? -16384 : want > 16383 ? 16383 : want;
    const int32_t got = dirseed::cosine(nx, ny, nz, ux, uy, uz);
    if (got != want && !failures++) printf("cosine((%d, %d, %d), (%d, %d, %d)) = %d, not %lld\n", nx, ny, nz, ux, uy, uz, got, (long long)want);
    for (uint32_t m = 4; m <= 8; m++)
        if (dirseed::cos_bin(got, m) >= (1u << m) && !failures++) printf("cos_bin(%d, %u) = %u\n", got, m, dirseed::cos_bin(got, m));
}

static void check_point(int32_t ax, int32_t ay, int32_t az)
{
    int32_t u[3];
    dirseed::unit_of_point(ax, ay, az, &u[0], &u[1], &u[2]);
    const int64_t a[3] = {ax, ay, az}, L2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    int64_t L = 0;
    while ((L + 1) * (L + 1) <= L2) L += (L + 1 + 4096) * (L + 1 + 4096) <= L2 ? 4096 : 1;
    for (int k = 0; k < 3; k++) {
        const int64_t want = L ? a[k] * 16384 / L : 0;
        if ((u[k] != want || u[k] > 16384 || u[k] < -16384) && !failures++) printf("unit_of_point(%d, %d, %d)[%d] = %d, not %lld\n", ax, ay, az, k, u[k], (long long)want);
    }
}

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint64_t draw() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }

int main()
{
    // every distance: d = floor(sqrt(dx^2 + dy^2 + dz^2)) >= |dx|, differences within 2^24, so d < 2^25
    const int64_t ends[] = {1, (1 << 24) - 1, 1 << 24, 12345677, 5592405};
    for (int64_t x : ends)
        for (uint64_t d = (uint64_t)x; d < (1ull << 25); d++) check_div(x, d);
    for (uint64_t d = (1ull << 25) - 4096; d < (1ull << 25); d++) { check_div(-(1 << 24), d); check_div(-1, d); }
    // the estimate's rounding boundaries: every x <= d for small d, both signs
    for (uint64_t d = 1; d <= 3000; d++)
        for (int64_t x = 0; x <= (int64_t)d; x++) { check_div(x, d); check_div(-x, d); }
    // samples over the whole range, the ends x = d and d - 1, and exact quotients with their lower neighbours: a divisor e that is a
    // multiple of 16384 divides x * 16384 for every x that is a multiple of e / 16384
    for (int i = 0; i < 2000000; i++) {
        const uint64_t d = 1 + draw() % ((1ull << 25) - 1);
        const int64_t x = (int64_t)(draw() % (d + 1));
        check_div(x, d); check_div(-x, d); check_div((int64_t)d, d); check_div((int64_t)d - 1, d);
        const uint64_t e = (d >> 14) << 14;
        if (e) { const int64_t y = (int64_t)((draw() % 16384 + 1) * (e >> 14)); if ((uint64_t)y <= e) { check_div(y, e); check_div(y - 1, e); check_div(-y, e); } }
    }
    // the dot product and the clamp at the extremes
    const int32_t mags[] = {16384, 16383, 9459, 1, 0};
    for (int32_t a : mags)
        for (int32_t b : mags)
            for (int s = 0; s < 64; s++)
                check_cosine(s & 1 ? -a : a, s & 2 ? -a : a, s & 4 ? -a : a, s & 8 ? -b : b, s & 16 ? -b : b, s & 32 ? -b : b);
    for (int i = 0; i < 200000; i++)
        check_cosine((int32_t)(draw() % 32769) - 16384, (int32_t)(draw() % 32769) - 16384, (int32_t)(draw() % 32769) - 16384, (int32_t)(draw() % 32769) - 16384,
                     (int32_t)(draw() % 32769) - 16384, (int32_t)(draw() % 32769) - 16384);
    // the renormalisation: every short point, sampled long ones, the corners
    for (int32_t x = -40; x <= 40; x++)
        for (int32_t y = -40; y <= 40; y++)
            for (int32_t z = -40; z <= 40; z++) check_point(x, y, z);
    for (int i = 0; i < 300000; i++) check_point((int32_t)(draw() % 65537) - 32768, (int32_t)(draw() % 65537) - 32768, (int32_t)(draw() % 65537) - 32768);
    for (int s = 0; s < 27; s++) check_point((s % 3 - 1) * 32768, (s / 3 % 3 - 1) * 32768, (s / 9 - 1) * 32768);
    if (!failures) printf("ok\n");
    return failures ? 1 : 0;
}
