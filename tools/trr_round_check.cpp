// trr_f64_bits_to_f32_bits (gorder_amd/csrc/trr_round.h, the conversion k_trr_unpack does on the device) against the
// host's `(float)` cast — what the host's TRR reader does — on the CPU: edge values, every f32 exponent with halfway and
// near-halfway mantissas, and random bit patterns.  NaN is compared as NaN.
// usage: trr_round_check [millions of random patterns, default 20]      exit status 0: all equal
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include "../gorder_amd/csrc/trr_round.h"

int main(int argc, char **argv) {
    const long rounds = (argc > 1 ? atol(argv[1]) : 20) * 1000000l;
    long n = 0, bad = 0;
    auto check = [&](uint64_t b) {
        double d;
        memcpy(&d, &b, 8);
        const float f = (float)d;
        uint32_t want;
        memcpy(&want, &f, 4);
        const uint32_t got = trr_f64_bits_to_f32_bits(b);
        n++;
        float g;
        memcpy(&g, &got, 4);
        const bool same = std::isnan(d) ? std::isnan(g) : got == want;
        if (!same && bad++ < 10) printf("%016llx: %08x, the cast gives %08x\n", (unsigned long long)b, got, want);
    };
    const double edges[] = {0.0, -0.0, INFINITY, -INFINITY, NAN, 1e39, -1e39, 5e-324, 2.2250738585072014e-308,
                            3.4028234663852886e38, 3.4028235677973366e38, 1.401298464324817e-45, 7.006492321624085e-46};
    for (double d : edges) { uint64_t b; memcpy(&b, &d, 8); check(b); check(b + 1); check(b - 1); }
    std::mt19937_64 rng(1);
    for (uint64_t e = 1023 - 160; e < 1023 + 135; e++)           // every exponent around the f32 range
        for (uint64_t sign = 0; sign < 2; sign++)
            for (int k = 0; k < 2000; k++) {
                uint64_t m = rng() & 0xfffffffffffffull;
                const int mode = k % 5;
                if (mode == 1) m = (m & ~0x1fffffffull) | 0x10000000ull;                  // exactly halfway for a normal result
                if (mode == 2) m &= ~((1ull << (rng() % 52)) - 1ull);                     // trailing zeros: ties of denormal results
                if (mode == 3) m |= (1ull << (rng() % 52)) - 1ull;                        // trailing ones: carries
                if (mode == 4) m = (m & ~0x1fffffffull) | (0x10000000ull + (rng() % 3) - 1ull);
                check((sign << 63) | (e << 52) | m);
            }
    for (long k = 0; k < rounds; k++) check(rng());
    printf("%ld patterns, %ld differ\n", n, bad);
    return bad != 0;
}
