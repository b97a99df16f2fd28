// Drives gorder_amd/csrc/ordermap_final.h without a device (built with -fsanitize=address,undefined by
// tests/test_ordermap_final_cpu.py): prints the bit pattern of om_tile_value for every (sum, count, min_samples, negate) line
// of the file named on the command line — the test compares them with its numpy restatement —, checks the properties that
// need no second opinion, and the validation of the groups.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ordermap_final.h"

using namespace gorder;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                           \
        }                                                                           \
    } while (0)

static uint32_t bits(float v) {
    uint32_t b;
    std::memcpy(&b, &v, sizeof(b));
    return b;
}

int main(int argc, char **argv) {
    // below min_samples: NaN whatever the sum; at it: a number
    CHECK(om_tile_value(5, 0, 1, true) != om_tile_value(5, 0, 1, true));
    CHECK(om_tile_value((uint64_t)-7, 4, 5, false) != om_tile_value((uint64_t)-7, 4, 5, false));
    CHECK(om_tile_value((uint64_t)-7, 5, 5, false) == om_tile_value((uint64_t)-7, 5, 5, false));
    // a zero sum: +0.0, and -0.0 when negated
    CHECK(bits(om_tile_value(0, 3, 1, false)) == 0u && bits(om_tile_value(0, 3, 1, true)) == 0x80000000u);
    // the negation touches the sign bit only
    CHECK((bits(om_tile_value(1234567, 7, 1, false)) ^ bits(om_tile_value(1234567, 7, 1, true))) == 0x80000000u);
    // the f32 division, not calc_order's truncating one: -7 ticks over 2 samples is -3.5e-6, not -3e-6
    CHECK(om_tile_value((uint64_t)-7, 2, 1, false) == (float)(-7.0 / 1e6) / 2.0f);
    CHECK(om_tile_value((uint64_t)-7, 2, 1, false) != (float)(-3.0 / 1e6));

    // groups and min_samples
    {
        const uint32_t begin[] = {0, 2, 3, 6}, slots[] = {4, 0, 7, 1, 2, 7};
        TwGroupStatus gs = kTwGroupEmpty;
        uint32_t bad = 99;
        CHECK(om_check(begin, slots, 3, 8, 1, &gs, &bad) == kOmOk && gs == kTwGroupsOk);
        CHECK(om_check(begin, slots, 3, 8, 0, &gs, &bad) == kOmMinSamples);
        CHECK(om_check(begin, slots, 3, 7, 1, &gs, &bad) == kOmGroups && gs == kTwGroupSlotRange && bad == 2);
        CHECK(om_check(begin, slots, 0, 8, 1, &gs, &bad) == kOmGroups && gs == kTwGroupsNone);
        CHECK(om_check(nullptr, slots, 3, 8, 1, &gs, &bad) == kOmGroups && gs == kTwGroupsNone);
        CHECK(om_check(begin, nullptr, 3, 8, 1, nullptr, nullptr) == kOmGroups);
        const uint32_t empty[] = {0, 2, 2, 6}, down[] = {0, 3, 2, 6};
        CHECK(om_check(empty, slots, 3, 8, 1, &gs, &bad) == kOmGroups && gs == kTwGroupEmpty && bad == 1);
        CHECK(om_check(down, slots, 3, 8, 1, &gs, &bad) == kOmGroups && gs == kTwGroupsNotAscending && bad == 1);
        CHECK(om_check(begin + 1, slots, 2, 8, 5, &gs, &bad) == kOmOk);                  // group_begin need not start at 0
    }
    // the size of the raw arrays
    CHECK(om_map_words(64, 91, 91) == 3ull * 64 * 8281 && om_map_words(0, 4, 4) == 0 && om_map_words(4, 0, 4) == 0);
    CHECK(om_map_words(1, 0x80000000u, 0x80000000u) == 3ull << 62);
    CHECK(om_map_words(2, 0x80000000u, 0x80000000u) == 0);                               // would pass 2^64

    if (argc > 1) {
        std::FILE *f = std::fopen(argv[1], "r");
        CHECK(f != nullptr);
        int64_t sum;
        uint64_t count;
        uint32_t min_samples, negate;
        while (std::fscanf(f, "%" SCNd64 " %" SCNu64 " %" SCNu32 " %" SCNu32, &sum, &count, &min_samples, &negate) == 4)
            std::printf("%08" PRIx32 "\n", bits(om_tile_value((uint64_t)sum, count, min_samples, negate != 0)));
        std::fclose(f);
    }
    std::printf("ordermap_final ok\n");
    return 0;
}
