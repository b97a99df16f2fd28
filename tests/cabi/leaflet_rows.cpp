// Drives gorder_amd/csrc/leaflet_rows.h (the flag row every frame of a batch is routed by) without a device and prints what
// plan_assignment_rows makes of a full sweep: every leaflet method, frequency 0 (once) to 3, with and without an earlier
// assignment and earlier clusters, every batch of 0 to 5 frames that starts at frame 0, 1 or 4 with stride 1 or 2, and one
// batch with an irregular list of frames.  One line per case:
//   method frequency have_assignment cl_have_carry : frames : status last_assign_frame : arow : aframes : is0
// The caller's vectors go in holding sentinels (is0 = {7, 7}, last_assign_frame = 99), so that "left as it was" shows.
// Built with -fsanitize=address,undefined by tests/test_leaflet_rows_cpu.py, which holds the expected values.
#include <cstdio>
#include <vector>

#include "leaflet_rows.h"

namespace {

template <typename T>
void print_list(const std::vector<T> &v) {
    printf(" :");
    for (const T &x : v) printf(" %llu", (unsigned long long)x);
}

void run_case(uint32_t method, uint32_t frequency, bool have, bool carry, const std::vector<uint64_t> &frames) {
    std::vector<uint32_t> arow(3, 5u), aframes(2, 5u);      // (stale contents of an earlier batch)
    std::vector<uint8_t> is0(2, 7);
    uint64_t last = 99;
    const gorder::LeafletRowsStatus st = gorder::plan_assignment_rows(method, frequency, have, carry, frames.data(), (uint32_t)frames.size(),
                                                                      arow, aframes, is0, last);
    printf("%u %u %d %d", method, frequency, have ? 1 : 0, carry ? 1 : 0);
    print_list(frames);
    printf(" : %d %llu", (int)st, (unsigned long long)last);
    if (st != gorder::kLeafletRowsOk) { arow.clear(); aframes.clear(); }      // (not to be used: only is0 is part of the contract)
    print_list(arow);
    print_list(aframes);
    print_list(is0);
    printf("\n");
}

}  // namespace

int main() {
    std::vector<std::vector<uint64_t>> batches;
    for (uint32_t n = 0; n <= 5; n++)
        for (uint64_t first : {0, 1, 4})
            for (uint64_t stride : {1, 2}) {
                std::vector<uint64_t> frames(n);
                for (uint32_t f = 0; f < n; f++) frames[f] = first + f * stride;
                batches.push_back(frames);
            }
    batches.push_back({5, 0, 2, 3, 9, 6, 6});
    for (uint32_t method = GORDER_LEAFLETS_NONE; method <= GORDER_LEAFLETS_CLUSTERING; method++)
        for (uint32_t frequency = 0; frequency <= 3; frequency++)
            for (int have = 0; have < 2; have++)
                for (int carry = 0; carry < 2; carry++)
                    for (const std::vector<uint64_t> &frames : batches) run_case(method, frequency, have != 0, carry != 0, frames);
    return 0;
}
