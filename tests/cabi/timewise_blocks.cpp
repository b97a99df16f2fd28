// Drives gorder_amd/csrc/timewise_blocks.h without a device (built with -fsanitize=address,undefined by
// tests/test_timewise_device_cpu.py): the block grid, the walk of a chunk over the grid at every offset for small frame
// counts, block sizes and first positions — summed exactly like k_tw_blocks sums — and the validation of groups.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "timewise_blocks.h"

using namespace gorder;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                           \
        }                                                                           \
    } while (0)

// the walk of k_tw_blocks with a chunk of `chunk` rows: block_of_row[r] for the rows it folds, the number of adds
static uint64_t walk(uint64_t first, uint64_t n_rows, uint64_t bs, uint32_t n_blocks, uint64_t chunk, std::vector<int64_t> &block_of_row) {
    block_of_row.assign(n_rows, -1);
    const uint64_t n_used = tw_rows_used(first, n_rows, bs, n_blocks);
    CHECK(n_used <= n_rows);
    uint64_t adds = 0;
    for (uint64_t c0 = 0; c0 < n_used; c0 += chunk) {
        uint64_t r = c0;
        const uint64_t end = c0 + chunk < n_used ? c0 + chunk : n_used;
        while (r < end) {
            const uint64_t b = tw_block_of(first, r, bs);
            const uint64_t e = tw_segment_end(first, r, end, b, bs);
            CHECK(b < n_blocks);
            CHECK(e > r && e <= end);
            for (uint64_t q = r; q < e; q++) {
                CHECK(block_of_row[q] == -1);
                block_of_row[q] = (int64_t)b;
            }
            adds++;
            r = e;
        }
    }
    return adds;
}

int main() {
    CHECK(kTwChunkFrames >= 2);
    // the grid: the remainder is dropped, fewer frames than blocks is an empty grid
    CHECK(tw_block_size(13, 5) == 2 && tw_block_size(4, 5) == 0 && tw_block_size(10, 5) == 2 && tw_block_size(0, 5) == 0);
    CHECK(tw_block_size(7, 0) == 0);
    CHECK(tw_rows_used(0, 13, 2, 5) == 10 && tw_rows_used(0, 4, 0, 5) == 0 && tw_rows_used(10, 3, 2, 5) == 0);
    CHECK(tw_rows_used(7, 6, 2, 5) == 3 && tw_rows_used(7, 2, 2, 5) == 2 && tw_rows_used(11, 2, 2, 5) == 0);
    CHECK(tw_n_chunks(0) == 0 && tw_n_chunks(1) == 1 && tw_n_chunks(kTwChunkFrames) == 1 && tw_n_chunks(kTwChunkFrames + 1) == 2);
    CHECK(tw_positions_ok(0, 0) && tw_positions_ok(~(uint64_t)0 - 5, 5) && !tw_positions_ok(~(uint64_t)0 - 5, 6));
    // large positions: nothing wraps below 2^64
    {
        const uint64_t total = (uint64_t)1 << 62, bs = tw_block_size(total, 4), first = 3 * bs - 2;
        CHECK(bs == (uint64_t)1 << 60);
        CHECK(tw_block_of(first, 0, bs) == 2 && tw_block_of(first, 2, bs) == 3);
        CHECK(tw_segment_end(first, 0, 10, 2, bs) == 2 && tw_segment_end(first, 2, 10, 3, bs) == 10);
        CHECK(tw_rows_used(first, 10, bs, 4) == 10 && tw_rows_used(4 * bs - 3, 10, bs, 4) == 3);
    }
    // every split: all shards [first, first + n_rows) of analyses of up to 23 frames, chunks of 1..9 rows
    std::vector<int64_t> got;
    for (uint64_t total = 0; total <= 23; total++)
        for (uint32_t n_blocks = 2; n_blocks <= 7; n_blocks++) {
            const uint64_t bs = tw_block_size(total, n_blocks);
            for (uint64_t first = 0; first <= total; first++)
                for (uint64_t n_rows = 0; first + n_rows <= total; n_rows++)
                    for (uint64_t chunk = 1; chunk <= 9; chunk++) {
                        const uint64_t adds = walk(first, n_rows, bs, n_blocks, chunk, got);
                        uint64_t want_adds = 0;
                        for (uint64_t r = 0; r < n_rows; r++) {
                            const int64_t want = bs && (first + r) / bs < n_blocks ? (int64_t)((first + r) / bs) : -1;
                            CHECK(got[r] == want);
                            // one add per (chunk, block) pair that holds a row
                            if (want >= 0 && (r == 0 || r % chunk == 0 || got[r - 1] != want)) want_adds++;
                        }
                        CHECK(adds == want_adds);
                    }
        }
    // groups
    {
        const uint32_t begin[] = {0, 2, 3, 6}, slots[] = {4, 0, 7, 1, 2, 7};
        uint32_t bad = 99;
        CHECK(tw_check_groups(begin, slots, 3, 8, &bad) == kTwGroupsOk);
        CHECK(tw_check_groups(begin, slots, 3, 7, &bad) == kTwGroupSlotRange && bad == 2);
        CHECK(tw_check_groups(begin + 1, slots, 2, 8, nullptr) == kTwGroupsOk);          // group_begin need not start at 0
        CHECK(tw_check_groups(begin + 1, slots, 2, 7, &bad) == kTwGroupSlotRange && bad == 2);
        CHECK(tw_check_groups(begin + 2, slots, 1, 7, &bad) == kTwGroupSlotRange && bad == 5);
        CHECK(tw_check_groups(begin, slots, 1, 5, &bad) == kTwGroupsOk);                 // slots past the last group are not read
        CHECK(tw_check_groups(begin, slots, 0, 8, &bad) == kTwGroupsNone);
        CHECK(tw_check_groups(nullptr, slots, 3, 8, &bad) == kTwGroupsNone && tw_check_groups(begin, nullptr, 3, 8, &bad) == kTwGroupsNone);
        const uint32_t empty[] = {0, 2, 2, 6}, down[] = {0, 3, 2, 6};
        CHECK(tw_check_groups(empty, slots, 3, 8, &bad) == kTwGroupEmpty && bad == 1);
        CHECK(tw_check_groups(down, slots, 3, 8, &bad) == kTwGroupsNotAscending && bad == 1);
        for (int s = kTwGroupsOk; s <= kTwGroupSlotRange; s++) CHECK(tw_group_status_text((TwGroupStatus)s)[0] != '?');
    }
    std::printf("timewise_blocks ok\n");
    return 0;
}
