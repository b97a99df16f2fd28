// timewise_blocks.h — the arithmetic around the per-frame rows that is not a sum: the block grid of estimate_error
// (timewise.rs:191-231), how a chunk of kTwChunkFrames rows falls onto that grid, and the validation of accumulator groups.
// The kernels of kernels_timewise.h and the host side call the same functions, and there is no HIP call in here, so
// tests/cabi/timewise_blocks.cpp can drive all of it without a device.
//
// The grid belongs to the WHOLE analysis: block size = total_frames / n_blocks, the frames past n_blocks * block size are
// dropped as the reference drops them.  A handle that holds the rows of the positions [first_position, first_position + n_rows)
// of that analysis — a shard — puts its row r into block (first_position + r) / block size, so the block sums of the shards
// add up to the block sums of the whole run element by element.
#ifndef GORDER_TIMEWISE_BLOCKS_H
#define GORDER_TIMEWISE_BLOCKS_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GORDER_TW_HD __host__ __device__ inline
#else
#define GORDER_TW_HD inline
#endif

namespace gorder {

// rows a workgroup of k_tw_blocks folds before it touches global memory; also the chunk of the convergence scan
constexpr uint32_t kTwChunkFrames = 64;

GORDER_TW_HD uint64_t tw_block_size(uint64_t total_frames, uint32_t n_blocks) { return n_blocks ? total_frames / n_blocks : 0; }

// first_position + n_rows must not wrap
GORDER_TW_HD bool tw_positions_ok(uint64_t first_position, uint64_t n_rows) { return first_position <= ~(uint64_t)0 - n_rows; }

// How many of the handle's rows (always its first ones) lie in a block of the grid: those at a position below
// n_blocks * block_size.  0 for an empty grid (block_size 0).
GORDER_TW_HD uint64_t tw_rows_used(uint64_t first_position, uint64_t n_rows, uint64_t block_size, uint32_t n_blocks) {
    if (block_size == 0) return 0;
    const uint64_t limit = block_size * n_blocks;       // <= total_frames: no overflow
    if (first_position >= limit) return 0;
    const uint64_t room = limit - first_position;
    return n_rows < room ? n_rows : room;
}

GORDER_TW_HD uint64_t tw_block_of(uint64_t first_position, uint64_t row, uint64_t block_size) { return (first_position + row) / block_size; }

// Row `row` lies in block `block`; the rows [row, return value) are the ones of [row, end) that lie in it as well.
// (A chunk is walked as: r = begin; while (r < end) { b = tw_block_of(r); e = tw_segment_end(r, end, b); fold [r, e); r = e; }.)
GORDER_TW_HD uint64_t tw_segment_end(uint64_t first_position, uint64_t row, uint64_t end, uint64_t block, uint64_t block_size) {
    const uint64_t block_end = (block + 1u) * block_size - first_position;   // > row, as row lies in `block`
    return block_end < end ? block_end : end;
}

GORDER_TW_HD uint64_t tw_n_chunks(uint64_t n_rows) { return (n_rows + kTwChunkFrames - 1u) / kTwChunkFrames; }

// Groups of accumulator slots in CSR form: group g = slots[group_begin[g] .. group_begin[g + 1]).
enum TwGroupStatus { kTwGroupsOk = 0, kTwGroupsNone = 1, kTwGroupsNotAscending = 2, kTwGroupEmpty = 3, kTwGroupSlotRange = 4 };

// *bad: the offending group (kTwGroupsNotAscending, kTwGroupEmpty) or the offending entry of slots[] (kTwGroupSlotRange)
inline TwGroupStatus tw_check_groups(const uint32_t *group_begin, const uint32_t *slots, uint32_t n_groups, uint32_t n_acc,
                                     uint32_t *bad) {
    if (!group_begin || !slots || n_groups == 0) return kTwGroupsNone;
    for (uint32_t g = 0; g < n_groups; g++) {
        if (bad) *bad = g;
        if (group_begin[g + 1] < group_begin[g]) return kTwGroupsNotAscending;
        if (group_begin[g + 1] == group_begin[g]) return kTwGroupEmpty;
    }
    for (uint32_t k = group_begin[0]; k < group_begin[n_groups]; k++)
        if (slots[k] >= n_acc) {
            if (bad) *bad = k;
            return kTwGroupSlotRange;
        }
    return kTwGroupsOk;
}

inline const char *tw_group_status_text(TwGroupStatus st) {
    switch (st) {
    case kTwGroupsOk: return "ok";
    case kTwGroupsNone: return "no groups";
    case kTwGroupsNotAscending: return "group_begin is not ascending";
    case kTwGroupEmpty: return "an empty group";
    case kTwGroupSlotRange: return "a slot is not below the number of accumulators";
    }
    return "?";
}

}  // namespace gorder

#endif
