// replay_rows.h — host side of the whole-trajectory manual tables (gorder_hip_set_manual_leaflet_table,
// gorder_hip_set_manual_normal_table): which table row a frame reads, which rows of a batch have to be expanded and
// which one is carried into the next batch, and the packing of flag bytes into the words the device keeps.  No HIP call in
// here, so tests/cabi/replay_rows.cpp can drive all of it without a device.
//
// The lookups are the reference's: a frame's leaflets are row frame / frequency of the file (row 0 for Frequency::Once,
// leaflets.rs:835-839), its normals row frame / step, and a frame off the step is refused (normal.rs:276-283).  A table
// holds the window [first_row, first_row + n_rows) of those rows; a frame whose row lies outside it is FrameNotFound.
#ifndef GORDER_REPLAY_ROWS_H
#define GORDER_REPLAY_ROWS_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace gorder {

enum ReplayStatus { kReplayOk = 0, kReplayMissingRow = 1, kReplayBadStep = 2 };

// words of a bit-packed flag row, as collect_flag_words: bit (m & 63) of word (m >> 6) = molecule m's flag
inline size_t replay_flag_words(size_t n_mol) { return (n_mol + 63u) / 64u; }

// Upper = 0 / Lower = 1 in bit 0 of every byte (what gorder_hip_set_manual_leaflets reads); the bits past the last molecule are 0
inline void replay_pack_flags(const uint8_t *flags, size_t n_mol, uint64_t *words) {
    for (size_t w = 0; w < replay_flag_words(n_mol); w++) words[w] = 0;
    for (size_t m = 0; m < n_mol; m++)
        if (flags[m] & 1u) words[m >> 6] |= (uint64_t)1 << (m & 63u);
}

// what k_replay_flags makes of a word: the byte of molecule `m`
inline uint8_t replay_flag_of(const uint64_t *words, size_t m, bool flip) {
    return (uint8_t)(((words[m >> 6] >> (m & 63u)) & 1u) ^ (flip ? 1u : 0u));
}

inline uint64_t replay_assignment_index(uint32_t frequency, uint64_t frame) { return frequency ? frame / frequency : 0; }
inline bool replay_should_assign(uint32_t frequency, uint64_t frame) {   // leaflets.rs:435-441
    return frequency == 0 ? frame == 0 : (frame % frequency) == 0;
}

// a window of table rows; `local` = the row inside the device copy
struct ReplayWindow {
    uint64_t first_row = 0, n_rows = 0;
    bool holds(uint64_t row) const { return row >= first_row && row - first_row < n_rows; }
};

// The leaflet rows of one batch.  Row 0 of the expanded flags is the carry (the assignment the last batch ended with),
// rows 1.. are the table rows this batch opens, in order: expand[k] (a row inside the window) becomes row k + 1.
struct ReplayLeafletBatch {
    std::vector<uint32_t> arow;            // per frame: the expanded row its molecules are routed by
    std::vector<uint32_t> expand;          // table rows (inside the window) to expand
    std::vector<uint32_t> collect_rows;    // expanded rows opened by an assignment frame (should_assign) ...
    std::vector<uint64_t> collect_frames;  // ... and those frames: what GORDER_COLLECT_LEAFLETS appends
    bool have_carry = false;               // after the batch
    uint64_t carry_index = 0;              // assignment index of the newest row = the next batch's carry
};

// Walk the frames of a batch.  `have_carry` / `carry_index`: what the handle holds from the batch before.  A frame whose
// assignment index differs from the one before it opens a new row; one that continues the carry reads row 0.
// kReplayMissingRow: *bad_frame is the first frame whose row the window does not hold, `out` is not to be used.
inline ReplayStatus replay_plan_leaflets(uint32_t frequency, const ReplayWindow &win, bool have_carry, uint64_t carry_index,
                                         const uint64_t *frame_index, uint32_t n_frames, ReplayLeafletBatch &out,
                                         uint64_t *bad_frame) {
    out.arow.assign(n_frames, 0u);
    out.expand.clear();
    out.collect_rows.clear();
    out.collect_frames.clear();
    bool have = have_carry;
    uint64_t prev = carry_index;
    for (uint32_t f = 0; f < n_frames; f++) {
        const uint64_t idx = replay_assignment_index(frequency, frame_index[f]);
        if (!have || idx != prev) {
            if (!win.holds(idx)) {
                if (bad_frame) *bad_frame = frame_index[f];
                return kReplayMissingRow;
            }
            out.expand.push_back((uint32_t)(idx - win.first_row));
            if (replay_should_assign(frequency, frame_index[f])) {
                out.collect_rows.push_back((uint32_t)out.expand.size());
                out.collect_frames.push_back(frame_index[f]);
            }
            have = true;
            prev = idx;
        }
        out.arow[f] = (uint32_t)out.expand.size();
    }
    out.have_carry = have;
    out.carry_index = prev;
    return kReplayOk;
}

// The normals rows of one batch: row_of_frame[f] = the table row (inside the window) frame f reads.
// kReplayBadStep: *bad_frame is the first frame that is no multiple of `step`; kReplayMissingRow as above.  The first
// offending frame of the batch decides which of the two is returned.
inline ReplayStatus replay_plan_normals(uint32_t step, const ReplayWindow &win, const uint64_t *frame_index, uint32_t n_frames,
                                        std::vector<uint32_t> &row_of_frame, uint64_t *bad_frame) {
    row_of_frame.assign(n_frames, 0u);
    for (uint32_t f = 0; f < n_frames; f++) {
        const uint64_t frame = frame_index[f];
        if (step == 0 || frame % step != 0) {
            if (bad_frame) *bad_frame = frame;
            return kReplayBadStep;
        }
        const uint64_t row = frame / step;
        if (!win.holds(row)) {
            if (bad_frame) *bad_frame = frame;
            return kReplayMissingRow;
        }
        row_of_frame[f] = (uint32_t)(row - win.first_row);
    }
    return kReplayOk;
}

// a table of n_rows rows must be addressable by the 32-bit rows above and must not wrap the 64-bit row numbers
inline bool replay_window_ok(uint64_t first_row, uint64_t n_rows) {
    return n_rows <= 0xffffffffull && first_row <= ~(uint64_t)0 - n_rows;
}

}  // namespace gorder

#endif
