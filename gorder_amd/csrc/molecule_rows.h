// molecule_rows.h — host side of the per-molecule order rows (gorder_hip_set_molecule_rows): the groups of accumulator
// slots checked, and the lane order k_bonds_tiled_mol reads.  No HIP, no handle: tests/cabi/molecule_rows.cpp drives it with
// random tiles and group maps.
//
// A row holds, per analysed frame, one packed 64-bit word per (group, molecule): (samples << 42) + tick sum, the ordermaps'
// word (kMapOne of kernels_common.h).  The kernel leaves every lane's word of a frame in LDS; so that ONE thread can add up
// what a tile contributes to a (group, molecule) word, the tile's items are copied in the order (group of the item's slot,
// molecule) — stable, items of ungrouped slots last — and a run table says which lanes go where:
//   MolRun {lane0, n, word}: lanes [lane0, lane0 + n) of the tile add into word = group * n_mol_total + molecule of a frame's row.
// Plan::items_by_slot / item_run are the same idea per slot.  The runs of a tile ascend in `word`, so the threads that send
// a frame's atomics go to neighbouring molecules of one group: contiguous 8-byte words.
#ifndef GORDER_MOLECULE_ROWS_H
#define GORDER_MOLECULE_ROWS_H
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <vector>

#include "plan.h"

namespace gorder {

// A group holds at most this many slots: a molecule has one sample per slot and frame, |tick| <= 10^6, and the sum of a
// (group, molecule, frame) is handed out as int32 — 2047 x 10^6 < 2^31.  (The packed word itself would hold 2^21 samples.)
constexpr uint32_t kMolRowsMaxGroupSlots = 2047;
constexpr uint32_t kMolRowsNoGroup = 0xffffffffu;
constexpr unsigned kMolRowsCountShift = 42;          // = log2(kMapOne); kernels_molrows.h asserts it
static_assert((uint64_t)kMolRowsMaxGroupSlots * 1000000ull < (1ull << 31), "a group's tick sum of one molecule and frame fits int32");

struct MolRun {
    uint16_t lane0, n;      // lanes of the tile (in the order of MolRows::items)
    uint32_t word;          // group * n_mol_total + molecule
};

struct MolRows {
    uint32_t n_groups = 0;
    std::vector<uint32_t> group_of_slot;    // [n_acc], kMolRowsNoGroup: in no group
    std::vector<Item> items;                // every tile's items in lane order (same ranges as Plan::items)
    std::vector<MolRun> runs;               // tile by tile
    std::vector<uint32_t> run_begin;        // [n_tiles + 1] (CSR)
    uint64_t n_runs = 0;                    // = atomics per frame
    uint32_t max_runs_per_tile = 0;
    uint32_t max_tiles_per_word = 0;        // how many tiles add into one (group, molecule) word
};

// the packed word of a (frame, group, molecule) -> tick sum and samples (map_unpack of kernels_common.h, for the host)
inline void molecule_word_unpack(uint64_t w, int64_t &sum, uint64_t &cnt) {
    sum = (int64_t)(w << (64 - kMolRowsCountShift)) >> (64 - kMolRowsCountShift);
    cnt = (w - (uint64_t)sum) >> kMolRowsCountShift;
}

// Groups in CSR form over accumulator slots -> group_of_slot.  nullptr when they are fine, else what is wrong.
inline const char *molecule_groups_check(const uint32_t *group_begin, const uint32_t *slots, uint32_t n_groups, uint32_t n_acc,
                                         std::vector<uint32_t> &group_of_slot) {
    group_of_slot.assign(n_acc, kMolRowsNoGroup);
    if (group_begin[0] != 0) return "group_begin[0] is not 0";
    for (uint32_t g = 0; g < n_groups; g++) {
        if (group_begin[g + 1] < group_begin[g]) return "group_begin is not ascending";
        if (group_begin[g + 1] == group_begin[g]) return "an empty group";
        if (group_begin[g + 1] - group_begin[g] > kMolRowsMaxGroupSlots) return "a group of more than 2047 slots";
        for (uint32_t q = group_begin[g]; q < group_begin[g + 1]; q++) {
            if (slots[q] >= n_acc) return "a slot is out of range (>= n_acc)";
            if (group_of_slot[slots[q]] != kMolRowsNoGroup) return "a slot is in two groups";
            group_of_slot[slots[q]] = g;
        }
    }
    return nullptr;
}

// The lane order and the run tables of every tile (see above).  group_of_slot: [n_acc].
inline void build_molecule_rows(const std::vector<Tile> &tiles, const std::vector<Item> &items, const std::vector<uint32_t> &tile_slots,
                                const std::vector<uint32_t> &group_of_slot, uint32_t n_groups, uint32_t n_mol_total, MolRows &out) {
    out.n_groups = n_groups;
    out.group_of_slot = group_of_slot;
    out.items = items;
    out.runs.clear();
    out.run_begin.assign(1, 0u);
    out.max_runs_per_tile = 0;
    std::map<uint32_t, uint32_t> tiles_of_word;
    for (const Tile &tile : tiles) {
        auto group_of = [&](const Item &it) { return group_of_slot[tile_slots[tile.slot0 + it.lslot]]; };
        Item *first = out.items.data() + tile.item0;
        std::stable_sort(first, first + tile.n_items, [&](const Item &x, const Item &y) {
            const uint32_t gx = group_of(x), gy = group_of(y);      // (kMolRowsNoGroup is the largest: ungrouped last)
            if (gx != gy) return gx < gy;
            return x.mol < y.mol;
        });
        uint32_t n_here = 0;
        for (uint32_t i = 0; i < tile.n_items;) {
            const uint32_t g = group_of(first[i]);
            if (g == kMolRowsNoGroup) break;
            uint32_t n = 1;
            while (i + n < tile.n_items && group_of(first[i + n]) == g && first[i + n].mol == first[i].mol) n++;
            const uint32_t word = g * n_mol_total + first[i].mol;
            out.runs.push_back({(uint16_t)i, (uint16_t)n, word});
            tiles_of_word[word]++;
            n_here++;
            i += n;
        }
        out.run_begin.push_back((uint32_t)out.runs.size());
        out.max_runs_per_tile = std::max(out.max_runs_per_tile, n_here);
    }
    out.n_runs = out.runs.size();
    out.max_tiles_per_word = 0;
    for (const auto &kv : tiles_of_word) out.max_tiles_per_word = std::max(out.max_tiles_per_word, kv.second);
}

// frames of one staging sub-range: what `staging_bytes` of 64-bit words hold, at least one, at most the batch
inline uint32_t molecule_rows_subrange(uint32_t n_frames, size_t words_per_frame, size_t staging_bytes) {
    const size_t fit = std::max<size_t>(1, staging_bytes / (words_per_frame * sizeof(uint64_t)));
    return (uint32_t)std::min<size_t>(fit, n_frames);
}

}  // namespace gorder
#endif
