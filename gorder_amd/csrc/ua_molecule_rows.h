// ua_molecule_rows.h — host side of the per-molecule order rows over united-atom tiles (gorder_hip_set_molecule_rows with
// GORDER_FLAG_UA_SAMPLES; k_ua_mol of kernels_ua_samples.h reads the tables).  No HIP, no handle:
// tests/cabi/ua_molecule_rows.cpp drives it with random tiles and group maps.
//
// A lane of a united-atom tile is one carbon with up to three virtual hydrogens, each with an accumulator slot of its own
// (local slot lslot0 + k), and the lanes go by (kind, slot, molecule): the hydrogens of one carbon may sit in different
// groups or in none, and the samples of one molecule in one group are neither neighbouring lanes nor in one tile.  So no
// lane order is copied (molecule_rows.h does that for bond tiles); instead, per tile:
//   words[word_begin[tile] .. word_begin[tile + 1])  the distinct (group, molecule) words the tile adds into, ascending;
//                                                    word = group * n_mol_total + molecule.  At most 3 * kBlock of them.
//   lane_words[item].w[k]                            the LOCAL index of hydrogen k's word in that list, kUaMolNoWord where the
//                                                    hydrogen's slot is in no group or the carbon has no hydrogen k
// The kernel keeps one 64-bit LDS word per (frame of a stage, local word), every lane adds its hydrogens' packed words in,
// and behind the stage's barrier a thread per (local word, frame) sends one global atomic.
#ifndef GORDER_UA_MOLECULE_ROWS_H
#define GORDER_UA_MOLECULE_ROWS_H
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <vector>

#include "molecule_rows.h"
#include "plan.h"

namespace gorder {

constexpr uint16_t kUaMolNoWord = 0xffffu;
#ifndef GORDER_UA_MOL_STAGE
#define GORDER_UA_MOL_STAGE 4               // (2 and 8 measured against it: DESIGN 6j.1)
#endif
constexpr uint32_t kUaMolStage = GORDER_UA_MOL_STAGE;   // frames of a stage of k_ua_mol: one barrier per stage
static_assert(3u * kBlock < kUaMolNoWord, "a local word index fits 16 bits beside the 'none' value");

struct UaLaneWords {
    uint16_t w[4];          // hydrogen 0, 1, 2; w[3] pads the record to 8 bytes
};

struct UaMolRows {
    std::vector<UaLaneWords> lane_words;    // [Plan::ua_items]
    std::vector<uint32_t> words;            // tile by tile, ascending inside a tile
    std::vector<uint32_t> word_begin;       // [n_ua_tiles + 1] (CSR)
    uint32_t max_local = 0;                 // the longest list of one tile
    bool on() const { return !word_begin.empty(); }
};

inline uint32_t ua_hydrogens(uint32_t kind) { return kind == GORDER_UA_CH3 ? 3u : kind == GORDER_UA_CH2 ? 2u : 1u; }

// The word lists and the lanes' local indices of every united-atom tile.  group_of_slot: [n_acc] (molecule_groups_check).
// tiles_of_word: how many tiles (of either kind) add into a word; the caller seeds it with the bond tiles' runs.
inline void build_ua_molecule_rows(const std::vector<Tile> &ua_tiles, const std::vector<UaItem> &ua_items,
                                   const std::vector<uint32_t> &ua_tile_slots, const std::vector<uint32_t> &group_of_slot,
                                   uint32_t n_mol_total, std::map<uint32_t, uint32_t> &tiles_of_word, UaMolRows &out) {
    out.lane_words.assign(ua_items.size(), UaLaneWords{{kUaMolNoWord, kUaMolNoWord, kUaMolNoWord, kUaMolNoWord}});
    out.words.clear();
    out.word_begin.assign(1, 0u);
    out.max_local = 0;
    std::vector<uint32_t> here;
    for (const Tile &tile : ua_tiles) {
        auto word_of = [&](const UaItem &it, uint32_t k) {
            const uint32_t g = group_of_slot[ua_tile_slots[tile.slot0 + it.lslot0 + k]];
            return g == kMolRowsNoGroup ? kMolRowsNoGroup : g * n_mol_total + it.mol;
        };
        // (a word equal to kMolRowsNoGroup cannot occur: groups x molecules <= 2^32 - 1 is the setter's check, and the last
        // word of the last group is one below that product)
        here.clear();
        for (uint32_t i = 0; i < tile.n_items; i++) {
            const UaItem &it = ua_items[tile.item0 + i];
            for (uint32_t k = 0; k < ua_hydrogens(it.kind); k++) {
                const uint32_t w = word_of(it, k);
                if (w != kMolRowsNoGroup) here.push_back(w);
            }
        }
        std::sort(here.begin(), here.end());
        here.erase(std::unique(here.begin(), here.end()), here.end());
        for (uint32_t i = 0; i < tile.n_items; i++) {
            const UaItem &it = ua_items[tile.item0 + i];
            for (uint32_t k = 0; k < ua_hydrogens(it.kind); k++) {
                const uint32_t w = word_of(it, k);
                if (w == kMolRowsNoGroup) continue;
                out.lane_words[tile.item0 + i].w[k] = (uint16_t)(std::lower_bound(here.begin(), here.end(), w) - here.begin());
            }
        }
        for (uint32_t w : here) tiles_of_word[w]++;
        out.words.insert(out.words.end(), here.begin(), here.end());
        out.word_begin.push_back((uint32_t)out.words.size());
        out.max_local = std::max(out.max_local, (uint32_t)here.size());
    }
}

// dynamic LDS of k_ua_mol: the tile's word list, then `n_buf` buffers of kUaMolStage rows of max_local 64-bit words.  Two
// buffers (one barrier a stage) where they fit the budget, else one (two barriers a stage).
constexpr size_t kUaMolWordBudget = 40u * 1024u;
inline uint32_t ua_mol_buffers(uint32_t max_local) { return 2u * kUaMolStage * max_local * sizeof(uint64_t) <= kUaMolWordBudget ? 2u : 1u; }
inline size_t ua_mol_list_bytes(uint32_t max_local) { return ((size_t)max_local * sizeof(uint32_t) + 15u) / 16u * 16u; }
inline size_t ua_mol_lds_bytes(uint32_t max_local) {
    return ua_mol_list_bytes(max_local) + (size_t)ua_mol_buffers(max_local) * kUaMolStage * max_local * sizeof(uint64_t);
}

}  // namespace gorder
#endif
