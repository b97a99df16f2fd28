// Drives gorder_amd/csrc/ua_molecule_rows.h without a device (built with -fsanitize=address,undefined by
// tests/test_ua_samples_cpu.py): random united-atom tiles and random group maps, the invariants of the word lists checked
// here, one summary line per seed for the test to read.
//
//   ua_molecule_rows SEED0 N        seeds SEED0 .. SEED0 + N - 1 -> "seed tiles items grouped words max_local max_tiles_per_word"
//   ua_molecule_rows lds            the LDS sizing at its edges -> "max_local buffers bytes"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "ua_molecule_rows.h"

using namespace gorder;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);          \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static void one(uint32_t seed) {
    std::mt19937 rng(seed);
    auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    const uint32_t n_mol = 1 + below(300), n_carbon_types = 1 + below(40);
    // the carbon types of the run: kind and first accumulator slot
    std::vector<uint32_t> kind(n_carbon_types), slot0(n_carbon_types);
    uint32_t n_acc = 0;
    static const uint32_t kinds[] = {GORDER_UA_CH3, GORDER_UA_CH2, GORDER_UA_CH1_SAT, GORDER_UA_CH1_UNSAT};
    for (uint32_t c = 0; c < n_carbon_types; c++) {
        kind[c] = kinds[below(4)];
        slot0[c] = n_acc;
        n_acc += ua_hydrogens(kind[c]);
    }
    // groups: every slot in a random group or in none (one seed in four: every slot grouped; one in eight: none)
    const uint32_t n_groups = 1 + below(5), mode = below(8);
    std::vector<uint32_t> group_of_slot(n_acc);
    for (uint32_t s = 0; s < n_acc; s++)
        group_of_slot[s] = mode == 0 ? kMolRowsNoGroup : (mode >= 6 || below(4) != 0) ? below(n_groups) : kMolRowsNoGroup;
    // tiles: up to kBlock carbons each, a local slot list with nh entries per distinct carbon type, any molecules
    std::vector<Tile> tiles;
    std::vector<UaItem> items;
    std::vector<uint32_t> tile_slots;
    const uint32_t n_tiles = 1 + below(12);
    for (uint32_t t = 0; t < n_tiles; t++) {
        Tile tile{};
        tile.item0 = (uint32_t)items.size();
        tile.slot0 = (uint32_t)tile_slots.size();
        tile.n_items = below(8) == 0 ? kBlock : 1 + below(kBlock);
        std::map<uint32_t, uint32_t> local_of_type;
        uint32_t n_local_slots = 0;
        for (uint32_t i = 0; i < tile.n_items; i++) {
            const uint32_t c = below(n_carbon_types);
            if (!local_of_type.count(c)) {
                local_of_type[c] = n_local_slots;
                for (uint32_t k = 0; k < ua_hydrogens(kind[c]); k++) tile_slots.push_back(slot0[c] + k);
                n_local_slots += ua_hydrogens(kind[c]);
            }
            UaItem it{};
            it.lslot0 = (uint16_t)local_of_type[c];
            it.kind = (uint16_t)kind[c];
            it.mol = below(n_mol);
            items.push_back(it);
        }
        tile.n_slots = n_local_slots;
        tiles.push_back(tile);
    }
    std::map<uint32_t, uint32_t> tiles_of_word;
    tiles_of_word[0] = 5;       // a seed from the bond tiles: kept and added to
    UaMolRows out;
    build_ua_molecule_rows(tiles, items, tile_slots, group_of_slot, n_mol, tiles_of_word, out);
    CHECK(out.on() && out.lane_words.size() == items.size() && out.word_begin.size() == tiles.size() + 1 && out.word_begin[0] == 0);
    CHECK(out.word_begin.back() == out.words.size());
    uint64_t grouped = 0;
    uint32_t max_local = 0;
    std::map<uint32_t, uint32_t> want_tiles{{0u, 5u}};
    for (uint32_t t = 0; t < n_tiles; t++) {
        const Tile &tile = tiles[t];
        const uint32_t w0 = out.word_begin[t], n_local = out.word_begin[t + 1] - w0;
        CHECK(out.word_begin[t + 1] >= w0 && n_local <= 3 * kBlock);
        max_local = std::max(max_local, n_local);
        for (uint32_t r = 1; r < n_local; r++) CHECK(out.words[w0 + r] > out.words[w0 + r - 1]);       // distinct, ascending
        std::set<uint32_t> used;
        for (uint32_t i = 0; i < tile.n_items; i++) {
            const UaItem &it = items[tile.item0 + i];
            const UaLaneWords &lw = out.lane_words[tile.item0 + i];
            for (uint32_t k = 0; k < 4; k++) {
                if (k >= ua_hydrogens(it.kind)) { CHECK(lw.w[k] == kUaMolNoWord); continue; }
                const uint32_t g = group_of_slot[tile_slots[tile.slot0 + it.lslot0 + k]];
                if (g == kMolRowsNoGroup) { CHECK(lw.w[k] == kUaMolNoWord); continue; }
                CHECK(lw.w[k] < n_local && out.words[w0 + lw.w[k]] == g * n_mol + it.mol);
                used.insert(lw.w[k]);
                grouped++;
            }
        }
        CHECK(used.size() == n_local);      // no word that no lane feeds
        for (uint32_t r = 0; r < n_local; r++) want_tiles[out.words[w0 + r]]++;
    }
    CHECK(max_local == out.max_local && want_tiles == tiles_of_word);
    uint32_t most = 0;
    for (const auto &kv : tiles_of_word) most = std::max(most, kv.second);
    if (mode == 0) CHECK(out.words.empty() && grouped == 0);
    std::printf("%u %u %zu %llu %zu %u %u\n", seed, n_tiles, items.size(), (unsigned long long)grouped, out.words.size(), out.max_local, most);
}

int main(int argc, char **argv) {
    if (argc == 2 && std::strcmp(argv[1], "lds") == 0) {
        for (uint32_t n : {0u, 1u, 64u, 192u, 576u, 640u, 641u, 767u, 768u})
            std::printf("%u %u %zu\n", n, ua_mol_buffers(n), ua_mol_lds_bytes(n));
        return 0;
    }
    if (argc != 3) {
        std::fprintf(stderr, "usage: ua_molecule_rows SEED0 N | ua_molecule_rows lds\n");
        return 2;
    }
    const uint32_t s0 = (uint32_t)std::strtoul(argv[1], nullptr, 0), n = (uint32_t)std::strtoul(argv[2], nullptr, 0);
    for (uint32_t s = s0; s < s0 + n; s++) one(s);
    return 0;
}
