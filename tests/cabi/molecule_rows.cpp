// Drives gorder_amd/csrc/molecule_rows.h without a device (built by tests/test_molecule_rows_cpu.py, once plainly and once
// with -fsanitize=address,undefined).
//
//   molecule_rows lanes SEED N     N random plans (tiles, items, slot lists, group maps): the lane order and the run tables of
//                                  build_molecule_rows checked against brute force; prints "ok N <runs checked>" or the first
//                                  thing that is wrong (exit status 1)
//   molecule_rows groups           molecule_groups_check on the cases the C ABI refuses; one line per case
//   molecule_rows words            molecule_word_unpack on packed sums of random samples; prints "ok"
//   molecule_rows subrange         molecule_rows_subrange at its edges: "frames words bytes -> sub" per line
//   molecule_rows truncate         CollectStore::truncate (what takes a failed batch's rows back) against a plain vector
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <tuple>
#include <vector>

#include "collect_store.h"
#include "molecule_rows.h"

using namespace gorder;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("plan %u: ", plan_no);            \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            return 1;                                     \
        }                                                 \
    } while (0)

static int lanes(uint32_t seed, uint32_t n_plans) {
    std::mt19937 rng(seed);
    auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    uint64_t runs_checked = 0;
    for (uint32_t plan_no = 0; plan_no < n_plans; plan_no++) {
        const uint32_t n_acc = 1 + below(40), n_mol = 1 + below(50), n_groups = 1 + below(std::min(n_acc, 5u));
        // a random group map: every group gets a slot, the rest go to a random group or to none
        std::vector<uint32_t> group_of_slot(n_acc, kMolRowsNoGroup);
        {
            std::vector<uint32_t> order(n_acc);
            for (uint32_t s = 0; s < n_acc; s++) order[s] = s;
            std::shuffle(order.begin(), order.end(), rng);
            for (uint32_t g = 0; g < n_groups; g++) group_of_slot[order[g]] = g;
            for (uint32_t k = n_groups; k < n_acc; k++)
                if (below(4)) group_of_slot[order[k]] = below(n_groups);
        }
        // the same map through the CSR check
        {
            std::vector<uint32_t> begin(1, 0u), flat, back;
            for (uint32_t g = 0; g < n_groups; g++) {
                for (uint32_t s = 0; s < n_acc; s++)
                    if (group_of_slot[s] == g) flat.push_back(s);
                begin.push_back((uint32_t)flat.size());
            }
            const char *why = molecule_groups_check(begin.data(), flat.data(), n_groups, n_acc, back);
            CHECK(!why, "groups refused: %s", why ? why : "");
            CHECK(back == group_of_slot, "group_of_slot differs");
        }
        // random tiles: up to kBlock items each, a (slot, molecule) pair at most once in the whole plan
        std::vector<Tile> tiles;
        std::vector<Item> items;
        std::vector<uint32_t> tile_slots;
        std::set<std::pair<uint32_t, uint32_t>> used;
        const uint32_t n_tiles = 1 + below(6);
        for (uint32_t t = 0; t < n_tiles; t++) {
            Tile tile{};
            tile.atom0 = below(1000); tile.n_window = 1 + below(kMaxWindow);
            tile.item0 = (uint32_t)items.size(); tile.slot0 = (uint32_t)tile_slots.size();
            std::vector<uint32_t> slots;
            const uint32_t want = 1 + below(kBlock);
            for (uint32_t tries = 0; tries < 4 * want && tile.n_items < want; tries++) {
                const uint32_t slot = below(n_acc), mol = below(n_mol);
                if (!used.insert({slot, mol}).second) continue;
                uint32_t ls = 0;
                for (; ls < slots.size(); ls++)
                    if (slots[ls] == slot) break;
                if (ls == slots.size()) slots.push_back(slot);
                items.push_back({(uint16_t)below(tile.n_window), (uint16_t)below(tile.n_window), (uint16_t)ls, 0, mol});
                tile.n_items++;
            }
            if (!tile.n_items) continue;
            tile.n_slots = (uint32_t)slots.size();
            tile_slots.insert(tile_slots.end(), slots.begin(), slots.end());
            tiles.push_back(tile);
        }
        MolRows mr;
        build_molecule_rows(tiles, items, tile_slots, group_of_slot, n_groups, n_mol, mr);
        CHECK(mr.items.size() == items.size() && mr.run_begin.size() == tiles.size() + 1 && mr.run_begin[0] == 0, "sizes");
        CHECK(mr.n_groups == n_groups && mr.n_runs == mr.runs.size() && mr.run_begin.back() == mr.runs.size(), "counts");
        auto key = [](const Item &it) { return std::make_tuple(it.li, it.lj, it.lslot, it.pad, it.mol); };
        std::map<uint32_t, uint32_t> tiles_of_word;
        uint64_t brute_runs = 0;
        uint32_t brute_max_runs = 0;
        for (size_t t = 0; t < tiles.size(); t++) {
            const Tile &tile = tiles[t];
            auto group_of = [&](const Item &it) { return group_of_slot[tile_slots[tile.slot0 + it.lslot]]; };
            // every item exactly once per tile
            std::multiset<std::tuple<uint16_t, uint16_t, uint16_t, uint16_t, uint32_t>> a, b;
            for (uint32_t q = 0; q < tile.n_items; q++) { a.insert(key(items[tile.item0 + q])); b.insert(key(mr.items[tile.item0 + q])); }
            CHECK(a == b, "tile %zu: the lane order is no permutation of the tile's items", t);
            // brute force: the (group, molecule) pairs of the tile
            std::set<std::pair<uint32_t, uint32_t>> pairs;
            for (uint32_t q = 0; q < tile.n_items; q++)
                if (group_of(items[tile.item0 + q]) != kMolRowsNoGroup) pairs.insert({group_of(items[tile.item0 + q]), items[tile.item0 + q].mol});
            const uint32_t r0 = mr.run_begin[t], r1 = mr.run_begin[t + 1];
            CHECK(r1 >= r0 && r1 - r0 == pairs.size(), "tile %zu: %u runs for %zu (group, molecule) pairs: runs are not maximal", t, r1 - r0, pairs.size());
            brute_runs += pairs.size();
            brute_max_runs = std::max(brute_max_runs, (uint32_t)pairs.size());
            std::vector<uint32_t> covered(tile.n_items, 0);
            uint32_t next_lane = 0;
            for (uint32_t r = r0; r < r1; r++) {
                const MolRun &run = mr.runs[r];
                CHECK(run.n >= 1 && (uint32_t)run.lane0 + run.n <= tile.n_items, "tile %zu run %u: lanes out of the tile", t, r);
                CHECK(run.lane0 == next_lane, "tile %zu run %u: not in lane order (starts at %u, expected %u)", t, r, run.lane0, next_lane);
                next_lane = run.lane0 + run.n;
                CHECK(r == r0 || mr.runs[r - 1].word < run.word, "tile %zu run %u: destination words do not ascend", t, r);
                for (uint32_t j = 0; j < run.n; j++) {
                    const Item &it = mr.items[tile.item0 + run.lane0 + j];
                    const uint32_t g = group_of(it);
                    CHECK(g != kMolRowsNoGroup, "tile %zu run %u: an ungrouped item in a run", t, r);
                    CHECK(run.word == g * n_mol + it.mol, "tile %zu run %u: destination word %u, item wants %u", t, r, run.word, g * n_mol + it.mol);
                    covered[run.lane0 + j]++;
                }
                tiles_of_word[run.word]++;
                runs_checked++;
            }
            for (uint32_t q = 0; q < tile.n_items; q++) {
                const bool grouped = group_of(mr.items[tile.item0 + q]) != kMolRowsNoGroup;
                CHECK(covered[q] == (grouped ? 1u : 0u), "tile %zu lane %u: in %u runs", t, q, covered[q]);
                CHECK(grouped || q >= next_lane, "tile %zu lane %u: an ungrouped item ahead of the runs", t, q);
            }
            // stable: items of one (group, molecule) keep the order they had
            for (uint32_t r = r0; r < r1; r++) {
                const MolRun &run = mr.runs[r];
                std::vector<std::tuple<uint16_t, uint16_t, uint16_t, uint16_t, uint32_t>> got, want;
                for (uint32_t j = 0; j < run.n; j++) got.push_back(key(mr.items[tile.item0 + run.lane0 + j]));
                for (uint32_t q = 0; q < tile.n_items; q++) {
                    const Item &it = items[tile.item0 + q];
                    if (group_of(it) != kMolRowsNoGroup && group_of(it) * n_mol + it.mol == run.word) want.push_back(key(it));
                }
                CHECK(got == want, "tile %zu run %u: not stable", t, r);
            }
        }
        uint32_t brute_max_tiles = 0;
        for (const auto &kv : tiles_of_word) brute_max_tiles = std::max(brute_max_tiles, kv.second);
        CHECK(mr.n_runs == brute_runs, "n_runs %llu, brute force %llu", (unsigned long long)mr.n_runs, (unsigned long long)brute_runs);
        CHECK(mr.max_runs_per_tile == brute_max_runs, "max_runs_per_tile %u, brute force %u", mr.max_runs_per_tile, brute_max_runs);
        CHECK(mr.max_tiles_per_word == brute_max_tiles, "max_tiles_per_word %u, brute force %u", mr.max_tiles_per_word, brute_max_tiles);
    }
    std::printf("ok %u %llu\n", n_plans, (unsigned long long)runs_checked);
    return 0;
}

static void groups() {
    struct Case { const char *name; std::vector<uint32_t> begin, slots; uint32_t n_acc; };
    std::vector<uint32_t> big_begin{0, 2048}, big(2048);
    for (uint32_t k = 0; k < 2048; k++) big[k] = k;
    std::vector<uint32_t> fit_begin{0, 2047}, fit(2047);
    for (uint32_t k = 0; k < 2047; k++) fit[k] = k;
    const std::vector<Case> cases = {
        {"fine", {0, 2, 3}, {0, 1, 5}, 6},
        {"empty", {0, 2, 2}, {0, 1}, 6},
        {"range", {0, 2}, {0, 6}, 6},
        {"twice", {0, 2, 3}, {0, 1, 1}, 6},
        {"twice_in_one", {0, 2}, {3, 3}, 6},
        {"descending", {0, 2, 1}, {0, 1, 2}, 6},
        {"first", {1, 2}, {0, 1, 2}, 6},
        {"2048", big_begin, big, 4096},
        {"2047", fit_begin, fit, 4096},
    };
    for (const Case &c : cases) {
        std::vector<uint32_t> gos;
        const char *why = molecule_groups_check(c.begin.data(), c.slots.data(), (uint32_t)c.begin.size() - 1, c.n_acc, gos);
        std::printf("%s: %s\n", c.name, why ? why : "ok");
    }
}

static int words() {
    std::mt19937_64 rng(7);
    for (int trial = 0; trial < 20000; trial++) {
        const uint32_t n = (uint32_t)(rng() % (kMolRowsMaxGroupSlots + 1));
        uint64_t w = 0;
        int64_t want = 0;
        for (uint32_t k = 0; k < n; k++) {
            const int tick = trial % 3 == 0 ? -500000 : trial % 3 == 1 ? 1000000 : (int)(rng() % 1500001) - 500000;
            w += ((uint64_t)1 << kMolRowsCountShift) + (uint64_t)(int64_t)tick;
            want += tick;
        }
        int64_t s;
        uint64_t c;
        molecule_word_unpack(w, s, c);
        if (s != want || c != n || (int64_t)(int32_t)s != s) {
            std::printf("trial %d: %u samples, sum %lld: unpacked %lld, %llu\n", trial, n, (long long)want, (long long)s, (unsigned long long)c);
            return 1;
        }
    }
    std::printf("ok\n");
    return 0;
}

static void subrange() {
    for (uint32_t nf : {1u, 2u, 11u, 4000u})
        for (size_t words : {(size_t)1, (size_t)104, (size_t)512, (size_t)83333})
            for (size_t bytes : {(size_t)1, (size_t)1664, (size_t)8192, (size_t)1 << 30})
                std::printf("%u %zu %zu -> %u\n", nf, words, bytes, molecule_rows_subrange(nf, words, bytes));
}

// rows of 24 bytes in chunks of 5 rows: append batches, truncate to random lengths, append again; the rows read back must be
// the model's, chunk memory must never move or grow while earlier chunks have room
static int truncate() {
    std::mt19937 rng(11);
    CollectStore store;
    store.configure(24, CollectAlloc{[](size_t b) { return std::malloc(b); }, [](void *p) { std::free(p); }}, 5 * 24);
    std::vector<uint64_t> model;
    uint64_t next = 100;
    for (int step = 0; step < 400; step++) {
        if (rng() % 3 == 0) {
            const uint64_t keep = rng() % (model.size() + 2);      // (may exceed the rows: then nothing happens)
            store.truncate(keep);
            if (keep < model.size()) model.resize((size_t)keep);
        } else {
            const size_t n = 1 + rng() % 12;
            std::vector<uint64_t> frames(n);
            for (size_t k = 0; k < n; k++) frames[k] = next++;
            std::vector<CollectPiece> pieces;
            if (!store.reserve(frames.data(), n, pieces)) { std::printf("reserve failed\n"); return 1; }
            size_t k = 0;
            for (const CollectPiece &pc : pieces)
                for (size_t r = 0; r < pc.rows; r++, k++) {
                    uint64_t row[3] = {frames[k], ~frames[k], frames[k] * 3};
                    std::memcpy(static_cast<char *>(pc.host) + r * 24, row, 24);
                }
            if (k != n) { std::printf("step %d: pieces hold %zu rows of %zu\n", step, k, n); return 1; }
            model.insert(model.end(), frames.begin(), frames.end());
        }
        if (store.n_rows() != model.size() || store.frames() != model) { std::printf("step %d: frames differ\n", step); return 1; }
        bool ok = true;
        uint64_t seen = 0;
        store.for_each_row([&](uint64_t r, const void *row) {
            uint64_t v[3];
            std::memcpy(v, row, 24);
            ok = ok && r == seen && r < model.size() && v[0] == model[r] && v[1] == ~model[r] && v[2] == model[r] * 3;
            seen++;
        });
        if (!ok || seen != model.size()) { std::printf("step %d: rows differ\n", step); return 1; }
    }
    std::printf("ok %zu\n", store.n_chunks());
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && std::strcmp(argv[1], "truncate") == 0) return truncate();
    if (argc == 4 && std::strcmp(argv[1], "lanes") == 0)
        return lanes((uint32_t)std::strtoul(argv[2], nullptr, 0), (uint32_t)std::strtoul(argv[3], nullptr, 0));
    if (argc == 2 && std::strcmp(argv[1], "groups") == 0) { groups(); return 0; }
    if (argc == 2 && std::strcmp(argv[1], "words") == 0) return words();
    if (argc == 2 && std::strcmp(argv[1], "subrange") == 0) { subrange(); return 0; }
    std::fprintf(stderr, "usage: molecule_rows lanes SEED N | groups | words | subrange | truncate\n");
    return 2;
}
