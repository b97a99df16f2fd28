// Drives gorder_amd/csrc/order_route.h without a device (built with -fsanitize=address,undefined by
// tests/test_order_route_cpu.py, which holds the expected values).
//
//   order_route routes LO HI   one line per input LO <= i < HI: the route of input i as six hex digits
//   order_route chunks         one line per call of a chunking function: its name, its arguments, its result
//
// Input i: bit k of i is the k-th fact of kBits below (24 facts: every boolean a predicate reads, frames_per_stage 4 / 8,
// a window of 340 / 341 atoms = the last that fits four prefetch registers and the first that does not).  pbc and axis
// stay at their defaults: no predicate reads them, they are not part of the route.
// Route word: family (3 bits, BondFamily's order) | npf == 5 | mom | tw_maps | maps_only | items_by_slot |
// ua_mode + 1 (3 bits) | ua_fast | map_accumulate | direct | fixup_ac | fixup_tw | speculative | extras |
// label (3 bits: position in kLabels, 7 = none of them).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "order_route.h"

using namespace gorder;

static OrderRouteIn input(uint32_t i) {
    OrderRouteIn in;
    uint32_t k = 0;
    auto bit = [&]() { return ((i >> k++) & 1u) != 0; };
    in.maps = bit(); in.map_staged = bit(); in.tw = bit(); in.geom = bit(); in.dyn_or_manual = bit(); in.acos = bit();
    in.use_gather = bit(); in.item_run = bit();
    in.frames_per_stage = bit() ? 8 : 4;
    in.max_window = bit() ? 341u : 340u;
    in.npf5 = bit(); in.tw_gather = bit(); in.maps_gather = bit();
    in.bond_tiles = bit(); in.ua_tiles = bit(); in.direct_items = bit(); in.ua_fast_flag = bit(); in.leaflets = bit();
    in.global_leaflets = bit(); in.spec_enabled = bit(); in.have_assignment = bit(); in.every_frame_assigns = bit();
    in.manual_frames = bit(); in.normal_table = bit();
    return in;
}

static const char *const kLabels[] = {"", "k_bonds_tiled", "k_bonds_gather", "k_bonds_tiled_tw", "k_bonds_tiled_maps", "k_bonds_extras"};

static uint32_t word(const OrderRoute &r) {
    uint32_t label = 7;
    for (uint32_t l = 0; l < 6; l++)
        if (std::strcmp(r.label ? r.label : "", kLabels[l]) == 0) label = l;
    if (r.npf != 4 && r.npf != 5) std::exit(2);
    if (r.ua_mode < -1 || r.ua_mode > 3) std::exit(2);
    return (uint32_t)r.family | (r.npf == 5) << 3 | r.mom << 4 | r.tw_maps << 5 | r.maps_only << 6 | r.items_by_slot << 7 |
           (uint32_t)(r.ua_mode + 1) << 8 | r.ua_fast << 11 | r.map_accumulate << 12 | r.direct << 13 | r.fixup_ac << 14 |
           r.fixup_tw << 15 | r.speculative << 16 | r.extras << 17 | label << 18;
}

static void chunks() {
    const uint32_t cap = 1536;      // co-resident workgroups: 12 x cap = 18432, 8 x cap = 12288
    for (uint32_t G : {4u, 8u})
        for (uint32_t nf : {1u, G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1, (4 * G - 1) * G, 4 * G * G, 4 * G * G + 1, 100u, 3000u, 100000u})
            for (uint32_t nt : {1u, 7u, 96u, 18432u, 18433u, 50000u})
                for (uint32_t target : {0u, 1u, 64u, 5000u}) {
                    const FrameChunks c = tiled_chunks(nf, G, nt, target, cap);
                    std::printf("tiled %u %u %u %u %u -> %u %u\n", nf, G, nt, target, cap, c.frames_per_chunk, c.n_chunks);
                }
    for (uint32_t nf : {1u, 3u, 4u, 5u, 15u, 16u, 17u, 31u, 32u, 33u, 100u, 3000u})
        for (uint32_t nt : {1u, 96u, 12288u, 12289u, 50000u})
            for (uint32_t target : {0u, 1u, 500u})
                for (int staged = 0; staged < 2; staged++)
                    for (int whole = 0; whole < 2; whole++) {
                        const FrameChunks c = extras_chunks(nf, nt, target, cap, staged, whole);
                        std::printf("extras %u %u %u %u %d %d -> %u %u\n", nf, nt, target, cap, staged, whole, c.frames_per_chunk, c.n_chunks);
                    }
    for (uint32_t nf : {1u, 2u, 7u, 100u, 3000u})
        for (uint32_t bpc : {1u, 3u, 2047u, 2048u, 2049u})
            for (uint32_t target : {0u, 1u, 500u}) {
                const FrameChunks c = direct_chunks(nf, bpc, target);
                std::printf("direct %u %u %u -> %u %u\n", nf, bpc, target, c.frames_per_chunk, c.n_chunks);
            }
    for (uint32_t nf : {1u, 15u, 16u, 17u, 31u, 32u, 33u, 100u, 3000u})
        for (uint32_t n_acc : {0u, 1u, 3u, 100u, 512u, 513u, 2000u})
            for (uint32_t forced : {0u, 1u, 4u, 1000u}) {
                const FrameChunks c = map_chunks(nf, n_acc, forced);
                std::printf("map %u %u %u -> %u %u\n", nf, n_acc, forced, c.frames_per_chunk, c.n_chunks);
            }
    for (uint32_t nf : {1u, 16u, 100u, 3000u})
        for (int maps = 0; maps < 2; maps++)
            for (int staged = 0; staged <= maps; staged++)
                for (uint64_t limit : {(uint64_t)2, (uint64_t)1000, (uint64_t)1 << 20, (uint64_t)1 << 40})
                    for (uint32_t max_mol : {1u, 7u, 256u})
                        for (size_t words : {(size_t)256, (size_t)3 << 20, (size_t)1 << 27, ((size_t)1 << 27) + 1}) {
                            const uint32_t sub = map_subrange(nf, maps, staged, limit, max_mol, words);
                            std::printf("sub %u %d %d %llu %u %zu -> %u\n", nf, maps, staged, (unsigned long long)limit, max_mol, words, sub);
                        }
}

int main(int argc, char **argv) {
    if (argc == 2 && std::strcmp(argv[1], "chunks") == 0) {
        chunks();
        return 0;
    }
    if (argc != 4 || std::strcmp(argv[1], "routes") != 0) {
        std::fprintf(stderr, "usage: order_route routes LO HI | order_route chunks\n");
        return 2;
    }
    const uint32_t lo = (uint32_t)std::strtoul(argv[2], nullptr, 0), hi = (uint32_t)std::strtoul(argv[3], nullptr, 0);
    std::string out;
    out.reserve(1u << 20);
    char line[16];
    for (uint32_t i = lo; i < hi; i++) {
        std::snprintf(line, sizeof line, "%06x\n", word(choose_order_route(input(i))));
        out += line;
        if (out.size() >= (1u << 20) - 16 || i + 1 == hi) {
            if (std::fwrite(out.data(), 1, out.size(), stdout) != out.size()) return 1;
            out.clear();
        }
    }
    return 0;
}
