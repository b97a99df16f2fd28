// Drives the united-atom kernel choice of gorder_amd/csrc/order_route.h without a device (built with
// -fsanitize=address,undefined by tests/test_ua_samples_cpu.py, which holds the expected values).
//
//   ua_samples_route flag       every one of the 2^24 inputs of tests/cabi/order_route.cpp (same bit order), dist = mol_rows = false:
//                               the route with and without ua_samples_flag, field by field -> "inputs differing wrong_kernel"
//   ua_samples_route kernels    the facts a handle with an order histogram or molecule rows can meet (the setters refuse maps,
//                               per-frame rows, dynamic or manual normals, direct items and the fast construction; a geometry
//                               selection goes with the histogram only), 2^16 inputs x flag x {none, dist, mol_rows}: one line
//                               "bits flag feature ua_kernel family ua_mode extras same" each, `same` = every field but
//                               ua_kernel equals the flag-less route's
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "order_route.h"

using namespace gorder;

static OrderRouteIn input24(uint32_t i) {       // (tests/cabi/order_route.cpp: input())
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

// every field but ua_kernel
static bool same_but_kernel(const OrderRoute &a, const OrderRoute &b) {
    return a.family == b.family && a.label == b.label && a.npf == b.npf && a.mom == b.mom && a.tw_maps == b.tw_maps &&
           a.maps_only == b.maps_only && a.items_by_slot == b.items_by_slot && a.extras == b.extras && a.ua_mode == b.ua_mode &&
           a.ua_fast == b.ua_fast && a.map_accumulate == b.map_accumulate && a.direct == b.direct && a.speculative == b.speculative &&
           a.fixup_ac == b.fixup_ac && a.fixup_tw == b.fixup_tw;
}

static int flag_alone() {
    uint64_t differing = 0, wrong_kernel = 0;
    for (uint32_t i = 0; i < (1u << 24); i++) {
        OrderRouteIn in = input24(i);
        const OrderRoute off = choose_order_route(in);
        in.ua_samples_flag = true;
        const OrderRoute on = choose_order_route(in);
        if (!same_but_kernel(on, off) || on.ua_kernel != off.ua_kernel) differing++;
        if (off.ua_kernel != (in.ua_tiles ? UaKernel::Extras : UaKernel::None)) wrong_kernel++;
        if ((off.ua_mode >= 0) != (off.ua_kernel != UaKernel::None)) wrong_kernel++;
    }
    std::printf("%u %llu %llu\n", 1u << 24, (unsigned long long)differing, (unsigned long long)wrong_kernel);
    return 0;
}

static int kernels() {
    std::string out;
    char line[96];
    for (uint32_t i = 0; i < (1u << 16); i++) {
        OrderRouteIn base;
        uint32_t k = 0;
        auto bit = [&]() { return ((i >> k++) & 1u) != 0; };
        base.acos = bit(); base.geom = bit(); base.use_gather = bit(); base.item_run = bit();
        base.frames_per_stage = bit() ? 8 : 4;
        base.max_window = bit() ? 341u : 340u;
        base.npf5 = bit(); base.tw_gather = bit(); base.maps_gather = bit();
        base.bond_tiles = bit(); base.ua_tiles = bit(); base.leaflets = bit(); base.global_leaflets = bit(); base.spec_enabled = bit();
        base.have_assignment = bit(); base.every_frame_assigns = bit();
        for (int feature = 0; feature < 3; feature++) {        // 0: neither, 1: dist, 2: mol_rows
            if (feature == 2 && base.geom) continue;            // (the rows refuse a geometry selection)
            OrderRouteIn in = base;
            in.dist = feature == 1; in.mol_rows = feature == 2;
            const OrderRoute off = choose_order_route(in);
            for (int flag = 0; flag < 2; flag++) {
                in.ua_samples_flag = flag != 0;
                const OrderRoute r = choose_order_route(in);
                std::snprintf(line, sizeof line, "%u %d %d %d %d %d %d %d\n", i, flag, feature, (int)r.ua_kernel, (int)r.family, r.ua_mode,
                              (int)r.extras, (int)same_but_kernel(r, off));
                out += line;
            }
        }
        if (out.size() >= (1u << 20) || i + 1 == (1u << 16)) {
            if (std::fwrite(out.data(), 1, out.size(), stdout) != out.size()) return 1;
            out.clear();
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && std::strcmp(argv[1], "flag") == 0) return flag_alone();
    if (argc == 2 && std::strcmp(argv[1], "kernels") == 0) return kernels();
    std::fprintf(stderr, "usage: ua_samples_route flag | ua_samples_route kernels\n");
    return 2;
}
