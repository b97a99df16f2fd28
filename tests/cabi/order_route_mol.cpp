// Drives choose_order_route of gorder_amd/csrc/order_route.h with OrderRouteIn::mol_rows set (built with
// -fsanitize=address,undefined by tests/test_molecule_rows_cpu.py; tests/cabi/order_route.cpp sweeps everything else and never
// sets it).
//
//   order_route_mol    one line per input: the input's number i, then
//                      family label npf mom speculative extras items_by_slot ua_mode direct | family of the same facts without mol_rows
// Input i: bit k of i is the k-th of: bond_tiles, acos, use_gather, leaflets, global_leaflets, spec_enabled, have_assignment,
// every_frame_assigns, pbc, wide (a window of 341 atoms instead of 340), npf5, item_run; bits 12-13: axis - 1 ... the facts a
// handle with molecule rows can have (no maps, per-frame rows, geometry, dynamic or manual normals, united atoms, direct items).
#include <cstdint>
#include <cstdio>

#include "order_route.h"

using namespace gorder;

int main() {
    for (uint32_t i = 0; i < (1u << 14); i++) {
        OrderRouteIn in;
        uint32_t k = 0;
        auto bit = [&]() { return ((i >> k++) & 1u) != 0; };
        in.bond_tiles = bit(); in.acos = bit(); in.use_gather = bit(); in.leaflets = bit(); in.global_leaflets = bit();
        in.spec_enabled = bit(); in.have_assignment = bit(); in.every_frame_assigns = bit(); in.pbc = bit();
        in.max_window = bit() ? 341u : 340u;
        in.npf5 = bit(); in.item_run = bit();
        in.axis = (int)((i >> 12) & 3u) - 1;
        OrderRouteIn plain = in;
        in.mol_rows = true;
        const OrderRoute r = choose_order_route(in), q = choose_order_route(plain);
        std::printf("%u %d %s %d %d %d %d %d %d %d | %d\n", i, (int)r.family, r.label ? r.label : "-", r.npf, (int)r.mom, (int)r.speculative,
                    (int)r.extras, (int)r.items_by_slot, r.ua_mode, (int)r.direct, (int)q.family);
    }
    return 0;
}
