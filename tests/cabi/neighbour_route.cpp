// Drives choose_order_route of gorder_amd/csrc/order_route.h with OrderRouteIn::classes set, without a device (built by
// tests/test_neighbour_classes_cpu.py; tests/cabi/order_route.cpp never sets classes).
//
//   neighbour_route      one line per input: the input's number i, then
//                        family label npf mom speculative extras items_by_slot ua_mode direct maps_only map_accumulate | family of the same facts without classes
//   Input i: bit k of i is the k-th of: bond_tiles, acos, use_gather, leaflets, global_leaflets, spec_enabled, have_assignment,
//   every_frame_assigns, pbc, npf5, item_run; bits 11-12: axis - 1 ... the facts a handle with neighbour classes can have (no
//   maps, rows, geometry, dynamic or manual normals, united atoms or direct items: the setter refuses them).
#include <cstdint>
#include <cstdio>

#include "order_route.h"

using namespace gorder;

int main() {
    for (uint32_t i = 0; i < (1u << 13); i++) {
        OrderRouteIn in;
        uint32_t k = 0;
        auto bit = [&]() { return ((i >> k++) & 1u) != 0; };
        in.bond_tiles = bit(); in.acos = bit(); in.use_gather = bit(); in.leaflets = bit(); in.global_leaflets = bit();
        in.spec_enabled = bit(); in.have_assignment = bit(); in.every_frame_assigns = bit(); in.pbc = bit();
        in.npf5 = bit(); in.item_run = bit();
        in.axis = (int)((i >> 11) & 3u) - 1;
        in.max_window = 340u;
        OrderRouteIn plain = in;
        in.classes = true;
        const OrderRoute r = choose_order_route(in), q = choose_order_route(plain);
        std::printf("%u %d %s %d %d %d %d %d %d %d %d %d | %d\n", i, (int)r.family, r.label ? r.label : "-", r.npf, (int)r.mom, (int)r.speculative,
                    (int)r.extras, (int)r.items_by_slot, r.ua_mode, (int)r.direct, (int)r.maps_only, (int)r.map_accumulate, (int)q.family);
    }
    return 0;
}
