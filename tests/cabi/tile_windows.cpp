// Runs gorder_amd/csrc/plan.h's build_plan on index tables read from stdin and prints what the planner made of them (built with
// -fsanitize=address,undefined by tests/test_tile_windows_cpu.py, which holds the expected values).  No device, no HIP.
//
// Input, whitespace-separated unsigned integers (tests/tile_windows.py: plan_text):
//   n_atoms n_types leaflets_method n_membrane   membrane[n_membrane]
//   per molecule type: n_molecules n_bond_types has_heads   bonds[n_bond_types][n_molecules][2]   heads[n_molecules] if has_heads
// Output, one record per line:
//   plan status S selfcheck C max_window W n_direct D spec_ok B n_tiles T n_acc A n_mol M
//   tile K atom0 n_window n_items n_slots
//   items K li lj slot mol  li lj slot mol ...      the tile's items in lane order, window-relative atoms, accumulator slot
//   own K lo hi                                     with spec_ok only: the atoms tile K owns
//   heads K rel mol  rel mol ...                    with spec_ok only: the heads tile K owns (window-relative atom, molecule)
//   direct i j slot mol
#include <cstdint>
#include <cstdio>
#include <vector>

#include "plan.h"

using namespace gorder;

static bool read_u32(uint32_t &v) {
    unsigned long long x;
    if (std::scanf("%llu", &x) != 1 || x > 0xffffffffull) return false;
    v = (uint32_t)x;
    return true;
}

int main() {
    uint32_t n_atoms, n_types, method, n_membrane;
    if (!read_u32(n_atoms) || !read_u32(n_types) || !read_u32(method) || !read_u32(n_membrane)) return 2;
    if (n_types > (1u << 20) || n_membrane > (1u << 26)) return 2;
    std::vector<uint32_t> membrane(n_membrane);
    for (uint32_t &m : membrane)
        if (!read_u32(m)) return 2;
    std::vector<gorder_moltype_t> types(n_types);
    std::vector<std::vector<uint32_t>> bonds(n_types), heads(n_types);
    for (uint32_t t = 0; t < n_types; t++) {
        uint32_t n_mol, n_bt, has_heads;
        if (!read_u32(n_mol) || !read_u32(n_bt) || !read_u32(has_heads)) return 2;
        if ((uint64_t)n_mol * n_bt > (1u << 24)) return 2;
        bonds[t].resize(2 * (size_t)n_mol * n_bt);
        for (uint32_t &b : bonds[t])
            if (!read_u32(b)) return 2;
        if (has_heads) {
            heads[t].resize(n_mol);
            for (uint32_t &h : heads[t])
                if (!read_u32(h)) return 2;
        }
        gorder_moltype_t mt{};
        mt.n_molecules = n_mol;
        mt.n_bond_types = n_bt;
        mt.bonds = bonds[t].empty() ? nullptr : bonds[t].data();
        mt.heads = has_heads ? heads[t].data() : nullptr;
        types[t] = mt;
    }
    gorder_tables_t tb{};
    tb.n_atoms = n_atoms;
    tb.n_molecule_types = n_types;
    tb.molecule_types = types.data();
    tb.handle_pbc = 1;
    tb.normal[2] = 1.0f;
    tb.leaflets.method = method;
    tb.leaflets.normal_dim = 2;
    tb.leaflets.frequency = 1;
    tb.leaflets.n_membrane = n_membrane;
    tb.leaflets.membrane = membrane.empty() ? nullptr : membrane.data();

    Plan p;
    const int st = build_plan(tb, false, p);
    const int check = st == GORDER_OK ? selfcheck_plan(tb, p) : -1;
    std::printf("plan status %d selfcheck %d max_window %u n_direct %zu spec_ok %d n_tiles %zu n_acc %u n_mol %u\n", st, check, p.max_window,
                p.direct.size(), p.spec_ok ? 1 : 0, p.tiles.size(), p.n_acc, p.n_mol_total);
    if (st != GORDER_OK) return 0;
    for (size_t k = 0; k < p.tiles.size(); k++) {
        const Tile &t = p.tiles[k];
        std::printf("tile %zu %u %u %u %u\n", k, t.atom0, t.n_window, t.n_items, t.n_slots);
        std::printf("items %zu", k);
        for (uint32_t q = 0; q < t.n_items; q++) {
            const Item &it = p.items[t.item0 + q];
            std::printf(" %u %u %u %u", (unsigned)it.li, (unsigned)it.lj, p.tile_slots[t.slot0 + it.lslot], it.mol);
        }
        std::printf("\n");
        if (p.spec_ok) {
            std::printf("own %zu %u %u\n", k, p.own[2 * k], p.own[2 * k + 1]);
            std::printf("heads %zu", k);
            for (uint32_t q = p.own_head_begin[k]; q < p.own_head_begin[k + 1]; q++) std::printf(" %u %u", p.own_heads[2 * q], p.own_heads[2 * q + 1]);
            std::printf("\n");
        }
    }
    for (const DirectItem &d : p.direct) std::printf("direct %u %u %u %u\n", d.i, d.j, d.slot, d.mol);
    return 0;
}
