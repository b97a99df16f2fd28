// switches.h — the development switches of the library: environment variables that pick a route, a launch geometry or a
// buffer size for A/B runs and tests.  None changes results.  kSwitches is the one list of them; read_switches reads every
// one exactly once, gorder_hip_create keeps the answer in the handle (gorder_hip_handle::sw) and nothing looks at the
// environment afterwards (gorder_hip_plan_tables, which has no handle, reads them at its call).  No HIP, no handle:
// tests/cabi/switches.cpp drives the parsing without a device.
#ifndef GORDER_SWITCHES_H
#define GORDER_SWITCHES_H
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

#include "neighbour_classes.h"
#include "order_route.h"

namespace gorder {

struct Switches {
    // the order kernels
    bool kernel_gather = false;         // k_bonds_gather (L1 gather) instead of LDS staging
    uint32_t wg_target = 0;             // the workgroup count the chunking aims at; 0: not set
    bool npf5 = false, tw_gather = false, maps_gather = false;      // OrderRouteIn's switches (order_route.h)
    bool force_direct = false;          // build_plan: every bond a direct item, no tiles
    bool ua_slot_waves = false;         // build_plan: united-atom waves of one slot, not 4 slots x 16 molecules
    uint32_t replicas = 32;             // copies of the accumulators the kernels add into
    // ordermaps
    bool map_direct = false;            // one atomic per sample even where a slot's packed map fits LDS
    uint32_t map_chunks = 0;            // chunks of frames of k_map_accumulate; 0: not forced
    long map_fold_limit = 0;            // samples a packed word may hold before a fold, as written: the site keeps [2, kMapFoldLimit]
    // leaflets
    bool no_speculate = false;          // global leaflets: never one read for leaflets + order parameters
    bool leaflets_generic = false;      // the membrane's index list even where the membrane is the whole frame in order
    uint32_t spherical_slab = 0;        // lowers the assignment frames per launch of k_leaflets_spherical; 0: not set
    bool cluster_stored_w = false;      // S v reads W stored once a frame instead of recomputing it
    uint32_t local_slab = 0;            // cap on the assignment frames per launch group (local leaflets, dynamic normals), >= 4; 0: not set
    bool local_atoms_only = false;      // no rows of cells: every candidate atom by atom
    bool local_three_kernels = false;   // cell list by k_local_bin / _scan / _scatter, as beyond kLocalBuildMax atoms
    bool local_no_decide = false;       // no k_local_decide before the rows kernel
    bool local_no_sums = false;         // no k_local_sums: the cell list for every frame
    bool local_no_prune = false;        // the exact path for every head, no bound
    bool local_decide_nothing = false;  // the bound leaves every head open (a measuring aid)
    // radial shells, order distributions, neighbour classes, bond reorientation, per-molecule rows
    bool radial_direct = false;         // per-sample global atomics even where the table fits LDS
    bool dist_direct = false;           // likewise
    uint32_t dist_samples_per_word = kDistSamplesPerWord;       // dist_chunks
    bool nb_direct = false;             // likewise
    uint32_t nb_subrange = 0;           // class_subrange's forced length; 0: not set
    uint64_t nb_row_bytes = kClassRowBytes;     // the most the class rows take (tests set it small)
    uint32_t corr_subrange = 0;         // corr_subrange's forced length; 0: not set
    bool corr_grid_chunks = false;      // a workgroup of k_bond_corr walks every group of lags of its chunk
    size_t mol_rows_staging = (size_t)1 << 30;  // bytes of the per-molecule rows' device staging (tests set it small)
    // gorder_hip_run_trajectory, device decode
    uint32_t prefix_q16 = 0;            // a fixed part of every XTC block to copy, in 1/65536, whatever it leads to; 0: not set
    bool no_prefix = false;             // copy whole blocks, learn no part
};

struct Switch {
    const char *name;
    void (*parse)(Switches &, const char *);    // (the value, or nullptr where the variable is not set)
    const char *meaning;
};

namespace switch_parse {
inline bool on(const char *v) { return v && *v && strcmp(v, "0") != 0; }
inline bool is(const char *v, const char *word) { return v && strcmp(v, word) == 0; }
}   // namespace switch_parse

// in the order of the struct
inline constexpr Switch kSwitches[] = {
    {"GORDER_HIP_KERNEL", [](Switches &s, const char *v) { s.kernel_gather = switch_parse::is(v, "gather"); },
     "=gather: the L1-gather order kernel instead of LDS staging (plain bond tiles only)"},
    {"GORDER_HIP_WG_TARGET", [](Switches &s, const char *v) { if (v && atoi(v) > 0) s.wg_target = (uint32_t)atoi(v); },
     "=N: the workgroup count the frame chunks of a batch aim at"},
    {"GORDER_HIP_NPF5", [](Switches &s, const char *v) { s.npf5 = switch_parse::on(v); },
     "five prefetch registers in the tiled kernels where four would do"},
    {"GORDER_HIP_TW_GATHER", [](Switches &s, const char *v) { s.tw_gather = switch_parse::on(v); },
     "per-frame rows through k_bonds_extras instead of k_bonds_tiled_tw"},
    {"GORDER_HIP_MAPS_GATHER", [](Switches &s, const char *v) { s.maps_gather = switch_parse::on(v); },
     "staged ordermaps through k_bonds_extras instead of k_bonds_tiled_maps"},
    {"GORDER_HIP_FORCE_DIRECT", [](Switches &s, const char *v) { s.force_direct = switch_parse::on(v); },
     "every bond a direct item (k_bonds_direct), no tiles"},
    {"GORDER_HIP_UA_SLOT_WAVES", [](Switches &s, const char *v) { s.ua_slot_waves = switch_parse::on(v); },
     "united-atom waves of one slot instead of 4 slots x 16 molecules"},
    {"GORDER_HIP_REPLICAS", [](Switches &s, const char *v) { if (v && atoi(v) >= 1 && atoi(v) <= 1024) s.replicas = (uint32_t)atoi(v); },
     "=N in [1, 1024]: copies of the accumulators the kernels add into (32)"},
    {"GORDER_HIP_MAP_DIRECT", [](Switches &s, const char *v) { s.map_direct = switch_parse::on(v); },
     "ordermaps by one atomic per sample even where a slot's map fits LDS"},
    {"GORDER_HIP_MAP_CHUNKS", [](Switches &s, const char *v) { if (v) s.map_chunks = (uint32_t)std::max(1, atoi(v)); },
     "=N: chunks of frames of k_map_accumulate"},
    {"GORDER_HIP_MAP_FOLD_LIMIT", [](Switches &s, const char *v) { if (v) s.map_fold_limit = atol(v); },
     "=N in [2, 2^21]: samples a packed ordermap word may hold before it is folded (tests)"},
    {"GORDER_HIP_NO_SPECULATE", [](Switches &s, const char *v) { s.no_speculate = switch_parse::on(v); },
     "global leaflets by k_leaflets_global first, never one read for leaflets and order parameters"},
    {"GORDER_HIP_LEAFLETS_GENERIC", [](Switches &s, const char *v) { s.leaflets_generic = switch_parse::on(v); },
     "the membrane's index list even where the membrane is every atom of the frame in order"},
    {"GORDER_HIP_SPHERICAL_SLAB", [](Switches &s, const char *v) { if (v) s.spherical_slab = (uint32_t)std::max(1, atoi(v)); },
     "=N: at most N assignment frames per launch of k_leaflets_spherical (tests; only lowers the cap)"},
    {"GORDER_HIP_CLUSTER_STORED_W", [](Switches &s, const char *v) { s.cluster_stored_w = switch_parse::on(v); },
     "spectral clustering reads W stored once a frame instead of recomputing it"},
    {"GORDER_HIP_LOCAL_SLAB", [](Switches &s, const char *v) { if (v) s.local_slab = (uint32_t)std::max(4, atoi(v)); },
     "=N >= 4: at most N assignment frames per launch group of local leaflets and dynamic normals"},
    {"GORDER_HIP_LOCAL_ATOMS_ONLY", [](Switches &s, const char *v) { s.local_atoms_only = switch_parse::on(v); },
     "local leaflets without rows of cells: every candidate atom by atom (k_local_flags)"},
    {"GORDER_HIP_LOCAL_THREE_KERNELS", [](Switches &s, const char *v) { s.local_three_kernels = switch_parse::on(v); },
     "the cell list by k_local_bin, k_local_scan and k_local_scatter instead of k_local_build"},
    {"GORDER_HIP_LOCAL_NO_DECIDE", [](Switches &s, const char *v) { s.local_no_decide = switch_parse::on(v); },
     "local leaflets without k_local_decide: the rows kernel for every frame"},
    {"GORDER_HIP_LOCAL_NO_SUMS", [](Switches &s, const char *v) { s.local_no_sums = switch_parse::on(v); },
     "local leaflets without k_local_sums: the cell list for every frame"},
    {"GORDER_HIP_LOCAL_NO_PRUNE", [](Switches &s, const char *v) { s.local_no_prune = switch_parse::on(v); },
     "local leaflets: the exact path for every head, no bound"},
    {"GORDER_HIP_LOCAL_DECIDE_NOTHING", [](Switches &s, const char *v) { s.local_decide_nothing = switch_parse::on(v); },
     "local leaflets: the bound leaves every head open (a measuring aid)"},
    {"GORDER_HIP_RADIAL_DIRECT", [](Switches &s, const char *v) { s.radial_direct = switch_parse::on(v); },
     "radial shells by per-sample global atomics even where the table fits LDS"},
    {"GORDER_HIP_DIST_DIRECT", [](Switches &s, const char *v) { s.dist_direct = switch_parse::on(v); },
     "order distributions by per-sample global atomics even where the table fits LDS"},
    {"GORDER_HIP_DIST_SAMPLES_PER_WORD",
     [](Switches &s, const char *v) { if (v) s.dist_samples_per_word = (uint32_t)std::min(std::max(0, atoi(v)), 1 << 16); },
     "=N in [0, 65536]: samples per table word the chunks of k_bonds_dist are cut for (8)"},
    {"GORDER_HIP_NB_DIRECT", [](Switches &s, const char *v) { s.nb_direct = switch_parse::on(v); },
     "neighbour classes by per-sample global atomics even where the table fits LDS"},
    {"GORDER_HIP_NB_SUBRANGE", [](Switches &s, const char *v) { if (v) s.nb_subrange = (uint32_t)std::max(0, atoi(v)); },
     "=N: neighbour classes in sub-ranges of at most N frames"},
    {"GORDER_HIP_NB_ROW_BYTES", [](Switches &s, const char *v) { if (v && atoll(v) > 0) s.nb_row_bytes = (uint64_t)atoll(v); },
     "=N: the most bytes the class rows of one sub-range take (1 GiB; tests set it small)"},
    {"GORDER_HIP_CORR_SUBRANGE", [](Switches &s, const char *v) { if (v) s.corr_subrange = (uint32_t)std::max(0, atoi(v)); },
     "=N: bond reorientation in sub-ranges of at most N frames"},
    {"GORDER_HIP_CORR_GRID", [](Switches &s, const char *v) { s.corr_grid_chunks = switch_parse::is(v, "chunks"); },
     "=chunks: a workgroup of k_bond_corr walks every group of lags of its chunk"},
    {"GORDER_HIP_MOL_ROWS_STAGING", [](Switches &s, const char *v) { if (v && atoll(v) > 0) s.mol_rows_staging = (size_t)atoll(v); },
     "=N: bytes of the per-molecule rows' device staging (1 GiB; tests set it small)"},
    {"GORDER_HIP_PREFIX_Q16", [](Switches &s, const char *v) { if (v) s.prefix_q16 = (uint32_t)std::max(1l, std::min(65536l, atol(v))); },
     "=N in [1, 65536]: device decode copies N/65536 of every XTC block, whatever it leads to (tests)"},
    {"GORDER_HIP_NO_PREFIX", [](Switches &s, const char *v) { s.no_prefix = switch_parse::on(v); },
     "device decode copies whole XTC blocks and learns no part"},
};

// `get`: anything callable as const char *(const char *); the library passes ::getenv
template <typename Getenv> Switches read_switches(Getenv get) {
    Switches s;
    for (const Switch &w : kSwitches) w.parse(s, get(w.name));
    return s;
}

}   // namespace gorder
#endif
