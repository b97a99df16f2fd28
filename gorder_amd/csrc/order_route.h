// order_route.h — which kernels the order pass of a batch runs and how it cuts the frames into chunks, decided once per
// batch (gorder_hip_submit_device) from plain facts about the handle, the plan and the batch; launch_orders launches what
// the route says.  No HIP, no handle: tests/cabi/order_route.cpp drives every input without a device.
//   bond tiles, no extras (maps / per-frame rows / geometry / dynamic or manual normals)  -> Tiled (Gather on request)
//   per-frame rows only, or rows + staged maps; default cosine, LDS staging, item runs   -> TiledTw
//   staged maps only; default cosine, LDS staging                                         -> TiledMaps
//   any other extras                                                                      -> Extras
//   radial shells (gorder_hip_set_radial_shells: a cylinder or sphere selection, no other extra) -> Shells
//   united-atom tiles                                                                     -> k_ua_extras<mode> (+ _fast)
//   per-molecule rows (gorder_hip_set_molecule_rows: bond tiles, no other extra, either cosine)  -> TiledMol
//   order distributions (gorder_hip_set_order_histogram: bond tiles, at most a geometry selection, either cosine) -> Dist
//   neighbour classes (gorder_hip_set_neighbour_classes: bond tiles, no other extra, either cosine)              -> Classes
//   united-atom tiles with GORDER_FLAG_UA_SAMPLES and per-molecule rows / an order histogram -> k_ua_mol / k_ua_dist
//     (UaKernel; the bond tiles of the same handle take TiledMol / Dist as above)
// A batch speculates (one read for global leaflets and order parameters) only where Tiled or the unstaged TiledTw runs:
// those are the kernels with a MOM variant, and k_spec_check / k_spec_fixup read what that variant wrote.  TiledMol has
// none, and no gather variant either: GORDER_HIP_KERNEL=gather does not apply to a handle with rows (the rows need the lanes'
// ticks in LDS).  With per-molecule rows global leaflets take the two-kernel path (k_leaflets_global, then the order kernel), no
// one-read speculation.  Dist runs through the extras' sub-range and chunk loop like Shells (its chunks: dist_chunks); it
// has no MOM or gather variant either, so a handle with a histogram never speculates and GORDER_HIP_KERNEL=gather does not apply.
// Classes likewise: k_neighbour_counts, then k_bonds_classes per sub-range of that loop, its chunks shells_chunks.
#ifndef GORDER_ORDER_ROUTE_H
#define GORDER_ORDER_ROUTE_H
#include <stddef.h>
#include <stdint.h>
#include <algorithm>

namespace gorder {
constexpr uint32_t kStageFrames = 4;   // frames of a stage of the tiled kernels (kRecFrames of kernels_bonds.h)

struct OrderRouteIn {
    // trig and geometry (pbc and axis only pick a template argument: no decision below reads them)
    bool acos = false, pbc = false, leaflets = false; int axis = -1;
    // extras
    bool maps = false, map_staged = false, tw = false, geom = false, dyn_or_manual = false;
    // kernel choice
    bool use_gather = false, item_run = false, bond_tiles = false, ua_tiles = false, direct_items = false, ua_fast_flag = false;
    int frames_per_stage = (int)kStageFrames; uint32_t max_window = 0;   // (atoms of the widest tile window)
    // speculation: GLOBAL leaflets, the handle allows it, row 0 holds an earlier assignment, every frame of the batch assigns, supplied normals
    bool global_leaflets = false, spec_enabled = false, have_assignment = false, every_frame_assigns = false, manual_frames = false, normal_table = false;
    // switches (GORDER_HIP_NPF5, GORDER_HIP_TW_GATHER, GORDER_HIP_MAPS_GATHER)
    bool npf5 = false, tw_gather = false, maps_gather = false;
    // radial shells are set on the handle (they come with a geometry selection and exclude every other extra)
    bool shells = false;
    // per-molecule rows are set on the handle (they exclude every extra, direct items, and united atoms unless ua_samples_flag)
    bool mol_rows = false;
    // an order histogram is set on the handle (it excludes every extra but a geometry selection, direct items, and united atoms
    // unless ua_samples_flag)
    bool dist = false;
    // neighbour classes are set on the handle (they exclude every extra, united atoms and direct items)
    bool classes = false;
    // GORDER_FLAG_UA_SAMPLES: the two setters above accepted united-atom tiles (without it they refuse them, and mol_rows /
    // dist never meet ua_tiles)
    bool ua_samples_flag = false;
};
enum class UaKernel { None, Extras, Dist, Mol };    // what runs over the united-atom tiles
enum class BondFamily { None, Tiled, Gather, TiledTw, TiledMaps, Extras, Shells, TiledMol, Dist, Classes };

struct OrderRoute {
    BondFamily family = BondFamily::None;   // what runs over the bond tiles
    const char *label = nullptr;            // ... and its timing group
    int npf = 4;                            // prefetch registers (float4) per thread of the tiled kernels
    bool mom = false, tw_maps = false;      // MOM: the speculative variant (moments and head coordinates as a second output); MAPS of k_bonds_tiled_tw
    bool maps_only = false;                 // staged ordermap samples and nothing else (MO of k_bonds_extras, mode 1 of k_ua_extras)
    bool items_by_slot = false;             // the bond pass reads the items in slot order
    bool extras = false;                    // some scatter-bound extra is on
    int ua_mode = -1; bool ua_fast = false; // MODE of k_ua_extras, -1: no united-atom pass; k_ua_extras_fast
    bool map_accumulate = false, direct = false;   // k_map_accumulate behind every extras pass; k_bonds_direct
    bool speculative = false, fixup_ac = false, fixup_tw = false;   // k_spec_check + k_spec_fixup<AC, TW> follow
    // k_ua_extras<ua_mode> (+ _fast) as ever, or with GORDER_FLAG_UA_SAMPLES k_ua_dist (from the extras' loop, beside Dist) /
    // k_ua_mol (from the molecule rows' sub-range loop, beside TiledMol); ua_mode and ua_fast are then not read
    UaKernel ua_kernel = UaKernel::None;
};

inline OrderRoute choose_order_route(const OrderRouteIn &in) {
    OrderRoute r;
    const bool staged = in.maps && in.map_staged;
    const bool rows_or_maps_only = !in.geom && !in.dyn_or_manual;
    const bool tiled_out = !in.acos && !in.use_gather && in.frames_per_stage == (int)kStageFrames;   // the tiled staging with a second output
    r.extras = in.maps || in.tw || in.geom || in.dyn_or_manual || in.dist || in.classes;     // (Dist and Classes launch from the extras' loop)
    r.maps_only = staged && !in.tw && rows_or_maps_only;
    r.npf = (3u * in.max_window + 6u) / 4u <= 4u * 64u && !in.npf5 ? 4 : 5;      // enough float4 for the widest window (64 threads stage a frame)
    if (!in.bond_tiles) r.family = BondFamily::None;
    else if (in.mol_rows) r.family = BondFamily::TiledMol;
    else if (in.dist) r.family = BondFamily::Dist;
    else if (in.classes) r.family = BondFamily::Classes;
    else if (!r.extras) r.family = in.use_gather ? BondFamily::Gather : BondFamily::Tiled;
    else if (in.shells) r.family = BondFamily::Shells;
    else if (r.maps_only && tiled_out && !in.maps_gather) r.family = BondFamily::TiledMaps;
    else if (in.tw && (!in.maps || staged) && rows_or_maps_only && tiled_out && in.item_run && !in.tw_gather) r.family = BondFamily::TiledTw;
    else r.family = BondFamily::Extras;
    static const char *const labels[] = {nullptr, "k_bonds_tiled", "k_bonds_gather", "k_bonds_tiled_tw", "k_bonds_tiled_maps", "k_bonds_extras", "k_bonds_shells",
                                         "k_bonds_tiled_mol", "k_bonds_dist", "k_bonds_classes"};
    r.label = labels[(int)r.family];
    r.tw_maps = r.family == BondFamily::TiledTw && staged;
    r.items_by_slot = r.family == BondFamily::TiledTw || r.family == BondFamily::TiledMaps || (r.family == BondFamily::Extras && staged);
    r.ua_mode = !in.ua_tiles ? -1 : r.maps_only ? 1 : in.tw && !in.maps && rows_or_maps_only ? 3 : r.extras ? 2 : 0;
    r.ua_fast = in.ua_tiles && in.ua_fast_flag && !in.acos;     // (the two flags exclude each other at gorder_hip_create)
    r.ua_kernel = !in.ua_tiles ? UaKernel::None : in.ua_samples_flag && in.mol_rows ? UaKernel::Mol : in.ua_samples_flag && in.dist ? UaKernel::Dist : UaKernel::Extras;
    r.map_accumulate = staged; r.direct = in.direct_items;
    r.speculative = (r.family == BondFamily::Tiled || (r.family == BondFamily::TiledTw && !r.tw_maps)) && in.leaflets && in.global_leaflets &&
                    in.spec_enabled && in.have_assignment && in.every_frame_assigns && !in.manual_frames && !in.normal_table;
    r.mom = r.speculative;
    r.fixup_tw = in.tw; r.fixup_ac = in.acos && !in.tw;
    return r;
}

// ---- frames per workgroup ------------------------------------------------------------------------------------------------
struct FrameChunks { uint32_t frames_per_chunk, n_chunks; };
inline uint32_t ceil_div(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// k_bonds_tiled / k_bonds_gather: equal work per workgroup, so many short co-resident rounds (12: measured best of 8-12; the last,
// partial one then costs little), at least four stages per workgroup, whole stages.  wg_target: GORDER_HIP_WG_TARGET, 0 = not set.
inline FrameChunks tiled_chunks(uint32_t n_frames, uint32_t stage, uint32_t n_tiles, uint32_t wg_target, uint32_t wg_capacity) {
    const uint32_t n_stages = ceil_div(n_frames, stage);
    uint32_t n_chunks = std::max(1u, (wg_target ? wg_target : 12u * wg_capacity) / n_tiles);
    n_chunks = std::min(n_chunks, std::max(1u, n_stages / 4u));
    const uint32_t fpc = ceil_div(n_stages, n_chunks) * stage;
    return {fpc, ceil_div(n_frames, fpc)};
}

// the extras passes over the frames of one ordermap sub-range: 8 x capacity; staged samples go in whole blocks of 16
// frames (whole lines per workgroup), k_bonds_tiled_tw takes whole stages
inline FrameChunks extras_chunks(uint32_t n_frames, uint32_t n_tiles, uint32_t wg_target, uint32_t wg_capacity, bool staged, bool whole_stages) {
    const uint32_t n_chunks = std::min(std::max(1u, (wg_target ? wg_target : 8u * wg_capacity) / n_tiles), n_frames);
    uint32_t fpc = ceil_div(n_frames, n_chunks);
    if (staged) fpc = ceil_div(fpc, 16u) * 16u;
    if (whole_stages) fpc = ceil_div(fpc, kStageFrames) * kStageFrames;
    return {fpc, ceil_div(n_frames, fpc)};
}

// k_bonds_shells, k_bonds_classes: the extras' chunks, none longer than max_chunk frames (the packed words of a workgroup's shell table)
inline FrameChunks shells_chunks(uint32_t n_frames, uint32_t n_tiles, uint32_t wg_target, uint32_t wg_capacity, uint32_t max_chunk) {
    const FrameChunks c = extras_chunks(n_frames, n_tiles, wg_target, wg_capacity, false, false);
    if (c.frames_per_chunk <= max_chunk) return c;
    return {max_chunk, ceil_div(n_frames, max_chunk)};
}

// k_bonds_dist: the extras' chunks, but none so short that the epilogue — up to table_words words of the workgroup's LDS
// table read, the non-zero ones sent out as global atomics — outweighs the chunk's 256 samples a frame: at least
// samples_per_word samples per table word (kDistSamplesPerWord unless GORDER_HIP_DIST_SAMPLES_PER_WORD says otherwise; 0, or
// table_words = 0 — the direct route, no table —: the extras' chunks as they are), and none longer than max_chunk
constexpr uint32_t kDistSamplesPerWord = 8;
inline FrameChunks dist_chunks(uint32_t n_frames, uint32_t n_tiles, uint32_t wg_target, uint32_t wg_capacity, uint32_t table_words,
                               uint32_t samples_per_word, uint32_t max_chunk) {
    const FrameChunks c = extras_chunks(n_frames, n_tiles, wg_target, wg_capacity, false, false);
    const uint64_t floor_fpc = ((uint64_t)table_words * samples_per_word + 255u) / 256u;
    const uint32_t fpc = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(std::max<uint64_t>(c.frames_per_chunk, floor_fpc), max_chunk), n_frames);
    return {fpc, ceil_div(n_frames, fpc)};
}

// k_bonds_direct: blocks_per_chunk workgroups cover the items of one chunk of frames
inline FrameChunks direct_chunks(uint32_t n_frames, uint32_t blocks_per_chunk, uint32_t wg_target) {
    const uint32_t n_chunks = std::min(std::max(1u, ceil_div(wg_target ? wg_target : 256u * 8u, blocks_per_chunk)), n_frames);
    const uint32_t fpc = ceil_div(n_frames, n_chunks);
    return {fpc, ceil_div(n_frames, fpc)};
}

// k_map_accumulate: enough blocks for ~2 per CU; a block flushes up to a whole map of atomics, so its chunk stays long
// (whole blocks of 16 frames).  forced: GORDER_HIP_MAP_CHUNKS, 0 = not set.
inline FrameChunks map_chunks(uint32_t n_frames, uint32_t n_acc, uint32_t forced) {
    uint32_t n_chunks = forced ? forced : std::max(1u, 512u / std::max(1u, n_acc));
    n_chunks = std::min(n_chunks, std::max(1u, n_frames / 16u));
    const uint32_t fpc = ceil_div(ceil_div(n_frames, n_chunks), 16u) * 16u;
    return {fpc, ceil_div(n_frames, fpc)};
}

// (k_bonds_tiled_mol: the chunks of extras_chunks(..., staged = false, whole_stages = true) per staging sub-range,
// molecule_rows.h: molecule_rows_subrange)

// frames of one ordermap sub-range: short enough for the packed map words (k_fold_maps: fold_limit samples per word, at
// most max_mol a frame) and, staged, for 1 GiB of staging (words_per_frame 64-bit words a frame); everything without maps
inline uint32_t map_subrange(uint32_t n_frames, bool maps, bool staged, uint64_t fold_limit, uint32_t max_mol, size_t words_per_frame) {
    uint32_t sub = maps ? (uint32_t)std::max<uint64_t>(1, (fold_limit - 1) / max_mol) : n_frames;
    if (staged) sub = std::min(std::min<uint32_t>(sub, (uint32_t)std::max<size_t>(1, ((size_t)1 << 27) / words_per_frame)), n_frames);
    return sub;
}

}  // namespace gorder
#endif
