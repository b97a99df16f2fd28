// kernels_tile.h — what the bond-tile kernels have in common, once: the prologue of a workgroup, the epilogue of the
// ordinary sums, and the undefined position of the tiled kernels.
// Part of the single translation unit gorder_hip.hip (included there between kernels_common.h and kernels_bonds.h);
// device code for gfx950 only.  Callers: k_bonds_tiled, k_bonds_gather (kernels_bonds.h), k_bonds_tiled_maps
// (kernels_extras.h) and k_bonds_tiled_mol (kernels_molrows.h) use all of it; k_bonds_tiled_tw (kernels_extras.h) all but
// tile_prologue; k_bonds_extras (kernels_extras.h), k_bonds_shells (kernels_radial.h), k_bonds_classes (kernels_neighbours.h)
// and k_bonds_dist (kernels_hist.h) fold_tile_sums only.
//
// Every function is inlined into its kernel, none has a template parameter or a flag that says which kernel called it:
// where two kernels differ, the difference is at the call.  The contracts:
//
//   tile_prologue                   no barrier, no LDS.  Every thread of the workgroup calls it; grid.x = n_tiles * n_chunks.
//       A lane at or past the tile's n_items is not `active` and holds the all-zero Item (atoms atom0, local slot 0,
//       molecule 0: loads through it stay inside the tile's window, nothing may be booked for it).  frame_base is
//       FrameArgs::frame0 for the kernels that launch sub-ranges and a literal 0 for k_bonds_tiled and k_bonds_gather,
//       which always start at frame 0 and so pay no instruction for it.
//   fold_tile_sums                  TWO barriers, both its own: one behind the zeroing of the LDS it was handed, one
//       behind the LDS atomics.  ALL kBlock threads of the workgroup must reach it, in uniform control flow (a kernel
//       that returns early for some threads must do so behind it).  The caller hands it [2][kBlock] u64 + [2][kBlock] u32
//       of LDS (kTileFoldBytes in one piece, 8-byte aligned, or the two arrays) that no thread reads or writes for
//       another purpose from the caller's last barrier on: static __shared__ arrays of its own, or LDS that held
//       something else — then the CALLER's barrier ends the last reads of that something, and the comment at the call
//       says which barrier that is.  The helper does not open with a barrier.  slot_of() yields the accumulator slot of
//       local slot `tid` and is called only where tid < n_slots and the slot has samples.  Integer sums: the result does
//       not depend on the order (order.rs:44-60).
//   note_undefined, raise_tile_errors    no barrier.  raise_tile_errors reads tile_slots through the lane's Item, which is
//       in range for inactive lanes too (local slot 0; every tile has a slot).
//   tiled_map_out (kernels_extras.h, next to the ExtraArgs it reads) belongs to the same set.
//
// The shape of the parameters is part of the contract, because the kernels' code must not change with their text
// (profiles/tile_helpers_resources.txt).  A local struct that a helper takes BY REFERENCE stays in memory until the helper
// is inlined, behind the compiler's first clean-up of the kernel, and the code that comes out differs.  So:
//   - no helper takes the kernel's FrameArgs (or its by-value argument a_in): the fields come as scalars.  The two lines
//     that copy a_in and set the __restrict__ streams therefore stay in every kernel.
//   - the SampleAcc comes by value (by reference k_bonds_tiled grew by 12 bytes and two SGPRs).
//   - the TileCtx may come by reference: in the tiled kernels that costs nothing.  In k_bonds_extras, k_bonds_shells and
//     k_bonds_dist it does — they spill up to 102 SGPRs into VGPR lanes, and tile_prologue moved the VGPR count of four of
//     their twelve instantiations by one or two — so these three keep their own prologue and hand fold_tile_sums a
//     TileCtx made of their locals.  k_bonds_tiled_tw does the same for another reason: it fetches the item and the
//     item's run under one test of `active`; behind tile_prologue that became two, and the kernel measured 0.5 % slower.
//
// Left alone on purpose — do not fold these in:
//   the frame loop of k_bonds_extras, k_bonds_shells, k_bonds_dist (the two-frames-ahead gather walk, the signed minimum
//                      image, the undefined-position raise, the choice of gm_sch_axis, the leaflet lookup): shared as
//                      helpers it changed the VGPR count of nine of the twelve instantiations by up to six, in every
//                      parameter shape that was tried (a walk object, plain local arrays handed to free functions, box
//                      edges returned or loaded at the geometry, scalars instead of FrameArgs).
//   the united-atom tiles     three slots per lane, a kUaLS stride and a strided slot loop: a helper that served them and the
//                      bond tiles would branch on its caller.  They share among themselves: kernels_ua.h.
//   k_bonds_direct     has no tile (a thread per sample, global atomics straight away).
//   TiledStage, bond_sample     are the shared per-sample arithmetic already.
//   the host side (launch_orders, the handle), kernel names, timing labels, order_route.h, the ABI.
#pragma once

namespace {

constexpr uint32_t kNoNan = 0xffffffffu;   // "this sample has met no undefined position yet"
struct SampleAcc {
    long long s_tot = 0, s_up = 0;
    uint32_t n_tot = 0, n_up = 0;
};

// ---- prologue ------------------------------------------------------------------------------------
struct TileCtx {
    Tile t;
    Item it;                    // this lane's sample; all zero where !active
    uint32_t tile_id, chunk, tid;
    bool active;
    uint32_t f_begin, f_end;    // the frames of this workgroup's chunk
};
__device__ __forceinline__ TileCtx tile_prologue(const Tile *tiles, const Item *items, uint32_t n_tiles, uint32_t frame_base,
                                                 uint32_t frames_per_chunk, uint32_t n_frames) {
    TileCtx c;
    c.tile_id = blockIdx.x % n_tiles;
    c.chunk = blockIdx.x / n_tiles;
    c.t = tiles[c.tile_id];
    c.tid = threadIdx.x;
    c.active = c.tid < c.t.n_items;
    c.it = Item{0, 0, 0, 0, 0};
    if (c.active) c.it = items[c.t.item0 + c.tid];
    c.f_begin = frame_base + c.chunk * frames_per_chunk;
    c.f_end = min(n_frames, c.f_begin + frames_per_chunk);
    return c;
}

// ---- epilogue of the ordinary sums: fold the block's samples per accumulator slot in LDS, then one global atomic
// per (slot, field)
constexpr uint32_t kTileFoldBytes = kBlock * 24u;
template <class SlotOf>
__device__ __forceinline__ void fold_tile_sums(unsigned long long *rep, uint32_t n_rep, uint32_t n_acc, const TileCtx &c, const SampleAcc acc,
                                               unsigned long long *l_s /* [2][kBlock] */, uint32_t *l_n /* [2][kBlock] */,
                                               SlotOf slot_of) {
    const uint32_t tid = c.tid;
    l_s[tid] = 0; l_s[kBlock + tid] = 0; l_n[tid] = 0; l_n[kBlock + tid] = 0;
    __syncthreads();
    if (c.active && acc.n_tot) {
        atomicAdd(&l_s[c.it.lslot], (unsigned long long)acc.s_tot);
        atomicAdd(&l_n[c.it.lslot], acc.n_tot);
        if (acc.n_up) {
            atomicAdd(&l_s[kBlock + c.it.lslot], (unsigned long long)acc.s_up);
            atomicAdd(&l_n[kBlock + c.it.lslot], acc.n_up);
        }
    }
    __syncthreads();
    if (tid < c.t.n_slots && l_n[tid]) {
        // spread the blocks over n_rep replicas of the accumulator block: same-address atomics of
        // thousands of blocks would otherwise serialise in L2
        unsigned long long *mine = rep + (size_t)(blockIdx.x % n_rep) * 4u * n_acc;
        const uint32_t slot = slot_of();
        atomicAdd(&mine[slot], l_s[tid]);
        atomicAdd(&mine[2u * n_acc + slot], (unsigned long long)l_n[tid]);
        if (l_n[kBlock + tid]) {
            atomicAdd(&mine[n_acc + slot], l_s[kBlock + tid]);
            atomicAdd(&mine[3u * n_acc + slot], (unsigned long long)l_n[kBlock + tid]);
        }
    }
}
// the same with the LDS in one piece of kTileFoldBytes: the sums first, the counts behind them
template <class SlotOf>
__device__ __forceinline__ void fold_tile_sums(unsigned long long *rep, uint32_t n_rep, uint32_t n_acc, const TileCtx &c, const SampleAcc acc,
                                               void *lds, SlotOf slot_of) {
    unsigned long long *l_s = reinterpret_cast<unsigned long long *>(lds);
    fold_tile_sums(rep, n_rep, n_acc, c, acc, l_s, reinterpret_cast<uint32_t *>(l_s + 2 * kBlock), slot_of);
}

// ---- undefined position, tiled kernels: a sample whose S came out NaN writes down which of its atoms is undefined in
// frame f (p1 before p2, bond.rs:410-416); the caller asks only while nan_frame == kNoNan, so the FIRST one stays
__device__ __forceinline__ void note_undefined(float p1x, float p2x, uint32_t f, uint32_t &nan_which, uint32_t &nan_frame) {
    if (p1x != p1x) { nan_which = 0; nan_frame = f; }
    else if (p2x != p2x) { nan_which = 1; nan_frame = f; }
}
// ... and behind the frame loop it is raised, then the box range (the literal minimum-image loops gave up)
__device__ __forceinline__ void raise_tile_errors(uint32_t *err, const TileCtx &c, const uint32_t *tile_slots,
                                                  uint32_t nan_which, uint32_t nan_frame, int bad) {
    if (nan_frame != kNoNan)
        raise_error(err, GORDER_ERR_UNDEFINED_POSITION, nan_frame, kStageTypes, tile_slots[c.t.slot0 + c.it.lslot], 1, c.it.mol, nan_which);
    if (bad) raise_box_range(err, c.f_begin);
}

}  // namespace
