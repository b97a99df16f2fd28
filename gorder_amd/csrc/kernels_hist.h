// kernels_hist.h — order distributions: sample counts per bin of the tick, accumulator slot and leaflet plane, for the
// whole run (k_bonds_dist; gorder_hip_set_order_histogram).
// Part of the single translation unit gorder_hip.hip (included there behind kernels_radial.h); device code for gfx950 only.
#pragma once

namespace {

// A table word is a u32 count.  At most 256 items of a tile share a slot, so a word receives at most 256 samples a frame
// and cannot overflow while the workgroup's chunk is at most 2^23 frames (2^31 samples).  The host cuts the chunks
// accordingly (dist_chunks).
static_assert(gorder::kHistMaxBins == GORDER_HIST_MAX_BINS, "order_hist.h and gorder_hip.h agree on the bins");
constexpr uint32_t kDistChunkMax = 1u << 23;
static_assert((unsigned long long)kDistChunkMax * 256u <= 0xffffffffull, "a u32 table word must not overflow in one chunk");
// dynamic LDS: the edges (int32, room for GORDER_HIST_MAX_BINS + 1, 16-byte multiple), then the table — or, once the table
// has been sent out, and on the direct route from the start, the [2][256] u64 + [2][256] u32 of the ordinary sums' reduction
constexpr uint32_t kDistEdgeBytes = (GORDER_HIST_MAX_BINS + 1u + 3u) / 4u * 16u;
constexpr uint32_t kDistReduceBytes = kBlock * 24u;

struct DistArgs {
    uint32_t n_edges;                       // 2..GORDER_HIST_MAX_BINS + 1
    const int32_t *edges;                   // [n_edges] ascending ticks
    unsigned long long *rep;                // [n_rep][n_edges - 1][2][n_acc]: count_total, count_upper per bin
    uint32_t n_rep;
};

// k_bonds_extras for a static normal and at most a geometry selection (no maps, rows, per-molecule normals), with every
// sample's tick booked in its bin as well.  grid = n_tiles * n_chunks, a thread owns one bond sample over its chunk.
//   LDS route: the table u32 [planes][n bins][t.n_slots] counts the workgroup's samples of its whole frame range; planes =
//     upper, lower with leaflets (a sample touches its own plane only, total = upper + lower), else one.  Per sample:
//     hist_bin over the edges in LDS, then one 32-bit LDS add without a return value.  The bin of a sample changes almost
//     every frame, so no word is kept open in registers.  The slot is the minor index: the 64 bonds of an all-atom lipid
//     are 64 consecutive lanes, so the 32 lanes of a half wave sit on 32 distinct banks whatever their bins.
//     The epilogue strides the table and adds the non-zero words to the global replicas.
//   DIRECT: the table does not fit (or GORDER_HIP_DIST_DIRECT): one or two global atomics per sample on the replicas.
// The ordinary sums stay in registers on both routes and are reduced by fold_tile_sums (kernels_tile.h): gorder_hip_finish
// sees what k_bonds_extras would have left.
template <bool ACOS_COS, bool DIRECT>
__global__ __launch_bounds__(kBlock) void k_bonds_dist(FrameArgs a_in, ExtraArgs e, DistArgs s, const float *__restrict__ xyz,
                                                        const float *__restrict__ box9,
                                                        const uint8_t *__restrict__ aflags,
                                                        const uint32_t *__restrict__ arow,
                                                        const Tile *__restrict__ tiles,
                                                        const Item *__restrict__ items,
                                                        const uint32_t *__restrict__ tile_slots, uint32_t n_tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char l_dist[];
    int32_t *const l_edges = reinterpret_cast<int32_t *>(l_dist);
    uint32_t *const l_tab = reinterpret_cast<uint32_t *>(l_dist + kDistEdgeBytes);
    FrameArgs a = a_in;
    a.xyz = xyz; a.box9 = box9; a.aflags = aflags; a.arow = arow;
    const uint32_t tile_id = blockIdx.x % n_tiles, chunk = blockIdx.x / n_tiles;
    const Tile t = tiles[tile_id];
    const uint32_t tid = threadIdx.x;
    const bool active = tid < t.n_items;
    Item it{0, 0, 0, 0, 0};
    if (active) it = items[t.item0 + tid];
    const uint32_t gslot = active ? tile_slots[t.slot0 + it.lslot] : 0;
    const uint32_t f_begin = a.frame0 + chunk * a.frames_per_chunk;
    const uint32_t f_end = min(a.n_frames, f_begin + a.frames_per_chunk);
    const TileCtx tc{t, it, tile_id, chunk, tid, active, f_begin, f_end};      // (for fold_tile_sums; kernels_tile.h says why not tile_prologue)
    const size_t fstride = (size_t)a.n_atoms * 3u;
    const float *pi = xyz + ((size_t)t.atom0 + it.li) * 3u;
    const float *pj = xyz + ((size_t)t.atom0 + it.lj) * 3u;
    const uint32_t planes = a.leaflets ? 2u : 1u, ns = t.n_slots, n_bins = s.n_edges - 1u;
    for (uint32_t k = tid; k < s.n_edges; k += kBlock) l_edges[k] = s.edges[k];
    if (!DIRECT)
        for (uint32_t k = tid; k < planes * n_bins * ns; k += kBlock) l_tab[k] = 0;
    __syncthreads();
    unsigned long long *const dist_rep = s.rep + (size_t)(blockIdx.x % s.n_rep) * n_bins * 2u * a.n_acc;
    SampleAcc acc;
    int bad = 0;
    // the two atoms of the next frames are fetched ahead of the arithmetic of this one (the gather is latency-bound)
    constexpr uint32_t kAhead = 2;
    float nx1[kAhead][3], nx2[kAhead][3];
#pragma unroll
    for (uint32_t u = 0; u < kAhead; u++) {
        const uint32_t fu = min(f_begin + u, a.n_frames - 1u);
#pragma unroll
        for (int d = 0; d < 3; d++) { nx1[u][d] = pi[(size_t)fu * fstride + d]; nx2[u][d] = pj[(size_t)fu * fstride + d]; }
    }
    for (uint32_t f = f_begin; f < f_end; f++) {
        const float p1x = nx1[0][0], p1y = nx1[0][1], p1z = nx1[0][2];
        const float p2x = nx2[0][0], p2y = nx2[0][1], p2z = nx2[0][2];
#pragma unroll
        for (uint32_t u = 0; u + 1 < kAhead; u++)
#pragma unroll
            for (int d = 0; d < 3; d++) { nx1[u][d] = nx1[u + 1][d]; nx2[u][d] = nx2[u + 1][d]; }
        {
            const uint32_t fu = min(f + kAhead, a.n_frames - 1u);
#pragma unroll
            for (int d = 0; d < 3; d++) {
                nx1[kAhead - 1][d] = pi[(size_t)fu * fstride + d];
                nx2[kAhead - 1][d] = pj[(size_t)fu * fstride + d];
            }
        }
        if (!active) continue;
        float vx = p2x - p1x, vy = p2y - p1y, vz = p2z - p1z;
        if (a.pbc) {
            const float *b = a.box9 + 9 * (size_t)f;
            vx = gm_min_image(vx, b[0], bad);
            vy = gm_min_image(vy, b[4], bad);
            vz = gm_min_image(vz, b[8], bad);
        }
        if (p1x != p1x) raise_error(a.err, GORDER_ERR_UNDEFINED_POSITION, f, kStageTypes, gslot, 1, it.mol, 0);
        else if (p2x != p2x) raise_error(a.err, GORDER_ERR_UNDEFINED_POSITION, f, kStageTypes, gslot, 1, it.mol, 1);
        // bond position = p1 + v / 2 (bond.rs:422); geometry filter (bond.rs:424-426)
        if (e.geom_kind) {
            const float mx = p1x + vx / 2.0f, my = p1y + vy / 2.0f, mz = p1z + vz / 2.0f;
            float box[3] = {1.0f, 1.0f, 1.0f};
            if (a.pbc) { const float *b = a.box9 + 9 * (size_t)f; box[0] = b[0]; box[1] = b[4]; box[2] = b[8]; }
            if (!geom_inside(e, e.shapes + 8 * (size_t)f, mx, my, mz, box, a.pbc != 0, bad)) continue;
        }
        float sch;
        if (!ACOS_COS && e.axis >= 0) {     // the static normal is a coordinate axis: K1's short form, same bits
            bool rare = false;
            sch = e.axis == 0 ? gm_sch_axis<0>(vx, vy, vz, rare) : (e.axis == 1 ? gm_sch_axis<1>(vx, vy, vz, rare) : gm_sch_axis<2>(vx, vy, vz, rare));
            if (__builtin_expect(rare, 0)) sch = gm_calc_sch<ACOS_COS>(vx, vy, vz, a.nx, a.ny, a.nz, a.n2, a.n2sq);
        } else {
            sch = gm_calc_sch<ACOS_COS>(vx, vy, vz, a.nx, a.ny, a.nz, a.n2, a.n2sq);
        }
        const int tick = gm_tick(sch);
        int leaflet = -1;
        if (a.leaflets) leaflet = a.aflags[(size_t)a.arow[f] * a.n_mol_total + it.mol] ? 1 : 0;
        acc.s_tot += tick;
        acc.n_tot += 1;
        if (leaflet == 0) { acc.s_up += tick; acc.n_up += 1; }
        const int bin = gorder::hist_bin(l_edges, s.n_edges, tick);
        if (bin < 0) continue;
        if (DIRECT) {
            unsigned long long *p = dist_rep + (size_t)bin * 2u * a.n_acc + gslot;
            atomicAdd(p, 1ull);
            if (leaflet == 0) atomicAdd(p + a.n_acc, 1ull);
        } else {
            atomicAdd(&l_tab[((leaflet > 0 ? n_bins : 0u) + (uint32_t)bin) * ns + it.lslot], 1u);
        }
    }
    if (bad) raise_box_range(a.err, f_begin);
    __syncthreads();
    if (!DIRECT) {
        const uint32_t words = n_bins * ns;
        for (uint32_t k = tid; k < words; k += kBlock) {
            const uint32_t w0 = l_tab[k], w1 = a.leaflets ? l_tab[words + k] : 0u;
            if (!(w0 | w1)) continue;
            const uint32_t b = k / ns, slot = tile_slots[t.slot0 + (k - b * ns)];
            unsigned long long *p = dist_rep + (size_t)b * 2u * a.n_acc + slot;
            atomicAdd(p, (unsigned long long)w0 + w1);
            if (a.leaflets && w0) atomicAdd(p + a.n_acc, (unsigned long long)w0);
        }
        __syncthreads();        // the table's words are read: its place now serves the reduction below
    }
    // the place of the table (behind the edges, which stay): the barrier just above ended the table's reads; on the direct
    // route nothing has been there
    fold_tile_sums(a.rep, a.n_rep, a.n_acc, tc, acc, l_tab, [&] { return tile_slots[tc.t.slot0 + tc.tid]; });
}

}  // namespace
