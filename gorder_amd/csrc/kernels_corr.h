// kernels_corr.h — bond reorientation: the second-rank autocorrelation of every bond vector over a list of lags, for the
// whole run (k_bond_units, k_bond_corr; gorder_hip_set_bond_correlation).
// Part of the single translation unit gorder_hip.hip (included there behind kernels_hist.h); device code for gfx950 only.
//
// An additional pass of a batch, not a bond family: it reads the coordinates, the box and the leaflet flag rows the batch's
// own kernels have finished, and nothing of the order pass.  The handle keeps a ring of frame planes float4 [R][n_tiles *
// kBlock] = (vx, vy, vz, n2sq) of every bond vector (bond_corr.h has the ring's arithmetic); k_bond_units writes the planes
// of a sub-range of the batch, k_bond_corr then pairs every frame of the sub-range with its earlier frames.
#pragma once

namespace {

static_assert(gorder::kCorrMaxLags == GORDER_CORR_MAX_LAGS && gorder::kCorrMaxLag == GORDER_CORR_MAX_LAG, "bond_corr.h and gorder_hip.h agree on the limits");
// a lane's i32 sum of one lag takes at most one tick, |tick| <= 10^6, per frame of its chunk
static_assert((long long)gorder::kCorrChunkMax * 1000000ll < (1ll << 31), "an i32 sum must not overflow in one chunk");
static_assert(gorder::kCorrMaxLags % gorder::kCorrLagBlock == 0, "the padded lag list is whole groups");

struct CorrArgs {
    float4 *ring;                   // [ring_planes][plane_items]
    uint32_t ring_planes;           // R = max_lag + sub-range
    uint32_t plane_items;           // n_tiles * kBlock
    uint32_t base;                  // the plane of the batch's frame 0: (analysed frames before the batch) mod R
    uint32_t history;               // analysed frames before the batch since create / reset, capped at GORDER_CORR_MAX_LAG
    uint32_t frame0, n_frames;      // the sub-range [frame0, n_frames) of the batch
    uint32_t frames_per_chunk;
    uint32_t n_chunks;              // k_bond_corr, tile-major grid: chunks of the sub-range (0: the chunk-major grid)
    uint32_t n_lags;
    const uint32_t *lags;           // [n_lags rounded up to whole groups], the tail kCorrNoLag
    unsigned long long *rep;        // [n_rep][n_lags][4][n_acc]: sum, sum_upper, count, count_upper
    uint32_t n_rep, n_acc;
    int leaflets;
    const uint8_t *aflags;          // the batch's final flag rows
    const uint32_t *arow;
    uint32_t n_mol_total;
    // k_bond_units
    const float *xyz, *box9;
    uint32_t n_atoms;
    int pbc;
};

// The bond vector of every item of every frame of the sub-range, once: two loads, the minimum image, n2sq, one 16-byte
// store.  grid = n_tiles * frames.  Raises nothing: the order kernel of the same batch reports undefined positions and a
// box the minimum image gives up on.  A lane past the tile's items stores zeros, so that every word of a plane is defined.
__global__ __launch_bounds__(kBlock) void k_bond_units(CorrArgs c, const Tile *__restrict__ tiles, const Item *__restrict__ items, uint32_t n_tiles) {
    const uint32_t tile_id = blockIdx.x % n_tiles, f = c.frame0 + blockIdx.x / n_tiles, tid = threadIdx.x;
    const Tile t = tiles[tile_id];
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (tid < t.n_items) {
        const Item it = items[t.item0 + tid];
        const float *frame = c.xyz + (size_t)f * c.n_atoms * 3u;
        const float *p1 = frame + ((size_t)t.atom0 + it.li) * 3u, *p2 = frame + ((size_t)t.atom0 + it.lj) * 3u;
        float vx = p2[0] - p1[0], vy = p2[1] - p1[1], vz = p2[2] - p1[2];
        if (c.pbc) {
            const float *b = c.box9 + 9 * (size_t)f;
            int bad = 0;
            vx = gm_min_image(vx, b[0], bad);
            vy = gm_min_image(vy, b[4], bad);
            vz = gm_min_image(vz, b[8], bad);
        }
        out = make_float4(vx, vy, vz, (vx * vx + vy * vy) + vz * vz);
    }
    const uint32_t plane = (c.base + f) % c.ring_planes;
    c.ring[(size_t)plane * c.plane_items + (size_t)tile_id * kBlock + tid] = out;
}

// Every pair (frame s of the sub-range, frame s - lag) of every item: tick = gm_tick(gm_calc_sch<false>(v_s, v_{s - lag},
// sqrtf(n2sq), n2sq)), the later frame the sample, the earlier one the normal — the arithmetic of a per-molecule manual
// normal (k_bonds_extras), always in the default squared-cosine form.  A thread owns one item over the frames of its
// workgroup's chunk (the two grids: below).  The lags go in groups of LB with a compile-time trip count (the accumulators of a group
// are LB registers each, indexed by constants only); per group and frame the lane loads its own entry of frame s once,
// then the LB earlier entries (16-byte loads, coalesced over the tile: 4 KB a frame, mostly L2 hits), then ticks and adds.
// A pair is booked on the leaflet of its molecule in frame s.  A lag with less history than it needs (the run's first
// frames, and the kCorrNoLag that pads the last group) reads the lane's own plane instead and adds nothing: no branch per
// lag.  Behind each group the lanes of a local slot are folded in LDS the way fold_tile_sums folds the ordinary sums, and
// one 64-bit atomic per (lag, slot, field) goes to the replicas.
// Two grids.  Tile-major (n_chunks != 0, the default): grid = n_tiles * n_chunks * groups, a workgroup takes ONE group of
// lags of its chunk, and the workgroups of a tile are neighbours in the grid — the workgroups resident at one time then
// share the planes of a few tiles, which the caches behind L2 can hold, where the chunk-major grid spreads them over every
// tile's ring.  Chunk-major (n_chunks == 0, GORDER_HIP_CORR_GRID=chunks): grid = n_tiles * n_chunks, a workgroup walks
// every group of its chunk in turn.  The integers are the same (DESIGN 6l has both timings).
template <uint32_t LB>
__global__ __launch_bounds__(kBlock) void k_bond_corr(CorrArgs c, const Tile *__restrict__ tiles, const Item *__restrict__ items,
                                                      const uint32_t *__restrict__ tile_slots, uint32_t n_tiles) {
    __shared__ unsigned long long l_s[2 * kBlock];
    __shared__ uint32_t l_n[2 * kBlock];
    const uint32_t tid = threadIdx.x;
    uint32_t tile_id = blockIdx.x % n_tiles, chunk = blockIdx.x / n_tiles, g_begin = 0, g_end = c.n_lags;
    if (c.n_chunks) {
        const uint32_t n_groups = (c.n_lags + LB - 1u) / LB, per_tile = c.n_chunks * n_groups, r = blockIdx.x % per_tile;
        tile_id = blockIdx.x / per_tile;
        chunk = r / n_groups;
        g_begin = (r % n_groups) * LB;
        g_end = g_begin + 1u;       // (one group)
    }
    const Tile t = tiles[tile_id];
    const bool active = tid < t.n_items;
    Item it{0, 0, 0, 0, 0};
    if (active) it = items[t.item0 + tid];
    const uint32_t f_begin = c.frame0 + chunk * c.frames_per_chunk;
    const uint32_t f_end = min(c.n_frames, f_begin + c.frames_per_chunk);
    const uint32_t R = c.ring_planes;
    const float4 *const mine = c.ring + (size_t)tile_id * kBlock + tid;
    const uint8_t *const flag = c.aflags + it.mol;
    unsigned long long *const rep = c.rep + (size_t)(blockIdx.x % c.n_rep) * c.n_lags * 4u * c.n_acc;
    for (uint32_t g = g_begin; g < g_end; g += LB) {
        uint32_t lag[LB];
        int32_t sum[LB], sum_up[LB];
        uint32_t n[LB], n_up[LB];
#pragma unroll
        for (uint32_t u = 0; u < LB; u++) { lag[u] = c.lags[g + u]; sum[u] = 0; sum_up[u] = 0; n[u] = 0; n_up[u] = 0; }
        uint32_t ps = (c.base + f_begin) % R;       // the plane of frame f
        for (uint32_t f = f_begin; f < f_end; f++) {
            // the frames before f since create / reset, as far as a lag can ask
            const uint32_t before = min(c.history + min(f, GORDER_CORR_MAX_LAG), GORDER_CORR_MAX_LAG);
            const float4 v = mine[(size_t)ps * c.plane_items];
            const bool up = c.leaflets && flag[(size_t)c.arow[f] * c.n_mol_total] == 0;
#pragma unroll
            for (uint32_t u = 0; u < LB; u++) {
                const bool valid = lag[u] <= before;
                const uint32_t back = valid ? lag[u] : 0u;
                const uint32_t pe = ps >= back ? ps - back : ps + R - back;
                const float4 e = mine[(size_t)pe * c.plane_items];
                const int tick = valid ? gm_tick(gm_calc_sch<false>(v.x, v.y, v.z, e.x, e.y, e.z, __builtin_sqrtf(e.w), e.w)) : 0;
                sum[u] += tick;
                n[u] += valid ? 1u : 0u;
                sum_up[u] += up ? tick : 0;
                n_up[u] += valid && up ? 1u : 0u;
            }
            ps = ps + 1u == R ? 0u : ps + 1u;
        }
#pragma unroll
        for (uint32_t u = 0; u < LB; u++) {
            if (g + u >= c.n_lags) break;           // (uniform: every thread of the workgroup takes the same barriers)
            // a thread zeroes and later reads only the words of its own index: the second barrier of the lag before is
            // enough between that lag's reads and these stores
            l_s[tid] = 0; l_s[kBlock + tid] = 0; l_n[tid] = 0; l_n[kBlock + tid] = 0;
            __syncthreads();
            if (active && n[u]) {
                atomicAdd(&l_s[it.lslot], (unsigned long long)(long long)sum[u]);
                atomicAdd(&l_n[it.lslot], n[u]);
                if (n_up[u]) {
                    atomicAdd(&l_s[kBlock + it.lslot], (unsigned long long)(long long)sum_up[u]);
                    atomicAdd(&l_n[kBlock + it.lslot], n_up[u]);
                }
            }
            __syncthreads();
            if (tid < t.n_slots && l_n[tid]) {
                unsigned long long *out = rep + (size_t)(g + u) * 4u * c.n_acc;
                const uint32_t slot = tile_slots[t.slot0 + tid];
                atomicAdd(&out[slot], l_s[tid]);
                atomicAdd(&out[2u * c.n_acc + slot], (unsigned long long)l_n[tid]);
                if (l_n[kBlock + tid]) {
                    atomicAdd(&out[c.n_acc + slot], l_s[kBlock + tid]);
                    atomicAdd(&out[3u * c.n_acc + slot], (unsigned long long)l_n[kBlock + tid]);
                }
            }
        }
    }
}

}  // namespace
