// kernels_extras.h — scatter modes: ordermaps, timewise rows, geometry filter (k_bonds_extras, k_map_accumulate; ExtraArgs, geom_inside, extras_add and extras_flush_tw also serve kernels_ua.h).
// Part of the single translation unit gorder_hip.hip (included there, in this order: common, bonds, extras,
// leaflets, normals); device code for gfx950 only.
#pragma once

namespace {

// =============================================================================================
// "Extras" kernels: ordermaps (ordermap.rs:100-113), timewise partial sums (timewise.rs:130-186,
// 277-283) and the united-atom path (uaorder.rs:375-437, 947-1104).  These modes are bound by their
// scatter atomics, not by the coordinate stream, so they use a plain structure: a thread owns one
// sample (or one united-atom carbon), gathers its atoms straight from global memory and walks the
// frames of its chunk one by one.  The main accumulators are kept in registers exactly like K1.
// =============================================================================================
struct ExtraArgs {
    int maps;                        // ordermaps on
    uint32_t plane;                  // 0 xy, 1 xz, 2 yz -> (z, y)   (input/ordermap.rs:44-50)
    float x0, y0, binx, biny;
    uint32_t nx, ny;
    unsigned long long *map_packed;  // [leaflets ? 2 : 1][n_acc][nx*ny] packed (count << 42) + sum, see k_fold_maps
    // sample staging (k_map_accumulate), or null: 64-bit words (plane-tile << 32 | tick), kMapNoSample where a lane has
    // no sample.  The `n` lanes of a tile that hold the molecules of one slot (a MapRun, from lane tid0) own contiguous
    // pieces.  United atoms (K = 3 hydrogens): the words [((tile * K + k) * kBlock + tid0) * rec_stride ...) laid out
    // [frame - rec_frame0][n].  Bond tiles block the frames by kRecFrames = 4: a tile's words of one block of frames are
    // [frame block][lane][frame in block] — a thread writes its own four samples of a stage, 32 bytes, no transposition —
    // and a run's piece of a frame block the kRecFrames * n words from kRecFrames * tid0 (128 bytes for the four molecules
    // a tile of the 256-lipid membrane holds per slot: whole cache lines for the reader).
    // (Five-byte samples — a 32-bit word and a byte in a second array — were tried: the producer gained 20 us per 3000
    // frames, the reader lost 50: its pieces fell below the 128-byte line)
    unsigned long long *map_rec;
    const uint32_t *item_run;        // per item: (tid0 << 16) | n
    uint32_t rec_frame0, rec_stride; // rec_stride: words per lane = frames of the sub-range rounded up to 16
    const float4 *dyn;               // dynamic membrane normals [n_frames][n_mol_total] (nx, ny, nz, cloud size) or null
    int bin_core;                    // both bin widths in [2^-40, 2^40]: grid_index may use the division core
    float inv_binx, inv_biny;        // 1 / bin (IEEE, from the host): GORDER_FLAG_UA_FAST_NORMALISE's tile index
    int axis;                        // the static normal is this coordinate axis (0..2), or -1
    int tw;                          // timewise on
    unsigned long long *tw_sums;     // [rows][3][n_acc]
    unsigned long long *tw_cnts;     // [rows][3][n_acc]
    unsigned long long tw_row0;      // row of this batch's frame 0
    // united atoms: sin/cos of the construction angles, evaluated on the host with libm like the reference
    float sin_tet, cos_tet, sin_ch3, cos_ch3, sin_half, cos_half;
    // geometry selection (geometry.rs): per-frame shapes [n_frames][8] = anchor xyz, extents xyz, radius, height
    int geom_kind, geom_invert, geom_orient;
    float geom_thr;                  // cylinder / sphere: local_radius_threshold(radius), d2 < geom_thr == sqrt(d2) < radius
    const float *shapes;
    // GORDER_FLAG_UA_FAST_NORMALISE: box edges and 1 / box edge per frame [n_frames][8] (k_inv_box: IEEE divisions, once per frame instead
    // of once per lane and frame), or null
    const float *inv_box;
    // collected normals (gorder_hip_set_collect) of a bond system with a geometry selection: [n_frames][n_mol_total], 1 where a
    // sample fetched the molecule's normal of that frame; null otherwise
    uint8_t *touched;
};

// groan_rs Rectangular / Cylinder / Sphere ::inside (oracle: inside_shape), XOR invert (geometry.rs:181-189).
// No array is indexed by a run-time value (the cylinder's axis picks its operands by selects: arrays indexed by it went
// to scratch memory), and `sqrt(d2) < radius` is `d2 < e.geom_thr` (local_radius_threshold: the smallest float whose
// correctly rounded square root reaches the radius — the same samples, no IEEE square root per sample).
__device__ __forceinline__ bool geom_inside(const ExtraArgs &e, const float *sh, float px, float py, float pz,
                                            const float *box, bool pbc, int &bad) {
    bool in = true;
    if (e.geom_kind == GORDER_GEOM_CUBOID) {
        float x = px - sh[0], y = py - sh[1], z = pz - sh[2];
        if (pbc) {
            x = gm_wrap(x, box[0], bad); y = gm_wrap(y, box[1], bad); z = gm_wrap(z, box[2], bad);
            in = (x <= sh[3]) && (y <= sh[4]) && (z <= sh[5]);
        } else {
            in = (x >= 0.0f) && (x <= sh[3]) && (y >= 0.0f) && (y <= sh[4]) && (z >= 0.0f) && (z <= sh[5]);
        }
    } else if (e.geom_kind == GORDER_GEOM_CYLINDER) {
        // orientation o, in-plane axes a = (o + 1) % 3 and b = (o + 2) % 3
        const int o = e.geom_orient;
        const float dx = px - sh[0], dy = py - sh[1], dz = pz - sh[2];
        float x = o == 0 ? dx : (o == 1 ? dy : dz), da = o == 0 ? dy : (o == 1 ? dz : dx), db = o == 0 ? dz : (o == 1 ? dx : dy);
        if (pbc) {
            const float bo = o == 0 ? box[0] : (o == 1 ? box[1] : box[2]), ba = o == 0 ? box[1] : (o == 1 ? box[2] : box[0]),
                        bb = o == 0 ? box[2] : (o == 1 ? box[0] : box[1]);
            da = gm_min_image(da, ba, bad); db = gm_min_image(db, bb, bad); x = gm_wrap(x, bo, bad);
        }
        in = (da * da + db * db < e.geom_thr) && (pbc ? true : (x >= 0.0f)) && (x <= sh[7]);
    } else {
        float dx = px - sh[0], dy = py - sh[1], dz = pz - sh[2];
        if (pbc) { dx = gm_min_image(dx, box[0], bad); dy = gm_min_image(dy, box[1], bad); dz = gm_min_image(dz, box[2], bad); }
        in = (dx * dx + dy * dy) + dz * dz < e.geom_thr;
    }
    return in != (e.geom_invert != 0);
}

// BondLike::add_order for the scatter targets (bond.rs:184-215): maps and the per-frame LDS partials
template <bool STAGED_ONLY = false, bool NO_MAPS = false>
__device__ __forceinline__ void extras_add(const FrameArgs &a, const ExtraArgs &e, uint32_t gslot, uint32_t lslot,
                                           int tick, float px, float py, float pz, int leaflet /* -1 none */,
                                           int *l_tw, uint32_t *l_twn, uint32_t lstride,
                                           unsigned long long *rec = nullptr, bool skip_tw = false, bool fast_bin = false) {
    if (!NO_MAPS && (STAGED_ONLY || e.maps)) {
        float x, y;
        if (e.plane == 0) { x = px; y = py; }
        else if (e.plane == 1) { x = px; y = pz; }
        else { x = pz; y = py; }
        int ix, iy;
        if (fast_bin) {     // (united atoms with GORDER_FLAG_UA_FAST_NORMALISE, carbons the fast construction kept)
            ix = grid_index_fast(x, e.x0, e.inv_binx, e.nx);
            iy = grid_index_fast(y, e.y0, e.inv_biny, e.ny);
        } else {
            ix = grid_index(x, e.x0, e.binx, e.nx, e.bin_core != 0);
            iy = grid_index(y, e.y0, e.biny, e.ny, e.bin_core != 0);
        }
        if (ix >= 0 && iy >= 0) {
            // ONE atomic per sample: count and tick sum share a 64-bit word, and with leaflets only the
            // sample's own leaflet plane is touched (total = upper + lower, bond.rs:199-213); k_fold_maps
            // unpacks.  Scattered 64-bit atomics run at ~24 G/s on gfx950 whatever the scope or table size
            // (tools/microbench/atomic_scatter.hip), so their number is what counts.
            const size_t nt = (size_t)e.nx * e.ny, t = (size_t)ix * e.ny + (size_t)iy;
            if (STAGED_ONLY || rec) {   // staged: (plane * tiles + tile) << 32 | tick, added to the map by k_map_accumulate
                *rec = ((unsigned long long)((leaflet > 0 ? nt : 0) + t) << 32) | (unsigned long long)(uint32_t)tick;
            } else {
                const size_t w = leaflet > 0 ? a.n_acc : 0;
                atomicAdd(&e.map_packed[(w + gslot) * nt + t], kMapOne + (unsigned long long)(long long)tick);
            }
        }
    }
    if (!STAGED_ONLY && e.tw && !skip_tw) {
        atomicAdd(&l_tw[lslot], tick);
        atomicAdd(&l_twn[lslot], 1u);
        if (leaflet == 0) {         // (the lower leaflet's row is total - upper: gorder_hip_timewise takes the difference)
            atomicAdd(&l_tw[lstride + lslot], tick);
            atomicAdd(&l_twn[lstride + lslot], 1u);
        }
    }
}

// flush the block's per-frame partial sums to the timewise rows (one frame)
__device__ __forceinline__ void extras_flush_tw(const FrameArgs &a, const ExtraArgs &e, const uint32_t *slots,
                                                uint32_t n_slots, uint32_t f, int *l_tw, uint32_t *l_twn,
                                                uint32_t lstride) {
    for (uint32_t ls = threadIdx.x; ls < n_slots; ls += blockDim.x) {
        const size_t row = ((size_t)e.tw_row0 + f) * 3u * a.n_acc;
        for (uint32_t w = 0; w < 2; w++) {          // total, upper (the lower leaflet's row is their difference)
            const uint32_t n = l_twn[w * lstride + ls];
            if (n) {
                atomicAdd(&e.tw_sums[row + (size_t)w * a.n_acc + slots[ls]],
                          (unsigned long long)(long long)l_tw[w * lstride + ls]);
                atomicAdd(&e.tw_cnts[row + (size_t)w * a.n_acc + slots[ls]], (unsigned long long)n);
            }
            l_tw[w * lstride + ls] = 0;
            l_twn[w * lstride + ls] = 0;
        }
    }
}


// A thread's staged samples of one block of kRecFrames frames (from frame f_first; kMapNoSample where there is none) to
// the blocked layout described at ExtraArgs::map_rec: 32 bytes of its own.
__device__ __forceinline__ void rec_store(const ExtraArgs &e, uint32_t tile_id, uint32_t f_first, uint32_t tid,
                                          const unsigned long long (&v)[kRecFrames]) {
    static_assert(kRecFrames == 4, "a thread's four words");
    typedef unsigned long long ull2 __attribute__((ext_vector_type(2)));
    ull2 *row = reinterpret_cast<ull2 *>(e.map_rec + (size_t)tile_id * kBlock * e.rec_stride +
                                         (size_t)((f_first - e.rec_frame0) / kRecFrames) * (kRecFrames * kBlock) + (size_t)tid * kRecFrames);
    __builtin_nontemporal_store(ull2{v[0], v[1]}, row);               // (written once, read once by k_map_accumulate)
    __builtin_nontemporal_store(ull2{v[2], v[3]}, row + 1);
}
// the ordermap's grid for the tiled kernels' staged words, which go to `words` (a thread's kRecFrames of a stage); no tick words
__device__ __forceinline__ TiledMapOut tiled_map_out(const ExtraArgs &e, unsigned long long *words) {
    TiledMapOut mo{};
    mo.plane = e.plane; mo.x0 = e.x0; mo.y0 = e.y0; mo.binx = e.binx; mo.biny = e.biny; mo.nx = e.nx; mo.ny = e.ny;
    mo.bin_core = e.bin_core; mo.words = words;
    return mo;
}

// MAPS_ONLY: staged ordermap samples and nothing else (no geometry selection, timewise rows, per-molecule normals)
template <bool ACOS_COS, bool MAPS_ONLY>
__global__ __launch_bounds__(kBlock) void k_bonds_extras(FrameArgs a_in, ExtraArgs e, const float *__restrict__ xyz,
                                                          const float *__restrict__ box9,
                                                          const uint8_t *__restrict__ aflags,
                                                          const uint32_t *__restrict__ arow,
                                                          const Tile *__restrict__ tiles,
                                                          const Item *__restrict__ items,
                                                          const uint32_t *__restrict__ tile_slots, uint32_t n_tiles) {
    __shared__ unsigned long long l_s[2 * kBlock];
    __shared__ uint32_t l_n[2 * kBlock];
    __shared__ int l_tw[MAPS_ONLY ? 1 : 3 * kBlock];
    __shared__ uint32_t l_twn[MAPS_ONLY ? 1 : 3 * kBlock];
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
    if (!MAPS_ONLY)
        for (uint32_t k = tid; k < 3 * kBlock; k += kBlock) { l_tw[k] = 0; l_twn[k] = 0; }
    __syncthreads();
    SampleAcc acc;
    unsigned long long recs[kRecFrames] = {kMapNoSample, kMapNoSample, kMapNoSample, kMapNoSample};
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
        unsigned long long rec = kMapNoSample;
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
        if (active) {
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
            const float mx = p1x + vx / 2.0f, my = p1y + vy / 2.0f, mz = p1z + vz / 2.0f;
            bool in = true;
            if (!MAPS_ONLY && e.geom_kind) {
                float box[3] = {1.0f, 1.0f, 1.0f};
                if (a.pbc) { const float *b = a.box9 + 9 * (size_t)f; box[0] = b[0]; box[1] = b[4]; box[2] = b[8]; }
                in = geom_inside(e, e.shapes + 8 * (size_t)f, mx, my, mz, box, a.pbc != 0, bad);
            }
            if (in) {
                float sch;
                if (!MAPS_ONLY && e.dyn) {   // the molecule's own normal of this frame, fetched after the geometry test (bond.rs:429-431)
                    const float4 n = e.dyn[(size_t)f * a.n_mol_total + it.mol];
                    if (e.touched) e.touched[(size_t)f * a.n_mol_total + it.mol] = 1;     // (racing lanes store the same byte)
                    if (n.w < 3.0f) raise_error(a.err, GORDER_ERR_DYNAMIC_NORMAL, f, kStageTypes, gslot, 1, it.mol, (uint32_t)n.w);
                    const float n2sq = (n.x * n.x + n.y * n.y) + n.z * n.z;
                    sch = gm_calc_sch<ACOS_COS>(vx, vy, vz, n.x, n.y, n.z, __builtin_sqrtf(n2sq), n2sq);
                } else if (!ACOS_COS && e.axis >= 0) {     // the static normal is a coordinate axis: K1's short form, same bits
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
                extras_add<MAPS_ONLY>(a, e, gslot, it.lslot, tick, mx, my, mz, leaflet, l_tw, l_twn, kBlock,
                                      (MAPS_ONLY || e.map_rec) ? &rec : nullptr);
            }
        }
        if (MAPS_ONLY || e.map_rec) {   // staged samples: a thread's words of kRecFrames frames go out together
            const uint32_t c = (f - f_begin) % kRecFrames;      // the host keeps f_begin - rec_frame0 a multiple of kRecFrames
#pragma unroll
            for (uint32_t m = 0; m < kRecFrames; m++) recs[m] = m == c ? rec : recs[m];      // (selects: the array stays in registers)
            if (c == kRecFrames - 1 || f + 1 == f_end) {
                rec_store(e, tile_id, f - c, tid, recs);
#pragma unroll
                for (uint32_t m = 0; m < kRecFrames; m++) recs[m] = kMapNoSample;
            }
        }
        if (!MAPS_ONLY && e.tw) {
            __syncthreads();
            extras_flush_tw(a, e, tile_slots + t.slot0, t.n_slots, f, l_tw, l_twn, kBlock);
            __syncthreads();
        }
    }
    if (bad) raise_box_range(a.err, f_begin);
    // static arrays of its own, untouched so far: no barrier ahead of the fold
    fold_tile_sums(a.rep, a.n_rep, a.n_acc, tc, acc, l_s, l_n, [&] { return tile_slots[tc.t.slot0 + tc.tid]; });
}

// ---- ordermaps and nothing else, bonds: K1's staging (kernels_bonds.h: a tile's atom window of G = kRecFrames frames
// HBM -> registers -> LDS, every byte read once, the next stage's loads in flight) with the staged map words as a second
// output: compute_core<MAPS> leaves a thread's word per frame of the stage in registers, and they go out as one 16-byte
// store + one of four bytes (rec_store).  k_bonds_extras<*, true> — a thread gathers its two atoms per frame from global memory — took 294 us per
// 3000 frames of the 256-lipid all-atom membrane where this kernel's read-only twin takes 144.
// grid = n_tiles * n_chunks (frames_per_chunk a multiple of kRecFrames, a.frame0 = the sub-range's first frame).
template <int NPF, bool PBC, bool LEAF, int AXIS>
__global__ __launch_bounds__(kBlock, 4) void k_bonds_tiled_maps(FrameArgs a_in, ExtraArgs e, const float *__restrict__ xyz,
                                                               const float *__restrict__ box9, const uint8_t *__restrict__ aflags,
                                                               const uint32_t *__restrict__ arow, const Tile *__restrict__ tiles,
                                                               const Item *__restrict__ items, const uint32_t *__restrict__ tile_slots,
                                                               uint32_t n_tiles, uint32_t lw) {
    constexpr int G = (int)kRecFrames;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using S = TiledStage<G, NPF, false, PBC, LEAF, AXIS>;
    FrameArgs a = a_in;
    a.xyz = xyz; a.box9 = box9; a.aflags = aflags; a.arow = arow;
    const TileCtx tc = tile_prologue(tiles, items, n_tiles, a.frame0, a.frames_per_chunk, a.n_frames);
    const auto &[t, it, tile_id, chunk, tid, active, f_begin, f_end] = tc;
    const uint32_t sk = tid / S::TPF, si = tid % S::TPF;
    const uint32_t f_full = f_begin + ((f_end - f_begin) / G) * G;
    unsigned long long words[kRecFrames] = {kMapNoSample, kMapNoSample, kMapNoSample, kMapNoSample};       // (padding lanes: none)
    const TiledMapOut mo = tiled_map_out(e, words);
    SampleAcc acc;
    int bad = 0;
    uint32_t nan_which = 0, nan_frame = kNoNan;
    v4f pre[NPF];
    if (f_begin < f_full) S::template load<false>(a, t, f_begin, f_end, sk, si, pre);
    for (uint32_t f0 = f_begin; f0 < f_full; f0 += G) {
        S::template store<false>(a, t, f0, f_end, sk, si, pre, lds, lw);
        __syncthreads();
        if (f0 + G < f_full) S::template load<false>(a, t, f0 + G, f_end, sk, si, pre);
        if (active) S::template compute<1>(a, t, it, f0, lds, lw, acc, bad, nan_which, nan_frame, &mo);
        rec_store(e, tile_id, f0, tid, words);
        __syncthreads();
    }
    if (f_full < f_end) {   // last, partial stage of the sub-range
        S::template load<true>(a, t, f_full, f_end, sk, si, pre);
        S::template store<true>(a, t, f_full, f_end, sk, si, pre, lds, lw);
        __syncthreads();
#pragma unroll
        for (uint32_t m = 0; m < kRecFrames; m++) words[m] = kMapNoSample;
        if (active) S::template compute_tail<1>(a, t, it, f_full, f_end, lds, lw, acc, bad, nan_which, nan_frame, &mo);
        rec_store(e, tile_id, f_full, tid, words);
        __syncthreads();
    }
    raise_tile_errors(a.err, tc, tile_slots, nan_which, nan_frame, bad);
    // the head of the staging LDS: this barrier ends its reads (so does the one that closes every stage: this one is kept
    // so that the kernel's code stays what it was)
    __syncthreads();
    fold_tile_sums(a.rep, a.n_rep, a.n_acc, tc, acc, lds, [&] { return tile_slots[tc.t.slot0 + tc.tid]; });
}

// ---- per-frame rows (timewise sums, timewise.rs:130-186), alone or (MAPS) with staged ordermaps, bonds: K1's staging
// again, the stage's ticks as a second output (and the ordermap words as a third, written like k_bonds_tiled_maps').  The tile's items come in slot order (MapRun), so the samples of a slot are neighbouring lanes: a
// lane leaves its tick (and leaflet) of each frame of the stage in LDS, and one thread per slot of the tile adds its run
// up — no LDS atomics (k_bonds_extras: two to four per sample, one lane per cycle) — and sends the frame's partial sums
// to the rows with the same global atomics as extras_flush_tw.  No barrier of its own: the ticks are written before the
// barrier that ends a stage and read behind it, next to the staging of the next stage.
// grid = n_tiles * n_chunks; items = the slot-ordered copy, e.item_run its runs.
// MOM: as in k_bonds_tiled — the tile's share of the membrane group's normal coordinates summed on the way, for a batch whose
// leaflets are assigned from this kernel's own read of the frames.
template <int NPF, bool PBC, bool LEAF, int AXIS, bool MAPS, bool MOM = false>
__global__ __launch_bounds__(kBlock, 4) void k_bonds_tiled_tw(FrameArgs a_in, ExtraArgs e, const float *__restrict__ xyz,
                                                             const float *__restrict__ box9, const uint8_t *__restrict__ aflags,
                                                             const uint32_t *__restrict__ arow, const Tile *__restrict__ tiles,
                                                             const Item *__restrict__ items, const uint32_t *__restrict__ tile_slots,
                                                             uint32_t n_tiles, uint32_t lw) {
    constexpr int G = (int)kRecFrames;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int l_tick[kRecFrames][kBlock];
    __shared__ uint8_t l_side[kRecFrames][kBlock];      // 0 upper, 1 lower (LEAF), 2: no sample
    __shared__ uint32_t l_slot_run[kBlock];             // per slot of the tile: (first lane << 16) | lanes
    __shared__ uint32_t l_slot_id[kBlock];              // ... and its accumulator slot
    using S = TiledStage<G, NPF, false, PBC, LEAF, AXIS>;
    FrameArgs a = a_in;
    a.xyz = xyz; a.box9 = box9; a.aflags = aflags; a.arow = arow;
    const uint32_t tile_id = blockIdx.x % n_tiles, chunk = blockIdx.x / n_tiles;
    const Tile t = tiles[tile_id];
    const uint32_t tid = threadIdx.x;
    const uint32_t sk = tid / S::TPF, si = tid % S::TPF;
    const bool active = tid < t.n_items;
    Item it{0, 0, 0, 0, 0};
    if (active) {       // (its own prologue, not tile_prologue: the item and its run come in under ONE test of `active`)
        it = items[t.item0 + tid];
        const uint32_t run = e.item_run[t.item0 + tid];
        if ((run >> 16) == tid) l_slot_run[it.lslot] = run;          // the first lane of a run writes it down
    }
    const uint32_t f_begin = a.frame0 + chunk * a.frames_per_chunk;
    const uint32_t f_end = min(a.n_frames, f_begin + a.frames_per_chunk);
    const TileCtx tc{t, it, tile_id, chunk, tid, active, f_begin, f_end};      // (for raise_tile_errors and fold_tile_sums)
    unsigned long long words[kRecFrames], mwords[MAPS ? kRecFrames : 1];
    TiledMapOut mo{};
    if (MAPS) {                     // the ordermap words as well (staged like k_bonds_tiled_maps')
        mo = tiled_map_out(e, mwords);
        mo.ticks = words;
    } else {
        mo.nx = 0;                  // ticks only: word = (lower << 32) | tick
        mo.words = words;
    }
    SampleAcc acc;
    int bad = 0;
    uint32_t nan_which = 0, nan_frame = kNoNan;
    v4f pre[NPF];
    const uint32_t my_slot = tid < t.n_slots ? tile_slots[t.slot0 + tid] : 0u;
    l_slot_id[tid] = my_slot;
    uint2 own = make_uint2(0u, 0u), my_head = make_uint2(0u, 0xffffffffu);
    if (MOM) {
        own = a.own[tile_id];
        const uint32_t hq = a.own_head_begin[tile_id] + (tid & 63u);
        if (hq < a.own_head_begin[tile_id + 1u]) my_head = a.own_heads[hq];
    }
    if (f_begin + G <= f_end) S::template load<false>(a, t, f_begin, f_end, sk, si, pre);
    for (uint32_t fs = f_begin; fs < f_end; fs += G) {
        const bool full = fs + G <= f_end;
        bool finite;
        if (full) {
            finite = S::template store<false, MOM>(a, t, fs, f_end, sk, si, pre, lds, lw);
        } else {
            S::template load<true>(a, t, fs, f_end, sk, si, pre);
            finite = S::template store<true, MOM>(a, t, fs, f_end, sk, si, pre, lds, lw);
        }
        __syncthreads();
        if (full && fs + 2u * G <= f_end) S::template load<false>(a, t, fs + G, f_end, sk, si, pre);     // next stage in flight
        if (MOM && fs + sk < f_end) {
            static_assert(!MOM || (uint32_t)G * 64u == kBlock, "a wave per frame slot");
            tiled_moments(a, t, own, tile_id, n_tiles, fs + sk, lds + (size_t)sk * lw, finite, my_head);
        }
#pragma unroll
        for (uint32_t k = 0; k < kRecFrames; k++) { words[k] = kMapNoSample; if (MAPS) mwords[k] = kMapNoSample; }
        if (active) {
            if (full) S::template compute<MAPS ? 3 : 2>(a, t, it, fs, lds, lw, acc, bad, nan_which, nan_frame, &mo);
            else S::template compute_tail<MAPS ? 3 : 2>(a, t, it, fs, f_end, lds, lw, acc, bad, nan_which, nan_frame, &mo);
        }
        if constexpr (MAPS) rec_store(e, tile_id, fs, tid, mwords);
#pragma unroll
        for (uint32_t k = 0; k < kRecFrames; k++) {
            l_tick[k][tid] = (int)(uint32_t)words[k];
            l_side[k][tid] = words[k] == kMapNoSample ? (uint8_t)2 : (uint8_t)(words[k] >> 32);
        }
        __syncthreads();
        // a thread per (slot of the tile, frame of the stage) adds the slot's run up; the next stage's staging goes on
        // meanwhile (other LDS), and its ticks are written behind its own barrier
        for (uint32_t w = tid; w < kRecFrames * t.n_slots; w += kBlock) {
            const uint32_t k = w % kRecFrames, ls = w / kRecFrames;
            if (fs + k >= f_end) continue;
            const uint32_t run = l_slot_run[ls], tid0 = run >> 16, n = run & 0xffffu;
            int s_all = 0, s_low = 0;
            uint32_t n_all = 0, n_low = 0;
            for (uint32_t j = 0; j < n; j++) {
                const uint32_t side = l_side[k][tid0 + j];
                const int tick = l_tick[k][tid0 + j];
                if (side == 2u) continue;
                s_all += tick; n_all += 1u;
                if (side == 1u) { s_low += tick; n_low += 1u; }
            }
            if (!n_all) continue;
            const uint32_t slot = l_slot_id[ls];
            const size_t row = ((size_t)e.tw_row0 + fs + k) * 3u * a.n_acc;
            atomicAdd(&e.tw_sums[row + slot], (unsigned long long)(long long)s_all);
            atomicAdd(&e.tw_cnts[row + slot], (unsigned long long)n_all);
            if (LEAF) {
                const uint32_t n_up = n_all - n_low;
                if (n_up) {
                    atomicAdd(&e.tw_sums[row + (size_t)a.n_acc + slot], (unsigned long long)(long long)(s_all - s_low));
                    atomicAdd(&e.tw_cnts[row + (size_t)a.n_acc + slot], (unsigned long long)n_up);
                }
                // (no atomics for the lower leaflet: its row is total - upper, taken by gorder_hip_timewise — a third of this
                // kernel's row traffic)
            }
        }
    }
    // the head of the staging LDS: its last reads, the last stage's samples, ended at that stage's second barrier (the run
    // sums behind it read other LDS); this barrier is kept so that the kernel's code stays what it was
    __syncthreads();
    raise_tile_errors(a.err, tc, tile_slots, nan_which, nan_frame, bad);
    fold_tile_sums(a.rep, a.n_rep, a.n_acc, tc, acc, lds, [&] { return my_slot; });      // (the slot came in with l_slot_id: no second load)
}

// ---- ordermaps, second step ------------------------------------------------------------------------
// The sample kernels stage every sample as five bytes (tick, plane-tile: ExtraArgs::map_rec), run by run; here a block
// owns ONE accumulator slot for a range of frames: it reads the slot's runs (gorder::MapRun, contiguous pieces),
// adds the samples into a packed map held in LDS (ds_add_u64) and flushes the tiles it touched
// into the global packed map with one atomic each.  Scattered global atomics run at ~24 G/s on this chip
// whatever one does (tools/microbench/atomic_scatter.hip); this way their number drops from one per sample to
// at most one per (slot, chunk, tile).
constexpr uint32_t kMapRunBatch = 1024;          // runs of a slot whose lanes k_map_accumulate lays out at a time
__global__ __launch_bounds__(1024) void k_map_accumulate(const unsigned long long *__restrict__ rec,
                                                         const gorder::MapRun *__restrict__ runs,
                                                         const uint32_t *__restrict__ run_begin, uint32_t n_slots,
                                                         uint32_t rec_frames, uint32_t rec_stride,
                                                         uint32_t frames_per_chunk, uint32_t k_max,
                                                         uint32_t n_words /* planes * tiles */, uint32_t n_tiles_map,
                                                         unsigned long long *__restrict__ map_packed, uint32_t n_acc) {
    extern __shared__ unsigned long long l_map[];
    typedef unsigned long long ull2 __attribute__((ext_vector_type(2)));
    const uint32_t slot = blockIdx.x % n_slots, chunk = blockIdx.x / n_slots;
    const uint32_t r0 = run_begin[slot], r1 = run_begin[slot + 1];
    if (r0 == r1) return;                               // no samples of this kind (bond / united atom) in the slot
    const uint32_t f0 = chunk * frames_per_chunk, f1 = min(rec_frames, f0 + frames_per_chunk);
    for (uint32_t w = threadIdx.x; w < n_words; w += blockDim.x) l_map[w] = 0ull;
    __syncthreads();
    auto add = [&](unsigned long long v) {
        if (v != kMapNoSample) atomicAdd(&l_map[(uint32_t)(v >> 32)], kMapOne + (unsigned long long)(long long)(int)(uint32_t)v);
    };
    if (k_max == 1u) {
        // Bond tiles.  A lane takes ONE molecule of the slot — lane j of a run — and walks its samples through the frame
        // blocks of its share of the chunk, in time order (the addresses are base + block * stride: no run table in the
        // loop, the next block's loads go out before this one's samples are added); samples that follow each other into
        // the same tile — a molecule moves less than a tile between most frames — are added up in registers and cost
        // ONE ds_add_u64.
        __shared__ uint32_t l_pref[kMapRunBatch + 1];
        const uint32_t fb0 = f0 / kRecFrames, fb1 = (f1 + kRecFrames - 1) / kRecFrames;
        for (uint32_t rb = r0; rb < r1; rb += kMapRunBatch) {
            const uint32_t nr = min(kMapRunBatch, r1 - rb);
            for (uint32_t i = threadIdx.x; i < nr; i += blockDim.x) l_pref[i + 1u] = runs[rb + i].n;
            if (threadIdx.x == 0) l_pref[0] = 0;
            __syncthreads();
            if (threadIdx.x < 64u) {            // inclusive scan by one wave
                uint32_t carry = 0;
                for (uint32_t i0 = 1; i0 <= nr; i0 += 64u) {
                    const uint32_t i = i0 + threadIdx.x, v = i <= nr ? l_pref[i] : 0u;
                    const uint32_t incl = wave_scan_shfl(v, threadIdx.x);
                    if (i <= nr) l_pref[i] = carry + incl;
                    carry += __shfl(incl, 63, 64);
                }
            }
            __syncthreads();
            const uint32_t total = l_pref[nr];
            // fewer molecules than threads: the frame blocks of the chunk are shared out among `parts` lanes per molecule
            const uint32_t parts = total ? max(1u, min(blockDim.x / total, fb1 - fb0)) : 1u;
            const uint32_t fb_per = (fb1 - fb0 + parts - 1u) / parts;
            for (uint32_t lane_item = threadIdx.x; lane_item < total * parts; lane_item += blockDim.x) {
                const uint32_t item = lane_item % total, part = lane_item / total;
                const uint32_t fb_lo = fb0 + part * fb_per, fb_hi = min(fb1, fb_lo + fb_per);
                uint32_t lo = 0, hi = nr;                      // the run with l_pref[lo] <= item < l_pref[lo + 1]
                while (hi - lo > 1u) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (l_pref[mid] <= item) lo = mid; else hi = mid;
                }
                const gorder::MapRun run = runs[rb + lo];
                const unsigned long long *base = rec + (size_t)run.tile * kBlock * rec_stride + kRecFrames * (run.tid0 + (item - l_pref[lo]));
                uint32_t cur = 0;
                unsigned long long sum = 0ull;
                ull2 wa, wb, na, nb;
                auto fetch = [&](uint32_t fb, ull2 &a2, ull2 &b2) {
                    const ull2 *p = reinterpret_cast<const ull2 *>(base + (size_t)fb * (kRecFrames * kBlock));
                    a2 = __builtin_nontemporal_load(p);
                    b2 = __builtin_nontemporal_load(p + 1);
                };
                if (fb_lo < fb_hi) fetch(fb_lo, na, nb);
                for (uint32_t fb = fb_lo; fb < fb_hi; fb++) {
                    wa = na; wb = nb;
                    if (fb + 1u < fb_hi) fetch(fb + 1u, na, nb);
                    const unsigned long long w[4] = {wa.x, wa.y, wb.x, wb.y};
#pragma unroll
                    for (uint32_t m = 0; m < 4u; m++) {
                        if (w[m] == kMapNoSample) continue;
                        const uint32_t pt = (uint32_t)(w[m] >> 32);
                        if (sum != 0ull && pt != cur) { atomicAdd(&l_map[cur], sum); sum = 0ull; }
                        cur = pt;
                        sum += kMapOne + (unsigned long long)(long long)(int)(uint32_t)w[m];
                    }
                }
                if (sum != 0ull) atomicAdd(&l_map[cur], sum);
            }
            __syncthreads();
        }
    } else {
        // united-atom tiles: few long runs — the whole block strides over each run's contiguous piece of the frames
        // [f0, f1) —, or many short ones: a wave per run at a time
        const uint32_t n_waves = blockDim.x >> 6;
        const bool per_wave = r1 - r0 >= n_waves;
        const uint32_t r_first = r0 + (per_wave ? threadIdx.x >> 6 : 0u), r_step = per_wave ? n_waves : 1u;
        const uint32_t i_first = per_wave ? threadIdx.x & 63u : threadIdx.x, i_step = per_wave ? 64u : blockDim.x;
        for (uint32_t r = r_first; r < r1; r += r_step) {
            const gorder::MapRun run = runs[r];
            const uint32_t total = (f1 - f0) * run.n;
            const unsigned long long *piece = rec + (((size_t)run.tile * k_max + run.k) * kBlock + run.tid0) * rec_stride + (size_t)f0 * run.n;
            // (the piece starts at a multiple of 16 words: pairs — 16-byte loads —, then the last chunk's odd word)
            for (uint32_t i = i_first; i < total / 2u; i += i_step) {
                const ull2 w = __builtin_nontemporal_load(reinterpret_cast<const ull2 *>(piece) + i);
                add(w.x);
                add(w.y);
            }
            if ((total & 1u) && i_first == 0u) add(piece[total - 1u]);
        }
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < n_words; w += blockDim.x) {
        const unsigned long long v = l_map[w];
        if (!v) continue;
        const uint32_t plane = w / n_tiles_map, t = w % n_tiles_map;
        atomicAdd(&map_packed[((size_t)plane * n_acc + slot) * n_tiles_map + t], v);
    }
}

}  // namespace
