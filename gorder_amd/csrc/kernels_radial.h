// kernels_radial.h — radial profiles: order sums per shell of distance from the reference of a cylinder or sphere selection
// (k_bonds_shells; gorder_hip_set_radial_shells).
// Part of the single translation unit gorder_hip.hip (included there behind kernels_extras.h); device code for gfx950 only.
#pragma once

namespace {

// A workgroup's packed table words hold (count << 42) + tick sum like the ordermap words (kernels_common.h): at most 256
// items of a tile share a slot, so a word receives at most 256 samples a frame and stays below kMapFoldLimit = 2^21 samples
// while the workgroup's chunk is at most 4096 frames (2^20 samples).  The host cuts the chunks accordingly (shells_chunks).
constexpr uint32_t kShellChunkMax = 4096;
static_assert((unsigned long long)kShellChunkMax * 256u < kMapFoldLimit, "a packed shell word must not overflow in one chunk");

struct ShellArgs {
    uint32_t n;                             // shells in use, 1..GORDER_RADIAL_MAX_SHELLS
    // local_radius_threshold(radii[k]); +inf from n on.  thr[n - 1] is ExtraArgs::geom_thr bit for bit: the selection itself.
    float thr[GORDER_RADIAL_MAX_SHELLS];
    unsigned long long *rep;                // [n_rep][n][4][n_acc]: sum_total, sum_upper, cnt_total, cnt_upper per shell
    uint32_t n_rep;
};

// The shell of a sample inside the selection (d2 < thr[n - 1]): the number of thresholds at or below d2.  Shell k is
// thr[k - 1] <= d2 < thr[k], i.e. r[k - 1] <= sqrt(d2) < r[k] (local_radius_threshold).  The thresholds are uniform and
// come through the kernel arguments; the loop is unrolled so that none is picked by a run-time index.
__device__ __forceinline__ uint32_t shell_index(const ShellArgs &s, float d2) {
    uint32_t k = 0;
#pragma unroll
    for (int i = 0; i + 1 < GORDER_RADIAL_MAX_SHELLS; i++) k += d2 >= s.thr[i] ? 1u : 0u;
    return min(k, s.n - 1u);        // (k < n already: the host keeps the thresholds ascending; the table index stays in range regardless)
}

// geom_inside of a cylinder or sphere without its radius test: the squared distance d2 in geom_inside's operation order,
// and whether the sample passes everything that does not depend on the radius (the cylinder's span and x >= 0).
__device__ __forceinline__ bool shell_geom(const ExtraArgs &e, const float *sh, float px, float py, float pz,
                                           const float *box, bool pbc, int &bad, float &d2) {
    if (e.geom_kind == GORDER_GEOM_CYLINDER) {
        const int o = e.geom_orient;
        const float dx = px - sh[0], dy = py - sh[1], dz = pz - sh[2];
        float x = o == 0 ? dx : (o == 1 ? dy : dz), da = o == 0 ? dy : (o == 1 ? dz : dx), db = o == 0 ? dz : (o == 1 ? dx : dy);
        if (pbc) {
            const float bo = o == 0 ? box[0] : (o == 1 ? box[1] : box[2]), ba = o == 0 ? box[1] : (o == 1 ? box[2] : box[0]),
                        bb = o == 0 ? box[2] : (o == 1 ? box[0] : box[1]);
            da = gm_min_image(da, ba, bad); db = gm_min_image(db, bb, bad); x = gm_wrap(x, bo, bad);
        }
        d2 = da * da + db * db;
        return (pbc ? true : (x >= 0.0f)) && (x <= sh[7]);
    }
    float dx = px - sh[0], dy = py - sh[1], dz = pz - sh[2];
    if (pbc) { dx = gm_min_image(dx, box[0], bad); dy = gm_min_image(dy, box[1], bad); dz = gm_min_image(dz, box[2], bad); }
    d2 = (dx * dx + dy * dy) + dz * dz;
    return true;
}

// k_bonds_extras for a cylinder or sphere selection and nothing else (no maps, rows, per-molecule normals), with the
// selection's samples booked per shell as well.  grid = n_tiles * n_chunks, a thread owns one bond sample over its chunk.
//   LDS route: dynamic LDS holds the workgroup's table [planes][n shells][t.n_slots] of packed words for its whole frame
//     range; planes = upper, lower with leaflets (a sample touches its own plane only, total = upper + lower), else one.
//     A lipid stays in its shell and leaflet for many frames, so a thread keeps the open word of its current (shell, plane)
//     in registers and sends it to the table — one 64-bit LDS atomic — only when that pair changes, and at the end.
//     The epilogue, a thread per slot of the tile, adds the non-empty entries to the global shell replicas and their sum
//     over the shells to the handle's ordinary replica block: gorder_hip_finish sees what k_bonds_extras would have left.
//   DIRECT: the table does not fit (or GORDER_HIP_RADIAL_DIRECT): two to four global atomics per sample on the shell
//     replicas, the ordinary sums in registers and reduced by fold_tile_sums (dynamic LDS: kTileFoldBytes).
template <bool ACOS_COS, bool DIRECT>
__global__ __launch_bounds__(kBlock) void k_bonds_shells(FrameArgs a_in, ExtraArgs e, ShellArgs s, const float *__restrict__ xyz,
                                                          const float *__restrict__ box9,
                                                          const uint8_t *__restrict__ aflags,
                                                          const uint32_t *__restrict__ arow,
                                                          const Tile *__restrict__ tiles,
                                                          const Item *__restrict__ items,
                                                          const uint32_t *__restrict__ tile_slots, uint32_t n_tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long l_tab[];
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
    const uint32_t planes = a.leaflets ? 2u : 1u, ns = t.n_slots;
    if (!DIRECT) {
        for (uint32_t k = tid; k < planes * s.n * ns; k += kBlock) l_tab[k] = 0;
        __syncthreads();
    }
    unsigned long long *const shell_rep = s.rep + (size_t)(blockIdx.x % s.n_rep) * s.n * 4u * a.n_acc;
    SampleAcc acc;                              // DIRECT
    uint32_t open_at = 0;                       // LDS route: table index of the open word ...
    unsigned long long open_word = 0;           // ... and what this thread has added to it since it was opened
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
        float box[3] = {1.0f, 1.0f, 1.0f};
        if (a.pbc) {
            const float *b = a.box9 + 9 * (size_t)f;
            box[0] = b[0]; box[1] = b[4]; box[2] = b[8];
            vx = gm_min_image(vx, box[0], bad);
            vy = gm_min_image(vy, box[1], bad);
            vz = gm_min_image(vz, box[2], bad);
        }
        if (p1x != p1x) raise_error(a.err, GORDER_ERR_UNDEFINED_POSITION, f, kStageTypes, gslot, 1, it.mol, 0);
        else if (p2x != p2x) raise_error(a.err, GORDER_ERR_UNDEFINED_POSITION, f, kStageTypes, gslot, 1, it.mol, 1);
        // bond position = p1 + v / 2 (bond.rs:422); geometry filter (bond.rs:424-426), the radius test against the last threshold
        const float mx = p1x + vx / 2.0f, my = p1y + vy / 2.0f, mz = p1z + vz / 2.0f;
        float d2;
        const bool rest = shell_geom(e, e.shapes + 8 * (size_t)f, mx, my, mz, box, a.pbc != 0, bad, d2);
        if (!(rest && d2 < e.geom_thr)) continue;
        const uint32_t shell = shell_index(s, d2);
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
        if (DIRECT) {
            acc.s_tot += tick;
            acc.n_tot += 1;
            unsigned long long *p = shell_rep + (size_t)shell * 4u * a.n_acc + gslot;
            atomicAdd(p, (unsigned long long)(long long)tick);
            atomicAdd(p + 2u * (size_t)a.n_acc, 1ull);
            if (leaflet == 0) {
                acc.s_up += tick; acc.n_up += 1;
                atomicAdd(p + a.n_acc, (unsigned long long)(long long)tick);
                atomicAdd(p + 3u * (size_t)a.n_acc, 1ull);
            }
        } else {
            const uint32_t at = ((leaflet > 0 ? s.n : 0u) + shell) * ns + it.lslot;
            if (at != open_at) {
                if (open_word) atomicAdd(&l_tab[open_at], open_word);
                open_at = at; open_word = 0;
            }
            open_word += kMapOne + (unsigned long long)(long long)tick;
        }
    }
    if (bad) raise_box_range(a.err, f_begin);
    unsigned long long *accp = a.rep + (size_t)(blockIdx.x % a.n_rep) * 4u * a.n_acc;
    if (DIRECT) {
        // the dynamic LDS, which this route has not touched so far: no barrier ahead of the fold
        fold_tile_sums(a.rep, a.n_rep, a.n_acc, tc, acc, l_tab, [&] { return tile_slots[tc.t.slot0 + tc.tid]; });
        return;
    }
    if (open_word) atomicAdd(&l_tab[open_at], open_word);
    __syncthreads();
    if (tid >= ns) return;
    const uint32_t slot = tile_slots[t.slot0 + tid];
    long long s_tot = 0, s_up = 0;
    unsigned long long n_tot = 0, n_up = 0;
    for (uint32_t k = 0; k < s.n; k++) {
        const unsigned long long w0 = l_tab[k * ns + tid], w1 = a.leaflets ? l_tab[(s.n + k) * ns + tid] : 0ull;
        if (!(w0 | w1)) continue;
        long long s0, s1 = 0;
        unsigned long long c0, c1 = 0;
        map_unpack(w0, s0, c0);
        if (a.leaflets) map_unpack(w1, s1, c1);
        unsigned long long *p = shell_rep + (size_t)k * 4u * a.n_acc + slot;
        atomicAdd(p, (unsigned long long)(s0 + s1));
        atomicAdd(p + 2u * (size_t)a.n_acc, c0 + c1);
        s_tot += s0 + s1; n_tot += c0 + c1;
        if (a.leaflets && c0) {
            atomicAdd(p + a.n_acc, (unsigned long long)s0);
            atomicAdd(p + 3u * (size_t)a.n_acc, c0);
            s_up += s0; n_up += c0;
        }
    }
    if (n_tot) {
        atomicAdd(&accp[slot], (unsigned long long)s_tot);
        atomicAdd(&accp[2u * a.n_acc + slot], n_tot);
        if (n_up) {
            atomicAdd(&accp[a.n_acc + slot], (unsigned long long)s_up);
            atomicAdd(&accp[3u * a.n_acc + slot], n_up);
        }
    }
}

}  // namespace
