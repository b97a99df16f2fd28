// kernels_neighbours.h — order by local composition: every molecule's count of neighbour atoms within a radius of its
// centre atom, frame by frame (k_neighbour_counts), and the order sums booked per class of that count (k_bonds_classes;
// gorder_hip_set_neighbour_classes).
// Part of the single translation unit gorder_hip.hip (included there behind kernels_radial.h); device code for gfx950 only.
#pragma once

namespace {

// The packed words of a workgroup's class table are the shell table's (kernels_radial.h): (count << 42) + tick sum, at most
// 256 samples a frame and word, chunks of at most kShellChunkMax frames (shells_chunks).
static_assert((unsigned long long)kShellChunkMax * kBlock < kMapFoldLimit, "a packed class word must not overflow in one chunk");
static_assert(gorder::kNeighbourPiece % 256u == 0 && gorder::kNeighbourPiece * sizeof(float4) == 16u * 1024u, "a piece of neighbour atoms is 16 KB of LDS");
static_assert(gorder::kNeighbourMaxClasses <= 256u, "a class is a byte");

struct ClassArgs {
    const uint32_t *centres;        // [n_mol_total] the centre atom of every molecule
    const uint32_t *neighbours;     // [n_neighbours] ascending atom indices
    uint32_t n_neighbours;
    float thr;                      // local_radius_threshold(radius): d2 < thr == sqrt(d2) < radius
    uint32_t n;                     // classes in use, 2..GORDER_NEIGHBOUR_MAX_CLASSES
    uint8_t *rows;                  // [frames][n_mol_total] the class of (frame, molecule); the row of frame f is f - row_base
    uint32_t row_base;
    int axis;                       // the static normal is this coordinate axis (0..2), or -1
    unsigned long long *rep;        // [n_rep][n][4][n_acc]: sum_total, sum_upper, cnt_total, cnt_upper per class
    uint32_t n_rep;
};

// Step 1 — the class of every (frame, molecule).  grid = (ceil(n_mol_total / 256), frames of the sub-range), block = 256; a
// thread owns one molecule's centre.  The neighbour atoms go through LDS in pieces of kNeighbourPiece float4 (x, y, z, the
// atom index as bits), loaded by the whole workgroup — four atoms a thread, consecutive lanes consecutive list entries —; the
// lane that stages an atom raises on an undefined position.  Every lane then walks the piece at the same address (a broadcast
// read: no bank conflict), four entries in flight.  The arithmetic of a pair is `take` of k_dyn_cov: the f32 difference, the
// minimum image per component under the frame's own box — one select chain, gm_min_image_step; a pair more than 1.5 box
// lengths apart goes through the literal loops for all three, which give the select's bits wherever one shift was enough —,
// d2 = (dx*dx + dy*dy) + dz*dz, counted where d2 < thr.  The centre atom itself is skipped by its index.  Lanes past the last
// molecule shadow the last one and write nothing.
__global__ __launch_bounds__(256) void k_neighbour_counts(ClassArgs c, const float *__restrict__ xyz, const float *__restrict__ box9,
                                                          uint32_t n_atoms, uint32_t n_mol_total, int pbc_in, uint32_t frame0, uint32_t *err) {
    __shared__ float4 l_piece[gorder::kNeighbourPiece];
    const uint32_t tid = threadIdx.x, f = frame0 + blockIdx.y;
    const uint32_t m_raw = blockIdx.x * 256u + tid;
    const bool mol_ok = m_raw < n_mol_total;
    const uint32_t m = mol_ok ? m_raw : n_mol_total - 1u;
    const float *x = xyz + (size_t)f * n_atoms * 3u;
    const uint32_t centre = c.centres[m];
    const float hx = x[3u * (size_t)centre], hy = x[3u * (size_t)centre + 1u], hz = x[3u * (size_t)centre + 2u];
    if (mol_ok && hx != hx) raise_error(err, GORDER_ERR_UNDEFINED_POSITION, f, kStageSystem, 0, 0, m, 0);
    const bool pbc = pbc_in != 0;
    float Lx = 1.0f, Ly = 1.0f, Lz = 1.0f;
    if (pbc) {
        const float *b = box9 + 9 * (size_t)f;
        Lx = b[0]; Ly = b[4]; Lz = b[8];
    }
    const float thr = c.thr;
    int bad = 0;
    uint32_t cnt = 0;
    auto take = [&](const float4 r, bool valid) {
        float dx = r.x - hx, dy = r.y - hy, dz = r.z - hz;
        if (pbc) {
            bool slow = false;
            const float sx = gm_min_image_step(dx, Lx, slow), sy = gm_min_image_step(dy, Ly, slow), sz = gm_min_image_step(dz, Lz, slow);
            if (__builtin_expect(slow, 0)) {
                dx = gm_min_image_loop(dx, Lx, bad); dy = gm_min_image_loop(dy, Ly, bad); dz = gm_min_image_loop(dz, Lz, bad);
            } else {
                dx = sx; dy = sy; dz = sz;
            }
        }
        const bool in = (dx * dx + dy * dy) + dz * dz < thr;      // == sqrt(..) < radius (local_radius_threshold)
        cnt += (valid && in && __float_as_uint(r.w) != centre) ? 1u : 0u;
    };
    const uint32_t n_pieces = gorder::neighbour_pieces(c.n_neighbours);
    for (uint32_t piece = 0; piece < n_pieces; piece++) {
        const uint32_t p0 = piece * gorder::kNeighbourPiece, len = gorder::neighbour_piece_len(c.n_neighbours, piece);
        __syncthreads();                // the walk over the piece before this one is through
#pragma unroll
        for (uint32_t k = 0; k < gorder::kNeighbourPiece / 256u; k++) {
            const uint32_t j = k * 256u + tid;
            if (j < len) {
                const uint32_t atom = c.neighbours[p0 + j];
                const float *p = x + 3u * (size_t)atom;
                const float4 r = make_float4(p[0], p[1], p[2], __uint_as_float(atom));
                // (every workgroup of the frame stages every atom: the first one speaks for all)
                if (r.x != r.x && blockIdx.x == 0) raise_error(err, GORDER_ERR_UNDEFINED_POSITION, f, kStageSystem, 1, 0, p0 + j, 1);
                l_piece[j] = r;
            }
        }
        __syncthreads();
        for (uint32_t j = 0; j < len; j += 4u) {
            float4 r[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) r[u] = l_piece[min(j + u, len - 1u)];
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) take(r[u], j + u < len);
        }
    }
    if (bad) raise_box_range(err, f);
    if (mol_ok) c.rows[(size_t)(f - c.row_base) * n_mol_total + m] = (uint8_t)min(cnt, c.n - 1u);
}

// Step 2 — k_bonds_shells with the class byte of (frame, molecule) in the shell's place and no geometry: every bond sample's
// ordinary tick (the one k_bonds_extras books for a static normal, either cosine) goes to (class, slot, leaflet) and to the
// ordinary sums.  grid = n_tiles * n_chunks, a thread owns one bond sample over its chunk.
//   LDS route: dynamic LDS holds the workgroup's table [planes][n classes][t.n_slots] of packed words for its whole frame
//     range; planes = upper, lower with leaflets (total = upper + lower), else one.  A lipid keeps its class and leaflet for
//     many frames, so a thread keeps the open word of its current (class, plane) in registers and sends it to the table — one
//     64-bit LDS atomic — only when that pair changes, and at the end.  The epilogue, a thread per slot of the tile, adds the
//     non-empty entries to the global class replicas and their sum over the classes to the handle's ordinary replica block:
//     gorder_hip_finish sees what the plain kernels would have left.
//   DIRECT: the table does not fit (or GORDER_HIP_NB_DIRECT): two to four global atomics per sample on the class replicas,
//     the ordinary sums in registers and reduced by fold_tile_sums (dynamic LDS: kTileFoldBytes).
template <bool ACOS_COS, bool DIRECT>
__global__ __launch_bounds__(kBlock) void k_bonds_classes(FrameArgs a_in, ClassArgs s, const float *__restrict__ xyz,
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
    unsigned long long *const class_rep = s.rep + (size_t)(blockIdx.x % s.n_rep) * s.n * 4u * a.n_acc;
    const uint8_t *const crow = s.rows + it.mol;
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
        if (a.pbc) {
            const float *b = a.box9 + 9 * (size_t)f;
            vx = gm_min_image(vx, b[0], bad);
            vy = gm_min_image(vy, b[4], bad);
            vz = gm_min_image(vz, b[8], bad);
        }
        if (p1x != p1x) raise_error(a.err, GORDER_ERR_UNDEFINED_POSITION, f, kStageTypes, gslot, 1, it.mol, 0);
        else if (p2x != p2x) raise_error(a.err, GORDER_ERR_UNDEFINED_POSITION, f, kStageTypes, gslot, 1, it.mol, 1);
        const uint32_t cls = min((uint32_t)crow[(size_t)(f - s.row_base) * a.n_mol_total], s.n - 1u);     // (k_neighbour_counts clamps already: the table index stays in range regardless)
        float sch;
        if (!ACOS_COS && s.axis >= 0) {     // the static normal is a coordinate axis: K1's short form, same bits
            bool rare = false;
            sch = s.axis == 0 ? gm_sch_axis<0>(vx, vy, vz, rare) : (s.axis == 1 ? gm_sch_axis<1>(vx, vy, vz, rare) : gm_sch_axis<2>(vx, vy, vz, rare));
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
            unsigned long long *p = class_rep + (size_t)cls * 4u * a.n_acc + gslot;
            atomicAdd(p, (unsigned long long)(long long)tick);
            atomicAdd(p + 2u * (size_t)a.n_acc, 1ull);
            if (leaflet == 0) {
                acc.s_up += tick; acc.n_up += 1;
                atomicAdd(p + a.n_acc, (unsigned long long)(long long)tick);
                atomicAdd(p + 3u * (size_t)a.n_acc, 1ull);
            }
        } else {
            const uint32_t at = ((leaflet > 0 ? s.n : 0u) + cls) * ns + it.lslot;
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
        unsigned long long *p = class_rep + (size_t)k * 4u * a.n_acc + slot;
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
