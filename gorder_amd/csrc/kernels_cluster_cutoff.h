// kernels_cluster_cutoff.h — spectral-clustering leaflets with a cut-off (GORDER_FLAG_CLUSTER_CUTOFF) for groups of up to
// kClCutMaxGroup atoms.  Part of the single translation unit gorder_hip.hip (behind kernels_cluster.h); gfx950 only.
//
// The definition is kernels_cluster.h's, truncated where f32 cannot see the difference: W_ij = cl_weight (expf(-d_ij^2), the
// one 3-D minimum image of the pair) where d_ij^2 < 36 nm^2 and 0 otherwise (expf(-36) = 2.3e-16 against a degree >= 1).
// Everything behind W is the dense route's: degrees, q = D^1/2 1 deflated exactly, Lanczos with min(n - 1, 300) steps from
// the same start vector, classical Gram-Schmidt twice against q and every earlier vector, the small problem every fourth
// step (cl_sturm, cl_inverse_iteration; tolerance and breakdown unchanged), row normalisation, the literal 2-means, and
// k_cluster_orient itself.  What differs is where the work runs: a frame is spread over (row tile, frame) grids, and a
// kernel boundary is the only grid-wide synchronisation.
//
// Per launch of up to `slab` assignment frames:
//   k_clcut_grid      frames x 256: the frame's cell grid: per dimension floor(L / 6 nm) cells (>= 1), the largest count
//                     lowered while the product exceeds kClCutMaxCells; L is the box edge, or without a box the extent of the
//                     heads' bounding box (cells only ever grow: always correct)
//   k_clcut_count     (ceil(n / 1024), frames) x 1024: cell of every atom, a histogram per block of 1024 atoms
//   k_clcut_scan      frames x 1024: per cell the running sum over the blocks, then the exclusive scan over the cells
//   k_clcut_scatter   (ceil(n / 1024), frames) x 1024: stable counting sort — an atom goes behind the earlier blocks' atoms
//                     of its cell and behind the earlier atoms of its own block: every cell holds ascending group indices
//   k_clcut_degrees   (ceil(n / 256), frames) x 256: deg, s = deg^-1/2, q = deg^1/2 in cell-sorted order
//   k_clcut_start     frames x 1024: |q|^2 and the start vector (element i of the group gets the dense route's value)
//   per Lanczos step j (the host queues all m_max steps; a frame whose `done` word is set leaves every kernel at once):
//     k_clcut_spmv    (row tiles, frames) x 256: w = S v_j, a row a thread, W recomputed from the sorted positions: the
//                     cells around the row's cell in a fixed order (z, y, x ascending offsets), inside a cell ascending;
//                     then the tile's part of b_d . w for q and v_0 .. v_j (a wave a vector, butterfly)
//     k_clcut_coef    frames x 512: the tiles' parts added in tile order: the Gram-Schmidt coefficients, alpha_j
//     k_clcut_update  (row tiles, frames) x 256: w -= sum coef_d b_d; second pass: the tile's part of |w|^2
//     k_clcut_dots    (row tiles, frames) x 256: the parts of b_d . w again (second pass)
//     k_clcut_small   frames x 1024: beta_j; every fourth step T's three largest eigenvalues and two Ritz vectors; sets `done`
//     k_clcut_scale   (row tiles, frames) x 256: v_{j+1} = w / beta_j
//   k_clcut_ritz      (row tiles, frames) x 256: the two Ritz vectors V y, written back in group order
//   k_clcut_embed     frames x 1024: k_cluster_embed with the rows in memory instead of registers (any n)
//   k_cluster_orient  (kernels_cluster.h)
// Every floating sum is a thread's own sequential sum, a wave_ops.h reduction of such sums, or a sum of per-tile parts in
// tile order; no floating-point atomics.  A frame's labels and statistics depend on the frame alone.
#pragma once

namespace {

constexpr uint32_t kClCutMaxGroup = 131072;   // bound on n_membrane with the flag: the basis of one frame is 158 MB
constexpr float kClCutR = 6.0f;               // cut-off distance (the reference's), nm
constexpr float kClCutR2 = 36.0f;
constexpr uint32_t kClCutMaxCells = 4096;     // cells a frame (the counting sort's histogram lives in LDS)
constexpr uint32_t kClCutTile = 256;          // rows a workgroup of the row-tile kernels
constexpr uint32_t kClCutSort = 1024;         // atoms a block of the counting sort
constexpr uint32_t kClCutNn = kClLd - 1;      // slot of a tile's |w|^2 in its row of parts (the dots take 0 .. m_max)
constexpr uint32_t kClCutScal = 8;            // doubles per frame: |q|^2, alpha_j, beta_j

struct ClCutGrid { float org[3], inv[3]; uint32_t nc[3], pad[3]; };      // 48 bytes: cell = (x - org) * inv per dimension

struct ClCutArgs {
    ClArgs c;                  // the dense route's arguments; pos, s, q, V are in cell-sorted order here, W is null
    ClCutGrid *grid;           // [slot]
    uint32_t *cell_of;         // [slot][n] cell of group atom i
    uint32_t *cnt;             // [slot][n_sort][kClCutMaxCells] atoms of the block in the cell, then: of the earlier blocks
    uint32_t *cell_start;      // [slot][kClCutMaxCells + 1]
    uint32_t *perm;            // [slot][n] group index of sorted row k
    double *part;              // [slot][n_tiles][kClLd] per-tile parts of the dot products, [kClCutNn]: of |w|^2
    double *coef;              // [slot][kClLd]
    double *albe;              // [slot][2][kClLd] alpha, beta
    double *scal;              // [slot][kClCutScal]
    float *e0, *e1;            // [slot][n] embedding rows in group order
    uint32_t *done;            // [slot] != 0: the frame's Lanczos run has ended
    uint32_t n_tiles, n_sort;
};

// cell of a coordinate along one dimension; NaN and anything outside go to a defined cell (such a frame fails by its degrees)
__device__ __forceinline__ uint32_t clcut_cell1(float x, float org, float inv, uint32_t nc, int pbc) {
    if (nc <= 1u) return 0u;
    float t = (x - org) * inv;
    if (pbc) t -= floorf(t / (float)nc) * (float)nc;
    return t >= 0.0f ? (uint32_t)fminf(t, (float)(nc - 1u)) : 0u;
}
__device__ __forceinline__ void clcut_cell3(const ClCutGrid &g, float x, float y, float z, int pbc, uint32_t (&c)[3]) {
    c[0] = clcut_cell1(x, g.org[0], g.inv[0], g.nc[0], pbc);
    c[1] = clcut_cell1(y, g.org[1], g.inv[1], g.nc[1], pbc);
    c[2] = clcut_cell1(z, g.org[2], g.inv[2], g.nc[2], pbc);
}

__global__ __launch_bounds__(256) void k_clcut_grid(ClCutArgs a) {
    __shared__ float red[2 * 16];
    const uint32_t slot = blockIdx.x, tid = threadIdx.x, n = a.c.n;
    const uint32_t f = a.c.aframes[slot];
    float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3];
    if (a.c.pbc) {
        cl_box(a.c, f, hi);
    } else {
        const float *x = a.c.xyz + (size_t)f * a.c.n_atoms * 3u;
        for (int d = 0; d < 3; d++) { lo[d] = 3.0e38f; hi[d] = -3.0e38f; }
        for (uint32_t i = tid; i < n; i += 256u) {
            const float *p = x + 3u * (size_t)a.c.group[i];
            for (int d = 0; d < 3; d++)
                if (p[d] - p[d] == 0.0f) { lo[d] = fminf(lo[d], p[d]); hi[d] = fmaxf(hi[d], p[d]); }
        }
        for (int d = 0; d < 3; d++) block_minmax(lo[d], hi[d], red);
    }
    if (tid != 0) return;
    ClCutGrid g{};
    float len[3];
    for (int d = 0; d < 3; d++) {
        len[d] = hi[d] - lo[d];
        const bool ok = (len[d] - len[d] == 0.0f) && len[d] > 0.0f;
        g.nc[d] = ok ? max(1u, (uint32_t)fminf(floorf(len[d] / kClCutR), (float)kClCutMaxCells)) : 1u;
    }
    while ((size_t)g.nc[0] * g.nc[1] * g.nc[2] > kClCutMaxCells) {
        int big = 0;
        if (g.nc[1] > g.nc[big]) big = 1;
        if (g.nc[2] > g.nc[big]) big = 2;
        g.nc[big]--;
    }
    for (int d = 0; d < 3; d++) { g.org[d] = lo[d]; g.inv[d] = g.nc[d] > 1u ? (float)g.nc[d] / len[d] : 0.0f; }
    a.grid[slot] = g;
}

__global__ __launch_bounds__(1024) void k_clcut_count(ClCutArgs a) {
    __shared__ uint32_t hist[kClCutMaxCells];
    const uint32_t slot = blockIdx.y, tid = threadIdx.x, n = a.c.n, i = blockIdx.x * kClCutSort + tid;
    for (uint32_t k = tid; k < kClCutMaxCells; k += 1024u) hist[k] = 0u;
    __syncthreads();
    if (i < n) {
        const ClCutGrid g = a.grid[slot];
        const float *p = a.c.xyz + ((size_t)a.c.aframes[slot] * a.c.n_atoms + a.c.group[i]) * 3u;
        uint32_t c[3];
        clcut_cell3(g, p[0], p[1], p[2], a.c.pbc, c);
        const uint32_t cell = (c[2] * g.nc[1] + c[1]) * g.nc[0] + c[0];
        a.cell_of[(size_t)slot * n + i] = cell;
        atomicAdd(&hist[cell], 1u);
    }
    __syncthreads();
    uint32_t *cnt = a.cnt + ((size_t)slot * a.n_sort + blockIdx.x) * kClCutMaxCells;
    for (uint32_t k = tid; k < kClCutMaxCells; k += 1024u) cnt[k] = hist[k];
}

__global__ __launch_bounds__(1024) void k_clcut_scan(ClCutArgs a) {
    __shared__ uint32_t wsum[16];
    const uint32_t slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t *cnt = a.cnt + (size_t)slot * a.n_sort * kClCutMaxCells;
    // cells 4 tid .. 4 tid + 3: the blocks' counts become the counts of the blocks before
    uint32_t tot[4] = {0u, 0u, 0u, 0u};
    for (uint32_t b = 0; b < a.n_sort; b++) {
        uint4 *at = (uint4 *)(cnt + (size_t)b * kClCutMaxCells) + tid;
        const uint4 v = *at;
        *at = make_uint4(tot[0], tot[1], tot[2], tot[3]);
        tot[0] += v.x; tot[1] += v.y; tot[2] += v.z; tot[3] += v.w;
    }
    const uint32_t mine = tot[0] + tot[1] + tot[2] + tot[3];
    const uint32_t incl = wave_scan_shfl(mine, lane);
    if (lane == 63u) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine;
    for (uint32_t w = 0; w < wave; w++) before += wsum[w];
    uint32_t *cs = a.cell_start + (size_t)slot * (kClCutMaxCells + 1u);
    for (int k = 0; k < 4; k++) { cs[4u * tid + k] = before; before += tot[k]; }
    if (tid == 1023u) cs[kClCutMaxCells] = before;
}

__global__ __launch_bounds__(1024) void k_clcut_scatter(ClCutArgs a) {
    __shared__ uint32_t lc[kClCutSort];
    const uint32_t slot = blockIdx.y, tid = threadIdx.x, n = a.c.n, i = blockIdx.x * kClCutSort + tid;
    const uint32_t cell = i < n ? a.cell_of[(size_t)slot * n + i] : 0xffffffffu;
    lc[tid] = cell;
    __syncthreads();
    if (i >= n) return;
    uint32_t rank = 0;
    for (uint32_t j = 0; j < tid; j++) rank += lc[j] == cell ? 1u : 0u;
    const uint32_t dest = a.cell_start[(size_t)slot * (kClCutMaxCells + 1u) + cell] +
                          a.cnt[((size_t)slot * a.n_sort + blockIdx.x) * kClCutMaxCells + cell] + rank;
    if (dest >= n) return;                  // (cannot happen: the counts are those of the same cell_of)
    const float *p = a.c.xyz + ((size_t)a.c.aframes[slot] * a.c.n_atoms + a.c.group[i]) * 3u;
    float *pos = a.c.pos + (size_t)slot * 3u * n;
    pos[dest] = p[0]; pos[n + dest] = p[1]; pos[2u * n + dest] = p[2];
    a.perm[(size_t)slot * n + dest] = i;
}

// sum over the cells around row k's cell of W_kj (DEG) or of W_kj (s_j v_j), in double; the order is fixed by the row's cell
template <bool DEG>
__device__ __forceinline__ double clcut_row(const ClCutArgs &a, uint32_t slot, const ClCutGrid &g, const float *pos, const float *s,
                                            const float *v, uint32_t k, const float (&box)[3], int &bad) {
    const uint32_t n = a.c.n;
    const int pbc = a.c.pbc;
    const float px = pos[k], py = pos[n + k], pz = pos[2u * n + k];
    const uint32_t *cs = a.cell_start + (size_t)slot * (kClCutMaxCells + 1u);
    uint32_t home[3];
    clcut_cell3(g, px, py, pz, pbc, home);
    // a dimension with fewer than three cells is walked once over all of them: no pair is met twice
    int first[3], count[3];
    for (int d = 0; d < 3; d++) {
        if (g.nc[d] < 3u) { first[d] = 0; count[d] = (int)g.nc[d]; }
        else { first[d] = (int)home[d] - 1; count[d] = 3; }
    }
    double acc = 0.0;
    for (int iz = 0; iz < count[2]; iz++) {
        int cz = first[2] + iz;
        if (cz < 0 || cz >= (int)g.nc[2]) { if (!pbc) continue; cz += cz < 0 ? (int)g.nc[2] : -(int)g.nc[2]; }
        for (int iy = 0; iy < count[1]; iy++) {
            int cy = first[1] + iy;
            if (cy < 0 || cy >= (int)g.nc[1]) { if (!pbc) continue; cy += cy < 0 ? (int)g.nc[1] : -(int)g.nc[1]; }
            for (int ix = 0; ix < count[0]; ix++) {
                int cx = first[0] + ix;
                if (cx < 0 || cx >= (int)g.nc[0]) { if (!pbc) continue; cx += cx < 0 ? (int)g.nc[0] : -(int)g.nc[0]; }
                const uint32_t cell = ((uint32_t)cz * g.nc[1] + (uint32_t)cy) * g.nc[0] + (uint32_t)cx;
                const uint32_t jb = cs[cell], je = min(cs[cell + 1u], n);
                for (uint32_t j = jb; j < je; j++) {
                    const float qx = pos[j], qy = pos[n + j], qz = pos[2u * n + j];
                    // cl_weight's distance, statement for statement (the compiler folds the two)
                    float vx = px - qx, vy = py - qy, vz = pz - qz;
                    if (pbc) { vx = gm_min_image(vx, box[0], bad); vy = gm_min_image(vy, box[1], bad); vz = gm_min_image(vz, box[2], bad); }
                    const float d2 = (vx * vx + vy * vy) + vz * vz;
                    if (d2 >= kClCutR2) continue;                    // (a NaN distance stays in and fails the frame)
                    const float wv = cl_weight(px, py, pz, qx, qy, qz, box, pbc, bad);
                    if (DEG) acc += (double)wv;
                    else acc += (double)(wv * (s[j] * v[j]));
                }
            }
        }
    }
    return acc;
}

__global__ __launch_bounds__(256) void k_clcut_degrees(ClCutArgs a) {
    const uint32_t slot = blockIdx.y, n = a.c.n, k = blockIdx.x * kClCutTile + threadIdx.x;
    if (k >= n) return;
    const uint32_t f = a.c.aframes[slot];
    float box[3];
    cl_box(a.c, f, box);
    int bad = 0;
    const ClCutGrid g = a.grid[slot];
    const double deg = clcut_row<true>(a, slot, g, a.c.pos + (size_t)slot * 3u * n, nullptr, nullptr, k, box, bad);
    const float d = (float)deg;
    const bool finite = (d - d) == 0.0f;
    if (bad) { raise_box_range(a.c.err, f); atomicOr(&a.c.fail[slot], 2u); }
    if (!finite) { raise_error(a.c.err, GORDER_ERR_CLUSTERING, f, kStageSystem); atomicOr(&a.c.fail[slot], 1u); }
    a.c.s[(size_t)slot * n + k] = (finite && d > 1e-10f) ? 1.0f / __builtin_sqrtf(d) : 0.0f;
    a.c.q[(size_t)slot * n + k] = finite ? __builtin_sqrtf(d) : 0.0f;
}

__global__ __launch_bounds__(1024) void k_clcut_start(ClCutArgs a) {
    __shared__ double red[16];
    const uint32_t slot = blockIdx.x, tid = threadIdx.x, n = a.c.n;
    if (a.c.fail[slot]) {                                                       // (uniform)
        if (tid == 0) { a.c.sol[(size_t)slot * kClSol + 2 * kClLd + 3] = 0.0; a.done[slot] = 1u; }
        return;
    }
    const float *q = a.c.q + (size_t)slot * n;
    const uint32_t *perm = a.perm + (size_t)slot * n;
    float *V = a.c.V + (size_t)slot * (a.c.m_max + 1u) * n;
    double qq[1] = {0.0};
    for (uint32_t k = tid; k < n; k += 1024u) qq[0] += (double)q[k] * (double)q[k];
    block_sum_n<1>(qq, red);
    const double qn = qq[0];
    double d1[1] = {0.0};
    for (uint32_t k = tid; k < n; k += 1024u) {
        const float st = (float)((perm[k] * 2654435761u) >> 16) * (1.0f / 65536.0f) - 0.5f;
        V[k] = st;
        d1[0] += (double)st * (double)q[k];
    }
    block_sum_n<1>(d1, red);
    const double c = d1[0] / qn;
    double d2[1] = {0.0};
    for (uint32_t k = tid; k < n; k += 1024u) {
        const float v = (float)((double)V[k] - c * (double)q[k]);
        V[k] = v;
        d2[0] += (double)v * (double)v;
    }
    block_sum_n<1>(d2, red);
    const float inv = (float)(1.0 / sqrt(d2[0]));
    for (uint32_t k = tid; k < n; k += 1024u) V[k] *= inv;
    if (tid == 0) a.scal[(size_t)slot * kClCutScal] = qn;
}

// the tile's parts of b_d . w for d = 0 .. j + 1 (b_{j+1} = q): a wave a vector, the tile's rows over the lanes
__device__ __forceinline__ void clcut_tile_dots(const ClCutArgs &a, uint32_t slot, uint32_t tile, int j, const float *V,
                                                const float *q, const float *lw) {
    const uint32_t n = a.c.n, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, k0 = tile * kClCutTile;
    const uint32_t len = min(kClCutTile, n - k0);
    double *part = a.part + ((size_t)slot * a.n_tiles + tile) * kClLd;
    for (int d = (int)wave; d <= j + 1; d += (int)(kClCutTile / 64u)) {
        const float *b = (d <= j ? V + (size_t)d * n : q) + k0;
        double sum = 0.0;
        for (uint32_t r = lane; r < len; r += 64u) sum += (double)b[r] * (double)lw[r];
        sum = wave_sum_bfly(sum);
        if (lane == 0u) part[d] = sum;
    }
}

__global__ __launch_bounds__(256) void k_clcut_spmv(ClCutArgs a, int j) {
    __shared__ float lw[kClCutTile];
    const uint32_t slot = blockIdx.y, tid = threadIdx.x, n = a.c.n, k = blockIdx.x * kClCutTile + tid;
    if (a.done[slot]) return;                                                   // (uniform)
    const uint32_t f = a.c.aframes[slot];
    float box[3];
    cl_box(a.c, f, box);
    int bad = 0;
    const float *s = a.c.s + (size_t)slot * n, *q = a.c.q + (size_t)slot * n;
    float *V = a.c.V + (size_t)slot * (a.c.m_max + 1u) * n;
    float w = 0.0f;
    if (k < n) {
        const ClCutGrid g = a.grid[slot];
        const double acc = clcut_row<false>(a, slot, g, a.c.pos + (size_t)slot * 3u * n, s, V + (size_t)j * n, k, box, bad);
        w = s[k] * (float)acc;
        V[(size_t)(j + 1) * n + k] = w;
    }
    lw[tid] = w;
    if (bad) raise_box_range(a.c.err, f);
    __syncthreads();
    clcut_tile_dots(a, slot, blockIdx.x, j, V, q, lw);
}

__global__ __launch_bounds__(256) void k_clcut_dots(ClCutArgs a, int j) {
    __shared__ float lw[kClCutTile];
    const uint32_t slot = blockIdx.y, tid = threadIdx.x, n = a.c.n, k = blockIdx.x * kClCutTile + tid;
    if (a.done[slot]) return;                                                   // (uniform)
    const float *V = a.c.V + (size_t)slot * (a.c.m_max + 1u) * n;
    lw[tid] = k < n ? V[(size_t)(j + 1) * n + k] : 0.0f;
    __syncthreads();
    clcut_tile_dots(a, slot, blockIdx.x, j, V, a.c.q + (size_t)slot * n, lw);
}

__global__ __launch_bounds__(512) void k_clcut_coef(ClCutArgs a, int j, int pass) {
    const uint32_t slot = blockIdx.x;
    const int d = (int)threadIdx.x;
    if (a.done[slot] || d > j + 1) return;
    const double *part = a.part + (size_t)slot * a.n_tiles * kClLd + d;
    double sum = 0.0;
    for (uint32_t t = 0; t < a.n_tiles; t++) sum += part[(size_t)t * kClLd];
    double *scal = a.scal + (size_t)slot * kClCutScal;
    if (d == j + 1) sum /= scal[0];
    a.coef[(size_t)slot * kClLd + d] = sum;
    if (d == j) scal[1] = pass ? scal[1] + sum : sum;
}

__global__ __launch_bounds__(256) void k_clcut_update(ClCutArgs a, int j, int pass) {
    __shared__ double coef[kClLd];
    __shared__ double red[16];
    const uint32_t slot = blockIdx.y, tid = threadIdx.x, n = a.c.n, k = blockIdx.x * kClCutTile + tid;
    if (a.done[slot]) return;                                                   // (uniform)
    for (int d = (int)tid; d <= j + 1; d += (int)kClCutTile) coef[d] = a.coef[(size_t)slot * kClLd + d];
    __syncthreads();
    float *V = a.c.V + (size_t)slot * (a.c.m_max + 1u) * n;
    double ww = 0.0;
    if (k < n) {
        double sum = coef[j + 1] * (double)a.c.q[(size_t)slot * n + k];
        for (int d = 0; d <= j; d++) sum += coef[d] * (double)V[(size_t)d * n + k];
        const float w = (float)((double)V[(size_t)(j + 1) * n + k] - sum);
        V[(size_t)(j + 1) * n + k] = w;
        ww = (double)w * (double)w;
    }
    if (!pass) return;                                                          // (uniform)
    ww = block_sum(ww, red);
    if (tid == 0) a.part[((size_t)slot * a.n_tiles + blockIdx.x) * kClLd + kClCutNn] = ww;
}

// beta_j, and on every fourth step (or at the end) the small problem exactly as k_cluster_lanczos states it
__global__ __launch_bounds__(1024) void k_clcut_small(ClCutArgs a, int j) {
    __shared__ double al[kClLd], be[kClLd];
    __shared__ double wk[2][6][kClLd];
    __shared__ double s_lo[3], s_hi[3], s_x[3][256], s_beta;
    __shared__ int s_sel[3];
    const uint32_t slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (a.done[slot]) return;                                                   // (uniform)
    double *albe = a.albe + (size_t)slot * 2u * kClLd, *scal = a.scal + (size_t)slot * kClCutScal;
    const int m = j + 1, m_max = (int)a.c.m_max;
    if (tid == 0) {
        const double *part = a.part + (size_t)slot * a.n_tiles * kClLd + kClCutNn;
        double nn = 0.0;
        for (uint32_t t = 0; t < a.n_tiles; t++) nn += part[(size_t)t * kClLd];
        const double beta = sqrt(nn);
        albe[j] = scal[1]; albe[kClLd + j] = beta; scal[2] = beta;
        s_beta = beta;
    }
    __syncthreads();
    const double beta = s_beta;
    const bool breakdown = !(beta >= kClBreakdown);
    if (!(breakdown || m == m_max || m % kClCheckEvery == 0)) return;           // (uniform)
    for (int i = (int)tid; i < m; i += 1024) { al[i] = albe[i]; be[i] = albe[kClLd + i]; }
    __syncthreads();
    if (tid < 3u) {
        double lo = 1e300, hi = -1e300;
        for (int i = 0; i < m; i++) {
            const double rad = (i > 0 ? fabs(be[i - 1]) : 0.0) + (i + 1 < m ? fabs(be[i]) : 0.0);
            lo = fmin(lo, al[i] - rad); hi = fmax(hi, al[i] + rad);
        }
        const double pad = 1e-6 * (1.0 + fmax(fabs(lo), fabs(hi)));
        s_lo[tid] = lo - pad; s_hi[tid] = hi + pad;
    }
    __syncthreads();
    const uint32_t e = tid >> 8, g = tid & 255u;
    for (int round = 0; round < 5; round++) {
        if (tid < 3u) s_sel[tid] = 256;
        __syncthreads();
        if (e < 3u && (int)e < m) {
            const double x = s_lo[e] + (s_hi[e] - s_lo[e]) * (double)(g + 1u) / 257.0;
            s_x[e][g] = x;
            if (cl_sturm(al, be, m, x) > m - 1 - (int)e) atomicMin(&s_sel[e], (int)g);
        }
        __syncthreads();
        if (tid < 3u && (int)tid < m) {
            const int sel = s_sel[tid];
            if (sel < 256) { s_hi[tid] = s_x[tid][sel]; if (sel > 0) s_lo[tid] = s_x[tid][sel - 1]; }
            else s_lo[tid] = s_x[tid][255];
        }
        __syncthreads();
    }
    if (lane == 0u && wave < 2u && (int)wave < m)
        cl_inverse_iteration(al, be, m, 0.5 * (s_lo[wave] + s_hi[wave]), wk[wave], (int)wave);
    __syncthreads();
    if (tid == 0 && m >= 2) {
        double *y0 = wk[0][4], *y1 = wk[1][4], dot = 0.0, nn1 = 0.0;
        for (int i = 0; i < m; i++) dot += y0[i] * y1[i];
        for (int i = 0; i < m; i++) { y1[i] -= dot * y0[i]; nn1 += y1[i] * y1[i]; }
        nn1 = sqrt(nn1);
        if (nn1 > 0.0) for (int i = 0; i < m; i++) y1[i] /= nn1;
    }
    __syncthreads();
    const int nw = m < 2 ? m : 2;
    double res = 0.0;
    for (int k = 0; k < nw; k++) res = fmax(res, fabs(be[m - 1] * wk[k][4][m - 1]));
    if (!(breakdown || m == m_max || res < kClRitzTol)) return;                 // (every thread reads the same LDS values)
    double *sol = a.c.sol + (size_t)slot * kClSol;
    for (uint32_t k = tid; k < 2u * kClLd; k += 1024u) {
        const int which = (int)(k / kClLd), idx = (int)(k % kClLd);
        sol[k] = (which < m && idx < m) ? wk[which][4][idx] : 0.0;
    }
    if (tid < 3u) sol[2 * kClLd + tid] = (int)tid < m ? 0.5 * (s_lo[tid] + s_hi[tid]) : __builtin_nan("");
    if (tid == 3u) { sol[2 * kClLd + 3] = (double)m; a.done[slot] = 1u; }
}

__global__ __launch_bounds__(256) void k_clcut_scale(ClCutArgs a, int j) {
    const uint32_t slot = blockIdx.y, n = a.c.n, k = blockIdx.x * kClCutTile + threadIdx.x;
    if (a.done[slot] || k >= n) return;
    const float inv = (float)(1.0 / a.scal[(size_t)slot * kClCutScal + 2]);
    a.c.V[((size_t)slot * (a.c.m_max + 1u) + (size_t)(j + 1)) * n + k] *= inv;
}

__global__ __launch_bounds__(256) void k_clcut_ritz(ClCutArgs a) {
    __shared__ double y[2][kClLd];
    const uint32_t slot = blockIdx.y, tid = threadIdx.x, n = a.c.n, k = blockIdx.x * kClCutTile + tid;
    if (a.c.fail[slot]) return;                                                 // (uniform)
    const double *sol = a.c.sol + (size_t)slot * kClSol;
    const int m = (int)sol[2 * kClLd + 3];
    for (uint32_t i = tid; i < 2u * kClLd; i += kClCutTile) y[i / kClLd][i % kClLd] = sol[i];
    __syncthreads();
    if (k >= n) return;
    const float *V = a.c.V + (size_t)slot * (a.c.m_max + 1u) * n;
    double s0 = 0.0, s1 = 0.0;
    for (int d = 0; d < m; d++) { const double v = (double)V[(size_t)d * n + k]; s0 += v * y[0][d]; s1 += v * y[1][d]; }
    const uint32_t i = a.perm[(size_t)slot * n + k];
    a.e0[(size_t)slot * n + i] = (float)s0;
    a.e1[(size_t)slot * n + i] = (float)s1;
}

// k_cluster_embed behind k_clcut_ritz: the same statements in the same order, the rows in memory
__global__ __launch_bounds__(1024) void k_clcut_embed(ClCutArgs a) {
    __shared__ double red[6 * 16];
    __shared__ float s_row[4];
    const uint32_t slot = blockIdx.x, tid = threadIdx.x, n = a.c.n;
    const double *sol = a.c.sol + (size_t)slot * kClSol;
    float *meta = a.c.meta + (size_t)slot * kClMeta;
    uint8_t *lab = a.c.lab + (size_t)slot * n;
    float *emb = a.c.emb + (size_t)slot * n, *e0 = a.e0 + (size_t)slot * n, *e1 = a.e1 + (size_t)slot * n;
    if (a.c.fail[slot]) {                                                       // (uniform)
        for (uint32_t i = tid; i < n; i += 1024u) { lab[i] = 0; emb[i] = 0.0f; }
        if (tid < kClMeta) meta[tid] = 0.0f;
        return;
    }
    const int m = (int)sol[2 * kClLd + 3];
    // the sign of v2: row 0's coordinate is not negative
    if (tid == 0) s_row[0] = e0[0];
    __syncthreads();
    const float sgn = s_row[0] < 0.0f ? -1.0f : 1.0f;
    __syncthreads();
    for (uint32_t i = tid; i < n; i += 1024u) {
        float x = e0[i] * sgn, y = e1[i];
        const float nr = __builtin_sqrtf(x * x + y * y);
        if (nr > 1e-10f) { x /= nr; y /= nr; }
        e0[i] = x; e1[i] = y; emb[i] = x;
    }
    __syncthreads();
    // ---- 2-means (clustering.rs:614-696): centroids = rows 0 and 1
    if (tid == 0) { s_row[0] = e0[0]; s_row[1] = e1[0]; s_row[2] = e0[1]; s_row[3] = e1[1]; }
    __syncthreads();
    float c0x = s_row[0], c0y = s_row[1], c1x = s_row[2], c1y = s_row[3];
    const float r0x = c0x, r0y = c0y;
    bool first = true;
    int rounds = 0;
    double cnt[6] = {0, 0, 0, 0, 0, 0};
    for (int it = 0; it < 100; it++) {
        bool changed = first;
        for (int q = 0; q < 6; q++) cnt[q] = 0.0;
        for (uint32_t i = tid; i < n; i += 1024u) {
            const float x = e0[i], y = e1[i];
            float dx = x - c0x, dy = y - c0y;
            const float d0 = __builtin_sqrtf((0.0f + dx * dx) + dy * dy);
            dx = x - c1x; dy = y - c1y;
            const float d1 = __builtin_sqrtf((0.0f + dx * dx) + dy * dy);
            float mn = __builtin_inff();
            uint32_t best = 0;
            if (d0 < mn) { mn = d0; best = 0; }
            if (d1 < mn) { mn = d1; best = 1; }
            if (!first && lab[i] != (uint8_t)best) changed = true;
            lab[i] = (uint8_t)best;
            cnt[best] += 1.0; cnt[2 + 2 * best] += (double)x; cnt[3 + 2 * best] += (double)y;
        }
        rounds++;
        double ch[1] = {changed ? 1.0 : 0.0};
        block_sum_n<1>(ch, red);
        block_sum_n<6>(cnt, red);
        if (ch[0] == 0.0) break;
        if (cnt[0] > 0.0) { c0x = (float)cnt[2] / (float)cnt[0]; c0y = (float)cnt[3] / (float)cnt[0]; } else { c0x = r0x; c0y = r0y; }
        if (cnt[1] > 0.0) { c1x = (float)cnt[4] / (float)cnt[1]; c1y = (float)cnt[5] / (float)cnt[1]; } else { c1x = r0x; c1y = r0y; }
        first = false;
    }
    if (tid == 0) {
        meta[0] = (float)(1.0 - sol[2 * kClLd + 0]); meta[1] = (float)(1.0 - sol[2 * kClLd + 1]); meta[2] = (float)(1.0 - sol[2 * kClLd + 2]);
        meta[3] = (float)m; meta[4] = (float)rounds; meta[5] = (float)cnt[0]; meta[6] = (float)cnt[1]; meta[7] = 0.0f;
    }
}

}  // namespace
