// kernels_cluster.h — spectral-clustering leaflets (GORDER_LEAFLETS_CLUSTERING) for membranes of any shape.
// Part of the single translation unit gorder_hip.hip (included behind kernels_leaflets.h); device code for gfx950 only.
//
// LeafletClassification::clustering (clustering.rs:478-800), the precise route only, one definition for every frame:
//   W_ij = expf(-sigma d_ij^2) over the n atoms of "ClusterHeads" (sigma = 1, no cut-off), deg = W 1, s = deg^-1/2,
//   S = diag(s) W diag(s), L = I - S.  The eigenvector of L's eigenvalue 0 is q = D^1/2 1 in closed form; it is deflated
//   and the two largest eigenpairs of S on q's complement are the embedding (v2, v3); rows normalised, literal 2-means
//   from rows 0 and 1, orientation ab initio (frame 0) or by overlap with the previous assignment frame's clusters.
// Four kernels per launch of up to `slab` assignment frames, every frame independent until the last one:
//   k_cluster_degrees   (ceil(n / 256), frames) x 256: compact positions, deg (column tiles of positions in LDS), s, sqrt(deg)
//   k_cluster_lanczos   frames x 1024: Lanczos with full reorthogonalisation (classical Gram-Schmidt, twice) on S, W
//                       recomputed from positions staged in LDS; T's three largest eigenvalues by multisection of the
//                       Sturm count, the two wanted Ritz vectors of T by inverse iteration, stop on their residuals
//   k_cluster_embed     frames x 1024: Ritz vectors V y, row normalisation, 2-means, populations
//   k_cluster_orient    1 x 1024: walks the frames in order against the carried clusters, writes the molecule flags
// Every floating sum is either a thread's own sequential sum or a wave_ops.h reduction of such sums: a frame's labels and
// statistics depend on the frame alone (and, for the orientation, on its predecessor).
#pragma once

namespace {

constexpr uint32_t kClMaxGroup = 8192;     // documented bound on n_membrane for this dense route (reference: 5 000)
constexpr uint32_t kClMinGroup = 2;        // NotEnoughAtomsToCluster, leaflets.rs:96-105
constexpr int kClMaxSteps = 300;           // LANCZOS_ITERATIONS
constexpr int kClLd = 304;                 // leading dimension of the small arrays (>= kClMaxSteps)
constexpr float kClSigma = 1.0f;           // PRECISE_SIGMA
constexpr double kClRitzTol = 5e-6;        // stop when |beta_m y_m| of both wanted pairs is below this (|S| = 1)
constexpr double kClBreakdown = 1e-6;      // beta below this: the Krylov space is exhausted
constexpr int kClCheckEvery = 4;           // the small eigenproblem is solved every fourth step
constexpr uint32_t kClTile = 512;          // column tile of positions in LDS
constexpr uint32_t kClSol = 2 * kClLd + 8; // doubles per frame: y2, y3, theta[3], steps
constexpr uint32_t kClMeta = 8;            // floats per frame: L's eigenvalues 2-4, steps, 2-means rounds, |c1|, |c2|

struct ClArgs {
    const float *xyz;
    const float *box9;
    uint32_t n_atoms;
    const uint32_t *aframes;   // [n_assign] frame in the batch of each assignment frame of this launch
    uint32_t n_assign;
    const uint32_t *group;     // [n] atoms of "ClusterHeads"
    uint32_t n;
    int pbc;
    uint32_t m_max;            // min(n - 1, kClMaxSteps)
    // scratch, one slot per assignment frame of the launch
    float *pos;                // [slot][3][n]
    float *s;                  // [slot][n] deg^-1/2
    float *q;                  // [slot][n] deg^1/2
    float *V;                  // [slot][m_max + 1][n] Lanczos basis
    float *W;                  // [slot][n][n] the weights stored once a frame (development switch), or null: recomputed
    double *sol;               // [slot][kClSol]
    float *emb;                // [slot][n] first embedding coordinate, row-normalised
    uint8_t *lab;              // [slot][n] 2-means labels
    float *meta;               // [slot][kClMeta]
    uint32_t *fail;            // [slot] != 0: the frame raised an error, later kernels skip it
    uint32_t *err;
};

struct ClOrientArgs {
    const uint32_t *aframes;
    uint32_t n_assign, n, row0;
    const uint8_t *is_frame0;  // [n_assign] frame_index == 0: ab-initio orientation
    const uint8_t *lab;
    const float *emb;
    const float *meta;
    const uint32_t *fail;
    uint8_t *carry;            // [n] oriented labels (0 upper, 1 lower, before flip) of the previous assignment frame
    uint8_t *aflags;           // [rows][n_mol_total]
    uint32_t n_mol_total;
    const uint32_t *head_slot; // [n_mol_total] slot of heads[k] in the group
    float *adist;              // [n_mol_total] written for the last frame (or null)
    float *stats;              // [12] written for the last frame (or null)
    int flip;
    uint32_t *err;
};

// squared minimum-image distance (PBC3D::distance over XYZ, as sph_distance) -> weight
__device__ __forceinline__ float cl_weight(float px, float py, float pz, float qx, float qy, float qz, const float (&box)[3],
                                           int pbc, int &bad) {
    float vx = px - qx, vy = py - qy, vz = pz - qz;
    if (pbc) { vx = gm_min_image(vx, box[0], bad); vy = gm_min_image(vy, box[1], bad); vz = gm_min_image(vz, box[2], bad); }
    const float d2 = (vx * vx + vy * vy) + vz * vz;
    return expf(-kClSigma * d2);
}

__device__ __forceinline__ void cl_box(const ClArgs &a, uint32_t f, float (&box)[3]) {
    box[0] = box[1] = box[2] = 1.0f;
    if (a.pbc) { const float *b = a.box9 + 9 * (size_t)f; box[0] = b[0]; box[1] = b[4]; box[2] = b[8]; }
}

__global__ __launch_bounds__(256) void k_cluster_degrees(ClArgs a) {
    __shared__ float tx[256], ty[256], tz[256];
    const uint32_t slot = blockIdx.y, tid = threadIdx.x, n = a.n, i = blockIdx.x * 256u + tid;
    const uint32_t f = a.aframes[slot];
    const float *x = a.xyz + (size_t)f * a.n_atoms * 3u;
    float box[3];
    cl_box(a, f, box);
    int bad = 0;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (i < n) { const float *p = x + 3u * (size_t)a.group[i]; px = p[0]; py = p[1]; pz = p[2]; }
    double deg = 0.0;
    for (uint32_t c0 = 0; c0 < n; c0 += 256u) {
        const uint32_t j = c0 + tid;
        if (j < n) { const float *p = x + 3u * (size_t)a.group[j]; tx[tid] = p[0]; ty[tid] = p[1]; tz[tid] = p[2]; }
        __syncthreads();
        const uint32_t len = min(256u, n - c0);
        if (i < n)
            for (uint32_t jj = 0; jj < len; jj++) {
                const float wv = cl_weight(px, py, pz, tx[jj], ty[jj], tz[jj], box, a.pbc, bad);
                deg += (double)wv;
                if (a.W) a.W[((size_t)slot * n + (c0 + jj)) * n + i] = wv;      // W_ji = W_ij bit for bit: column i, coalesced
            }
        __syncthreads();
    }
    if (i >= n) return;
    const float d = (float)deg;
    const bool finite = (d - d) == 0.0f;
    if (bad) { raise_box_range(a.err, f); atomicOr(&a.fail[slot], 2u); }
    if (!finite) { raise_error(a.err, GORDER_ERR_CLUSTERING, f, kStageSystem); atomicOr(&a.fail[slot], 1u); }
    float *pos = a.pos + (size_t)slot * 3u * n;
    pos[i] = px; pos[n + i] = py; pos[2u * n + i] = pz;
    a.s[(size_t)slot * n + i] = (finite && d > 1e-10f) ? 1.0f / __builtin_sqrtf(d) : 0.0f;
    a.q[(size_t)slot * n + i] = finite ? __builtin_sqrtf(d) : 0.0f;
}

// number of eigenvalues of the tridiagonal (al, be) of order m below x (Sturm count)
__device__ __forceinline__ int cl_sturm(const double *al, const double *be, int m, double x) {
    int c = 0;
    double qv = al[0] - x;
    if (qv < 0.0) c++;
    for (int i = 1; i < m; i++) {
        if (fabs(qv) < 1e-30) qv = qv < 0.0 ? -1e-30 : 1e-30;
        qv = (al[i] - x) - be[i - 1] * be[i - 1] / qv;
        if (qv < 0.0) c++;
    }
    return c;
}

// (T - theta) y = b twice from b = 1 (inverse iteration), tridiagonal elimination with partial pivoting; y normalised in w[4]
// (start 0: b = 1; start 1: b alternates in sign and grows along the index — another vector of a shared eigenplane)
__device__ __noinline__ void cl_inverse_iteration(const double *al, const double *be, int m, double theta, double (*w)[kClLd],
                                                  int start) {
    double *d = w[0], *du = w[1], *du2 = w[2], *fc = w[3], *b = w[4];
    if (m == 1) { b[0] = 1.0; return; }
    for (int i = 0; i < m; i++) { d[i] = al[i] - theta; du[i] = i + 1 < m ? be[i] : 0.0; du2[i] = 0.0; b[i] = start ? ((i & 1) ? -1.0 : 1.0) * (1.0 + (double)i / (double)m) : 1.0; }
    // factorise; fc[i] is the multiplier, its sign bit trick is avoided: du2[i] != 0 or the flag in fc's companion tells a swap
    // (a swap is recorded by storing the multiplier in fc[i] and 1.0 in w[5][i])
    double *sw = w[5];
    for (int i = 0; i + 1 < m; i++) {
        const double dl = be[i];
        if (fabs(d[i]) >= fabs(dl)) {
            if (fabs(d[i]) < 1e-30) d[i] = 1e-30;
            const double fact = dl / d[i];
            d[i + 1] -= fact * du[i];
            fc[i] = fact; sw[i] = 0.0;
        } else {
            const double fact = d[i] / dl;
            d[i] = dl;
            const double temp = d[i + 1];
            d[i + 1] = du[i] - fact * temp;
            if (i + 2 < m) { du2[i] = du[i + 1]; du[i + 1] = -fact * du2[i]; }
            du[i] = temp;
            fc[i] = fact; sw[i] = 1.0;
        }
    }
    if (fabs(d[m - 1]) < 1e-30) d[m - 1] = 1e-30;
    for (int it = 0; it < 2; it++) {
        for (int i = 0; i + 1 < m; i++) {
            if (sw[i] == 0.0) b[i + 1] -= fc[i] * b[i];
            else { const double t = b[i]; b[i] = b[i + 1]; b[i + 1] = t - fc[i] * b[i]; }
        }
        b[m - 1] /= d[m - 1];
        if (m > 1) b[m - 2] = (b[m - 2] - du[m - 2] * b[m - 1]) / d[m - 2];
        for (int i = m - 3; i >= 0; i--) b[i] = (b[i] - du[i] * b[i + 1] - du2[i] * b[i + 2]) / d[i];
        double big = 0.0;
        for (int i = 0; i < m; i++) big = fmax(big, fabs(b[i]));
        if (!(big > 0.0) || !(big < 1e300)) { for (int i = 0; i < m; i++) b[i] = i == 0 ? 1.0 : 0.0; big = 1.0; }
        double nn = 0.0;
        for (int i = 0; i < m; i++) { b[i] /= big; nn += b[i] * b[i]; }
        nn = sqrt(nn);
        for (int i = 0; i < m; i++) b[i] /= nn;
    }
}

__global__ __launch_bounds__(1024) void k_cluster_lanczos(ClArgs a) {
    __shared__ float tp[3][kClTile], tu[kClTile];
    __shared__ double part[1024];
    __shared__ double al[kClLd], be[kClLd], coef[kClLd + 1];
    __shared__ double red[3 * 16];
    __shared__ double wk[2][6][kClLd];
    __shared__ double s_lo[3], s_hi[3], s_x[3][256];
    __shared__ int s_sel[3];
    const uint32_t slot = blockIdx.x, tid = threadIdx.x, n = a.n, lane = tid & 63u, wave = tid >> 6;
    double *sol = a.sol + (size_t)slot * kClSol;
    if (a.fail[slot]) { if (tid == 0) sol[2 * kClLd + 3] = 0.0; return; }      // (uniform)
    const uint32_t f = a.aframes[slot];
    float box[3];
    cl_box(a, f, box);
    int bad = 0;
    const float *pos = a.pos + (size_t)slot * 3u * n, *s = a.s + (size_t)slot * n, *q = a.q + (size_t)slot * n;
    float *V = a.V + (size_t)slot * (a.m_max + 1u) * n;
    const float *Wst = a.W ? a.W + (size_t)slot * n * n : nullptr;
    const int m_max = (int)a.m_max;
    // rows x column slices: P threads share a row while P n <= 1024
    uint32_t P = 1;
    while (2u * P * n <= 1024u) P *= 2u;
    const uint32_t rows_pad = 1024u / P, r = tid % rows_pad, p = tid / rows_pad;

    // |q|^2 = sum of the degrees
    double qq[1] = {0.0};
    for (uint32_t i = tid; i < n; i += 1024u) qq[0] += (double)q[i] * (double)q[i];
    block_sum_n<1>(qq, red);
    const double qn = qq[0];
    // fixed start vector, made orthogonal to q and normalised
    {
        double d1[1] = {0.0};
        for (uint32_t i = tid; i < n; i += 1024u) {
            const float st = (float)((i * 2654435761u) >> 16) * (1.0f / 65536.0f) - 0.5f;
            V[i] = st;
            d1[0] += (double)st * (double)q[i];
        }
        block_sum_n<1>(d1, red);
        const double c = d1[0] / qn;
        double d2[1] = {0.0};
        for (uint32_t i = tid; i < n; i += 1024u) {
            const float v = (float)((double)V[i] - c * (double)q[i]);
            V[i] = v;
            d2[0] += (double)v * (double)v;
        }
        block_sum_n<1>(d2, red);
        const float inv = (float)(1.0 / sqrt(d2[0]));
        for (uint32_t i = tid; i < n; i += 1024u) V[i] *= inv;
        __syncthreads();
    }

    int m = 0;
    bool done = false;
    for (int j = 0; j < m_max && !done; j++) {
        const float *vj = V + (size_t)j * n;
        float *w = V + (size_t)(j + 1) * n;
        // ---- w = S v_j: u = s v_j staged with the tile's positions; a chunk of rows_pad rows at a time (one chunk up to
        // 1024 atoms: the tiles are staged once)
        for (uint32_t rb = 0; rb < n; rb += rows_pad) {
            const uint32_t i = rb + r;
            float px = 0.0f, py = 0.0f, pz = 0.0f;
            if (i < n) { px = pos[i]; py = pos[n + i]; pz = pos[2u * n + i]; }
            double acc = 0.0;
            for (uint32_t c0 = 0; c0 < n; c0 += kClTile) {
                const uint32_t len = min(kClTile, n - c0);
                if (tid < len) {
                    const uint32_t jj = c0 + tid;
                    tp[0][tid] = pos[jj]; tp[1][tid] = pos[n + jj]; tp[2][tid] = pos[2u * n + jj];
                    tu[tid] = s[jj] * vj[jj];
                }
                __syncthreads();
                const uint32_t cw = (len + P - 1u) / P, cb = min(p * cw, len), ce = min(cb + cw, len);
                if (i < n) {
                    if (Wst)
                        for (uint32_t jj = cb; jj < ce; jj++) acc += (double)(Wst[(size_t)(c0 + jj) * n + i] * tu[jj]);
                    else
                        for (uint32_t jj = cb; jj < ce; jj++)
                            acc += (double)(cl_weight(px, py, pz, tp[0][jj], tp[1][jj], tp[2][jj], box, a.pbc, bad) * tu[jj]);
                }
                __syncthreads();
            }
            if (P > 1u) {
                part[tid] = acc;
                __syncthreads();
                if (p == 0u && i < n) {
                    double sum = 0.0;
                    for (uint32_t pp = 0; pp < P; pp++) sum += part[pp * rows_pad + r];
                    w[i] = s[i] * (float)sum;
                }
            } else if (i < n) {
                w[i] = s[i] * (float)acc;
            }
        }
        __syncthreads();
        // ---- full reorthogonalisation, classical Gram-Schmidt twice: against q and v_0 .. v_j; alpha_j = v_j . w
        double alpha = 0.0;
        for (int pass = 0; pass < 2; pass++) {
            for (int d = (int)wave; d <= j + 1; d += 16) {
                const float *b = d <= j ? V + (size_t)d * n : q;
                double sum = 0.0;
                for (uint32_t i = lane; i < n; i += 64u) sum += (double)b[i] * (double)w[i];
                sum = wave_sum_bfly(sum);
                if (lane == 0u) coef[d] = d <= j ? sum : sum / qn;
            }
            __syncthreads();
            alpha += coef[j];
            for (uint32_t i = tid; i < n; i += 1024u) {
                double sum = coef[j + 1] * (double)q[i];
                for (int d = 0; d <= j; d++) sum += coef[d] * (double)V[(size_t)d * n + i];
                w[i] = (float)((double)w[i] - sum);
            }
            __syncthreads();
        }
        double nn[1] = {0.0};
        for (uint32_t i = tid; i < n; i += 1024u) nn[0] += (double)w[i] * (double)w[i];
        block_sum_n<1>(nn, red);
        const double beta = sqrt(nn[0]);
        if (tid == 0) { al[j] = alpha; be[j] = beta; }
        m = j + 1;
        const bool breakdown = !(beta >= kClBreakdown);
        if (!breakdown) {
            const float inv = (float)(1.0 / beta);
            for (uint32_t i = tid; i < n; i += 1024u) w[i] *= inv;
        }
        __syncthreads();
        if (!(breakdown || m == m_max || m % kClCheckEvery == 0)) continue;
        // ---- the small problem: T's three largest eigenvalues by multisection of the Sturm count (256 points an
        // eigenvalue and round, five rounds), the two wanted eigenvectors by inverse iteration
        // The bracket is Gershgorin's for T (its off-diagonals are beta_0 .. beta_{m-2}), a little widened: no assumption on
        // the sign of S's eigenvalues (a minimum-image Gaussian kernel need not be positive semi-definite).
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
        // the second vector orthogonal to the first: with (nearly) equal Ritz values both solves return vectors of one
        // plane — different ones, their starts differ — and this makes them a basis of it
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
        done = breakdown || m == m_max || res < kClRitzTol;       // (every thread reads the same LDS values)
        __syncthreads();
    }
    if (bad) raise_box_range(a.err, f);
    // ---- hand the Ritz pairs on
    for (uint32_t k = tid; k < 2u * kClLd; k += 1024u) {
        const int which = (int)(k / kClLd), idx = (int)(k % kClLd);
        sol[k] = (which < m && idx < m) ? wk[which][4][idx] : 0.0;
    }
    if (tid < 3u) sol[2 * kClLd + tid] = (int)tid < m ? 0.5 * (s_lo[tid] + s_hi[tid]) : __builtin_nan("");
    if (tid == 3u) sol[2 * kClLd + 3] = (double)m;
}

__global__ __launch_bounds__(1024) void k_cluster_embed(ClArgs a) {
    __shared__ double y[2][kClLd];
    __shared__ double red[6 * 16];
    __shared__ float s_row[4];
    const uint32_t slot = blockIdx.x, tid = threadIdx.x, n = a.n;
    const double *sol = a.sol + (size_t)slot * kClSol;
    float *meta = a.meta + (size_t)slot * kClMeta;
    uint8_t *lab = a.lab + (size_t)slot * n;
    float *emb = a.emb + (size_t)slot * n;
    if (a.fail[slot]) {                                                         // (uniform)
        for (uint32_t i = tid; i < n; i += 1024u) { lab[i] = 0; emb[i] = 0.0f; }
        if (tid < kClMeta) meta[tid] = 0.0f;
        return;
    }
    const int m = (int)sol[2 * kClLd + 3];
    for (uint32_t k = tid; k < 2u * kClLd; k += 1024u) y[k / kClLd][k % kClLd] = sol[k];
    __syncthreads();
    const float *V = a.V + (size_t)slot * (a.m_max + 1u) * n;
    // ---- Ritz vectors V y; rows i = tid + 1024 k stay in registers
    float e0[8], e1[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t i = (uint32_t)k * 1024u + tid;
        e0[k] = e1[k] = 0.0f;
        if (i < n) {
            double s0 = 0.0, s1 = 0.0;
            for (int d = 0; d < m; d++) { const double v = (double)V[(size_t)d * n + i]; s0 += v * y[0][d]; s1 += v * y[1][d]; }
            e0[k] = (float)s0; e1[k] = (float)s1;
        }
    }
    // the sign of v2: row 0's coordinate is not negative
    if (tid == 0) s_row[0] = e0[0];
    __syncthreads();
    const float sgn = s_row[0] < 0.0f ? -1.0f : 1.0f;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t i = (uint32_t)k * 1024u + tid;
        if (i < n) {
            e0[k] *= sgn;
            const float nr = __builtin_sqrtf(e0[k] * e0[k] + e1[k] * e1[k]);
            if (nr > 1e-10f) { e0[k] /= nr; e1[k] /= nr; }
            emb[i] = e0[k];
        }
    }
    // ---- 2-means (clustering.rs:614-696): centroids = rows 0 and 1
    if (tid == 0) { s_row[0] = e0[0]; s_row[1] = e1[0]; }
    if (tid == 1u) { s_row[2] = e0[0]; s_row[3] = e1[0]; }
    __syncthreads();
    float c0x = s_row[0], c0y = s_row[1], c1x = s_row[2], c1y = s_row[3];
    const float r0x = c0x, r0y = c0y;
    uint32_t labels = 0, prev = 0xffffffffu;          // bit k: label of row k of this thread; prev: all "unset"
    bool first = true;
    int rounds = 0;
    double cnt[6] = {0, 0, 0, 0, 0, 0};
    for (int it = 0; it < 100; it++) {
        labels = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t i = (uint32_t)k * 1024u + tid;
            if (i < n) {
                float dx = e0[k] - c0x, dy = e1[k] - c0y;
                const float d0 = __builtin_sqrtf((0.0f + dx * dx) + dy * dy);
                dx = e0[k] - c1x; dy = e1[k] - c1y;
                const float d1 = __builtin_sqrtf((0.0f + dx * dx) + dy * dy);
                float mn = __builtin_inff();
                uint32_t best = 0;
                if (d0 < mn) { mn = d0; best = 0; }
                if (d1 < mn) { mn = d1; best = 1; }
                labels |= best << k;
            }
        }
        rounds++;
        double ch[1] = {(first || labels != prev) ? 1.0 : 0.0};
        block_sum_n<1>(ch, red);
        for (int k = 0; k < 6; k++) cnt[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t i = (uint32_t)k * 1024u + tid;
            if (i < n) {
                const int l = (labels >> k) & 1u;
                cnt[l] += 1.0; cnt[2 + 2 * l] += (double)e0[k]; cnt[3 + 2 * l] += (double)e1[k];
            }
        }
        block_sum_n<6>(cnt, red);
        if (ch[0] == 0.0) break;
        if (cnt[0] > 0.0) { c0x = (float)cnt[2] / (float)cnt[0]; c0y = (float)cnt[3] / (float)cnt[0]; } else { c0x = r0x; c0y = r0y; }
        if (cnt[1] > 0.0) { c1x = (float)cnt[4] / (float)cnt[1]; c1y = (float)cnt[5] / (float)cnt[1]; } else { c1x = r0x; c1y = r0y; }
        prev = labels;
        first = false;
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t i = (uint32_t)k * 1024u + tid;
        if (i < n) lab[i] = (uint8_t)((labels >> k) & 1u);
    }
    if (tid == 0) {
        meta[0] = (float)(1.0 - sol[2 * kClLd + 0]); meta[1] = (float)(1.0 - sol[2 * kClLd + 1]); meta[2] = (float)(1.0 - sol[2 * kClLd + 2]);
        meta[3] = (float)m; meta[4] = (float)rounds; meta[5] = (float)cnt[0]; meta[6] = (float)cnt[1]; meta[7] = 0.0f;
    }
}

__global__ __launch_bounds__(1024) void k_cluster_orient(ClOrientArgs a) {
    __shared__ double red[3 * 16];
    const uint32_t tid = threadIdx.x, n = a.n;
    for (uint32_t slot = 0; slot < a.n_assign; slot++) {
        const uint32_t f = a.aframes[slot];
        uint8_t *row = a.aflags + (size_t)(a.row0 + slot) * a.n_mol_total;
        const bool last = slot + 1u == a.n_assign;
        if (a.fail[slot]) {                                                     // (uniform)
            for (uint32_t mo = tid; mo < a.n_mol_total; mo += 1024u) row[mo] = 0;
            continue;
        }
        const uint8_t *lab = a.lab + (size_t)slot * n;
        const float *meta = a.meta + (size_t)slot * kClMeta;
        const bool ab_initio = a.is_frame0[slot] != 0;
        double c[3] = {0, 0, 0};            // |c1|, |c1 and previous upper|, |c1 and previous lower|
        for (uint32_t i = tid; i < n; i += 1024u) {
            if (lab[i] == 0) {
                c[0] += 1.0;
                if (!ab_initio) { if (a.carry[i] == 0) c[1] += 1.0; else c[2] += 1.0; }
            }
        }
        block_sum_n<3>(c, red);
        const float n1 = (float)c[0], n2 = (float)n - n1;
        float o_up = __builtin_nanf(""), o_lo = __builtin_nanf("");
        bool c1_upper;
        if (ab_initio) {
            c1_upper = n1 > n2 ? true : (n1 < n2 ? false : lab[0] == 0);
        } else {
            o_up = (float)c[1] / n1; o_lo = (float)c[2] / n1;
            if (o_up < 0.8f && o_lo < 0.8f && tid == 0) raise_error(a.err, GORDER_ERR_CLUSTER_MATCH, f, kStageSystem);
            c1_upper = !(o_up < o_lo);
        }
        __syncthreads();                    // every read of the old carry lies before its overwrite
        for (uint32_t i = tid; i < n; i += 1024u) a.carry[i] = (uint8_t)(((lab[i] == 0) == c1_upper) ? 0 : 1);
        __syncthreads();
        const float *emb = a.emb + (size_t)slot * n;
        for (uint32_t mo = tid; mo < a.n_mol_total; mo += 1024u) {
            const uint32_t hs = a.head_slot[mo];
            row[mo] = (uint8_t)(a.carry[hs] ^ (a.flip ? 1 : 0));
            if (last && a.adist) a.adist[mo] = emb[hs];
        }
        if (last && a.stats && tid == 0) {
            float *o = a.stats;
            o[0] = meta[0]; o[1] = meta[1]; o[2] = meta[2]; o[3] = meta[3]; o[4] = meta[4];
            o[5] = n1; o[6] = n2; o[7] = c1_upper ? n1 : n2; o[8] = c1_upper ? n2 : n1;
            o[9] = o_up; o[10] = o_lo; o[11] = 0.0f;
        }
    }
}

}  // namespace
