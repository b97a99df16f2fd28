// kernels_replay.h — manual leaflets and manual membrane normals replayed from whole-trajectory tables that stay on the
// device in packed form (gorder_hip_set_manual_leaflet_table / _normal_table; host logic: replay_rows.h).  Both kernels
// run on the handle's stream ahead of the order kernels and only unpack what those consume: a byte per molecule of every
// assignment row the batch opens, a float4 per (frame, molecule).  They move a few bytes per molecule and are not tuned
// beyond coalescing: no LDS, no atomics, plain vector loads and stores.
#pragma once

// Table rows `rows[r]` (bit (m & 63) of word (m >> 6) = molecule m's flag, Upper = 0 / Lower = 1 before `flip`) ->
// out [n_expand][n_mol] bytes, the layout the order kernels route by.  A wave owns one 64-molecule word of one expanded
// row: the word is read at a wave-uniform address, every lane takes its bit and stores its byte (64 consecutive bytes a
// wave).  Lanes past n_mol store nothing.
__global__ __launch_bounds__(256) void k_replay_flags(const unsigned long long *__restrict__ table, const uint32_t *__restrict__ rows,
                                                      uint32_t n_expand, uint32_t words_per_row, uint32_t n_mol, uint32_t flip,
                                                      uint8_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long w = (unsigned long long)blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= (unsigned long long)n_expand * words_per_row) return;
    const uint32_t r = (uint32_t)(w / words_per_row), k = (uint32_t)(w % words_per_row);
    const unsigned long long word = table[(size_t)rows[r] * words_per_row + k];
    const uint32_t m = k * 64u + lane;
    if (m < n_mol) out[(size_t)r * n_mol + m] = (uint8_t)(((word >> lane) & 1u) ^ (flip & 1u));
}

struct ReplayVec3 { float x, y, z; };

// Table rows of three floats a molecule -> dyn [n_frames][n_mol] (x, y, z, 3.0f): the layout k_bonds_extras and k_ua_extras
// consume as "a computed normal with enough points" (any length: calc_sch normalises).  A thread per (frame, molecule);
// frame f reads table row row_of_frame[f].  A wave loads 768 and stores 1 024 consecutive bytes.
__global__ __launch_bounds__(256) void k_replay_normals(const ReplayVec3 *__restrict__ table, const uint32_t *__restrict__ row_of_frame,
                                                        uint32_t n_mol, unsigned long long n, float4 *__restrict__ dyn) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = (uint32_t)(i / n_mol), m = (uint32_t)(i % n_mol);
    const ReplayVec3 v = table[(size_t)row_of_frame[f] * n_mol + m];
    dyn[i] = make_float4(v.x, v.y, v.z, 3.0f);
}
