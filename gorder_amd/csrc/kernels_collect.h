// kernels_collect.h — the per-frame history a host may collect (gorder_hip_set_collect): every assignment frame's leaflet
// flags, bit-packed, and every analysed frame's dynamic membrane normals, three floats a molecule.  Both kernels only
// repack what the batch's kernels left on the device into a staging block that one stream-ordered copy then moves to
// the host (collect_store.h); they move a few bytes per molecule and frame and are not tuned beyond coalescing.
#pragma once

// `n_rows` rows of d_aflags -> words [n_rows][words_per_row], bit (m & 63) of word (m >> 6) = molecule m's flag.
// A wave owns the 64 molecules of one word: every lane reads its molecule's byte (64 consecutive bytes), the word is the
// wave's ballot and lane 0 stores it.  Lanes past the row's end vote 0, so the last word's high bits are 0.
__global__ __launch_bounds__(256) void k_collect_flags(const uint8_t *__restrict__ aflags, uint32_t n_mol, uint32_t n_rows,
                                                       uint32_t words_per_row, unsigned long long *__restrict__ words) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long w = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);     // wave-uniform
    if (w >= (unsigned long long)n_rows * words_per_row) return;
    const uint32_t row = (uint32_t)(w / words_per_row);
    const uint32_t m = (uint32_t)(w % words_per_row) * 64u + lane;
    const bool flag = m < n_mol && aflags[(size_t)row * n_mol + m] != 0;
    const unsigned long long word = __ballot(flag);
    if (lane == 0u) words[w] = word;
}

struct CollectVec3 { float x, y, z; };

// d_dyn_normals (nx, ny, nz, cloud size) [n] -> three packed floats per (frame, molecule); NaN where `touched` is given
// and 0: no bond of that molecule passed the geometry test in that frame, so the reference never fetched its normal
// (bond.rs:424-431).  A thread per (frame, molecule): lane i stores the 12 bytes at 12 i, a wave 768 consecutive bytes.
__global__ __launch_bounds__(256) void k_collect_normals(const float4 *__restrict__ dyn, const uint8_t *__restrict__ touched,
                                                         unsigned long long n, CollectVec3 *__restrict__ out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 v = dyn[i];
    CollectVec3 o{v.x, v.y, v.z};
    if (touched && !touched[i]) o.x = o.y = o.z = __builtin_nanf("");
    out[i] = o;
}
