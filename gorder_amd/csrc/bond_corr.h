// bond_corr.h — bond reorientation: the check of the lags, the arithmetic of the ring of frame planes, the frames a
// workgroup of k_bond_corr walks, and the pair count of a lag (gorder_hip_set_bond_correlation, kernels_corr.h).
// No HIP: the setter, the submit path and tests/cabi/bond_corr.cpp share this one definition.
#ifndef GORDER_BOND_CORR_H
#define GORDER_BOND_CORR_H
#include <stddef.h>
#include <stdint.h>
#include <algorithm>

namespace gorder {
constexpr uint32_t kCorrMaxLags = 64;       // GORDER_CORR_MAX_LAGS
constexpr uint32_t kCorrMaxLag = 4096;      // GORDER_CORR_MAX_LAG
constexpr uint32_t kCorrLagBlock = 8;       // LB: the lags one pass of k_bond_corr keeps in registers
constexpr uint32_t kCorrNoLag = 0xffffffffu;    // pads the last group of a lag list: no frame has that much history
constexpr uint32_t kCorrChunkMax = 2048;    // frames a workgroup of k_bond_corr sums in i32
constexpr uint32_t kCorrChunkMin = 64;      // ... and the fewest it takes where the range has them: the fold is paid per chunk
constexpr uint32_t kCorrMinSubrange = 64;   // the ring has room for this many frames of a batch at once where the budget allows
constexpr uint64_t kCorrRingBudget = (uint64_t)2 << 30;     // bytes of the ring, at most

// null, or why the lags are refused: 1..kCorrMaxLags strictly ascending values, none above kCorrMaxLag (0 is a lag)
inline const char *corr_lags_check(const uint32_t *lags, uint32_t n_lags) {
    if (n_lags == 0) return "no lags";
    if (n_lags > kCorrMaxLags) return "more than GORDER_CORR_MAX_LAGS lags";
    if (!lags) return "no lags";
    for (uint32_t k = 0; k < n_lags; k++) {
        if (k && !(lags[k] > lags[k - 1])) return "the lags are not strictly ascending";
        if (lags[k] > kCorrMaxLag) return "a lag above GORDER_CORR_MAX_LAG";
    }
    return nullptr;
}

// ---- the ring: R = max_lag + S planes, the plane of analysed frame g (counted from the handle's first frame) is g mod R.
// While the S frames [g, g + S) of a sub-range are written and read, the oldest frame still needed is g - max_lag: the
// max_lag + S frames [g - max_lag, g + S) are consecutive, so their planes are distinct.
inline uint64_t corr_plane_bytes(uint64_t n_tiles, uint32_t block) { return n_tiles * block * 16u; }      // float4 per item, tiles padded
inline uint32_t corr_ring_planes(uint32_t max_lag, uint32_t subrange) { return max_lag + subrange; }
inline uint32_t corr_plane_of(uint64_t frame, uint32_t ring_planes) { return (uint32_t)(frame % ring_planes); }
// the largest sub-range whose ring stays inside `budget` bytes; 0: not even one frame fits (the setter refuses)
inline uint64_t corr_subrange_fit(uint64_t plane_bytes, uint32_t max_lag, uint64_t budget) {
    const uint64_t planes = plane_bytes ? budget / plane_bytes : 0;
    return planes > max_lag ? planes - max_lag : 0;
}
// the sub-range of a handle, fixed when the ring is allocated (the first batch): what fits, capped by that batch's length
// but not below kCorrMinSubrange (later batches may be longer), and by `forced` (GORDER_HIP_CORR_SUBRANGE; 0: not set)
inline uint32_t corr_subrange(uint64_t fit, uint32_t batch_frames, uint32_t forced) {
    uint64_t s = std::min<uint64_t>(fit, std::max(batch_frames, kCorrMinSubrange));
    if (forced) s = std::min<uint64_t>(s, forced);
    return (uint32_t)std::max<uint64_t>(s, 1);
}

// frames per workgroup of k_bond_corr over a sub-range of n_frames: about 8 co-resident rounds of workgroups, but no chunk
// shorter than kCorrChunkMin (the fold behind every group of lags is paid per chunk) or longer than kCorrChunkMax (i32 sums)
struct CorrChunks { uint32_t frames_per_chunk, n_chunks; };
inline CorrChunks corr_chunks(uint32_t n_frames, uint32_t n_tiles, uint32_t wg_target, uint32_t wg_capacity) {
    const uint32_t want = std::min(std::max(1u, (wg_target ? wg_target : 8u * wg_capacity) / std::max(1u, n_tiles)), std::max(1u, n_frames));
    uint32_t fpc = (n_frames + want - 1) / want;
    fpc = std::min(std::min(std::max(fpc, kCorrChunkMin), kCorrChunkMax), std::max(1u, n_frames));
    return {fpc, (n_frames + fpc - 1) / fpc};
}

// pairs a slot with `samples` bond samples a frame has booked for `lag` after `frames` analysed frames
inline uint64_t corr_pair_count(uint64_t frames, uint32_t lag, uint64_t samples) { return frames > lag ? (frames - lag) * samples : 0; }
}  // namespace gorder
#endif
