// ordermap_final.h — what turns an ordermap tile's raw (tick sum, sample count) into the value the reference writes
// (ResultsConverter::convert_ordermap, converter.rs:226-256; From<OrderValue> for f32, order.rs:28-32; OrderType::convert,
// presentation/mod.rs:618-690), and the validation of the groups of accumulator slots whose tiles are added before that.
// k_map_finalise (kernels_ordermap.h) and the host side call the same functions, and there is no HIP call in here, so
// tests/cabi/ordermap_final.cpp can drive all of it without a device.
//
// The sequence is NOT AnalysisOrder::calc_order's (order.rs:101-107, tw_mean in kernels_timewise.h), which divides the i64
// sum by the count and truncates before it leaves the integers.  A map converts the sum to f32 first and divides two
// floats: the two differ by under one tick of 1e-6.
#ifndef GORDER_ORDERMAP_FINAL_H
#define GORDER_ORDERMAP_FINAL_H

#include <stddef.h>
#include <stdint.h>

#include "timewise_blocks.h"

#if defined(__HIPCC__)
#define GORDER_OM_HD __host__ __device__ inline
#else
#define GORDER_OM_HD inline
#endif

namespace gorder {

// One tile: `sum` the i64 tick sum as its 64-bit word, `count` the samples.  Every step is one IEEE operation, in this
// order; the file that includes this is compiled with contraction off and correctly rounded f32 division (Makefile).
GORDER_OM_HD float om_tile_value(uint64_t sum, uint64_t count, uint32_t min_samples, bool negate) {
    if (count < (uint64_t)min_samples) return __builtin_nanf("");
    float v = (float)((double)(int64_t)sum / 1e6);      // From<OrderValue> for f32
    v = v / (float)count;                               // `samples as f32`: rounds above 2^24
    return negate ? -v : v;                             // AAOrder / UAOrder::convert: a zero sum gives -0.0
}

// The groups come in the CSR form of the error estimates (timewise_blocks.h); a map has nothing to add to those rules.
// min_samples == 0 would let a tile without samples through to 0 / 0.
enum OmStatus { kOmOk = 0, kOmMinSamples = 1, kOmGroups = 2 };

// *groups: what tw_check_groups found (kTwGroupsOk unless kOmGroups is returned); *bad: as there
inline OmStatus om_check(const uint32_t *group_begin, const uint32_t *slots, uint32_t n_groups, uint32_t n_acc, uint32_t min_samples,
                         TwGroupStatus *groups, uint32_t *bad) {
    if (groups) *groups = kTwGroupsOk;
    if (min_samples == 0) return kOmMinSamples;
    const TwGroupStatus gs = tw_check_groups(group_begin, slots, n_groups, n_acc, bad);
    if (groups) *groups = gs;
    return gs == kTwGroupsOk ? kOmOk : kOmGroups;
}

// words of one of the two raw arrays [3][n_acc][nx * ny]; 0 if that does not fit 64 bits
inline uint64_t om_map_words(uint32_t n_acc, uint32_t nx, uint32_t ny) {
    const uint64_t tiles = (uint64_t)nx * ny;
    if (tiles == 0 || n_acc == 0) return 0;
    if (tiles > (~(uint64_t)0 / 3u) / n_acc) return 0;
    return 3u * (uint64_t)n_acc * tiles;
}

}  // namespace gorder

#endif
