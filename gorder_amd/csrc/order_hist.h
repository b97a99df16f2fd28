// order_hist.h — order distributions: the bin of a sample's tick among ascending integer edges, and the check of the edges
// (gorder_hip_set_order_histogram, k_bonds_dist).  No HIP: the kernel, the setter and tests/cabi/order_hist.cpp
// share this one definition.
#ifndef GORDER_ORDER_HIST_H
#define GORDER_ORDER_HIST_H
#include <stdint.h>

#if defined(__HIPCC__)
#define GORDER_HIST_HD __host__ __device__
#else
#define GORDER_HIST_HD
#endif

namespace gorder {
constexpr uint32_t kHistMaxBins = 256;      // GORDER_HIST_MAX_BINS

// Bin k is edges[k] <= tick < edges[k + 1]; -1 below edges[0] and at or above edges[n_edges - 1].  edges: n_edges >= 2
// strictly ascending values (hist_edges_check).  A binary search without a data-dependent branch: `pos` ends as the number
// of edges at or below the tick, after floor(log2(n_edges)) + 1 steps whatever the tick, and no step reads past the edges.
GORDER_HIST_HD inline int hist_bin(const int32_t *edges, uint32_t n_edges, int32_t tick) {
    uint32_t step = 1;
    while (step * 2u <= n_edges) step *= 2u;        // (uniform: the same for every sample of a launch)
    uint32_t pos = 0;
    for (; step; step >>= 1) {
        const uint32_t q = pos + step;
        const uint32_t at = (q <= n_edges ? q : n_edges) - 1u;
        pos = (q <= n_edges && edges[at] <= tick) ? q : pos;
    }
    return (pos == 0 || pos == n_edges) ? -1 : (int)pos - 1;
}

// null, or why the edges are refused
inline const char *hist_edges_check(const int32_t *edges, uint32_t n_edges) {
    if (n_edges < 2) return "fewer than 2 edges";
    if (n_edges > kHistMaxBins + 1u) return "more than GORDER_HIST_MAX_BINS + 1 edges";
    if (!edges) return "no edges";
    for (uint32_t k = 1; k < n_edges; k++)
        if (!(edges[k] > edges[k - 1])) return "the edges are not strictly ascending";
    return nullptr;
}
}  // namespace gorder
#endif
