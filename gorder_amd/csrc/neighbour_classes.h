// neighbour_classes.h — order by local composition: the argument check of gorder_hip_set_neighbour_classes, the pieces in
// which k_neighbour_counts stages the neighbour atoms, whether k_bonds_classes' LDS table fits, and the frame sub-range of
// the class rows.  No HIP calls: the setter (the check, the table), the launch code (the sub-range), the kernel
// (the pieces) and tests/cabi/neighbour_classes.cpp share this one definition.
#ifndef GORDER_NEIGHBOUR_CLASSES_H
#define GORDER_NEIGHBOUR_CLASSES_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GORDER_NB_HD __host__ __device__
#else
#define GORDER_NB_HD
#endif

namespace gorder {
constexpr uint32_t kNeighbourMaxAtoms = 16384;      // GORDER_NEIGHBOUR_MAX_ATOMS
constexpr uint32_t kNeighbourMaxClasses = 32;       // GORDER_NEIGHBOUR_MAX_CLASSES
constexpr uint32_t kNeighbourPiece = 1024;          // neighbour atoms a workgroup of k_neighbour_counts holds in LDS at a time (float4: 16 KB)
constexpr uint64_t kClassRowBytes = (uint64_t)1 << 30;      // the class bytes [frames][n_mol_total] of one sub-range, at most
constexpr uint32_t kClassTableBytes = 64u * 1024u;          // LDS a workgroup of k_bonds_classes may take for its table
constexpr uint32_t kClassGridRows = 65535;                  // rows of gridDim.y: frames of one launch of k_neighbour_counts, at most

// null, or why the arguments are refused (n_neighbours > 0: the feature is being switched on)
inline const char *neighbour_args_check(const uint32_t *centres, uint32_t n_mol_total, const uint32_t *neighbours, uint32_t n_neighbours,
                                        float radius, uint32_t n_classes, uint32_t n_atoms) {
    if (n_neighbours > kNeighbourMaxAtoms) return "more than GORDER_NEIGHBOUR_MAX_ATOMS neighbours";
    if (n_classes < 2) return "fewer than 2 classes";
    if (n_classes > kNeighbourMaxClasses) return "more than GORDER_NEIGHBOUR_MAX_CLASSES classes";
    if (!isfinite(radius) || !(radius > 0.0f)) return "the radius is not finite and > 0";
    if (!centres || !neighbours) return "no centres or no neighbours";
    for (uint32_t m = 0; m < n_mol_total; m++)
        if (centres[m] >= n_atoms) return "a centre index >= n_atoms";
    for (uint32_t q = 0; q < n_neighbours; q++) {
        if (neighbours[q] >= n_atoms) return "a neighbour index >= n_atoms";
        if (q && !(neighbours[q] > neighbours[q - 1])) return "the neighbours are not strictly ascending";
    }
    return nullptr;
}

// the pieces of n neighbour atoms: piece k holds the atoms [k * kNeighbourPiece, k * kNeighbourPiece + neighbour_piece_len(n, k))
// (k_neighbour_counts walks exactly these)
GORDER_NB_HD inline uint32_t neighbour_pieces(uint32_t n) { return (n + kNeighbourPiece - 1u) / kNeighbourPiece; }
GORDER_NB_HD inline uint32_t neighbour_piece_len(uint32_t n, uint32_t k) {
    const uint64_t begin = (uint64_t)k * kNeighbourPiece;
    return begin >= n ? 0u : (uint32_t)(n - begin < kNeighbourPiece ? n - begin : kNeighbourPiece);
}

// bytes of k_bonds_classes' table [planes][n_classes][slots of the widest tile] of packed 64-bit words, and whether a
// workgroup can hold it; where it cannot, the kernel's direct route books every sample with global atomics
inline uint64_t class_table_bytes(uint32_t planes, uint32_t n_classes, uint32_t max_tile_slots) {
    return (uint64_t)planes * n_classes * max_tile_slots * 8u;
}
inline bool class_table_fits(uint32_t planes, uint32_t n_classes, uint32_t max_tile_slots) {
    return class_table_bytes(planes, n_classes, max_tile_slots) <= kClassTableBytes;
}

// whether the class rows hold a whole batch (gorder_hip_neighbour_class_rows then returns it), or one sub-range at a time
inline bool class_rows_whole(uint32_t n_frames, uint32_t n_mol_total, uint64_t row_bytes = kClassRowBytes) {
    return (uint64_t)n_frames * n_mol_total <= row_bytes;
}

// frames of one sub-range of a batch: one launch of k_neighbour_counts (a frame per row of gridDim.y: kClassGridRows at
// most) whose class rows fit (a byte per frame and molecule, row_bytes at most — unless the rows hold the whole batch), at
// least one frame, a forced length (GORDER_HIP_NB_SUBRANGE, 0 = not set) where that is shorter
inline uint32_t class_subrange(uint32_t n_frames, uint32_t n_mol_total, uint32_t forced, uint64_t row_bytes = kClassRowBytes) {
    uint64_t sub = class_rows_whole(n_frames, n_mol_total, row_bytes) ? n_frames : row_bytes / (n_mol_total ? n_mol_total : 1u);
    if (sub < 1) sub = 1;
    if (sub > kClassGridRows) sub = kClassGridRows;
    if (forced && forced < sub) sub = forced;
    if (sub > n_frames) sub = n_frames;
    return (uint32_t)(sub ? sub : 1u);
}
}  // namespace gorder
#endif
