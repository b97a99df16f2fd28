// kernels_ordermap.h — ordermaps finished where they lie: the tiles of a group of accumulator slots added and turned into the
// values the reference writes (ResultsConverter::convert_ordermap, converter.rs:226-256; host arithmetic: ordermap_final.h).
//
// The raw maps are map_sums / map_cnts [3][n_acc][nx * ny] words of 64 bits (i64 tick sums, u64 sample counts; k_fold_maps,
// kernels_common.h).  A group is a list of slots in CSR form — a bond, a heavy atom's bonds, a molecule type, the system —
// and its map the tile-wise sum of its members' maps: exact integer addition, then om_tile_value once per tile.  Nothing
// depends on the launch geometry.  A slot that is a member of four groups is read four times; the rows are read once each
// per membership, coalesced, and nothing but the floats is written.
//
// gfx950 only.  All offsets into the maps are 64-bit.
#pragma once

typedef unsigned long long om_u64;

// Workgroup b: (group, plane) = b / tile_blocks, the tiles [(b % tile_blocks) * 256, + 256): consecutive lanes take
// consecutive tiles of every member's row, 8 bytes a lane.  The member list is uniform over the workgroup.
// planes: 3 with leaflets; 1 without — the upper and lower planes of the output are then NaN and their rows are not read.
// out [n_groups][3][n_tiles].
__global__ __launch_bounds__(256) void k_map_finalise(const om_u64 *__restrict__ map_sums, const om_u64 *__restrict__ map_cnts,
                                                      uint32_t n_acc, om_u64 n_tiles, uint32_t tile_blocks, uint32_t planes,
                                                      const uint32_t *__restrict__ group_begin, const uint32_t *__restrict__ slots,
                                                      uint32_t min_samples, int negate, float *__restrict__ out) {
    const uint32_t gw = blockIdx.x / tile_blocks;                   // group * 3 + plane
    const uint32_t g = gw / 3u, w = gw % 3u;
    const om_u64 t = (om_u64)(blockIdx.x % tile_blocks) * 256u + threadIdx.x;
    if (t >= n_tiles) return;
    float v = __builtin_nanf("");
    if (w < planes) {
        const om_u64 plane = (om_u64)w * n_acc;
        om_u64 s = 0, c = 0;
        for (uint32_t m = group_begin[g], m1 = group_begin[g + 1]; m < m1; m++) {
            const om_u64 at = (plane + slots[m]) * n_tiles + t;
            s += map_sums[at];
            c += map_cnts[at];
        }
        v = gorder::om_tile_value(s, c, min_samples, negate != 0);
    }
    out[(om_u64)gw * n_tiles + t] = v;
}
