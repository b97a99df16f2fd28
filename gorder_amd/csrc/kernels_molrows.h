// kernels_molrows.h — k_bonds_tiled_mol: the order pass with every molecule's own sums as a second output
// (gorder_hip_set_molecule_rows; molecule_rows.h has the lane order and the layout).  Part of the single translation unit
// gorder_hip.hip, behind kernels_extras.h; device code for gfx950 only.
#pragma once

namespace {

static_assert(kMapOne == 1ull << gorder::kMolRowsCountShift, "molecule_rows.h unpacks the ordermaps' packed word");
// a (frame, group, molecule) word receives one sample per slot of the group: far below what the word holds, and the sum fits int32
static_assert(gorder::kMolRowsMaxGroupSlots < kMapFoldLimit && (unsigned long long)gorder::kMolRowsMaxGroupSlots * 1000000ull < (1ull << 31),
              "group size limit of the molecule rows against the packed word and the int32 sums");

struct MolRowArgs {
    const gorder::MolRun *runs;         // tile by tile (MolRows::runs)
    const uint32_t *run_begin;          // [n_tiles + 1]
    unsigned long long *stage;          // [frames of the sub-range][n_groups][n_mol_total] packed words, zeroed ahead of the launch
    uint32_t words_per_frame;           // n_groups * n_mol_total
};

constexpr uint32_t kMolPad = kBlock + kBlock / 32u;      // a lane's word sits at lane + lane / 32: runs of 32 lanes start in different banks
__device__ __forceinline__ uint32_t mol_pad(uint32_t lane) { return lane + (lane >> 5); }

// ---- per-molecule rows, bonds: k_bonds_tiled_tw's structure (K1's staging, the stage's ticks as a second output) without
// MAPS and MOM.  The tile's items come in (group, molecule) order, so the samples of one molecule in one group are
// neighbouring lanes: a lane leaves its packed word (kMapOne + tick; 0: no sample) of each frame of the stage in LDS before
// the barrier that ends the stage, and behind it a thread per (run of the tile, frame of the stage) adds its run up and
// sends ONE 64-bit atomic to the staging word of (frame, group, molecule).  No LDS atomics.  Thread w of a pass takes
// run w % n_runs of frame w / n_runs: the lanes of a wave hold consecutive runs of ONE frame, and a tile's runs ascend in
// (group, molecule), so a wave's atomics go to neighbouring 8-byte words.
// The ordinary sums leave through the same epilogue as k_bonds_tiled's, into the same replicas.
// grid = n_tiles * n_chunks (frames_per_chunk a multiple of kRecFrames, a.frame0 = the sub-range's first frame);
// items = MolRows::items.
template <int NPF, bool ACOS_COS, bool PBC, bool LEAF, int AXIS>
__global__ __launch_bounds__(kBlock, 4) void k_bonds_tiled_mol(FrameArgs a_in, MolRowArgs mr, const float *__restrict__ xyz,
                                                              const float *__restrict__ box9, const uint8_t *__restrict__ aflags,
                                                              const uint32_t *__restrict__ arow, const Tile *__restrict__ tiles,
                                                              const Item *__restrict__ items, const uint32_t *__restrict__ tile_slots,
                                                              uint32_t n_tiles, uint32_t lw) {
    constexpr int G = (int)kRecFrames;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ unsigned long long l_word[kRecFrames][kMolPad];
    __shared__ uint2 l_run[kBlock];                     // the tile's runs: ((lane0 << 16) | n, word)
    using S = TiledStage<G, NPF, ACOS_COS, PBC, LEAF, AXIS>;
    FrameArgs a = a_in;
    a.xyz = xyz; a.box9 = box9; a.aflags = aflags; a.arow = arow;
    const TileCtx tc = tile_prologue(tiles, items, n_tiles, a.frame0, a.frames_per_chunk, a.n_frames);
    const auto &[t, it, tile_id, chunk, tid, active, f_begin, f_end] = tc;
    const uint32_t sk = tid / S::TPF, si = tid % S::TPF;
    const uint32_t run0 = mr.run_begin[tile_id], n_runs = mr.run_begin[tile_id + 1u] - run0;    // (<= n_items <= kBlock)
    if (tid < n_runs) {
        const gorder::MolRun r = mr.runs[run0 + tid];
        l_run[tid] = make_uint2(((uint32_t)r.lane0 << 16) | (uint32_t)r.n, r.word);
    }
    unsigned long long words[kRecFrames];
    TiledMapOut mo{};
    mo.nx = 0;                      // ticks only: word = (lower << 32) | tick
    mo.words = words;
    SampleAcc acc;
    int bad = 0;
    uint32_t nan_which = 0, nan_frame = kNoNan;
    v4f pre[NPF];
    if (f_begin + G <= f_end) S::template load<false>(a, t, f_begin, f_end, sk, si, pre);
    for (uint32_t fs = f_begin; fs < f_end; fs += G) {
        const bool full = fs + G <= f_end;
        if (full) {
            S::template store<false>(a, t, fs, f_end, sk, si, pre, lds, lw);
        } else {
            S::template load<true>(a, t, fs, f_end, sk, si, pre);
            S::template store<true>(a, t, fs, f_end, sk, si, pre, lds, lw);
        }
        __syncthreads();
        if (full && fs + 2u * G <= f_end) S::template load<false>(a, t, fs + G, f_end, sk, si, pre);     // next stage in flight
#pragma unroll
        for (uint32_t k = 0; k < kRecFrames; k++) words[k] = kMapNoSample;
        if (active) {
            if (full) S::template compute<2>(a, t, it, fs, lds, lw, acc, bad, nan_which, nan_frame, &mo);
            else S::template compute_tail<2>(a, t, it, fs, f_end, lds, lw, acc, bad, nan_which, nan_frame, &mo);
        }
#pragma unroll
        for (uint32_t k = 0; k < kRecFrames; k++)
            l_word[k][mol_pad(tid)] = words[k] == kMapNoSample ? 0ull : kMapOne + (unsigned long long)(long long)(int)(uint32_t)words[k];
        __syncthreads();
        // a thread per (run of the tile, frame of the stage); the next stage's staging goes on meanwhile (other LDS), and its
        // words are written behind its own barrier
        for (uint32_t w = tid; w < kRecFrames * n_runs; w += kBlock) {
            const uint32_t k = w / n_runs, r = w - k * n_runs;
            if (fs + k >= f_end) break;                          // (k only grows with w)
            const uint2 run = l_run[r];
            const uint32_t lane0 = run.x >> 16, n = run.x & 0xffffu;
            unsigned long long s = 0;
            for (uint32_t j = 0; j < n; j++) s += l_word[k][mol_pad(lane0 + j)];
            if (s) atomicAdd(&mr.stage[(size_t)(fs + k - a.frame0) * mr.words_per_frame + run.y], s);
        }
    }
    // the head of the staging LDS: its last reads, the last stage's samples, ended at that stage's second barrier (the run
    // sums behind it read other LDS); this barrier is kept so that the kernel's code stays what it was
    __syncthreads();
    raise_tile_errors(a.err, tc, tile_slots, nan_which, nan_frame, bad);
    fold_tile_sums(a.rep, a.n_rep, a.n_acc, tc, acc, lds, [&] { return tile_slots[tc.t.slot0 + tc.tid]; });
}

}  // namespace
