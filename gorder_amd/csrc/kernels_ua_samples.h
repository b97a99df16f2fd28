// kernels_ua_samples.h — united-atom tiles with every virtual C-H sample booked a second time (GORDER_FLAG_UA_SAMPLES):
// k_ua_dist, the order histogram (gorder_hip_set_order_histogram), and k_ua_mol, the per-molecule rows
// (gorder_hip_set_molecule_rows; ua_molecule_rows.h has the tables).  Part of the single translation unit
// gorder_hip.hip, behind kernels_ua.h and kernels_hist.h (DistArgs); device code for gfx950 only.
//
// Both are k_ua_extras' exact path through the shared pieces of kernels_ua.h — ua_tile_work, ua_tile_lane, ua_fetch,
// ua_raise_undefined, ua_carbon_exact, ua_tick, ua_fold_sums — with a second output, which is all this file holds.
// gorder_hip_finish of a handle with either feature returns what it returns without.
#pragma once

namespace {

struct UaMolArgs {
    const uint32_t *word_begin;             // [n_ua_tiles + 1] (UaMolRows::word_begin)
    const uint32_t *words;                  // the tiles' word lists: group * n_mol_total + molecule
    const gorder::UaLaneWords *lane_words;  // per item: the local word of each hydrogen, kUaMolNoWord: none
    unsigned long long *stage;              // [frames of the sub-range][n_groups][n_mol_total] packed words (MolRowArgs::stage)
    uint32_t words_per_frame;
    uint32_t list_bytes;                    // ua_mol_list_bytes(max_local): where the word buffers begin in the dynamic LDS
    uint32_t n_buf;                         // ua_mol_buffers(max_local)
};

// MOL = false: k_ua_dist.  Dynamic LDS: the edges (kDistEdgeBytes), then the table u32 [planes][n bins][t.n_slots] — local
// slot it.lslot0 + k the minor index — whose place serves the epilogue's sums once it has been sent out (DIRECT: from the
// start).  A geometry selection is tested on the bond position as MODE 2 of k_ua_extras does: a sample outside is in no
// sum and in no bin.
// MOL = true: k_ua_mol.  Static LDS: the epilogue's sums.  Dynamic: the tile's word list, then n_buf buffers
// u64 [kUaMolStage][n_local]: a lane adds (1 << 42) + tick per hydrogen into the word of (frame of the stage, local word)
// — a 64-bit LDS add without a return value —, and behind the stage's barrier a thread per (frame, local word) sends ONE
// global atomic for each non-zero word and zeroes it.  Two buffers alternate, so the next stage's adds need no second
// barrier (the buffer they go to was zeroed before the barrier of the stage in between); with one buffer a second
// barrier ends the stage.  The frame loop is not unrolled over the stage: no per-frame register arrays, no scratch from it.
template <bool ACOS_COS, bool MOL, bool DIRECT>
__device__ __forceinline__ void ua_samples_body(FrameArgs a_in, ExtraArgs e, DistArgs s, UaMolArgs m, GORDER_UA_KERNEL_ARGS, unsigned char *l_dyn,
                                                unsigned long long *l_s, uint32_t *l_n) {
    constexpr uint32_t LS = kUaLS, G = gorder::kUaMolStage;
    FrameArgs a = a_in;
    a.xyz = xyz; a.box9 = box9; a.aflags = aflags; a.arow = arow;
    const UaWork wk = ua_tile_work(n_tiles, a_in.frame0, a_in.frames_per_chunk, a_in.n_frames);
    if (wk.padding) return;
    const UaLane tc = ua_tile_lane(tiles, items, tile_slots, wk.tile_id);
    const Tile t = tc.t;
    const gorder::UaItem it = tc.it;
    const uint32_t tile_id = wk.tile_id, tid = tc.tid, gslot0 = tc.gslot0, f_begin = wk.f_begin, f_end = wk.f_end;
    const bool active = tc.active;
    const size_t fstride = (size_t)a.n_atoms * 3u;
    // ---- the second output's LDS
    int32_t *const l_edges = reinterpret_cast<int32_t *>(l_dyn);
    uint32_t *const l_tab = reinterpret_cast<uint32_t *>(l_dyn + kDistEdgeBytes);
    const uint32_t planes = a.leaflets ? 2u : 1u, ns = t.n_slots, n_bins = MOL ? 0u : s.n_edges - 1u;
    uint32_t *const l_wid = reinterpret_cast<uint32_t *>(l_dyn);
    unsigned long long *const l_word = reinterpret_cast<unsigned long long *>(l_dyn + (MOL ? m.list_bytes : 0u));
    uint32_t word0 = 0, n_loc = 0;
    gorder::UaLaneWords lw{{gorder::kUaMolNoWord, gorder::kUaMolNoWord, gorder::kUaMolNoWord, gorder::kUaMolNoWord}};
    if (MOL) {
        word0 = m.word_begin[tile_id];
        n_loc = m.word_begin[tile_id + 1u] - word0;
        if (active) lw = m.lane_words[t.item0 + tid];
        for (uint32_t k = tid; k < n_loc; k += kBlock) l_wid[k] = m.words[word0 + k];
        for (uint32_t k = tid; k < m.n_buf * G * n_loc; k += kBlock) l_word[k] = 0ull;
    } else {
        for (uint32_t k = tid; k < s.n_edges; k += kBlock) l_edges[k] = s.edges[k];
        if (!DIRECT)
            for (uint32_t k = tid; k < planes * n_bins * ns; k += kBlock) l_tab[k] = 0;
    }
    if (MOL || DIRECT)
        for (uint32_t k = tid; k < 2 * LS; k += kBlock) { l_s[k] = 0; l_n[k] = 0; }
    __syncthreads();
    unsigned long long *const dist_rep = MOL ? nullptr : s.rep + (size_t)(blockIdx.x % s.n_rep) * n_bins * 2u * a.n_acc;
    UaAcc acc;
    int bad = 0;
    const bool pbc = a.pbc != 0;
    const UaConsts uc{e.sin_tet, e.cos_tet, e.sin_ch3, e.cos_ch3, e.sin_half, e.cos_half};
    const float axis_x = e.axis == 0 ? 1.0f : 0.0f, axis_y = e.axis == 1 ? 1.0f : 0.0f, axis_z = e.axis == 2 ? 1.0f : 0.0f;
    const float *src[4];
    ua_sources(src, xyz, tc);
    // one frame of this lane's carbon; book(k, tick, leaflet) is the second output of hydrogen k
    auto frame = [&](const uint32_t f, auto &&book) {
        V3 bx3{1.0f, 1.0f, 1.0f};
        if (pbc) bx3 = ua_box_edges(a.box9, f);
        uint8_t lf_raw = 0;
        if (a.leaflets) lf_raw = a.aflags[(size_t)a.arow[f] * a.n_mol_total + it.mol];
        const UaCarbon c = ua_fetch(src, f, fstride);
        ua_raise_undefined(a.err, c, f, gslot0, it.mol);
        const UaBonds ub = ua_carbon_exact(tc.kind, c, uc, bx3, pbc, bad);
        int leaflet = -1;
        if (a.leaflets) leaflet = lf_raw ? 1 : 0;
        auto sample = [&](const int k, const V3 v, const V3 b) {
            if (k >= tc.nh) return;
            const int tick = ua_tick<ACOS_COS>(v, e.axis >= 0, axis_x, axis_y, axis_z, a.nx, a.ny, a.nz, a.n2, a.n2sq);
            if (!MOL) {
                const float box[3] = {bx3.x, bx3.y, bx3.z};
                if (e.geom_kind && !geom_inside(e, e.shapes + 8 * (size_t)f, b.x, b.y, b.z, box, pbc, bad)) return;
            }
            acc.s_tot[k] += tick;
            acc.n_tot[k] += 1;
            if (leaflet == 0) { acc.s_up[k] += tick; acc.n_up[k] += 1; }
            book(k, tick, leaflet);
        };
        sample(0, ub.v0, ub.b0);
        sample(1, ub.v1, ub.b1);
        sample(2, ub.v2, ub.b2);
    };
    if (MOL) {
        uint32_t st = 0;
        for (uint32_t fs = f_begin; fs < f_end; fs += G, st++) {
            unsigned long long *const buf = l_word + (size_t)(m.n_buf == 2u ? (st & 1u) : 0u) * G * n_loc;
            const uint32_t fe = min(f_end, fs + G);
            if (active)
                for (uint32_t f = fs; f < fe; f++)
                    frame(f, [&](const int k, const int tick, const int) {
                        const uint32_t w = lw.w[k];
                        if (w != gorder::kUaMolNoWord) atomicAdd(&buf[(f - fs) * n_loc + w], kMapOne + (unsigned long long)(long long)tick);
                    });
            __syncthreads();
            // a wave's threads take consecutive local words of one frame: the tile's words ascend in (group, molecule)
            for (uint32_t w = tid; w < (fe - fs) * n_loc; w += kBlock) {
                const unsigned long long v = buf[w];
                if (!v) continue;
                const uint32_t k = w / n_loc;
                atomicAdd(&m.stage[(size_t)(fs + k - a.frame0) * m.words_per_frame + l_wid[w - k * n_loc]], v);
                buf[w] = 0ull;
            }
            if (m.n_buf != 2u) __syncthreads();
        }
    } else {
        for (uint32_t f = f_begin; f < f_end; f++) {
            if (!active) continue;
            frame(f, [&](const int k, const int tick, const int leaflet) {
                const int bin = gorder::hist_bin(l_edges, s.n_edges, tick);
                if (bin < 0) return;
                if (DIRECT) {
                    unsigned long long *p = dist_rep + (size_t)bin * 2u * a.n_acc + gslot0 + (uint32_t)k;
                    atomicAdd(p, 1ull);
                    if (leaflet == 0) atomicAdd(p + a.n_acc, 1ull);
                } else {
                    atomicAdd(&l_tab[((leaflet > 0 ? n_bins : 0u) + (uint32_t)bin) * ns + it.lslot0 + (uint32_t)k], 1u);
                }
            });
        }
    }
    if (bad) raise_box_range(a.err, f_begin);
    if (!MOL && !DIRECT) {
        __syncthreads();
        const uint32_t words = n_bins * ns;
        for (uint32_t k = tid; k < words; k += kBlock) {
            const uint32_t w0 = l_tab[k], w1 = a.leaflets ? l_tab[words + k] : 0u;
            if (!(w0 | w1)) continue;
            const uint32_t b = k / ns, slot = tile_slots[t.slot0 + (k - b * ns)];
            unsigned long long *p = dist_rep + (size_t)b * 2u * a.n_acc + slot;
            atomicAdd(p, (unsigned long long)w0 + w1);
            if (a.leaflets && w0) atomicAdd(p + a.n_acc, (unsigned long long)w0);
        }
        __syncthreads();        // the table's words are read: its place now serves the sums below
        for (uint32_t k = tid; k < 2 * LS; k += kBlock) { l_s[k] = 0; l_n[k] = 0; }
        __syncthreads();
    }
    // ---- the ordinary sums.  l_s, l_n: zeroed before the first barrier of this body and untouched since (k_ua_mol, DIRECT), or
    // the table's place: the barrier behind the read-out above ended its last reads, the one behind the zeroing the zeroing
    ua_fold_sums(a.rep, a.n_rep, a.n_acc, t, tile_slots, active, it.lslot0, tid, acc, l_s, l_n);
}

// grid = n_ua_tiles * n_chunks padded to a multiple of 8 (dist_chunks with the united-atom tile count); dynamic LDS =
// kDistEdgeBytes + max(kUaSumBytes, the table of the widest tile)
template <bool ACOS_COS, bool DIRECT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_ua_dist(FrameArgs a_in, ExtraArgs e, DistArgs s,
                                                                                               GORDER_UA_KERNEL_ARGS) {
    extern __shared__ __attribute__((aligned(16))) unsigned char l_ua_dyn[];
    unsigned long long *const l_s = reinterpret_cast<unsigned long long *>(l_ua_dyn + kDistEdgeBytes);
    ua_samples_body<ACOS_COS, false, DIRECT>(a_in, e, s, UaMolArgs{}, xyz, box9, aflags, arow, tiles, items, tile_slots, n_tiles, l_ua_dyn,
                                             l_s, reinterpret_cast<uint32_t *>(l_s + 2u * kUaLS));
}

// grid likewise (extras_chunks in whole stages of k_bonds_tiled_mol per staging sub-range — the stage loop here takes any chunk
// length, its last stage the tail —, a.frame0 = the sub-range's first frame); dynamic LDS = ua_mol_lds_bytes(max_local)
template <bool ACOS_COS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_ua_mol(FrameArgs a_in, ExtraArgs e, UaMolArgs m,
                                                                                              GORDER_UA_KERNEL_ARGS) {
    extern __shared__ __attribute__((aligned(16))) unsigned char l_ua_dyn[];
    __shared__ unsigned long long l_s[2 * kUaLS];
    __shared__ uint32_t l_n[2 * kUaLS];
    ua_samples_body<ACOS_COS, true, false>(a_in, e, DistArgs{}, m, xyz, box9, aflags, arow, tiles, items, tile_slots, n_tiles, l_ua_dyn, l_s, l_n);
}
#undef GORDER_UA_KERNEL_ARGS

}  // namespace
