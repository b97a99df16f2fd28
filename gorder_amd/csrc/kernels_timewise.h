// kernels_timewise.h — estimate_error and the convergence columns from the per-frame rows, where the rows lie
// (TimeWiseData::estimate_error, timewise.rs:191-231; prefix_average, timewise.rs:259-274; host arithmetic: timewise_blocks.h).
//
// The rows are tw_sums / tw_cnts [rows][3][n_acc] words of 64 bits (i64 tick sums, u64 sample counts; kernels_extras.h).  With
// leaflets the order kernels fill total and upper only and the lower leaflet's words stay 0: lower = total - upper, which is
// linear, so it is taken once behind the sums (k_tw_lower, k_tw_group_rows) and a third of the rows is never read.
// Everything is integer addition modulo 2^64 until the last step — block sums, group sums, running sums —, so no result
// depends on the launch geometry, on how the frames were cut into batches or on the shard that held them.  The floating
// steps (one truncating division, f64 / 1e6 -> f32, and for the error the reference's f32 sequence) run in one lane, in
// order; the file is compiled with contraction off and correctly rounded f32 divide / sqrt (Makefile).
//
// gfx950 only.  All offsets into the rows are 64-bit.
#pragma once

using gorder::kTwChunkFrames;
typedef unsigned long long tw_u64;

// AnalysisOrder::calc_order (order.rs:101-107) on 64-bit words: the i64 division truncates toward zero; count != 0
__device__ __forceinline__ float tw_mean(tw_u64 sum, tw_u64 count) {
    const long long q = (long long)sum / (long long)count;
    return (float)((double)q / 1e6);
}

// ---- block sums -------------------------------------------------------------------------------------------------------
// Workgroup (x, y): the rows [x * kTwChunkFrames, + kTwChunkFrames) below n_used, the words y * blockDim.x + lane of a row
// (consecutive lanes read consecutive words of a frame).  A thread folds its word over the chunk's rows in registers and
// adds once per block the chunk touches — a chunk that straddles a block boundary adds twice — with a 64-bit atomic.
// fold_words: 2 * n_acc with leaflets (total, upper), else the whole row; out_* [n_blocks][row_words], zeroed before.
__global__ __launch_bounds__(256) void k_tw_blocks(const tw_u64 *__restrict__ tw_sums, const tw_u64 *__restrict__ tw_cnts,
                                                   uint32_t row_words, uint32_t fold_words, tw_u64 n_used, tw_u64 first_position,
                                                   tw_u64 block_size, tw_u64 *__restrict__ out_sums, tw_u64 *__restrict__ out_cnts) {
    const uint32_t j = blockIdx.y * blockDim.x + threadIdx.x;
    if (j >= fold_words) return;
    tw_u64 r = (tw_u64)blockIdx.x * kTwChunkFrames;
    const tw_u64 end = r + kTwChunkFrames < n_used ? r + kTwChunkFrames : n_used;
    while (r < end) {
        const tw_u64 b = gorder::tw_block_of(first_position, r, block_size);
        const tw_u64 e = gorder::tw_segment_end(first_position, r, end, b, block_size);
        tw_u64 s = 0, c = 0;
        for (tw_u64 q = r; q < e; q++) {
            s += tw_sums[q * row_words + j];
            c += tw_cnts[q * row_words + j];
        }
        atomicAdd(&out_sums[b * row_words + j], s);
        atomicAdd(&out_cnts[b * row_words + j], c);
        r = e;
    }
}

// the lower leaflet's block sums: total - upper (leaflets only); a thread per (block, slot)
__global__ __launch_bounds__(256) void k_tw_lower(tw_u64 *__restrict__ sums, tw_u64 *__restrict__ cnts, uint32_t n_acc, tw_u64 n) {
    const tw_u64 i = (tw_u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const tw_u64 at = (i / n_acc) * 3u * n_acc + i % n_acc;
    sums[at + 2u * n_acc] = sums[at] - sums[at + n_acc];
    cnts[at + 2u * n_acc] = cnts[at] - cnts[at + n_acc];
}

// ---- errors -----------------------------------------------------------------------------------------------------------
// One wave per (group, leaflet): workgroup g * 3 + w, 64 threads.  Per block the lanes add the members' sums and counts
// (wave_sum_rows, exact), every lane then holds the block's mean and runs the same f32 sequence as structure.estimate_error —
// sum in block order, / n_blocks; sum of (mean - x)^2, / (n_blocks - 1); sqrt.  The blocks are walked twice rather than
// their means stored.  A block without samples: NaN.
__global__ __launch_bounds__(64) void k_tw_errors(const tw_u64 *__restrict__ block_sums, const tw_u64 *__restrict__ block_cnts,
                                                  uint32_t n_blocks, uint32_t n_acc, const uint32_t *__restrict__ group_begin,
                                                  const uint32_t *__restrict__ slots, float *__restrict__ errors) {
    const uint32_t g = blockIdx.x / 3u, w = blockIdx.x % 3u, lane = threadIdx.x;
    const uint32_t m0 = group_begin[g], m1 = group_begin[g + 1];
    float mean = 0.0f, var = 0.0f;
    bool empty = false;
    for (int pass = 0; pass < 2; pass++) {
        for (uint32_t b = 0; b < n_blocks; b++) {
            const tw_u64 *bs = block_sums + ((tw_u64)b * 3u + w) * n_acc, *bc = block_cnts + ((tw_u64)b * 3u + w) * n_acc;
            tw_u64 s = 0, c = 0;
            for (uint32_t m = m0 + lane; m < m1; m += 64u) { s += bs[slots[m]]; c += bc[slots[m]]; }
            s = wave_sum_rows(s);
            c = wave_sum_rows(c);
            if (c == 0) { empty = true; continue; }
            const float x = tw_mean(s, c);
            if (pass == 0) mean = mean + x;
            else { const float d = mean - x; var = var + d * d; }
        }
        if (pass == 0) mean = mean / (float)n_blocks;
    }
    if (lane == 0) errors[blockIdx.x] = empty ? __builtin_nanf("") : sqrtf(var / (float)(n_blocks - 1u));
}

// ---- convergence ------------------------------------------------------------------------------------------------------
// Per frame and group the members' (sum, count): one wave per (frame, group), the lanes over the members (a molecule type's
// slots are consecutive words of the row), wave_sum_rows.  rows_* [n_frames][3][n_groups]; column = leaflet * n_groups + group.
__global__ __launch_bounds__(256) void k_tw_group_rows(const tw_u64 *__restrict__ tw_sums, const tw_u64 *__restrict__ tw_cnts,
                                                       uint32_t n_acc, int leaflets, tw_u64 n_frames, uint32_t n_groups,
                                                       const uint32_t *__restrict__ group_begin, const uint32_t *__restrict__ slots,
                                                       tw_u64 *__restrict__ rows_sums, tw_u64 *__restrict__ rows_cnts) {
    const uint32_t lane = threadIdx.x & 63u;
    const tw_u64 item = (tw_u64)blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= n_frames * n_groups) return;            // (a whole wave leaves)
    const tw_u64 f = item / n_groups;
    const uint32_t g = (uint32_t)(item % n_groups);
    const tw_u64 *rs = tw_sums + f * 3u * n_acc, *rc = tw_cnts + f * 3u * n_acc;
    tw_u64 s[3] = {0, 0, 0}, c[3] = {0, 0, 0};
    for (uint32_t m = group_begin[g] + lane; m < group_begin[g + 1]; m += 64u) {
        const uint32_t k = slots[m];
        s[0] += rs[k]; c[0] += rc[k];
        s[1] += rs[n_acc + k]; c[1] += rc[n_acc + k];
        if (!leaflets) { s[2] += rs[2u * n_acc + k]; c[2] += rc[2u * n_acc + k]; }
    }
#pragma unroll
    for (int w = 0; w < 3; w++) { s[w] = wave_sum_rows(s[w]); c[w] = wave_sum_rows(c[w]); }
    if (leaflets) { s[2] = s[0] - s[1]; c[2] = c[0] - c[1]; }
    if (lane == 0) {
        const tw_u64 at = f * 3u * n_groups + g;
#pragma unroll
        for (int w = 0; w < 3; w++) { rows_sums[at + (tw_u64)w * n_groups] = s[w]; rows_cnts[at + (tw_u64)w * n_groups] = c[w]; }
    }
}

// Inclusive prefix sums over the frames, reduce-then-scan.  Step 1: a thread per (chunk of kTwChunkFrames frames, column)
// adds the chunk's rows; consecutive lanes take consecutive columns.  tot_* [n_chunks][n_cols].
__global__ __launch_bounds__(256) void k_tw_chunk_totals(const tw_u64 *__restrict__ rows_sums, const tw_u64 *__restrict__ rows_cnts,
                                                         tw_u64 n_frames, uint32_t n_cols, tw_u64 n_items,
                                                         tw_u64 *__restrict__ tot_sums, tw_u64 *__restrict__ tot_cnts) {
    const tw_u64 i = (tw_u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items) return;
    const tw_u64 chunk = i / n_cols, col = i % n_cols;
    const tw_u64 f0 = chunk * kTwChunkFrames, f1 = f0 + kTwChunkFrames < n_frames ? f0 + kTwChunkFrames : n_frames;
    tw_u64 s = 0, c = 0;
    for (tw_u64 f = f0; f < f1; f++) { s += rows_sums[f * n_cols + col]; c += rows_cnts[f * n_cols + col]; }
    tot_sums[i] = s;
    tot_cnts[i] = c;
}

// exclusive scan of 256 values, one per thread, over the workgroup (wave_scan_rows, then the waves' totals in wave order);
// *total: the sum of all 256.  scratch: 4 words.
__device__ __forceinline__ tw_u64 tw_block_scan_exclusive(tw_u64 v, tw_u64 *scratch, tw_u64 *total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const tw_u64 incl = wave_scan_rows(v, lane);
    if (lane == 63u) scratch[wave] = incl;
    __syncthreads();
    tw_u64 before = 0, all = 0;
    for (uint32_t k = 0; k < 4u; k++) { if (k < wave) before += scratch[k]; all += scratch[k]; }
    __syncthreads();
    *total = all;
    return before + incl - v;
}

// Step 2: one workgroup of 256 threads per column.  Thread t owns the chunks [t * per, (t + 1) * per): it adds them, the
// workgroup scans the 256 partial sums, and the thread replaces each of its chunk totals by carry + the sum of all chunks
// before it.  end_* [n_cols] = carry + everything: the next shard's carry.  carry_* may be null (zero).
__global__ __launch_bounds__(256) void k_tw_scan_totals(tw_u64 *__restrict__ tot_sums, tw_u64 *__restrict__ tot_cnts, tw_u64 n_chunks,
                                                        uint32_t n_cols, const tw_u64 *__restrict__ carry_sums,
                                                        const tw_u64 *__restrict__ carry_cnts, tw_u64 *__restrict__ end_sums,
                                                        tw_u64 *__restrict__ end_cnts) {
    __shared__ tw_u64 scratch[4];
    const uint32_t col = blockIdx.x;
    const tw_u64 per = (n_chunks + 255u) / 256u;
    const tw_u64 k0 = threadIdx.x * per < n_chunks ? threadIdx.x * per : n_chunks;
    const tw_u64 k1 = k0 + per < n_chunks ? k0 + per : n_chunks;
    tw_u64 s = 0, c = 0;
    for (tw_u64 k = k0; k < k1; k++) { s += tot_sums[k * n_cols + col]; c += tot_cnts[k * n_cols + col]; }
    tw_u64 all_s, all_c;
    tw_u64 run_s = tw_block_scan_exclusive(s, scratch, &all_s) + (carry_sums ? carry_sums[col] : 0ull);
    tw_u64 run_c = tw_block_scan_exclusive(c, scratch, &all_c) + (carry_cnts ? carry_cnts[col] : 0ull);
    for (tw_u64 k = k0; k < k1; k++) {
        const tw_u64 ts = tot_sums[k * n_cols + col], tc = tot_cnts[k * n_cols + col];
        tot_sums[k * n_cols + col] = run_s;
        tot_cnts[k * n_cols + col] = run_c;
        run_s += ts;
        run_c += tc;
    }
    if (threadIdx.x == 0) {
        end_sums[col] = all_s + (carry_sums ? carry_sums[col] : 0ull);
        end_cnts[col] = all_c + (carry_cnts ? carry_cnts[col] : 0ull);
    }
}

// Step 3: a thread per (chunk, column) walks its frames from the chunk's offset and writes the running average:
// NaN while the cumulative count is 0, then the truncating quotient / 1e6 as f32.  prefix [n_frames][n_cols].
__global__ __launch_bounds__(256) void k_tw_apply(const tw_u64 *__restrict__ rows_sums, const tw_u64 *__restrict__ rows_cnts,
                                                  const tw_u64 *__restrict__ tot_sums, const tw_u64 *__restrict__ tot_cnts,
                                                  tw_u64 n_frames, uint32_t n_cols, tw_u64 n_items, float *__restrict__ prefix) {
    const tw_u64 i = (tw_u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items) return;
    const tw_u64 chunk = i / n_cols, col = i % n_cols;
    const tw_u64 f0 = chunk * kTwChunkFrames, f1 = f0 + kTwChunkFrames < n_frames ? f0 + kTwChunkFrames : n_frames;
    tw_u64 s = tot_sums[i], c = tot_cnts[i];
    for (tw_u64 f = f0; f < f1; f++) {
        s += rows_sums[f * n_cols + col];
        c += rows_cnts[f * n_cols + col];
        prefix[f * n_cols + col] = c == 0 ? __builtin_nanf("") : tw_mean(s, c);
    }
}
