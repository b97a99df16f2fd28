// wave_ops.h — reductions and scans over a wave (64 lanes) and over a workgroup, once each.
// Included by kernels_common.h; device code for gfx950 only.
//
// The order in which a floating sum is associated is part of the results (flags and statistics must not depend on the
// batch, the submit or the shard that carried a frame), so every kernel takes its reductions from here, and a call site
// says by the function's name which of the two orders it uses.  x[l] is lane l's value, a "row" the 16 lanes 16 r .. 16 r + 15.
//
//   ROW ORDER (*_rows, row_sum, rows_to_wave; DPP only, no LDS — six ds_bpermute round trips a butterfly sum are dearer):
//     steps 1-4  row_shr:1, :2, :4, :8   x[l] += x[l - n] where l mod 16 >= n, all lanes at once (Hillis-Steele inside
//                                        the row): lane 16 r + k ends with the sum of lanes 16 r .. 16 r + k added
//                                        in that tree, lane 16 r + 15 with the row's total R_r.          (row_sum)
//     step 5     row_bcast:15, rows 1, 3 x[l] += x[15] in row 1, += x[47] in row 3: lane 31 = R_1 + R_0, lane 63 = R_3 + R_2
//     step 6     row_bcast:31, rows 2, 3 x[l] += x[31] in rows 2 and 3: lane 63 = (R_3 + R_2) + (R_1 + R_0)   (rows_to_wave)
//     The result is defined in LANE 63 only; wave_*_rows hand it to every lane by v_readlane.  Minima and maxima take the
//     same six steps.  The inclusive scan takes steps 1-4 and then adds, in lane l, R_0, R_1, R_2 (read from lanes 15,
//     31, 47 by v_readlane: a __shfl is a trip through the LDS each) in this order, each only if its row lies before l's.
//     Every lane of the wave must be there.
//   BUTTERFLY (*_bfly; __shfl_xor through the LDS crossbar):
//     steps off = 32, 16, 8, 4, 2, 1     x[l] = x[l] + x[l ^ off], all lanes at once.  EVERY lane ends with the result,
//                                        the same bits in all of them (a + b = b + a).
//   The __shfl_up scan (wave_scan_shfl): off = 1, 2, 4, .., 32: x[l] += x[l - off] where l >= off (Hillis-Steele over
//   the 64 lanes).
//   BLOCK (block_*): the wave's result by butterfly, lane 0 of wave w parks it in scratch[w], and after a barrier every
//   thread folds the parked values in wave order w = 0, 1, .. starting from 0.0 (sums) or from its own wave's result
//   (extrema): every thread gets the same bits.  block_finfo_record is such a fold of (min, max, flags) that ends in a
//   frame's finfo record, which is why the record's key encoding (local_float_key) lives here too.
#pragma once

namespace {

// ---- DPP steps ------------------------------------------------------------------------------------
// The value of the lane that CTRL names (0x111, 0x112, 0x114, 0x118 = row_shr:1, 2, 4, 8; 0x142 = row_bcast:15;
// 0x143 = row_bcast:31).  A lane whose source lane does not exist (a shift across the start of its row), or whose row
// is not in ROW_MASK (bit r = row r), gets 0 from dpp_or_zero — bound_ctrl, so the move folds into the add that uses
// it — and its own value from dpp_or_self (for minima and maxima).
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ int dpp_or_zero(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, true); }
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp_or_zero(uint32_t v) { return (uint32_t)dpp_or_zero<CTRL, ROW_MASK>((int)v); }
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_or_zero(float v) { return __int_as_float(dpp_or_zero<CTRL, ROW_MASK>(__float_as_int(v))); }
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double dpp_or_zero(double v) {            // two 32-bit moves
    const int lo = dpp_or_zero<CTRL, ROW_MASK>(__double2loint(v)), hi = dpp_or_zero<CTRL, ROW_MASK>(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ unsigned long long dpp_or_zero(unsigned long long v) {   // two 32-bit moves: the exact i64 / u64 sums of kernels_timewise.h
    const uint32_t lo = dpp_or_zero<CTRL, ROW_MASK>((uint32_t)v), hi = dpp_or_zero<CTRL, ROW_MASK>((uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_or_self(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
// the value one lane holds, for every lane (lane index known at compile time: v_readlane, no LDS)
__device__ __forceinline__ int lane_value(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ uint32_t lane_value(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ float lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ double lane_value(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ unsigned long long lane_value(unsigned long long v, int l) {
    return ((unsigned long long)lane_value((uint32_t)(v >> 32), l) << 32) | lane_value((uint32_t)v, l);
}

// ---- row order (int, uint32_t, unsigned long long, float, double) -----------------------------------------------------
template <class T>
__device__ __forceinline__ T row_sum(T v) {             // steps 1-4: lane 15 of every row gets the row's total
    v = v + dpp_or_zero<0x111>(v); v = v + dpp_or_zero<0x112>(v); v = v + dpp_or_zero<0x114>(v); v = v + dpp_or_zero<0x118>(v);
    return v;
}
// several row sums step by step together (a DPP read waits two states behind the write of its source: the others' steps fill them)
template <int CTRL, class... T>
__device__ __forceinline__ void row_step(T &...v) { ((v = v + dpp_or_zero<CTRL>(v)), ...); }
template <class... T>
__device__ __forceinline__ void row_sums(T &...v) { row_step<0x111>(v...); row_step<0x112>(v...); row_step<0x114>(v...); row_step<0x118>(v...); }
template <class T>
__device__ __forceinline__ T rows_to_wave(T v) {        // steps 5-6 behind row_sum: lane 63 gets the wave's total
    v = v + dpp_or_zero<0x142, 0xa>(v); v = v + dpp_or_zero<0x143, 0xc>(v);
    return v;
}
template <class T>
__device__ __forceinline__ T wave_sum_rows(T v) { return lane_value(rows_to_wave(row_sum(v)), 63); }
__device__ __forceinline__ float wave_min_rows(float v) {
    v = fminf(v, dpp_or_self<0x111>(v)); v = fminf(v, dpp_or_self<0x112>(v));
    v = fminf(v, dpp_or_self<0x114>(v)); v = fminf(v, dpp_or_self<0x118>(v));
    v = fminf(v, dpp_or_self<0x142, 0xa>(v)); v = fminf(v, dpp_or_self<0x143, 0xc>(v));
    return lane_value(v, 63);
}
__device__ __forceinline__ float wave_max_rows(float v) {
    v = fmaxf(v, dpp_or_self<0x111>(v)); v = fmaxf(v, dpp_or_self<0x112>(v));
    v = fmaxf(v, dpp_or_self<0x114>(v)); v = fmaxf(v, dpp_or_self<0x118>(v));
    v = fmaxf(v, dpp_or_self<0x142, 0xa>(v)); v = fmaxf(v, dpp_or_self<0x143, 0xc>(v));
    return lane_value(v, 63);
}
// inclusive scan over the 64 lanes (lane = this thread's lane); the f64 form is exact — and so independent of the
// order — for what its callers scan: integers below 2^40
__device__ __forceinline__ uint32_t wave_scan_rows(uint32_t v, uint32_t lane) {
    v = row_sum(v);
    const uint32_t t0 = lane_value(v, 15), t1 = lane_value(v, 31), t2 = lane_value(v, 47);
    const uint32_t r = lane >> 4;
    return v + (r > 0u ? t0 : 0u) + (r > 1u ? t1 : 0u) + (r > 2u ? t2 : 0u);
}
__device__ __forceinline__ unsigned long long wave_scan_rows(unsigned long long v, uint32_t lane) {
    v = row_sum(v);
    const unsigned long long t0 = lane_value(v, 15), t1 = lane_value(v, 31), t2 = lane_value(v, 47);
    const uint32_t r = lane >> 4;
    return v + (r > 0u ? t0 : 0ull) + (r > 1u ? t1 : 0ull) + (r > 2u ? t2 : 0ull);
}
__device__ __forceinline__ double wave_scan_rows(double v, uint32_t lane) {
    v = row_sum(v);
    const double t0 = lane_value(v, 15), t1 = lane_value(v, 31), t2 = lane_value(v, 47);
    const uint32_t r = lane >> 4;
    return v + (r > 0u ? t0 : 0.0) + (r > 1u ? t1 : 0.0) + (r > 2u ? t2 : 0.0);
}

// ---- butterfly ------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_bfly(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max_bfly(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off, 64));
    return v;
}
// Several quantities through ONE butterfly, step by step together: their trips through the LDS overlap (one call after
// the other waits for every __shfl before it sends the next).  Each quantity's own order is the butterfly's.
__device__ __forceinline__ void wave_minmax_bfly(float &lo, float &hi) {
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
}
__device__ __forceinline__ void wave_minmax_or_bfly(float &lo, float &hi, uint32_t &flags) {
    for (int off = 32; off >= 1; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
        flags |= (uint32_t)__shfl_xor((int)flags, off, 64);
    }
}
__device__ __forceinline__ void wave_sum2_minmax_bfly(double &s, double &q, float &lo, float &hi) {
    for (int off = 32; off >= 1; off >>= 1) {
        s += __shfl_xor(s, off, 64); q += __shfl_xor(q, off, 64);
        lo = fminf(lo, __shfl_xor(lo, off, 64)); hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
}
// inclusive scan over the 64 lanes by __shfl_up (lane = this thread's lane)
__device__ __forceinline__ uint32_t wave_scan_shfl(uint32_t v, uint32_t lane) {
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint32_t t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// ---- block ----------------------------------------------------------------------------------------
// N sums for the price (two barriers) of one, every thread gets the same totals; scratch holds N x 16 doubles
// (a loop over the waves per sum: one loop that adds all N keeps N accumulators live — 20 VGPRs and a wave of occupancy
// in the spherical kernel, which calls this with N = 6)
template <int N>
__device__ __forceinline__ void block_sum_n(double (&v)[N], double *scratch) {
    const uint32_t wave = threadIdx.x >> 6, n_waves = (blockDim.x + 63u) >> 6;
#pragma unroll
    for (int q = 0; q < N; q++) {
        v[q] = wave_sum_bfly(v[q]);
        if ((threadIdx.x & 63u) == 0) scratch[16 * q + wave] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; q++) {
        double r = 0.0;
        for (uint32_t w = 0; w < n_waves; w++) r += scratch[16 * q + w];
        v[q] = r;
    }
    __syncthreads();
}
__device__ __forceinline__ double block_sum(double v, double *scratch /* 16 */) {
    double a[1] = {v};
    block_sum_n<1>(a, scratch);
    return a[0];
}
__device__ __forceinline__ void block_minmax(float &lo, float &hi, float *scratch /* 2 x 16 */) {
    wave_minmax_bfly(lo, hi);
    const uint32_t wave = threadIdx.x >> 6, n_waves = (blockDim.x + 63u) >> 6;
    if ((threadIdx.x & 63u) == 0) { scratch[wave] = lo; scratch[16 + wave] = hi; }
    __syncthreads();
    for (uint32_t w = 0; w < n_waves; w++) { lo = fminf(lo, scratch[w]); hi = fmaxf(hi, scratch[16 + w]); }
    __syncthreads();
}

// ordered-integer image of a float (monotonic for every non-NaN value): atomicMin / atomicMax on floats of either sign
__device__ __forceinline__ uint32_t local_float_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float local_key_float(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// A frame's finfo record from a workgroup of 1024 threads: *out = (key of the minimum of zlo, key of the maximum of zhi,
// the or of flags & record_mask, 2), or (0xffffffff, 0, flags, 2) if no thread had a value (zlo > zhi everywhere).
// Butterflies, one barrier, thread 0 folds the 16 waves' entries and writes; it alone leaves with the block's flags
// (unmasked) in `flags`.  l_lo, l_hi, l_flags: 16 entries each (a smaller workgroup: the absent waves' entries must
// hold 3.0e38f, -3.0e38f, 0).
__device__ __forceinline__ void block_finfo_record(float zlo, float zhi, uint32_t &flags, uint32_t record_mask, float *l_lo,
                                                   float *l_hi, uint32_t *l_flags, uint4 *out) {
    wave_minmax_or_bfly(zlo, zhi, flags);
    const uint32_t tid = threadIdx.x;
    if ((tid & 63u) == 0u) { l_lo[tid >> 6] = zlo; l_hi[tid >> 6] = zhi; l_flags[tid >> 6] = flags; }
    __syncthreads();
    if (tid == 0u) {
        for (uint32_t w = 1; w < 16u; w++) { zlo = fminf(zlo, l_lo[w]); zhi = fmaxf(zhi, l_hi[w]); flags |= l_flags[w]; }
        *out = zlo <= zhi ? make_uint4(local_float_key(zlo), local_float_key(zhi), flags & record_mask, 2u)
                          : make_uint4(0xffffffffu, 0u, flags & record_mask, 2u);
    }
}

}  // namespace
