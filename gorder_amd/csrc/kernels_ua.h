// kernels_ua.h — the united-atom family: the hydrogen construction (V3, the Pbc* policies, ua_carbon, ua_carbon_pairs,
// ua_carbon_fast, ua_carbon_slow), what its four tile kernels have in common, once, and k_ua_extras / k_ua_extras_fast.
// Part of the single translation unit gorder_hip.hip, behind kernels_extras.h (ExtraArgs, geom_inside, extras_add,
// extras_flush_tw) and before kernels_hist.h and kernels_ua_samples.h (k_ua_dist, k_ua_mol); device code for gfx950 only.
//
// The shared pieces are inlined into their kernel; none has a template parameter or a flag that says which kernel called
// it: where two kernels differ, the difference is at the call (the rule of kernels_tile.h).  The contracts:
//
//   ua_tile_work, ua_tile_lane      no barrier, no LDS.  Every thread of the workgroup calls ua_tile_work (grid.x =
//       ua_grid(n_tiles, n_chunks) of the host: a multiple of 8); the KERNEL returns on `padding`, before ua_tile_lane
//       loads anything.  They are two because the return sits between them in the kernel's own text: as one function
//       that returns early or loads regardless, k_ua_dist gained 16 bytes of scratch and 2-5 VGPR spills.  A lane at or
//       past the tile's n_items is not `active` and holds the all-zero UaItem (kind 0, one hydrogen, atoms atom0, local
//       slot 0, molecule 0: loads through it stay inside the tile, nothing may be booked for it).
//   ua_sources, ua_fetch, ua_box_edges      no barrier.  Every lane may fetch (an idle lane reads the tile's first atom
//       four times): ua_extras_body's PREFETCH ring relies on it.
//   ua_raise_undefined              the first undefined atom in index order; the smallest key wins in raise_error.
//   ua_carbon_exact                 the only caller of ua_carbon_slow besides ua_extras_body.  `bad` is OR-ed, never cleared.
//   ua_tick                         the caller says whether the axis short form is allowed and hands in the normal: the
//       static one, or ua_extras_body's per-molecule one (then axis_allowed is false).
//   ua_fold_sums                    ONE barrier, its own, behind the LDS atomics.  ALL kBlock threads must reach it in
//       uniform control flow.  The caller hands it [2][kUaLS] u64 + [2][kUaLS] u32 of LDS that it has ZEROED and that no
//       thread reads or writes for another purpose from the caller's last barrier on: static arrays zeroed before the
//       first barrier of the kernel (k_ua_extras*, k_ua_mol, k_ua_dist<.., DIRECT>), or the place of k_ua_dist's table —
//       then the caller's barrier behind the table's read-out ends the last reads, the caller zeroes, and a second
//       barrier of the caller ends the zeroing; the comment at the call names them.  The accumulators come by value.
//       Integer sums: the result does not depend on the order.
//
// No helper takes FrameArgs (the fields come as scalars; the two lines that copy a_in and set the __restrict__ streams
// stay in both bodies), as in kernels_tile.h.  The kernels' code must not change with their text: all 18 instantiations
// keep VGPRs, AGPRs, scratch, VGPR spills, LDS and occupancy (profiles/ua_helpers_resources.txt).
//
// Left alone on purpose — ua_samples_body (kernels_ua_samples.h) uses every piece; ua_extras_body restates four, because
// its exact instantiations sit on a knife's edge of the register allocator (126-128 VGPRs, up to 43 VGPR spills).
// Measured piece by piece, everything else as in the parent (cross-compiled, VGPR spills unless named otherwise):
//   ua_tile_work + ua_tile_lane     all 8 k_ua_extras change: <false, 0> 128 -> 126 VGPRs, 2 -> 0 spills, code 18 576 -> 15 020
//                      bytes (the compiler then drops a second copy of part of the construction), <false, 2> 42 -> 33,
//                      scratch 272 -> 240; k_ua_extras_fast<2> 31 -> 32.  As one function that returns early: the same, and
//                      k_ua_extras_fast<0> and <3> +1-2 VGPRs.
//   ua_carbon_exact    the same flip of all 8 k_ua_extras (<false, 0> 128 -> 124 VGPRs, 15 020 bytes, 0 spills; <true, 2>
//                      43 -> 29, scratch 288 -> 224) with the fast kernels untouched; with the hand-over to ua_carbon_slow
//                      as a helper of its own for the fast branch, k_ua_extras_fast<2> 31 -> 35 spills.
//                      Both flips make the exact kernels smaller and spill less: a change of the kernels' code that wants
//                      its own timing, not a move of text.
//   ua_raise_undefined all 12 change in every shape tried (the carbon by value or by reference, four scalars; with the test
//                      at the call or inside): k_ua_extras<false, 1> 8 -> 15 spills, <true, 1> 126 -> 128 VGPRs, three of
//                      the four fast kernels +2 VGPRs.  (One raise_error with a selected atom index instead of the chain
//                      of four: k_ua_extras_fast<0> 116 -> 110 VGPRs — other code again.)
//   ua_sources         k_ua_extras<false, 2> alone: 42 -> 43 spills, scratch 272 -> 288.
// Speed (profiles/ua_helpers_bench.json): every kernel group inside the parent's spread but k_ua_dist with its LDS table,
// 0.866, 0.864 | 0.878, 0.880 ms parent | change in the first session and 0.875, 0.876, 0.882 | 0.879, 0.880, 0.881 in a second,
// in which builds that shared one group of pieces each scattered over 0.866-0.904: no piece stood out, none went back.
// So a change to the padding test, the error order or the slow-path condition is made here AND in ua_extras_body;
// tests/test_sample_edges_gpu.py drives both through the same degenerate carbons (test_ua, test_ua_samples).
//   the fast construction's arithmetic, ua_carbon / ua_carbon_pairs / ua_carbon_fast as three functions (the reference's
//                      operation order, case by case), the host side, kernel names, timing labels, order_route.h, the ABI.
#pragma once

namespace {

constexpr uint32_t kUaLS = 3u * kBlock;                     // local slots of a united-atom tile (<= 3 hydrogens per carbon)
constexpr uint32_t kUaSumBytes = 2u * kUaLS * 12u;          // ua_fold_sums' [2][kUaLS] u64 sums + [2][kUaLS] u32 counts

// ---- united atoms: hydrogen construction, restating uaorder.rs:947-1104 with the operation order of
// nalgebra's Rotation3::from_axis_angle / matrix * vector and groan_rs' shift / wrap (oracle:
// gorder_oracle_predict_hydrogens).  All f32, no FMA.
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3_cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float v3_norm(V3 a) { return __builtin_sqrtf((a.x * a.x + a.y * a.y) + a.z * a.z); }
__device__ __forceinline__ V3 v3_unit(V3 a) { const float n = v3_norm(a); return {a.x / n, a.y / n, a.z / n}; }
__device__ __forceinline__ V3 v3_rotate(V3 u, float s, float c, V3 v) {
    const float sqx = u.x * u.x, sqy = u.y * u.y, sqz = u.z * u.z, omc = 1.0f - c;
    const float m11 = sqx + (1.0f - sqx) * c, m12 = u.x * u.y * omc - u.z * s, m13 = u.x * u.z * omc + u.y * s;
    const float m21 = u.x * u.y * omc + u.z * s, m22 = sqy + (1.0f - sqy) * c, m23 = u.y * u.z * omc - u.x * s;
    const float m31 = u.x * u.z * omc - u.y * s, m32 = u.y * u.z * omc + u.x * s, m33 = sqz + (1.0f - sqz) * c;
    return {(m11 * v.x + m12 * v.y) + m13 * v.z, (m21 * v.x + m22 * v.y) + m23 * v.z,
            (m31 * v.x + m32 * v.y) + m33 * v.z};
}
// Periodic-boundary policies for the hydrogen construction.  PbcStep does one select-only shift per
// operation and raises `slow` when that was not enough; PbcLoop is the literal `while` form of the
// reference.  The kernel evaluates a carbon with PbcStep and, only if `slow` came up, again with PbcLoop.
// (all state in scalars and every aggregate passed by value: nothing here may end up in scratch)
struct PbcStep {
    V3 box;
    bool pbc;
    bool slow = false;
    int bad = 0;
    __device__ __forceinline__ float len(int k) const { return k == 0 ? box.x : (k == 1 ? box.y : box.z); }
    __device__ __forceinline__ float mi(float d, int k) { return pbc ? gm_min_image_step(d, len(k), slow) : d; }
    __device__ __forceinline__ float wr(float x, int k) {
        if (!pbc) return x;
        const float L = len(k);
        const float r = x > L ? x - L : (x < 0.0f ? x + L : x);
        slow = slow || (r > L) || (r < 0.0f);
        return r;
    }
    // a / |a| with the cores of the IEEE square root and division (gm_sqrt_core, gm_div_core) and ONE reciprocal
    // refinement for the three quotients: the same bits as v3_unit while |a|^2 lies in [2^-40, 2^40] (a component
    // below 2^-103 aside, which no coordinate difference produces); anything else raises `slow`.
    __device__ __forceinline__ V3 unit(V3 a) {
        const float s2 = (a.x * a.x + a.y * a.y) + a.z * a.z;
        slow = slow || !(s2 >= 0x1p-40f && s2 <= 0x1p+40f);
        const float n = gm_sqrt_core(s2);
        float r = __builtin_amdgcn_rcpf(n);
        r = __builtin_fmaf(__builtin_fmaf(-n, r, 1.0f), r, r);
        auto quot = [&](float c) {
            float q = c * r;
            q = __builtin_fmaf(__builtin_fmaf(-n, q, c), r, q);
            return __builtin_fmaf(__builtin_fmaf(-n, q, c), r, q);
        };
        return {quot(a.x), quot(a.y), quot(a.z)};
    }
};
struct PbcLoop {
    V3 box;
    bool pbc;
    bool slow = false;
    int bad = 0;
    __device__ __forceinline__ float len(int k) const { return k == 0 ? box.x : (k == 1 ? box.y : box.z); }
    __device__ __forceinline__ float mi(float d, int k) { return pbc ? gm_min_image_loop(d, len(k), bad) : d; }
    __device__ __forceinline__ float wr(float x, int k) { return pbc ? gm_wrap(x, len(k), bad) : x; }
    __device__ __forceinline__ V3 unit(V3 a) { return v3_unit(a); }
};
template <typename PB>
__device__ __forceinline__ V3 v3_to(V3 p1, V3 p2, PB &pb) {
    return {pb.mi(p2.x - p1.x, 0), pb.mi(p2.y - p1.y, 1), pb.mi(p2.z - p1.z, 2)};
}
template <typename PB>
__device__ __forceinline__ V3 v3_shift_wrap(V3 t, V3 dir, PB &pb) {
    const V3 u = pb.unit(dir);
    return {pb.wr(t.x + u.x * 0.109f, 0), pb.wr(t.y + u.y * 0.109f, 1), pb.wr(t.z + u.z * 0.109f, 2)};   // BOND_LENGTH
}

struct UaConsts {
    float sin_tet, cos_tet, sin_ch3, cos_ch3, sin_half, cos_half;
};
struct UaCarbon {       // the carbon's atoms: helper1,target,helper2,- or h1,h2,h3,target (CH1 saturated)
    V3 p0, p1, p2, p3;
};
struct UaBonds {        // per hydrogen: the C->H vector and the bond position (unused entries are zero)
    V3 v0, v1, v2, b0, b1, b2;
    int bad;
};

// hydrogens of one united-atom carbon, then per hydrogen the C->H vector and the bond position
// (UAAtom::calculate_sch, uaorder.rs:375-397: vec = target -> H, position = H + vec / 2 (sic))
template <typename PB>
__device__ __forceinline__ UaBonds ua_carbon(uint32_t kind, UaCarbon c, UaConsts e, PB &pb) {
    const V3 zero{0.0f, 0.0f, 0.0f};
    V3 h0 = zero, h1 = zero, h2 = zero, target = c.p1;
    if (kind == GORDER_UA_CH3) {            // uaorder.rs:947-981
        const V3 th1 = v3_to(target, c.p0, pb), th2 = v3_to(target, c.p2, pb);
        const V3 ua = pb.unit(v3_cross(th2, th1));
        const V3 hv1 = v3_rotate(ua, e.sin_tet, e.cos_tet, th1);
        h0 = v3_shift_wrap(target, hv1, pb);
        const V3 n1 = pb.unit(th1);
        h1 = v3_shift_wrap(target, v3_rotate(n1, e.sin_ch3, e.cos_ch3, hv1), pb);
        h2 = v3_shift_wrap(target, v3_rotate(n1, -e.sin_ch3, e.cos_ch3, hv1), pb);
    } else if (kind == GORDER_UA_CH2) {     // uaorder.rs:985-1020
        const V3 th1 = pb.unit(v3_to(target, c.p0, pb)), th2 = pb.unit(v3_to(target, c.p2, pb));
        const V3 pn = v3_cross(th2, th1);
        const V3 ra = pb.unit(V3{th1.x - th2.x, th1.y - th2.y, th1.z - th2.z});
        const V3 rv = v3_cross(pn, ra);
        const V3 ura = pb.unit(ra);
        h0 = v3_shift_wrap(target, v3_rotate(ura, e.sin_half, e.cos_half, rv), pb);
        h1 = v3_shift_wrap(target, v3_rotate(ura, -e.sin_half, e.cos_half, rv), pb);
    } else if (kind == GORDER_UA_CH1_UNSAT) {   // uaorder.rs:1024-1045
        const V3 th1 = v3_to(target, c.p0, pb), th2 = v3_to(target, c.p2, pb);
        const float prod = (th1.x * th2.x + th1.y * th2.y) + th1.z * th2.z;
        const float n1 = v3_norm(th1), n2 = v3_norm(th2);
        float gamma = 0.0f;
        if (!(n1 == 0.0f || n2 == 0.0f)) {
            float cs = prod / (n1 * n2);
            cs = cs < -1.0f ? -1.0f : (cs > 1.0f ? 1.0f : cs);
            gamma = gm_acosf(cs);
        }
        const float ang = 3.14159265358979323846f - (gamma / 2.0f);
        // own sin / cos kernels (gm_math.h), restated by the oracle's non-libm modes: the hydrogen is the same bits there
        const float sn = gm_sinf_0pi(ang), cs = gm_cosf(ang);
        const V3 ua = pb.unit(v3_cross(th1, th2));
        h0 = v3_shift_wrap(target, ang == 0.0f ? th2 : v3_rotate(ua, sn, cs, th2), pb);
    } else {                                // CH1 saturated, uaorder.rs:1087-1104 (h1, h2, h3, target)
        target = c.p3;
        const V3 t1 = pb.unit(v3_to(target, c.p0, pb)), t2 = pb.unit(v3_to(target, c.p1, pb)),
                 t3 = pb.unit(v3_to(target, c.p2, pb));
        h0 = v3_shift_wrap(target, V3{-((t1.x + t2.x) + t3.x), -((t1.y + t2.y) + t3.y), -((t1.z + t2.z) + t3.z)}, pb);
    }
    UaBonds r;
    r.v0 = v3_to(target, h0, pb);
    r.b0 = {h0.x + r.v0.x / 2.0f, h0.y + r.v0.y / 2.0f, h0.z + r.v0.z / 2.0f};
    r.v1 = r.v2 = r.b1 = r.b2 = zero;
    if (kind == GORDER_UA_CH3 || kind == GORDER_UA_CH2) {
        r.v1 = v3_to(target, h1, pb);
        r.b1 = {h1.x + r.v1.x / 2.0f, h1.y + r.v1.y / 2.0f, h1.z + r.v1.z / 2.0f};
    }
    if (kind == GORDER_UA_CH3) {
        r.v2 = v3_to(target, h2, pb);
        r.b2 = {h2.x + r.v2.x / 2.0f, h2.y + r.v2.y / 2.0f, h2.z + r.v2.z / 2.0f};
    }
    r.bad = pb.bad;
    return r;
}
// ---- the same constructions with PAIRS of vectors in packed registers (v_pk_mul / v_pk_add / v_pk_fma_f32 do two
// f32 operations per lane and instruction).  A methylene carbon does everything twice — two helper vectors are made
// periodic and normalised, two hydrogens are rotated (by +- the same angle about the same axis), shifted, wrapped and
// turned into bond vectors — and a methyl carbon does so for its second and third hydrogen.  Lane 0 / lane 1 of an `f2`
// hold the two instances; every component goes through exactly the operations of the scalar code above (IEEE
// multiplication is sign-symmetric, so u * (-s) = -(u * s) and a - (-b) = a + b bit for bit), hence the same bits.
typedef float f2 __attribute__((ext_vector_type(2)));
typedef int i2 __attribute__((ext_vector_type(2)));
struct V3P { f2 x, y, z; };
__device__ __forceinline__ f2 f2_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 f2_splat(float v) { return f2{v, v}; }
__device__ __forceinline__ V3 v3p_lane0(V3P a) { return {a.x.x, a.y.x, a.z.x}; }
__device__ __forceinline__ V3 v3p_lane1(V3P a) { return {a.x.y, a.y.y, a.z.y}; }
struct PbcStep2 {       // PbcStep on pairs
    V3 box;
    bool pbc;
    i2 slow2 = {0, 0};       // the "one shift was not enough" conditions, OR-ed per lane; reduced once by slow()
    __device__ __forceinline__ bool slow() const { return (slow2.x | slow2.y) != 0; }
    __device__ __forceinline__ f2 mi(f2 d, float L) {
        if (!pbc) return d;
        const f2 Lv = f2_splat(L), half = Lv / 2.0f;
        const f2 r = __builtin_elementwise_abs(d) > half ? d - __builtin_elementwise_copysign(Lv, d) : d;
        slow2 |= __builtin_elementwise_abs(r) > half;
        return r;
    }
    __device__ __forceinline__ f2 wr(f2 x, float L) {
        if (!pbc) return x;
        const f2 Lv = f2_splat(L), zero = f2_splat(0.0f);
        const f2 r = x > Lv ? x - Lv : (x < zero ? x + Lv : x);
        slow2 |= (r > Lv) | (r < zero);
        return r;
    }
    __device__ __forceinline__ V3P unit(V3P a) {       // PbcStep::unit, twice
        const f2 s2 = (a.x * a.x + a.y * a.y) + a.z * a.z;
        slow2 |= ~((s2 >= f2_splat(0x1p-40f)) & (s2 <= f2_splat(0x1p+40f)));
        const f2 s = f2{__builtin_amdgcn_sqrtf(s2.x), __builtin_amdgcn_sqrtf(s2.y)};      // gm_sqrt_core
        const i2 si = __builtin_bit_cast(i2, s);
        const f2 sm = __builtin_bit_cast(f2, si - 1), sp = __builtin_bit_cast(f2, si + 1);
        const f2 rm = f2_fma(-sm, s, s2), rp = f2_fma(-sp, s, s2);
        f2 n = rm <= f2_splat(0.0f) ? sm : s;
        n = rp > f2_splat(0.0f) ? sp : n;
        f2 r = f2{__builtin_amdgcn_rcpf(n.x), __builtin_amdgcn_rcpf(n.y)};
        r = f2_fma(f2_fma(-n, r, f2_splat(1.0f)), r, r);
        auto quot = [&](f2 c) {
            f2 q = c * r;
            q = f2_fma(f2_fma(-n, q, c), r, q);
            return f2_fma(f2_fma(-n, q, c), r, q);
        };
        return {quot(a.x), quot(a.y), quot(a.z)};
    }
};
// target -> the two points (p, q), periodic
__device__ __forceinline__ V3P v3p_to(V3 t, V3 p, V3 q, PbcStep2 &pb) {
    return {pb.mi(f2{p.x, q.x} - f2_splat(t.x), pb.box.x), pb.mi(f2{p.y, q.y} - f2_splat(t.y), pb.box.y),
            pb.mi(f2{p.z, q.z} - f2_splat(t.z), pb.box.z)};
}
__device__ __forceinline__ V3P v3p_to(V3 t, V3P h, PbcStep2 &pb) {
    return {pb.mi(h.x - f2_splat(t.x), pb.box.x), pb.mi(h.y - f2_splat(t.y), pb.box.y), pb.mi(h.z - f2_splat(t.z), pb.box.z)};
}
// v rotated about the unit axis u by +angle (lane 0) and -angle (lane 1): v3_rotate with s = (+s, -s)
__device__ __forceinline__ V3P v3p_rotate_pm(V3 u, float s, float c, V3 v) {
    const float sqx = u.x * u.x, sqy = u.y * u.y, sqz = u.z * u.z, omc = 1.0f - c;
    const f2 sv = f2{s, -s};
    const f2 uxs = f2_splat(u.x) * sv, uys = f2_splat(u.y) * sv, uzs = f2_splat(u.z) * sv;
    const float xy = u.x * u.y * omc, xz = u.x * u.z * omc, yz = u.y * u.z * omc;
    const float m11 = sqx + (1.0f - sqx) * c, m22 = sqy + (1.0f - sqy) * c, m33 = sqz + (1.0f - sqz) * c;
    const f2 m12 = f2_splat(xy) - uzs, m13 = f2_splat(xz) + uys;
    const f2 m21 = f2_splat(xy) + uzs, m23 = f2_splat(yz) - uxs;
    const f2 m31 = f2_splat(xz) - uys, m32 = f2_splat(yz) + uxs;
    const f2 vx = f2_splat(v.x), vy = f2_splat(v.y), vz = f2_splat(v.z);
    return {(f2_splat(m11) * vx + m12 * vy) + m13 * vz, (m21 * vx + f2_splat(m22) * vy) + m23 * vz,
            (m31 * vx + m32 * vy) + f2_splat(m33) * vz};
}
__device__ __forceinline__ V3P v3p_shift_wrap(V3 t, V3P dir, PbcStep2 &pb) {
    const V3P u = pb.unit(dir);
    return {pb.wr(f2_splat(t.x) + u.x * 0.109f, pb.box.x), pb.wr(f2_splat(t.y) + u.y * 0.109f, pb.box.y),
            pb.wr(f2_splat(t.z) + u.z * 0.109f, pb.box.z)};   // BOND_LENGTH
}
// CH2 and CH3 carbons by pairs; `slow` comes back raised when a literal-loop evaluation is needed instead
__device__ __forceinline__ UaBonds ua_carbon_pairs(uint32_t kind, UaCarbon c, UaConsts e, V3 box, bool pbc, bool &slow) {
    const V3 zero{0.0f, 0.0f, 0.0f};
    const V3 target = c.p1;
    PbcStep ps{box, pbc};
    PbcStep2 pp{box, pbc};
    UaBonds r;
    r.v2 = r.b2 = zero;
    V3P h;                                   // CH2: hydrogens 0, 1; CH3: hydrogens 1, 2
    if (kind == GORDER_UA_CH2) {            // uaorder.rs:985-1020
        const V3P th = pp.unit(v3p_to(target, c.p0, c.p2, pp));
        const V3 th1 = v3p_lane0(th), th2 = v3p_lane1(th);
        const V3 pn = v3_cross(th2, th1);
        const V3 ra = ps.unit(V3{th1.x - th2.x, th1.y - th2.y, th1.z - th2.z});
        const V3 rv = v3_cross(pn, ra);
        const V3 ura = ps.unit(ra);
        h = v3p_shift_wrap(target, v3p_rotate_pm(ura, e.sin_half, e.cos_half, rv), pp);
    } else {                                // CH3, uaorder.rs:947-981
        const V3P th = v3p_to(target, c.p0, c.p2, pp);
        const V3 th1 = v3p_lane0(th), th2 = v3p_lane1(th);
        const V3 ua = ps.unit(v3_cross(th2, th1));
        const V3 hv1 = v3_rotate(ua, e.sin_tet, e.cos_tet, th1);
        const V3 h0 = v3_shift_wrap(target, hv1, ps);
        const V3 n1 = ps.unit(th1);
        h = v3p_shift_wrap(target, v3p_rotate_pm(n1, e.sin_ch3, e.cos_ch3, hv1), pp);
        r.v0 = v3_to(target, h0, ps);
        r.b0 = {h0.x + r.v0.x / 2.0f, h0.y + r.v0.y / 2.0f, h0.z + r.v0.z / 2.0f};
    }
    // bond vectors target -> H and bond positions H + v / 2 (UAAtom::calculate_sch, uaorder.rs:375-397)
    const V3P v = v3p_to(target, h, pp);
    const V3P b = {h.x + v.x / 2.0f, h.y + v.y / 2.0f, h.z + v.z / 2.0f};
    if (kind == GORDER_UA_CH2) {
        r.v0 = v3p_lane0(v); r.b0 = v3p_lane0(b);
        r.v1 = v3p_lane1(v); r.b1 = v3p_lane1(b);
    } else {
        r.v1 = v3p_lane0(v); r.b1 = v3p_lane0(b);
        r.v2 = v3p_lane1(v); r.b2 = v3p_lane1(b);
    }
    r.bad = 0;
    slow = ps.slow || pp.slow();
    return r;
}

// ---- GORDER_FLAG_UA_FAST_NORMALISE: the same constructions with tolerance-bounded arithmetic ---------------------------
// Opt-in (include/gorder_hip.h).  The exact path above spends most of its instructions on being the reference's bits:
// six normalisations by correctly rounded square root and division (46 instructions each as pairs), select chains for
// the periodic shifts.  Here
//  * a / |a| is a * rsqrt(|a|^2) with |a|^2 by fused multiply-adds and rsqrt by an integer seed and three Newton steps
//    (every step an IEEE mul / fma: the oracle's FAST mode restates it operation for operation, so device and oracle sums
//    stay EQUAL; relative error ~1e-7, the reference's own two roundings leave 6e-8);
//  * the axis that is already a unit vector is not normalised again (Unit::new_normalize(rot_axis), uaorder.rs:990-1003);
//  * the hydrogen is target + dir * (rsqrt * 0.109) by one fma per component;
//  * minimum image and wrap are d - L * rint(d / L) and x - L * floor(x / L) with 1 / L from k_inv_box: for shifts of
//    at most one box length the same values as the reference's loops except AT the boundaries (|d| = L / 2, x = L) and
//    where d / L rounds across one; more than one box length (|k| > 1) goes to the literal-loop evaluation like before;
//  * rotations by Rodrigues' formula, v c + (u x v) s [+ u (u.v)(1 - c)], instead of nalgebra's rotation matrix — the
//    axis is perpendicular to the rotated vector by construction in all but the second methyl rotation;
//  * the C -> H vector is taken from the hydrogen BEFORE it is wrapped, (target + dir r) - target, not as the minimum
//    image of the wrapped hydrogen (the same vector; the reference's form loses the last bits of it when the hydrogen
//    lands across a box face), and the wrapped hydrogen — consumed only through the bond position of ordermaps and
//    geometry selections — is not computed at all when neither is on (POS = false).
// What it costs in fidelity is measured, not assumed: tools/ua_fast_fidelity.py (fraction of samples that move by a tick
// against the libm oracle, fraction of bond positions that change ordermap tile) -> profiles/r04_ua_fast_fidelity.json.
__device__ __forceinline__ float ua_fast_rsqrt(float x) {
    float y = __int_as_float(0x5f375a86 - (__float_as_int(x) >> 1));
    const float hx = 0.5f * x;
    y = y * __builtin_fmaf(-(hx * y), y, 1.5f);
    y = y * __builtin_fmaf(-(hx * y), y, 1.5f);
    y = y * __builtin_fmaf(-(hx * y), y, 1.5f);
    return y;
}
struct PbcFast {
    V3 box, inv;
    bool pbc;
    bool slow = false;
    __device__ __forceinline__ float mi1(float d, float L, float iL) {
        if (!pbc) return d;
        const float k = __builtin_rintf(d * iL);
        slow = slow || (__builtin_fabsf(k) > 1.0f);
        return __builtin_fmaf(-L, k, d);
    }
    __device__ __forceinline__ float wr1(float x, float L, float iL) {
        if (!pbc) return x;
        const float k = __builtin_floorf(x * iL);
        slow = slow || (__builtin_fabsf(k) > 1.0f);
        return __builtin_fmaf(-L, k, x);
    }
    __device__ __forceinline__ V3 to(V3 p1, V3 p2) {
        return {mi1(p2.x - p1.x, box.x, inv.x), mi1(p2.y - p1.y, box.y, inv.y), mi1(p2.z - p1.z, box.z, inv.z)};
    }
    // 1 / |a|; |a|^2 outside [2^-40, 2^40] (zero, inf, NaN included) raises `slow`
    __device__ __forceinline__ float rnorm(V3 a) {
        const float s2 = __builtin_fmaf(a.z, a.z, __builtin_fmaf(a.y, a.y, a.x * a.x));
        slow = slow || !(s2 >= 0x1p-40f && s2 <= 0x1p+40f);
        return ua_fast_rsqrt(s2);
    }
    __device__ __forceinline__ V3 unit(V3 a) { const float r = rnorm(a); return {a.x * r, a.y * r, a.z * r}; }
    // target + dir / |dir| * BOND_LENGTH, NOT wrapped
    __device__ __forceinline__ V3 shift(V3 t, V3 dir) {
        const float r = rnorm(dir) * 0.109f;
        return {__builtin_fmaf(dir.x, r, t.x), __builtin_fmaf(dir.y, r, t.y), __builtin_fmaf(dir.z, r, t.z)};
    }
    __device__ __forceinline__ V3 wrap(V3 h) { return {wr1(h.x, box.x, inv.x), wr1(h.y, box.y, inv.y), wr1(h.z, box.z, inv.z)}; }
};
// v rotated about the unit axis u perpendicular to it: v c + (u x v) s
__device__ __forceinline__ V3 v3_rotate_perp(V3 u, float s, float c, V3 v) {
    const V3 w = v3_cross(u, v);
    return {__builtin_fmaf(w.x, s, v.x * c), __builtin_fmaf(w.y, s, v.y * c), __builtin_fmaf(w.z, s, v.z * c)};
}
// ... by +angle (lane 0) and -angle (lane 1)
__device__ __forceinline__ V3P v3p_rotate_perp_pm(V3 u, float s, float c, V3 v) {
    const V3 w = v3_cross(u, v);
    const f2 sv = f2{s, -s};
    return {f2_fma(f2_splat(w.x), sv, f2_splat(v.x * c)), f2_fma(f2_splat(w.y), sv, f2_splat(v.y * c)),
            f2_fma(f2_splat(w.z), sv, f2_splat(v.z * c))};
}
// ... about any unit axis: v c + (u x v) s + u (u.v)(1 - c)
__device__ __forceinline__ V3P v3p_rotate_rod_pm(V3 u, float s, float c, V3 v) {
    const V3 w = v3_cross(u, v);
    const float k = __builtin_fmaf(u.z, v.z, __builtin_fmaf(u.y, v.y, u.x * v.x)) * (1.0f - c);
    const f2 sv = f2{s, -s};
    return {f2_fma(f2_splat(u.x), f2_splat(k), f2_fma(f2_splat(w.x), sv, f2_splat(v.x * c))),
            f2_fma(f2_splat(u.y), f2_splat(k), f2_fma(f2_splat(w.y), sv, f2_splat(v.y * c))),
            f2_fma(f2_splat(u.z), f2_splat(k), f2_fma(f2_splat(w.z), sv, f2_splat(v.z * c)))};
}
struct PbcFast2 {       // PbcFast on pairs
    V3 box, inv;
    bool pbc;
    i2 slow2 = {0, 0};
    __device__ __forceinline__ bool slow() const { return (slow2.x | slow2.y) != 0; }
    __device__ __forceinline__ f2 mi1(f2 d, float L, float iL) {
        if (!pbc) return d;
        const f2 q = d * iL;
        const f2 k = f2{__builtin_rintf(q.x), __builtin_rintf(q.y)};
        slow2 |= __builtin_elementwise_abs(k) > f2_splat(1.0f);
        return f2_fma(f2_splat(-L), k, d);
    }
    __device__ __forceinline__ f2 wr1(f2 x, float L, float iL) {
        if (!pbc) return x;
        const f2 q = x * iL;
        const f2 k = f2{__builtin_floorf(q.x), __builtin_floorf(q.y)};
        slow2 |= __builtin_elementwise_abs(k) > f2_splat(1.0f);
        return f2_fma(f2_splat(-L), k, x);
    }
    __device__ __forceinline__ V3P to(V3 t, V3 p, V3 q) {
        return {mi1(f2{p.x, q.x} - f2_splat(t.x), box.x, inv.x), mi1(f2{p.y, q.y} - f2_splat(t.y), box.y, inv.y),
                mi1(f2{p.z, q.z} - f2_splat(t.z), box.z, inv.z)};
    }
    __device__ __forceinline__ V3P to(V3 t, V3P h) {
        return {mi1(h.x - f2_splat(t.x), box.x, inv.x), mi1(h.y - f2_splat(t.y), box.y, inv.y), mi1(h.z - f2_splat(t.z), box.z, inv.z)};
    }
    __device__ __forceinline__ f2 rnorm(V3P a) {
        const f2 s2 = f2_fma(a.z, a.z, f2_fma(a.y, a.y, a.x * a.x));
        slow2 |= ~((s2 >= f2_splat(0x1p-40f)) & (s2 <= f2_splat(0x1p+40f)));
        const i2 seed = i2{0x5f375a86, 0x5f375a86} - (__builtin_bit_cast(i2, s2) >> 1);
        f2 y = __builtin_bit_cast(f2, seed);
        const f2 hx = s2 * 0.5f;
        y = y * f2_fma(-(hx * y), y, f2_splat(1.5f));
        y = y * f2_fma(-(hx * y), y, f2_splat(1.5f));
        y = y * f2_fma(-(hx * y), y, f2_splat(1.5f));
        return y;
    }
    __device__ __forceinline__ V3P unit(V3P a) { const f2 r = rnorm(a); return {a.x * r, a.y * r, a.z * r}; }
    __device__ __forceinline__ V3P shift(V3 t, V3P dir) {
        const f2 r = rnorm(dir) * 0.109f;
        return {f2_fma(dir.x, r, f2_splat(t.x)), f2_fma(dir.y, r, f2_splat(t.y)), f2_fma(dir.z, r, f2_splat(t.z))};
    }
    __device__ __forceinline__ V3P wrap(V3P h) { return {wr1(h.x, box.x, inv.x), wr1(h.y, box.y, inv.y), wr1(h.z, box.z, inv.z)}; }
};
// every kind of carbon with the fast forms; `slow` comes back raised when the literal-loop evaluation is needed instead.
// POS: the bond positions (hydrogen wrapped into the box + half the bond vector) are consumed — ordermaps, geometry.
// (need_pos: the same at run time — the general kernel is compiled with POS and asks its arguments)
template <bool POS>
__device__ __forceinline__ UaBonds ua_carbon_fast(uint32_t kind, UaCarbon c, UaConsts e, V3 box, V3 inv, bool pbc, bool need_pos, bool &slow) {
    const V3 zero{0.0f, 0.0f, 0.0f};
    PbcFast ps{box, inv, pbc};
    PbcFast2 pp{box, inv, pbc};
    UaBonds r;
    r.v0 = r.v1 = r.v2 = r.b0 = r.b1 = r.b2 = zero;
    r.bad = 0;
    // C -> H from the unwrapped hydrogen; position = wrapped H + v / 2.  (Values in, values out: with `V3 &` parameters the
    // results of the branches below met as a phi of POINTERS and stayed in scratch.)
    auto bond_v = [&](V3 target, V3 hu) { return V3{hu.x - target.x, hu.y - target.y, hu.z - target.z}; };
    auto bond_b = [&](V3 hu, V3 v) {
        if (!(POS && need_pos)) return zero;
        const V3 h = ps.wrap(hu);
        return V3{h.x + v.x / 2.0f, h.y + v.y / 2.0f, h.z + v.z / 2.0f};
    };
    if (kind == GORDER_UA_CH2 || kind == GORDER_UA_CH3) {
        const V3 target = c.p1;
        V3P hu;                                  // CH2: hydrogens 0, 1; CH3: hydrogens 1, 2 (not wrapped)
        if (kind == GORDER_UA_CH2) {            // uaorder.rs:985-1020
            const V3P th = pp.unit(pp.to(target, c.p0, c.p2));
            const V3 th1 = v3p_lane0(th), th2 = v3p_lane1(th);
            const V3 pn = v3_cross(th2, th1);
            const V3 ra = ps.unit(V3{th1.x - th2.x, th1.y - th2.y, th1.z - th2.z});      // (not normalised a second time)
            const V3 rv = v3_cross(pn, ra);                                                // perpendicular to ra
            hu = pp.shift(target, v3p_rotate_perp_pm(ra, e.sin_half, e.cos_half, rv));
        } else {                                // CH3, uaorder.rs:947-981
            const V3P th = pp.to(target, c.p0, c.p2);
            const V3 th1 = v3p_lane0(th), th2 = v3p_lane1(th);
            const V3 ua = ps.unit(v3_cross(th2, th1));                                     // perpendicular to th1
            const V3 hv1 = v3_rotate_perp(ua, e.sin_tet, e.cos_tet, th1);
            const V3 h0 = ps.shift(target, hv1);
            r.v0 = bond_v(target, h0);
            r.b0 = bond_b(h0, r.v0);
            const V3 n1 = ps.unit(th1);
            hu = pp.shift(target, v3p_rotate_rod_pm(n1, e.sin_ch3, e.cos_ch3, hv1));
        }
        const V3P v = {hu.x - f2_splat(target.x), hu.y - f2_splat(target.y), hu.z - f2_splat(target.z)};
        V3P b = {f2_splat(0.0f), f2_splat(0.0f), f2_splat(0.0f)};
        if (POS && need_pos) { const V3P h = pp.wrap(hu); b = {h.x + v.x / 2.0f, h.y + v.y / 2.0f, h.z + v.z / 2.0f}; }
        // The pair is hydrogens (0, 1) of a methylene and (1, 2) of a methyl carbon.  As selects of VALUES: assigning
        // `r.v0, r.v1` in one branch and `r.v1, r.v2` in the other made the compiler keep the result in scratch and index
        // it by the kind (two scratch stores and loads per frame, and a wait for every load in flight behind them).
        const bool ch2 = kind == GORDER_UA_CH2;
        const V3 v_lo = v3p_lane0(v), v_hi = v3p_lane1(v), b_lo = v3p_lane0(b), b_hi = v3p_lane1(b);
        r.v0 = V3{ch2 ? v_lo.x : r.v0.x, ch2 ? v_lo.y : r.v0.y, ch2 ? v_lo.z : r.v0.z};
        r.b0 = V3{ch2 ? b_lo.x : r.b0.x, ch2 ? b_lo.y : r.b0.y, ch2 ? b_lo.z : r.b0.z};
        r.v1 = V3{ch2 ? v_hi.x : v_lo.x, ch2 ? v_hi.y : v_lo.y, ch2 ? v_hi.z : v_lo.z};
        r.b1 = V3{ch2 ? b_hi.x : b_lo.x, ch2 ? b_hi.y : b_lo.y, ch2 ? b_hi.z : b_lo.z};
        r.v2 = v_hi; r.b2 = b_hi;                  // (a methylene carbon has no third hydrogen: never read)
    } else {
        V3 target = c.p1, hu;
        if (kind == GORDER_UA_CH1_UNSAT) {      // uaorder.rs:1024-1045
            const V3 th1 = ps.to(target, c.p0), th2 = ps.to(target, c.p2);
            const float prod = (th1.x * th2.x + th1.y * th2.y) + th1.z * th2.z;
            const float n1 = v3_norm(th1), n2 = v3_norm(th2);
            float gamma = 0.0f;
            if (!(n1 == 0.0f || n2 == 0.0f)) {
                float cs = prod / (n1 * n2);
                cs = cs < -1.0f ? -1.0f : (cs > 1.0f ? 1.0f : cs);
                gamma = gm_acosf(cs);
            }
            const float ang = 3.14159265358979323846f - (gamma / 2.0f);
            const float sn = gm_sinf_0pi(ang), cs = gm_cosf(ang);
            const V3 ua = ps.unit(v3_cross(th1, th2));                                     // perpendicular to th2
            hu = ps.shift(target, ang == 0.0f ? th2 : v3_rotate_perp(ua, sn, cs, th2));
        } else {                                // CH1 saturated, uaorder.rs:1087-1104 (h1, h2, h3, target)
            target = c.p3;
            const V3 t1 = ps.unit(ps.to(target, c.p0)), t2 = ps.unit(ps.to(target, c.p1)), t3 = ps.unit(ps.to(target, c.p2));
            hu = ps.shift(target, V3{-((t1.x + t2.x) + t3.x), -((t1.y + t2.y) + t3.y), -((t1.z + t2.z) + t3.z)});
        }
        r.v0 = bond_v(target, hu);
        r.b0 = bond_b(hu, r.v0);
    }
    slow = ps.slow || pp.slow();
    return r;
}

// the literal-loop variant, kept out of line: it runs only for carbons more than 1.5 box lengths away
// from a helper
__device__ __noinline__ UaBonds ua_carbon_slow(uint32_t kind, UaCarbon c, UaConsts e, V3 box, bool pbc) {
    PbcLoop pl{box, pbc};
    return ua_carbon(kind, c, e, pl);
}

// ---- what the four tile kernels share (the contracts: the head comment) ---------------------------------------------
// Workgroups go to the 8 XCDs round-robin; the tiles of one molecule group share their atoms, so each XCD takes a
// contiguous range of (chunk, tile) pairs — a group's tiles then run next to each other behind ONE L2.  The host pads the
// grid to a multiple of 8 (ua_grid): a workgroup past the last chunk is `padding`, and the kernel returns on it.
struct UaWork { uint32_t tile_id, f_begin, f_end; bool padding; };     // [f_begin, f_end): the frames of this workgroup's chunk
__device__ __forceinline__ UaWork ua_tile_work(uint32_t n_tiles, uint32_t frame0, uint32_t frames_per_chunk, uint32_t n_frames) {
    const uint32_t per_xcd = gridDim.x / 8u, work = (blockIdx.x % 8u) * per_xcd + blockIdx.x / 8u, chunk = work / n_tiles;
    const uint32_t f_begin = frame0 + chunk * frames_per_chunk;
    return {work % n_tiles, f_begin, min(n_frames, f_begin + frames_per_chunk), (size_t)chunk * frames_per_chunk >= n_frames - frame0};
}
// the tile and this lane's carbon (all zero where !active), its number of hydrogens and the accumulator slot of the first
struct UaLane { Tile t; gorder::UaItem it; uint32_t tid, kind, gslot0; int nh; bool active; };
__device__ __forceinline__ UaLane ua_tile_lane(const Tile *tiles, const gorder::UaItem *items, const uint32_t *tile_slots, uint32_t tile_id) {
    UaLane c;
    c.t = tiles[tile_id];
    c.tid = threadIdx.x;
    c.active = c.tid < c.t.n_items;
    c.it = gorder::UaItem{};
    if (c.active) c.it = items[c.t.item0 + c.tid];
    c.kind = c.it.kind;
    c.nh = c.kind == GORDER_UA_CH3 ? 3 : (c.kind == GORDER_UA_CH2 ? 2 : 1);
    c.gslot0 = c.active ? tile_slots[c.t.slot0 + c.it.lslot0] : 0;
    return c;
}

// where frame 0 holds the carbon's four atoms (an idle lane: the tile's first atom), one frame of them, a frame's box edges
__device__ __forceinline__ void ua_sources(const float *(&src)[4], const float *xyz, const UaLane &c) {
#pragma unroll
    for (int q = 0; q < 4; q++) src[q] = xyz + ((size_t)c.t.atom0 + (c.active ? c.it.l[q] : 0u)) * 3u;
}
__device__ __forceinline__ UaCarbon ua_fetch(const float *const (&src)[4], uint32_t f, size_t fstride) {
    UaCarbon c;
    const size_t o = (size_t)f * fstride;
    c.p0 = {src[0][o], src[0][o + 1], src[0][o + 2]};
    c.p1 = {src[1][o], src[1][o + 1], src[1][o + 2]};
    c.p2 = {src[2][o], src[2][o + 1], src[2][o + 2]};
    c.p3 = {src[3][o], src[3][o + 1], src[3][o + 2]};
    return c;
}
__device__ __forceinline__ V3 ua_box_edges(const float *box9, uint32_t f) {
    const float *b = box9 + 9 * (size_t)f;
    return {b[0], b[4], b[8]};
}

// the atoms are checked in index order (uaorder.rs:400-437 via get_position of each helper); the smallest key wins
// (one test for the four first — two unordered compares —, the chain only where it fires)
__device__ __forceinline__ void ua_raise_undefined(uint32_t *err, const UaCarbon &c, uint32_t f, uint32_t gslot0, uint32_t mol) {
    if (__builtin_expect((int)__builtin_isunordered(c.p0.x, c.p1.x) | (int)__builtin_isunordered(c.p2.x, c.p3.x), 0)) {
        if (c.p0.x != c.p0.x) raise_error(err, GORDER_ERR_UNDEFINED_POSITION, f, kStageTypes, gslot0, 1, mol, 0);
        else if (c.p1.x != c.p1.x) raise_error(err, GORDER_ERR_UNDEFINED_POSITION, f, kStageTypes, gslot0, 1, mol, 1);
        else if (c.p2.x != c.p2.x) raise_error(err, GORDER_ERR_UNDEFINED_POSITION, f, kStageTypes, gslot0, 1, mol, 2);
        else if (c.p3.x != c.p3.x) raise_error(err, GORDER_ERR_UNDEFINED_POSITION, f, kStageTypes, gslot0, 1, mol, 3);
    }
}

// the reference's bits: the two common kinds by paired arithmetic, the others one by one; a construction that raised `slow`
// is done again by the literal loops, which may give up (`bad`)
__device__ __forceinline__ UaBonds ua_carbon_exact(uint32_t kind, UaCarbon c, UaConsts uc, V3 box, bool pbc, int &bad) {
    bool slow = false;
    UaBonds ub;
    if (kind == GORDER_UA_CH2 || kind == GORDER_UA_CH3) {
        ub = ua_carbon_pairs(kind, c, uc, box, pbc, slow);
    } else {
        PbcStep ps{box, pbc};
        ub = ua_carbon(kind, c, uc, ps);
        slow = ps.slow;
    }
    if (__builtin_expect(slow, 0)) {
        ub = ua_carbon_slow(kind, c, uc, box, pbc);
        bad |= ub.bad;
    }
    return ub;
}

// The tick of one virtual hydrogen.  axis_allowed: the normal is static and along an axis; with |v|^2 in the guarded range the
// squared cosine then comes from the division core, no clamp (gm_sch_axis has the argument); anything else takes the general
// routine with the normal (nx, ny, nz), its norm n2 and squared norm n2sq.  The axis component is taken by a unit vector (ax,
// ay, az) in scalar registers — x * 1 + y * 0 + z * 0, exact for the finite components this branch holds (|v|^2 <= 2^40), the
// sign of a zero aside, which the square drops —: as selects the two lane masks `axis == 0`, `axis == 1` lived in spilled scalar
// registers and were read back (v_readlane) for every hydrogen.
template <bool ACOS_COS>
__device__ __forceinline__ int ua_tick(const V3 v, bool axis_allowed, float ax, float ay, float az, float nx, float ny, float nz, float n2, float n2sq) {
    float sch;
    const float s2 = (v.x * v.x + v.y * v.y) + v.z * v.z;
    if (!ACOS_COS && axis_allowed && s2 >= 0x1p-40f && s2 <= 0x1p+40f) {
        const float prod = __builtin_fmaf(v.z, az, __builtin_fmaf(v.y, ay, v.x * ax));
        sch = (1.5f * gm_div_core(prod * prod, s2)) - 0.5f;
    } else {
        sch = gm_calc_sch<ACOS_COS>(v.x, v.y, v.z, nx, ny, nz, n2, n2sq);
    }
    return gm_tick(sch);
}

// a lane's ordinary sums, per hydrogen: all samples and those of the upper leaflet
struct UaAcc {
    long long s_tot[3] = {0, 0, 0}, s_up[3] = {0, 0, 0};
    uint32_t n_tot[3] = {0, 0, 0}, n_up[3] = {0, 0, 0};
};
// the epilogue: the lanes' sums per local slot in LDS, then one global atomic per (slot, field) on the block's replica
__device__ __forceinline__ void ua_fold_sums(unsigned long long *rep, uint32_t n_rep, uint32_t n_acc, const Tile t, const uint32_t *tile_slots, bool active,
                                             uint32_t lslot0, uint32_t tid, const UaAcc acc, unsigned long long *l_s, uint32_t *l_n /* [2][kUaLS] each */) {
    if (active) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (!acc.n_tot[k]) continue;
            atomicAdd(&l_s[lslot0 + k], (unsigned long long)acc.s_tot[k]);
            atomicAdd(&l_n[lslot0 + k], acc.n_tot[k]);
            if (acc.n_up[k]) {
                atomicAdd(&l_s[kUaLS + lslot0 + k], (unsigned long long)acc.s_up[k]);
                atomicAdd(&l_n[kUaLS + lslot0 + k], acc.n_up[k]);
            }
        }
    }
    __syncthreads();
    unsigned long long *accp = rep + (size_t)(blockIdx.x % n_rep) * 4u * n_acc;
    for (uint32_t ls = tid; ls < t.n_slots; ls += kBlock) {
        if (!l_n[ls]) continue;
        const uint32_t slot = tile_slots[t.slot0 + ls];
        atomicAdd(&accp[slot], l_s[ls]);
        atomicAdd(&accp[2u * n_acc + slot], (unsigned long long)l_n[ls]);
        if (l_n[kUaLS + ls]) {
            atomicAdd(&accp[n_acc + slot], l_s[kUaLS + ls]);
            atomicAdd(&accp[3u * n_acc + slot], (unsigned long long)l_n[kUaLS + ls]);
        }
    }
}

// the streams and tables of every united-atom tile kernel and body, behind its argument structs (#undef: kernels_ua_samples.h, the last user)
#define GORDER_UA_KERNEL_ARGS                                                                                              \
    const float *__restrict__ xyz, const float *__restrict__ box9, const uint8_t *__restrict__ aflags,                        \
        const uint32_t *__restrict__ arow, const Tile *__restrict__ tiles, const gorder::UaItem *__restrict__ items,          \
        const uint32_t *__restrict__ tile_slots, uint32_t n_tiles

// MODE 0: order parameters only; 1: + staged ordermap samples, nothing else (no geometry selection, timewise rows or
// per-molecule normals — the common ordermap run, and a much smaller kernel); 2: every extra; 3: per-frame rows, nothing else
// FAST: GORDER_FLAG_UA_FAST_NORMALISE (ua_carbon_fast; inv_box holds 1 / box edge per frame).  PREFETCH: the next frame's
// atoms are requested before this frame's arithmetic (the fast arithmetic no longer hides the gather's latency by itself;
// the exact path is bound by its arithmetic and keeps its registers).
// The body is shared by k_ua_extras (the exact path) and k_ua_extras_fast.
// (Measured and NOT kept in round 4: the tile's needed atoms staged in LDS per frame by coalesced loads, two buffers, one
// barrier per frame — every test green, 0.36 -> 0.47 ms per 3 000 frames for the exact path and 0.30 -> 0.35 for the fast
// one: a frame is only ~300 instructions per lane, a barrier and seventeen LDS operations per frame cost more than the
// gather they replace.)
// (Also measured and not kept: periodic boundaries as a template parameter, so that the `if (!pbc)` in front of every
// minimum image and wrap disappears and the x / y / z chains interleave — 0.284 -> 0.279 ms for the fast path, the exact
// path with maps 0.42 -> 0.49: twice the kernels for nothing.)
template <bool ACOS_COS, int MODE, bool FAST, bool PREFETCH>
__device__ __forceinline__ void ua_extras_body(FrameArgs a_in, ExtraArgs e, GORDER_UA_KERNEL_ARGS, const float *__restrict__ inv_box) {
    constexpr bool EXTRAS = MODE != 0, GENERAL = MODE >= 2, FULL = MODE == 2, MAPS_POSSIBLE = MODE == 1 || MODE == 2;
    constexpr uint32_t LS = kUaLS;
    __shared__ unsigned long long l_s[2 * LS];
    __shared__ uint32_t l_n[2 * LS];
    __shared__ int l_tw[GENERAL ? 3 * LS : 1];
    __shared__ uint32_t l_twn[GENERAL ? 3 * LS : 1];
    FrameArgs a = a_in;
    a.xyz = xyz; a.box9 = box9; a.aflags = aflags; a.arow = arow;
    // ua_tile_work, ua_tile_lane and, further down, ua_sources, ua_raise_undefined and ua_carbon_exact restated: the head comment has the reason
    const uint32_t per_xcd = gridDim.x / 8u, work = (blockIdx.x % 8u) * per_xcd + blockIdx.x / 8u;
    const uint32_t tile_id = work % n_tiles, chunk = work / n_tiles;
    if ((size_t)chunk * a_in.frames_per_chunk >= a_in.n_frames - a_in.frame0) return;    // padding workgroup
    const Tile t = tiles[tile_id];
    const uint32_t tid = threadIdx.x;
    const bool active = tid < t.n_items;
    gorder::UaItem it{};
    if (active) it = items[t.item0 + tid];
    const uint32_t kind = it.kind;
    const int nh = kind == GORDER_UA_CH3 ? 3 : (kind == GORDER_UA_CH2 ? 2 : 1);
    const uint32_t gslot0 = active ? tile_slots[t.slot0 + it.lslot0] : 0;
    const uint32_t f_begin = a.frame0 + chunk * a.frames_per_chunk;
    const uint32_t f_end = min(a.n_frames, f_begin + a.frames_per_chunk);
    const size_t fstride = (size_t)a.n_atoms * 3u;
    // Per-frame rows: when the lanes of every DPP ROW (16 lanes) of the tile hold carbons of ONE kind and slot (the tiles are
    // cut from groups of 64 molecules ordered so that a wave is 4 slots x 16 molecules: the normal case) a frame's sums per
    // slot are sums over a row — DPP adds, then the row's last lane sends them to the rows —: no LDS atomic per hydrogen
    // (two to four, served one lane per cycle) and no barriers per frame.  Otherwise the LDS partials of extras_add /
    // extras_flush_tw.
    __shared__ uint32_t l_mixed;
    if (GENERAL && tid == 0) l_mixed = 0u;
    if (GENERAL)
        for (uint32_t k = tid; k < 3 * LS; k += kBlock) { l_tw[k] = 0; l_twn[k] = 0; }
    for (uint32_t k = tid; k < 2 * LS; k += kBlock) { l_s[k] = 0; l_n[k] = 0; }
    __syncthreads();
    uint32_t row_slot0 = 0;      // the row's first lane: its first slot and its number of hydrogens (active lanes come first)
    int row_nh = 0;
    if (GENERAL) {
        const uint32_t key = active ? ((uint32_t)it.lslot0 << 8) | kind : 0xffffffffu;
        const int lane0 = (int)(tid & 63u & ~15u);
        const uint32_t first = (uint32_t)__shfl((int)key, lane0, 64);
        row_slot0 = (uint32_t)__shfl((int)gslot0, lane0, 64);
        row_nh = first == 0xffffffffu ? 0 : __shfl(nh, lane0, 64);
        if (!__all(!active || key == first)) l_mixed = 1u;
    }
    __syncthreads();
    const bool tw_waves = GENERAL && e.tw && l_mixed == 0u;                     // (uniform over the workgroup)
    const int nh_wave = GENERAL ? (__any(row_nh > 2) ? 3 : (__any(row_nh > 1) ? 2 : 1)) : 0;      // (uniform over the wave)
    // all four rows of the wave hold the same slot (a slot per wave: the lane order of per-frame rows alone): one lane of the
    // wave sends the sums instead of one per row
    const bool wave_one_slot = GENERAL && __all(row_nh == 0 || (row_slot0 == (uint32_t)__builtin_amdgcn_readfirstlane((int)row_slot0) &&
                                                                  row_nh == __builtin_amdgcn_readfirstlane(row_nh)));
    UaAcc acc;
    int bad = 0;
    const bool pbc = a.pbc != 0;
    const UaConsts uc{e.sin_tet, e.cos_tet, e.sin_ch3, e.cos_ch3, e.sin_half, e.cos_half};
    const float axis_x = e.axis == 0 ? 1.0f : 0.0f, axis_y = e.axis == 1 ? 1.0f : 0.0f, axis_z = e.axis == 2 ? 1.0f : 0.0f;
    unsigned long long *rec_row = nullptr;
    uint32_t rec_n = 0;
    const size_t rec_plane = (size_t)kBlock * e.rec_stride;      // hydrogen k of the same lanes: k planes further
    if (MAPS_POSSIBLE && (!GENERAL || e.map_rec) && active) {
        const uint32_t run = e.item_run[t.item0 + tid], tid0 = run >> 16;
        rec_n = run & 0xffffu;
        rec_row = e.map_rec + ((size_t)tile_id * 3u * kBlock + tid0) * e.rec_stride + (tid - tid0);
    }
    const float *src[4];
#pragma unroll
    for (int q = 0; q < 4; q++) src[q] = xyz + ((size_t)t.atom0 + (active ? it.l[q] : 0u)) * 3u;
    auto fetch = [&](uint32_t f) { return ua_fetch(src, f, fstride); };
    // PREFETCH: the next frame's four atoms are asked for before this frame's arithmetic, by EVERY lane (idle lanes point
    // at the tile's first atom) and without a branch (the last frame asks for itself again): inside `if (active)` or
    // behind `f + 1 < f_end` the loaded registers are copied into the loop-carried ones at the end of the conditional
    // block, and the wait for the loads lands right behind them — a prefetch that hides nothing.
    // The frame's box lengths (and their reciprocals): scalar loads at the top of the frame.
    auto fetch_box = [&](uint32_t f, V3 &bx, V3 &inv) {
        bx = {1.0f, 1.0f, 1.0f};
        inv = {1.0f, 1.0f, 1.0f};
        if (pbc) {
            if (FAST) {         // (k_inv_box's record of the frame: one scalar load)
                const float4 *ib = reinterpret_cast<const float4 *>(inv_box) + 2 * (size_t)f;
                const float4 lo = ib[0], hi = ib[1];
                bx = {lo.x, lo.y, lo.z};
                inv = {hi.x, hi.y, hi.z};
            } else {
                bx = ua_box_edges(a.box9, f);
            }
        }
    };
    auto fetch_flag = [&](uint32_t f) { return a.aflags[(size_t)a.arow[f] * a.n_mol_total + (active ? it.mol : 0u)]; };
    UaCarbon c_next{};
    uint8_t lf_next = 0;
    if (PREFETCH && f_begin < f_end) {
        c_next = fetch(f_begin);
        if (a.leaflets) lf_next = fetch_flag(f_begin);
    }
    for (uint32_t f = f_begin; f < f_end; f++) {
        int tw_s[3] = {0, 0, 0}, tw_sl[3] = {0, 0, 0}, tw_n[3] = {0, 0, 0};      // tw_waves: this lane's ticks, lower-leaflet ticks, counts (all | lower << 16)
        UaCarbon c_now{};
        V3 bx3{1.0f, 1.0f, 1.0f}, inv3{1.0f, 1.0f, 1.0f};
        if (PREFETCH) {
            c_now = c_next;
            const uint32_t fn = f + 1 < f_end ? f + 1 : f;
            c_next = fetch(fn);
            fetch_box(f, bx3, inv3);        // (scalar loads; a frame ahead they bought nothing and cost six scalar registers)
        } else {
            fetch_box(f, bx3, inv3);
        }
        // (the molecule's leaflet flag: a frame ahead with the atoms — its load is waited for where the flag is first
        // looked at, which the compiler puts right behind the load —, or up here)
        uint8_t lf_raw = 0;
        if (PREFETCH) {
            lf_raw = lf_next;
            if (a.leaflets) lf_next = fetch_flag(f + 1 < f_end ? f + 1 : f);
        } else if (a.leaflets) {
            lf_raw = fetch_flag(f);
        }
        if (active) {
            const UaCarbon c = PREFETCH ? c_now : fetch(f);
            if (__builtin_expect((int)__builtin_isunordered(c.p0.x, c.p1.x) | (int)__builtin_isunordered(c.p2.x, c.p3.x), 0)) {
                if (c.p0.x != c.p0.x) raise_error(a.err, GORDER_ERR_UNDEFINED_POSITION, f, kStageTypes, gslot0, 1, it.mol, 0);
                else if (c.p1.x != c.p1.x) raise_error(a.err, GORDER_ERR_UNDEFINED_POSITION, f, kStageTypes, gslot0, 1, it.mol, 1);
                else if (c.p2.x != c.p2.x) raise_error(a.err, GORDER_ERR_UNDEFINED_POSITION, f, kStageTypes, gslot0, 1, it.mol, 2);
                else if (c.p3.x != c.p3.x) raise_error(a.err, GORDER_ERR_UNDEFINED_POSITION, f, kStageTypes, gslot0, 1, it.mol, 3);
            }
            bool slow = false;
            UaBonds ub;
            if (FAST) {
                ub = ua_carbon_fast<MAPS_POSSIBLE>(kind, c, uc, bx3, inv3, pbc, e.maps != 0 || e.geom_kind != 0, slow);
            } else if (kind == GORDER_UA_CH2 || kind == GORDER_UA_CH3) {
                ub = ua_carbon_pairs(kind, c, uc, bx3, pbc, slow);
            } else {
                PbcStep ps{bx3, pbc};
                ub = ua_carbon(kind, c, uc, ps);
                slow = ps.slow;
            }
            if (__builtin_expect(slow, 0)) {
                ub = ua_carbon_slow(kind, c, uc, bx3, pbc);
                bad |= ub.bad;
            }
            int leaflet = -1;
            if (a.leaflets) leaflet = lf_raw ? 1 : 0;
            float nrx = a.nx, nry = a.ny, nrz = a.nz, nr2 = a.n2, nr2sq = a.n2sq;
            if (FULL && e.dyn) {   // fetched for every molecule, before the geometry test (uaorder.rs:412-413)
                const float4 n = e.dyn[(size_t)f * a.n_mol_total + it.mol];
                if (n.w < 3.0f) raise_error(a.err, GORDER_ERR_DYNAMIC_NORMAL, f, kStageTypes, gslot0, 1, it.mol, (uint32_t)n.w);
                nrx = n.x; nry = n.y; nrz = n.z;
                nr2sq = (n.x * n.x + n.y * n.y) + n.z * n.z;
                nr2 = __builtin_sqrtf(nr2sq);
            }
            unsigned long long recs[3] = {kMapNoSample, kMapNoSample, kMapNoSample};
            auto sample = [&](const int k, const V3 v, const V3 b) {
                if (k >= nh) return;
                const int tick = ua_tick<ACOS_COS>(v, e.axis >= 0 && !(FULL && e.dyn), axis_x, axis_y, axis_z, nrx, nry, nrz, nr2, nr2sq);
                if (FULL) {
                    const float box[3] = {bx3.x, bx3.y, bx3.z};
                    if (e.geom_kind && !geom_inside(e, e.shapes + 8 * (size_t)f, b.x, b.y, b.z, box, pbc, bad)) return;
                }
                acc.s_tot[k] += tick;
                acc.n_tot[k] += 1;
                if (leaflet == 0) { acc.s_up[k] += tick; acc.n_up[k] += 1; }
                if (tw_waves) {
                    tw_s[k] = tick;
                    tw_sl[k] = leaflet == 1 ? tick : 0;
                    tw_n[k] = 1 | (leaflet == 1 ? 1 << 16 : 0);
                }
                if (EXTRAS)
                    extras_add<!GENERAL, !MAPS_POSSIBLE>(a, e, gslot0 + (uint32_t)k, it.lslot0 + (uint32_t)k, tick, b.x, b.y, b.z, leaflet, l_tw,
                                                         l_twn, LS, (MAPS_POSSIBLE && (!GENERAL || e.map_rec)) ? &recs[k] : nullptr, tw_waves,
                                                         FAST && !slow);
            };
            sample(0, ub.v0, ub.b0);
            sample(1, ub.v1, ub.b1);
            sample(2, ub.v2, ub.b2);
            if (MAPS_POSSIBLE && (!GENERAL || e.map_rec)) {   // one word per hydrogen this carbon has, into its run's piece
                unsigned long long *row = rec_row + (size_t)(f - e.rec_frame0) * rec_n;
                row[0] = recs[0];
                if (nh > 1) row[rec_plane] = recs[1];
                if (nh > 2) row[2u * rec_plane] = recs[2];
            }
        }
        if (tw_waves) {             // every lane of the wave is here
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (k >= nh_wave) break;                            // (uniform)
                int s_all = row_sum(tw_s[k]), s_low = row_sum(tw_sl[k]), n = row_sum(tw_n[k]);
                if (wave_one_slot) { s_all = rows_to_wave(s_all); s_low = rows_to_wave(s_low); n = rows_to_wave(n); }
                const uint32_t n_all = (uint32_t)n & 0xffffu, n_low = (uint32_t)n >> 16;
                const bool sender = wave_one_slot ? (tid & 63u) == 63u : (tid & 15u) == 15u;
                // (a wave that ends inside the tile: its last rows are idle, the wave's slot is that of its first lane)
                const int send_nh = wave_one_slot ? __builtin_amdgcn_readfirstlane(row_nh) : row_nh;
                const uint32_t send_slot0 = wave_one_slot ? (uint32_t)__builtin_amdgcn_readfirstlane((int)row_slot0) : row_slot0;
                if (sender && k < send_nh && n_all) {
                    const size_t row = ((size_t)e.tw_row0 + f) * 3u * a.n_acc;
                    const uint32_t slot = send_slot0 + (uint32_t)k;
                    atomicAdd(&e.tw_sums[row + slot], (unsigned long long)(long long)s_all);
                    atomicAdd(&e.tw_cnts[row + slot], (unsigned long long)n_all);
                    if (a.leaflets) {
                        const uint32_t n_up_w = n_all - n_low;
                        if (n_up_w) {
                            atomicAdd(&e.tw_sums[row + (size_t)a.n_acc + slot], (unsigned long long)(long long)(s_all - s_low));
                            atomicAdd(&e.tw_cnts[row + (size_t)a.n_acc + slot], (unsigned long long)n_up_w);
                        }
                        // (the lower leaflet's row: total - upper, gorder_hip_timewise)
                    }
                }
            }
        } else if (GENERAL && e.tw) {
            __syncthreads();
            extras_flush_tw(a, e, tile_slots + t.slot0, t.n_slots, f, l_tw, l_twn, LS);
            __syncthreads();
        }
    }
    if (bad) raise_box_range(a.err, f_begin);
    // (l_s, l_n: zeroed before the first barrier of this body and touched by nothing since)
    ua_fold_sums(a.rep, a.n_rep, a.n_acc, t, tile_slots, active, it.lslot0, tid, acc, l_s, l_n);
}

#ifndef GORDER_UA_PREFETCH
#define GORDER_UA_PREFETCH 0        // the exact kernel is bound by VALU issue: a frame ahead buys nothing there (measured, round 4)
#endif
template <bool ACOS_COS, int MODE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_ua_extras(FrameArgs a_in, ExtraArgs e, GORDER_UA_KERNEL_ARGS,
                                                                                                 const float *__restrict__ inv_box) {
    ua_extras_body<ACOS_COS, MODE, false, GORDER_UA_PREFETCH != 0>(a_in, e, xyz, box9, aflags, arow, tiles, items, tile_slots, n_tiles, inv_box);
}
// GORDER_FLAG_UA_FAST_NORMALISE (the default cosine only)
#ifndef GORDER_UA_FAST_WAVES
#define GORDER_UA_FAST_WAVES 4      // (3, 5 and 6 waves per SIMD measured in round 4: see DESIGN)
#endif
template <int MODE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(GORDER_UA_FAST_WAVES, GORDER_UA_FAST_WAVES))) void k_ua_extras_fast(
    FrameArgs a_in, ExtraArgs e, GORDER_UA_KERNEL_ARGS, const float *__restrict__ inv_box) {
    ua_extras_body<false, MODE, true, true>(a_in, e, xyz, box9, aflags, arow, tiles, items, tile_slots, n_tiles, inv_box);
}

}  // namespace
