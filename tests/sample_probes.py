"""Bond vectors that sit on the edges of the sample arithmetic, and that arithmetic stated literally.

Plain numpy, no GPU, no ctypes, nothing of this project imported (the united-atom part at the end takes the lipid it is
handed).  Three parts:

(a) `literal_tick`: the default squared-cosine sample and its tick, operation for operation as gm_calc_sch<false> and
    gm_tick (gorder_amd/csrc/gm_math.h) state them, every float32 operation rounded on its own; `literal_vector`: p2 - p1
    and the reference's minimum-image loops.  A third witness next to the kernels and the oracle's C.  The keyword
    arguments plant the mutants the CPU test must see.
(b) probe families, every probe labelled with the rule it targets:
      guards     |v|^2 = (vx^2 + vy^2) + vz^2 ON 2^-40 and 2^40 and on the floats one and two either side, along the
                 normal, across it, oblique, with a numerator below 2^-103 and with a denormal numerator;
      norm       |v| = 0 three ways, |v|^2 denormal, |v|^2 infinite from finite components, |v|^2 beyond the upper guard;
      products   two squared norms, each finite and not zero, whose product underflows to 0 or overflows to inf;
      images     |dx| at L/2, L, 3L/2, 5L/2, one float either side of each, and 4.5 L, per dimension and combined;
      nonfinite  +inf or -inf in the y or z coordinate of one atom (NaN in x is the undefined-position error: not here);
      ordinary   bonds of 0.1 - 0.5 nm, so that every slot and every frame also holds everyday samples.
(c) `probe_system`: M molecules of B bonds each, one bond per accumulator slot and molecule, the probes rotating over
    the slots frame by frame; every molecule has a head that is NOT a probe atom (leaflets, membrane group, clouds and
    reference groups are made of heads only, so no side and no centre depends on a probe).
"""
from __future__ import annotations

import dataclasses

import numpy as np

F = np.float32
INF = F(np.inf)
GUARD_LO, GUARD_HI = F(2.0 ** -40), F(2.0 ** 40)
MI_MAX_ITER = 8
INT_MIN = -2 ** 31
N_FRAMES = 9                       # two stages of four frames and a partial one


def step(x, n: int) -> np.float32:
    """The float `n` places above (below for n < 0) x."""
    x = F(x)
    for _ in range(abs(int(n))):
        x = np.nextafter(x, INF if n > 0 else -INF)
    return F(x)


# ---- (a) the literal statements ---------------------------------------------------------------------------------------
def dot3(a, b) -> np.float32:
    """nalgebra's dot of two 3-vectors: (a0 b0 + a1 b1) + a2 b2 — the products with 0 are kept (0 * inf is NaN)."""
    with np.errstate(all="ignore"):
        return F(F(F(F(a[0]) * F(b[0])) + F(F(a[1]) * F(b[1]))) + F(F(a[2]) * F(b[2])))


def norm2(v) -> np.float32:
    return dot3(v, v)


def min_image_literal(dx, L, shifts=MI_MAX_ITER) -> np.float32:
    """groan_rs' loops: while dx > L/2: dx -= L; while dx < -L/2: dx += L.  `shifts`: at most so many turns of each loop
    (1: the mutant without a second shift)."""
    dx, L = F(dx), F(L)
    half = F(L / F(2))
    with np.errstate(all="ignore"):
        it = 0
        while dx > half and it < shifts:
            dx = F(dx - L)
            it += 1
        it = 0
        while dx < -half and it < shifts:
            dx = F(dx + L)
            it += 1
    return dx


def literal_vector(p1, p2, box=None, shifts=MI_MAX_ITER) -> np.ndarray:
    with np.errstate(all="ignore"):
        v = [F(F(p2[d]) - F(p1[d])) for d in range(3)]
    if box is not None:
        v = [min_image_literal(v[d], box[d], shifts) for d in range(3)]
    return np.array(v, dtype=F)


def slow_literal(d, box) -> bool:
    """gm_min_image_step's `slow`: one shift per dimension was not enough."""
    for k in range(3):
        L, half = F(box[k]), F(F(box[k]) / F(2))
        r = F(d[k] - np.copysign(L, d[k])) if abs(d[k]) > half else F(d[k])
        if abs(r) > half:
            return True
    return False


def slow_magnitude(d, box) -> bool:
    """compute_core's shortcut: min(Lx - |dx|, Ly - |dy|, Lz - |dz|) < 0."""
    return bool(min(F(F(box[k]) - F(abs(d[k]))) for k in range(3)) < 0)


def literal_sch(v, n, zero_norm_nan=False) -> np.float32:
    """gm_calc_sch<false>: q = (v.n)^2 / (|v|^2 |n|^2), clamped at 1 (NaN passes), 1 where a squared norm is 0."""
    with np.errstate(all="ignore"):
        s2, n2sq, prod = norm2(v), norm2(n), dot3(v, n)
        q = F(F(prod * prod) / F(s2 * n2sq))
        if q > 1:
            q = F(1.0)
        if (s2 == 0 or n2sq == 0) and not zero_norm_nan:
            q = F(1.0)
        return F(F(F(1.5) * q) - F(0.5))


def literal_round(s, nan_tick=0) -> int:
    """gm_tick: round-half-away of f64(S) * 1e6; NaN -> 0 (Rust's `as i64`, order.rs:21-26)."""
    t = np.float64(F(s)) * 1000000.0
    if t != t:
        return nan_tick
    return int(np.trunc(t + np.copysign(0.5, t)))


def literal_tick(v, n, nan_tick=0, zero_norm_nan=False, guard=None) -> int:
    """The tick of bond vector v against normal n.  The keywords are the planted mutants: `nan_tick` what a NaN sample
    becomes, `zero_norm_nan` drops the zero-norm rule, `guard` = (lo, hi) states the fast path WITHOUT its fallback — a
    sample whose |v|^2 lies outside [lo, hi] is left as the first pass wrote it, which is not its tick (here: INT_MIN)."""
    if guard is not None:
        s2 = norm2(v)
        if not (s2 >= guard[0] and s2 <= guard[1]):
            return INT_MIN
    return literal_round(literal_sch(v, n, zero_norm_nan), nan_tick)


def axis_normal(axis) -> np.ndarray:
    n = np.zeros(3, dtype=F)
    n[axis] = 1
    return n


# ---- (b) probes ---------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Probe:
    family: str
    rule: str                       # the rule this probe targets, in words
    p1: np.ndarray
    p2: np.ndarray
    s2: object = None               # the float |v|^2 must BE (None: not fitted)
    where: object = None            # guards: floats from the guard (< 0 below); images: (place in L, floats off) per dimension
    outside: object = None          # |v|^2 lies outside [2^-40, 2^40]: the fast path must hand the sample over
    slow: object = None             # images: (literal `slow`, magnitude-form `slow`) as the label says, not as computed


def _fit(target, free, fixed, reach=160):
    """A vector whose literal |v|^2 IS `target`: components `fixed` {k: value} as given, the (one or two) `free` ones
    = {k: weight} near weight * sqrt(target), scanned over the floats around until the sum lands.  None if none does."""
    target = F(target)
    root = float(np.sqrt(np.float64(target)))
    ks = list(free)
    grids = []
    for k in ks:
        x0 = F(free[k] * root)
        bits = int(x0.view(np.int32))
        grids.append(np.arange(bits - reach, bits + reach + 1, dtype=np.int64).astype(np.int32).view(F))
    comp = [None, None, None]
    for k, val in fixed.items():
        comp[k] = np.array(F(val))
    if len(ks) == 1:
        comp[ks[0]] = grids[0]
    else:
        comp[ks[0]], comp[ks[1]] = grids[0][:, None], grids[1][None, :]
    with np.errstate(all="ignore"):
        sq = [(c * c).astype(F) for c in comp]
        s2 = ((sq[0] + sq[1]).astype(F) + sq[2]).astype(F)
    hit = np.argwhere(np.atleast_1d(s2) == target)
    if not hit.size:
        return None
    h = hit[len(hit) // 2]
    v = np.zeros(3, dtype=F)
    for k, val in fixed.items():
        v[k] = val
    if len(ks) == 1:
        v[ks[0]] = grids[0][h[0]]
    else:
        v[ks[0]], v[ks[1]] = grids[0][h[0]], grids[1][h[1]]
    assert norm2(v) == target
    return v


GUARD_STEPS = (-2, -1, 0, 1, 2)
ORIENTATIONS = ("along", "across", "oblique", "tiny numerator", "denormal numerator")


def guard_probes(axis, upper):
    """Around 2^-40 (`upper`: 2^40): for each float -2 .. +2 places from the guard a bond in each orientation whose
    |v|^2 IS that float.  Along the normal only the squares of floats can be met: every other float (0 and +-2)."""
    g = GUARD_HI if upper else GUARD_LO
    a, b = (axis + 1) % 3, (axis + 2) % 3
    out = []
    for k in GUARD_STEPS:
        t = step(g, k)
        outside = bool(t > g) if upper else bool(t < g)
        for o in ORIENTATIONS:
            if o == "along":
                v = _fit(t, {axis: 1.0}, {a: 0.0, b: 0.0}, reach=8)
                if v is None:
                    assert k % 2, "the square of a float meets every other float around a power of four"
                    continue
            elif o == "across":
                v = _fit(t, {a: 0.8, b: 0.6}, {axis: 0.0})
            elif o == "oblique":
                # (a fixed third square that falls half way between two floats of the sum makes every sum a tie, and
                # ties go to even: only every other float is met — take the next weight then)
                fits = (_fit(t, {a: 0.8 * np.sqrt(1 - w * w), axis: 0.6 * np.sqrt(1 - w * w)}, {b: F(w * np.sqrt(np.float64(t)))})
                        for w in (0.48, 0.47, 0.46, 0.45, 0.44, 0.43))
                v = next((x for x in fits if x is not None), None)
            elif o == "tiny numerator":         # prod^2 = 2^-120 < 2^-103, a normal float
                v = _fit(t, {a: 0.8, b: 0.6}, {axis: F(2.0 ** -60)})
            else:                                # prod^2 = 2^-140: a denormal
                v = _fit(t, {a: 0.8, b: 0.6}, {axis: F(2.0 ** -70)})
            assert v is not None, f"no bond {o} at {k} floats from 2^{40 if upper else -40}"
            out.append(Probe("guard", f"{'upper' if upper else 'lower'} guard {k:+d}, {o}", np.zeros(3, dtype=F), v,
                             s2=t, where=k, outside=outside))
    return out


def norm_probes(axis, periodic):
    a, b = (axis + 1) % 3, (axis + 2) % 3
    z = np.zeros(3, dtype=F)

    def vec(**kw):
        v = np.zeros(3, dtype=F)
        for name, val in kw.items():
            v[{"n": axis, "a": a, "b": b}[name]] = val
        return v

    spot = np.array([0.5, 0.25, 0.125], dtype=F)
    out = [Probe("norm", "zero norm: both atoms on one spot -> S = 1", spot, spot.copy(), s2=F(0), outside=True),
           Probe("norm", "zero norm: +0 against -0 -> S = 1", z, np.array([-0.0, 0.0, -0.0], dtype=F), s2=F(0), outside=True),
           Probe("norm", "zero norm: the squares underflow to 0, the dot product does not -> S = 1", z, vec(a=1e-30, n=1e-30),
                 s2=F(0), outside=True),
           Probe("norm", "denormal squared norm, oblique", z, vec(a=1e-21, n=1e-21), outside=True),
           Probe("norm", "denormal squared norm, along the normal", z, vec(n=1e-21), outside=True)]
    if not periodic:            # a far atom needs no periodic image
        out += [Probe("norm", "squared norm overflows, numerator finite -> q = 0", z, vec(a=2e19, n=1e19), s2=INF, outside=True),
                Probe("norm", "squared norm and numerator overflow -> NaN -> tick 0, counted", z, vec(n=1e25), s2=INF, outside=True),
                Probe("norm", "squared norm overflows, oblique 1e25", z, vec(a=1e25, b=-1e25, n=1e25), s2=INF, outside=True),
                Probe("norm", "squared norm 1e38: finite, far beyond the upper guard", z, vec(n=1e19), outside=True)]
    return out


def product_probes(periodic=False):
    """Bond vectors for a normal (or a lagged vector) of squared norm 2^-80 or 2^80: each squared norm finite and not 0,
    the product s2 * n2sq 0, a denormal, or inf (by Cauchy-Schwarz the
    numerator underflows with it: 0 / 0, never x / 0).  -> (probes, the normals that go with them)."""
    z = np.zeros(3, dtype=F)
    t, big = F(2.0 ** -40), F(2.0 ** 40)
    probes = [Probe("product", "s2 n2sq underflows, numerator too: 0 / 0 = NaN -> tick 0", z, np.array([t, 0, t], dtype=F)),
              Probe("product", "s2 n2sq is a denormal, the numerator too: a quotient of two denormals", z,
                    np.array([F(2.0 ** -30), 0, F(2.0 ** -30)], dtype=F)),
              Probe("product", "s2 n2sq overflows, numerator finite -> q = 0", z, np.array([big, -big, 0], dtype=F)),
              Probe("product", "s2 n2sq and numerator overflow: inf / inf = NaN -> tick 0", z, np.array([big, big, big], dtype=F))]
    normals = {"tiny": np.array([t, t, F(2.0 ** -41)], dtype=F), "huge": np.array([big, big, F(2.0 ** 39)], dtype=F)}
    if periodic:        # (a bond vector of 2^40 nm needs no periodic image; the tiny ones fit any box)
        probes = probes[:2]
    return probes, normals


IMAGE_PLACES = (0.5, 1.0, 1.5, 2.5)
BOXES = {"dyadic": (16.0, 16.0, 16.0), "three edges": (11.3, 13.7, 17.9)}


def image_probes(box):
    """p1 at the origin, p2 = the offset itself, so that p2 - p1 is exact.  Per dimension: |dx| = RN(place * L) and one
    float either side, signs alternating, and 4.5 L in both signs; then combinations over the dimensions.  `slow` is the
    LABEL — decided from the real numbers: the literal form needs its loops where |dx| - L > L/2, the magnitude form's
    condition fires where |dx| > L — and the CPU test holds the float32 statements against it."""
    box = np.array(box, dtype=F)
    rest = np.array([0.25, -0.125, 0.375], dtype=F)
    out = []

    def label(d, where):
        exact = [abs(np.float64(d[k])) / np.float64(box[k]) for k in range(3)]
        return (any(x > 1.5 for x in exact), any(x > 1.0 for x in exact))

    def offset(k, place, off, sign):
        return F(sign * step(F(np.float64(box[k]) * place), off))

    for k in range(3):
        i = 0
        for place in IMAGE_PLACES:
            for off in (-1, 0, 1):
                d = rest.copy()
                d[k] = offset(k, place, off, 1 if i % 2 == 0 else -1)
                where = [None] * 3
                where[k] = (place, off)
                out.append(Probe("image", f"|d{'xyz'[k]}| = {place} L {off:+d}", np.zeros(3, dtype=F), d, where=where, slow=label(d, where)))
                i += 1
        for sign in (1, -1):
            d = rest.copy()
            d[k] = offset(k, 4.5, 0, sign)
            where = [None] * 3
            where[k] = (4.5, 0)
            out.append(Probe("image", f"d{'xyz'[k]} = {sign * 4.5} L", np.zeros(3, dtype=F), d, where=where, slow=label(d, where)))
    combos = [((0.5, 0), (0.5, 0), (0.5, 0), (1, -1, 1)), ((1.0, 1), (0.5, -1), (1.5, 0), (-1, 1, -1)),
              ((1.0, -1), (1.0, 0), (1.0, 1), (1, 1, -1)), ((1.5, 1), (1.0, -1), (0.5, 1), (-1, -1, 1)),
              ((1.5, 0), (1.5, -1), (1.5, 0), (1, -1, -1)), ((2.5, 0), (0.5, 1), (1.0, 0), (-1, 1, 1)),
              ((0.5, -1), (2.5, 1), (1.5, 1), (1, 1, 1)), ((4.5, 0), (2.5, -1), (4.5, 0), (-1, -1, -1))]
    for *where, signs in combos:
        d = np.array([offset(k, where[k][0], where[k][1], signs[k]) for k in range(3)], dtype=F)
        out.append(Probe("image", "combined: " + ", ".join(f"{w[0]} L {w[1]:+d}" for w in where), np.zeros(3, dtype=F), d,
                         where=list(where), slow=label(d, where)))
    assert all(max(abs(np.float64(p.p2[k])) / np.float64(box[k]) for k in range(3)) < MI_MAX_ITER for p in out)
    return out


def nonfinite_probes():
    """(non-periodic) one coordinate +-inf, never x: the generic dot product's 0 * inf is NaN; every one is tick 0, counted."""
    out = []
    for which in (0, 1):
        for k in (1, 2):
            for val in (INF, -INF):
                p = [np.array([0.5, 0.25, 0.125], dtype=F), np.array([0.75, 0.5, 0.25], dtype=F)]
                p[which][k] = val
                out.append(Probe("nonfinite", f"{'-' if val < 0 else '+'}inf in {'xyz'[k]} of atom {which + 1} -> NaN -> tick 0, counted",
                                 p[0], p[1], outside=True))
    return out


def ordinary_probes(n, seed=7):
    """Bonds of 0.1 - 0.5 nm in every direction, their first atom within a nanometre of the origin."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        u = rng.normal(size=3)
        u *= (0.1 + 0.4 * rng.random()) / np.linalg.norm(u)
        p1 = rng.uniform(-1, 1, size=3).astype(F)
        out.append(Probe("ordinary", "an everyday bond", p1, (p1 + u.astype(F)).astype(F), outside=False))
    return out


def bond_probes(axis=2, box=None, products=False):
    """The probes a table can take: without a box both guards, the overflowing norms and the infinities; with one the
    lower guard and the images.  Every fourth probe is an ordinary bond."""
    periodic = box is not None
    special = guard_probes(axis, upper=False) + norm_probes(axis, periodic)
    if periodic:
        special += image_probes(box)
    else:
        special += guard_probes(axis, upper=True) + nonfinite_probes()
    if products:
        special += product_probes()[0]
    plain = ordinary_probes((len(special) + 2) // 3)
    out = []
    for i, p in enumerate(special):
        out.append(p)
        if i % 3 == 2:
            out.append(plain[i // 3])
    return out


# ---- (c) a system that shows every probe on its own -----------------------------------------------------------------------
B_SLOTS = 16


@dataclasses.dataclass
class ProbeSystem:
    n_atoms: int
    n_mol: int
    bonds: np.ndarray               # uint32 [B, M, 2]
    heads: np.ndarray               # uint32 [M]
    xyz: np.ndarray                 # f32 [frames, n_atoms, 3]
    box9: object                    # f32 [frames, 3, 3] or None
    which: np.ndarray               # [frames, M, B]: the probe in slot b of molecule m
    probes: list
    upper: np.ndarray               # bool [frames, M]: the head lies above the mid-plane
    cloud: object = None            # uint32: the atoms of the dynamic-normal cloud (heads and lattice; no probe atom)

    def vectors(self, shifts=MI_MAX_ITER):
        """The literal bond vector of every probe [P, 3]."""
        box = None if self.box9 is None else np.diag(self.box9[0])
        return np.array([literal_vector(p.p1, p.p2, box, shifts) for p in self.probes], dtype=F)

    def slot_sums(self, ticks, mask=None):
        """What (sums, counts) [B] of one plane must be for per-probe `ticks`; mask [frames, M]: the molecules of the plane."""
        t = np.asarray(ticks, dtype=np.int64)[self.which]
        m = np.ones(self.which.shape[:2], dtype=bool) if mask is None else mask
        return (t * m[:, :, None]).sum(axis=(0, 1)), np.broadcast_to(m[:, :, None], t.shape).sum(axis=(0, 1)).astype(np.uint64)


def probe_system(probes, axis=2, box=None, n_frames=N_FRAMES, swap_from=None, head_offset=2.0, cloud=False):
    """M = ceil(P / 16) molecules (an even number) of 16 bonds; molecule m = one head and 32 probe atoms; the heads are the
    first M atoms of the frame (one contiguous range: what the one-read leaflet path asks of a membrane group).  Frame f puts
    probe (16 m + b + f) % P' into slot b of molecule m (P' = 16 M; the list is padded with ordinary bonds).  Heads sit
    `head_offset` nm above (even m) or below (odd m) the mid-plane along `axis` — the box centre, or 0 without a box —
    on dyadic in-plane places; from frame `swap_from` on molecules 0 and 1 have changed sides.  `cloud`: a lattice of
    further atoms in the two planes of heads (ps.cloud: the heads and the lattice) — a dynamic-normal cloud with dyadic
    coordinates in a coordinate plane, so that its covariance sums are exact in any order and its normal is the axis."""
    probes = list(probes)
    n_mol = -(-len(probes) // B_SLOTS)
    n_mol += n_mol % 2
    probes += ordinary_probes(n_mol * B_SLOTS - len(probes), seed=11)
    n_p = len(probes)
    per = 2 * B_SLOTS
    n_atoms = n_mol * (1 + per)
    bonds = np.zeros((B_SLOTS, n_mol, 2), dtype=np.uint32)
    for m in range(n_mol):
        for b in range(B_SLOTS):
            bonds[b, m] = (n_mol + m * per + 2 * b, n_mol + m * per + 2 * b + 1)
    heads = np.arange(n_mol).astype(np.uint32)
    which = (np.arange(n_mol)[None, :, None] * B_SLOTS + np.arange(B_SLOTS)[None, None, :] + np.arange(n_frames)[:, None, None]) % n_p
    p1 = np.array([p.p1 for p in probes], dtype=F)
    p2 = np.array([p.p2 for p in probes], dtype=F)
    xyz = np.zeros((n_frames, n_atoms, 3), dtype=F)
    upper = np.zeros((n_frames, n_mol), dtype=bool)
    mid = F(0.0) if box is None else F(F(box[axis]) / F(2))
    a, b_ = (axis + 1) % 3, (axis + 2) % 3
    for f in range(n_frames):
        for m in range(n_mol):
            up = m % 2 == 0
            if swap_from is not None and f >= swap_from and m < 2:
                up = not up
            upper[f, m] = up
            h = np.zeros(3, dtype=F)
            h[axis] = mid + F(head_offset if up else -head_offset)
            h[a], h[b_] = F(1.0 + 0.5 * m), F(2.0 + 0.25 * m)
            xyz[f, m] = h
            xyz[f, n_mol + m * per:n_mol + (m + 1) * per:2] = p1[which[f, m]]
            xyz[f, n_mol + m * per + 1:n_mol + (m + 1) * per:2] = p2[which[f, m]]
    box9 = None
    if box is not None:
        box9 = np.zeros((n_frames, 3, 3), dtype=F)
        box9[:, 0, 0], box9[:, 1, 1], box9[:, 2, 2] = box
    ps = ProbeSystem(n_atoms, n_mol, bonds, heads, xyz, box9, which, probes, upper)
    if cloud:       # 2 x 20 atoms behind the probe atoms: a 5 x 4 lattice, 1 nm apart, in each of the two planes of heads
        grid = np.zeros((2, 5, 4, 3), dtype=F)
        grid[..., a] = np.arange(5, dtype=F)[None, :, None]
        grid[..., b_] = np.arange(1, 5, dtype=F)[None, None, :]
        grid[0, ..., axis], grid[1, ..., axis] = mid + F(head_offset), mid - F(head_offset)
        ps.xyz = np.concatenate([xyz, np.broadcast_to(grid.reshape(1, 40, 3), (n_frames, 40, 3))], axis=1).astype(F)
        ps.cloud = np.concatenate([heads, np.arange(n_atoms, n_atoms + 40)]).astype(np.uint32)
        ps.n_atoms = n_atoms + 40
    return ps


# ---- supplied normals ---------------------------------------------------------------------------------------------------------
# the zero vector, a NaN component, lengths 1e-25 (its square underflows: a zero norm) and 1e25 (its square overflows), a
# non-unit oblique vector, the everyday unit vector, and the two whose squared norm times an everyday bond's leaves the range
SUPPLIED = np.array([[0.0, 0.0, 0.0], [0.0, np.nan, 1.0], [0.0, 6e-26, 8e-26], [6e24, 0.0, 8e24], [0.3, -1.2, 2.5], [0.0, 0.0, 1.0],
                     [2.0 ** -40, 2.0 ** -40, 2.0 ** -41], [2.0 ** 40, 2.0 ** 40, 2.0 ** 39]], dtype=F)


def supplied_normals(n_mol, n_frames=N_FRAMES):
    """[frames, molecules, 3]: molecule m takes normal (m + f) % 8 in frame f — with 16 bonds a molecule and the probes
    moving on by one slot a frame, every probe meets most of them, guards and everyday bonds alike."""
    k = (np.arange(n_mol)[None, :] + np.arange(n_frames)[:, None]) % len(SUPPLIED)
    return SUPPLIED[k]


def literal_ticks_with_normals(ps, normals):
    """int64 [frames, molecules, slots]: the literal tick of every sample against its molecule's normal of that frame."""
    v = ps.vectors()
    t = np.zeros(ps.which.shape, dtype=np.int64)
    for (f, m, b), i in np.ndenumerate(ps.which):
        t[f, m, b] = literal_tick(v[i], normals[f, m])
    return t


# ---- (d) degenerate united-atom carbons ---------------------------------------------------------------------------------------
UA_CASES = ("carbon on a helper", "two helpers on one spot", "helper, carbon, helper collinear", "helper 2.5 box lengths away")
DYADIC = 2.0 ** -10


def ua_degenerate(xyz, carbons, n_lipids, apl, box=None):
    """Frames of united-atom lipids (synthetic.ua_membrane's layout: `apl` atoms a lipid) with exactly degenerate carbons.
    Every coordinate is first put on the 2^-10 nm lattice (exact in float32, and so is every difference), then in frame
    f, for lipid m and each (carbon, first helper, second helper) of `carbons` — lipid-relative atoms, one entry per
    carbon kind — case (f + m + j) % 4 of UA_CASES is planted:
      the first helper takes the carbon's coordinates (a zero helper vector);
      the second helper takes the first one's (two equal helper vectors: a zero cross product);
      the helpers sit at carbon + d and carbon - d (antiparallel: a zero cross product and a zero sum);
      the first helper moves 2.5 box lengths along x, y or z (with a box: the literal loops; without: an everyday carbon
      with a far helper).
    -> (frames, label [frames, lipids, carbons])."""
    xyz = (np.round(np.asarray(xyz, dtype=np.float64) / DYADIC) * DYADIC).astype(F)
    label = np.zeros((xyz.shape[0], n_lipids, len(carbons)), dtype=int)
    d = np.array([0.125, -0.0625, 0.09375], dtype=F)
    for f in range(xyz.shape[0]):
        for m in range(n_lipids):
            for j, (c, h1, h2) in enumerate(carbons):
                c, h1, h2 = (m * apl + k for k in (c, h1, h2))
                case = (f + m + j) % len(UA_CASES)
                label[f, m, j] = case
                if case == 0:
                    xyz[f, h1] = xyz[f, c]
                elif case == 1:
                    xyz[f, h2] = xyz[f, h1]
                elif case == 2:
                    xyz[f, h1], xyz[f, h2] = xyz[f, c] + d, xyz[f, c] - d
                else:
                    k = (f + m) % 3
                    xyz[f, h1, k] += F(2.5) * F(8.0 if box is None else box[k])
    return xyz, label
