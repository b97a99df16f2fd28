"""Coordinates that sit on the floats where the analysis path decides, and the decisions stated literally.

Plain numpy, no GPU, no ctypes, nothing of this project imported.  Two parts:

(a) the reference's comparisons in float32, every operation rounded on its own (groan_rs Sphere / Cylinder /
    Rectangular ::inside without periodic boundaries, GridMap's nearest-tile index and tile count) — an independent
    statement that shares no code with oracle/ or the kernels;
(b) constructors of probes: in-plane and 3-D offsets whose squared length lands on a chosen float around the
    threshold of `sqrt(d2) < r`, coordinates on and next to the half-tile lines of an ordermap, offsets on and next
    to the faces of a cuboid or the ends of a cylinder.

`radius_threshold` is the definition the kernels' `d2 < thr` shortcut relies on (the smallest float whose correctly
rounded square root reaches the radius), computed here from that definition.
"""
from __future__ import annotations

import numpy as np

F = np.float32
INF = F(np.inf)
FLT_MAX = np.finfo(np.float32).max

RADII = (2.0, 2.5, 2.3, 1.7, 3.1415927, 0.1, 1e-3, 300.0, 2.2, 3.0)
BINS = (0.1, 0.25, 0.3, 0.7, 1.0, 1.0 / 3.0)
LOS = (0.0, 2.0, -1.5)
KS = (-3, -2, -1, 0, 1, 2, 3)


# ---- float32 helpers --------------------------------------------------------------------------------
def step(x, n: int) -> np.float32:
    """The float `n` places above (below for n < 0) x."""
    x = F(x)
    for _ in range(abs(int(n))):
        x = np.nextafter(x, INF if n > 0 else -INF)
    return F(x)


def ulp(x) -> np.float32:
    return F(np.spacing(F(abs(F(x)))))


def round_half_away(q) -> float:
    """C's roundf of a float32, done in float64 on the float32 value (np.round is half-to-even)."""
    q = float(F(q))
    return float(np.trunc(q + np.copysign(0.5, q)))


def round_half_even(q) -> float:
    """The WRONG rounding, for the tests' own sensitivity checks."""
    return float(np.round(float(F(q))))


# ---- (a) the literal statements ---------------------------------------------------------------------
def radius_threshold(r) -> np.float32:
    """Smallest float32 t with fl(sqrt(t)) >= r: `sqrt(d2) < r` <=> `d2 < t` because sqrt is monotonic."""
    r = F(r)
    if not r > 0:
        return F(0.0)
    t = F(r * r)
    while np.sqrt(t) < r:
        t = step(t, 1)
    while t > 0 and np.sqrt(step(t, -1)) >= r:
        t = step(t, -1)
    return t


def dist2_plane(da, db) -> np.float32:
    da, db = F(da), F(db)
    return F(F(da * da) + F(db * db))


def dist2_space(dx, dy, dz) -> np.float32:
    dx, dy, dz = F(dx), F(dy), F(dz)
    return F(F(F(dx * dx) + F(dy * dy)) + F(dz * dz))        # nalgebra: (x x + y y) + z z


def inside_sphere(p, ref, radius, thr=None) -> bool:
    """Sphere::inside, no periodic boundaries: |p - ref| < radius.  `thr`: evaluate `d2 < thr` instead (sensitivity)."""
    d = [F(F(p[k]) - F(ref[k])) for k in range(3)]
    d2 = dist2_space(*d)
    return bool(d2 < thr) if thr is not None else bool(np.sqrt(d2) < F(radius))


def inside_cylinder(p, ref, radius, orientation, span=(-np.inf, np.inf), thr=None) -> bool:
    """Cylinder::inside, no periodic boundaries: in-plane distance < radius and 0 <= along the axis <= height, the
    cylinder's base at ref + span[0] (an unbounded one: anywhere)."""
    o = int(orientation)
    a, b = (o + 1) % 3, (o + 2) % 3
    da, db = F(F(p[a]) - F(ref[a])), F(F(p[b]) - F(ref[b]))
    d2 = dist2_plane(da, db)
    near = bool(d2 < thr) if thr is not None else bool(np.sqrt(d2) < F(radius))
    if span[0] == -np.inf and span[1] == np.inf:
        return near
    base, height = F(F(ref[o]) + F(span[0])), F(F(span[1]) - F(span[0]))
    e = F(F(p[o]) - base)
    return near and bool(e >= 0) and bool(e <= height)


def inside_cuboid(p, ref, xdim, ydim, zdim) -> bool:
    """Rectangular::inside, no periodic boundaries: 0 <= p - (ref + lo) <= hi - lo per dimension."""
    for k, dim in enumerate((xdim, ydim, zdim)):
        if dim[0] == -np.inf and dim[1] == np.inf:
            continue
        e = F(F(p[k]) - F(F(ref[k]) + F(dim[0])))
        if not (e >= 0 and e <= F(F(dim[1]) - F(dim[0]))):
            return False
    return True


def tile_quotient(x, lo, bin) -> np.float32:
    return F(F(F(x) - F(lo)) / F(bin))


def tile_index(x, lo, bin, n, rounding=round_half_away) -> int:
    """GridMap::get_mut_at: the nearest tile centre lo + k bin, -1 outside the n tiles."""
    k = rounding(tile_quotient(x, lo, bin))
    if not (k >= 0.0) or not (k < float(F(n))):
        return -1
    return int(k)


def n_tiles(lo, hi, bin, rounding=round_half_away) -> int:
    """GridMap::new: round((hi - lo) / bin) + 1 tiles."""
    n = rounding(F(F(F(hi) - F(lo)) / F(bin)))
    return 0 if n < 0 else int(n) + 1


# ---- (b) probes -------------------------------------------------------------------------------------
def radius_targets(r):
    """{label: float} the squared lengths to land on: thr + k ulp(thr) for k in -3..3, and the floats up to three
    places either side of thr (the two differ where thr is a power of two)."""
    thr = radius_threshold(r)
    out = {}
    for k in KS:
        out[("ulp", k)] = F(np.float64(thr) + k * np.float64(ulp(thr)))
        out[("step", k)] = step(thr, k)
    return out


def plane_probes(r):
    """[(dx, dy, d2)]: for every target of radius_targets an in-plane offset whose literal squared length IS the target
    (dx a few dozen ulps below r, dy from the remainder), then the single-axis offsets r -3 .. +3 ulps."""
    r = F(r)
    out, missing = [], []
    for label, target in radius_targets(r).items():
        for j in range(16, 96):
            dx = step(r, -j)
            rest = np.float64(target) - np.float64(F(dx * dx))
            if rest <= 0:
                continue
            dy = F(np.sqrt(rest))
            if dist2_plane(dx, dy) == target:
                out.append((dx, dy, target))
                break
        else:
            missing.append(label)
    assert not missing, f"radius {r}: no offset reaches {missing}"
    for s in range(-3, 4):
        dx = step(r, s)
        out.append((dx, F(0.0), dist2_plane(dx, 0.0)))
    return out


def space_probes(r):
    """[(d[3], d2)]: the same with a third component, the solved component in each of the three places so that the
    order (x x + y y) + z z of the sum matters; then the plane probes with a zero third component."""
    r = F(r)
    out, missing = [], []
    for label, target in radius_targets(r).items():
        for place in range(3):
            for j in range(16, 160):
                big = step(F(r * F(0.984375)), -j)
                mid = F(r * F(0.03125) * F(1 + (j % 4)))                  # a small second component that varies
                fixed = [big, mid]
                partial = {0: F(fixed[0] * fixed[0]), 1: F(fixed[1] * fixed[1])}
                rest = np.float64(target) - np.float64(partial[0]) - np.float64(partial[1])
                if rest <= 0:
                    continue
                solved = F(np.sqrt(rest))
                d = fixed[:]
                d.insert(place, solved)
                if dist2_space(*d) == target:
                    out.append((np.array(d, dtype=F), target))
                    break
            else:
                missing.append((label, place))
    assert not missing, f"radius {r}: no 3-D offset reaches {missing}"
    for dx, dy, d2 in plane_probes(r):
        out.append((np.array([dx, dy, 0.0], dtype=F), d2))
    return out


def tile_family(lo, bin, span=3.0):
    """(lo, hi, bin, n, [x]): coordinates on and around the half-tile lines of the map lo .. lo + span."""
    lo, bin = F(lo), F(bin)
    if 2.0 ** -30 < bin < 2.0 ** 30:
        hi = F(np.float64(lo) + span)                       # an everyday bin: a map `span` nm wide
    else:
        hi = F(np.float64(lo) + span * np.float64(bin))     # a bin of 2^-41 or 2^41: a map `span` bins wide
    n = n_tiles(lo, hi, bin)
    xs = []

    def around(v, reach=2):
        v = F(v)
        for s in range(-reach, reach + 1):
            xs.append(step(v, s))

    def line(k, must=False):    # the coordinate whose quotient is k + 1/2 exactly if there is one nearby, and its neighbours
        x0 = F(np.float64(lo) + (k + 0.5) * np.float64(bin))
        for s in sorted(range(-6, 7), key=abs):
            if float(tile_quotient(step(x0, s), lo, bin)) == k + 0.5:
                around(step(x0, s))
                return True
        if not must:
            around(x0)
        return False

    exact = [line(k) for k in sorted({0, 1, n - 2, n - 1}) if k >= 0]
    exact.append(line(-1))  # lo - bin / 2: the lower edge of tile 0
    if not any(exact):      # (x - lo is too coarse to meet those lines: take the first line that some float does meet)
        assert any(line(k, must=True) for k in range(2, n - 2)), f"no float on a half-tile line of ({lo}, {bin})"
    xs.append(lo)
    xs.append(hi)
    return lo, hi, bin, n, np.array(xs, dtype=F)


def tile_families():
    fams = [tile_family(lo, b) for b in BINS for lo in LOS]
    fams.append(tile_family(0.0, 2.0 ** -41))       # outside [2^-40, 2^40]: the plain division, not its Newton core
    fams.append(tile_family(0.0, 2.0 ** 41))
    return fams


def half_spans():
    """[(lo, hi, bin)]: spans whose (hi - lo) / bin is within an ulp of m + 1/2 — where the tile COUNT rounds."""
    out = []
    for b in BINS:
        for lo in LOS:
            for m in (2, 7):
                hi0 = F(np.float64(F(lo)) + (m + 0.5) * np.float64(F(b)))
                for s in (-1, 0, 1):
                    out.append((F(lo), step(hi0, s), F(b)))
    return out


def extent_probes(lo, hi):
    """Coordinates p (reference at the origin) whose offset p - lo is 0, the extent hi - lo, and one float either side."""
    lo, hi = F(lo), F(hi)
    ps = [lo, step(lo, -1), step(lo, 1), hi, step(hi, -1), step(hi, 1), F(0.5) * F(lo + hi)]
    if lo == 0:
        ps.append(F(-0.0))
    return np.array(ps, dtype=F)


# ---- (c) what the engines' results must be for the probes (the index tables are built by the tests) ----
def slot_counts(decisions, which):
    """What counts[0] must be when probe i is accumulated iff decisions[i]; which [n_frames, B] = the probe that sits
    in slot b in frame f."""
    return np.asarray(decisions, dtype=np.uint64)[which].sum(axis=0)


def geometry_points(offsets, orientation=2):
    """In-plane offsets (da, db) of a cylinder with the given axis as points [n, 3] (axis coordinate 0)."""
    a, b = (orientation + 1) % 3, (orientation + 2) % 3
    pts = np.zeros((len(offsets), 3), dtype=F)
    for i, off in enumerate(offsets):
        pts[i, a], pts[i, b] = off[0], off[1]
    return pts


def map_points(family, plane):
    """The family's coordinates along the map's x (y at the centre of tile 1), then along its y -> (points [2n, 3],
    x [2n], y [2n]); Plane::projection2plane: xy, xz, (z, y)."""
    lo, hi, bin, n, xs = family
    centre = F(np.float64(lo) + np.float64(bin))
    ux = np.concatenate([xs, np.full(xs.size, centre, dtype=F)])
    uy = np.concatenate([np.full(xs.size, centre, dtype=F), xs])
    pts = np.zeros((ux.size, 3), dtype=F)
    ax, ay = {0: (0, 1), 1: (0, 2), 2: (2, 1)}[plane]
    pts[:, ax], pts[:, ay] = ux, uy
    return pts, ux, uy


def map_tiles(family, ux, uy, rounding=round_half_away):
    """-> [n_probes, 2] tile (ix, iy) of each probe, -1 where it is outside."""
    lo, hi, bin, n, _ = family
    return np.array([[tile_index(x, lo, bin, n, rounding), tile_index(y, lo, bin, n, rounding)] for x, y in zip(ux, uy)])


def map_counts(tiles, which, n):
    """What map_counts[0] [B, n, n] must be for the frames of slot_system."""
    out = np.zeros((which.shape[1], n, n), dtype=np.uint64)
    for f in range(which.shape[0]):
        for b in range(which.shape[1]):
            ix, iy = tiles[which[f, b]]
            if ix >= 0 and iy >= 0:
                out[b, ix, iy] += 1
    return out


# ---- (b, continued) probes in a periodic box -------------------------------------------------------------
# There the decision quantity is made from e = min_image(fl(p - anchor)) or wrap(fl(p - anchor)): an offset added to an
# anchor of several nm is rounded to the anchor's ulp, so the offsets above do not survive.  These constructors search
# the floats around a wanted place for positions whose LITERAL chain lands on the target.
def min_image(e, L):
    """The reference's minimum-image loops on float32 arrays (one turn each is all these probes need)."""
    e, L = np.asarray(e, dtype=F), F(L)
    half = F(L / F(2))
    e = np.where(e > half, (e - L).astype(F), e)
    return np.where(e < -half, (e + L).astype(F), e).astype(F)


def wrap(x, L):
    """Vector3D::wrap, one turn: into [0, L]."""
    x, L = np.asarray(x, dtype=F), F(L)
    x = np.where(x > L, (x - L).astype(F), x)
    return np.where(x < 0, (x + L).astype(F), x).astype(F)


def floats_around(x0, reach, coarse):
    """2 reach + 1 floats around x0 > 0, as many floats apart as it takes to move by an ulp of `coarse` (a difference
    p - h is rounded to the ulp of the larger operand: finer steps would repeat it)."""
    x0 = F(x0)
    stride = max(1, int(round(float(ulp(coarse)) / float(ulp(x0)))))
    bits = int(x0.view(np.int32))
    assert x0 > 0 and bits > reach * stride
    return (np.arange(bits - reach * stride, bits + reach * stride + 1, stride, dtype=np.int64).astype(np.int32)).view(F)


def plane_search(anchor, approx, L, targets, third=0.0, reach=200):
    """Positions (pa, pb) near `approx` whose literal squared distance from `anchor` in the periodic box —
    fl(fl(fl(ea ea) + fl(eb eb)) + fl(third third)), e = min_image(fl(p - anchor)) — IS each of `targets`.
    L: the two box edges.  -> [(pa, pb)] in the order of the targets."""
    L = (L, L) if np.ndim(L) == 0 else L
    for wider in (reach, 4 * reach, 8 * reach):     # (a coarse lattice of offsets meets few sums: widen before giving up)
        try:
            return _plane_search(anchor, approx, L, targets, third, wider)
        except AssertionError:
            if wider == 8 * reach:
                raise


def _plane_search(anchor, approx, L, targets, third, reach):
    pa, pb = floats_around(approx[0], reach, anchor[0]), floats_around(approx[1], reach, anchor[1])
    ea, eb = min_image((pa - F(anchor[0])).astype(F), L[0]), min_image((pb - F(anchor[1])).astype(F), L[1])
    d2 = ((ea * ea).astype(F)[:, None] + (eb * eb).astype(F)[None, :]).astype(F)
    d2 = (d2 + F(F(third) * F(third))).astype(F)
    out = []
    for t in targets:
        hit = np.argwhere(d2 == F(t))
        assert hit.size, f"no position at squared distance {t!r} of {anchor}"
        i, j = hit[len(hit) // 2]
        out.append((pa[i], pb[j]))
    return out


def wrapped_extent_probes(pos, size, L, reach=64):
    """Coordinates p whose offset from a cuboid's (or cylinder's) base in the periodic box, e = wrap(fl(p - pos)), is 0,
    the smallest e above 0, (p one float below pos: e wraps to about L), the extent itself, and the nearest e either
    side of the extent that a float can give.  -> [(p, e)]."""
    pos, size, L = F(pos), F(size), F(L)
    out = [(pos, F(0.0)), (step(pos, 1), wrap(F(step(pos, 1) - pos), L)), (step(pos, -1), wrap(F(step(pos, -1) - pos), L))]
    far = float(pos) + float(size)
    far = far - float(L) if far >= float(L) else far
    ps = floats_around(far, reach, L)
    e = wrap((ps - pos).astype(F), L)
    on, above, below = np.flatnonzero(e == size), np.flatnonzero(e > size), np.flatnonzero(e < size)
    assert on.size and above.size and below.size, f"no float at extent {size!r} from {pos!r}"
    for i in (on[0], above[np.argmin(e[above])], below[np.argmax(e[below])]):
        out.append((ps[i], e[i]))
    return out


# the cell grid the device prunes with (kernels_leaflets.h: kLocalFine, kLocalFineRows, kLocalMaxCells1D, local_axis,
# and the cell of a wrapped coordinate); tests/test_boundary_probes_cpu.py checks the constants against the header
K_FINE, K_FINE_ROWS, MAX_CELLS = 4, 7, 128


def local_axis(L, radius, k_max, nc_max=MAX_CELLS):
    """(cells, reach) along a box edge."""
    for kk in range(k_max, 0, -1):
        fine = np.floor(F(F(F(L) / F(F(radius) / F(kk))) * F(0.9999)))
        if 2 * kk + 1 <= fine <= nc_max:
            return int(fine), kk
    return 1, 0


def cell_of(x, L, nc):
    return int(min(max(np.floor(F(F(F(x) / F(L)) * F(nc))), 0), nc - 1))


def cell_line_probes(r, k_max):
    """Heads ON a line of the cell grid (and at 0 and box - ulp) with a partner at thr - 1 ulp (inside) and at thr
    (outside): across the line, across the periodic face, and on the diagonal.
    -> (box edge L, [(head (a, b), partner (a, b), inside)])."""
    L = F(18.5) if k_max == K_FINE_ROWS else F(16.25)
    nc, reach = local_axis(L, r, k_max, MAX_CELLS - 2 * K_FINE_ROWS if k_max == K_FINE_ROWS else MAX_CELLS)
    w = F(L / F(nc))
    assert reach == k_max and float(w) * nc == float(L), "the cell width is not a float: no coordinate is ON a line"
    line, line2 = F(20 * w), F(9 * w)
    for x, c in ((line, 20), (line2, 9)):       # ON the line: the float below lies in the cell before
        assert cell_of(x, L, nc) == c and cell_of(step(x, -1), L, nc) == c - 1
    top = step(L, -1)
    assert cell_of(0.0, L, nc) == 0 and cell_of(top, L, nc) == nc - 1
    thr = radius_threshold(r)
    targets = (step(thr, -1), thr)
    dx = float(np.sqrt(float(thr) - 0.01))
    da, db = float(r) * np.cos(0.61), float(r) * np.sin(0.61)     # (not 45 degrees: equal steps along both axes reach few sums)
    mid = float(F(5.5 * w))
    layouts = [((line, mid), (line - dx, mid + 0.1)),                    # across the line, into the cells below
               ((line, mid), (line + dx, mid - 0.1)),
               ((F(0.0), mid), (float(L) - dx, mid + 0.1)),             # across the periodic face
               ((top, mid), (dx, mid - 0.1)),
               ((line, line2), (line - da, line2 - db)),                # the diagonal, both coordinates on a line
               ((F(0.0), F(0.0)), (float(L) - da, float(L) - db)),      # the corner of the box
               ((top, top), (da, db))]
    out = []
    for head, approx in layouts:
        for partner, inside in zip(plane_search(head, approx, L, targets), (True, False)):
            out.append((head, partner, inside))
    return L, out


def periodic_radius_probes(anchor, box, r, axes, third_axis=None):
    """Positions in the box whose literal squared distance from `anchor` (in-plane `axes`; with `third_axis` the sphere's
    (x x + y y) + z z, the third offset a fixed 0.25 r) is thr - 2, thr - 1, thr, thr + 1 floats, in four directions —
    towards and across whatever faces are near.  -> (points [n, 3], d2 [n])."""
    thr = radius_threshold(r)
    targets = [step(thr, k) for k in (-2, -1, 0, 1)]
    a, b = axes
    third = F(0.25) * F(r) if third_axis is not None else F(0.0)
    rr = float(np.sqrt(float(thr) - float(third) ** 2))
    pts, d2 = [], []
    for ang in (0.61, 2.2, 3.9, 5.5):
        approx = [(float(anchor[a]) + rr * np.cos(ang)) % float(box[a]), (float(anchor[b]) + rr * np.sin(ang)) % float(box[b])]
        base = np.array(anchor, dtype=F)
        if third_axis is not None:
            base[third_axis] = F(anchor[third_axis]) + third
            e3 = min_image(F(base[third_axis] - F(anchor[third_axis])), box[third_axis])
        else:
            e3 = F(0.0)
        for t, (pa, pb) in zip(targets, plane_search((anchor[a], anchor[b]), approx, (box[a], box[b]), targets, third=e3)):
            p = base.copy()
            p[a], p[b] = pa, pb
            pts.append(p)
            d2.append(t)
    return np.array(pts, dtype=F), np.array(d2, dtype=F)
