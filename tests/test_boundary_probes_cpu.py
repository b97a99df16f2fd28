"""The probes of tests/boundary_probes.py hit the floats they claim, and its literal float32 statements of the
reference's comparisons agree with the oracle on every one of them (no tolerance, no probe left out).  CPU only."""
import numpy as np
import pytest

import boundary_probes as bp
from boundary_probes import F
from gorder_amd.abi import (GEOM_CUBOID, GEOM_CYLINDER, GEOM_SPHERE, GEOMREF_BOX_CENTER, GEOMREF_POINT, LEAFLETS_LOCAL,
                            DynamicNormal, Geometry, Leaflets, MolType, OrderMap, Tables)
from oracle import oracle

ORIGIN = (0.0, 0.0, 0.0)


def oracle_counts(tables, xyz):
    o = oracle.OracleEngine(tables, trig=oracle.TRIG_DIRECT)
    o.submit(xyz, None)
    return o.finish()


@pytest.mark.parametrize("r", bp.RADII)
def test_radius_probes_land_on_the_threshold_and_its_neighbours(r):
    thr = bp.radius_threshold(r)
    # the definition: sqrt(thr) reaches r, sqrt of the float below does not
    assert np.sqrt(thr) >= F(r) and np.sqrt(bp.step(thr, -1)) < F(r)
    for probes, d2_of in ((bp.plane_probes(r), lambda p: bp.dist2_plane(p[0], p[1])),
                          (bp.space_probes(r), lambda p: bp.dist2_space(*p[0]))):
        d2 = np.array([d2_of(p) for p in probes], dtype=F)
        assert np.array_equal(d2, np.array([p[-1] for p in probes], dtype=F))        # each probe IS where it says
        for target in bp.radius_targets(r).values():
            assert (d2 == target).any(), f"no probe at {target!r}"
        assert (d2 == thr).any() and (d2 == np.nextafter(thr, F(0))).any()
        literal = np.sqrt(d2) < F(r)
        assert np.array_equal(literal, d2 < thr)                                     # inside below thr, outside from thr on
        assert not literal[d2 == thr].any() and literal[d2 == np.nextafter(thr, F(0))].all()
        # an off-by-one-ulp threshold or a <= would show
        assert not np.array_equal(literal, d2 < bp.step(thr, 1)) and not np.array_equal(literal, d2 < bp.step(thr, -1))
        assert not np.array_equal(literal, d2 <= thr)


def test_threshold_is_not_the_rounded_square_for_these_radii():
    for r in (2.5, 2.3, 0.1, 1e-3, 300.0):
        assert bp.radius_threshold(r) == bp.step(F(r) * F(r), -1)
    for r in (2.0, 1.7, 3.0):
        assert bp.radius_threshold(r) == F(r) * F(r)


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("shape", ["sphere", "cylinder-x", "cylinder-y", "cylinder-z"])
def test_literal_radius_decisions_are_the_oracles(built, shape, invert):
    for r in bp.RADII:
        if shape == "sphere":
            pts = np.array([p[0] for p in bp.space_probes(r)], dtype=F)
            geom = Geometry(kind=GEOM_SPHERE, reference=GEOMREF_POINT, point=ORIGIN, radius=r, invert=invert)
            literal = [bp.inside_sphere(p, ORIGIN, r) != invert for p in pts]
        else:
            o = "xyz".index(shape[-1])
            pts = bp.geometry_points(bp.plane_probes(r), o)
            geom = Geometry(kind=GEOM_CYLINDER, reference=GEOMREF_POINT, point=ORIGIN, radius=r, orientation=o, invert=invert)
            literal = [bp.inside_cylinder(p, ORIGIN, r, o) != invert for p in pts]
        tables, xyz, which = slot_system(pts, handle_pbc=False, geometry=geom)
        got = oracle_counts(tables, xyz)
        np.testing.assert_array_equal(got.counts[0], bp.slot_counts(literal, which), err_msg=f"{shape} r={r}")
        assert 0 < sum(literal) < len(literal)


CUBOID_DIMS = [(0.0, 1.5), (-1.0, 0.5), (0.25, 0.7)]


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_literal_cuboid_and_height_decisions_are_the_oracles(built, axis, invert):
    for lo, hi in CUBOID_DIMS:
        ps = bp.extent_probes(lo, hi)
        pts = np.full((ps.size, 3), 0.125, dtype=F)
        pts[:, axis] = ps
        dims = [(-0.5, 0.5)] * 3
        dims[axis] = (lo, hi)
        geom = Geometry(kind=GEOM_CUBOID, reference=GEOMREF_POINT, point=ORIGIN, xdim=dims[0], ydim=dims[1], zdim=dims[2],
                        invert=invert)
        literal = [bp.inside_cuboid(p, ORIGIN, *dims) != invert for p in pts]
        tables, xyz, which = slot_system(pts, handle_pbc=False, geometry=geom)
        np.testing.assert_array_equal(oracle_counts(tables, xyz).counts[0], bp.slot_counts(literal, which))
        assert sum(literal) not in (0, len(literal))
        # the ends of a cylinder along `axis`
        geom = Geometry(kind=GEOM_CYLINDER, reference=GEOMREF_POINT, point=ORIGIN, radius=1.0, orientation=axis,
                        span=(lo, hi), invert=invert)
        literal = [bp.inside_cylinder(p, ORIGIN, 1.0, axis, (lo, hi)) != invert for p in pts]
        tables, xyz, which = slot_system(pts, handle_pbc=False, geometry=geom)
        np.testing.assert_array_equal(oracle_counts(tables, xyz).counts[0], bp.slot_counts(literal, which))
        assert sum(literal) not in (0, len(literal))


FAMILIES = bp.tile_families()


@pytest.mark.parametrize("k", range(len(FAMILIES)))
def test_tile_probes_meet_a_half_tile_line(k):
    lo, hi, bin, n, xs = FAMILIES[k]
    q = np.array([float(bp.tile_quotient(x, lo, bin)) for x in xs])
    t = np.array([bp.tile_index(x, lo, bin, n) for x in xs])
    on_line = np.flatnonzero(q % 1.0 == 0.5)
    assert on_line.size, "no probe on a half-tile line"
    triple = False
    for i in on_line:
        below, above = bp.step(xs[i], -1), bp.step(xs[i], 1)
        if below not in xs or above not in xs:      # (an outermost probe of a group: its neighbours are not probes)
            continue
        triple |= bp.tile_index(below, lo, bin, n) != bp.tile_index(above, lo, bin, n)
    assert triple, "the neighbours of no on-line probe land in different tiles"
    assert t[xs == lo][0] == 0 and t[xs == hi][0] in (n - 1, -1)
    # half-to-even instead of half-away would show
    assert any(bp.tile_index(x, lo, bin, n, bp.round_half_even) != bp.tile_index(x, lo, bin, n) for x in xs)


@pytest.mark.parametrize("plane", [0, 1, 2])
def test_literal_tiles_are_the_oracles(built, plane):
    for fam in FAMILIES:
        lo, hi, bin, n, _ = fam
        pts, ux, uy = bp.map_points(fam, plane)
        om = OrderMap(enabled=True, plane=plane, span_x=(lo, hi), span_y=(lo, hi), bin=(bin, bin))
        tables, xyz, which = slot_system(pts, n_frames=3, handle_pbc=False, ordermap=om)
        got = oracle_counts(tables, xyz)
        assert got.map_counts.shape[2:] == (n, n)
        np.testing.assert_array_equal(got.map_counts[0], bp.map_counts(bp.map_tiles(fam, ux, uy), which, n),
                                      err_msg=f"lo={lo} bin={bin}")


def test_literal_tile_counts_are_the_oracles(built):
    changed = 0
    for lo, hi, bin in bp.half_spans():
        om = OrderMap(enabled=True, plane=0, span_x=(lo, hi), span_y=(lo, bp.step(hi, 1)), bin=(bin, bin))
        tables, xyz, _ = slot_system(np.zeros((1, 3), dtype=F), n_frames=1, handle_pbc=False, ordermap=om)
        o = oracle.OracleEngine(tables, trig=oracle.TRIG_DIRECT)
        got = o.finish()
        assert got.map_counts.shape[2:] == (bp.n_tiles(lo, hi, bin), bp.n_tiles(lo, bp.step(hi, 1), bin))
        changed += bp.n_tiles(lo, hi, bin, bp.round_half_even) != bp.n_tiles(lo, hi, bin)
    assert changed, "no span sits on m + 1/2: the probes would not see another rounding"


# ---- index tables that make a probe's decision visible on its own (shared with the GPU test) ------------------
def slot_system(points, n_frames=9, **tables_kw):
    """One molecule whose B bonds are B accumulator slots; bond b joins atoms 2b and 2b + 1, both AT a probe, so the
    bond position p1 + v / 2 is the probe itself.  Frame f puts probe (b + f) % B into slot b.
    -> (tables, xyz [n_frames, 2B, 3], which [n_frames, B] = the probe in each slot)."""
    points = np.asarray(points, dtype=F).reshape(-1, 3)
    nb = points.shape[0]
    bonds = np.arange(2 * nb, dtype=np.uint32).reshape(nb, 1, 2)
    tables = Tables(n_atoms=2 * nb, molecule_types=[MolType(n_molecules=1, bonds=bonds)], **tables_kw)
    which = (np.arange(nb)[None, :] + np.arange(n_frames)[:, None]) % nb
    xyz = np.repeat(points[which], 2, axis=1).astype(F)
    return tables, xyz, which


def local_system(heads, partners, pbc, r):
    """Per frame one head (atom 0), an anchor 1 nm below it (atom 1) and a partner 10 nm above (atom 2) at the probe's
    in-plane place: with the partner inside the cylinder the centre rises above the head (lower leaflet, flag 1),
    without it the centre is between head and anchor (upper, 0)."""
    n = len(heads)
    xyz = np.zeros((n, 3, 3), dtype=F)
    for f, (h, p) in enumerate(zip(heads, partners)):
        xyz[f, 0] = (h[0], h[1], 15.0)
        xyz[f, 1] = (h[0], h[1], 14.0)
        xyz[f, 2] = (p[0], p[1], 25.0)
    tables = Tables(n_atoms=3, handle_pbc=pbc, timewise=True,
                    molecule_types=[MolType(n_molecules=1, bonds=np.array([[[0, 1]]], dtype=np.uint32), heads=np.array([0]))],
                    leaflets=Leaflets(method=LEAFLETS_LOCAL, normal_dim=2, frequency=1, radius=r, membrane=np.arange(3)))
    return tables, xyz


def dynamic_system(heads, partners, pbc, r, L=None):
    """Per frame a head (atom 0) whose cloud is itself, two atoms a quarter radius away (1, 2) and the probe (3)."""
    n = len(heads)
    q = F(F(r) / F(4))
    xyz = np.zeros((n, 4, 3), dtype=F)
    for f, (h, p) in enumerate(zip(heads, partners)):
        hz = F(10.0) if len(p) == 2 else F(0.0)
        xyz[f, 0] = (h[0], h[1], hz)
        xyz[f, 1] = (h[0] + q, h[1], hz + q)
        xyz[f, 2] = (h[0], h[1] + q, hz - q)
        xyz[f, 3] = (p[0], p[1], hz) if len(p) == 2 else p
        if L is not None:
            xyz[f, 1:3, :2] = np.mod(xyz[f, 1:3, :2], F(L))
    tables = Tables(n_atoms=4, handle_pbc=pbc,
                    molecule_types=[MolType(n_molecules=1, bonds=np.array([[[0, 1]]], dtype=np.uint32),
                                            normal_heads=np.array([0]))],
                    dynamic_normal=DynamicNormal(enabled=True, radius=r, cloud=np.arange(4)))
    return tables, xyz


def periodic_reference(where, box):
    """-> (reference point, Geometry keywords): the box centre, or a fixed point next to three faces."""
    box = np.array(box, dtype=F)
    if where == "box centre":
        return (box / F(2)).astype(F), dict(reference=GEOMREF_BOX_CENTER)
    ref = np.array([0.05, float(box[1]) - 0.03, 7.0], dtype=F)
    return ref, dict(reference=GEOMREF_POINT, point=tuple(float(x) for x in ref), structure_box=tuple(float(x) for x in box))


def periodic_radius_case(shape, where, box, r):
    """Sphere or cylinder (span -0.5 .. 0.5 along its axis) in a periodic box -> (geometry, points, literal decisions,
    [decisions of a wrong form]): positions at thr - 2 .. thr + 1 floats of squared distance in four directions, and for
    the cylinder the positions whose wrapped offset along the axis is 0, the height and the floats around them."""
    ref, kw = periodic_reference(where, box)
    thr = bp.radius_threshold(r)
    if shape == "sphere":
        pts, d2 = bp.periodic_radius_probes(ref, box, r, (0, 1), 2)
        geom = Geometry(kind=GEOM_SPHERE, radius=r, **kw)
        ends = np.ones(len(pts), dtype=bool)
        strict_ends = ends
    else:
        o = "xyz".index(shape[-1])
        pts, d2 = bp.periodic_radius_probes(ref, box, r, ((o + 1) % 3, (o + 2) % 3))
        base = bp.wrap(F(ref[o] + F(-0.5)), box[o])
        height = F(F(0.5) - F(-0.5))
        pts[:, o] = F(base + F(0.25))
        ends = [True] * len(pts)
        strict_ends = list(ends)
        for p, e in bp.wrapped_extent_probes(base, height, box[o]):      # on the axis: d2 = 0
            q = np.array(ref, dtype=F)
            q[o] = p
            pts, d2 = np.vstack([pts, q]), np.append(d2, F(0.0))
            ends.append(bool(e <= height))
            strict_ends.append(bool(e < height))
        ends, strict_ends = np.array(ends), np.array(strict_ends)
        assert not np.array_equal(ends, strict_ends)
        geom = Geometry(kind=GEOM_CYLINDER, radius=r, orientation=o, span=(-0.5, 0.5), **kw)
    assert (d2 == thr).any() and (d2 == bp.step(thr, -1)).any()
    literal = (np.sqrt(d2) < F(r)) & ends
    assert np.array_equal(literal, (d2 < thr) & ends)
    mutants = [(d2 < bp.step(thr, 1)) & ends, (d2 < bp.step(thr, -1)) & ends, (d2 <= thr) & ends]
    if shape != "sphere":
        mutants.append((d2 < thr) & strict_ends)
    return geom, pts, literal, mutants


def periodic_cuboid_case(where, box):
    """A cuboid -1 .. 0.5 nm around the reference in a periodic box: per axis the positions whose wrapped offset from the
    cuboid's corner is 0, the float above, the float below (wraps to the far side: outside), the extent, and the
    nearest float either side of it; Rectangular::inside there is `wrap(p - corner) <= extent`."""
    ref, kw = periodic_reference(where, box)
    lo, hi = F(-1.0), F(0.5)
    size = F(hi - lo)
    corner = np.array([bp.wrap(F(ref[k] + lo), box[k]) for k in range(3)], dtype=F)
    inside_pt = np.array([bp.wrap(F(corner[k] + F(0.25)), box[k]) for k in range(3)], dtype=F)
    pts, literal, strict = [], [], []
    for k in range(3):
        for p, e in bp.wrapped_extent_probes(corner[k], size, box[k]):
            q = inside_pt.copy()
            q[k] = p
            pts.append(q)
            literal.append(bool(e <= size))
            strict.append(bool(e < size))
    geom = Geometry(kind=GEOM_CUBOID, xdim=(lo, hi), ydim=(lo, hi), zdim=(lo, hi), **kw)
    return geom, np.array(pts, dtype=F), np.array(literal), [np.array(strict)]


PBC_BOX = (12.0, 13.0, 14.0)


@pytest.mark.parametrize("where", ["box centre", "near a face"])
@pytest.mark.parametrize("shape", ["sphere", "cylinder-x", "cylinder-y", "cylinder-z", "cuboid"])
def test_periodic_probes_land_where_they_claim_and_the_oracle_agrees(built, shape, where):
    cases = [periodic_cuboid_case(where, PBC_BOX)] if shape == "cuboid" else \
        [periodic_radius_case(shape, where, PBC_BOX, r) for r in (2.0, 2.5, 2.3, 1.7, 3.1415927, 0.1, 2.2, 3.0)]
    for geom, pts, literal, mutants in cases:
        assert 0 < literal.sum() < literal.size
        for wrong in mutants:
            assert not np.array_equal(wrong, literal)
        tables, xyz, which = slot_system(pts, 3, handle_pbc=True, geometry=geom)
        o = oracle.OracleEngine(tables, trig=oracle.TRIG_DIRECT)
        b9 = np.zeros((3, 3, 3), dtype=F)
        b9[:, 0, 0], b9[:, 1, 1], b9[:, 2, 2] = PBC_BOX
        o.submit(xyz, b9)
        np.testing.assert_array_equal(o.finish().counts[0], bp.slot_counts(literal, which), err_msg=f"r={geom.radius}")


def test_cell_grid_constants_are_the_kernels():
    """boundary_probes restates the device's pruning grid to put heads ON its lines: if the header changes, say so."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(__file__), "..", "gorder_amd", "csrc", "kernels_leaflets.h")).read()
    for name, value in (("kLocalFine", bp.K_FINE), ("kLocalFineRows", bp.K_FINE_ROWS), ("kLocalMaxCells1D", bp.MAX_CELLS)):
        assert int(re.search(rf"constexpr uint32_t {name} = (\d+);", src).group(1)) == value
    assert "floorf(L / (radius / (float)kk) * 0.9999f)" in src and "floorf(wa / box[da] * (float)nca)" in src


@pytest.mark.parametrize("k_max", [bp.K_FINE, bp.K_FINE_ROWS])
def test_cell_line_probes_and_the_oracles_cylinder_and_cloud(built, k_max):
    r = 2.0
    L, probes = bp.cell_line_probes(r, k_max)
    n = len(probes)
    literal = np.array([int(p[2]) for p in probes])
    assert n >= 9 and literal.sum() == n // 2
    b9 = np.zeros((n, 3, 3), dtype=F)
    b9[:, 0, 0], b9[:, 1, 1], b9[:, 2, 2] = L, L, 40.0
    tables, xyz = local_system([p[0] for p in probes], [p[1] for p in probes], True, r)
    o = oracle.OracleEngine(tables, trig=oracle.TRIG_DIRECT)
    o.submit(xyz, b9)
    np.testing.assert_array_equal(o.timewise(n)[1][:, 2, 0], literal)       # the sample went to the lower leaflet
    tables, xyz = dynamic_system([p[0] for p in probes], [p[1] for p in probes], True, r, L)
    for f in range(n):
        o = oracle.OracleEngine(tables, trig=oracle.TRIG_DIRECT)
        o.submit(xyz[f:f + 1], b9[f:f + 1])
        assert int(o.normals()[1][0]) == 3 + literal[f]
