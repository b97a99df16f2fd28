"""Every comparison the kernels replace by a cheaper form, probed on the floats where the decision flips.

The device evaluates `sqrt(d2) < r` as `d2 < thr` (geom_inside, the local-leaflet cylinder, k_dyn_cov), the ordermap
tile as roundf of a Newton-core quotient, the tile counts on the host, the cuboid / cylinder-end tests on wrapped
offsets, and prunes neighbours with a cell grid.  tests/boundary_probes.py builds coordinates whose decision quantity
lands on thr, on the floats around it, on the half-tile lines and on the faces; here each probe owns an accumulator
slot (or a frame), so its decision shows on its own, and must equal the literal float32 statement and the oracle."""
import numpy as np
import pytest

import boundary_probes as bp
from boundary_probes import F
from gorder_amd import HipEngine
from gorder_amd.abi import (GEOM_CUBOID, GEOM_CYLINDER, GEOM_SPHERE, GEOMREF_BOX_CENTER, GEOMREF_POINT, LEAFLETS_LOCAL,
                            DynamicNormal, Geometry, Leaflets, MolType, OrderMap, Tables)
from oracle import oracle
from test_boundary_probes_cpu import (dynamic_system, local_system, periodic_cuboid_case, periodic_radius_case, slot_system)

pytestmark = pytest.mark.gpu

ORIGIN = (0.0, 0.0, 0.0)
N_FRAMES = 9                       # two stages of four frames and a partial one
# (GORDER_HIP_FORCE_DIRECT is no route of these tests: gorder_hip_create refuses geometry, ordermaps and per-frame rows
# for bonds that are not in an atom window, so k_bonds_direct never evaluates a shape or a tile)
BOND_ROUTES = {"tiled": {}, "gather": {"GORDER_HIP_KERNEL": "gather"}}
# every switch a test of this file sets; set_route clears them first
ALL_SWITCHES = ("GORDER_HIP_KERNEL", "GORDER_HIP_MAP_DIRECT", "GORDER_HIP_MAPS_GATHER", "GORDER_HIP_LOCAL_THREE_KERNELS",
                "GORDER_HIP_LOCAL_ATOMS_ONLY", "GORDER_HIP_LOCAL_NO_PRUNE")


def set_route(monkeypatch, env):
    for name in ALL_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def box9(box, n):
    b = np.zeros((n, 3, 3), dtype=F)
    b[:, 0, 0], b[:, 1, 1], b[:, 2, 2] = box
    return b


def both(tables, xyz, box=None):
    """The frames through the device and the oracle -> (device results, oracle results, engine, oracle engine)."""
    n = xyz.shape[0]
    eng = HipEngine(tables)
    eng.submit_host(xyz, box, np.arange(n))
    got = eng.finish()
    o = oracle.OracleEngine(tables, trig=oracle.TRIG_DIRECT)
    o.submit(xyz, box)
    return got, o.finish(), eng, o


# ---- geometry: sqrt(d2) < r as d2 < thr -----------------------------------------------------------------
def radius_case(shape, r, invert):
    """-> (points, geometry, decide(thr=None)): the literal decisions, or those of `d2 < thr` for a given thr."""
    if shape == "sphere":
        pts = np.array([p[0] for p in bp.space_probes(r)], dtype=F)
        geom = Geometry(kind=GEOM_SPHERE, reference=GEOMREF_POINT, point=ORIGIN, radius=r, invert=invert)
        return pts, geom, lambda thr=None: [bp.inside_sphere(p, ORIGIN, r, thr) != invert for p in pts]
    o = "xyz".index(shape[-1])
    pts = bp.geometry_points(bp.plane_probes(r), o)
    geom = Geometry(kind=GEOM_CYLINDER, reference=GEOMREF_POINT, point=ORIGIN, radius=r, orientation=o, invert=invert)
    return pts, geom, lambda thr=None: [bp.inside_cylinder(p, ORIGIN, r, o, thr=thr) != invert for p in pts]


@pytest.mark.parametrize("route", list(BOND_ROUTES))
@pytest.mark.parametrize("shape", ["sphere", "cylinder-x", "cylinder-y", "cylinder-z"])
def test_geometry_radius_threshold(built, monkeypatch, shape, route):
    """counts[0][slot] of every probe at thr + k ulp, k = -3 .. 3: inside below thr, outside from thr on."""
    set_route(monkeypatch, BOND_ROUTES[route])
    for r in bp.RADII:
        for invert in (False, True):
            pts, geom, decide = radius_case(shape, r, invert)
            tables, xyz, which = slot_system(pts, N_FRAMES, handle_pbc=False, geometry=geom)
            got, want, _, _ = both(tables, xyz)
            literal = decide()
            print(f"{shape} {route} r={r} invert={invert}: {len(literal)} probes, {sum(literal)} accumulated")
            np.testing.assert_array_equal(want.counts[0], bp.slot_counts(literal, which), err_msg=f"oracle, r={r}")
            np.testing.assert_array_equal(got.counts[0], bp.slot_counts(literal, which), err_msg=f"device, r={r} invert={invert}")
            np.testing.assert_array_equal(got.sums, want.sums)
            # the probes see a threshold that is one float off, either way
            thr = bp.radius_threshold(r)
            assert decide(thr) == literal
            assert decide(bp.step(thr, 1)) != literal and decide(bp.step(thr, -1)) != literal


CUBOID_DIMS = [(0.0, 1.5), (-1.0, 0.5), (0.25, 0.7)]


@pytest.mark.parametrize("route", list(BOND_ROUTES))
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_geometry_faces_and_cylinder_ends(built, monkeypatch, axis, route):
    """Offsets 0, -0, the extent and one float either side: `>= 0` and `<= extent`, both inclusive."""
    set_route(monkeypatch, BOND_ROUTES[route])
    for lo, hi in CUBOID_DIMS:
        ps = bp.extent_probes(lo, hi)
        pts = np.full((ps.size, 3), 0.125, dtype=F)
        pts[:, axis] = ps
        dims = [(-0.5, 0.5)] * 3
        dims[axis] = (lo, hi)
        for invert in (False, True):
            cases = [(Geometry(kind=GEOM_CUBOID, reference=GEOMREF_POINT, point=ORIGIN, xdim=dims[0], ydim=dims[1],
                               zdim=dims[2], invert=invert),
                      [bp.inside_cuboid(p, ORIGIN, *dims) != invert for p in pts]),
                     (Geometry(kind=GEOM_CYLINDER, reference=GEOMREF_POINT, point=ORIGIN, radius=1.0, orientation=axis,
                               span=(lo, hi), invert=invert),
                      [bp.inside_cylinder(p, ORIGIN, 1.0, axis, (lo, hi)) != invert for p in pts])]
            for geom, literal in cases:
                tables, xyz, which = slot_system(pts, N_FRAMES, handle_pbc=False, geometry=geom)
                got, want, _, _ = both(tables, xyz)
                np.testing.assert_array_equal(want.counts[0], bp.slot_counts(literal, which))
                np.testing.assert_array_equal(got.counts[0], bp.slot_counts(literal, which),
                                              err_msg=f"kind {geom.kind} axis {axis} dims {(lo, hi)} invert {invert}")
                # the faces themselves are inside, the floats beyond them are not: a strict compare would show
                e = (pts[:, axis] - F(lo)).astype(F)
                strict = [bool((0 < x < F(hi) - F(lo))) != invert for x in e]
                assert strict != literal


PBC_BOX = (12.0, 13.0, 14.0)
PBC_RADII = (2.0, 2.5, 2.3, 1.7, 3.1415927, 0.1, 2.2, 3.0)


@pytest.mark.parametrize("where", ["box centre", "near a face"])
@pytest.mark.parametrize("shape", ["sphere", "cylinder-x", "cylinder-y", "cylinder-z", "cuboid"])
def test_geometry_in_a_periodic_box(built, monkeypatch, shape, where):
    """Around a reference in a periodic box gm_min_image / gm_wrap come before the compare, so the probes are searched
    in the wrapped frame: positions whose literal min-image chain lands on thr and the floats around it, and whose
    wrapped offset IS 0, the extent, or the nearest float either side.  Device == oracle == the literal decision."""
    cases = [periodic_cuboid_case(where, PBC_BOX)] if shape == "cuboid" else \
        [periodic_radius_case(shape, where, PBC_BOX, r) for r in PBC_RADII]
    for geom, pts, literal, mutants in cases:
        for wrong in mutants:              # a threshold one float off, a <=, a strict end: the probes would see it
            assert not np.array_equal(wrong, literal)
        for invert in (False, True):
            geom.invert = invert
            tables, xyz, which = slot_system(pts, N_FRAMES, handle_pbc=True, geometry=geom)
            expect = bp.slot_counts(np.asarray(literal) != invert, which)
            for route, env in BOND_ROUTES.items():
                set_route(monkeypatch, env)
                got, want, _, _ = both(tables, xyz, box9(PBC_BOX, N_FRAMES))
                np.testing.assert_array_equal(want.counts[0], expect, err_msg=f"oracle {shape} {where} r={geom.radius}")
                np.testing.assert_array_equal(got.counts[0], expect, err_msg=f"{shape} {where} r={geom.radius} {route} invert={invert}")
                np.testing.assert_array_equal(got.sums, want.sums)


# ---- ordermap tiles ----------------------------------------------------------------------------------------
FAMILIES = bp.tile_families()
MAP_ROUTES = {"tiled maps": {}, "maps gather": {"GORDER_HIP_MAPS_GATHER": "1"}, "gather": {"GORDER_HIP_KERNEL": "gather"}}


@pytest.mark.parametrize("route", list(MAP_ROUTES))
@pytest.mark.parametrize("plane", [0, 1, 2])
def test_ordermap_tiles_at_the_half_tile_lines(built, monkeypatch, plane, route):
    """map_counts per slot and tile for coordinates on the lines between two tiles and the floats next to them, at the
    first and last tiles, at lo - bin / 2 and lo + (n - 1/2) bin, and for bins outside the division core's range."""
    set_route(monkeypatch, MAP_ROUTES[route])
    for fam in FAMILIES:
        lo, hi, bin, n, _ = fam
        pts, ux, uy = bp.map_points(fam, plane)
        om = OrderMap(enabled=True, plane=plane, span_x=(lo, hi), span_y=(lo, hi), bin=(bin, bin))
        tables, xyz, which = slot_system(pts, N_FRAMES, handle_pbc=False, ordermap=om)
        got, want, eng, _ = both(tables, xyz)
        assert eng.ordermap_dims() == (n, n)
        literal = bp.map_counts(bp.map_tiles(fam, ux, uy), which, n)
        np.testing.assert_array_equal(want.map_counts[0], literal, err_msg=f"oracle lo={lo} bin={bin}")
        np.testing.assert_array_equal(got.map_counts[0], literal, err_msg=f"device lo={lo} bin={bin}")
        np.testing.assert_array_equal(got.map_sums, want.map_sums)
        # half-to-even instead of half-away-from-zero would show in this family
        assert not np.array_equal(bp.map_counts(bp.map_tiles(fam, ux, uy, bp.round_half_even), which, n), literal)


def test_ordermap_dims_where_the_span_is_half_a_bin_over(built):
    """nx, ny = round((hi - lo) / bin) + 1 on the host for spans within an ulp of (m + 1/2) bins."""
    changed = 0
    for lo, hi, bin in bp.half_spans():
        om = OrderMap(enabled=True, plane=0, span_x=(lo, hi), span_y=(lo, bp.step(hi, 1)), bin=(bin, bin))
        tables, _, _ = slot_system(np.zeros((1, 3), dtype=F), 1, handle_pbc=False, ordermap=om)
        want = (bp.n_tiles(lo, hi, bin), bp.n_tiles(lo, bp.step(hi, 1), bin))
        eng = HipEngine(tables)
        assert eng.ordermap_dims() == want, f"lo={lo} hi={hi} bin={bin}"
        eng.close()
        assert oracle.OracleEngine(tables, trig=oracle.TRIG_DIRECT).finish().map_counts.shape[2:] == want
        changed += bp.n_tiles(lo, hi, bin, bp.round_half_even) != want[0]
    assert changed


# ---- local leaflets and dynamic normals: the cylinder / sphere around a head, behind a cell grid ------------
LOCAL_ROUTES = {"default": {}, "three kernels": {"GORDER_HIP_LOCAL_THREE_KERNELS": "1"},
                "atoms only": {"GORDER_HIP_LOCAL_ATOMS_ONLY": "1"}, "no prune": {"GORDER_HIP_LOCAL_NO_PRUNE": "1"}}

def local_sides(tables, xyz, box):
    """-> (device, oracle): 1 where the frame's sample went to the lower leaflet."""
    n = xyz.shape[0]
    _, _, eng, o = both(tables, xyz, box)
    (_, gc), (_, wc) = eng.timewise(n), o.timewise(n)
    assert (gc[:, 0, 0] == 1).all() and (wc[:, 0, 0] == 1).all()
    return gc[:, 2, 0].astype(int), wc[:, 2, 0].astype(int)


@pytest.mark.parametrize("pbc", [False, True])
@pytest.mark.parametrize("route", list(LOCAL_ROUTES))
def test_local_leaflet_cylinder_threshold(built, monkeypatch, route, pbc):
    """ea ea + eb eb < thr in the local-leaflet kernels: one radius probe per frame, the head's side tells."""
    set_route(monkeypatch, LOCAL_ROUTES[route])
    for r in bp.RADII:
        probes = bp.plane_probes(r)
        signs = [(1, 1), (-1, 1), (1, -1), (-1, -1)]
        partners = [(F(p[0] * signs[i % 4][0]), F(p[1] * signs[i % 4][1])) for i, p in enumerate(probes)]
        tables, xyz = local_system([(0.0, 0.0)] * len(probes), partners, pbc, r)
        edge = max(16.0, 4.0 * r)
        box = box9((edge, edge, 40.0), len(probes)) if pbc else None
        got, want = local_sides(tables, xyz, box)
        literal = np.array([int(np.sqrt(p[2]) < F(r)) for p in probes])
        print(f"local {route} pbc={pbc} r={r}: {literal.sum()} of {literal.size} partners inside")
        np.testing.assert_array_equal(want, literal, err_msg=f"oracle r={r}")
        np.testing.assert_array_equal(got, literal, err_msg=f"device r={r}")
        thr = bp.radius_threshold(r)
        d2 = np.array([p[2] for p in probes], dtype=F)
        assert np.array_equal(literal, d2 < thr)
        assert not np.array_equal(literal, d2 < bp.step(thr, 1)) and not np.array_equal(literal, d2 < bp.step(thr, -1))


@pytest.mark.parametrize("route", list(LOCAL_ROUTES))
def test_local_leaflet_heads_on_cell_lines(built, monkeypatch, route):
    """A neighbour a whole radius away of a head that sits exactly on a line of the cell grid, at coordinate 0 or at
    box - ulp: across the line, across the periodic face, on the diagonal — thr - 1 ulp is a member, thr is not."""
    set_route(monkeypatch, LOCAL_ROUTES[route])
    r = 2.0
    L, probes = bp.cell_line_probes(r, bp.K_FINE if route == "atoms only" else bp.K_FINE_ROWS)
    tables, xyz = local_system([p[0] for p in probes], [p[1] for p in probes], True, r)
    got, want = local_sides(tables, xyz, box9((L, L, 40.0), len(probes)))
    literal = np.array([int(p[2]) for p in probes])
    assert len(probes) >= N_FRAMES and 0 < literal.sum() < literal.size
    np.testing.assert_array_equal(want, literal)
    np.testing.assert_array_equal(got, literal)
    # every pair is (thr - 1 float, thr): a threshold one float off either way turns one of each pair
    thr = bp.radius_threshold(r)
    d2 = np.where(literal == 1, bp.step(thr, -1), thr)
    assert np.array_equal(literal, d2 < thr)
    assert not np.array_equal(literal, d2 < bp.step(thr, 1)) and not np.array_equal(literal, d2 < bp.step(thr, -1))


def cloud_sizes(tables, xyz, box):
    """The cloud size of every frame's head, device and oracle: gorder_hip_normals reports the LAST frame of a batch,
    so frame i is read as the last of the nine frames i - 8 .. i."""
    n = xyz.shape[0]
    eng, o = HipEngine(tables), oracle.OracleEngine(tables, trig=oracle.TRIG_DIRECT)
    got, want = [], []
    for i in range(n):
        fr = np.arange(i - N_FRAMES + 1, i + 1) % n
        b = None if box is None else box[fr]
        eng.submit_host(xyz[fr], b, np.arange(N_FRAMES) + i * N_FRAMES)
        eng.finish()
        o.submit(xyz[fr], b, np.arange(N_FRAMES) + i * N_FRAMES)
        got.append(int(eng.normals()[1][0]))
        want.append(int(o.normals()[1][0]))
    return np.array(got), np.array(want)


@pytest.mark.parametrize("pbc", [False, True])
def test_dynamic_normal_cloud_threshold(built, pbc):
    """(dx dx + dy dy) + dz dz < thr in k_dyn_cov: three atoms are always in the cloud, the fourth is a radius probe."""
    for r in bp.RADII:
        probes = bp.space_probes(r)[::2] + bp.space_probes(r)[1::6]
        signs = np.array([[1, 1, 1], [-1, 1, -1], [1, -1, 1], [-1, -1, -1]], dtype=F)
        partners = [(p[0] * signs[i % 4]).astype(F) for i, p in enumerate(probes)]
        tables, xyz = dynamic_system([(0.0, 0.0)] * len(probes), partners, pbc, r)
        edge = max(16.0, 4.0 * r)
        box = box9((edge, edge, edge), len(probes)) if pbc else None
        got, want = cloud_sizes(tables, xyz, box)
        d2 = np.array([p[1] for p in probes], dtype=F)
        literal = 3 + (np.sqrt(d2) < F(r)).astype(int)
        np.testing.assert_array_equal(want, literal, err_msg=f"oracle r={r}")
        np.testing.assert_array_equal(got, literal, err_msg=f"device r={r}")
        thr = bp.radius_threshold(r)
        assert np.array_equal(literal, 3 + (d2 < thr)) and (d2 == thr).any() and (d2 == bp.step(thr, -1)).any()
        assert not np.array_equal(literal, 3 + (d2 < bp.step(thr, 1))) and not np.array_equal(literal, 3 + (d2 < bp.step(thr, -1)))


def test_dynamic_normal_heads_on_cell_lines(built):
    r = 2.0
    L, probes = bp.cell_line_probes(r, bp.K_FINE)
    tables, xyz = dynamic_system([p[0] for p in probes], [p[1] for p in probes], True, r, L)
    got, want = cloud_sizes(tables, xyz, box9((L, L, 40.0), len(probes)))
    literal = np.array([3 + int(p[2]) for p in probes])
    np.testing.assert_array_equal(want, literal)
    np.testing.assert_array_equal(got, literal)
    thr = bp.radius_threshold(r)
    d2 = np.where(literal == 4, bp.step(thr, -1), thr)
    assert np.array_equal(literal, 3 + (d2 < thr))
    assert not np.array_equal(literal, 3 + (d2 < bp.step(thr, 1))) and not np.array_equal(literal, 3 + (d2 < bp.step(thr, -1)))


# ---- united atoms: the sample is a constructed hydrogen, so the shape and the map are fitted to the sample ----
def ua_case(fast=False):
    """One united-atom lipid without periodic boundaries, nine frames -> (system, xyz, bond positions [frames, slots, 3],
    slots whose construction has no data-dependent angle).  The positions are the reference's: hydrogen + (hydrogen -
    target) / 2 (uaorder.rs:375-397), each operation in float32.  `fast`: GORDER_FLAG_UA_FAST_NORMALISE in the tables and
    the positions of the fast construction as the oracle restates it (gorder_oracle_predict_hydrogens_fast)."""
    import ctypes as C
    from gorder_amd import abi, synthetic
    system = synthetic.ua_membrane(1, handle_pbc=False)
    if fast:
        system.tables.flags |= abi.FLAG_UA_FAST_NORMALISE
    xyz = system.frames(N_FRAMES, seed=5)
    pos = np.zeros((N_FRAMES, system.tables.n_acc, 3), dtype=F)
    plain = []
    lib = oracle.load()
    for f in range(N_FRAMES):
        slot = 0
        for kind, idx in system.tables.molecule_types[0].ua_atoms:
            sat = int(kind) == abi.UA_CH1_SAT
            atoms = xyz[f, idx[0, :4 if sat else 3]]
            target = atoms[3 if sat else 1]
            if fast:
                p4, box = np.zeros((4, 3), dtype=F), np.ones(3, dtype=F)
                p4[:len(atoms)] = atoms
                hs, vs, slow = np.zeros((3, 3), dtype=F), np.zeros((3, 3), dtype=F), C.c_int(0)
                nh = lib.gorder_oracle_predict_hydrogens_fast(C.c_uint32(int(kind)), C.c_void_p(p4.ctypes.data),
                                                              C.c_void_p(box.ctypes.data), 0, C.c_void_p(hs.ctypes.data),
                                                              C.c_void_p(vs.ctypes.data), C.byref(slow))
                assert nh == abi.UA_N_H[int(kind)] and not slow.value      # (no carbon of this lipid takes the literal loops)
                pairs = [(hs[k], vs[k]) for k in range(nh)]
            else:
                pairs = [(hy, (hy - target).astype(F)) for hy in oracle.predict_hydrogens(int(kind), atoms, (1.0, 1.0, 1.0), pbc=False)]
            for hy, v in pairs:
                pos[f, slot] = (hy + (v / F(2)).astype(F)).astype(F)
                if f == 0:
                    plain.append(int(kind) != abi.UA_CH1_UNSAT)
                slot += 1
    return system, xyz, pos, np.array(plain)


def fitted_radii(d2, plain, wanted=8):
    """{radius: (frame, slot)}: radii whose threshold IS a sample's squared distance (that sample is outside) or the float
    above it (inside), alternately."""
    radii = {}
    for (f, s), v in np.ndenumerate(d2):
        if not plain[s] or len(radii) >= wanted:
            continue
        for k in (-1, 0, 1):
            r = bp.step(np.sqrt(v), k)
            thr = bp.radius_threshold(r)
            if (v == thr and len(radii) % 2 == 0) or (v == bp.step(thr, -1) and len(radii) % 2 == 1):
                radii[float(r)] = (f, s)
                break
    assert len(radii) >= 4, "too few samples can be met by a radius"
    return radii


@pytest.mark.parametrize("shape", ["sphere", "cylinder-x", "cylinder-y", "cylinder-z"])
def test_united_atom_samples_on_a_shape_fitted_to_them(built, shape):
    """k_ua_extras: radii chosen so that a hydrogen sample's squared distance from the shape's centre or axis IS thr
    (outside) or the float below (inside); inverted and not."""
    system, xyz, pos, plain = ua_case()
    if shape == "sphere":
        d2 = np.array([[bp.dist2_space(*p) for p in fr] for fr in pos], dtype=F)
    else:
        o = "xyz".index(shape[-1])
        d2 = np.array([[bp.dist2_plane(p[(o + 1) % 3], p[(o + 2) % 3]) for p in fr] for fr in pos], dtype=F)
    for r, (f, s) in fitted_radii(d2, plain).items():
        thr = bp.radius_threshold(r)
        literal = np.sqrt(d2) < F(r)
        assert d2[f, s] in (thr, bp.step(thr, -1)) and np.array_equal(literal, d2 < thr)
        # the fitted sample alone makes a threshold one float off visible
        assert (d2 < bp.step(thr, 1))[f, s] != literal[f, s] or (d2 < bp.step(thr, -1))[f, s] != literal[f, s]
        for invert in (False, True):
            kw = dict(kind=GEOM_SPHERE) if shape == "sphere" else dict(kind=GEOM_CYLINDER, orientation=o)
            system.tables.geometry = Geometry(reference=GEOMREF_POINT, point=ORIGIN, radius=r, invert=invert, **kw)
            got, want, _, _ = both(system.tables, xyz)
            np.testing.assert_array_equal(want.counts[0][plain], (literal != invert).sum(axis=0)[plain])
            np.testing.assert_array_equal(got.counts[0], want.counts[0], err_msg=f"{shape} r={r!r} fitted to frame {f} slot {s}")


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_united_atom_samples_on_a_cuboid_face_fitted_to_them(built, axis):
    """k_ua_extras: a cuboid from 0 to a hydrogen sample's own coordinate — the sample's offset IS the extent (inside)."""
    system, xyz, pos, plain = ua_case()
    for f, s in ((0, 3), (4, 30), (8, 50)):
        assert plain[s]
        hi = pos[f, s, axis]
        dims = [(-np.inf, np.inf)] * 3
        dims[axis] = (0.0, float(hi))
        literal = np.array([[bp.inside_cuboid(p, ORIGIN, *dims) for p in fr] for fr in pos])
        strict = (pos[:, :, axis] > 0) & (pos[:, :, axis] < hi)
        assert literal[f, s] and not strict[f, s]
        for invert in (False, True):
            system.tables.geometry = Geometry(kind=GEOM_CUBOID, reference=GEOMREF_POINT, point=ORIGIN, xdim=dims[0],
                                              ydim=dims[1], zdim=dims[2], invert=invert)
            got, want, _, _ = both(system.tables, xyz)
            np.testing.assert_array_equal(want.counts[0][plain], (literal != invert).sum(axis=0)[plain])
            np.testing.assert_array_equal(got.counts[0], want.counts[0], err_msg=f"axis {axis} extent {hi!r}")


def fitted_bins(xs, plain, wanted=6):
    """{bin: (frame, slot, m)}: bin widths for which a sample's literal quotient x / bin IS m + 1/2, odd and even m."""
    bins = {}
    for parity in (1, 0, 1, 0, 1, 0):
        for (f, s), x in np.ndenumerate(xs):
            if not plain[s] or not x > 1 or any(v[:2] == (f, s) for v in bins.values()):
                continue
            m = int(float(x) / 0.3)
            m += (m % 2) != parity
            b0 = F(float(x) / (m + 0.5))
            hit = [k for k in sorted(range(-8, 9), key=abs) if float(bp.tile_quotient(x, 0.0, bp.step(b0, k))) == m + 0.5]
            if hit:
                bins[float(bp.step(b0, hit[0]))] = (f, s, m)
                break
    assert len(bins) >= 3 and any(m % 2 == 0 for _, _, m in bins.values()), "too few samples can be put on a half-tile line"
    return bins


def ua_map_literal(pos, lo, hi, b, index):
    """map_counts[0] [slots, nx, ny] for bond positions pos, x binned by `index`(x, lo, b, nx), y by 0.9-nm tiles."""
    nx, ny = bp.n_tiles(lo, hi, b), bp.n_tiles(0.0, 9.0, 0.9)
    out = np.zeros((pos.shape[1], nx, ny), dtype=np.uint64)
    for (f, s), _ in np.ndenumerate(pos[:, :, 0]):
        ix, iy = index(pos[f, s, 0], lo, b, nx), bp.tile_index(pos[f, s, 1], 0.0, 0.9, ny)
        if ix >= 0 and iy >= 0:
            out[s, ix, iy] += 1
    return out


@pytest.mark.parametrize("direct", [False, True])
def test_united_atom_samples_on_a_tile_line_fitted_to_them(built, monkeypatch, direct):
    """United-atom ordermaps, staged (k_ua_extras + k_map_accumulate) and with GORDER_HIP_MAP_DIRECT=1: bin widths chosen
    so that a hydrogen sample's quotient IS m + 1/2."""
    set_route(monkeypatch, {"GORDER_HIP_MAP_DIRECT": "1"} if direct else {})
    system, xyz, pos, plain = ua_case()
    bins = fitted_bins(pos[:, :, 0], plain)
    even_differs = 0
    for b, (f, s, m) in bins.items():
        system.tables.ordermap = OrderMap(enabled=True, plane=0, span_x=(0.0, 9.0), span_y=(0.0, 9.0), bin=(b, 0.9))
        got, want, eng, _ = both(system.tables, xyz)
        literal = ua_map_literal(pos, 0.0, 9.0, b, bp.tile_index)
        assert eng.ordermap_dims() == literal.shape[1:]
        np.testing.assert_array_equal(want.map_counts[0][plain], literal[plain])
        np.testing.assert_array_equal(got.map_counts[0], want.map_counts[0], err_msg=f"bin={b!r} fitted to frame {f} slot {s}")
        nx = literal.shape[1]
        assert bp.tile_index(pos[f, s, 0], 0.0, b, nx) == m + 1
        even_differs += bp.tile_index(pos[f, s, 0], 0.0, b, nx, bp.round_half_even) != m + 1
    assert even_differs, "half-to-even would put every fitted sample into the same tile: fit an even m"


def fast_tile_index(x, lo, bin, n):
    """grid_index_fast (kernels_bonds.h) restated: floor(fma(x - lo, 1 / bin, 1/2)) — the product of two floats and the
    sum with 1/2 are exact in float64 for these magnitudes, so one rounding to float32, like the fma."""
    d, inv = F(F(x) - F(lo)), F(F(1.0) / F(bin))
    k = float(np.floor(F(np.float64(d) * np.float64(inv) + 0.5)))
    return int(k) if 0.0 <= k < float(n) else -1


def near_a_line(x, lo, bin, n, ulps=2):
    """The offset x - lo that both forms divide is within `ulps` floats of one whose literal tile is another."""
    d = F(F(x) - F(lo))
    return bp.tile_index(bp.step(d, -ulps), 0.0, bin, n) != bp.tile_index(bp.step(d, ulps), 0.0, bin, n)


@pytest.mark.parametrize("direct", [False, True])
def test_united_atom_fast_tile_index_at_the_half_tile_lines(built, monkeypatch, direct):
    """GORDER_FLAG_UA_FAST_NORMALISE: the tile is floor(fma(x - lo, 1 / bin, 1/2)) (k_ua_extras_fast).  The maps must EQUAL
    the oracle's fast mode (gridmap_index_fast) for bins fitted so that a sample's literal quotient IS m + 1/2 and for
    the bins and origins of the tile probes; and — the documented bound — a sample whose offset x - lo is not within two
    floats of a half-tile line lands in the literal tile."""
    set_route(monkeypatch, {"GORDER_HIP_MAP_DIRECT": "1"} if direct else {})
    system, xyz, pos, plain = ua_case(fast=True)
    cases = [(0.0, b) for b in fitted_bins(pos[:, :, 0], plain)] + [(lo, b) for b in bp.BINS for lo in bp.LOS]
    near_total = moved = 0
    for lo, b in cases:
        hi = float(F(lo) + F(10.0))
        system.tables.ordermap = OrderMap(enabled=True, plane=0, span_x=(lo, hi), span_y=(0.0, 9.0), bin=(b, 0.9))
        got, want, eng, _ = both(system.tables, xyz)
        nx = bp.n_tiles(lo, hi, b)
        np.testing.assert_array_equal(got.map_counts, want.map_counts, err_msg=f"lo={lo} bin={b!r}")
        np.testing.assert_array_equal(got.map_sums, want.map_sums)
        fast = ua_map_literal(pos, lo, hi, b, fast_tile_index)
        np.testing.assert_array_equal(want.map_counts[0][plain], fast[plain], err_msg="the restated fast index is not the oracle's")
        for (f, s), x in np.ndenumerate(pos[:, :, 0]):
            near = near_a_line(x, lo, b, nx)
            near_total += near
            moved += fast_tile_index(x, lo, b, nx) != bp.tile_index(x, lo, b, nx)
            assert near or fast_tile_index(x, lo, b, nx) == bp.tile_index(x, lo, b, nx), \
                f"x={x!r} lo={lo} bin={b!r}: more than two floats from a line, yet in another tile than the literal one"
    assert near_total >= len(cases) - 18, "the fitted bins put no sample next to a line"
    print(f"fast tile index: {near_total} samples within two floats of a line, {moved} in another tile than the literal one")
