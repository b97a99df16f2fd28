"""Radial profiles (gorder_hip_set_radial_shells, k_bonds_shells): the sums and counts of every shell r[k-1] <= d < r[k]
around the reference of a cylinder or sphere selection, made in the same pass as the selection's own sums.

The reference for shell k is oracle(radius r[k]) - oracle(radius r[k-1]) (oracle(r[0]) for the first): membership is
`sqrtf(d2) < r` and nothing else in the test depends on the radius, so selections of increasing radius around one
reference are nested exactly.  Every comparison of sums and counts is integer EQUAL."""
import dataclasses

import numpy as np
import pytest

from gorder_amd import HipEngine, abi, synthetic
from gorder_amd import structure as st
from gorder_amd.abi import (GEOM_CUBOID, GEOM_CYLINDER, GEOM_SPHERE, GEOMREF_BOX_CENTER, GEOMREF_GROUP, GEOMREF_POINT,
                            LEAFLETS_GLOBAL, LEAFLETS_INDIVIDUAL, LEAFLETS_MANUAL, LEAFLETS_NONE, Geometry, OrderMap)
from oracle import oracle

pytestmark = pytest.mark.gpu

CYL_RADII = (0.7, 1.5, 2.2, 3.1)
SPH_RADII = (1.5, 2.5, 3.5, 4.5)
N = 9

GEOMS = {
    "cylinder-group-span": (Geometry(kind=GEOM_CYLINDER, reference=GEOMREF_GROUP, span=(-2.0, 2.5), orientation=2), CYL_RADII),
    "cylinder-point-x": (Geometry(kind=GEOM_CYLINDER, reference=GEOMREF_POINT, point=(1.0, 3.0, 5.0), orientation=0), CYL_RADII),
    "cylinder-centre": (Geometry(kind=GEOM_CYLINDER, reference=GEOMREF_BOX_CENTER, orientation=2), CYL_RADII),
    "sphere-group": (Geometry(kind=GEOM_SPHERE, reference=GEOMREF_GROUP), SPH_RADII),
    "sphere-point": (Geometry(kind=GEOM_SPHERE, reference=GEOMREF_POINT, point=(3.3, 3.2, 5.0)), SPH_RADII),
}


def f32(radii):
    return [float(np.float32(r)) for r in radii]


def membrane(pbc=True, leaflets=LEAFLETS_GLOBAL, **kw):
    return synthetic.cg_membrane(160, leaflets=leaflets, n_types=2, handle_pbc=pbc, **kw)


def with_geometry(system, geom, radius, pbc):
    geom = dataclasses.replace(geom, radius=float(np.float32(radius)), structure_box=tuple(float(x) for x in system.box))
    if geom.reference == GEOMREF_GROUP:
        p0 = system.frames(1, seed=0)[0].astype(np.float64)      # a localised group (2-nm blob): its centre is well defined
        d = p0 - p0[0]
        if pbc:
            d -= system.box.astype(np.float64) * np.round(d / system.box.astype(np.float64))
        geom.group = np.flatnonzero(np.linalg.norm(d, axis=1) < 2.0).astype(np.uint32)
    system.tables.geometry = geom
    return system.tables


def batches_of(n, k=2):
    e = np.linspace(0, n, k + 1).astype(int)
    return [(int(a), int(b)) for a, b in zip(e[:-1], e[1:]) if b > a]


def oracle_nested(tables, radii, xyz, box, trig=oracle.TRIG_DIRECT, feed=None):
    """[(sums, counts)] per shell: the integer differences of the oracle's selections of radius r[k] and r[k - 1]; and the
    oracle's Results at the outer radius."""
    nested = []
    for r in f32(radii):
        t = dataclasses.replace(tables, geometry=dataclasses.replace(tables.geometry, radius=r))
        o = oracle.OracleEngine(t, trig=trig, n_threads=2)
        if feed is None:
            o.submit(xyz, box, np.arange(len(xyz)))
        else:
            feed(o)
        nested.append(o.finish())
    shells = []
    for k, res in enumerate(nested):
        s, c = res.sums.copy(), res.counts.astype(np.int64)
        if k:
            s -= nested[k - 1].sums
            c -= nested[k - 1].counts.astype(np.int64)
        assert (c >= 0).all()           # nested exactly
        shells.append((s, c.astype(np.uint64)))
    return shells, nested[-1]


def device_shells(tables, radii, xyz, box, cuts=None, before=None):
    eng = HipEngine(tables)
    eng.set_radial_shells(f32(radii))
    if before:
        before(eng)
    for a, b in cuts or batches_of(len(xyz)):
        eng.submit_host(xyz[a:b], None if box is None else box[a:b], np.arange(a, b))
    shells = eng.radial_shells()
    return eng, shells, eng.finish()


def same_shells(got, want):
    assert len(got) == len(want)
    for k, (res, (s, c)) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(res.counts, c, err_msg=f"counts of shell {k}")
        np.testing.assert_array_equal(res.sums, s, err_msg=f"sums of shell {k}")


def add_up(shells):
    return sum(r.sums for r in shells), sum(r.counts for r in shells)


def check_all(shells, total, want_shells, want_total):
    same_shells(shells, want_shells)
    s, c = add_up(shells)
    np.testing.assert_array_equal(c, total.counts)
    np.testing.assert_array_equal(s, total.sums)
    np.testing.assert_array_equal(total.counts, want_total.counts)
    np.testing.assert_array_equal(total.sums, want_total.sums)


def case(name, pbc):
    geom, radii = GEOMS[name]
    system = membrane(pbc)
    tables = with_geometry(system, geom, radii[-1], pbc)
    return system, tables, radii, system.frames(N, seed=13), system.box9(N) if pbc else None


CASES_1 = [(g, p) for g in GEOMS for p in (True, False) if p or g != "cylinder-centre"]


@pytest.fixture(scope="module")
def first_case(built):
    """Test 1's first case and its oracle differences, shared by the tests that rerun it."""
    system, tables, radii, xyz, box = case("cylinder-group-span", True)
    want_shells, want_total = oracle_nested(tables, radii, xyz, box)
    return tables, radii, xyz, box, want_shells, want_total


@pytest.mark.parametrize("name,pbc", CASES_1)
def test_shells_against_nested_selections(built, name, pbc):
    system, tables, radii, xyz, box = case(name, pbc)
    want_shells, want_total = oracle_nested(tables, radii, xyz, box)
    eng, shells, total = device_shells(tables, radii, xyz, box)
    assert total.n_frames == N and all(r.n_frames == N for r in shells)
    check_all(shells, total, want_shells, want_total)
    both = [k for k, r in enumerate(shells) if r.counts[1].sum() > 0 and r.counts[2].sum() > 0]
    assert len(both) >= 3


FAN_RADII = (0.75, 1.5, 2.5, 3.25)


def ulp_fan():
    """No PBC, a cylinder along z around the point (4, 3, 5).  In frame 1 the first bond of lipids 0..63 has its midpoint at
    in-plane offset (x, 0), x = radius m % 4 stepped by m // 4 - 8 ulps (np.nextafter), its atoms at x -+ 0.125 in the plane and
    -+ 0.25 along the axis.  `away` is the same trajectory with those 64 bonds far outside every radius: the difference of
    the oracle's counts on the two tells where the placed samples fall.
    With these positions the CPU oracle puts 4 / 18 / 17 / 16 of the 64 samples into the four shells and 9 outside: of the 16
    samples around each radius 4, 6, 7 and 7 fall below it, so both sides of every threshold are hit."""
    system = membrane(False)
    geom = Geometry(kind=GEOM_CYLINDER, reference=GEOMREF_POINT, point=(4.0, 3.0, 5.0), orientation=2)
    tables = with_geometry(system, geom, FAN_RADII[-1], False)
    xyz = system.frames(3, seed=4)
    away = xyz.copy()
    for m in range(64):
        i, j = 12 * m, 12 * m + 1                  # the lipid's first bond (synthetic._CG_BONDS)
        x = np.float32(FAN_RADII[m % 4])
        steps = m // 4 - 8
        for _ in range(abs(steps)):
            x = np.nextafter(x, np.float32(np.inf if steps > 0 else -np.inf))
        xyz[1, i] = (np.float32(4.0) + (x - np.float32(0.125)), np.float32(3.0), np.float32(5.25))
        xyz[1, j] = (np.float32(4.0) + (x + np.float32(0.125)), np.float32(3.0), np.float32(5.75))
        away[1, i], away[1, j] = (100.0, 100.0, 5.25), (100.25, 100.0, 5.75)
    return tables, xyz, away


@pytest.fixture(scope="module")
def fan(built):
    tables, xyz, away = ulp_fan()
    want_shells, want_total = oracle_nested(tables, FAN_RADII, xyz, None)
    # where the placed samples fall: slot 0 of either molecule type is the lipids' first bond
    first_bond = [0, tables.molecule_types[0].n_bond_types]
    with_fan, _ = oracle_nested(tables, FAN_RADII, xyz[1:2], None)
    without, _ = oracle_nested(tables, FAN_RADII, away[1:2], None)
    placed = [int(a[1][0][first_bond].sum()) - int(b[1][0][first_bond].sum()) for a, b in zip(with_fan, without)]
    return tables, xyz, want_shells, want_total, placed


@pytest.mark.parametrize("chunks", ["a frame per workgroup", "one workgroup per tile"])
@pytest.mark.parametrize("direct", [False, True])
def test_one_ulp_fan_across_every_radius(fan, monkeypatch, direct, chunks):
    """The default launch cuts a batch this short into chunks of one frame.  With GORDER_HIP_WG_TARGET=1 one workgroup walks
    all three frames of a tile: the 64 placed bonds sit elsewhere in frames 0 and 2, so their threads close the open word
    of one shell and open another's twice."""
    if chunks == "one workgroup per tile":
        monkeypatch.setenv("GORDER_HIP_WG_TARGET", "1")
    tables, xyz, want_shells, want_total, placed = fan
    assert placed == [4, 18, 17, 16]
    below, carried = [], 0                       # of the 16 samples around radius q: how many fall below it
    for n in placed:
        below.append(n - carried)
        carried = 16 - below[-1]
    assert all(0 < n < 16 for n in below)        # both sides of every threshold are hit
    if direct:
        monkeypatch.setenv("GORDER_HIP_RADIAL_DIRECT", "1")
    eng, shells, total = device_shells(tables, FAN_RADII, xyz, None, cuts=[(0, 3)])
    check_all(shells, total, want_shells, want_total)


def test_the_two_routes_agree(first_case, monkeypatch):
    tables, radii, xyz, box, want_shells, want_total = first_case
    _, lds_shells, lds_total = device_shells(tables, radii, xyz, box)
    monkeypatch.setenv("GORDER_HIP_RADIAL_DIRECT", "1")
    _, shells, total = device_shells(tables, radii, xyz, box)
    check_all(shells, total, want_shells, want_total)
    monkeypatch.setenv("GORDER_HIP_WG_TARGET", "1")         # ... and with one workgroup per tile and batch (4 and 5 frames)
    for route in ("1", "0"):
        monkeypatch.setenv("GORDER_HIP_RADIAL_DIRECT", route)
        _, long_shells, long_total = device_shells(tables, radii, xyz, box)
        check_all(long_shells, long_total, want_shells, want_total)
    same_shells(shells, [(r.sums, r.counts) for r in lds_shells])
    np.testing.assert_array_equal(total.sums, lds_total.sums)
    np.testing.assert_array_equal(total.counts, lds_total.counts)


def test_one_shell_is_the_plain_selection(first_case):
    tables, radii, xyz, box, want_shells, want_total = first_case
    eng, shells, total = device_shells(tables, radii[-1:], xyz, box)
    assert len(shells) == 1
    np.testing.assert_array_equal(shells[0].sums, want_total.sums)
    np.testing.assert_array_equal(shells[0].counts, want_total.counts)
    np.testing.assert_array_equal(total.sums, want_total.sums)
    np.testing.assert_array_equal(total.counts, want_total.counts)


def test_thirty_two_shells_and_the_empty_ones(built):
    """Radii 0.2 (k + 1) in the 7.2-nm periodic box: the minimum image keeps every in-plane distance below 7.2 / sqrt(2) =
    5.1 nm, so the shells from 5.2 nm on are empty: all zero, their order NaN."""
    radii = [0.2 * (k + 1) for k in range(abi.RADIAL_MAX_SHELLS)]
    system = membrane(True)
    assert abs(float(system.box[0]) - 7.2) < 1e-5 and abs(float(system.box[1]) - 7.2) < 1e-5
    tables = with_geometry(system, Geometry(kind=GEOM_CYLINDER, reference=GEOMREF_BOX_CENTER, orientation=2), radii[-1], True)
    xyz, box = system.frames(4, seed=21), system.box9(4)
    want_shells, want_total = oracle_nested(tables, radii, xyz, box)
    eng, shells, total = device_shells(tables, radii, xyz, box)
    check_all(shells, total, want_shells, want_total)
    empty = [k for k, r in enumerate(shells) if r.counts[0].sum() == 0]
    assert empty and set(range(26, 32)) <= set(empty)
    for k in empty:
        assert not shells[k].sums.any() and not shells[k].counts.any()
        assert np.isnan(shells[k].order()).all()
    groups = [list(range(tables.n_acc))]
    prof = st.radial_profile(shells, f32(radii), groups, "cg")
    assert np.isnan(prof[0, :, empty]).all() and np.isfinite(prof[0, 0, 5])


def test_a_chunk_longer_than_the_packed_words_allow_is_cut(built, monkeypatch):
    """GORDER_HIP_WG_TARGET=1 asks for one workgroup per tile over all 4100 frames of the batch: more than the 4096 frames
    a workgroup's packed table words are proven for (kShellChunkMax), so the host cuts the range in two.  The beads jitter
    by 0.3 nm, so inside a chunk a thread's sample moves between shells, and in and out of the selection, many times."""
    monkeypatch.setenv("GORDER_HIP_WG_TARGET", "1")
    n = 4100
    system = synthetic.cg_membrane(16, leaflets=LEAFLETS_GLOBAL, handle_pbc=True)
    system.jitter = 0.3
    radii = (0.5, 0.9, 1.3)
    tables = with_geometry(system, Geometry(kind=GEOM_CYLINDER, reference=GEOMREF_BOX_CENTER, orientation=2), radii[-1], True)
    xyz, box = system.frames(n, seed=2), system.box9(n)
    # the shell of every lipid's first bond per frame (f64, min image about the box centre): it changes between
    # neighbouring frames of the first chunk thousands of times — far more than rounding at a threshold could explain away
    i, j = np.arange(16) * 12, np.arange(16) * 12 + 1
    edge = system.box.astype(np.float64)[:2]
    v = xyz[:, j, :2].astype(np.float64) - xyz[:, i, :2]
    mid = xyz[:, i, :2] + (v - edge * np.round(v / edge)) / 2 - edge / 2
    d = np.linalg.norm(mid - edge * np.round(mid / edge), axis=2)
    shell = np.searchsorted(np.array(radii), d, side="right")          # len(radii): outside
    inside = (shell[:-1] < len(radii)) & (shell[1:] < len(radii))
    assert ((shell[:-1] != shell[1:]) & inside)[:4095].sum() > 1000
    want_shells, want_total = oracle_nested(tables, radii, xyz, box)
    eng, shells, total = device_shells(tables, radii, xyz, box, cuts=[(0, n)])
    check_all(shells, total, want_shells, want_total)
    assert all(r.counts[0].sum() > 0 for r in shells)


def test_literal_cosine(built):
    system, tables, radii, xyz, box = case("sphere-group", True)
    tables.flags = abi.FLAG_TRIG_ACOS_COS
    want_shells, want_total = oracle_nested(tables, radii, xyz, box, trig=oracle.TRIG_MIRROR)
    eng, shells, total = device_shells(tables, radii, xyz, box)
    check_all(shells, total, want_shells, want_total)


def test_general_normal(built):
    geom, radii = GEOMS["cylinder-point-x"]
    s = float(np.float32(1.0 / np.sqrt(2.0)))
    system = membrane(True, normal=(s, s, 0.0))
    tables = with_geometry(system, geom, radii[-1], True)
    xyz, box = system.frames(N, seed=13), system.box9(N)
    want_shells, want_total = oracle_nested(tables, radii, xyz, box)
    eng, shells, total = device_shells(tables, radii, xyz, box)
    check_all(shells, total, want_shells, want_total)


def test_individual_leaflets(built):
    geom, radii = GEOMS["cylinder-group-span"]
    system = membrane(True, leaflets=LEAFLETS_INDIVIDUAL)
    tables = with_geometry(system, geom, radii[-1], True)
    xyz, box = system.frames(N, seed=13), system.box9(N)
    want_shells, want_total = oracle_nested(tables, radii, xyz, box)
    eng, shells, total = device_shells(tables, radii, xyz, box)
    check_all(shells, total, want_shells, want_total)
    assert total.counts[1].sum() > 0 and total.counts[2].sum() > 0


def test_manual_leaflet_table_that_alternates(built, monkeypatch):
    """A manual table at frequency 2 whose flags alternate per assignment frame.  GORDER_HIP_WG_TARGET=1 makes one workgroup
    per tile walk all 8 frames of the one batch (the default launch would give every frame a workgroup of its own), so
    every molecule changes side three times inside a workgroup's frame range and a thread's open word has to be closed
    and reopened in the other plane."""
    monkeypatch.setenv("GORDER_HIP_WG_TARGET", "1")
    geom, radii = GEOMS["cylinder-group-span"]
    system = membrane(True, leaflets=LEAFLETS_MANUAL, frequency=2)
    tables = with_geometry(system, geom, radii[-1], True)
    n = 8
    xyz, box = system.frames(n, seed=13), system.box9(n)
    n_mol = tables.n_molecules_total
    rows = np.zeros((n // 2, n_mol), dtype=np.uint8)
    rows[0::2, 0::2] = 1
    rows[1::2, 1::2] = 1

    def feed(o):
        for r in range(n // 2):
            fr = np.arange(2 * r, 2 * r + 2)
            o.set_manual_leaflets(rows[r], 2 * r)
            o.submit(xyz[fr], box[fr], fr)

    want_shells, want_total = oracle_nested(tables, radii, xyz, box, feed=feed)
    eng, shells, total = device_shells(tables, radii, xyz, box, cuts=[(0, n)], before=lambda e: e.set_manual_leaflet_table(rows))
    check_all(shells, total, want_shells, want_total)
    assert total.counts[1].sum() > 0 and total.counts[2].sum() > 0


def run_with_error(tables, radii, xyz, box, cuts):
    eng = HipEngine(tables)
    if radii is not None:
        eng.set_radial_shells(f32(radii))
    with pytest.raises(abi.GorderHipError) as e:
        for a, b in cuts:
            eng.submit_host(xyz[a:b], box[a:b], np.arange(a, b))
        eng.finish()
    return e.value


def test_errors_unchanged(built):
    # (no leaflets: the global classifier reads every atom and would meet the undefined position first)
    geom, radii = GEOMS["cylinder-group-span"]
    system = membrane(True, leaflets=LEAFLETS_NONE)
    tables = with_geometry(system, geom, radii[-1], True)
    xyz, box = system.frames(N, seed=13), system.box9(N)
    cuts = [(0, 3), (3, 6), (6, 9)]
    atom = int(tables.molecule_types[1].bonds[2, 5, 1])
    bad = xyz.copy()
    bad[4, atom, 0] = np.nan
    plain, shelled = run_with_error(tables, None, bad, box, cuts), run_with_error(tables, radii, bad, box, cuts)
    assert plain.status == abi.ERR_UNDEFINED_POSITION
    assert (shelled.status, shelled.index, shelled.frame) == (plain.status, plain.index, plain.frame)
    assert shelled.frame == 4
    far = xyz.copy()
    far[4, atom] = 1e9
    plain, shelled = run_with_error(tables, None, far, box, cuts), run_with_error(tables, radii, far, box, cuts)
    assert plain.status == abi.ERR_BOX_RANGE and shelled.status == abi.ERR_BOX_RANGE


def refused(tables, radii, before=None):
    eng = HipEngine(tables)
    if before:
        before(eng)
    with pytest.raises(abi.GorderHipError) as e:
        eng.set_radial_shells(radii)
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
    return str(e.value)


def test_refused_combinations(built):
    geom, radii = GEOMS["cylinder-centre"]
    radii = f32(radii)

    def tables_of(system, g=geom, radius=radii[-1]):
        return with_geometry(system, g, radius, True)

    assert "cylinder or sphere" in refused(membrane().tables, radii)
    cuboid = Geometry(kind=GEOM_CUBOID, reference=GEOMREF_BOX_CENTER, xdim=(-2.0, 2.0))
    assert "cylinder or sphere" in refused(tables_of(membrane(), cuboid), radii)
    assert "inverted" in refused(tables_of(membrane(), dataclasses.replace(geom, invert=True)), radii)
    assert "united-atom" in refused(tables_of(synthetic.ua_membrane(24)), radii)
    om = OrderMap(enabled=True, plane=0, span_x=(0.0, 7.2), span_y=(0.0, 7.2), bin=(0.4, 0.4))
    assert "ordermaps" in refused(tables_of(membrane(ordermap=om)), radii)
    assert "timewise" in refused(tables_of(membrane(timewise=True)), radii)
    dyn = membrane()
    dyn.tables.dynamic_normal = abi.DynamicNormal(enabled=True, radius=2.0, cloud=np.concatenate([m.heads for m in dyn.tables.molecule_types]))
    for m in dyn.tables.molecule_types:
        m.normal_heads = m.heads
    assert "dynamic" in refused(tables_of(dyn), radii)
    # GORDER_COLLECT_NORMALS exists on a handle with dynamic normals only (set_collect): refused with them
    assert "dynamic" in refused(tables_of(dyn), radii, before=lambda e: e.set_collect(abi.COLLECT_NORMALS))
    t = tables_of(membrane())
    n_mol = t.n_molecules_total
    up = np.tile(np.array([0.0, 0.0, 1.0], dtype=np.float32), (2, n_mol, 1))
    assert "normal table" in refused(t, radii, before=lambda e: e.set_manual_normal_table(up))
    assert "gorder_hip_set_normals" in refused(t, radii, before=lambda e: e.set_normals(up))
    # ... and the other way round: a handle with shells takes no normals
    eng = HipEngine(t)
    eng.set_radial_shells(radii)
    for call in (lambda: eng.set_normals(up), lambda: eng.set_manual_normal_table(up)):
        with pytest.raises(abi.GorderHipError) as e:
            call()
        assert e.value.status == abi.ERR_INVALID_ARGUMENT and "radial shells" in str(e.value)
    # the radii themselves
    assert "ascending" in refused(t, [0.7, 2.2, 1.5, radii[-1]])
    assert "ascending" in refused(t, [0.7, 0.7, radii[-1]])
    assert "finite" in refused(t, [0.7, float("nan"), radii[-1]])
    assert "finite" in refused(t, [0.7, float("inf")])
    assert "finite" in refused(t, [0.0, radii[-1]])
    assert "GORDER_RADIAL_MAX_SHELLS" in refused(t, list(np.linspace(0.05, radii[-1], 33)))
    assert "geometry.radius" in refused(t, [0.7, 1.5, float(np.nextafter(np.float32(radii[-1]), np.float32(0)))])
    # after the first submit
    system = membrane()
    t = tables_of(system)
    eng = HipEngine(t)
    eng.submit_host(system.frames(1), system.box9(1), np.arange(1))
    with pytest.raises(abi.GorderHipError) as e:
        eng.set_radial_shells(radii)
    assert e.value.status == abi.ERR_INVALID_ARGUMENT and "first submit" in str(e.value)
    eng.reset()
    eng.set_radial_shells(radii)          # right after reset: accepted


def test_lifecycle(first_case):
    tables, radii, xyz, box, want_shells, want_total = first_case
    eng = HipEngine(tables)
    eng.kernel_time()                     # switches the timing on
    eng.set_radial_shells(f32(radii))
    cuts = batches_of(N)
    for a, b in cuts:
        eng.submit_host(xyz[a:b], box[a:b], np.arange(a, b))
    first = eng.radial_shells()
    same_shells(first, want_shells)
    same_shells(eng.radial_shells(), want_shells)      # reading twice changes nothing
    eng.kernel_time()
    assert "k_bonds_shells" in eng.kernel_names() and "k_bonds_extras" not in eng.kernel_names()
    assert "k_bonds_shells" in [g[0] for g in eng.kernel_groups()]
    eng.reset()
    for r in eng.radial_shells():
        assert not r.sums.any() and not r.counts.any() and r.n_frames == 0
    for a, b in cuts:
        eng.submit_host(xyz[a:b], box[a:b], np.arange(a, b))
    same_shells(eng.radial_shells(), want_shells)      # the radii stayed
    # a handle that never asks for shells runs what it ran before, with the same result
    plain = HipEngine(tables)
    plain.kernel_time()
    for a, b in cuts:
        plain.submit_host(xyz[a:b], box[a:b], np.arange(a, b))
    total = plain.finish()
    plain.kernel_time()
    assert "k_bonds_shells" not in plain.kernel_names() and "k_bonds_extras" in plain.kernel_names()
    assert plain.radial_shells() == []
    np.testing.assert_array_equal(total.sums, want_total.sums)
    np.testing.assert_array_equal(total.counts, want_total.counts)


def test_the_references_own_data(built):
    """golden_cases._cg_sphere: a sphere of 2.5 nm around `resid 1` of the reference's coarse-grained membrane, in three
    shells; added up they print the reference's own result file."""
    from golden_cases import _cg_sphere
    from golden_util import Fixture, expected
    c = _cg_sphere({"cg": Fixture("cg")})
    radii = (0.9, 1.7, 2.5)
    xyz = np.ascontiguousarray(c.fx.xyz[c.frames][:, c.midx, :])
    box = c.fx.boxes[c.frames]
    eng = HipEngine(c.tables)
    eng.set_radial_shells(f32(radii))
    half = (len(c.frames) + 1) // 2
    for a, b in ((0, half), (half, len(c.frames))):
        eng.submit_host(xyz[a:b], box[a:b], c.fidx[a:b])
    shells = eng.radial_shells()
    s, cnt = add_up(shells)
    bad = st.compare_trees(st.results_tree(abi.Results(s, cnt, shells[0].n_frames), c.labels, "cg", c.leaflets, c.min_samples),
                           expected("cg_order_sphere.yaml"))
    assert not bad, bad[:10]
    assert all(r.counts[0].sum() > 0 for r in shells)

    def feed(o):
        o.submit(xyz, box, c.fidx)

    want_shells, want_total = oracle_nested(c.tables, radii, xyz, box, feed=feed)
    same_shells(shells, want_shells)
    total = eng.finish()
    np.testing.assert_array_equal(total.sums, want_total.sums)
    np.testing.assert_array_equal(total.counts, want_total.counts)
