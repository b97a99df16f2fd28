"""Leaflets and order parameters with the membrane normal along x and y: the device against the oracle, dim in {0, 1, 2}.

tests/axis_rotation.py relabels a z system's coordinates cyclically and moves every axis-valued setting with them;
tests/test_axis_rotation_cpu.py ties the oracle on such input to the oracle along z.  Here every route of the device that
reads `leaflets.normal_dim` or the static normal as an axis runs on the rotated input (dim = 2, unrotated, is the control):

1. the project's usual bar on the SAME rotated input: counts, sums, ordermaps and per-frame rows EQUAL to the oracle, the
   leaflet flags of every assignment frame equal to the oracle's (with dynamic normals: at most one tick);
2. metamorphic: the device's flags of every assignment frame on the rotated input are its flags on the z input, for
   every molecule; rotated ordermap counts are the z run's, transposed where the plane's axes come out exchanged.

Every input keeps its heads away from the mid-plane — the oracle's smallest |distance| is asserted to be above 1e-3 nm —
so that no flag may differ and no head is left out.  Every box has three different edges: a box edge read at the wrong
index, the two in-plane axes exchanged or a cell grid sized from the wrong edge show.
"""
import dataclasses

import numpy as np
import pytest

import axis_rotation as ar
from gorder_amd import HipEngine, abi, synthetic
from gorder_amd.abi import (COLLECT_LEAFLETS, GEOM_CUBOID, GEOM_CYLINDER, GEOMREF_BOX_CENTER, GEOMREF_POINT, LEAFLETS_GLOBAL,
                            LEAFLETS_INDIVIDUAL, LEAFLETS_LOCAL, LEAFLETS_MANUAL, LEAFLETS_NONE, DynamicNormal, Geometry,
                            Leaflets, OrderMap)
from oracle import oracle
from test_decision_boundaries_gpu import ALL_SWITCHES, LOCAL_ROUTES

pytestmark = pytest.mark.gpu

DIMS = [2, 0, 1]                      # the control first: its flags and maps are what the other two are compared with
BOX_A = (7.0, 9.5, 8.0)
BOX_B = (11.0, 13.0, 30.0)
N_FRAMES = 9
EDGES = (0, 4, 7, 9)                  # three submits: with frequency 3 frame 3 is inside a batch, frame 6 ends one
MIN_DISTANCE = 1e-3                   # nm; the suite's exemption is for heads within 1e-4 nm of the mid-plane
SWITCHES = tuple(ALL_SWITCHES) + ("GORDER_HIP_LEAFLETS_GENERIC", "GORDER_HIP_NO_SPECULATE", "GORDER_HIP_TW_GATHER")


def set_route(monkeypatch, env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def assignment_frames(frequency, n):
    return np.array([f for f in range(n) if (f == 0 if frequency == 0 else f % frequency == 0)])


def oracle_run(tables, xyz, box):
    """One frame per submit -> (flags [F, n_mol], distances [F, n_mol], results, engine)."""
    trig = oracle.TRIG_MIRROR if (tables.flags & abi.FLAG_TRIG_ACOS_COS) else oracle.TRIG_DIRECT
    o = oracle.OracleEngine(tables, trig=trig)
    n = xyz.shape[0]
    flags = np.zeros((n, tables.n_molecules_total), dtype=np.uint8)
    dist = np.zeros((n, tables.n_molecules_total), dtype=np.float32)
    for f in range(n):
        o.submit(xyz[f:f + 1], None if box is None else box[f:f + 1], np.arange(f, f + 1))
        if tables.leaflets.method != LEAFLETS_NONE:
            flags[f], dist[f], _ = o.leaflets()
    return flags, dist, o.finish(), o


def device_run(tables, xyz, box, edges=EDGES):
    """-> (engine, results, flags of every assignment frame [rows, n_mol], their frames)."""
    eng = HipEngine(tables)
    lf = tables.leaflets.method != LEAFLETS_NONE
    if lf:
        eng.set_collect(COLLECT_LEAFLETS)
    for a, b in zip(edges[:-1], edges[1:]):
        eng.submit_host(xyz[a:b], None if box is None else box[a:b], np.arange(a, b))
    rows, frames = eng.collected_leaflets() if lf else (None, None)
    return eng, eng.finish(), rows, frames


_Z_RUNS = {}


def check(key, tables, xyz, box, dim, edges=EDGES, loose=False):
    """Both assertions of the module for one z system (tables, xyz, box) at one `dim`; `key` names the z system and the
    route, so that the z run is made once for the three dims.  -> (engine, device results, oracle engine)."""
    rt, rx, rb = ar.rotate(tables, xyz, box, dim)
    n = rx.shape[0]
    lf = rt.leaflets.method != LEAFLETS_NONE
    assert rt.normal[dim] == 1.0 and (not lf or rt.leaflets.normal_dim == dim)
    oflags, odist, want, o = oracle_run(rt, rx, rb)
    eng, got, rows, frames = device_run(rt, rx, rb, edges)
    assert got.n_frames == want.n_frames == n
    np.testing.assert_array_equal(got.counts, want.counts)
    if lf:
        assign = assignment_frames(rt.leaflets.frequency, n)
        smallest = float(np.abs(odist[assign]).min())
        print(f"{key} dim={dim}: smallest |distance| = {smallest:.4f} nm")
        assert smallest > MIN_DISTANCE
        np.testing.assert_array_equal(frames, assign)
        np.testing.assert_array_equal(rows, oflags[assign])
        assert 0 < rows[-1].sum() < rows.shape[1]
        np.testing.assert_allclose(eng.leaflet_distances(), odist[assign[-1]], atol=5e-5)
        np.testing.assert_array_equal(got.counts[1] + got.counts[2], got.counts[0])
    if loose:       # dynamic normals: the cloud is summed in another order
        assert np.abs(got.order_ticks() - want.order_ticks()).max() <= 1
    else:
        np.testing.assert_array_equal(got.sums, want.sums)
    if rt.ordermap.enabled:
        np.testing.assert_array_equal(got.map_counts, want.map_counts)
        assert got.map_counts.sum() > 0
        if not loose:
            np.testing.assert_array_equal(got.map_sums, want.map_sums)
    if rt.timewise:
        (gs, gc), (ws, wc) = eng.timewise(n), o.timewise(n)
        np.testing.assert_array_equal(gc, wc)
        if not loose:
            np.testing.assert_array_equal(gs, ws)
    # ---- against the device's own z run
    if dim == 2:
        _Z_RUNS[key] = (rows, got.counts, got.map_counts)
    elif key not in _Z_RUNS:
        _, zgot, zrows, _ = device_run(tables, xyz, box, edges)
        _Z_RUNS[key] = (zrows, zgot.counts, zgot.map_counts)
    zrows, zcounts, zmaps = _Z_RUNS[key]
    if lf:
        np.testing.assert_array_equal(rows, zrows)
    np.testing.assert_array_equal(got.counts, zcounts)       # (a geometry decides coordinate by coordinate: the same samples)
    if rt.ordermap.enabled:
        np.testing.assert_array_equal(ar.maps_like_z(got.map_counts, tables.ordermap.plane, dim), zmaps)
        assert dim == 2 or ar.maps_transposed(tables.ordermap.plane, dim)
    return eng, got, o


def frames_with_movers(system, n_movers, atoms_per_lipid, seed, n=N_FRAMES):
    """The first lipids change sides from frame 4 on (mirrored in the mid-plane): the assignment frame matters, and the
    one-read route has sides to correct."""
    xyz = system.frames(n, seed=seed)
    k = n_movers * atoms_per_lipid
    xyz[4:, :k, 2] = (system.box[2] - xyz[4:, :k, 2]).astype(np.float32)
    return xyz


# ---- global leaflets ------------------------------------------------------------------------------------------------------
GLOBAL_ROUTES = {
    # name: (kind, switches, membrane as an index list of every second atom?)
    "contiguous": ("cg", {"GORDER_HIP_NO_SPECULATE": "1"}, False),
    "generic": ("cg", {"GORDER_HIP_LEAFLETS_GENERIC": "1", "GORDER_HIP_NO_SPECULATE": "1"}, False),
    "subset": ("cg", {}, True),
    "one read": ("cg", {}, False),
    "one read aa": ("aa", {}, False),
    "one read off": ("aa", {"GORDER_HIP_NO_SPECULATE": "1"}, False),
}


def global_system(kind, frequency, subset):
    if kind == "aa":
        system = synthetic.aa_membrane(36, box=BOX_A, leaflets=LEAFLETS_GLOBAL, frequency=frequency)
        xyz = frames_with_movers(system, 2, 98, seed=51)
    else:
        system = synthetic.cg_membrane(240, n_types=2, box=BOX_A, leaflets=LEAFLETS_GLOBAL, frequency=frequency)
        xyz = frames_with_movers(system, 8, 12, seed=53)
    if subset:
        system.tables.leaflets.membrane = np.arange(0, system.n_atoms, 2, dtype=np.uint32)
    return system, xyz


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("frequency", [1, 3, 0])
@pytest.mark.parametrize("route", list(GLOBAL_ROUTES))
def test_global_leaflets(built, monkeypatch, route, frequency, dim):
    kind, env, subset = GLOBAL_ROUTES[route]
    set_route(monkeypatch, env)
    system, xyz = global_system(kind, frequency, subset)
    eng, got, _ = check(("global", route, frequency), system.tables, xyz, system.box9(N_FRAMES), dim)
    stats = eng.speculation_stats()
    if route.startswith("one read") and not env:
        assert eng.plan()["leaflets_one_read"] == 1
        # a batch takes the one read when each of its frames is an assignment frame and an earlier assignment exists
        assert stats["batches"] == (2 if frequency == 1 else 0) and stats["exact_frames"] == 0
        assert frequency != 1 or (stats["moved"] > 0 and stats["enabled"])
    elif env:
        assert stats["batches"] == 0
    else:
        assert subset and eng.plan()["leaflets_one_read"] == 0


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("route", ["one read", "generic", "subset"])
def test_global_leaflets_across_the_periodic_face_along_the_normal(built, monkeypatch, route, dim):
    """Translated by half a box along the normal (before the rotation) the membrane sits at both ends of the box: the plain
    mean of the normal coordinates is not the centre, the one-read route hands every frame to the exact kernel, and every
    kernel needs the box edge of the NORMAL axis."""
    _, env, subset = GLOBAL_ROUTES[route]
    set_route(monkeypatch, env)
    system = synthetic.cg_membrane(240, n_types=2, box=BOX_A, leaflets=LEAFLETS_GLOBAL)
    if subset:
        system.tables.leaflets.membrane = np.arange(0, system.n_atoms, 2, dtype=np.uint32)
    xyz = system.frames(N_FRAMES, seed=55)
    L = float(system.box[2])
    xyz[:, :, 2] = np.mod(xyz[:, :, 2] + L / 2, L).astype(np.float32)
    eng, _, _ = check(("global", "across", route), system.tables, xyz, system.box9(N_FRAMES), dim)
    stats = eng.speculation_stats()
    if route == "one read":
        assert eng.plan()["leaflets_one_read"] == 1 and stats["batches"] >= 1 and stats["exact_frames"] >= 3
    else:
        assert stats["batches"] == 0


# ---- individual leaflets ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("pbc", [True, False])
def test_individual_leaflets(built, monkeypatch, pbc, dim):
    set_route(monkeypatch, {})
    system = synthetic.cg_membrane(240, n_types=2, box=BOX_A, leaflets=LEAFLETS_INDIVIDUAL, frequency=3, handle_pbc=pbc)
    xyz = frames_with_movers(system, 8, 12, seed=57)
    if pbc:      # heads and methyls on either side of the periodic face along the normal: the distance needs that edge
        xyz[:, :, 2] = np.mod(xyz[:, :, 2] + 2.0, system.box[2]).astype(np.float32)
    check(("individual", pbc), system.tables, xyz, system.box9(N_FRAMES) if pbc else None, dim)


# ---- local leaflets: every route of the cell list ----------------------------------------------------------------------------
def local_case(shape):
    """-> (system, frames, box or None) of 300 CG lipids, radius 2.0."""
    kw = dict(n_types=2, leaflets=LEAFLETS_LOCAL, radius=2.0)
    n = 6
    if shape == "undulating":        # the shape of test_local_leaflets_of_an_undulating_membrane: box_z 10.0, amplitude 1.2
        system = synthetic.cg_membrane(300, box=(14.0, 17.0, 10.0), **kw)
        xyz = system.frames(n, seed=61)
        wave = 1.2 * np.sin(2 * np.pi * xyz[:, :, 0] / 14.0) * np.cos(2 * np.pi * xyz[:, :, 1] / 17.0)
        xyz[:, :, 2] = (xyz[:, :, 2] + wave + 0.37).astype(np.float32)          # (not wrapped: some atoms may leave the box)
        return system, xyz, system.box9(n)
    if shape == "wide":              # flat and wide: the two in-plane cell counts differ by a lot
        system = synthetic.cg_membrane(300, box=(60.0, 90.0, 10.0), **kw)
        return system, system.frames(n, seed=63), system.box9(n)
    pbc = shape == "periodic"
    system = synthetic.cg_membrane(300, box=BOX_B, handle_pbc=pbc, **kw)
    return system, system.frames(n, seed=65), system.box9(n) if pbc else None


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("shape", ["periodic", "not periodic", "undulating", "wide"])
@pytest.mark.parametrize("route", list(LOCAL_ROUTES))
def test_local_leaflets(built, monkeypatch, route, shape, dim):
    set_route(monkeypatch, LOCAL_ROUTES[route])
    system, xyz, box = local_case(shape)
    check(("local", route, shape), system.tables, xyz, box, dim, edges=(0, 4, 6))


# ---- the static normal as an axis, with per-frame rows, ordermaps, united atoms ---------------------------------------------------
def xy_map(box, bins):
    return OrderMap(enabled=True, plane=0, span_x=(0.0, float(box[0])), span_y=(0.0, float(box[1])), bin=bins)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("mode", ["tiled", "gather", "literal cosine"])
def test_per_frame_rows_through_both_producers(built, monkeypatch, mode, dim):
    set_route(monkeypatch, {"GORDER_HIP_TW_GATHER": "1"} if mode == "gather" else {})
    system = synthetic.cg_membrane(230, n_types=3, box=BOX_A, leaflets=LEAFLETS_GLOBAL, timewise=True)
    if mode == "literal cosine":
        system.tables.flags = abi.FLAG_TRIG_ACOS_COS
    xyz = frames_with_movers(system, 8, 12, seed=67)
    eng, _, _ = check(("rows", mode), system.tables, xyz, system.box9(N_FRAMES), dim)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("gather", [False, True])
def test_ordermaps_across_the_normal_through_both_producers(built, monkeypatch, gather, dim):
    set_route(monkeypatch, {"GORDER_HIP_MAPS_GATHER": "1"} if gather else {})
    system = synthetic.cg_membrane(230, n_types=3, box=BOX_A, leaflets=LEAFLETS_INDIVIDUAL)
    system.tables.ordermap = xy_map(system.box, (0.45, 0.8))
    xyz = system.frames(N_FRAMES, seed=69)
    eng, got, _ = check(("maps", gather), system.tables, xyz, system.box9(N_FRAMES), dim)
    nx, ny = round(BOX_A[0] / 0.45) + 1, round(BOX_A[1] / 0.8) + 1
    assert eng.ordermap_dims() == ((nx, ny) if dim == 2 else (ny, nx))


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("direct", [False, True])
def test_united_atom_ordermaps_staged_and_direct(built, monkeypatch, direct, dim):
    set_route(monkeypatch, {"GORDER_HIP_MAP_DIRECT": "1"} if direct else {})
    system = synthetic.ua_membrane(40, box=BOX_A, leaflets=LEAFLETS_GLOBAL)
    system.tables.ordermap = xy_map(system.box, (0.9, 0.6))
    xyz = system.frames(N_FRAMES, seed=71)
    eng, _, _ = check(("ua maps", direct), system.tables, xyz, system.box9(N_FRAMES), dim)
    assert eng.plan()["map_staged"] == int(not direct)


# ---- geometry selection ----------------------------------------------------------------------------------------------------
GEOMETRIES = {
    "cylinder along the normal": dict(kind=GEOM_CYLINDER, radius=2.5, span=(-1.5, 2.0), orientation=2),
    "cuboid": dict(kind=GEOM_CUBOID, xdim=(-2.0, 2.5), ydim=(-3.0, 1.5), zdim=(-1.0, 3.0)),
}


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("reference", ["point", "box centre"])
@pytest.mark.parametrize("shape", list(GEOMETRIES))
def test_geometry_selection(built, monkeypatch, shape, reference, dim):
    set_route(monkeypatch, {})
    system = synthetic.cg_membrane(230, n_types=3, box=BOX_A, leaflets=LEAFLETS_GLOBAL)
    ref = dict(reference=GEOMREF_POINT, point=(5.5, 2.0, 4.5)) if reference == "point" else dict(reference=GEOMREF_BOX_CENTER)
    system.tables.geometry = Geometry(structure_box=BOX_A, **GEOMETRIES[shape], **ref)
    xyz = system.frames(N_FRAMES, seed=73)
    _, got, _ = check(("geometry", shape, reference), system.tables, xyz, system.box9(N_FRAMES), dim)
    assert 0 < got.counts[0].sum() < N_FRAMES * system.tables.n_samples_per_frame      # the shape really filters


# ---- dynamic normals ---------------------------------------------------------------------------------------------------------
def with_dynamic_normals(system, radius):
    cloud = []
    for mt in system.tables.molecule_types:
        mt.normal_heads = np.asarray(mt.heads, dtype=np.uint32)
        cloud.append(mt.normal_heads)
    system.tables.dynamic_normal = DynamicNormal(enabled=True, radius=radius, cloud=np.concatenate(cloud))
    return system


_Z_NORMALS = {}


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", ["cg", "ua"])
def test_dynamic_normals(built, monkeypatch, kind, dim):
    """The reference takes the heads within a SPHERE around a molecule's head (normal.rs:160-199, pbc.rs:142-161, 321-350)
    and the direction of least variance of that cloud (normal.rs:421-458): nothing follows the membrane normal, the
    device's x-y cell grid only prunes.  So the normals of the rotated system are the z system's, components permuted — up
    to the sign: a normal is a direction, and its sign is fixed by the last non-zero COMPONENT."""
    set_route(monkeypatch, {})
    if kind == "cg":
        system = synthetic.cg_membrane(300, n_types=2, box=BOX_B, leaflets=LEAFLETS_INDIVIDUAL)
    else:
        system = synthetic.ua_membrane(40, box=BOX_A, leaflets=LEAFLETS_GLOBAL)
    with_dynamic_normals(system, 2.2)
    xyz = system.frames(N_FRAMES, seed=75)
    eng, _, o = check(("dynamic", kind), system.tables, xyz, system.box9(N_FRAMES), dim, loose=True)
    n_gpu, k_gpu = eng.normals()
    n_ref, k_ref = o.normals()
    np.testing.assert_array_equal(k_gpu, k_ref)
    assert k_ref.min() >= 3 and np.abs(n_gpu - n_ref).max() < 1e-6
    assert 0.8 < np.abs(n_ref[:, dim]).mean() < 0.99999          # near the rotated normal, and not the static axis itself
    if dim == 2:
        _Z_NORMALS[kind] = n_gpu
    elif kind not in _Z_NORMALS:
        zeng, _, _, _ = device_run(system.tables, xyz, system.box9(N_FRAMES))
        _Z_NORMALS[kind] = zeng.normals()[0]
    back = ar.unrotate_vectors(n_gpu, dim)
    back = back * np.sign((back * _Z_NORMALS[kind]).sum(axis=1, keepdims=True))
    assert np.abs(back - _Z_NORMALS[kind]).max() < 1e-6


# ---- collect and replay --------------------------------------------------------------------------------------------------------
def test_collected_flags_along_x_replayed_with_other_batching(built, monkeypatch):
    set_route(monkeypatch, {})
    system = synthetic.cg_membrane(240, n_types=2, box=BOX_A, leaflets=LEAFLETS_GLOBAL, frequency=2)
    xyz = frames_with_movers(system, 8, 12, seed=77)
    rt, rx, rb = ar.rotate(system.tables, xyz, system.box9(N_FRAMES), 0)
    _, want, rows, frames = device_run(rt, rx, rb)
    np.testing.assert_array_equal(frames, [0, 2, 4, 6, 8])
    assert not np.array_equal(rows[0], rows[-1]) and want.counts[1].sum() > 0 and want.counts[2].sum() > 0
    manual = dataclasses.replace(rt, leaflets=Leaflets(method=LEAFLETS_MANUAL, normal_dim=0, frequency=2))
    eng = HipEngine(manual)
    eng.set_manual_leaflet_table(rows)
    for a, b in ((0, 1), (1, 6), (6, N_FRAMES)):
        eng.submit_host(rx[a:b], rb[a:b], np.arange(a, b))
    got = eng.finish()
    np.testing.assert_array_equal(got.counts, want.counts)
    np.testing.assert_array_equal(got.sums, want.sums)
