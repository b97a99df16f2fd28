"""Every sampling kernel at the edges of the sample arithmetic: the probes of tests/sample_probes.py — bonds on and next
to the guards of the fast division, of zero, denormal and infinite squared norm, one to four and a half box lengths
long, with an infinite coordinate, against degenerate normals — through every route that evaluates a sample.

One test per route.  Each builds a system of a few hundred atoms and nine frames (two whole stages and a partial one,
cut once mid-batch), in which every probe visits every frame in another accumulator slot, and compares the device
with the oracle and — where the cosine is the default squared form — with the literal float32 statement
(sample_probes.literal_tick), integer for integer.  The expectations of the features the oracle does not have (shells,
histograms, per-molecule rows, correlation) are derived from the split-table oracle's per-sample ticks the way those
features' own tests derive them.  Each test also asserts, through gorder_hip_kernel_time_names, that the kernel group it
is named after ran.

Families left out by construction (never skipped at run time): the upper guard, the overflowing norms and the infinite
coordinates need an atom farther away than a periodic box lets a bond vector be — they are in the tables without a box;
the images need a box."""
import dataclasses

import numpy as np
import pytest

import sample_probes as sp
from sample_probes import F
from gorder_amd import HipEngine, abi
from gorder_amd.abi import (FLAG_TRIG_ACOS_COS, GEOM_CYLINDER, GEOM_SPHERE, GEOMREF_POINT, LEAFLETS_GLOBAL, Geometry, Leaflets,
                            OrderMap)
from oracle import oracle
from test_sample_probes_cpu import GENERIC, case, probe_tables
from test_order_histogram_gpu import oracle_samples, want_hist
from test_molecule_rows_gpu import oracle_rows
from test_radial_gpu import oracle_nested, same_shells

pytestmark = pytest.mark.gpu

N = sp.N_FRAMES
CUTS = [(0, 5), (5, N)]                         # a stage and a partial one, then a whole stage
FRAMES = np.arange(N, dtype=np.uint64)         # (from 0: leaflets every third frame are assigned in frames 0, 3 and 6)
BOX_NAMES = (None, "dyadic", "three edges")
# every switch a test of this file sets; set_route clears them first
ALL_SWITCHES = ("GORDER_HIP_KERNEL", "GORDER_HIP_FORCE_DIRECT", "GORDER_HIP_TW_GATHER", "GORDER_HIP_MAPS_GATHER", "GORDER_HIP_MAP_DIRECT",
                "GORDER_HIP_RADIAL_DIRECT", "GORDER_HIP_DIST_DIRECT", "GORDER_HIP_CORR_GRID", "GORDER_HIP_NO_SPECULATE")


def set_route(monkeypatch, env):
    for name in ALL_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def normal_of(name, axis):
    return GENERIC if name == "generic" else tuple(float(x) for x in sp.axis_normal(axis))


def trig_of(tables):
    return oracle.TRIG_MIRROR if tables.flags & FLAG_TRIG_ACOS_COS else oracle.TRIG_DIRECT


def device(tables, ps, setup=None, cuts=CUTS, frames=FRAMES):
    eng = HipEngine(tables)
    eng.kernel_time()                           # (switches the event pairs on: the kernels of the batches are then named)
    if setup:
        setup(eng)
    for a, b in cuts:
        eng.submit_host(ps.xyz[a:b], None if ps.box9 is None else ps.box9[a:b], frames[a:b])
    return eng


def reference(tables, ps, setup=None, frames=FRAMES):
    o = oracle.OracleEngine(tables, trig=trig_of(tables))
    if setup:
        setup(o)
    o.submit(ps.xyz, ps.box9, frames)
    return o


def ran(eng, kernel, never=()):
    eng.kernel_time()
    names = eng.kernel_names().split(" + ")
    assert kernel in names and not set(never) & set(names), names


def same_results(got, want):
    np.testing.assert_array_equal(got.counts, want.counts)
    np.testing.assert_array_equal(got.sums, want.sums)
    assert got.n_frames == want.n_frames == N
    if want.map_sums is not None:
        np.testing.assert_array_equal(got.map_counts, want.map_counts)
        np.testing.assert_array_equal(got.map_sums, want.map_sums)


def same_rows(eng, o):
    (gs, gc), (ws, wc) = eng.timewise(N), o.timewise(N)
    np.testing.assert_array_equal(gc, wc)
    np.testing.assert_array_equal(gs, ws)


def literal_ticks(ps, normal, tables):
    """One tick per probe from the literal statement, or None where the cosine is not the default squared form."""
    if tables.flags & FLAG_TRIG_ACOS_COS:
        return None
    n = np.array(normal, dtype=F)
    return np.array([sp.literal_tick(v, n) for v in ps.vectors()])


def sides(ps, frequency):
    """bool [frames, molecules]: the sample is booked on the upper leaflet — the head's side in the frame that assigned."""
    f = np.arange(N)
    return ps.upper[(f // frequency) * frequency] if frequency else ps.upper[np.zeros(N, dtype=int)]


def same_as_literal(got, ps, ticks, upper=None):
    if ticks is None:
        return
    s, c = ps.slot_sums(ticks)
    np.testing.assert_array_equal(got.counts[0], c)
    np.testing.assert_array_equal(got.sums[0], s)
    if upper is not None:
        s, c = ps.slot_sums(ticks, upper)
        np.testing.assert_array_equal(got.counts[1], c)
        np.testing.assert_array_equal(got.sums[1], s)
        s, c = ps.slot_sums(ticks, ~upper)
        np.testing.assert_array_equal(got.counts[2], c)
        np.testing.assert_array_equal(got.sums[2], s)


def global_leaflets(axis, frequency):
    return Leaflets(method=LEAFLETS_GLOBAL, normal_dim=axis, frequency=frequency)


# ---- Tiled ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaflets", [None, 3])           # 3: global leaflets every third frame — the two-kernel path
@pytest.mark.parametrize("acos", [False, True])
@pytest.mark.parametrize("box_name", BOX_NAMES)
@pytest.mark.parametrize("normal,axis", [("axis", 0), ("axis", 1), ("axis", 2), ("generic", 2)])
def test_tiled(built, monkeypatch, normal, axis, box_name, acos, leaflets):
    """k_bonds_tiled: compute_core's three minimum-image / cosine branches (axis and default cosine and periodic: the
    magnitude form; axis: gm_sch_axis / gm_sch_axis_acos with the rare pass; generic: `nonfinite` and NaN) for whole
    stages, bond_sample for the ninth frame."""
    set_route(monkeypatch, {})
    ps = case(axis, box_name, swap_from=5)
    n = normal_of(normal, axis)
    tables = probe_tables(ps, n, global_leaflets(axis, leaflets) if leaflets else None, flags=FLAG_TRIG_ACOS_COS if acos else 0)
    eng = device(tables, ps)
    got, want = eng.finish(), reference(tables, ps).finish()
    ran(eng, "k_bonds_tiled")
    same_results(got, want)
    same_as_literal(got, ps, literal_ticks(ps, n, tables), sides(ps, leaflets) if leaflets else None)
    if leaflets:
        assert got.counts[1].all() and got.counts[2].all() and "k_spec_check + k_spec_fixup" not in eng.kernel_names()


@pytest.mark.parametrize("acos", [False, True])
@pytest.mark.parametrize("name,box_name", [("tiny", None), ("tiny", "dyadic"), ("tiny", "three edges"), ("huge", None)])
def test_tiled_with_a_normal_whose_squared_norm_times_the_bonds_leaves_the_range(built, monkeypatch, name, box_name, acos):
    """A static normal of length 2^-40 or 2^40: s2 * n2sq underflows to 0 (0 / 0: NaN, tick 0, counted — in a periodic box
    too) or overflows to inf (a bond of 2^40 nm: without a box) with both squared norms finite and not 0."""
    set_route(monkeypatch, {})
    probes, normals = sp.product_probes(periodic=box_name is not None)
    box = None if box_name is None else sp.BOXES[box_name]
    ps = sp.probe_system(probes + sp.bond_probes(2, box), 2, box)
    tables = probe_tables(ps, normals[name], flags=FLAG_TRIG_ACOS_COS if acos else 0)
    eng = device(tables, ps)
    got = eng.finish()
    ran(eng, "k_bonds_tiled")
    same_results(got, reference(tables, ps).finish())
    same_as_literal(got, ps, literal_ticks(ps, normals[name], tables))


# ---- one read + fixup ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acos", [False, True])
@pytest.mark.parametrize("box_name", BOX_NAMES)
def test_one_read_and_fixup(built, monkeypatch, box_name, acos):
    """Global leaflets assigned every frame, two batches: the second is speculative (k_bonds_tiled<MOM> books every molecule
    on the side it had), molecules 0 and 1 have changed sides, and k_spec_fixup recomputes their samples — probes among
    them in every frame — with bond_sample's arithmetic."""
    set_route(monkeypatch, {})
    ps = case(2, box_name, swap_from=5)
    tables = probe_tables(ps, leaflets=global_leaflets(2, 1), flags=FLAG_TRIG_ACOS_COS if acos else 0)
    eng = device(tables, ps)
    got = eng.finish()
    stats = eng.speculation_stats()
    ran(eng, "k_bonds_tiled")
    same_results(got, reference(tables, ps).finish())
    same_as_literal(got, ps, literal_ticks(ps, (0.0, 0.0, 1.0), tables), sides(ps, 1))
    assert eng.plan()["leaflets_one_read"] == 1
    ran(eng, "k_spec_fixup")
    # two molecules on the other side in each of the second batch's four frames: the fixed pairs
    assert stats["batches"] == 1 and stats["moved"] == 2 * (N - 5), stats
    # an infinite coordinate anywhere in a tile's window leaves the frame's centre to the exact kernel (the one-read path's
    # stand-in for the reference's check of the membrane atoms), and every frame of the table without a box holds one;
    # the sides still come from k_spec_check and the samples from k_spec_fixup
    assert stats["exact_frames"] == (N - 5 if box_name is None else 0), stats


def test_one_read_and_fixup_without_a_box_and_without_infinities(built, monkeypatch):
    """The table without a box, less the family that keeps the one-read path from deciding (above): the upper guard and the
    overflowing norms reach k_spec_fixup."""
    set_route(monkeypatch, {})
    ps = sp.probe_system([p for p in sp.bond_probes(2, None) if p.family != "nonfinite"], 2, None, swap_from=5)
    for acos in (False, True):
        tables = probe_tables(ps, leaflets=global_leaflets(2, 1), flags=FLAG_TRIG_ACOS_COS if acos else 0)
        eng = device(tables, ps)
        got = eng.finish()
        stats = eng.speculation_stats()
        same_results(got, reference(tables, ps).finish())
        same_as_literal(got, ps, literal_ticks(ps, (0.0, 0.0, 1.0), tables), sides(ps, 1))
        assert stats["batches"] == 1 and stats["exact_frames"] == 0 and stats["moved"] == 2 * (N - 5), stats
        ran(eng, "k_spec_fixup")


# ---- Gather, Direct ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acos", [False, True])
@pytest.mark.parametrize("box_name", BOX_NAMES)
def test_gather(built, monkeypatch, box_name, acos):
    """k_bonds_gather: bond_sample for every frame — the signed step, the literal loops, plain gm_calc_sch."""
    set_route(monkeypatch, {"GORDER_HIP_KERNEL": "gather"})
    ps = case(2, box_name)
    for n in ((0.0, 0.0, 1.0), GENERIC):
        tables = probe_tables(ps, n, flags=FLAG_TRIG_ACOS_COS if acos else 0)
        eng = device(tables, ps)
        got = eng.finish()
        ran(eng, "k_bonds_gather", never=["k_bonds_tiled"])
        same_results(got, reference(tables, ps).finish())
        same_as_literal(got, ps, literal_ticks(ps, n, tables))


@pytest.mark.parametrize("acos", [False, True])
@pytest.mark.parametrize("box_name", BOX_NAMES)
def test_direct(built, monkeypatch, box_name, acos):
    """k_bonds_direct (GORDER_HIP_FORCE_DIRECT: no bond is in a window)."""
    set_route(monkeypatch, {"GORDER_HIP_FORCE_DIRECT": "1"})
    ps = case(2, box_name, swap_from=5)
    for lf in (None, global_leaflets(2, 3)):
        tables = probe_tables(ps, leaflets=lf, flags=FLAG_TRIG_ACOS_COS if acos else 0)
        eng = device(tables, ps)
        got = eng.finish()
        assert eng.plan()["n_tiles"] == 0 and eng.plan()["n_direct_items"] == ps.n_mol * sp.B_SLOTS
        ran(eng, "k_bonds_direct", never=["k_bonds_tiled", "k_bonds_gather"])
        same_results(got, reference(tables, ps).finish())
        same_as_literal(got, ps, literal_ticks(ps, (0.0, 0.0, 1.0), tables), sides(ps, 3) if lf else None)


# ---- TiledTw, TiledMaps -------------------------------------------------------------------------------------------------------------
def probe_map(plane):
    """A 5 x 5 map of 1-nm tiles around the origin: everyday bonds land on it, the far ends of the long ones, the
    overflowing ones and those at +-inf add to the sums and to no tile."""
    return OrderMap(enabled=True, plane=plane, span_x=(-2.0, 2.0), span_y=(-2.0, 2.0), bin=(1.0, 1.0))


def maps_hold_less_than_the_sums(got, want_fewer):
    tot = got.map_counts[0].sum(axis=(1, 2))
    assert (tot <= got.counts[0]).all() and tot.sum() > 0 and (not want_fewer or (tot < got.counts[0]).any())


@pytest.mark.parametrize("leaflets", [None, 3])
@pytest.mark.parametrize("maps", [False, True])
@pytest.mark.parametrize("box_name", BOX_NAMES)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_tiled_tw(built, monkeypatch, axis, box_name, maps, leaflets):
    """k_bonds_tiled_tw: compute<2> (with staged maps: compute<3>) — the rare pass rewrites the (side, tick) word and the
    map word of the stage — and bond_sample for the tail."""
    set_route(monkeypatch, {})
    ps = case(axis, box_name, swap_from=5)
    n = normal_of("axis", axis)
    tables = probe_tables(ps, n, global_leaflets(axis, leaflets) if leaflets else None, timewise=True,
                          ordermap=probe_map(0) if maps else OrderMap())
    eng, o = device(tables, ps), reference(tables, ps)
    got = eng.finish()
    ran(eng, "k_bonds_tiled_tw", never=["k_bonds_extras"])
    assert not maps or eng.plan()["map_staged"] == 1
    same_results(got, o.finish())
    same_rows(eng, o)
    upper = sides(ps, leaflets) if leaflets else None
    ticks = literal_ticks(ps, n, tables)
    same_as_literal(got, ps, ticks, upper)
    # the rows, frame by frame, from the literal ticks
    gs, gc = eng.timewise(N)
    t = ticks[ps.which]
    np.testing.assert_array_equal(gs[:, 0], t.sum(axis=1))
    if leaflets:
        np.testing.assert_array_equal(gs[:, 1], (t * upper[:, :, None]).sum(axis=1))
        np.testing.assert_array_equal(gc[:, 2], np.broadcast_to((~upper)[:, :, None], t.shape).sum(axis=1))
    if maps:
        maps_hold_less_than_the_sums(got, True)


@pytest.mark.parametrize("leaflets", [None, 3])
@pytest.mark.parametrize("plane", [0, 1, 2])
@pytest.mark.parametrize("box_name", BOX_NAMES)
def test_tiled_maps(built, monkeypatch, box_name, plane, leaflets):
    """k_bonds_tiled_maps: compute<1> — the rare pass rewrites the staged map word (its tick AND its tile: the bond
    position comes from the signed minimum-image vector, which the first pass does not have for a long bond)."""
    set_route(monkeypatch, {})
    for axis in (2, 0):
        ps = case(axis, box_name, swap_from=5)
        n = normal_of("axis", axis)
        tables = probe_tables(ps, n, global_leaflets(axis, leaflets) if leaflets else None, ordermap=probe_map(plane))
        eng = device(tables, ps)
        got = eng.finish()
        ran(eng, "k_bonds_tiled_maps", never=["k_bonds_extras"])
        assert "k_map_accumulate" in eng.kernel_names() and eng.ordermap_dims() == (5, 5)
        same_results(got, reference(tables, ps).finish())
        same_as_literal(got, ps, literal_ticks(ps, n, tables), sides(ps, leaflets) if leaflets else None)
        maps_hold_less_than_the_sums(got, True)
        # the map's sums are ticks of the literal statement too: every sample of a slot that is on the map, added up
        ticks = literal_ticks(ps, n, tables)
        box = None if ps.box9 is None else np.diag(ps.box9[0])
        on_map = np.array([on_the_map(p, v, plane) for p, v in zip(ps.probes, ps.vectors())])
        s, c = ps.slot_sums(np.where(on_map, ticks, 0))
        np.testing.assert_array_equal(got.map_sums[0].sum(axis=(1, 2)), s)
        np.testing.assert_array_equal(got.map_counts[0].sum(axis=(1, 2)), on_map[ps.which].sum(axis=(0, 1)))
        # at +-inf or 1e19 nm in a direction of the plane: in the sums (above), on no tile
        ax = list({0: (0, 1), 1: (0, 2), 2: (2, 1)}[plane])
        far = [i for i, p in enumerate(ps.probes) if not (np.abs(np.stack([p.p1, p.p2])[:, ax]) < 1e18).all()]
        assert not on_map[far].any() and (box is not None or len(far) >= 6)


def on_the_map(p, v, plane):
    """The bond position p1 + v / 2 (bond.rs:422) lies on probe_map: the nearest tile centre of -2 .. 2 in both directions."""
    with np.errstate(all="ignore"):
        pos = [F(F(p.p1[k]) + F(F(v[k]) / F(2))) for k in range(3)]
    ax, ay = {0: (0, 1), 1: (0, 2), 2: (2, 1)}[plane]

    def tile(x):
        k = np.float64(F(F(x - F(-2.0)) / F(1.0)))
        k = np.trunc(k + np.copysign(0.5, k))
        return k >= 0 and k < 5
    return bool(tile(pos[ax]) and tile(pos[ay]))


# ---- Extras --------------------------------------------------------------------------------------------------------------------
def probe_cylinder(axis, radius=3.0):
    return Geometry(kind=GEOM_CYLINDER, reference=GEOMREF_POINT, point=(0.0, 0.0, 0.0), radius=radius, orientation=axis,
                    structure_box=(16.0, 16.0, 16.0))


EXTRAS = {"geometry": ({}, dict(geometry=True)),
          "acos + timewise": ({}, dict(flags=FLAG_TRIG_ACOS_COS, timewise=True)),
          "tw gather": ({"GORDER_HIP_TW_GATHER": "1"}, dict(timewise=True)),
          "maps gather": ({"GORDER_HIP_MAPS_GATHER": "1"}, dict(ordermap=True)),
          "map direct": ({"GORDER_HIP_MAP_DIRECT": "1"}, dict(ordermap=True, timewise=True))}


@pytest.mark.parametrize("box_name", BOX_NAMES)
@pytest.mark.parametrize("axis", [0, 1, 2])               # the run-time e.axis branches: gm_sch_axis<0 / 1 / 2> + the local recompute
@pytest.mark.parametrize("mode", list(EXTRAS))
def test_extras(built, monkeypatch, mode, axis, box_name):
    """k_bonds_extras: gm_min_image per component, e.axis picks gm_sch_axis<axis> with a `rare` recompute of its own."""
    env, kw = EXTRAS[mode]
    set_route(monkeypatch, env)
    ps = case(axis, box_name, swap_from=5)
    n = normal_of("axis", axis)
    kw = dict(kw)
    if kw.pop("geometry", False):
        kw["geometry"] = probe_cylinder(axis)
    if kw.pop("ordermap", False):
        kw["ordermap"] = probe_map(0)
    tables = probe_tables(ps, n, global_leaflets(axis, 3), **kw)
    eng, o = device(tables, ps), reference(tables, ps)
    got = eng.finish()
    ran(eng, "k_bonds_extras", never=["k_bonds_tiled", "k_bonds_tiled_tw", "k_bonds_tiled_maps"])
    same_results(got, o.finish())
    if tables.timewise:
        same_rows(eng, o)
    if mode != "geometry":
        same_as_literal(got, ps, literal_ticks(ps, n, tables), sides(ps, 3))
    else:                          # the selection drops the far ends: fewer samples than there are, and not none
        assert 0 < got.counts[0].sum() < ps.which.size
    if tables.ordermap.enabled:
        maps_hold_less_than_the_sums(got, True)


def same_as_literal_normals(got, ps, normals, tables):
    if tables.flags & FLAG_TRIG_ACOS_COS:
        return
    t = sp.literal_ticks_with_normals(ps, normals)
    np.testing.assert_array_equal(got.sums[0], t.sum(axis=(0, 1)))
    np.testing.assert_array_equal(got.counts[0], np.full(sp.B_SLOTS, N * ps.n_mol, dtype=np.uint64))
    assert (t == 0).sum() > N * ps.n_mol                      # NaN samples by the dozen, every one counted


@pytest.mark.parametrize("acos", [False, True])
@pytest.mark.parametrize("box_name", BOX_NAMES)
@pytest.mark.parametrize("how", ["set_normals", "normal table"])
def test_extras_with_supplied_normals(built, monkeypatch, how, box_name, acos):
    """k_bonds_extras with a normal per molecule and frame (gorder_hip_set_normals, gorder_hip_set_manual_normal_table):
    sqrtf(n2sq) and gm_calc_sch on data.  Both setters take every value as it is — the reference reads a normal from a file
    and uses it — so there is no refusal to assert: the degenerate normals must give the oracle's integers."""
    set_route(monkeypatch, {})
    ps = case(2, box_name)
    normals = sp.supplied_normals(ps.n_mol)
    tables = probe_tables(ps, flags=FLAG_TRIG_ACOS_COS if acos else 0)
    if how == "set_normals":
        eng = HipEngine(tables)
        eng.kernel_time()
        for a, b in CUTS:
            eng.set_normals(normals[a:b])
            eng.submit_host(ps.xyz[a:b], None if ps.box9 is None else ps.box9[a:b], FRAMES[a:b])
    else:
        eng = device(tables, ps, lambda e: e.set_manual_normal_table(normals))
    got = eng.finish()
    ran(eng, "k_bonds_extras")
    want = reference(tables, ps, lambda o: o.set_normals(normals)).finish()
    same_results(got, want)
    same_as_literal_normals(got, ps, normals, tables)


@pytest.mark.parametrize("acos", [False, True])
@pytest.mark.parametrize("box_name", BOX_NAMES)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_extras_with_dynamic_normals(built, monkeypatch, axis, box_name, acos):
    """k_dyn_cov + k_bonds_extras: the cloud of every head is a lattice of dyadic coordinates in a plane across `axis` (and
    holds no probe atom), so the f64 covariance sums are exact in any order and the normal IS the axis: equality, no
    tolerance — with the oracle and with the literal statement for the axis normal."""
    set_route(monkeypatch, {})
    ps = case(axis, box_name, cloud=True)
    assert not set(ps.cloud.tolist()) & set(ps.bonds.reshape(-1).tolist())
    n = normal_of("axis", axis)
    tables = probe_tables(ps, n, dynamic_normal=abi.DynamicNormal(enabled=True, radius=3.0, cloud=ps.cloud),
                          flags=FLAG_TRIG_ACOS_COS if acos else 0)
    tables.molecule_types[0].normal_heads = ps.heads
    eng, o = device(tables, ps), reference(tables, ps)
    got = eng.finish()
    ran(eng, "k_bonds_extras")
    same_results(got, o.finish())
    (gn, gk), (wn, wk) = eng.normals(), o.normals()
    np.testing.assert_array_equal(gk, wk)
    np.testing.assert_array_equal(np.abs(gn), np.tile(sp.axis_normal(axis), (ps.n_mol, 1)))       # exactly the axis
    same_as_literal(got, ps, literal_ticks(ps, n, tables))


# ---- Shells, Dist, TiledMol -------------------------------------------------------------------------------------------------------
SHELL_RADII = (0.25, 1.0, 3.0)


@pytest.mark.parametrize("acos", [False, True])
@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("box_name", BOX_NAMES)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_shells(built, monkeypatch, axis, box_name, direct, acos):
    """k_bonds_shells, the LDS table and GORDER_HIP_RADIAL_DIRECT: its own copy of the e.axis branches and the `rare`
    recompute; the shell of a sample comes from its bond position, so long bonds and bonds at infinity are in none."""
    set_route(monkeypatch, {"GORDER_HIP_RADIAL_DIRECT": "1"} if direct else {})
    ps = case(axis, box_name, swap_from=5)
    n = normal_of("axis", axis)
    for kind in (GEOM_CYLINDER, GEOM_SPHERE):
        geom = dataclasses.replace(probe_cylinder(axis, SHELL_RADII[-1]), kind=kind)
        tables = probe_tables(ps, n, global_leaflets(axis, 3), geometry=geom, flags=FLAG_TRIG_ACOS_COS if acos else 0)
        want_shells, want_total = oracle_nested(tables, SHELL_RADII, ps.xyz, ps.box9, trig=trig_of(tables))
        eng = device(tables, ps, lambda e: e.set_radial_shells([float(F(r)) for r in SHELL_RADII]))
        shells, total = eng.radial_shells(), eng.finish()
        ran(eng, "k_bonds_shells", never=["k_bonds_extras"])
        same_shells(shells, want_shells)
        same_results(total, want_total)
        assert all(r.counts[0].sum() > 0 for r in shells) and 0 < total.counts[0].sum() < ps.which.size


EDGES = np.array([-500000, -499999, 0, 1, 999999, 1000000, 1000001])      # an edge on the lowest tick, on 0 (NaN), on the highest


@pytest.mark.parametrize("acos", [False, True])
@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("box_name", BOX_NAMES)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_dist(built, monkeypatch, axis, box_name, direct, acos):
    """k_bonds_dist, the LDS table and GORDER_HIP_DIST_DIRECT: the bins [-500000, -499999), [0, 1) and [1000000, 1000001)
    hold exactly the samples across the normal, the NaN samples (tick 0, counted) and the samples along it or of zero
    length."""
    set_route(monkeypatch, {"GORDER_HIP_DIST_DIRECT": "1"} if direct else {})
    ps = case(axis, box_name, swap_from=5)
    n = normal_of("axis", axis)
    tables = probe_tables(ps, n, global_leaflets(axis, 3), flags=FLAG_TRIG_ACOS_COS if acos else 0)
    samples = oracle_samples(tables, ps.xyz, ps.box9, trig_of(tables))
    flags = (~sides(ps, 3)).astype(np.uint8)
    eng = device(tables, ps, lambda e: e.set_order_histogram(EDGES))
    hist, got = eng.order_histogram(), eng.finish()
    ran(eng, "k_bonds_dist", never=["k_bonds_extras"])
    np.testing.assert_array_equal(hist, want_hist(samples, EDGES, flags, sp.B_SLOTS))
    same_results(got, reference(tables, ps).finish())
    np.testing.assert_array_equal(hist.sum(axis=0), got.counts)                  # the edges cover every tick
    ticks = literal_ticks(ps, n, tables)
    same_as_literal(got, ps, ticks, sides(ps, 3))
    if ticks is not None:
        for k, t in ((0, -500000), (2, 0), (5, 1000000)):
            np.testing.assert_array_equal(hist[k, 0], (ticks == t)[ps.which].sum(axis=(0, 1)))
        assert hist[5, 0].sum() >= 6 * N and hist[0, 0].sum() >= 6 * N and (box_name is not None or hist[2, 0].sum() >= 8 * N)


GROUPS = [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9, 10], [12, 13, 14, 15]]                 # slot 11: in no group


@pytest.mark.parametrize("leaflets", [None, 3])
@pytest.mark.parametrize("acos", [False, True])
@pytest.mark.parametrize("box_name", BOX_NAMES)
@pytest.mark.parametrize("normal,axis", [("axis", 0), ("axis", 1), ("axis", 2), ("generic", 2)])
def test_tiled_mol(built, monkeypatch, normal, axis, box_name, acos, leaflets):
    """k_bonds_tiled_mol: compute_core for whole stages and bond_sample for the tail, the ticks folded per molecule."""
    set_route(monkeypatch, {})
    ps = case(axis, box_name, swap_from=5)
    n = normal_of(normal, axis)
    tables = probe_tables(ps, n, global_leaflets(axis, leaflets) if leaflets else None, flags=FLAG_TRIG_ACOS_COS if acos else 0)
    want = oracle_rows(tables, GROUPS, ps.xyz, ps.box9, trig_of(tables))
    eng = device(tables, ps, lambda e: e.set_molecule_rows(GROUPS))
    sums, counts, frames = eng.molecule_rows()
    got = eng.finish()
    ran(eng, "k_bonds_tiled_mol", never=["k_bonds_tiled", "k_bonds_extras"])
    np.testing.assert_array_equal(frames, FRAMES)
    np.testing.assert_array_equal(counts.astype(np.int64), want[1])
    np.testing.assert_array_equal(sums.astype(np.int64), want[0])
    same_results(got, reference(tables, ps).finish())
    ticks = literal_ticks(ps, n, tables)
    same_as_literal(got, ps, ticks, sides(ps, leaflets) if leaflets else None)
    if ticks is not None:
        t = ticks[ps.which]                                                      # [frames, molecules, slots]
        for g, slots in enumerate(GROUPS):
            np.testing.assert_array_equal(sums[:, g], t[:, :, slots].sum(axis=2))


# ---- Corr --------------------------------------------------------------------------------------------------------------------------
LAGS = [0, 1, 2, 5]


def pair_ticks(ps, tables, lag):
    """int64 [N - lag, molecules, slots]: the tick of (frame lag + f, frame f) from the per-sample oracle, the earlier
    frame's literal bond vectors handed over as manual normals (the way tests/test_bond_correlation_gpu.py derives it)."""
    v = ps.vectors()[ps.which].reshape(N, -1, 3)                                  # [frames, samples, 3]
    atoms = np.transpose(ps.bonds, (1, 0, 2)).reshape(-1, 2)                        # molecule-major, as `which`
    split = dataclasses.replace(tables, molecule_types=[abi.MolType(n_molecules=1, bonds=a.reshape(1, 1, 2)) for a in atoms],
                                leaflets=Leaflets(), timewise=True, flags=0)
    ref = oracle.OracleEngine(split, trig=oracle.TRIG_DIRECT)
    ref.set_normals(np.ascontiguousarray(v[:N - lag]))
    ref.submit(ps.xyz[lag:], None if ps.box9 is None else ps.box9[lag:], FRAMES[lag:])
    s, c = ref.timewise(N - lag)
    assert (c[:, 0] == 1).all()
    return s[:, 0].astype(np.int64).reshape(N - lag, ps.n_mol, sp.B_SLOTS), v.reshape(N, ps.n_mol, sp.B_SLOTS, 3)


@pytest.mark.parametrize("grid", ["tiles", "chunks"])
@pytest.mark.parametrize("leaflets", [None, 3])
@pytest.mark.parametrize("box_name", BOX_NAMES)
def test_corr(built, monkeypatch, box_name, leaflets, grid):
    """k_bond_units + k_bond_corr: gm_calc_sch<false> of two DATA vectors, sqrtf(e.w), s2 * n2sq of two squared data norms.
    The probes move on by one slot a frame, and every fourth is an everyday bond: a slot's pairs hold a probe in the
    current vector, in the lagged one, and in both (lag 0: the same probe twice — S = 1, or NaN where its norm overflows)."""
    set_route(monkeypatch, {"GORDER_HIP_CORR_GRID": "chunks"} if grid == "chunks" else {})
    ps = case(2, box_name, swap_from=5)
    tables = probe_tables(ps, leaflets=global_leaflets(2, leaflets) if leaflets else None)
    eng = device(tables, ps, lambda e: e.set_bond_correlation(LAGS))
    sums, counts = eng.bond_correlation()
    got = eng.finish()
    ran(eng, "k_bond_corr")
    assert "k_bond_units" in eng.kernel_names()
    same_results(got, reference(tables, ps).finish())
    upper = sides(ps, leaflets) if leaflets else None
    special = np.array([p.family != "ordinary" for p in ps.probes])[ps.which]     # [frames, molecules, slots]
    seen = set()
    for k, lag in enumerate(LAGS):
        t, v = pair_ticks(ps, tables, lag)
        for (f, m, b), tick in np.ndenumerate(t):                                 # the literal statement, pair by pair
            assert tick == sp.literal_tick(v[lag + f, m, b], v[f, m, b]), (lag, f, m, b)
        np.testing.assert_array_equal(sums[k, 0], t.sum(axis=(0, 1)))
        np.testing.assert_array_equal(counts[k, 0], np.full(sp.B_SLOTS, (N - lag) * ps.n_mol, dtype=np.uint64))
        if leaflets:
            up = upper[lag:]                                                       # the leaflet of the LATER frame
            np.testing.assert_array_equal(sums[k, 1], (t * up[:, :, None]).sum(axis=(0, 1)))
            np.testing.assert_array_equal(counts[k, 2], np.broadcast_to((~up)[:, :, None], t.shape).sum(axis=(0, 1)))
        else:
            assert not sums[k, 1:].any() and not counts[k, 1:].any()
        if lag:
            seen |= set(zip(special[lag:].reshape(-1).tolist(), special[:N - lag].reshape(-1).tolist()))
    assert seen == {(True, True), (True, False), (False, True), (False, False)}


# ---- UA --------------------------------------------------------------------------------------------------------------------------
from test_sample_probes_cpu import UA_BOX, ua_case        # noqa: E402

UA_MAP = OrderMap(enabled=True, plane=0, span_x=(0.0, 8.0), span_y=(0.0, 8.0), bin=(1.0, 0.5))
UA_MODES = {"0 plain": dict(),
            "1 maps only": dict(ordermap=UA_MAP),
            "2 maps and rows": dict(ordermap=UA_MAP, timewise=True),
            "2 geometry": dict(geometry=Geometry(kind=GEOM_CYLINDER, reference=GEOMREF_POINT, point=(4.0, 4.0, 4.0), radius=3.0,
                                                 orientation=2, structure_box=UA_BOX)),
            "3 rows only": dict(timewise=True)}
UA_FLAGS = {"exact": 0, "exact acos": FLAG_TRIG_ACOS_COS, "fast": abi.FLAG_UA_FAST_NORMALISE}


@pytest.mark.parametrize("flags", list(UA_FLAGS))
@pytest.mark.parametrize("pbc", [True, False])
@pytest.mark.parametrize("mode", list(UA_MODES))
def test_ua(built, monkeypatch, mode, pbc, flags):
    """k_ua_extras<mode> and k_ua_extras_fast<mode>: in every frame a methyl, a methylene, a double-bond and a saturated CH
    carbon of every lipid is exactly degenerate — the carbon on a helper, two helpers on one spot, helper, carbon and helper
    collinear, a helper 2.5 box lengths away — so ua_carbon_pairs, ua_carbon and ua_carbon_fast raise `slow`, ua_carbon_slow
    makes the hydrogens the reference makes (NaN ones among them: tick 0, counted, on no tile and in no shape), and the
    inline guard of the sample hands them to gm_calc_sch."""
    set_route(monkeypatch, {})
    kw = dict(UA_MODES[mode])
    geometry = kw.pop("geometry", None)
    tables, xyz, box9, label = ua_case(pbc, leaflets=LEAFLETS_GLOBAL, flags=UA_FLAGS[flags], **kw)
    if geometry is not None:
        tables.geometry = geometry
    eng = HipEngine(tables)
    eng.kernel_time()
    o = oracle.OracleEngine(tables, trig=trig_of(tables))
    for a, b in CUTS:
        eng.submit_host(xyz[a:b], None if box9 is None else box9[a:b], FRAMES[a:b])
    o.submit(xyz, box9, FRAMES)
    got, want = eng.finish(), o.finish()
    ran(eng, "k_ua_extras", never=["k_bonds_tiled", "k_bonds_extras"])
    same_results(got, want)
    if tables.timewise:
        same_rows(eng, o)
    if geometry is None:
        assert (got.counts[0] == N * len(label[0])).all() and got.counts[1].all() and got.counts[2].all()
    else:
        assert 0 < got.counts[0].sum() < N * len(label[0]) * tables.n_acc
    if tables.ordermap.enabled:
        assert 0 < got.map_counts[0].sum() < got.counts[0].sum()                # the NaN hydrogens are on no tile


# ---- UA, every sample booked a second time -------------------------------------------------------------------------------------
import functools        # noqa: E402

import test_ua_samples_gpu as uas        # noqa: E402

UA_SAMPLE_FLAGS = {"exact": abi.FLAG_UA_SAMPLES, "exact acos": abi.FLAG_UA_SAMPLES | FLAG_TRIG_ACOS_COS}


@functools.lru_cache(maxsize=None)
def ua_samples_reference(pbc, flags):
    """The degenerate carbons with GORDER_FLAG_UA_SAMPLES -> (tables, xyz, box9, the split oracle's per-sample ticks, the
    unsplit oracle's leaflet flags and its finish())."""
    tables, xyz, box9, _ = ua_case(pbc, leaflets=LEAFLETS_GLOBAL, flags=UA_SAMPLE_FLAGS[flags])
    o = oracle.OracleEngine(dataclasses.replace(tables, flags=tables.flags & FLAG_TRIG_ACOS_COS), trig=trig_of(tables))
    o.submit(xyz, box9, FRAMES)
    return (tables, xyz, box9, uas.oracle_samples(tables, xyz, box9, trig_of(tables), FRAMES), uas.oracle_flags(tables, xyz, box9, FRAMES),
            o.finish())


@pytest.mark.parametrize("output", ["histogram lds", "histogram direct", "rows"])
@pytest.mark.parametrize("flags", list(UA_SAMPLE_FLAGS))
@pytest.mark.parametrize("pbc", [True, False])
def test_ua_samples(built, monkeypatch, pbc, flags, output):
    """k_ua_dist (the LDS table and the direct route) and k_ua_mol on test_ua's carbons: the same hand-over to ua_carbon_slow
    and the same guard of the tick as k_ua_extras, so the NaN hydrogens are tick 0, counted, in the bin [0, 1) and in their
    molecule's word.  Expected: the split oracle of test_ua_samples_gpu.py; finish() is the unsplit oracle's."""
    set_route(monkeypatch, {"GORDER_HIP_DIST_DIRECT": "1"} if output == "histogram direct" else {})
    tables, xyz, box9, samples, sides_, want = ua_samples_reference(pbc, flags)
    assert samples.present.all() and (samples.tick == 0).any() and 0 < int(sides_.sum()) < sides_.size
    eng = HipEngine(tables)
    eng.kernel_time()
    groups = [[s] for s in range(tables.n_acc)]
    if output == "rows":
        eng.set_molecule_rows(groups)
    else:
        eng.set_order_histogram(EDGES)
        assert eng.order_histogram_route()["direct"] == (output == "histogram direct")
    for a, b in CUTS:
        eng.submit_host(xyz[a:b], None if box9 is None else box9[a:b], FRAMES[a:b])
    if output == "rows":
        sums, counts, frames = eng.molecule_rows()
        want_s, want_c = uas.want_rows(samples, groups, tables.n_molecules_total)
        np.testing.assert_array_equal(frames, FRAMES)
        np.testing.assert_array_equal(counts.astype(np.int64), want_c)
        np.testing.assert_array_equal(sums.astype(np.int64), want_s)
        assert counts.sum() == N * tables.n_samples_per_frame
    else:
        got = eng.order_histogram()
        hist = uas.want_hist(samples, EDGES, sides_, tables.n_acc)
        assert got.dtype == np.uint64 and got.shape == hist.shape
        np.testing.assert_array_equal(got, hist)
        assert EDGES[2] == 0 and int(got[2, 0].sum()) == int((samples.tick == 0).sum()) > 0     # the bin [0, 1): the NaN hydrogens
    res = eng.finish()
    ran(eng, "k_ua_mol" if output == "rows" else "k_ua_dist", never=["k_ua_extras", "k_bonds_tiled", "k_bonds_extras"])
    same_results(res, want)
