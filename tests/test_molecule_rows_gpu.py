"""Per-molecule order rows (gorder_hip_set_molecule_rows, k_bonds_tiled_mol) on the device.

The reference for every integer is the existing oracle on SPLIT tables: every molecule its own molecule type, no leaflets,
timewise rows on — row [f, 0, slot(type, molecule, bond)] of its timewise() is then the single tick and count of that
sample, and a group's per-molecule value is the sum over the group's bonds.  TRIG_DIRECT restates the device's default
cosine, TRIG_MIRROR its literal one (FLAG_TRIG_ACOS_COS).  Every comparison of sums and counts is integer equality.

Systems: the coarse-grained membrane of 40 lipids in two molecule types (440 samples: one full and one partial tile; a lipid
has 11 bonds, so the 24th lipid's bonds lie in both tiles: a (group, molecule) word two tiles add into) with two disjoint
groups per type and one slot left ungrouped, and the all-atom membrane of 12 lipids (768 samples, three tiles) with the slots
0-31 and 32-63.  An all-atom lipid has 64 bonds and a tile 256 lanes, so at EVERY lipid count a tile holds exactly four whole
lipids: max_tiles_per_word is 1 there whatever the count, and 12 lipids stay.  The molecule split across tiles is therefore
asserted on the coarse-grained case and on "aa63", the same all-atom membrane without its last bond type (63 bonds a lipid:
the fifth lipid's bonds lie in two tiles)."""
import dataclasses

import numpy as np
import pytest

from gorder_amd import HipEngine, abi, synthetic, xtc
from gorder_amd.abi import (COLLECT_LEAFLETS, FLAG_TRIG_ACOS_COS, LEAFLETS_GLOBAL, LEAFLETS_LOCAL, LEAFLETS_NONE, Geometry, Leaflets, MolType, OrderMap,
                            Tables)
from oracle import oracle

pytestmark = pytest.mark.gpu

N = 11                                   # two full stages of four frames and a tail of three
FRAMES = np.arange(100, 100 + N, dtype=np.uint64)
CUTS = {"one": [(0, N)], "three": [(0, 4), (4, 5), (5, N)]}
CG_GROUPS = [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [11, 12, 13, 14, 15], [16, 17, 18, 19, 20, 21]]     # slot 10: in no group
AA_GROUPS = [list(range(0, 32)), list(range(32, 64))]


def split_tables(tables):
    """Every molecule its own molecule type -> (tables, slot0 [type][molecule]: the first slot of that molecule's bonds)."""
    mts, slot0, slot = [], [], 0
    for mt in tables.molecule_types:
        bonds = np.asarray(mt.bonds)
        slot0.append([])
        for i in range(mt.n_molecules):
            mts.append(MolType(n_molecules=1, bonds=bonds[:, i:i + 1, :]))
            slot0[-1].append(slot)
            slot += bonds.shape[0]
    return Tables(n_atoms=tables.n_atoms, molecule_types=mts, handle_pbc=tables.handle_pbc, normal=tables.normal,
                  leaflets=Leaflets(), timewise=True), slot0


def oracle_rows(tables, groups, xyz, box, trig):
    """(sums int64, counts int64) [frames, groups, molecules] from the split oracle."""
    split, slot0 = split_tables(tables)
    ref = oracle.OracleEngine(split, trig=trig)
    ref.submit(xyz, box, FRAMES[:len(xyz)])
    tw_s, tw_c = ref.timewise(len(xyz))
    assert int(tw_c[:, 0].max()) <= 1
    group_of = {s: g for g, slots in enumerate(groups) for s in slots}
    sums = np.zeros((len(xyz), len(groups), tables.n_molecules_total), dtype=np.int64)
    counts = np.zeros_like(sums)
    slot_t, mol = 0, 0
    for t, mt in enumerate(tables.molecule_types):
        for i in range(mt.n_molecules):
            for b in range(mt.n_bond_types):
                g = group_of.get(slot_t + b)
                if g is not None:
                    sums[:, g, mol] += tw_s[:, 0, slot0[t][i] + b]
                    counts[:, g, mol] += tw_c[:, 0, slot0[t][i] + b].astype(np.int64)
            mol += 1
        slot_t += mt.n_bond_types
    return sums, counts


@dataclasses.dataclass
class Case:
    system: object
    groups: list
    xyz: np.ndarray
    box: np.ndarray
    want: tuple


def make_case(system, groups, trig=oracle.TRIG_DIRECT, seed=5):
    xyz = system.frames(N, seed=seed)
    box = system.box9(N) if system.tables.handle_pbc else None
    return Case(system, groups, xyz, box, oracle_rows(system.tables, groups, xyz, box, trig))


def aa63():
    system = synthetic.aa_membrane(12)
    mt = system.tables.molecule_types[0]
    mt.bonds = np.ascontiguousarray(np.asarray(mt.bonds)[:63])
    return system


@pytest.fixture(scope="module")
def cases(built):
    return {"cg": make_case(synthetic.cg_membrane(40, leaflets=LEAFLETS_GLOBAL, n_types=2), CG_GROUPS),
            "aa": make_case(synthetic.aa_membrane(12), AA_GROUPS),
            "aa63": make_case(aa63(), [list(range(0, 32)), list(range(32, 63))]),
            # a static normal along x: this route runs the general normal's code where the plain handle runs the axis form
            "cgx": make_case(synthetic.cg_membrane(40, leaflets=LEAFLETS_GLOBAL, n_types=2, normal=(1.0, 0.0, 0.0)), CG_GROUPS)}


def run(case, cuts=CUTS["one"], groups=None, tables=None, engine=None):
    eng = engine or HipEngine(tables or case.system.tables)
    if engine is None:
        eng.set_molecule_rows(case.groups if groups is None else groups)
    for a, b in cuts:
        eng.submit_host(case.xyz[a:b], None if case.box is None else case.box[a:b], FRAMES[a:b])
    return eng


def assert_rows(eng, want, n=N):
    sums, counts, frames = eng.molecule_rows()
    assert sums.dtype == np.int32 and counts.dtype == np.uint32 and frames.dtype == np.uint64
    np.testing.assert_array_equal(frames, FRAMES[:n])
    np.testing.assert_array_equal(counts.astype(np.int64), want[1][:n])
    np.testing.assert_array_equal(sums.astype(np.int64), want[0][:n])
    assert eng.molecule_rows_count() == n
    return sums, counts


# ---- 1. rows against the split oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("wg_target", [None, 1])
@pytest.mark.parametrize("cuts", list(CUTS))
@pytest.mark.parametrize("name", ["cg", "aa", "aa63"])
def test_rows_against_the_split_oracle(cases, monkeypatch, name, cuts, wg_target):
    case = cases[name]
    if wg_target:
        monkeypatch.setenv("GORDER_HIP_WG_TARGET", str(wg_target))       # one workgroup walks all frames of a tile
    eng = run(case, CUTS[cuts])
    stats = eng.molecule_rows_stats()
    n_samples = {"cg": 440, "aa": 768, "aa63": 756}[name]
    assert case.system.tables.n_samples_per_frame == n_samples and eng.plan()["n_tiles"] == (2 if name == "cg" else 3)
    assert stats["max_runs_per_tile"] >= 2                               # a tile shared by molecules
    if name == "aa":
        assert stats["max_tiles_per_word"] == 1                          # four whole lipids a tile (the module's docstring)
        assert stats["n_runs"] == 12 * 2
    else:
        assert stats["max_tiles_per_word"] >= 2                          # a molecule split across tiles
    sums, counts = assert_rows(eng, case.want)
    assert counts.sum() > 0 and (counts == 0).any() == (name == "cg")    # cg: a group holds one type's slots only


# ---- 2. the ordinary results are untouched -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cg", "aa", "cgx"])
def test_finish_is_untouched(cases, name):
    case = cases[name]
    eng = run(case, CUTS["three"])
    plain = HipEngine(case.system.tables)
    for a, b in CUTS["three"]:
        plain.submit_host(case.xyz[a:b], case.box[a:b], FRAMES[a:b])
    got, want = eng.finish(), plain.finish()
    np.testing.assert_array_equal(got.sums, want.sums)
    np.testing.assert_array_equal(got.counts, want.counts)
    assert got.n_frames == want.n_frames == N and want.counts[0].min() > 0
    sums, counts, _ = eng.molecule_rows()
    for g, slots in enumerate(case.groups):
        assert int(sums[:, g].astype(np.int64).sum()) == int(want.sums[0, slots].sum())
        assert int(counts[:, g].astype(np.int64).sum()) == int(want.counts[0, slots].sum())


# ---- 3. leaflets do not enter ----------------------------------------------------------------------------------------------
def test_leaflets_do_not_enter(cases):
    case = cases["cg"]
    none = synthetic.cg_membrane(40, leaflets=LEAFLETS_NONE, n_types=2)
    np.testing.assert_array_equal(none.base, case.system.base)
    with_lf, without = run(case), run(case, tables=none.tables)
    a, b = with_lf.molecule_rows(), without.molecule_rows()
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert_rows(without, case.want)
    # collected leaflets next to the rows
    both = HipEngine(case.system.tables)
    both.set_collect(COLLECT_LEAFLETS)
    both.set_molecule_rows(case.groups)
    only = HipEngine(case.system.tables)
    only.set_collect(COLLECT_LEAFLETS)
    for eng in (both, only):
        for lo, hi in CUTS["three"]:
            eng.submit_host(case.xyz[lo:hi], case.box[lo:hi], FRAMES[lo:hi])
    (f1, r1), (f2, r2) = both.collected_leaflets(), only.collected_leaflets()
    np.testing.assert_array_equal(f1, f2)
    np.testing.assert_array_equal(r1, FRAMES)
    np.testing.assert_array_equal(r2, FRAMES)
    assert 0 < int(f1.sum()) < f1.size
    assert_rows(both, case.want)
    # the upper and lower sums of finish() are those of a handle without rows too (test 2 compares all three planes)
    np.testing.assert_array_equal(both.finish().sums, only.finish().sums)


# ---- 4. literal cosine, a general static normal, no periodic boundaries ---------------------------------------------------
def test_literal_cosine(built):
    system = synthetic.cg_membrane(40, leaflets=LEAFLETS_GLOBAL, n_types=2)
    system.tables.flags = FLAG_TRIG_ACOS_COS
    case = make_case(system, CG_GROUPS, trig=oracle.TRIG_MIRROR)
    assert_rows(run(case, CUTS["three"]), case.want)
    direct = oracle_rows(system.tables, CG_GROUPS, case.xyz, case.box, oracle.TRIG_DIRECT)
    assert (direct[0] != case.want[0]).any()                             # the two cosine modes do differ on these frames


def test_general_static_normal(built):
    r = float(np.float32(1.0 / np.sqrt(2.0)))
    case = make_case(synthetic.cg_membrane(40, leaflets=LEAFLETS_GLOBAL, n_types=2, normal=(r, r, 0.0)), CG_GROUPS)
    assert_rows(run(case, CUTS["three"]), case.want)


def test_static_normal_along_x(cases):
    case = cases["cgx"]
    assert_rows(run(case, CUTS["three"]), case.want)
    z = cases["cg"]
    assert (z.want[0] != case.want[0]).any()


@pytest.mark.parametrize("method, frequency, flip", [(LEAFLETS_GLOBAL, 5, True), (LEAFLETS_LOCAL, 1, False), (LEAFLETS_LOCAL, 5, False)])
def test_other_leaflet_methods_and_frequencies(cases, method, frequency, flip):
    """Assignment frames 100, 105, 110 only (fewer assignment rows than frames), flip, local leaflets: the rows are the same
    integers, and finish() — upper and lower sums included — is that of a handle without rows."""
    case = cases["cg"]
    system = synthetic.cg_membrane(40, leaflets=method, frequency=frequency, flip=flip, n_types=2, radius=1.2)
    np.testing.assert_array_equal(system.base, case.system.base)
    eng = run(case, CUTS["three"], tables=system.tables)
    assert_rows(eng, case.want)
    plain = HipEngine(system.tables)
    for a, b in CUTS["three"]:
        plain.submit_host(case.xyz[a:b], case.box[a:b], FRAMES[a:b])
    got, want = eng.finish(), plain.finish()
    np.testing.assert_array_equal(got.sums, want.sums)
    np.testing.assert_array_equal(got.counts, want.counts)
    assert want.counts[1].sum() > 0 and want.counts[2].sum() > 0


def test_no_periodic_boundaries(built):
    case = make_case(synthetic.cg_membrane(40, leaflets=LEAFLETS_NONE, n_types=2, handle_pbc=False), CG_GROUPS)
    assert case.box is None
    assert_rows(run(case, CUTS["three"]), case.want)


# ---- 5. staging sub-ranges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cg", "aa"])
def test_staging_subranges(cases, monkeypatch, name):
    case = cases[name]
    monkeypatch.setenv("GORDER_HIP_MOL_ROWS_STAGING", str(2 * len(case.groups) * case.system.tables.n_molecules_total * 8))   # two frames fill it
    eng = run(case)
    monkeypatch.delenv("GORDER_HIP_MOL_ROWS_STAGING")
    assert_rows(eng, case.want)
    plain = HipEngine(case.system.tables)
    plain.submit_host(case.xyz, case.box, FRAMES)
    np.testing.assert_array_equal(eng.finish().sums, plain.finish().sums)


# ---- 6. from a file --------------------------------------------------------------------------------------------------------
def test_from_a_file_decoded_on_the_device(cases, tmp_path):
    case = cases["cg"]
    path = str(tmp_path / "cg.xtc")
    xtc.write_trajectory(path, case.xyz, case.box.reshape(N, 3, 3), precision=1000.0)
    decoded = xtc.read_trajectory([path])[0]
    host = HipEngine(case.system.tables)
    host.set_molecule_rows(case.groups)
    host.submit_host(decoded, case.box, FRAMES)
    want = host.molecule_rows()
    eng = HipEngine(case.system.tables)
    eng.set_molecule_rows(case.groups)
    stats = eng.run_trajectory([path], threads=2, batch_frames=4, first_frame_index=100, device_decode=True)
    assert stats["n_frames"] == N and stats["device_decode"] == 1
    got = eng.molecule_rows()
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(got[2], FRAMES)
    np.testing.assert_array_equal(eng.finish().sums, host.finish().sums)
    ref = oracle_rows(case.system.tables, case.groups, decoded, case.box, oracle.TRIG_DIRECT)
    np.testing.assert_array_equal(got[0].astype(np.int64), ref[0])


# ---- 7. errors unchanged ---------------------------------------------------------------------------------------------------
def test_errors_are_unchanged(built):
    system = synthetic.cg_membrane(40, leaflets=LEAFLETS_NONE, n_types=2)
    xyz, box = system.frames(N, seed=5), system.box9(N)
    xyz[4, 12 * 7 + 5] = np.nan                                          # a bead of lipid 7, in the middle of its chain
    seen = []
    for rows in (False, True):
        eng = HipEngine(system.tables)
        if rows:
            eng.set_molecule_rows(CG_GROUPS)
        with pytest.raises(abi.GorderHipError) as e:
            for a, b in CUTS["three"]:
                eng.submit_host(xyz[a:b], box[a:b], FRAMES[a:b])
            eng.finish()
        seen.append((e.value.status, e.value.index, e.value.frame))
    assert seen[0] == seen[1] and seen[0][0] == abi.ERR_UNDEFINED_POSITION and seen[0][2] == 104
    assert eng.molecule_rows_count() == 4                                # the rows end where the run ended
    with pytest.raises(abi.GorderHipError):
        eng.molecule_rows()
    # the rows of the batch before the failing one are the oracle's
    eng.reset()
    eng.submit_host(xyz[:4], box[:4], FRAMES[:4])
    want = oracle_rows(system.tables, CG_GROUPS, xyz[:4], box[:4], oracle.TRIG_DIRECT)
    assert_rows(eng, want, 4)


# ---- 8. reset ---------------------------------------------------------------------------------------------------------------
def test_reset_clears_the_rows_and_keeps_the_groups(cases):
    case = cases["cg"]
    eng = run(case, CUTS["three"])
    first = eng.molecule_rows()
    stats = eng.molecule_rows_stats()
    eng.reset()
    assert eng.molecule_rows_count() == 0 and eng.molecule_rows()[0].shape == (0, len(case.groups), 40)
    assert eng.molecule_rows_stats() == stats
    run(case, CUTS["one"], engine=eng)
    for x, y in zip(eng.molecule_rows(), first):
        np.testing.assert_array_equal(x, y)
    assert_rows(eng, case.want)


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------
def refused(tables, groups=None, before=None):
    eng = HipEngine(tables)
    if before:
        before(eng)
    with pytest.raises(abi.GorderHipError) as e:
        eng.set_molecule_rows(CG_GROUPS if groups is None else groups)
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
    return str(e.value)


def test_refusals(cases):
    def membrane(**kw):
        return synthetic.cg_membrane(40, leaflets=LEAFLETS_GLOBAL, n_types=2, **kw)

    assert "united-atom" in refused(synthetic.ua_membrane(24).tables, [[0]])
    om = OrderMap(enabled=True, plane=0, span_x=(0.0, 4.0), span_y=(0.0, 4.0), bin=(0.4, 0.4))
    assert "ordermaps" in refused(membrane(ordermap=om).tables)
    assert "timewise" in refused(membrane(timewise=True).tables)
    geom = membrane()
    geom.tables.geometry = Geometry(kind=abi.GEOM_SPHERE, reference=abi.GEOMREF_BOX_CENTER, radius=2.0)
    assert "geometry" in refused(geom.tables)
    dyn = membrane()
    dyn.tables.dynamic_normal = abi.DynamicNormal(enabled=True, radius=2.0, cloud=np.concatenate([m.heads for m in dyn.tables.molecule_types]))
    for m in dyn.tables.molecule_types:
        m.normal_heads = m.heads
    assert "dynamic" in refused(dyn.tables)
    t = membrane().tables
    up = np.tile(np.array([0.0, 0.0, 1.0], dtype=np.float32), (2, t.n_molecules_total, 1))
    assert "normal table" in refused(t, before=lambda e: e.set_manual_normal_table(up))
    assert "gorder_hip_set_normals" in refused(t, before=lambda e: e.set_normals(up))
    shells = membrane()
    shells.tables.geometry = Geometry(kind=abi.GEOM_CYLINDER, reference=abi.GEOMREF_BOX_CENTER, orientation=2, radius=2.0,
                                      structure_box=tuple(float(x) for x in shells.box))
    assert "radial shells" in refused(shells.tables, before=lambda e: e.set_radial_shells([1.0, 2.0]))
    wide = synthetic.cg_membrane(200, leaflets=LEAFLETS_GLOBAL, n_types=2)
    b = np.asarray(wide.tables.molecule_types[0].bonds).copy()
    b[0, 0] = (0, 12 * 199 + 11)                                       # 2400 atoms apart: more than the 1024-atom window
    wide.tables.molecule_types[0].bonds = b
    assert "LDS window" in refused(wide.tables)
    # the groups themselves
    assert "empty" in refused(t, [[0, 1], [], [2]])
    assert "out of range" in refused(t, [[0, 22]])
    assert "two groups" in refused(t, [[0, 1], [1, 2]])
    assert "2047" in refused(t, [list(range(2048))])
    eng = HipEngine(t)
    begin, slots = np.array([0, 2, 1], dtype=np.uint32), np.array([0, 1, 2], dtype=np.uint32)
    st = eng.lib.gorder_hip_set_molecule_rows(eng._h, begin.ctypes.data, slots.ctypes.data, 2)
    assert st == abi.ERR_INVALID_ARGUMENT and "ascending" in eng.lib.gorder_hip_last_error_message(eng._h).decode()
    # a handle with rows refuses what the rows refuse
    eng.set_molecule_rows(CG_GROUPS)
    for call, word in ((lambda: eng.set_normals(up), "molecule rows"), (lambda: eng.set_manual_normal_table(up), "molecule rows"),
                       (lambda: eng.set_radial_shells([1.0, 2.0]), "molecule rows")):
        with pytest.raises(abi.GorderHipError) as e:
            call()
        assert e.value.status == abi.ERR_INVALID_ARGUMENT and word in str(e.value)
    sh = HipEngine(shells.tables)
    with pytest.raises(abi.GorderHipError) as e:                        # (rows on a handle with a selection: refused before the shells can be)
        sh.set_molecule_rows(CG_GROUPS)
    assert "geometry" in str(e.value)
    # after the first submit; reset opens the setter again; an empty list switches the rows off
    case = cases["cg"]
    eng = HipEngine(case.system.tables)
    eng.submit_host(case.xyz[:1], case.box[:1], FRAMES[:1])
    with pytest.raises(abi.GorderHipError) as e:
        eng.set_molecule_rows(CG_GROUPS)
    assert e.value.status == abi.ERR_INVALID_ARGUMENT and "first submit" in str(e.value)
    eng.reset()
    eng.set_molecule_rows(CG_GROUPS)
    eng.reset()
    eng.set_molecule_rows([])
    assert eng.molecule_rows_count() == 0
    eng.submit_host(case.xyz, case.box, FRAMES)
    with pytest.raises(abi.GorderHipError) as e:
        eng.molecule_rows()
    assert e.value.status == abi.ERR_INVALID_ARGUMENT and "off" in str(e.value)
    plain = HipEngine(case.system.tables)
    plain.submit_host(case.xyz, case.box, FRAMES)
    np.testing.assert_array_equal(eng.finish().sums, plain.finish().sums)
    assert "k_bonds_tiled_mol" not in eng.kernel_names()
