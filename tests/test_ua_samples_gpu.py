"""United atoms in order histograms and per-molecule rows (GORDER_FLAG_UA_SAMPLES: k_ua_dist, k_ua_mol) on the device.

The reference for every integer is the existing oracle on SPLIT tables: every molecule its own molecule type (the `ua_atoms`
rows sliced as [(kind, idx[i:i + 1])], bond tables as bonds[:, i:i + 1]), Leaflets(), timewise on, flags 0 — row [f, 0, slot]
of its timewise() is then the single tick of that sample with count 1, or count 0 outside a geometry selection.  The leaflet
planes use the flags of the UNSPLIT oracle, taken frame by frame with OracleEngine.leaflets().  TRIG_DIRECT restates the
device's default cosine, TRIG_MIRROR its literal one.  Every comparison is integer equality.

Systems, 11 frames each (k_ua_mol stages four frames: two full stages and a tail of three), frame indices from 100:
  ua6    synthetic.ua_membrane(6): one partial tile of 192 lanes with all four carbon kinds in it (waves mix kinds) and 62
         local slots, the widest tile there is
  ua17   ua_membrane(17): a full block of 16 molecules and a block of one in the (kind, quad, 16-molecule) lane order
  ua70   ua_membrane(70): a group of 64 molecules gives eight full tiles of 4 slots x 64 molecules, the group of 6 a partial
         one; tile boundaries fall inside a kind; a whole-lipid word is fed by eight tiles
  mixed  40 coarse-grained lipids in two types, then six united-atom lipids, on one handle: bond tiles and united-atom tiles,
         84 slots"""
import dataclasses

import numpy as np
import pytest

from gorder_amd import HipEngine, abi, structure, synthetic, xtc
from gorder_amd.abi import (COLLECT_LEAFLETS, FLAG_TRIG_ACOS_COS, FLAG_UA_FAST_NORMALISE, FLAG_UA_SAMPLES, LEAFLETS_GLOBAL, LEAFLETS_INDIVIDUAL,
                            LEAFLETS_LOCAL, LEAFLETS_NONE, Geometry, Leaflets, MolType, OrderMap, Tables)
from oracle import oracle

pytestmark = pytest.mark.gpu

N = 11                                   # two full stages of four frames and a tail of three
FRAMES = np.arange(100, 100 + N, dtype=np.uint64)
CUTS = {"one": [(0, N)], "three": [(0, 4), (4, 5), (5, N)]}
BOX = (9.0, 9.0, 8.0)


# ---- the split oracle --------------------------------------------------------------------------------------------------------
def split_tables(tables):
    """Every molecule its own molecule type -> (tables, slot0 [type][molecule]: the first slot of that molecule's samples).
    Everything else of the tables (normal, periodic boundaries, geometry) stays."""
    mts, slot0, slot = [], [], 0
    for mt in tables.molecule_types:
        slot0.append([])
        for i in range(mt.n_molecules):
            mts.append(MolType(n_molecules=1, bonds=None if mt.bonds is None else np.asarray(mt.bonds)[:, i:i + 1, :],
                               ua_atoms=[(kind, np.asarray(idx)[i:i + 1]) for kind, idx in mt.ua_atoms]))
            slot0[-1].append(slot)
            slot += mt.n_slots
    return dataclasses.replace(tables, molecule_types=mts, leaflets=Leaflets(), timewise=True, flags=0), slot0


@dataclasses.dataclass
class Samples:
    tick: np.ndarray        # int64 [frames, samples]
    present: np.ndarray     # bool  [frames, samples]: the oracle counted the sample (inside the selection)
    slot: np.ndarray        # [samples] accumulator slot of the unsplit tables
    mol: np.ndarray         # [samples] molecule (molecule-type-major, as the leaflet flags)


def oracle_samples(tables, xyz, box, trig, frames=FRAMES):
    split, slot0 = split_tables(tables)
    ref = oracle.OracleEngine(split, trig=trig)
    ref.submit(xyz, box, frames[:len(xyz)])
    tw_s, tw_c = ref.timewise(len(xyz))
    assert int(tw_c[:, 0].max()) == 1                                    # a slot of the split tables is one sample
    cols, slots, mols = [], [], []
    slot_t, mol = 0, 0
    for t, mt in enumerate(tables.molecule_types):
        for i in range(mt.n_molecules):
            for b in range(mt.n_slots):
                cols.append(slot0[t][i] + b); slots.append(slot_t + b); mols.append(mol)
            mol += 1
        slot_t += mt.n_slots
    return Samples(tw_s[:, 0, cols].astype(np.int64), tw_c[:, 0, cols] == 1, np.array(slots), np.array(mols))


def oracle_flags(tables, xyz, box, frames=FRAMES):
    """uint8 [frames, molecules]: the side (Upper = 0) every frame's samples are booked on, or None without leaflets."""
    if tables.leaflets.method == LEAFLETS_NONE:
        return None
    ref = oracle.OracleEngine(dataclasses.replace(tables, flags=0), trig=oracle.TRIG_DIRECT)
    rows = []
    for f in range(len(xyz)):
        ref.submit(xyz[f:f + 1], None if box is None else box[f:f + 1], frames[f:f + 1])
        rows.append(ref.leaflets()[0].copy())
    return np.array(rows)


def want_hist(samples, edges, flags, n_acc, frames=slice(None)):
    """uint64 [n_bins, 3, n_acc] from the oracle's ticks, with numpy integers."""
    edges = np.asarray(edges, dtype=np.int64)
    n_bins = len(edges) - 1
    tick, present = samples.tick[frames], samples.present[frames]
    bins = np.searchsorted(edges, tick, "right") - 1
    ok = present & (bins >= 0) & (bins < n_bins)
    slot = np.broadcast_to(samples.slot, tick.shape)
    out = np.zeros((n_bins, 3, n_acc), dtype=np.uint64)
    np.add.at(out[:, 0], (bins[ok], slot[ok]), 1)
    if flags is not None:
        upper = flags[frames][:, samples.mol] == 0
        np.add.at(out[:, 1], (bins[ok & upper], slot[ok & upper]), 1)
        np.add.at(out[:, 2], (bins[ok & ~upper], slot[ok & ~upper]), 1)
    return out


def want_rows(samples, groups, n_mol):
    """(sums, counts) int64 [frames, groups, molecules] from the oracle's ticks."""
    group_of = {s: g for g, slots in enumerate(groups) for s in slots}
    sums = np.zeros((samples.tick.shape[0], len(groups), n_mol), dtype=np.int64)
    counts = np.zeros_like(sums)
    for q, (slot, mol) in enumerate(zip(samples.slot, samples.mol)):
        g = group_of.get(int(slot))
        if g is not None:
            sums[:, g, mol] += np.where(samples.present[:, q], samples.tick[:, q], 0)
            counts[:, g, mol] += samples.present[:, q]
    return sums, counts


def data_edges(samples):
    """Edges ..., t, t + 1, ... around ticks the oracle observed — the most frequent one, the smallest, the middle one and the
    largest: three at least — so that both sides of the half-open rule are pinned on real samples -> (edges, [(t, multiplicity)])."""
    seen, mult = np.unique(samples.tick[samples.present], return_counts=True)
    picks = sorted({int(seen[np.argmax(mult)]), int(seen[0]), int(seen[len(seen) // 2]), int(seen[-1])})
    assert len(picks) >= 3
    edges = sorted({-500000, 1000001} | {t for t in picks} | {t + 1 for t in picks})
    return np.array(edges), [(t, int(mult[seen == t][0])) for t in picks]


# ---- systems -----------------------------------------------------------------------------------------------------------------
def ua(n, **kw):
    system = synthetic.ua_membrane(n, **kw)
    system.tables.flags = FLAG_UA_SAMPLES
    return system


def mixed():
    cg, u = synthetic.cg_membrane(40, box=BOX, n_types=2), synthetic.ua_membrane(6, box=BOX)
    assert cg.n_atoms == 480 and u.n_atoms == 312
    mts = list(cg.tables.molecule_types)
    mts.append(MolType(n_molecules=6, ua_atoms=[(kind, np.asarray(idx) + 480) for kind, idx in u.tables.molecule_types[0].ua_atoms], name="POPC"))
    tables = Tables(n_atoms=792, molecule_types=mts, handle_pbc=True, normal=(0.0, 0.0, 1.0), flags=FLAG_UA_SAMPLES)
    assert tables.n_acc == 84
    return synthetic.System("mixed", tables, np.concatenate([cg.base, u.base]), np.asarray(BOX, dtype=np.float32), jitter=0.01)


def type_groups(tables):
    """One group per molecule type — what structure.molecule_groups gives for these tables' labels (asserted below)."""
    labels, slot = [], 0
    for mt in tables.molecule_types:
        if mt.ua_atoms:
            carbons = [structure.UaCarbonLabel(q, f"C{q}", int(kind), abi.UA_N_H[int(kind)]) for q, (kind, _) in enumerate(mt.ua_atoms)]
            labels.append(structure.UaMolLabels(mt.name, carbons, mt.n_molecules, slot))
        else:
            bond = structure.BondLabel(1, "A", 2, "B")
            labels.append(structure.MolLabels(mt.name, [bond] * mt.n_bond_types, n_molecules=mt.n_molecules, slot0=slot))
        slot += mt.n_slots
    groups, _ = structure.molecule_groups(labels, "ua")
    assert sorted(s for g in groups for s in g) == list(range(tables.n_acc))
    return groups


def split_groups(tables):
    """Groups that split a carbon's hydrogens: the slots of hydrogen 0 of every united-atom carbon, the slots of hydrogens 1
    and 2, and one slot (the last hydrogen-0 slot) in no group; bond slots, where there are any, in a group of their own."""
    first, rest, bonds, slot = [], [], [], 0
    for mt in tables.molecule_types:
        bonds += list(range(slot, slot + mt.n_bond_types))
        slot += mt.n_bond_types
        for kind, _ in mt.ua_atoms:
            nh = abi.UA_N_H[int(kind)]
            first.append(slot)
            rest += list(range(slot + 1, slot + nh))
            slot += nh
    return [g for g in (first[:-1], rest, bonds) if g]


@dataclasses.dataclass
class Case:
    system: object
    xyz: np.ndarray
    box: np.ndarray
    samples: Samples
    flags: np.ndarray

    @property
    def tables(self):
        return self.system.tables

    @property
    def n_acc(self):
        return self.system.tables.n_acc


def make_case(system, trig=oracle.TRIG_DIRECT, seed=5, xyz=None):
    xyz = system.frames(N, seed=seed) if xyz is None else xyz
    box = system.box9(N) if system.tables.handle_pbc else None
    return Case(system, xyz, box, oracle_samples(system.tables, xyz, box, trig), oracle_flags(system.tables, xyz, box))


@pytest.fixture(scope="module")
def cases(built):
    return {"ua6": make_case(ua(6)), "ua17": make_case(ua(17)), "ua70": make_case(ua(70)), "mixed": make_case(mixed())}


def submit(eng, case, cuts):
    for a, b in cuts:
        eng.submit_host(case.xyz[a:b], None if case.box is None else case.box[a:b], FRAMES[a:b])
    return eng


def run_hist(case, edges, cuts=CUTS["one"], tables=None):
    eng = HipEngine(tables or case.tables)
    eng.set_order_histogram(edges)
    return submit(eng, case, cuts)


def run_rows(case, groups, cuts=CUTS["one"], tables=None):
    eng = HipEngine(tables or case.tables)
    eng.set_molecule_rows(groups)
    return submit(eng, case, cuts)


def run_plain(case, cuts=CUTS["three"], tables=None):
    return submit(HipEngine(tables or case.tables), case, cuts)


def assert_hist(eng, case, edges, flags="case"):
    got = eng.order_histogram()
    want = want_hist(case.samples, edges, case.flags if isinstance(flags, str) else flags, case.n_acc)
    assert got.dtype == np.uint64 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    return got


def assert_rows(eng, case, groups, n=N):
    want = want_rows(case.samples, groups, case.tables.n_molecules_total)
    sums, counts, frames = eng.molecule_rows()
    assert sums.dtype == np.int32 and counts.dtype == np.uint32 and frames.dtype == np.uint64
    np.testing.assert_array_equal(frames, FRAMES[:n])
    np.testing.assert_array_equal(counts.astype(np.int64), want[1][:n])
    np.testing.assert_array_equal(sums.astype(np.int64), want[0][:n])
    assert eng.molecule_rows_count() == n
    return sums, counts


# ---- 1. histogram counts against the split oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lds", "direct"])
@pytest.mark.parametrize("wg_target", [None, 1])
@pytest.mark.parametrize("cuts", list(CUTS))
@pytest.mark.parametrize("name", ["ua6", "ua17", "ua70", "mixed"])
def test_histogram_against_the_split_oracle(cases, monkeypatch, name, cuts, wg_target, route):
    case = cases[name]
    if wg_target:
        monkeypatch.setenv("GORDER_HIP_WG_TARGET", str(wg_target))       # one workgroup walks all frames of a tile
    if route == "direct":
        monkeypatch.setenv("GORDER_HIP_DIST_DIRECT", "1")
    n_samples = {"ua6": 372, "ua17": 1054, "ua70": 4340, "mixed": 440 + 372}[name]
    assert case.tables.n_samples_per_frame == n_samples and case.samples.present.all()
    derived, picks = data_edges(case.samples)
    for label, edges in {"derived": derived, "uniform16": structure.order_edges(16)}.items():
        eng = run_hist(case, edges, CUTS[cuts])
        assert eng.order_histogram_route()["direct"] == (route == "direct")
        got = assert_hist(eng, case, edges)
        np.testing.assert_array_equal(got.sum(axis=0), eng.finish().counts)      # covering edges: the bins add up to finish()
        assert int(got[:, 0].sum()) == N * n_samples
        if label == "derived":
            for t, m in picks:
                k = int(np.flatnonzero(edges == t)[0])
                assert edges[k + 1] == t + 1 and int(got[k, 0].sum()) == m, (t, m)


def test_the_widest_tile_takes_the_direct_route_by_itself(cases):
    """ua6 is one tile of 62 local slots: with 256 bins and two leaflet planes its table is 2 x 256 x 62 x 4 B = 127 KB."""
    system = ua(6, leaflets=LEAFLETS_GLOBAL)
    np.testing.assert_array_equal(system.base, cases["ua6"].system.base)
    case = make_case(system)
    wide, narrow = structure.order_edges(256), structure.order_edges(16)
    eng = run_hist(case, wide, CUTS["three"])
    assert eng.order_histogram_route() == {"direct": True, "table_bytes": 2 * 256 * 62 * 4}
    got = assert_hist(eng, case, wide)
    np.testing.assert_array_equal(got[:, 1] + got[:, 2], got[:, 0])
    eng = run_hist(case, narrow, CUTS["three"])
    assert eng.order_histogram_route() == {"direct": False, "table_bytes": 2 * 16 * 62 * 4}
    assert_hist(eng, case, narrow)


# ---- 2. molecule rows against the split oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("grouping", ["types", "split"])
@pytest.mark.parametrize("wg_target", [None, 1])
@pytest.mark.parametrize("cuts", list(CUTS))
@pytest.mark.parametrize("name", ["ua6", "ua17", "ua70", "mixed"])
def test_rows_against_the_split_oracle(cases, monkeypatch, name, cuts, wg_target, grouping):
    case = cases[name]
    if wg_target:
        monkeypatch.setenv("GORDER_HIP_WG_TARGET", str(wg_target))
    groups = type_groups(case.tables) if grouping == "types" else split_groups(case.tables)
    if grouping == "split":
        assert len(groups) == (3 if name == "mixed" else 2) and len(groups[0]) == 31 and len(groups[1]) == 30
        assert sum(len(g) for g in groups) == case.n_acc - 1             # one slot in no group
    eng = run_rows(case, groups, CUTS[cuts])
    stats = eng.molecule_rows_stats()
    if name == "ua70" and grouping == "types":
        assert stats["max_tiles_per_word"] >= 8                          # a whole-lipid word is fed by eight tiles
    if name == "ua6":                                                    # one tile: a word per (group, molecule)
        assert stats == {"n_runs": 6 * len(groups), "max_runs_per_tile": 6 * len(groups), "max_tiles_per_word": 1}
    sums, counts = assert_rows(eng, case, groups)
    assert counts.sum() == N * sum(len(g) * m for g, m in zip(groups, group_molecules(case.tables, groups)))


def group_molecules(tables, groups):
    """How many molecules have the slots of each group (every group here lies inside one kind of molecule type)."""
    out = []
    for g in groups:
        slot = 0
        for mt in tables.molecule_types:
            if slot <= g[0] < slot + mt.n_slots:
                out.append(mt.n_molecules)
            slot += mt.n_slots
    # (the two coarse-grained types of `mixed` share the bonds' group: 11 slots of each type, 20 molecules each)
    return out


# ---- 3. the ordinary results are untouched, and the flag alone changes nothing ----------------------------------------------
@pytest.mark.parametrize("name", ["ua70", "ua6x"])
def test_finish_is_untouched(cases, name):
    case = cases["ua70"] if name == "ua70" else make_case(ua(6, normal=(1.0, 0.0, 0.0)))
    edges = structure.tilt_edges(90)[0]
    groups = type_groups(case.tables)
    hist, rows, flagged = HipEngine(case.tables), HipEngine(case.tables), HipEngine(case.tables)
    plain = HipEngine(dataclasses.replace(case.tables, flags=0))
    hist.set_order_histogram(edges)
    rows.set_molecule_rows(groups)
    for e in (hist, rows, flagged, plain):
        e.kernel_time()                   # switches the timing on
        submit(e, case, CUTS["three"])
    want = plain.finish()
    assert want.n_frames == N and want.counts[0].min() > 0
    for e in (hist, rows, flagged):
        got = e.finish()
        np.testing.assert_array_equal(got.sums, want.sums)
        np.testing.assert_array_equal(got.counts, want.counts)
        assert got.n_frames == N
    for e in (hist, rows, flagged, plain):
        e.kernel_time()
    # a flagged handle that calls neither setter queues what a flag-less one queues
    assert flagged.kernel_names() == plain.kernel_names() and "k_ua_extras" in plain.kernel_names()
    assert "k_ua_dist" in hist.kernel_names() and "k_ua_extras" not in hist.kernel_names()
    assert "k_ua_mol" in rows.kernel_names() and "k_ua_extras" not in rows.kernel_names()
    assert "k_ua_dist" not in plain.kernel_names() and "k_ua_mol" not in plain.kernel_names()
    assert_hist(hist, case, edges)
    assert_rows(rows, case, groups)
    if name == "ua6x":
        assert (cases["ua6"].samples.tick != case.samples.tick).any()    # the normal does enter


# ---- 4. leaflets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method, frequency", [(LEAFLETS_GLOBAL, 1), (LEAFLETS_GLOBAL, 5), (LEAFLETS_LOCAL, 1), (LEAFLETS_INDIVIDUAL, 1)])
def test_leaflets(cases, method, frequency):
    case = cases["ua70"]
    system = ua(70, leaflets=method, frequency=frequency, radius=2.0)
    np.testing.assert_array_equal(system.base, case.system.base)
    flags = oracle_flags(system.tables, case.xyz, case.box)
    assert 0 < int(flags.sum()) < flags.size
    edges = structure.order_edges(16)
    groups = type_groups(system.tables)
    plain = run_plain(case, tables=dataclasses.replace(system.tables, flags=0)).finish()
    collect = HipEngine(system.tables)
    collect.set_collect(COLLECT_LEAFLETS)
    collect.set_order_histogram(edges)
    for eng in (run_hist(case, edges, CUTS["three"], tables=system.tables), submit(collect, case, CUTS["three"])):
        got = assert_hist(eng, case, edges, flags)
        np.testing.assert_array_equal(got[:, 1] + got[:, 2], got[:, 0])
        assert got[:, 1].sum() > 0 and got[:, 2].sum() > 0
        np.testing.assert_array_equal(got.sum(axis=0), plain.counts)
        np.testing.assert_array_equal(eng.finish().sums, plain.sums)
    rows, frames = collect.collected_leaflets()
    np.testing.assert_array_equal(frames, FRAMES[::frequency])
    np.testing.assert_array_equal(rows, flags[::frequency])
    # the rows do not depend on leaflets; collected leaflets next to them are the oracle's flags
    both = HipEngine(system.tables)
    both.set_collect(COLLECT_LEAFLETS)
    both.set_molecule_rows(groups)
    submit(both, case, CUTS["three"])
    assert_rows(both, case, groups)
    np.testing.assert_array_equal(both.finish().sums, plain.sums)
    rows, frames = both.collected_leaflets()
    np.testing.assert_array_equal(frames, FRAMES[::frequency])
    np.testing.assert_array_equal(rows, flags[::frequency])


# ---- 5. literal cosine -----------------------------------------------------------------------------------------------------------
def test_literal_cosine(cases):
    system = ua(17)
    system.tables.flags = FLAG_TRIG_ACOS_COS | FLAG_UA_SAMPLES
    case = make_case(system, trig=oracle.TRIG_MIRROR)
    assert (cases["ua17"].samples.tick != case.samples.tick).any()       # the two cosine modes do differ on these frames
    edges, _ = data_edges(case.samples)
    for e in (edges, structure.tilt_edges(90)[0]):
        assert_hist(run_hist(case, e, CUTS["three"]), case, e)
    for groups in (type_groups(case.tables), split_groups(case.tables)):
        assert_rows(run_rows(case, groups, CUTS["three"]), case, groups)


# ---- 6. no periodic boundaries, a general static normal ---------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{"handle_pbc": False}, {"normal": (0.3, -0.2, 0.9)}], ids=["no_pbc", "general_normal"])
def test_no_pbc_and_general_normal(cases, kw):
    case = make_case(ua(6, **kw))
    assert (case.box is None) == ("handle_pbc" in kw)
    if "normal" in kw:                    # (none of the six lipids straddles a face: without the box the ticks are the same)
        assert (cases["ua6"].samples.tick != case.samples.tick).any()
    edges, _ = data_edges(case.samples)
    for e in (edges, structure.order_edges(16)):
        assert_hist(run_hist(case, e, CUTS["three"]), case, e)
    for groups in (type_groups(case.tables), split_groups(case.tables)):
        assert_rows(run_rows(case, groups, CUTS["three"]), case, groups)


# ---- 7. a geometry selection (histogram) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lds", "direct"])
@pytest.mark.parametrize("invert", [False, True])
def test_cylinder_selection(monkeypatch, built, invert, route):
    if route == "direct":
        monkeypatch.setenv("GORDER_HIP_DIST_DIRECT", "1")
    system = ua(17)
    system.tables.geometry = Geometry(kind=abi.GEOM_CYLINDER, invert=invert, reference=abi.GEOMREF_BOX_CENTER, orientation=2, radius=3.0,
                                      structure_box=tuple(float(x) for x in system.box))
    case = make_case(system)
    inside = int(case.samples.present.sum())
    assert 0.1 * case.samples.present.size <= inside <= 0.9 * case.samples.present.size
    edges = structure.tilt_edges(90)[0]
    eng = run_hist(case, edges, CUTS["three"])
    got = assert_hist(eng, case, edges)
    assert int(got[:, 0].sum()) == inside                                # a sample outside the selection is in no bin
    plain = run_plain(case, tables=dataclasses.replace(system.tables, flags=0)).finish()
    np.testing.assert_array_equal(eng.finish().sums, plain.sums)
    np.testing.assert_array_equal(got.sum(axis=0), plain.counts)


# ---- 8. from a file decoded on the device -----------------------------------------------------------------------------------
def test_from_a_file_decoded_on_the_device(cases, tmp_path):
    case = cases["ua17"]
    path = str(tmp_path / "ua17.xtc")
    xtc.write_trajectory(path, case.xyz, case.box.reshape(N, 3, 3), precision=1000.0)
    decoded = xtc.read_trajectory([path])[0]
    ref = make_case(case.system, xyz=decoded)
    edges = structure.tilt_edges(90)[0]
    groups = type_groups(case.tables)
    hist, rows = HipEngine(case.tables), HipEngine(case.tables)
    hist.set_order_histogram(edges)
    rows.set_molecule_rows(groups)
    for eng in (hist, rows):
        stats = eng.run_trajectory([path], threads=2, batch_frames=4, first_frame_index=100, device_decode=True)
        assert stats["n_frames"] == N and stats["device_decode"] == 1
    assert_hist(hist, ref, edges)
    assert_rows(rows, ref, groups)
    host_hist, host_rows = run_hist(ref, edges), run_rows(ref, groups)
    np.testing.assert_array_equal(hist.order_histogram(), host_hist.order_histogram())
    np.testing.assert_array_equal(hist.finish().sums, host_hist.finish().sums)
    for x, y in zip(rows.molecule_rows(), host_rows.molecule_rows()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(rows.finish().sums, host_rows.finish().sums)


# ---- 9. reset ---------------------------------------------------------------------------------------------------------------------
def test_reset_zeroes_counts_and_rows_and_keeps_edges_and_groups(cases):
    case = cases["ua17"]
    edges = structure.order_edges(16)
    groups = split_groups(case.tables)
    hist, rows = run_hist(case, edges, CUTS["three"]), run_rows(case, groups, CUTS["three"])
    first = assert_hist(hist, case, edges)
    assert_rows(rows, case, groups)
    hist.reset()
    rows.reset()
    zero = hist.order_histogram()
    assert zero.shape == first.shape and not zero.any()
    assert rows.molecule_rows_count() == 0 and rows.molecule_rows()[0].shape == (0, len(groups), 17)
    submit(hist, case, CUTS["one"])
    submit(rows, case, CUTS["one"])
    np.testing.assert_array_equal(hist.order_histogram(), first)
    assert_rows(rows, case, groups)
    # half a run: the counts of a handle grow batch by batch
    hist.reset()
    hist.submit_host(case.xyz[:4], case.box[:4], FRAMES[:4])
    np.testing.assert_array_equal(hist.order_histogram(), want_hist(case.samples, edges, None, case.n_acc, slice(0, 4)))


# ---- 10. errors are unchanged -------------------------------------------------------------------------------------------------
def test_errors_are_unchanged(built):
    system = ua(17)
    xyz, box = system.frames(N, seed=5), system.box9(N)
    xyz[4, 52 * 7 + 19] = np.nan                                         # a helper atom of lipid 7's carbons 18 and 20
    groups = type_groups(system.tables)
    seen = []
    for feature in ("plain", "hist", "rows"):
        eng = HipEngine(dataclasses.replace(system.tables, flags=0) if feature == "plain" else system.tables)
        if feature == "hist":
            eng.set_order_histogram(structure.order_edges(16))
        if feature == "rows":
            eng.set_molecule_rows(groups)
        with pytest.raises(abi.GorderHipError) as e:
            for a, b in CUTS["three"]:
                eng.submit_host(xyz[a:b], box[a:b], FRAMES[a:b])
            eng.finish()
        seen.append((e.value.status, e.value.index, e.value.frame))
        if feature == "hist":
            with pytest.raises(abi.GorderHipError) as e:
                eng.order_histogram()
            assert e.value.status == seen[0][0]
    assert seen[0] == seen[1] == seen[2] and seen[0][0] == abi.ERR_UNDEFINED_POSITION and seen[0][2] == 104


# ---- 11. refusals ---------------------------------------------------------------------------------------------------------------
def refused(tables, call, before=None):
    eng = HipEngine(tables)
    if before:
        before(eng)
    with pytest.raises(abi.GorderHipError) as e:
        call(eng)
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
    return str(e.value)


def test_refusals(built):
    set_hist = lambda e: e.set_order_histogram(structure.order_edges(16))
    set_rows = lambda e: e.set_molecule_rows([[0, 1], [2]])
    setters = (set_hist, set_rows)
    # without the flag: the pinned behaviour
    for call in setters:
        assert "united-atom" in refused(synthetic.ua_membrane(24).tables, call)
    # with the flag
    fast = ua(24)
    fast.tables.flags = FLAG_UA_SAMPLES | FLAG_UA_FAST_NORMALISE
    om = OrderMap(enabled=True, plane=0, span_x=(0.0, 4.0), span_y=(0.0, 4.0), bin=(0.4, 0.4))
    dyn = ua(24, leaflets=LEAFLETS_GLOBAL)
    mt = dyn.tables.molecule_types[0]
    dyn.tables.dynamic_normal = abi.DynamicNormal(enabled=True, radius=2.0, cloud=np.asarray(mt.heads))
    mt.normal_heads = mt.heads
    shells = ua(24)
    shells.tables.geometry = Geometry(kind=abi.GEOM_CYLINDER, reference=abi.GEOMREF_BOX_CENTER, orientation=2, radius=2.0,
                                      structure_box=tuple(float(x) for x in shells.box))
    for call in setters:
        assert "fast" in refused(fast.tables, call)
        assert "ordermaps" in refused(ua(24, ordermap=om).tables, call)
        assert "timewise" in refused(ua(24, timewise=True).tables, call)
        assert "dynamic" in refused(dyn.tables, call)
    # radial shells, bond correlation and neighbour classes still answer united-atom, with or without the flag
    for flags in (0, FLAG_UA_SAMPLES):
        t = dataclasses.replace(shells.tables, flags=flags)
        assert "united-atom" in refused(t, lambda e: e.set_radial_shells([1.0, 2.0]))
        assert "united-atom" in refused(t, lambda e: e.set_bond_correlation([0, 1, 2]))
        lf = dataclasses.replace(dyn.tables, flags=flags, dynamic_normal=abi.DynamicNormal())
        assert "united-atom" in refused(lf, lambda e: e.set_neighbour_classes(structure.neighbour_centres(lf), np.arange(0, 24 * 52, 52), 1.0, 3))
    # the rows still refuse a geometry selection; the two features still exclude each other
    assert "geometry" in refused(shells.tables, set_rows)
    t = ua(24).tables
    assert "molecule rows" in refused(t, set_hist, before=set_rows)
    assert "order histogram" in refused(t, set_rows, before=set_hist)
    assert "a slot is in two groups" in refused(t, lambda e: e.set_molecule_rows([[0, 1], [1]]))
    assert "ascending" in refused(t, lambda e: e.set_order_histogram([0, 5, 5, 9]))
