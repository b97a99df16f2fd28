"""Bond reorientation (gorder_hip_set_bond_correlation, k_bond_units + k_bond_corr) on the device.

The reference for every integer is the existing oracle on PER-SAMPLE tables: every bond sample its own molecule type with one
molecule and one bond, timewise rows on, no leaflets, TRIG_DIRECT.  A P2 of a bond against its own earlier vector is a P2
against a per-molecule manual normal, and the oracle uses supplied normals as given (gorder_oracle_set_normals copies them,
calc_sch takes dot3(n, n) of them: nothing is normalised).  For one lag the oracle is handed the numpy-f32 bond vectors of
frames 0 .. F - lag - 1 as normals and frames lag .. F - 1 as the batch: row [f, 0, sample] of its timewise() is that pair's
tick.  The vectors are p2 - p1 in float32 with the literal minimum image, the same IEEE operations as the device's.  The
leaflet planes mask by the flags of the UNSPLIT oracle in the LATER frame, taken frame by frame with OracleEngine.leaflets().
Every comparison is integer equality.

Systems, 13 frames each: the coarse-grained membrane of 40 lipids in two molecule types (440 samples: one full and one partial
tile, a lipid split across them) with global leaflets and periodic boundaries, and the all-atom membrane of 12 lipids (768
samples, three tiles) without leaflets, with periodic boundaries and without."""
import dataclasses

import numpy as np
import pytest

from gorder_amd import HipEngine, abi, structure, synthetic
from gorder_amd.abi import FLAG_TRIG_ACOS_COS, LEAFLETS_GLOBAL, LEAFLETS_NONE, Geometry, Leaflets, MolType, Tables
from oracle import oracle

pytestmark = pytest.mark.gpu

N = 13
CUTS = {"one": [(0, N)], "three": [(0, 4), (4, 5), (5, N)], "singles": [(f, f + 1) for f in range(N)]}
LAG_SETS = {"spread": [0, 1, 2, 3, 5, 8, 12, 20],          # lag 20 exceeds the run: zeros
            "nine": list(range(9)),                         # one full group of 8 and a group of one
            "single": [4],
            "mixed": list(range(9)) + [12, 20]}


def frame_labels(n):
    return np.arange(100, 100 + n, dtype=np.uint64)


def sample_table(tables):
    """-> (atoms [n_samples, 2], slot [n_samples], mol [n_samples]) in the order type, molecule, bond."""
    atoms, slots, mols = [], [], []
    slot_t, mol = 0, 0
    for mt in tables.molecule_types:
        bonds = np.asarray(mt.bonds)
        for i in range(mt.n_molecules):
            for b in range(bonds.shape[0]):
                atoms.append(bonds[b, i]); slots.append(slot_t + b); mols.append(mol)
            mol += 1
        slot_t += bonds.shape[0]
    return np.array(atoms, dtype=np.uint32), np.array(slots), np.array(mols)


def bond_vectors(xyz, box, atoms):
    """float32 [frames, samples, 3] and whether the minimum image shifted a component: p2 - p1, then literally
    a = dx > L/2 ? dx - L : dx; b = a < -L/2 ? a + L : a."""
    d = xyz[:, atoms[:, 1]] - xyz[:, atoms[:, 0]]
    assert d.dtype == np.float32
    if box is None:
        return d, np.zeros(d.shape, dtype=bool)
    L = np.stack([box[:, 0, 0], box[:, 1, 1], box[:, 2, 2]], axis=1)[:, None, :].astype(np.float32)
    half = L / np.float32(2.0)
    a = np.where(d > half, d - L, d)
    b = np.where(a < -half, a + L, a)
    assert b.dtype == np.float32 and (np.abs(b) <= half).all()
    return b, b != d


@dataclasses.dataclass
class Case:
    system: object
    xyz: np.ndarray
    box: np.ndarray
    atoms: np.ndarray
    slot: np.ndarray
    mol: np.ndarray
    v: np.ndarray
    shifted: np.ndarray
    flags: np.ndarray
    split: object
    ticks: dict = dataclasses.field(default_factory=dict)

    @property
    def n_acc(self):
        return self.system.tables.n_acc

    @property
    def n_frames(self):
        return len(self.xyz)

    def pair_ticks(self, lag):
        """int64 [F - lag, samples]: row f is the tick of (frame lag + f, frame f), from the oracle; computed once."""
        if lag not in self.ticks:
            F = self.n_frames
            ref = oracle.OracleEngine(self.split, trig=oracle.TRIG_DIRECT)
            ref.set_normals(self.v[:F - lag])
            ref.submit(self.xyz[lag:], None if self.box is None else self.box[lag:], frame_labels(F)[lag:])
            s, c = ref.timewise(F - lag)
            assert (c[:, 0] == 1).all() and s.shape[2] == len(self.atoms)
            self.ticks[lag] = s[:, 0].astype(np.int64)
            self.ticks[lag].setflags(write=False)
        return self.ticks[lag]

    def want(self, lags):
        F = self.n_frames
        sums = np.zeros((len(lags), 3, self.n_acc), dtype=np.int64)
        counts = np.zeros((len(lags), 3, self.n_acc), dtype=np.uint64)
        for k, lag in enumerate(lags):
            if lag >= F:
                continue
            t = self.pair_ticks(lag)
            np.add.at(sums[k, 0], self.slot, t.sum(axis=0))
            np.add.at(counts[k, 0], self.slot, np.uint64(F - lag))
            if self.flags is not None:
                upper = self.flags[lag:][:, self.mol] == 0                  # the leaflet of the LATER frame
                np.add.at(sums[k, 1], self.slot, (t * upper).sum(axis=0))
                np.add.at(counts[k, 1], self.slot, upper.sum(axis=0).astype(np.uint64))
                sums[k, 2] = sums[k, 0] - sums[k, 1]
                counts[k, 2] = counts[k, 0] - counts[k, 1]
        return sums, counts


def oracle_flags(tables, xyz, box):
    if tables.leaflets.method == LEAFLETS_NONE:
        return None
    ref = oracle.OracleEngine(tables, trig=oracle.TRIG_DIRECT)
    labels = frame_labels(len(xyz))
    rows = []
    for f in range(len(xyz)):
        ref.submit(xyz[f:f + 1], None if box is None else box[f:f + 1], labels[f:f + 1])
        rows.append(ref.leaflets()[0].copy())
    return np.array(rows)


def make_case(system, n=N, seed=5):
    tables = system.tables
    xyz = system.frames(n, seed=seed)
    box = system.box9(n) if tables.handle_pbc else None
    atoms, slot, mol = sample_table(tables)
    v, shifted = bond_vectors(xyz, box, atoms)
    mts = [MolType(n_molecules=1, bonds=a.reshape(1, 1, 2)) for a in atoms]
    split = dataclasses.replace(tables, molecule_types=mts, leaflets=Leaflets(), timewise=True, flags=0)
    for a in (xyz, v):
        a.setflags(write=False)
    return Case(system, xyz, box, atoms, slot, mol, v, shifted, oracle_flags(tables, xyz, box), split)


def cg(**kw):
    return synthetic.cg_membrane(40, n_types=2, **{"leaflets": LEAFLETS_GLOBAL, **kw})


@pytest.fixture(scope="module")
def cases(built):
    return {"cg": make_case(cg()), "aa": make_case(synthetic.aa_membrane(12)),
            "aa_nopbc": make_case(synthetic.aa_membrane(12, handle_pbc=False)), "cg70": make_case(cg(), n=70)}


def run(case, lags, cuts=None, engine=None, device=False, tables=None):
    eng = engine or HipEngine(tables or case.system.tables)
    if engine is None and lags is not None:
        eng.set_bond_correlation(lags)
    labels = frame_labels(case.n_frames)
    for a, b in cuts or [(0, case.n_frames)]:
        if device:
            import torch
            d_xyz = torch.from_numpy(np.array(case.xyz[a:b])).cuda()
            d_box = None if case.box is None else torch.from_numpy(np.array(case.box[a:b])).cuda()
            eng.submit_device(d_xyz, d_box, labels[a:b])
            eng.synchronize()               # (the tensors go out of scope behind this)
        else:
            eng.submit_host(case.xyz[a:b], None if case.box is None else case.box[a:b], labels[a:b])
    return eng


def assert_corr(eng, case, lags):
    sums, counts = eng.bond_correlation()
    want_s, want_c = case.want(lags)
    assert sums.dtype == np.int64 and counts.dtype == np.uint64 and sums.shape == counts.shape == want_s.shape
    np.testing.assert_array_equal(counts, want_c)
    np.testing.assert_array_equal(sums, want_s)
    # the pair count of a lag: max(0, F - lag) x samples of the slot
    per_slot = np.bincount(case.slot, minlength=case.n_acc)
    for k, lag in enumerate(lags):
        np.testing.assert_array_equal(counts[k, 0], max(0, case.n_frames - lag) * per_slot)
    return sums, counts


# ---- 1. every lag set against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("lag_set", ["spread", "nine", "single"])
@pytest.mark.parametrize("name", ["cg", "aa", "aa_nopbc"])
def test_lags_against_the_oracle(cases, name, lag_set):
    case, lags = cases[name], LAG_SETS[lag_set]
    assert case.system.tables.n_samples_per_frame == len(case.atoms) == (440 if name == "cg" else 768)
    if name == "cg":
        assert case.shifted.any(axis=(1, 2)).any()                       # a frame in which the minimum image moved a bond
        assert 0 < int(case.flags.sum()) < case.flags.size
    if name == "aa_nopbc":
        assert case.box is None and not case.shifted.any()
    eng = run(case, lags)
    assert eng.plan()["n_tiles"] == (2 if name == "cg" else 3)
    sums, counts = assert_corr(eng, case, lags)
    if 20 in lags:
        k = lags.index(20)
        assert not sums[k].any() and not counts[k].any()
    if case.flags is None:
        assert not sums[:, 1:].any() and not counts[:, 1:].any()
    else:
        assert counts[0, 1].sum() > 0 and counts[0, 2].sum() > 0
    if 0 in lags:                                                        # a vector against itself: S = 1 up to the rounding of q
        assert (np.abs(sums[0, 0] - 1000000 * counts[0, 0].astype(np.int64)) <= counts[0, 0].astype(np.int64)).all()


# ---- 2. cuts into batches, sub-ranges, launch geometry, the device route ---------------------------------------------------
@pytest.mark.parametrize("variant", ["three", "singles", "subrange3", "subrange3_three", "wg_target1", "device", "device_three", "chunk_major",
                                     "chunk_major_three"])
@pytest.mark.parametrize("name", ["cg", "aa"])
def test_cuts_and_switches_give_the_same_integers(cases, monkeypatch, name, variant):
    case, lags = cases[name], LAG_SETS["mixed"]
    if variant.startswith("subrange3"):
        monkeypatch.setenv("GORDER_HIP_CORR_SUBRANGE", "3")
    if variant == "wg_target1":
        monkeypatch.setenv("GORDER_HIP_WG_TARGET", "1")
    if variant.startswith("chunk_major"):
        monkeypatch.setenv("GORDER_HIP_CORR_GRID", "chunks")             # a workgroup walks every group of lags of its chunk
    cuts = CUTS["three"] if variant.endswith("three") else CUTS.get(variant, CUTS["one"])
    eng = run(case, lags, cuts, device=variant.startswith("device"))
    got = assert_corr(eng, case, lags)
    monkeypatch.undo()
    one = run(case, lags).bond_correlation()
    np.testing.assert_array_equal(got[0], one[0])
    np.testing.assert_array_equal(got[1], one[1])


def test_64_lags_over_70_frames(cases, monkeypatch):
    case, lags = cases["cg70"], list(range(64))
    first = assert_corr(run(case, lags), case, lags)
    # batches shorter than the largest lag, sub-ranges shorter than the batches: the history spans many of both
    monkeypatch.setenv("GORDER_HIP_CORR_SUBRANGE", "7")
    again = run(case, lags, [(0, 30), (30, 31), (31, 70)]).bond_correlation()
    np.testing.assert_array_equal(again[0], first[0])
    np.testing.assert_array_equal(again[1], first[1])
    monkeypatch.undo()
    monkeypatch.setenv("GORDER_HIP_CORR_GRID", "chunks")                 # two chunks of frames, eight groups of lags in one workgroup
    other = run(case, lags).bond_correlation()
    np.testing.assert_array_equal(other[0], first[0])
    np.testing.assert_array_equal(other[1], first[1])


# ---- 3. the ordinary results are untouched ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cg", "aa"])
def test_finish_is_untouched(cases, name):
    case, lags = cases[name], LAG_SETS["mixed"]
    eng, plain = HipEngine(case.system.tables), HipEngine(case.system.tables)
    eng.set_bond_correlation(lags)
    for e in (eng, plain):
        e.kernel_time()                   # switches the timing on
        run(case, None, CUTS["three"], engine=e)
    got, want = eng.finish(), plain.finish()
    for e in (eng, plain):
        e.kernel_time()
    assert "k_bond_corr" in eng.kernel_names() and "k_bond_units" in eng.kernel_names()
    assert "k_bond_corr" not in plain.kernel_names() and "k_bond_units" not in plain.kernel_names()
    np.testing.assert_array_equal(got.sums, want.sums)
    np.testing.assert_array_equal(got.counts, want.counts)
    assert got.n_frames == want.n_frames == N and want.counts[0].min() > 0
    assert_corr(eng, case, lags)
    s, c = plain.bond_correlation()
    assert s.shape == c.shape == (0, 3, case.n_acc)


def test_timewise_on_the_same_handle(cases):
    case, lags = cases["cg"], LAG_SETS["nine"]
    tables = cg(timewise=True).tables
    eng = run(case, lags, CUTS["three"], tables=tables)
    plain = run(case, None, CUTS["three"], engine=HipEngine(tables))
    for a, b in zip(eng.timewise(N), plain.timewise(N)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(eng.finish().sums, plain.finish().sums)
    assert_corr(eng, case, lags)


def test_the_literal_cosine_flag_does_not_reach_the_correlation(cases):
    case, lags = cases["cg"], LAG_SETS["nine"]
    tables = cg().tables
    tables.flags = FLAG_TRIG_ACOS_COS
    eng = run(case, lags, CUTS["three"], tables=tables)
    assert_corr(eng, case, lags)
    plain = run(case, None, CUTS["three"], engine=HipEngine(tables))
    np.testing.assert_array_equal(eng.finish().sums, plain.finish().sums)


# ---- 4. reset ---------------------------------------------------------------------------------------------------------------
def test_reset_forgets_the_history_and_keeps_the_lags(cases):
    case, lags = cases["cg"], LAG_SETS["mixed"]
    eng = run(case, lags, CUTS["three"])
    first = assert_corr(eng, case, lags)
    eng.reset()
    zero = eng.bond_correlation()
    assert zero[0].shape == first[0].shape and not zero[0].any() and not zero[1].any()
    run(case, None, CUTS["singles"], engine=eng)
    again = eng.bond_correlation()
    np.testing.assert_array_equal(again[0], first[0])
    np.testing.assert_array_equal(again[1], first[1])


# ---- 5. a known answer that owes nothing to the oracle ---------------------------------------------------------------------
def test_axis_swapping_bonds_by_hand(built):
    d = np.float32(0.3)
    schedule = np.array([0, 0, 1, 2, 2, 0, 1, 1, 2, 0, 0, 1])             # bond b points along axis (b + schedule[f]) % 3
    F = len(schedule)
    tables = Tables(n_atoms=6, molecule_types=[MolType(n_molecules=1, bonds=np.array([[[0, 1]], [[2, 3]], [[4, 5]]], dtype=np.uint32))],
                    handle_pbc=False)
    xyz = np.zeros((F, 6, 3), dtype=np.float32)
    axis = (np.arange(3)[None, :] + schedule[:, None]) % 3                # [F, bond]
    # the first atom sits at 0 on the bond's axis, the second at d there and at the first atom's place elsewhere: p2 - p1 is exact
    for f in range(F):
        for b in range(3):
            xyz[f, 2 * b] = xyz[f, 2 * b + 1] = (1.0 + b, 2.0, 3.0)
            xyz[f, 2 * b, axis[f, b]] = 0.0
            xyz[f, 2 * b + 1, axis[f, b]] = d
    v = xyz[:, 1::2] - xyz[:, 0::2]
    for f in range(F):
        for b in range(3):
            want_v = np.zeros(3, dtype=np.float32); want_v[axis[f, b]] = d
            np.testing.assert_array_equal(v[f, b], want_v)
    lags = [0, 1, 2, 3, 5, 7]
    eng = HipEngine(tables)
    eng.set_bond_correlation(lags)
    eng.submit_host(xyz[:5], None, np.arange(5))
    eng.submit_host(xyz[5:], None, np.arange(5, F))
    sums, counts = eng.bond_correlation()
    seen_orthogonal = 0
    for k, lag in enumerate(lags):
        for b in range(3):
            parallel = int((axis[lag:, b] == axis[:F - lag, b]).sum())
            orthogonal = (F - lag) - parallel
            seen_orthogonal += orthogonal
            assert int(counts[k, 0, b]) == F - lag
            hand = 1000000 * parallel - 500000 * orthogonal              # P2 = 1 or -0.5
            assert abs(int(sums[k, 0, b]) - hand) <= parallel, (lag, b)  # a parallel tick is within one of 10^6
            if parallel == 0:
                assert int(sums[k, 0, b]) == hand                        # an orthogonal pair is -500 000 exactly
    assert seen_orthogonal > 0 and not sums[:, 1:].any() and not counts[:, 1:].any()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def refused(tables, lags=(0, 1, 2), before=None):
    eng = HipEngine(tables)
    if before:
        before(eng)
    with pytest.raises(abi.GorderHipError) as e:
        eng.set_bond_correlation(lags)
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
    return str(e.value)


def test_refusals(cases):
    assert "united-atom" in refused(synthetic.ua_membrane(24).tables)
    geom = cg()
    geom.tables.geometry = Geometry(kind=abi.GEOM_CYLINDER, reference=abi.GEOMREF_BOX_CENTER, orientation=2, radius=1.4,
                                    structure_box=tuple(float(x) for x in geom.box))
    assert "geometry selection" in refused(geom.tables)
    wide = synthetic.cg_membrane(200, leaflets=LEAFLETS_GLOBAL, n_types=2)
    b = np.asarray(wide.tables.molecule_types[0].bonds).copy()
    b[0, 0] = (0, 12 * 199 + 11)                                       # 2400 atoms apart: more than the 1024-atom window
    wide.tables.molecule_types[0].bonds = b
    assert "LDS window" in refused(wide.tables)
    none = cg()
    for m in none.tables.molecule_types:
        m.bonds = np.asarray(m.bonds)[:0]
    assert "no bond samples" in refused(none.tables)
    # the lags themselves
    t = cg().tables
    assert "GORDER_CORR_MAX_LAGS" in refused(t, np.arange(65))
    assert "ascending" in refused(t, [0, 5, 5, 9])
    assert "ascending" in refused(t, [0, 5, 4, 9])
    assert "GORDER_CORR_MAX_LAG" in refused(t, [0, 4097])
    HipEngine(t).set_bond_correlation([0, 4096])                        # the largest lag is allowed
    HipEngine(t).set_bond_correlation(np.arange(64))                    # ... and the longest list
    with pytest.raises(ValueError):
        HipEngine(t).set_bond_correlation([0.5, 1.5])
    with pytest.raises(ValueError):
        HipEngine(t).set_bond_correlation([-1, 2])
    # a ring over budget: 3 072 lipids are 132 tiles, 540 672 bytes a plane, 4 097 planes pass 2 GiB
    big = synthetic.cg_membrane(3072).tables
    why = refused(big, [0, 4096])
    assert "over budget" in why and "540672" in why and str(4097 * 540672) in why
    HipEngine(big).set_bond_correlation([0, 3000])
    # after the first submit; reset opens the setter again; an empty list switches the correlation off
    case = cases["cg"]
    eng = HipEngine(case.system.tables)
    labels = frame_labels(N)
    eng.submit_host(case.xyz[:1], case.box[:1], labels[:1])
    with pytest.raises(abi.GorderHipError) as e:
        eng.set_bond_correlation([0, 1])
    assert e.value.status == abi.ERR_INVALID_ARGUMENT and "first submit" in str(e.value)
    eng.reset()
    eng.set_bond_correlation([0, 1])
    eng.reset()
    eng.set_bond_correlation([])
    eng.submit_host(case.xyz, case.box, labels)
    assert eng.bond_correlation()[0].shape == (0, 3, case.n_acc)
    plain = HipEngine(case.system.tables)
    plain.submit_host(case.xyz, case.box, labels)
    np.testing.assert_array_equal(eng.finish().sums, plain.finish().sums)
