"""Order by local composition (gorder_hip_set_neighbour_classes, k_neighbour_counts + k_bonds_classes) on the device.

Expected values.  The tick of every sample comes from the existing oracle on SPLIT tables: every molecule its own molecule
type, no leaflets, timewise rows on — row [f, 0, slot(type, molecule, bond)] of its timewise() is then the single tick of that
sample (the split_tables / oracle_samples of tests/test_order_histogram_gpu.py, restated here).  The leaflet planes use the
flags of the UNSPLIT oracle, taken frame by frame.  The expected class of every (frame, molecule) is a numpy float32
restatement of the device's arithmetic: d = x_q - x_c per component, the minimum image where(|d| > L/2, d - copysign(L, d), d),
d2 = (dx dx + dy dy) + dz dz (boundary_probes.dist2_space's order), counted where d2 < boundary_probes.radius_threshold(radius),
the centre atom itself skipped, the class min(count, n_classes - 1).  neighbour_class_rows() is compared with these classes and
neighbour_classes() with the ticks binned by them.  Every comparison is integer equality.

No pair of the systems below lies within 16 float32 places of its threshold (asserted: a condition on the inputs, not a
tolerance), so no comparison rests on a tie — except in test_ties, whose radii are fitted so that a real pair's d2 IS the
threshold (not counted) or the float below it (counted)."""
import dataclasses

import numpy as np
import pytest

from gorder_amd import HipEngine, abi, structure, synthetic, xtc
from gorder_amd.abi import FLAG_TRIG_ACOS_COS, LEAFLETS_GLOBAL, LEAFLETS_LOCAL, LEAFLETS_NONE, Geometry, Leaflets, MolType, OrderMap
from oracle import oracle
import boundary_probes as bp

pytestmark = pytest.mark.gpu

F32 = np.float32
N = 11                                   # two full stages of four frames and a tail of three
FRAMES = np.arange(100, 100 + N, dtype=np.uint64)
CUTS = {"one": [(0, N)], "three": [(0, 4), (4, 5), (5, N)]}


# ---- the oracle's ticks and flags (tests/test_order_histogram_gpu.py) --------------------------------------------------------
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
    return dataclasses.replace(tables, molecule_types=mts, leaflets=Leaflets(), timewise=True, flags=0), slot0


@dataclasses.dataclass
class Samples:
    tick: np.ndarray        # int64 [frames, samples]
    slot: np.ndarray        # [samples] accumulator slot of the unsplit tables
    mol: np.ndarray         # [samples] molecule (molecule-type-major, as the leaflet flags)


def oracle_samples(tables, xyz, box, trig, n_threads=1):
    split, slot0 = split_tables(tables)
    ref = oracle.OracleEngine(split, trig=trig, n_threads=n_threads)
    ref.submit(xyz, box, FRAMES[:len(xyz)])
    tw_s, tw_c = ref.timewise(len(xyz))
    assert int(tw_c[:, 0].max()) == 1 == int(tw_c[:, 0].min())         # a slot of the split tables is one sample, every frame
    cols, slots, mols = [], [], []
    slot_t, mol = 0, 0
    for t, mt in enumerate(tables.molecule_types):
        for i in range(mt.n_molecules):
            for b in range(mt.n_bond_types):
                cols.append(slot0[t][i] + b); slots.append(slot_t + b); mols.append(mol)
            mol += 1
        slot_t += mt.n_bond_types
    return Samples(tw_s[:, 0, cols].astype(np.int64), np.array(slots), np.array(mols))


def oracle_flags(tables, xyz, box):
    """uint8 [frames, molecules]: the side (Upper = 0) every frame's samples are booked on, or None without leaflets."""
    if tables.leaflets.method == LEAFLETS_NONE:
        return None
    ref = oracle.OracleEngine(tables, trig=oracle.TRIG_DIRECT)
    rows = []
    for f in range(len(xyz)):
        ref.submit(xyz[f:f + 1], None if box is None else box[f:f + 1], FRAMES[f:f + 1])
        rows.append(ref.leaflets()[0].copy())
    return np.array(rows)


# ---- the classes, restated in numpy float32 ----------------------------------------------------------------------------------
def min_image_loops(d, L, half):
    """The literal loops (gm_min_image_loop), vectorised: up to nine shifts down, then up to nine up, in float32."""
    for _ in range(9):
        d = np.where(d > half, d - L, d).astype(F32)
    for _ in range(9):
        d = np.where(d < -half, d + L, d).astype(F32)
    assert (np.abs(d) <= half).all()                                    # (nobody is so far out that the loops give up)
    return d


def pair_d2(xyz, box, centres, neighbours, far=False):
    """float32 [frames, molecules, neighbours]: d2 of every pair in the device's operation order.  far: some pairs are more
    than 1.5 box lengths apart in a component — the device then sends all three components of THAT pair through the loops."""
    xyz = np.asarray(xyz, dtype=F32)
    d = xyz[:, None, neighbours, :] - xyz[:, centres, None, :]          # x_q - x_c, float32
    assert d.dtype == F32
    if box is not None:
        L = np.asarray(box, dtype=F32).reshape(len(xyz), 3, 3)[:, [0, 1, 2], [0, 1, 2]][:, None, None, :]
        half = L / F32(2.0)
        select = np.where(np.abs(d) > half, d - np.copysign(L, d), d).astype(F32)
        slow = (np.abs(select) > half).any(axis=-1, keepdims=True)
        if far:
            loops = min_image_loops(d, L, half)
            assert slow.any() and (loops.view(np.uint32) == select.view(np.uint32))[np.broadcast_to(~slow, d.shape)].all()
            d = np.where(slow, loops, select).astype(F32)
        else:
            assert not slow.any()                                       # one shift was enough: the select form is the whole function
            d = select
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == F32
    return d2


def places(a, b):
    """How many float32 lie between the non-negative floats a and b."""
    return np.abs(np.asarray(a, dtype=F32).view(np.int32).astype(np.int64) - np.asarray(b, dtype=F32).view(np.int32).astype(np.int64))


def neighbour_counts(d2, thr, centres, neighbours, rule="<"):
    other = np.asarray(centres)[:, None] != np.asarray(neighbours)[None, :]
    inside = (d2 < thr) if rule == "<" else (d2 <= thr)
    return (inside & other[None]).sum(axis=2)


def want_classes(samples, classes, flags, n_classes, n_acc, frames=slice(None)):
    """(sums int64, counts uint64) [n_classes, 3, n_acc] from the oracle's ticks, with numpy integers."""
    tick = samples.tick[frames]
    cls = classes[frames][:, samples.mol].astype(np.int64)
    slot = np.broadcast_to(samples.slot, tick.shape)
    sums = np.zeros((n_classes, 3, n_acc), dtype=np.int64)
    counts = np.zeros((n_classes, 3, n_acc), dtype=np.uint64)
    planes = [(0, np.ones(tick.shape, dtype=bool))]
    if flags is not None:
        upper = flags[frames][:, samples.mol] == 0
        planes += [(1, upper), (2, ~upper)]
    for w, ok in planes:
        np.add.at(sums[:, w], (cls[ok], slot[ok]), tick[ok])
        np.add.at(counts[:, w], (cls[ok], slot[ok]), 1)
    return sums, counts


@dataclasses.dataclass
class Case:
    system: object
    xyz: np.ndarray
    box: np.ndarray
    samples: Samples
    flags: np.ndarray
    centres: np.ndarray
    neighbours: np.ndarray
    radius: float
    d2: np.ndarray = None
    counts: np.ndarray = None       # [frames, molecules]
    far: bool = False               # pair_d2's
    ties_allowed: bool = False      # millions of pairs: some lie next to the threshold (test_ties pins the rule there)

    def __post_init__(self):
        self.thr = bp.radius_threshold(self.radius)
        assert self.thr == abi.radial_thresholds([self.radius])[0]
        self.d2 = pair_d2(self.xyz, self.box, self.centres, self.neighbours, self.far)
        f, m, q = 0, len(self.centres) - 1, 0
        d = self.xyz[f, self.neighbours[q]] - self.xyz[f, self.centres[m]]
        if self.box is None:                                             # the vectorised order is dist2_space's
            assert self.d2[f, m, q] == bp.dist2_space(*d)
        self.counts = neighbour_counts(self.d2, self.thr, self.centres, self.neighbours)
        other = self.centres[:, None] != self.neighbours[None, :]
        self.nearest = int(places(self.d2, self.thr)[:, other].min())
        assert self.nearest > 16 or self.ties_allowed                    # no comparison rests on a tie

    @property
    def n_acc(self):
        return self.system.tables.n_acc

    def classes(self, n_classes):
        return np.minimum(self.counts, n_classes - 1).astype(np.uint8)


def make_case(system, centres, neighbours, radius, trig=oracle.TRIG_DIRECT, n_frames=N, seed=5, xyz=None, n_threads=1, **kw):
    xyz = system.frames(n_frames, seed=seed) if xyz is None else xyz
    box = system.box9(len(xyz)) if system.tables.handle_pbc else None
    return Case(system, xyz, box, oracle_samples(system.tables, xyz, box, trig, n_threads), oracle_flags(system.tables, xyz, box),
                np.asarray(centres, dtype=np.uint32), np.asarray(neighbours, dtype=np.uint32), radius, **kw)


def cg(**kw):
    return synthetic.cg_membrane(40, n_types=3, **{"leaflets": LEAFLETS_GLOBAL, **kw})


def cg_atoms(system):
    """centres = bead 1 of every lipid (molecule-type-major); neighbours = bead 1 of the lipids of type 1"""
    lipids = np.arange(system.tables.n_atoms // 12)
    centres = np.concatenate([lipids[lipids % 3 == ty] * 12 + 1 for ty in range(3)])
    return centres, np.sort(lipids[lipids % 3 == 1] * 12 + 1)


def cg_case(system=None, **kw):
    system = system or cg()
    centres, neighbours = cg_atoms(system)
    return make_case(system, centres, neighbours, 1.0, **kw)


def aa_case(**kw):
    system = synthetic.aa_membrane(12, **kw)
    first = np.arange(12) * (system.tables.n_atoms // 12)               # centres = neighbours = first atom of every lipid
    return make_case(system, first, first, 3.0)


@pytest.fixture(scope="module")
def cases(built):
    out = {"cg": cg_case(), "aa": aa_case()}
    np.testing.assert_array_equal(out["cg"].centres, structure.neighbour_centres(out["cg"].system.tables))
    assert out["cg"].system.box.tolist() == [4.0, pytest.approx(3.2), 10.0]
    return out


@pytest.fixture(scope="module")
def big(built):
    system = synthetic.cg_membrane(1100, n_types=3, leaflets=LEAFLETS_GLOBAL)
    centres, _ = cg_atoms(system)
    return make_case(system, centres, np.sort(centres), 1.0, n_frames=3)


def run(case, n_classes, cuts=CUTS["one"], tables=None, engine=None, neighbours=None, radius=None, check_rows=True, submit="host"):
    """Submit the case's frames batch by batch; after every batch the class rows of that batch are the expected ones."""
    eng = engine or HipEngine(tables or case.system.tables)
    if engine is None:
        eng.set_neighbour_classes(case.centres, case.neighbours if neighbours is None else neighbours, case.radius if radius is None else radius,
                                  n_classes)
    n = len(case.xyz)
    for a, b in cuts:
        a, b = min(a, n), min(b, n)
        if a == b:
            continue
        box = None if case.box is None else case.box[a:b]
        if submit == "device":
            import torch
            eng.submit_device(torch.from_numpy(case.xyz[a:b]).cuda(), None if box is None else torch.from_numpy(box).cuda(), FRAMES[a:b])
            eng.synchronize()
        else:
            eng.submit_host(case.xyz[a:b], box, FRAMES[a:b])
        if check_rows:
            rows = eng.neighbour_class_rows()
            assert rows.dtype == np.uint8 and rows.shape == (b - a, len(case.centres))
            np.testing.assert_array_equal(rows, case.classes(n_classes)[a:b])
    return eng


def assert_classes(eng, case, n_classes, flags="case", classes=None, frames=slice(None)):
    got = eng.neighbour_classes()
    assert len(got) == n_classes
    sums, counts = want_classes(case.samples, case.classes(n_classes) if classes is None else classes,
                                case.flags if isinstance(flags, str) else flags, n_classes, case.n_acc, frames)
    for k, res in enumerate(got):
        assert res.sums.dtype == np.int64 and res.counts.dtype == np.uint64 and res.sums.shape == (3, case.n_acc)
        np.testing.assert_array_equal(res.counts, counts[k])
        np.testing.assert_array_equal(res.sums, sums[k])
    return np.array([r.sums for r in got]), np.array([r.counts for r in got])


# ---- 0. the inputs are the ones the bounds were written for ------------------------------------------------------------------
def test_inputs(cases):
    cg_, aa = cases["cg"], cases["aa"]
    assert np.bincount(cg_.counts.ravel()).tolist() == [96, 171, 126, 47]
    assert int((cg_.counts[1:] != cg_.counts[:-1]).sum()) == 62         # a lipid does change its class from frame to frame
    assert cg_.nearest == 2468
    assert np.bincount(aa.counts.ravel()).tolist() == [23, 50, 59] and aa.nearest == 15466
    open_ = neighbour_counts(pair_d2(aa.xyz, None, aa.centres, aa.neighbours), aa.thr, aa.centres, aa.neighbours)
    assert np.bincount(open_.ravel()).tolist() == [33, 64, 35]           # the minimum image is exercised


# ---- 1. rows and sums against the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lds", "direct"])
@pytest.mark.parametrize("cuts", list(CUTS))
@pytest.mark.parametrize("name", ["cg", "aa"])
def test_classes_against_the_oracle(cases, monkeypatch, name, cuts, route):
    case = cases[name]
    if route == "direct":
        monkeypatch.setenv("GORDER_HIP_NB_DIRECT", "1")
    for n_classes in (4, 3, 2, 32):                                      # (3: count 3 clamps into class 2)
        eng = run(case, n_classes, CUTS[cuts])
        sums, counts = assert_classes(eng, case, n_classes)
        res = eng.finish()
        np.testing.assert_array_equal(sums.sum(axis=0), res.sums)      # the classes add up to finish()
        np.testing.assert_array_equal(counts.sum(axis=0), res.counts)
        assert res.n_frames == N
        populated = [k for k in range(n_classes) if counts[k, 0].sum()]
        assert populated == list(range(min(n_classes, int(case.counts.max()) + 1)))


@pytest.mark.parametrize("env", [{"GORDER_HIP_NB_SUBRANGE": "3"}, {"GORDER_HIP_WG_TARGET": "1"},
                                 {"GORDER_HIP_NB_SUBRANGE": "3", "GORDER_HIP_NB_DIRECT": "1"}])
def test_sub_ranges_and_launch_geometry(cases, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for name in ("cg", "aa"):
        case = cases[name]
        eng = HipEngine(case.system.tables)
        eng.set_neighbour_classes(case.centres, case.neighbours, case.radius, 4)
        eng.kernel_time()                                                # switches the timing on
        run(case, 4, CUTS["one"], engine=eng)
        assert_classes(eng, case, 4)
        eng.kernel_time()
        segments = {name_: k for name_, _, k in eng.kernel_groups()}
        want = -(-N // 3) if "GORDER_HIP_NB_SUBRANGE" in env else 1
        assert segments["k_neighbour_counts"] == segments["k_bonds_classes"] == want


def test_literal_cosine(cases):
    system = cg()
    system.tables.flags = FLAG_TRIG_ACOS_COS
    case = cg_case(system, trig=oracle.TRIG_MIRROR)
    assert (cases["cg"].samples.tick != case.samples.tick).any()         # the two cosine modes do differ on these frames
    for cuts in CUTS.values():
        assert_classes(run(case, 4, cuts), case, 4)


def test_general_static_normal_and_no_periodic_boundaries(built):
    r = float(np.float32(1.0 / np.sqrt(2.0)))
    case = cg_case(cg(normal=(r, r, 0.0), leaflets=LEAFLETS_NONE, handle_pbc=False))
    assert case.box is None and case.flags is None
    assert_classes(run(case, 4, CUTS["three"]), case, 4)


def test_aa_without_periodic_boundaries(cases):
    system = synthetic.aa_membrane(12, handle_pbc=False)
    pbc = cases["aa"]
    case = make_case(system, pbc.centres, pbc.neighbours, 3.0)
    assert (case.counts != pbc.counts).any()
    assert_classes(run(case, 3), case, 3)


def test_submit_device(cases):
    case = cases["cg"]
    assert_classes(run(case, 4, CUTS["three"], submit="device"), case, 4)


def test_from_a_file_decoded_on_the_device(cases, tmp_path):
    case = cases["cg"]
    path = str(tmp_path / "cg.xtc")
    xtc.write_trajectory(path, case.xyz, case.box.reshape(N, 3, 3), precision=1000.0)
    decoded = xtc.read_trajectory([path])[0]
    ref = make_case(case.system, case.centres, case.neighbours, case.radius, xyz=decoded)
    eng = HipEngine(case.system.tables)
    eng.set_neighbour_classes(case.centres, case.neighbours, case.radius, 4)
    stats = eng.run_trajectory([path], threads=2, batch_frames=4, first_frame_index=100, device_decode=True)
    assert stats["n_frames"] == N and stats["device_decode"] == 1
    assert_classes(eng, ref, 4)
    np.testing.assert_array_equal(eng.neighbour_class_rows(), ref.classes(4)[8:])    # the last batch: frames 8..10
    host = run(ref, 4)
    np.testing.assert_array_equal(eng.finish().sums, host.finish().sums)


# ---- 2. leaflet planes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method, frequency, flip", [(LEAFLETS_GLOBAL, 5, True), (LEAFLETS_LOCAL, 1, False), (LEAFLETS_LOCAL, 5, False)])
def test_leaflet_planes(cases, method, frequency, flip):
    case = cases["cg"]
    system = cg(leaflets=method, frequency=frequency, flip=flip, radius=1.2)
    np.testing.assert_array_equal(system.base, case.system.base)
    flags = oracle_flags(system.tables, case.xyz, case.box)
    assert 0 < int(flags.sum()) < flags.size
    if flip:
        assert (flags[0] != case.flags[0]).all()
    eng = run(case, 4, CUTS["three"], tables=system.tables)
    sums, counts = assert_classes(eng, case, 4, flags)
    np.testing.assert_array_equal(counts[:, 1] + counts[:, 2], counts[:, 0])
    np.testing.assert_array_equal(sums[:, 1] + sums[:, 2], sums[:, 0])
    assert counts[:, 1].sum() > 0 and counts[:, 2].sum() > 0
    plain = HipEngine(system.tables)
    for a, b in CUTS["three"]:
        plain.submit_host(case.xyz[a:b], case.box[a:b], FRAMES[a:b])
    np.testing.assert_array_equal(eng.finish().sums, plain.finish().sums)
    np.testing.assert_array_equal(eng.finish().counts, plain.finish().counts)


def test_without_leaflets_the_planes_are_zero(cases):
    sums, counts = assert_classes(run(cases["aa"], 3), cases["aa"], 3)
    assert counts[:, 0].sum() > 0 and not counts[:, 1:].any() and not sums[:, 1:].any()


# ---- 3. the piece and block edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_neighbours", [1023, 1024, 1025, 1100])
def test_piece_and_block_edges(big, n_neighbours):
    assert len(big.centres) == 1100 == 4 * 256 + 76 and len(big.neighbours) == 1100
    assert int(big.counts.min()) == 2 and int(big.counts.max()) == 7 and big.nearest == 875
    neighbours = big.neighbours[:n_neighbours]
    counts = neighbour_counts(big.d2[:, :, :n_neighbours], big.thr, big.centres, neighbours)
    if n_neighbours < 1100:
        assert (counts != big.counts).any()                              # the atoms left out were somebody's neighbours
    for n_classes in ((4, 3, 2, 32) if n_neighbours == 1100 else (8, 4)):
        classes = np.minimum(counts, n_classes - 1).astype(np.uint8)
        eng = run(big, n_classes, [(0, 3)], neighbours=neighbours, check_rows=False)
        rows = eng.neighbour_class_rows()
        np.testing.assert_array_equal(rows, classes)
        assert (classes[:, 1024:] > 0).sum() >= 3 * 60                   # the molecules past the fourth block have neighbours to count
        assert_classes(eng, big, n_classes, classes=classes)


# ---- 3b. the launch limits: the rows of gridDim.y, the bytes of the class rows (DESIGN: launch limits, rows 18 and 19) -------------
GRID_Y_MAX = 65535              # neighbour_classes.h kClassGridRows: k_neighbour_counts takes a frame per row of gridDim.y
MANY_FRAMES, MANY_TAIL = 65600, 65530


def test_past_the_rows_of_grid_y(built):
    """65 600 frames in one submit: k_neighbour_counts and k_bonds_classes are launched twice (65 535 + 65 frames), the second
    time with frame0 = 65 535 and the rows of the whole batch.  From frame 65 530 on a lipid stands elsewhere, so the second
    launch's classes are not the first's."""
    system = synthetic.cg_membrane(8)
    n = MANY_FRAMES
    assert n > GRID_Y_MAX and MANY_TAIL < GRID_Y_MAX < n - 1
    xyz = system.frames(n, seed=7)
    a = slice(12, 24)                                                    # lipid 1, moved by half a lattice spacing
    xyz[MANY_TAIL:, a, 0] = np.mod(xyz[MANY_TAIL:, a, 0] + F32(0.4), system.box[0]).astype(F32)
    centres = np.arange(8) * 12 + 1
    case = make_case(system, centres, centres, 0.85, xyz=xyz, n_threads=4, ties_allowed=True)
    classes = case.classes(4)
    head, tail = np.bincount(classes[:MANY_TAIL].ravel(), minlength=4) / MANY_TAIL, np.bincount(classes[GRID_Y_MAX:].ravel(), minlength=4) / (n - GRID_Y_MAX)
    assert np.abs(head - tail).max() > 0.1 and (classes[GRID_Y_MAX:] != classes[:n - GRID_Y_MAX]).any()
    eng = HipEngine(system.tables)
    eng.set_neighbour_classes(case.centres, case.neighbours, case.radius, 4)
    eng.kernel_time()
    eng.submit_host(case.xyz, case.box, np.arange(n))
    rows = eng.neighbour_class_rows()
    assert rows.shape == (n, 8)
    for f in (0, GRID_Y_MAX - 1, GRID_Y_MAX, GRID_Y_MAX + 1, n - 1):
        np.testing.assert_array_equal(rows[f], classes[f])
    np.testing.assert_array_equal(rows, classes)
    sums, counts = assert_classes(eng, case, 4)
    res = eng.finish()
    assert res.n_frames == n
    np.testing.assert_array_equal(sums.sum(axis=0), res.sums)
    eng.kernel_time()
    segments = {name: k for name, _, k in eng.kernel_groups()}
    assert segments["k_neighbour_counts"] == segments["k_bonds_classes"] == 2


@pytest.mark.parametrize("cuts", list(CUTS))
def test_class_rows_one_sub_range_at_a_time(cases, monkeypatch, cuts):
    """The class rows are bounded (1 GiB; GORDER_HIP_NB_ROW_BYTES here: three frames of 40 molecules): a batch beyond the bound
    is walked in sub-ranges that reuse the rows — row_base = the sub-range's first frame — and the read-out returns the last."""
    case = cases["cg"]
    monkeypatch.setenv("GORDER_HIP_NB_ROW_BYTES", str(3 * len(case.centres) + 7))
    eng = HipEngine(case.system.tables)
    eng.set_neighbour_classes(case.centres, case.neighbours, case.radius, 4)
    eng.kernel_time()
    launches = 0
    for a, b in CUTS[cuts]:
        eng.submit_host(case.xyz[a:b], case.box[a:b], FRAMES[a:b])
        whole = b - a <= 3
        last = a if whole else a + (b - a - 1) // 3 * 3                  # the first frame of the batch's last sub-range
        np.testing.assert_array_equal(eng.neighbour_class_rows(), case.classes(4)[last:b])
        launches += -(-(b - a) // 3)
    assert_classes(eng, case, 4)
    eng.kernel_time()
    segments = {name: k for name, _, k in eng.kernel_groups()}
    assert segments["k_neighbour_counts"] == segments["k_bonds_classes"] == launches and launches == {"one": 4, "three": 5}[cuts]
    plain = HipEngine(case.system.tables)
    plain.submit_host(case.xyz, case.box, FRAMES)
    np.testing.assert_array_equal(eng.finish().sums, plain.finish().sums)


# ---- 3c. pairs more than 1.5 box lengths apart: the minimum image's loops ---------------------------------------------------------
def test_far_pairs_take_the_loops(cases):
    """A neighbour atom (the centre of its own lipid too) written two box lengths away in x, then in y: its pairs leave the
    select form — |d - copysign(L, d)| > L/2 — and all three components go through the literal loops.  The atom is where it
    was, as far as anybody's minimum image is concerned, up to the rounding of the shift."""
    base = cases["cg"]
    system = cg(leaflets=LEAFLETS_NONE)
    np.testing.assert_array_equal(system.base, base.system.base)
    xyz = base.xyz.copy()
    atom = int(base.neighbours[2])
    assert atom in base.centres
    xyz[3, atom, 0] += F32(2.0) * system.box[0]
    xyz[7, atom, 1] -= F32(2.0) * system.box[1]
    xyz[8, atom, 0] -= F32(3.0) * system.box[0]
    xyz[8, atom, 2] += F32(2.0) * system.box[2]
    case = make_case(system, base.centres, base.neighbours, base.radius, xyz=xyz, far=True)
    assert case.counts.max() == 3 and case.counts[3].sum() > 0
    for env in ({}, {"GORDER_HIP_NB_DIRECT": "1"}):
        with pytest.MonkeyPatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            assert_classes(run(case, 4, CUTS["three"]), case, 4)


# ---- 4. ties --------------------------------------------------------------------------------------------------------------------
def test_ties(built):
    """Radii fitted so that a real pair's d2 is the threshold itself — sqrt(d2) < r is false: not counted — or the float
    below it — counted.  The `<=` rule would give other rows for every one of them."""
    case = cg_case(cg(leaflets=LEAFLETS_NONE, handle_pbc=False), n_frames=2)
    other = case.centres[:, None] != case.neighbours[None, :]
    fitted = []                                                          # (frame, radius, the pair is counted)
    f = 0
    cand = np.argwhere(other & (case.d2[f] > 0.3) & (case.d2[f] < 2.0))
    for m, q in cand:
        d2 = case.d2[f, m, q]
        for target, counted in ((d2, False), (bp.step(d2, 1), True)):
            for k in range(-2, 3):
                r = bp.step(np.sqrt(F32(target)), k)
                if bp.radius_threshold(r) == target:
                    fitted.append((float(r), counted, int(m), int(q)))
                    break
        if sum(1 for x in fitted if not x[1]) >= 3 and sum(1 for x in fitted if x[1]) >= 3:
            break
    assert len(fitted) >= 4 and any(c for _, c, _, _ in fitted) and any(not c for _, c, _, _ in fitted)
    one = Case(case.system, case.xyz[:1], None, Samples(case.samples.tick[:1], case.samples.slot, case.samples.mol), None,
               case.centres, case.neighbours, 1.0)
    for r, counted, m, q in fitted[:8]:
        thr = bp.radius_threshold(r)
        d2 = case.d2[0, m, q]
        assert (d2 < thr) == counted and places(d2, thr) == (1 if counted else 0)
        literal = neighbour_counts(one.d2, thr, one.centres, one.neighbours)
        wrong = neighbour_counts(one.d2, thr if not counted else bp.step(thr, -1), one.centres, one.neighbours, "<=" if not counted else "<")
        assert literal[0, m] - wrong[0, m] == (1 if counted else -1)     # the other rule, or a threshold one float off, is seen
        n_classes = 32
        assert not np.array_equal(np.minimum(literal, 31), np.minimum(wrong, 31))
        eng = HipEngine(case.system.tables)
        eng.set_neighbour_classes(one.centres, one.neighbours, r, n_classes)
        eng.submit_host(one.xyz, None, FRAMES[:1])
        np.testing.assert_array_equal(eng.neighbour_class_rows(), np.minimum(literal, 31).astype(np.uint8))
        assert_classes(eng, one, n_classes, classes=np.minimum(literal, 31).astype(np.uint8))


# ---- 5. invariants -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cg", "aa"])
def test_finish_is_untouched_and_the_groups_add_up(cases, name):
    case = cases[name]
    eng, plain = HipEngine(case.system.tables), HipEngine(case.system.tables)
    eng.set_neighbour_classes(case.centres, case.neighbours, case.radius, 4)
    for e in (eng, plain):
        e.kernel_time()                   # switches the timing on
        for a, b in CUTS["three"]:
            e.submit_host(case.xyz[a:b], case.box[a:b], FRAMES[a:b])
    got, want = eng.finish(), plain.finish()
    total, launches = eng.kernel_time()
    groups = eng.kernel_groups()
    names = [g[0] for g in groups]
    assert "k_bonds_classes" in names and "k_neighbour_counts" in names and "k_bonds_tiled" not in names and "k_bonds_extras" not in names
    assert names.index("k_neighbour_counts") < names.index("k_bonds_classes") < names.index("k_batch_end")
    assert "k_bonds_classes" in eng.kernel_names() and "k_neighbour_counts" in eng.kernel_names()
    assert launches == 3 and abs(sum(g[1] for g in groups) - total) <= 1e-6 * max(1.0, total)
    if name == "cg":                     # global leaflets: their own kernel ahead of the counts, no speculation
        assert names[0].startswith("k_leaflets_global") and eng.speculation_stats()["batches"] == 0
    np.testing.assert_array_equal(got.sums, want.sums)
    np.testing.assert_array_equal(got.counts, want.counts)
    assert got.n_frames == want.n_frames == N and want.counts[0].min() > 0
    assert_classes(eng, case, 4)
    plain.kernel_time()
    assert "k_bonds_classes" not in plain.kernel_names() and "k_neighbour_counts" not in plain.kernel_names() and "k_bonds_tiled" in plain.kernel_names()
    assert plain.neighbour_classes() == [] and plain.neighbour_class_rows().shape == (0, 0)


def test_reset_zeroes_the_arrays_and_keeps_the_setting(cases):
    case = cases["cg"]
    eng = run(case, 4, CUTS["three"])
    first = assert_classes(eng, case, 4)
    again = assert_classes(eng, case, 4)                                 # reading twice changes nothing
    np.testing.assert_array_equal(first[0], again[0])
    eng.reset()
    for r in eng.neighbour_classes():
        assert not r.sums.any() and not r.counts.any() and r.n_frames == 0
    assert eng.neighbour_class_rows().shape[0] == 0
    run(case, 4, CUTS["one"], engine=eng)
    assert_classes(eng, case, 4)
    # half a run, then the whole: the arrays of a handle grow batch by batch
    eng.reset()
    eng.submit_host(case.xyz[:4], case.box[:4], FRAMES[:4])
    assert_classes(eng, case, 4, frames=slice(0, 4))
    eng.submit_host(case.xyz[4:], case.box[4:], FRAMES[4:])
    assert_classes(eng, case, 4)
    # an empty list switches the feature off
    eng.reset()
    eng.set_neighbour_classes(case.centres, [], case.radius, 4)
    eng.submit_host(case.xyz, case.box, FRAMES)
    assert eng.neighbour_classes() == []
    plain = HipEngine(case.system.tables)
    plain.submit_host(case.xyz, case.box, FRAMES)
    np.testing.assert_array_equal(eng.finish().sums, plain.finish().sums)
    eng.kernel_time()
    assert "k_bonds_classes" not in eng.kernel_names()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["centre", "neighbour"])
def test_an_undefined_position_is_raised(cases, which):
    case = cases["cg"]
    system = cg(leaflets=LEAFLETS_NONE)                                  # (the same frames: the leaflets do not enter the coordinates)
    np.testing.assert_array_equal(system.base, case.system.base)
    xyz = case.xyz.copy()
    # every bead of these lipids is in a bond, whose kernel raises the same status for it at the molecule-type stage: the
    # system stage of the same frame comes first in the key, so it is k_neighbour_counts that is heard
    if which == "centre":
        atom = int(case.centres[7])
        neighbours = case.neighbours[case.neighbours != atom]
    else:                                                                # bead 0 of a lipid: nobody's centre
        atom = 12 * 4
        neighbours = np.sort(np.append(case.neighbours, atom))
    xyz[6, atom] = np.nan
    eng = HipEngine(system.tables)
    eng.set_neighbour_classes(case.centres, neighbours, case.radius, 4)
    with pytest.raises(abi.GorderHipError) as e:
        for a, b in CUTS["three"]:
            eng.submit_host(xyz[a:b], case.box[a:b], FRAMES[a:b])
        eng.finish()
    assert (e.value.status, e.value.index, e.value.frame) == (abi.ERR_UNDEFINED_POSITION, atom, 106)
    with pytest.raises(abi.GorderHipError) as e:
        eng.neighbour_classes()
    assert e.value.status == abi.ERR_UNDEFINED_POSITION


def refused(tables, before=None, centres=None, neighbours=None, radius=1.0, n_classes=4):
    eng = HipEngine(tables)
    if before:
        before(eng)
    n_mol = tables.n_molecules_total
    with pytest.raises(abi.GorderHipError) as e:
        eng.set_neighbour_classes(np.arange(n_mol) if centres is None else centres, [0, 5, 9] if neighbours is None else neighbours, radius, n_classes)
    assert e.value.status == abi.ERR_INVALID_ARGUMENT and "gorder_hip_set_neighbour_classes" in str(e.value)
    return str(e.value)


def test_refusals(cases):
    assert "united-atom" in refused(synthetic.ua_membrane(24).tables)
    om = OrderMap(enabled=True, plane=0, span_x=(0.0, 4.0), span_y=(0.0, 4.0), bin=(0.4, 0.4))
    assert "ordermaps" in refused(cg(ordermap=om).tables)
    assert "timewise" in refused(cg(timewise=True).tables)
    geo = cg()
    geo.tables.geometry = Geometry(kind=abi.GEOM_CYLINDER, reference=abi.GEOMREF_BOX_CENTER, orientation=2, radius=2.0,
                                   structure_box=tuple(float(x) for x in geo.box))
    assert "geometry selection" in refused(geo.tables)
    dyn = cg()
    dyn.tables.dynamic_normal = abi.DynamicNormal(enabled=True, radius=2.0, cloud=np.concatenate([m.heads for m in dyn.tables.molecule_types]))
    for m in dyn.tables.molecule_types:
        m.normal_heads = m.heads
    assert "dynamic" in refused(dyn.tables)
    t = cg().tables
    up = np.tile(np.array([0.0, 0.0, 1.0], dtype=np.float32), (2, t.n_molecules_total, 1))
    assert "normal table" in refused(t, before=lambda e: e.set_manual_normal_table(up))
    assert "gorder_hip_set_normals" in refused(t, before=lambda e: e.set_normals(up))
    assert "molecule rows" in refused(t, before=lambda e: e.set_molecule_rows([[0, 1], [2]]))
    assert "order histogram" in refused(t, before=lambda e: e.set_order_histogram(structure.order_edges(16)))
    wide = synthetic.cg_membrane(200, leaflets=LEAFLETS_GLOBAL, n_types=2)
    b = np.asarray(wide.tables.molecule_types[0].bonds).copy()
    b[0, 0] = (0, 12 * 199 + 11)                                       # 2400 atoms apart: more than the 1024-atom window
    wide.tables.molecule_types[0].bonds = b
    assert "direct items" in refused(wide.tables)
    none = cg()
    for m in none.tables.molecule_types:
        m.bonds = np.asarray(m.bonds)[:0]
    assert "no bond samples" in refused(none.tables)
    # the arguments themselves
    n_atoms, n_mol = t.n_atoms, t.n_molecules_total
    assert "centre index >= n_atoms" in refused(t, centres=np.append(np.arange(n_mol - 1), n_atoms))
    assert "neighbour index >= n_atoms" in refused(t, neighbours=[0, n_atoms])
    assert "ascending" in refused(t, neighbours=[0, 5, 5])
    assert "ascending" in refused(t, neighbours=[0, 5, 4])
    big_t = synthetic.cg_membrane(1400, n_types=1).tables                # 16 800 atoms: room for one neighbour too many
    assert "GORDER_NEIGHBOUR_MAX_ATOMS" in refused(big_t, neighbours=np.arange(abi.NEIGHBOUR_MAX_ATOMS + 1))
    HipEngine(big_t).set_neighbour_classes(np.arange(1400), np.arange(abi.NEIGHBOUR_MAX_ATOMS), 1.0, 2)     # the most
    assert "fewer than 2 classes" in refused(t, n_classes=1)
    assert "GORDER_NEIGHBOUR_MAX_CLASSES" in refused(t, n_classes=abi.NEIGHBOUR_MAX_CLASSES + 1)
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        assert "radius" in refused(t, radius=radius)
    with pytest.raises(ValueError):
        HipEngine(t).set_neighbour_classes(np.arange(n_mol - 1), [0, 5], 1.0, 4)
    # a handle with classes refuses what the classes refuse: the mirror messages
    eng = HipEngine(t)
    eng.set_neighbour_classes(np.arange(n_mol), [0, 5, 9], 1.0, abi.NEIGHBOUR_MAX_CLASSES)
    for call in (lambda: eng.set_normals(up), lambda: eng.set_manual_normal_table(up), lambda: eng.set_molecule_rows([[0, 1], [2]]),
                 lambda: eng.set_order_histogram(structure.order_edges(16))):
        with pytest.raises(abi.GorderHipError) as e:
            call()
        assert e.value.status == abi.ERR_INVALID_ARGUMENT and "neighbour classes" in str(e.value)
    with pytest.raises(abi.GorderHipError) as e:
        eng.set_radial_shells([1.0, 2.0])
    assert e.value.status == abi.ERR_INVALID_ARGUMENT and "neighbour classes" in str(e.value)
    assert "radial shells" in refused(geo.tables, before=lambda e: e.set_radial_shells([1.0, 2.0]))
    # after the first submit; reset opens the setter again
    case = cases["cg"]
    eng = HipEngine(case.system.tables)
    eng.submit_host(case.xyz[:1], case.box[:1], FRAMES[:1])
    with pytest.raises(abi.GorderHipError) as e:
        eng.set_neighbour_classes(case.centres, case.neighbours, 1.0, 4)
    assert e.value.status == abi.ERR_INVALID_ARGUMENT and "first submit" in str(e.value)
    eng.reset()
    eng.set_neighbour_classes(case.centres, case.neighbours, 1.0, 4)
    run(case, 4, engine=eng)
    assert_classes(eng, case, 4)
