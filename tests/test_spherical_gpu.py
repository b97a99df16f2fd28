"""Spherical-clustering leaflets on the device (GORDER_LEAFLETS_SPHERICAL, k_leaflets_spherical).

Expected order sums come from the oracle with LEAFLETS_MANUAL, fed per assignment frame the flags of the CPU statement of
the method (tests/spherical_ref.py): sums, counts and rows must be EQUAL, flags equal for every molecule."""
import copy

import numpy as np
import pytest

import spherical_ref as sr
from gorder_amd import HipEngine, abi, synthetic
from gorder_amd.abi import LEAFLETS_MANUAL, LEAFLETS_SPHERICAL, Leaflets, MolType, OrderMap, Tables
from oracle import oracle

pytestmark = pytest.mark.gpu


def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def should_assign(frequency, frame):
    return frame == 0 if frequency == 0 else frame % frequency == 0


def manual_tables(tables):
    t = copy.copy(tables)
    t.leaflets = Leaflets(method=LEAFLETS_MANUAL, frequency=1)
    return t


def helper_flags(tables, xyz, box, frame_index):
    """{frame: flags} of the assignment frames among frame_index (flip applied)."""
    out = {}
    for k, fi in enumerate(frame_index):
        if should_assign(tables.leaflets.frequency, int(fi)):
            out[int(fi)] = sr.molecule_flags(tables, xyz[k], None if box is None else box[k])
    return out


def manual_route(engine_cls, tables, xyz, box, frame_index, flags_of, **kw):
    """The frames through LEAFLETS_MANUAL with the helper's flags set at every assignment frame -> Results."""
    eng = engine_cls(manual_tables(tables), **kw)
    start = 0
    n = len(frame_index)
    for k in range(n + 1):
        if k == n or (k > start and int(frame_index[k]) in flags_of):
            eng.submit_host(xyz[start:k], None if box is None else box[start:k], frame_index[start:k])
            start = k
        if k < n and int(frame_index[k]) in flags_of:
            eng.set_manual_leaflets(flags_of[int(frame_index[k])], int(frame_index[k]))
    return eng, eng.finish()


def oracle_route(tables, xyz, box, frame_index, flags_of):
    return manual_route(oracle.OracleEngine, tables, xyz, box, frame_index, flags_of, trig=oracle.TRIG_DIRECT)[1]


def assert_equal_results(got, want):
    assert got.n_frames == want.n_frames
    np.testing.assert_array_equal(got.counts, want.counts)
    np.testing.assert_array_equal(got.sums, want.sums)
    if want.map_sums is not None:
        np.testing.assert_array_equal(got.map_counts, want.map_counts)
        np.testing.assert_array_equal(got.map_sums, want.map_sums)


@pytest.mark.parametrize("name", sr.SEPARATED)
def test_separated_vesicles(built, name):
    """Flags of EVERY molecule in every frame = helper = the generator's true sides; sums / counts EQUAL to the oracle route;
    flip inverts exactly; statistics against the float32 helper within four times the recorded float32 / float64 gap."""
    torch_cuda()
    system, sides = sr.make_fixture(name)
    n = 3
    xyz, box = system.frames(n, seed=sr.GAP_SEED), system.box9(n)
    fi = np.arange(n)
    gap = sr.load_kat()["gaps"][name]
    eng = HipEngine(system.tables)
    for k in range(n):
        eng.submit_host(xyz[k:k + 1], box[k:k + 1], fi[k:k + 1])
        flags, frame = eng.leaflets()
        ref = sr.classify(xyz[k], system.tables.leaflets.membrane, system.box)
        want = sr.molecule_flags(system.tables, xyz[k], system.box, result=ref)
        assert frame == k
        np.testing.assert_array_equal(flags, want)
        np.testing.assert_array_equal(flags, sides)
        st = eng.spherical_stats()
        p = ref["params"]
        d = eng.leaflet_distances()
        print(name, k, st, {q: float(v) for q, v in p.items()}, ref["iterations"])
        assert st["iterations"] == ref["iterations"]
        assert st["n_outer"] == int((sides == 0).sum())
        cd = np.abs(st["centre"].astype(np.float64) - ref["centre"])
        cd = np.minimum(cd, system.box - cd)
        assert cd.max() <= 4 * gap["centre"]
        assert abs(float(st["mean_a"]) - float(p["mean_a"])) <= 4 * gap["mean"] and abs(float(st["mean_b"]) - float(p["mean_b"])) <= 4 * gap["mean"]
        assert abs(float(st["var_a"]) - float(p["var_a"])) <= 4 * gap["var"] and abs(float(st["var_b"]) - float(p["var_b"])) <= 4 * gap["var"]
        assert abs(float(st["weight_a"]) - float(p["weight_a"])) <= 4 * gap["weight"]
        assert (d >= 0).all() and np.abs(d - sr.head_distances(system.tables, ref)).max() <= 4 * gap["centre"] + 1e-5
    got = eng.finish()
    flags_of = helper_flags(system.tables, xyz, box, fi)
    assert_equal_results(got, oracle_route(system.tables, xyz, box, fi, flags_of))
    assert (got.counts[1] > 0).all() and (got.counts[2] > 0).all()
    flipped, _ = sr.make_fixture(name, flip=True)
    e2 = HipEngine(flipped.tables)
    e2.submit_host(xyz, box, fi)
    g2 = e2.finish()
    np.testing.assert_array_equal(e2.leaflets()[0], 1 - sides)
    np.testing.assert_array_equal(g2.sums[1], got.sums[2])
    np.testing.assert_array_equal(g2.sums[2], got.sums[1])
    np.testing.assert_array_equal(g2.counts[1], got.counts[2])


@pytest.mark.parametrize("name", ["v600", "v3000"])
def test_across_the_periodic_faces_and_without_a_box(built, name):
    """The vesicle translated so that it straddles all three periodic faces, and its unwrapped copy with handle_pbc = 0:
    identical flags."""
    torch_cuda()
    system, sides = sr.make_fixture(name, centre=(0.3, 0.2, 0.1))
    n = 2
    xyz, box = system.frames(n, seed=2), system.box9(n)
    assert (np.ptp(xyz[0], axis=0) > 0.9 * system.box).all()          # it does straddle the faces
    eng = HipEngine(system.tables)
    eng.submit_host(xyz, box)
    wrapped = eng.leaflets()[0]
    np.testing.assert_array_equal(wrapped, sides)
    np.testing.assert_array_equal(wrapped, sr.molecule_flags(system.tables, xyz[-1], system.box))
    assert_equal_results(eng.finish(), oracle_route(system.tables, xyz, box, np.arange(n), helper_flags(system.tables, xyz, box, np.arange(n))))
    free = copy.copy(system.tables)
    free.handle_pbc = False
    raw = system.frames_unwrapped(n, seed=2)
    e2 = HipEngine(free)
    e2.submit_host(raw, None)
    np.testing.assert_array_equal(e2.leaflets()[0], wrapped)
    assert_equal_results(e2.finish(), oracle_route(free, raw, None, np.arange(n), helper_flags(free, raw, None, np.arange(n))))


@pytest.mark.parametrize("frequency", [1, 5, 0])
def test_frequency_batching_and_shards(built, frequency):
    """Every(1), Every(5), Once; one submit of 64 frames == 64 submits of one == two primed shards: flags, statistics, sums,
    counts and per-frame rows EQUAL, and equal to the oracle route."""
    torch = torch_cuda()
    system, _ = sr.make_fixture("v600", frequency=frequency, timewise=True)
    t = system.tables
    n = 64
    xyz, box = system.frames(n, seed=4), system.box9(n)
    fi = np.arange(n)
    a = HipEngine(t)
    a.submit_host(xyz, box, fi)
    ra = a.finish()
    b = HipEngine(t)
    for k in range(n):
        b.submit_host(xyz[k:k + 1], box[k:k + 1], fi[k:k + 1])
    rb = b.finish()
    cut = 37
    sums, counts, rows = [], [], []
    for lo, hi in ((0, cut), (cut, n)):
        c = HipEngine(t)
        if not should_assign(frequency, lo):
            assign = 0 if frequency == 0 else lo // frequency * frequency
            c.prime_leaflets_device(torch.from_numpy(xyz[assign]).cuda(), torch.from_numpy(box[assign]).cuda(), assign)
        c.submit_host(xyz[lo:hi], box[lo:hi], fi[lo:hi])
        rc = c.finish()
        sums.append(rc.sums); counts.append(rc.counts); rows.append(c.timewise(hi - lo))
    assert_equal_results(rb, ra)
    np.testing.assert_array_equal(sums[0] + sums[1], ra.sums)
    np.testing.assert_array_equal(counts[0] + counts[1], ra.counts)
    tw_a, tw_b = a.timewise(n), b.timewise(n)
    for q in (0, 1):
        np.testing.assert_array_equal(tw_a[q], tw_b[q])
        np.testing.assert_array_equal(np.concatenate([rows[0][q], rows[1][q]]), tw_a[q])
    np.testing.assert_array_equal(a.leaflets()[0], b.leaflets()[0])
    np.testing.assert_array_equal(a.leaflets()[0], c.leaflets()[0])
    assert a.leaflets()[1] == b.leaflets()[1] == c.leaflets()[1] == (0 if frequency == 0 else (n - 1) // frequency * frequency)
    sa, sb, sc = a.spherical_stats(), b.spherical_stats(), c.spherical_stats()
    for q in sa:
        assert np.array_equal(sa[q], sb[q]) and np.array_equal(sa[q], sc[q]), q
    flags_of = helper_flags(t, xyz, box, fi)
    assert len(flags_of) == {1: 64, 5: 13, 0: 1}[frequency]
    eng_o, want = manual_route(oracle.OracleEngine, t, xyz, box, fi, flags_of, trig=oracle.TRIG_DIRECT)
    assert_equal_results(ra, want)
    tw_o = eng_o.timewise(n)
    np.testing.assert_array_equal(tw_a[0], tw_o[0])
    np.testing.assert_array_equal(tw_a[1], tw_o[1])
    # a reset handle is a fresh one
    a.reset()
    a.submit_host(xyz, box, fi)
    assert_equal_results(a.finish(), ra)


def test_group_larger_than_the_registers(built):
    """20 000 heads: 16 384 distances live in registers, the rest in the frame's scratch row."""
    torch_cuda()
    system, sides = synthetic.cg_vesicle(20000, 12.0, 16.0, box=(40.0, 40.0, 40.0), sigma=0.3, seed=9, heads_only=True)
    n = 3
    xyz, box = system.frames(n, seed=1), system.box9(n)
    eng = HipEngine(system.tables)
    eng.submit_host(xyz, box)
    got = eng.finish()
    flags = eng.leaflets()[0]
    ref = sr.classify(xyz[-1], system.tables.leaflets.membrane, system.box)
    np.testing.assert_array_equal(flags, sides)
    np.testing.assert_array_equal(flags, sr.molecule_flags(system.tables, xyz[-1], system.box, result=ref))
    assert eng.spherical_stats()["iterations"] == ref["iterations"]
    fi = np.arange(n)
    assert_equal_results(got, oracle_route(system.tables, xyz, box, fi, helper_flags(system.tables, xyz, box, fi)))
    one = HipEngine(system.tables)
    for k in range(n):
        one.submit_host(xyz[k:k + 1], box[k:k + 1], fi[k:k + 1])
    assert_equal_results(one.finish(), got)


def test_with_an_ordermap_and_with_dynamic_normals(built):
    torch_cuda()
    system, sides = sr.make_fixture("v600", ordermap=OrderMap(enabled=True, plane=0, span_x=(5.0, 14.0), span_y=(5.0, 14.0), bin=(0.1, 0.1)))
    t = system.tables
    n = 6
    xyz, box = system.frames(n, seed=8), system.box9(n)
    fi = np.arange(n)
    flags_of = helper_flags(t, xyz, box, fi)
    eng = HipEngine(t)
    assert eng.ordermap_dims() == (91, 91)
    eng.submit_host(xyz, box, fi)
    got = eng.finish()
    assert got.map_counts[1].sum() > 0 and got.map_counts[2].sum() > 0
    assert_equal_results(got, oracle_route(t, xyz, box, fi, flags_of))
    # dynamic normals: the leaflet split (counts) EQUAL to the oracle route; the normals' own arithmetic is compared as the
    # dynamic-normal tests do (order parameters within one tick), and the device's manual route with the helper's flags
    # gives EQUAL sums
    from gorder_amd.abi import DynamicNormal
    dyn, _ = sr.make_fixture("v600")
    td = dyn.tables
    td.molecule_types[0].normal_heads = np.asarray(td.molecule_types[0].heads, dtype=np.uint32)
    td.dynamic_normal = DynamicNormal(enabled=True, radius=2.0, cloud=np.asarray(td.leaflets.membrane, dtype=np.uint32))
    e2 = HipEngine(td)
    e2.submit_host(xyz, box, fi)
    g2 = e2.finish()
    want = oracle_route(td, xyz, box, fi, flags_of)
    np.testing.assert_array_equal(g2.counts, want.counts)
    assert np.abs(g2.order_ticks() - want.order_ticks()).max() <= 1
    assert_equal_results(g2, manual_route(HipEngine, td, xyz, box, fi, flags_of)[1])
    np.testing.assert_array_equal(e2.leaflets()[0], sides)


def test_overlapping_vesicle(built):
    """Shells 6 and 8 nm, sigma 0.45: a head may be left out of the comparison only if the float64 twin's responsibility
    lies within 1e-3 of 0.5 (at most 0.5 % of the heads; the fixture's frames have none, tests/test_spherical_cpu.py)."""
    torch_cuda()
    system, _ = sr.make_fixture(sr.OVERLAPPING)
    t = system.tables
    n = sr.OVERLAP_FRAMES
    xyz, box = system.frames(n, seed=sr.GAP_SEED), system.box9(n)
    gap = sr.load_kat()["gaps"]["overlapping"]
    eng = HipEngine(t)
    for k in range(n):
        eng.submit_host(xyz[k:k + 1], box[k:k + 1], np.array([k]))
        flags = eng.leaflets()[0]
        f32 = sr.classify(xyz[k], t.leaflets.membrane, system.box)
        f64 = sr.classify(xyz[k], t.leaflets.membrane, system.box, True, np.float64)
        left_out = np.abs(sr.head_responsibilities(t, f64) - 0.5) <= 1e-3
        assert left_out.mean() <= 0.005
        want = sr.molecule_flags(t, xyz[k], system.box, result=f32)
        st = eng.spherical_stats()
        print("overlapping", k, "left out", int(left_out.sum()), "differ", int((flags != want).sum()), st, f32["params"], f32["iterations"])
        np.testing.assert_array_equal(flags[~left_out], want[~left_out])
        assert st["iterations"] == f32["iterations"]
        p = f32["params"]
        assert abs(float(st["mean_a"]) - float(p["mean_a"])) <= 4 * gap["mean"] and abs(float(st["mean_b"]) - float(p["mean_b"])) <= 4 * gap["mean"]
        assert abs(float(st["var_a"]) - float(p["var_a"])) <= 4 * gap["var"] and abs(float(st["var_b"]) - float(p["var_b"])) <= 4 * gap["var"]
        assert abs(float(st["weight_a"]) - float(p["weight_a"])) <= 4 * gap["weight"]


def small_vesicle(extra_group_atom=False):
    """200 lipids of two beads; optionally one more head-group atom that belongs to no analysed molecule."""
    system, sides = synthetic.cg_vesicle(200, 2.5, 5.0, box=(16.0, 16.0, 16.0), sigma=0.2, seed=3, heads_only=True)
    if extra_group_atom:
        t = system.tables
        t.n_atoms += 1
        t.leaflets.membrane = np.append(t.leaflets.membrane, t.n_atoms - 1).astype(np.uint32)
        extra = (system.box / 2 + np.array([5.0, 0.0, 0.0])).astype(np.float32)
        system.base = np.vstack([system.base, extra])
    return system, sides


def test_refusals_and_the_clustering_error(built):
    torch_cuda()
    system, sides = small_vesicle()

    def status_of(tables):
        with pytest.raises(abi.GorderHipError) as e:
            HipEngine(tables)
        return e.value.status

    t = copy.deepcopy(system.tables)
    t.leaflets.membrane = t.leaflets.membrane[:1]
    assert status_of(t) == abi.ERR_INVALID_ARGUMENT                      # one group atom: NotEnoughAtomsToCluster
    t = copy.deepcopy(system.tables)
    t.leaflets.membrane = t.leaflets.membrane[1:]
    assert status_of(t) == abi.ERR_INVALID_ARGUMENT                      # a head outside the group
    t = copy.deepcopy(system.tables)
    t.molecule_types[0].heads = None
    assert status_of(t) == abi.ERR_INVALID_ARGUMENT                      # no heads
    t = copy.deepcopy(system.tables)
    t.leaflets.membrane[3] = t.n_atoms
    assert status_of(t) == abi.ERR_INVALID_ARGUMENT                      # index out of range
    eng = HipEngine(system.tables)
    with pytest.raises(abi.GorderHipError) as e:
        eng.spherical_stats()                                            # before any assignment
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
    # a NaN coordinate of a group atom that belongs to no analysed molecule, in frame 3 of 8
    system, sides = small_vesicle(extra_group_atom=True)
    xyz, box = system.frames(8, seed=1), system.box9(8)
    eng = HipEngine(system.tables)
    eng.submit_host(xyz, box)
    np.testing.assert_array_equal(eng.leaflets()[0], sides)             # (the extra atom is classified with the others)
    bad = xyz.copy()
    bad[3, -1, 1] = np.nan
    eng = HipEngine(system.tables)
    eng.submit_host(bad, box)
    with pytest.raises(abi.GorderHipError) as e:
        eng.finish()
    assert e.value.status == abi.ERR_CLUSTERING and e.value.index == 3 and e.value.frame == 3
    zero = box.copy()
    zero[5] = 0.0
    eng = HipEngine(system.tables)
    eng.submit_host(bad, zero)
    with pytest.raises(abi.GorderHipError) as e:
        eng.finish()
    assert e.value.status == abi.ERR_CLUSTERING and e.value.index == 3    # still the first error in trajectory order
    eng = HipEngine(system.tables)
    eng.submit_host(xyz, zero)
    with pytest.raises(abi.GorderHipError) as e:
        eng.finish()
    assert e.value.status == abi.ERR_ZERO_BOX


def test_degenerate_input(built):
    """Four group atoms at the same distance from their centre (the corners of a square, no box): every responsibility is
    exp(-ln 2), within an ulp of 0.5 — which cluster they fall into is not asserted; the call succeeds within the 50
    iterations, all molecules come out on one side, upper + lower = total."""
    torch_cuda()
    corners = np.array([[1, 1, 0], [-1, 1, 0], [-1, -1, 0], [1, -1, 0]], dtype=np.float32)
    frame = np.zeros((8, 3), dtype=np.float32)
    frame[0::2] = corners
    frame[1::2] = corners * np.float32(0.5) + np.array([0, 0, 0.3], dtype=np.float32)
    bonds = np.array([[[2 * m, 2 * m + 1] for m in range(4)]], dtype=np.uint32)
    heads = np.arange(0, 8, 2, dtype=np.uint32)
    t = Tables(n_atoms=8, molecule_types=[MolType(n_molecules=4, bonds=bonds, heads=heads)], handle_pbc=False,
               leaflets=Leaflets(method=LEAFLETS_SPHERICAL, membrane=heads.copy()))
    eng = HipEngine(t)
    eng.submit_host(frame[None], None)
    got = eng.finish()
    flags = eng.leaflets()[0]
    st = eng.spherical_stats()
    assert 1 <= st["iterations"] <= 50
    assert len(set(flags.tolist())) == 1
    np.testing.assert_array_equal(got.counts[1] + got.counts[2], got.counts[0])
    assert got.counts[0].sum() == 4
    np.testing.assert_allclose(eng.leaflet_distances(), np.sqrt(2.0), rtol=1e-6)
