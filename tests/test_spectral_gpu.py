"""Spectral-clustering leaflets on the device (GORDER_LEAFLETS_CLUSTERING, k_cluster_*).

Expected flags come from the CPU statement of the method (tests/spectral_ref.py), expected order sums from the oracle with
LEAFLETS_MANUAL fed those flags per assignment frame: flags equal for every molecule, sums, counts and rows EQUAL.
An input is admitted only if the float32 and float64 twins agree on every molecule (asserted where the twins are run).

Eigenvalue tolerance: the largest deviation of the float32 twin from the float64 twin over the inputs of test_statistics
is computed and printed by that test (measured: 7.2e-8); the device is allowed four times that figure, 2.9e-7, and was
measured at 1.5e-8 (cg.npz, 92 Lanczos steps) and 3.3e-9 (the buckled membrane, 60 steps) from the float64 twin."""
import copy

import numpy as np
import pytest

import spectral_ref as sr
from golden_util import Fixture, cg_setup, aa_setup, expected
from gorder_amd import HipEngine, abi, synthetic
from gorder_amd import structure as st
from gorder_amd.abi import (LEAFLETS_CLUSTERING, LEAFLETS_GLOBAL, LEAFLETS_MANUAL, DynamicNormal, Leaflets, MolType, OrderMap,
                            Tables)
from oracle import oracle

pytestmark = pytest.mark.gpu

_CACHE = {}


def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def manual_tables(tables):
    t = copy.copy(tables)
    t.leaflets = Leaflets(method=LEAFLETS_MANUAL, frequency=1)
    return t


def helper_flags(tables, xyz, box, frame_index):
    return {fi: sr.molecule_flags(tables, res) for fi, res in sr.run(tables, xyz, box, frame_index).items()}


def manual_route(engine_cls, tables, xyz, box, frame_index, flags_of, **kw):
    eng = engine_cls(manual_tables(tables), **kw)
    start, n = 0, len(frame_index)
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


def two_sheets(n, pbc, seed=0, n_upper=None, timewise=False, frequency=1, flip=False):
    """n two-bead molecules (head, tail) on two flat sheets 3 nm apart, 0.7 nm between neighbours; molecules 0 and 1 are in
    the upper sheet (n > 2), which holds n_upper (default: 60 %) of them -> (tables, frame [2 n, 3], box [3], sides).
    Above 300 molecules the neighbours are 0.3 nm apart, so that the sheets stay small against their separation."""
    rng = np.random.default_rng(seed)
    sp = 0.7 if n <= 300 else 0.3
    n_up = n_upper if n_upper is not None else (1 if n == 2 else max(2, (3 * n + 4) // 5))
    sides = np.ones(n, dtype=np.uint8)
    sides[:2 if n > 2 else 1] = 0
    rest = np.arange(2 if n > 2 else 1, n)
    sides[rng.permutation(rest)[:n_up - (2 if n > 2 else 1)]] = 0
    side_len = int(np.ceil(np.sqrt(max(n_up, n - n_up))))
    L = side_len * sp + 6.0
    frame = np.zeros((2 * n, 3), dtype=np.float32)
    for s in (0, 1):
        ids = np.flatnonzero(sides == s)
        g = np.arange(len(ids))
        xy = np.stack([(g % side_len) * sp + 3.0, (g // side_len) * sp + 3.0], axis=1) + rng.normal(0, 0.05, (len(ids), 2))
        z = 6.0 + (1.5 if s == 0 else -1.5)
        frame[2 * ids, 0:2] = xy
        frame[2 * ids, 2] = z + rng.normal(0, 0.05, len(ids))
        frame[2 * ids + 1, 0:2] = xy + rng.normal(0, 0.1, (len(ids), 2))
        frame[2 * ids + 1, 2] = z - (0.4 if s == 0 else -0.4)
    heads = (2 * np.arange(n)).astype(np.uint32)
    bonds = np.array([[[2 * m, 2 * m + 1] for m in range(n)]], dtype=np.uint32)
    t = Tables(n_atoms=2 * n, molecule_types=[MolType(n_molecules=n, bonds=bonds, heads=heads)], handle_pbc=pbc,
               leaflets=Leaflets(method=LEAFLETS_CLUSTERING, membrane=heads.copy(), frequency=frequency, flip=flip),
               timewise=timewise)
    return t, frame, np.array([L, L, 12.0], dtype=np.float32), sides


def box9(box, n):
    b = np.zeros((n, 3, 3), dtype=np.float32)
    b[:, 0, 0], b[:, 1, 1], b[:, 2, 2] = box
    return b


@pytest.mark.parametrize("pbc", [True, False])
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 257, 1030])
def test_minimal_groups(built, n, pbc):
    """The reference's minimum (2), 3 (Krylov space exhausted after two steps), the wave and row-split edges, and 1030 heads —
    more than a workgroup has threads.  Rows 0 and 1 lie in the same leaflet for n > 2."""
    torch_cuda()
    t, frame, box, sides = two_sheets(n, pbc)
    res = sr.classify(frame, t.leaflets.membrane, box, pbc)
    r64 = sr.classify(frame, t.leaflets.membrane, box, pbc, np.float64)
    np.testing.assert_array_equal(res["upper"], r64["upper"])
    want = sr.molecule_flags(t, res)
    if n != 3:
        # Three heads: after row normalisation the rows of a pair and a single head are the corners of an equilateral triangle
        # ((1/2, +-sqrt(3)/2) and (-1, 0)) wherever the heads lie, so the literal 2-means decides the third row on a tie or
        # on rounding — no three-head layout makes it find the sheets.  The flags are the helper's, as for every size.
        np.testing.assert_array_equal(want, sides)
    eng = HipEngine(t)
    eng.submit_host(frame[None], box9(box, 1) if pbc else None, np.array([0]))
    flags, at = eng.leaflets()
    stt = eng.clustering_stats()
    print(n, pbc, stt, res["eig"], res["rounds"], res["n_cluster"])
    np.testing.assert_array_equal(flags, want)
    assert at == 0 and stt["n_upper"] == int(res["upper"].sum()) and stt["n_lower"] == int((~res["upper"]).sum())
    assert stt["steps"] <= min(n - 1, 300) and np.isnan(stt["o_up"]) and np.isnan(stt["o_lo"])
    assert_equal_results(eng.finish(), oracle_route(t, frame[None], box9(box, 1) if pbc else None, np.array([0]), {0: want}))


def cg_case():
    if "cg" not in _CACHE:
        fx = Fixture("cg")
        tables, labels, midx = cg_setup(fx, leaflets=LEAFLETS_CLUSTERING)
        frames = fx.window()
        xyz = np.ascontiguousarray(fx.xyz[frames][:, midx, :])
        box = fx.boxes[frames]
        fi = np.asarray(frames)
        _CACHE["cg"] = (fx, tables, labels, midx, xyz, box, fi, sr.run(tables, xyz, box, fi))
    return _CACHE["cg"]


def test_cg_fixture_every_frame(built):
    """All 101 frames of the flat CG membrane, one submit a frame: flags = helper = GORDER_LEAFLETS_GLOBAL for every molecule,
    sums EQUAL the oracle fed those flags, and the result reproduces the reference's cg_order_leaflets.yaml."""
    torch_cuda()
    fx, tables, labels, midx, xyz, box, fi, ref = cg_case()
    assert len(fi) == 101 and len(tables.leaflets.membrane) == 508
    tg, _, _ = cg_setup(fx, leaflets=LEAFLETS_GLOBAL)
    eng, glob = HipEngine(tables), HipEngine(tg)
    flags_of = {}
    for k in range(len(fi)):
        eng.submit_host(xyz[k:k + 1], box[k:k + 1], fi[k:k + 1])
        glob.submit_host(xyz[k:k + 1], box[k:k + 1], fi[k:k + 1])
        flags = eng.leaflets()[0]
        flags_of[int(fi[k])] = sr.molecule_flags(tables, ref[int(fi[k])])
        np.testing.assert_array_equal(flags, flags_of[int(fi[k])], err_msg=f"frame {k}")
        np.testing.assert_array_equal(flags, glob.leaflets()[0], err_msg=f"frame {k}")
    res = eng.finish()
    assert_equal_results(res, oracle_route(tables, xyz, box, fi, flags_of))
    bad = st.compare_trees(st.results_tree(res, labels, "cg", leaflets=True), expected("cg_order_leaflets.yaml"))
    assert not bad, bad[:10]


def test_pcpepg_fixture(built):
    """The atomistic membrane (274 `name P` heads, all 51 frames), one submit a frame, each frame matched against its
    predecessor: flags = helper = GORDER_LEAFLETS_GLOBAL for every molecule, sums and counts EQUAL the oracle fed those flags,
    and the result reproduces the reference's aa_order_leaflets.yaml.  The float32 and float64 twins agree on every frame."""
    torch_cuda()
    fx = Fixture("pcpepg")
    tables, labels, midx = aa_setup(fx, leaflets=LEAFLETS_CLUSTERING)
    tg, _, _ = aa_setup(fx, leaflets=LEAFLETS_GLOBAL)
    frames = fx.window()
    xyz, box, fi = np.ascontiguousarray(fx.xyz[frames][:, midx, :]), fx.boxes[frames], np.asarray(frames)
    assert len(fi) == 51 and len(tables.leaflets.membrane) == 274
    ref, r64 = sr.run(tables, xyz, box, fi), sr.run(tables, xyz, box, fi, np.float64)
    eng, glob = HipEngine(tables), HipEngine(tg)
    flags_of = {}
    for k in range(len(fi)):
        np.testing.assert_array_equal(ref[int(fi[k])]["upper"], r64[int(fi[k])]["upper"], err_msg=f"twins, frame {k}")
        eng.submit_host(xyz[k:k + 1], box[k:k + 1], fi[k:k + 1])
        glob.submit_host(xyz[k:k + 1], box[k:k + 1], fi[k:k + 1])
        flags = eng.leaflets()[0]
        flags_of[int(fi[k])] = sr.molecule_flags(tables, ref[int(fi[k])])
        np.testing.assert_array_equal(flags, flags_of[int(fi[k])], err_msg=f"frame {k}")
        np.testing.assert_array_equal(flags, glob.leaflets()[0], err_msg=f"frame {k}")
    res = eng.finish()
    assert_equal_results(res, oracle_route(tables, xyz, box, fi, flags_of))
    bad = st.compare_trees(st.results_tree(res, labels, "aa", leaflets=True), expected("aa_order_leaflets.yaml"))
    assert not bad, bad[:10]


def test_three_equal_clusters(built):
    """Three equal clusters on an equilateral triangle: eigenvalues 2 and 3 of L are (nearly) equal, the two Ritz vectors
    span one plane.  The embedding must stay two-dimensional: the clusters' rows lie 120 degrees apart on the circle, so
    their first coordinates add up to zero (a collapsed embedding gives +-0.707 each).  Which two clusters share a leaflet
    depends on the basis of that plane and is not asserted; every cluster stays whole and both leaflets are populated."""
    torch_cuda()
    rng = np.random.default_rng(2)
    square = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [0.5, 0.5, 0]], dtype=np.float64)
    corners = 4.0 * np.array([[0, 0, 0], [1, 0, 0], [0.5, np.sqrt(3) / 2, 0]])
    heads_xyz = np.concatenate([c + square for c in corners]) + 5.0
    n = len(heads_xyz)
    frame = np.zeros((2 * n, 3), dtype=np.float32)
    frame[0::2] = heads_xyz
    frame[1::2] = heads_xyz + np.array([0.0, 0.0, 0.4]) + rng.normal(0, 0.05, (n, 3))
    heads = (2 * np.arange(n)).astype(np.uint32)
    bonds = np.array([[[2 * m, 2 * m + 1] for m in range(n)]], dtype=np.uint32)
    t = Tables(n_atoms=2 * n, molecule_types=[MolType(n_molecules=n, bonds=bonds, heads=heads)], handle_pbc=False,
               leaflets=Leaflets(method=LEAFLETS_CLUSTERING, membrane=heads.copy()))
    eng = HipEngine(t)
    eng.submit_host(frame[None], None, np.array([0]))
    flags, d, stt = eng.leaflets()[0], eng.leaflet_distances(), eng.clustering_stats()
    print(stt, d)
    assert abs(float(stt["eigenvalues"][0]) - float(stt["eigenvalues"][1])) < 1e-5
    per_cluster = d.reshape(3, 4)
    assert np.abs(per_cluster - per_cluster[:, :1]).max() < 1e-3
    assert abs(per_cluster[:, 0].sum()) < 1e-2
    assert all(len(set(flags[4 * c:4 * c + 4].tolist())) == 1 for c in range(3))
    assert stt["n_upper"] == 8 and stt["n_lower"] == 4
    eng.finish()


def test_buckled_membrane(built):
    """synthetic.cg_buckled at the CPU test's parameters: flags equal the construction, global leaflets on the same input do not."""
    torch_cuda()
    system, sides = synthetic.cg_buckled(**sr.BUCKLED)
    n = 2
    xyz, box, fi = system.frames(n, seed=1), system.box9(n), np.arange(n)
    eng = HipEngine(system.tables)
    eng.submit_host(xyz, box, fi)
    np.testing.assert_array_equal(eng.leaflets()[0], sides)
    flags_of = helper_flags(system.tables, xyz, box, fi)
    assert_equal_results(eng.finish(), oracle_route(system.tables, xyz, box, fi, flags_of))
    d = eng.leaflet_distances()
    assert ((d > 0) == (sides == sides[0])).all()          # the number behind the flag: the sign of v2, head 0 positive
    g, _ = synthetic.cg_buckled(leaflets=LEAFLETS_GLOBAL, **sr.BUCKLED)
    e2 = HipEngine(g.tables)
    e2.submit_host(xyz, box, fi)
    assert 50 < (e2.leaflets()[0] != sides).sum() < len(sides) - 50


def moved(frame, sides, k):
    """The frame with the first k lower-sheet molecules (from molecule 2 on) lifted into the upper sheet, and as many back."""
    out = frame.copy()
    lo, up = np.flatnonzero(sides == 1)[:k], np.flatnonzero(sides == 0)[2:2 + k]
    for a, b in zip(lo, up):
        out[[2 * a, 2 * a + 1, 2 * b, 2 * b + 1]] = frame[[2 * b, 2 * b + 1, 2 * a, 2 * a + 1]]
    return out


def test_orientation_rules(built):
    torch_cuda()
    # unequal populations: the larger sheet is upper even when molecule 0 lies in the smaller one — turn the sheets over
    t, frame, box, sides = two_sheets(65, True)
    turned = frame.copy()
    turned[:, 2] = 12.0 - turned[:, 2]
    eng = HipEngine(t)
    eng.submit_host(turned[None], box9(box, 1), np.array([0]))
    np.testing.assert_array_equal(eng.leaflets()[0], sides)
    # a tie: the cluster of the lowest atom is upper, whichever sheet that is
    t, frame, box, sides = two_sheets(64, True, n_upper=32)
    for fr in (frame, turned_z(frame)):
        eng = HipEngine(t)
        eng.submit_host(fr[None], box9(box, 1), np.array([0]))
        np.testing.assert_array_equal(eng.leaflets()[0], sides)
        assert eng.clustering_stats()["n_upper"] == 32
    # flip
    tf = copy.deepcopy(t)
    tf.leaflets.flip = True
    eng = HipEngine(tf)
    eng.submit_host(frame[None], box9(box, 1), np.array([0]))
    np.testing.assert_array_equal(eng.leaflets()[0], 1 - sides)
    # a later frame with three molecules of each sheet exchanged still matches: 29 of 32 stay
    few = moved(frame, sides, 3)
    xyz = np.stack([frame, few])
    eng = HipEngine(t)
    eng.submit_host(xyz, box9(box, 2), np.arange(2))
    ref = sr.run(t, xyz, box9(box, 2), np.arange(2))
    np.testing.assert_array_equal(eng.leaflets()[0], sr.molecule_flags(t, ref[1]))
    stt = eng.clustering_stats()
    assert abs(float(max(stt["o_up"], stt["o_lo"])) - 29 / 32) < 1e-6 and (eng.leaflets()[0] != sides).sum() == 6
    eng.finish()
    # half of them exchanged: neither overlap reaches 80 %
    half = moved(frame, sides, 15)
    with pytest.raises(sr.MatchError):
        sr.run(t, np.stack([frame, frame, half]), box9(box, 3), np.arange(3))
    eng = HipEngine(t)
    eng.submit_host(np.stack([frame, frame, half]), box9(box, 3), np.arange(3))
    with pytest.raises(abi.GorderHipError) as e:
        eng.finish()
    assert e.value.status == abi.ERR_CLUSTER_MATCH and e.value.frame == 2


def turned_z(frame):
    out = frame.copy()
    out[:, 2] = 12.0 - out[:, 2]
    return out


@pytest.mark.parametrize("frequency", [1, 5, 0])
def test_batching_independence(built, frequency):
    """One submit of 64 frames == 64 submits of one == two primed shards: flags, sums, rows and statistics EQUAL."""
    torch = torch_cuda()
    t, frame, box, sides = two_sheets(65, True, timewise=True, frequency=frequency)
    n = 64
    rng = np.random.default_rng(5)
    xyz = (frame[None] + rng.normal(0, 0.03, (n,) + frame.shape)).astype(np.float32)
    bx, fi = box9(box, n), np.arange(n)
    a = HipEngine(t)
    a.submit_host(xyz, bx, fi)
    ra = a.finish()
    b = HipEngine(t)
    for k in range(n):
        b.submit_host(xyz[k:k + 1], bx[k:k + 1], fi[k:k + 1])
    rb = b.finish()
    assert_equal_results(rb, ra)
    cut = 37
    sums, counts, rows = [], [], []
    for lo, hi in ((0, cut), (cut, n)):
        c = HipEngine(t)
        if lo:
            c.prime_leaflets_device(torch.from_numpy(xyz[0]).cuda(), torch.from_numpy(bx[0]).cuda(), 0)
            last = 0 if frequency == 0 else (lo - 1) // frequency * frequency
            if last:
                c.prime_leaflets_device(torch.from_numpy(xyz[last]).cuda(), torch.from_numpy(bx[last]).cuda(), last)
        c.submit_host(xyz[lo:hi], bx[lo:hi], fi[lo:hi])
        rc = c.finish()
        sums.append(rc.sums); counts.append(rc.counts); rows.append(c.timewise(hi - lo))
    np.testing.assert_array_equal(sums[0] + sums[1], ra.sums)
    np.testing.assert_array_equal(counts[0] + counts[1], ra.counts)
    tw_a, tw_b = a.timewise(n), b.timewise(n)
    for q in (0, 1):
        np.testing.assert_array_equal(tw_a[q], tw_b[q])
        np.testing.assert_array_equal(np.concatenate([rows[0][q], rows[1][q]]), tw_a[q])
    np.testing.assert_array_equal(a.leaflets()[0], b.leaflets()[0])
    np.testing.assert_array_equal(a.leaflets()[0], c.leaflets()[0])
    sa, sb, sc = a.clustering_stats(), b.clustering_stats(), c.clustering_stats()
    for q in sa:
        assert np.array_equal(sa[q], sb[q], equal_nan=True) and np.array_equal(sa[q], sc[q], equal_nan=True), q
    assert_equal_results(ra, oracle_route(t, xyz, bx, fi, helper_flags(t, xyz, bx, fi)))
    # gorder_hip_reset forgets the carry: a later frame first is refused, the whole run again gives the same
    a.reset()
    with pytest.raises(abi.GorderHipError) as e:
        a.submit_host(xyz[1:2], bx[1:2], np.array([5]))
    assert e.value.status == abi.ERR_LEAFLETS_NOT_PRIMED
    a.reset()
    a.submit_host(xyz, bx, fi)
    assert_equal_results(a.finish(), ra)


def test_errors(built):
    torch_cuda()
    t, frame, box, sides = two_sheets(65, True)

    def status_of(tables):
        with pytest.raises(abi.GorderHipError) as e:
            HipEngine(tables)
        return e.value.status, str(e.value)

    small = copy.deepcopy(t)
    small.leaflets.membrane = small.leaflets.membrane[:1]
    assert status_of(small)[0] == abi.ERR_INVALID_ARGUMENT                     # below the minimum of 2
    outside = copy.deepcopy(t)
    outside.leaflets.membrane = outside.leaflets.membrane[1:]
    assert status_of(outside)[0] == abi.ERR_INVALID_ARGUMENT                   # a head outside the group
    big = copy.deepcopy(t)
    big.n_atoms = 2 * 65 + sr.MAX_GROUP
    big.leaflets.membrane = np.concatenate([big.leaflets.membrane, np.arange(130, 130 + sr.MAX_GROUP)]).astype(np.uint32)
    status, text = status_of(big)
    assert status == abi.ERR_INVALID_ARGUMENT and str(sr.MAX_GROUP) in text    # above the bound, which the message names
    eng = HipEngine(t)
    with pytest.raises(abi.GorderHipError) as e:
        eng.clustering_stats()                                                 # before any assignment
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
    with pytest.raises(abi.GorderHipError) as e:
        eng.submit_host(frame[None], box9(box, 1), np.array([3]))              # a later frame, nothing held
    assert e.value.status == abi.ERR_LEAFLETS_NOT_PRIMED
    bad = np.stack([frame] * 4)
    bad[2, 2 * 7, 1] = np.nan
    eng = HipEngine(t)
    eng.submit_host(bad, box9(box, 4), np.arange(4))
    with pytest.raises(abi.GorderHipError) as e:
        eng.finish()
    assert e.value.status == abi.ERR_CLUSTERING and e.value.frame == 2


def test_statistics(built):
    """Eigenvalues 2-4 of L against the float64 twin within four times the float32 twin's largest deviation over these
    inputs; populations and 2-means rounds EQUAL the helper where the twins agree on them."""
    torch_cuda()
    fx, tables, labels, midx, xyz, box, fi, ref = cg_case()
    system, _ = synthetic.cg_buckled(**sr.BUCKLED)
    bx = system.frames(1, seed=1)
    cases = [(tables, xyz[0], box[0]), (tables, xyz[50], box[50]), (system.tables, bx[0], system.box9(1)[0])]
    twins = [(sr.classify(f, t.leaflets.membrane, b, True, np.float32), sr.classify(f, t.leaflets.membrane, b, True, np.float64))
             for t, f, b in cases]
    gap = max(float(np.abs(a["eig"] - b["eig"]).max()) for a, b in twins)
    print("float32 twin against float64 twin, largest eigenvalue deviation:", gap)
    for (t, f, b), (r32, r64) in zip(cases, twins):
        np.testing.assert_array_equal(r32["upper"], r64["upper"])
        eng = HipEngine(t)
        eng.submit_host(f[None], b[None], np.array([0]))
        stt = eng.clustering_stats()
        dev = float(np.abs(stt["eigenvalues"].astype(np.float64) - r64["eig"]).max())
        print("device against float64 twin:", dev, stt, r64["eig"], r64["rounds"])
        assert dev <= 4 * gap
        if r32["n_cluster"] == r64["n_cluster"]:
            assert stt["n_cluster"] == r64["n_cluster"]
        if r32["rounds"] == r64["rounds"]:
            assert stt["rounds"] == r64["rounds"]
        eng.finish()


def test_other_routes(built):
    """Ordermaps, per-frame rows and dynamic normals take the flags as they take the spherical method's."""
    torch_cuda()
    system, sides = synthetic.cg_buckled(n_lipids=200, box=(16.0, 5.0, 16.0), amplitude=3.0, seed=3, timewise=True,
                                         ordermap=OrderMap(enabled=True, plane=0, span_x=(0.0, 16.0), span_y=(0.0, 5.0), bin=(0.5, 0.5)))
    t = system.tables
    n = 4
    xyz, box, fi = system.frames(n, seed=2), system.box9(n), np.arange(n)
    ref = sr.run(t, xyz, box, fi)
    r64 = sr.run(t, xyz, box, fi, np.float64)
    flags_of = {}
    for k in ref:
        np.testing.assert_array_equal(ref[k]["upper"], r64[k]["upper"])
        flags_of[k] = sr.molecule_flags(t, ref[k])
        np.testing.assert_array_equal(flags_of[k], sides)
    eng = HipEngine(t)
    eng.submit_host(xyz, box, fi)
    got = eng.finish()
    eng_o, want = manual_route(oracle.OracleEngine, t, xyz, box, fi, flags_of, trig=oracle.TRIG_DIRECT)
    assert_equal_results(got, want)
    assert got.map_counts[1].sum() > 0 and got.map_counts[2].sum() > 0
    for q in (0, 1):
        np.testing.assert_array_equal(eng.timewise(n)[q], eng_o.timewise(n)[q])
    dyn, _ = synthetic.cg_buckled(n_lipids=200, box=(16.0, 5.0, 16.0), amplitude=3.0, seed=3)
    td = dyn.tables
    td.molecule_types[0].normal_heads = np.asarray(td.molecule_types[0].heads, dtype=np.uint32)
    td.dynamic_normal = DynamicNormal(enabled=True, radius=2.0, cloud=np.asarray(td.leaflets.membrane, dtype=np.uint32))
    e2 = HipEngine(td)
    e2.submit_host(xyz, box, fi)
    g2 = e2.finish()
    np.testing.assert_array_equal(e2.leaflets()[0], sides)
    assert_equal_results(g2, manual_route(HipEngine, td, xyz, box, fi, flags_of)[1])
