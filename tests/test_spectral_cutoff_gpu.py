"""Cut-off spectral-clustering leaflets on the device (GORDER_FLAG_CLUSTER_CUTOFF, k_clcut_*).

Expected flags come from the CPU statement of the method (tests/spectral_ref.py), from the construction of the input and from
a dense-route handle on the same frames; expected order sums from the oracle with LEAFLETS_MANUAL fed those flags per
assignment frame: sums, counts and rows EQUAL.

Eigenvalue tolerance (test_short_box_edges): the rule of test_spectral_gpu.py::test_statistics on this input — four times the
float32 twin's largest distance from the float64 twin, printed by the test."""
import copy

import numpy as np
import pytest

import spectral_cutoff_ref as scr
import spectral_ref as sr
from gorder_amd import HipEngine, abi, synthetic
from gorder_amd.abi import (COLLECT_LEAFLETS, FLAG_CLUSTER_CUTOFF, LEAFLETS_CLUSTERING, LEAFLETS_GLOBAL, LEAFLETS_MANUAL,
                            Leaflets, MolType, Tables)
from oracle import oracle

pytestmark = pytest.mark.gpu

LARGE = dict(n_lipids=2000, box=(40.0, 14.0, 16.0), amplitude=3.0, seed=13)
ABOVE = dict(n_lipids=8400, box=(84.0, 28.0, 16.0), amplitude=3.0, seed=13)


def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def with_flag(tables):
    t = copy.copy(tables)
    t.flags = tables.flags | FLAG_CLUSTER_CUTOFF
    return t


def oracle_route(tables, xyz, box, frame_index, flags_of):
    """The oracle with LEAFLETS_MANUAL fed flags_of[frame] at every assignment frame."""
    t = copy.copy(tables)
    t.flags = 0
    t.leaflets = Leaflets(method=LEAFLETS_MANUAL, frequency=1)
    eng = oracle.OracleEngine(t, trig=oracle.TRIG_DIRECT)
    start, n = 0, len(frame_index)
    for k in range(n + 1):
        if k == n or (k > start and int(frame_index[k]) in flags_of):
            eng.submit_host(xyz[start:k], None if box is None else box[start:k], frame_index[start:k])
            start = k
        if k < n and int(frame_index[k]) in flags_of:
            eng.set_manual_leaflets(flags_of[int(frame_index[k])], int(frame_index[k]))
    return eng.finish()


def assert_equal_results(got, want):
    assert got.n_frames == want.n_frames
    np.testing.assert_array_equal(got.counts, want.counts)
    np.testing.assert_array_equal(got.sums, want.sums)


def two_sheets(n, pbc, seed=0):
    """n two-bead molecules (head, tail) on two flat sheets 3 nm apart, 0.7 nm between neighbours (0.3 nm above 300
    molecules); molecules 0 and 1 are in the upper sheet (n > 2), which holds 60 % of them
    -> (tables, frame [2 n, 3], box [3], sides).  The builder of test_spectral_gpu.py, restated."""
    rng = np.random.default_rng(seed)
    sp = 0.7 if n <= 300 else 0.3
    n_up = 1 if n == 2 else max(2, (3 * n + 4) // 5)
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
               leaflets=Leaflets(method=LEAFLETS_CLUSTERING, membrane=heads.copy(), frequency=1))
    return t, frame, np.array([L, L, 12.0], dtype=np.float32), sides


def box9(box, n):
    b = np.zeros((n, 3, 3), dtype=np.float32)
    b[:, 0, 0], b[:, 1, 1], b[:, 2, 2] = box
    return b


@pytest.mark.parametrize("pbc", [True, False])
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 257, 1030])
def test_small_groups(built, n, pbc):
    """Krylov exhaustion (2, 3), the wave and row-tile edges, more than one workgroup a frame (1030): flags equal the dense
    handle's and the helper's, the result EQUAL to the dense handle's and the oracle's."""
    torch_cuda()
    t, frame, box, sides = two_sheets(n, pbc)
    res = sr.classify(frame, t.leaflets.membrane, box, pbc)
    want = sr.molecule_flags(t, res)
    if n != 3:      # three heads: the 2-means decides the third row on a tie (test_spectral_gpu.py::test_minimal_groups)
        np.testing.assert_array_equal(want, sides)
    bx, fi = (box9(box, 1) if pbc else None), np.array([0])
    dense, cut = HipEngine(t), HipEngine(with_flag(t))
    dense.submit_host(frame[None], bx, fi)
    cut.submit_host(frame[None], bx, fi)
    flags, at = cut.leaflets()
    stt, std = cut.clustering_stats(), dense.clustering_stats()
    print(n, pbc, stt, std)
    np.testing.assert_array_equal(flags, want)
    np.testing.assert_array_equal(flags, dense.leaflets()[0])
    assert at == 0 and stt["n_upper"] == std["n_upper"] and stt["n_lower"] == std["n_lower"]
    assert stt["steps"] <= min(n - 1, 300) and np.isnan(stt["o_up"]) and np.isnan(stt["o_lo"])
    got = cut.finish()
    assert_equal_results(got, dense.finish())
    assert_equal_results(got, oracle_route(t, frame[None], bx, fi, {0: want}))


def test_short_box_edges(built):
    """20 x 8 x 16 nm: three cells along x, one along y, two along z — the walked-once rule and an edge below 2 r_c."""
    torch_cuda()
    system, sides = synthetic.cg_buckled(**sr.BUCKLED)
    t = system.tables
    xyz, box, fi = system.frames(2, seed=1), system.box9(2), np.arange(2)
    dense, cut = HipEngine(t), HipEngine(with_flag(t))
    dense.submit_host(xyz, box, fi)
    cut.submit_host(xyz, box, fi)
    np.testing.assert_array_equal(cut.leaflets()[0], sides)
    np.testing.assert_array_equal(cut.leaflets()[0], dense.leaflets()[0])
    group = t.leaflets.membrane
    r32, r64 = sr.classify(xyz[1], group, box[1], True, np.float32), sr.classify(xyz[1], group, box[1], True, np.float64)
    np.testing.assert_array_equal(r32["upper"], r64["upper"])
    gap = float(np.abs(r32["eig"] - r64["eig"]).max())
    stt = cut.clustering_stats()
    dev = float(np.abs(stt["eigenvalues"].astype(np.float64) - r64["eig"]).max())
    print("float32 twin against float64 twin:", gap, "device (cut-off) against float64 twin:", dev, stt, r64["eig"])
    assert dev <= 4 * gap
    flags_of = {k: sr.molecule_flags(t, r) for k, r in sr.run(t, xyz, box, fi).items()}
    got = cut.finish()
    assert_equal_results(got, dense.finish())
    assert_equal_results(got, oracle_route(t, xyz, box, fi, flags_of))


def test_four_or_more_cells(built):
    """40 x 14 x 16 nm: six cells along x, so a row's walk leaves cells out."""
    torch_cuda()
    system, sides = synthetic.cg_buckled(**LARGE)
    t = system.tables
    xyz, box, fi = system.frames(1, seed=1), system.box9(1), np.arange(1)
    dense, cut = HipEngine(t), HipEngine(with_flag(t))
    dense.submit_host(xyz, box, fi)
    cut.submit_host(xyz, box, fi)
    print(cut.clustering_stats(), dense.clustering_stats())
    np.testing.assert_array_equal(cut.leaflets()[0], sides)
    np.testing.assert_array_equal(cut.leaflets()[0], dense.leaflets()[0])
    assert_equal_results(cut.finish(), dense.finish())


def test_above_the_dense_bound(built):
    """8400 heads: refused without the flag; with it both frames' flags are the construction's, frame 1 is matched against
    frame 0, and the sums EQUAL the oracle's.  (Eigenvalues 3 and 4 of L are nearly double here: not asserted.)"""
    torch_cuda()
    system, sides = synthetic.cg_buckled(**ABOVE)
    t = system.tables
    assert len(t.leaflets.membrane) == 8400 > sr.MAX_GROUP
    with pytest.raises(abi.GorderHipError) as e:
        HipEngine(t)
    assert e.value.status == abi.ERR_INVALID_ARGUMENT and str(sr.MAX_GROUP) in str(e.value)
    xyz, box, fi = system.frames(2, seed=1), system.box9(2), np.arange(2)
    cut = HipEngine(with_flag(t))
    cut.submit_host(xyz[:1], box[:1], fi[:1])
    np.testing.assert_array_equal(cut.leaflets()[0], sides)
    cut.submit_host(xyz[1:], box[1:], fi[1:])
    flags, at = cut.leaflets()
    stt = cut.clustering_stats()
    print(stt)
    np.testing.assert_array_equal(flags, sides)
    assert at == 1 and max(float(stt["o_up"]), float(stt["o_lo"])) >= 0.8
    assert_equal_results(cut.finish(), oracle_route(t, xyz, box, fi, {0: sides, 1: sides}))


def test_batching_independence(built):
    """Six frames, assignment every second: one submit == submits of 1, 2 and 3 frames — collected rows, the last frame's
    statistics and the sums identical."""
    torch_cuda()
    system, sides = synthetic.cg_buckled(frequency=2, **sr.BUCKLED)
    t = with_flag(system.tables)
    n = 6
    xyz, box, fi = system.frames(n, seed=1), system.box9(n), np.arange(n)
    runs = []
    for step in (n, 1, 2, 3):
        eng = HipEngine(t)
        eng.set_collect(COLLECT_LEAFLETS)
        for lo in range(0, n, step):
            eng.submit_host(xyz[lo:lo + step], box[lo:lo + step], fi[lo:lo + step])
        res = eng.finish()
        runs.append((eng.collected_leaflets(), eng.clustering_stats(), res))
    (rows0, frames0), st0, res0 = runs[0]
    assert list(frames0) == [0, 2, 4]
    for k in range(3):
        np.testing.assert_array_equal(rows0[k], sides)
    for (rows, frames), stt, res in runs[1:]:
        np.testing.assert_array_equal(rows, rows0)
        np.testing.assert_array_equal(frames, frames0)
        for q in st0:
            assert np.array_equal(st0[q], stt[q], equal_nan=True), q
        assert_equal_results(res, res0)


def test_errors(built):
    torch_cuda()
    t, frame, box, sides = two_sheets(65, True)
    tc = with_flag(t)

    def status_of(tables):
        with pytest.raises(abi.GorderHipError) as e:
            HipEngine(tables)
        return e.value.status, str(e.value)

    bad = np.stack([frame] * 4)
    bad[2, 2 * 7, 1] = np.nan
    eng = HipEngine(tc)
    eng.submit_host(bad, box9(box, 4), np.arange(4))
    with pytest.raises(abi.GorderHipError) as e:
        eng.finish()
    assert e.value.status == abi.ERR_CLUSTERING and e.value.frame == 2
    eng = HipEngine(tc)
    with pytest.raises(abi.GorderHipError) as e:
        eng.submit_host(frame[None], box9(box, 1), np.array([3]))              # a later frame, nothing held
    assert e.value.status == abi.ERR_LEAFLETS_NOT_PRIMED
    glob = copy.deepcopy(tc)
    glob.leaflets = Leaflets(method=LEAFLETS_GLOBAL, normal_dim=2, frequency=1, membrane=np.arange(130, dtype=np.uint32))
    assert status_of(copy.copy(glob))[0] == abi.ERR_INVALID_ARGUMENT           # the flag with another method
    big = copy.deepcopy(tc)                                                    # one above the bound: index arrays only
    extra = scr.MAX_GROUP + 1 - 65
    big.n_atoms = 2 * 65 + extra
    big.leaflets.membrane = np.concatenate([big.leaflets.membrane, np.arange(130, 130 + extra)]).astype(np.uint32)
    assert len(big.leaflets.membrane) == scr.MAX_GROUP + 1
    status, text = status_of(big)
    assert status == abi.ERR_INVALID_ARGUMENT and str(scr.MAX_GROUP) in text
