"""Spherical-clustering leaflets without a GPU: the CPU statement of the method (tests/spherical_ref.py) against the
reference's own unit-test known answers, the vesicle generator, and the host-side interface of the new method."""
import os
import re

import numpy as np
import pytest

import spherical_ref as sr
from gorder_amd import abi, synthetic
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clusters_known_answer(built):
    k = sr.load_kat()["clusters_from_responsibilities"]
    for dtype in (np.float32, np.float64):
        upper = sr.clusters_from_responsibilities(k["responsibilities"], k["distances"], dtype)
        assert sorted(np.flatnonzero(upper)) == k["upper"] and sorted(np.flatnonzero(~upper)) == k["lower"]


def test_empty_cluster_rule(built):
    """One cluster empty: its mean is NaN, `cluster1 > cluster2` is false, cluster 2 is upper — whichever is empty."""
    d = [3.0, 4.0, 5.0]
    assert sr.clusters_from_responsibilities([0.9, 0.8, 0.7], d).all()          # all in cluster 2 -> all upper
    assert not sr.clusters_from_responsibilities([0.1, 0.2, 0.3], d).any()      # all in cluster 1 -> cluster 2 (empty) upper


def test_fit_gmm_property(built):
    for case in sr.load_kat()["fit_gmm"]:
        for dtype in (np.float32, np.float64):
            _, resp, _, iters = sr.fit_gmm(case["data"], dtype)
            assert iters <= sr.GMM_MAX_ITERATIONS
            assert np.array_equal(resp > 0.5, np.array(case["component_a"])), case["seed"]
            assert not np.any(resp == 0.5)


def test_min_image_is_the_oracles(built):
    system, _ = sr.make_fixture("v600", centre=(0.3, 0.2, 0.1))
    frame = system.frames(1, seed=3)[0]
    group = system.tables.leaflets.membrane
    centre, dist = sr.distances(frame, group, system.box, True)
    for i in range(0, len(group), 7):
        v = oracle.vector_to(centre, frame[group[i]], system.box, True)
        assert np.float32(np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])) == dist[i]


@pytest.mark.parametrize("name", sr.SEPARATED)
def test_vesicle_sides(built, name):
    """The helper finds the generator's true sides on the separated vesicles, in float32 and float64, wrapped across the
    periodic faces and unwrapped without a box; the recorded float32 / float64 gap is what it measures."""
    system, sides = sr.make_fixture(name)
    t = system.tables
    assert t.leaflets.method == abi.LEAFLETS_SPHERICAL and len(t.leaflets.membrane) == t.n_molecules_total == len(sides)
    assert 0 < sides.sum() < len(sides) and not np.array_equal(np.sort(sides), sides)      # shuffled
    frames = system.frames(sr.GAP_FRAMES, seed=sr.GAP_SEED)
    assert (frames >= 0).all() and (frames <= system.box).all()
    recorded = sr.load_kat()["gaps"][name]
    for k, fr in enumerate(frames):
        a = sr.classify(fr, t.leaflets.membrane, system.box, True, np.float32)
        b = sr.classify(fr, t.leaflets.membrane, system.box, True, np.float64)
        assert np.array_equal(sr.molecule_flags(t, fr, system.box, result=a), sides)
        assert np.array_equal(a["upper"], b["upper"]) and a["iterations"] == b["iterations"]
        assert not np.any((b["resp"] > 0.001) & (b["resp"] < 0.999))
        gap = sr.stats_gap(fr, t.leaflets.membrane, system.box)
        print(name, k, gap, a["iterations"])
        for q in ("centre", "mean", "var", "weight"):
            assert gap[q] <= recorded[q] * 1.5 + 1e-9, (q, gap[q], recorded[q])
    shifted, sides2 = sr.make_fixture(name, centre=(0.3, 0.2, 0.1))
    assert np.array_equal(sides, sides2)
    fr = shifted.frames(1, seed=2)[0]
    assert np.array_equal(sr.molecule_flags(shifted.tables, fr, shifted.box), sides)
    t.handle_pbc = False
    assert np.array_equal(sr.molecule_flags(t, shifted.frames_unwrapped(1, seed=2)[0], None), sides)


def test_overlapping_vesicle_seed(built):
    """The overlapping fixture: about a tenth of the heads between the components, yet no responsibility of the float64
    twin within 1e-3 of 0.5 and the same sides from both twins — the GPU test may then leave out no head on its own."""
    system, _ = sr.make_fixture(sr.OVERLAPPING)
    t = system.tables
    for fr in system.frames(sr.OVERLAP_FRAMES, seed=sr.GAP_SEED):
        a = sr.classify(fr, t.leaflets.membrane, system.box, True, np.float32)
        b = sr.classify(fr, t.leaflets.membrane, system.box, True, np.float64)
        mid = np.mean((b["resp"] > 0.01) & (b["resp"] < 0.99))
        print("overlapping: share between 0.01 and 0.99 =", mid, "iterations", a["iterations"])
        assert 0.05 < mid < 0.2
        assert not np.any(np.abs(b["resp"] - 0.5) <= 1e-3)
        assert np.array_equal(a["upper"], b["upper"]) and a["iterations"] == b["iterations"]


def test_interface(built):
    assert abi.LEAFLETS_SPHERICAL == 5 and abi.ERR_CLUSTERING == 107
    header = open(os.path.join(ROOT, "include", "gorder_hip.h")).read()
    assert re.search(r"GORDER_LEAFLETS_SPHERICAL\s*=\s*5\b", header) and re.search(r"GORDER_ERR_CLUSTERING\s*=\s*107\b", header)
    assert re.search(r"int\s+gorder_hip_spherical_stats\s*\(\s*gorder_hip_handle\s*\*h,\s*float\s+out\[12\]\)", header)
    assert "gorder_hip_spherical_stats" in abi._EXPORTS
    lib = abi.load_library()
    assert lib.gorder_hip_strerror(abi.ERR_CLUSTERING).decode() != "unknown status"
    system, _ = synthetic.cg_vesicle(400, 3.0, 6.0, seed=2)
    plan = abi.plan_tables(system.tables)
    assert plan["selfcheck"] == 0 and plan["leaflets_one_read"] == 0 and plan["n_direct_items"] == 0


def test_build_tables_from_masks(built):
    """build_tables with the method: the group is `heads` restricted to the master atoms — heads of molecules that are not
    analysed stay in it —, one head per analysed molecule."""
    from gorder_amd.structure import Structure, build_tables
    n_mol, per = 6, 3          # chains of three beads: P - A - B; the last two molecules are not analysed (no A / B selected)
    n = n_mol * per
    names = ["P", "A", "B"] * n_mol
    bonds = [[] for _ in range(n)]
    for m in range(n_mol):
        a = m * per
        bonds[a] += [a + 1]; bonds[a + 1] += [a, a + 2]; bonds[a + 2] += [a + 1]
    s = Structure(resids=np.repeat(np.arange(1, n_mol + 1), per), resnames=["LIP"] * n, names=names,
                  box=np.array([10.0, 10.0, 10.0], dtype=np.float32), bonds=bonds)
    sel = np.zeros(n, dtype=bool)
    sel[:4 * per] = True
    heads = np.array([nm == "P" for nm in names])
    tables, labels, midx = build_tables(s, "cg", sel, leaflets={"method": abi.LEAFLETS_SPHERICAL, "heads": heads, "frequency": 5,
                                                               "flip": True})
    lf = tables.leaflets
    assert lf.method == abi.LEAFLETS_SPHERICAL and lf.frequency == 5 and lf.flip
    assert len(lf.membrane) == n_mol                      # every P of the master group, the unanalysed molecules' too
    assert np.array_equal(midx[lf.membrane], np.flatnonzero(heads))
    assert tables.n_molecules_total == 4
    for mt in tables.molecule_types:
        assert set(mt.heads) <= set(lf.membrane)
    assert abi.plan_tables(tables)["selfcheck"] == 0
