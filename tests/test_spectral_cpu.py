"""The CPU statement of spectral-clustering leaflets (tests/spectral_ref.py) on the inputs the GPU tests use: the inputs are
fair — the float32 and float64 twins agree on every molecule and give the sides the construction (or the z coordinate
of a flat bilayer) gives — and the orientation rules reproduce the reference's unit-test facts."""
import numpy as np
import pytest

import spectral_ref as sr
from golden_util import Fixture
from gorder_amd import abi, synthetic


def z_sides(frame, heads):
    z = frame[heads, 2]
    return z > z.mean()


@pytest.mark.parametrize("pbc", [True, False])
@pytest.mark.parametrize("name,head", [("cg", "PO4"), ("pcpepg", "P")])
def test_flat_fixtures_follow_z(name, head, pbc):
    """Every frame, both twins: every head on the side its z coordinate gives (both leaflets hold the same number of
    heads; the tie goes to the cluster of the first head)."""
    fx = Fixture(name)
    heads = np.flatnonzero(fx.name_in(head))
    for k in range(len(fx.xyz)):
        got = [sr.classify(fx.xyz[k], heads, fx.boxes[k].reshape(-1), pbc, dt)["upper"] for dt in (np.float32, np.float64)]
        np.testing.assert_array_equal(got[0], got[1])
        above = z_sides(fx.xyz[k], heads)
        c1, c2 = np.flatnonzero(above), np.flatnonzero(~above)          # the z split, oriented by the ab-initio rule
        upper, _ = sr.classify_ab_initio(c1, c2, 0 if above[0] else 1)
        np.testing.assert_array_equal(np.flatnonzero(got[0]), sorted(upper))


def test_buckled_membrane_needs_clustering():
    """synthetic.cg_buckled(**BUCKLED): a plane misplaces molecules, both twins equal the construction for every molecule."""
    system, sides = synthetic.cg_buckled(**sr.BUCKLED)
    xyz = system.frames(2, seed=1)
    heads = np.asarray(system.tables.leaflets.membrane)
    for k in range(2):
        plane = np.where(z_sides(xyz[k], heads), 0, 1)
        assert 50 < (plane != sides).sum() < len(sides) - 50
        for dt in (np.float32, np.float64):
            res = sr.classify(xyz[k], heads, system.box, True, dt)
            np.testing.assert_array_equal(sr.molecule_flags(system.tables, res), sides)


def test_reference_unit_test_facts():
    kat = sr.load_kat()
    pick = lambda f, got: None if got is None else ("cluster1" if got[0] == set(f["cluster1"]) else "cluster2")
    for key in ("ab_initio_unequal", "ab_initio_equal"):
        f = kat[key]
        assert pick(f, sr.classify_ab_initio(f["cluster1"], f["cluster2"], f["min_index_cluster"])) == f["upper"]
    e = kat["ab_initio_equal"]
    ref_upper, ref_lower = sr.classify_ab_initio(e["cluster1"], e["cluster2"], e["min_index_cluster"])
    for key in ("matching_perfect", "matching_small_mismatch", "matching_large_mismatch"):
        f = kat[key]
        got = sr.classify_by_match(ref_upper, ref_lower, f["cluster1"], f["cluster2"])
        assert pick(f, got) == f["upper"]
        if got is not None:      # the clusters handed over in the other order: the same leaflets
            assert sr.classify_by_match(ref_upper, ref_lower, f["cluster2"], f["cluster1"]) == got


def test_names_of_the_interface():
    assert abi.LEAFLETS_CLUSTERING == 6 and abi.ERR_CLUSTER_MATCH == 108
    assert "gorder_hip_clustering_stats" in abi._EXPORTS
    assert sr.MIN_GROUP == 2 and sr.MAX_GROUP >= 5000
