"""The cut-off route of spectral-clustering leaflets on the reference statement alone (tests/spectral_cutoff_ref.py): the
inputs of tests/test_spectral_cutoff_gpu.py stay inside the conditions under which a 6 nm cut-off changes no label, and the
flag reaches the tables."""
import numpy as np

import spectral_cutoff_ref as scr
import spectral_ref as sr
from gorder_amd import abi, synthetic

LARGE = dict(n_lipids=2000, box=(40.0, 14.0, 16.0), amplitude=3.0, seed=13)
ABOVE = dict(n_lipids=8400, box=(84.0, 28.0, 16.0), amplitude=3.0, seed=13)


def test_flag_constant_and_tables():
    assert abi.FLAG_CLUSTER_CUTOFF == 4
    assert abi.FLAG_CLUSTER_CUTOFF & (abi.FLAG_TRIG_ACOS_COS | abi.FLAG_UA_FAST_NORMALISE) == 0
    system, _ = synthetic.cg_buckled(n_lipids=20, box=(8.0, 8.0, 16.0))
    t = system.tables
    t.flags = abi.FLAG_CLUSTER_CUTOFF
    assert t.as_ctypes()[0].flags == 4
    assert abi.Tables(n_atoms=1, molecule_types=[], flags=abi.FLAG_CLUSTER_CUTOFF).flags == 4
    assert scr.MAX_GROUP == 131072 and sr.MAX_GROUP == 8192


def test_short_box_edges_labels_equal_dense():
    """500 heads in 20 x 8 x 16 nm (an edge below 2 r_c): the truncated W gives the dense statement's labels, both frames."""
    system, sides = synthetic.cg_buckled(**sr.BUCKLED)
    xyz, box = system.frames(2, seed=1), system.box9(2)
    group = system.tables.leaflets.membrane
    for k in range(2):
        dense = sr.classify(xyz[k], group, box[k], True)
        cut = scr.classify(xyz[k], group, box[k], True)
        np.testing.assert_array_equal(cut["labels"], dense["labels"])
        np.testing.assert_array_equal(cut["upper"], dense["upper"])
        np.testing.assert_array_equal(np.where(cut["upper"], 0, 1), sides)
        print("frame", k, "eigenvalues, cut-off against dense:", np.abs(cut["eig"] - dense["eig"]).max())
        assert np.abs(cut["eig"] - dense["eig"]).max() < 1e-6


def test_four_cells_labels_equal_dense():
    """2000 heads in 40 x 14 x 16 nm (six cells along x): labels equal the dense statement's and the construction."""
    system, sides = synthetic.cg_buckled(**LARGE)
    xyz, box = system.frames(1, seed=1), system.box9(1)
    group = system.tables.leaflets.membrane
    dense = sr.classify(xyz[0], group, box[0], True)
    cut = scr.classify(xyz[0], group, box[0], True)
    np.testing.assert_array_equal(cut["labels"], dense["labels"])
    np.testing.assert_array_equal(np.where(cut["upper"], 0, 1), sides)


def test_above_the_dense_bound_labels_equal_construction():
    """8400 heads in 84 x 28 x 16 nm, float64 sparse statement: the separation is the construction's on both frames."""
    system, sides = synthetic.cg_buckled(**ABOVE)
    xyz, box = system.frames(2, seed=1), system.box9(2)
    group = system.tables.leaflets.membrane
    assert len(group) == 8400 > sr.MAX_GROUP
    for k in range(2):
        res = scr.classify_sparse(xyz[k], group, box[k], True)
        print("frame", k, "eigenvalues of L:", res["eig"], "populations:", res["n_cluster"], "rounds:", res["rounds"])
        assert sorted(res["n_cluster"]) == [4200, 4200]
        np.testing.assert_array_equal(np.where(res["upper"], 0, 1), sides)
