"""Radial profiles without a device: the thresholds k_bonds_shells compares against, the profile arithmetic, the text
layout, and the new entry points of the library and of HipEngine."""
import numpy as np

from gorder_amd import abi, writers
from gorder_amd import structure as st
from gorder_amd.abi import Results

TEST_RADII = [0.7, 1.5, 2.2, 3.1, 1.5, 2.5, 3.5, 4.5, 0.75, 1.5, 2.5, 3.25, 0.9, 1.7, 2.5] + [0.2 * (k + 1) for k in range(32)]


def test_thresholds_are_the_references_square_root_test(built):
    """d2 < thr is exactly sqrt(f32 d2) < r (numpy's float32 square root is IEEE's, correctly rounded) for the floats at and
    around every threshold: two ulps either side."""
    rng = np.random.default_rng(5)
    radii = np.concatenate([np.exp(rng.uniform(np.log(0.01), np.log(50.0), 200)), TEST_RADII]).astype(np.float32)
    thr = abi.radial_thresholds(radii)
    assert thr.dtype == np.float32 and thr.shape == radii.shape
    inf = np.float32(np.inf)
    for r, t in zip(radii, thr):
        around = [t, np.nextafter(t, inf), np.nextafter(t, -inf)]
        around += [np.nextafter(around[1], inf), np.nextafter(around[2], -inf)]
        for d2 in around:
            assert d2 >= 0
            assert bool(d2 < t) == bool(np.sqrt(np.float32(d2)) < r), (r, t, d2)
    assert (np.diff(abi.radial_thresholds(np.sort(radii))) >= 0).all()
    assert abi.radial_thresholds([0.0, -1.0]).tolist() == [0.0, 0.0]


def shell(sums, counts):
    return Results(np.array(sums, dtype=np.int64), np.array(counts, dtype=np.uint64), 3)


def test_radial_profile_arithmetic():
    # 3 slots; groups: slot 0 alone, slots 1 and 2 together
    shells = [shell([[-7, 10, 5], [-7, 0, 5], [0, 10, 0]], [[2, 3, 1], [2, 0, 1], [0, 3, 0]]),
              shell([[0, -1000001, -1000000], [0, 0, 0], [0, -1000001, -1000000]], [[0, 1, 2], [0, 0, 0], [0, 1, 2]])]
    groups = [[0], [1, 2]]
    cg = st.radial_profile(shells, [1.0, 2.0], groups, "cg")
    assert cg.dtype == np.float32 and cg.shape == (2, 3, 2)
    f = np.float32
    # truncation toward zero on a negative sum: -7 / 2 -> -3 ticks (a floor would give -4)
    assert cg[0, 0, 0] == f(-3 / 1e6) and cg[0, 1, 0] == f(-3 / 1e6) and np.isnan(cg[0, 2, 0])
    # a group of several slots is added before the division: (10 + 5) / (3 + 1) -> 3 ticks (the slots' own means are 3 and 5)
    assert cg[1, 0, 0] == f(3 / 1e6) and cg[1, 1, 0] == f(5 / 1e6) and cg[1, 2, 0] == f(3 / 1e6)
    # (-1000001 - 1000000) / 3 -> -666667 ticks
    assert cg[1, 0, 1] == f(-666667 / 1e6) and np.isnan(cg[0, 0, 1]) and np.isnan(cg[1, 1, 1])
    # negated for "aa"
    aa = st.radial_profile(shells, [1.0, 2.0], groups, "aa")
    assert aa[0, 0, 0] == f(3 / 1e6) and aa[1, 0, 1] == f(666667 / 1e6) and np.isnan(aa[0, 2, 0])
    # NaN below min_samples: 4 samples pass 4 and fail 5
    assert st.radial_profile(shells, [1.0, 2.0], groups, "cg", min_samples=4)[1, 0, 0] == f(3 / 1e6)
    lim = st.radial_profile(shells, [1.0, 2.0], groups, "cg", min_samples=5)
    assert np.isnan(lim).all()
    counts = st.radial_counts(shells, groups)
    assert counts.dtype == np.uint64 and counts[:, 0, :].tolist() == [[2, 0], [4, 3]]


def test_radial_profile_text():
    nan = float("nan")
    values = np.array([[[0.12344, 0.2, nan], [0.1, nan, nan], [0.15, 0.25, nan]],
                       [[-0.05, 0.0, 1.0], [-0.5, 0.33336, 0.5], [nan, nan, nan]]], dtype=np.float32)
    text = writers.radial_profile_text(values, None, [0.5, 1.25, 2.0], ["POPC", "POPE C1"], header="# made by a test")
    assert text == """# made by a test
# shell k holds the samples at distance r_inner <= d < r_outer [nm] from the reference of the selection
# column 1: r_inner
# column 2: r_outer
# column 3: POPC full
# column 4: POPC upper
# column 5: POPC lower
# column 6: POPE C1 full
# column 7: POPE C1 upper
# column 8: POPE C1 lower
0.0000 0.5000   0.1234   0.1000   0.1500  -0.0500  -0.5000      NaN
0.5000 1.2500   0.2000      NaN   0.2500   0.0000   0.3334      NaN
1.2500 2.0000      NaN      NaN      NaN   1.0000   0.5000      NaN
"""
    counts = np.arange(18, dtype=np.uint64).reshape(2, 3, 3)
    rows = writers.radial_profile_text(values, counts, [0.5, 1.25, 2.0], ["a", "b"]).splitlines()
    assert rows[0] == "# radial profile of order parameters" and "# column 6: a samples" in rows and "# column 10: b samples" in rows
    assert rows[-1] == "1.2500 2.0000      NaN      NaN      NaN 2   1.0000   0.5000      NaN 11"


def test_entry_points_exist(built):
    lib = abi.load_library()
    for name in ("gorder_hip_set_radial_shells", "gorder_hip_radial_shells", "gorder_hip_radial_thresholds"):
        assert hasattr(lib, name) and name in abi._EXPORTS
    assert abi.RADIAL_MAX_SHELLS == 32
    assert callable(abi.HipEngine.set_radial_shells) and callable(abi.HipEngine.radial_shells)
    assert callable(abi.radial_thresholds)
