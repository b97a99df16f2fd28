"""Order distributions without a GPU: the bin search and the edge check of gorder_amd/csrc/order_hist.h and the route of the
order pass with OrderRouteIn::dist set through a stand-alone program (tests/cabi/order_hist.cpp; built plainly and with the
address and undefined-behaviour sanitizers, both binaries run directly), and the Python side: structure.order_edges,
structure.tilt_edges, structure.histogram_groups, structure.order_density, writers.order_histogram_text."""
import os
import subprocess

import numpy as np
import pytest

from gorder_amd import structure, writers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gorder_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def compile_driver(directory, flags):
    exe = str(directory / "order_hist")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", *flags, f"-I{CSRC}", os.path.join(ROOT, "tests", "cabi", "order_hist.cpp"), "-o", exe])

    def run(*args):
        res = subprocess.run([exe, *map(str, args)], capture_output=True, timeout=300)
        err = res.stderr.decode()
        assert res.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, res.stdout.decode() + err
        return res.stdout.decode()
    return run


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("order_hist_" + request.param), SANITIZE if request.param == "sanitized" else [])


EDGE_SETS = {
    "two": np.array([-500000, 1000001]),
    "257": -500000 + 5859 * np.arange(257),                     # 256 bins: the most the ABI takes
    "uniform": structure.order_edges(16),
    "tilt": structure.tilt_edges(90)[0],
    "three": np.array([-3, 0, 3]),                              # an odd count: the search's last step is a partial one
    "limits": np.array([-2**31, 0, 2**31 - 1]),
}


# ---- 1. the bin search ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EDGE_SETS))
def test_hist_bin_against_searchsorted(driver, tmp_path, name):
    edges = np.asarray(EDGE_SETS[name], dtype=np.int64)
    path = tmp_path / "edges.txt"
    path.write_text("".join(f"{int(e)}\n" for e in edges))
    got = np.array([line.split() for line in driver("bins", path).splitlines()], dtype=np.int64)
    ticks, bins = got[:, 0], got[:, 1]
    assert len(ticks) >= min(3 * len(edges), 6) and {-500000, 1000000} <= set(ticks.tolist())
    want = np.searchsorted(edges, ticks, "right") - 1
    want[want == len(edges) - 1] = -1                           # at or above the last edge: in no bin
    np.testing.assert_array_equal(bins, want)
    # both sides of the half-open rule on every inner edge, and the two ends
    for k, e in enumerate(edges.tolist()):
        at = {int(t): int(b) for t, b in zip(ticks, bins)}
        assert at[e] == (k if k < len(edges) - 1 else -1)
        if e - 1 in at:
            assert at[e - 1] == k - 1
    if name in ("uniform", "tilt", "two"):
        assert bins[ticks == -500000][0] == 0 and bins[ticks == 1000000][0] == len(edges) - 2


def test_edge_check_names_what_is_wrong(driver):
    got = dict(line.split(": ", 1) for line in driver("check").splitlines())
    assert got["two"] == "ok" and got["257"] == "ok" and got["limits"] == "ok"
    for case, word in [("one", "fewer than 2"), ("none", "fewer than 2"), ("258", "GORDER_HIST_MAX_BINS"), ("equal", "ascending"),
                       ("descending", "ascending"), ("null", "no edges")]:
        assert word in got[case], (case, got[case])


# ---- 2. the route ---------------------------------------------------------------------------------------------------------
def test_route_with_a_histogram(driver):
    lines = driver("route").splitlines()
    assert len(lines) == 1 << 14
    DIST, NONE = 8, 0
    seen_plain = set()
    for line in lines:
        left, plain_family = line.split(" | ")
        i, family, label, npf, mom, spec, extras, by_slot, ua_mode, direct = left.split()
        i = int(i)
        bond_tiles, npf5 = i & 1, (i >> 10) & 1
        if not bond_tiles:
            assert int(family) == NONE and label == "-"
        else:
            assert int(family) == DIST and label == "k_bonds_dist"
        # never speculative (global leaflets take the two-kernel path), the items in tile order, launched from the extras' loop
        assert (int(mom), int(spec), int(extras), int(by_slot), int(ua_mode), int(direct)) == (0, 0, 1, 0, -1, 0), line
        assert int(npf) == (5 if npf5 else 4)
        seen_plain.add(int(plain_family))
    # the same facts without the histogram take the plain kernels or, with a selection, k_bonds_extras
    assert seen_plain == {0, 1, 2, 5}


def test_chunks_keep_the_epilogue_small(driver):
    got = {tuple(map(int, line.split("->")[0].split())): tuple(map(int, line.split("->")[1].split())) for line in driver("chunks").splitlines()}
    for (frames, tiles, target, words, per_word), (fpc, n_chunks) in got.items():
        assert 1 <= fpc <= min(frames, 1 << 23) and n_chunks == -(-frames // fpc)
        # at least per_word samples (256 a frame) per table word, unless the whole range is shorter
        assert fpc * 256 >= per_word * words or fpc == frames
    assert got[(4000, 64, 0, 11520, 8)] == (360, 12) and got[(4000, 64, 1, 11520, 8)] == (4000, 1)
    assert got[(20000000, 1, 1, 64, 8)] == (1 << 23, 3)          # a u32 table word cannot overflow
    # the direct route has no table, and 0 samples per word asks for none: the extras' chunks
    assert got[(4000, 64, 0, 0, 8)] == got[(4000, 64, 0, 11520, 0)] == (16, 250)
    assert got[(4000, 64, 0, 11520, 65536)] == (4000, 1)


# ---- 3. Python ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [1, 7, 16, 150, 256])
def test_order_edges(n_bins):
    e = structure.order_edges(n_bins)
    assert e.dtype == np.int32 and len(e) == n_bins + 1 and e[0] == -500000 and e[-1] == 1000001
    assert (np.diff(e.astype(np.int64)) > 0).all()
    assert np.abs(np.diff(e[:-1].astype(np.int64)) - 1500000 / n_bins).max() < 1 if n_bins > 1 else True
    with pytest.raises(ValueError):
        structure.order_edges(257)


def test_tilt_edges():
    e, a = structure.tilt_edges(90)
    assert e.dtype == np.int32 and len(e) == len(a) == 91 and e[0] == -500000 and e[-1] == 1000001
    assert (np.diff(e.astype(np.int64)) > 0).all() and (np.diff(a) == -1.0).all() and a[0] == 90.0 and a[-1] == 0.0
    c = np.cos(np.deg2rad(a[1:-1]))
    np.testing.assert_array_equal(e[1:-1], np.rint(1e6 * (1.5 * c * c - 0.5)).astype(np.int64))
    assert e[45] == 250000                                       # 45 degrees: S = 0.25
    assert (np.diff(structure.tilt_edges(256)[0].astype(np.int64)) > 0).all()
    with pytest.raises(ValueError):
        structure.tilt_edges(0)


def test_histogram_groups_add_slots():
    rng = np.random.default_rng(3)
    hist = rng.integers(0, 1 << 40, size=(5, 3, 7)).astype(np.uint64)
    groups = [[0, 1, 2], [6], [3, 5]]
    got = structure.histogram_groups(hist, groups)
    assert got.dtype == np.uint64 and got.shape == (3, 3, 5)
    for g, slots in enumerate(groups):
        for w in range(3):
            for k in range(5):
                assert int(got[g, w, k]) == sum(int(hist[k, w, s]) for s in slots)
    with pytest.raises(ValueError):
        structure.histogram_groups(hist[:, :2], groups)


@pytest.mark.parametrize("analysis", ["aa", "ua", "cg"])
def test_density_integrates_to_one(analysis):
    rng = np.random.default_rng(4)
    edges, _ = structure.tilt_edges(90)
    counts = rng.integers(0, 1000, size=(2, 3, 90)).astype(np.uint64)
    counts[1, 2] = 0                                             # no sample in any bin: NaN, not a division error
    density, lo, hi = structure.order_density(counts, edges, analysis)
    assert density.shape == counts.shape and (np.diff(lo) > 0).all() and (hi > lo).all()
    integral = (density * (hi - lo)).sum(axis=-1)
    np.testing.assert_allclose(integral[counts.sum(axis=-1) > 0], 1.0, rtol=1e-12)
    assert np.isnan(density[1, 2]).all()
    if analysis == "cg":
        assert lo[0] == -0.5 and hi[-1] == 1.000001
        np.testing.assert_allclose(density[0, 0, 0], counts[0, 0, 0] / counts[0, 0].sum() / (hi[0] - lo[0]))
    else:                                                        # -S: the bins reversed
        assert hi[-1] == 0.5 and lo[0] == -1.000001
        np.testing.assert_allclose(density[0, 0, -1], counts[0, 0, 0] / counts[0, 0].sum() / (hi[-1] - lo[-1]))
    with pytest.raises(ValueError):
        structure.order_density(counts[..., :89], edges, analysis)


def test_text_round_trips_the_counts():
    rng = np.random.default_rng(6)
    edges, angles = structure.tilt_edges(9)
    counts = rng.integers(0, 1 << 50, size=(2, 3, 9)).astype(np.uint64)
    for with_angles in (False, True):
        text = writers.order_histogram_text(counts, edges, ["POPC", "POPE"], angles if with_angles else None)
        assert text.endswith("\n")
        rows = [ln.split() for ln in text.splitlines() if not ln.startswith("#")]
        assert len(rows) == 9
        skip = 4 if with_angles else 2
        back = np.array([[int(x) for x in r[skip:]] for r in rows], dtype=np.uint64).reshape(9, 2, 3).transpose(1, 2, 0)
        np.testing.assert_array_equal(back, counts)
        np.testing.assert_array_equal([int(r[0]) for r in rows], edges[:-1])
        np.testing.assert_array_equal([int(r[1]) for r in rows], edges[1:])
        names = [ln for ln in text.splitlines() if ln.startswith("# column")]
        assert len(names) == skip + 6 and names[-1] == f"# column {skip + 6}: POPE lower"
        if with_angles:
            assert rows[0][2] == "90.0000" and rows[-1][3] == "0.0000"
    assert writers.order_histogram_text(counts, edges, ["a", "b"], header="# mine").splitlines()[0] == "# mine"
    with pytest.raises(ValueError):
        writers.order_histogram_text(counts, edges[:-1], ["a", "b"])
    with pytest.raises(ValueError):
        writers.order_histogram_text(counts, edges, ["a"])
