"""Shared by the ordermap finalisation tests (test_ordermap_final_cpu.py, test_ordermap_final_gpu.py)."""
import os

import numpy as np

from gorder_amd import writers
from golden_util import GOLDEN, compare_maps, read_map

MAP_DIR = os.path.join(GOLDEN, "expected", "ordermaps_ua")
PLANES = ("full", "upper", "lower")
MIN_SAMPLES = 5                     # of the reference's united-atom ordermap tests (tests_ua.rs:351-507)


def golden_names():
    return sorted(n[:-len(".dat")] for n in os.listdir(MAP_DIR) if n.endswith(".dat"))


def parse_map(text):
    """The `x y value` lines of an ordermap file -> {(x, y): value}, as golden_util.read_map reads a golden."""
    out = {}
    for line in text.splitlines():
        p = line.split()
        if len(p) == 3 and p[0][0] in "0123456789-":
            out[(p[0], p[1])] = float(p[2])
    return out


def golden_values(name, shape):
    """The values of a golden file in file order (x-major) as float32 [nx, ny], and its lines."""
    with open(os.path.join(MAP_DIR, name + ".dat")) as f:
        lines = f.read().split("\n")
    vals = [float(line.split()[2]) for line in lines if line and line[0] in "0123456789-"]
    return np.array(vals, dtype=np.float32).reshape(shape), lines


def same_bits(got, want):
    """Equal float32 arrays bit for bit; every NaN counts as the same NaN."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(nan_g, nan_w)
    g, w = got.view(np.uint32)[~nan_g], want.view(np.uint32)[~nan_w]
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (bad.size, [(hex(g[k]), hex(w[k])) for k in bad[:5]])


def check_goldens(values, groups, om, leaflets):
    """Every golden of the united-atom system that `groups` (structure.ordermap_groups) names, against values
    [n_groups, 3, nx, ny], through the text a user gets, by compare_maps' rule.  Returns the names of the goldens compared."""
    seen = set()
    for vals, group in zip(values, groups):
        for _, stem, comment in group.files:
            for w in range(3 if leaflets else 1):
                got = parse_map(writers.ordermap_text(vals[w], om, "ua", comment))
                bad = compare_maps(got, read_map(f"{stem}_{PLANES[w]}.dat"))
                assert not bad, (stem, PLANES[w], bad[:5])
                seen.add(f"{stem}_{PLANES[w]}")
    return seen
