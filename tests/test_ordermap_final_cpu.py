"""Ordermap finalisation without a GPU: the tile arithmetic and the group validation of gorder_amd/csrc/ordermap_final.h driven
by a stand-alone program under the address and undefined-behaviour sanitizers, structure.ordermap_values and the writers on
the oracle's united-atom maps against the reference's 36 ordermap files, the names of structure.ordermap_groups, the directory
tree, and the new entry point of the built library."""
import os
import re
import subprocess

import numpy as np
import pytest

from gorder_amd import abi, writers
from gorder_amd import structure as st
from golden_util import Fixture, aa_setup, cg_setup
from oracle import oracle
from test_golden_oracle import master_frames, ordermap_setup
import ordermap_final_util as ou

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tile_cases():
    """(sum, count, min_samples, negate): sums of both signs that do not divide their count, a zero sum, counts around
    min_samples, counts that f32 cannot hold, sums that f64 cannot hold or whose quotient by 1e6 is far from a float."""
    sums = [7, -7, 1234567, -999999, 1, -1, 0, 333333333, -2 ** 31 - 5,
            2 ** 53 // 1000 + 1, -(2 ** 53 // 1000 + 7), 2 ** 53 + 1, -(2 ** 53 + 3), 2 ** 62 + 12345, -(2 ** 62 + 54321)]
    counts = [0, 1, 2, 3, 4, 5, 13, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 32 + 12345, 2 ** 40 + 1, 2 ** 63 + 2 ** 39 + 1]
    return [(s, c, m, neg) for s in sums for c in counts for m in (1, 5) for neg in (0, 1)]


def restated(s, c, min_samples, negate):
    if c < min_samples:
        return np.float32(np.nan)
    v = np.float32(np.float64(s) / 1e6) / np.float32(np.uint64(c))
    return np.float32(-v) if negate else np.float32(v)


def test_host_arithmetic_under_sanitizers(tmp_path):
    exe, cases_file = str(tmp_path / "ordermap_final"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", f"-I{os.path.join(ROOT, 'gorder_amd', 'csrc')}",
                           os.path.join(ROOT, "tests", "cabi", "ordermap_final.cpp"), "-o", exe])
    cases = tile_cases()
    with open(cases_file, "w") as f:
        f.write("".join(f"{s} {c} {m} {neg}\n" for s, c, m, neg in cases))
    res = subprocess.run([exe, cases_file], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ordermap_final ok" in res.stdout and "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    got = res.stdout.split()[:-2]
    assert len(got) == len(cases)
    n_numbers = 0
    for case, word in zip(cases, got):
        want = restated(*case)
        if np.isnan(want):
            assert np.isnan(np.array([int(word, 16)], dtype=np.uint32).view(np.float32)[0]), case
        else:
            assert int(word, 16) == int(np.array([want], dtype=np.float32).view(np.uint32)[0]), (case, word, want)
            n_numbers += 1
    assert n_numbers > len(cases) // 2
    # the cases do tell the converter's f32 division from calc_order's truncating one, and -0.0 from 0.0
    assert restated(-7, 2, 1, 0) != np.float32(st._mean_ticks(-7, 2))
    assert np.signbit(restated(0, 3, 1, 1)) and not np.signbit(restated(0, 3, 1, 0))


@pytest.fixture(scope="module")
def ua(built):
    return Fixture("ua")


@pytest.fixture(scope="module")
def oracle_maps(ua):
    """(res, labels, om) of the oracle on the reference's united-atom ordermap analysis, per leaflets switch, made once."""
    cache = {}

    def run(leaflets):
        if leaflets not in cache:
            tables, labels, midx, om = ordermap_setup(ua, leaflets=leaflets)
            frames = ua.window()
            eng = oracle.OracleEngine(tables, trig=oracle.TRIG_LIBM, n_threads=3)
            eng.submit(master_frames(ua, midx, frames), ua.boxes[frames], frames)
            cache[leaflets] = (eng.finish(), labels, om)
        return cache[leaflets]
    return run


@pytest.mark.parametrize("leaflets", [False, True])
def test_ordermap_values_reproduce_the_goldens(oracle_maps, leaflets):
    res, labels, om = oracle_maps(leaflets)
    groups = st.ordermap_groups(labels, "ua")
    values = st.ordermap_values(res, [g.slots for g in groups], ou.MIN_SAMPLES, negate=True)
    assert values.shape == (len(groups), 3, 14, 4) and values.dtype == np.float32
    seen = ou.check_goldens(values, groups, om, leaflets)
    names = ou.golden_names()
    assert len(names) == 36
    assert seen == (set(names) if leaflets else {n for n in names if n.endswith("_full")})
    if not leaflets:
        assert np.isnan(values[:, 1:]).all()                  # no upper or lower plane without leaflets
    # the restatement tile by tile, in Python integers
    s = res.map_sums[:, groups[1].slots].sum(axis=1)
    c = res.map_counts[:, groups[1].slots].sum(axis=1)
    want = np.array([restated(int(a), int(b), ou.MIN_SAMPLES, 1) for a, b in zip(s.ravel(), c.ravel())]).reshape(s.shape)
    ou.same_bits(values[1], want)
    with pytest.raises(ValueError):
        st.ordermap_values(res, [[0]], 0)


@pytest.mark.parametrize("stem,comment_has,has_nan", [("ordermap_POPC-C50-49--POPC-H2-49", "virtual hydrogen #2", True),
                                                      ("ordermap_POPC-C20-19", "an atom type POPC-C20-19", True),
                                                      ("ordermap_average", "a molecule type POPC", False)])
def test_ordermap_text_gives_a_golden_back(oracle_maps, stem, comment_has, has_nan):
    _, labels, om = oracle_maps(True)
    files = {(sub, s): c for g in st.ordermap_groups(labels, "ua") for sub, s, c in g.files}
    comment = files["POPC", stem]
    assert comment_has in comment
    some_nan = False
    for plane in ou.PLANES:
        values, lines = ou.golden_values(f"{stem}_{plane}", (14, 4))
        some_nan |= bool(np.isnan(values).any())
        text = writers.ordermap_text(values, om, "ua", comment)
        got = text.split("\n")
        assert got[0] == lines[0]                              # the reference's own comment
        assert got[1].startswith("# Calculated with '") and got[1] != lines[1]
        assert got[2:] == lines[2:]                            # byte for byte from the third line on
        assert text.endswith("\n") and len(got) == 8 + 56 + 1
    assert some_nan == has_nan                                 # the bond's and the atom's maps have tiles below min_samples


def test_ordermap_text_of_other_planes_analyses_and_special_values():
    om = abi.OrderMap(enabled=True, plane=2, span_x=(-1.0, 0.0), span_y=(0.25, 1.0), bin=(0.5, 0.25))
    values = np.array([[np.nan, -0.0, 0.0], [0.12345, -0.99995, 1.0]], dtype=np.float32)
    text = writers.ordermap_text(values, om, "cg", "# a comment", calculated_with="this test")
    assert text == ("# a comment\n# Calculated with 'this test'.\n@ xlabel z-dimension [nm]\n@ ylabel y-dimension [nm]\n"
                    "@ zlabel order parameter ($S$)\n@ zrange -0.5 1.0 0.25\n$ type colorbar\n$ colormap seismic_r\n"
                    "-1.0000 0.2500 NaN\n-1.0000 0.5000 -0.0000\n-1.0000 0.7500 0.0000\n"
                    "-0.5000 0.2500 0.1235\n-0.5000 0.5000 -0.9999\n-0.5000 0.7500 1.0000\n")
    om.plane = 1
    assert "@ xlabel x-dimension [nm]\n@ ylabel z-dimension [nm]\n@ zlabel order parameter ($-S_{CH}$)\n@ zrange -1.0 0.5 0.25\n" in \
        writers.ordermap_text(values, om, "aa", "# c")


def test_ordermap_groups_of_the_united_atom_system(oracle_maps):
    _, labels, _ = oracle_maps(True)
    groups = st.ordermap_groups(labels, "ua")
    assert [g.slots for g in groups] == st.error_groups(labels, "ua")
    stems = {f"{stem}_{plane}" for g in groups for _, stem, _ in g.files for plane in ou.PLANES}
    assert stems == set(ou.golden_names())
    # one molecule type: its average and the system's are one slot set with two files, the system's at the top
    (both,) = [g for g in groups if len(g.files) == 2 and g.files[0][1] == "ordermap_average"]
    assert [f[:2] for f in both.files] == [("POPC", "ordermap_average"), ("", "ordermap_average")]
    assert both.files[1][2] == "# Map of average order parameters calculated for all bonds of all molecule types."
    assert all(sub == "POPC" for g in groups if g is not both for sub, _, _ in g.files)


BOND_STEM = re.compile(r"^ordermap_[^-\s]+-[^-\s]+-\d+--[^-\s]+-[^-\s]+-\d+$")
ATOM_STEM = re.compile(r"^ordermap_[^-\s]+-[^-\s]+-\d+$")


@pytest.mark.parametrize("kind", ["aa", "cg"])
def test_ordermap_groups_of_bond_systems(built, kind):
    fx = Fixture("pcpepg" if kind == "aa" else "cg")
    _, labels, _ = (aa_setup if kind == "aa" else cg_setup)(fx)
    groups = st.ordermap_groups(labels, kind)
    assert [g.slots for g in groups] == st.error_groups(labels, kind)
    n_acc = sum(len(ml.bonds) for ml in labels)
    bond_files = [(g.slots, f) for g in groups for f in g.files if "--" in f[1]]
    assert sorted(s[0] for s, _ in bond_files) == list(range(n_acc)) and all(len(s) == 1 for s, _ in bond_files)
    for slots, (sub, stem, comment) in bond_files:
        ml = [m for m in labels if m.slot0 <= slots[0] < m.slot0 + len(m.bonds)][0]
        b = ml.bonds[slots[0] - ml.slot0]
        assert BOND_STEM.match(stem), stem
        assert stem == f"ordermap_{b.res1 or ml.name}-{b.name1}-{b.rel1}--{b.res2 or ml.name}-{b.name2}-{b.rel2}"
        assert sub == ml.name and comment.startswith("# Map of average order parameters calculated for bonds between atom types ")
        assert comment.endswith(f" of a molecule type {ml.name}.")
    others = [f for g in groups for f in g.files if "--" not in f[1]]
    averages = [f for f in others if f[1] == "ordermap_average"]
    assert [f[0] for f in averages] == [ml.name for ml in labels] + [""]
    atoms = [f for f in others if f[1] != "ordermap_average"]
    assert all(ATOM_STEM.match(f[1]) for f in atoms)
    assert (len(atoms) == sum(len(ml.heavy_atoms) for ml in labels)) if kind == "aa" else not atoms
    assert len({(f[0], f[1]) for g in groups for f in g.files}) == len(bond_files) + len(others)     # no name twice


@pytest.mark.parametrize("leaflets", [False, True])
def test_write_ordermaps_makes_the_reference_tree(oracle_maps, tmp_path, leaflets):
    res, labels, om = oracle_maps(leaflets)
    groups = st.ordermap_groups(labels, "ua")
    values = st.ordermap_values(res, [g.slots for g in groups], ou.MIN_SAMPLES)
    out = tmp_path / "maps"
    written = writers.write_ordermaps(str(out), values, groups, om, "ua", leaflets)
    planes = ou.PLANES if leaflets else ou.PLANES[:1]
    names = [n for n in ou.golden_names() if n.rsplit("_", 1)[1] in planes]
    want = {os.path.join("POPC", n + ".dat") for n in names} | {f"ordermap_average_{p}.dat" for p in planes}
    found = {os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs}
    assert found == want == set(written) and len(written) == len(want)
    assert sorted(os.listdir(out)) == sorted(["POPC"] + [f"ordermap_average_{p}.dat" for p in planes])
    assert not any("plot" in f for f in found)
    for n in names:                                            # what lies there is the text of ordermap_text, golden from line 3 on
        with open(out / "POPC" / (n + ".dat")) as f:
            got = f.read().split("\n")
        _, lines = ou.golden_values(n, (14, 4))
        assert ou.compare_maps(ou.parse_map("\n".join(got)), ou.read_map(n + ".dat")) == [] and got[2:8] == lines[2:8]
    with open(out / "ordermap_average_full.dat") as f:
        assert f.readline() == "# Map of average order parameters calculated for all bonds of all molecule types.\n"
    with pytest.raises(ValueError):
        writers.write_ordermaps(str(out), values[:-1], groups, om, "ua", leaflets)


def test_abi_symbol_is_in_the_built_library(built):
    lib = abi.load_library()
    assert "gorder_hip_ordermaps" in abi._EXPORTS and lib.gorder_hip_ordermaps is not None
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "gorder_amd", "libgorder_hip.so")], capture_output=True, text=True)
    assert nm.returncode == 0 and re.search(r" T gorder_hip_ordermaps$", nm.stdout, re.M)
    assert callable(abi.HipEngine.ordermaps)
