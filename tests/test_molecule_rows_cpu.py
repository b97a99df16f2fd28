"""Per-molecule order rows without a GPU: the lane order and the group check of gorder_amd/csrc/molecule_rows.h through a
stand-alone program (tests/cabi/molecule_rows.cpp; built plainly and with the address and undefined-behaviour sanitizers,
both binaries run directly), the route of the order pass with OrderRouteIn::mol_rows set (tests/cabi/order_route_mol.cpp),
and the Python side: structure.molecule_groups, structure.molecule_order, writers.molecule_order_text."""
import os
import subprocess

import numpy as np
import pytest

from gorder_amd import structure, writers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gorder_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def compile_driver(directory, source, name, flags):
    exe = str(directory / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", *flags, f"-I{CSRC}", os.path.join(ROOT, "tests", "cabi", source), "-o", exe])

    def run(*args):
        res = subprocess.run([exe, *map(str, args)], capture_output=True, timeout=300)
        err = res.stderr.decode()
        assert res.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, res.stdout.decode() + err
        return res.stdout.decode()
    return run


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("molecule_rows"), "molecule_rows.cpp", "molecule_rows_" + request.param,
                          SANITIZE if request.param == "sanitized" else [])


# ---- 1. the lane order ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_lane_order_against_brute_force(driver, seed):
    """Random tiles and group maps: every item once per tile, runs maximal and in lane order, destination words right,
    ungrouped items in no run, the three statistics equal to a brute-force count (the checks are in the program)."""
    word, plans, runs = driver("lanes", seed, 400).split()
    assert word == "ok" and int(plans) == 400 and int(runs) > 10000


def test_group_check_names_what_is_wrong(driver):
    got = dict(line.split(": ", 1) for line in driver("groups").splitlines())
    assert got["fine"] == "ok" and got["2047"] == "ok"
    for case, word in [("empty", "empty"), ("range", "out of range"), ("twice", "two groups"), ("twice_in_one", "two groups"),
                       ("descending", "ascending"), ("first", "group_begin[0]"), ("2048", "2047")]:
        assert word in got[case], (case, got[case])


def test_packed_word_unpacks(driver):
    """Up to 2047 samples of -500000 .. 1000000 ticks in one word: sum and count come back, the sum fits int32."""
    assert driver("words").strip() == "ok"


def test_staging_subrange(driver):
    got = {tuple(map(int, line.replace("->", "").split()[:3])): int(line.split()[-1]) for line in driver("subrange").splitlines()}
    for (frames, words, limit), sub in got.items():
        assert sub == min(frames, max(1, limit // (8 * words)))
    assert got[(11, 104, 1664)] == 2 and got[(4000, 83333, 1 << 30)] == 1610 and got[(11, 512, 1)] == 1


def test_store_truncate(driver):
    """What takes the rows of a failed batch back: rows, labels and chunk reuse against a plain list."""
    assert driver("truncate").split()[0] == "ok"


# ---- 2. the route ---------------------------------------------------------------------------------------------------------
def test_route_with_molecule_rows(tmp_path_factory):
    run = compile_driver(tmp_path_factory.mktemp("order_route_mol"), "order_route_mol.cpp", "order_route_mol", SANITIZE)
    lines = run().splitlines()
    assert len(lines) == 1 << 14
    TILED_MOL, NONE = 7, 0
    seen_plain = set()
    for line in lines:
        left, plain_family = line.split(" | ")
        i, family, label, npf, mom, spec, extras, by_slot, ua_mode, direct = left.split()
        i = int(i)
        bond_tiles, wide, npf5 = i & 1, (i >> 9) & 1, (i >> 10) & 1
        if not bond_tiles:
            assert int(family) == NONE and label == "-"
        else:
            assert int(family) == TILED_MOL and label == "k_bonds_tiled_mol"
        # never speculative: global leaflets take the two-kernel path on this route
        assert (int(mom), int(spec), int(extras), int(by_slot), int(ua_mode), int(direct)) == (0, 0, 0, 0, -1, 0), line
        assert int(npf) == (5 if wide or npf5 else 4)
        seen_plain.add(int(plain_family))
    # the same facts without the rows take the plain kernels (some of them speculatively): the switch alone moves the route
    assert seen_plain == {0, 1, 2}


# ---- 3. Python ------------------------------------------------------------------------------------------------------------
def labels():
    bond = structure.BondLabel(1, "A", 2, "B")
    return [structure.MolLabels("POPC", [bond] * 5, n_molecules=3, slot0=0), structure.MolLabels("CHOL", [], n_molecules=2, slot0=5),
            structure.MolLabels("POPE", [bond] * 2, n_molecules=4, slot0=5)]


def test_molecule_groups():
    groups, names = structure.molecule_groups(labels(), "cg")
    assert groups == [[0, 1, 2, 3, 4], [5, 6]] and names == ["POPC", "POPE"]
    with pytest.raises(ValueError):
        structure.molecule_groups(labels(), "ua")


@pytest.mark.parametrize("analysis", ["aa", "cg"])
@pytest.mark.parametrize("min_samples", [1, 3])
def test_molecule_order_against_mean_ticks(analysis, min_samples):
    rng = np.random.default_rng(5)
    counts = rng.integers(0, 6, size=(7, 2, 9)).astype(np.uint32)
    sums = (rng.integers(-500000, 1000001, size=counts.shape) * counts).astype(np.int32)
    sums[0, 0, :4] = [-11, 11, -2999999, 2999999]
    counts[0, 0, :4] = [3, 3, 3, 3]                       # truncation toward zero on both sides
    sums[1, 1, 0], counts[1, 1, 0] = 0, 4
    got = structure.molecule_order(sums, counts, analysis, min_samples)
    assert got.dtype == np.float32 and got.shape == sums.shape
    sign = -1.0 if analysis == "aa" else 1.0
    for idx in np.ndindex(*sums.shape):
        v = structure._mean_ticks(int(sums[idx]), int(counts[idx]), min_samples)
        if v != v:
            assert np.isnan(got[idx]), idx
        else:
            assert got[idx] == np.float32(sign * v), (idx, got[idx], v)
    assert np.isnan(got).any() and (~np.isnan(got)).any()
    assert got[0, 0, 0] == np.float32(sign * -3e-6) and got[0, 0, 1] == np.float32(sign * 3e-6)


def test_molecule_order_text():
    values = np.array([[[0.12344, np.nan], [-0.5, 1.0]], [[0.0, 0.25], [np.nan, np.nan]]], dtype=np.float32)
    text = writers.molecule_order_text(values, [100, 105], ["POPC", "POPE"])
    lines = text.splitlines()
    assert text.endswith("\n") and [ln for ln in lines if not ln.startswith("#")] == \
        ["100 0.1234 NaN -0.5000 1.0000", "105 0.0000 0.2500 NaN NaN"]
    assert "# column 1: frame index" in lines and "# columns 2-3: POPC, molecules 0-1" in lines and "# columns 4-5: POPE, molecules 0-1" in lines
    assert writers.molecule_order_text(values, [100, 105], ["a", "b"], header="# mine").splitlines()[0] == "# mine"
    with pytest.raises(ValueError):
        writers.molecule_order_text(values, [100], ["POPC", "POPE"])
    with pytest.raises(ValueError):
        writers.molecule_order_text(values, [100, 105], ["POPC"])
