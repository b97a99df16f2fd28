"""United atoms in order histograms and per-molecule rows (GORDER_FLAG_UA_SAMPLES) without a GPU: the host table of k_ua_mol
(gorder_amd/csrc/ua_molecule_rows.h) on random tiles and group maps, and the united-atom kernel choice of the route
(order_route.h), both through stand-alone programs under the address and undefined-behaviour sanitizers; then the Python
helpers on united-atom labels.

The route's expected values restate the rule, not the header: the united-atom tiles run k_ua_mol where the flag is set and
the handle has molecule rows, k_ua_dist where the flag is set and it has a histogram, k_ua_extras otherwise; no other field
of the route moves, and the flag alone moves nothing."""
import os
import subprocess

import numpy as np
import pytest

from gorder_amd import abi, structure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UA_NONE, UA_EXTRAS, UA_DIST, UA_MOL = range(4)
FAMILY_NONE, TILED, GATHER, TILED_MOL, DIST = 0, 1, 2, 7, 8
KERNEL_BITS = ["acos", "geom", "use_gather", "item_run", "stage8", "wide", "npf5", "tw_gather", "maps_gather", "bond_tiles", "ua_tiles",
               "leaflets", "global_leaflets", "spec_enabled", "have_assignment", "every_frame_assigns"]


def build(tmp_path_factory, name):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", f"-I{os.path.join(ROOT, 'gorder_amd', 'csrc')}", f"-I{os.path.join(ROOT, 'include')}",
                           os.path.join(ROOT, "tests", "cabi", name + ".cpp"), "-o", exe])

    def run(*args):
        res = subprocess.run([exe, *map(str, args)], capture_output=True, timeout=300)
        err = res.stderr.decode()
        assert res.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err
        return res.stdout.decode()
    return run


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return build(tmp_path_factory, "ua_molecule_rows")


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    return build(tmp_path_factory, "ua_samples_route")


# ---- 1. the host table ------------------------------------------------------------------------------------------------------
def test_word_lists_on_random_tiles(table):
    """The program checks the invariants itself (every grouped (lane, hydrogen) -> exactly one local word whose global index
    is group * n_mol_total + molecule, ungrouped -> none, local words distinct, n_local <= 3 * 256, every word fed) and exits
    non-zero where one fails; here: it ran every seed, and the seeds reach the cases that matter."""
    rows = np.array([[int(x) for x in line.split()] for line in table(1, 400).splitlines()])
    assert rows.shape == (400, 7) and (rows[:, 0] == np.arange(1, 401)).all()
    tiles, items, grouped, words, max_local, most = rows[:, 1:].T
    assert (max_local <= 3 * 256).all() and (words <= grouped).all()
    assert (grouped == 0).any() and (words[grouped == 0] == 0).all()              # nothing grouped: empty lists
    assert max_local.max() > 256                                                  # more words than lanes: hydrogens in different groups
    assert (most >= 5).all() and (most > 5).any()                                 # the bond tiles' seed is kept and added to
    assert (tiles > 1).any() and (items >= 256).any()


def test_lds_sizing(table):
    rows = {n: (b, size) for n, b, size in ([int(x) for x in line.split()] for line in table("lds").splitlines())}
    for n, (bufs, size) in rows.items():
        # two buffers of four frames while they fit 40 KB, else one; the word list in front, padded to 16 bytes
        assert bufs == (2 if 2 * 4 * n * 8 <= 40 * 1024 else 1)
        assert size == (4 * n + 15) // 16 * 16 + bufs * 4 * n * 8
    assert rows[640][0] == 2 and rows[641][0] == 1 and rows[768][1] < 32 * 1024   # the widest tile: one buffer, 27 KB


# ---- 2. the route -------------------------------------------------------------------------------------------------------------
def test_the_flag_alone_changes_no_field(route):
    n, differing, wrong_kernel = map(int, route("flag").split())
    assert n == 1 << 24 and differing == 0 and wrong_kernel == 0


def test_the_united_atom_kernel_chosen(route):
    rows = np.array([[int(x) for x in line.split()] for line in route("kernels").splitlines()])
    bits, flag, feature, ua_kernel, family, ua_mode, extras, same = rows.T
    f = {name: ((bits >> k) & 1).astype(bool) for k, name in enumerate(KERNEL_BITS)}
    assert rows.shape[0] == (1 << 16) * 2 * 2 + (1 << 15) * 2                     # (no geometry selection with the rows)
    flag, dist, mol = flag == 1, feature == 1, feature == 2
    want = np.select([~f["ua_tiles"], flag & mol, flag & dist], [UA_NONE, UA_MOL, UA_DIST], UA_EXTRAS)
    np.testing.assert_array_equal(ua_kernel, want)
    assert same.all()                                                             # every other field: the flag-less route's
    # the bond tiles of the same handle keep their kernels, and a histogram launches from the extras' loop
    np.testing.assert_array_equal(family[mol], np.where(f["bond_tiles"][mol], TILED_MOL, FAMILY_NONE))
    np.testing.assert_array_equal(family[dist], np.where(f["bond_tiles"][dist], DIST, FAMILY_NONE))
    assert extras[dist].all() and not extras[mol].any()
    assert ((ua_mode >= 0) == f["ua_tiles"]).all()
    for k in (UA_NONE, UA_EXTRAS, UA_DIST, UA_MOL):
        assert (ua_kernel == k).any()
    assert (f["bond_tiles"] & (ua_kernel == UA_MOL)).any() and (f["bond_tiles"] & (ua_kernel == UA_DIST)).any()     # mixed handles


# ---- 3. Python ----------------------------------------------------------------------------------------------------------------
def ua_labels():
    c = structure.UaCarbonLabel
    popc = [c(10, "C1", abi.UA_CH3, 3, "POPC"), c(11, "C2", abi.UA_CH2, 2, "POPC"), c(12, "C3", abi.UA_CH1_SAT, 1, "POPC")]
    return [structure.UaMolLabels("POPC", popc, n_molecules=3, slot0=0), structure.UaMolLabels("CHOL", [], n_molecules=2, slot0=6),
            structure.UaMolLabels("POPE", popc[:2], n_molecules=4, slot0=6)]


def test_flag_value():
    assert abi.FLAG_UA_SAMPLES == 8
    header = open(os.path.join(ROOT, "include", "gorder_hip.h")).read()
    assert "GORDER_FLAG_UA_SAMPLES = 8u" in header
    assert "GORDER_FLAG_UA_SAMPLES" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_molecule_groups_of_united_atom_labels():
    groups, names = structure.molecule_groups(ua_labels(), "ua")
    assert groups == [[0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10]] and names == ["POPC", "POPE"]
    for analysis in ("aa", "cg", "xx"):
        with pytest.raises(ValueError):
            structure.molecule_groups(ua_labels(), analysis)
    # bond labels beside united-atom ones (a mixed handle): "ua"
    bond = structure.BondLabel(1, "A", 2, "B")
    mixed = [structure.MolLabels("LIP0", [bond] * 3, n_molecules=5, slot0=0)] + [
        structure.UaMolLabels(m.name, m.carbons, m.n_molecules, m.slot0 + 3) for m in ua_labels()]
    groups, names = structure.molecule_groups(mixed, "ua")
    assert groups == [[0, 1, 2], [3, 4, 5, 6, 7, 8], [9, 10, 11, 12, 13]] and names == ["LIP0", "POPC", "POPE"]


def test_molecule_order_and_density_report_minus_s_for_united_atoms():
    counts = np.array([[[2, 0, 3]]], dtype=np.uint32)
    sums = np.array([[[-300001, 0, 2999999]]], dtype=np.int32)
    ua, aa, cg = (structure.molecule_order(sums, counts, a) for a in ("ua", "aa", "cg"))
    np.testing.assert_array_equal(ua, aa)
    np.testing.assert_array_equal(ua[0, 0, [0, 2]], -cg[0, 0, [0, 2]])
    assert ua[0, 0, 0] == np.float32(0.15) and np.isnan(ua[0, 0, 1]) and ua[0, 0, 2] == np.float32(-0.999999)
    hist = np.zeros((4, 3, 5), dtype=np.uint64)
    hist[:, 0, 2], hist[:, 0, 3] = [1, 2, 3, 4], [4, 0, 0, 0]
    grouped = structure.histogram_groups(hist, [[2, 3]])
    assert grouped.shape == (1, 3, 4) and list(grouped[0, 0]) == [5, 2, 3, 4]
    edges = structure.order_edges(4)
    d_ua, lo, hi = structure.order_density(grouped, edges, "ua")
    d_aa, lo_aa, hi_aa = structure.order_density(grouped, edges, "aa")
    np.testing.assert_array_equal(d_ua, d_aa)
    np.testing.assert_array_equal(lo, lo_aa)
    assert lo[0] == -edges[-1] / 1e6 and hi[-1] == 0.5 and (np.diff(lo) > 0).all()     # the axis is -S
    assert abs(float((d_ua[0, 0] * (hi - lo)).sum()) - 1.0) < 1e-12
