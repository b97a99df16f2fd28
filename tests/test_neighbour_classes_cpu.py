"""Order by local composition without a GPU: the argument check, the piece arithmetic, the table fit and the sub-range of
gorder_amd/csrc/neighbour_classes.h through a stand-alone program (tests/cabi/neighbour_classes.cpp; built plainly and with
the address and undefined-behaviour sanitizers, both binaries run directly), the route of the order pass with
OrderRouteIn::classes set through a program of its own (tests/cabi/neighbour_route.cpp), and the Python side:
structure.neighbour_centres, structure.class_profile, structure.class_counts, writers.class_profile_text."""
import os
import subprocess

import numpy as np
import pytest

from gorder_amd import structure, synthetic, writers
from gorder_amd.abi import LEAFLETS_GLOBAL, Results

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gorder_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
MAX_ATOMS, MAX_CLASSES, PIECE, GRID_ROWS = 16384, 32, 1024, 65535


def compile_driver(directory, source, flags):
    exe = str(directory / source)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", *flags, f"-I{CSRC}", os.path.join(ROOT, "tests", "cabi", source + ".cpp"), "-o", exe])

    def run(*args):
        res = subprocess.run([exe, *map(str, args)], capture_output=True, timeout=300)
        err = res.stderr.decode()
        assert res.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, res.stdout.decode() + err
        return res.stdout.decode()
    return run


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("neighbour_classes_" + request.param), "neighbour_classes",
                          SANITIZE if request.param == "sanitized" else [])


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def route_driver(request, tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("neighbour_route_" + request.param), "neighbour_route",
                          SANITIZE if request.param == "sanitized" else [])


# ---- 1. neighbour_classes.h ------------------------------------------------------------------------------------------------
def test_the_limits_are_the_headers(driver):
    header = open(os.path.join(ROOT, "include", "gorder_hip.h")).read()
    assert f"#define GORDER_NEIGHBOUR_MAX_ATOMS {MAX_ATOMS}\n" in header and f"#define GORDER_NEIGHBOUR_MAX_CLASSES {MAX_CLASSES}\n" in header
    from gorder_amd import abi
    assert (abi.NEIGHBOUR_MAX_ATOMS, abi.NEIGHBOUR_MAX_CLASSES) == (MAX_ATOMS, MAX_CLASSES)


def test_argument_check_names_what_is_wrong(driver):
    got = dict(line.split(": ", 1) for line in driver("check").splitlines())
    for case in ("plain", "one neighbour", "most neighbours", "two classes", "most classes", "radius tiny", "radius huge", "centre last atom",
                 "neighbour last atom", "centres twice"):
        assert got[case] == "ok", (case, got[case])
    for case, word in [("too many neighbours", "GORDER_NEIGHBOUR_MAX_ATOMS"), ("one class", "fewer than 2 classes"), ("no class", "fewer than 2 classes"),
                       ("too many classes", "GORDER_NEIGHBOUR_MAX_CLASSES"), ("radius zero", "radius"), ("radius negative", "radius"),
                       ("radius nan", "radius"), ("radius inf", "radius"), ("centre past the atoms", "centre index >= n_atoms"),
                       ("neighbour past the atoms", "neighbour index >= n_atoms"), ("equal", "strictly ascending"),
                       ("descending", "strictly ascending"), ("null centres", "no centres")]:
        assert word in got[case], (case, got[case])


def test_pieces(driver):
    got = {}
    for line in driver("pieces").splitlines():
        left, lens = line.split(":")
        n, n_pieces = map(int, left.split(" -> "))
        got[n] = (n_pieces, [int(x) for x in lens.split()])
    assert sorted(got) == [0, 1, 1023, 1024, 1025, 2048, 2049, 16383, 16384]
    for n, (n_pieces, lens) in got.items():
        assert n_pieces == -(-n // PIECE) and len(lens) == n_pieces + 1 and lens[-1] == 0      # nothing past the last piece
        assert sum(lens) == n and all(0 < x <= PIECE for x in lens[:-1]) and all(x == PIECE for x in lens[:-2])
    assert got[0] == (0, [0]) and got[1] == (1, [1, 0]) and got[1023] == (1, [1023, 0]) and got[1024] == (1, [1024, 0])
    assert got[1025] == (2, [1024, 1, 0]) and got[16384][0] == 16 and got[16383][1][-2] == 1023


def test_table_fit_at_the_64_kb_edge(driver):
    got = {tuple(map(int, line.split(" -> ")[0].split())): tuple(map(int, line.split(" -> ")[1].split())) for line in driver("table").splitlines()}
    for (planes, n_classes, slots), (nbytes, fits) in got.items():
        assert nbytes == planes * n_classes * slots * 8 and fits == int(nbytes <= 64 * 1024)
    assert got[(2, 32, 128)] == (65536, 1) and got[(2, 32, 129)] == (66048, 0)      # the edge itself fits, one slot more does not
    assert got[(2, 16, 256)][1] == 1 and got[(2, 17, 256)][1] == 0 and got[(1, 32, 256)][1] == 1 and got[(2, 32, 256)][1] == 0
    assert got[(2, 32, 0xffffffff)][1] == 0                                          # no 32-bit wrap makes a huge table fit


def test_sub_ranges(driver):
    both = {tuple(map(int, line.split(" -> ")[0].split())): tuple(map(int, line.split(" -> ")[1].split())) for line in driver("subrange").splitlines()}
    got = {k: v[0] for k, v in both.items()}
    gib = 1 << 30
    for (frames, n_mol, forced, row_bytes), (sub, whole) in both.items():
        assert 1 <= sub <= min(frames, GRID_ROWS)                                    # a frame per row of gridDim.y
        assert sub * (n_mol & 0xffffffff) <= row_bytes or sub == 1                   # the rows fit, or it is a single frame
        assert whole == int(frames * (n_mol & 0xffffffff) <= row_bytes)
        if forced:
            assert sub <= forced
    assert got[(4000, 3072, 0, gib)] == 4000 and got[(11, 40, 3, gib)] == 3 and got[(11, 40, 0, gib)] == 11
    assert got[(11, 40, 11, gib)] == 11 and got[(11, 40, 12, gib)] == 11 and got[(1, 1, 0, gib)] == 1
    assert got[(4000, 3072, 0, 3072 * 100)] == 100 and got[(4000, 3072, 0, 3072 * 100 + 3071)] == 100
    assert got[(4000, 3072, 0, 1)] == 1 and got[(4000, 3072, 7, 3072 * 5)] == 5
    assert got[(0xffffffff, 1, 0, gib)] == GRID_ROWS and got[(100, gib, 0, gib)] == 1 and got[(100, gib + 1, 0, gib)] == 1
    # the rows of gridDim.y: 65 535 frames a launch, whatever the rows would hold; the rows still hold the whole batch
    assert got[(65534, 8, 0, gib)] == 65534 and got[(65535, 8, 0, gib)] == 65535 and got[(65536, 8, 0, gib)] == 65535
    assert both[(65600, 8, 0, gib)] == (65535, 1) and both[(65600, 8, 70000, gib)] == (65535, 1) and both[(65600, 8, 0, 8 * 70000)] == (65535, 1)
    assert both[(200000, 16384, 0, gib)] == (65535, 0) and both[(200000, 16385, 0, gib)] == (65532, 0)    # past 16 384 molecules the rows bind


# ---- 2. the route -----------------------------------------------------------------------------------------------------------
def test_route_with_classes(route_driver):
    lines = route_driver().splitlines()
    assert len(lines) == 1 << 13
    CLASSES, NONE = 9, 0
    seen_plain = set()
    for line in lines:
        left, plain_family = line.split(" | ")
        i, family, label, npf, mom, spec, extras, by_slot, ua_mode, direct, maps_only, map_acc = left.split()
        i = int(i)
        bond_tiles, npf5 = i & 1, (i >> 9) & 1
        if not bond_tiles:
            assert int(family) == NONE and label == "-"
        else:
            assert int(family) == CLASSES and label == "k_bonds_classes"
        # never speculative (global leaflets take the two-kernel path), the items in tile order, launched from the extras' loop
        assert (int(mom), int(spec), int(extras), int(by_slot), int(ua_mode), int(direct), int(maps_only), int(map_acc)) == (0, 0, 1, 0, -1, 0, 0, 0), line
        assert int(npf) == (5 if npf5 else 4)
        seen_plain.add(int(plain_family))
    assert seen_plain == {0, 1, 2}                                       # the same facts without classes: the plain kernels


# ---- 3. Python ------------------------------------------------------------------------------------------------------------
def test_neighbour_centres():
    system = synthetic.cg_membrane(40, n_types=3, leaflets=LEAFLETS_GLOBAL)
    got = structure.neighbour_centres(system.tables)
    want = [12 * m + 1 for ty in range(3) for m in range(40) if m % 3 == ty]
    assert got.dtype == np.uint32 and got.tolist() == want
    with pytest.raises(ValueError):
        structure.neighbour_centres(synthetic.cg_membrane(40, n_types=3).tables)     # no leaflets: the types have no heads


def truncating_mean(s, c, min_samples):
    if c < max(1, min_samples):
        return float("nan")
    q = abs(s) // c
    return float(np.float32((-q if s < 0 else q) / 1e6))


@pytest.mark.parametrize("analysis", ["aa", "cg"])
def test_class_profile_against_plain_loops(analysis):
    rng = np.random.default_rng(8)
    n_classes, n_acc = 5, 7
    classes = []
    for k in range(n_classes):
        counts = rng.integers(0, 50, size=(3, n_acc)).astype(np.uint64)
        sums = (rng.integers(-500000, 1000001, size=(3, n_acc)) * counts.astype(np.int64)).astype(np.int64) + rng.integers(-3, 4, size=(3, n_acc))
        classes.append(Results(sums, counts, 11))
    classes[2].counts[:, 3] = 0                                          # a slot without samples in a class
    classes[4].counts[1] = 0                                             # a plane without samples: NaN, not a division error
    groups = [[0, 1, 2], [6], [3, 5]]
    for min_samples in (1, 40):
        got = structure.class_profile(classes, groups, analysis, min_samples)
        assert got.dtype == np.float32 and got.shape == (3, 3, n_classes)
        cnt = structure.class_counts(classes, groups)
        assert cnt.dtype == np.uint64 and cnt.shape == (3, 3, n_classes)
        some_nan = some_negative = False
        for g, slots in enumerate(groups):
            for w in range(3):
                for k in range(n_classes):
                    s = sum(int(classes[k].sums[w, q]) for q in slots)
                    c = sum(int(classes[k].counts[w, q]) for q in slots)
                    assert int(cnt[g, w, k]) == c
                    v = truncating_mean(s, c, min_samples)
                    some_negative |= s < 0 and c >= min_samples
                    if v != v:
                        assert np.isnan(got[g, w, k])
                        some_nan = True
                    else:
                        assert got[g, w, k] == np.float32((-1.0 if analysis == "aa" else 1.0) * v)
        assert some_nan and some_negative
    # the arithmetic is radial_profile's own
    np.testing.assert_array_equal(structure.radial_profile(classes, np.arange(1, n_classes + 1), groups, analysis, 1),
                                  structure.class_profile(classes, groups, analysis, 1))
    # truncation, not rounding: 5 ticks over 3 samples is 1 tick, and -5 over 3 is -1
    one = [Results(np.array([[5], [-5], [0]], dtype=np.int64), np.array([[3], [3], [0]], dtype=np.uint64), 1)]
    v = structure.class_profile(one, [[0]], "cg", 1)[0, :, 0]
    assert v[0] == np.float32(1e-6) and v[1] == np.float32(-1e-6) and np.isnan(v[2])


def test_class_profile_text():
    rng = np.random.default_rng(9)
    values = rng.uniform(-0.5, 1.0, size=(2, 3, 4)).astype(np.float32)
    values[1, 2, 3] = np.nan
    counts = rng.integers(0, 1 << 40, size=(2, 3, 4)).astype(np.uint64)
    text = writers.class_profile_text(values, counts, ["POPC", "CHOL"])
    assert text.endswith("\n")
    rows = [ln.split() for ln in text.splitlines() if not ln.startswith("#")]
    assert [r[0] for r in rows] == ["0", "1", "2", ">=3"]                # the last class holds every larger count
    for k, r in enumerate(rows):
        assert len(r) == 1 + 2 * 4
        for g in range(2):
            cells = r[1 + 4 * g:5 + 4 * g]
            assert int(cells[3]) == int(counts[g, 0, k])
            for w in range(3):
                assert cells[w] == ("NaN" if np.isnan(values[g, w, k]) else f"{float(values[g, w, k]):.4f}")
    names = [ln for ln in text.splitlines() if ln.startswith("# column")]
    assert names[0] == "# column 1: neighbours" and len(names) == 9 and names[-1] == "# column 9: CHOL samples"
    bare = writers.class_profile_text(values, None, ["POPC", "CHOL"], header="# mine")
    assert bare.splitlines()[0] == "# mine" and len([ln for ln in bare.splitlines() if not ln.startswith("#")][0].split()) == 7
    with pytest.raises(ValueError):
        writers.class_profile_text(values, counts, ["POPC"])
    with pytest.raises(ValueError):
        writers.class_profile_text(values, counts[:, :, :3], ["POPC", "CHOL"])
