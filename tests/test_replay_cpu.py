"""Whole-trajectory manual tables without a GPU: the host logic (gorder_amd/csrc/replay_rows.h) driven by a stand-alone
program under the address and undefined-behaviour sanitizers, the readers of the reference's two manual-input files
against its own files and against this repo's writers, and the new entry points of the built library."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from gorder_amd import abi, manual, writers
from golden_util import GOLDEN, expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_text(name):
    with open(os.path.join(GOLDEN, "expected", name)) as f:
        return f.read()


def labels_of(tree):
    return [SimpleNamespace(name=name, n_molecules=len(rows[0])) for name, rows in tree.items()]


def test_host_rows_under_sanitizers(tmp_path):
    exe = str(tmp_path / "replay_rows")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", f"-I{os.path.join(ROOT, 'gorder_amd', 'csrc')}",
                           os.path.join(ROOT, "tests", "cabi", "replay_rows.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "replay_rows ok" in res.stdout and "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr


@pytest.mark.parametrize("name,frequency,n_rows", [("aa_leaflets_every5.yaml", 5, 11), ("aa_leaflets_once.yaml", 0, 1),
                                                   ("aa_leaflets_every1.yaml", 1, 51), ("ua_leaflets_once.yaml", 0, 1)])
def test_read_leaflets_file(name, frequency, n_rows):
    tree, text = expected(name), golden_text(name)
    labels = labels_of(tree)
    flags = manual.read_leaflets_file(text, labels)
    assert flags.dtype == np.uint8 and flags.shape == (n_rows, sum(m.n_molecules for m in labels))
    # the YAML library's reading of the same file: 1 = upper there, Upper = 0 here
    want = np.concatenate([1 - np.array(tree[m.name], dtype=np.uint8) for m in labels], axis=1)
    np.testing.assert_array_equal(flags, want)
    assert 0 < flags.sum() < flags.size
    # the inverse of the writer, both ways round
    frames = np.arange(n_rows) * frequency
    out = writers.leaflets_export_text(flags, frames, labels, frequency)
    assert out.splitlines()[1:] == text.splitlines()[1:]
    np.testing.assert_array_equal(manual.read_leaflets_file(out, labels), flags)
    # the molecule types in another order: the columns follow the labels
    swapped = manual.read_leaflets_file(text, labels[::-1])
    np.testing.assert_array_equal(swapped[:, :labels[-1].n_molecules], flags[:, -labels[-1].n_molecules:])


def test_read_normals_file():
    tree, text = expected("ua_normals.yaml"), golden_text("ua_normals.yaml")
    labels = labels_of(tree)
    normals = manual.read_normals_file(text, labels)
    assert normals.dtype == np.float32 and normals.shape == (51, sum(m.n_molecules for m in labels), 3)
    want = np.concatenate([np.array(tree[m.name], dtype=np.float64) for m in labels], axis=1).astype(np.float32)
    assert normals.tobytes() == want.tobytes()
    out = writers.normals_export_text(normals, np.arange(51), labels)
    assert out.splitlines()[1:] == text.splitlines()[1:]
    assert manual.read_normals_file(out, labels).tobytes() == normals.tobytes()
    # random float32 vectors: what the writer prints (6 decimals) is what the reader returns, and writing that again
    # gives the same text; a normal that was never computed stays NaN
    rng = np.random.default_rng(5)
    given = rng.normal(size=(4, normals.shape[1], 3)).astype(np.float32)
    given[2, 7] = np.nan
    once = writers.normals_export_text(given, np.arange(4), labels)
    back = manual.read_normals_file(once, labels)
    assert np.isnan(back[2, 7]).all() and np.isnan(back).sum() == 3
    keep = ~np.isnan(given)
    np.testing.assert_array_equal(back[keep], np.round(given[keep].astype(np.float64), 6).astype(np.float32))
    assert writers.normals_export_text(back, np.arange(4), labels) == once


def test_readers_refuse_what_the_reference_refuses():
    labels = [SimpleNamespace(name="POPC", n_molecules=3), SimpleNamespace(name="POPE", n_molecules=2)]
    good = "# c\nPOPC:\n# Frame index 1\n  - [1,0,1]\nPOPE:\n  - [0,0]\n"
    np.testing.assert_array_equal(manual.read_leaflets_file(good, labels), [[0, 1, 0, 1, 1]])
    with pytest.raises(ValueError, match="POPE"):
        manual.read_leaflets_file("POPC:\n  - [1,0,1]\n", labels)                       # MoleculeNotFound
    with pytest.raises(ValueError, match="expected 3"):
        manual.read_leaflets_file(good.replace("[1,0,1]", "[1,0]"), labels)              # InconsistentNumberOfMolecules
    with pytest.raises(ValueError, match="0 or 1"):
        manual.read_leaflets_file(good.replace("[1,0,1]", "[1,2,1]"), labels)
    with pytest.raises(ValueError, match="different numbers of rows"):
        manual.read_leaflets_file(good + "  - [1,1]\n", labels)
    with pytest.raises(ValueError, match="3 components"):
        manual.read_normals_file("POPC:\n  - [[0,0,1],[0,0,1],[0,1]]\nPOPE:\n  - [[0,0,1],[0,0,1]]\n", labels)


def test_abi_symbols_are_in_the_built_library(built):
    lib = abi.load_library()
    for name in ("gorder_hip_set_manual_leaflet_table", "gorder_hip_set_manual_normal_table"):
        assert name in abi._EXPORTS and getattr(lib, name) is not None
    assert (abi.ERR_MANUAL_LEAFLET_FRAME, abi.ERR_MANUAL_NORMAL_FRAME) == (8, 9)
    assert b"leaflet" in lib.gorder_hip_strerror(8) and b"normal" in lib.gorder_hip_strerror(9)
    assert lib.gorder_hip_strerror(8) != lib.gorder_hip_strerror(9) != lib.gorder_hip_strerror(12345)
    for name in ("set_manual_leaflet_table", "set_manual_normal_table"):
        assert callable(getattr(abi.HipEngine, name))
