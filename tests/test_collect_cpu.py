"""Collected history without a GPU: the two export writers against the reference's files, the new entry points of the
built library, and the host side of the history (gorder_amd/csrc/collect_store.h) driven by a stand-alone program under
the address and undefined-behaviour sanitizers."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from gorder_amd import abi, writers
from golden_util import expected
from test_writers_cpu import golden, same_tokens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def labels_of(tree):
    return [SimpleNamespace(name=name, n_molecules=len(rows[0])) for name, rows in tree.items()]


@pytest.mark.parametrize("name,frequency", [("aa_leaflets_every5.yaml", 5), ("aa_leaflets_once.yaml", 0)])
def test_leaflets_export_text_round_trip(name, frequency):
    from test_golden_wide_oracle import assignment_rows
    tree = expected(name)
    labels = labels_of(tree)
    flags = np.array(assignment_rows(tree, labels))                  # this repo's encoding: Upper = 0
    frames = np.arange(len(flags)) * frequency
    assert flags.shape == ((11 if frequency else 1), sum(m.n_molecules for m in labels)) and 0 < flags.sum() < flags.size
    text = writers.leaflets_export_text(flags, frames, labels, frequency)
    same_tokens(text, golden(name))
    assert text.splitlines()[1:] == golden(name).splitlines()[1:]
    with pytest.raises(ValueError):
        writers.leaflets_export_text(flags, frames + 1, labels, frequency)


def test_normals_export_text_round_trip():
    tree = expected("ua_normals.yaml")
    labels = labels_of(tree)
    normals = np.concatenate([np.array(tree[m.name], dtype=np.float64) for m in labels], axis=1)
    assert normals.shape == (51, sum(m.n_molecules for m in labels), 3)
    text = writers.normals_export_text(normals, np.arange(51), labels)
    same_tokens(text, golden("ua_normals.yaml"))
    assert text.splitlines()[1:] == golden("ua_normals.yaml").splitlines()[1:]
    # a normal that was never computed: NaN in the same 9 columns
    normals[3, 1] = np.nan
    line = writers.normals_export_text(normals.astype(np.float32), np.arange(51), labels).splitlines()[3 + 2 * 3]
    assert line.startswith("  - [[") and ",[      NaN,      NaN,      NaN],[" in line


def test_abi_symbols_are_in_the_built_library(built):
    lib = abi.load_library()
    for name in ("gorder_hip_set_collect", "gorder_hip_collected_counts", "gorder_hip_collected_leaflets",
                 "gorder_hip_collected_normals"):
        assert name in abi._EXPORTS and getattr(lib, name) is not None
    assert (abi.COLLECT_LEAFLETS, abi.COLLECT_NORMALS) == (1, 2)


def test_host_chunks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "collect_chunks")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", f"-I{os.path.join(ROOT, 'gorder_amd', 'csrc')}",
                           os.path.join(ROOT, "tests", "cabi", "collect_chunks.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "collect_chunks ok" in res.stdout and "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
