"""The device route for error estimates and convergence, without a GPU: the host arithmetic (gorder_amd/csrc/timewise_blocks.h)
driven by a stand-alone program under the address and undefined-behaviour sanitizers, the `errors=` and `prefix=` routes of the
tree builders and the convergence writer against the routes that take the rows (on the oracle's rows), the order of
error_groups, the constructions the GPU tests rely on, and the new entry points of the built library."""
import os
import subprocess

import numpy as np
import pytest

from gorder_amd import abi, writers
from gorder_amd import structure as st
from golden_util import METHODS, Fixture, aa_setup, cg_setup, ua_setup
from oracle import oracle
import timewise_device_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETUPS = {"aa": aa_setup, "cg": cg_setup, "ua": ua_setup}


def test_host_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "timewise_blocks")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", f"-I{os.path.join(ROOT, 'gorder_amd', 'csrc')}",
                           os.path.join(ROOT, "tests", "cabi", "timewise_blocks.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "timewise_blocks ok" in res.stdout and "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr


@pytest.fixture(scope="module")
def fixtures(built):
    return {"aa": Fixture("pcpepg"), "cg": Fixture("cg"), "ua": Fixture("ua")}


@pytest.fixture(scope="module")
def runs(fixtures):
    """(res, rows, labels) of the oracle per (kind, leaflets), made once."""
    cache = {}

    def run(kind, leaflets):
        if (kind, leaflets) not in cache:
            fx = fixtures[kind]
            tables, labels, midx = SETUPS[kind](fx, leaflets=METHODS["global"] if leaflets else None, timewise=True)
            frames = fx.window()
            eng = oracle.OracleEngine(tables, trig=oracle.TRIG_LIBM, n_threads=4)
            eng.submit(np.ascontiguousarray(fx.xyz[frames][:, midx, :]), fx.boxes[frames], frames)
            cache[kind, leaflets] = (eng.finish(), eng.timewise(len(frames)), labels)
        return cache[kind, leaflets]
    return run


class Recording(dict):
    """An `errors` mapping that notes what it is asked for."""

    def __init__(self, *a):
        super().__init__(*a)
        self.asked = []

    def __getitem__(self, key):
        self.asked.append(key)
        return super().__getitem__(key)


def tree_of(kind, res, labels, leaflets, **kw):
    return (st.results_tree_ua(res, labels, leaflets=leaflets, **kw) if kind == "ua"
            else st.results_tree(res, labels, kind, leaflets=leaflets, **kw))


def same_tree(a, b):
    """Equal trees, NaN equal to NaN."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b)
        for k in a:
            same_tree(a[k], b[k])
    elif isinstance(a, list):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            same_tree(x, y)
    else:
        assert a == b or (a != a and b != b), (a, b)


@pytest.mark.parametrize("kind,leaflets", [("aa", False), ("cg", True), ("ua", True)])
def test_error_groups_are_what_the_tree_asks_for_and_errors_reproduce_the_rows_route(runs, kind, leaflets):
    res, tw, labels = runs(kind, leaflets)
    groups = st.error_groups(labels, kind)
    assert len(set(map(tuple, groups))) == len(groups) and all(len(g) for g in groups)
    n_acc = tw[0].shape[2]
    assert groups[-1] == list(range(n_acc)) or len(labels) == 1           # the whole system is asked for last
    assert sorted(g[0] for g in groups if len(g) == 1) == list(range(n_acc))   # every accumulator on its own
    for n_blocks in (5, 10):
        errors = Recording(zip(map(tuple, groups), tu.host_errors(tw, groups, n_blocks)))
        got = tree_of(kind, res, labels, leaflets, errors=errors)
        first = list(dict.fromkeys(errors.asked))
        assert first == [tuple(g) for g in groups]                         # the same groups in the same order
        same_tree(got, tree_of(kind, res, labels, leaflets, timewise=tw, n_blocks=n_blocks))
    # the min_samples rule stays on the host: a NaN mean prints a NaN error and asks for none
    errors = Recording(zip(map(tuple, groups), tu.host_errors(tw, groups, 5)))
    limit = int(np.median(res.counts[0]))
    got = tree_of(kind, res, labels, leaflets, errors=errors, min_samples=limit)
    same_tree(got, tree_of(kind, res, labels, leaflets, timewise=tw, min_samples=limit))
    assert len(set(errors.asked)) < len(groups)


def test_default_trees_are_unchanged(runs):
    res, _, labels = runs("aa", False)
    tree = st.results_tree(res, labels, "aa", leaflets=False)
    assert isinstance(tree["average order"]["total"], float)


@pytest.mark.parametrize("kind,leaflets", [("aa", False), ("aa", True), ("cg", True), ("ua", True)])
def test_convergence_text_from_prefix_columns(runs, kind, leaflets):
    _, tw, labels = runs(kind, leaflets)
    groups = writers.convergence_groups(labels)
    assert [g[0] for g in groups] == [ml.slot0 for ml in labels] and sum(map(len, groups)) == tw[0].shape[2]
    prefix, _ = tu.host_prefix(tw, groups)
    tu.same_floats(writers._prefix_columns(tw, groups), prefix)            # the writer's own columns are the restatement's
    for step in (1, 5):
        want = writers.convergence_text(tw, labels, kind, leaflets, step=step)
        assert writers.convergence_text(None, labels, kind, leaflets, step=step, prefix=prefix) == want


def test_prefix_restatement_chains_through_the_carry(runs):
    _, tw, labels = runs("cg", True)
    groups = writers.convergence_groups(labels)
    whole, end = tu.host_prefix(tw, groups)
    k = 7
    a, mid = tu.host_prefix((tw[0][:k], tw[1][:k]), groups)
    b, end2 = tu.host_prefix((tw[0][k:], tw[1][k:]), groups, carry=mid)
    tu.same_floats(np.concatenate([a, b]), whole)
    np.testing.assert_array_equal(end2[0], end[0])
    np.testing.assert_array_equal(end2[1], end[1])


def test_the_gap_constructions_hold_with_the_oracle(built):
    """The selection of timewise_device_util.gap_case is empty in exactly the frames of GAP — one whole block of the five —
    and the error is NaN there for that reason alone; leading_gap_case starts with five such frames."""
    system, xyz = tu.gap_case()
    eng = oracle.OracleEngine(system.tables, trig=oracle.TRIG_DIRECT)
    eng.submit(xyz, None)
    eng.finish()
    sums, counts = eng.timewise(tu.GAP_FRAMES)
    per_frame = counts[:, 0, :].sum(axis=1)
    assert (per_frame[tu.GAP[0]:tu.GAP[1]] == 0).all()
    full = int(system.tables.n_samples_per_frame)
    assert (np.delete(per_frame, np.arange(*tu.GAP)) == full).all()
    bs = tu.GAP_FRAMES // tu.GAP_BLOCKS
    empty_blocks = [b for b in range(tu.GAP_BLOCKS) if per_frame[b * bs:(b + 1) * bs].sum() == 0]
    assert empty_blocks == [2]
    groups = tu.type_groups(system)
    assert np.isnan(tu.host_errors((sums, counts), groups, tu.GAP_BLOCKS)[:, 0]).all()
    assert not np.isnan(tu.host_errors((sums, counts), groups, 2)[:, 0]).any()      # two blocks of ten: both sampled
    system, xyz = tu.leading_gap_case()
    eng = oracle.OracleEngine(system.tables, trig=oracle.TRIG_DIRECT)
    eng.submit(xyz, None)
    eng.finish()
    tw = eng.timewise(len(xyz))
    assert (tw[1][:5, 0].sum(axis=1) == 0).all() and (tw[1][5:, 0].sum(axis=1) == full).all()
    prefix, _ = tu.host_prefix(tw, groups)
    assert np.isnan(prefix[:5, 0]).all() and not np.isnan(prefix[5:, 0]).any()


def test_the_planar_bonds_give_negative_sums_that_do_not_divide(built):
    system, xyz = tu.planar_aa_case()
    eng = oracle.OracleEngine(system.tables, trig=oracle.TRIG_DIRECT)
    eng.submit(xyz, system.box9(len(xyz)))
    res = eng.finish()
    assert (res.sums[0] < 0).all() and (res.order()[0] < -0.45).all()
    bs, bc, _ = tu.host_blocks(eng.timewise(len(xyz)), 5)
    assert ((bs[:, 0] < 0) & (np.abs(bs[:, 0]) % bc[:, 0].astype(np.int64) != 0)).any()


def test_abi_symbols_are_in_the_built_library(built):
    lib = abi.load_library()
    for name in ("gorder_hip_timewise_chunk_frames", "gorder_hip_timewise_rows", "gorder_hip_timewise_blocks",
                 "gorder_hip_error_estimate", "gorder_hip_convergence"):
        assert name in abi._EXPORTS and getattr(lib, name) is not None
    chunk = abi.timewise_chunk_frames()                                    # no device needed
    assert chunk >= 2 and chunk == lib.gorder_hip_timewise_chunk_frames()
    for name in ("timewise_blocks", "error_estimate", "convergence", "timewise_rows"):
        assert callable(getattr(abi.HipEngine, name))
    begin, slots = abi._pack_groups([[3, 1], [2], [0, 1, 2, 3]])
    assert begin.tolist() == [0, 2, 3, 7] and slots.tolist() == [3, 1, 2, 0, 1, 2, 3] and begin.dtype == slots.dtype == np.uint32
