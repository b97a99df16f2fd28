"""A handle keeps the development switches it found at gorder_hip_create (gorder_amd/csrc/switches.h): the environment is
flipped between create and the first submit, and the route, the statistics and the results are those of the setting at
create.  Three switches that used to be read at every submit — the two routes of the per-frame rows, k_local_decide on and
off, five prefetch registers — each against the oracle."""
import numpy as np
import pytest

from gorder_amd import HipEngine, synthetic
from gorder_amd.abi import LEAFLETS_GLOBAL, LEAFLETS_LOCAL, LEAFLETS_NONE, OrderMap
from oracle import oracle

pytestmark = pytest.mark.gpu


def flip(monkeypatch, name, at_create):
    """the setting at create -> the opposite one"""
    if at_create:
        monkeypatch.delenv(name)
    else:
        monkeypatch.setenv(name, "1")


def create_under(monkeypatch, name, at_create, tables, timing=False):
    """an engine created with `name` set or not, handed back with the environment saying the opposite"""
    if at_create:
        monkeypatch.setenv(name, "1")
    else:
        monkeypatch.delenv(name, raising=False)
    eng = HipEngine(tables)
    if timing:
        eng.kernel_time()                       # (switches the event pairs on: the kernels of the batches are then named)
    flip(monkeypatch, name, at_create)
    return eng


def run(eng, o, xyz, box, batches):
    for a, b in batches:
        eng.submit_host(xyz[a:b], box[a:b], np.arange(a, b))
        if o is not None:
            o.submit(xyz[a:b], box[a:b], np.arange(a, b))
    return eng.finish(), None if o is None else o.finish()


# ---- 1. GORDER_HIP_TW_GATHER: which kernel writes the per-frame rows -------------------------------------------------------
TW_FRAMES, TW_BATCHES = 41, ((0, 19), (19, 41))


@pytest.fixture(scope="module")
def rows_case(built):
    """test_extras_gpu.py's system with per-frame rows and staged maps, and the oracle's results, made once"""
    system = synthetic.cg_membrane(210, leaflets=LEAFLETS_NONE, n_types=2, timewise=True)
    bx = system.box
    system.tables.ordermap = OrderMap(enabled=True, plane=0, span_x=(0.0, float(bx[0])), span_y=(0.0, float(bx[1])), bin=(0.5, 0.7))
    xyz, box = system.frames(TW_FRAMES, seed=14), system.box9(TW_FRAMES)
    o = oracle.OracleEngine(system.tables, trig=oracle.TRIG_DIRECT, n_threads=2)
    for a, b in TW_BATCHES:
        o.submit(xyz[a:b], box[a:b], np.arange(a, b))
    want = o.finish()
    return system, xyz, box, want, o.timewise(TW_FRAMES)


@pytest.mark.parametrize("at_create", [True, False], ids=["set at create, deleted before the submits", "unset at create, set before the submits"])
def test_the_rows_kernel_is_the_one_chosen_at_create(rows_case, monkeypatch, at_create):
    system, xyz, box, want, (want_rows, want_row_counts) = rows_case
    eng = create_under(monkeypatch, "GORDER_HIP_TW_GATHER", at_create, system.tables, timing=True)
    got, _ = run(eng, None, xyz, box, TW_BATCHES)
    names = eng.kernel_names().split(" + ")
    assert ("k_bonds_extras" in names) == at_create and ("k_bonds_tiled_tw" in names) == (not at_create), names
    np.testing.assert_array_equal(got.sums, want.sums)
    np.testing.assert_array_equal(got.counts, want.counts)
    rows, row_counts = eng.timewise(TW_FRAMES)
    np.testing.assert_array_equal(rows, want_rows)
    np.testing.assert_array_equal(row_counts, want_row_counts)
    assert row_counts[:, 0].sum() > 0


# ---- 2. GORDER_HIP_LOCAL_NO_DECIDE: whether k_local_decide runs before the rows kernel ----------------------------------------
def test_local_decide_runs_as_decided_at_create(built, monkeypatch):
    system = synthetic.cg_membrane(700, leaflets=LEAFLETS_LOCAL, radius=2.5, n_types=2)
    n, batches = 8, ((0, 4), (4, 8))
    xyz, box = system.frames(n, seed=73), system.box9(n)
    o = oracle.OracleEngine(system.tables, trig=oracle.TRIG_DIRECT, n_threads=2)
    o.submit(xyz, box, np.arange(n))
    want = o.finish()
    assert want.counts[1].sum() > 0 and want.counts[2].sum() > 0
    got = {}
    for at_create, submits in ((False, 2), (True, 0)):
        eng = create_under(monkeypatch, "GORDER_HIP_LOCAL_NO_DECIDE", at_create, system.tables)
        got[at_create], _ = run(eng, None, xyz, box, batches)
        assert eng.local_decide_stats()["submits"] == submits, at_create
        np.testing.assert_array_equal(got[at_create].sums, want.sums)
        np.testing.assert_array_equal(got[at_create].counts, want.counts)
    np.testing.assert_array_equal(got[True].sums, got[False].sums)


# ---- 3. GORDER_HIP_NPF5: five prefetch registers (the kernel's name does not show the template argument) -------------------
def test_five_prefetch_registers_chosen_at_create(built, monkeypatch):
    """test_order_route_gpu.py's "orders" case: 70 lipids, global leaflets every frame, 9 frames as 5 + 4"""
    system = synthetic.cg_membrane(70, leaflets=LEAFLETS_GLOBAL, n_types=2)
    n, batches = 9, ((0, 5), (5, 9))
    xyz, box = system.frames(n, seed=21), system.box9(n)
    eng = create_under(monkeypatch, "GORDER_HIP_NPF5", True, system.tables, timing=True)
    o = oracle.OracleEngine(system.tables, trig=oracle.TRIG_DIRECT, n_threads=2)
    got, want = run(eng, o, xyz, box, batches)
    assert "k_bonds_tiled" in eng.kernel_names().split(" + ")
    stats = eng.speculation_stats()
    assert stats["batches"] == 1 and stats["enabled"], stats      # the second batch
    assert want.counts[1].sum() > 0 and want.counts[2].sum() > 0
    np.testing.assert_array_equal(got.sums, want.sums)
    np.testing.assert_array_equal(got.counts, want.counts)
