"""The arm of the order route (gorder_amd/csrc/order_route.h) that nothing else reaches at a small size: GORDER_HIP_NPF5
makes the three tiled kernels take five prefetch registers per thread where four would do.  A CG membrane of 70 lipids in two
molecule types with global leaflets every frame, 9 frames submitted as 5 + 4 (one whole stage and a partial one per batch;
the second batch can speculate): plain orders, per-frame rows and staged ordermaps, with and without the switch, against
the oracle and against each other."""
import numpy as np
import pytest

from gorder_amd import HipEngine, synthetic
from gorder_amd.abi import LEAFLETS_GLOBAL, OrderMap
from oracle import oracle

pytestmark = pytest.mark.gpu

N_FRAMES = 9
BATCHES = ((0, 5), (5, 9))
KERNEL = {"orders": "k_bonds_tiled", "rows": "k_bonds_tiled_tw", "maps": "k_bonds_tiled_maps"}


def make(case):
    system = synthetic.cg_membrane(70, leaflets=LEAFLETS_GLOBAL, n_types=2, timewise=case == "rows")
    if case == "maps":
        bx = system.box
        system.tables.ordermap = OrderMap(enabled=True, plane=0, span_x=(0.0, float(bx[0])), span_y=(0.0, float(bx[1])), bin=(0.5, 0.7))
    return system, system.frames(N_FRAMES, seed=21), system.box9(N_FRAMES)


def outputs(eng, case):
    res = eng.finish()
    out = {"sums": res.sums, "counts": res.counts}
    if case == "rows":
        out["row sums"], out["row counts"] = eng.timewise(N_FRAMES)
    if case == "maps":
        out["map sums"], out["map counts"] = res.map_sums, res.map_counts
    return out


@pytest.fixture(scope="module")
def want():
    """The oracle's outputs per case, made once."""
    cache = {}

    def get(case):
        if case not in cache:
            system, xyz, box = make(case)
            o = oracle.OracleEngine(system.tables, trig=oracle.TRIG_DIRECT, n_threads=2)
            for a, b in BATCHES:
                o.submit(xyz[a:b], box[a:b], np.arange(a, b))
            cache[case] = outputs(o, case)
        return cache[case]
    return get


@pytest.mark.parametrize("case", ["orders", "rows", "maps"])
def test_five_prefetch_registers_change_nothing(built, monkeypatch, want, case):
    system, xyz, box = make(case)
    got = {}
    for npf5 in (False, True):
        if npf5:
            monkeypatch.setenv("GORDER_HIP_NPF5", "1")
        else:
            monkeypatch.delenv("GORDER_HIP_NPF5", raising=False)
        eng = HipEngine(system.tables)
        eng.kernel_time()                       # (switches the event pairs on: the kernels of the batch are then named)
        for a, b in BATCHES:
            eng.submit_host(xyz[a:b], box[a:b], np.arange(a, b))
        got[npf5] = outputs(eng, case)
        names = eng.kernel_names().split(" + ")
        assert KERNEL[case] in names and ("k_map_accumulate" in names) == (case == "maps"), names
        stats = eng.speculation_stats()
        if case == "orders":
            assert stats["batches"] == 1 and stats["enabled"], stats      # the second batch
        if case == "maps":
            assert stats["batches"] == 0, stats
    ref = want(case)
    assert ref["counts"][1].sum() > 0 and ref["counts"][2].sum() > 0
    for key, value in ref.items():
        assert value.sum() != 0, key
        np.testing.assert_array_equal(got[False][key], value, err_msg=key)
        np.testing.assert_array_equal(got[True][key], got[False][key], err_msg=key)
