"""Ordermaps finished on the device (gorder_hip_ordermaps, k_map_finalise; kernels_ordermap.h).  The yardstick is never the
code under test: it is structure.ordermap_values on the raw maps the same handle's finish() copies to the host, and the
reference's own ordermap files.  Every comparison of values is bit for bit with NaN in the same tiles."""
import ctypes as C

import numpy as np
import pytest

from gorder_amd import HipEngine, abi, synthetic
from gorder_amd import structure as st
from gorder_amd.abi import LEAFLETS_GLOBAL, LEAFLETS_NONE, OrderMap
from golden_util import Fixture
from test_golden_oracle import master_frames, ordermap_setup
import ordermap_final_util as ou

pytestmark = pytest.mark.gpu

N_FRAMES = 4
GRIDS = {"91x91": ((0.1, 0.1), (91, 91)),         # 8281 tiles: 32 workgroups of 256 and one of 89, most tiles empty
         "7x5": ((1.5, 2.25), (7, 5))}            # 35 tiles: odd, less than one wave
N_ACC = 64                                        # bond types of synthetic.aa_membrane
GROUPS = [[5], [3, 40], [63, 5, 3, 40], list(range(N_ACC))]    # one slot, two apart, slots of other groups again, all


def aa_system(leaflets, grid):
    bin, _ = GRIDS[grid]
    system = synthetic.aa_membrane(n_lipids=8, leaflets=leaflets)
    system.tables.ordermap = OrderMap(enabled=True, plane=0, span_x=(0.0, float(system.box[0])), span_y=(0.0, float(system.box[1])),
                                      bin=bin)
    return system, system.frames(N_FRAMES, seed=9)


def engine(system, xyz, lo=0, hi=None):
    hi = len(xyz) if hi is None else hi
    eng = HipEngine(system.tables)
    eng.submit_host(xyz[lo:hi], system.box9(hi - lo), np.arange(lo, hi))
    return eng


@pytest.fixture(scope="module")
def ua(built):
    return Fixture("ua")


@pytest.mark.parametrize("leaflets", [False, True])
def test_the_united_atom_golden_system(ua, leaflets):
    tables, labels, midx, om = ordermap_setup(ua, leaflets=leaflets)
    frames = ua.window()
    eng = HipEngine(tables)
    eng.submit_host(master_frames(ua, midx, frames), ua.boxes[frames], frames)
    groups = st.ordermap_groups(labels, "ua")
    slots = [g.slots for g in groups]
    got = eng.ordermaps(slots, min_samples=ou.MIN_SAMPLES, negate=True)
    assert got.shape == (len(groups), 3, 14, 4) and got.dtype == np.float32        # 56 tiles: less than one wave
    ou.same_bits(got, st.ordermap_values(eng.finish(), slots, ou.MIN_SAMPLES, negate=True))
    seen = ou.check_goldens(got, groups, om, leaflets)
    assert seen == (set(ou.golden_names()) if leaflets else {n for n in ou.golden_names() if n.endswith("_full")})
    assert np.isnan(got[:, 0]).any() and not np.isnan(got[:, 0]).all()
    if not leaflets:
        assert np.isnan(got[:, 1:]).all()


@pytest.fixture(scope="module")
def aa_runs(built):
    """(engine, its finish(), system, frames) per (leaflets, grid), made once; no test changes them."""
    cache = {}

    def run(leaflets, grid):
        if (leaflets, grid) not in cache:
            system, xyz = aa_system(LEAFLETS_GLOBAL if leaflets else LEAFLETS_NONE, grid)
            eng = engine(system, xyz)
            cache[leaflets, grid] = (eng, eng.finish(), system, xyz)
        return cache[leaflets, grid]
    return run


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("min_samples", [1, 3])
def test_synthetic_membrane_with_leaflets(aa_runs, grid, min_samples):
    eng, res, _, _ = aa_runs(True, grid)
    assert eng.n_acc == N_ACC and eng.ordermap_dims() == GRIDS[grid][1]
    plain = eng.ordermaps(GROUPS, min_samples=min_samples, negate=False)
    want = st.ordermap_values(res, GROUPS, min_samples, negate=False)
    assert plain.shape == (len(GROUPS), 3) + GRIDS[grid][1]
    ou.same_bits(plain, want)
    numbers = ~np.isnan(want)
    assert numbers[3].any() and not numbers[3].all()                    # tiles above and below min_samples
    assert numbers[:, 1].any() and numbers[:, 2].any()                  # both leaflets hold numbers
    if min_samples == 1:
        assert numbers[0].any() and numbers[1].any()                    # the small groups too
    assert (want[numbers] > 0).any() and (want[numbers] < 0).any()
    negated = eng.ordermaps(GROUPS, min_samples=min_samples, negate=True)
    ou.same_bits(negated, st.ordermap_values(res, GROUPS, min_samples, negate=True))
    np.testing.assert_array_equal(np.isnan(negated), np.isnan(plain))
    np.testing.assert_array_equal(negated.view(np.uint32)[numbers] ^ plain.view(np.uint32)[numbers], np.uint32(0x80000000))


@pytest.mark.parametrize("grid", list(GRIDS))
def test_synthetic_membrane_without_leaflets(aa_runs, grid):
    eng, res, _, _ = aa_runs(False, grid)
    for min_samples in (1, 3):
        got = eng.ordermaps(GROUPS, min_samples=min_samples, negate=True)
        assert np.isnan(got[:, 1:]).all() and not np.isnan(got[:, 0]).all()
        ou.same_bits(got, st.ordermap_values(res, GROUPS, min_samples, negate=True))


def exported(eng, shape):
    import torch
    s = torch.zeros(int(np.prod(shape)), dtype=torch.int64, device="cuda")
    c = torch.zeros_like(s)
    eng.export_maps(s, c)
    return s, c


@pytest.mark.parametrize("grid", list(GRIDS))
def test_device_maps_of_two_shards(aa_runs, grid):
    whole, res, system, xyz = aa_runs(True, grid)
    want = whole.ordermaps(GROUPS, min_samples=2)
    a, b = engine(system, xyz, 0, N_FRAMES // 2), engine(system, xyz, N_FRAMES // 2, N_FRAMES)
    (sa, ca), (sb, cb) = exported(a, res.map_sums.shape), exported(b, res.map_sums.shape)
    sums, counts = sa + sb, ca + cb
    ou.same_bits(a.ordermaps(GROUPS, min_samples=2, device_maps=(sums, counts)), want)
    np.testing.assert_array_equal(sums.cpu().numpy().reshape(res.map_sums.shape), res.map_sums)      # (the arrays were left alone)
    assert not np.array_equal(a.ordermaps(GROUPS, min_samples=2).view(np.uint32), want.view(np.uint32))   # a's own maps: half the frames
    # a tile that was sampled and whose ticks add up to nothing: 0.0, and -0.0 when negated
    tile = int(np.flatnonzero(res.map_counts[0, 5].ravel() >= 1)[0])
    sums[5 * res.map_sums[0, 0].size + tile] = 0
    zero = a.ordermaps([[5]], min_samples=1, negate=False, device_maps=(sums, counts))[0, 0].ravel()
    minus = a.ordermaps([[5]], min_samples=1, negate=True, device_maps=(sums, counts))[0, 0].ravel()
    assert zero.view(np.uint32)[tile] == 0 and minus.view(np.uint32)[tile] == 0x80000000


def test_own_maps_after_the_library_allreduce(aa_runs):
    """gorder_hip_allreduce on a communicator of one rank (all one GPU can host; most of this test's time is RCCL's start):
    the handle's own maps are then those of the whole analysis, and the call reads them."""
    whole, _, system, xyz = aa_runs(True, "7x5")
    one = engine(system, xyz)
    comm = one.comm_create(HipEngine.comm_unique_id(), 1, 0)
    one.allreduce(comm)
    ou.same_bits(one.ordermaps(GROUPS, min_samples=2), whole.ordermaps(GROUPS, min_samples=2))
    one.comm_destroy(comm)


def test_after_reset_and_after_more_submits(built):
    system, xyz = aa_system(LEAFLETS_GLOBAL, "7x5")
    eng = engine(system, xyz, 0, 2)
    before = eng.finish()
    first = eng.ordermaps(GROUPS, min_samples=1)
    after = eng.finish()
    np.testing.assert_array_equal(before.map_sums, after.map_sums)              # the call leaves the maps intact
    np.testing.assert_array_equal(before.map_counts, after.map_counts)
    ou.same_bits(first, st.ordermap_values(before, GROUPS, 1))
    eng.submit_host(xyz[2:], system.box9(N_FRAMES - 2), np.arange(2, N_FRAMES))
    second = eng.ordermaps(GROUPS, min_samples=1)                               # no finish() in between: the call folds the maps itself
    longer = eng.finish()
    assert longer.n_frames == N_FRAMES and longer.map_counts.sum() > before.map_counts.sum()
    ou.same_bits(second, st.ordermap_values(longer, GROUPS, 1))
    assert not np.array_equal(np.isnan(first), np.isnan(second)) or not np.array_equal(first[~np.isnan(first)], second[~np.isnan(second)])
    eng.reset()
    empty = eng.ordermaps(GROUPS, min_samples=1)
    assert empty.shape == second.shape and np.isnan(empty).all()


def test_after_run_trajectory(built, tmp_path):
    """The frames from an XTC file through gorder_hip_run_trajectory, two batches: the call finishes that run's maps."""
    from gorder_amd import xtc
    system, xyz = aa_system(LEAFLETS_GLOBAL, "7x5")
    path = str(tmp_path / "frames.xtc")
    xtc.write_trajectory(path, xyz, system.box9(N_FRAMES), precision=1000.0)
    eng = HipEngine(system.tables)
    stats = eng.run_trajectory([path], threads=2, batch_frames=3)
    assert stats["n_frames"] == N_FRAMES
    got = eng.ordermaps(GROUPS, min_samples=1)
    res = eng.finish()
    assert res.n_frames == N_FRAMES and res.map_counts.sum() > 0
    ou.same_bits(got, st.ordermap_values(res, GROUPS, 1))


def call(eng, begin, slots, n_groups, min_samples=1, d_sums=None, d_counts=None, n_u64=0, out=True):
    """gorder_hip_ordermaps as a C client calls it -> (status, message)."""
    begin, slots = np.asarray(begin, dtype=np.uint32), np.asarray(slots, dtype=np.uint32)
    nx, ny = eng.ordermap_dims()
    buf = np.zeros(max(1, n_groups * 3 * nx * ny), dtype=np.float32)
    st_ = eng.lib.gorder_hip_ordermaps(eng._h, begin.ctypes.data_as(C.c_void_p), slots.ctypes.data_as(C.c_void_p), n_groups, min_samples, 1,
                                       d_sums, d_counts, n_u64, buf.ctypes.data_as(C.c_void_p) if out else None)
    return st_, eng.lib.gorder_hip_last_error_message(eng._h).decode()


def test_invalid_arguments(aa_runs):
    eng, res, system, xyz = aa_runs(True, "7x5")
    n = res.map_sums.size
    s, c = exported(eng, res.map_sums.shape)
    ps, pc = C.c_void_p(s.data_ptr()), C.c_void_p(c.data_ptr())
    assert call(eng, [0, 2, 3], [1, 2, 3], 2, d_sums=ps, d_counts=pc, n_u64=n)[0] == abi.OK
    cases = {
        "min_samples == 0": dict(begin=[0, 2], slots=[1, 2], n_groups=1, min_samples=0),
        "no group": dict(begin=[0], slots=[1], n_groups=0),
        "an empty group": dict(begin=[0, 2, 2, 3], slots=[1, 2, 3], n_groups=3),
        "a slot >= n_acc": dict(begin=[0, 2], slots=[1, N_ACC], n_groups=1),
        "group_begin not ascending": dict(begin=[0, 3, 2, 3], slots=[1, 2, 3], n_groups=3),
        "only d_sums": dict(begin=[0, 1], slots=[1], n_groups=1, d_sums=ps, n_u64=n),
        "only d_counts": dict(begin=[0, 1], slots=[1], n_groups=1, d_counts=pc, n_u64=n),
        "n_u64 too small": dict(begin=[0, 1], slots=[1], n_groups=1, d_sums=ps, d_counts=pc, n_u64=n - 1),
        "n_u64 too large": dict(begin=[0, 1], slots=[1], n_groups=1, d_sums=ps, d_counts=pc, n_u64=n + 1),
        "a null output": dict(begin=[0, 1], slots=[1], n_groups=1, out=False),
    }
    seen = set()
    for name, kw in cases.items():
        status, message = call(eng, **kw)
        assert status == abi.ERR_INVALID_ARGUMENT, name
        assert message.startswith("gorder_hip_ordermaps: ") and len(message) > len("gorder_hip_ordermaps: "), (name, message)
        seen.add(message)
    assert len(seen) >= 8                                                       # the messages tell the cases apart
    # through the Python class the same refusals raise
    with pytest.raises(abi.GorderHipError) as e:
        eng.ordermaps([[1], []])
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
    with pytest.raises(abi.GorderHipError):
        eng.ordermaps([])
    # ordermaps off
    off = HipEngine(synthetic.aa_membrane(n_lipids=8).tables)
    status, message = call(off, [0, 1], [1], 1)
    assert status == abi.ERR_INVALID_ARGUMENT and message.startswith("gorder_hip_ordermaps: ")
    with pytest.raises(abi.GorderHipError):
        off.ordermaps([[1]])
    # and the handle still works
    ou.same_bits(eng.ordermaps(GROUPS), st.ordermap_values(res, GROUPS, 1))
