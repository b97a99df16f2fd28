"""Every host loop that cuts a batch into launch groups ("slabs") and every grid-stride loop behind a capped grid, run past
its limit ("Launch limits"): the offsets a second slab or a second trip of a grid-stride loop works with are
wrong silently — plausible numbers from there on — unless a test goes there.

Every comparison is exact: sums, counts, flags and cloud sizes EQUAL the oracle's (TRIG_DIRECT; flags of the clustering
methods from tests/spectral_ref.py / tests/spherical_ref.py), and where the same handle can run in one launch group the
result is bit-equal to that run as well.  The two inexact comparisons are the suite's own, taken over as they are: dynamic
normals against the oracle < 1e-6 (test_extras_gpu.py::test_dynamic_normals), leaflet distances atol = 2e-5
(test_speculation_gpu.py::both).  No head of these inputs lies near its mid-plane (asserted: min |distance| > 1e-3 nm on the
oracle's distances), so flags are compared outright.

The limits are the constants below, each with the place in gorder_amd/csrc that states it; every test asserts that its
sizes lie beyond its limit, and where the handle tells (kernel_groups(), speculation_stats()) that the work was cut."""
import numpy as np
import pytest

import spectral_ref as spec_ref
import spherical_ref as sph_ref
import test_spectral_gpu as tsg
import test_spherical_gpu as tsp
from gorder_amd import HipEngine, abi, synthetic, xtc
from gorder_amd.abi import (COLLECT_LEAFLETS, COLLECT_NORMALS, FLAG_CLUSTER_CUTOFF, FLAG_TRIG_ACOS_COS, LEAFLETS_GLOBAL,
                            LEAFLETS_INDIVIDUAL, LEAFLETS_LOCAL)
from oracle import oracle
from test_extras_gpu import _with_dynamic_normals
from test_spectral_cutoff_gpu import with_flag
from test_trr_device_gpu import tiny_engine, unpack
from trr_files import write_trr

pytestmark = pytest.mark.gpu

# (file:line as of the commit that added this file; the launch expressions are easier to find by the kernel's name)
LOCAL_SLAB_MIN = 4              # kernels_leaflets.h:640 local_slab_frames: GORDER_HIP_LOCAL_SLAB is raised to at least 4
SPEC_CHECK_GRID = 2048          # gorder_hip.hip:2156 k_spec_check: min(n_frames, 2048) workgroups
SPEC_EXACT_GRID = 512           # gorder_hip.hip:1802 run_leaflets: the global kernels behind a speculative batch, min(frames, 512)
SPEC_FIXUP_PAIRS = 4096 * 64    # gorder_hip.hip:2159 k_spec_fixup: min(pairs / 64, 4096) workgroups of 64 threads
GRID_Y_MAX = 65535              # gorder_hip.hip:1816 k_leaflets_individual and :3281 k_trr_unpack
BATCH_END_THREADS = 256 * 256   # gorder_hip.hip:2205 k_batch_end: min(frames / 256, 256) workgroups of 256 threads
CLUSTER_SLAB_MAX = 1024         # gorder_hip.hip:1452 cl_slab = min(512 MiB / bytes per frame, 1024)
SPHERICAL_RESIDENT = 16 * 1024  # gorder_hip.hip:1407 and kernels_leaflets.h:2194: kSphKeep = 16 distances in each of 1024 threads

SWITCHES = ("GORDER_HIP_LOCAL_SLAB", "GORDER_HIP_LOCAL_THREE_KERNELS", "GORDER_HIP_LOCAL_NO_DECIDE",
                  "GORDER_HIP_LOCAL_DECIDE_NOTHING", "GORDER_HIP_LOCAL_NO_SUMS", "GORDER_HIP_LOCAL_ATOMS_ONLY",
                  "GORDER_HIP_LOCAL_NO_PRUNE", "GORDER_HIP_SPHERICAL_SLAB", "GORDER_HIP_NO_SPECULATE")
_CACHE = {}


def clean_env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def segments(eng, name):
    """how often the timed group `name` was opened by the submits since kernel_time(reset=True)"""
    eng.kernel_time()
    return sum(n for label, _, n in eng.kernel_groups() if label == name)


def oracle_frame_by_frame(tables, xyz, box, frames=None, trig=oracle.TRIG_DIRECT):
    """The oracle fed a frame at a time (as test_collect_gpu.py does) -> (Results, assignment frames, flags [rows, molecules],
    distances [rows, molecules]); `frames`: the trajectory indices of xyz's frames."""
    o = oracle.OracleEngine(tables, trig=trig)
    frames = np.arange(xyz.shape[0]) if frames is None else np.asarray(frames)
    at, flags, dist = [], [], []
    for k, f in enumerate(frames):
        o.submit(xyz[[k]], None if box is None else box[[k]], [int(f)])
        fl, d, a = o.leaflets()
        if a == f:
            at.append(a); flags.append(fl); dist.append(d)
    return o.finish(), np.array(at), np.array(flags), np.array(dist)


def oracle_first_error(tables, xyz, box, first=0):
    """The oracle fed a frame at a time from frame `first` on -> (status, index, frame) of the frame that fails."""
    o = oracle.OracleEngine(tables, trig=oracle.TRIG_DIRECT)
    for f in range(first, xyz.shape[0]):
        try:
            o.submit(xyz[[f]], None if box is None else box[[f]], [f])
        except oracle.OracleError as e:
            return e.status, e.index, f
    raise AssertionError("the oracle accepts every frame")


def device_error(tables, xyz, box):
    eng = HipEngine(tables)
    with pytest.raises(abi.GorderHipError) as e:
        eng.submit_host(xyz, box, np.arange(xyz.shape[0]))
        eng.finish()
    return e.value.status, e.value.index, e.value.frame


# ---- 1. local leaflets across slabs ----------------------------------------------------------------------------------------
LOCAL_ROUTES = {"default": None, "three kernels": "GORDER_HIP_LOCAL_THREE_KERNELS", "no decide": "GORDER_HIP_LOCAL_NO_DECIDE",
                "decide nothing": "GORDER_HIP_LOCAL_DECIDE_NOTHING", "no sums": "GORDER_HIP_LOCAL_NO_SUMS"}
LOCAL_CASES = [(True, route, fq, False) for route in LOCAL_ROUTES for fq in (1, 2)] + \
              [(False, "default", fq, False) for fq in (1, 2)] + [(pbc, "default", fq, True) for pbc in (True, False) for fq in (1, 2)]


def local_case(pbc, frequency, movers=False):
    """movers: from every frame on another lipid is on the other side, so that no two assignment frames have the same flags
    (the plain membrane's rows are all alike: a row of another frame in a frame's place would not show in them)"""
    key = ("local", pbc, frequency, movers)
    if key not in _CACHE:
        system = synthetic.cg_membrane(96, leaflets=LEAFLETS_LOCAL, radius=2.0, n_types=2, handle_pbc=pbc, frequency=frequency)
        n = 11 if frequency == 1 else 19
        xyz, box = system.frames(n, seed=17), (system.box9(n) if pbc else None)
        if movers:
            for f in range(1, n):
                a = slice(12 * 5 * f, 12 * 5 * f + 12)
                xyz[f:, a, 2] = system.box[2] - xyz[f:, a, 2]
        _CACHE[key] = (system, xyz, box) + oracle_frame_by_frame(system.tables, xyz, box)
    return _CACHE[key]


def local_run(system, xyz, box):
    eng = HipEngine(system.tables)
    eng.set_collect(COLLECT_LEAFLETS)
    eng.kernel_time(reset=True)
    eng.submit_host(xyz, box, np.arange(xyz.shape[0]))
    return eng, eng.finish()


@pytest.mark.parametrize("pbc,route,frequency,movers", LOCAL_CASES)
def test_local_leaflets_across_slabs(built, monkeypatch, pbc, route, frequency, movers):
    """11 (frequency 2: 10, every other frame) assignment frames in slabs of 4 + 4 + 3 (4 + 4 + 2): lo.aframes + done,
    lo.row0 + done, the distances of the last slab's last frame, the per-slab scratch (d_lneed, d_lcell_fill) and the report
    summed over the slabs."""
    clean_env(monkeypatch)
    system, xyz, box, want, want_at, want_flags, want_dist = local_case(pbc, frequency, movers)
    n_assign = len(want_at)
    assert n_assign == (11 if frequency == 1 else 10) and n_assign > 2 * LOCAL_SLAB_MIN
    np.testing.assert_array_equal(want_at, np.arange(0, xyz.shape[0], frequency))
    assert np.abs(want_dist).min() > 1e-3
    if movers:
        assert all((want_flags[f] != want_flags[g]).any() for f in range(n_assign) for g in range(f))
    if LOCAL_ROUTES[route]:
        monkeypatch.setenv(LOCAL_ROUTES[route], "1")
    whole, whole_res = local_run(system, xyz, box)
    monkeypatch.setenv("GORDER_HIP_LOCAL_SLAB", str(LOCAL_SLAB_MIN))
    eng, got = local_run(system, xyz, box)
    cell_list = "k_local_bin + k_local_scan + k_local_scatter" if route == "three kernels" else "k_local_build"
    assert segments(eng, cell_list) >= 3 and segments(whole, cell_list) == 1
    flags, at = eng.collected_leaflets()
    np.testing.assert_array_equal(at, want_at)
    np.testing.assert_array_equal(flags, want_flags)
    assert 0 < flags.sum() < flags.size
    np.testing.assert_array_equal(got.sums, want.sums)
    np.testing.assert_array_equal(got.counts, want.counts)
    assert got.n_frames == want.n_frames == xyz.shape[0]
    last, last_at = eng.leaflets()
    assert last_at == want_at[-1]
    np.testing.assert_array_equal(last, want_flags[-1])
    np.testing.assert_allclose(eng.leaflet_distances(), want_dist[-1], atol=2e-5)
    # one launch group: the same bits
    np.testing.assert_array_equal(flags, whole.collected_leaflets()[0])
    np.testing.assert_array_equal(got.sums, whole_res.sums)
    np.testing.assert_array_equal(got.counts, whole_res.counts)
    # (the distances are compared with the oracle's above and not bit for bit: the records of a cell are summed in the order
    # the cell list's atomics placed them, which differs from run to run in the last bit of a local centre)
    stats = eng.local_decide_stats()
    assert stats == whole.local_decide_stats()
    if pbc and route != "no decide":
        assert stats["submits"] == 1 and stats["frames"] == n_assign      # the report is the sum over the slabs


@pytest.mark.parametrize("pbc", [True, False])
def test_local_leaflets_error_frame_across_slabs(built, monkeypatch, pbc):
    """An undefined head in the second and in the third slab: the first one is reported, under its frame of the trajectory."""
    clean_env(monkeypatch)
    system, xyz, box = local_case(pbc, 1)[:3]
    monkeypatch.setenv("GORDER_HIP_LOCAL_SLAB", str(LOCAL_SLAB_MIN))
    both = xyz.copy()
    both[9, 5 * 12 + 1, 0] = np.nan
    both[6, 7 * 12 + 1, 0] = np.nan
    want = oracle_first_error(system.tables, both, box)
    assert want[2] == 6
    assert device_error(system.tables, both, box) == want
    third = xyz.copy()
    third[9, 5 * 12 + 1, 0] = np.nan
    want = oracle_first_error(system.tables, third, box)
    assert want[2] == 9
    assert device_error(system.tables, third, box) == want


# ---- 2. dynamic normals across slabs ---------------------------------------------------------------------------------------
def dynamic_case(pbc):
    system = _with_dynamic_normals(synthetic.cg_membrane(300, leaflets=LEAFLETS_INDIVIDUAL, n_types=2, handle_pbc=pbc), 2.2)
    n = 11
    return system, system.frames(n, seed=12), (system.box9(n) if pbc else None)


def dynamic_run(system, xyz, box):
    eng = HipEngine(system.tables)
    eng.set_collect(COLLECT_NORMALS)
    eng.kernel_time(reset=True)
    eng.submit_host(xyz, box, np.arange(xyz.shape[0]))
    return eng, eng.finish()


@pytest.mark.parametrize("pbc", [True, False])
def test_dynamic_normals_across_slabs(built, monkeypatch, pbc):
    """11 frames in slabs of 4 + 4 + 3: lo.frame0 = done, the cell list and d_dyn_cov reused by every slab, k_dyn_eigen writing
    under the frame of the batch.  (The handle gives the cloud sizes of the last frame only; the other frames' sizes are
    behind their normals, which are compared for every frame.)"""
    clean_env(monkeypatch)
    system, xyz, box = dynamic_case(pbc)
    n = xyz.shape[0]
    assert n > 2 * LOCAL_SLAB_MIN
    whole, whole_res = dynamic_run(system, xyz, box)
    monkeypatch.setenv("GORDER_HIP_LOCAL_SLAB", str(LOCAL_SLAB_MIN))
    eng, got = dynamic_run(system, xyz, box)
    assert segments(eng, "k_dyn_cov + k_dyn_eigen") == 3 and segments(whole, "k_dyn_cov + k_dyn_eigen") == 1
    normals, at = eng.collected_normals()
    np.testing.assert_array_equal(at, np.arange(n))
    assert normals.shape == (n, system.tables.n_molecules_total, 3) and not np.isnan(normals).any()
    assert normals.tobytes() == whole.collected_normals()[0].tobytes()
    assert all(normals[f].tobytes() != normals[f - LOCAL_SLAB_MIN].tobytes() for f in range(LOCAL_SLAB_MIN, n))
    last, k_last = eng.normals()
    w_last, wk_last = whole.normals()
    assert last.tobytes() == w_last.tobytes() == normals[-1].tobytes()
    np.testing.assert_array_equal(k_last, wk_last)
    np.testing.assert_array_equal(got.sums, whole_res.sums)
    np.testing.assert_array_equal(got.counts, whole_res.counts)
    o = oracle.OracleEngine(system.tables, trig=oracle.TRIG_DIRECT, n_threads=2)
    o.submit(xyz, box, np.arange(n))
    want = o.finish()
    n_ref, k_ref = o.normals()
    np.testing.assert_array_equal(k_last, k_ref)
    assert k_ref.min() >= 3 and np.abs(last - n_ref).max() < 1e-6
    np.testing.assert_array_equal(got.counts, want.counts)
    assert np.abs(got.order_ticks() - want.order_ticks()).max() <= 1


@pytest.mark.parametrize("pbc", [True, False])
def test_dynamic_normals_error_frame_across_slabs(built, monkeypatch, pbc):
    clean_env(monkeypatch)
    system, xyz, box = dynamic_case(pbc)
    monkeypatch.setenv("GORDER_HIP_LOCAL_SLAB", str(LOCAL_SLAB_MIN))
    xyz[9, 5 * 12 + 1, 0] = np.nan              # the head of lipid 5, third slab
    want = oracle_first_error(system.tables, xyz, box)
    assert want[2] == 9
    assert device_error(system.tables, xyz, box) == want


# ---- 3-5. a speculative batch of 2 100 frames ------------------------------------------------------------------------------
SPEC_FRAMES, SPEC_FIRST = 2103, 3
SPEC_SHIFTED = (8, 603, 2053, 2102)


def speculative_input():
    """Six lipids that change sides every few frames (the recipe of test_molecules_that_change_sides_are_moved) and four
    frames shifted by half a box along the normal, which k_spec_check leaves to the exact kernel."""
    if "spec" not in _CACHE:
        system = synthetic.cg_membrane(128, leaflets=LEAFLETS_GLOBAL, n_types=2)
        n = SPEC_FRAMES
        xyz = system.frames(n, seed=7).astype(np.float32)
        L = float(system.box[2])
        zc = L / 2
        movers = np.random.default_rng(3).choice(128, 6, replace=False)
        for f in range(n):
            for k, m in enumerate(movers):
                if (f // (2 + k % 5)) % 2:
                    a = slice(m * 12, m * 12 + 12)
                    xyz[f, a, 2] = (2 * zc - xyz[f, a, 2]).astype(np.float32)
        for f in SPEC_SHIFTED:
            xyz[f, :, 2] = np.mod(xyz[f, :, 2] + L / 2, L).astype(np.float32)
        box = system.box9(n)
        _, at, flags, dist = oracle_frame_by_frame(system.tables, xyz, box)
        np.testing.assert_array_equal(at, np.arange(n))
        _CACHE["spec"] = (xyz, box, flags, dist)
    return _CACHE["spec"]


def speculative_run(tables, xyz, box, monkeypatch, speculate):
    if speculate:
        monkeypatch.delenv("GORDER_HIP_NO_SPECULATE", raising=False)
    else:
        monkeypatch.setenv("GORDER_HIP_NO_SPECULATE", "1")
    eng = HipEngine(tables)
    eng.set_collect(COLLECT_LEAFLETS)
    n = xyz.shape[0]
    eng.submit_host(xyz[:SPEC_FIRST], box[:SPEC_FIRST], np.arange(SPEC_FIRST))
    eng.submit_host(xyz[SPEC_FIRST:], box[SPEC_FIRST:], np.arange(SPEC_FIRST, n))
    return eng, eng.finish()


@pytest.mark.parametrize("kind", ["plain", "per-frame rows", "literal cosine"])
def test_a_speculative_batch_past_every_grid_cap(built, monkeypatch, kind):
    """Frames 3-2102 as one batch: k_spec_check takes frames past its 2 048 workgroups in a second trip, k_spec_fixup pairs past
    4 096 x 64, and the exact kernel behind the batch (512 workgroups, the frames taken in turn) finds frames it must not
    skip at batch positions past 512."""
    clean_env(monkeypatch)
    xyz, box, want_flags, want_dist = speculative_input()
    n, n_batch, n_mol = SPEC_FRAMES, SPEC_FRAMES - SPEC_FIRST, 128
    assert np.abs(want_dist).min() > 1e-3
    # what the batch mispredicts (it routes by the assignment of the frame before it) and leaves to the exact kernel
    wrong = want_flags[SPEC_FIRST:] != want_flags[SPEC_FIRST - 1]
    exact_at = np.array(SPEC_SHIFTED) - SPEC_FIRST
    assert n_batch > SPEC_CHECK_GRID and n_batch * n_mol > SPEC_FIXUP_PAIRS
    assert 0 < wrong.sum() < n_batch * n_mol // 16 and wrong[SPEC_CHECK_GRID:].sum() > 0
    assert wrong.reshape(-1)[SPEC_FIXUP_PAIRS:].sum() > 0
    assert len(exact_at) < n_batch // 8 and (exact_at >= SPEC_EXACT_GRID).sum() >= 2
    system = synthetic.cg_membrane(128, leaflets=LEAFLETS_GLOBAL, n_types=2, timewise=kind == "per-frame rows")
    trig = oracle.TRIG_DIRECT
    if kind == "literal cosine":
        system.tables.flags |= FLAG_TRIG_ACOS_COS          # k_spec_fixup<true, false>
        trig = oracle.TRIG_MIRROR
    eng, got = speculative_run(system.tables, xyz, box, monkeypatch, True)
    stats = eng.speculation_stats()
    assert stats["batches"] == 1 and stats["exact_frames"] == len(SPEC_SHIFTED) and stats["moved"] > 0 and stats["enabled"]
    flags, at = eng.collected_leaflets()
    np.testing.assert_array_equal(at, np.arange(n))
    np.testing.assert_array_equal(flags, want_flags)
    o = oracle.OracleEngine(system.tables, trig=trig, n_threads=4)
    o.submit(xyz, box, np.arange(n))
    want = o.finish()
    plain, plain_res = speculative_run(system.tables, xyz, box, monkeypatch, False)
    assert plain.speculation_stats()["batches"] == 0
    for res in (got, plain_res):
        assert res.n_frames == n
        np.testing.assert_array_equal(res.sums, want.sums)
        np.testing.assert_array_equal(res.counts, want.counts)
    np.testing.assert_array_equal(plain.collected_leaflets()[0], want_flags)
    last, last_at = eng.leaflets()
    assert last_at == n - 1
    np.testing.assert_array_equal(last, want_flags[-1])
    np.testing.assert_allclose(eng.leaflet_distances(), want_dist[-1], atol=2e-5)
    if kind == "per-frame rows":
        ws, wc = o.timewise(n)
        for e in (eng, plain):
            gs, gc = e.timewise(n)
            np.testing.assert_array_equal(gc, wc)
            np.testing.assert_array_equal(gs, ws)


# ---- 6-7. 65 600 frames through individual leaflets and the box check -------------------------------------------------------
MANY_FRAMES, MANY_TAIL = 65600, 65530


def many_frames_case():
    if "many" not in _CACHE:
        system = synthetic.cg_membrane(8, leaflets=LEAFLETS_INDIVIDUAL)
        xyz = system.frames(MANY_FRAMES, seed=7)
        zc = float(system.box[2]) / 2
        for m in (1, 4, 6):                      # on the other side from frame 65 530 on: the second launch's rows differ
            a = slice(m * 12, m * 12 + 12)
            xyz[MANY_TAIL:, a, 2] = (2 * zc - xyz[MANY_TAIL:, a, 2]).astype(np.float32)
        _CACHE["many"] = (system, xyz, system.box9(MANY_FRAMES))
    return _CACHE["many"]


def test_individual_leaflets_past_grid_y(built, monkeypatch):
    """65 600 assignment frames in one submit: k_leaflets_individual is launched twice (65 535 + 65 rows of gridDim.y), the
    second time with aframes + done and row0 + done, the distances written by the last launch only."""
    clean_env(monkeypatch)
    system, xyz, box = many_frames_case()
    n = MANY_FRAMES
    assert n > GRID_Y_MAX and MANY_TAIL < GRID_Y_MAX < n - 1
    o = oracle.OracleEngine(system.tables, trig=oracle.TRIG_DIRECT, n_threads=4)
    o.submit(xyz, box, np.arange(n))
    want = o.finish()
    tail = np.arange(MANY_TAIL, n)
    _, at, want_flags, want_dist = oracle_frame_by_frame(system.tables, xyz[MANY_TAIL:], box[MANY_TAIL:], tail)
    np.testing.assert_array_equal(at, tail)
    assert np.abs(want_dist).min() > 1e-3
    before = oracle_frame_by_frame(system.tables, xyz[MANY_TAIL - 1:MANY_TAIL], box[:1], [MANY_TAIL - 1])[2][0]
    assert (want_flags != before).any(axis=1).all()                     # the tail's rows are not the rows before it
    eng = HipEngine(system.tables)
    eng.set_collect(COLLECT_LEAFLETS)
    eng.submit_host(xyz, box, np.arange(n))
    got = eng.finish()
    assert got.n_frames == n
    np.testing.assert_array_equal(got.sums, want.sums)
    np.testing.assert_array_equal(got.counts, want.counts)
    flags, frames = eng.collected_leaflets()
    np.testing.assert_array_equal(frames, np.arange(n))
    np.testing.assert_array_equal(flags[MANY_TAIL:], want_flags)
    np.testing.assert_array_equal(flags[MANY_TAIL - 1], before)
    last, last_at = eng.leaflets()
    assert last_at == n - 1
    np.testing.assert_array_equal(last, want_flags[-1])
    np.testing.assert_allclose(eng.leaflet_distances(), want_dist[-1], atol=2e-5)


def test_box_check_past_its_grid(built, monkeypatch):
    """k_batch_end checks the boxes with 256 workgroups of 256 threads: frame 65 590 is looked at in a thread's second trip."""
    clean_env(monkeypatch)
    system, xyz, box = many_frames_case()
    bad_at = 65590
    assert bad_at >= BATCH_END_THREADS
    bad = box.copy()
    bad[bad_at, 0, 1] = 0.3
    status, index, frame = oracle_first_error(system.tables, xyz, bad, first=bad_at - 10)
    assert (status, frame) == (abi.ERR_NOT_ORTHOGONAL_BOX, bad_at)
    assert device_error(system.tables, xyz, bad)[::2] == (status, frame)


# ---- 8. clustering past 1 024 assignment frames ----------------------------------------------------------------------------
CLUSTER_FRAMES, CLUSTER_MOVED_FROM = 1030, 1026


def cluster_case():
    if "cluster" not in _CACHE:
        t, frame, box, sides = tsg.two_sheets(64, True, seed=1)
        n = CLUSTER_FRAMES
        base = np.tile(frame[None], (n, 1, 1))
        base[CLUSTER_MOVED_FROM:] = tsg.moved(frame, sides, 3)      # 29 of 32 stay: matched (test_orientation_rules)
        xyz = (base + np.random.default_rng(5).normal(0, 0.01, (n,) + frame.shape)).astype(np.float32)
        bx, fi = tsg.box9(box, n), np.arange(n)
        ref = spec_ref.run(t, xyz, bx, fi)
        flags_of = {f: spec_ref.molecule_flags(t, ref[f]) for f in range(n)}
        # the float64 twin agrees where the input is not the plain sheets' (from the frame before the change on)
        tail = slice(CLUSTER_MOVED_FROM - 1, n)
        r64 = spec_ref.run(t, xyz[tail], bx[tail], fi[tail], np.float64)
        for f in fi[tail]:
            np.testing.assert_array_equal(ref[f]["upper"], r64[f]["upper"], err_msg=f"twins, frame {f}")
        want = tsg.oracle_route(t, xyz, bx, fi, flags_of)
        _CACHE["cluster"] = (t, xyz, bx, sides, ref, flags_of, want)
    return _CACHE["cluster"]


@pytest.mark.parametrize("route", ["dense", "cut-off"])
def test_clustering_past_the_slab(built, monkeypatch, route):
    """1 030 assignment frames, 1 024 + 6: aframes + done, row0 + done, cl_is0 + done, the orientation carried from frame 1 023
    into the second slab, statistics of the last frame.  From frame 1 026 on three molecules of each sheet have changed
    places, so the second slab's rows are not the first slab's.  (The larger sheet is upper with or without the carry: this
    input does not tell a carried orientation from a fresh one.)"""
    import torch
    clean_env(monkeypatch)
    t, xyz, bx, sides, ref, flags_of, want = cluster_case()
    n = CLUSTER_FRAMES
    assert n > CLUSTER_SLAB_MAX
    if route == "cut-off":
        t = with_flag(t)
    assert t.flags & FLAG_CLUSTER_CUTOFF == (FLAG_CLUSTER_CUTOFF if route == "cut-off" else 0)
    eng = HipEngine(t)
    eng.set_collect(COLLECT_LEAFLETS)
    eng.submit_host(xyz, bx, np.arange(n))
    got = eng.finish()
    flags, at = eng.collected_leaflets()
    np.testing.assert_array_equal(at, np.arange(n))
    np.testing.assert_array_equal(flags, np.array([flags_of[f] for f in range(n)]))
    np.testing.assert_array_equal(flags[:CLUSTER_MOVED_FROM], np.tile(sides, (CLUSTER_MOVED_FROM, 1)))
    assert ((flags[CLUSTER_MOVED_FROM:] != sides).sum(axis=1) == 6).all()
    tsg.assert_equal_results(got, want)
    last, last_at = eng.leaflets()
    assert last_at == n - 1
    np.testing.assert_array_equal(last, flags_of[n - 1])
    # the statistics are those of the last frame: a handle primed with the frame before it and given that frame alone
    stats = eng.clustering_stats()
    assert stats["n_upper"] == int(ref[n - 1]["upper"].sum()) and stats["n_lower"] == int((~ref[n - 1]["upper"]).sum())
    one = HipEngine(t)
    for f in (0, n - 2):
        one.prime_leaflets_device(torch.from_numpy(xyz[f]).cuda(), torch.from_numpy(bx[f]).cuda(), f)
    one.submit_host(xyz[n - 1:], bx[n - 1:], [n - 1])
    one.finish()
    alone = one.clustering_stats()
    for q in stats:
        assert np.array_equal(stats[q], alone[q]), q
    slab_end = HipEngine(t)                                  # (and not those of the first slab's last frame)
    for f in (0, CLUSTER_SLAB_MAX - 2):
        slab_end.prime_leaflets_device(torch.from_numpy(xyz[f]).cuda(), torch.from_numpy(bx[f]).cuda(), f)
    slab_end.submit_host(xyz[CLUSTER_SLAB_MAX - 1:CLUSTER_SLAB_MAX], bx[:1], [CLUSTER_SLAB_MAX - 1])
    slab_end.finish()
    assert not np.array_equal(slab_end.clustering_stats()["eigenvalues"], stats["eigenvalues"])


# ---- 9. spherical leaflets with spill rows across slabs ---------------------------------------------------------------------
def test_spherical_spill_rows_across_slabs(built, monkeypatch):
    """20 000 heads (16 384 distances in registers, the rest in a scratch row per frame of a launch), 5 frames in launches of
    2 + 2 + 1 (GORDER_HIP_SPHERICAL_SLAB=2): the rows reused by every launch, row0 + done, statistics and distances of the
    last launch."""
    clean_env(monkeypatch)
    system, sides = synthetic.cg_vesicle(20000, 12.0, 16.0, box=(40.0, 40.0, 40.0), sigma=0.3, seed=9, heads_only=True)
    t = system.tables
    assert len(t.leaflets.membrane) > SPHERICAL_RESIDENT
    n, slab = 5, 2
    xyz, box, fi = system.frames(n, seed=1), system.box9(n), np.arange(n)
    # three lipids of each shell change places with three of the other, other ones in every frame: the same points, another
    # row of flags for every frame (the plain vesicle's rows are all the same, and a row in the wrong place would not show)
    outer, inner = np.flatnonzero(sides == 0), np.flatnonzero(sides == 1)
    lipids = xyz.reshape(n, len(sides), 2, 3)
    for f in range(1, n):
        a, b = outer[3 * f:3 * f + 3], inner[3 * f:3 * f + 3]
        lipids[f, np.concatenate([a, b])] = lipids[f, np.concatenate([b, a])]

    def run(frames):
        eng = HipEngine(t)
        eng.set_collect(COLLECT_LEAFLETS)
        eng.submit_host(xyz[frames], box[frames], fi[frames])
        return eng, eng.finish()

    whole, whole_res = run(slice(0, n))
    monkeypatch.setenv("GORDER_HIP_SPHERICAL_SLAB", str(slab))
    assert n > 2 * slab
    eng, got = run(slice(0, n))
    flags, at = eng.collected_leaflets()
    np.testing.assert_array_equal(at, fi)
    flags_of = tsp.helper_flags(t, xyz, box, fi)
    np.testing.assert_array_equal(flags, np.array([flags_of[f] for f in range(n)]))
    np.testing.assert_array_equal(flags[0], sides)
    assert all((flags[f] != flags[g]).sum() >= 6 for f in range(n) for g in range(f))
    np.testing.assert_array_equal(flags, whole.collected_leaflets()[0])
    tsp.assert_equal_results(got, whole_res)
    tsp.assert_equal_results(got, tsp.oracle_route(t, xyz, box, fi, flags_of))
    assert eng.leaflets()[1] == n - 1
    # statistics and distances of the last frame: bit-equal to the one-launch handle's and to a handle given that frame alone
    alone, _ = run(slice(n - 1, n))
    first, _ = run(slice(0, 1))
    stats, w_stats, a_stats, f_stats = (e.spherical_stats() for e in (eng, whole, alone, first))
    for q in stats:
        assert np.array_equal(stats[q], w_stats[q]) and np.array_equal(stats[q], a_stats[q]), q
    assert not np.array_equal(stats["centre"], f_stats["centre"])
    assert eng.leaflet_distances().tobytes() == whole.leaflet_distances().tobytes() == alone.leaflet_distances().tobytes()
    ref = sph_ref.classify(xyz[-1], t.leaflets.membrane, system.box)
    assert stats["iterations"] == ref["iterations"]


# ---- 10. TRR frames past gridDim.y -----------------------------------------------------------------------------------------
def test_trr_unpack_past_grid_y(built, tmp_path):
    """65 540 single-precision frames of 5 atoms decoded by one launch: a block of k_trr_unpack takes frame blockIdx.y and, five
    of them, frame blockIdx.y + 65 535."""
    n, n_atoms = 65540, 5
    assert n > GRID_Y_MAX
    rng = np.random.default_rng(10)
    xyz = rng.uniform(-50.0, 50.0, size=(n, n_atoms, 3)).astype(np.float32)
    path = str(tmp_path / "many.trr")
    write_trr(path, xyz, None, np.arange(n, dtype=np.float64))
    ws = xtc.pack_trajectory([path], chunk=n)
    assert len(ws) == 1 and len(ws[0]["frames"]) == n
    w = ws[0]
    got = unpack(tiny_engine(), w["blob"], w["frames"], n_atoms, w["n_stop"], w["slot_of"], n_atoms)
    want = xyz.view(np.uint32)
    for f in (0, n - 1, 65534, 65535, 65536, 65537, 65538, 65539):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"frame {f}")
    assert not np.array_equal(want[65535], want[0]) and not np.array_equal(want[n - 1], want[n - 1 - GRID_Y_MAX])
    np.testing.assert_array_equal(got, want)
