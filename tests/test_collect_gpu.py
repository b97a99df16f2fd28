"""Collected history (gorder_hip_set_collect): every assignment frame's leaflet flags and every analysed frame's dynamic
membrane normals come out of the handle however the frames were cut into batches — several assignment frames in one
batch, the one-read speculative path, bit-packed rows at the word edges, the touched rule of bond systems with a
geometry selection, the trajectory driver with shards, and the life cycle of the switch."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gorder_amd import GorderHipError, HipEngine, abi, synthetic
from gorder_amd.abi import (COLLECT_LEAFLETS, COLLECT_NORMALS, GEOM_SPHERE, GEOMREF_POINT, LEAFLETS_GLOBAL, LEAFLETS_MANUAL,
                            DynamicNormal, Geometry, Leaflets, MolType, Tables)
from oracle import oracle
from golden_util import GOLDEN, METHODS, Fixture, cg_setup, expected
from test_golden_wide_oracle import EXPORTS, assignment_rows, check_normals, export_setup, normals_setup

pytestmark = pytest.mark.gpu

SPLITS = {"one batch": ((0, 51),), "three batches": ((0, 17), (17, 40), (40, 51))}   # an assignment frame first, inside, last


@pytest.fixture(scope="module")
def fixtures(built):
    return {k: Fixture(k) for k in ("pcpepg", "ua")}


# ---- 1. the reference's exported assignments, all frames in one batch ----------------------------------------------------
@pytest.mark.parametrize("kind,want,freq,n_rows", EXPORTS)
@pytest.mark.parametrize("method", ["global", "local", "individual"])
def test_leaflet_goldens_in_one_batch(fixtures, kind, want, freq, n_rows, method):
    fx, (tables, labels, midx) = export_setup(kind, freq, fixtures, method)
    rows = np.array(assignment_rows(expected(want), labels))
    assert len(rows) == n_rows
    xyz = np.ascontiguousarray(fx.xyz[:51][:, midx, :])
    for split in SPLITS.values():
        eng = HipEngine(tables)
        eng.set_collect(COLLECT_LEAFLETS)
        for a, b in split:
            eng.submit_host(xyz[a:b], fx.boxes[a:b], np.arange(a, b))
        flags, frames = eng.collected_leaflets()
        np.testing.assert_array_equal(frames, np.arange(0, 51, freq) if freq else [0])
        np.testing.assert_array_equal(flags, rows)
        assert eng.collected_counts() == (n_rows, 0)


# ---- 2. the one-read speculative path ----------------------------------------------------------------------------------
def speculative_case(n_lipids):
    system = synthetic.aa_membrane(n_lipids, leaflets=LEAFLETS_GLOBAL)
    return system, system.frames(12, seed=5), system.box9(12)


def speculative_rows(n_lipids):
    system, xyz, box = speculative_case(n_lipids)
    eng = HipEngine(system.tables)
    eng.set_collect(COLLECT_LEAFLETS)
    eng.submit_host(xyz[:5], box[:5], np.arange(5))
    eng.submit_host(xyz[5:], box[5:], np.arange(5, 12))
    flags, frames = eng.collected_leaflets()
    return flags, frames, eng.speculation_stats()["batches"]


@pytest.mark.parametrize("n_lipids", [8, 70])       # one partial ballot word; the word boundary at 64
def test_speculative_batches_keep_every_row(built, monkeypatch, tmp_path, n_lipids):
    monkeypatch.delenv("GORDER_HIP_NO_SPECULATE", raising=False)
    flags, frames, spec_batches = speculative_rows(n_lipids)
    assert spec_batches >= 1                          # gorder_hip_speculation_stats out[0]: the second batch ran in one read
    np.testing.assert_array_equal(frames, np.arange(12))
    system, xyz, box = speculative_case(n_lipids)
    o = oracle.OracleEngine(system.tables, trig=oracle.TRIG_DIRECT)
    for f in range(12):
        o.submit(xyz[[f]], box[[f]], [f])
        np.testing.assert_array_equal(flags[f], o.leaflets()[0])
    assert 0 < flags.sum() < flags.size
    # the two-kernel path, in a process of its own (the switch is read when a handle is created)
    code = ("import sys, numpy as np\nsys.path[:0] = [%r, %r]\nimport test_collect_gpu as t\n"
            "flags, frames, n = t.speculative_rows(%d)\nassert n == 0\nnp.save(sys.argv[1], flags)\n"
            % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)), n_lipids))
    out = str(tmp_path / "two_kernel_rows.npy")
    subprocess.run([sys.executable, "-c", code, out], check=True, timeout=120, env=dict(os.environ, GORDER_HIP_NO_SPECULATE="1"))
    np.testing.assert_array_equal(np.load(out), flags)


# ---- 3. bit packing at the word edges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mol", [1, 63, 64, 65, 129])
def test_bit_packing_edges(built, n_mol):
    ids = np.arange(n_mol, dtype=np.uint32)
    bonds = np.stack([2 * ids, 2 * ids + 1], axis=1)[None]
    tables = Tables(n_atoms=2 * n_mol, molecule_types=[MolType(n_molecules=n_mol, bonds=bonds, name="M")],
                    leaflets=Leaflets(method=LEAFLETS_MANUAL, frequency=3))
    rng = np.random.default_rng(n_mol)
    xyz = rng.uniform(0.5, 3.5, size=(3, 2 * n_mol, 3)).astype(np.float32)
    box = np.tile(np.diag([4.0, 4.0, 4.0]).astype(np.float32), (3, 1, 1))
    given = rng.integers(0, 2, size=(5, n_mol)).astype(np.uint8)
    given[1, -1], given[2, -1] = 1, 0                  # the last molecule's bit both ways
    at = [0, 3, 6, 9, 1000000000007]
    eng = HipEngine(tables)
    eng.set_collect(COLLECT_LEAFLETS)
    for k, f in enumerate(at):
        eng.set_manual_leaflets(given[k], f)
        if k < 4:
            eng.submit_host(xyz, box, np.arange(f, f + 3))
    flags, frames = eng.collected_leaflets()
    np.testing.assert_array_equal(frames, np.array(at, dtype=np.uint64))
    np.testing.assert_array_equal(flags, given)


# ---- 4. the reference's exported normals -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def normals_frame_by_frame(fixtures):
    fx, (tables, labels, midx) = normals_setup(fixtures)
    eng = HipEngine(tables)
    rows = []
    for f in range(51):
        eng.submit_host(np.ascontiguousarray(fx.xyz[[f]][:, midx, :]), fx.boxes[[f]], [f])
        rows.append(eng.normals()[0])
    return np.array(rows)


@pytest.mark.parametrize("split", sorted(SPLITS))
def test_normals_golden(fixtures, normals_frame_by_frame, split):
    fx, (tables, labels, midx) = normals_setup(fixtures)
    want = expected("ua_normals.yaml")
    xyz = np.ascontiguousarray(fx.xyz[:51][:, midx, :])
    eng = HipEngine(tables)
    eng.set_collect(COLLECT_NORMALS)
    for a, b in SPLITS[split]:
        eng.submit_host(xyz[a:b], fx.boxes[a:b], np.arange(a, b))
    normals, frames = eng.collected_normals()
    np.testing.assert_array_equal(frames, np.arange(51))
    assert normals.shape == (51, tables.n_molecules_total, 3) and normals.dtype == np.float32
    loose = sum(check_normals(normals[f].astype(np.float64), want, labels, f) for f in range(51))
    assert loose <= 30                                 # (the budget of the frame-by-frame test: it belongs to the golden)
    assert normals.tobytes() == normals_frame_by_frame.tobytes()


# ---- 5. AA / CG fetch a molecule's normal after the geometry test ------------------------------------------------------
TOUCHED_LIPIDS, TOUCHED_FRAMES, TOUCHED_SEED = 64, 6, 3
TOUCHED_POINT, TOUCHED_RADIUS = (2.4, 2.4, 5.0), 2.0


def touched_system(geometry: bool):
    system = synthetic.cg_membrane(TOUCHED_LIPIDS)
    mt = system.tables.molecule_types[0]
    mt.normal_heads = (np.arange(TOUCHED_LIPIDS) * 12 + 1).astype(np.uint32)
    system.tables.dynamic_normal = DynamicNormal(enabled=True, radius=2.0, cloud=mt.normal_heads)
    if geometry:
        system.tables.geometry = Geometry(kind=GEOM_SPHERE, reference=GEOMREF_POINT, point=TOUCHED_POINT, radius=TOUCHED_RADIUS,
                                          structure_box=tuple(float(x) for x in system.box))
    return system


def touched_reference(system, xyz):
    """numpy f64: per (frame, molecule) whether any bond's minimum-image midpoint lies inside the sphere, and whether one
    lies within 1e-4 nm of its surface (such a molecule is left out of the comparison)."""
    box = system.box.astype(np.float64)
    bonds = np.asarray(system.tables.molecule_types[0].bonds, dtype=np.int64)          # [types, molecules, 2]
    x = xyz.astype(np.float64)
    p1, p2 = x[:, bonds[..., 0], :], x[:, bonds[..., 1], :]                           # [frames, types, molecules, 3]
    v = p2 - p1
    v -= box * np.round(v / box)
    d = p1 + v / 2 - np.array(TOUCHED_POINT)
    d -= box * np.round(d / box)
    r = np.sqrt((d * d).sum(axis=-1))
    return (r < TOUCHED_RADIUS).any(axis=1), (np.abs(r - TOUCHED_RADIUS) < 1e-4).any(axis=1)


def test_touched_rule(built):
    system = touched_system(True)
    xyz, box = system.frames(TOUCHED_FRAMES, seed=TOUCHED_SEED), system.box9(TOUCHED_FRAMES)
    inside, near = touched_reference(system, xyz)
    assert near.mean() <= 0.02 and 0.3 < inside.mean() < 0.7
    fi = np.arange(TOUCHED_FRAMES)
    eng = HipEngine(system.tables)
    eng.set_collect(COLLECT_NORMALS)
    eng.submit_host(xyz, box, fi)
    normals, frames = eng.collected_normals()
    np.testing.assert_array_equal(frames, fi)
    isnan = np.isnan(normals)
    assert (isnan.all(axis=2) == isnan.any(axis=2)).all()
    np.testing.assert_array_equal(isnan.all(axis=2)[~near], ~inside[~near])
    # the normals that are there are the ones a frame-by-frame run reads back
    one = HipEngine(system.tables)
    for f in fi:
        one.submit_host(xyz[[f]], box[[f]], [f])
        keep = ~isnan[f].any(axis=1)
        assert normals[f][keep].tobytes() == one.normals()[0][keep].tobytes()
    # collection changes no order sum
    plain = HipEngine(system.tables)
    plain.submit_host(xyz, box, fi)
    got, want = eng.finish(), plain.finish()
    np.testing.assert_array_equal(got.sums, want.sums)
    np.testing.assert_array_equal(got.counts, want.counts)
    assert want.counts.sum() > 0
    # without a geometry selection every molecule's normal is fetched
    free = touched_system(False)
    eng = HipEngine(free.tables)
    eng.set_collect(COLLECT_NORMALS)
    eng.submit_host(xyz[:4], box[:4], fi[:4])
    eng.submit_host(xyz[4:], box[4:], fi[4:])
    normals, _ = eng.collected_normals()
    assert normals.shape[0] == TOUCHED_FRAMES and not np.isnan(normals).any()
    plain = HipEngine(free.tables)
    plain.submit_host(xyz, box, fi)
    np.testing.assert_array_equal(eng.finish().sums, plain.finish().sums)


# ---- 6. the trajectory driver, whole and in shards ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def cg(built):
    return Fixture("cg")


@pytest.mark.parametrize("device_decode", [False, True])
@pytest.mark.parametrize("source", ["cg3.xtc", "eleven frames"])
def test_driver_and_shards(cg, tmp_path, source, device_decode):
    """tests/golden/cg3.xtc holds a single frame (shard 0 of 2 is empty, shard 1 analyses it); the second file, eleven frames
    of the same fixture, makes shard 1 begin at frame 5, between two assignment frames: it primes with frame 4, which
    must not show up among its rows."""
    from gorder_amd import xtc
    tables, labels, midx = cg_setup(cg, leaflets=METHODS["global"], frequency=2)
    if source == "cg3.xtc":
        path = os.path.join(GOLDEN, "cg3.xtc")
    else:
        path = str(tmp_path / "eleven.xtc")
        fr = np.arange(11)
        xtc.write_trajectory(path, cg.xyz[fr], cg.boxes[fr], times=cg.times[fr], precision=100.0)

    def run(shard):
        eng = HipEngine(tables)
        eng.set_collect(COLLECT_LEAFLETS)
        stats = eng.run_trajectory([path], group=midx, step=1, threads=2, batch_frames=3, device_decode=device_decode, shard=shard)
        return eng.collected_leaflets() + (stats["n_frames"],)

    flags, frames, n = run(None)
    assert n == (1 if source == "cg3.xtc" else 11)
    np.testing.assert_array_equal(frames, np.arange(0, n, 2))
    assert 0 < flags.sum() < flags.size
    parts = [run((i, 2)) for i in range(2)]
    assert parts[0][2] + parts[1][2] == n and parts[1][2] > 0
    np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), frames)          # every assignment frame once
    np.testing.assert_array_equal(np.concatenate([p[0] for p in parts]), flags)


# ---- 7. life cycle -------------------------------------------------------------------------------------------------------
def test_lifecycle(built):
    system = synthetic.cg_membrane(40, leaflets=LEAFLETS_GLOBAL, frequency=2)
    xyz, box = system.frames(5, seed=2), system.box9(5)
    eng = HipEngine(system.tables)
    with pytest.raises(GorderHipError) as e:
        eng.set_collect(COLLECT_NORMALS)                 # no dynamic normals
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
    with pytest.raises(GorderHipError) as e:
        eng.collected_leaflets()                         # not being collected
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
    eng.set_collect(COLLECT_LEAFLETS)
    eng.submit_host(xyz, box, np.arange(5))
    with pytest.raises(GorderHipError) as e:
        eng.set_collect(0)                               # after a submit
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
    assert eng.collected_counts() == (3, 0)
    # a capacity too small: refused, the count reported
    import ctypes as C
    n = C.c_uint64(77)
    small = np.zeros((2, 40), dtype=np.uint8)
    st = eng.lib.gorder_hip_collected_leaflets(eng._h, small.ctypes.data_as(C.c_void_p), None, 2, C.byref(n))
    assert st == abi.ERR_INVALID_ARGUMENT and n.value == 3
    st = eng.lib.gorder_hip_collected_leaflets(eng._h, None, None, 0, C.byref(n))      # only the count
    assert st == abi.OK and n.value == 3
    first = eng.collected_leaflets()
    eng.release_staging()                                # keeps what was collected
    np.testing.assert_array_equal(eng.collected_leaflets()[0], first[0])
    # reset empties the rows and keeps the switch
    eng.reset()
    assert eng.collected_counts() == (0, 0)
    eng.submit_host(xyz, box, np.arange(5))
    flags, frames = eng.collected_leaflets()
    np.testing.assert_array_equal(frames, [0, 2, 4])
    np.testing.assert_array_equal(flags, first[0])
    eng.reset()
    eng.set_collect(0)                                   # right after reset: accepted
    eng.submit_host(xyz, box, np.arange(5))
    with pytest.raises(GorderHipError):
        eng.collected_leaflets()


def test_a_handle_without_collection_queues_what_it_queued_before(built):
    """The kernel groups of a plain batch, as the library reported them before collection existed."""
    system = synthetic.cg_membrane(40)
    eng = HipEngine(system.tables)
    eng.kernel_time(reset=True)
    eng.submit_host(system.frames(5, seed=2), system.box9(5), np.arange(5))
    eng.finish()
    eng.kernel_time()
    assert eng.kernel_names() == "k_bonds_tiled + k_batch_end"
    lf = synthetic.cg_membrane(40, leaflets=LEAFLETS_GLOBAL)
    eng = HipEngine(lf.tables)
    eng.kernel_time(reset=True)
    eng.submit_host(lf.frames(5, seed=2), lf.box9(5), np.arange(5))
    eng.finish()
    eng.kernel_time()
    assert eng.kernel_names() == "k_leaflets_global_contig + k_bonds_tiled + k_batch_end"
    eng = HipEngine(lf.tables)
    eng.set_collect(COLLECT_LEAFLETS)
    eng.kernel_time(reset=True)
    eng.submit_host(lf.frames(5, seed=2), lf.box9(5), np.arange(5))
    eng.finish()
    eng.kernel_time()
    assert eng.kernel_names() == "k_leaflets_global_contig + k_bonds_tiled + k_collect_flags + k_batch_end"
