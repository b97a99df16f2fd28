"""Whole-trajectory manual tables (gorder_hip_set_manual_leaflet_table / gorder_hip_set_manual_normal_table): what an
earlier run collected, or the reference's own files, replayed from packed tables on the device however the frames are
cut into batches — against the run that produced the rows, the oracle fed row by row, the one-row / one-batch route the
tables replace, the trajectory driver with shards, and the errors and life cycle of the tables."""
import dataclasses
import os

import numpy as np
import pytest

from gorder_amd import GorderHipError, HipEngine, abi, manual, synthetic
from gorder_amd.abi import COLLECT_LEAFLETS, LEAFLETS_GLOBAL, LEAFLETS_MANUAL, Leaflets, MolType, Tables
from oracle import oracle
from golden_util import GOLDEN, METHODS, Fixture, aa_setup, cg_setup, ua_setup
import replay_names

pytestmark = pytest.mark.gpu

N = 12
SPLITS = {"one batch": ((0, N),), "three batches": ((0, 5), (5, 6), (6, N))}
EDGE_CUTS = ((0, 4), (4, 9), (9, N))            # frequency 3: cut inside an interval (4) and on an assignment frame (9)


def same(got, want):
    np.testing.assert_array_equal(got.counts, want.counts)
    np.testing.assert_array_equal(got.sums, want.sums)
    assert got.n_frames == want.n_frames


def golden_text(name):
    with open(os.path.join(GOLDEN, "expected", name)) as f:
        return f.read()


# ---- 1. round trip: classify, collect, replay ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def classified(built):
    """Global leaflets of aa_membrane(70) run once per frequency with collection: (results, rows, frames)."""
    out = {}
    for frequency in (1, 5):
        system = synthetic.aa_membrane(70, leaflets=LEAFLETS_GLOBAL, frequency=frequency)
        eng = HipEngine(system.tables)
        eng.set_collect(COLLECT_LEAFLETS)
        eng.submit_host(system.frames(N, seed=5), system.box9(N), np.arange(N))
        rows, frames = eng.collected_leaflets()
        out[frequency] = (eng.finish(), rows, frames)
    return out


@pytest.mark.parametrize("frequency,split", [(1, "one batch"), (1, "three batches"), (5, "one batch"), (5, "three batches")])
def test_round_trip(classified, frequency, split):
    want, rows, frames = classified[frequency]
    np.testing.assert_array_equal(frames, np.arange(0, N, frequency))
    assert 0 < rows.sum() < rows.size and want.counts[1].sum() > 0 and want.counts[2].sum() > 0
    system = synthetic.aa_membrane(70, leaflets=LEAFLETS_MANUAL, frequency=frequency)
    xyz, box = system.frames(N, seed=5), system.box9(N)
    eng = HipEngine(system.tables)
    eng.set_manual_leaflet_table(rows)
    for a, b in SPLITS[split]:
        eng.submit_host(xyz[a:b], box[a:b], np.arange(a, b))
    same(eng.finish(), want)
    flags, frame = eng.leaflets()
    np.testing.assert_array_equal(flags, rows[-1])
    assert frame == frames[-1]


# ---- 2. / 3. word edges: against the oracle fed row by row, and against the one-row route ----------------------------------
def edge_case(n_mol, flip):
    ids = np.arange(n_mol, dtype=np.uint32)
    bonds = np.stack([2 * ids, 2 * ids + 1], axis=1)[None]
    tables = Tables(n_atoms=2 * n_mol, molecule_types=[MolType(n_molecules=n_mol, bonds=bonds, name="M")],
                    leaflets=Leaflets(method=LEAFLETS_MANUAL, frequency=3, flip=flip))
    rng = np.random.default_rng(1000 + n_mol)
    xyz = rng.uniform(0.5, 3.5, size=(N, 2 * n_mol, 3)).astype(np.float32)
    box = np.tile(np.diag([4.0, 4.0, 4.0]).astype(np.float32), (N, 1, 1))
    given = rng.integers(0, 2, size=(4, n_mol)).astype(np.uint8)
    given[1, -1], given[2, -1] = 1, 0                  # the last molecule's bit both ways
    return tables, xyz, box, given


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("n_mol", [1, 63, 64, 65, 129])
def test_word_edges(built, n_mol, flip):
    """`flip` is applied when a row is expanded, as gorder_hip_set_manual_leaflets applies it: what leaflets() and the
    collected rows show is the given row after `flip`, exactly what the one-row route and the oracle show."""
    tables, xyz, box, given = edge_case(n_mol, flip)
    o = oracle.OracleEngine(tables, trig=oracle.TRIG_DIRECT)
    old = HipEngine(tables)                            # the route the table replaces: one submit per row
    old.set_collect(COLLECT_LEAFLETS)
    for r in range(4):
        fr = np.arange(3 * r, 3 * r + 3)
        o.set_manual_leaflets(given[r], 3 * r)
        o.submit(xyz[fr], box[fr], fr)
        old.set_manual_leaflets(given[r], 3 * r)
        old.submit_host(xyz[fr], box[fr], fr)
    want = o.finish()
    assert want.counts[0].sum() == N * n_mol
    eng = HipEngine(tables)
    eng.set_collect(COLLECT_LEAFLETS)
    eng.set_manual_leaflet_table(given)
    for a, b in EDGE_CUTS:
        eng.submit_host(xyz[a:b], box[a:b], np.arange(a, b))
    same(eng.finish(), want)
    same(eng.finish(), old.finish())
    flags, frame = eng.leaflets()
    np.testing.assert_array_equal(flags, given[-1] ^ int(flip))
    np.testing.assert_array_equal(flags, o.leaflets()[0])
    np.testing.assert_array_equal(flags, old.leaflets()[0])
    assert frame == 9
    rows, frames = eng.collected_leaflets()
    np.testing.assert_array_equal(frames, [0, 3, 6, 9])
    np.testing.assert_array_equal(rows, given ^ int(flip))
    old_rows, old_frames = old.collected_leaflets()
    np.testing.assert_array_equal(rows, old_rows)
    np.testing.assert_array_equal(frames, old_frames)


# ---- 4. the normals table --------------------------------------------------------------------------------------------------
def normals_case(kind):
    system = synthetic.cg_membrane(90, leaflets=LEAFLETS_GLOBAL, n_types=2) if kind == "cg" else \
        synthetic.ua_membrane(30, leaflets=LEAFLETS_GLOBAL)
    n_mol = system.tables.n_molecules_total
    z = np.zeros((N, n_mol, 3), dtype=np.float32)
    z[:, :, 2] = 1.0
    tilted = np.random.default_rng(2).normal(size=(N, n_mol, 3)).astype(np.float32) * 0.4 + z     # not unit length
    return system, system.frames(N, seed=41), system.box9(N), tilted


@pytest.fixture(scope="module")
def normals_reference(built):
    """Per (kind, step): the oracle and the engine's own set_normals route, both fed the same normals in two batches."""
    out = {}
    for kind in ("cg", "ua"):
        system, xyz, box, tilted = normals_case(kind)
        for step in (1, 2):
            o = oracle.OracleEngine(system.tables, trig=oracle.TRIG_DIRECT, n_threads=2)
            eng = HipEngine(system.tables)
            for a, b in ((0, 4), (4, N)):
                fi = np.arange(a, b) * step
                o.set_normals(tilted[a:b])
                o.submit(xyz[a:b], box[a:b], fi)
                eng.set_normals(tilted[a:b])
                eng.submit_host(xyz[a:b], box[a:b], fi)
            out[kind, step] = (o.finish(), eng.finish())
    return out


@pytest.mark.parametrize("split", sorted(SPLITS))
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("kind", ["cg", "ua"])
def test_normals_table(normals_reference, kind, step, split):
    system, xyz, box, tilted = normals_case(kind)
    want_oracle, want_route = normals_reference[kind, step]
    assert want_route.counts[0].sum() > 0
    eng = HipEngine(system.tables)
    eng.set_manual_normal_table(tilted, step=step)
    for a, b in SPLITS[split]:
        eng.submit_host(xyz[a:b], box[a:b], np.arange(a, b) * step)
    got = eng.finish()
    print(f"{kind} step {step} {split}: max |sum - oracle| = {np.abs(got.sums - want_oracle.sums).max()}, "
          f"max |sum - set_normals route| = {np.abs(got.sums - want_route.sums).max()}")
    same(got, want_route)
    same(got, want_oracle)
    # the table changes the result (the static normal is z)
    plain = HipEngine(system.tables)
    plain.submit_host(xyz, box, np.arange(N) * step)
    assert (plain.finish().sums != got.sums).any()


# ---- 5. the reference's own files ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixtures(built):
    return {k: Fixture(k) for k in ("pcpepg", "ua", "cg")}


@pytest.mark.parametrize("name,frequency", [("aa_leaflets_every5.yaml", 5), ("aa_leaflets_once.yaml", 0)])
def test_reference_leaflet_files(fixtures, name, frequency):
    fx = fixtures["pcpepg"]
    tables, labels, midx = aa_setup(fx, leaflets=METHODS["global"], frequency=frequency)
    xyz = np.ascontiguousarray(fx.xyz[:51][:, midx, :])
    classifier = HipEngine(tables)
    classifier.submit_host(xyz, fx.boxes[:51], np.arange(51))
    want = classifier.finish()
    rows = manual.read_leaflets_file(golden_text(name), labels)
    assert rows.shape == ((11 if frequency else 1), tables.n_molecules_total)
    replay = dataclasses.replace(tables, leaflets=Leaflets(method=LEAFLETS_MANUAL, frequency=frequency))
    eng = HipEngine(replay)
    eng.set_manual_leaflet_table(rows)
    for a, b in ((0, 17), (17, 40), (40, 51)):
        eng.submit_host(xyz[a:b], fx.boxes[a:b], np.arange(a, b))
    same(eng.finish(), want)
    assert want.counts[1].sum() > 0 and want.counts[2].sum() > 0


def test_reference_normals_file(fixtures):
    fx = fixtures["ua"]
    tables, labels, midx = ua_setup(fx)
    normals = manual.read_normals_file(golden_text("ua_normals.yaml"), labels)
    assert normals.shape == (51, tables.n_molecules_total, 3)
    xyz = np.ascontiguousarray(fx.xyz[:51][:, midx, :])
    o = oracle.OracleEngine(tables, trig=oracle.TRIG_DIRECT, n_threads=2)
    o.set_normals(normals)
    o.submit(xyz, fx.boxes[:51], np.arange(51))
    want = o.finish()
    eng = HipEngine(tables)
    eng.set_manual_normal_table(normals)
    for a, b in ((0, 17), (17, 40), (40, 51)):
        eng.submit_host(xyz[a:b], fx.boxes[a:b], np.arange(a, b))
    got = eng.finish()
    print(f"ua_normals.yaml: max |sum - oracle| = {np.abs(got.sums - want.sums).max()}")
    same(got, want)
    assert want.counts[0].sum() > 0


# ---- 6. the trajectory driver, whole and in shards -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver_case(fixtures, tmp_path_factory):
    """Eleven frames of the cg fixture as an XTC file, manual leaflets every second frame and manual normals for every
    frame; the single-submit result on the decoded coordinates."""
    from gorder_amd import xtc
    cg = fixtures["cg"]
    tables, labels, midx = cg_setup(cg, leaflets=METHODS["global"], frequency=2)
    tables = dataclasses.replace(tables, leaflets=Leaflets(method=LEAFLETS_MANUAL, frequency=2))
    path = str(tmp_path_factory.mktemp("replay") / "eleven.xtc")
    fr = np.arange(11)
    xtc.write_trajectory(path, cg.xyz[fr], cg.boxes[fr], times=cg.times[fr], precision=100.0)
    xyz, box, _ = xtc.read_trajectory([path], group=midx)
    n_mol = tables.n_molecules_total
    rng = np.random.default_rng(6)
    flags = rng.integers(0, 2, size=(6, n_mol)).astype(np.uint8)
    normals = (rng.normal(size=(11, n_mol, 3)) * 0.4 + np.array([0.0, 0.0, 1.0])).astype(np.float32)
    eng = HipEngine(tables)
    eng.set_manual_leaflet_table(flags)
    eng.set_manual_normal_table(normals)
    eng.submit_host(xyz, box, fr)
    want = eng.finish()
    assert want.n_frames == 11 and want.counts[1].sum() > 0 and want.counts[2].sum() > 0
    return tables, midx, path, flags, normals, want


@pytest.mark.parametrize("device_decode", [False, True])
def test_driver_and_shards(driver_case, device_decode):
    tables, midx, path, flags, normals, want = driver_case

    def run(shard, window=False):
        eng = HipEngine(tables)
        if window:      # a rank uploads only the rows of its share: shard 1 of 2 analyses frames 5..10
            eng.set_manual_leaflet_table(flags[2:], first_row=2)
            eng.set_manual_normal_table(normals[5:], first_row=5)
        else:
            eng.set_manual_leaflet_table(flags)
            eng.set_manual_normal_table(normals)
        stats = eng.run_trajectory([path], group=midx, step=1, threads=2, batch_frames=3, device_decode=device_decode, shard=shard)
        assert stats["device_decode"] == int(device_decode)
        return eng.finish()

    same(run(None), want)
    parts = [run((i, 2)) for i in range(2)]
    assert parts[0].n_frames + parts[1].n_frames == 11 and parts[1].n_frames == 6
    np.testing.assert_array_equal(parts[0].sums + parts[1].sums, want.sums)
    np.testing.assert_array_equal(parts[0].counts + parts[1].counts, want.counts)
    same(run((1, 2), window=True), parts[1])


# ---- 7. errors and life cycle ----------------------------------------------------------------------------------------------
def status_of(call, *args, **kw):
    with pytest.raises(GorderHipError) as e:
        call(*args, **kw)
    return e.value


def test_leaflet_table_errors_and_lifecycle(built):
    tables, xyz, box, given = edge_case(65, False)
    eng = HipEngine(tables)
    eng.set_manual_leaflet_table(given[:3])                         # one row short: frames 9..11 have none
    eng.submit_host(xyz[:4], box[:4], np.arange(4))
    before = eng.finish()
    err = status_of(eng.submit_host, xyz[4:], box[4:], np.arange(4, N))
    assert err.status == abi.ERR_MANUAL_LEAFLET_FRAME == 8 and err.frame == 9
    same(eng.finish(), before)                                      # the batch was refused whole
    assert before.n_frames == 4
    eng.submit_host(xyz[4:9], box[4:9], np.arange(4, 9))            # the frames that have rows still go through
    assert eng.finish().n_frames == 9
    # the one-row call is refused while a table is set
    assert status_of(eng.set_manual_leaflets, given[3], 9).status == abi.ERR_INVALID_ARGUMENT
    # reset keeps the table and forgets the carried row: a batch inside an interval expands its row again
    eng.reset()
    eng.submit_host(xyz[4:9], box[4:9], np.arange(4, 9))
    part = eng.finish()
    ref = HipEngine(tables)
    ref.set_manual_leaflet_table(given)
    ref.submit_host(xyz[4:9], box[4:9], np.arange(4, 9))
    same(part, ref.finish())
    # a window: rows 2 and 3 only
    eng.set_manual_leaflet_table(given[2:], first_row=2)
    eng.reset()
    err = status_of(eng.submit_host, xyz[5:8], box[5:8], np.arange(5, 8))
    assert err.status == abi.ERR_MANUAL_LEAFLET_FRAME and err.frame == 5
    eng.submit_host(xyz[6:], box[6:], np.arange(6, N))
    assert eng.finish().n_frames == 6
    # n_rows = 0 removes the table: today's behaviour
    eng.set_manual_leaflet_table(None)
    eng.reset()
    assert status_of(eng.submit_host, xyz[:3], box[:3], np.arange(3)).status == abi.ERR_LEAFLETS_NOT_PRIMED
    eng.set_manual_leaflets(given[0], 0)
    eng.submit_host(xyz[:3], box[:3], np.arange(3))
    one = HipEngine(tables)
    one.set_manual_leaflets(given[0], 0)
    one.submit_host(xyz[:3], box[:3], np.arange(3))
    same(eng.finish(), one.finish())
    # the table needs GORDER_LEAFLETS_MANUAL
    other = HipEngine(synthetic.cg_membrane(40, leaflets=LEAFLETS_GLOBAL).tables)
    assert status_of(other.set_manual_leaflet_table, np.zeros((2, 40), dtype=np.uint8)).status == abi.ERR_INVALID_ARGUMENT


def test_normal_table_errors_and_lifecycle(built):
    system, xyz, box, tilted = normals_case("cg")
    eng = HipEngine(system.tables)
    eng.set_manual_normal_table(tilted[:N - 1], step=2)             # one row short: frame 22 has none
    eng.submit_host(xyz[:4], box[:4], np.arange(4) * 2)
    before = eng.finish()
    err = status_of(eng.submit_host, xyz[4:], box[4:], np.arange(4, N) * 2)
    assert err.status == abi.ERR_MANUAL_NORMAL_FRAME == 9 and err.frame == 22
    same(eng.finish(), before)
    assert before.n_frames == 4
    # a frame off the step
    err = status_of(eng.submit_host, xyz[4:7], box[4:7], [8, 10, 13])
    assert err.status == abi.ERR_INVALID_ARGUMENT and err.frame == 13
    same(eng.finish(), before)
    # the one-batch call is refused while a table is set
    assert status_of(eng.set_normals, tilted[:2]).status == abi.ERR_INVALID_ARGUMENT
    assert status_of(eng.set_manual_normal_table, tilted, step=0).status == abi.ERR_INVALID_ARGUMENT
    # reset keeps the table
    eng.reset()
    eng.submit_host(xyz[:6], box[:6], np.arange(6) * 2)
    ref = HipEngine(system.tables)
    ref.set_normals(tilted[:6])
    ref.submit_host(xyz[:6], box[:6], np.arange(6) * 2)
    same(eng.finish(), ref.finish())
    # n_rows = 0 removes it: the static normal again, and the one-batch call works
    eng.set_manual_normal_table(None)
    eng.reset()
    eng.submit_host(xyz, box, np.arange(N))
    plain = HipEngine(system.tables)
    plain.submit_host(xyz, box, np.arange(N))
    same(eng.finish(), plain.finish())
    eng.set_normals(tilted[:2])
    eng.submit_host(xyz[:2], box[:2], np.arange(2))


# what gorder_hip_kernel_time_names reports for these handles on the commit before the tables existed: read off that
# commit's launch code ("cg40 plain" and the k_leaflets_global_contig prefix are the strings tests/test_collect_gpu.py
# recorded on a device); `python tests/replay_names.py` with that commit's library (GORDER_HIP_LIB) prints them
NAMES_BEFORE = {
    "aa70 manual leaflets, one row": "k_bonds_tiled + k_batch_end",
    "cg90 global leaflets, set_normals": "k_leaflets_global_contig + k_bonds_extras + k_batch_end",
    "ua30 global leaflets, set_normals": "k_leaflets_global_contig + k_ua_extras + k_batch_end",
    "cg40 plain": "k_bonds_tiled + k_batch_end",
    "cg64 dynamic normals": "k_local_build + k_dyn_cov + k_dyn_eigen + k_bonds_extras + k_batch_end",
}


@pytest.mark.parametrize("case", sorted(replay_names.CASES))
def test_a_handle_without_tables_queues_what_it_queued_before(built, case):
    assert replay_names.names_of(case) == NAMES_BEFORE[case]


def test_the_replay_kernels_are_timed_groups(built):
    tables, xyz, box, given = edge_case(129, True)
    eng = HipEngine(tables)
    eng.set_manual_leaflet_table(given)
    eng.kernel_time(reset=True)
    eng.submit_host(xyz, box, np.arange(N))
    eng.finish()
    total, launches = eng.kernel_time()
    groups = eng.kernel_groups()
    assert [g[0] for g in groups] == ["k_replay_flags", "k_bonds_tiled", "k_batch_end"] and launches == 1
    assert abs(sum(g[1] for g in groups) - total) <= 1e-6 * max(1.0, total)
    system, xyz, box, tilted = normals_case("cg")
    eng = HipEngine(system.tables)
    eng.set_manual_normal_table(tilted)
    eng.kernel_time(reset=True)
    eng.submit_host(xyz, box, np.arange(N))
    eng.finish()
    total, _ = eng.kernel_time()
    groups = eng.kernel_groups()
    assert [g[0] for g in groups] == ["k_leaflets_global_contig", "k_replay_normals", "k_bonds_extras", "k_batch_end"]
    assert abs(sum(g[1] for g in groups) - total) <= 1e-6 * max(1.0, total)
