"""What the planner (gorder_amd/csrc/plan.h) makes of the systems of tests/tile_windows.py, without a GPU: a stand-alone
program under the address and undefined-behaviour sanitizers (tests/cabi/tile_windows.cpp) runs build_plan and prints the
tiles, their items, the ownership ranges and the direct items.

For every system tests/test_tile_windows_gpu.py runs — 13 widths x {spaced, abutting} — the tiles are the intended ones, and
the COVERAGE condition holds: for every alignment phase, every slot of a stage and every place the staging code can put a
float (each prefetch register, the first late-load trip, a later one, the window's first and last granule), some float that
a sample reads lies there.  It is computed in plain Python from the printed tiles and items (tile_windows.staging_classes),
for four and for five prefetch registers where the GPU test runs both.  No class may be missing.

Then the planner's edges around the 1024-atom window and the 64 heads a tile may own."""
import os
import subprocess

import numpy as np
import pytest

import tile_windows as tw
from gorder_amd import abi
from gorder_amd.abi import MolType, Tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("spaced", "abutting")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tile_windows") / "tile_windows")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", f"-I{os.path.join(ROOT, 'gorder_amd', 'csrc')}",
                           os.path.join(ROOT, "tests", "cabi", "tile_windows.cpp"), "-o", exe])

    def run(tables):
        res = subprocess.run([exe], input=tw.plan_text(tables).encode(), capture_output=True, timeout=120)
        err = res.stderr.decode()
        assert res.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err
        out = tw.parse_plan(res.stdout.decode())
        assert out["plan"]["status"] == 0 and out["plan"]["selfcheck"] == 0, out["plan"]
        return out
    return run


def small(n_atoms, bonds, **kw):
    """one molecule type, one molecule, a bond type per pair"""
    return Tables(n_atoms=n_atoms, molecule_types=[MolType(n_molecules=1, bonds=np.array(bonds, dtype=np.uint32).reshape(-1, 1, 2))], **kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("width", tw.WIDTHS)
def test_tiles_are_the_intended_ones(built, planner, width, kind):
    system, info = tw.make(width, kind)
    t = system.tables
    out = planner(t)
    plan, tiles = out["plan"], out["tiles"]
    leaflets = kind == "abutting"
    assert t.n_atoms % 4 == 1
    assert plan["max_window"] == width and plan["n_direct"] == 0 and not out["direct"]
    assert plan["spec_ok"] == int(leaflets) and plan["n_tiles"] == tw.N_TILES == len(tiles)
    assert plan["n_acc"] == 2 * tw.SAMPLES and plan["n_mol"] == 2 * tw.N_TILES
    assert sorted(tile["atom0"] % 4 for tile in tiles) == [0, 1, 2, 3]
    for k, tile in enumerate(tiles):
        assert (tile["atom0"], tile["n_window"], tile["n_items"], tile["n_slots"]) == (info.starts[k], width, tw.SAMPLES, tw.SAMPLES), (k, tile)
        # the items are the block's samples (in whatever lane order), each in a slot of its own
        got = sorted(map(tuple, tile["items"][:, :2].tolist()))
        assert got == sorted(map(tuple, info.samples[k].tolist()))
        assert len(set(tile["items"][:, 2].tolist())) == tw.SAMPLES
        atoms = set(tile["items"][:, :2].reshape(-1).tolist())
        assert 0 in atoms and width - 1 in atoms
        for p in range(4):
            last = tw.n_granules(p, width) - 1
            for g in tw.EDGE_GRANULES + (last,):
                if g <= last:
                    assert atoms & set(tw.atoms_in_granule(p, g, width)), (k, p, g)
        if leaflets:
            nxt = tiles[k + 1]["atom0"] if k + 1 < len(tiles) else info.starts[-1] + width
            assert tile["own"] == (tile["atom0"], nxt) and nxt <= tile["atom0"] + width
            assert sorted(tile["heads"][:, 0].tolist()) == sorted(info.heads[k]) and len(tile["heads"]) <= 64
            assert all(tile["own"][0] <= tile["atom0"] + h < tile["own"][1] for h in tile["heads"][:, 0])
    if kind == "spaced":
        assert all(b["atom0"] - (a["atom0"] + width - 1) > tw.MAX_WINDOW for a, b in zip(tiles, tiles[1:]))
    else:
        assert np.array_equal(t.leaflets.membrane, np.arange(tiles[0]["atom0"], tiles[-1]["atom0"] + width))
    # every slot receives two samples a frame, from two tiles — with leaflets one from each sheet
    slots = np.concatenate([tile["items"][:, 2] for tile in tiles])
    assert np.array_equal(np.bincount(slots), np.full(plan["n_acc"], 2))
    mols = np.concatenate([tile["items"][:, 3] for tile in tiles])
    for s in range(0, plan["n_acc"], 37):
        a, b = mols[slots == s]
        assert info.upper[a] != info.upper[b]
    # the library's own view of the same tables
    lib = abi.plan_tables(t)
    assert lib["selfcheck"] == 0 and lib["n_tiles"] == tw.N_TILES and lib["max_window_atoms"] == width and lib["n_direct_items"] == 0
    assert lib["leaflets_one_read"] == int(leaflets)
    lw = tw.lds_pitch(width)
    assert lib["lds_bytes"] == max(4 * lw * 4, 256 * 24) <= 64 * 1024 and lw >= max(tw.n_granules(p, width) for p in range(4)) * 4


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("width", tw.WIDTHS)
def test_every_staging_class_is_read(planner, width, kind):
    system, info = tw.make(width, kind)
    out = planner(system.tables)
    tiles = [(tile["atom0"], tile["n_window"], set(tile["items"][:, :2].reshape(-1).tolist())) for tile in out["tiles"]]
    counts = {tw.STAGE, tw.n_frames_of(width), tw.FIRST_BATCH}
    for npf in sorted({tw.npf_of(width), 5}) if width <= 340 else [tw.npf_of(width)]:
        for n in sorted(counts):
            exist, hit = tw.staging_classes(tiles, system.tables.n_atoms, n, npf)
            assert not exist - hit, (npf, n, sorted(exist - hit, key=str))
            assert hit <= exist
            # the classes are the intended ones: every place the width has in a phase, in all four slots of a stage (the first and
            # the last granule and the first register in all 16 pairs; a register or late trip that begins with the window's last
            # granule in the phases that reach it)
            for where in {c[0] for c in exist}:
                phases = {c[1] for c in exist if c[0] == where}
                assert {c[1:] for c in exist if c[0] == where} == {(p, s) for p in phases for s in range(4)}, where
                if where in ("first", "last", ("register", 0)):
                    assert phases == {0, 1, 2, 3}
    # the regimes the widths were chosen for
    n4 = [tw.n_granules(p, width) for p in range(4)]
    npf = tw.npf_of(width)
    places = {c[0] for c in tw.staging_classes(tiles, system.tables.n_atoms, tw.STAGE, npf)[0]}
    assert (("late", 0) in places) == (max(n4) > npf * tw.LANES) and (("late", 1) in places) == (max(n4) > (npf + 1) * tw.LANES)
    expect = {3: (4, 0), 85: (4, 0), 339: (4, 0), 340: (4, 0), 341: (5, 0), 342: (5, 0), 425: (5, 0), 426: (5, 1), 427: (5, 1), 428: (5, 1),
              860: (5, 2), 1023: (5, 2), 1024: (5, 2)}[width]
    assert (npf, int(("late", 0) in places) + int(("late", 1) in places)) == expect
    # granules per phase at the edges: 256 fill four registers, 320 five; where the phase decides, both sides occur
    edges = {339: (255, 255, 255, 255), 340: (255, 256, 256, 256), 341: (256, 256, 257, 257), 342: (257, 257, 257, 258),
             425: (319, 319, 320, 320), 426: (320, 320, 320, 321), 427: (321, 321, 321, 321), 1024: (768, 769, 769, 769)}
    if width in edges:
        assert tuple(n4) == edges[width]


def test_geometry_and_sentinels(built):
    """CPU side of the inputs: short bonds, some across a face, sheets that stay apart — the oracle's flags are the same in
    every frame — and sentinels exactly on the atoms nothing refers to."""
    from oracle import oracle
    for width, kind in ((3, "abutting"), (340, "abutting"), (427, "abutting"), (341, "spaced"), (1024, "spaced")):
        system, info = tw.make(width, kind)
        n = tw.n_frames_of(width)
        xyz, box = system.frames(n, seed=1), system.box9(n)
        bad = np.isnan(xyz[:, :, 0]) if kind == "spaced" else xyz[:, :, 0] > 1e38
        assert np.array_equal(bad, np.tile(~info.referenced, (n, 1))) and (~info.referenced).sum() >= 1
        if kind == "spaced" and width > 3:
            assert (~info.referenced[:info.starts[0] + width]).sum() > width // 4       # sentinels inside the windows too
        pairs = np.concatenate([info.samples[k] + info.starts[k] for k in range(tw.N_TILES)])
        d = xyz[0, pairs[:, 1]] - xyz[0, pairs[:, 0]]
        crossing = (np.abs(d) > system.box / 2).any(axis=1)
        assert crossing.sum() >= 8
        d -= system.box * np.round(d / system.box)
        length = np.linalg.norm(d, axis=1)
        assert 0.1 < np.median(length) < 0.5 and (length > 1.0).sum() <= (12 if kind == "abutting" and width % 2 == 0 else 0)
        if kind == "abutting":
            o = oracle.OracleEngine(system.tables, trig=oracle.TRIG_DIRECT)
            for f in range(n):
                o.submit(xyz[[f]], box[[f]], [f])
                flags, dist, at = o.leaflets()
                assert at == f and np.array_equal(flags == 0, info.upper) and np.abs(dist).min() > 1.0
            z = xyz[0, info.referenced, 2]
            assert z.min() > 2.0 and z.max() < tw.BOX[2] - 2.0


# ---- the planner's edges ---------------------------------------------------------------------------------------------------
def test_a_window_ends_at_1024_atoms(planner):
    out = planner(small(2000, [(0, 1023)]))
    assert out["plan"]["n_direct"] == 0 and [(t["atom0"], t["n_window"]) for t in out["tiles"]] == [(0, 1024)]
    out = planner(small(2000, [(0, 1024)]))
    assert out["plan"]["n_tiles"] == 0 and out["direct"] == [(0, 1024, 0, 0)]
    out = planner(small(2000, [(5, 1028), (5, 1029), (7, 9)]))              # (one among tiled samples: the tile goes on packing)
    assert out["direct"] == [(5, 1029, 1, 0)] and [(t["atom0"], t["n_window"], t["n_items"]) for t in out["tiles"]] == [(5, 1024, 2)]
    # a tile stops growing at 1024 atoms: the third sample would make it 1025
    out = planner(small(2000, [(0, 1), (1000, 1023), (1001, 1024)]))
    assert [(t["atom0"], t["n_window"], t["n_items"]) for t in out["tiles"]] == [(0, 1024, 2), (1001, 24, 1)] and not out["direct"]
    assert out["plan"]["max_window"] == 1024


def test_sixty_five_heads_or_1025_owned_atoms_turn_the_one_read_plan_off(planner):
    system, info = tw.make(85, "abutting", types_per_block=32)
    before = planner(system.tables)
    assert before["plan"]["spec_ok"] == 1 and [len(t["heads"]) for t in before["tiles"]] == [64] * tw.N_TILES
    # the head of a molecule of block 1 moved into block 0's range: 65 there
    mt = system.tables.molecule_types[32]
    assert info.starts[1] <= mt.heads[0] < info.starts[2]
    mt.heads = np.array([info.starts[0] + 7, mt.heads[1]], dtype=np.uint32)
    after = planner(system.tables)
    assert after["plan"]["spec_ok"] == 0 and after["plan"]["max_window"] == 85 and "own" not in after["tiles"][0]
    for a, b in zip(before["tiles"], after["tiles"]):
        assert all(a[q] == b[q] for q in ("atom0", "n_window", "n_items", "n_slots")) and np.array_equal(a["items"], b["items"])
    assert abi.plan_tables(system.tables)["leaflets_one_read"] == 0
    # the group one atom longer than the last window: the last tile would have to own, and stage, 1025 atoms
    system, info = tw.make(1024, "abutting")
    before = planner(system.tables)
    end = info.starts[-1] + 1024
    assert before["plan"]["spec_ok"] == 1 and end < system.tables.n_atoms
    system.tables.leaflets.membrane = np.arange(0, end + 1, dtype=np.uint32)
    after = planner(system.tables)
    assert after["plan"]["spec_ok"] == 0 and after["plan"]["max_window"] == 1024
    for a, b in zip(before["tiles"], after["tiles"]):
        assert all(a[q] == b[q] for q in ("atom0", "n_window", "n_items", "n_slots")) and np.array_equal(a["items"], b["items"])
    # ... and at a width below the limit the same longer group only widens the last window
    system, info = tw.make(1023, "abutting")
    system.tables.leaflets.membrane = np.arange(0, info.starts[-1] + 1024, dtype=np.uint32)
    wide = planner(system.tables)
    assert wide["plan"]["spec_ok"] == 1 and wide["plan"]["max_window"] == 1024 and [t["n_window"] for t in wide["tiles"]] == [1023] * 3 + [1024]


# ---- what the suite staged before ------------------------------------------------------------------------------------------
def test_what_the_older_suite_staged(built):
    """The window widths of the synthetic membranes the GPU suite runs, as abi.plan_tables prints them (the docstring of
    tests/test_tile_windows_gpu.py quotes them), and their atom counts: multiples of four but for an odd number of all-atom
    lipids, which is 2 modulo 4 — two alignment phases at most, never an odd one."""
    from gorder_amd import synthetic
    from gorder_amd.abi import LEAFLETS_GLOBAL
    seen = {}
    for name, system in (("cg40", synthetic.cg_membrane(40, leaflets=LEAFLETS_GLOBAL, n_types=2)), ("cg70", synthetic.cg_membrane(70, leaflets=LEAFLETS_GLOBAL, n_types=2)),
                         ("cg300", synthetic.cg_membrane(300)), ("cg3072", synthetic.cg_membrane(3072)), ("aa12", synthetic.aa_membrane(12)),
                         ("aa13", synthetic.aa_membrane(13)), ("aa256", synthetic.aa_membrane(256)), ("ua24", synthetic.ua_membrane(24))):
        seen[name] = abi.plan_tables(system.tables)["max_window_atoms"]
        assert system.tables.n_atoms % 4 == (2 if name == "aa13" else 0)
    print(seen)
    assert seen == {"cg40": 280, "cg70": 283, "cg300": 283, "cg3072": 283, "aa12": 391, "aa13": 391, "aa256": 391, "ua24": 0}
    # test_parity_gpu.py::test_wide_windows_fit_the_default_lds_budget
    wide = np.stack([np.arange(60), np.arange(60) + 800], axis=1)
    near = np.stack([np.arange(1500, 1560), np.arange(1501, 1561)], axis=1)
    t = Tables(n_atoms=3000, molecule_types=[MolType(n_molecules=60, bonds=np.stack([wide, near]).astype(np.uint32))])
    assert abi.plan_tables(t)["max_window_atoms"] == 860
