"""The window staging of the tiled order kernels (TiledStage::load / TiledStage::store, gorder_amd/csrc/kernels_bonds.h) at every
width and alignment edge, on the device.  The systems are those of tests/tile_windows.py: four tiles whose windows are
exactly `width` atoms wide, all four alignment phases in every stage, samples that read the first and last atom and both
sides of every granule at which the staging code changes what it does, NaN (one-read routes: 3e38) in every atom nothing
refers to.  tests/test_tile_windows_cpu.py shows without a device that every (place, phase, stage slot) class is read.

Widths: 3, 85 | 339, 340 (four prefetch registers; at 340 the phase decides whether the fourth is full) | 341, 342, 425 (the
fifth register; at 341 in phases 2 and 3 only) | 426 (one late-loaded granule in phase 3 only), 427, 428 (the first late-load
trip) | 860, 1023, 1024 (further trips; 1024 = kMaxWindow, 49 216 bytes of LDS).  Before this file the suite staged windows of
280 and 283 atoms (cg_membrane of 40 and of 70 to 3072 lipids), 391 (aa_membrane of 12 to 256 lipids) and one of 860 atoms
(test_wide_windows_fit_the_default_lds_budget; plain k_bonds_tiled only) — as abi.plan_tables prints them;
test_tile_windows_cpu.py::test_what_the_older_suite_staged asserts it — and n_atoms was a multiple of four wherever the tiled
kernels ran, but for aa_membrane with an odd lipid count: phases 0 and 2 at most, never an odd one.

Every width runs through seven routes; every route is compared with oracle.OracleEngine(trig=TRIG_DIRECT; the literal cosine:
TRIG_MIRROR) by INTEGER EQUALITY.  Nothing in this file takes a tolerance.
    tiled       k_bonds_tiled, no leaflets (spaced layout)                              sums, counts
    tiled-mom   k_bonds_tiled<MOM>: global leaflets every frame, abutting layout, two batches, the second speculative
                                                                                        sums, counts (3 rows), flags of every frame
    tw          k_bonds_tiled_tw, per-frame rows                                        + timewise() rows
    tw-mom      k_bonds_tiled_tw<MOM>, as tiled-mom                                     + timewise() rows
    tw-maps     k_bonds_tiled_tw<MAPS>, rows and staged ordermaps                       + map sums, map counts
    maps        k_bonds_tiled_maps                                                      sums, counts, map sums, map counts
    mol         k_bonds_tiled_mol, per-molecule rows                                    sums, counts, molecule_rows() against the split oracle
A speculative case also asserts that its second batch did speculate, that no frame was left to the exact kernel and that the
fix-up moved nothing (speculation_stats()).

Frames: tile_windows.n_frames_of — one or two whole stages and a partial one of 1, 2 or 3 frames; one case per route with
GORDER_HIP_WG_TARGET and 33 frames (nine stages in two chunks a tile); k_bonds_tiled_mol and k_bonds_tiled_maps once more at 860
atoms with sub-ranges of six frames (GORDER_HIP_MOL_ROWS_STAGING, GORDER_HIP_MAP_FOLD_LIMIT: the second sub-range begins at frame 6).
Cross-sections at 341, 427 and 1024 atoms: no periodic boundaries, a general static normal, a normal along x, the literal
cosine (tiled and mol), GORDER_HIP_KERNEL=gather; and GORDER_HIP_NPF5=1 at 3, 85, 339 and 340 atoms on every route.

A wrong sum names its slot: a slot holds one sample of each of two tiles, and the message lists their atoms and the granules
these lie in for each phase (explain())."""
import dataclasses

import numpy as np
import pytest

import tile_windows as tw
from gorder_amd import HipEngine, abi
from gorder_amd.abi import COLLECT_LEAFLETS, FLAG_TRIG_ACOS_COS
from oracle import oracle
from test_molecule_rows_gpu import split_tables

pytestmark = pytest.mark.gpu

SWITCHES = ("GORDER_HIP_NPF5", "GORDER_HIP_KERNEL", "GORDER_HIP_WG_TARGET", "GORDER_HIP_MOL_ROWS_STAGING", "GORDER_HIP_MAP_FOLD_LIMIT",
            "GORDER_HIP_NO_SPECULATE", "GORDER_HIP_TW_GATHER", "GORDER_HIP_MAPS_GATHER", "GORDER_HIP_MAP_DIRECT", "GORDER_HIP_FORCE_DIRECT",
            "GORDER_HIP_MAP_CHUNKS", "GORDER_HIP_REPLICAS")
ROUTES = {          # kind, timewise, ordermap, speculative, per-molecule rows, the label in kernel_names()
    "tiled": ("spaced", False, False, False, False, "k_bonds_tiled"),
    "tiled-mom": ("abutting", False, False, True, False, "k_bonds_tiled"),
    "tw": ("spaced", True, False, False, False, "k_bonds_tiled_tw"),
    "tw-mom": ("abutting", True, False, True, False, "k_bonds_tiled_tw"),
    "tw-maps": ("spaced", True, True, False, False, "k_bonds_tiled_tw"),
    "maps": ("spaced", False, True, False, False, "k_bonds_tiled_maps"),
    "mol": ("spaced", False, False, False, True, "k_bonds_tiled_mol"),
}
VARIANTS = {        # handle_pbc, normal, flags
    "plain": (True, (0.0, 0.0, 1.0), 0),
    "no pbc": (False, (0.0, 0.0, 1.0), 0),
    "general normal": (True, (0.48, -0.6, 0.64), 0),
    "normal along x": (True, (1.0, 0.0, 0.0), 0),
    "literal cosine": (True, (0.0, 0.0, 1.0), FLAG_TRIG_ACOS_COS),
}
CROSS_WIDTHS = (341, 427, 1024)
MOL_GROUPS = [list(range(s, s + 8)) for s in range(0, 2 * tw.SAMPLES, 8)]          # 64 groups of eight slots (none across two types)
_CACHE = {}


@dataclasses.dataclass
class Case:
    system: object
    info: object
    xyz: np.ndarray
    box: object
    cuts: list
    want: dict


def molecule_rows_oracle(tables, groups, xyz, box, trig):
    """test_molecule_rows_gpu.py's reference: the oracle on split tables (every molecule its own type, per-frame rows) ->
    (sums, counts) int64 [frames, groups, molecules]"""
    split, slot0 = split_tables(tables)
    ref = oracle.OracleEngine(split, trig=trig)
    ref.submit(xyz, box, np.arange(len(xyz)))
    tw_s, tw_c = ref.timewise(len(xyz))
    assert int(tw_c[:, 0].max()) <= 1
    group_of = {s: g for g, slots in enumerate(groups) for s in slots}
    sums = np.zeros((len(xyz), len(groups), tables.n_molecules_total), dtype=np.int64)
    counts = np.zeros_like(sums)
    slot_t, mol = 0, 0
    for t, mt in enumerate(tables.molecule_types):
        for i in range(mt.n_molecules):
            for b in range(mt.n_bond_types):
                g = group_of.get(slot_t + b)
                if g is not None:
                    sums[:, g, mol] += tw_s[:, 0, slot0[t][i] + b]
                    counts[:, g, mol] += tw_c[:, 0, slot0[t][i] + b].astype(np.int64)
            mol += 1
        slot_t += mt.n_bond_types
    return sums, counts


def case_of(route, width, variant="plain", n_frames=None):
    """The system, its frames and the oracle's outputs — made once per (route, width, variant, frames) and left unchanged."""
    n = tw.n_frames_of(width) if n_frames is None else n_frames
    key = (route, width, variant, n)
    if key in _CACHE:
        return _CACHE[key]
    kind, timewise, ordermap, spec, mol, _ = ROUTES[route]
    pbc, normal, flags = VARIANTS[variant]
    system, info = tw.make(width, kind, timewise=timewise, ordermap=ordermap, handle_pbc=pbc, normal=normal, flags=flags)
    total = n + (tw.FIRST_BATCH if spec else 0)
    assert total < 40 and system.tables.n_atoms < 9000
    xyz = system.frames(total, seed=width)
    box = system.box9(total) if pbc else None
    cuts = [(0, tw.FIRST_BATCH), (tw.FIRST_BATCH, total)] if spec else [(0, total)]
    trig = oracle.TRIG_MIRROR if flags & FLAG_TRIG_ACOS_COS else oracle.TRIG_DIRECT
    o = oracle.OracleEngine(system.tables, trig=trig)
    want = {}
    if spec:
        flags_of = []
        for f in range(total):
            o.submit(xyz[[f]], box[[f]], [f])
            fl, dist, at = o.leaflets()
            assert at == f and np.abs(dist).min() > 1.0
            flags_of.append(fl)
        want["flags"] = np.array(flags_of)
        assert np.array_equal(want["flags"] == 0, np.tile(info.upper, (total, 1)))
    else:
        o.submit(xyz, box, np.arange(total))
    res = o.finish()
    assert res.n_frames == total
    want["sums"], want["counts"] = res.sums, res.counts
    assert (res.counts[0] == 2 * total).all()
    if spec:
        assert (res.counts[1] == total).all() and (res.counts[2] == total).all()
    if timewise:
        want["row sums"], want["row counts"] = o.timewise(total)
    if ordermap:
        want["map sums"], want["map counts"] = res.map_sums, res.map_counts
        assert int(res.map_counts[0].sum()) == tw.N_TILES * tw.SAMPLES * total        # every sample lies on the map
    if mol:
        want["molecule sums"], want["molecule counts"] = molecule_rows_oracle(system.tables, MOL_GROUPS, xyz, box, trig)
        assert int(want["molecule counts"].sum()) == tw.N_TILES * tw.SAMPLES * total
    _CACHE[key] = Case(system, info, xyz, box, cuts, want)
    return _CACHE[key]


def explain(info, n_atoms, slots):
    """the samples behind accumulator slots: tile, window-relative atoms and the granules of these for the four phases"""
    half = tw.SAMPLES // 2
    lines = []
    for s in list(slots)[:6]:
        t, b = divmod(int(s), half)
        for tile, q in ((t, b), ((t + 1) % tw.N_TILES, half + b)):
            i, j = (int(a) for a in info.samples[tile][q])
            gran = {p: [((p + 3 * a) >> 2, (p + 3 * a + 2) >> 2) for a in (i, j)] for p in range(4)}
            lines.append(f"slot {s}: tile {tile} (atom0 {info.starts[tile]}, n_atoms {n_atoms}) atoms {i}, {j}; granules by phase {gran}")
    return "\n".join(lines)


def run_and_compare(monkeypatch, route, width, variant="plain", n_frames=None, env=None, label=None, npf=None):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    case = case_of(route, width, variant, n_frames)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, str(value))
    kind, timewise, ordermap, spec, mol, route_label = ROUTES[route]
    t = case.system.tables
    eng = HipEngine(t)
    eng.kernel_time()                       # (switches the event pairs on: the kernels of the batches are then named)
    if spec:
        eng.set_collect(COLLECT_LEAFLETS)
    if mol:
        eng.set_molecule_rows(MOL_GROUPS)
    plan = eng.plan()
    lw = tw.lds_pitch(width)
    assert plan["max_window_atoms"] == width and plan["n_tiles"] == tw.N_TILES and plan["n_direct_items"] == 0
    assert plan["lds_bytes"] == max(4 * lw * 4, 256 * 24) <= 64 * 1024
    assert plan["leaflets_one_read"] == int(kind == "abutting")
    if ordermap:
        assert plan["map_staged"] == 1
    for a, b in case.cuts:
        eng.submit_host(case.xyz[a:b], None if case.box is None else case.box[a:b], np.arange(a, b))
    res = eng.finish()
    total = len(case.xyz)
    got = {"sums": res.sums, "counts": res.counts}
    if spec:
        got["flags"], at = eng.collected_leaflets()
        np.testing.assert_array_equal(at, np.arange(total))
    if timewise:
        got["row sums"], got["row counts"] = eng.timewise(total)
    if ordermap:
        got["map sums"], got["map counts"] = res.map_sums, res.map_counts
    if mol:
        ms, mc, frames = eng.molecule_rows()
        np.testing.assert_array_equal(frames, np.arange(total))
        got["molecule sums"], got["molecule counts"] = ms.astype(np.int64), mc.astype(np.int64)
    names = eng.kernel_names().split(" + ")
    assert (label or route_label) in names, names
    assert ("k_map_accumulate" in names) == ordermap, names
    assert res.n_frames == total
    assert set(got) == set(case.want)
    bad = np.flatnonzero((got["sums"] != case.want["sums"]).any(axis=0) | (got["counts"] != case.want["counts"]).any(axis=0))
    assert bad.size == 0, explain(case.info, t.n_atoms, bad)
    for key, value in case.want.items():
        np.testing.assert_array_equal(got[key], value, err_msg=key)
    stats = eng.speculation_stats()
    if spec:
        assert stats == {"batches": 1, "moved": 0, "exact_frames": 0, "enabled": True}, stats
    else:
        assert stats["batches"] == 0, stats
    return eng


# ---- 1. every width through every route ------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", tw.WIDTHS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_every_width_through_every_route(built, monkeypatch, route, width):
    run_and_compare(monkeypatch, route, width)


def test_partial_stages_of_one_two_and_three_frames_occur():
    tails = [tw.n_frames_of(w) % tw.STAGE for w in tw.WIDTHS]
    assert all(tails.count(k) >= 4 for k in (1, 2, 3)) and all(tw.n_frames_of(w) > tw.STAGE for w in tw.WIDTHS)
    assert tw.FIRST_BATCH % tw.STAGE == 1 and tw.FIRST_BATCH > tw.STAGE


# ---- 2. frames of a tile in two chunks; sub-ranges that begin inside a stage ------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
def test_two_chunks_a_tile(built, monkeypatch, route):
    """GORDER_HIP_WG_TARGET = 8 with four tiles: two workgroups a tile.  The frame counts per workgroup restate order_route.h
    (tiled_chunks: whole stages, at least four a workgroup; extras_chunks: whole stages, staged samples in blocks of 16)."""
    n, per_tile = tw.WG_FRAMES, tw.WG_TARGET // tw.N_TILES
    stages = -(-n // tw.STAGE)
    assert stages >= 8 and per_tile == 2
    if route in ("tiled", "tiled-mom"):
        fpc = -(-stages // min(per_tile, stages // 4)) * tw.STAGE
    else:
        fpc = -(-n // per_tile)
        if ROUTES[route][2]:
            fpc = -(-fpc // 16) * 16
        fpc = -(-fpc // tw.STAGE) * tw.STAGE
    assert -(-n // fpc) == 2 and fpc % tw.STAGE == 0
    run_and_compare(monkeypatch, route, 860, n_frames=n, env={"GORDER_HIP_WG_TARGET": tw.WG_TARGET})


@pytest.mark.parametrize("route", ["mol", "maps"])
def test_sub_ranges_that_begin_inside_a_stage(built, monkeypatch, route):
    """14 frames in sub-ranges of six: frames 6-11 and 12-13 are staged from a frame that is no multiple of four, so a frame's
    slot in its stage is no longer f & 3 and the (slot, phase) pairs are others than in every other case."""
    n = tw.SUB_FRAMES
    assert tw.SUB_RANGE % tw.STAGE != 0 and n > 2 * tw.SUB_RANGE
    if route == "mol":
        env = {"GORDER_HIP_MOL_ROWS_STAGING": tw.SUB_RANGE * len(MOL_GROUPS) * 2 * tw.N_TILES * 8}      # (molecule_rows.h: molecule_rows_subrange)
    else:
        env = {"GORDER_HIP_MAP_FOLD_LIMIT": 2 * tw.SUB_RANGE + 1}      # (order_route.h: map_subrange, two molecules a type)
    eng = run_and_compare(monkeypatch, route, 860, n_frames=n, env=env)
    eng.kernel_time()
    segments = sum(k for name, _, k in eng.kernel_groups() if name == ROUTES[route][5])
    assert segments == -(-n // tw.SUB_RANGE) == 3


# ---- 3. cross-sections ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", CROSS_WIDTHS)
@pytest.mark.parametrize("route", ["tiled", "tw", "maps", "mol"])
@pytest.mark.parametrize("variant", ["no pbc", "general normal", "normal along x"])
def test_other_boundaries_and_normals(built, monkeypatch, variant, route, width):
    run_and_compare(monkeypatch, route, width, variant)
    plain = case_of(route, width)
    assert (case_of(route, width, variant).want["sums"] != plain.want["sums"]).any()       # the variant does change the result


@pytest.mark.parametrize("width", CROSS_WIDTHS)
@pytest.mark.parametrize("route", ["tiled", "mol"])
def test_literal_cosine(built, monkeypatch, route, width):
    run_and_compare(monkeypatch, route, width, "literal cosine")
    assert (case_of(route, width, "literal cosine").want["sums"] != case_of(route, width).want["sums"]).any()


@pytest.mark.parametrize("width", [3, 85, 339, 340])
@pytest.mark.parametrize("route", list(ROUTES))
def test_five_prefetch_registers_where_four_would_do(built, monkeypatch, route, width):
    """GORDER_HIP_NPF5=1 on windows of up to 256 granules: at 340 atoms the fifth register holds a clamped duplicate in
    every phase and the fourth is full in phases 1 to 3 only."""
    assert tw.npf_of(width) == 4
    run_and_compare(monkeypatch, route, width, env={"GORDER_HIP_NPF5": 1})


@pytest.mark.parametrize("width", CROSS_WIDTHS)
def test_the_gather_kernel_gives_the_same_integers(built, monkeypatch, width):
    run_and_compare(monkeypatch, "tiled", width, env={"GORDER_HIP_KERNEL": "gather"}, label="k_bonds_gather")


# ---- 4. the alignment refusal -----------------------------------------------------------------------------------------------
def test_frames_that_are_not_16_byte_aligned_are_refused(built, monkeypatch):
    """gorder_hip_submit_device refuses coordinates that do not begin at a multiple of 16 bytes (the staging code's 16-byte
    loads rely on it, kernels_bonds.h), names the reason, and the handle goes on to take the aligned frames."""
    import torch
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    case = case_of("tiled", 341)
    t = case.system.tables
    n = len(case.xyz)
    flat = torch.from_numpy(case.xyz).reshape(-1)
    pool = torch.empty(flat.numel() + 4, dtype=torch.float32, device="cuda")
    d_box = torch.from_numpy(case.box).cuda()
    assert pool.data_ptr() % 16 == 0
    eng = HipEngine(t)
    for shift in (1, 2, 3):
        view = pool[shift:shift + flat.numel()]
        view.copy_(flat)
        view = view.view(n, t.n_atoms, 3)
        assert view.data_ptr() % 16 == 4 * shift and view.is_contiguous()
        with pytest.raises(abi.GorderHipError) as e:
            eng.submit_device(view, d_box)
        assert e.value.status == abi.ERR_INVALID_ARGUMENT and "d_xyz must be 16-byte aligned" in str(e.value)
    view = pool[:flat.numel()]
    view.copy_(flat)
    torch.cuda.synchronize()
    eng.submit_device(view.view(n, t.n_atoms, 3), d_box)
    res = eng.finish()
    assert res.n_frames == n                                              # the refused calls counted no frame
    np.testing.assert_array_equal(res.sums, case.want["sums"])
    np.testing.assert_array_equal(res.counts, case.want["counts"])
