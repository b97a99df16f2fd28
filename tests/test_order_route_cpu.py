"""The route of the order pass (gorder_amd/csrc/order_route.h) without a GPU: a stand-alone program under the address and
undefined-behaviour sanitizers prints the route of EVERY input and the result of the chunking functions at their edges;
the expected values here restate the predicates as they stood in gorder_hip.hip before the route existed (commit 6bcc07e:
launch_orders, lines 513-794, and gorder_hip_submit_device, lines 2022-2029 and 2150-2158 — the numbers in the comments),
not the header.

Every boolean that occurs in a predicate is swept, 2^24 inputs, no sampling.  pbc and axis are read by no predicate (they
only pick a template argument at the launch) and are no part of the route, so they are not swept."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# bit k of an input's number (tests/cabi/order_route.cpp: input())
BITS = ["maps", "map_staged", "tw", "geom", "dyn_or_manual", "acos", "use_gather", "item_run", "stage8", "wide", "npf5",
        "tw_gather", "maps_gather", "bond_tiles", "ua_tiles", "direct_items", "ua_fast_flag", "leaflets", "global_leaflets",
        "spec_enabled", "have_assignment", "every_frame_assigns", "manual_frames", "normal_table"]
N_INPUTS = 1 << len(BITS)
RANGES = 8
NONE, TILED, GATHER, TILED_TW, TILED_MAPS, EXTRAS = range(6)
# the route's word (tests/cabi/order_route.cpp: word()): (name, first bit, bits)
FIELDS = [("family", 0, 3), ("npf5", 3, 1), ("mom", 4, 1), ("tw_maps", 5, 1), ("maps_only", 6, 1), ("items_by_slot", 7, 1),
          ("ua_mode1", 8, 3), ("ua_fast", 11, 1), ("map_accumulate", 12, 1), ("direct", 13, 1), ("fixup_ac", 14, 1),
          ("fixup_tw", 15, 1), ("speculative", 16, 1), ("extras", 17, 1), ("label", 18, 3)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("order_route") / "order_route")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", f"-I{os.path.join(ROOT, 'gorder_amd', 'csrc')}",
                           os.path.join(ROOT, "tests", "cabi", "order_route.cpp"), "-o", exe])

    def run(*args):
        res = subprocess.run([exe, *map(str, args)], capture_output=True, timeout=300)
        err = res.stderr.decode()
        assert res.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err
        return res.stdout
    return run


def parent_routes(i):
    """The fields of the route for the inputs i (an array of input numbers), from the predicates of the parent commit."""
    f = {name: ((i >> k) & 1).astype(bool) for k, name in enumerate(BITS)}
    maps, tw, geom, ac, gather = f["maps"], f["tw"], f["geom"], f["acos"], f["use_gather"]
    dyn = f["dyn_or_manual"]                                  # e.dyn != nullptr (632): h->dyn || h->manual_active
    stage4 = ~f["stage8"]                                     # h->frames_per_stage == kRecFrames
    window = np.where(f["wide"], 341, 340)
    extras = maps | tw | geom | dyn                           # 516
    plain = f["bond_tiles"] & ~extras                         # 538
    pass0 = f["bond_tiles"] & extras                          # 655-656: nt = extras ? n_tiles : 0
    staged = maps & f["map_staged"]                           # 636
    npf4 = ((3 * window + 6) // 4 <= 4 * 64) & ~f["npf5"]     # 609 and again 720
    tiled_tw = pass0 & tw & (~maps | staged) & ~geom & ~dyn & ~ac & ~gather & f["item_run"] & stage4 & ~f["tw_gather"]   # 664-665
    maps_only = staged & ~tw & ~geom & ~dyn                   # 682; 740 adds `extras &&`, which staged implies
    tiled_maps = pass0 & maps_only & ~ac & ~gather & stage4 & ~f["maps_gather"]      # 685-686
    family = np.select([plain & gather, plain, tiled_maps, tiled_tw, pass0], [GATHER, TILED, TILED_MAPS, TILED_TW, EXTRAS], NONE)   # 604-606, 718-724
    # the batch speculates (2025-2029; inside `if (leaflets)`, 1997).  `!h->dyn && !h->manual_frames && !h->d_ntable`:
    # h->dyn implies dyn_or_manual, and so do the other two wherever the caller's facts are consistent
    tw_tiled = tw & ~ac & f["item_run"] & stage4 & ~f["tw_gather"]
    spec = (f["leaflets"] & f["spec_enabled"] & f["global_leaflets"] & f["have_assignment"] & f["every_frame_assigns"] & ~maps &
            (~tw | tw_tiled) & ~geom & ~dyn & ~f["manual_frames"] & ~f["normal_table"] & ~gather & f["bond_tiles"])
    # ... and the kernel that runs is the MOM variant: `LF_ && h->spec_now` (558), `tiled_tw && !staged && LF_ && h->spec_now` (689)
    mom = f["leaflets"] & spec & ((family == TILED) | ((family == TILED_TW) & ~staged))
    ua_mode = np.select([~f["ua_tiles"], maps_only, extras & tw & ~maps & ~geom & ~dyn, extras], [-1, 1, 3, 2], 0)   # 655, 742-745
    return {
        "family": family, "label": family,                    # 604, 718: the label names the family
        "npf5": ~npf4, "mom": mom, "speculative": spec,
        "tw_maps": tiled_tw & staged,                         # 692: the only arm with MAPS = true
        "maps_only": maps_only,
        "items_by_slot": pass0 & (staged | tiled_tw),         # 678; the plain kernels read d_items (560)
        "ua_mode1": ua_mode + 1,
        "ua_fast": ~ac & f["ua_fast_flag"] & f["ua_tiles"],   # 624, 732
        "map_accumulate": staged,                             # 749
        "direct": f["direct_items"],                          # 773
        "fixup_tw": tw, "fixup_ac": ~tw & ac,                 # 2150-2158
        "extras": extras,
    }, f, staged


def decode(out, n):
    """n lines of six hex digits -> the fields."""
    text = np.frombuffer(out, dtype=np.uint8)
    assert text.size == 7 * n
    text = text.reshape(n, 7)
    assert (text[:, 6] == ord("\n")).all()
    digits = text[:, :6].astype(np.int64)
    digits = np.where(digits >= ord("a"), digits - ord("a") + 10, digits - ord("0"))
    assert ((digits >= 0) & (digits < 16)).all()
    word = (digits << (4 * np.arange(5, -1, -1))).sum(axis=1)
    return {name: (word >> at) & ((1 << bits) - 1) for name, at, bits in FIELDS}


@pytest.mark.parametrize("part", range(RANGES))
def test_every_input_takes_the_parents_route(driver, part):
    lo, hi = part * N_INPUTS // RANGES, (part + 1) * N_INPUTS // RANGES
    got = decode(driver("routes", lo, hi), hi - lo)
    want, f, staged = parent_routes(np.arange(lo, hi, dtype=np.int64))
    assert set(got) == set(want)
    for name in got:
        bad = np.flatnonzero(got[name] != want[name].astype(np.int64))
        assert bad.size == 0, (name, hex(lo + int(bad[0])), int(got[name][bad[0]]), int(want[name][bad[0]]), bad.size)
    # what the parent held only because two predicates agreed
    spec, mom, family = got["speculative"] == 1, got["mom"] == 1, got["family"]
    assert (~spec | (mom & ((family == TILED) | ((family == TILED_TW) & (got["tw_maps"] == 0))))).all()
    assert (spec == mom).all()                                 # no MOM kernel without the check kernels behind it either
    assert (~mom | f["leaflets"]).all()
    assert (~(family == TILED_MAPS) | (staged & (got["maps_only"] == 1))).all()
    assert (~(got["ua_fast"] == 1) | ~f["acos"]).all()
    assert ((got["label"] == family) & (family <= EXTRAS)).all()


def test_the_sweep_reaches_every_family_and_mode(driver):
    """The product is not vacuous: every family, both speculative kernels, every united-atom mode occur."""
    want, _, _ = parent_routes(np.arange(N_INPUTS, dtype=np.int64))
    assert sorted(np.unique(want["family"])) == list(range(6)) and sorted(np.unique(want["ua_mode1"])) == list(range(5))
    assert sorted(np.unique(want["family"][want["speculative"]])) == [TILED, TILED_TW]
    # the window: (3 w + 6) / 4 float4 in 4 x 64 registers — 339 and 340 atoms fit, 341 do not
    assert [(3 * w + 6) // 4 <= 256 for w in (339, 340, 341)] == [True, True, False]


def ceil_div(a, b):
    return (a + b - 1) // b


def parent_chunks(name, a):
    """(frames per chunk, chunks) — or the sub-range length — as launch_orders computed them."""
    if name == "tiled":                                       # 543-550
        nf, G, nt, target, cap = a
        n_stages = ceil_div(nf, G)
        target = target if target else 12 * cap
        n_chunks = min(max(1, target // nt), max(1, n_stages // 4))
        fpc = ceil_div(n_stages, n_chunks) * G
        return [fpc, ceil_div(nf, fpc)]
    if name == "extras":                                      # 657-667
        nf, nt, target, cap, staged, whole = a
        n_chunks = min(max(1, (target if target else 8 * cap) // nt), nf)
        fpc = ceil_div(nf, n_chunks)
        if staged:
            fpc = ceil_div(fpc, 16) * 16
        if whole:
            fpc = ceil_div(fpc, 4) * 4
        return [fpc, ceil_div(nf, fpc)]
    if name == "direct":                                      # 775-780
        nf, bpc, target = a
        n_chunks = min(max(1, ceil_div(target if target else 256 * 8, bpc)), nf)
        fpc = ceil_div(nf, n_chunks)
        return [fpc, ceil_div(nf, fpc)]
    if name == "map":                                         # 756-760
        nf, n_acc, forced = a
        mchunks = forced if forced else max(1, 512 // max(1, n_acc))
        mchunks = min(mchunks, max(1, nf // 16))
        mfpc = ceil_div(ceil_div(nf, mchunks), 16) * 16
        return [mfpc, ceil_div(nf, mfpc)]
    assert name == "sub"                                      # 635-640
    nf, maps, staged, limit, max_mol, words = a
    sub = (max(1, (limit - 1) // max_mol) & 0xffffffff) if maps else nf
    if staged:
        sub = min(sub, max(1, (1 << 27) // words), nf)
    return [sub]


def test_chunking_at_its_edges(driver):
    seen = {}
    for line in driver("chunks").decode().splitlines():
        name, *rest = line.split()
        at = rest.index("->")
        a, got = list(map(int, rest[:at])), list(map(int, rest[at + 1:]))
        assert got == parent_chunks(name, a), line
        seen.setdefault(name, []).append(a)
    assert set(seen) == {"tiled", "extras", "direct", "map", "sub"}
    # the edges: 1, G - 1, G, G + 1 frames; 4 G - 1 and 4 G stages (the first count that allows a second chunk is 8 stages,
    # 4 per workgroup); more tiles than the target; GORDER_HIP_WG_TARGET set; staged rounding to 16; fewer than 16 frames
    # for k_map_accumulate
    for G in (4, 8):
        frames = {a[0] for a in seen["tiled"] if a[1] == G}
        assert {1, G - 1, G, G + 1, 4 * G - 1, 4 * G, (4 * G - 1) * G, 4 * G * G} <= frames
    assert any(a[2] > 12 * a[4] and a[3] == 0 for a in seen["tiled"]) and any(a[3] for a in seen["tiled"])
    assert any(a[1] > 8 * a[3] and a[2] == 0 for a in seen["extras"]) and any(a[2] for a in seen["extras"])
    assert any(a[4] and a[0] % 16 for a in seen["extras"]) and any(a[5] and not a[4] and a[0] % 4 for a in seen["extras"])
    assert any(a[0] < 16 for a in seen["map"]) and any(a[2] for a in seen["map"])
