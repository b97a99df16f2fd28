"""Index tables whose tiles have atom windows of a CHOSEN width, for the staging code of the tiled order kernels
(TiledStage::load / TiledStage::store, gorder_amd/csrc/kernels_bonds.h).  Used by tests/test_tile_windows_cpu.py (what the
planner makes of them, and the coverage condition) and tests/test_tile_windows_gpu.py (the kernels against the oracle).

make(width, kind) builds N_TILES = 4 blocks of `width` atoms; the planner (plan.h: build_plan) makes exactly one tile of each,
with n_window == width and atom0 the block's first atom:

  spaced     every block begins 1025 to 1028 atoms behind the end of the one before: a window of 1024 atoms cannot reach
             from one block into the next.  The first atoms' indices are 0, 1, 2, 3 modulo 4.  No leaflets.
  abutting   the blocks lie back to back and each carries exactly 256 samples, so a tile closes on its sample count.  The
             membrane group is the one range over all blocks, global leaflets are assigned in every frame, every head lies
             in the group and a tile owns two heads (types_per_block = 1) — the planner's one-read plan (Plan::spec_ok,
             leaflets_one_read) holds and its ownership ranges leave every window at `width`.  An ODD width gives first atoms
             0, w, 2w, 3w: all four residues modulo 4.  With an EVEN width back-to-back blocks would all begin at the same
             one or two residues, so there each block begins 0 to 3 atoms before the end of the one before (the overlap that
             puts its first atom at residue k): two neighbouring windows then share up to three atoms, which the later tile
             owns.  A sample's lower atom never lies in the shared atoms, so the samples still sort block by block.

n_atoms is 1 modulo 4 (one to four atoms behind the last block, in no sample and no group): the alignment phase
(3 (f n_atoms + atom0)) & 3 of a tile then takes its four values in four consecutive frames, and with the four residues of
atom0 every (stage slot f & 3, phase) pair occurs.

Samples: every tile has 256, made of two molecules with 128 bond types each (types_per_block = 1): molecule type t has its
first molecule in block t and its second in block t + 1, so an accumulator slot receives exactly two samples a frame, one
from each of two tiles — and with leaflets one per side: a wrong atom shows in one named slot.  The atoms a tile's samples
read: its first and last atom; for each of the four phases the lowest and the highest atom with a float in the granules
0, 63, 64, 255, 256, 257, 319, 320, 321 and in the last granule (where the window has them), and one in the middle of every
run of 64 granules (a prefetch register or a late-load trip); the partners are drawn at random over the window.

Geometry: the atoms of a block are a cloud of 0.12 nm (x, y) by 0.1 nm (z) around the block's centre, so bonds are a few tenths
of a nanometre long; two centres lie within 0.1 nm of a face of the 6 x 6 x 10 nm box, so that the wrapped atoms of those
blocks sit on both sides of it and their bonds cross it.  The blocks alternate between two sheets 1.6 nm above and below the
mid-plane, away from the faces along z: no molecule changes sides.  (Even widths, abutting: the shared atoms are placed with
the later block, so the few samples of the earlier tile that read them are some nanometres long — well inside half a box.)

Sentinels: every atom that is in no sample, no membrane group and no head list is NaN in every frame (WindowSystem.frames).
The oracle reads referenced atoms only; a kernel that reads one granule off reads NaN.  One exception: the abutting layout
uses 3e38 instead.  There the only such atoms are the ones behind the last block, whose first floats share a 16-byte granule
with the last window's end and with the next frame's first window; the one-read order kernel checks every float it stages for
finiteness (TiledStage::store<.., FINITE>, its stand-in for the reference's check of the membrane atoms) and hands a frame
with a NaN in such a granule to the exact kernel — legitimately, but that is not the route under test."""
import dataclasses

import numpy as np

from gorder_amd import synthetic
from gorder_amd.abi import LEAFLETS_GLOBAL, Leaflets, MolType, OrderMap, Tables

N_TILES = 4
SAMPLES = 256                # samples of a tile = threads of a workgroup (plan.h: kBlock)
MAX_WINDOW = 1024            # plan.h: kMaxWindow
STAGE = 4                    # frames of a stage (order_route.h: kStageFrames)
LANES = 64                   # threads that stage one frame = granules per prefetch register and per late-load trip
EDGE_GRANULES = (0, 63, 64, 255, 256, 257, 319, 320, 321)
BOX = (6.0, 6.0, 10.0)
SHEET = 1.6
CENTRES = ((0.05, 3.0), (2.0, 5.95), (5.9, 0.1), (4.0, 2.0))
WIDTHS = (3, 85, 339, 340, 341, 342, 425, 426, 427, 428, 860, 1023, 1024)
FIRST_BATCH = 5            # the batch ahead of a speculative one: a whole stage and one frame
WG_FRAMES, WG_TARGET = 33, 2 * N_TILES      # nine stages, two workgroups a tile: GORDER_HIP_WG_TARGET's case
SUB_FRAMES, SUB_RANGE = 14, 6               # sub-ranges of six frames: the second begins at a frame that is no multiple of four


def n_frames_of(width):
    """frames of a width's batch: one or two whole stages and a partial one of 1, 2 or 3 frames (each occurs four times or more)"""
    i = WIDTHS.index(width)
    return STAGE * (1 + i % 2) + 1 + i % 3


def n_granules(phase, width):
    """16-byte granules the staging code moves for a window in alignment phase `phase` (TiledStage: n4)"""
    return (phase + 3 * width + 3) >> 2


def npf_of(width):
    """prefetch registers the route picks for a widest window of `width` atoms (order_route.h: choose_order_route)"""
    return 4 if (3 * width + 6) // 4 <= 4 * LANES else 5


def lds_pitch(width):
    """floats of one staged frame in LDS (gorder_hip.hip: h->lw)"""
    return ((3 * width + 6) // 4) * 4


def atoms_in_granule(phase, g, width):
    """the window-relative atoms with at least one float in granule g"""
    return range(max(0, -((phase + 2 - 4 * g) // 3)), min(width - 1, (4 * g + 3 - phase) // 3) + 1)


def block_starts(width, kind, n_tiles=N_TILES):
    starts = [0]
    for k in range(1, n_tiles):
        if kind == "spaced":
            a = starts[-1] + width + MAX_WINDOW + 1
            a += (k - a) % 4
        elif width % 2:
            a = starts[-1] + width
        else:
            a = starts[-1] + width - (starts[-1] + width - k) % 4
        starts.append(a)
    return starts


def wanted_atoms(width):
    need = {0, width - 1}
    for p in range(4):
        last = n_granules(p, width) - 1
        for g in EDGE_GRANULES + (last,):
            if g <= last:
                r = atoms_in_granule(p, g, width)
                need.update((r[0], r[-1]))
        for g in range(LANES // 2, last + 1, LANES):
            need.add(atoms_in_granule(p, g, width)[0])
    return sorted(need)


def tile_samples(width, rng, lo_limit):
    """SAMPLES pairs (i < j) of window-relative atoms; the lower atom of every pair lies below lo_limit"""
    need = wanted_atoms(width)
    assert len(need) <= SAMPLES
    # (the atoms a window shares with the next one are read once each: they lie with the next block)
    shared, own = [a for a in need if a >= lo_limit], [a for a in need if a < lo_limit]
    firsts = shared + [own[s % len(own)] for s in range(SAMPLES - len(shared))]
    pairs = []
    for a in firsts:
        while True:
            b = int(rng.integers(0, min(width, lo_limit)))
            if b != a:
                break
        pairs.append((min(a, b), max(a, b)))
    return np.array(pairs, dtype=np.uint32)


class WindowSystem(synthetic.System):
    """A System whose unreferenced atoms hold the sentinel in every frame"""
    unreferenced = None
    sentinel = np.nan

    def frames(self, n_frames, seed=0, first=0):
        out = super().frames(n_frames, seed, first)
        out[:, self.unreferenced] = self.sentinel
        return out


@dataclasses.dataclass
class Info:
    width: int
    kind: str
    starts: list
    samples: list            # per tile: [SAMPLES, 2] window-relative atoms
    heads: list              # per tile: the window-relative head atoms placed in it
    referenced: np.ndarray   # bool [n_atoms]: in a sample, the membrane group or a head list
    upper: np.ndarray        # bool [n_molecules_total]: the molecule's sheet


def make(width, kind, types_per_block=1, seed=11, timewise=False, ordermap=False, handle_pbc=True, normal=(0.0, 0.0, 1.0), flags=0,
         n_tiles=N_TILES):
    assert kind in ("spaced", "abutting") and 3 <= width <= MAX_WINDOW and n_tiles % 2 == 0 and (SAMPLES // 2) % types_per_block == 0
    starts = block_starts(width, kind, n_tiles)
    end = starts[-1] + width
    n_atoms = end + 1 + (-end) % 4
    assert n_atoms % 4 == 1 and n_atoms > end
    samples = []
    for k in range(n_tiles):
        nxt = starts[k + 1] if k + 1 < n_tiles else end
        samples.append(tile_samples(width, np.random.default_rng([seed, width, k]), min(width, nxt - starts[k])))
    head_rel = (0, width - 1) if width < 8 else (3, width - 4)          # (never one of the atoms two windows share)
    # molecule type (t, p): its first molecule in block t (samples [p * nb, (p + 1) * nb)), its second in block t + 1 (the same
    # range of that block's second half)
    nb = SAMPLES // 2 // types_per_block
    mts, upper = [], []
    leaflets = kind == "abutting"
    for t in range(n_tiles):
        t2 = (t + 1) % n_tiles
        for p in range(types_per_block):
            bonds = np.empty((nb, 2, 2), dtype=np.uint32)
            bonds[:, 0] = samples[t][p * nb:(p + 1) * nb] + starts[t]
            bonds[:, 1] = samples[t2][SAMPLES // 2 + p * nb:SAMPLES // 2 + (p + 1) * nb] + starts[t2]
            heads = np.array([starts[t] + head_rel[0], starts[t2] + head_rel[1]], dtype=np.uint32)
            mts.append(MolType(n_molecules=2, bonds=bonds, heads=heads if leaflets else None, name=f"T{t}_{p}"))
            upper += [t % 2 == 0, t2 % 2 == 0]
    rng = np.random.default_rng([seed, width, 99])
    base = np.zeros((n_atoms, 3))
    owner = np.full(n_atoms, -1)
    for k in range(n_tiles):
        owner[starts[k]:starts[k] + width] = k          # (shared atoms: the later block's)
    for k in range(n_tiles):
        at = owner == k
        cx, cy = CENTRES[k % 4]
        base[at, 0] = cx + rng.normal(0.0, 0.12, at.sum())
        base[at, 1] = cy + rng.normal(0.0, 0.12, at.sum())
        base[at, 2] = BOX[2] / 2 + (SHEET if k % 2 == 0 else -SHEET) + rng.normal(0.0, 0.1, at.sum())
    box = np.asarray(BOX, dtype=np.float32)
    base = np.mod(base, box).astype(np.float32)
    referenced = np.zeros(n_atoms, dtype=bool)
    for k in range(n_tiles):
        referenced[samples[k].reshape(-1) + starts[k]] = True
    lf = Leaflets()
    if leaflets:
        lf = Leaflets(method=LEAFLETS_GLOBAL, normal_dim=2, frequency=1, membrane=np.arange(starts[0], end, dtype=np.uint32))
        referenced[starts[0]:end] = True
    om = OrderMap(enabled=True, plane=0, span_x=(0.0, BOX[0]), span_y=(0.0, BOX[1]), bin=(1.2, 1.5)) if ordermap else OrderMap()
    tables = Tables(n_atoms=n_atoms, molecule_types=mts, handle_pbc=handle_pbc, normal=normal, leaflets=lf, ordermap=om, timewise=timewise,
                    flags=flags)
    system = WindowSystem(f"{kind}{width}", tables, base, box, jitter=0.02)
    system.unreferenced = ~referenced
    system.sentinel = np.float32(3e38) if leaflets else np.float32(np.nan)
    heads = [[head_rel[0], head_rel[1]] * types_per_block if leaflets else [] for _ in range(n_tiles)]
    return system, Info(width, kind, starts, samples, heads, referenced, np.array(upper))


# ---- what a frame count runs, in plain Python ------------------------------------------------------------------------------
def staging_classes(tiles, n_atoms, n_frames, npf):
    """tiles: [(atom0, n_window, referenced window-relative atoms)] as the planner printed them.  Every float of a tile's
    window in frame f (frames cut into stages of STAGE from frame 0) falls into the classes
        (where, phase, slot):  where = ("register", r) for granule // 64 = r < npf, ("late", 0) for the first late-load trip,
                               ("late", 1) for any later one, and also "first" / "last" for the window's first / last granule
    -> (the classes that exist, the classes a referenced float falls into)"""
    exist, hit = set(), set()
    for atom0, width, atoms in tiles:
        atoms = np.asarray(sorted(atoms))
        for f in range(n_frames):
            slot = f % STAGE
            phase = ((f * n_atoms + atom0) * 3) & 3
            n4 = n_granules(phase, width)
            for into, floats in ((exist, phase + np.arange(3 * width)), (hit, (phase + 3 * atoms[:, None] + np.arange(3)).reshape(-1))):
                g = floats >> 2
                assert g.min() >= 0 and g.max() < n4
                for r in np.unique(g // LANES):
                    into.add((("register", int(r)) if r < npf else ("late", min(int(r) - npf, 1)), phase, slot))
                if (g == 0).any():
                    into.add(("first", phase, slot))
                if (g == n4 - 1).any():
                    into.add(("last", phase, slot))
    return exist, hit


def plan_text(tables):
    """the tables as tests/cabi/tile_windows.cpp reads them"""
    lf = tables.leaflets
    mem = [] if lf.membrane is None else [int(a) for a in lf.membrane]
    out = [f"{tables.n_atoms} {len(tables.molecule_types)} {lf.method} {len(mem)}", " ".join(map(str, mem))]
    for mt in tables.molecule_types:
        b = np.asarray(mt.bonds, dtype=np.uint32).reshape(-1, mt.n_molecules, 2)
        out.append(f"{mt.n_molecules} {b.shape[0]} {0 if mt.heads is None else 1}")
        out.append(" ".join(map(str, b.reshape(-1).tolist())))
        if mt.heads is not None:
            out.append(" ".join(str(int(h)) for h in mt.heads))
    return "\n".join(out) + "\n"


def parse_plan(text):
    """the program's output -> dict(plan=..., tiles=[dict(atom0, n_window, n_items, n_slots, items [n, 4], own, heads)], direct=[...])"""
    plan, tiles, direct = {}, [], []
    for line in text.splitlines():
        w = line.split()
        if w[0] == "plan":
            plan = {w[i]: int(w[i + 1]) for i in range(1, len(w), 2)}
        elif w[0] == "tile":
            tiles.append(dict(zip(("atom0", "n_window", "n_items", "n_slots"), map(int, w[2:]))))
        elif w[0] == "items":
            tiles[int(w[1])]["items"] = np.array(w[2:], dtype=np.int64).reshape(-1, 4)
        elif w[0] == "own":
            tiles[int(w[1])]["own"] = (int(w[2]), int(w[3]))
        elif w[0] == "heads":
            tiles[int(w[1])]["heads"] = np.array(w[2:], dtype=np.int64).reshape(-1, 2)
        elif w[0] == "direct":
            direct.append(tuple(map(int, w[1:])))
    return {"plan": plan, "tiles": tiles, "direct": direct}
