"""What the tests of the device route for error estimates and convergence share: numpy restatements on the copied per-frame
rows (the yardsticks: structure.estimate_error and the cumulative-sum formulation of writers.convergence_text), labels for
the synthetic systems, and the constructions of the NaN and negative-sum cases."""
import numpy as np

from gorder_amd import structure as st
from gorder_amd import synthetic
from gorder_amd.abi import GEOM_CUBOID, GEOMREF_POINT, LEAFLETS_GLOBAL, Geometry


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_floats(got, want):
    """Bit for bit, NaN in the same places."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    keep = ~np.isnan(want)
    np.testing.assert_array_equal(bits(got[keep]), bits(want[keep]))


def host_blocks(tw, n_blocks, total_frames=None, first_position=0):
    """Block sums of the rows `tw` = (sums, counts) [frames][3][n_acc] that sit at the positions first_position.. of an
    analysis of total_frames frames: block size = total_frames // n_blocks, the remainder is dropped."""
    sums, counts = tw
    n = len(sums)
    total = n if total_frames is None else total_frames
    bs = total // n_blocks
    out_s = np.zeros((n_blocks,) + sums.shape[1:], dtype=np.int64)
    out_c = np.zeros((n_blocks,) + counts.shape[1:], dtype=np.uint64)
    for r in range(n):
        b = (first_position + r) // bs if bs else n_blocks
        if b < n_blocks:
            out_s[b] += sums[r]
            out_c[b] += counts[r]
    return out_s, out_c, bs


def host_errors(tw, groups, n_blocks):
    """structure.estimate_error on the members' rows added up, per (group, leaflet) -> float32 [n_groups, 3]."""
    sums, counts = tw
    out = np.zeros((len(groups), 3), dtype=np.float32)
    for g, slots in enumerate(groups):
        for w in range(3):
            out[g, w] = st.estimate_error(sums[:, w, slots].sum(axis=1), counts[:, w, slots].sum(axis=1), n_blocks)
    return out


def host_prefix(tw, groups, carry=None):
    """The convergence columns, restated: cumulative sum / cumulative count per (leaflet, group), truncating toward zero,
    / 1e6 as f32, NaN while the count is 0 -> (prefix float32 [frames, 3, n_groups], (end sums, end counts) [3, n_groups])."""
    sums, counts = tw
    n = len(sums)
    prefix = np.full((n, 3, len(groups)), np.nan, dtype=np.float32)
    end_s = np.zeros((3, len(groups)), dtype=np.int64) if carry is None else np.array(carry[0], dtype=np.int64)
    end_c = np.zeros((3, len(groups)), dtype=np.uint64) if carry is None else np.array(carry[1], dtype=np.uint64)
    for g, slots in enumerate(groups):
        for w in range(3):
            cs = int(end_s[w, g]) + np.cumsum(sums[:, w, slots].sum(axis=1).astype(np.int64))
            cn = int(end_c[w, g]) + np.cumsum(counts[:, w, slots].sum(axis=1).astype(np.int64))
            for f in range(n):
                if cn[f] != 0:
                    q = abs(int(cs[f])) // int(cn[f])
                    prefix[f, w, g] = np.float32((-q if cs[f] < 0 else q) / 1e6)
            if n:
                end_s[w, g], end_c[w, g] = cs[-1], cn[-1]
    return prefix, (end_s, end_c)


# ---- labels of the synthetic systems (slot = bond type, molecule type major) ----------------------------------------
def cg_labels(system):
    labels, slot0 = [], 0
    for mt in system.tables.molecule_types:
        bl = [st.BondLabel(int(a), f"B{a}", int(b), f"B{b}") for a, b in synthetic._CG_BONDS]
        labels.append(st.MolLabels(mt.name, bl, [], mt.n_molecules, slot0))
        slot0 += len(bl)
    return labels


def aa_labels(system):
    carbons, tbonds, _, h_per_c = synthetic._aa_template()
    bl = [st.BondLabel(int(c), f"C{c}", int(h), f"H{h}") for c, h in tbonds]
    heavy = [(int(c), f"C{c}", "POPC") for c, nh in zip(carbons, h_per_c) if nh]
    mt = system.tables.molecule_types[0]
    return [st.MolLabels(mt.name, bl, heavy, mt.n_molecules, 0)]


def type_groups(system):
    """One group per molecule type: what the convergence file prints."""
    out, slot0 = [], 0
    for mt in system.tables.molecule_types:
        out.append(list(range(slot0, slot0 + mt.n_slots)))
        slot0 += mt.n_slots
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------
GAP_FRAMES, GAP_BLOCKS = 20, 5                     # blocks of 4 frames
GAP = (6, 13)                                      # frames [6, 13) hold no sample: block 2 = frames 8..11 lies inside


def gap_case():
    """A geometry selection that is empty for a run of frames covering one whole block: no periodic boundaries, a cuboid
    around the origin that holds the whole box in z, and the membrane moved 100 nm up in the frames of GAP.  The frames
    before the gap start sampled, so the prefix columns are NaN nowhere; see leading_gap_case for that."""
    system = synthetic.cg_membrane(12, handle_pbc=False, timewise=True, n_types=3)
    inf = float("inf")
    system.tables.geometry = Geometry(kind=GEOM_CUBOID, reference=GEOMREF_POINT, point=(0.0, 0.0, 0.0), xdim=(-inf, inf),
                                      ydim=(-inf, inf), zdim=(-1.0, float(system.box[2]) + 1.0))
    xyz = system.frames(GAP_FRAMES, seed=8)
    xyz[GAP[0]:GAP[1], :, 2] += 100.0
    return system, xyz


def leading_gap_case():
    """The same with the gap first: frames [0, 5) hold no sample, so the prefix columns start with five NaN rows."""
    system, xyz = gap_case()
    xyz = np.concatenate([xyz[GAP[0]:GAP[0] + 5], xyz[:GAP[0]], xyz[GAP[1]:]])
    return system, xyz


def planar_aa_case(n_frames=10):
    """All-atom bonds that lie in the membrane plane: every hydrogen 0.109 nm from its carbon in a direction with z = 0,
    so S = (3 cos^2 - 1) / 2 is about -0.5 and every tick sum is negative."""
    system = synthetic.aa_membrane(8, leaflets=LEAFLETS_GLOBAL, timewise=True)
    system.jitter = 0.004
    _, tbonds, apl, _ = synthetic._aa_template()
    rng = np.random.default_rng(17)
    base = system.base.astype(np.float64)
    for m in range(8):
        phi = rng.uniform(0.0, 2.0 * np.pi, len(tbonds))
        for b, (ci, hi) in enumerate(tbonds):
            base[m * apl + hi] = base[m * apl + ci] + 0.109 * np.array([np.cos(phi[b]), np.sin(phi[b]), 0.0])
    system.base = np.mod(base, system.box).astype(np.float32)
    return system, system.frames(n_frames, seed=2)
