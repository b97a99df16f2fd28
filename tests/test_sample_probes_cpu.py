"""The probes of tests/sample_probes.py hit the floats they claim; its literal float32 statement of the default sample
agrees with the oracle on every one of them (split tables, one sample per slot, no tolerance, no probe left out); the
oracle's restatement of the literal cosine equals the host's libm on every probe; and four planted mutants of the
literal statement are each seen by a probe of the family that names the rule.  CPU only."""
import platform

import numpy as np
import pytest

import sample_probes as sp
from sample_probes import F
from gorder_amd.abi import FLAG_TRIG_ACOS_COS, Leaflets, MolType, Tables
from oracle import oracle
from test_order_histogram_gpu import oracle_samples

AXES = (0, 1, 2)
BOX_NAMES = (None, "dyadic", "three edges")
GENERIC = (1.0, 1.0, 0.5)
LIBM_IS_GLIBC = platform.libc_ver()[0] == "glibc" and "2.28" <= platform.libc_ver()[1] <= "2.40"   # (tests/test_parity_gpu.py)


# ---- tables for a probe system (shared with the GPU test) ------------------------------------------------------------------
def probe_tables(ps, normal=(0.0, 0.0, 1.0), leaflets=None, **kw):
    """One molecule type of ps.n_mol molecules; heads only where leaflets want them.  The membrane group of global
    leaflets is the heads: no probe atom is in any group."""
    lf = leaflets or Leaflets()
    if lf.method and lf.membrane is None:
        lf.membrane = ps.heads
    mt = MolType(n_molecules=ps.n_mol, bonds=ps.bonds, heads=ps.heads if lf.method else None)
    return Tables(n_atoms=ps.n_atoms, molecule_types=[mt], handle_pbc=ps.box9 is not None,
                  normal=tuple(float(x) for x in normal), leaflets=lf, **kw)


def case(axis, box_name, products=False, **kw):
    box = None if box_name is None else sp.BOXES[box_name]
    return sp.probe_system(sp.bond_probes(axis, box, products), axis, box, **kw)


def probe_ticks(ps, samples):
    """The oracle's per-sample ticks [frames, samples] as one tick per probe: every frame must tell the same."""
    which = ps.which.reshape(len(ps.xyz), -1)
    out = np.zeros(len(ps.probes), dtype=np.int64)
    out[which[0]] = samples.tick[0]
    np.testing.assert_array_equal(samples.tick, out[which], err_msg="a probe's tick depends on its slot or frame")
    return out


# ---- 1. the probes are where they say ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", AXES)
def test_guard_and_norm_probes_land_on_their_floats(axis):
    for upper in (False, True):
        g = sp.GUARD_HI if upper else sp.GUARD_LO
        probes = sp.guard_probes(axis, upper)
        for o in sp.ORIENTATIONS:
            steps = sorted(p.where for p in probes if p.rule.endswith(o))
            assert steps == ([-2, 0, 2] if o == "along" else list(sp.GUARD_STEPS)), (o, steps)
        n = sp.axis_normal(axis)
        for p in probes:
            v = sp.literal_vector(p.p1, p.p2)
            s2 = sp.norm2(v)
            assert s2 == p.s2 == sp.step(g, p.where), p.rule                        # the intended float, exactly
            assert p.outside == (not (s2 >= sp.GUARD_LO and s2 <= sp.GUARD_HI)), p.rule
            num = F(sp.dot3(v, n) * sp.dot3(v, n))
            if p.rule.endswith("along"):
                assert num == s2 and sp.literal_tick(v, n) == 1000000               # the quotient is exactly 1
            if p.rule.endswith("across"):
                assert num == 0 and sp.literal_tick(v, n) == -500000
            if p.rule.endswith("tiny numerator"):
                assert 0 < num < F(2.0 ** -103) and num >= np.finfo(np.float32).tiny
            if p.rule.endswith("denormal numerator"):
                assert 0 < num < np.finfo(np.float32).tiny
            if p.rule.endswith("oblique"):
                assert -400000 < sp.literal_tick(v, n) < 900000
    for periodic in (False, True):
        for p in sp.norm_probes(axis, periodic):
            s2 = sp.norm2(sp.literal_vector(p.p1, p.p2))
            assert p.s2 is None or s2 == p.s2, p.rule
            assert not (s2 >= sp.GUARD_LO and s2 <= sp.GUARD_HI), p.rule
            if "denormal" in p.rule:
                assert 0 < s2 < np.finfo(np.float32).tiny
            if "underflow" in p.rule:
                assert sp.dot3(sp.literal_vector(p.p1, p.p2), sp.axis_normal(axis)) != 0
            if "1e38" in p.rule:
                assert sp.GUARD_HI < s2 < sp.INF
            assert np.isfinite(p.p1).all() and np.isfinite(p.p2).all()
    for p in sp.nonfinite_probes():
        assert np.isfinite(p.p1[0]) and np.isfinite(p.p2[0]) and np.isinf(np.concatenate([p.p1, p.p2])).sum() == 1
        assert sp.literal_tick(sp.literal_vector(p.p1, p.p2), sp.axis_normal(axis)) == 0
        assert sp.literal_tick(sp.literal_vector(p.p1, p.p2), np.array(GENERIC, dtype=F)) == 0


def test_product_probes_over_and_underflow_with_finite_norms():
    probes, normals = sp.product_probes()
    seen = []
    for p, n in zip(probes, [normals["tiny"]] * 2 + [normals["huge"]] * 2):
        v = sp.literal_vector(p.p1, p.p2)
        s2, n2sq = sp.norm2(v), sp.norm2(n)
        assert 0 < s2 < sp.INF and 0 < n2sq < sp.INF
        with np.errstate(all="ignore"):
            seen.append((float(F(s2 * n2sq)), sp.literal_tick(v, n)))
    assert seen[0] == (0.0, 0) and seen[2] == (float("inf"), -500000) and seen[3] == (float("inf"), 0)       # NaN twice: tick 0
    assert 0 < seen[1][0] < np.finfo(np.float32).tiny and -500000 < seen[1][1] < 1000000


@pytest.mark.parametrize("box_name", ["dyadic", "three edges"])
def test_image_probes_fire_the_slow_conditions_where_the_label_says(box_name):
    box = np.array(sp.BOXES[box_name], dtype=F)
    probes = sp.image_probes(box)
    fired = {"literal": 0, "magnitude": 0, "magnitude only": 0}
    for p in probes:
        d = sp.literal_vector(p.p1, p.p2)                                          # p1 is the origin: the offset itself
        assert np.array_equal(d, p.p2)
        for k in range(3):
            if p.where[k] is not None:
                place, off = p.where[k]
                assert abs(d[k]) == sp.step(F(np.float64(box[k]) * place), off) and abs(d[k]) < sp.MI_MAX_ITER * box[k]
        lit, mag = sp.slow_literal(d, box), sp.slow_magnitude(d, box)
        assert (lit, mag) == p.slow, p.rule
        assert mag or not lit                                                      # the magnitude form's condition is a superset
        fired["literal"] += lit
        fired["magnitude"] += mag
        fired["magnitude only"] += mag and not lit
        v = sp.literal_vector(p.p1, p.p2, box)
        assert (np.abs(v) <= box / F(2)).all()
        if not lit:                                                                # one shift per dimension was the whole loop
            assert np.array_equal(v, sp.literal_vector(p.p1, p.p2, box, shifts=1))
    assert min(fired.values()) >= 6, fired
    # every place, both signs, every dimension
    for k in range(3):
        places = {(p.where[k][0], p.where[k][1], bool(p.p2[k] > 0)) for p in probes if p.where[k] is not None}
        assert {(a, b) for a, b, _ in places} >= {(x, o) for x in sp.IMAGE_PLACES for o in (-1, 0, 1)} | {(4.5, 0)}
        assert (4.5, 0, True) in places and (4.5, 0, False) in places


def test_no_probe_atom_is_a_head_and_heads_keep_their_distance():
    for axis in AXES:
        for box_name in BOX_NAMES:
            ps = case(axis, box_name, swap_from=5)
            bonded = set(ps.bonds.reshape(-1).tolist())
            assert not bonded & set(ps.heads.tolist()) and len(bonded) == 2 * ps.n_mol * sp.B_SLOTS
            mid = 0.0 if ps.box9 is None else float(ps.box9[0, axis, axis]) / 2
            assert (np.abs(ps.xyz[:, ps.heads, axis] - mid) >= 1.0).all()
            assert np.array_equal(ps.xyz[:, ps.heads, axis] > mid, ps.upper)
            assert ps.upper[:, 0].tolist() == [True] * 5 + [False] * 4 and ps.upper.sum(axis=1).tolist() == [ps.n_mol // 2] * 9
            assert ps.n_atoms <= 400 and sorted(np.unique(ps.which).tolist()) == list(range(len(ps.probes)))


# ---- 2. the oracle against the literal statement, probe by probe ------------------------------------------------------------------
def normals_of(axis):
    return [tuple(float(x) for x in sp.axis_normal(axis)), GENERIC]


@pytest.mark.parametrize("box_name", BOX_NAMES)
@pytest.mark.parametrize("axis", AXES)
def test_the_oracle_is_the_literal_statement_on_every_probe(built, axis, box_name):
    ps = case(axis, box_name)
    v = ps.vectors()
    for normal in normals_of(axis):
        tables = probe_tables(ps, normal)
        ticks = probe_ticks(ps, oracle_samples(tables, ps.xyz, ps.box9, oracle.TRIG_DIRECT))
        literal = np.array([sp.literal_tick(x, np.array(normal, dtype=F)) for x in v])
        bad = np.flatnonzero(ticks != literal)
        assert not bad.size, [(ps.probes[i].rule, int(ticks[i]), int(literal[i])) for i in bad[:8]]
        if normal != GENERIC:       # every end of the range is met: NaN, S = 1, S = -1/2
            assert (literal == 1000000).sum() >= 3 and (literal == -500000).sum() >= 3
            # (in a periodic box every bond vector is finite and short: no NaN without a degenerate normal)
            assert (literal == 0).sum() >= (0 if box_name else 8)


@pytest.mark.parametrize("name", ["tiny", "huge"])
def test_the_oracle_is_the_literal_statement_where_the_product_of_the_norms_leaves_the_range(built, name):
    probes, normals = sp.product_probes()
    ps = sp.probe_system(probes + sp.bond_probes(2, None))
    n = normals[name]
    ticks = probe_ticks(ps, oracle_samples(probe_tables(ps, n), ps.xyz, None, oracle.TRIG_DIRECT))
    literal = np.array([sp.literal_tick(x, n) for x in ps.vectors()])
    np.testing.assert_array_equal(ticks, literal)
    assert {int(t) for t in literal[:4]} >= {0, -500000}


@pytest.mark.parametrize("box_name", BOX_NAMES)
@pytest.mark.parametrize("axis", AXES)
def test_the_restated_libm_is_the_hosts_on_every_probe(built, axis, box_name):
    ps = case(axis, box_name)
    for normal in normals_of(axis):
        tables = probe_tables(ps, normal, flags=FLAG_TRIG_ACOS_COS)
        mirror = probe_ticks(ps, oracle_samples(tables, ps.xyz, ps.box9, oracle.TRIG_MIRROR))
        assert ((mirror >= -500000) & (mirror <= 1000000)).all()
        if LIBM_IS_GLIBC:
            np.testing.assert_array_equal(mirror, probe_ticks(ps, oracle_samples(tables, ps.xyz, ps.box9, oracle.TRIG_LIBM)))
        # the literal cosine keeps the zero-norm rule and the NaN rule of the default form
        direct = probe_ticks(ps, oracle_samples(tables, ps.xyz, ps.box9, oracle.TRIG_DIRECT))
        for i, p in enumerate(ps.probes):
            if p.rule.startswith("zero norm"):
                assert mirror[i] == direct[i] == 1000000
            if p.family == "nonfinite":
                assert mirror[i] == direct[i] == 0


@pytest.mark.parametrize("box_name", BOX_NAMES)
def test_the_oracle_is_the_literal_statement_against_supplied_normals(built, box_name):
    """Normals handed over per molecule and frame are used as they are: zero, NaN, of length 1e-25 and 1e25, oblique."""
    ps = case(2, box_name)
    normals = sp.supplied_normals(ps.n_mol)
    n2 = np.array([sp.norm2(n) for n in sp.SUPPLIED])
    assert n2[0] == 0 and np.isnan(n2[1]) and n2[2] == 0 and n2[3] == sp.INF and 0 < n2[6] < sp.GUARD_LO ** 2 * 4 and n2[7] > sp.GUARD_HI
    split = probe_tables(ps)
    ref = oracle.OracleEngine(split_per_sample(split, ps), trig=oracle.TRIG_DIRECT)
    ref.set_normals(np.repeat(normals, sp.B_SLOTS, axis=1))                      # a molecule of the split tables is one sample
    ref.submit(ps.xyz, ps.box9)
    s, c = ref.timewise(sp.N_FRAMES)
    assert (c[:, 0] == 1).all()
    literal = sp.literal_ticks_with_normals(ps, normals)
    np.testing.assert_array_equal(s[:, 0].reshape(literal.shape), literal)
    kinds = (np.arange(ps.n_mol)[None, :] + np.arange(sp.N_FRAMES)[:, None]) % len(sp.SUPPLIED)
    assert (literal[kinds == 0] == 1000000).all() and (literal[kinds == 2] == 1000000).all()      # a zero norm: S = 1
    zero_bond = np.array([p.rule.startswith("zero norm") for p in ps.probes])[ps.which]
    nan_normal = np.broadcast_to((kinds == 1)[:, :, None], literal.shape)
    assert not literal[nan_normal & ~zero_bond].any()                        # a NaN normal: tick 0 ...
    assert (literal[nan_normal & zero_bond] == 1000000).all()                # ... but the zero-norm rule comes last: S = 1
    # every probe family meets every kind of normal
    fam = np.array([p.family for p in ps.probes])[ps.which]
    for name in set(fam.reshape(-1).tolist()):
        assert len({int(k) for k in np.broadcast_to(kinds[:, :, None], fam.shape)[fam == name]}) == len(sp.SUPPLIED), name


def split_per_sample(tables, ps):
    """Every bond sample a molecule type of its own (one molecule, one bond), molecule-major like ps.which; per-frame rows."""
    import dataclasses
    atoms = np.transpose(ps.bonds, (1, 0, 2)).reshape(-1, 2)
    return dataclasses.replace(tables, molecule_types=[MolType(n_molecules=1, bonds=a.reshape(1, 1, 2)) for a in atoms],
                               leaflets=Leaflets(), timewise=True, flags=0)


def test_the_oracles_tick_is_rusts_cast():
    """`(value as f64 * 1e6).round() as i64` (order.rs:21-26): NaN is 0, an infinity saturates.  gorder_oracle_tick tests
    for both before it converts: no float-to-int conversion of a non-finite value is left to C."""
    assert oracle.tick(np.nan) == 0 and oracle.tick(np.inf) == 2 ** 63 - 1 and oracle.tick(-np.inf) == -2 ** 63
    for s in (1.0, -0.5, 0.4999995, -0.4999995, 1e-7, -1e-7, 0.0):
        assert oracle.tick(s) == sp.literal_round(s)


# ---- 3. planted mutants of the literal statement -------------------------------------------------------------------------------
def all_probes(axis=2):
    out = []
    for box_name in BOX_NAMES:
        box = None if box_name is None else sp.BOXES[box_name]
        out += [(p, box) for p in sp.bond_probes(axis, box)]
    return out


def ticks_with(probes, normal, shifts=sp.MI_MAX_ITER, **kw):
    return np.array([sp.literal_tick(sp.literal_vector(p.p1, p.p2, box, shifts), normal, **kw) for p, box in probes])


@pytest.mark.parametrize("axis", AXES)
def test_planted_mutants_are_seen_by_the_family_that_names_the_rule(axis):
    probes = all_probes(axis)
    family = np.array([p.family for p, _ in probes])
    n = sp.axis_normal(axis)
    right = ticks_with(probes, n)

    def seen_by(wrong):
        return set(family[wrong != right].tolist())

    # a NaN sample becomes INT_MIN (C's cast on the host) instead of 0
    assert "nonfinite" in seen_by(ticks_with(probes, n, nan_tick=sp.INT_MIN)) and "norm" in seen_by(ticks_with(probes, n, nan_tick=sp.INT_MIN))
    # a zero norm gives NaN instead of S = 1
    wrong = ticks_with(probes, n, zero_norm_nan=True)
    assert seen_by(wrong) == {"norm"}
    assert all(p.rule.startswith("zero norm") for (p, _), w, r in zip(probes, wrong, right) if w != r)
    assert sum(p.rule.startswith("zero norm") for (p, _), w, r in zip(probes, wrong, right) if w != r) == 9      # three forms, three tables
    # the fast path without its fallback: with the guard where it is, exactly the probes labelled `outside` are left
    # unwritten; a guard one float off, either way and at either end, moves a probe of the guard family and no other
    stated = ticks_with(probes, n, guard=(sp.GUARD_LO, sp.GUARD_HI))
    outside = np.array([bool(p.outside) for p, _ in probes])
    assert np.array_equal(stated != right, outside) and outside[family == "guard"].any() and not outside[family == "guard"].all()
    for lo_off, hi_off, where, upper in ((1, 0, 0, False), (-1, 0, -1, False), (0, -1, 0, True), (0, 1, 1, True)):
        wrong = ticks_with(probes, n, guard=(sp.step(sp.GUARD_LO, lo_off), sp.step(sp.GUARD_HI, hi_off)))
        moved = [p for (p, _), w, s in zip(probes, wrong, stated) if w != s]
        assert moved and all(p.family == "guard" and p.where == where and ("upper" in p.rule) == upper for p in moved)
        # every orientation at that float (no bond along the normal on an odd float), in every table that holds that guard
        assert len(moved) == (len(sp.ORIENTATIONS) - where % 2) * (1 if upper else len(BOX_NAMES))
    # no second image shift
    wrong = ticks_with(probes, n, shifts=1)
    assert seen_by(wrong) == {"image"}
    assert all(p.slow[0] for (p, _), w, r in zip(probes, wrong, right) if w != r)
    assert (wrong != right).sum() >= 12


# ---- 4. degenerate united-atom carbons -------------------------------------------------------------------------------------------
UA_BOX = (8.0, 8.0, 8.0)
UA_LIPIDS, UA_APL = 6, 52
# (carbon, first helper, second helper), lipid-relative, one per kind and no atom twice: the methyl 41, the methylene 12,
# the double-bond carbon 20 and the saturated CH 15 (its third helper, 24, stays where it is)
UA_CARBONS = [(41, 40, 39), (12, 11, 13), (20, 19, 21), (15, 14, 16)]


def ua_case(pbc, leaflets=0, flags=0, **kw):
    """synthetic.ua_membrane, six lipids in a dyadic box, nine frames with the degenerate carbons of sample_probes planted
    -> (tables, xyz, box9, label).  The membrane group of global leaflets is the heads alone: no planted atom is in it."""
    from gorder_amd import synthetic
    system = synthetic.ua_membrane(UA_LIPIDS, box=UA_BOX, handle_pbc=pbc, leaflets=leaflets, frequency=3, **kw)
    mt = system.tables.molecule_types[0]
    if leaflets:
        system.tables.leaflets.membrane = np.asarray(mt.heads)
    system.tables.flags = flags
    xyz, label = sp.ua_degenerate(system.frames(sp.N_FRAMES, seed=3), UA_CARBONS, UA_LIPIDS, UA_APL, UA_BOX if pbc else None)
    return system.tables, xyz, system.box9(sp.N_FRAMES) if pbc else None, label


@pytest.mark.parametrize("pbc", [True, False])
def test_degenerate_carbons_are_exactly_degenerate_and_the_oracle_takes_them(built, pbc):
    from gorder_amd import abi
    tables, xyz, box9, label = ua_case(pbc, leaflets=abi.LEAFLETS_GLOBAL)
    mt = tables.molecule_types[0]
    kind_of = {int(idx[0, 3]) if int(k) == abi.UA_CH1_SAT else int(idx[0, 1]): int(k) for k, idx in mt.ua_atoms}
    assert [kind_of[c] for c, _, _ in UA_CARBONS] == [abi.UA_CH3, abi.UA_CH2, abi.UA_CH1_UNSAT, abi.UA_CH1_SAT]
    planted = {m * UA_APL + k for m in range(UA_LIPIDS) for trio in UA_CARBONS for k in trio}
    assert not planted & set(np.asarray(mt.heads).tolist()) and set(np.asarray(tables.leaflets.membrane).tolist()) == set(np.asarray(mt.heads).tolist())
    assert (np.abs(xyz[:, np.asarray(mt.heads), 2] - UA_BOX[2] / 2) >= 1.0).all()      # no head near the mid-plane
    box = UA_BOX if pbc else None
    seen = set()
    for (f, m, j), case in np.ndenumerate(label):
        c, h1, h2 = (m * UA_APL + k for k in UA_CARBONS[j])
        raw1 = (xyz[f, h1] - xyz[f, c]).astype(F)
        th1, th2 = sp.literal_vector(xyz[f, c], xyz[f, h1], box), sp.literal_vector(xyz[f, c], xyz[f, h2], box)
        cross = np.cross(th1.astype(np.float64), th2.astype(np.float64))          # (exact: the coordinates are dyadic)
        if case == 0:
            assert not th1.any()
        elif case == 1:
            assert np.array_equal(th1, th2) and th1.any() and not cross.any()
        elif case == 2:
            assert np.array_equal(th1, -th2) and th1.any() and not cross.any()
        else:
            assert np.abs(raw1).max() > 2.0 * UA_BOX[0] and (not pbc or sp.slow_literal(raw1, UA_BOX))
        seen.add((j, int(case)))
    assert len(seen) == len(UA_CARBONS) * len(sp.UA_CASES)
    for trig, flags in ((oracle.TRIG_DIRECT, 0), (oracle.TRIG_MIRROR, FLAG_TRIG_ACOS_COS), (oracle.TRIG_LIBM, FLAG_TRIG_ACOS_COS),
                        (oracle.TRIG_DIRECT, abi.FLAG_UA_FAST_NORMALISE)):
        tables.flags = flags
        o = oracle.OracleEngine(tables, trig=trig)
        o.submit(xyz, box9)
        res = o.finish()
        assert (res.counts[0] == sp.N_FRAMES * UA_LIPIDS).all()                     # a NaN hydrogen is tick 0, and counted
        if trig == oracle.TRIG_MIRROR:
            mirror = res
        if trig == oracle.TRIG_LIBM and LIBM_IS_GLIBC:
            np.testing.assert_array_equal(res.sums, mirror.sums)
