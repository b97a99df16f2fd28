"""Error estimates and convergence columns made on the device from the per-frame rows (gorder_hip_timewise_blocks,
gorder_hip_error_estimate, gorder_hip_convergence; kernels_timewise.h).  The yardstick is never the code under test: it is
structure.estimate_error and the cumulative-sum formulation of the convergence writer applied to the rows gorder_hip_timewise
copies to the host (tests/timewise_device_util.py), and the reference's own files.  Every comparison is exact: integers by
array_equal, floats bit for bit with NaN in the same places."""
import numpy as np
import pytest

from gorder_amd import HipEngine, abi, synthetic, writers
from gorder_amd import structure as st
from gorder_amd.abi import LEAFLETS_GLOBAL, LEAFLETS_MANUAL
from golden_util import METHODS, Fixture, aa_setup, cg_setup, ua_setup
from test_writers_cpu import golden, same_items, same_tokens
import timewise_device_util as tu

pytestmark = pytest.mark.gpu

C = abi.timewise_chunk_frames()
BLOCK_COUNTS = (2, 5, 7)


def engine(system, xyz, cuts=(), box=True, first=0):
    """A handle fed the frames in the batches [0, cuts[0]), [cuts[0], cuts[1]), ..."""
    eng = HipEngine(system.tables)
    feed(eng, system, xyz, cuts, box, first)
    return eng


def feed(eng, system, xyz, cuts=(), box=True, first=0):
    edges = [0, *cuts, len(xyz)]
    for a, b in zip(edges[:-1], edges[1:]):
        if b > a:
            eng.submit_host(xyz[a:b], system.box9(b - a) if box else None, np.arange(first + a, first + b))


def rows(eng):
    eng.finish()
    return eng.timewise(eng.timewise_rows())


@pytest.fixture(scope="module")
def cg(built):
    """CG, three molecule types, global leaflets: the system, its longest run of frames, its labels."""
    system = synthetic.cg_membrane(12, leaflets=LEAFLETS_GLOBAL, timewise=True, n_types=3)
    return system, system.frames(2 * C + 3, seed=5), tu.cg_labels(system)


@pytest.mark.parametrize("n_frames", [1, 4, 13, C - 1, C, C + 1, 2 * C + 3])
def test_block_sums(cg, n_frames):
    system, xyz, _ = cg
    xyz = xyz[:n_frames]
    one = engine(system, xyz)
    three = engine(system, xyz, cuts=(n_frames // 5, n_frames // 5 + (n_frames + 1) // 2))
    tw = rows(one)
    assert len(tw[0]) == n_frames and one.timewise_rows() == three.timewise_rows() == n_frames
    for n_blocks in BLOCK_COUNTS:
        want_s, want_c, want_bs = tu.host_blocks(tw, n_blocks)
        for eng in (one, three):
            s, c, bs = eng.timewise_blocks(n_blocks)
            assert bs == want_bs == n_frames // n_blocks
            np.testing.assert_array_equal(s, want_s)
            np.testing.assert_array_equal(c, want_c)
        if want_bs:
            assert want_c[:, 0].all() and (want_c[:, 1] + want_c[:, 2] == want_c[:, 0]).all()
        else:
            assert not want_c.any()


@pytest.mark.parametrize("kind", ["cg", "aa"])
def test_errors_of_the_groups_of_the_result_tree(cg, kind):
    if kind == "cg":
        system, xyz, labels = cg
        xyz = xyz[:C + 9]
    else:
        system = synthetic.aa_membrane(8, leaflets=LEAFLETS_GLOBAL, timewise=True)
        xyz, labels = system.frames(23, seed=3), tu.aa_labels(system)
    groups = st.error_groups(labels, kind)
    sizes = {len(g) for g in groups}
    assert 1 in sizes and system.tables.n_acc in sizes and len(sizes) >= 3      # singletons, the system, groups in between
    eng = engine(system, xyz, cuts=(5,))
    tw = rows(eng)
    for n_blocks in BLOCK_COUNTS:
        want = tu.host_errors(tw, groups, n_blocks)
        assert not np.isnan(want).any()
        tu.same_floats(eng.error_estimate(groups, n_blocks), want)
    # members in another order, a group listed twice, one slot in several groups: sums do not care
    odd = [groups[-1][::-1], groups[0], groups[0], [0, system.tables.n_acc - 1, 3]]
    tu.same_floats(eng.error_estimate(odd), tu.host_errors(tw, odd, 5))


def test_nan_rules(built):
    # every lipid in the upper leaflet: the lower leaflet holds no sample, its error and its columns are NaN
    system = synthetic.cg_membrane(12, leaflets=LEAFLETS_MANUAL, timewise=True, n_types=3)
    eng = HipEngine(system.tables)
    eng.set_manual_leaflets(np.zeros(12, dtype=np.uint8))
    feed(eng, system, system.frames(11, seed=1))
    tw, groups = rows(eng), tu.type_groups(system)
    assert not tw[1][:, 2].any() and tw[1][:, 1].all()
    errors = eng.error_estimate(groups, 5)
    tu.same_floats(errors, tu.host_errors(tw, groups, 5))
    assert np.isnan(errors[:, 2]).all() and not np.isnan(errors[:, :2]).any()
    prefix, end = eng.convergence(groups)
    tu.same_floats(prefix, tu.host_prefix(tw, groups)[0])
    assert np.isnan(prefix[:, 2]).all() and not np.isnan(prefix[:, :2]).any() and not end[1][2].any()
    # a geometry selection that is empty in the frames of one whole block (the construction is checked against the oracle
    # in test_timewise_device_cpu.py): that block's count is 0 and the error NaN; with two blocks it is a number
    system, xyz = tu.gap_case()
    eng = engine(system, xyz, cuts=(9,), box=False)
    tw, groups = rows(eng), tu.type_groups(system)
    per_frame = tw[1][:, 0].sum(axis=1)
    assert (per_frame[tu.GAP[0]:tu.GAP[1]] == 0).all() and np.delete(per_frame, np.arange(*tu.GAP)).all()
    s, c, bs = eng.timewise_blocks(tu.GAP_BLOCKS)
    assert bs == 4 and not c[2].any() and c[[0, 1, 3, 4], 0].all()
    for n_blocks in (tu.GAP_BLOCKS, 2):
        errors = eng.error_estimate(groups, n_blocks)
        tu.same_floats(errors, tu.host_errors(tw, groups, n_blocks))
        assert np.isnan(errors[:, 0]).all() == (n_blocks == tu.GAP_BLOCKS)
    # the prefix columns are NaN exactly while the cumulative count is 0
    system, xyz = tu.leading_gap_case()
    eng = engine(system, xyz, box=False)
    tw = rows(eng)
    prefix, _ = eng.convergence(groups)
    tu.same_floats(prefix, tu.host_prefix(tw, groups)[0])
    np.testing.assert_array_equal(np.isnan(prefix[:, 0, :]), np.cumsum(tw[1][:, 0].sum(axis=1))[:, None].repeat(3, 1) == 0)
    assert np.isnan(prefix[:5, 0]).all() and not np.isnan(prefix[5:, 0]).any() and np.isnan(prefix[:, 1:]).all()


def test_negative_sums_truncate_toward_zero(built):
    system, xyz = tu.planar_aa_case()
    eng = engine(system, xyz, cuts=(3,))
    tw, labels = rows(eng), tu.aa_labels(system)
    s, c, _ = eng.timewise_blocks(5)
    want_s, want_c, _ = tu.host_blocks(tw, 5)
    np.testing.assert_array_equal(s, want_s)
    np.testing.assert_array_equal(c, want_c)
    # the case cannot pass by floor division: a negative block sum that its count does not divide
    assert ((s[:, 0] < 0) & (np.abs(s[:, 0]) % c[:, 0].astype(np.int64) != 0)).any() and (s[:, 0] < 0).all()
    groups = st.error_groups(labels, "aa")
    tu.same_floats(eng.error_estimate(groups, 5), tu.host_errors(tw, groups, 5))
    prefix, _ = eng.convergence(tu.type_groups(system))
    want, _ = tu.host_prefix(tw, tu.type_groups(system))
    tu.same_floats(prefix, want)
    assert (want[:, 0] < -0.45).all()
    floor = np.float32(np.floor_divide(np.cumsum(tw[0][:, 0].sum(axis=1)), np.cumsum(tw[1][:, 0].sum(axis=1)).astype(np.int64)) / 1e6)
    assert (floor != want[:, 0, 0]).any()


@pytest.mark.parametrize("leaflets", [True, False])
@pytest.mark.parametrize("n_frames", [1, C, C + 1, 2 * C + 3])
def test_convergence_columns(cg, leaflets, n_frames):
    system, xyz, _ = cg
    if not leaflets:
        system = synthetic.cg_membrane(12, timewise=True, n_types=3)
    eng = engine(system, xyz[:n_frames], cuts=(n_frames // 3,))
    tw, groups = rows(eng), tu.type_groups(system)
    assert len(groups) == 3
    prefix, end = eng.convergence(groups)
    want, want_end = tu.host_prefix(tw, groups)
    tu.same_floats(prefix, want)
    np.testing.assert_array_equal(end[0], want_end[0])
    np.testing.assert_array_equal(end[1], want_end[1])
    assert np.isnan(prefix[:, 1:]).all() == (not leaflets) and not np.isnan(prefix[:, 0]).any()


@pytest.mark.parametrize("k", ["two blocks", 3, "two blocks and five", C + 1])
def test_two_shards_on_one_card(cg, k):
    system, xyz, labels = cg
    n_frames, n_blocks = C + 7, 5                     # more than one chunk; the last frames are dropped unless 5 divides C + 7
    xyz = xyz[:n_frames]
    size = n_frames // n_blocks
    k = {"two blocks": 2 * size, "two blocks and five": 2 * size + 5}.get(k, k)
    assert 0 < k < n_frames and (k % size == 0) == (k == 2 * size) and size > 5
    whole = engine(system, xyz)
    a, b = engine(system, xyz[:k]), engine(system, xyz[k:], first=k)
    s, c, bs = whole.timewise_blocks(n_blocks)
    sa, ca, bsa = a.timewise_blocks(n_blocks, total_frames=n_frames)
    sb, cb, bsb = b.timewise_blocks(n_blocks, total_frames=n_frames, first_position=k)
    assert bs == bsa == bsb == n_frames // n_blocks
    np.testing.assert_array_equal(sa + sb, s)
    np.testing.assert_array_equal(ca + cb, c)
    assert sa.any() and sb.any()
    groups = st.error_groups(labels, "cg")
    want = whole.error_estimate(groups, n_blocks)
    tu.same_floats(want, tu.host_errors(rows(whole), groups, n_blocks))
    for eng in (a, b):                                # either rank may finish the merged blocks
        tu.same_floats(eng.error_estimate(groups, n_blocks, blocks=(sa + sb, ca + cb)), want)
    types = tu.type_groups(system)
    prefix, end = whole.convergence(types)
    pa, mid = a.convergence(types)
    pb, end_b = b.convergence(types, carry=mid)
    tu.same_floats(np.concatenate([pa, pb]), prefix)
    np.testing.assert_array_equal(end_b[0], end[0])
    np.testing.assert_array_equal(end_b[1], end[1])


def test_life_cycle_and_refusals(cg):
    system, xyz, labels = cg
    groups = tu.type_groups(system)
    eng = engine(system, xyz[:9])
    first = eng.error_estimate(groups, 2)
    tu.same_floats(first, tu.host_errors(rows(eng), groups, 2))
    feed(eng, system, xyz[9:C + 20], first=9)         # a longer history (the rows were reallocated on the way)
    tw = rows(eng)
    assert len(tw[0]) == C + 20
    tu.same_floats(eng.error_estimate(groups, 2), tu.host_errors(tw, groups, 2))
    tu.same_floats(eng.convergence(groups)[0], tu.host_prefix(tw, groups)[0])
    np.testing.assert_array_equal(eng.timewise(C + 20)[0], tw[0])            # the calls leave the rows as they are
    eng.reset()
    assert eng.timewise_rows() == 0
    assert np.isnan(eng.error_estimate(groups, 5)).all()                     # zero rows: NaN, status OK
    s, c, bs = eng.timewise_blocks(5)
    assert bs == 0 and not s.any() and not c.any()
    carry = (np.arange(9, dtype=np.int64).reshape(3, 3), np.arange(9, dtype=np.uint64).reshape(3, 3))
    prefix, end = eng.convergence(groups, carry=carry)
    assert prefix.shape == (0, 3, 3) and (end[0] == carry[0]).all() and (end[1] == carry[1]).all()
    feed(eng, system, xyz[:3])                        # fewer frames than blocks: an empty grid, NaN, status OK
    assert np.isnan(eng.error_estimate(groups, 5)).all() and not np.isnan(eng.error_estimate(groups, 3)).any()
    tu.same_floats(eng.error_estimate(groups, 3), tu.host_errors(rows(eng), groups, 3))

    def refused(call, *words):
        with pytest.raises(abi.GorderHipError) as e:
            call()
        assert e.value.status == abi.ERR_INVALID_ARGUMENT == 100
        text = str(e.value)
        assert any(w in text for w in words), text
    refused(lambda: eng.error_estimate(groups, 1), "n_blocks")
    refused(lambda: eng.timewise_blocks(0), "n_blocks")
    refused(lambda: eng.error_estimate([[0], [system.tables.n_acc]], 5), "slot")
    refused(lambda: eng.error_estimate([[0], [], [1]], 5), "empty")
    refused(lambda: eng.convergence([[0], []]), "empty")
    refused(lambda: eng.convergence([]), "no groups")
    begin, slots, out = np.array([0, 3, 2, 4], np.uint32), np.arange(4, dtype=np.uint32), np.zeros((3, 3), np.float32)
    vp = lambda a: a.ctypes.data
    assert eng.lib.gorder_hip_error_estimate(eng._h, 5, vp(begin), vp(slots), 3, None, None, vp(out)) == 100
    assert b"ascending" in eng.lib.gorder_hip_last_error_message(eng._h)
    tu.same_floats(eng.error_estimate(groups, 3), tu.host_errors(rows(eng), groups, 3))   # a refusal leaves the handle usable
    off = HipEngine(synthetic.cg_membrane(12, leaflets=LEAFLETS_GLOBAL, n_types=3).tables)            # timewise = 0
    feed(off, system, xyz[:4])
    assert off.timewise_rows() == 0
    for call in (lambda: off.error_estimate(groups, 5), lambda: off.timewise_blocks(5), lambda: off.convergence(groups)):
        with pytest.raises(abi.GorderHipError) as e:
            call()
        assert e.value.status == 100 and "timewise" in str(e.value)


@pytest.fixture(scope="module")
def fixtures(built):
    return {"aa": Fixture("pcpepg"), "cg": Fixture("cg"), "ua": Fixture("ua")}


def golden_run(fixtures, kind, leaflets, step=1, batches=3):
    fx = fixtures[kind]
    setup = {"aa": aa_setup, "cg": cg_setup, "ua": ua_setup}[kind]
    tables, labels, midx = setup(fx, leaflets=METHODS["global"] if leaflets else None, timewise=True)
    frames = fx.window(None, None, step)
    eng = HipEngine(tables)
    xyz = np.ascontiguousarray(fx.xyz[frames][:, midx, :])
    fi = np.arange(len(frames)) * step if step > 1 else np.asarray(frames)
    edges = np.linspace(0, len(frames), batches + 1).astype(int)
    for a, b in zip(edges[:-1], edges[1:]):
        eng.submit_host(xyz[a:b], fx.boxes[frames][a:b], fi[a:b])
    return eng, eng.finish(), labels


@pytest.mark.parametrize("kind,leaflets,name", [("aa", False, "aa_order_error"), ("cg", True, "cg_order_error_leaflets"),
                                                ("ua", False, "ua_order_error"), ("ua", True, "ua_order_leaflets_error")])
def test_error_files_of_the_reference_from_the_device_route(fixtures, kind, leaflets, name):
    eng, res, labels = golden_run(fixtures, kind, leaflets)
    groups = st.error_groups(labels, kind)
    errors = dict(zip(map(tuple, groups), eng.error_estimate(groups)))
    tree = (st.results_tree_ua(res, labels, leaflets=leaflets, errors=errors) if kind == "ua"
            else st.results_tree(res, labels, kind, leaflets=leaflets, errors=errors))
    same_items(writers.yaml_text(tree, header="# made here"), golden(name + ".yaml"), skip=1)
    same_items(writers.csv_text(tree), golden(name + ".csv"), sep=",")
    same_tokens(writers.tab_text(tree), golden(name + ".tab"))
    tu.same_floats(np.array(list(errors.values())), tu.host_errors(eng.timewise(eng.timewise_rows()), groups, 5))


@pytest.mark.parametrize("kind,leaflets,step,name", [("aa", False, 1, "aa_order_convergence.xvg"), ("aa", True, 1, "aa_order_leaflets_convergence.xvg"),
                                                     ("aa", False, 5, "aa_order_convergence_s5.xvg"),
                                                     ("cg", True, 1, "cg_order_leaflets_convergence.xvg"), ("cg", False, 5, "cg_order_convergence_s5.xvg"),
                                                     ("ua", False, 1, "ua_order_convergence.xvg"), ("ua", True, 1, "ua_order_leaflets_convergence.xvg")])
def test_convergence_files_of_the_reference_from_the_device_route(fixtures, kind, leaflets, step, name):
    eng, _, labels = golden_run(fixtures, kind, leaflets, step=step, batches=2)
    prefix, _ = eng.convergence(writers.convergence_groups(labels))
    same_tokens(writers.convergence_text(None, labels, kind, leaflets, step=step, prefix=prefix), golden(name))
