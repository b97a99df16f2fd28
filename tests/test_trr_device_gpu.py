"""k_trr_unpack (the big-endian f32 / f64 positions of TRR frames made into f32 coordinates on the device) against the
host reader gorder_xtc_next, bit for bit, and the trajectory driver's device route on TRR files against its host route.
The TRR bytes are written here from the format description (tests/trr_files.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from gorder_amd import HipEngine, abi, synthetic, xtc
from gorder_amd.abi import LEAFLETS_GLOBAL, CXtcFrame
from golden_util import GOLDEN, METHODS, Fixture, cg_setup
from test_trajectory_cpu import _write_gro
from trr_files import write_trr

pytestmark = pytest.mark.gpu
SENTINEL = np.uint32(0x7fc5a5a5)        # a NaN no file here holds
WINDOWS = (dict(), dict(begin=2.5, end=12.5, step=2), dict(begin=0.0, step=3))


def tiny_engine():
    mt = abi.MolType(n_molecules=1, bonds=np.array([[[0, 1]]], dtype=np.uint32))
    return HipEngine(abi.Tables(n_atoms=2, molecule_types=[mt]))


def merged(windows):
    """several packed windows as ONE blob and ONE frame table (what a batch of the driver filled across files is)"""
    blob = np.concatenate([w["blob"] for w in windows])
    frames, at = [], 0
    for w in windows:
        fr = w["frames"].copy()
        fr["offset"] += at
        at += w["blob"].size
        frames.append(fr)
    return blob, np.concatenate(frames)


def unpack(engine, blob, frames, n_file, n_stop, slot_of, n_out, pad=4):
    """-> uint32 [F, n_out, 3] as the device wrote it; the output lies `pad` words into a buffer of sentinels that must be
    sentinels still before and behind it"""
    n = len(frames)
    d_blob = torch.from_numpy(blob).cuda()
    d_frames = torch.from_numpy(frames.view(np.uint8).reshape(-1).copy()).cuda()
    d_slot = None if slot_of is None else torch.from_numpy(slot_of).cuda()
    words = n * n_out * 3
    buf = torch.from_numpy(np.full(words + pad + 64, SENTINEL, dtype=np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    engine.xtc_decode(d_blob.data_ptr(), d_blob.numel(), d_frames.data_ptr(), n, n_file, 0 if d_slot is None else d_slot.data_ptr(),
                      n_stop, buf.data_ptr() + 4 * pad, n_out)
    engine.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    assert np.all(got[:pad] == SENTINEL) and np.all(got[pad + words:] == SENTINEL), "written outside the frames"
    return got[pad:pad + words].reshape(n, n_out, 3)


def groups_of(n, rng):
    """none; the leading range; a scattered ascending list with gaps; a permuted list; only the last atom"""
    out = [None]
    if n * 2 // 3 >= 1:
        out.append(np.arange(n * 2 // 3, dtype=np.uint32))
    out.append(np.sort(rng.choice(n, size=max(1, n // 3), replace=False)).astype(np.uint32))
    out.append(rng.permutation(n)[:max(1, n * 3 // 4)].astype(np.uint32))
    out.append(np.array([n - 1], dtype=np.uint32))
    return out


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 257, 1000])
def test_unpack_equals_the_host_reader(built, tmp_path, n, double):
    """5 frames: for n not divisible by 4 the output frames start at 0, 4, 8 and 12 bytes modulo 16 (and, with the output
    one word into its buffer, at the other three phases too)"""
    rng = np.random.default_rng(1000 * n + double)
    xyz = rng.uniform(-50.0, 50.0, size=(5, n, 3))
    xyz = xyz if double else xyz.astype(np.float32)         # doubles that are NOT floats: every one is rounded
    path = str(tmp_path / "t.trr")
    write_trr(path, xyz, np.tile(np.eye(3) * 7.0, (5, 1, 1)), 2.5 * np.arange(5), double=double)
    engine = tiny_engine()
    for group in groups_of(n, rng):
        host = xtc.read_trajectory([path], group=group)[0]
        n_out = n if group is None else len(group)
        assert host.shape == (5, n_out, 3)
        ws = xtc.pack_trajectory([path], group=group, chunk=8)
        assert len(ws) == 1
        w = ws[0]
        for pad in ((4, 1) if group is None or len(group) == n * 2 // 3 else (4,)):
            got = unpack(engine, w["blob"], w["frames"], n, w["n_stop"], w["slot_of"], n_out, pad=pad)
            np.testing.assert_array_equal(got, host.view(np.uint32))
        assert not np.any(host.view(np.uint32) == SENTINEL)           # (so: every slot was written)
        if group is not None and np.array_equal(group, np.arange(len(group))):
            # the leading range without a table (what the driver does for it): one flat stream into a narrower frame
            got = unpack(engine, w["blob"], w["frames"], n, w["n_stop"], None, n_out)
            np.testing.assert_array_equal(got, host.view(np.uint32))


def test_double_precision_edge_values(built, tmp_path):
    """round to nearest even like the host's (float) cast = numpy's astype(float32): halfway cases, results that are f32
    denormals (not flushed), below half the smallest denormal, beyond FLT_MAX, +-0, +-inf, NaN"""
    e = np.float64(2.0) ** np.arange(-160, 130)
    vals = np.concatenate([
        # ties at 1 and their neighbours; FLT_MAX + half an ulp (a tie, to infinity), its neighbour below, FLT_MAX
        [1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 2.0 ** -24 - 2.0 ** -52,
         (2.0 - 2.0 ** -24) * 2.0 ** 127, np.nextafter((2.0 - 2.0 ** -24) * 2.0 ** 127, 0.0), 3.4028234663852886e38,
         # results that are denormals, ties among them, the smallest one, half of it (a tie, to zero), just above, below
         1.3 * 2.0 ** -140, 2.0 ** -149, 1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149, 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -50),
         2.0 ** -151, 2.0 ** -126 * (1 - 2.0 ** -25), 2.0 ** -126 * (1 - 2.0 ** -24), 5e-324, 2.2250738585072014e-308,
         0.0, -0.0, np.inf, -np.inf, np.nan, 1e39, -1e39, 1e300, -1e300],
        e, -e, e * (1 + 2.0 ** -24), e * (1 + 2.0 ** -23 + 2.0 ** -24), -e * (1 + 2.0 ** -24 + 2.0 ** -40)])
    vals = np.concatenate([vals, -vals[:18]])
    vals = np.concatenate([vals, np.zeros((-len(vals)) % 3)])
    n = len(vals) // 3
    xyz = np.stack([vals.reshape(n, 3), vals[::-1].reshape(n, 3)])
    path = str(tmp_path / "edge.trr")
    write_trr(path, xyz, None, [0.0, 1.0], double=True)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        want = xyz.astype(np.float32)
    denormal = (want != 0) & (np.abs(want) < np.float32(2.0 ** -126))
    assert denormal.sum() >= 40 and np.isinf(want).sum() >= 10 and np.isnan(want).sum() == 2     # the cases are in there
    engine = tiny_engine()
    rng = np.random.default_rng(8)
    for group in (None, rng.permutation(n).astype(np.uint32)):
        w = xtc.pack_trajectory([path], group=group)[0]
        got = unpack(engine, w["blob"], w["frames"], n, w["n_stop"], w["slot_of"], n).view(np.float32)
        ref = want if group is None else want[:, group]
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan)
        np.testing.assert_array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan])
        host = xtc.read_trajectory([path], group=group)[0]                 # and the host reader says the same
        np.testing.assert_array_equal(host.view(np.uint32)[~nan], ref.view(np.uint32)[~nan])


def test_single_precision_bits_pass_through(built, tmp_path):
    """denormals, NaN payloads (a signalling one too), signed zeros and infinities of an f32 file arrive bit for bit"""
    bits = np.array([0x00000001, 0x007fffff, 0x80000001, 0x807fffff, 0x00400000, 0x7fc12345, 0x7f800001, 0xffc00001,
                     0xff8abcde, 0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7f7fffff, 0x00800000, 0x3f800001,
                     0x12345678, 0x89abcdef], dtype=np.uint32)
    n = len(bits) // 3
    xyz = np.stack([bits.reshape(n, 3), bits[::-1].reshape(n, 3), np.roll(bits, 5).reshape(n, 3)]).view(np.float32)
    path = str(tmp_path / "bits.trr")
    write_trr(path, xyz, None, [0.0, 1.0, 2.0])
    engine = tiny_engine()
    for group in (None, np.array([4, 0, 5, 2], dtype=np.uint32)):
        w = xtc.pack_trajectory([path], group=group)[0]
        n_out = n if group is None else len(group)
        got = unpack(engine, w["blob"], w["frames"], n, w["n_stop"], w["slot_of"], n_out)
        np.testing.assert_array_equal(got, xyz.view(np.uint32) if group is None else xyz.view(np.uint32)[:, group])


def test_mixed_table(built, tmp_path):
    """3 XTC frames, 3 TRR f32 frames and 2 TRR f64 frames of the same 300 atoms in ONE table and ONE call"""
    rng = np.random.default_rng(12)
    n = 300
    box = np.tile(np.eye(3, dtype=np.float32) * 6.0, (3, 1, 1))
    paths = [str(tmp_path / name) for name in ("a.xtc", "b.trr", "c.trr")]
    xtc.write_trajectory(paths[0], rng.uniform(0, 6, size=(3, n, 3)).astype(np.float32), box, times=[0.0, 1.0, 2.0])
    write_trr(paths[1], rng.uniform(0, 6, size=(3, n, 3)).astype(np.float32), box, [3.0, 4.0, 5.0])
    write_trr(paths[2], rng.uniform(0, 6, size=(2, n, 3)), box[:2], [6.0, 7.0], double=True)
    engine = tiny_engine()
    engine.kernel_time()                                           # switches the timing on
    for group in (None, rng.permutation(n)[:200].astype(np.uint32)):
        host = xtc.read_trajectory(paths, group=group)[0]
        ws = xtc.pack_trajectory(paths, group=group)
        assert [len(w["time"]) for w in ws] == [3, 3, 2]
        blob, frames = merged(ws)
        assert frames["kind"].tolist() == [0, 0, 0, 4, 4, 4, 8, 8]
        n_out = n if group is None else len(group)
        got = unpack(engine, blob, frames, n, ws[0]["n_stop"], ws[0]["slot_of"], n_out)
        np.testing.assert_array_equal(got, host.view(np.uint32))
    assert "k_trr_unpack" in engine.kernel_names()
    assert any(name == "k_trr_unpack" and ms > 0.0 and seg == 2 for name, ms, seg in engine.kernel_groups())
    engine.kernel_time(reset=True)
    w = xtc.pack_trajectory(paths[:1])[0]                           # a table of XTC frames alone queues no k_trr_unpack
    got = unpack(engine, w["blob"], w["frames"], n, n, None, n)
    np.testing.assert_array_equal(got, xtc.read_trajectory(paths[:1])[0].view(np.uint32))
    assert "k_trr_unpack" not in engine.kernel_names()


def same_results(a, b):
    assert a.n_frames == b.n_frames
    np.testing.assert_array_equal(a.sums, b.sums)
    np.testing.assert_array_equal(a.counts, b.counts)


def test_reference_trr_through_the_device_route(built):
    """tests/golden/cg3.trr (the whole CG system with its water, one frame) on the CG tables: the device route is taken,
    nothing is left to the host, and the results are the host route's"""
    cg = Fixture("cg")
    tables, labels, midx = cg_setup(cg, leaflets=METHODS["global"])
    path = os.path.join(GOLDEN, "cg3.trr")
    dev = HipEngine(tables)
    s1 = dev.run_trajectory([path], group=midx, threads=2, device_decode=True)
    assert s1["device_decode"] == 1 and s1["frames_decoded_by_host"] == 0 and s1["n_frames"] == 1
    host = HipEngine(tables)
    s0 = host.run_trajectory([path], group=midx, threads=2, device_decode=False)
    assert s0["device_decode"] == 0 and s0["n_frames"] == 1
    same_results(dev.finish(), host.finish())


N_SOLVENT = 40


def membrane_files(tmp_path, double, solvent_first=False):
    """aa_membrane(8) with global leaflets every 4th frame, 12 frames (t = 2.5 k), 40 solvent atoms behind (or in front of)
    the lipids -> (tables, group, the whole file, [XTC of frames 0..6, TRR of frames 6..11], [TRR of 0..6, XTC of 6..11])"""
    system = synthetic.aa_membrane(n_lipids=8, leaflets=LEAFLETS_GLOBAL, frequency=4)
    n = system.n_atoms
    lipids = system.frames(12, seed=2)
    water = np.random.default_rng(3).uniform(0.0, 8.0, size=(12, N_SOLVENT, 3)).astype(np.float32)
    xyz = np.concatenate([water, lipids] if solvent_first else [lipids, water], axis=1)
    if double:              # doubles that are not floats
        xyz = xyz.astype(np.float64) + np.random.default_rng(4).uniform(-1e-9, 1e-9, size=xyz.shape)
    group = np.arange(n, dtype=np.uint32) + (N_SOLVENT if solvent_first else 0)
    box, times = system.box9(12), 2.5 * np.arange(12)
    whole, a, b = (str(tmp_path / name) for name in ("whole.trr", "a.xtc", "b.trr"))
    write_trr(whole, xyz, box, times, double=double)
    xtc.write_trajectory(a, xyz[:7].astype(np.float32), box[:7], times=times[:7])
    write_trr(b, xyz[6:], box[6:], times[6:], double=double)           # starts with the frame a ends with
    c, d = str(tmp_path / "c.trr"), str(tmp_path / "d.xtc")            # the other order: the run OPENS with TRR batches
    write_trr(c, xyz[:7], box[:7], times[:7], double=double)
    xtc.write_trajectory(d, xyz[6:].astype(np.float32), box[6:], times=times[6:])
    return system.tables, group, whole, [a, b], [c, d]


def both_routes(tables, paths, group, **kw):
    out = []
    for dev in (True, False):
        eng = HipEngine(tables)
        st = eng.run_trajectory(paths, group=group, threads=2, batch_frames=5, device_decode=dev, **kw)
        assert st["device_decode"] == int(dev) and st["frames_decoded_by_host"] == 0
        out.append((st, eng.finish()))
    assert out[0][0]["n_frames"] == out[1][0]["n_frames"]
    same_results(out[0][1], out[1][1])
    return out[0]


@pytest.mark.parametrize("double", [False, True])
def test_driver_windows_and_bytes(built, tmp_path, double):
    tables, group, whole, _, _ = membrane_files(tmp_path, double)
    for kw, frames in zip(WINDOWS, (12, 3, 4)):
        st, res = both_routes(tables, [whole], group, **kw)
        assert st["n_frames"] == frames == res.n_frames
        # What travels per frame: the positions of the analysed atoms as the file holds them, in whole 64-byte pieces and
        # one piece of zeros; the box; the frame's row of the table (the driver counts it for XTC frames too).  Not the
        # solvent behind the lipids.
        block = (len(group) * 3 * (8 if double else 4) + 63) // 64 * 64 + 64
        assert st["bytes_h2d"] == frames * (block + 36 + C.sizeof(CXtcFrame))


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("order", ["xtc_then_trr", "trr_then_xtc"])
def test_driver_concatenation_of_both_formats(built, tmp_path, double, order):
    """In either order.  The part of an XTC block that travels is learned from the decoder's reports: a batch of TRR frames
    alone reports nothing and must teach nothing — a run that opens with TRR batches still leaves no XTC frame to the host
    (both_routes asserts frames_decoded_by_host == 0)."""
    tables, group, _, xtc_first, trr_first = membrane_files(tmp_path, double)
    parts = xtc_first if order == "xtc_then_trr" else trr_first
    for kw, frames in zip(WINDOWS, (12, 3, 4)):
        st, res = both_routes(tables, parts, group, **kw)
        assert st["n_frames"] == frames == res.n_frames


@pytest.mark.parametrize("double", [False, True])
def test_driver_group_behind_the_solvent(built, tmp_path, double):
    """the analysed atoms do not lead the frame: the whole block travels and a slot table places the atoms"""
    tables, group, whole, parts, _ = membrane_files(tmp_path, double, solvent_first=True)
    both_routes(tables, [whole], group)
    both_routes(tables, parts, group, begin=2.5, end=22.5, step=2)


@pytest.mark.parametrize("double", [False, True])
def test_driver_shards(built, tmp_path, double):
    """two shards of 6 frames, leaflets assigned every 4th frame: the second shard starts at frame 6 and primes itself
    with frame 4 — the sums of the shards added are those of the whole run, and of the host route"""
    tables, group, whole, parts, _ = membrane_files(tmp_path, double)
    for paths in ([whole], parts):
        st, want = both_routes(tables, paths, group)
        sums, counts = np.zeros_like(want.sums), np.zeros_like(want.counts)
        for i in range(2):
            eng = HipEngine(tables)
            s = eng.run_trajectory(paths, group=group, threads=2, batch_frames=5, device_decode=True, shard=(i, 2))
            assert s["device_decode"] == 1 and s["n_frames"] == 6 and s["shard_first"] == 6 * i and s["shard_frames_total"] == 12
            r = eng.finish()
            sums += r.sums
            counts += r.counts
        np.testing.assert_array_equal(sums, want.sums)
        np.testing.assert_array_equal(counts, want.counts)


def test_fallback_to_the_host_route(built, tmp_path):
    """a GRO file in the run, or a group that lists an atom twice: the host decodes the whole run, as before"""
    rng = np.random.default_rng(6)
    n = 60
    xyz = np.round(rng.uniform(0.5, 5.5, size=(6, n, 3)), 3).astype(np.float32)
    box = np.tile(np.eye(3, dtype=np.float32) * 6.0, (6, 1, 1))
    trr, gro = str(tmp_path / "a.trr"), str(tmp_path / "b.gro")
    write_trr(trr, xyz[:3], box[:3], [0.0, 1.0, 2.0])
    _write_gro(gro, xyz[3:], [(6.0, 6.0, 6.0)] * 3, [3.0, 4.0, 5.0])
    bonds = np.arange(n, dtype=np.uint32).reshape(1, n // 2, 2)
    tables = abi.Tables(n_atoms=n, molecule_types=[abi.MolType(n_molecules=n // 2, bonds=bonds)])
    group = np.arange(n, dtype=np.uint32)
    twice = group.copy()
    twice[7] = 3                                                    # atom 3 fills two slots
    res = {}
    for name, paths, grp in (("gro", [trr, gro], group), ("twice", [trr], twice), ("plain", [trr], group)):
        for dev in (True, False):
            eng = HipEngine(tables)
            st = eng.run_trajectory(paths, group=grp, threads=2, device_decode=dev)
            assert st["device_decode"] == (1 if dev and name == "plain" else 0)
            assert st["n_frames"] == (6 if name == "gro" else 3)
            res[name, dev] = eng.finish()
        same_results(res[name, True], res[name, False])
    # ... and the right sums: those of the host reader's frames handed over directly
    for name, paths, grp in (("gro", [trr, gro], group), ("twice", [trr], twice), ("plain", [trr], group)):
        x, b, _ = xtc.read_trajectory(paths, group=grp)
        eng = HipEngine(tables)
        eng.submit_host(x, b, np.arange(len(x)))
        same_results(res[name, True], eng.finish())
    np.testing.assert_array_equal(xtc.read_trajectory([trr], group=twice)[0], xyz[:3][:, twice])
