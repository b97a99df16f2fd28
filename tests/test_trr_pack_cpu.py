"""gorder_xtc_pack_window on TRR readers (host half of the TRR device route): the frames it selects, their boxes and
times are those of gorder_xtc_read_window; of every frame exactly the leading gorder_xtc_n_atoms_needed atoms of the
positions block lie in the blob, as they are in the file.  No GPU: the unpacking is compared in
tests/test_trr_device_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from gorder_amd import xtc
from gorder_amd.abi import CXtcFrame
from test_trajectory_cpu import _trr_frame
from trr_files import HEADER_BYTES, trr_frame

HERE = os.path.dirname(os.path.abspath(__file__))
N = 37
WINDOWS = (dict(), dict(begin=2.5, end=12.5, step=2), dict(begin=0.0, step=3))
GROUPS = (None, list(range(20)), [3, 5, 30], [36])


def make_file(path, double, first=0, last=7, rng_seed=5):
    """frames first..last-1 of SEVEN frames of 37 atoms (times 2.5 k); behind the file's first frame lies a frame that holds
    velocities only (not a frame), frame 4 has no box -> (positions [7, N, 3] f32, file offsets of the positions blocks)"""
    rng = np.random.default_rng(rng_seed)
    xyz = rng.uniform(-3.0, 9.0, size=(7, N, 3)).astype(np.float32)
    vel = rng.normal(size=(N, 3)).astype(np.float32)
    box = np.diag([5.0, 6.0, 7.0]).astype(np.float32)
    data, where = b"", {}
    rs = 8 if double else 4
    for k in range(first, last):
        b = None if k == 4 else box
        where[k] = len(data) + HEADER_BYTES[double] + (0 if b is None else 9 * rs)
        data += trr_frame(10 * k, 2.5 * k, b, x=xyz[k], double=double)
        if k == first:
            data += trr_frame(10 * k + 5, 2.5 * k + 1.0, box, x=None, v=vel, double=double)
    with open(path, "wb") as f:
        f.write(data)
    return xyz, where


def test_the_writer_here_writes_what_the_reader_test_writes():
    rng = np.random.default_rng(1)
    x, v = rng.uniform(0, 5, (N, 3)).astype(np.float32), rng.normal(size=(N, 3)).astype(np.float32)
    box = np.diag([5.0, 6.0, 7.0])
    for double in (False, True):
        assert trr_frame(3, 7.5, box, x=x, v=v, double=double) == _trr_frame(3, 7.5, box, x=x, v=v, double=double)
        assert trr_frame(3, 7.5, None, x=None, v=v, double=double) == _trr_frame(3, 7.5, None, x=None, v=v, double=double)


@pytest.mark.parametrize("double", [False, True])
def test_pack_selects_what_read_selects(built, tmp_path, double):
    whole = str(tmp_path / "whole.trr")
    make_file(whole, double)
    a, b = str(tmp_path / "a.trr"), str(tmp_path / "b.trr")
    make_file(a, double, 0, 4)
    make_file(b, double, 3, 7)            # starts with the frame a ends with: dropped
    for paths in ([whole], [a, b]):
        for kw in WINDOWS:
            x, bx, t = xtc.read_trajectory(paths, **kw)
            assert len(t) == {1: 7, 2: 3, 3: 3}[kw.get("step", 1)]
            for chunk in (64, 2):
                ws = xtc.pack_trajectory(paths, chunk=chunk, threads=3, **kw)
                np.testing.assert_array_equal(np.concatenate([w["time"] for w in ws]), t)
                np.testing.assert_array_equal(np.concatenate([w["box"] for w in ws]).view(np.uint32), bx.view(np.uint32))
            # `state` and `last_time` behind every file: those of gorder_xtc_read_window
            assert final_state(paths, kw, pack=True) == final_state(paths, kw, pack=False)
    assert xtc.read_trajectory([whole])[1][4].tolist() == np.zeros((3, 3)).tolist()       # box_size == 0: nine zeros


def final_state(paths, kw, pack):
    lib = xtc._lib()
    state, last = C.c_uint64(0), C.c_double(float("-inf"))
    seen = []
    for path in paths:
        r = C.c_void_p()
        assert lib.gorder_xtc_open(path.encode(), None, 0, C.byref(r)) == 0
        blob, frames, used = np.empty(1 << 16, np.uint8), (CXtcFrame * 8)(), C.c_uint64(0)
        x, box, t = np.empty((8, N, 3), np.float32), np.empty((8, 9), np.float32), np.empty(8, np.float32)
        while True:
            if pack:
                got = lib.gorder_xtc_pack_window(r, kw.get("begin", 0.0), kw.get("end", -1.0), kw.get("step", 1), C.byref(state),
                                                 C.byref(last), blob.ctypes.data, blob.size, C.byref(used),
                                                 C.cast(frames, C.c_void_p), box.ctypes.data, t.ctypes.data, 8, 2)
            else:
                got = lib.gorder_xtc_read_window(r, kw.get("begin", 0.0), kw.get("end", -1.0), kw.get("step", 1), C.byref(state),
                                                 C.byref(last), x.ctypes.data, box.ctypes.data, t.ctypes.data, 8)
            assert got >= 0
            if got == 0:
                break
        lib.gorder_xtc_close(r)
        seen.append((state.value, last.value))
    return seen


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("group", GROUPS)
def test_table_fields_and_blob_bytes(built, tmp_path, double, group):
    path = str(tmp_path / "t.trr")
    _, where = make_file(path, double)
    raw = open(path, "rb").read()
    rs = 8 if double else 4
    n_stop = N if group is None else max(group) + 1
    grp = None if group is None else np.array(group, dtype=np.uint32)
    ws = xtc.pack_trajectory([path], group=grp, chunk=3, threads=2)
    assert sum(len(w["time"]) for w in ws) == 7
    k = 0
    for w in ws:
        assert w["n_stop"] == n_stop and w["n_atoms_file"] == N
        for f in w["frames"]:
            off, nb = int(f["offset"]), int(f["n_bytes"])
            assert off % 64 == 0
            assert int(f["kind"]) == (8 if double else 4)
            assert nb == n_stop * 3 * rs
            assert bytes(w["blob"][off:off + nb]) == raw[where[k]:where[k] + nb]
            end = off + (nb + 63) // 64 * 64 + 64
            assert end <= w["blob"].size and not w["blob"][off + nb:end].any()
            # the XTC-only fields are zero
            assert int(f["recip1"]) == int(f["recip2"]) == 0 and not f["minint"].any() and not f["sizeint"].any()
            assert int(f["smallidx"]) == 0 and float(f["inv_precision"]) == 0.0 and int(f["bitsize"]) == int(f["bitsizeint"]) == 0
            k += 1
        ends = w["frames"]["offset"] + (w["frames"]["n_bytes"].astype(np.uint64) + 63) // 64 * 64 + 64
        assert np.all(ends[:-1] <= w["frames"]["offset"][1:])


def open_and_pack_args(path, capacity_frames=8):
    lib = xtc._lib()
    r = C.c_void_p()
    assert lib.gorder_xtc_open(path.encode(), None, 0, C.byref(r)) == 0
    keep = dict(state=C.c_uint64(0), last=C.c_double(float("-inf")), used=C.c_uint64(0), blob=np.empty(1 << 16, np.uint8),
                frames=(CXtcFrame * capacity_frames)(), box=np.empty((capacity_frames, 9), np.float32),
                t=np.empty(capacity_frames, np.float32))
    args = lambda cap, prefix=None: (r, 0.0, -1.0, 1, C.byref(keep["state"]), C.byref(keep["last"]), keep["blob"].ctypes.data, cap,
                                     C.byref(keep["used"]), C.cast(keep["frames"], C.c_void_p), keep["box"].ctypes.data,
                                     keep["t"].ctypes.data, capacity_frames, 2)
    return lib, r, keep, args


@pytest.mark.parametrize("double", [False, True])
def test_blob_capacity(built, tmp_path, double):
    path = str(tmp_path / "t.trr")
    make_file(path, double)
    per_frame = (N * 3 * (8 if double else 4) + 63) // 64 * 64 + 64
    lib, r, keep, args = open_and_pack_args(path)
    # below one frame: nothing happens
    assert lib.gorder_xtc_pack_window(*args(per_frame - 1)) == -4                 # GORDER_XTC_ERR_NO_SPACE
    assert keep["state"].value == 0 and keep["last"].value == float("-inf")
    # room for two frames: two, then the third opens the next call
    assert lib.gorder_xtc_pack_window(*args(2 * per_frame + per_frame // 2)) == 2
    assert keep["used"].value == 2 * per_frame
    np.testing.assert_array_equal(keep["t"][:2], [0.0, 2.5])
    assert keep["state"].value == 2 and keep["last"].value == 2.5
    assert lib.gorder_xtc_pack_window(*args(1 << 16)) == 5
    np.testing.assert_array_equal(keep["t"][:5], [5.0, 7.5, 10.0, 12.5, 15.0])
    assert lib.gorder_xtc_pack_window(*args(1 << 16)) == 0
    lib.gorder_xtc_close(r)


@pytest.mark.parametrize("double", [False, True])
def test_format_errors(built, tmp_path, double):
    path = str(tmp_path / "t.trr")
    xyz, where = make_file(path, double)
    raw = open(path, "rb").read()
    rs = 8 if double else 4
    cut = str(tmp_path / "cut.trr")
    open(cut, "wb").write(raw[:where[5] + N * 3 * rs // 2])              # the file ends inside frame 5's positions
    with pytest.raises(IOError, match="pack error -2"):
        xtc.pack_trajectory([cut])
    # ... found before anything is copied, also when only a LEADING part of that block would travel
    with pytest.raises(IOError, match="pack error -2"):
        xtc.pack_trajectory([cut], group=np.array([0, 1], dtype=np.uint32))
    box = np.diag([5.0, 6.0, 7.0])
    bad = str(tmp_path / "bad.trr")
    open(bad, "wb").write(trr_frame(0, 0.0, box, x=xyz[0], double=double) +
                          trr_frame(1, 2.5, box, x=xyz[1], double=double, x_size=(N - 1) * 3 * rs) +
                          trr_frame(2, 5.0, box, x=xyz[2], double=double))
    with pytest.raises(IOError, match="pack error -2"):
        xtc.pack_trajectory([bad])
    with pytest.raises(IOError, match="read error -2"):                 # as the host decoder says
        xtc.read_trajectory([bad])


@pytest.mark.parametrize("double", [False, True])
def test_read_at_probe_and_can_pack(built, tmp_path, double):
    path = str(tmp_path / "t.trr")
    make_file(path, double)
    group = np.array([30, 3, 5], dtype=np.uint32)
    host = xtc.read_trajectory([path], group=group)
    ws = xtc.pack_trajectory([path], group=group, chunk=3, file_pos=True)
    pos = np.concatenate([w["file_pos"] for w in ws])
    assert len(pos) == 7 and np.all(np.diff(pos) > 0)
    for k in (6, 0, 4, 1):            # in any order
        x, b = xtc.read_at(path, int(pos[k]), group=group)
        np.testing.assert_array_equal(x.view(np.uint32), host[0][k].view(np.uint32))
        np.testing.assert_array_equal(b, host[1][k])
    # `prefix_q16` is ignored: the same table and bytes whatever part is asked for
    lib = xtc._lib()
    r = C.c_void_p()
    assert lib.gorder_xtc_open(path.encode(), None, 0, C.byref(r)) == 0
    state, last, used = C.c_uint64(0), C.c_double(float("-inf")), C.c_uint64(0)
    blob, frames = np.zeros(1 << 16, np.uint8), (CXtcFrame * 8)()
    box, t = np.empty((8, 9), np.float32), np.empty(8, np.float32)
    assert lib.gorder_xtc_pack_window_ex(r, 0.0, -1.0, 1, C.byref(state), C.byref(last), blob.ctypes.data, blob.size, C.byref(used),
                                         C.cast(frames, C.c_void_p), box.ctypes.data, t.ctypes.data, 8, 1, None, 1000, None) == 7
    lib.gorder_xtc_close(r)
    fr = np.frombuffer(frames, dtype=np.dtype(CXtcFrame))[:7]
    whole = xtc.pack_trajectory([path], chunk=8)[0]
    assert np.all(fr["kind"] == (8 if double else 4)) and np.array_equal(fr["n_bytes"], whole["frames"]["n_bytes"])
    assert bytes(blob[:used.value]) == bytes(whole["blob"])

    p = xtc.probe_format(path)
    rs = 8 if double else 4
    assert p["format"] == xtc.FORMAT_TRR and p["n_atoms"] == N and p["file_bytes"] == os.path.getsize(path)
    assert p["first_frame_bytes"] == HEADER_BYTES[double] + N * 3 * rs
    # a file whose FIRST frame holds no positions: the first frame that has some
    vfirst = str(tmp_path / "v.trr")
    vel = np.ones((N, 3), np.float32)
    open(vfirst, "wb").write(trr_frame(0, 0.0, np.eye(3), x=None, v=vel, double=double) + open(path, "rb").read())
    assert xtc.probe_format(vfirst)["first_frame_bytes"] == HEADER_BYTES[double] + N * 3 * rs
    assert lib.gorder_xtc_probe(path.encode(), None, None, None) == 0          # "1 = XTC" is what callers depend on
    cg3 = os.path.join(HERE, "golden", "cg3.xtc")
    px = xtc.probe_format(cg3)
    assert px["format"] == xtc.FORMAT_XTC and px["n_atoms"] == 16769 and 0 < px["first_frame_bytes"] <= px["file_bytes"]
    gro = str(tmp_path / "one.gro")
    with open(gro, "w") as f:
        f.write("one atom t= 0.00000 step= 0\n    1\n    1POPC    C1    1   1.000   2.000   3.000\n   5.00000   5.00000   5.00000\n")
    assert xtc.probe_format(gro)["format"] == xtc.FORMAT_OTHER and xtc.probe_format(gro)["n_atoms"] == 0
    assert [xtc.can_pack(q) for q in (cg3, path, gro)] == [True, True, False]
    with pytest.raises(IOError, match="neither"):
        xtc.pack_trajectory([gro])
    assert xtc.probe_format(os.path.join(HERE, "golden", "cg3.trr"))["format"] == xtc.FORMAT_TRR


def test_device_rounding_equals_the_host_cast(tmp_path):
    """trr_f64_bits_to_f32_bits (gorder_amd/csrc/trr_round.h: what k_trr_unpack does to a double) against the host's
    `(float)` cast, on the CPU: tools/trr_round_check.cpp built and run (edge values, every exponent of the f32 range with
    halfway mantissas, two million random patterns)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "trr_round_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "..", "tools", "trr_round_check.cpp")])
    res = subprocess.run([exe, "2"], capture_output=True, text=True)
    assert res.returncode == 0 and " 0 differ" in res.stdout, res.stdout[-2000:]
