"""GROMACS TRR files for the tests of the TRR device route, written from the format description (XDR, big-endian):
frame = {magic 1993, version string "GMX_trn_file", 13 ints: the sizes in bytes of ir, e, box, vir, pres, top, sym, x, v,
f, then natoms, step, nre; t and lambda as reals} + box + positions (+ velocities).  A real is 4 or 8 bytes.  The
values go in as BITS (numpy byte swaps, no arithmetic), so that NaN payloads, denormals and signed zeros arrive as given."""
import struct

import numpy as np

VERSION = b"GMX_trn_file"
HEADER_BYTES = {False: 8 + 4 + len(VERSION) + 52 + 8, True: 8 + 4 + len(VERSION) + 52 + 16}


def _reals(a, double):
    """the big-endian bytes of an array of reals (f32 arrays stay bit for bit in a single-precision file, f64 ones in a
    double-precision file; the other way round is a cast)"""
    a = np.ascontiguousarray(a, dtype=np.float64 if double else np.float32)
    return a.view(np.uint64 if double else np.uint32).astype(">u8" if double else ">u4").tobytes()


def trr_frame(step, t, box, x=None, v=None, double=False, x_size=None):
    """One frame.  box None: box_size = 0.  x None: a frame without positions.  x_size: a positions size for the header
    other than the true one (a corrupt frame)."""
    n = len(x if x is not None else v)
    rs = 8 if double else 4
    sizes = [0, 0, 9 * rs if box is not None else 0, 0, 0, 0, 0, 3 * n * rs if x is not None else 0,
             3 * n * rs if v is not None else 0, 0]
    if x_size is not None:
        sizes[7] = x_size
    out = struct.pack(">ii", 1993, len(VERSION) + 1) + struct.pack(">i", len(VERSION)) + VERSION
    out += struct.pack(">13i", *sizes, n, step, 0)
    out += _reals(np.array([t, 0.0]), double)
    if box is not None:
        out += _reals(np.asarray(box).reshape(9), double)
    for arr in (x, v):
        if arr is not None:
            out += _reals(np.asarray(arr).reshape(-1), double)
    return out


def write_trr(path, xyz, boxes, times, double=False):
    """frames [F, N, 3] (+ boxes [F, 3, 3] or None, times [F]) as one TRR file -> the file offset of every positions block"""
    data, where, at = [], [], 0
    for k in range(len(xyz)):
        box = None if boxes is None else boxes[k]
        where.append(at + HEADER_BYTES[double] + (0 if box is None else 9 * (8 if double else 4)))
        data.append(trr_frame(k, float(times[k]), box, x=xyz[k], double=double))      # (a list: 65 540 frames in a second)
        at += len(data[-1])
    with open(path, "wb") as f:
        f.write(b"".join(data))
    return where
