"""The wave and block reductions of gorder_amd/csrc/wave_ops.h, restated literally in numpy: loops over the 64 lanes that
apply the steps in sequence, in the operands' own type (f64, f32 or wrapping u32).  A block is an array of n = 64 w values,
thread t = lane t % 64 of wave t // 64; every function returns what EVERY thread holds afterwards."""
import functools

import numpy as np

ROW_SHR = {1: 0x111, 2: 0x112, 4: 0x114, 8: 0x118}
ROW_BCAST15, ROW_BCAST31 = 0x142, 0x143


def _waves(x):
    x = np.asarray(x)
    assert x.ndim == 1 and len(x) % 64 == 0 and len(x) >= 64
    return x.reshape(-1, 64)


@functools.lru_cache(maxsize=None)
def dpp_sources(ctrl, row_mask):
    """Per lane: the lane `ctrl` names, or -1 where it does not exist or the lane's row of 16 is not in row_mask."""
    src = np.full(64, -1)
    for lane in range(64):
        row, k = divmod(lane, 16)
        if not (row_mask >> row) & 1:
            continue
        if ctrl == ROW_BCAST15:
            src[lane] = 16 * row - 1 if row >= 1 else -1
        elif ctrl == ROW_BCAST31:
            src[lane] = 31 if row >= 2 else -1
        else:
            n = {v: k_ for k_, v in ROW_SHR.items()}[ctrl]
            src[lane] = lane - n if k >= n else -1
    return src


def dpp(x, ctrl, row_mask=0xf, or_self=False):
    """One wave [64]: the value each lane gets from its source lane; 0 (or its own value) where it has none."""
    src = dpp_sources(ctrl, row_mask)
    return np.where(src >= 0, x[src], x if or_self else np.zeros_like(x))


def _per_wave(fn, x):
    with np.errstate(over="ignore"):
        return np.concatenate([fn(w.copy()) for w in _waves(x)])


# ---- row order ---------------------------------------------------------------------------------------
def _row_sum(w):
    for n in (1, 2, 4, 8):
        w = w + dpp(w, ROW_SHR[n])
    return w


def _rows_to_wave(w):
    w = w + dpp(w, ROW_BCAST15, 0xA)
    return w + dpp(w, ROW_BCAST31, 0xC)


def row_sum(x):
    return _per_wave(_row_sum, x)


def rows_to_wave(x):
    return _per_wave(_rows_to_wave, x)


def _lane(w, lane):
    return np.full_like(w, w[lane])


def wave_sum_rows(x):
    return _per_wave(lambda w: _lane(_rows_to_wave(_row_sum(w)), 63), x)


def _extremum_rows(w, op):
    for n in (1, 2, 4, 8):
        w = op(w, dpp(w, ROW_SHR[n], or_self=True))
    w = op(w, dpp(w, ROW_BCAST15, 0xA, or_self=True))
    w = op(w, dpp(w, ROW_BCAST31, 0xC, or_self=True))
    return _lane(w, 63)


def wave_min_rows(x):
    return _per_wave(lambda w: _extremum_rows(w, np.minimum), x)


def wave_max_rows(x):
    return _per_wave(lambda w: _extremum_rows(w, np.maximum), x)


def _scan_rows(w):
    v = _row_sum(w)
    zero = v.dtype.type(0)
    r = np.arange(64) >> 4
    for k, t in enumerate((v[15], v[31], v[47])):    # the totals of the rows before, in this order (0 where the row is not before)
        v = v + np.where(r > k, t, zero)
    return v


def wave_scan_rows(x):
    return _per_wave(_scan_rows, x)


def lane_value(x, lane):
    return _per_wave(lambda w: _lane(w, lane), x)


# ---- butterfly ---------------------------------------------------------------------------------------
def _bfly(w, op):
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = op(w, w[lanes ^ off])
    return w


def wave_sum_bfly(x):
    return _per_wave(lambda w: _bfly(w, np.add), x)


def wave_min_bfly(x):
    return _per_wave(lambda w: _bfly(w, np.minimum), x)


def wave_max_bfly(x):
    return _per_wave(lambda w: _bfly(w, np.maximum), x)


def wave_or_bfly(x):
    return _per_wave(lambda w: _bfly(w, np.bitwise_or), x)


def _scan_shfl(w):
    for off in (1, 2, 4, 8, 16, 32):
        up = w.copy()
        up[off:] = w[:-off]
        w = np.where(np.arange(64) >= off, w + up, w)
    return w


def wave_scan_shfl(x):
    return _per_wave(_scan_shfl, x)


# ---- block -------------------------------------------------------------------------------------------
def block_sum(x):
    totals = wave_sum_bfly(x)[::64]              # what lane 0 of every wave parks
    r = x.dtype.type(0)
    for t in totals:                             # wave order, from zero
        r = r + t
    return np.full_like(x, r)


def _block_extremum(x, wave_fn, op):
    mine = wave_fn(x)
    out = mine.copy()
    for t in mine[::64]:                         # every thread starts from its own wave's result
        out = op(out, t)
    return out


def block_min(x):
    return _block_extremum(x, wave_min_bfly, np.minimum)


def block_max(x):
    return _block_extremum(x, wave_max_bfly, np.maximum)


def float_key(v):
    b = int(np.float32(v).view(np.uint32))
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def finfo_record(zlo, zhi, flags, mask=0xFFFFFFFF):
    """(record [4], flags thread 0 is left with): 16 entries, the waves that are not there hold the identities."""
    lo, hi, fl = wave_min_bfly(zlo)[::64], wave_max_bfly(zhi)[::64], wave_or_bfly(flags)[::64]
    n_w = len(lo)
    a, b, f = lo[0], hi[0], int(fl[0])
    for w in range(1, 16):
        a = np.minimum(a, lo[w] if w < n_w else np.float32(3.0e38))
        b = np.maximum(b, hi[w] if w < n_w else np.float32(-3.0e38))
        f |= int(fl[w]) if w < n_w else 0
    rec = [float_key(a), float_key(b), f & mask, 2] if a <= b else [0xFFFFFFFF, 0, f & mask, 2]
    return np.array(rec, dtype=np.uint32), f


# ---- the rows of gorder_hip_selftest_wave_ops (include/gorder_hip.h) -------------------------------------
def selftest_rows(f64, f32, u32, finfo_empty=False):
    f64 = np.asarray(f64, dtype=np.float64)
    f32 = np.asarray(f32, dtype=np.float32)
    u32 = np.asarray(u32, dtype=np.uint32)
    three = f64 * np.float64(3.0)
    o64 = np.stack([row_sum(f64), rows_to_wave(row_sum(f64)), wave_sum_rows(f64), wave_scan_rows(f64), wave_sum_bfly(f64),
                    block_sum(f64), block_sum(three), lane_value(f64, 47), wave_sum_bfly(f64), wave_sum_bfly(three)])
    o32 = np.stack([row_sum(f32), rows_to_wave(row_sum(f32)), wave_sum_rows(f32), wave_min_rows(f32), wave_max_rows(f32),
                    wave_min_bfly(f32), wave_max_bfly(f32), block_min(f32), block_max(f32),
                    _per_wave(lambda w: dpp(w, ROW_SHR[1], or_self=True), f32), _per_wave(lambda w: dpp(w, ROW_BCAST31, 0xC), f32),
                    lane_value(f32, 47), wave_min_bfly(f32), wave_max_bfly(f32), wave_min_bfly(f32), wave_max_bfly(f32)])
    with np.errstate(over="ignore"):
        as_int = wave_sum_rows(u32.view(np.int32)).view(np.uint32)
    ou = np.stack([row_sum(u32), rows_to_wave(row_sum(u32)), wave_sum_rows(u32), wave_scan_rows(u32), wave_scan_shfl(u32),
                   wave_or_bfly(u32), wave_max_bfly(u32), as_int, lane_value(u32, 47)])
    zlo = np.full_like(f32, 3.0e38) if finfo_empty else f32
    zhi = np.full_like(f32, -3.0e38) if finfo_empty else f32
    rec_all, left = finfo_record(zlo, zhi, u32)
    rec_bit0, _ = finfo_record(zlo, zhi, u32, 1)
    return o64, o32, ou, np.concatenate([rec_all, rec_bit0, np.array([left], dtype=np.uint32)])


# ---- inputs ------------------------------------------------------------------------------------------
MIXED_SEED = 10     # with this seed the first wave's sum differs between row order, butterfly and np.sum, in f64 and in f32


def mixed_values(n, dtype, seed=MIXED_SEED):
    """The first n of 1024 values with magnitudes around 2^60, 1 and 2^-30, random mantissas and signs, shuffled: another
    association of their sum gives another bit pattern (test_wave_ops_cpu.py asserts that it does)."""
    rng = np.random.default_rng(seed)
    mag = np.exp2(rng.choice([60.0, 0.0, -30.0], size=1024)) * (1.0 + rng.random(1024))
    return (mag * rng.choice([-1.0, 1.0], size=1024)).astype(dtype)[:n]


def distinct_floats(n, seed):
    """n distinct finite non-zero floats of both signs, none the smallest or the largest representable."""
    rng = np.random.default_rng(seed)
    v = (rng.permutation(n).astype(np.float32) - np.float32(n / 2 + 0.25)) * np.float32(0.37)
    assert len(np.unique(v)) == n and not (v == 0).any()
    return v


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])
