"""tests/wave_ops_ref.py — the literal restatement of the kernels' two reduction orders (csrc/wave_ops.h) — against itself
and against exact sums, so that a mistake in the helper is found without a device.  On integers every order gives the same
sum; on floats every order lies within the classical bound (n - 1) u sum|x| (1 + O(u)) of the exact sum (math.fsum)."""
import math

import numpy as np
import pytest

import wave_ops_ref as wr

BLOCKS = (64, 256, 1024)


@pytest.mark.parametrize("n", BLOCKS)
def test_integer_sums_scans_and_or_agree_in_every_order(n):
    rng = np.random.default_rng(n)
    u = rng.integers(0, 1 << 20, size=n, dtype=np.uint32)
    w = u.reshape(-1, 64)
    totals = np.repeat(w.sum(axis=1, dtype=np.uint32), 64)
    cums = np.cumsum(w, axis=1, dtype=np.uint32).reshape(-1)
    assert np.array_equal(wr.wave_sum_rows(u), totals)
    assert np.array_equal(wr.wave_sum_bfly(u), totals)
    assert np.array_equal(wr.rows_to_wave(wr.row_sum(u))[63::64], totals[63::64])
    assert np.array_equal(wr.row_sum(u).reshape(-1, 16)[:, 15], u.reshape(-1, 16).sum(axis=1, dtype=np.uint32))
    assert np.array_equal(wr.wave_scan_rows(u), cums)
    assert np.array_equal(wr.wave_scan_shfl(u), cums)
    assert np.array_equal(wr.wave_or_bfly(u), np.repeat(np.bitwise_or.reduce(w, axis=1), 64))
    assert np.array_equal(wr.wave_max_bfly(u), np.repeat(w.max(axis=1), 64))
    assert np.array_equal(wr.block_sum(u.astype(np.float64)), np.full(n, float(u.sum(dtype=np.uint64))))
    d = rng.integers(0, 1 << 40, size=n).astype(np.float64)          # the f64 scan's domain: exact in any order
    assert np.array_equal(wr.wave_scan_rows(d), np.cumsum(d.reshape(-1, 64), axis=1).reshape(-1))


@pytest.mark.parametrize("lane", (0, 15, 16, 47, 63))
def test_single_lane_reaches_the_result(lane):
    u = np.zeros(64, dtype=np.uint32)
    u[lane] = 0x12345
    assert (wr.wave_sum_rows(u) == 0x12345).all() and (wr.wave_sum_bfly(u) == 0x12345).all()
    assert np.array_equal(wr.wave_scan_rows(u), np.where(np.arange(64) >= lane, 0x12345, 0))
    assert np.array_equal(wr.wave_scan_shfl(u), wr.wave_scan_rows(u))
    ones = np.full(64, 0xFFFFFFFF, dtype=np.uint32)
    assert np.array_equal(wr.wave_scan_rows(ones), (np.arange(64, dtype=np.uint64) + 1) * 0xFFFFFFFF & 0xFFFFFFFF)


@pytest.mark.parametrize("dtype,u", ((np.float64, 2.0 ** -53), (np.float32, 2.0 ** -24)))
@pytest.mark.parametrize("n", BLOCKS)
def test_float_sums_within_the_bound_and_the_orders_differ(n, dtype, u):
    x = wr.mixed_values(n, dtype)
    for w in x.reshape(-1, 64):
        exact, bound = math.fsum(map(float, w)), 1.01 * 63 * u * math.fsum(map(abs, map(float, w)))
        rows, bfly = wr.wave_sum_rows(w), wr.wave_sum_bfly(w)
        assert abs(float(rows[0]) - exact) <= bound and abs(float(bfly[0]) - exact) <= bound
        assert len(set(wr.bits(rows))) == 1 and len(set(wr.bits(bfly))) == 1
    # this input tells the orders apart: row order, butterfly and numpy's pairwise sum all round differently
    w = x[:64]
    got = {int(wr.bits(wr.wave_sum_rows(w))[0]), int(wr.bits(wr.wave_sum_bfly(w))[0]), int(wr.bits(np.array([np.sum(w)], dtype=dtype))[0])}
    assert len(got) == 3
    exact_block, bound_block = math.fsum(map(float, x)), 1.01 * (n - 1) * u * math.fsum(map(abs, map(float, x)))
    assert abs(float(wr.block_sum(x)[0]) - exact_block) <= bound_block
    benign = np.random.default_rng(3).random(n).astype(dtype)
    assert abs(float(wr.block_sum(benign)[0]) - math.fsum(map(float, benign))) <= 1.01 * (n - 1) * u * math.fsum(map(float, benign))


@pytest.mark.parametrize("n", BLOCKS)
def test_extrema_from_every_position(n):
    base = wr.distinct_floats(n, seed=n)
    for wave in range(n // 64):
        for lane in (0, 15, 16, 31, 32, 63):
            x = base.copy()
            x[64 * wave + lane] = np.float32(-1.0e6)
            x[64 * ((wave + 1) % (n // 64)) + (lane ^ 1)] = np.float32(1.0e6)
            for fn in (wr.block_min, wr.block_max):
                want = x.min() if fn is wr.block_min else x.max()
                assert (fn(x) == want).all()
            w = x.reshape(-1, 64)
            assert np.array_equal(wr.wave_min_rows(x), np.repeat(w.min(axis=1), 64))
            assert np.array_equal(wr.wave_max_rows(x), np.repeat(w.max(axis=1), 64))
            assert np.array_equal(wr.wave_min_bfly(x), wr.wave_min_rows(x)) and np.array_equal(wr.wave_max_bfly(x), wr.wave_max_rows(x))


def test_finfo_record():
    n = 1024
    x = wr.distinct_floats(n, seed=5)
    flags = np.zeros(n, dtype=np.uint32)
    rec, left = wr.finfo_record(x, x, flags)
    assert list(rec) == [wr.float_key(x.min()), wr.float_key(x.max()), 0, 2] and left == 0
    assert wr.float_key(-1.0) < wr.float_key(-0.5) < wr.float_key(0.5) < wr.float_key(1.0)
    flags[n - 1 - 17] = 2                          # one lane of the last wave
    rec, left = wr.finfo_record(x, x, flags, 1)
    assert list(rec) == [wr.float_key(x.min()), wr.float_key(x.max()), 0, 2] and left == 2
    empty_lo, empty_hi = np.full(n, 3.0e38, dtype=np.float32), np.full(n, -3.0e38, dtype=np.float32)
    rec, _ = wr.finfo_record(empty_lo, empty_hi, flags)
    assert list(rec) == [0xFFFFFFFF, 0, 2, 2]


def test_selftest_rows_shapes():
    o64, o32, ou, fi = wr.selftest_rows(np.arange(64.0), np.arange(64, dtype=np.float32) + 1, np.arange(64, dtype=np.uint32))
    assert o64.shape == (10, 64) and o32.shape == (16, 64) and ou.shape == (9, 64) and fi.shape == (9,)
    assert o64.dtype == np.float64 and o32.dtype == np.float32 and ou.dtype == np.uint32 and fi.dtype == np.uint32
    assert (o64[2] == 2016.0).all() and (o64[5] == 2016.0).all() and (o64[6] == 6048.0).all() and (o64[7] == 47.0).all()
    assert (o32[3] == 1.0).all() and (o32[4] == 64.0).all() and o32[9][0] == 1.0 and o32[9][1] == 1.0 and o32[10][32] == 32.0
