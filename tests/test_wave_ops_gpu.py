"""The device's wave and block reductions (csrc/wave_ops.h, run by gorder_hip_selftest_wave_ops in one workgroup of 64,
256 and 1024 threads) against their literal restatement tests/wave_ops_ref.py: every lane of every primitive, bit for bit.
No tolerance anywhere.  NaN and inputs that hold both zeros are left out of the extrema: fminf / fmaxf do not define which
zero wins, and no caller depends on it."""
import numpy as np
import pytest

import wave_ops_ref as wr
from gorder_amd import abi

pytestmark = pytest.mark.gpu

BLOCKS = (64, 256, 1024)
NAMES = ("f64", "f32", "u32", "finfo")


def check(f64, f32, u32, finfo_empty=False):
    got = abi.selftest_wave_ops(f64, f32, u32, finfo_empty)
    want = wr.selftest_rows(f64, f32, u32, finfo_empty)
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        diff = np.argwhere(wr.bits(g) != wr.bits(w))
        assert len(diff) == 0, f"{name}: first difference at (row, thread) {diff[0]}: device {g[tuple(diff[0])]!r}, helper {w[tuple(diff[0])]!r}"
    return got


@pytest.mark.parametrize("n", BLOCKS)
def test_float_sums_of_mixed_magnitude(n):
    rng = np.random.default_rng(n)
    check(wr.mixed_values(n, np.float64), wr.mixed_values(n, np.float32), rng.integers(0, 1 << 20, size=n, dtype=np.uint32))
    # the f64 scan in its stated domain (integers below 2^40); the f32 values stay away from both zeros
    check(rng.integers(0, 1 << 40, size=n).astype(np.float64), wr.distinct_floats(n, seed=1),
          rng.integers(0, 1 << 20, size=n, dtype=np.uint32))


@pytest.mark.parametrize("n", BLOCKS)
def test_integer_sums_scans_and_or(n):
    f64, f32 = np.arange(n, dtype=np.float64), wr.distinct_floats(n, seed=2)
    for fill in (0, 1, 0xFFFFFFFF):                 # (u32 arithmetic wraps, on the device as in the helper)
        check(f64, f32, np.full(n, fill, dtype=np.uint32))
    for lane in (0, 15, 16, 47, 63):
        u = np.zeros(n, dtype=np.uint32)
        u[n - 64 + lane] = 0x00ABCDEF
        o64, o32, ou, fi = check(f64, f32, u)
        assert (ou[2][n - 64:] == 0x00ABCDEF).all() and (ou[5][n - 64:] == 0x00ABCDEF).all() and (ou[2][:n - 64] == 0).all()


@pytest.mark.parametrize("n", BLOCKS)
def test_extrema_from_every_position(n):
    base, f64, u = wr.distinct_floats(n, seed=n), np.zeros(n), np.zeros(n, dtype=np.uint32)
    n_w = n // 64
    for wave in range(n_w):
        for lane in (0, 15, 16, 31, 32, 63):
            x = base.copy()
            x[64 * wave + lane] = np.float32(-1.0e6)
            x[64 * ((wave + 1) % n_w) + (lane ^ 1)] = np.float32(1.0e6)
            o64, o32, ou, fi = check(f64, x, u)
            assert (o32[7] == np.float32(-1.0e6)).all() and (o32[8] == np.float32(1.0e6)).all()
            assert list(fi[:4]) == [wr.float_key(-1.0e6), wr.float_key(1.0e6), 0, 2]


@pytest.mark.parametrize("n", BLOCKS)
def test_finfo_record(n):
    f64, x = np.zeros(n), wr.distinct_floats(n, seed=3)
    flags = np.zeros(n, dtype=np.uint32)
    o64, o32, ou, fi = check(f64, x, flags, finfo_empty=True)
    assert list(fi) == [0xFFFFFFFF, 0, 0, 2, 0xFFFFFFFF, 0, 0, 2, 0]
    flags[n - 1 - 17] = 3                           # one lane of the last wave only
    o64, o32, ou, fi = check(f64, x, flags, finfo_empty=True)
    assert list(fi) == [0xFFFFFFFF, 0, 3, 2, 0xFFFFFFFF, 0, 1, 2, 3]
    o64, o32, ou, fi = check(f64, x, flags)
    assert list(fi) == [wr.float_key(x.min()), wr.float_key(x.max()), 3, 2, wr.float_key(x.min()), wr.float_key(x.max()), 1, 2, 3]
