"""The two buffers of a submit that grow and KEEP what they hold: the leaflet flag rows (row 0, the assignment carried over
from the batch before) and the per-frame rows (every frame analysed so far).  One run that crosses both growth points in its
second batch, against the oracle."""
import numpy as np
import pytest

from gorder_amd import HipEngine, synthetic
from gorder_amd.abi import LEAFLETS_GLOBAL
from oracle import oracle

pytestmark = pytest.mark.gpu


def test_flag_rows_and_per_frame_rows_grow_with_their_contents(built):
    """Global leaflets every 4th frame, per-frame rows on, 41 frames in two batches.  Frames 0..5: assignment frames 0 and 4,
    three flag rows, room for 12 per-frame rows.  Frames 6..40: frames 6 and 7 read the carried row (the sides of frame 4),
    nine assignment frames make the flag rows grow around it, and 41 frames make the per-frame rows grow with the six
    already there copied over."""
    system = synthetic.aa_membrane(8, leaflets=LEAFLETS_GLOBAL, frequency=4, timewise=True)
    n = 41
    xyz = system.frames(n, seed=21)
    box = system.box9(n)
    eng = HipEngine(system.tables)
    o = oracle.OracleEngine(system.tables, trig=oracle.TRIG_DIRECT, n_threads=2)
    for a, b in ((0, 6), (6, n)):
        fi = np.arange(a, b)
        assert [int(f) for f in fi if f % 4 == 0] == ([0, 4] if a == 0 else list(range(8, 41, 4)))
        eng.submit_host(xyz[a:b], box[a:b], fi)
        o.submit(xyz[a:b], box[a:b], fi)
    got, want = eng.finish(), o.finish()
    assert got.n_frames == want.n_frames == n
    np.testing.assert_array_equal(got.sums, want.sums)
    np.testing.assert_array_equal(got.counts, want.counts)
    gs, gc = eng.timewise(n)
    ws, wc = o.timewise(n)
    np.testing.assert_array_equal(gs, ws)
    np.testing.assert_array_equal(gc, wc)
    flags, frame = eng.leaflets()
    oflags, _, oframe = o.leaflets()
    assert frame == oframe == 40
    np.testing.assert_array_equal(flags, oflags)
    # both leaflets are there in every frame's row, the carried frames 6 and 7 included, and the rows add up to the totals
    assert gc[:, 1].sum(axis=1).min() > 0 and gc[:, 2].sum(axis=1).min() > 0
    np.testing.assert_array_equal(gc.sum(axis=0), got.counts)
    np.testing.assert_array_equal(gs.sum(axis=0), got.sums)
