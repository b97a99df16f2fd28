"""k_xtc_scan + k_xtc_chunks against the independent decoder of tests/xtc_streams.py AND the host decoder on the handcrafted
families: states of the format that no encoder-written file reaches (small atoms of 54..72 bits, runs of 9 and 10,
sizes of 1, joint maxima, launches whose frames mix the forms).  Every comparison is equality of f32 bit patterns."""
import numpy as np
import pytest
import torch

import xtc_streams as xs
from gorder_amd import HipEngine, abi, xtc

pytestmark = pytest.mark.gpu
FAMILY_NAMES = list(xs.FAMILIES)


@pytest.fixture(scope="module")
def engine(built):
    mt = abi.MolType(n_molecules=1, bonds=np.array([[[0, 1]]], dtype=np.uint32))
    return HipEngine(abi.Tables(n_atoms=2, molecule_types=[mt]))


@pytest.fixture(scope="module")
def paths(built, tmp_path_factory):
    return xs.write_files(tmp_path_factory.mktemp("xtc_streams"), xs.all_files() + xs.family("refused"))


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_device_equals_reference_and_host(engine, paths, family):
    """whole frames and every analysed group of the family's files, each file in ONE launch"""
    for f in xs.family(family):
        path, ref = paths[f.name], xs.reference_of(f)[1]
        xs.same_bits(xtc.read_trajectory([path], chunk=130)[0], ref, f.name + ": host")
        xs.same_bits(xs.device_decode(engine, [path], chunk=130), ref, f.name + ": device")
        for group in f.default_groups():
            what = f"{f.name}, group of {group.size} ending at atom {int(group.max())}"
            xs.same_bits(xtc.read_trajectory([path], group=group, chunk=130)[0], ref[:, group], what + ": host")
            xs.same_bits(xs.device_decode(engine, [path], group=group, chunk=130), ref[:, group], what + ": device")


@pytest.mark.parametrize("name", ["mixed_alternating", "mixed_one_wide"])
def test_driver_on_a_launch_of_mixed_forms(built, paths, name):
    """run_trajectory with device_decode against the host route: a bond per pair of atoms, equal sums and counts"""
    f = [f for f in xs.family("mixed_launch") if f.name == name][0]
    bonds = np.arange(f.natoms, dtype=np.uint32).reshape(1, f.natoms // 2, 2)
    tables = abi.Tables(n_atoms=f.natoms, molecule_types=[abi.MolType(n_molecules=f.natoms // 2, bonds=bonds)])
    res = {}
    for dev in (False, True):
        eng = HipEngine(tables)
        st = eng.run_trajectory([paths[name]], threads=2, device_decode=dev)
        assert st["n_frames"] == len(f.frames) and st["device_decode"] == int(dev)
        if dev:
            assert st["frames_decoded_by_host"] == 0
        res[dev] = eng.finish()
    np.testing.assert_array_equal(res[False].sums, res[True].sums)
    np.testing.assert_array_equal(res[False].counts, res[True].counts)
    # (two empty results would be equal too: the samples are there — sums are i64 ticks, there is no NaN to hide in)
    assert res[True].n_frames == len(f.frames) and int(np.asarray(res[True].counts).sum()) > 0
    assert np.asarray(res[True].sums).dtype == np.int64 and np.asarray(res[True].sums).any()


@pytest.mark.parametrize("index", range(4))
def test_refused_frame_is_named_and_the_others_are_decoded(built, paths, index):
    """a step of smallidx to 8 and to 73, a run past the last atom, a block that ends inside an atom — in the middle
    frame of five: GORDER_ERR_TRAJECTORY_FORMAT names it, the four others equal the reference, and the rows before and
    behind the launch's output stay as they were (what the refused frame's own rows hold is not asserted)"""
    f = xs.family("refused")[index]
    windows = xtc.pack_trajectory([paths[f.name]], chunk=8)
    assert len(windows) == 1 and len(windows[0]["time"]) == 5
    w, n, na = windows[0], 5, f.natoms
    mt = abi.MolType(n_molecules=1, bonds=np.array([[[0, 1]]], dtype=np.uint32))
    eng = HipEngine(abi.Tables(n_atoms=2, molecule_types=[mt]))
    blob = torch.from_numpy(w["blob"]).cuda()
    frames = torch.from_numpy(w["frames"].view(np.uint8).reshape(-1).copy()).cuda()
    out = torch.full((n + 2, na, 3), float("nan"), dtype=torch.float32, device="cuda")       # a guard row on either side
    torch.cuda.synchronize()
    eng.xtc_decode(blob.data_ptr(), blob.numel(), frames.data_ptr(), n, na, 0, na, out[1].data_ptr(), na)
    with pytest.raises(abi.GorderHipError) as ei:
        eng.synchronize()
    assert ei.value.status == abi.ERR_TRAJECTORY_FORMAT
    assert "frame 2" in str(ei.value)
    got = out.cpu().numpy()
    assert np.isnan(got[0]).all() and np.isnan(got[n + 1]).all()
    for k in (0, 1, 3, 4):
        xs.same_bits(got[1 + k], xs.reference_decode(f.frames[k])[1], f"{f.name} frame {k}")
