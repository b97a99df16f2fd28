"""The host XTC decoder (gorder_xtc_next, xtc_reader.cpp) against an independent one (tests/xtc_streams.py) on handcrafted
streams that visit the states of the format no encoder-written file reaches: every comparison is equality of integers
or of f32 bit patterns.  The reference decoder is itself pinned to three GROMACS-written files, to the builder (what
was put in comes out), and shown to be sensitive: four planted mutants of it each turn a named family red."""
import os
import subprocess

import numpy as np
import pytest

import xtc_streams as xs
from gorder_amd import xtc
from golden_util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY_NAMES = list(xs.FAMILIES)


@pytest.fixture(scope="module")
def paths(built, tmp_path_factory):
    return xs.write_files(tmp_path_factory.mktemp("xtc_streams"), xs.all_files() + xs.family("refused"))


@pytest.mark.parametrize("name", ["cg3.xtc", "pcpepg4.xtc", "multiple_resid_same_name.xtc"])
def test_reference_decoder_on_gromacs_written_files(built, name):
    """files of a writer that is not ours: whole frames and a scattered group"""
    path = os.path.join(GOLDEN, name)
    ref = np.stack([d[1] for d in xs.decode_file(open(path, "rb").read())])
    host = xtc.read_trajectory([path])[0]
    assert host.shape[0] >= 1
    xs.same_bits(host, ref)
    n = host.shape[1]
    group = np.unique(np.random.default_rng(4).integers(0, n, size=max(3, n // 7))).astype(np.uint32)[::-1].copy()
    xs.same_bits(xtc.read_trajectory([path], group=group)[0], ref[:, group])


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_builder_and_reference_agree_and_the_family_reaches_its_states(family):
    for f in xs.family(family):
        ints, xyz, traces = xs.reference_of(f)
        np.testing.assert_array_equal(ints, np.array(f.expected, dtype=np.int64))
        assert ints.shape == (len(f.frames), f.natoms, 3) and len(f.frames) <= 130
        got = xs.reached(traces)
        for key, claim in f.claims.items():
            assert claim <= got[key], (f.name, key, sorted(claim - got[key]))


def test_values_reach_the_corners_of_the_box():
    """atoms all zero, all size - 1 (the joint maximum of the mixed-radix number), size - 1 in one dimension at a time"""
    for f in xs.family("values"):
        ints = xs.reference_of(f)[0]
        for k, chosen in enumerate(f.chosen):
            lo = np.array(chosen["minint"], np.int64)
            hi = lo + np.array(chosen["sizeint"], np.int64) - 1
            rows = {tuple(r) for r in ints[k]}
            assert tuple(lo) in rows and tuple(hi) in rows, (f.name, k)
            for c in range(3):
                one = lo.copy()
                one[c] = hi[c]
                assert tuple(one) in rows, (f.name, k, c)
    f = xs.family("values")[2]
    ints = xs.reference_of(f)[0]
    assert ints.min() == xs.INT_MIN and ints.max() == xs.INT_MAX - 1


def test_small_atoms_reach_their_extremes_in_all_three_dimensions():
    """(0, 0, 0), (magic - 1,) * 3 — the joint maximum, all ones at 72 bits — and (magic / 2,) * 3 at every smallidx
    where the bounding box has room for an offset of magic / 2: everywhere under the wide fields; up to 69 under the
    67-bit atom (edges of 5.3 million steps); up to 55 under the 53-bit cube (edges of 185 000 steps >= magic[55] / 2),
    which is every width at which the simple loop divides a small atom in f64, magic[53]^3 - 1 < 2^53 included; up
    to 17 under the 53-bit box whose third edge is 31 steps (>= magic[17] / 2)"""
    simple, wide, fields, cube = xs.family("small_widths")
    for got in xs.small_extremes(fields):
        assert got == set(range(xs.FIRST_IDX, xs.LAST_IDX))
    for got in xs.small_extremes(wide):
        assert got >= set(range(xs.FIRST_IDX, 70))
    for got in xs.small_extremes(cube):
        assert got >= set(range(xs.FIRST_IDX, 56))
    for got in xs.small_extremes(simple):
        assert got >= set(range(xs.FIRST_IDX, 18))
    assert xs.MAGIC[53] ** 3 - 1 < 2 ** 53 <= xs.MAGIC[54] ** 3


def test_checkpoints_fall_on_every_residue_and_chunks_reach_266_atoms():
    """the first group boundary at or behind 256 c — where k_xtc_scan puts checkpoint c — lies 0..8 atoms behind it in
    the files of 9-atom groups, exactly on it included; groups of 11 give chunks of 265 and 266 atoms"""
    def chunks(trace, natoms):
        starts = [before for (_, before, _, _, _, _) in trace] + [natoms]
        cps = [min(b for b in starts if b >= 256 * c) for c in range((natoms + 255) // 256)] + [natoms]
        return cps
    nine, eleven, _ = xs.family("checkpoints")
    behind = {(c, cp - 256 * c) for trace in xs.reference_of(nine)[2] for c, cp in enumerate(chunks(trace, nine.natoms)[:-1])}
    assert behind >= {(c, r) for c in (1, 2, 3) for r in range(9)}
    lengths = {b - a for trace in xs.reference_of(eleven)[2] for a, b in zip(chunks(trace, eleven.natoms), chunks(trace, eleven.natoms)[1:])}
    assert {265, 266} <= lengths and max(lengths) == 266


def test_the_stretches_of_run_8_span_a_reload_of_the_scan_window():
    """k_xtc_scan keeps 8 KB of the stream in LDS and looks 63 groups ahead: a stretch that is longer than what is
    left of the window behind its first step makes it load again inside the stretch"""
    f = [f for f in xs.family("runs") if f.name == "runs_stretch8"][0]
    spans = []
    for trace in xs.reference_of(f)[2]:
        start = None
        for k, (bit, _, width, r5, smallidx, run) in enumerate(trace):
            if r5 is None and run == 24 and start is None:
                start = bit
            if r5 is not None and start is not None:
                spans.append((bit - start) // 8 + 63 * (width + 1 + 8 * smallidx) // 8)
                start = None
    assert max(spans) > 8192 + 64


def test_small_offsets_cross_int_max_on_the_way():
    """d + prev - smallnum with prev close to INT_MAX: the sum passes INT_MAX before smallnum comes off (the host adds
    in uint32_t; the sanitizer run below would name a signed overflow)"""
    crossed = 0
    for f in xs.family("values")[2:] + xs.family("small_widths")[2:3]:
        for trace, ints in zip(xs.reference_of(f)[2], xs.reference_of(f)[0]):
            for (_, before, _, _, smallidx, run) in trace:
                # the run's first small atom (it precedes the full atom): d + prev = atom + smallnum
                if run and ints[before].max() + xs.MAGIC[smallidx] // 2 > xs.INT_MAX:
                    crossed += 1
    assert crossed > 0


@pytest.mark.parametrize("family", FAMILY_NAMES)
@pytest.mark.parametrize("threads", [1, 4])
def test_host_decoder_equals_the_reference(paths, family, threads):
    for f in xs.family(family):
        ref = xs.reference_of(f)[1]
        xs.same_bits(xtc.read_trajectory([paths[f.name]], threads=threads, chunk=130)[0], ref)
        for group in f.default_groups():
            xs.same_bits(xtc.read_trajectory([paths[f.name]], group=group, threads=threads, chunk=130)[0], ref[:, group])


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_frame_table_holds_what_the_builder_chose(paths, family):
    for f in xs.family(family):
        windows = xtc.pack_trajectory([paths[f.name]], chunk=130)
        assert len(windows) == 1
        table = windows[0]["frames"]
        assert len(table) == len(f.frames)
        for row, chosen in zip(table, f.chosen):
            assert int(row["bitsize"]) == chosen["bitsize"] and int(row["bitsizeint"]) == chosen["bitsizeint"]
            assert [int(s) for s in row["sizeint"]] == chosen["sizeint"] and int(row["smallidx"]) == chosen["smallidx"]
            assert [int(m) for m in row["minint"]] == chosen["minint"]
            assert np.float32(row["inv_precision"]) == np.float32(1) / np.float32(chosen["precision"])


def test_refused_streams_are_io_errors(paths):
    for f in xs.family("refused"):
        valid = {}
        for k, frame in enumerate(f.frames):
            if k == 2:
                with pytest.raises(xs.Refused):
                    xs.reference_decode(frame)
            else:
                valid[k] = xs.reference_decode(frame)[1]
        for threads in (1, 4):
            with pytest.raises(IOError):
                xtc.read_trajectory([paths[f.name]], threads=threads)
        xs.same_bits(xtc.read_trajectory([paths[f.name]], end=1.0)[0], np.stack([valid[0], valid[1]]))


@pytest.mark.parametrize("mutant,family", [("no swap", "runs"), ("unflagged resets run", "runs"),
                                           ("smallnum after step", "small_widths"), ("chunks msb first", "values")])
def test_planted_mutants_of_the_reference_are_caught(mutant, family):
    """the family named turns red: the mutant decodes other integers than the builder put in, or refuses the stream"""
    caught = 0
    for f in xs.family(family):
        for frame, want in zip(f.frames, f.expected):
            try:
                ints = xs.reference_decode(frame, mutant)[0]
            except xs.Refused:
                caught += 1
                continue
            caught += int(not np.array_equal(ints, np.array(want, dtype=np.int64)))
    assert caught > 0


def checksums(x):
    u = np.ascontiguousarray(x).view(np.uint32).reshape(-1).astype(np.uint64)
    return int(u.sum(dtype=np.uint64)), int((u * np.arange(1, u.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def test_host_decoder_is_clean_under_sanitizers_on_every_family(paths, tmp_path):
    """tests/cabi/xtc_streams_sanitize.cpp + xtc_reader.cpp under address,undefined: no report, and the checksums of
    what it decoded are the reference's"""
    exe = str(tmp_path / "xtc_streams_sanitize")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-pthread",
           f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "cabi", "xtc_streams_sanitize.cpp"),
           os.path.join(ROOT, "gorder_amd", "csrc", "xtc_reader.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    files = xs.all_files() + xs.family("refused")
    res = subprocess.run([exe] + [paths[f.name] for f in files], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr[:4000]
    lines = iter(res.stdout.splitlines())
    for f in files:
        refused = f.name.startswith("refused")
        for k, frame in enumerate(f.frames):
            words = next(lines).split()
            assert words[:2] == [paths[f.name], str(k)]
            if refused and k == 2:
                assert words[2:] == ["refused"]
                continue
            xyz = xs.reference_decode(frame)[1] if refused else xs.reference_of(f)[1][k]
            assert [int(w) for w in words[2:]] == list(checksums(xyz) + checksums(xyz[::3])), (f.name, k)
    assert next(lines, None) is None
