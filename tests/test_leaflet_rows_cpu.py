"""The assignment rows of a batch (gorder_amd/csrc/leaflet_rows.h) without a GPU: a stand-alone program under the address and
undefined-behaviour sanitizers prints plan_assignment_rows for a full sweep of its inputs (tests/cabi/leaflet_rows.cpp); the
expected values here restate the loop as it stood in gorder_hip_submit_device before the header existed (commit 4c5c830,
gorder_amd/csrc/gorder_hip.hip lines 2157-2183, and should_assign, lines 464-466 — the numbers in the comments), not the
header.  The two ways that loop refused a batch (GORDER_ERR_LEAFLETS_NOT_PRIMED with either message) are part of what is
compared, and so is what it had done to the handle's cl_is0 by then."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, GLOBAL, LOCAL, INDIVIDUAL, MANUAL, SPHERICAL, CLUSTERING = range(7)     # gorder_leaflets_method_t
OK, NO_CLUSTERS, NOT_PRIMED = range(3)                                          # gorder::LeafletRowsStatus
IRREGULAR = [5, 0, 2, 3, 9, 6, 6]


def should_assign(frequency, frame):                                            # 464-466
    return frame == 0 if frequency == 0 else frame % frequency == 0


def parent_rows(method, frequency, have_assignment, cl_have_carry, frames, cl_is0, assignment_frame):
    """(status, last_assign_frame, arow, aframes, cl_is0) of the parent's loop; cl_is0 and assignment_frame: the handle's."""
    cl_is0 = list(cl_is0)
    last = assignment_frame                                                     # 2158
    arow, aframes = [0] * len(frames), []                                       # 2157, 2160
    cur, have = 0, have_assignment                                              # 2161-2162
    for f, frame in enumerate(frames):                                          # 2166
        if method != MANUAL and should_assign(frequency, frame):                # 2167
            if method == CLUSTERING:                                            # 2168
                if not aframes:                                                 # 2170
                    cl_is0 = []
                if not aframes and frame != 0 and not cl_have_carry:            # 2171-2172: "clustering: no clusters of an earlier ..."
                    return NO_CLUSTERS, assignment_frame, [], [], cl_is0
                cl_is0.append(1 if frame == 0 else 0)                           # 2173
            aframes.append(f)                                                   # 2175
            cur = len(aframes)                                                  # 2176
            have = True                                                         # 2177
            last = frame                                                        # 2178
        if not have:                                                            # 2180: "no leaflet assignment for the first frame"
            return NOT_PRIMED, assignment_frame, [], [], cl_is0
        arow[f] = cur                                                           # 2181
    return OK, last, arow, aframes, cl_is0


def batches():
    out = [[first + f * stride for f in range(n)] for n in range(6) for first in (0, 1, 4) for stride in (1, 2)]
    return out + [IRREGULAR]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("leaflet_rows") / "leaflet_rows")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", f"-I{os.path.join(ROOT, 'gorder_amd', 'csrc')}",
                           os.path.join(ROOT, "tests", "cabi", "leaflet_rows.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, timeout=300)
    err = res.stderr.decode()
    assert res.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err
    return res.stdout.decode().splitlines()


def test_every_case_plans_the_parents_rows(lines):
    cases = list(itertools.product(range(7), range(4), (False, True), (False, True), batches()))
    assert len(lines) == len(cases) == 7 * 4 * 2 * 2 * (6 * 3 * 2 + 1)
    seen = set()
    for line, (method, frequency, have, carry, frames) in zip(lines, cases):
        head, got_frames, result, arow, aframes, is0 = ([int(x) for x in part.split()] for part in line.split(":"))
        assert head == [method, frequency, int(have), int(carry)] and got_frames == frames, line
        status, last, want_arow, want_aframes, want_is0 = parent_rows(method, frequency, have, carry, frames, [7, 7], 99)
        assert (result, arow, aframes, is0) == ([status, last], want_arow, want_aframes, want_is0), line
        seen.add((method, status))
    # the sweep is not vacuous: every method plans rows and is refused for want of an assignment (a method that assigns: where
    # the first frame comes before the first assignment frame), clustering alone for want of clusters
    assert seen == {(m, s) for m in range(7) for s in (OK, NOT_PRIMED)} | {(CLUSTERING, NO_CLUSTERS)}


def test_the_sweep_holds_what_the_issue_names(lines):
    """Frequencies 1, 2 and 3 (and 0: once), both flags both ways, 0 to 5 frames from 0, 1 and 4 in steps of 1 and 2, and the
    irregular list: read back from the program's own lines."""
    heads = {tuple(int(x) for x in line.split(":")[0].split()) for line in lines}
    assert heads == set(itertools.product(range(7), range(4), (0, 1), (0, 1)))
    frames = {tuple(int(x) for x in line.split(":")[1].split()) for line in lines}
    assert frames == {tuple(b) for b in batches()}
    assert tuple(IRREGULAR) in frames and any(len(b) == 5 and b[0] == 4 and b[1] == 6 for b in frames)
