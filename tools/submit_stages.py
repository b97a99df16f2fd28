#!/usr/bin/env python3
"""What a change to the submit path (gorder_hip_submit_device and the launch functions under it) must leave alone, from the
outside: which kernel groups a batch launches, in which order and how often, and what a submit costs the host.

    tools/submit_stages.py labels [OUT.json]      # profiles/submit_stages_labels.json
    tools/submit_stages.py host-time [RUNS]

labels: for every workload bench.py knows (its default, what --full adds, and the rest of make_system), 3 submits of 8
frames with kernel timing on; per workload the labels of gorder_hip_kernel_time_names in order and the segments each one
opened (gorder_hip_kernel_time_group).  The output has no times in it: two builds that launch the same compare equal.

host-time: the smallest synthetic system (a 16-lipid coarse-grained membrane, no leaflets), 2000 device submits of one frame
each, then one synchronize; wall time per submit in microseconds, RUNS times (default 5) after one untimed round.

GORDER_HIP_LIB picks the build (gorder_amd/abi.py): run once per build and compare."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import bench
from gorder_amd import HipEngine, synthetic

WORKLOADS = ["aa256", "cg1m",                                      # the default line; --full's scaling reference
             "aa256-leaflets", "aa256-leaflets-maps", "aa256-leaflets-timewise", "aa256-leaflets-subset", "aa256-timewise",
             "aa256-maps", "aa256-maps-timewise", "aa256-cylinder", "cg3k", "cg3k-leaflets", "cg3k-local", "cg3k-dynamic",
             "ua256", "ua256-maps", "ua256-timewise", "ua256-fast", "ua256-maps-fast", "cg1m-local-r2.5"]
FRAMES, SUBMITS = 8, 3


def labels(out_path):
    out = {}
    for name in WORKLOADS:
        system, _ = bench.make_system(name)
        d_xyz, d_box = system.frames_device(FRAMES * SUBMITS, seed=1)
        eng = HipEngine(system.tables)
        eng.use_torch_stream()
        eng.kernel_time(reset=True)
        for k in range(SUBMITS):
            at = slice(k * FRAMES, (k + 1) * FRAMES)
            eng.submit_device(d_xyz[at], d_box[at], np.arange(at.start, at.stop, dtype=np.uint64))
        eng.synchronize()
        groups = eng.kernel_groups()
        assert " + ".join(g for g, _, _ in groups) == eng.kernel_names()
        out[name] = [[g, n] for g, _, n in groups]
        print(name, out[name], flush=True)
        del eng
    text = json.dumps({"frames_per_submit": FRAMES, "submits": SUBMITS, "labels": out}, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


def host_time(runs, submits=2000):
    system = synthetic.cg_membrane(16)
    d_xyz, d_box = system.frames_device(1, seed=1)
    eng = HipEngine(system.tables)
    eng.use_torch_stream()
    fidx = np.zeros(1, dtype=np.uint64)
    us = []
    for r in range(runs + 1):
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(submits):
            eng.submit_device(d_xyz, d_box, fidx)
        eng.synchronize()
        us.append((time.perf_counter() - t0) / submits * 1e6)
    print(json.dumps({"lib": os.environ.get("GORDER_HIP_LIB", "in-tree"), "submits": submits,
                      "us_per_submit": [round(x, 3) for x in us[1:]]}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "labels":
        labels(sys.argv[2] if len(sys.argv) > 2 else None)
    elif len(sys.argv) > 1 and sys.argv[1] == "host-time":
        host_time(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    else:
        sys.exit(__doc__)
