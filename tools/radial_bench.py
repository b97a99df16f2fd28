#!/usr/bin/env python3
"""Radial profiles: one pass with shells against one pass per radius.
python tools/radial_bench.py [--frames 4000] [--shells 8] [--outer 4.0] [--reps 5] [--jitter NM] [--out profiles/radial_bench.json]

V-AA (synthetic.aa_membrane(): 256 lipids, 64 accumulators), a cylinder along z around the box centre, --shells equal steps
out to --outer nm, --frames frames resident in device memory.  One process runs, alternating, after a warm-up of each:
  (a) nested   one handle per radius with the nested cylinders, over the same device frames, their times added: what an
               analysis without shells has to do for the same profile
  (b) outer    one handle with the outer cylinder alone: the floor
  (c) shells   one handle with the shells (k_bonds_shells, the workgroup's table in LDS)
  (d) direct   the same with GORDER_HIP_RADIAL_DIRECT=1 (per-sample global atomics)
A time is a host clock around submit_device + synchronize of an already created handle that was reset before; the median
of --reps is reported with the spread, and the device time of the order kernel of (b), (c), (d) from
gorder_hip_kernel_time_group.  The shells of (c) and (d) must be equal and add up to (b)'s sums, and every shell must be the
difference of two of (a)'s selections (checked).  The GPU work runs in a child process under a time limit; the parent
prints ONE JSON line (and writes it to --out).
--jitter NM replaces the synthetic system's positional noise (0.02 nm: a sample all but never changes its shell) — at the
width of a shell nearly every sample changes it from frame to frame, the worst case of (c)'s open word."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import dataclasses

    import numpy as np
    import torch
    from gorder_amd import HipEngine, synthetic
    from gorder_amd.abi import GEOM_CYLINDER, GEOMREF_BOX_CENTER, Geometry

    assert torch.cuda.is_available(), "radial_bench needs a GPU"
    system = synthetic.aa_membrane()
    if args.jitter is not None:
        system.jitter = args.jitter
    radii = [float(np.float32(args.outer * (k + 1) / args.shells)) for k in range(args.shells)]
    geom = Geometry(kind=GEOM_CYLINDER, reference=GEOMREF_BOX_CENTER, orientation=2, radius=radii[-1],
                    structure_box=tuple(float(x) for x in system.box))

    def tables_of(radius):
        return dataclasses.replace(system.tables, geometry=dataclasses.replace(geom, radius=radius))

    d_xyz, d_box = system.frames_device(args.frames, seed=1000)
    fi = np.arange(args.frames)
    nested = [HipEngine(tables_of(r)) for r in radii]
    outer = HipEngine(tables_of(radii[-1]))
    shells = HipEngine(tables_of(radii[-1]))
    shells.set_radial_shells(radii)
    os.environ["GORDER_HIP_RADIAL_DIRECT"] = "1"          # read once, when a handle is made
    direct = HipEngine(tables_of(radii[-1]))
    del os.environ["GORDER_HIP_RADIAL_DIRECT"]
    direct.set_radial_shells(radii)

    def run(engines):
        for e in engines:
            e.reset()
        for e in engines:
            e.synchronize()
        t0 = time.perf_counter()
        for e in engines:                                    # one after the other: the times of (a) add
            e.submit_device(d_xyz, d_box, fi)
            e.synchronize()
        return time.perf_counter() - t0

    routes = {"nested": nested, "outer": [outer], "shells": [shells], "direct": [direct]}
    for engines in routes.values():                          # warm-up
        run(engines)
    # the four routes give one profile
    want = [e.finish() for e in nested]
    total = outer.finish()
    got, got_direct = shells.radial_shells(), direct.radial_shells()
    agree = bool((total.sums == want[-1].sums).all() and (total.counts == want[-1].counts).all())
    for k in range(len(radii)):
        s = want[k].sums - (want[k - 1].sums if k else 0)
        c = want[k].counts.astype(np.int64) - (want[k - 1].counts.astype(np.int64) if k else 0)
        for r in (got[k], got_direct[k]):
            agree = agree and bool((r.sums == s).all() and (r.counts.astype(np.int64) == c).all())
    agree = agree and bool((shells.finish().sums == total.sums).all() and (direct.finish().sums == total.sums).all())
    times = {name: [] for name in routes}
    for _ in range(args.reps):
        for name, engines in routes.items():
            times[name].append(run(engines))
    kernel_ms = {}
    for name in ("outer", "shells", "direct"):
        e = routes[name][0]
        e.reset()
        e.kernel_time(reset=True)                             # switches the events on
        e.submit_device(d_xyz, d_box, fi)
        e.synchronize()
        e.kernel_time()
        kernel_ms[name] = {g: ms for g, ms, _ in e.kernel_groups()}
        e.kernel_time(reset=True)
    samples = [int(r.counts[0].sum()) for r in got]
    out = {"tool": "tools/radial_bench.py", "device": torch.cuda.get_device_name(0), "system": system.name,
           "n_acc": int(system.tables.n_acc), "jitter_nm": float(system.jitter), "frames": args.frames, "radii_nm": radii, "reps": args.reps,
           "routes_agree": agree, "samples_per_shell": samples,
           "samples_per_frame": int(system.tables.n_samples_per_frame),
           "seconds_median": {k: float(np.median(v)) for k, v in times.items()},
           "seconds_spread": {k: [float(min(v)), float(max(v))] for k, v in times.items()},
           "frames_per_second": {k: float(args.frames / np.median(v)) for k, v in times.items()},
           "kernel_ms": kernel_ms}
    print("RADIAL_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--shells", type=int, default=8)
    ap.add_argument("--outer", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--jitter", type=float, default=None, help="positional noise of the synthetic frames in nm (default: the system's 0.02)")
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    line = next((ln for ln in res.stdout.splitlines() if ln.startswith("RADIAL_BENCH ")), None)
    if res.returncode != 0 or line is None:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        sys.exit(res.returncode or 1)
    sys.stderr.write(res.stderr[-2000:])
    line = line[len("RADIAL_BENCH "):]
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
