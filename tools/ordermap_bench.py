#!/usr/bin/env python3
"""Finished ordermaps: the route over the host against the route on the device.
python tools/ordermap_bench.py [--grids 91,501] [--frames 100] [--reps 5] [--out profiles/ordermap_bench.json]

V-AA with global leaflets (synthetic.aa_membrane(256): 64 accumulators) and ordermaps of N x N tiles over its 9 nm box, for
every N of --grids.  After --frames frames, on the same handle and the same maps, two routes to the values of every map the
reference writes (structure.ordermap_groups):
  host    eng.finish() (every raw tile crosses the link, 16 bytes a slot and plane) + structure.ordermap_values
  device  eng.ordermaps(groups) (k_map_finalise; one float per group, plane and tile crosses the link)
Both must give the same bits (checked).  Times are host clocks (median of --reps after a warm-up, the routes alternating):
`fetch_s` until the numbers are in host memory, `values_s` until the finished values are; the device time of k_map_finalise
comes from gorder_hip_kernel_time_group.  The GPU work runs in a child process under a time limit; the parent prints ONE
JSON line (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def aa_labels(system):
    from gorder_amd import structure as st
    from gorder_amd import synthetic
    carbons, tbonds, _, h_per_c = synthetic._aa_template()
    bl = [st.BondLabel(int(c), f"C{c}", int(h), f"H{h}") for c, h in tbonds]
    heavy = [(int(c), f"C{c}", "POPC") for c, nh in zip(carbons, h_per_c) if nh]
    mt = system.tables.molecule_types[0]
    return [st.MolLabels(mt.name, bl, heavy, mt.n_molecules, 0)]


def child(args):
    import numpy as np
    import torch
    from gorder_amd import HipEngine, synthetic
    from gorder_amd import structure as st
    from gorder_amd.abi import LEAFLETS_GLOBAL, OrderMap

    assert torch.cuda.is_available(), "ordermap_bench needs a GPU"
    cases = []
    for n in [int(x) for x in args.grids.split(",")]:
        system = synthetic.aa_membrane(256, leaflets=LEAFLETS_GLOBAL)
        bx = float(system.box[0])
        bin = bx / (n - 1)                                                  # GridMap: round(span / bin) + 1 tiles
        system.tables.ordermap = OrderMap(enabled=True, plane=0, span_x=(0.0, bx), span_y=(0.0, float(system.box[1])), bin=(bin, bin))
        labels = aa_labels(system)
        groups = [g.slots for g in st.ordermap_groups(labels, "aa")]
        n_acc = system.tables.n_acc
        eng = HipEngine(system.tables)
        nx, ny = eng.ordermap_dims()
        d_xyz, d_box = system.frames_device(args.frames, seed=1000)
        eng.submit_device(d_xyz, d_box, np.arange(args.frames))
        eng.synchronize()

        def host_route():
            t0 = time.perf_counter()
            res = eng.finish()
            t1 = time.perf_counter()
            values = st.ordermap_values(res, groups, args.min_samples, negate=True)
            return t1 - t0, time.perf_counter() - t0, values

        def device_route():
            t0 = time.perf_counter()
            values = eng.ordermaps(groups, min_samples=args.min_samples, negate=True)
            t1 = time.perf_counter()
            return t1 - t0, t1 - t0, values

        a, b = host_route(), device_route()                                # warm-up, and the two routes agree
        nan = np.isnan(a[2])
        same = bool(np.array_equal(nan, np.isnan(b[2])) and np.array_equal(a[2].view(np.uint32)[~nan], b[2].view(np.uint32)[~nan]))
        sampled = float((~nan[:, 0]).mean())
        del a, b
        times = {"host": [], "device": []}
        for _ in range(args.reps):
            for name, route in (("host", host_route), ("device", device_route)):
                fetch, total, _ = route()
                times[name].append((fetch, total))
        eng.kernel_time(reset=True)                                        # switches the events on
        for _ in range(args.reps):
            eng.ordermaps(groups, min_samples=args.min_samples, negate=True)
        kernel = {g: (ms, k) for g, ms, k in eng.kernel_groups()}
        eng.kernel_time(reset=True)
        k_ms, k_n = kernel.get("k_map_finalise", (float("nan"), 0))
        memberships = sum(len(g) for g in groups)
        read = memberships * 3 * nx * ny * 16
        written = len(groups) * 3 * nx * ny * 4

        def med(name, k):
            return float(np.median([t[k] for t in times[name]]))
        cases.append({
            "tiles": [nx, ny], "groups": len(groups), "slot_memberships": memberships, "routes_agree": same,
            "fraction_of_tiles_with_a_value_full_plane": sampled,
            "host": {"bytes_to_host": int(2 * 3 * n_acc * nx * ny * 8), "fetch_s": med("host", 0), "values_s": med("host", 1)},
            "device": {"bytes_to_host": int(written), "fetch_s": med("device", 0), "values_s": med("device", 1),
                       "k_map_finalise_ms": k_ms / k_n if k_n else None, "k_map_finalise_launches_timed": k_n,
                       "k_map_finalise_bytes_read": int(read), "k_map_finalise_bytes_written": int(written),
                       "k_map_finalise_TB_per_s": (read + written) / (k_ms / k_n * 1e-3) / 1e12 if k_n else None},
            "spread_values_s": {k: [float(min(t[1] for t in v)), float(max(t[1] for t in v))] for k, v in times.items()}})
        del eng, d_xyz, d_box
    out = {"tool": "tools/ordermap_bench.py", "device": torch.cuda.get_device_name(0), "system": "aa256, global leaflets",
           "n_acc": int(n_acc), "frames": args.frames, "min_samples": args.min_samples, "reps": args.reps, "cases": cases}
    print("ORDERMAP_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="91,501", help="tiles along x and y, one case each")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--min-samples", dest="min_samples", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    line = next((ln for ln in res.stdout.splitlines() if ln.startswith("ORDERMAP_BENCH ")), None)
    if res.returncode != 0 or line is None:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        sys.exit(res.returncode or 1)
    sys.stderr.write(res.stderr[-2000:])
    line = line[len("ORDERMAP_BENCH "):]
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
