#!/usr/bin/env python3
"""Error estimates and convergence columns: the route over the host against the route on the device.
python tools/error_bench.py [--frames 10000,200000] [--reps 5] [--leaflets] [--out profiles/error_bench.json]

V-AA (synthetic.aa_membrane(256): 64 accumulators) with per-frame rows; --resident frames are generated in HBM and
submitted in turn until the handle holds F rows.  Then, on the same handle and the same rows, two routes to the error tree
and the convergence text:
  host    eng.timewise() (every row crosses the link) + results_tree(timewise=...) + convergence_text(timewise)
  device  eng.error_estimate(error_groups) + results_tree(errors=...) + eng.convergence() + convergence_text(prefix=...)
Both must give the same tree and the same text (checked).  Times are host clocks (median of --reps after a warm-up, the
routes alternating), split into the part that fetches the numbers and the Python that formats them; the device time of
the k_tw_* kernels comes from gorder_hip_kernel_time_group.  A frame count whose rows do not fit the free device memory is
skipped with a printed reason.  The GPU work runs in a child process under a time limit; the parent prints ONE JSON line
(and writes it to --out)."""
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
    from gorder_amd import HipEngine, synthetic, writers
    from gorder_amd import structure as st
    from gorder_amd.abi import LEAFLETS_GLOBAL, LEAFLETS_NONE

    assert torch.cuda.is_available(), "error_bench needs a GPU"
    system = synthetic.aa_membrane(256, leaflets=LEAFLETS_GLOBAL if args.leaflets else LEAFLETS_NONE, timewise=True)
    labels = aa_labels(system)
    n_acc = system.tables.n_acc
    groups = st.error_groups(labels, "aa")
    types = writers.convergence_groups(labels)
    d_xyz, d_box = system.frames_device(args.resident, seed=1000)
    cases = []
    for F in [int(x) for x in args.frames.split(",")]:
        need = 2 * F * 3 * n_acc * 16 * 2 + F * 3 * len(types) * 40       # the rows (grown by doubling), the scan's scratch
        free = torch.cuda.mem_get_info()[0]
        if need > free:
            reason = f"{F} frames skipped: the rows need about {need >> 20} MiB, {free >> 20} MiB are free"
            print(reason, file=sys.stderr)
            cases.append({"frames": F, "skipped": reason})
            continue
        eng = HipEngine(system.tables)
        done = 0
        while done < F:
            n = min(args.resident, F - done)
            eng.submit_device(d_xyz[:n], d_box[:n], np.arange(done, done + n))
            done += n
        res = eng.finish()
        assert eng.timewise_rows() == F

        def host_route():
            t0 = time.perf_counter()
            tw = eng.timewise(F)
            t1 = time.perf_counter()
            tree = st.results_tree(res, labels, "aa", leaflets=args.leaflets, timewise=tw, n_blocks=args.blocks)
            text = writers.convergence_text(tw, labels, "aa", args.leaflets)
            return t1 - t0, time.perf_counter() - t1, tree, text

        def device_route():
            t0 = time.perf_counter()
            errors = eng.error_estimate(groups, args.blocks)
            prefix, _ = eng.convergence(types)
            t1 = time.perf_counter()
            tree = st.results_tree(res, labels, "aa", leaflets=args.leaflets, errors=dict(zip(map(tuple, groups), errors)))
            text = writers.convergence_text(None, labels, "aa", args.leaflets, prefix=prefix)
            return t1 - t0, time.perf_counter() - t1, tree, text

        a, b = host_route(), device_route()                                # warm-up, and the two routes agree
        same = repr(a[2]) == repr(b[2]) and a[3] == b[3]
        times = {"host": [], "device": []}
        for _ in range(args.reps):
            for name, route in (("host", host_route), ("device", device_route)):
                fetch, fmt, _, _ = route()
                times[name].append((fetch, fmt))
        eng.kernel_time(reset=True)                                        # switches the events on
        eng.error_estimate(groups, args.blocks)
        eng.convergence(types)
        kernel_ms = {g: ms for g, ms, _ in eng.kernel_groups()}
        eng.kernel_time(reset=True)

        def med(name, k):
            return float(np.median([t[k] for t in times[name]]))
        cases.append({
            "frames": F, "routes_agree": bool(same),
            "host": {"fetch_s": med("host", 0), "python_s": med("host", 1), "total_s": float(np.median([sum(t) for t in times["host"]])),
                     "bytes_to_host": int(2 * F * 3 * n_acc * 8)},
            "device": {"fetch_s": med("device", 0), "python_s": med("device", 1),
                       "total_s": float(np.median([sum(t) for t in times["device"]])),
                       "bytes_to_host": int(len(groups) * 3 * 4 + F * 3 * len(types) * 4 + 2 * 3 * len(types) * 8),
                       "kernel_ms": kernel_ms, "kernel_ms_total": float(sum(kernel_ms.values())),
                       "row_bytes_read_by_k_tw_blocks": int(F * (2 if args.leaflets else 3) * n_acc * 16)},
            "spread_s": {k: [float(min(sum(t) for t in v)), float(max(sum(t) for t in v))] for k, v in times.items()}})
        del eng
    out = {"tool": "tools/error_bench.py", "device": torch.cuda.get_device_name(0), "system": system.name, "n_acc": int(n_acc),
           "leaflets": bool(args.leaflets), "n_blocks": args.blocks, "error_groups": len(groups), "convergence_groups": len(types),
           "resident_frames": args.resident, "reps": args.reps, "cases": cases}
    print("ERROR_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="10000,200000")
    ap.add_argument("--resident", type=int, default=2000, help="frames generated in device memory and submitted in turn")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--leaflets", action="store_true", help="global leaflets: three columns per value")
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    line = next((ln for ln in res.stdout.splitlines() if ln.startswith("ERROR_BENCH ")), None)
    if res.returncode != 0 or line is None:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        sys.exit(res.returncode or 1)
    sys.stderr.write(res.stderr[-2000:])
    line = line[len("ERROR_BENCH "):]
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
