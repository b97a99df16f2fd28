#!/usr/bin/env python3
"""Per-molecule order rows against the only other way to get them.
python tools/molecule_rows_bench.py [--systems aa,cg] [--frames 4000] [--reps 5] [--out profiles/molecule_rows_bench.json]

Systems: V-AA (synthetic.aa_membrane(): 256 lipids, 64 accumulators; two groups, slots 0-31 and 32-63) and the coarse-grained
membrane (synthetic.cg_membrane(): 3072 lipids, 11 accumulators; one group per molecule type), --frames frames resident in
device memory.  One process runs, alternating, after a warm-up of each:
  (a) plain   no rows: k_bonds_tiled, the floor
  (b) rows_tw tables.timewise = 1: k_bonds_tiled_tw, the comparable second output (rows per slot, left on the device)
  (c) split   what the rows replace: one molecule type per lipid plus timewise = 1, and timewise() to the host — the only
              way to get the numbers out
  (d) mol     set_molecule_rows, and molecule_rows() to the host
A time is a host clock around submit_device + the route's read-out of an already created handle that was reset before; the
median of --reps is reported with the spread, the device time of the order kernel group (gorder_hip_kernel_time_group), the
bytes each route brings to the host and (d)'s n_runs.  (d)'s integers must equal (c)'s, folded by group, and (d)'s finish()
must equal (a)'s, and (d) must be faster than (c): the run ends with a non-zero status where one of the three does not
hold.  The GPU work runs in a child process under a time limit; the parent prints ONE JSON line (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_system(name, args):
    import dataclasses

    import numpy as np
    from gorder_amd import HipEngine, synthetic
    from gorder_amd.abi import Leaflets, MolType, Tables

    if name == "aa":
        system, groups = synthetic.aa_membrane(), [list(range(0, 32)), list(range(32, 64))]
    else:
        system, groups = synthetic.cg_membrane(), [list(range(0, 11))]
    t = system.tables
    assert len(t.molecule_types) == 1
    mt = t.molecule_types[0]
    n_mol, nb = mt.n_molecules, mt.n_bond_types
    bonds = np.asarray(mt.bonds)
    split = Tables(n_atoms=t.n_atoms, molecule_types=[MolType(n_molecules=1, bonds=bonds[:, i:i + 1, :]) for i in range(n_mol)],
                   handle_pbc=t.handle_pbc, normal=t.normal, leaflets=Leaflets(), timewise=True)
    d_xyz, d_box = system.frames_device(args.frames, seed=1000)
    fi = np.arange(args.frames)
    plain, rows_tw, spl, mol = HipEngine(t), HipEngine(dataclasses.replace(t, timewise=True)), HipEngine(split), HipEngine(t)
    mol.set_molecule_rows(groups)
    out = {}

    def read(route, e):
        if route == "split":
            out["split"] = e.timewise(args.frames)
        elif route == "mol":
            out["mol"] = e.molecule_rows()
        else:
            e.synchronize()

    routes = {"plain": plain, "rows_tw": rows_tw, "split": spl, "mol": mol}

    def run(route):
        e = routes[route]
        e.reset()
        e.synchronize()
        out.pop(route, None)
        t0 = time.perf_counter()
        e.submit_device(d_xyz, d_box, fi)
        read(route, e)
        return time.perf_counter() - t0

    for route in routes:                                      # warm-up
        run(route)
    # (d)'s integers against (c)'s, (d)'s totals against (a)'s
    tw_s, tw_c = out["split"]
    ms, mc, mf = out["mol"]
    agree = bool((mf == fi).all())
    for g, slots in enumerate(groups):
        agree = agree and bool((tw_s[:, 0].reshape(args.frames, n_mol, nb)[:, :, slots].sum(axis=2) == ms[:, g]).all())
        agree = agree and bool((tw_c[:, 0].reshape(args.frames, n_mol, nb)[:, :, slots].sum(axis=2) == mc[:, g]).all())
    a, d = plain.finish(), mol.finish()
    totals_agree = bool((a.sums == d.sums).all() and (a.counts == d.counts).all())
    times = {route: [] for route in routes}
    for _ in range(args.reps):
        for route in routes:
            times[route].append(run(route))
    kernel_ms = {}
    for route, e in routes.items():
        e.reset()
        e.kernel_time(reset=True)                             # switches the events on
        e.submit_device(d_xyz, d_box, fi)
        e.synchronize()
        e.kernel_time()
        kernel_ms[route] = {g: ms_ for g, ms_, _ in e.kernel_groups()}
        e.kernel_time(reset=True)
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {"system": system.name, "n_molecules": int(n_mol), "n_acc": int(t.n_acc), "n_acc_split": int(split.n_acc), "groups": len(groups),
            "samples_per_frame": int(t.n_samples_per_frame), "rows_agree_with_split": agree, "finish_agrees_with_plain": totals_agree,
            "lane_order": mol.molecule_rows_stats(),
            "seconds_median": med, "seconds_spread": {k: [float(min(v)), float(max(v))] for k, v in times.items()},
            "frames_per_second": {k: float(args.frames / v) for k, v in med.items()},
            "kernel_ms": kernel_ms,
            "bytes_to_host": {"plain": 0, "rows_tw": 0, "split": int(2 * args.frames * 3 * split.n_acc * 8),
                              "mol": int(args.frames * len(groups) * n_mol * 8)},
            "mol_over_plain": med["mol"] / med["plain"], "mol_over_rows_tw": med["mol"] / med["rows_tw"],
            "split_over_mol": med["split"] / med["mol"], "mol_faster_than_split": bool(med["mol"] < med["split"])}


def child(args):
    import torch

    assert torch.cuda.is_available(), "molecule_rows_bench needs a GPU"
    out = {"tool": "tools/molecule_rows_bench.py", "device": torch.cuda.get_device_name(0), "frames": args.frames, "reps": args.reps,
           "systems": {name: bench_system(name, args) for name in args.systems.split(",")}}
    print("MOLECULE_ROWS_BENCH " + json.dumps(out))
    failed = [f"{name}: {key}" for name, r in out["systems"].items()
              for key in ("rows_agree_with_split", "finish_agrees_with_plain", "mol_faster_than_split") if not r[key]]
    if failed:
        sys.stderr.write("molecule_rows_bench: FAILED " + ", ".join(failed) + "\n")
        sys.exit(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="aa,cg")
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    line = next((ln for ln in res.stdout.splitlines() if ln.startswith("MOLECULE_ROWS_BENCH ")), None)
    if line is None:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        sys.exit(res.returncode or 1)
    sys.stderr.write(res.stderr[-2000:])
    line = line[len("MOLECULE_ROWS_BENCH "):]
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(json.loads(line), indent=1) + "\n")
    sys.exit(res.returncode)      # not 0 where (d) disagrees with (c) or (a), or is not faster than (c): the figures are kept all the same


if __name__ == "__main__":
    main()
