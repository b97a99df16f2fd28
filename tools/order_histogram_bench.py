#!/usr/bin/env python3
"""Order distributions against the only other way to get them.
python tools/order_histogram_bench.py [--systems aa,cg] [--frames 4000] [--reps 5] [--bins 90] [--out profiles/order_histogram_bench.json]

Systems: V-AA (synthetic.aa_membrane(): 256 lipids, 64 accumulators) and the coarse-grained membrane (synthetic.cg_membrane():
3072 lipids, 11 accumulators), --frames frames resident in device memory, --bins tilt bins (structure.tilt_edges).  One process
runs, alternating, after a warm-up of each:
  (a) plain   no histogram: k_bonds_tiled, the floor
  (b) lds     set_order_histogram: k_bonds_dist with its LDS table, and order_histogram() to the host
  (b') direct the same with GORDER_HIP_DIST_DIRECT=1: a global atomic per sample
  (c) split   the only other way: one molecule type per lipid plus timewise = 1, timewise() to the host, numpy.searchsorted
              and numpy.bincount over every sample's tick
A time is a host clock around submit_device + the route's read-out of an already created handle that was reset before; the
median of --reps is reported with the spread and the device time of the order kernel group (gorder_hip_kernel_time_group).
Then the chunk length of (b) is swept (GORDER_HIP_DIST_SAMPLES_PER_WORD: 0 = the extras' chunks, 2, 8 = the default, 32, and
one workgroup per tile), device time of the kernel group only: what the epilogue costs at short chunks.
(b), (b') and (c) must give the same integers, (b)'s finish() must equal (a)'s, and (b) must be faster than (c): the run ends
with a non-zero status where one of them does not hold.  The GPU work runs in a child process under a time limit; the parent
prints ONE JSON line (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def engine_with(env, make):
    """An engine created with `env` set: the switches are read once at creation."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return make()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def bench_system(name, args):
    import numpy as np
    from gorder_amd import HipEngine, structure, synthetic
    from gorder_amd.abi import Leaflets, MolType, Tables

    system = synthetic.aa_membrane() if name == "aa" else synthetic.cg_membrane()
    t = system.tables
    assert len(t.molecule_types) == 1
    mt = t.molecule_types[0]
    n_mol, nb = mt.n_molecules, mt.n_bond_types
    bonds = np.asarray(mt.bonds)
    split = Tables(n_atoms=t.n_atoms, molecule_types=[MolType(n_molecules=1, bonds=bonds[:, i:i + 1, :]) for i in range(n_mol)],
                   handle_pbc=t.handle_pbc, normal=t.normal, leaflets=Leaflets(), timewise=True)
    edges = structure.tilt_edges(args.bins)[0]
    n_bins = len(edges) - 1
    d_xyz, d_box = system.frames_device(args.frames, seed=1000)
    fi = np.arange(args.frames)

    def with_hist(env):
        def make():
            e = HipEngine(t)
            e.set_order_histogram(edges)
            return e
        return engine_with(env, make)

    routes = {"plain": HipEngine(t), "lds": with_hist({}), "direct": with_hist({"GORDER_HIP_DIST_DIRECT": "1"}), "split": HipEngine(split)}
    out = {}

    def numpy_histogram(e):
        tw_s, tw_c = e.timewise(args.frames)
        hist = np.zeros(n_bins * t.n_acc, dtype=np.int64)
        slot = np.tile(np.arange(nb), n_mol)                  # slot of the split tables = molecule * nb + bond
        for lo in range(0, args.frames, 250):                 # (in pieces: the index arrays of all frames at once are gigabytes)
            ticks, present = tw_s[lo:lo + 250, 0], tw_c[lo:lo + 250, 0] == 1
            b = np.searchsorted(edges, ticks, "right") - 1
            ok = present & (b >= 0) & (b < n_bins)
            hist += np.bincount((b * t.n_acc + slot)[ok], minlength=hist.size)
        return hist.reshape(n_bins, t.n_acc)

    def read(route, e):
        if route == "split":
            out[route] = numpy_histogram(e)
        elif route == "plain":
            e.synchronize()
        else:
            out[route] = e.order_histogram()

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
    agree = bool((out["lds"] == out["direct"]).all() and (out["lds"][:, 0].astype(np.int64) == out["split"]).all() and not out["lds"][:, 1:].any())
    a, b = routes["plain"].finish(), routes["lds"].finish()
    totals_agree = bool((a.sums == b.sums).all() and (a.counts == b.counts).all())
    in_bins = int(out["lds"][:, 0].sum())
    times = {route: [] for route in routes}
    for _ in range(args.reps):
        for route in routes:
            times[route].append(run(route))

    def kernel_ms(e):
        e.reset()
        e.kernel_time(reset=True)                             # switches the events on
        e.submit_device(d_xyz, d_box, fi)
        e.synchronize()
        e.kernel_time()
        groups = {g: ms_ for g, ms_, _ in e.kernel_groups()}
        e.kernel_time(reset=True)
        return groups

    kernels = {route: kernel_ms(e) for route, e in routes.items()}
    sweep = {}
    for label, env in [("0", {"GORDER_HIP_DIST_SAMPLES_PER_WORD": "0"}), ("2", {"GORDER_HIP_DIST_SAMPLES_PER_WORD": "2"}),
                       ("8", {"GORDER_HIP_DIST_SAMPLES_PER_WORD": "8"}), ("32", {"GORDER_HIP_DIST_SAMPLES_PER_WORD": "32"}),
                       ("one_workgroup_per_tile", {"GORDER_HIP_WG_TARGET": "1"})]:
        e = with_hist(env)
        kernel_ms(e)                                          # warm-up
        sweep[label] = min(kernel_ms(e)["k_bonds_dist"] for _ in range(3))
        agree = agree and bool((e.order_histogram() == out["lds"]).all())
        e.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {"system": system.name, "n_molecules": int(n_mol), "n_acc": int(t.n_acc), "n_acc_split": int(split.n_acc), "bins": int(n_bins),
            "samples_per_frame": int(t.n_samples_per_frame), "samples_in_bins": in_bins, "n_tiles": int(routes["lds"].plan()["n_tiles"]),
            "histograms_agree": agree, "finish_agrees_with_plain": totals_agree,
            "seconds_median": med, "seconds_spread": {k: [float(min(v)), float(max(v))] for k, v in times.items()},
            "frames_per_second": {k: float(args.frames / v) for k, v in med.items()},
            "kernel_ms": kernels, "k_bonds_dist_ms_by_samples_per_word": sweep,
            "bytes_to_host": {"plain": 0, "lds": int(n_bins * 3 * t.n_acc * 8), "direct": int(n_bins * 3 * t.n_acc * 8),
                              "split": int(2 * args.frames * 3 * split.n_acc * 8)},
            "lds_over_plain": med["lds"] / med["plain"], "direct_over_lds": med["direct"] / med["lds"],
            "split_over_lds": med["split"] / med["lds"], "lds_faster_than_split": bool(med["lds"] < med["split"]),
            "direct_beats_lds": bool(med["direct"] < med["lds"])}


def child(args):
    import torch

    assert torch.cuda.is_available(), "order_histogram_bench needs a GPU"
    out = {"tool": "tools/order_histogram_bench.py", "device": torch.cuda.get_device_name(0), "frames": args.frames, "reps": args.reps,
           "systems": {name: bench_system(name, args) for name in args.systems.split(",")}}
    print("ORDER_HISTOGRAM_BENCH " + json.dumps(out))
    failed = [f"{name}: {key}" for name, r in out["systems"].items()
              for key in ("histograms_agree", "finish_agrees_with_plain", "lds_faster_than_split") if not r[key]]
    if failed:
        sys.stderr.write("order_histogram_bench: FAILED " + ", ".join(failed) + "\n")
        sys.exit(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="aa,cg")
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", type=int, default=90)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    line = next((ln for ln in res.stdout.splitlines() if ln.startswith("ORDER_HISTOGRAM_BENCH ")), None)
    if line is None:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        sys.exit(res.returncode or 1)
    sys.stderr.write(res.stderr[-2000:])
    line = line[len("ORDER_HISTOGRAM_BENCH "):]
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(json.loads(line), indent=1) + "\n")
    sys.exit(res.returncode)      # not 0 where the routes disagree or (b) is not faster than (c): the figures are kept all the same


if __name__ == "__main__":
    main()
