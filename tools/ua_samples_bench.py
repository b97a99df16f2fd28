#!/usr/bin/env python3
"""United atoms in order histograms and per-molecule rows against the only other way to get the numbers.
python tools/ua_samples_bench.py [--frames 4000] [--reps 5] [--bins 90] [--lipids 256] [--out profiles/ua_samples_bench.json]

System: V-UA (synthetic.ua_membrane(): 256 Berger-like lipids, 62 virtual C-H per lipid), --frames frames resident in device
memory, --bins tilt bins (structure.tilt_edges), the rows' groups from structure.molecule_groups (one group: the whole lipid).
One process runs, alternating, after a warm-up of each:
  (a) plain   no feature: k_ua_extras mode 0, the floor
  (b) lds     FLAG_UA_SAMPLES + set_order_histogram: k_ua_dist with its LDS table, and order_histogram() to the host
  (b') direct the same with GORDER_HIP_DIST_DIRECT=1: a global atomic per sample
  (d) mol     FLAG_UA_SAMPLES + set_molecule_rows: k_ua_mol, and molecule_rows() to the host
  (c) split   the only other way: every lipid its own molecule type plus timewise = 1, timewise() to the host, then numpy
              (searchsorted + bincount for the histogram, a sum over the slots for the rows; the time is the histogram's)
A time is a host clock around submit_device + the route's read-out of an already created handle that was reset before; the
median of --reps is reported with the spread and the device time per kernel group (gorder_hip_kernel_time_group).
(b), (b') and (c) must give the same integers, (d) must equal (c), finish() of (b) and of (d) must equal (a)'s, and (b) and
(d) must each be faster than (c): the run ends with a non-zero status where one of them does not hold.  No other time is
fixed in advance.  The GPU work runs in a child process under a time limit; the parent prints ONE JSON line (and writes it
to --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOT_MEASURED = ["leaflet planes (the run has no leaflets)", "the LDS / direct crossover in bins x slots (one edge set, one system)",
                "stages of k_ua_mol other than four frames", "mixed handles (bond tiles beside united-atom tiles)",
                "the literal cosine (FLAG_TRIG_ACOS_COS)"]


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


def bench(args):
    import dataclasses

    import numpy as np
    from gorder_amd import HipEngine, abi, structure, synthetic
    from gorder_amd.abi import Leaflets, MolType

    system = synthetic.ua_membrane(args.lipids)
    plain_t = system.tables
    t = dataclasses.replace(plain_t, flags=abi.FLAG_UA_SAMPLES)
    mt = t.molecule_types[0]
    n_mol, ns = mt.n_molecules, mt.n_slots
    split = dataclasses.replace(plain_t, leaflets=Leaflets(), timewise=True, molecule_types=[
        MolType(n_molecules=1, ua_atoms=[(kind, np.asarray(idx)[i:i + 1]) for kind, idx in mt.ua_atoms]) for i in range(n_mol)])
    labels = [structure.UaMolLabels(mt.name, [structure.UaCarbonLabel(q, f"C{q}", int(kind), abi.UA_N_H[int(kind)])
                                              for q, (kind, _) in enumerate(mt.ua_atoms)], n_mol, 0)]
    groups, _ = structure.molecule_groups(labels, "ua")
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

    mol = HipEngine(t)
    mol.set_molecule_rows(groups)
    routes = {"plain": HipEngine(plain_t), "lds": with_hist({}), "direct": with_hist({"GORDER_HIP_DIST_DIRECT": "1"}), "mol": mol,
              "split": HipEngine(split)}
    assert not routes["lds"].order_histogram_route()["direct"] and routes["direct"].order_histogram_route()["direct"]
    out = {}

    def numpy_histogram(tw_s, tw_c):
        hist = np.zeros(n_bins * t.n_acc, dtype=np.int64)
        slot = np.tile(np.arange(ns), n_mol)                  # slot of the split tables = molecule * ns + hydrogen slot
        for lo in range(0, args.frames, 250):                 # (in pieces: the index arrays of all frames at once are gigabytes)
            ticks, present = tw_s[lo:lo + 250, 0], tw_c[lo:lo + 250, 0] == 1
            b = np.searchsorted(edges, ticks, "right") - 1
            ok = present & (b >= 0) & (b < n_bins)
            hist += np.bincount((b * t.n_acc + slot)[ok], minlength=hist.size)
        return hist.reshape(n_bins, t.n_acc)

    def read(route, e):
        if route == "split":
            tw = e.timewise(args.frames)
            out["split"] = numpy_histogram(*tw)
            out["split_tw"] = tw
        elif route == "plain":
            e.synchronize()
        elif route == "mol":
            out[route] = e.molecule_rows()
        else:
            out[route] = e.order_histogram()

    def run(route):
        e = routes[route]
        e.reset()
        e.synchronize()
        out.pop(route, None)
        out.pop("split_tw", None)
        t0 = time.perf_counter()
        e.submit_device(d_xyz, d_box, fi)
        read(route, e)
        return time.perf_counter() - t0

    for route in routes:                                      # warm-up (split last: its rows are kept for the comparison)
        run(route)
    hist_agree = bool((out["lds"] == out["direct"]).all() and (out["lds"][:, 0].astype(np.int64) == out["split"]).all() and
                      not out["lds"][:, 1:].any())
    tw_s, tw_c = out["split_tw"]
    ms, mc, mf = out["mol"]
    rows_agree = bool((mf == fi).all())
    for g, slots in enumerate(groups):
        rows_agree = rows_agree and bool((tw_s[:, 0].reshape(args.frames, n_mol, ns)[:, :, slots].sum(axis=2) == ms[:, g]).all())
        rows_agree = rows_agree and bool((tw_c[:, 0].reshape(args.frames, n_mol, ns)[:, :, slots].sum(axis=2) == mc[:, g]).all())
    del tw_s, tw_c
    a = routes["plain"].finish()
    finish_agree = all(bool((a.sums == r.sums).all() and (a.counts == r.counts).all()) for r in (routes["lds"].finish(), routes["mol"].finish()))
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
        groups_ms = {g: ms_ for g, ms_, _ in e.kernel_groups()}
        e.kernel_time(reset=True)
        return groups_ms

    kernels = {route: kernel_ms(e) for route, e in routes.items()}
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {"system": system.name, "n_molecules": int(n_mol), "n_acc": int(t.n_acc), "n_acc_split": int(split.n_acc), "bins": int(n_bins),
            "groups": len(groups), "samples_per_frame": int(t.n_samples_per_frame), "samples_in_bins": in_bins,
            "histogram_route": routes["lds"].order_histogram_route(), "lane_words": mol.molecule_rows_stats(),
            "histograms_agree": hist_agree, "rows_agree_with_split": rows_agree, "finish_agrees_with_plain": finish_agree,
            "seconds_median": med, "seconds_spread": {k: [float(min(v)), float(max(v))] for k, v in times.items()},
            "frames_per_second": {k: float(args.frames / v) for k, v in med.items()},
            "kernel_ms": kernels,
            "bytes_to_host": {"plain": 0, "lds": int(n_bins * 3 * t.n_acc * 8), "direct": int(n_bins * 3 * t.n_acc * 8),
                              "mol": int(args.frames * len(groups) * n_mol * 8), "split": int(2 * args.frames * 3 * split.n_acc * 8)},
            "lds_over_plain": med["lds"] / med["plain"], "direct_over_lds": med["direct"] / med["lds"], "mol_over_plain": med["mol"] / med["plain"],
            "split_over_lds": med["split"] / med["lds"], "split_over_mol": med["split"] / med["mol"],
            "lds_faster_than_split": bool(med["lds"] < med["split"]), "mol_faster_than_split": bool(med["mol"] < med["split"]),
            "not_measured": NOT_MEASURED}


def child(args):
    import torch

    assert torch.cuda.is_available(), "ua_samples_bench needs a GPU"
    out = {"tool": "tools/ua_samples_bench.py", "device": torch.cuda.get_device_name(0), "frames": args.frames, "reps": args.reps}
    out.update(bench(args))
    print("UA_SAMPLES_BENCH " + json.dumps(out))
    failed = [key for key in ("histograms_agree", "rows_agree_with_split", "finish_agrees_with_plain", "lds_faster_than_split",
                              "mol_faster_than_split") if not out[key]]
    if failed:
        sys.stderr.write("ua_samples_bench: FAILED " + ", ".join(failed) + "\n")
        sys.exit(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", type=int, default=90)
    ap.add_argument("--lipids", type=int, default=256)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    line = next((ln for ln in res.stdout.splitlines() if ln.startswith("UA_SAMPLES_BENCH ")), None)
    if line is None:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        sys.exit(res.returncode or 1)
    sys.stderr.write(res.stderr[-2000:])
    line = line[len("UA_SAMPLES_BENCH "):]
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(json.loads(line), indent=1) + "\n")
    sys.exit(res.returncode)      # not 0 where the routes disagree or a feature is not faster than (c): the figures are kept all the same


if __name__ == "__main__":
    main()
