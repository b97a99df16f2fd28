#!/usr/bin/env python3
"""Bond reorientation against the route it replaces.
python tools/bond_correlation_bench.py [--systems aa,cg] [--frames 4000] [--reps 5] [--max-lag 2048] [--out profiles/bond_correlation_bench.json]

Systems: V-AA (synthetic.aa_membrane(): 256 lipids, 64 accumulators) and the coarse-grained membrane (synthetic.cg_membrane():
3072 lipids, 11 accumulators), --frames frames resident in device memory, the lags of structure.correlation_lags(--max-lag).
One process per system runs, alternating, after a warm-up of each:
  (a) plain   no correlation: k_bonds_tiled, the floor
  (b) corr    set_bond_correlation: the same order pass, then k_bond_units + k_bond_corr, and bond_correlation() to the host
  (b') chunks the same with GORDER_HIP_CORR_GRID=chunks: the chunk-major grid, a workgroup walks every group of lags in turn
  (c) torch   the route it replaces: the same frames as torch tensors on the same GPU, the bond vectors by indexed subtraction
              and the minimum image once, then per lag one batched P2 reduction (float32 arithmetic, float64 sums)
A time is a host clock around the route's work on frames already on the device, ended by its read-out on the host; the median
of --reps is reported with the spread, and the device time of (b)'s kernel groups (gorder_hip_kernel_time_group).
(b') must give (b)'s integers, (c)'s means must agree with (b)'s within 2e-6 (two ticks: the f32 rounding of the squared cosine plus the tick's own
rounding), (b)'s finish() must equal (a)'s, and (b) must be faster than (c): the run ends with a non-zero status where one of
them does not hold.  Every system's GPU work runs in a child process of its own under a time limit; the parent prints ONE JSON
line (and writes it to --out).
Not measured: the L2 hit rate of the lagged loads, a trajectory read from a file."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RING_BUDGET = 2 << 30       # kCorrRingBudget, kCorrMinSubrange of gorder_amd/csrc/bond_corr.h
MIN_SUBRANGE = 64


def bench_system(name, args):
    import numpy as np
    import torch
    from gorder_amd import HipEngine, structure, synthetic

    system = synthetic.aa_membrane() if name == "aa" else synthetic.cg_membrane()
    t = system.tables
    assert len(t.molecule_types) == 1 and t.handle_pbc
    mt = t.molecule_types[0]
    n_mol, nb = mt.n_molecules, mt.n_bond_types
    lags = structure.correlation_lags(args.max_lag)
    F = args.frames
    d_xyz, d_box = system.frames_device(F, seed=1000)
    fi = np.arange(F)
    bonds = torch.from_numpy(np.asarray(mt.bonds).astype(np.int64)).cuda()       # [nb, n_mol, 2]

    plain, corr = HipEngine(t), HipEngine(t)
    corr.set_bond_correlation(lags)
    os.environ["GORDER_HIP_CORR_GRID"] = "chunks"             # (read once, at creation)
    try:
        chunks = HipEngine(t)
    finally:
        del os.environ["GORDER_HIP_CORR_GRID"]
    chunks.set_bond_correlation(lags)
    out = {}

    def torch_route():
        v = d_xyz[:, bonds[..., 1]] - d_xyz[:, bonds[..., 0]]                   # [F, nb, n_mol, 3]
        L = torch.stack([d_box[:, 0, 0], d_box[:, 1, 1], d_box[:, 2, 2]], dim=1)[:, None, None, :]
        half = L / 2
        v = torch.where(v > half, v - L, v)
        v = torch.where(v < -half, v + L, v)
        n2 = (v * v).sum(dim=-1)
        means = torch.full((len(lags), nb), float("nan"), dtype=torch.float64, device=v.device)
        for k, lag in enumerate(int(x) for x in lags):
            if lag >= F:
                continue
            dot = (v[lag:] * v[:F - lag]).sum(dim=-1)
            s = 1.5 * (dot * dot / (n2[lag:] * n2[:F - lag])).clamp(max=1.0) - 0.5
            means[k] = s.sum(dim=(0, 2), dtype=torch.float64) / ((F - lag) * n_mol)
        return means.cpu().numpy()

    def run(route):
        for e in (plain, corr, chunks):
            e.synchronize()
        torch.cuda.synchronize()
        out.pop(route, None)
        if route == "torch":
            t0 = time.perf_counter()
            out[route] = torch_route()
            return time.perf_counter() - t0
        e = {"plain": plain, "corr": corr, "chunks": chunks}[route]
        e.reset()
        e.synchronize()
        t0 = time.perf_counter()
        e.submit_device(d_xyz, d_box, fi)
        if route != "plain":
            out[route] = e.bond_correlation()
        else:
            e.synchronize()
        return time.perf_counter() - t0

    routes = ("plain", "corr", "chunks", "torch")
    for route in routes:                                      # warm-up
        run(route)
    sums, counts = out["corr"]
    grids_agree = bool((out["chunks"][0] == sums).all() and (out["chunks"][1] == counts).all())
    per_slot = np.full(nb, n_mol, dtype=np.uint64)
    counts_ok = all((counts[k, 0] == max(0, F - int(lag)) * per_slot).all() for k, lag in enumerate(lags))
    with np.errstate(invalid="ignore", divide="ignore"):
        device_means = sums[:, 0].astype(np.float64) / counts[:, 0].astype(np.float64) / 1e6
    diff = np.abs(device_means - out["torch"])
    worst = float(np.nanmax(diff))
    means_agree = bool(counts_ok and worst <= 2e-6 and (np.isnan(device_means) == np.isnan(out["torch"])).all())
    a, b = plain.finish(), corr.finish()
    totals_agree = bool((a.sums == b.sums).all() and (a.counts == b.counts).all())
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

    kernel_ms(corr)
    kernel_ms(chunks)
    kernels = {"plain": kernel_ms(plain), "corr": kernel_ms(corr), "chunks": kernel_ms(chunks)}
    pairs = int(sum(max(0, F - int(lag)) for lag in lags)) * int(t.n_samples_per_frame)
    n_tiles = int(corr.plan()["n_tiles"])
    plane_bytes = n_tiles * 256 * 16
    max_lag = int(lags[-1])
    subrange = min(RING_BUDGET // plane_bytes - max_lag, max(F, MIN_SUBRANGE))
    med = {k: float(np.median(v)) for k, v in times.items()}
    corr_ms, units_ms = kernels["corr"]["k_bond_corr"], kernels["corr"]["k_bond_units"]
    c0 = device_means[0]
    return {"system": system.name, "n_molecules": int(n_mol), "n_acc": int(t.n_acc), "samples_per_frame": int(t.n_samples_per_frame),
            "n_tiles": n_tiles, "lags": [int(x) for x in lags], "n_lags": int(len(lags)), "pairs": pairs,
            "means_agree_with_torch": means_agree, "grids_agree": grids_agree, "worst_mean_difference": worst, "counts_are_the_pair_counts": bool(counts_ok),
            "finish_agrees_with_plain": totals_agree, "c_of_lag_0_min": float(np.nanmin(c0)), "c_of_last_lag_mean": float(np.nanmean(device_means[-1])),
            "seconds_median": med, "seconds_spread": {k: [float(min(v)), float(max(v))] for k, v in times.items()},
            "kernel_ms": kernels, "k_bond_corr_pairs_per_second": pairs / (corr_ms * 1e-3),
            "k_bond_corr_pairs_per_second_chunk_major": pairs / (kernels["chunks"]["k_bond_corr"] * 1e-3),
            "k_bond_units_share_of_the_pass": units_ms / (units_ms + corr_ms),
            "ring": {"plane_bytes": plane_bytes, "subrange": int(subrange), "planes": int(max_lag + subrange), "bytes": int((max_lag + subrange) * plane_bytes)},
            "bytes_to_host": int(2 * len(lags) * 3 * t.n_acc * 8),
            "corr_over_plain": med["corr"] / med["plain"], "torch_over_corr": med["torch"] / med["corr"],
            "corr_faster_than_torch": bool(med["corr"] < med["torch"])}


CHECKS = ("means_agree_with_torch", "grids_agree", "finish_agrees_with_plain", "corr_faster_than_torch")


def child(args):
    import torch

    assert torch.cuda.is_available(), "bond_correlation_bench needs a GPU"
    out = {"device": torch.cuda.get_device_name(0), "result": bench_system(args.systems, args)}
    print("BOND_CORRELATION_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="aa,cg")
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-lag", type=int, default=2048)
    ap.add_argument("--timeout", type=int, default=420, help="seconds, per system")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    out = {"tool": "tools/bond_correlation_bench.py", "frames": args.frames, "reps": args.reps, "max_lag": args.max_lag, "systems": {},
           "not_measured": ["L2 hit rate of the lagged loads", "a trajectory read from a file"]}
    status = 0
    for name in args.systems.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--systems", name, "--frames", str(args.frames), "--reps", str(args.reps),
               "--max-lag", str(args.max_lag)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        line = next((ln for ln in res.stdout.splitlines() if ln.startswith("BOND_CORRELATION_BENCH ")), None)
        if line is None or res.returncode != 0:     # a step that failed ends the run: nothing more is started on the device
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            sys.exit(res.returncode or 1)
        got = json.loads(line[len("BOND_CORRELATION_BENCH "):])
        out["device"] = got["device"]
        out["systems"][name] = got["result"]
        failed = [key for key in CHECKS if not got["result"][key]]
        if failed:
            sys.stderr.write(f"bond_correlation_bench: FAILED {name}: " + ", ".join(failed) + "\n")
            status = 3
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    sys.exit(status)      # not 0 where a check does not hold: the figures are kept all the same


if __name__ == "__main__":
    main()
