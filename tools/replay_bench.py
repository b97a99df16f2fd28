#!/usr/bin/env python3
"""What replaying manual leaflets and normals from whole-trajectory tables costs:
python tools/replay_bench.py [--frames F] [--reps R] [--out profiles/replay_bench.json]

The CG fixture of tools/cluster_bench.py's small case (tests/golden/cg.npz: 508 lipids, its frames repeated), resident in
HBM, goes through the same frames these ways:
  classifier     LEAFLETS_CLUSTERING assigned every frame, rows collected (what produces the table)
  table          LEAFLETS_MANUAL, the collected rows set once with set_manual_leaflet_table, ONE submit
  per_frame      LEAFLETS_MANUAL, the route the table replaces: set_manual_leaflets + a submit per frame
  none           LEAFLETS_NONE
and, for manual membrane normals (random vectors, no leaflets):
  normals_table      set_manual_normal_table once, ONE submit
  normals_per_batch  set_normals + a submit per batch of --batch frames
The table routes must give the sums of the routes they replace (checked).  Times are host clocks around submits that end in
a synchronise (median of the repetitions, the routes alternating); the share of the device step the two replay kernels
take comes from gorder_hip_kernel_time_group.  The GPU work runs in a child process under a time limit; the parent prints
ONE JSON line (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def child(args):
    import numpy as np
    import torch
    from cluster_bench import fixture_tables
    from gorder_amd import HipEngine
    from gorder_amd.abi import COLLECT_LEAFLETS

    assert torch.cuda.is_available(), "replay_bench needs a GPU"
    F = args.frames
    (t_none, t_every, _, t_manual), d_xyz, d_box, _ = fixture_tables(F)
    n_mol = t_manual.n_molecules_total
    fi = np.arange(F)

    classifier = HipEngine(t_every)
    classifier.set_collect(COLLECT_LEAFLETS)
    classifier.submit_device(d_xyz, d_box)
    rows, frames = classifier.collected_leaflets()
    want = classifier.finish()
    assert len(rows) == F
    normals = (np.random.default_rng(3).normal(size=(F, n_mol, 3)) * 0.4 + np.array([0.0, 0.0, 1.0])).astype(np.float32)

    engines = {"classifier": classifier, "table": HipEngine(t_manual), "per_frame": HipEngine(t_manual), "none": HipEngine(t_none),
               "normals_table": HipEngine(t_none), "normals_per_batch": HipEngine(t_none)}
    t0 = time.perf_counter()
    engines["table"].set_manual_leaflet_table(rows)
    upload_flags = time.perf_counter() - t0
    t0 = time.perf_counter()
    engines["normals_table"].set_manual_normal_table(normals)
    upload_normals = time.perf_counter() - t0
    n_per_frame = min(F, args.per_frame_frames)

    def run(route):
        e = engines[route]
        e.reset()
        t0 = time.perf_counter()
        if route == "per_frame":
            for k in range(n_per_frame):
                e.set_manual_leaflets(rows[k], k)
                e.submit_device(d_xyz[k:k + 1], d_box[k:k + 1], fi[k:k + 1])
            e.synchronize()
            return (time.perf_counter() - t0) / n_per_frame
        if route == "normals_per_batch":
            for a in range(0, F, args.batch):
                b = min(F, a + args.batch)
                e.set_normals(normals[a:b])
                e.submit_device(d_xyz[a:b], d_box[a:b], fi[a:b])
        else:
            e.submit_device(d_xyz, d_box)
        e.synchronize()
        return (time.perf_counter() - t0) / F

    order = list(engines)
    for route in order:
        run(route)
    equal = {"table_equals_classifier": bool(np.array_equal(engines["table"].finish().sums, want.sums)),
             "normals_table_equals_per_batch": bool(np.array_equal(engines["normals_table"].finish().sums,
                                                                   engines["normals_per_batch"].finish().sums))}
    per_frame = {k: [] for k in order}
    for _ in range(args.reps):
        for route in order:
            per_frame[route].append(run(route))
    shares = {}
    for route, group in (("table", "k_replay_flags"), ("normals_table", "k_replay_normals")):
        e = engines[route]
        e.kernel_time(reset=True)
        e.reset()
        e.submit_device(d_xyz, d_box)
        e.synchronize()
        total, _ = e.kernel_time()
        groups = {g: ms for g, ms, _ in e.kernel_groups()}
        e.kernel_time(reset=True)
        shares[group] = {"ms_per_frame": groups[group] / F, "share_of_step": groups[group] / total,
                         "device_ms_per_frame": {g: ms / F for g, ms in groups.items()}}
    med = {k: float(np.median(v)) for k, v in per_frame.items()}
    out = {"tool": "tools/replay_bench.py", "device": torch.cuda.get_device_name(0), "system": "cg_fixture",
           "atoms_per_frame": int(d_xyz.shape[1]), "molecules": int(n_mol), "frames": F, "reps": args.reps,
           "normals_batch_frames": args.batch, "per_frame_frames_timed": n_per_frame,
           "frames_per_s": {k: 1.0 / v for k, v in med.items()},
           "seconds_per_frame_spread": {k: [float(min(v)), float(max(v))] for k, v in per_frame.items()},
           "table_over_per_frame": med["per_frame"] / med["table"], "table_over_classifier": med["classifier"] / med["table"],
           "none_over_table": med["table"] / med["none"], "normals_table_over_per_batch": med["normals_per_batch"] / med["normals_table"],
           "upload_seconds": {"leaflet_table": upload_flags, "normal_table": upload_normals},
           "table_bytes": {"leaflet_table": int(F * ((n_mol + 63) // 64) * 8), "normal_table": int(F * n_mol * 12)},
           "replay_groups": shares, **equal}
    print("REPLAY_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--per-frame-frames", type=int, default=256)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    line = next((ln for ln in res.stdout.splitlines() if ln.startswith("REPLAY_BENCH ")), None)
    if res.returncode != 0 or line is None:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        sys.exit(res.returncode or 1)
    line = line[len("REPLAY_BENCH "):]
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
