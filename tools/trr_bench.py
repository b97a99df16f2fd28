#!/usr/bin/env python3
"""What the device route for TRR trajectories delivers:
python tools/trr_bench.py [--unique U] [--repeats R] [--reps N] [--out FILE (default profiles/trr_bench.json)] [--host-only]

The V-AA workload (bench.py's aa256: 25 088 analysed atoms) as a TRR file the tool writes once per case — bare, and in
front of three times as many solvent atoms (as tools/e2e_group_probe.py does for XTC), in single and in double precision —
read from the page cache through gorder_hip_run_trajectory:
  (a) frames/s with device_decode = 1 (the positions of the analysed atoms travel as the file holds them, k_trr_unpack)
  (b) frames/s of the same call with device_decode = 0 (host threads swap, round and copy; what a run of these files did
      before the device route existed — `--host-only` measures just this, for a checkout that has no device route, and
      `--parent-json` puts such a result beside (b))
  (c) k_trr_unpack alone on one resident batch (about 0.6 GB and more: not a cache's): device time per call from gorder_hip_kernel_time_group and the bytes it
      moves (12 or 24 in + 12 out per analysed atom) over that time — to be held against the streaming rate
      tools/microbench measures on the same card, not against the data sheet
  (d) bytes_h2d and the reader's busy time from the statistics
(a) and (b) alternate, median of --reps runs each and their spread; both routes must give the same sums (checked).
Every case is a child process of its own under `timeout -k 10`; the first one that fails ends the run.  The parent prints
ONE JSON line (and writes it to --out)."""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("bare", False), ("bare", True), ("solvent", False), ("solvent", True)]


def write_trr(path, xyz, box, double):
    """frames [F, N, 3] as a GROMACS TRR file (XDR, big-endian; box + positions per frame)"""
    import numpy as np
    rs, kind = (8, ">f8") if double else (4, ">f4")
    n = xyz.shape[1]
    ver = b"GMX_trn_file"
    with open(path, "wb") as f:
        for k in range(xyz.shape[0]):
            f.write(struct.pack(">ii", 1993, len(ver) + 1) + struct.pack(">i", len(ver)) + ver)
            f.write(struct.pack(">13i", 0, 0, 9 * rs, 0, 0, 0, 0, 3 * n * rs, 0, 0, n, k, 0))
            f.write(np.array([float(k), 0.0]).astype(kind).tobytes())
            f.write(box[k].astype(kind).tobytes())
            f.write(xyz[k].astype(kind).tobytes())


def child(args):
    import numpy as np
    import torch
    import bench
    from gorder_amd import HipEngine, xtc

    assert torch.cuda.is_available(), "trr_bench needs a GPU"
    layout, double = args.case.split(":")[0], args.case.endswith(":f64")
    system, _ = bench.make_system("aa256")
    n_sel, U = system.n_atoms, args.unique
    xyz = system.frames(U, seed=11)
    if layout == "solvent":
        rng = np.random.default_rng(7)
        water = rng.uniform(0.0, 9.0, size=(U, 3 * n_sel, 3)).astype(np.float32)
        xyz = np.concatenate([xyz, water], axis=1)
    group = np.arange(n_sel, dtype=np.uint32)
    cores = min(16, bench.host_cores())               # (what a rank of a node has; the copies saturate there)
    out = {"layout": layout, "precision": "double" if double else "single", "atoms_in_file": int(xyz.shape[1]),
           "atoms_analysed": int(n_sel), "unique_frames": U, "files_per_run": args.repeats, "threads": cores}
    with tempfile.TemporaryDirectory(prefix="gorder_trr_bench_") as tmp:
        path = os.path.join(tmp, "t.trr")
        write_trr(path, xyz, system.box9(U), double)
        out["file_bytes_per_frame"] = os.path.getsize(path) / U
        routes = [("host_decode", False)] if args.host_only else [("device_decode", True), ("host_decode", False)]
        # a handle per route: each keeps its staging buffers between runs (a handle that changes route pins them anew)
        engines = {route: HipEngine(system.tables) for route, _ in routes}
        sums, runs, last = {}, {r: [] for r, _ in routes}, {}
        for route, dev in routes:                      # page cache, kernels, the staging buffers of either route
            engines[route].run_trajectory([path] * args.repeats, group=group, threads=cores, device_decode=dev)
        for _ in range(args.reps):
            for route, dev in routes:
                eng = engines[route]
                eng.reset()
                st = eng.run_trajectory([path] * args.repeats, group=group, threads=cores, device_decode=dev)
                sums[route] = eng.finish().sums
                assert st["n_frames"] == U * args.repeats
                runs[route].append(st["n_frames"] / st["seconds_total"])
                last[route] = st
        if not args.host_only:
            assert np.array_equal(sums["host_decode"], sums["device_decode"]), "the two routes differ"
            assert last["device_decode"]["device_decode"] == 1 and last["host_decode"]["device_decode"] == 0
        for route, _ in routes:
            st, v = last[route], runs[route]
            out[route] = {"frames_per_s": float(np.median(v)), "frames_per_s_runs": [float(x) for x in v],
                          "spread": float((max(v) - min(v)) / np.median(v)), "frames": int(st["n_frames"]),
                          "bytes_h2d_per_frame": st["bytes_h2d"] / st["n_frames"], "batch_frames": int(st["batch_frames"]),
                          "reader_busy_s": st["seconds_decode"], "gpu_starved_s": st["seconds_gpu_starved"],
                          "reader_stalled_s": st["seconds_reader_stalled"], "seconds_total": st["seconds_total"],
                          "pcie_GBps": st["bytes_h2d"] / st["seconds_total"] / 1e9}
        if not args.host_only:
            out["device_over_host"] = out["device_decode"]["frames_per_s"] / out["host_decode"]["frames_per_s"]
            # (c) the kernel alone, on one resident batch of the file's frames taken --kernel-files times: blob and output
            # together beyond what the 256-MB last-level cache holds, so that the rate is HBM's
            ws = xtc.pack_trajectory([path] * args.kernel_files, group=group, chunk=U, threads=cores)
            blob = np.concatenate([w["blob"] for w in ws])
            table, at = [], 0
            for w in ws:
                fr = w["frames"].copy()
                fr["offset"] += at
                at += w["blob"].size
                table.append(fr)
            table = np.concatenate(table)
            U = len(table)
            assert U == args.unique * args.kernel_files
            d_blob = torch.from_numpy(blob).cuda()
            d_frames = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).cuda()
            d_out = torch.empty((U, n_sel, 3), dtype=torch.float32, device="cuda")
            k = HipEngine(system.tables)
            k.kernel_time()
            call = lambda: k.xtc_decode(d_blob.data_ptr(), d_blob.numel(), d_frames.data_ptr(), U, int(xyz.shape[1]), 0, n_sel,
                                        d_out.data_ptr(), n_sel)
            for _ in range(5):
                call()
            k.synchronize()
            k.kernel_time(reset=True)
            for _ in range(args.kernel_calls):
                call()
            k.synchronize()
            k.kernel_time()
            ms, seg = next((ms, seg) for name, ms, seg in k.kernel_groups() if name == "k_trr_unpack")
            moved = U * n_sel * ((24 if double else 12) + 12)
            out["k_trr_unpack"] = {"frames_per_call": U, "calls": int(seg), "ms_per_call": ms / seg, "bytes_per_call": moved,
                                   "TBps": moved / (ms / seg * 1e-3) / 1e12,
                                   "resident_bytes": int(d_blob.numel() + d_out.numel() * 4)}
            host = xtc.read_trajectory([path], group=group, threads=cores)[0]
            got = d_out.cpu().numpy().view(np.uint32).reshape(args.kernel_files, args.unique, n_sel, 3)
            assert all(np.array_equal(g, host.view(np.uint32)) for g in got), "k_trr_unpack differs from the host"
    out["device"] = torch.cuda.get_device_name(0)
    print("TRR_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unique", type=int, default=64, help="distinct frames in the file")
    ap.add_argument("--repeats", type=int, default=300, help="times the file is read per run")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-calls", type=int, default=30)
    ap.add_argument("--kernel-files", type=int, default=16, help="times the file's frames are taken for the resident batch of (c)")
    ap.add_argument("--timeout", type=int, default=280, help="seconds per case")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--parent-json", default=None, help="a --host-only result of the commit before the device route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trr_bench.json"))
    ap.add_argument("--case", default=None)
    args = ap.parse_args()
    if args.case:
        return child(args)
    passed = [a for k, a in enumerate(sys.argv[1:]) if a not in ("--out", "--parent-json") and
              (k == 0 or sys.argv[k] not in ("--out", "--parent-json"))]
    result = {"tool": "tools/trr_bench.py", "workload": "aa256", "cases": []}
    for layout, double in CASES:
        case = f"{layout}:{'f64' if double else 'f32'}"
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--case", case] + passed
        t0 = time.time()
        res = subprocess.run(cmd, capture_output=True, text=True)
        line = next((ln for ln in res.stdout.splitlines() if ln.startswith("TRR_BENCH ")), None)
        if res.returncode != 0 or line is None:           # the first failure ends the run: nothing more is started
            sys.stderr.write(f"{case}: exit status {res.returncode}\n" + res.stdout[-2000:] + res.stderr[-4000:])
            sys.exit(res.returncode or 1)
        one = json.loads(line[len("TRR_BENCH "):])
        one["case_seconds"] = time.time() - t0
        result["device"] = one.pop("device")
        result["cases"].append(one)
    if args.parent_json:
        with open(args.parent_json) as fh:
            parent = {(c["layout"], c["precision"]): c["host_decode"] for c in json.load(fh)["cases"]}
        for c in result["cases"]:
            c["host_decode_on_the_parent_commit"] = parent.get((c["layout"], c["precision"]))
    if not args.host_only:
        result["device_route_not_below_host_route"] = all(
            c["device_decode"]["frames_per_s"] >= c["host_decode"]["frames_per_s"] * (1.0 - c["host_decode"]["spread"])
            for c in result["cases"])
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
