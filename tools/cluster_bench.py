#!/usr/bin/env python3
"""What spectral-clustering leaflets cost: python tools/cluster_bench.py [--frames F] [--reps R] [--out FILE]

Two CG membranes resident in HBM — the flat CG fixture itself (tests/golden/cg.npz: 508 PO4 heads, its 101 frames repeated)
and a buckled one of 3 000 lipids (synthetic.cg_buckled) — go through the same frames these ways:
  none             LEAFLETS_NONE
  clustering       LEAFLETS_CLUSTERING assigned every frame, W recomputed in every Lanczos step (the shipped route)
  clustering_w     the same with GORDER_HIP_CLUSTER_STORED_W=1: W stored once a frame, S v reads it
  clustering_once  LEAFLETS_CLUSTERING assigned once (frame 0)
  manual_host      LEAFLETS_MANUAL, the only route before: per frame the heads copied back, the method in numpy (dense eigh
                   after projecting out D^1/2 1, 2-means, orientation by overlap), set_manual_leaflets, a submit per frame
A run whose frames the method cannot match (GORDER_ERR_CLUSTER_MATCH at the synchronise, after all the work) is timed all the
same and listed under "statuses".
With --cutoff the tool measures GORDER_FLAG_CLUSTER_CUTOFF instead (default --out profiles/cluster_cutoff_bench.json): the
buckled 3 000-lipid membrane on the dense and the cut-off route in one run (every frame and once), cg_buckled(n_lipids=8400,
box=(84, 28, 16)) and a 32 768-lipid membrane (box 166 x 56 x 16) on the cut-off route alone.  Times are host clocks around submits that end in a synchronise (median of the repetitions, the routes alternating).  The GPU
work runs in a child process under a time limit; the parent prints ONE JSON line (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_labels(x, box):
    """The method on the host for one frame (float32 numpy; heads [n, 3]) -> 2-means labels [n]."""
    import numpy as np
    f32 = np.float32
    d2 = np.zeros((len(x), len(x)), dtype=f32)
    for k in range(3):
        v = x[:, None, k] - x[None, :, k]
        v = v - box[k] * np.round(v / box[k])
        d2 += v * v
    W = np.exp(-d2)
    deg = W.sum(1)
    s = f32(1) / np.sqrt(deg)
    q = np.sqrt(deg)
    q /= np.sqrt((q * q).sum())
    S = s[:, None] * W * s[None, :]
    Sq = S @ q
    M = S - np.outer(q, Sq) - np.outer(Sq, q) + (q @ Sq) * np.outer(q, q)
    _, vec = np.linalg.eigh((M + M.T) / f32(2))
    rows = vec[:, [-1, -2]].copy()
    rows /= np.maximum(np.sqrt((rows * rows).sum(1)), f32(1e-10))[:, None]
    cen, prev = rows[:2].copy(), None
    for _ in range(100):
        d = np.stack([np.sqrt(((rows - c) ** 2).sum(1)) for c in cen], axis=1)
        lab = (d[:, 1] < d[:, 0]).astype(np.int64)
        if prev is not None and np.array_equal(lab, prev):
            break
        for c in (0, 1):
            cen[c] = rows[lab == c].mean(0) if (lab == c).any() else rows[0]
        prev = lab
    return lab


def host_flags(x, box, prev_upper):
    """-> (flags [n] uint8, upper [n] bool): ab initio without prev_upper, else cluster 0 goes where most of it was."""
    import numpy as np
    lab = host_labels(x, box)
    c1 = lab == 0
    if prev_upper is None:
        n1, n2 = int(c1.sum()), int((~c1).sum())
        c1_upper = n1 > n2 or (n1 == n2 and bool(c1[0]))
    else:
        c1_upper = not ((c1 & prev_upper).sum() < (c1 & ~prev_upper).sum())
    upper = c1 if c1_upper else ~c1
    return np.where(upper, 0, 1).astype(np.uint8), upper


def fixture_tables(F):
    """The CG fixture: (tables of the four routes, frames on the device, box)."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from golden_util import Fixture, cg_setup
    from gorder_amd.abi import LEAFLETS_CLUSTERING, LEAFLETS_MANUAL, Leaflets
    import copy
    fx = Fixture("cg")
    every, _, midx = cg_setup(fx, leaflets=LEAFLETS_CLUSTERING)
    once, _, _ = cg_setup(fx, leaflets=LEAFLETS_CLUSTERING, frequency=0)
    none, _, _ = cg_setup(fx)
    manual = copy.copy(every)
    manual.leaflets = Leaflets(method=LEAFLETS_MANUAL, frequency=1)
    pick = np.arange(F) % len(fx.xyz)
    xyz = np.ascontiguousarray(fx.xyz[pick][:, midx, :])
    return (none, every, once, manual), torch.from_numpy(xyz).cuda(), torch.from_numpy(np.ascontiguousarray(fx.boxes[pick])).cuda(), \
        np.array([fx.boxes[0][0, 0], fx.boxes[0][1, 1], fx.boxes[0][2, 2]], dtype=np.float32)


def synthetic_tables(make, F):
    import numpy as np
    from gorder_amd.abi import LEAFLETS_CLUSTERING, LEAFLETS_MANUAL, LEAFLETS_NONE
    ref = make(leaflets=LEAFLETS_CLUSTERING, frequency=1)[0]
    d_xyz, d_box = ref.frames_device(F, seed=1)
    return (make(leaflets=LEAFLETS_NONE)[0].tables, ref.tables, make(leaflets=LEAFLETS_CLUSTERING, frequency=0)[0].tables,
            make(leaflets=LEAFLETS_MANUAL)[0].tables), d_xyz, d_box, ref.box.astype(np.float32)


def measure(name, tables, d_xyz, d_box, box, F, reps, manual_frames):
    import numpy as np
    import torch
    from gorder_amd import HipEngine
    from gorder_amd.abi import GorderHipError

    t_none, t_every, t_once, t_manual = tables
    heads_np = np.concatenate([np.asarray(m.heads) for m in t_every.molecule_types]).astype(np.int64)
    heads = torch.from_numpy(heads_np).cuda()
    engines = {"none": HipEngine(t_none), "clustering": HipEngine(t_every), "clustering_once": HipEngine(t_once),
               "manual_host": HipEngine(t_manual)}
    os.environ["GORDER_HIP_CLUSTER_STORED_W"] = "1"
    engines["clustering_w"] = HipEngine(t_every)
    del os.environ["GORDER_HIP_CLUSTER_STORED_W"]
    statuses = {}

    def sync(route):
        try:
            engines[route].synchronize()
        except GorderHipError as err:
            statuses[route] = err.status
    for e in engines.values():
        e.use_torch_stream()
    n_manual = min(F, manual_frames)

    def run(route):
        e = engines[route]
        e.reset()
        t0 = time.perf_counter()
        if route != "manual_host":
            e.submit_device(d_xyz, d_box)
            sync(route)
            return (time.perf_counter() - t0) / F
        upper = None
        for k in range(n_manual):
            hx = d_xyz[k].index_select(0, heads).cpu().numpy()
            flags, upper = host_flags(hx, box, upper)
            e.set_manual_leaflets(flags, k)
            e.submit_device(d_xyz[k:k + 1], d_box[k:k + 1], np.array([k]))
        sync(route)
        return (time.perf_counter() - t0) / n_manual

    order = ["none", "clustering", "clustering_w", "clustering_once", "manual_host"]
    for route in order:
        run(route)
    per_frame = {k: [] for k in order}
    for _ in range(reps):
        for route in order:
            per_frame[route].append(run(route))
    # the last single-frame state of a fresh run of frame 0 alone: flags of both S v routes, the solver's statistics
    for route in ("clustering", "clustering_w"):
        engines[route].reset()
        engines[route].submit_device(d_xyz[:1], d_box[:1], np.array([0]))
    f_dev, f_w = engines["clustering"].leaflets()[0], engines["clustering_w"].leaflets()[0]
    stats = engines["clustering"].clustering_stats()
    e = engines["clustering"]
    e.kernel_time(reset=True)
    e.reset()
    e.submit_device(d_xyz, d_box)
    sync("clustering")
    groups = {g: ms for g, ms, _ in e.kernel_groups()}
    e.kernel_time(reset=True)
    med = {k: float(np.median(v)) for k, v in per_frame.items()}
    return {
        "system": name, "atoms_per_frame": int(d_xyz.shape[1]), "statuses": statuses, "heads": int(heads.numel()), "frames": F, "reps": reps,
        "frames_per_s": {k: 1.0 / v for k, v in med.items()},
        "seconds_per_frame_spread": {k: [float(min(v)), float(max(v))] for k, v in per_frame.items()},
        "manual_host_frames_timed": n_manual,
        "device_ms_per_frame": {g: ms / F for g, ms in groups.items() if g.startswith("k_cluster")},
        "lanczos_steps_frame_0": stats["steps"], "two_means_rounds_frame_0": stats["rounds"],
        "stored_w_over_recomputed": med["clustering_w"] / med["clustering"],
        "manual_host_over_clustering": med["manual_host"] / med["clustering"],
        "flags_stored_w_equal_recomputed": bool(np.array_equal(f_dev, f_w)),
    }


def measure_cutoff(name, make, F, reps, dense):
    """frames/s of the cut-off route (and of the dense route on the same frames) every frame and once."""
    import copy
    import numpy as np
    from gorder_amd import HipEngine
    from gorder_amd.abi import FLAG_CLUSTER_CUTOFF, LEAFLETS_CLUSTERING, GorderHipError
    ref = make(leaflets=LEAFLETS_CLUSTERING, frequency=1)[0]
    d_xyz, d_box = ref.frames_device(F, seed=1)
    tables = {"dense": ref.tables, "dense_once": make(leaflets=LEAFLETS_CLUSTERING, frequency=0)[0].tables}
    for k in ("dense", "dense_once"):
        t = copy.copy(tables[k])
        t.flags = t.flags | FLAG_CLUSTER_CUTOFF
        tables["cutoff" + k[5:]] = t
    order = [k for k in ("dense", "cutoff", "dense_once", "cutoff_once") if dense or not k.startswith("dense")]
    engines = {k: HipEngine(tables[k]) for k in order}
    statuses = {}
    for e in engines.values():
        e.use_torch_stream()

    def run(route):
        e = engines[route]
        e.reset()
        t0 = time.perf_counter()
        e.submit_device(d_xyz, d_box)
        try:
            e.synchronize()
        except GorderHipError as err:
            statuses[route] = err.status
        return (time.perf_counter() - t0) / F
    for route in order:
        run(route)
    per_frame = {k: [] for k in order}
    for _ in range(reps):
        for route in order:
            per_frame[route].append(run(route))
    flags, stats = {}, {}
    for route in order:
        if route.endswith("_once"):
            continue
        engines[route].reset()
        engines[route].submit_device(d_xyz[:1], d_box[:1], np.array([0]))
        flags[route], stats[route] = engines[route].leaflets()[0], engines[route].clustering_stats()
    e = engines["cutoff"]
    e.kernel_time(reset=True)
    e.reset()
    e.submit_device(d_xyz, d_box)
    try:
        e.synchronize()
    except GorderHipError:
        pass
    groups = {g: ms for g, ms, _ in e.kernel_groups()}
    e.kernel_time(reset=True)
    med = {k: float(np.median(v)) for k, v in per_frame.items()}
    out = {"system": name, "atoms_per_frame": int(d_xyz.shape[1]), "heads": len(ref.tables.leaflets.membrane), "frames": F,
           "reps": reps, "statuses": statuses, "frames_per_s": {k: 1.0 / v for k, v in med.items()},
           "seconds_per_frame_spread": {k: [float(min(v)), float(max(v))] for k, v in per_frame.items()},
           "device_ms_per_frame": {g: ms / F for g, ms in groups.items() if g.startswith("k_cl")},
           "lanczos_steps_frame_0": {k: v["steps"] for k, v in stats.items()}}
    if dense:
        out["flags_cutoff_equal_dense"] = bool(np.array_equal(flags["cutoff"], flags["dense"]))
        out["cutoff_over_dense_time"] = med["cutoff"] / med["dense"]
        out["cutoff_once_over_dense_once_time"] = med["cutoff_once"] / med["dense_once"]
    return out


def child_cutoff(args):
    import torch
    from gorder_amd import synthetic
    assert torch.cuda.is_available(), "cluster_bench needs a GPU"
    out = {"tool": "tools/cluster_bench.py --cutoff", "device": torch.cuda.get_device_name(0), "systems": [
        measure_cutoff("buckled3000", lambda **kw: synthetic.cg_buckled(n_lipids=3000, **kw), args.frames_large, args.reps, True),
        measure_cutoff("buckled8400", lambda **kw: synthetic.cg_buckled(n_lipids=8400, box=(84.0, 28.0, 16.0), **kw), 16,
                       args.reps, False),
        measure_cutoff("buckled32768", lambda **kw: synthetic.cg_buckled(n_lipids=32768, box=(166.0, 56.0, 16.0), **kw), 4,
                       args.reps, False),
    ]}
    print("CLUSTER_BENCH " + json.dumps(out))


def child(args):
    import torch
    from gorder_amd import synthetic
    assert torch.cuda.is_available(), "cluster_bench needs a GPU"
    out = {"tool": "tools/cluster_bench.py", "device": torch.cuda.get_device_name(0), "systems": [
        measure("cg_fixture", *fixture_tables(args.frames), args.frames, args.reps, args.manual_frames),
        measure("buckled3000", *synthetic_tables(lambda **kw: synthetic.cg_buckled(n_lipids=3000, **kw), args.frames_large),
                args.frames_large, args.reps, 2),
    ]}
    print("CLUSTER_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--frames-large", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--manual-frames", type=int, default=16)
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--cutoff", action="store_true")
    args = ap.parse_args()
    if args.cutoff and args.out is None:
        args.out = os.path.join(ROOT, "profiles", "cluster_cutoff_bench.json")
    if args.child:
        return child_cutoff(args) if args.cutoff else child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    line = next((ln for ln in res.stdout.splitlines() if ln.startswith("CLUSTER_BENCH ")), None)
    if res.returncode != 0 or line is None:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        sys.exit(res.returncode or 1)
    line = line[len("CLUSTER_BENCH "):]
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
