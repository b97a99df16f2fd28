#!/usr/bin/env python3
"""What spherical-clustering leaflets cost on a vesicle: python tools/vesicle_bench.py [--lipids N] [--frames F] [--reps R]

A CG vesicle (synthetic.cg_vesicle, 12-bead lipids) resident in HBM goes through the same frames four ways:
  (a) none            LEAFLETS_NONE
  (b) spherical       LEAFLETS_SPHERICAL assigned every frame (k_leaflets_spherical)
  (c) spherical_once  LEAFLETS_SPHERICAL assigned once
  (d) manual_host     LEAFLETS_MANUAL, the only route before the method existed: per assignment frame (every frame) the heads
                      are copied back, the flags computed on the host with numpy (the float32 statement of the method) and
                      pushed through set_manual_leaflets — a submit per frame
Times are host clocks around submits that end in a synchronise (median of the repetitions, the routes alternating); the
new kernel's time comes from gorder_hip_kernel_time_group.  The GPU work runs in a child process under a time limit; the
parent prints ONE JSON line (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_flags(heads_xyz, box):
    """The method on the host for one frame (float32 numpy; heads [n, 3]) -> flags [n] (0 = outer)."""
    import numpy as np
    f32 = np.float32
    th = heads_xyz * (f32(2 * np.pi) / box)
    est = (np.arctan2(-np.sin(th).sum(0), -np.cos(th).sum(0)) + f32(np.pi)) / (f32(2 * np.pi) / box)
    img = heads_xyz - box * np.round((heads_xyz - est) / box)
    centre = img.mean(0)
    v = img - centre
    x = np.sqrt((v * v).sum(1)).astype(f32)
    n = f32(x.size)
    srt = np.sort(x)
    var = max(f32(x.var(ddof=1)), f32(1e-6))
    w, ma, va, mb, vb = f32(0.5), srt[x.size // 4], var, srt[3 * x.size // 4], var
    ln2pi, prev = f32(np.log(2 * np.pi)), -np.inf
    iters = 0
    for _ in range(50):
        ja = np.log(w) - f32(0.5) * ((ln2pi + np.log(va)) + (x - ma) ** 2 / va)
        jb = np.log(f32(1) - w) - f32(0.5) * ((ln2pi + np.log(vb)) + (x - mb) ** 2 / vb)
        m = np.maximum(ja, jb)
        lpx = m + np.log(np.exp(ja - m) + np.exp(jb - m))
        r = np.exp(ja - lpx)
        iters += 1
        avg = lpx.sum() / n
        if abs(avg - prev) < 1e-4:
            break
        prev = avg
        sa = max(r.sum(), f32(1e-6))
        sb = max(n - r.sum(), f32(1e-6))
        w = min(max(sa / n, f32(1e-4)), f32(1 - 1e-4))
        ma, mb = (r * x).sum() / sa, ((1 - r) * x).sum() / sb
        va, vb = max((r * (x - ma) ** 2).sum() / sa, f32(1e-6)), max(((1 - r) * (x - mb) ** 2).sum() / sb, f32(1e-6))
    c1 = r < 0.5
    with np.errstate(all="ignore"):
        upper = c1 if x[c1].mean() > x[~c1].mean() else ~c1
    return np.where(upper, 0, 1).astype(np.uint8), iters


def child(args):
    import numpy as np
    import torch
    from gorder_amd import HipEngine, synthetic
    from gorder_amd.abi import LEAFLETS_MANUAL, LEAFLETS_NONE, LEAFLETS_SPHERICAL

    assert torch.cuda.is_available(), "vesicle_bench needs a GPU"
    n_out_r, n_in_r = args.outer, args.inner
    kw = dict(n_lipids=args.lipids, inner_radius=n_in_r, outer_radius=n_out_r, sigma=0.25, seed=5)
    systems = {
        "none": synthetic.cg_vesicle(leaflets=LEAFLETS_NONE, **kw)[0],
        "spherical": synthetic.cg_vesicle(leaflets=LEAFLETS_SPHERICAL, frequency=1, **kw)[0],
        "spherical_once": synthetic.cg_vesicle(leaflets=LEAFLETS_SPHERICAL, frequency=0, **kw)[0],
        "manual_host": synthetic.cg_vesicle(leaflets=LEAFLETS_MANUAL, **kw)[0],
    }
    ref = systems["spherical"]
    F = args.frames
    d_xyz, d_box = ref.frames_device(F, seed=1)
    heads = torch.from_numpy(np.asarray(ref.tables.leaflets.membrane, dtype=np.int64)).cuda()
    box = ref.box.astype(np.float32)
    engines = {k: HipEngine(s.tables) for k, s in systems.items()}
    for e in engines.values():
        e.use_torch_stream()
    n_manual = min(F, args.manual_frames)     # the host route is slow: it is timed on the first frames and scaled per frame

    def run(name):
        e = engines[name]
        e.reset()
        t0 = time.perf_counter()
        if name != "manual_host":
            e.submit_device(d_xyz, d_box)
            e.synchronize()
            return (time.perf_counter() - t0) / F
        for k in range(n_manual):
            hx = d_xyz[k].index_select(0, heads).cpu().numpy()          # this frame's heads copied back
            flags, _ = host_flags(hx, box)
            e.set_manual_leaflets(flags, k)
            e.submit_device(d_xyz[k:k + 1], d_box[k:k + 1], np.array([k]))
        e.synchronize()
        return (time.perf_counter() - t0) / n_manual

    order = ["none", "spherical", "spherical_once", "manual_host"]
    for name in order:                      # warm-up: code objects, allocations, clocks
        for _ in range(2):
            run(name)
    per_frame = {k: [] for k in order}
    for _ in range(args.reps):              # the routes alternate
        for name in order:
            per_frame[name].append(run(name))
    # flags of both routes agree (same method): the comparison is between equal results
    f_dev = engines["spherical"].leaflets()[0]
    f_host, _ = host_flags(d_xyz[F - 1].index_select(0, heads).cpu().numpy(), box)
    # the classifier kernel by itself: device time of its timing group over whole submits
    e = engines["spherical"]
    e.kernel_time(reset=True)
    for _ in range(args.reps):
        e.submit_device(d_xyz, d_box)
    e.synchronize()
    groups = {g: (ms, n) for g, ms, n in e.kernel_groups()}
    total_ms, submits = e.kernel_time(reset=True)
    k_ms, _ = groups["k_leaflets_spherical"]
    stats = e.spherical_stats()
    med = {k: float(np.median(v)) for k, v in per_frame.items()}
    out = {
        "tool": "tools/vesicle_bench.py", "device": torch.cuda.get_device_name(0),
        "lipids": args.lipids, "atoms_per_frame": ref.n_atoms, "heads": int(heads.numel()), "frames": F, "reps": args.reps,
        "inner_radius_nm": n_in_r, "outer_radius_nm": n_out_r,
        "frames_per_s": {k: 1.0 / v for k, v in med.items()},
        "seconds_per_frame_spread": {k: [float(min(v)), float(max(v))] for k, v in per_frame.items()},
        "manual_host_frames_timed": n_manual,
        "k_leaflets_spherical_ms_per_512_frames": k_ms / (submits * F) * 512.0,
        "device_ms_per_512_frames_all_kernels": total_ms / (submits * F) * 512.0,
        "classifier_share_of_device_step": k_ms / total_ms,
        "spherical_over_none": med["spherical"] / med["none"],
        "manual_host_over_spherical": med["manual_host"] / med["spherical"],
        "em_iterations_last_frame": stats["iterations"],
        "flags_device_equal_host_route": bool(np.array_equal(f_dev, f_host)),
    }
    print("VESICLE_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lipids", type=int, default=3000)
    ap.add_argument("--inner", type=float, default=6.0)
    ap.add_argument("--outer", type=float, default=10.0)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--manual-frames", type=int, default=256)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    line = next((ln for ln in res.stdout.splitlines() if ln.startswith("VESICLE_BENCH ")), None)
    if res.returncode != 0 or line is None:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        sys.exit(res.returncode or 1)
    line = line[len("VESICLE_BENCH "):]
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
