#!/usr/bin/env python3
"""Order by local composition against the only other way to get it.
python tools/neighbour_classes_bench.py [--systems aa,cg] [--frames 4000] [--reps 5] [--out profiles/neighbour_classes_bench.json]

Systems, --frames frames resident in device memory, 8 classes:
  aa   V-AA (synthetic.aa_membrane(): 256 lipids, 64 accumulators): centres = the first atom of every lipid, neighbours = the
       first atom of every other lipid (128 atoms), radius 1.5 nm
  cg   the coarse-grained membrane in three molecule types (synthetic.cg_membrane(n_types=3): 3072 lipids, 33 accumulators):
       centres = every lipid's head bead, neighbours = the heads of one type (1024 atoms), radius 1.0 nm
One process runs, alternating, after a warm-up of each:
  (a) plain   no classes: k_bonds_tiled, the floor
  (b) lds     set_neighbour_classes: k_neighbour_counts + k_bonds_classes with its LDS table, and neighbour_classes() to the host
  (b') direct the same with GORDER_HIP_NB_DIRECT=1: global atomics per sample
  (c) host    the route this replaces: molecule rows with one group per molecule type read to the host, the frames copied to
              the host, the neighbour count per frame on the host — scipy.spatial.cKDTree with `boxsize` finds the candidate
              pairs within a slightly larger radius where scipy imports (numpy over all pairs where it does not), numpy float32
              decides them with the device's arithmetic, so that the integers can be compared — then numpy.add.at per class
A time is a host clock around submit_device + the route's read-out of an already created handle that was reset before; the
median of --reps is reported with the spread and the device time of every kernel group (gorder_hip_kernel_time_group).
(b) and (b') must give the same integers, (b) summed over a type's slots must equal (c), (b)'s finish() must equal (a)'s, and
(b) must be faster than (c): the run ends with a non-zero status where one of them does not hold.  The GPU work runs in a
child process under a time limit; the parent prints ONE JSON line (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_CLASSES = 8


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


def host_counts(xyz, box, centres, neighbours, radius, thr, tree_cls):
    """uint8 [frames, molecules]: the neighbour count of every (frame, molecule) on the host, the device's float32 arithmetic."""
    import numpy as np
    f32 = np.float32
    L, half = box.astype(f32), box.astype(f32) / f32(2.0)
    out = np.zeros((len(xyz), len(centres)), dtype=np.int64)
    other_all = centres[:, None] != neighbours[None, :]
    for f in range(len(xyz)):
        c, q = xyz[f, centres], xyz[f, neighbours]
        if tree_cls is not None:
            # candidates within a slightly larger radius in float64, on coordinates folded into [0, box)
            fold = lambda p: np.mod(p.astype(np.float64), box.astype(np.float64))
            pairs = tree_cls(fold(c), boxsize=box.astype(np.float64)).sparse_distance_matrix(
                tree_cls(fold(q), boxsize=box.astype(np.float64)), radius * 1.001, output_type="ndarray")
            i, j = pairs["i"], pairs["j"]
            d = q[j] - c[i]
            other = centres[i] != neighbours[j]
        else:
            d = q[None, :, :] - c[:, None, :]
        d = np.where(np.abs(d) > half, d - np.copysign(L, d), d).astype(f32)
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        if tree_cls is not None:
            np.add.at(out[f], i[(d2 < thr) & other], 1)
        else:
            out[f] = ((d2 < thr) & other_all).sum(axis=1)
    return out


def bench_system(name, args):
    import numpy as np
    from gorder_amd import HipEngine, abi, synthetic
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None

    if name == "aa":
        system = synthetic.aa_membrane()
        n_mol = system.tables.n_molecules_total
        centres = (np.arange(n_mol) * (system.tables.n_atoms // n_mol)).astype(np.uint32)
        neighbours, radius = centres[::2].copy(), 1.5
    else:
        system = synthetic.cg_membrane(n_types=3)
        lipids = np.arange(system.tables.n_atoms // 12)
        centres = np.concatenate([lipids[lipids % 3 == ty] * 12 + 1 for ty in range(3)]).astype(np.uint32)
        neighbours, radius = np.sort(lipids[lipids % 3 == 1] * 12 + 1).astype(np.uint32), 1.0
    t = system.tables
    thr = abi.radial_thresholds([radius])[0]
    groups, s0 = [], 0      # one group per molecule type: all its slots
    for mt in t.molecule_types:
        groups.append(list(range(s0, s0 + mt.n_bond_types)))
        s0 += mt.n_bond_types
    d_xyz, d_box = system.frames_device(args.frames, seed=1000)
    fi = np.arange(args.frames)
    box = np.asarray(system.box, dtype=np.float32)

    def with_classes(env):
        def make():
            e = HipEngine(t)
            e.set_neighbour_classes(centres, neighbours, radius, N_CLASSES)
            return e
        return engine_with(env, make)

    def with_rows():
        e = HipEngine(t)
        e.set_molecule_rows(groups)
        return e

    routes = {"plain": HipEngine(t), "lds": with_classes({}), "direct": with_classes({"GORDER_HIP_NB_DIRECT": "1"}), "host": with_rows()}
    out = {}

    def host_route(e):
        sums, counts, frames = e.molecule_rows()                # [frames, groups, molecules]
        xyz = d_xyz.cpu().numpy()                               # the frames, copied to the host
        cls = np.minimum(host_counts(xyz, box, centres, neighbours, radius, thr, cKDTree), N_CLASSES - 1)
        got_s = np.zeros((N_CLASSES, len(groups)), dtype=np.int64)
        got_c = np.zeros((N_CLASSES, len(groups)), dtype=np.int64)
        for g in range(len(groups)):
            np.add.at(got_s[:, g], cls, sums[:, g, :].astype(np.int64))
            np.add.at(got_c[:, g], cls, counts[:, g, :].astype(np.int64))
        return got_s, got_c

    def read(route, e):
        if route == "host":
            out[route] = host_route(e)
        elif route == "plain":
            e.synchronize()
        else:
            res = e.neighbour_classes()
            out[route] = (np.array([r.sums for r in res]), np.array([r.counts for r in res]))

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
    lds_s, lds_c = out["lds"]
    routes_agree = bool((lds_s == out["direct"][0]).all() and (lds_c == out["direct"][1]).all())
    by_type_s = np.stack([lds_s[:, 0, g].sum(axis=1) for g in groups], axis=1)
    by_type_c = np.stack([lds_c[:, 0, g].sum(axis=1).astype(np.int64) for g in groups], axis=1)
    host_agrees = bool((by_type_s == out["host"][0]).all() and (by_type_c == out["host"][1]).all())
    a, b = routes["plain"].finish(), routes["lds"].finish()
    totals_agree = bool((a.sums == b.sums).all() and (a.counts == b.counts).all() and (lds_s.sum(axis=0) == a.sums).all()
                        and (lds_c.sum(axis=0) == a.counts).all())
    samples_per_class = [int(x) for x in lds_c[:, 0].sum(axis=1)]
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
        groups_ = {g: ms_ for g, ms_, _ in e.kernel_groups()}
        e.kernel_time(reset=True)
        return groups_

    kernels = {}
    for route, e in routes.items():
        kernel_ms(e)                                          # warm-up
        runs = [kernel_ms(e) for _ in range(3)]
        kernels[route] = {g: min(r[g] for r in runs) for g in runs[0]}
    med = {k: float(np.median(v)) for k, v in times.items()}
    n_pairs = int(len(centres)) * int(len(neighbours))
    counts_ms = kernels["lds"]["k_neighbour_counts"]
    rows_bytes = int(2 * args.frames * len(groups) * t.n_molecules_total * 4)
    return {"system": system.name, "n_molecules": int(t.n_molecules_total), "n_types": len(t.molecule_types), "n_acc": int(t.n_acc),
            "n_neighbours": int(len(neighbours)), "radius": radius, "classes": N_CLASSES, "samples_per_class": samples_per_class,
            "samples_per_frame": int(t.n_samples_per_frame), "n_tiles": int(routes["lds"].plan()["n_tiles"]),
            "host_neighbour_search": "scipy.spatial.cKDTree" if cKDTree is not None else "numpy, all pairs",
            "lds_and_direct_agree": routes_agree, "lds_agrees_with_host": host_agrees, "finish_agrees_with_plain": totals_agree,
            "seconds_median": med, "seconds_spread": {k: [float(min(v)), float(max(v))] for k, v in times.items()},
            "frames_per_second": {k: float(args.frames / v) for k, v in med.items()},
            "kernel_ms": kernels,
            "pairs_per_frame": n_pairs, "k_neighbour_counts_pairs_per_second": float(n_pairs * args.frames / (counts_ms * 1e-3)),
            "bytes_to_host": {"plain": 0, "lds": int(N_CLASSES * 3 * t.n_acc * 16), "direct": int(N_CLASSES * 3 * t.n_acc * 16),
                              "host": rows_bytes + int(args.frames * t.n_atoms * 12)},
            "lds_over_plain": med["lds"] / med["plain"], "direct_over_lds": med["direct"] / med["lds"],
            "host_over_lds": med["host"] / med["lds"], "lds_faster_than_host": bool(med["lds"] < med["host"])}


def child(args):
    import torch

    assert torch.cuda.is_available(), "neighbour_classes_bench needs a GPU"
    out = {"tool": "tools/neighbour_classes_bench.py", "device": torch.cuda.get_device_name(0), "frames": args.frames, "reps": args.reps,
           "systems": {name: bench_system(name, args) for name in args.systems.split(",")}}
    print("NEIGHBOUR_CLASSES_BENCH " + json.dumps(out))
    failed = [f"{name}: {key}" for name, r in out["systems"].items()
              for key in ("lds_and_direct_agree", "lds_agrees_with_host", "finish_agrees_with_plain", "lds_faster_than_host") if not r[key]]
    if failed:
        sys.stderr.write("neighbour_classes_bench: FAILED " + ", ".join(failed) + "\n")
        sys.exit(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="aa,cg")
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=1100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    line = next((ln for ln in res.stdout.splitlines() if ln.startswith("NEIGHBOUR_CLASSES_BENCH ")), None)
    if line is None:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        sys.exit(res.returncode or 1)
    sys.stderr.write(res.stderr[-2000:])
    line = line[len("NEIGHBOUR_CLASSES_BENCH "):]
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(json.loads(line), indent=1) + "\n")
    sys.exit(res.returncode)      # not 0 where the routes disagree or (b) is not faster than (c): the figures are kept all the same


if __name__ == "__main__":
    main()
