"""CPU statement of spectral-clustering leaflets (GORDER_LEAFLETS_CLUSTERING) — TEST HELPER, numpy only.

Restates the precise route of the reference's `SystemClusterClassification` (src/analysis/clustering.rs:478-800) as the
device defines it (include/gorder_hip.h): W_ij = exp(-d_ij^2) over the group "ClusterHeads" (3-D minimum image with a
box), deg = W 1, S = D^-1/2 W D^-1/2, L = I - S.  "Skip the first" is exact: q = D^1/2 1 is projected out and the two
largest eigenpairs of S on q's complement are taken (dense `eigh` of P S P); rows normalised; the literal 2-means
(clustering.rs:614-696); ab-initio orientation or the match against the previous frame's clusters (clustering.rs:731-800).

Two twins of one function: dtype float32 and float64 — the same statements with every array in that type.
"""
from __future__ import annotations

import json
import os

import numpy as np

SIGMA = 1.0                  # PRECISE_SIGMA
LIMIT = np.float32(0.8)      # CLUSTER_CLASSIFICATION_LIMIT
MIN_GROUP = 2                # leaflets.rs:96-105, behind test_cg_order_leaflets_clustering_fail_not_enough_atoms
MAX_GROUP = 8192             # the device's documented bound (kClMaxGroup)
KAT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spectral_kat.json")

# the buckled membrane of the tests: synthetic.cg_buckled(**BUCKLED).  Amplitude 3 nm over a half thickness of 2 nm: upper
# heads in the trough lie 1 nm below the mean plane, so a plane misplaces them.
BUCKLED = dict(n_lipids=500, box=(20.0, 8.0, 16.0), amplitude=3.0, seed=13)


def min_image(dx, L):
    """groan_rs minimum image of displacements dx in a box edge L (the `while` loops, at most 8 shifts)."""
    half = L / dx.dtype.type(2)
    for _ in range(8):
        dx = np.where(dx > half, dx - L, dx)
    for _ in range(8):
        dx = np.where(dx < -half, dx + L, dx)
    return dx


def box3(box):
    if box is None:
        return None
    b = np.asarray(box, dtype=np.float32).reshape(-1)
    return b[[0, 4, 8]] if b.size == 9 else b


def similarity(pos, box, pbc, dtype):
    """W [n, n] in dtype."""
    p = np.asarray(pos, dtype=np.float32).astype(dtype)
    d2 = np.zeros((len(p), len(p)), dtype=dtype)
    for d in range(3):
        v = p[:, None, d] - p[None, :, d]
        if pbc:
            v = min_image(v, dtype(box3(box)[d]))
        d2 = d2 + v * v if d else v * v
    return np.exp(-dtype(SIGMA) * d2).astype(dtype)


def embedding(pos, box, pbc, dtype=np.float32):
    """-> (rows [n, 2] normalised, eigenvalues 2, 3, 4 of L [3] (NaN where the group is too small))."""
    W = similarity(pos, box, pbc, dtype)
    n = len(W)
    deg = W.sum(axis=1, dtype=dtype)
    s = np.where(deg > dtype(1e-10), dtype(1) / np.sqrt(deg), dtype(0)).astype(dtype)
    S = (s[:, None] * W * s[None, :]).astype(dtype)
    q = np.sqrt(deg).astype(dtype)
    q = q / np.sqrt((q * q).sum(dtype=dtype))
    P = np.eye(n, dtype=dtype) - np.outer(q, q)
    M = (P @ S @ P).astype(dtype)
    M = (M + M.T) / dtype(2)
    val, vec = np.linalg.eigh(M)
    eig = np.full(3, np.nan, dtype=np.float64)
    for k in range(min(3, n - 1)):
        eig[k] = 1.0 - float(val[n - 1 - k])
    rows = np.zeros((n, 2), dtype=dtype)
    rows[:, 0] = vec[:, n - 1]
    if n - 1 >= 2:
        rows[:, 1] = vec[:, n - 2]
    if rows[0, 0] < 0:
        rows[:, 0] = -rows[:, 0]
    norm = np.sqrt(rows[:, 0] * rows[:, 0] + rows[:, 1] * rows[:, 1])
    ok = norm > dtype(1e-10)
    rows[ok] = rows[ok] / norm[ok, None]
    return rows, eig


def k_means(rows, dtype=np.float32):
    """clustering.rs:614-696 with k = 2 -> (labels [n], rounds): centroids start as rows 0 and 1, at most 100 rounds, a row
    goes to the strictly nearer centroid (tie: 0), stop when no label changed, an empty cluster takes row 0."""
    x = np.asarray(rows, dtype=dtype)
    cen = x[:2].copy()
    prev = np.full(len(x), -1)
    labels = np.zeros(len(x), dtype=np.int64)
    rounds = 0
    for _ in range(100):
        d = np.stack([np.sqrt(((x - cen[c]) ** 2).sum(axis=1, dtype=dtype)) for c in (0, 1)], axis=1)
        labels = np.where(d[:, 1] < d[:, 0], 1, 0)
        rounds += 1
        if np.array_equal(labels, prev):
            break
        for c in (0, 1):
            cen[c] = x[labels == c].sum(axis=0, dtype=dtype) / dtype((labels == c).sum()) if (labels == c).any() else x[0]
        prev = labels.copy()
    return labels, rounds


def classify_ab_initio(cluster1, cluster2, min_index_cluster):
    """Clusters::classify_ab_initio -> (upper, lower): the more populated cluster is upper; a tie: the cluster that holds
    the atom with the lowest index (min_index_cluster: 0 = cluster1)."""
    c1, c2 = set(cluster1), set(cluster2)
    if len(c1) < len(c2):
        return c2, c1
    if len(c1) > len(c2):
        return c1, c2
    return (c1, c2) if min_index_cluster == 0 else (c2, c1)


def overlaps(ref_upper, ref_lower, cluster1):
    c1 = set(cluster1)
    with np.errstate(all="ignore"):
        n = np.float32(len(c1))
        return np.float32(len(c1 & set(ref_upper))) / n, np.float32(len(c1 & set(ref_lower))) / n


def classify_by_match(ref_upper, ref_lower, cluster1, cluster2):
    """Clusters::classify_by_match -> (upper, lower) or None (CouldNotMatchLeaflets)."""
    o_up, o_lo = overlaps(ref_upper, ref_lower, cluster1)
    if o_up < LIMIT and o_lo < LIMIT:
        return None
    if o_up < o_lo:
        return set(cluster2), set(cluster1)
    return set(cluster1), set(cluster2)


class MatchError(Exception):
    pass


def classify(frame, group, box, pbc=True, dtype=np.float32, prev_upper=None):
    """One assignment frame -> dict.  prev_upper None: frame 0, ab initio; else bool [n], the previous frame's upper leaflet.
    upper [n] bool, labels, rounds, eig [3], rows [n, 2], n_cluster (|c1|, |c2|), o_up, o_lo."""
    group = np.asarray(group, dtype=np.uint32)
    pos = np.asarray(frame, dtype=np.float32)[group]
    rows, eig = embedding(pos, box, pbc, dtype)
    labels, rounds = k_means(rows, dtype)
    c1, c2 = set(np.flatnonzero(labels == 0)), set(np.flatnonzero(labels == 1))
    o_up = o_lo = np.float32(np.nan)
    if prev_upper is None:
        upper, _ = classify_ab_initio(c1, c2, int(labels[0]))
    else:
        ru, rl = set(np.flatnonzero(prev_upper)), set(np.flatnonzero(~np.asarray(prev_upper)))
        o_up, o_lo = overlaps(ru, rl, c1)
        got = classify_by_match(ru, rl, c1, c2)
        if got is None:
            raise MatchError((float(o_up), float(o_lo)))
        upper = got[0]
    up = np.zeros(len(group), dtype=bool)
    up[sorted(upper)] = True
    return {"upper": up, "labels": labels, "rounds": rounds, "eig": eig, "rows": rows, "n_cluster": (len(c1), len(c2)),
            "o_up": o_up, "o_lo": o_lo}


def head_slots(tables):
    group = np.asarray(tables.leaflets.membrane, dtype=np.uint32)
    slot = {int(a): k for k, a in enumerate(group)}
    heads = np.concatenate([np.asarray(m.heads, dtype=np.uint32) for m in tables.molecule_types])
    return np.array([slot[int(h)] for h in heads])


def molecule_flags(tables, res):
    """Leaflet flags per molecule (Upper = 0, Lower = 1, flip applied), molecule type major."""
    flags = np.where(res["upper"][head_slots(tables)], 0, 1).astype(np.uint8)
    return flags ^ np.uint8(1 if tables.leaflets.flip else 0)


def run(tables, xyz, box, frame_index, dtype=np.float32):
    """The assignment frames among frame_index in order -> {frame: result of classify}, each matched against its predecessor."""
    out = {}
    prev = None
    f = int(tables.leaflets.frequency)
    for k, fi in enumerate(frame_index):
        fi = int(fi)
        if (fi == 0) if f == 0 else (fi % f == 0):
            res = classify(xyz[k], tables.leaflets.membrane, None if box is None else box[k], tables.handle_pbc, dtype,
                           None if fi == 0 else prev)
            prev = res["upper"]
            out[fi] = res
    return out


def load_kat():
    with open(KAT_PATH) as fh:
        return json.load(fh)
