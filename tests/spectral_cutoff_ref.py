"""CPU statement of the cut-off route of spectral-clustering leaflets (GORDER_FLAG_CLUSTER_CUTOFF) — TEST HELPER.

The definition of tests/spectral_ref.py with W_ij = exp(-d_ij^2) kept only where d_ij^2 < 36 nm^2 (d_ij the one minimum
image of the pair) and 0 elsewhere; everything behind W is spectral_ref's.  Two statements of it:
  classify(...)         dense (numpy `eigh`), for groups spectral_ref itself can hold: comparable with spectral_ref.classify
  classify_sparse(...)  float64, W in CSR built a block of rows at a time, the two largest eigenpairs of S on the complement
                        of q = D^1/2 1 by scipy's `eigsh` on the deflated operator: for groups above spectral_ref.MAX_GROUP
"""
from __future__ import annotations

import numpy as np

import spectral_ref as sr

CUTOFF2 = 36.0               # r_c^2, nm^2: the reference's cut-off distance of 6 nm
MAX_GROUP = 131072           # the device's bound with the flag (kClCutMaxGroup)


def distances2(p, rows, box, pbc, dtype):
    """d^2 [len(rows), n] of the rows' atoms to all atoms, spectral_ref.similarity's statements."""
    d2 = None
    for d in range(3):
        v = p[rows, None, d] - p[None, :, d]
        if pbc:
            v = sr.min_image(v, dtype(sr.box3(box)[d]))
        d2 = v * v if d2 is None else d2 + v * v
    return d2


def similarity(pos, box, pbc, dtype):
    """W [n, n] in dtype with the cut-off."""
    p = np.asarray(pos, dtype=np.float32).astype(dtype)
    d2 = distances2(p, np.arange(len(p)), box, pbc, dtype)
    return np.where(d2 < dtype(CUTOFF2), np.exp(-dtype(sr.SIGMA) * d2), dtype(0)).astype(dtype)


def embedding(pos, box, pbc, dtype=np.float32):
    """spectral_ref.embedding on the truncated W."""
    keep = sr.similarity
    sr.similarity = similarity
    try:
        return sr.embedding(pos, box, pbc, dtype)
    finally:
        sr.similarity = keep


def classify(frame, group, box, pbc=True, dtype=np.float32, prev_upper=None):
    """spectral_ref.classify on the truncated W (same keys)."""
    keep = sr.similarity
    sr.similarity = similarity
    try:
        return sr.classify(frame, group, box, pbc, dtype, prev_upper)
    finally:
        sr.similarity = keep


def sparse_similarity(pos, box, pbc, block=256):
    """W in CSR, float64, built `block` rows at a time."""
    import scipy.sparse as sp
    p = np.asarray(pos, dtype=np.float32).astype(np.float64)
    n = len(p)
    data, rows_of, cols = [], [], []
    for r0 in range(0, n, block):
        rows = np.arange(r0, min(r0 + block, n))
        d2 = distances2(p, rows, box, pbc, np.float64)
        r, j = np.nonzero(d2 < CUTOFF2)
        rows_of.append(r + r0)
        cols.append(j)
        data.append(np.exp(-sr.SIGMA * d2[r, j]))
    return sp.csr_matrix((np.concatenate(data), (np.concatenate(rows_of), np.concatenate(cols))), shape=(n, n))


def classify_sparse(frame, group, box, pbc=True):
    """One frame, ab initio, float64 -> dict(upper [n] bool, labels, rounds, eig [3] of L, n_cluster)."""
    from scipy.sparse.linalg import LinearOperator, eigsh
    group = np.asarray(group, dtype=np.uint32)
    W = sparse_similarity(np.asarray(frame, dtype=np.float32)[group], box, pbc)
    n = W.shape[0]
    deg = np.asarray(W.sum(axis=1)).reshape(-1)
    s = np.where(deg > 1e-10, 1.0 / np.sqrt(deg), 0.0)
    q = np.sqrt(deg)
    q /= np.sqrt((q * q).sum())

    def apply(v):
        v = np.asarray(v, dtype=np.float64).reshape(-1)
        v = v - q * (q @ v)
        w = s * (W @ (s * v))
        return w - q * (q @ w)
    rng = np.random.default_rng(0)
    val, vec = eigsh(LinearOperator((n, n), matvec=apply, dtype=np.float64), k=3, which="LA", v0=rng.normal(size=n), ncv=64, tol=1e-9)
    order = np.argsort(-val)
    eig = 1.0 - val[order]
    rows = vec[:, order[:2]].copy()
    if rows[0, 0] < 0:
        rows[:, 0] = -rows[:, 0]
    norm = np.sqrt((rows * rows).sum(axis=1))
    ok = norm > 1e-10
    rows[ok] = rows[ok] / norm[ok, None]
    labels, rounds = sr.k_means(rows, np.float64)
    c1, c2 = set(np.flatnonzero(labels == 0)), set(np.flatnonzero(labels == 1))
    upper, _ = sr.classify_ab_initio(c1, c2, int(labels[0]))
    up = np.zeros(n, dtype=bool)
    up[sorted(upper)] = True
    return {"upper": up, "labels": labels, "rounds": rounds, "eig": eig, "n_cluster": (len(c1), len(c2))}
