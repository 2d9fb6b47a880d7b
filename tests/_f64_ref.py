"""Brute-force restatement of the ST-DBSCAN contract on float64 coordinates (numpy + scipy).

The contract of ``rpt_stdbscan_f64`` (csrc/stdbscan64.h), pinned to the reference's ``st_dbscan``
by tests/golden/make_f64_golden.py (every g15 case) and tests/test_stdbscan_f64_cpu.py:

* space: float64 ``d2 = ((xi-xj)^2 + (yi-yj)^2) [+ (zi-zj)^2]``, left to right, each operation
  rounded (numpy never fuses), ``<= eps_space^2``; no pair passes for a negative or NaN eps_space;
* time: ``|t_j - t_i| <= eps_time`` in the dtype of ``times`` -- float32 arithmetic against
  float32(eps_time) for float32 times (NEP 50), float64 for float64 and integer times;
* a point with a NaN or infinite time is nobody's neighbour, not even its own;
* core: at least min_samples neighbours, itself included; clusters are the components of the
  core-core graph numbered by their minimum core index; a border point takes the smallest
  adjacent id; noise is -1.
"""
from __future__ import annotations

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components


def adjacency(coords, times, eps_space: float, eps_time: float, chunk: int = 512) -> csr_matrix:
    """The neighbour relation as a boolean CSR matrix (row i: the neighbours of i)."""
    c = np.asarray(coords).astype(np.float64)
    t = np.asarray(times)
    n, dim = c.shape
    if t.dtype == np.float32:
        eps_t = np.float32(eps_time)
    else:
        t = t.astype(np.float64)
        eps_t = np.float64(eps_time)
    fin = np.isfinite(t)
    eps2 = np.float64(eps_space) * np.float64(eps_space)
    rows, cols = [], []
    if eps_space >= 0:  # (False for NaN)
        for a in range(0, n, chunk):
            b = min(a + chunk, n)
            with np.errstate(invalid="ignore", over="ignore"):
                dx = c[a:b, None, 0] - c[None, :, 0]
                dy = c[a:b, None, 1] - c[None, :, 1]
                d2 = dx * dx + dy * dy
                if dim == 3:
                    dz = c[a:b, None, 2] - c[None, :, 2]
                    d2 = d2 + dz * dz
                dt = np.abs(t[None, :] - t[a:b, None])
                ok = (d2 <= eps2) & (dt <= eps_t) & fin[None, :] & fin[a:b, None]
            r, k = np.nonzero(ok)
            rows.append(r + a)
            cols.append(k)
    if rows:
        rows = np.concatenate(rows)
        cols = np.concatenate(cols)
    else:
        rows = cols = np.zeros(0, np.int64)
    return csr_matrix((np.ones(len(rows), bool), (rows, cols)), shape=(n, n))


def labels_from_adjacency(adj: csr_matrix, min_samples: int) -> np.ndarray:
    n = adj.shape[0]
    counts = np.diff(adj.indptr)
    core = counts >= min_samples
    labels = np.full(n, -1, np.int32)
    idx = np.flatnonzero(core)
    if len(idx) == 0:
        return labels
    sub = adj[idx][:, idx]
    _, comp = connected_components(sub, directed=False)
    # number the components by their minimum core index: idx ascends, so by first appearance
    _, first = np.unique(comp, return_index=True)
    order = np.argsort(first)
    rank = np.empty(len(order), np.int32)
    rank[order] = np.arange(len(order), dtype=np.int32)
    labels[idx] = rank[comp]
    # border points: the smallest id among adjacent core points
    core_label = np.where(core, labels, np.iinfo(np.int32).max).astype(np.int64)
    for i in np.flatnonzero(~core):
        nb = adj.indices[adj.indptr[i]:adj.indptr[i + 1]]
        if len(nb):
            m = core_label[nb].min()
            if m != np.iinfo(np.int32).max:
                labels[i] = m
    return labels


def st_dbscan_ref(coords, times, eps_space: float, eps_time: float, min_samples: int) -> np.ndarray:
    return labels_from_adjacency(adjacency(coords, times, eps_space, eps_time), int(min_samples))


# ---- the grid rule of csrc/grid64.h, restated ---------------------------------------------------
GRID64_DOUBLINGS = 2200


def grid64_dim(ext: float, side: float) -> int:
    with np.errstate(all="ignore"):
        q = np.floor(np.float64(ext) / np.float64(side)) + 1.0
    if not q <= 1e9:
        return 1000000000
    return 1 if q < 1.0 else int(q)


def grid64_plan_py(lo, hi, n_finite_t: int, dim: int, eps_space: float, eps_time: float, n: int):
    """(lo[4], cs, ct, (nx, ny, nz, nt), cells, doublings, collapsed) by the rule of grid64.h."""
    margin = 1.0 + 2.0 ** -20
    floor_side = 2.0 ** -500
    lo = [float(v) for v in lo]
    with np.errstate(all="ignore"):
        ext = [float(np.float64(h) - np.float64(l)) for l, h in zip(lo, hi)]
    if dim != 3:
        lo[2], ext[2] = 0.0, 0.0
    if n_finite_t <= 0:
        lo[3], ext[3] = 0.0, 0.0
    with np.errstate(over="ignore"):
        cs = float(np.float64(max(eps_space, floor_side)) * margin) if eps_space > 0 else 1.0
        ct = float(np.float64(max(eps_time, floor_side)) * margin) if eps_time > 0 else 1.0
        if np.isinf(np.float64(eps_space) * np.float64(eps_space)):
            cs = float("inf")
    cmax = min(max(1 << 22, 4 * n), 1 << 30)
    fits, it = False, 0
    while True:
        nx, ny = grid64_dim(ext[0], cs), grid64_dim(ext[1], cs)
        nz = grid64_dim(ext[2], cs) if dim == 3 else 1
        nt = grid64_dim(ext[3], ct)
        if float(nx) * float(ny) * float(nz) * float(nt) <= float(cmax):
            fits = True
            break
        if it == GRID64_DOUBLINGS:
            break
        with np.errstate(over="ignore"):
            if float(nt) > float(nx) * float(ny) * float(nz):
                ct = float(np.float64(ct) * 2.0)
            else:
                cs = float(np.float64(cs) * 2.0)
        it += 1
    collapsed = 0
    if not fits:
        cs, nx, ny, nz, collapsed = float("inf"), 1, 1, 1, 1
        if nt > cmax:
            ct, nt, collapsed = float("inf"), 1, 3
    return lo, cs, ct, (nx, ny, nz, nt), nx * ny * nz * nt, it, collapsed


def grid64_index_py(v: float, lo: float, side: float, n: int) -> int:
    with np.errstate(all="ignore"):
        q = np.floor((np.float64(v) - np.float64(lo)) / np.float64(side))
    if not q >= 1.0:
        return 0
    return int(q) if q < n else n - 1


def grid64_of(coords, times, eps_space: float, eps_time: float):
    """The grid rpt_stdbscan_f64 builds for this input (eps_time as the kernel's time dtype
    rounds it): grid64_plan_py of its bounds."""
    c = np.asarray(coords).astype(np.float64)
    t = np.asarray(times)
    if t.dtype == np.float32:
        eps_time = float(np.float32(eps_time))
    t = t.astype(np.float64)
    tf = t[np.isfinite(t)]
    n, dim = c.shape
    lo = [c[:, k].min() for k in range(dim)] + [0.0] * (3 - dim) + [tf.min() if len(tf) else 0.0]
    hi = [c[:, k].max() for k in range(dim)] + [0.0] * (3 - dim) + [tf.max() if len(tf) else 0.0]
    return grid64_plan_py(lo, hi, len(tf), dim, eps_space, eps_time, n)
