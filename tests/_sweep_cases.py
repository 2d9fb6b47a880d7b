"""Inputs S1-S6 of the neighbour-count and min_samples-sweep tests, with their oracle results.

The generators are those of test_stdbscan_general_gpu.py (vol, planes), restated here so that no
test module imports another.  Every case carries the numbers the oracle gave when the case was
chosen; check_case() asserts them before a test makes its first device call, so a drift of the
generators (another numpy, another seed rule) shows as such and not as a device mismatch.
Oracle results are computed once per process and handed out read-only.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import oracle

SWEEP = (3, 10, 25, 60)


def vol(seed, n_blobs, per, noise, box, F, dim, jitter_t=0, spread=2.0, vel=1.0):
    """Moving Gaussian blobs plus uniform clutter, F frames, time = frame (+ jitter)."""
    rng = np.random.default_rng(seed)
    centres = rng.random((n_blobs, dim)) * box - box / 2
    vels = rng.normal(0, vel, (n_blobs, dim))
    pts, ts = [], []
    for f in range(F):
        for c, v in zip(centres, vels):
            m = int(rng.integers(per // 2, per * 2))
            pts.append(c + v * f + rng.normal(0, spread, (m, dim)))
            ts.append(np.full(m, f, np.float64))
        pts.append(rng.random((noise, dim)) * box * 1.2 - box * 0.6)
        ts.append(np.full(noise, f, np.float64))
    c = np.vstack(pts)
    t = np.concatenate(ts)
    if jitter_t:
        t = t + rng.random(len(t)) * jitter_t
    return c.astype(np.float32), t.astype(np.float32)


def planes(seed, noise, box, n_blobs, per, zs=(0, 250, 500)):
    """The stacked-gain PLY layout: the same 2-D blobs in the planes z = zs, time = gain index."""
    rng = np.random.default_rng(seed)
    centres = rng.random((n_blobs, 2)) * box - box / 2
    pts, ts = [], []
    for k, z in enumerate(zs):
        for c in centres:
            m = int(rng.integers(per // 2, per * 2))
            xy = c + rng.normal(0, 2, (m, 2))
            pts.append(np.column_stack([xy, np.full(m, float(z))]))
            ts.append(np.full(m, k, np.float64))
        xy = rng.random((noise, 2)) * box - box / 2
        pts.append(np.column_stack([xy, np.full(noise, float(z))]))
        ts.append(np.full(noise, k, np.float64))
    return np.vstack(pts).astype(np.float32), np.concatenate(ts).astype(np.float32)


# name: (input, (eps, eps_t), n, grid (nx, ny, nz, nt), cell-side doublings, occupied cells,
#        largest count, clusters at min_samples 3 / 10 / 25 / 60)
#   S1  the slab-sort grid with integral times, all-mutual cells
#   S2  generic (non-integral) time windows
#   S3  3-D
#   S4  36,172 occupied cells: more than a capped wave-per-cell grid holds (16,384), so the count
#       kernel strides; clutter, the median count is 1
#   S5  11-slab windows (eps_t = 5) and dense cells
#   S6  a grid coarsened twice: cells that are not mutual by their diagonal
CASES = {
    "S1": (lambda: vol(21, 12, 60, 300, 200.0, 8, dim=2), (5.0, 1.0),
           9489, (69, 69, 1, 8), 0, 3195, 332, (230, 11, 11, 11)),
    "S2": (lambda: vol(22, 12, 60, 300, 200.0, 8, dim=2, jitter_t=0.9), (5.0, 1.5),
           9420, (69, 69, 1, 6), 0, 2977, 350, (204, 8, 8, 9)),
    "S3": (lambda: vol(23, 12, 60, 300, 60.0, 6, dim=3), (5.0, 1.0),
           6767, (29, 29, 32, 6), 0, 4004, 277, (136, 8, 9, 9)),
    "S4": (lambda: vol(24, 10, 60, 6000, 1500.0, 6, dim=2), (5.0, 1.0),
           40151, (515, 515, 1, 6), 0, 36172, 283, (1196, 10, 10, 10)),
    "S5": (lambda: vol(25, 10, 60, 300, 150.0, 20, dim=2), (6.0, 5.0),
           21158, (43, 45, 1, 20), 0, 6889, 978, (1, 3, 6, 6)),
    "S6": (lambda: planes(31, 2000, 1000.0, 10, 200), (5.0, 1.0),
           13854, (100, 100, 50, 3), 2, 5554, 368, (65, 30, 30, 30)),
}


def grid(c, t, eps, et):
    """build_t's grid rule: (nx, ny, nz, nt), how often the cell side was doubled, and the number
    of occupied cells (cell index = floor((v - min) * (1 / side)), as cell_of computes it)."""
    n, dim = c.shape
    tf = t[np.isfinite(t)]
    integral = bool(np.all(tf == np.floor(tf)))
    margin = 1.0 + 2.0 ** -20
    cs = eps * (0.7 if dim == 2 else 0.5) * margin
    ct = 1.0 if integral else float(np.float32(et)) * margin
    cap = min(max(1 << 22, 4 * n), 1 << 30)
    lo = [float(c[:, k].min()) for k in range(dim)]
    ext = [float(c[:, k].max()) - lo[k] for k in range(dim)]
    t_lo = float(tf.min()) if len(tf) else 0.0
    ext_t = float(tf.max()) - t_lo if len(tf) else 0.0
    doubled = 0
    while True:
        d = [int(math.floor(e / cs)) + 1 for e in ext]
        nt = int(math.floor(ext_t / ct)) + 1
        cells = math.prod(d)
        if cells * nt <= cap:
            break
        if nt > cells:
            ct *= 2.0
        else:
            cs *= 2.0
            doubled += 1
    key = np.clip(np.floor((t.astype(np.float64) - t_lo) * (1.0 / ct)), 0, nt - 1)
    for k in reversed(range(dim)):
        idx = np.clip(np.floor((c[:, k].astype(np.float64) - lo[k]) * (1.0 / cs)), 0, d[k] - 1)
        key = key * d[k] + idx
    occupied = len(np.unique(key[np.isfinite(t)])) + int(np.any(~np.isfinite(t)))
    return tuple(d + [1] * (3 - dim) + [nt]), doubled, occupied


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def cloud(name):
    c, t = CASES[name][0]()
    assert c.dtype == np.float32 and t.dtype == np.float32
    return _frozen(c), _frozen(t)


@functools.lru_cache(maxsize=None)
def counts(name):
    """The oracle's exact neighbour counts of a case (self included)."""
    c, t = cloud(name)
    eps, et = CASES[name][1]
    return _frozen(oracle.neighbour_counts(c, t, eps, et))


@functools.lru_cache(maxsize=None)
def labels(name, m):
    """The oracle's BFS labels of a case at min_samples = m."""
    c, t = cloud(name)
    eps, et = CASES[name][1]
    return _frozen(oracle.stdbscan(c, t, eps, et, m))


@functools.lru_cache(maxsize=None)
def check_case(name, with_clusters=False):
    """The generator-drift guards of a case, on the oracle alone (no device call)."""
    _, (eps, et), n, dims, doubled, occupied, max_count, clusters = CASES[name]
    c, t = cloud(name)
    assert len(c) == len(t) == n, f"{name}: generator drift, n={len(c)}"
    got = grid(c, t, eps, et)
    assert got == (dims, doubled, occupied), f"{name}: grid {got}"
    assert int(counts(name).max()) == max_count, f"{name}: max count {int(counts(name).max())}"
    if with_clusters:
        ncl = tuple(int(labels(name, m).max()) + 1 for m in SWEEP)
        assert ncl == clusters, f"{name}: oracle clusters {ncl}"
    return True
