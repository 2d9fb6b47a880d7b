"""Inputs of the float64 ST-DBSCAN tests, shared by tests/golden/make_f64_golden.py (which runs
the reference on them), tests/test_stdbscan_f64_cpu.py and tests/test_stdbscan_f64_gpu.py.

Every array is built from integer draws of ``numpy.random.default_rng(seed)`` by a few exactly
rounded float64 operations, so the bytes are the same on every machine; g15 stores a sha256 of
each case's input bytes and the tests check it before they compare labels.
"""
from __future__ import annotations

import hashlib
from typing import Callable, Dict, NamedTuple

import numpy as np


class Case(NamedTuple):
    coords: np.ndarray
    times: np.ndarray
    eps_space: float
    eps_time: float
    min_samples: int
    discriminating: bool  # rounding the coordinates to float32 changes >= 100 labels
    route: str            # the precision st_dbscan must report for it


def digest(case: Case) -> str:
    h = hashlib.sha256()
    for a in (case.coords, case.times):
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    h.update(np.array([case.eps_space, case.eps_time], np.float64).tobytes())
    h.update(str(int(case.min_samples)).encode())
    return h.hexdigest()


# ---- generators -------------------------------------------------------------------------------
def lattice_side(eps: float, min_samples: int, n: int = 5000, frames: int = 3) -> int:
    """The lattice side at which a point has about min_samples neighbours in its own frame, so
    that the sites exactly eps away -- whose test is decided in the last bit -- decide who is
    core."""
    k = int(round(eps * 10))
    sites = sum(1 for a in range(-k, k + 1) for b in range(-k, k + 1) if a * a + b * b <= k * k)
    return int(round((sites * n / (frames * min_samples)) ** 0.5))


def lattice(seed: int, n: int = 5000, side: int = 98, offset: float = 0.0, frames: int = 3):
    """n random sites of a 0.1-spaced side x side lattice in `frames` integral frames (k * 0.1 is
    rarely a float32 value, and whether |a - b| <= 0.3 holds for sites three steps apart is
    decided in the last bit).  Meant for eps_time 0.5: neighbours share a frame."""
    rng = np.random.default_rng(seed)
    ij = rng.integers(0, side, size=(n, 2))
    t = rng.integers(0, frames, size=n)
    return ij.astype(np.float64) * 0.1 + offset, t.astype(np.float64)


def blobs(seed: int, n: int, dim: int, offset: float, n_blobs: int = 24, spread: int = 4000):
    """Blobs about 0.4 wide (sums of four uniform integer draws, in units of 2^-10) on centres a
    few units apart, offset far beyond float32's resolution at that magnitude; a sixth of the
    points are scattered."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, spread, size=(n_blobs, dim))
    which = rng.integers(0, n_blobs, size=n)
    jitter = rng.integers(0, 256, size=(n, dim, 4)).sum(axis=2) - 510
    q = centres[which] * 8 + jitter  # units of 2^-10... scaled below
    stray = rng.integers(0, 6, size=n) == 0
    q[stray] = rng.integers(0, spread * 8, size=(int(stray.sum()), dim))
    t = rng.integers(0, 4, size=n)
    return q.astype(np.float64) * (1.0 / 1024.0) + offset, t.astype(np.float64)


def _base_small(seed: int, n: int = 1500):
    """A small 2-D blob cloud on a 2^-10 grid (float32 values) for the dtype and edge cases."""
    c, t = blobs(seed, n, 2, 0.0, n_blobs=10, spread=1500)
    return c, t


def _cases() -> Dict[str, Callable[[], Case]]:
    d: Dict[str, Callable[[], Case]] = {}

    def add(name, fn):
        d[name] = fn

    # the 0.1 lattice
    for eps in (0.3, 0.5):
        for off in (0.0, 77.7):
            def f(eps=eps, off=off):
                c, t = lattice(11 + int(eps * 10) + int(off), side=lattice_side(eps, 5),
                               offset=off)
                return Case(c, t, eps, 0.5, 5, True, "float64")
            add(f"lattice_eps{eps}_off{off}", f)

    # blobs far from the origin
    for dim in (2, 3):
        for off in (4e6, 1e7):
            def f(dim=dim, off=off):
                c, t = blobs(100 + dim + int(off // 1e6), 4000, dim, off)
                return Case(c, t, 0.1 if dim == 2 else 0.15, 1.0, 5, True, "float64")
            add(f"blobs{dim}d_off{off:g}", f)

    def decimal_times():
        c, _ = lattice(31, n=3000, side=100)
        t = np.random.default_rng(32).integers(0, 12, size=3000).astype(np.float64) * 0.1
        return Case(c, t, 0.3, 0.3, 5, True, "float64")
    add("decimal_times", decimal_times)

    def epoch_f64():
        c, _ = _base_small(41)
        k = np.random.default_rng(42).integers(0, 40, size=len(c))
        return Case(c, 1.7e9 + k.astype(np.float64) * 0.25, 0.12, 0.5, 4, False, "float64")
    add("epoch_times_f64", epoch_f64)

    def epoch_i64():
        c, _ = _base_small(43)
        k = np.random.default_rng(44).integers(0, 8, size=len(c))
        return Case(c, (1_700_000_000 + k).astype(np.int64), 0.12, 1.5, 4, False, "float64")
    add("epoch_times_i64", epoch_i64)

    def f64_coords_f32_times():
        c, _ = lattice(51, n=3000, side=100)
        k =np.random.default_rng(52).integers(0, 12, size=3000)
        return Case(c, (k.astype(np.float32) * np.float32(0.1)), 0.3, 0.3, 5, True, "float64")
    add("f64_coords_f32_times", f64_coords_f32_times)

    def f32_coords_f64_times():
        c, _ = _base_small(53)
        k = np.random.default_rng(54).integers(0, 12, size=len(c))
        return Case(c.astype(np.float32), k.astype(np.float64) * 0.1, 0.12, 0.3, 4, False,
                    "float64")
    add("f32_coords_f64_times", f32_coords_f64_times)

    def int64_coords():
        rng = np.random.default_rng(61)
        centres = rng.integers(0, 4000, size=(12, 2))
        c = (1 << 25) + 1 + centres[rng.integers(0, 12, size=2000)] + \
            rng.integers(-6, 7, size=(2000, 2))
        t = rng.integers(0, 3, size=2000)
        return Case(c.astype(np.int64), t.astype(np.float32), 2.0, 1.0, 5, True, "float64")
    add("int64_coords", int64_coords)

    def nonfinite_times():
        c, t = lattice(71, n=3000, side=76)
        r = np.random.default_rng(72).integers(0, 60, size=3000)
        t = t.copy()
        t[r == 0] = np.nan
        t[r == 1] = np.inf
        t[r == 2] = -np.inf
        return Case(c, t, 0.3, 0.5, 5, False, "float64")
    add("nonfinite_times", nonfinite_times)

    # degenerate and extreme parameters on one decimal cloud
    def param(eps_space=0.3, eps_time=1.0, ms=5):
        def f():
            c, t = lattice(81, n=1500, side=60)
            m = len(c) + 1 if ms == "n+1" else ms
            return Case(c, t, eps_space, eps_time, m, False, "float64")
        return f
    add("eps_space_0", param(eps_space=0.0, ms=2))
    add("eps_space_neg", param(eps_space=-1.0))
    add("eps_space_nan", param(eps_space=float("nan")))
    add("eps_space_neg_ms0", param(eps_space=-1.0, ms=0))
    add("eps_time_0", param(eps_time=0.0))
    add("eps_time_neg", param(eps_time=-1.0))
    add("eps_time_inf", param(eps_time=float("inf")))
    add("min_samples_0", param(ms=0))
    add("min_samples_1", param(ms=1))
    add("min_samples_n_plus_1", param(ms="n+1"))

    add("n_1", lambda: Case(np.array([[0.1, 0.7]]), np.array([1.7e9 + 0.5]), 0.3, 1.0, 1, False,
                            "float64"))
    add("all_identical", lambda: Case(np.full((300, 3), 0.1) + 4e6,
                                      np.full(300, 0.3), 0.3, 0.5, 5, False, "float64"))
    return d


CASES = _cases()


def round_coords_f32(case: Case) -> Case:
    return case._replace(coords=np.asarray(case.coords).astype(np.float32).astype(np.float64))


# ---- the at-size clouds: float32 values on a 2^-13 grid, |x| < 1024, times on a 2^-10 grid -----
def quantised_cloud(seed: int, n: int, dim: int, extent, n_blobs: int, blob_w: int,
                    t_steps: int, t_quant: int = 1024, stray_one_in: int = 5):
    """n points of `dim` coordinates in [0, extent[k]) as float32 multiples of 2^-13: blobs of
    width ~blob_w / 8192 and scattered points; times k / t_quant for k < t_steps (float32)."""
    rng = np.random.default_rng(seed)
    ext = np.asarray(extent, np.int64) * 8192
    centres = np.stack([rng.integers(0, ext[k], size=n_blobs) for k in range(dim)], axis=1)
    which = rng.integers(0, n_blobs, size=n)
    q = centres[which] + rng.integers(0, blob_w, size=(n, dim, 2)).sum(axis=2) - blob_w
    stray = rng.integers(0, stray_one_in, size=n) == 0
    m = int(stray.sum())
    q[stray] = np.stack([rng.integers(0, ext[k], size=m) for k in range(dim)], axis=1)
    q = np.clip(q, 0, ext[None, :] - 1)
    x = (q.astype(np.float64) / 8192.0).astype(np.float32)
    t = (rng.integers(0, t_steps, size=n).astype(np.float64) / t_quant).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * 8192, q)
    return x, t
