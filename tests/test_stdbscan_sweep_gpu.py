"""rpt.processors.st_dbscan_sweep (rpt_stdbscan_sweep: one grid build and one exact count pass,
then core flags from the counts, the union and the labels per min_samples) on the cases S1-S6
of _sweep_cases.py at min_samples 3, 10, 25 and 60: every row against the oracle's BFS labels
(the same ids) and against st_dbscan, the per-set statistics against the oracle's counts.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import _sweep_cases as sc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _sweep(name):
    """One device sweep of a case over sc.SWEEP, shared by the tests that read it."""
    from rpt.processors import st_dbscan_sweep

    sc.check_case(name, True)
    c, t = sc.cloud(name)
    eps, et = sc.CASES[name][1]
    stats = {}
    rows = st_dbscan_sweep(c, t, eps, et, sc.SWEEP, stats=stats)
    rows.setflags(write=False)
    return rows, stats


@pytest.mark.parametrize("name", list(sc.CASES))
def test_rows_match_oracle(gpu, name):
    rows, _ = _sweep(name)
    c, _ = sc.cloud(name)
    assert rows.dtype == np.int32 and rows.shape == (len(sc.SWEEP), len(c))
    for k, m in enumerate(sc.SWEEP):
        exp = sc.labels(name, m)
        print(f"{name} m={m}: clusters={int(rows[k].max()) + 1} "
              f"differ={int((rows[k] != exp).sum())}")
        assert np.array_equal(rows[k], exp), f"{name}: row {k} (min_samples {m})"


@pytest.mark.parametrize("name", list(sc.CASES))
def test_rows_match_st_dbscan(gpu, name):
    from rpt.processors import st_dbscan

    rows, _ = _sweep(name)
    c, t = sc.cloud(name)
    eps, et = sc.CASES[name][1]
    for k, m in enumerate(sc.SWEEP):
        assert np.array_equal(rows[k], st_dbscan(c, t, eps, et, m)), f"{name}: min_samples {m}"


@pytest.mark.parametrize("name", list(sc.CASES))
def test_stats_per_set(gpu, name):
    rows, stats = _sweep(name)
    cnt = sc.counts(name)
    _, _, _, dims, _, _, _, clusters = sc.CASES[name]
    assert stats["min_samples"] == list(sc.SWEEP)
    assert stats["n_core"] == [int((cnt >= m).sum()) for m in sc.SWEEP]
    assert tuple(stats["n_clusters"]) == clusters
    assert stats["n_noise"] == [int((sc.labels(name, m) < 0).sum()) for m in sc.SWEEP]
    assert tuple(stats["grid_dims"]) == dims
    assert len(stats["ms_union"]) == len(stats["ms_label"]) == len(sc.SWEEP)
    assert stats["ms_core"] > 0 and all(v > 0 for v in stats["ms_union"] + stats["ms_label"])


@pytest.mark.parametrize("name", ["S1", "S3", "S5"])
def test_order_and_repeats(gpu, name):
    """The rows come in the order given, a repeated value twice."""
    from rpt.processors import st_dbscan_sweep

    rows, _ = _sweep(name)
    c, t = sc.cloud(name)
    eps, et = sc.CASES[name][1]
    order = (60, 3, 25, 10, 10)
    got = st_dbscan_sweep(c, t, eps, et, order)
    assert got.shape == (5, len(c))
    for k, m in enumerate(order):
        assert np.array_equal(got[k], rows[sc.SWEEP.index(m)]), f"{name}: row {k} ({m})"


@pytest.mark.parametrize("name", ["S2", "S6"])
def test_zero_min_samples_row(gpu, name):
    """An entry <= 0 (every point core) is legal: its row is st_dbscan's."""
    from rpt.processors import st_dbscan, st_dbscan_sweep

    rows, _ = _sweep(name)
    c, t = sc.cloud(name)
    eps, et = sc.CASES[name][1]
    stats = {}
    got = st_dbscan_sweep(c, t, eps, et, (10, 0, 25), stats=stats)
    assert np.array_equal(got[1], st_dbscan(c, t, eps, et, 0))
    assert np.array_equal(got[0], rows[1]) and np.array_equal(got[2], rows[2])
    assert stats["n_core"][1] == len(c) and stats["n_noise"][1] == 0
    assert stats["n_clusters"][1] == int(got[1].max()) + 1


def test_border_points_from_count_flags(gpu):
    """S5 at min_samples 10: 1,798 border points by the oracle (at least 1,000 asserted) take the
    smallest adjacent cluster id from core flags that no K5 pass wrote."""
    rows, _ = _sweep("S5")
    exp = sc.labels("S5", 10)
    border = (exp >= 0) & (sc.counts("S5") < 10)
    print(f"S5 m=10: border={int(border.sum())}")
    assert int(border.sum()) >= 1000
    assert np.array_equal(rows[1][border], exp[border])


def test_degenerate_eps_rows(gpu):
    """Negative eps_space: no pair passes, every row is all noise."""
    from rpt.processors import st_dbscan_sweep

    c, t = sc.cloud("S1")
    stats = {}
    got = st_dbscan_sweep(c, t, -1.0, 1.0, (3, 10), stats=stats)
    assert got.shape == (2, len(c)) and np.all(got == -1)
    assert stats["n_core"] == [0, 0] and stats["n_clusters"] == [0, 0]


def test_tensor_rows_on_device(gpu):
    import torch

    from rpt.processors import st_dbscan_sweep

    rows, _ = _sweep("S3")
    c, t = sc.cloud("S3")
    eps, et = sc.CASES["S3"][1]
    cd = torch.from_numpy(c.copy()).to(gpu)
    td = torch.from_numpy(t.copy()).to(gpu)
    got = st_dbscan_sweep(cd, td, eps, et, sc.SWEEP)  # (no stats: no per-set readback)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int32 and got.device == cd.device
    assert np.array_equal(got.cpu().numpy(), rows)
