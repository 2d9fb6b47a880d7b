"""rpt.processors.neighbour_counts (rpt_neighbour_counts, k_count_cells<2> / <3>) against the C
oracle's exact counts: np.array_equal on every point of the cases S1-S6 (_sweep_cases.py says
what each is there for), their permuted, SoA, NaN-time, duplicate and degenerate variants, and
the shared per-stream state across st_dbscan and neighbour_counts calls.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _sweep_cases as sc
import oracle

pytestmark = pytest.mark.gpu


def _nc(c, t, eps, et):
    from rpt.processors import neighbour_counts

    return neighbour_counts(c, t, eps, et)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_counts_match_oracle(gpu, name):
    sc.check_case(name)
    c, t = sc.cloud(name)
    eps, et = sc.CASES[name][1]
    got = _nc(c, t, eps, et)
    assert got.dtype == np.int32 and got.shape == (len(c),)
    exp = sc.counts(name)
    print(f"{name}: n={len(c)} max={int(got.max())} median={int(np.median(got))} "
          f"differ={int((got != exp).sum())}")
    assert np.array_equal(got, exp)


def test_counts_wide_time_window_3d(gpu):
    """S3 at eps_t = 5: every slab is in every window (6 x 125 positions), so a dense cell lists
    more undecided cells than the wave's list holds and counts in more than one pair phase."""
    sc.check_case("S3")
    c, t = sc.cloud("S3")
    exp = oracle.neighbour_counts(c, t, 5.0, 5.0)
    assert int(exp.max()) > 277  # (more than at eps_t = 1)
    assert np.array_equal(_nc(c, t, 5.0, 5.0), exp)


def test_counts_permuted_rows(gpu):
    sc.check_case("S1")
    c, t = sc.cloud("S1")
    p = np.random.default_rng(99).permutation(len(c))
    eps, et = sc.CASES["S1"][1]
    got = _nc(np.ascontiguousarray(c[p]), np.ascontiguousarray(t[p]), eps, et)
    assert np.array_equal(got, sc.counts("S1")[p])


def test_counts_soa_and_rows(gpu):
    """S3 as (N, 3) rows (stride 3) and as x, y, z tensors of their own (stride 1)."""
    from rpt.processors.clustering import neighbour_counts_soa

    sc.check_case("S3")
    c, t = sc.cloud("S3")
    eps, et = sc.CASES["S3"][1]
    cd = torch.from_numpy(c.copy()).to(gpu)
    td = torch.from_numpy(t.copy()).to(gpu)
    x, y, z = (cd[:, k].contiguous() for k in range(3))
    assert x.stride() == (1,) and cd.stride() == (3, 1)
    rows = _nc(cd, td, eps, et)
    soa = neighbour_counts_soa(x, y, td, eps, et, z=z)
    assert np.array_equal(rows.cpu().numpy(), sc.counts("S3"))
    assert np.array_equal(soa.cpu().numpy(), sc.counts("S3"))


def test_counts_nonfinite_times(gpu):
    """S3 with 5 % of the times NaN: those points count 0 (not even themselves)."""
    sc.check_case("S3")
    c, t = sc.cloud("S3")
    eps, et = sc.CASES["S3"][1]
    t = t.copy()
    nan = np.random.default_rng(5).random(len(t)) < 0.05
    t[nan] = np.nan
    assert 200 < int(nan.sum()) < 500
    exp = oracle.neighbour_counts(c, t, eps, et)
    assert np.all(exp[nan] == 0) and np.all(exp[~nan] >= 1)
    got = _nc(c, t, eps, et)
    assert np.all(got[nan] == 0)
    assert np.array_equal(got, exp)


@pytest.fixture(scope="module")
def duplicated():
    """S1 plus 3,000 copies of one of its points, and the oracle's counts at eps 5 and eps 0."""
    sc.check_case("S1")
    c, t = sc.cloud("S1")
    k = 4321
    c2 = np.concatenate([c, np.repeat(c[k:k + 1], 3000, axis=0)])
    t2 = np.concatenate([t, np.repeat(t[k:k + 1], 3000)])
    eps, et = sc.CASES["S1"][1]
    return c2, t2, k, oracle.neighbour_counts(c2, t2, eps, et), \
        oracle.neighbour_counts(c2, t2, 0.0, et)


def test_counts_duplicates(gpu, duplicated):
    c2, t2, k, exp, _ = duplicated
    eps, et = sc.CASES["S1"][1]
    assert int(exp[k]) >= 3001 and np.all(exp[len(c2) - 3000:] == exp[k])
    got = _nc(c2, t2, eps, et)
    assert int(got[k]) >= 3000
    assert np.array_equal(got, exp)


def test_counts_eps_space_zero(gpu, duplicated):
    """eps_space = 0: only exact duplicates (within eps_t) are neighbours."""
    c2, t2, k, _, exp0 = duplicated
    _, et = sc.CASES["S1"][1]
    assert int(exp0[k]) >= 3001 and int(np.median(exp0[:k])) == 1
    got = _nc(c2, t2, 0.0, et)
    assert np.array_equal(got, exp0)


@pytest.mark.parametrize("eps,et", [(-1.0, 1.0), (5.0, float("nan"))])
def test_counts_degenerate_eps(gpu, eps, et):
    c, t = sc.cloud("S1")
    got = _nc(c, t, eps, et)
    assert got.shape == (len(c),) and not got.any()


def test_counts_single_point(gpu):
    got = _nc(np.array([[1.5, -2.0]], np.float32), np.array([3.0], np.float32), 5.0, 1.0)
    assert got.tolist() == [1]


def test_counts_tensor_in_tensor_out(gpu):
    sc.check_case("S1")
    c, t = sc.cloud("S1")
    eps, et = sc.CASES["S1"][1]
    cd = torch.from_numpy(c.copy()).to(gpu)
    td = torch.from_numpy(t.copy()).to(gpu)
    got = _nc(cd, td, eps, et)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int32 and got.device == cd.device
    assert np.array_equal(got.cpu().numpy(), sc.counts("S1"))


def test_state_survives_between_calls(gpu):
    """st_dbscan, neighbour_counts, st_dbscan on one stream: the calls share the stream's state
    (grid, scratch, flags); the two label arrays are equal and the counts exact."""
    from rpt.processors import st_dbscan

    sc.check_case("S2")
    c, t = sc.cloud("S2")
    eps, et = sc.CASES["S2"][1]
    a = st_dbscan(c, t, eps, et, 10)
    got = _nc(c, t, eps, et)
    b = st_dbscan(c, t, eps, et, 10)
    assert np.array_equal(a, b)
    assert np.array_equal(a, sc.labels("S2", 10))
    assert np.array_equal(got, sc.counts("S2"))
