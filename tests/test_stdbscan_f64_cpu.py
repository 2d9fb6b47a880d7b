"""The host side of the float64 ST-DBSCAN (no GPU): which kernel an input is routed to
(rpt.processors.clustering._plan_inputs), the grid rule of csrc/grid64.h through its host export
against a Python restatement, and the brute-force restatement tests/_f64_ref.py against the
reference's labels in tests/golden/g15_stdbscan_f64.npz."""
from __future__ import annotations

import ctypes as C
import json

import numpy as np
import pytest
import torch

from _f64_cases import CASES, digest
from _f64_ref import grid64_index_py, grid64_plan_py, st_dbscan_ref

from rpt import _abi
from rpt.processors.clustering import _plan_inputs


# ------------------------------------------------------------------------------------- routing
def _xy(dtype, frac=False, n=64):
    k = np.arange(2 * n).reshape(n, 2)
    if frac:
        return (k.astype(np.float64) * 0.1).astype(dtype)  # 0.1 k: no float32 values
    return k.astype(dtype)


_F32_T = np.arange(64, dtype=np.float32) * np.float32(0.1)
_INT_T = np.arange(64) % 5

# (coords, times, eps_time) -> (precision, time dtype, eps_time passed on)
ROUTES = [
    # the float32 route, unchanged
    ("f32 / f32", _xy(np.float32, True), _F32_T, 0.35, ("float32", "float32", 0.35)),
    ("f64 exact / f32", _xy(np.float64), _F32_T, 0.35, ("float32", "float32", 0.35)),
    ("int32 small / int64 small", _xy(np.int32), _INT_T.astype(np.int64), 1.7,
     ("float32", "float32", 1.0)),
    ("f32 / f64 integral", _xy(np.float32), _INT_T.astype(np.float64), 2.5,
     ("float32", "float32", 2.0)),
    ("f32 / f16 integral", _xy(np.float32), _INT_T.astype(np.float16), 1.0,
     ("float32", "float32", 1.0)),
    ("f32 / uint8", _xy(np.float32), _INT_T.astype(np.uint8), float("inf"),
     ("float32", "float32", float("inf"))),
    ("longdouble exact / f32", _xy(np.longdouble), _F32_T, 0.35, ("float32", "float32", 0.35)),
    # the float64 route: coordinates
    ("f64 decimal / f32", _xy(np.float64, True), _F32_T, 0.35, ("float64", "float32", 0.35)),
    ("f64 decimal / f64 integral", _xy(np.float64, True), _INT_T.astype(np.float64), 2.5,
     ("float64", "float64", 2.5)),
    ("f64 decimal / int64 small", _xy(np.float64, True), _INT_T.astype(np.int64), 1.7,
     ("float64", "float64", 1.7)),
    ("int64 above 2^24 / f32", _xy(np.int64) + (1 << 25) + 1, _F32_T, 0.35,
     ("float64", "float32", 0.35)),
    ("longdouble decimal / f32", _xy(np.longdouble, True) / 3, _F32_T, 0.35,
     ("float64", "float32", 0.35)),
    # the float64 route: times
    ("f32 / f64 decimal", _xy(np.float32), _F32_T.astype(np.float64) * 0.1, 0.35,
     ("float64", "float64", 0.35)),
    ("f32 / f64 epoch", _xy(np.float32), 1.7e9 + _INT_T * 0.5, 0.5, ("float64", "float64", 0.5)),
    ("f32 / int64 epoch", _xy(np.float32), 1_700_000_000 + _INT_T.astype(np.int64), 1.5,
     ("float64", "float64", 1.5)),
    ("f32 / int64 at 2^53", _xy(np.float32), np.where(_INT_T > 2, 1 << 53, -(1 << 53)), 1.0,
     ("float64", "float64", 1.0)),
    ("f32 / uint64 large", _xy(np.float32), (_INT_T + (1 << 40)).astype(np.uint64), 1.0,
     ("float64", "float64", 1.0)),
]


# (torch has no longdouble, and no arithmetic on uint64)
_ROUTES_BOTH = [(*r, False) for r in ROUTES] + [
    (*r, True) for r in ROUTES if r[1].dtype != np.longdouble and r[2].dtype != np.uint64]


@pytest.mark.parametrize("name,coords,times,eps_t,want,as_torch", _ROUTES_BOTH,
                         ids=[f"{r[0]} [{'torch' if r[5] else 'numpy'}]" for r in _ROUTES_BOTH])
def test_routing_table(name, coords, times, eps_t, want, as_torch):
    if as_torch:
        coords, times = torch.from_numpy(coords), torch.from_numpy(times)
    plan = _plan_inputs(coords, times, eps_t)
    assert (plan.precision, plan.time_dtype, plan.eps_time) == want
    c = plan.coords.numpy() if as_torch else plan.coords
    t = plan.times.numpy() if as_torch else plan.times
    src_c = coords.numpy() if as_torch else coords
    src_t = times.numpy() if as_torch else times
    assert c.dtype == (np.float64 if want[0] == "float64" else np.float32)
    assert t.dtype == (np.float64 if want[1] == "float64" else np.float32)
    # the cast sklearn's check_array makes, and exact times
    np.testing.assert_array_equal(c, src_c.astype(np.float64).astype(c.dtype))
    np.testing.assert_array_equal(t.astype(np.float64), src_t.astype(np.float64))


REFUSED = [
    ("f64 decimal / f16 integral", _xy(np.float64, True), _INT_T.astype(np.float16),
     NotImplementedError),
    ("f32 / f16 decimal", _xy(np.float32), _F32_T.astype(np.float16), NotImplementedError),
    ("f32 / longdouble decimal", _xy(np.float32), _F32_T.astype(np.longdouble) / 3,
     NotImplementedError),
    ("f64 decimal / longdouble integral", _xy(np.float64, True), _INT_T.astype(np.longdouble),
     NotImplementedError),
    ("f32 / int64 beyond 2^53", _xy(np.float32), _INT_T.astype(np.int64) + (1 << 53) + 1,
     NotImplementedError),
    ("f32 / uint64 beyond 2^53", _xy(np.float32), _INT_T.astype(np.uint64) + np.uint64(1 << 60),
     NotImplementedError),
    ("f32 / complex", _xy(np.float32), _F32_T.astype(np.complex64), TypeError),
    ("f64 decimal / strings", _xy(np.float64, True), np.array(["a"] * 64), TypeError),
]


@pytest.mark.parametrize("name,coords,times,exc", REFUSED, ids=[r[0] for r in REFUSED])
def test_routing_still_refuses(name, coords, times, exc):
    with pytest.raises(exc):
        _plan_inputs(coords, times, 1.0)


def test_routing_torch_refuses_half_and_large_ints():
    c = torch.from_numpy(_xy(np.float32))
    with pytest.raises(NotImplementedError):
        _plan_inputs(c, torch.from_numpy(_F32_T).to(torch.float16), 1.0)
    with pytest.raises(NotImplementedError):
        _plan_inputs(c, torch.from_numpy(_INT_T.astype(np.int64) + (1 << 53) + 1), 1.0)


def test_nan_coordinates_keep_the_float32_route():
    """NaN round-trips through float32, so the float32 kernel still reports it (ValueError)."""
    c = _xy(np.float64)
    c[3, 1] = np.nan
    assert _plan_inputs(c, _F32_T, 1.0).precision == "float32"


# --------------------------------------------------------------------------------- the grid rule
def _plan_native(lo, hi, nft, dim, eps, et, n):
    lib = _abi.load()
    out = _abi.Grid64()
    r = lib.rpt_grid64_plan((C.c_double * 4)(*lo), (C.c_double * 4)(*hi), nft, dim, eps, et, n,
                            C.byref(out))
    assert r == 0, _abi.last_error()
    return (list(out.lo), out.cs, out.ct, tuple(out.dims), out.cells, out.doublings,
            out.collapsed)


EXTREME = [
    # (lo, hi, n_finite_t, dim, eps_space, eps_time, n)
    ([0, 0, 0, 0], [1e300, 1e300, 1e300, 1e300], 10, 3, 1.0, 1.0, 10),  # > 200 doublings
    ([-1e300, 0, 0, 0], [1e300, 1.0, 0, 5.0], 10, 2, 1e-300, 0.5, 1000),
    ([0, 0, 0, 0], [1.0, 1.0, 1.0, 1.0], 5, 3, 5e-324, 5e-324, 5),  # denormal eps
    ([0, 0, 0, 0], [1e-310, 1e-310, 0, 1e-310], 5, 2, 1e-315, 1e-315, 5),
    ([3.5, -2.0, 7.0, 1.7e9], [3.5, -2.0, 7.0, 1.7e9], 4, 3, 0.3, 0.5, 4),  # zero extent
    ([0.1, 0.2, 0.3, 0.4], [0.1, 0.2, 0.3, 0.4], 1, 2, 0.3, 1.0, 1),  # n = 1
    ([0, 0, 0, 0], [100.0, 100.0, 0, 1e9], 50, 2, 1.0, float("inf"), 50),  # one slab
    ([0, 0, 0, 0], [100.0, 100.0, 0, 1e9], 50, 2, 1.0, 0.0, 50),  # eps_t = 0: width 1
    ([0, 0, 0, 0], [100.0, 100.0, 50.0, 10.0], 50, 3, 0.0, 1.0, 50),  # eps = 0: side 1
    ([0, 0, 0, 0], [1e12, 1e12, 0, 3.0], 1000, 2, 1.0, 1.0, 1000),  # the cap coarsens
    ([0, 0, 0, 0], [10.0, 10.0, 0, 1e9], 1000, 2, 1.0, 0.5, 1000),  # ... the slabs
    ([-1.7e308, 0, 0, 0], [1.7e308, 1.0, 0, 1.0], 9, 2, 1.0, 1.0, 9),  # hi - lo overflows
    ([0, 0, 0, -1.7e308], [1.0, 1.0, 0, 1.7e308], 9, 2, 1.0, 1.0, 9),  # ... in time
    ([0, 0, 0, 0], [1.0, 1.0, 0, 0.0], 0, 2, 1.0, 1.0, 9),  # no finite time
    ([0, 0, 0, 0], [1e5, 1e5, 1e5, 100.0], 1 << 20, 3, 1.7e308, 1.7e308, 1 << 29),  # eps * margin
]


@pytest.mark.parametrize("args", EXTREME, ids=[str(i) for i in range(len(EXTREME))])
def test_grid64_plan_extremes(args):
    lo, hi, nft, dim, eps, et, n = args
    got = _plan_native(lo, hi, nft, dim, eps, et, n)
    want = grid64_plan_py(lo, hi, nft, dim, eps, et, n)
    assert got == want
    _, cs, ct, dims, cells, _, _ = got
    assert 1 <= cells <= min(max(1 << 22, 4 * n), 1 << 30)
    assert all(d >= 1 for d in dims) and cells == dims[0] * dims[1] * dims[2] * dims[3]
    if eps > 0 and cs != float("inf"):
        assert cs > eps  # the margin survives the rounding
    if et > 0 and ct != float("inf"):
        assert ct > et


def test_grid64_doubling_bound_cases():
    """Extents that need more than the float32 build's 200 doublings still fit by doubling; only
    an extent that is not finite collapses the axes."""
    g = _plan_native([0] * 4, [1e300, 1e300, 0, 1.0], 9, 2, 1.0, 1.0, 9)
    assert g[5] > 200 and g[6] == 0 and g[4] <= 1 << 22
    g = _plan_native([-1.7e308, 0, 0, 0], [1.7e308, 1.0, 0, 1.0], 9, 2, 1.0, 1.0, 9)
    assert g[5] == 2200 and g[6] == 1 and g[3][:3] == (1, 1, 1)
    g = _plan_native([0, 0, 0, -1.7e308], [1.0, 1.0, 0, 1.7e308], 9, 2, 1.0, 1.0, 9)
    assert g[6] == 3 and g[3] == (1, 1, 1, 1)


def test_grid64_plan_random():
    rng = np.random.default_rng(5)
    for _ in range(300):
        dim = int(rng.integers(2, 4))
        lo = (rng.standard_normal(4) * 10.0 ** rng.integers(-3, 9)).tolist()
        hi = [l + abs(float(e)) for l, e in zip(lo, rng.standard_normal(4) *
                                                10.0 ** rng.integers(-3, 12, size=4))]
        eps = float(10.0 ** rng.uniform(-6, 3))
        et = float(10.0 ** rng.uniform(-6, 3))
        n = int(rng.integers(1, 3_000_000))
        assert _plan_native(lo, hi, n, dim, eps, et, n) == grid64_plan_py(lo, hi, n, dim, eps, et,
                                                                         n)


def test_grid64_plan_rejects_bad_arguments():
    lib = _abi.load()
    out = _abi.Grid64()
    z = (C.c_double * 4)(0, 0, 0, 0)
    for eps, et, dim, n in ((-1.0, 1.0, 2, 5), (float("nan"), 1.0, 2, 5), (1.0, -1.0, 3, 5),
                            (1.0, 1.0, 4, 5), (1.0, 1.0, 2, 0)):
        assert lib.rpt_grid64_plan(z, z, 1, dim, eps, et, n, C.byref(out)) == _abi.RPT_EINVAL


def test_grid64_index():
    lib = _abi.load()
    rng = np.random.default_rng(6)
    vals = [0.0, -0.0, 1e-320, 0.3, 0.30000000000000004, 2.9999999999999996, 3.0, 1e300, -1e300,
            float("inf"), float("-inf"), float("nan")]
    vals += (rng.standard_normal(200) * 100).tolist()
    for side in (0.3 * (1 + 2.0 ** -20), 1.0, 5e-324, 1e300, float("inf")):
        for lo in (0.0, -77.7, 1e300, -1.7e308):
            for n in (1, 7, 1 << 30):
                for v in vals:
                    got = lib.rpt_grid64_index(v, lo, side, n)
                    assert got == grid64_index_py(v, lo, side, n)
                    assert 0 <= got < n


def test_neighbours_share_adjacent_cells_at_last_bit_distances():
    """Pairs exactly eps apart by the rounded test land in cells that differ by at most one."""
    eps = 0.3
    side = eps * (1 + 2.0 ** -20)
    for off in (0.0, 77.7, 4e6):
        x = np.arange(2000) * 0.1 + off
        lo = float(x.min())
        idx = np.array([grid64_index_py(v, lo, side, 1 << 30) for v in x])
        d = x[3:] - x[:-3]
        near = d * d <= eps * eps
        assert near.any() and (~near).any()  # (the last bit decides, both ways)
        assert np.all(np.abs(idx[3:] - idx[:-3])[near] <= 1)


# ----------------------------------------------------------- the restatement against the reference
@pytest.fixture(scope="module")
def g15(golden):
    z = golden("g15_stdbscan_f64.npz")
    return z, json.loads(bytes(z["meta"]).decode())["cases"]


def test_g15_holds_every_case(g15):
    z, meta = g15
    assert sorted(meta) == sorted(CASES)
    assert sorted(k for k in z.files if k != "meta") == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_reference_labels(g15, name):
    z, meta = g15
    case = CASES[name]()
    assert digest(case) == meta[name]["sha256"], "generator drift: regenerate g15"
    got = st_dbscan_ref(case.coords, case.times, case.eps_space, case.eps_time, case.min_samples)
    np.testing.assert_array_equal(got, z[name])


@pytest.mark.parametrize("name", list(CASES))
def test_g15_cases_take_the_float64_route(name):
    case = CASES[name]()
    assert _plan_inputs(case.coords, case.times, case.eps_time).precision == case.route
