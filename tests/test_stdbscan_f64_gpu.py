"""ST-DBSCAN on float64 coordinates and times (rpt_stdbscan_f64, csrc/stdbscan64.hip) through
rpt.processors.st_dbscan: exact label equality everywhere.

1. The reference's labels (tests/golden/g15_stdbscan_f64.npz) on every named case of
   tests/_f64_cases.py, numpy and torch inputs.
2. At size against the C oracle by exact transforms.  X is a float32 cloud on a 2^-13 grid with
   |x| < 1024, T float32 times on a 2^-10 grid, eps and eps_t float32 values; then
       (X + 2^30, T)     (X * 2^200, T) with eps * 2^200     (X, T + 1_700_000_000 as float64)
   have the labels of oracle.stdbscan(X, T, ...): every sum, product and difference involved is
   exact in double, and none of these inputs is float32-representable, so each runs the float64
   kernels (stats["precision"]), while X itself still runs the float32 ones.  (X * 2^100, T) with
   eps * 2^100 is run as well and must give the same labels, but X * 2^100 IS a float32 cloud
   (|x| < 2^110, the same 23 bits), so by the routing rule it keeps the float32 route, and that is
   what the test asserts for it; 2^200 is beyond float32's range.)
   Grid caps of the float64 kernels (blocks of 256 threads; above them a kernel strides):
       k64_bounds                          1,024 blocks   262,144 points
       k64_keys, k64_gather, k64_parent_init, k64_roots, k64_cid
                                           2,048 blocks   524,288 points
       k64_cell_start                      2,048 blocks   524,288 cells
       k64_core, k64_union, k64_label      65,536 blocks of 16 points   1,048,576 points
   Cases (oracle figures asserted before anything runs on the device):
       E2   2-D, 30,000 points, non-integral times, 24 x 24 x 1 x 8 cells; 1,602 border points,
            62 of them with core neighbours in two or more clusters
       B3   3-D, 90,000 points, 20 x 20 x 20 x 11 cells: windows clipped at every face; cells of
            up to 218 points (more than a wave, more than 13 rounds of a 16-lane group)
       C3   3-D, 60,000 points in a 1000^3 box at eps 2: the cell cap doubles the cell side twice
            (125^3 x 2 = 3,906,250 cells: k64_cell_start strides); cells of up to 743 points
       F3   3-D, 1,100,000 points, 80^3 x 4 = 2,048,000 cells: every capped grid strides; 38,404
            border points, 57 contended
3. The 0.1 lattice at n = 5,000 against the brute-force restatement tests/_f64_ref.py, over eps
   0.3 / 0.5, min_samples 5 / 9 and both time dtypes; rounding the coordinates to float32 first
   changes at least 100 labels of each.
4. Edges: the cell cap on an extent of 1e12, a time range of 1e9, coordinates of 1e200, the
   arena reused across grids of different shape, non-finite coordinates, n = 0.
"""
from __future__ import annotations

import functools
import json

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import oracle
from _f64_cases import CASES, Case, digest, lattice, lattice_side, quantised_cloud, round_coords_f32
from _f64_ref import grid64_of, st_dbscan_ref

pytestmark = pytest.mark.gpu


def _st(c, t, eps, et, ms, stats=None):
    from rpt.processors import st_dbscan

    return st_dbscan(c, t, eps, et, ms, stats=stats)


# ------------------------------------------------------------------------------------ 1. golden
@pytest.fixture(scope="module")
def g15(golden):
    z = golden("g15_stdbscan_f64.npz")
    return z, json.loads(bytes(z["meta"]).decode())["cases"]


@pytest.mark.parametrize("name", list(CASES))
def test_golden_numpy(gpu, g15, name):
    z, meta = g15
    case = CASES[name]()
    assert digest(case) == meta[name]["sha256"], "generator drift: regenerate g15"
    stats = {}
    got = _st(case.coords, case.times, case.eps_space, case.eps_time, case.min_samples, stats)
    assert stats["precision"] == case.route == "float64"
    assert isinstance(got, np.ndarray) and got.dtype == np.int32
    np.testing.assert_array_equal(got, z[name])
    assert stats["n_clusters"] == int(z[name].max()) + 1


@pytest.mark.parametrize("name", list(CASES))
def test_golden_torch(gpu, g15, name):
    """Device tensors in (float64 ones among them), a device int32 tensor out."""
    z, _ = g15
    case = CASES[name]()
    c = torch.from_numpy(np.ascontiguousarray(case.coords)).to(gpu)
    t = torch.from_numpy(np.ascontiguousarray(case.times)).to(gpu)
    stats = {}
    got = _st(c, t, case.eps_space, case.eps_time, case.min_samples, stats)
    assert stats["precision"] == "float64"
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int32 and got.device == c.device
    np.testing.assert_array_equal(got.cpu().numpy(), z[name])


def test_golden_strided_input(gpu, g15):
    """A non-contiguous view (every other row of a wider array) behaves as its copy."""
    z, _ = g15
    case = CASES["blobs3d_off4e+06"]()
    wide = np.zeros((2 * len(case.coords), 5))
    wide[::2, 1:4] = case.coords
    view = wide[::2, 1:4]
    assert not view.flags.c_contiguous
    got = _st(view, case.times, case.eps_space, case.eps_time, case.min_samples)
    np.testing.assert_array_equal(got, z["blobs3d_off4e+06"])


# ----------------------------------------------------------------- 2. at size, exact transforms
# name: (generator arguments, (eps, eps_t, min_samples),
#        (clusters, noise, core, border, contended), grid dims, doublings, largest cell)
SIZED = {
    "E2": (dict(seed=21, n=30000, dim=2, extent=(120, 120), n_blobs=40, blob_w=30000,
                t_steps=20 * 1024), (5.0, 2.5, 30),
           (16, 2477, 25921, 1602, 62), (24, 24, 1, 8), 0, 104),
    "B3": (dict(seed=22, n=90000, dim=3, extent=(100, 100, 100), n_blobs=40, blob_w=40000,
                t_steps=12, t_quant=1), (5.0, 1.0, 10),
           (26, 15104, 73676, 1220, 3), (20, 20, 20, 11), 0, 218),
    "C3": (dict(seed=23, n=60000, dim=3, extent=(1000, 1000, 1000), n_blobs=40, blob_w=30000,
                t_steps=3, t_quant=1), (2.0, 1.0, 8),
           (40, 12153, 47795, 52, 0), (125, 125, 125, 2), 2, 743),
    "F3": (dict(seed=24, n=1100000, dim=3, extent=(200, 200, 200), n_blobs=600, blob_w=50000,
                t_steps=5, t_quant=1), (2.5, 1.0, 10),
           (355, 185015, 876581, 38404, 57), (80, 80, 80, 4), 0, 114),
}
BFS_MAX = 200_000  # the sequential BFS up to here, the OpenMP set formulation above


def _contended(c, t, exp, core, eps, et):
    """Border points (labelled, not core) and how many of them have core neighbours in two or
    more oracle clusters; on the way, each has the smallest id among its core neighbours."""
    c64 = c.astype(np.float64)
    ci = np.flatnonzero(core)
    border = np.flatnonzero((exp >= 0) & ~core)
    tree = cKDTree(c64[ci])
    n_cont = 0
    for b, nb in zip(border, tree.query_ball_point(c64[border], eps * (1 + 1e-9))):
        nb = ci[np.asarray(nb, np.int64)]
        d = c64[nb] - c64[b]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        if c.shape[1] == 3:
            d2 = d2 + d[:, 2] * d[:, 2]
        ids = exp[nb[(d2 <= eps * eps) & (np.abs(t[nb] - t[b]) <= np.float32(et))]]
        assert ids.min() == exp[b]
        n_cont += int(ids.min() != ids.max())
    return len(border), n_cont


@functools.lru_cache(maxsize=None)
def _sized(name):
    """Input and oracle labels of a case, computed once; what the case is there for is asserted
    here, on the oracle alone.  No test writes to them."""
    kw, (eps, et, ms), figures, dims, doublings, max_cell = SIZED[name]
    c, t = quantised_cloud(**kw)
    assert c.dtype == np.float32 and t.dtype == np.float32 and len(c) == kw["n"]
    assert np.abs(c).max() < 1024 and np.array_equal(c * 8192, np.round(c * 8192))
    assert np.array_equal(t * 1024, np.round(t * 1024))
    assert all(float(np.float32(v)) == v for v in (eps, et))
    if len(c) <= BFS_MAX:
        exp = oracle.stdbscan(c, t, eps, et, ms)
        cnt = oracle.neighbour_counts(c, t, eps, et)
    else:
        exp = oracle.stdbscan_uf(c, t, eps, et, ms)
        cnt, _, _ = oracle.sample_check(c, t, eps, et, np.arange(len(c), dtype=np.int64),
                                        np.zeros(len(c), np.uint8), exp)
    core = cnt >= ms
    n_border, n_cont = _contended(c, t, exp, core, eps, et)
    got = (int(exp.max()) + 1, int((exp < 0).sum()), int(core.sum()), n_border, n_cont)
    assert got == figures, f"{name}: oracle figures {got}"
    # the float64 grid of the plain cloud (the transforms scale or shift it exactly)
    lo, cs, ct, gdims, cells, it, _ = grid64_of(c, t, eps, et)
    assert (gdims, it) == (dims, doublings), f"{name}: grid {gdims}, {it} doublings"
    c64 = c.astype(np.float64)
    key = np.zeros(len(c), np.int64)
    mul = 1
    for k in range(c.shape[1]):
        key += np.minimum(np.floor((c64[:, k] - lo[k]) / cs).astype(np.int64), gdims[k] - 1) * mul
        mul *= gdims[k]
    key += np.minimum(np.floor((t.astype(np.float64) - lo[3]) / ct).astype(np.int64),
                      gdims[3] - 1) * mul
    occ = np.bincount(key, minlength=cells)
    assert int(occ.max()) == max_cell, f"{name}: largest cell {int(occ.max())}"
    if name == "B3":  # windows clipped at every face: points in the first and last cell layers
        for k in range(3):
            idx = np.floor((c64[:, k] - lo[k]) / cs).astype(np.int64)
            assert (idx == 0).any() and (idx >= gdims[k] - 1).any()
        assert max_cell > 64
    if name == "F3":
        assert len(c) > 1_048_576 and cells > 524_288
    exp.setflags(write=False)
    return c, t, exp


def _transformed(name, how):
    (_, (eps, et, ms), *_), (c, t, _) = SIZED[name], _sized(name)
    c64 = c.astype(np.float64)
    if how == "shift":
        out = c64 + 2.0 ** 30, t, eps
        assert np.array_equal(out[0] - 2.0 ** 30, c64)
    elif how in ("scale100", "scale200"):
        f = 2.0 ** int(how[5:])
        out = c64 * f, t, eps * f
        assert np.array_equal(out[0] / f, c64) and (out[2] * out[2]) / (f * f) == eps * eps
    else:
        t64 = t.astype(np.float64) + 1_700_000_000.0
        assert np.array_equal(t64 - 1_700_000_000.0, t.astype(np.float64))
        out = c, t64, eps
    return out[0], out[1], out[2], et, ms


@pytest.mark.parametrize("how", ["shift", "scale200", "epoch", "scale100"])
@pytest.mark.parametrize("name", list(SIZED))
def test_at_size_matches_oracle(gpu, name, how):
    dims = SIZED[name][3]
    _, _, exp = _sized(name)
    c, t, eps, et, ms = _transformed(name, how)
    stats = {}
    got = _st(c, t, eps, et, ms, stats)
    print(f"{name}/{how}: grid={stats['grid_dims']} clusters={stats['n_clusters']} "
          f"ms core={stats['ms_core']:.3f} union={stats['ms_union']:.3f} "
          f"label={stats['ms_label']:.3f}")
    if how == "scale100":  # float32 values: the float32 route, as before
        assert stats["precision"] == "float32"
    else:
        assert stats["precision"] == "float64"
        assert stats["time_dtype"] == ("float64" if how == "epoch" else "float32")
        assert tuple(stats["grid_dims"]) == dims == grid64_of(c, t, eps, et)[3]
    np.testing.assert_array_equal(got, exp)
    assert stats["n_clusters"] == int(exp.max()) + 1


@pytest.mark.parametrize("name", list(SIZED))
def test_plain_cloud_keeps_the_float32_route(gpu, name):
    (_, (eps, et, ms), *_), (c, t, exp) = SIZED[name], _sized(name)
    stats = {}
    got = _st(c, t, eps, et, ms, stats)
    assert stats["precision"] == "float32" and stats["time_dtype"] == "float32"
    np.testing.assert_array_equal(got, exp)
    # ... and as float64 values that round-trip through float32
    stats = {}
    got = _st(c.astype(np.float64), t, eps, et, ms, stats)
    assert stats["precision"] == "float32"
    np.testing.assert_array_equal(got, exp)


def test_soa_strides_against_rows(gpu):
    """B3 shifted: (N, 3) rows (stride 3) through st_dbscan, and x, y, z arrays of their own
    (stride 1) through the C ABI."""
    from rpt import _abi
    from rpt._device import stream_handle

    _, _, exp = _sized("B3")
    c, t, eps, et, ms = _transformed("B3", "shift")
    cd = torch.from_numpy(c).to(gpu)
    td = torch.from_numpy(t.copy()).to(gpu)
    assert cd.stride() == (3, 1)
    rows = _st(cd, td, eps, et, ms)
    np.testing.assert_array_equal(rows.cpu().numpy(), exp)
    x, y, z = (cd[:, k].contiguous() for k in range(3))
    labels = torch.empty(len(c), dtype=torch.int32, device=gpu)
    with torch.cuda.device(gpu):
        r = _abi.load().rpt_stdbscan_f64(x.data_ptr(), y.data_ptr(), z.data_ptr(), 1,
                                         td.data_ptr(), _abi.TIME_F32, len(c), eps, et, ms,
                                         labels.data_ptr(), None, stream_handle(gpu))
    _abi.check(r, "rpt_stdbscan_f64")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(labels.cpu().numpy(), exp)


def test_c_abi_argument_errors(gpu):
    from rpt import _abi

    lib = _abi.load()
    x = torch.zeros(8, dtype=torch.float64, device=gpu)
    lab = torch.empty(8, dtype=torch.int32, device=gpu)
    p, lp = x.data_ptr(), lab.data_ptr()
    with torch.cuda.device(gpu):
        assert lib.rpt_stdbscan_f64(p, p, None, 1, p, 1, 0, 1.0, 1.0, 1, lp, None, None) == \
            _abi.RPT_EEMPTY
        assert lib.rpt_stdbscan_f64(p, p, None, 1, p, 1, (1 << 31) - 2, 1.0, 1.0, 1, lp, None,
                                    None) == _abi.RPT_ENOTSUP
        assert lib.rpt_stdbscan_f64(p, None, None, 1, p, 1, 8, 1.0, 1.0, 1, lp, None, None) == \
            _abi.RPT_EINVAL
        assert lib.rpt_stdbscan_f64(p, p, None, 0, p, 1, 8, 1.0, 1.0, 1, lp, None, None) == \
            _abi.RPT_EINVAL
        assert lib.rpt_stdbscan_f64(p, p, None, 1, p, 2, 8, 1.0, 1.0, 1, lp, None, None) == \
            _abi.RPT_EINVAL


# ------------------------------------------------------------------------- 3. brute force, 5,000
@functools.lru_cache(maxsize=None)
def _lattice_case(eps, ms, tf64):
    """The 0.1 lattice with decimal times (multiples of 0.1, eps_t 0.3): float64 times, or the
    float32 products float32(k) * float32(0.1)."""
    c, _ = lattice(300 + int(eps * 10) + ms, side=lattice_side(eps, ms, frames=2), offset=77.7)
    k = np.random.default_rng(301 + ms).integers(0, 12, size=len(c))
    t = k.astype(np.float64) * 0.1 if tf64 else k.astype(np.float32) * np.float32(0.1)
    case = Case(c, t, eps, 0.3, ms, True, "float64")
    want = st_dbscan_ref(c, t, eps, 0.3, ms)
    r = round_coords_f32(case)
    want32 = st_dbscan_ref(r.coords, r.times, eps, 0.3, ms)
    want.setflags(write=False)
    return case, want, int((want32 != want).sum())


@pytest.mark.parametrize("tf64", [False, True], ids=["t32", "t64"])
@pytest.mark.parametrize("ms", [5, 9])
@pytest.mark.parametrize("eps", [0.3, 0.5])
def test_lattice_matches_brute_force(gpu, eps, ms, tf64):
    case, want, changed_by_f32 = _lattice_case(eps, ms, tf64)
    assert len(case.coords) == 5000
    print(f"eps={eps} ms={ms} t64={tf64}: clusters={int(want.max()) + 1} "
          f"noise={int((want < 0).sum())} labels changed by float32 rounding={changed_by_f32}")
    assert changed_by_f32 >= 100
    stats = {}
    got = _st(case.coords, case.times, case.eps_space, case.eps_time, case.min_samples, stats)
    assert stats["precision"] == "float64"
    assert stats["time_dtype"] == ("float64" if tf64 else "float32")
    np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------------------------- 4. edges
def _small_blobs(seed, n=2000):
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 400, size=(10, 2))
    q = centres[rng.integers(0, 10, size=n)] * 8 + rng.integers(-12, 13, size=(n, 2))
    stray = rng.integers(0, 8, size=n) == 0
    q[stray] = rng.integers(0, 3200, size=(int(stray.sum()), 2))
    return q.astype(np.float64) * 0.1, rng.integers(0, 3, size=n).astype(np.float64)


def test_cell_cap_on_a_huge_extent(gpu):
    """Two groups of blobs 1e12 apart at eps 1: the cell cap coarsens the cells."""
    c, t = _small_blobs(1)
    c[len(c) // 2:] += 1e12
    _, cs, _, dims, cells, it, collapsed = grid64_of(c, t, 1.0, 1.0)
    assert it > 0 and collapsed == 0 and cs > 1e5 and cells <= 1 << 22
    want = st_dbscan_ref(c, t, 1.0, 1.0, 5)
    assert want.max() >= 10 and (want < 0).any()
    stats = {}
    got = _st(c, t, 1.0, 1.0, 5, stats)
    assert stats["precision"] == "float64" and tuple(stats["grid_dims"]) == dims
    np.testing.assert_array_equal(got, want)


def test_time_range_of_1e9(gpu):
    c, t = _small_blobs(2)
    t = 1.7e9 + t * 0.25
    t[len(t) // 2:] -= 1e9
    _, _, ct, dims, _, it, _ = grid64_of(c, t, 1.0, 0.5)
    assert it > 0 and ct > 100 and dims[3] > 1
    want = st_dbscan_ref(c, t, 1.0, 0.5, 5)
    assert want.max() >= 10
    stats = {}
    got = _st(c, t, 1.0, 0.5, 5, stats)
    assert stats["time_dtype"] == "float64" and tuple(stats["grid_dims"]) == dims
    np.testing.assert_array_equal(got, want)


def test_coordinates_of_1e200(gpu):
    """Distinct points 1e200 apart: d2 overflows to infinity, which is not <= eps^2."""
    rng = np.random.default_rng(3)
    c = rng.permutation(4000).reshape(2000, 2).astype(np.float64) * 1e200
    t = np.zeros(2000)
    assert grid64_of(c, t, 1.0, 1.0)[5] > 200  # more doublings than float32 extents ever need
    got = _st(c, t, 1.0, 1.0, 2)
    np.testing.assert_array_equal(got, st_dbscan_ref(c, t, 1.0, 1.0, 2))
    assert (got == -1).all()


def test_arena_reused_across_grids(gpu):
    """Three clouds of different grid shape in one process, the first one again at the end."""
    for name in ("B3", "E2", "C3", "B3"):
        _, _, exp = _sized(name)
        c, t, eps, et, ms = _transformed(name, "shift")
        np.testing.assert_array_equal(_st(c, t, eps, et, ms), exp, err_msg=name)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nonfinite_coordinates_raise(gpu, bad):
    c, t = _small_blobs(4, n=700)
    c[333, 1] = bad
    with pytest.raises(ValueError, match="NaN or infinity"):
        _st(c, t, 1.0, 1.0, 5)
    with pytest.raises(ValueError, match="NaN or infinity"):
        _st(torch.from_numpy(c).to(gpu), torch.from_numpy(t).to(gpu), 1.0, 1.0, 5)


def test_empty_input_raises(gpu):
    with pytest.raises(ValueError, match="0 sample"):
        _st(np.zeros((0, 2)), np.zeros(0), 1.0, 1.0, 5)
    with pytest.raises(ValueError, match="0 sample"):
        _st(np.zeros((0, 3)), np.zeros(0, np.int64), 1.0, 1.0, 5)
