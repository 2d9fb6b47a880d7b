"""The general forms of ST-DBSCAN (everything the 2-D time-ordered integral-time stack rules send
away from the slab counting sort, the fused / masked K5, the listed and pair unions, the per-cell
component ids and the xy-only points) at sizes where their grids stride, against the C oracle:
exact label equality (the same ids, not only the same partition) through
rpt.processors.st_dbscan on the shipped librpt.so.  No A/B switch is read or set.

Every case first asserts, on the oracle alone, that its input is what it is there for: the point
count, the oracle's cluster, noise and core counts, the grid dimensions the device reports (stats)
against build_t's rule restated in _grid below, and how often that rule doubled the cell side.

3-D cases run k_bounds<3>, k_keys<3>, the radix sort, k_gather<3>, k_cell_runs, k_occ_list,
k_cell_box<3>, k_slab_range<3>; k_core_cell_fast, k_core_cell_window<3>, k_core_fill<true>,
k_core_slow<3>; k_init_occ_cells, k_cell_min_pair, k_parent_init_pair, k_union_cells<3, false>,
k_union_cells<3, true>, k_union<3>; k_cell_roots, k_ccmin, k_word_popc, k_label_core and
k_label<3, false, 64> (one wave per queued point).

Size boundaries (grid_for(items, per block, cap) blocks of 256 threads, each striding past its cap):
  16,384 wave items   wave_grid: 4,096 blocks of 4 waves, one queue entry or cell per wave (two
                      per wave in k_label<2, false, 32>): k_core_cell_window, k_core_slow,
                      k_union_cells, k_union_cells_pair, k_union_listed, k_union_nm, k_label
  262,144 points      k_bounds (1,024 blocks)
  524,288 points      the 2,048-block grids: k_keys, k_gather, k_cell_runs, k_occ_list,
                      k_init_occ_cells, k_cell_min_pair, k_cell_roots
  1,048,576 points    the 4,096-block grids (k_cell_root_snapshot in 2-D) and more than 4,096
                      blocks of k_union (one block per 256 points, no cap)
  scan tiles          k_core_cell_fast, k_core_fill and k_ccmin append to their queues by tiles of
                      4,096 items (2,048 blocks: no stride below 8,388,608 points, so these cases
                      cross tiles, not that stride; nor do the eight-points-per-thread
                      k_parent_init_pair and k_label_core stride below 4,194,304)

  A   planes, 150,368 points, cell side doubled twice (2 eps): the `cluster` CLI's layout at its
      defaults; three occupied z planes in 50 z cells (101 x 101 x 50 x 3, 21-bit radix keys);
      58,593 + 525 non-core points queued for k_label<3>: the wave-per-item kernels stride; 37
      scan tiles.
  A'  A with its rows permuted: the radix sort orders the slabs itself, the component minima (and
      so the ids) sit at other rows.
  B   89,146 points, uncoarsened 54 x 55 x 51 x 12 grid (cell side 0.5 eps): 125-cell windows
      clipped at every face; 1,030 border points through k_label<3>; 21-bit keys; 22 scan tiles.
  B'  the same cloud in a larger box, cell side doubled once (eps): 27-cell windows hold every
      neighbour, cells are no longer mutual by their diagonal alone.
  C   3-D with non-integral times: slab width eps_t (1 + 2^-20), 24 slabs, generic (not tfree)
      time windows in every 3-D kernel; cell side doubled once.
  D   2-D, ordered, integral, eps_t = 5: slab_reach() = 5 > kCwMaxR, so oct_ok fails on the slab
      counting sort's grid: k_core_cell_fast, k_core_cell_window<2>, k_core_fill<true>,
      k_core_slow<2> (windows of 11 slabs), the cell minima from k_init_occ_cells /
      k_cell_min_pair instead of the fused K5, then the all-mutual grid's per-cell path on
      float4 points (k_parent_init_cells, k_union_cells_pair, k_cell_root_snapshot,
      k_union_listed, k_cell_comp, k_label_core_cells, k_label<2, false, 32, true>); 182,353
      points (45 scan tiles), a ~97 k-point cluster chained over 40 frames, 2,768 border points.
      (Only 4 of them have core neighbours in two clusters, and no seed from 14 to 1,561 of this
      recipe gives more than 46: the smallest-adjacent-id rule under contention rests on D''.)
  D'' vol(14, 30, 100, 800, 150.0, 20, dim=2) at eps 6, eps_t 5, min_samples 40: D's kernels
      (oct_ok fails through eps_t = 5; 44 x 46 x 1 x 20 cells, windows of 11 slabs) on a denser
      cloud, 91,560 points, 16 clusters, 5,905 border points of which 166 have core neighbours
      in two or more clusters: there k_label<2, false, 32, true> must pick the smallest of
      several adjacent ids (test_border_rule_under_contention asserts at least 100 such points,
      counted by a loop of its own over the oracle's border points).
  E   2-D with non-integral times: the radix build, ct = eps_t (1 + 2^-20), generic time windows
      in k_core_cell_window<2> / k_core_slow<2>, and (not an all-mutual grid) the per-point
      union and label forms: k_parent_init_pair, k_union_cells_pair, k_union_listed,
      k_union_nm<2>, k_cell_roots, k_ccmin, k_label_core, k_label<2, false, 32>; 28,612 points:
      7 scan tiles, 16-bit keys (fewer radix passes than the 21- to 23-bit grids).
  F   1,390,514 points on an uncoarsened 3-D grid (96^3 x 4, 22-bit keys): beyond 1,048,576, so
      every grid capped at 1,024, 2,048 or 4,096 blocks strides and k_union<3> runs 5,432 blocks;
      340 scan tiles; only 7,357 queued non-core points (k_label<3> does not stride here).
  G   1,424,739 points, cell side doubled twice, 52 x 55 x 51 x 30 (23-bit keys): the same
      strides on a coarsened grid with 178,819 noise points in the non-core queue.
  H   2-D, ordered, integral, eps_t = 1, but 515 x 515 cells per slab > kBucketCells = 16,384:
      the radix build (k_keys<2>, k_gather<2>) feeding the oct / masked K5 and the per-cell
      component path on an all-mutual grid (float4 points).

Further: B as structure-of-arrays (stride 1) against (N, 3) rows (stride 3); A, B, A in one
process (the per-stream working set grows and is reused across grids of different shape); B with
5 % NaN times (the isolated cell at size: 4,539 NaN-time points, all noise; 25 clusters).
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------- generators
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


def _permuted(c, t):
    p = np.random.default_rng(99).permutation(len(c))
    return np.ascontiguousarray(c[p]), np.ascontiguousarray(t[p])


# name: (input, (eps, eps_t, min_samples), n, clusters, noise, core, cell-side doublings)
CASES = {
    "A": (lambda: planes(11, 20000, 1000.0, 60, 400), (5.0, 1.0, 10),
          150368, 178, 58593, 91250, 2),
    "A_perm": (lambda: _permuted(*planes(11, 20000, 1000.0, 60, 400)), (5.0, 1.0, 10),
               150368, 178, 58593, 91250, 2),
    "B": (lambda: vol(12, 40, 120, 1500, 100.0, 12, dim=3), (5.0, 1.0, 10),
          89146, 25, 15937, 72179, 0),
    "B_wide": (lambda: vol(12, 40, 120, 1500, 160.0, 12, dim=3), (5.0, 1.0, 10),
               89146, 35, 17486, 71377, 1),
    "C": (lambda: vol(13, 40, 120, 1500, 160.0, 12, dim=3, jitter_t=0.9), (5.0, 0.5, 10),
          90484, 35, 17612, 72359, 1),
    "D": (lambda: vol(14, 30, 100, 800, 300.0, 40, dim=2), (6.0, 5.0, 20),
          182353, 16, 26118, 153467, 0),
    "D_contended": (lambda: vol(14, 30, 100, 800, 150.0, 20, dim=2), (6.0, 5.0, 40),
                    91560, 16, 4378, 81277, 0),
    "E": (lambda: vol(15, 30, 60, 600, 300.0, 10, dim=2, jitter_t=0.9), (6.0, 1.5, 12),
          28612, 21, 5364, 22992, 0),
    "F": (lambda: vol(16, 400, 700, 2000, 200.0, 4, dim=3, spread=1.5, vel=0.5), (5.0, 1.0, 10),
          1390514, 273, 7070, 1383157, 0),
    "G": (lambda: vol(17, 150, 220, 6000, 420.0, 30, dim=3), (5.0, 1.0, 10),
          1424739, 144, 178819, 1245237, 2),
    "H": (lambda: vol(18, 30, 100, 800, 1500.0, 6, dim=2), (5.0, 1.0, 10),
          26733, 30, 4783, 21941, 0),
}
BFS_MAX = 200_000  # the sequential BFS up to here, the OpenMP set formulation above


# ------------------------------------------------------------------------------- the oracle side
def _oracle_labels(c, t, eps, et, ms):
    fn = oracle.stdbscan if len(c) <= BFS_MAX else oracle.stdbscan_uf
    return fn(c, t, eps, et, ms)


def _oracle_core(c, t, eps, et, ms, exp):
    """Core flags from the oracle's exact neighbour counts (self included).  Above BFS_MAX the
    counts come from the OpenMP sample check over every point: the same counts
    (test_sample_check_counts_are_neighbour_counts, on B) in a third of the time of the
    sequential neighbour_counts."""
    if len(c) <= BFS_MAX:
        cnt = oracle.neighbour_counts(c, t, eps, et)
    else:
        cnt, _, _ = oracle.sample_check(c, t, eps, et, np.arange(len(c), dtype=np.int64),
                                        np.zeros(len(c), np.uint8), exp)
    return cnt >= ms


@functools.lru_cache(maxsize=None)
def _case(name):
    """Input, oracle labels and oracle core flags of a case: computed once and shared; no test
    writes to them."""
    make, (eps, et, ms), n, n_clusters, n_noise, n_core, _ = CASES[name]
    c, t = make()
    assert c.dtype == np.float32 and t.dtype == np.float32
    assert len(c) == len(t) == n, f"{name}: generator drift, n={len(c)}"
    exp = _oracle_labels(c, t, eps, et, ms)
    core = _oracle_core(c, t, eps, et, ms, exp)
    for a in (exp, core):  # (c and t go to the device through torch.from_numpy: writable)
        a.setflags(write=False)
    return c, t, exp, core


def _grid(c, t, eps, et):
    """build_t's grid rule: (nx, ny, nz, nt) and how often the cell side was doubled."""
    n, dim = c.shape
    tf = t[np.isfinite(t)]
    integral = bool(np.all(tf == np.floor(tf)))
    margin = 1.0 + 2.0 ** -20
    cs = eps * (0.7 if dim == 2 else 0.5) * margin
    ct = 1.0 if integral else float(np.float32(et)) * margin
    cap = min(max(1 << 22, 4 * n), 1 << 30)
    ext = [float(c[:, k].max()) - float(c[:, k].min()) for k in range(dim)]
    ext_t = float(tf.max()) - float(tf.min()) if len(tf) else 0.0
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
    return tuple(d + [1] * (3 - dim) + [nt]), doubled


def _st(c, t, eps, et, ms, stats=None):
    from rpt.processors import st_dbscan

    return st_dbscan(c, t, eps, et, ms, stats=stats)


def _contended_border(c, t, exp, core, eps, et):
    """How many border points (labelled, not core) have core neighbours in two or more oracle
    clusters: a plain loop over the border points, float64 distances and the float32 time test.
    On the way: the oracle gave each border point the smallest id among its core neighbours."""
    c64 = c.astype(np.float64)
    ci = np.flatnonzero(core)
    cc, ct, cl = c64[ci], t[ci], exp[ci]
    eps2, et32 = float(eps) * float(eps), np.float32(et)
    border = np.flatnonzero((exp >= 0) & ~core)
    contended = 0
    for tb in np.unique(t[border]):
        near = np.abs(ct - tb) <= et32  # (float32 - float32, as the oracle tests it)
        o = np.argsort(cc[near, 0])  # the window's core points by x: only to cut the loop short
        wc, wl = cc[near][o], cl[near][o]
        for b in border[t[border] == tb]:
            lo, hi = np.searchsorted(wc[:, 0], [c64[b, 0] - eps - 1e-6, c64[b, 0] + eps + 1e-6])
            d = wc[lo:hi] - c64[b]
            ids = wl[lo:hi][d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= eps2]
            assert ids.min() == exp[b]
            contended += int(ids.min() != ids.max())
    return len(border), contended


def _check_preconditions(name):
    _, (eps, et, ms), n, n_clusters, n_noise, n_core, doubled = CASES[name]
    c, t, exp, core = _case(name)
    assert len(c) == n
    assert int(exp.max()) + 1 == n_clusters, f"{name}: oracle clusters {int(exp.max()) + 1}"
    assert int((exp < 0).sum()) == n_noise, f"{name}: oracle noise {int((exp < 0).sum())}"
    assert int(core.sum()) == n_core, f"{name}: oracle core {int(core.sum())}"
    assert not np.any(core & (exp < 0))  # (a core point is never noise)
    dims, d = _grid(c, t, eps, et)
    assert d == doubled, f"{name}: cell side doubled {d} times, grid {dims}"
    return dims


# ------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", list(CASES))
def test_general_forms_match_oracle(gpu, name):
    _, (eps, et, ms), *_ = CASES[name]
    dims = _check_preconditions(name)
    c, t, exp, _ = _case(name)
    stats = {}
    got = _st(c, t, eps, et, ms, stats=stats)
    print(f"{name}: n={len(c)} grid_dims={stats['grid_dims']} expected={dims} "
          f"clusters={stats['n_clusters']}")
    assert tuple(stats["grid_dims"]) == dims
    if name == "H":  # more cells per slab than the slab counting sort's LDS histogram holds
        assert dims[0] * dims[1] > 16384
    np.testing.assert_array_equal(got, exp)
    assert stats["n_clusters"] == int(exp.max()) + 1


def test_border_rule_under_contention(gpu):
    """k_label's smallest-adjacent-id rule where it has a choice.  Case D (seed 14) has only 4
    border points with core neighbours in two or more oracle clusters (seeds 15 and 16: 8 and 19;
    no seed from 14 to 1,561 of D's recipe has more than 46), so this input departs from D's
    recipe: vol(14, 30, 100, 800, 150.0, 20, dim=2) at eps 6, eps_t 5, min_samples 40 (half the
    box, half the frames, twice the core threshold; eps_t = 5 still fails oct_ok, the kernels
    are D's).  Oracle: 91,560 points, 16 clusters, 5,905 border points, 166 of them with core
    neighbours in two or more clusters; at least 100 are asserted."""
    name = "D_contended"
    _, (eps, et, ms), *_ = CASES[name]
    dims = _check_preconditions(name)
    c, t, exp, core = _case(name)
    n_border, contended = _contended_border(c, t, exp, core, eps, et)
    print(f"{name}: border={n_border} contended={contended}")
    assert n_border == 5905
    assert contended >= 100
    stats = {}
    got = _st(c, t, eps, et, ms, stats=stats)
    assert tuple(stats["grid_dims"]) == dims
    np.testing.assert_array_equal(got, exp)


def test_sample_check_counts_are_neighbour_counts():
    """The core counts of F and G come from oracle.sample_check (_oracle_core): on case B it
    counts, point for point, what oracle.neighbour_counts counts."""
    _, (eps, et, ms), *_ = CASES["B"]
    c, t, exp, core = _case("B")
    cnt, _, _ = oracle.sample_check(c, t, eps, et, np.arange(len(c), dtype=np.int64),
                                    np.zeros(len(c), np.uint8), exp)
    np.testing.assert_array_equal(cnt, oracle.neighbour_counts(c, t, eps, et))
    np.testing.assert_array_equal(cnt >= ms, core)


def test_soa_and_aos_layouts(gpu):
    """Case B as x, y, z tensors of their own (stride 1) and as (N, 3) rows (stride 3)."""
    from rpt.processors.clustering import st_dbscan_soa

    _, (eps, et, ms), *_ = CASES["B"]
    _check_preconditions("B")
    c, t, exp, _ = _case("B")
    cd = torch.from_numpy(c.copy()).to(gpu)
    td = torch.from_numpy(t.copy()).to(gpu)
    x, y, z = (cd[:, k].contiguous() for k in range(3))
    assert x.stride() == (1,) and cd.stride() == (3, 1)
    soa = st_dbscan_soa(x, y, td, eps, et, ms, z=z)
    aos = _st(cd, td, eps, et, ms)
    np.testing.assert_array_equal(soa.cpu().numpy(), exp)
    np.testing.assert_array_equal(aos.cpu().numpy(), exp)


def test_state_reused_across_grids(gpu):
    """A, then B, then A again in one process: the per-stream working set grows and is reused
    across grids of different shape."""
    runs = []
    for name in ("A", "B", "A"):
        _, (eps, et, ms), *_ = CASES[name]
        _check_preconditions(name)
        c, t, exp, _ = _case(name)
        got = _st(c, t, eps, et, ms)
        np.testing.assert_array_equal(got, exp, err_msg=f"run {len(runs)} ({name})")
        runs.append(got)
    np.testing.assert_array_equal(runs[2], runs[0])


def test_nonfinite_times_at_size(gpu):
    """Case B with 5 % of the times NaN: those points are isolated (label -1), the rest labelled
    as the BFS labels them."""
    _, (eps, et, ms), *_ = CASES["B"]
    c, t, _, _ = _case("B")
    t = t.copy()
    rng = np.random.default_rng(5)
    nan = rng.random(len(t)) < 0.05
    t[nan] = np.nan
    assert len(c) == 89146 and int(nan.sum()) == 4539
    exp = oracle.stdbscan(c, t, eps, et, ms)
    core = oracle.neighbour_counts(c, t, eps, et) >= ms
    # the oracle on this variant: 25 clusters, 19,697 noise points (the 4,539 among them), 68,477 core
    assert np.all(exp[nan] == -1) and not np.any(core[nan])
    assert int(exp.max()) + 1 == 25
    assert int((exp < 0).sum()) == 19697
    assert int(core.sum()) == 68477
    dims, doubled = _grid(c, t, eps, et)
    assert dims == (54, 55, 51, 12) and doubled == 0
    stats = {}
    got = _st(c, t, eps, et, ms, stats=stats)
    assert tuple(stats["grid_dims"]) == dims
    assert np.all(got[nan] == -1)
    np.testing.assert_array_equal(got, exp)
