"""The per-cell component path of ST-DBSCAN (grids on which every occupied cell is mutual: 2-D,
integral times, uncoarsened 0.7 eps cells, min_samples >= 1 -- k_parent_init_cells, k_cell_comp,
k_label_core_cells, k_label's ALLMUT form) against the C oracle: exact label equality through
rpt.processors.st_dbscan, and the 14-frame stack through FrameStackPipeline against
oracle.run_path.  Every case first asserts on the CPU the structure it is there for (core flags
from neighbour counts by scipy cKDTree per frame, cells = floor((v - min) / (0.7 eps (1 + 2^-20)))).
The A/B children (librpt_ab.so) run the per-point kernels (RPT_CELL_COMP=0), the
original-order core-label pass (RPT_LABEL_ORIG=2), the compression pass (RPT_UF_COMPRESS=1, which
must keep the per-point init) and the defaults; each must match librpt.so bit for bit and report
the expected path (RPT_STATS)."""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import oracle

pytestmark = pytest.mark.gpu

EPS, EPS_T, MS = 8.0, 2.0, 15


def _st(xy, t, eps=EPS, et=EPS_T, ms=MS):
    from rpt.processors import st_dbscan

    return st_dbscan(xy, t, eps, et, ms)


def _core(xy, t, eps=EPS, et=EPS_T, ms=MS):
    """Core flags from neighbour counts (the point itself included), per time value."""
    xy64 = xy.astype(np.float64)
    core = np.zeros(len(xy), bool)
    for tv in np.unique(t):
        own = np.flatnonzero(t == tv)
        near = np.flatnonzero(np.abs(t - tv) <= et)
        cnt = cKDTree(xy64[near]).query_ball_point(xy64[own], eps, return_length=True)
        core[own] = cnt >= ms
    return core


def _cells(xy, t, eps=EPS):
    """One integer id per (time, y, x) cell of the device grid."""
    side = 0.7 * eps * (1.0 + 2.0 ** -20)
    cx = np.floor((xy[:, 0].astype(np.float64) - float(xy[:, 0].min())) / side).astype(np.int64)
    cy = np.floor((xy[:, 1].astype(np.float64) - float(xy[:, 1].min())) / side).astype(np.int64)
    ct = (t.astype(np.float64) - float(t.min())).astype(np.int64)
    return (ct * (cy.max() + 1) + cy) * (cx.max() + 1) + cx


def _check(xy, t, eps=EPS, et=EPS_T, ms=MS):
    assert len(xy) <= 20000 and xy.dtype == np.float32 and t.dtype == np.float32
    assert np.array_equal(t, np.floor(t))  # integral times
    exp = oracle.stdbscan(xy, t, eps, et, ms)
    got = _st(xy, t, eps, et, ms)
    np.testing.assert_array_equal(got, exp)
    return exp


def _blob_cloud(seed, frames, n_blobs=8, per=120, noise=400, box=160.0):
    rng = np.random.default_rng(seed)
    centers = rng.random((n_blobs, 2)) * box - box / 2
    pts, ts = [], []
    for f in frames:
        for c in centers:
            pts.append(c + rng.normal(0, 2.5, (per, 2)))
            ts.append(np.full(per, f))
        pts.append(rng.random((noise, 2)) * box * 1.3 - box * 0.65)
        ts.append(np.full(noise, f))
    return np.vstack(pts).astype(np.float32), np.concatenate(ts).astype(np.float32), rng


def test_mixed_cells_and_minimum_in_a_mixed_cell(gpu):
    """A cell holding core and non-core points, and a component whose smallest original index is
    a core point of such a cell (rows permuted, then that point moved to row 0: the component's
    key is taken from a cell that is not all core)."""
    xy, t, rng = _blob_cloud(11, range(4))
    p = rng.permutation(len(xy))
    xy, t = xy[p], t[p]
    core, cell = _core(xy, t), _cells(xy, t)
    n_core = np.bincount(cell, weights=core).astype(np.int64)
    n_all = np.bincount(cell)
    mixed = (n_core > 0) & (n_core < n_all)
    assert mixed.any()
    dense = int(np.argmax(n_all))
    pick = np.flatnonzero(core & mixed[cell] & (cell != dense))
    assert len(pick)
    i = int(pick[0])  # a core point of a mixed cell -> row 0, its component's smallest index
    xy[[0, i]], t[[0, i]] = xy[[i, 0]], t[[i, 0]]
    core, cell = _core(xy, t), _cells(xy, t)
    n_core = np.bincount(cell, weights=core).astype(np.int64)
    assert core[0] and 0 < n_core[cell[0]] < np.bincount(cell)[cell[0]]
    assert cell[0] != int(np.argmax(np.bincount(cell)))
    exp = _check(xy, t)
    assert exp[0] == 0 and (exp == 0).sum() > 1  # row 0 names the first component
    assert (exp[~core] >= 0).any() and (exp == -1).any()  # border points and noise


def _straddle_cloud():
    """One cell of 2,500 near-identical points (its run of sorted points crosses the 8 x 256 tile
    and several waves) next to a row of singleton cells, three frames."""
    rng = np.random.default_rng(5)
    pts, ts = [], []
    for f in range(3):
        pts.append(np.array([100.0, 100.0]) + rng.random((2500 if f == 1 else 40, 2)) * 1e-3)
        ts.append(np.full(len(pts[-1]), f))
        line = np.column_stack([100.0 + 6.0 * np.arange(1, 40), np.full(39, 100.0)])
        pts.append(line)
        ts.append(np.full(len(line), f))
    return np.vstack(pts).astype(np.float32), np.concatenate(ts).astype(np.float32)


def test_run_across_tiles_next_to_singleton_cells(gpu):
    xy, t = _straddle_cloud()
    cell = _cells(xy, t)
    cnt = np.bincount(cell)
    assert cnt.max() > 2048 and (cnt == 1).sum() >= 100
    core = _core(xy, t)
    assert core.any() and (~core).any()
    exp = _check(xy, t)
    assert (exp[~core] >= 0).any()  # singletons within eps of the big cell are border points


@pytest.mark.parametrize("n", [1, 63, 65])
def test_tiny_clouds(gpu, n):
    """Fewer points than a wave, and one more: a clump (core once it holds min_samples points)
    followed by singleton cells."""
    rng = np.random.default_rng(n)
    clump = np.array([10.0, 10.0]) + rng.random((40, 2))
    line = np.column_stack([10.0 + 6.0 * np.arange(1, 26), np.full(25, 10.0)])
    xy = np.vstack([clump, line]).astype(np.float32)[:n]
    t = np.zeros(n, np.float32)
    core = _core(xy, t)
    assert core.any() == (n >= MS)
    _check(xy, t)


def test_min_samples_one_every_point_core(gpu):
    """min_samples = 1: every point is core; isolated singleton components and occupied cells
    next to each other."""
    rng = np.random.default_rng(3)
    sparse = rng.random((1500, 2)) * 2000.0
    clumps = np.vstack([c + rng.normal(0, 4.0, (200, 2)) for c in rng.random((6, 2)) * 2000.0])
    xy = np.vstack([sparse, clumps]).astype(np.float32)
    t = rng.integers(0, 3, len(xy)).astype(np.float32)
    assert _core(xy, t, ms=1).all()
    side = 0.7 * EPS * (1.0 + 2.0 ** -20)
    cx = np.floor((xy[:, 0] - xy[:, 0].min()).astype(np.float64) / side).astype(np.int64)
    cy = np.floor((xy[:, 1] - xy[:, 1].min()).astype(np.float64) / side).astype(np.int64)
    occ = set(zip(t.astype(int).tolist(), cy.tolist(), cx.tolist()))
    assert any((f, y, x + 1) in occ for f, y, x in occ)  # adjacent occupied cells
    exp = _check(xy, t, ms=1)
    assert (exp >= 0).all()
    assert (np.bincount(exp) == 1).sum() >= 100  # isolated singleton components


@pytest.mark.parametrize("eps_t", [0.0, 3.0])
def test_time_gaps_and_reach(gpu, eps_t):
    """Times {0, 1, 4, 5, 9}: eps_t = 3 joins 1 and 4 (gap 3) but not 5 and 9 (gap 4); eps_t = 0
    joins nothing across frames."""
    xy, t, _ = _blob_cloud(21, [0, 1, 4, 5, 9], n_blobs=6, per=60, noise=200)
    assert sorted(np.unique(t).tolist()) == [0.0, 1.0, 4.0, 5.0, 9.0]
    exp = _check(xy, t, et=eps_t)
    spans = [set(np.unique(t[exp == k]).tolist()) for k in range(int(exp.max()) + 1)]
    assert spans
    if eps_t == 0.0:
        assert all(len(s) == 1 for s in spans)
    else:
        assert any({1.0, 4.0} <= s for s in spans)
        assert not any(9.0 in s and len(s) > 1 for s in spans)


@pytest.mark.parametrize("order", ["time_ordered", "shuffled"])
def test_both_grid_builds(gpu, order):
    """The same cloud time-ordered (slab counting sort) and row-shuffled (radix sort)."""
    xy, t, rng = _blob_cloud(31, range(5))
    if order == "shuffled":
        p = rng.permutation(len(xy))
        xy, t = xy[p], t[p]
        assert (np.diff(t) < 0).any()
    else:
        assert (np.diff(t) >= 0).all()
    core = _core(xy, t)
    assert core.any() and (~core).any()
    _check(xy, t)


def test_stack_path_against_oracle_run_path(gpu):
    from _stack_check import check_stack_vs_oracle, oracle_stack
    from oracle import path as op
    from rpt.pipeline import FrameStackPipeline, PathParams
    from rpt.synth import DeviceSynth, SynthConfig

    cfg = SynthConfig(n_frames=14, rows=1024, n_targets=14, clutter_density=0.01)
    ds = DeviceSynth(cfg, gpu)
    pipe = FrameStackPipeline(cfg.gains, cfg.rows, cfg.bins, PathParams(), gpu)
    pipe.set_geometry(np.full(cfg.rows, cfg.scale, np.float32), ds.geo.cos_t, ds.geo.sin_t,
                      cfg.n_frames * len(cfg.gains))
    echo = ds.echo()
    res = pipe.run(echo, keep_points=True)
    torch.cuda.synchronize()
    frames = oracle_stack(echo.cpu().numpy(), cfg, ds.geo)
    o_frames, o_labels, o_clusters, o_trk = op.run_path(frames)
    check_stack_vs_oracle(res, cfg.n_frames, frames, o_frames, o_labels, o_clusters, o_trk)


# ---- A/B parity: children on librpt_ab.so against librpt.so in this process, the 14-frame stack
RUN = r'''
import numpy as np, torch
from rpt.pipeline import FrameStackPipeline, PathParams
from rpt.synth import DeviceSynth, SynthConfig

def run_stack():
    dev = torch.device("cuda", 0)
    cfg = SynthConfig(n_frames=14, rows=1024, n_targets=14, clutter_density=0.01)
    ds = DeviceSynth(cfg, dev)
    pipe = FrameStackPipeline(cfg.gains, cfg.rows, cfg.bins, PathParams(), dev)
    pipe.set_geometry(np.full(cfg.rows, cfg.scale, np.float32), ds.geo.cos_t, ds.geo.sin_t,
                      cfg.n_frames * 3)
    res = pipe.run(ds.echo(), keep_points=True).finish()
    out = {"labels": res.labels.cpu().numpy()}
    seg = {k: np.asarray(v) for k, v in res.seg.items()}
    key = np.lexsort((seg["label"], seg["frame"]))
    for k, v in seg.items():
        out["s_" + k] = v[key]
    fo, order = res.frame_order_offsets, res.frame_order  # rows in reference order
    out["rows"] = np.array([(f, seg["label"][s], seg["count"][s], seg["cx"][s], seg["cy"][s],
                             seg["mi"][s]) for f in range(len(fo) - 1)
                            for s in order[fo[f]:fo[f + 1]]], np.float64).reshape(-1, 6)
    objs = res.tracker.objects()
    out["obj_id"] = np.array([o.object_id for o in objs])
    out["obj_pos"] = (np.vstack([np.vstack(o.positions) for o in objs]) if objs
                      else np.zeros((0, 2)))
    return out
'''


@pytest.fixture(scope="module")
def shipped_stack(gpu):
    from rpt import _abi

    assert _abi.load()._name.endswith("librpt.so")
    ns = {}
    exec(RUN, ns)  # noqa: S102 (the same code the children run)
    return ns["run_stack"]()


# (switches, per-cell path expected): RPT_UF_COMPRESS=1 keeps the per-point init because
# k_compress walks every core point's parent chain; the child without a switch pins down that
# the stack takes the per-cell path at all (the A/B build reports it under RPT_STATS)
AB_CASES = [({"RPT_CELL_COMP": "0"}, 0), ({"RPT_LABEL_ORIG": "2"}, 1),
            ({"RPT_UF_COMPRESS": "1"}, 0), ({}, 1)]


@pytest.mark.parametrize("switch,per_cell", AB_CASES,
                         ids=["cell_comp_off", "label_orig", "uf_compress", "defaults"])
def test_ab_children_match_shipped_library(gpu, shipped_stack, switch, per_cell):
    from rpt import _build

    assert _build.LIB_AB.exists(), "librpt_ab.so missing: run __graft_entry__.build()"
    ref = shipped_stack
    assert (ref["labels"] >= 0).any() and len(ref["rows"]) and len(ref["obj_id"])
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "out.npz")
        code = (f"import sys\nsys.path[:0] = {sys.path!r}\n" + RUN +
                "from rpt import _abi\nassert _abi.load()._name.endswith('librpt_ab.so')\n"
                f"import numpy as np\nnp.savez({out!r}, **run_stack())\n")
        env = dict(os.environ, RPT_LIB=str(_build.LIB_AB), RPT_STATS="1", **switch)
        r = subprocess.run([sys.executable, "-c", code], env=env, timeout=240,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        paths = [ln for ln in r.stderr.splitlines() if "cell_comp=" in ln]
        assert paths and all(f"all_mutual=1 cell_comp={per_cell}" in ln for ln in paths), paths
        got = np.load(out)
        assert sorted(got.files) == sorted(ref)
        for k in ref:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{k} with {switch}")
