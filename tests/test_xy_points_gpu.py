"""The xy-only sorted points of ST-DBSCAN (float2 {x, y} instead of float4 {x, y, t, t}: 2-D,
integral times and eps_t, one time value per slab, every time finite, time-ordered input, the
fused local run on its per-cell path with eps_t <= 2) against the C oracle: exact label equality
through rpt.processors.st_dbscan, the 14-frame stack through FrameStackPipeline against
oracle.run_path, and A/B children (librpt_ab.so) that must match librpt.so bit for bit and report
the expected layout on the `[rpt stats] ... cell_comp=... xy_points=...` line (RPT_STATS).  Every
case first asserts on the CPU the structure it is there for.

The layout rule (DbscanState::xy_rule): every point-reading kernel of the run must know the
float2 layout, and those are only the default fused per-cell path's.  So RPT_CELL_COMP=0 and
RPT_UF_COMPRESS=1 (per-point union paths: k_union_nm / k_compress keep float4) report
xy_points=0, as do RPT_XY_POINTS=0, non-integral, non-finite or unordered times, a fractional
eps_t, 3-D input and a coarsened cell side."""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import oracle
from test_cell_components_gpu import RUN, _blob_cloud, _cells, _core

pytestmark = pytest.mark.gpu

EPS, MS = 8.0, 15
SIDE = 0.7 * EPS * (1.0 + 2.0 ** -20)


def _st(xy, t, eps, et, ms):
    from rpt.processors import st_dbscan

    return st_dbscan(xy, t, eps, et, ms)


def _check(xy, t, eps=EPS, et=2.0, ms=MS):
    assert len(xy) <= 20000 and xy.dtype == np.float32 and t.dtype == np.float32
    exp = oracle.stdbscan(xy, t, eps, et, ms)
    got = _st(xy, t, eps, et, ms)
    np.testing.assert_array_equal(got, exp)
    return exp


# ---------------------------------------------------------------- the clouds
def _cell_size_cloud():
    """Per frame one row of adjacent cells holding 1, 4, 5, 16, 17 and N points (N = 2,500 in frame
    1: a run across several waves; 41 and 40 in frames 0 and 2), clumps at the cell centres: a
    cell's points are adjacent to the next cell's (5.6 apart) and to no cell's further on."""
    rng = np.random.default_rng(7)
    pts, ts = [], []
    for f, big in enumerate([41, 2500, 40]):
        for cx, k in enumerate([1, 4, 5, 16, 17, big]):
            c = np.array([(cx + 0.5) * SIDE, 0.5 * SIDE])
            p = c + (rng.random((k, 2)) - 0.5) * 0.5
            if f == 0 and cx == 0:
                p[:] = 0.0  # the grid origin
            pts.append(p)
            ts.append(np.full(k, f))
    return np.vstack(pts).astype(np.float32), np.concatenate(ts).astype(np.float32)


def _boundary_cloud():
    """Groups 200 apart in y, two frames (eps_t = 0 keeps them apart).  Core groups: a point A
    with 13 more points 0.02 - 0.05 to its left (14 in one cell) and a single point B at
    eps (1 + d) to its right, so A is core iff the A-B pair passes; border groups: 20 points
    (core whatever happens) with the rightmost, P, 0.02 clear of the rest, and a single Q at
    eps (1 + d) from P, labelled iff the P-Q pair passes.  d runs over both signs within 4e-6."""
    ds = [-4e-6, -2e-6, -1e-6, -3e-7, 3e-7, 1e-6, 2e-6, 4e-6]
    rng = np.random.default_rng(2)
    pts = []
    for g, d in enumerate(ds * 2):
        y = 200.0 * g
        k = 13 if g < len(ds) else 19
        a = np.array([1.0, y + 1.0])
        left = a - np.column_stack([0.02 + 0.03 * rng.random(k), np.zeros(k)])
        pts += [a[None], left, (a + np.array([EPS * (1.0 + d), 0.0]))[None]]
    one = np.vstack(pts)
    xy = np.vstack([one, one]).astype(np.float32)
    t = np.repeat([0.0, 1.0], len(one)).astype(np.float32)
    return xy, t


def _slab_cloud(frames, per_frame=36, seed=9):
    """per_frame points per frame within 8 x 8 cells: a clump of 20 and 16 scattered points."""
    rng = np.random.default_rng(seed)
    pts, ts = [], []
    for f in frames:
        pts.append(np.array([20.0, 20.0]) + rng.normal(0, 1.5, (20, 2)).clip(-7, 7))
        pts.append(rng.random((per_frame - 20, 2)) * 40.0)
        ts.append(np.full(per_frame, f))
    xy = np.vstack(pts).astype(np.float32)
    xy[0] = 0.0
    return xy, np.concatenate(ts).astype(np.float32)


def _writer_chunks(xy, t):
    """Blocks per slab of the grid build's counting sort, as build_t picks them at standard
    density (1: k_slab_bucket, more: k_slab_chunk_scatter)."""
    n = len(xy)
    nx = int(np.floor((float(xy[:, 0].max()) - float(xy[:, 0].min())) / SIDE)) + 1
    ny = int(np.floor((float(xy[:, 1].max()) - float(xy[:, 1].min())) / SIDE)) + 1
    nt = int(t.max() - t.min()) + 1
    assert n // nt <= 8 * 16384
    ch = min(max(1, (512 + nt - 1) // nt), 64)
    while ch > 1 and nt * ch * nx * ny > 4 * n:
        ch -= 1
    return ch


FALLBACK_T = 3  # frames of the fallback clouds
CELLS_ET, CELLS_MS = 1.0, 16  # the cell-size cloud: a lone point, border cells and core cells


def _fallback_clouds():
    xy, t, rng = _blob_cloud(41, range(FALLBACK_T), n_blobs=5, per=60, noise=150)
    out = {}
    t1 = t.copy()
    t1[len(t) // 2] += 0.5
    out["nonintegral_t"] = (xy, t1, 2.0)
    t2 = t.copy()
    t2[len(t) // 3] = np.nan
    out["nan_t"] = (xy, t2, 2.0)
    out["half_eps_t"] = (xy, t, 0.5)
    p = rng.permutation(len(xy))
    out["shuffled"] = (xy[p], t[p], 2.0)
    out["three_d"] = (np.column_stack([xy, rng.normal(0, 2.0, len(xy))]).astype(np.float32), t, 2.0)
    far = np.vstack([xy, [[13000.0, 13000.0]]]).astype(np.float32)
    out["coarsened"] = (far, np.append(t, t[-1]).astype(np.float32), 2.0)
    return out


# ---------------------------------------------------------------- A/B children over the clouds
CHILD = r'''
import sys
import numpy as np
from rpt import _abi
from rpt.processors import st_dbscan
assert _abi.load()._name.endswith("librpt_ab.so")
z = np.load(sys.argv[1])
out = {}
for name in sorted(k[3:] for k in z.files if k.startswith("xy_")):
    sys.stderr.write(f"[cloud] {name}\n")
    sys.stderr.flush()
    eps, et, ms = z["p_" + name]
    out[name] = st_dbscan(z["xy_" + name], z["t_" + name], float(eps), float(et), int(ms))
np.savez(sys.argv[2], **out)
'''


def _clouds():
    c = {"cells": (*_cell_size_cloud(), CELLS_ET), "slabs520": (*_slab_cloud(range(520)), 1.0),
         "slabs8": (*_slab_cloud(range(8)), 1.0)}
    c.update(_fallback_clouds())
    return c


@pytest.fixture(scope="module")
def shipped_labels(gpu):
    from rpt import _abi

    assert _abi.load()._name.endswith("librpt.so")
    return {k: _st(xy, t, EPS, et, _ms(k)) for k, (xy, t, et) in _clouds().items()}


def _ms(name):
    return CELLS_MS if name == "cells" else MS


def _run_children(switch):
    """One librpt_ab.so child over every cloud: {cloud: (labels, its `cell_comp=` lines)}."""
    from rpt import _build

    assert _build.LIB_AB.exists(), "librpt_ab.so missing: run __graft_entry__.build()"
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.npz"), os.path.join(d, "out.npz")
        arrs = {}
        for k, (xy, t, et) in _clouds().items():
            arrs["xy_" + k], arrs["t_" + k] = xy, t
            arrs["p_" + k] = np.array([EPS, et, _ms(k)])
        np.savez(src, **arrs)
        code = f"import sys\nsys.path[:0] = {sys.path!r}\n" + CHILD
        env = dict(os.environ, RPT_LIB=str(_build.LIB_AB), RPT_STATS="1", **switch)
        r = subprocess.run([sys.executable, "-c", code, src, dst], env=env, timeout=240,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        got = np.load(dst)
        lines, cur = {}, None
        for ln in r.stderr.splitlines():
            if ln.startswith("[cloud] "):
                cur = ln[8:]
                lines[cur] = []
            elif "cell_comp=" in ln:
                lines[cur].append(ln)
        return {k: (got[k], lines[k]) for k in got.files}


# (switches, xy_points expected on the eligible clouds)
CHILD_CASES = [({}, 1), ({"RPT_XY_POINTS": "0"}, 0),
               ({"RPT_SLAB_CHUNKS": "1", "RPT_CELL_BOX_MIXED": "2"}, 1),
               ({"RPT_CELL_BOX_MIXED": "0"}, 1),
               # the one-block-per-slab chunk scan where the coalesced scan is the default: the
               # "cells" cloud (3 frames, 6 x 1 cells: 64 chunks per slab); "slabs8" takes 2
               # chunks and "slabs520" one block, below the coalesced scan's 8
               ({"RPT_CHUNK_SCAN": "1"}, 1)]
ELIGIBLE = ("cells", "slabs520", "slabs8")


def _coalesced_scan(xy, t):
    """build_t's rule for the coalesced chunk scan: CH >= 8 and nt * CH * nx * ny <= 4 n (the
    second holds for every CH > 1 that _writer_chunks returns)."""
    return _writer_chunks(xy, t) >= 8


@pytest.mark.parametrize("switch,xy", CHILD_CASES,
                         ids=["defaults", "xy_off", "one_block_mixed_box", "lanes_box",
                              "chunk_scan"])
def test_children_over_the_clouds(gpu, shipped_labels, switch, xy):
    """Both writers (RPT_SLAB_CHUNKS=1: k_slab_bucket for every cloud; default: the chunked
    scatter for the short stacks) and both box kernels (RPT_CELL_BOX_MIXED=2: the one-lane small
    cells at <= kCbSmall = 4 points; 0 / default at this size: 16 lanes per cell), the layout
    each run reports, and labels equal to librpt.so's."""
    if "RPT_CHUNK_SCAN" in switch:
        scans = {k: _coalesced_scan(xy, t) for k, (xy, t, _) in _clouds().items() if k in ELIGIBLE}
        assert scans == {"cells": True, "slabs520": False, "slabs8": False}, scans
    res = _run_children(switch)
    assert sorted(res) == sorted(shipped_labels)
    for k, (lab, lines) in res.items():
        np.testing.assert_array_equal(lab, shipped_labels[k], err_msg=f"{k} with {switch}")
        want = xy if k in ELIGIBLE else 0
        assert lines and all(ln.rstrip().endswith(f"xy_points={want}") for ln in lines), (k, lines)
        if k in ELIGIBLE:
            assert all("all_mutual=1 cell_comp=1" in ln for ln in lines), (k, lines)


# ---------------------------------------------------------------- 1. cell sizes
def test_cell_sizes_around_the_small_cell_and_lane_group_limits(gpu):
    xy, t = _cell_size_cloud()
    cell = _cells(xy, t)
    cnt = np.bincount(cell)
    cnt = cnt[cnt > 0]
    assert {1, 4, 5, 16, 17, 2500} <= set(cnt.tolist())
    # the sorted order is (slab, cell): the 2,500-point run starts at an odd index (8-byte but not
    # 16-byte aligned in the float2 array)
    order = np.argsort(cell, kind="stable")
    big = int(np.argmax(np.bincount(cell)))
    start = int(np.flatnonzero(cell[order] == big)[0])
    assert start % 2 == 1, start
    core = _core(xy, t, EPS, CELLS_ET, CELLS_MS)
    assert core.any() and (~core).any()
    exp = _check(xy, t, et=CELLS_ET, ms=CELLS_MS)
    assert (exp[~core] >= 0).any() and (exp == -1).any()  # border points and noise


# ---------------------------------------------------------------- 2. the float64 boundary
def test_pairs_at_the_float64_boundary(gpu):
    xy, t = _boundary_cloud()
    x64 = xy.astype(np.float64)
    e2 = EPS * EPS
    lo, hi = e2 * (1.0 - 1e-5), e2 * (1.0 + 1e-5)
    sel = np.flatnonzero(t == 0.0)
    d2 = ((x64[sel, None, :] - x64[None, sel, :]) ** 2).sum(-1)
    near = (d2 > lo) & (d2 <= hi)  # the float32 screen's undecided band
    assert (near & (d2 <= e2)).any() and (near & (d2 > e2)).any()
    i, j = np.nonzero(near)
    assert (_cells(xy[sel], t[sel])[i] != _cells(xy[sel], t[sel])[j]).all()  # neighbouring cells
    # such a pair decides a core flag: the flags differ between the band's two ends
    core_lo, core_hi = (d2 <= lo).sum(1) >= MS, (d2 <= hi).sum(1) >= MS
    core = (d2 <= e2).sum(1) >= MS
    assert (core_lo != core_hi).any() and (core != core_lo).any() and (core != core_hi).any()
    # ... and a border label: a non-core point whose only core neighbours lie in the band
    has_lo = ((d2 <= lo) & core[None, :]).any(1)
    has_hi = ((d2 <= hi) & core[None, :]).any(1)
    has = ((d2 <= e2) & core[None, :]).any(1)
    dec = ~core & (has_lo != has_hi)
    assert (dec & has).any() and (dec & ~has).any()
    exp = _check(xy, t, et=0.0)
    e0 = exp[sel]
    assert ((e0 >= 0) == (core | has)).all()


# ---------------------------------------------------------------- 3. slab times
def _groups(times, eps_t):
    u = sorted(set(times))
    out = [[u[0]]]
    for a, b in zip(u, u[1:]):
        if b - a <= eps_t:
            out[-1].append(b)
        else:
            out.append([b])
    return [frozenset(g) for g in out]


@pytest.mark.parametrize("eps_t", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("frames", [[-3, -2, 0, 1, 5], [16777000, 16777001, 16777003, 16777005]],
                         ids=["negative_start_gaps", "near_2p24"])
def test_slab_times_with_gaps(gpu, frames, eps_t):
    """Integral times with empty slabs between occupied ones: a slab's time is its points' own
    value, not an index.  The blobs sit at the same place in every frame, so a cluster spans
    exactly a run of frames whose gaps are within eps_t."""
    xy, t, _ = _blob_cloud(23, frames, n_blobs=5, per=60, noise=150)
    assert sorted(np.unique(t).tolist()) == [float(f) for f in frames]  # exact in float32
    assert len(np.unique(t)) < int(t.max() - t.min()) + 1  # empty slabs
    exp = _check(xy, t, et=eps_t)
    spans = {frozenset(np.unique(t[exp == k]).tolist()) for k in range(int(exp.max()) + 1)}
    groups = _groups([float(f) for f in frames], eps_t)
    assert spans and all(any(s <= g for g in groups) for s in spans), spans
    assert all(g in spans for g in groups), (spans, groups)


# ---------------------------------------------------------------- 4. both writers
@pytest.mark.parametrize("frames", [520, 8])
def test_both_writers(gpu, frames):
    xy, t = _slab_cloud(range(frames))
    ch = _writer_chunks(xy, t)
    assert (ch == 1) if frames >= 512 else (ch > 1), ch
    core = _core(xy, t, EPS, 1.0, MS)
    assert core.any() and (~core).any()
    exp = _check(xy, t, et=1.0)
    assert (exp[~core] >= 0).any() and (exp == -1).any()  # border points and noise


# ---------------------------------------------------------------- 5. fallbacks
@pytest.mark.parametrize("name", ["nonintegral_t", "nan_t", "half_eps_t", "shuffled", "three_d",
                                  "coarsened"])
def test_fallbacks_stay_exact(gpu, name):
    xy, t, et = _fallback_clouds()[name]
    if name == "nonintegral_t":
        assert (t != np.floor(t)).sum() == 1
    elif name == "nan_t":
        assert np.isnan(t).sum() == 1
    elif name == "half_eps_t":
        assert np.array_equal(t, np.floor(t)) and et == 0.5
    elif name == "shuffled":
        assert (np.diff(t) < 0).any()
    elif name == "three_d":
        assert xy.shape[1] == 3
    else:  # more 0.7 eps cells than the cell cap: the side doubles
        ext = xy.max(0).astype(np.float64) - xy.min(0).astype(np.float64)
        cells = np.prod(np.floor(ext / SIDE) + 1.0) * FALLBACK_T
        assert cells > max(1 << 22, 4 * len(xy))
    exp = _check(xy, t, et=et)
    assert (exp >= 0).any() and (exp == -1).any()


# ---------------------------------------------------------------- 6. the stack path
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


@pytest.fixture(scope="module")
def shipped_stack(gpu):
    from rpt import _abi

    assert _abi.load()._name.endswith("librpt.so")
    ns = {}
    exec(RUN, ns)  # noqa: S102 (the same code the children run)
    return ns["run_stack"]()


# (switches, per-cell path, xy points): see the module docstring for the rule
STACK_CASES = [({}, 1, 1), ({"RPT_XY_POINTS": "0"}, 1, 0), ({"RPT_CELL_COMP": "0"}, 0, 0),
               ({"RPT_UF_COMPRESS": "1"}, 0, 0)]


@pytest.mark.parametrize("switch,per_cell,xy", STACK_CASES,
                         ids=["defaults", "xy_off", "cell_comp_off", "uf_compress"])
def test_stack_children_match_shipped_library(gpu, shipped_stack, switch, per_cell, xy):
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
        assert paths and all(f"all_mutual=1 cell_comp={per_cell} xy_points={xy}" in ln
                             for ln in paths), paths
        got = np.load(out)
        assert sorted(got.files) == sorted(ref)
        for k in ref:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{k} with {switch}")
