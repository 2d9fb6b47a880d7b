"""The stack driver's narrow point layout (u8 echo of 1024 bins: no per-point frame slots, a
point's frame comes from the frame offsets) against the oracle's run_path, on small hand-built
stacks: 1024 bins, 32-48 rows, 3 gains.

Every case runs the same pipeline twice (the first run sizes the buffers, the second takes the
speculative capacity-bounded K1 write) and checks both runs: K1 point count, labels, per-frame
cluster rows, tracker state (check_stack_vs_oracle), the frame offsets before and after the land
filter, and the keep_points hand-back (x, y, intensity as float32, frame ids, gain) against the
oracle's frames.  Every case first asserts on the CPU the structure it is there for."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest
import torch

from _stack_check import check_stack_vs_oracle
from oracle import path as op

pytestmark = pytest.mark.gpu

GAINS = (40, 50, 75)
BINS = 1024
SCALE = 231.5
TILE = 4096  # points per land-compaction tile (csrc/land.hip kCompTile)


def _geo(rows, step=16.0):
    from rpt.core.transforms import trig_tables

    angle = (np.arange(rows) * step).astype(np.float32)
    cos_t, sin_t = trig_tables(angle)
    return SimpleNamespace(cos_t=cos_t, sin_t=sin_t)


def _scene(F, R, seed, empty=(), clutter=0.004, targets=3, tgt=(4, 48), land=(6, 160)):
    """Clutter (11-39), `targets` blocks of tgt rows x bins (60-99, fill 0.8, drifting two bins a
    frame) and one persistent bright patch of land rows x bins (150-255, fill 0.5) in the last
    rows, in every frame not listed in `empty`."""
    rng = np.random.default_rng(seed)
    e = np.zeros((F, len(GAINS), R, BINS), np.uint8)
    for f in range(F):
        if f in empty:
            continue
        for g in range(len(GAINS)):
            m = rng.random((R, BINS)) < clutter
            e[f, g][m] = rng.integers(11, 40, int(m.sum()))
            for k in range(targets):
                r0, b0 = 2 + (tgt[0] + 2) * k, 300 + 150 * k + 2 * f
                m = rng.random(tgt) < 0.8
                blk = e[f, g, r0:r0 + tgt[0], b0:b0 + tgt[1]]
                blk[m] = rng.integers(60, 100, int(m.sum()))
            if land:
                m = rng.random(land) < 0.5
                blk = e[f, g, R - 2 - land[0]:R - 2, 820:820 + land[1]]
                blk[m] = rng.integers(150, 256, int(m.sum()))
    return e


def _frames(echo, geo, scale=SCALE, threshold=10.0, stride=4):
    F, G, R, _ = echo.shape
    sc = np.full(R, scale, np.float32)
    per_frame = [{gain: op.polar_scatter(echo[f, k], sc, geo.cos_t, geo.sin_t, threshold, stride)
                  for k, gain in enumerate(GAINS)} for f in range(F)]
    return op.build_frames(per_frame)


def _offsets(frames, F):
    n = np.zeros(F, np.int64)
    for fid, p, _ in frames:
        n[fid] = len(p)
    return np.concatenate([[0], np.cumsum(n)])


def _oracle(frames, resolution, **kw):
    """run_path with the land grid's resolution as a parameter: the gate of run_path (:954, more
    than 10 built frames), then run_path over the filtered frames."""
    cells = None
    if len(frames) > 10:
        frames_in, _, _, land, (xe, ye) = op.land_filter(frames, resolution=resolution)
        cells = (len(xe) - 1) * (len(ye) - 1)
        assert land.any() and sum(len(p) for _, p, _ in frames_in) < \
            sum(len(p) for _, p, _ in frames), "the land filter must remove points"
    else:
        frames_in = frames
    return op.run_path(frames_in, land=False, **kw), cells


def _run_and_check(gpu, echo, geo, monkeypatch, resolution=5.0, params=None, scale=SCALE,
                   full=True):
    """Two runs of one pipeline against the oracle.  Returns (result, frames, oracle outputs,
    land cells)."""
    from rpt import _abi, pipeline
    from rpt.pipeline import FrameStackPipeline, PathParams

    monkeypatch.setattr(pipeline, "LAND_GRID_RESOLUTION", float(resolution))
    p = params or PathParams()
    F, G, R, B = echo.shape
    assert B == 1024 and echo.dtype == np.uint8  # the grouped K1 path, hence the narrow layout
    frames = _frames(echo, geo, scale, p.threshold, p.stride)
    fo_k1 = _offsets(frames, F)
    if full:
        (o_frames, o_labels, o_clusters, o_trk), cells = _oracle(
            frames, resolution, eps_space=p.eps_space, eps_time=p.eps_time,
            min_samples=p.min_samples)
    else:
        assert len(frames) <= 10
        o_frames, o_labels, o_clusters, o_trk, cells = frames, None, None, None, None
    fo_in = _offsets(o_frames, F)
    pipe = FrameStackPipeline(GAINS, R, B, p, gpu)
    pipe.set_geometry(np.full(R, scale, np.float32), geo.cos_t, geo.sin_t, F * G)
    dev_echo = torch.from_numpy(echo).to(gpu)
    assert dev_echo.data_ptr() % 16 == 0
    res = None
    for _ in range(2):
        res = pipe.run(dev_echo, keep_points=True)
        torch.cuda.synchronize()
        for which, exp in ((0, fo_k1), (1, fo_in)):
            got = np.empty(F + 1, np.int64)
            _abi.check(pipe.lib.rpt_stack_frame_offsets(pipe._h, which,
                                                        got.ctypes.data_as(_abi.c_i64p)))
            np.testing.assert_array_equal(got, exp, err_msg=f"frame offsets {which}")
        assert res.n_points == fo_k1[-1] and res.n_clustered_input == fo_in[-1]
        pts = {k: v.cpu().numpy() for k, v in res.points.items()}
        assert pts["v"].dtype == np.float32
        exp_p = np.vstack([q for _, q, _ in o_frames])
        np.testing.assert_array_equal(pts["x"], exp_p[:, 0])
        np.testing.assert_array_equal(pts["y"], exp_p[:, 1])
        np.testing.assert_array_equal(pts["v"], exp_p[:, 2])
        np.testing.assert_array_equal(pts["gain"], np.concatenate([g for _, _, g in o_frames]))
        np.testing.assert_array_equal(
            pts["frame"], np.concatenate([np.full(len(q), fid, np.int32) for fid, q, _ in o_frames]))
        if full:
            check_stack_vs_oracle(res, F, frames, o_frames, o_labels, o_clusters, o_trk)
            assert (o_labels >= 0).any() and (o_labels == -1).any()
    return res, frames, (o_frames, o_labels, o_clusters, o_trk), cells


# ---------------------------------------------------------------- 1. empty frames
def test_empty_frames_among_built_ones(gpu, monkeypatch):
    F, empty = 16, (0, 7, 8, 15)
    echo = _scene(F, 32, 1, empty=empty)
    geo = _geo(32)
    frames = _frames(echo, geo)
    assert [fid for fid, _, _ in frames] == [f for f in range(F) if f not in empty]
    assert len(frames) > 10  # the land filter runs
    fo = _offsets(frames, F)
    assert fo[0] == fo[1] and fo[7] == fo[8] == fo[9] and fo[15] == fo[16]  # repeated offsets
    _run_and_check(gpu, echo, geo, monkeypatch)


# ---------------------------------------------------------------- 2. the land gate
@pytest.mark.parametrize("built", [10, 11])
def test_either_side_of_the_land_gate(gpu, monkeypatch, built):
    """10 built frames: no land filter, K9 and the hand-back take the K1 offsets (one empty frame
    among them); 11: the filter runs."""
    F = built + 1
    echo = _scene(F, 32, 2, empty=(3,))
    geo = _geo(32)
    assert len(_frames(echo, geo)) == built
    res, frames, (o_frames, *_), cells = _run_and_check(gpu, echo, geo, monkeypatch)
    filtered = sum(len(p) for _, p, _ in o_frames) < sum(len(p) for _, p, _ in frames)
    assert filtered == (built > 10) and (res.n_land_cells > 0) == (built > 10)


# ---------------------------------------------------------------- 3. many tiny frames
def test_many_tiny_frames_in_one_tile(gpu, monkeypatch):
    F = 120
    echo = _scene(F, 32, 3, empty=(40, 41, 42), clutter=0.0006, targets=1, tgt=(3, 32),
                  land=(3, 48))
    geo = _geo(32)
    fo = _offsets(_frames(echo, geo), F)
    n = np.diff(fo)
    assert n[n > 0].min() >= 24 and n.max() <= 300, (n.min(), n.max())
    per_tile = np.bincount(fo[:-1][n > 0] // TILE)
    assert fo[-1] > TILE and per_tile.max() >= 30, per_tile  # tens of frames begin in one tile
    _run_and_check(gpu, echo, geo, monkeypatch)


# ---------------------------------------------------------------- 4. a boundary on a tile edge
def _pad_frame_to(echo, f, target):
    """Clutter samples added to the last gain of frame f until the frame has `target` points
    (each sweep keeps every fourth sample above the threshold: ceil(kept / 4) points)."""
    cnt = lambda g: -(-int((echo[f, g] > 10).sum()) // 4)  # noqa: E731
    need = target - cnt(0) - cnt(1)
    g = len(GAINS) - 1
    assert need > cnt(g)
    rng = np.random.default_rng(99)
    free = np.flatnonzero(echo[f, g, :-10].ravel() == 0)
    add = rng.permutation(free)[:4 * need - int((echo[f, g] > 10).sum())]
    flat = echo[f, g].reshape(-1)
    flat[add] = rng.integers(11, 40, len(add))
    assert cnt(0) + cnt(1) + cnt(g) == target


def test_frame_boundary_on_a_tile_edge(gpu, monkeypatch):
    F = 12
    echo = _scene(F, 48, 4)
    _pad_frame_to(echo, 0, TILE)
    _pad_frame_to(echo, 5, 3 * TILE - int(_offsets(_frames(echo, _geo(48)), F)[5]))
    geo = _geo(48)
    fo = _offsets(_frames(echo, geo), F)
    assert fo[1] == TILE and fo[6] == 3 * TILE and fo[-1] % TILE != 0, fo
    _run_and_check(gpu, echo, geo, monkeypatch)


# ---------------------------------------------------------------- 5. less than one tile
def test_stack_smaller_than_one_tile(gpu, monkeypatch):
    F = 12
    echo = _scene(F, 32, 5, clutter=0.001, targets=2, tgt=(3, 40), land=(3, 64))
    geo = _geo(32)
    fo = _offsets(_frames(echo, geo), F)
    assert 0 < fo[-1] < TILE and (np.diff(fo) > 0).all()
    _run_and_check(gpu, echo, geo, monkeypatch)


# ---------------------------------------------------------------- 6. land grid sizes
def _cells(frames, res):
    x = np.concatenate([p[:, 0] for _, p, _ in frames])
    y = np.concatenate([p[:, 1] for _, p, _ in frames])
    return ((len(np.arange(x.min(), x.max() + res, res)) - 1) *
            (len(np.arange(y.min(), y.max() + res, res)) - 1))


@pytest.fixture(scope="module")
def grid_scene():
    echo = _scene(12, 48, 6)
    geo = _geo(48, step=40.0)  # a wide sector: the grid's extent is ~ 230 m x 200 m
    frames = _frames(echo, geo)
    # the resolutions on either side of 65,536 cells, from a scan of descending resolutions
    at_most, above = None, None
    for res in np.arange(1.2, 0.5, -0.001):
        c = _cells(frames, float(res))
        if c <= 65536:
            at_most = (float(res), c)
        else:
            above = (float(res), c)
            break
    assert at_most and above
    return echo, geo, at_most, above


@pytest.mark.parametrize("side", ["default", "at_most_65536", "above_65536"])
def test_land_grid_cell_counts(gpu, monkeypatch, grid_scene, side):
    """5 m cells (the LDS grid kernel), the finest grid of at most 65,536 cells (cell ids fit 16
    bits) and the next finer one (they do not)."""
    echo, geo, at_most, above = grid_scene
    res, want = {"default": (5.0, None), "at_most_65536": at_most, "above_65536": above}[side]
    assert want is None or (want <= 65536) == (side == "at_most_65536")
    if side == "at_most_65536":
        assert want > 65536 - 600, want  # within one row of cells of the limit
    *_, cells = _run_and_check(gpu, echo, geo, monkeypatch, resolution=res)
    assert want is None or cells == want
    assert side != "default" or cells < 10240


# ---------------------------------------------------------------- 7. intensity sums at 2^24
def test_mean_intensity_at_the_2p24_boundary(gpu, monkeypatch):
    """Every sample 255, stride 1, a 4 m scale (bins 4 mm apart, the 32 rows within 1.4 degrees)
    and eps 0.5 m: one frame is one cluster.  Frame 0
    holds 65,794 points (integer sum 16,777,470 >= 2^24: numpy's pairwise float32 sum), frame 5
    65,793 (16,777,215 < 2^24: exact in any order).  Each segment's mean intensity must equal
    np.mean of the handed-back float32 intensities of that run bit for bit."""
    from rpt.pipeline import PathParams

    R, F = 32, 6
    want = {0: 65794, 5: 65793}
    assert 255 * want[0] >= 2 ** 24 > 255 * want[5]
    echo = np.zeros((F, len(GAINS), R, BINS), np.uint8)
    for f, k in want.items():
        flat = echo[f].reshape(-1)
        flat[:k] = 255
    geo = _geo(R, step=1.0)
    p = PathParams(stride=1, eps_space=0.5, eps_time=2.0, min_samples=15)
    res, frames, _, _ = _run_and_check(gpu, echo, geo, monkeypatch, params=p, scale=4.0,
                                       full=False)
    assert [(fid, len(q)) for fid, q, _ in frames] == sorted(want.items())
    labels = res.labels.cpu().numpy()
    v = res.points["v"].cpu().numpy()
    fr = res.points["frame"].cpu().numpy()
    seg = res.seg
    assert res.n_segments == 2 and sorted(seg["frame"].tolist()) == [0, 5]
    for s in range(2):
        f = int(seg["frame"][s])
        m = (fr == f) & (labels == int(seg["label"][s]))
        assert int(m.sum()) == want[f] == int(seg["count"][s])  # the whole frame is one cluster
        exp = np.float32(np.mean(v[m]))
        print(f"frame {f}: mean intensity {seg['mi'][s]!r}, np.mean {exp!r}")
        assert np.float32(seg["mi"][s]).tobytes() == exp.tobytes()


# ---------------------------------------------------------------- 8. both u8 writers
def test_dense_groups_beside_staged_ones(gpu, monkeypatch):
    """Groups of 4 rows that keep more than 512 samples (written from the echo by the
    group-per-wave writer) beside sparse ones (staged by the count pass, written by the
    thread-per-output writer), in the same sweeps."""
    F, R = 12, 32
    echo = _scene(F, R, 8)
    rng = np.random.default_rng(8)
    for f in (1, 4, 9):
        for g in (0, 2):
            m = rng.random((4, BINS)) < 0.4
            blk = echo[f, g, 12:16]
            blk[m & (blk == 0)] = 12
    kept = (echo > 10).reshape(F, len(GAINS), R // 4, 4 * BINS).sum(-1)
    assert (kept > 512).sum() == 6 and (kept[kept <= 512] <= 400).all() and (kept > 0).all()
    _run_and_check(gpu, echo, _geo(R), monkeypatch)
