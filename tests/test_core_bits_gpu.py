"""The core-cell bitmaps of ST-DBSCAN's per-cell path (all-mutual 2-D grids, integral times):
core_bits (one bit per cell with a core point, k_parent_init_cells), near_bits (its dilation over
the label window: +-2 cells in x and y, +-g.rt slabs, k_near_bits), the non-core points that
k_label_core_cells labels -1 without queueing them (near bit clear), and k_label's candidates
taken from core_bits.  Every case compares rpt.processors.st_dbscan with the C oracle for exact
equality, and first asserts on the CPU the structure it is there for.

The CPU model of the bitmaps: `_window` is the true window of a cell (clipped at the grid),
`_flat` the device's dilation of the bit string (a shift by 1, nx or nx * ny bits per step, which
runs over row and slab ends): a superset of the true window."""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import oracle
from test_cell_components_gpu import _core

pytestmark = pytest.mark.gpu

EPS, MS = 8.0, 15
SIDE = 0.7 * EPS * (1.0 + 2.0 ** -20)
IN = 0.02  # inset of edge points from their cell's border


def _st(xy, t, eps, et, ms):
    from rpt.processors import st_dbscan

    return st_dbscan(xy, t, eps, et, ms)


# ---------------------------------------------------------------- the CPU model
class Grid:
    """The device grid of a cloud with integral times: cell of every point, core cells."""

    def __init__(self, xy, t, et, ms=MS):
        x64 = xy.astype(np.float64)
        self.cx = np.floor((x64[:, 0] - x64[:, 0].min()) / SIDE).astype(np.int64)
        self.cy = np.floor((x64[:, 1] - x64[:, 1].min()) / SIDE).astype(np.int64)
        self.cs = (t.astype(np.float64) - float(t.min())).astype(np.int64)
        self.nx, self.ny, self.nt = int(self.cx.max()) + 1, int(self.cy.max()) + 1, int(
            self.cs.max()) + 1
        assert self.nx * self.ny * self.nt <= max(1 << 22, 4 * len(xy))  # side not coarsened
        self.rt = min(int(np.floor(et)), self.nt)
        self.core = _core(xy, t, EPS, et, ms)
        self.cells = np.zeros((self.nt, self.ny, self.nx), bool)
        self.cells[self.cs[self.core], self.cy[self.core], self.cx[self.core]] = True
        self.key = (self.cs * self.ny + self.cy) * self.nx + self.cx

    def window(self):
        """Per point: does its true window (clipped at the grid) hold a core cell?"""
        c, d = self.cells, np.zeros_like(self.cells)
        for ds in range(-self.rt, self.rt + 1):
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    src = c[max(ds, 0):self.nt + min(ds, 0), max(dy, 0):self.ny + min(dy, 0),
                            max(dx, 0):self.nx + min(dx, 0)]
                    d[max(-ds, 0):self.nt + min(-ds, 0), max(-dy, 0):self.ny + min(-dy, 0),
                      max(-dx, 0):self.nx + min(-dx, 0)] |= src
        return d[self.cs, self.cy, self.cx]

    def flat(self):
        """Per point: its bit of the dilated bit string (guarded at the array's two ends only)."""
        b = self.cells.reshape(-1)
        d = np.zeros_like(b)
        for ds in range(-self.rt, self.rt + 1):
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    o = (ds * self.ny + dy) * self.nx + dx  # near[q] |= core[q + o]
                    if o >= 0:
                        d[:len(b) - o] |= b[o:]
                    else:
                        d[-o:] |= b[:len(b) + o]
        return d[self.key]

    def straddles(self, i):
        """Does a 5-bit row field of point i's window cross a 32-bit word?"""
        for s in range(max(self.cs[i] - self.rt, 0), min(self.cs[i] + self.rt, self.nt - 1) + 1):
            for y in range(max(self.cy[i] - 2, 0), min(self.cy[i] + 2, self.ny - 1) + 1):
                lo = (s * self.ny + y) * self.nx + max(self.cx[i] - 2, 0)
                hi = (s * self.ny + y) * self.nx + min(self.cx[i] + 2, self.nx - 1)
                if lo // 32 != hi // 32:
                    return True
        return False

    def clipped(self, i):
        return bool(self.cx[i] < 2 or self.cx[i] > self.nx - 3 or self.cy[i] < 2 or
                    self.cy[i] > self.ny - 3 or self.cs[i] < self.rt or
                    self.cs[i] > self.nt - 1 - self.rt)


def _run(xy, t, et, ms=MS, integral=True):
    """Oracle labels, device labels equal; the classes of the non-core points on the CPU."""
    assert len(xy) <= 20000 and xy.dtype == np.float32 and t.dtype == np.float32
    exp = oracle.stdbscan(xy, t, EPS, et, ms)
    assert len(exp) == len(xy)  # no point skipped
    if not integral:
        np.testing.assert_array_equal(_st(xy, t, EPS, et, ms), exp)
        return exp, None, None
    g = Grid(xy, t, et, ms)
    win, flat = g.window(), g.flat()
    nc = ~g.core
    assert (flat | ~win).all()  # the device's dilation is a superset of the window
    assert not (nc & (exp >= 0) & ~win).any()  # a labelled non-core point has a core cell in reach
    cls = {"border": nc & (exp >= 0), "near": nc & (exp < 0) & win, "far": nc & ~win,
           "wrapped": nc & ~win & flat}
    np.testing.assert_array_equal(_st(xy, t, EPS, et, ms), exp)
    return exp, g, cls


def _cell_pt(cx, cy, fx=0.5, fy=0.5):
    """The point at fraction (fx, fy) of cell (cx, cy); the grid origin is (0, 0)."""
    return [(cx + fx) * SIDE, (cy + fy) * SIDE]


def _clump(cx, cy, rng):
    """20 points of one cell, pairwise adjacent (the diagonal is below eps): its corners and edge
    midpoints IN from the border and 12 points within 0.3 of the centre.  A point two cells away
    is within eps of at most the three on the facing edge."""
    a, b = IN / SIDE, 1.0 - IN / SIDE
    p = [_cell_pt(cx, cy, fx, fy) for fx in (a, 0.5, b) for fy in (a, 0.5, b) if (fx, fy) != (0.5, 0.5)]
    c = np.array(_cell_pt(cx, cy)) + (rng.random((12, 2)) - 0.5) * 0.6 / np.sqrt(2.0)
    return np.vstack([np.array(p), c])


def _anchors(nx, ny, t0, t1):
    """Two lone points that fix the grid: the origin at time t0, the last cell at time t1."""
    return np.array([[0.0, 0.0], _cell_pt(nx - 1, ny - 1)]), np.array([t0, t1])


# ---------------------------------------------------------------- 1. reach in space
NX, NY = 37, 11


def _space_cloud(cx, cy):
    rng = np.random.default_rng(100 * cx + cy)
    a, b = IN / SIDE, 1.0 - IN / SIDE
    pts = [_clump(cx, cy, rng)]
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            if (sx, sy) == (0, 0):
                continue
            # the facing corner / edge of the cell two away (within eps), its far side (beyond
            # eps) and the cell three away
            fx_near = {-1: b, 0: 0.5, 1: a}[sx]
            fy_near = {-1: b, 0: 0.5, 1: a}[sy]
            for k, (fx, fy) in ((2, (fx_near, fy_near)), (2, (1.0 - fx_near, 1.0 - fy_near)),
                                (3, (0.5, 0.5))):
                px, py = cx + k * sx, cy + k * sy
                if 0 <= px < NX and 0 <= py < NY:
                    pts.append(np.array([_cell_pt(px, py, fx, fy)]))
    axy, at = _anchors(NX, NY, 0.0, 2.0)
    xy = np.vstack(pts)
    t = np.full(len(xy), 1.0)
    return (np.vstack([xy, axy]).astype(np.float32), np.concatenate([t, at]).astype(np.float32))


@pytest.mark.parametrize("cx,cy", [(0, 5), (36, 5), (18, 0), (18, 10), (18, 5)],
                         ids=["left", "right", "bottom", "top", "middle"])
def test_reach_in_space(gpu, cx, cy):
    xy, t = _space_cloud(cx, cy)
    exp, g, cls = _run(xy, t, 2.0)
    assert (g.nx, g.ny, g.nt) == (NX, NY, 3) and g.nx % 32 != 0
    assert g.core.sum() == 20 and g.cells.sum() == 1
    assert cls["border"].any() and cls["near"].any() and cls["far"].any()
    probes = np.flatnonzero(~g.core)
    # the probes two cells away: in x alone, in y alone and diagonally, both labelled and not
    dx, dy = np.abs(g.cx[probes] - cx), np.abs(g.cy[probes] - cy)
    for sel in ((dx == 2) & (dy == 0), (dx == 0) & (dy == 2), (dx == 2) & (dy == 2)):
        two = probes[sel & (g.cs[probes] == 1)]
        assert (exp[two] >= 0).any() and (exp[two] < 0).any()
    three = probes[(np.maximum(dx, dy) == 3) & (g.cs[probes] == 1)]
    assert len(three) and cls["far"][three].all()
    assert any(g.straddles(i) for i in probes)
    if (cx, cy) != (18, 5):
        assert any(g.clipped(i) for i in probes[cls["border"][probes] | cls["near"][probes]])


# ---------------------------------------------------------------- 2. reach in time
TNX, TNY, TNT = 9, 7, 9


def _time_cloud(s):
    """The clump in slab s; per slab s +- 1, 2, 3 one probe in the clump's cell and one two
    cells away in x within eps of the clump's facing edge."""
    cx, cy = {0: (0, 0), TNT - 1: (TNX - 1, TNY - 1)}.get(s, (4, 3))
    sx = 1 if cx + 2 < TNX else -1
    rng = np.random.default_rng(s)
    a, b = IN / SIDE, 1.0 - IN / SIDE
    pts, ts = [_clump(cx, cy, rng)], [np.full(20, float(s))]
    for k in (-3, -2, -1, 1, 2, 3):
        if 0 <= s + k < TNT:
            pts.append(np.array([_cell_pt(cx, cy), _cell_pt(cx + 2 * sx, cy, a if sx > 0 else b)]))
            ts.append(np.full(2, float(s + k)))
    axy, at = _anchors(TNX, TNY, 0.0, float(TNT - 1))
    if s == 0:  # (the clump's own corner point is the origin)
        axy, at = axy[1:], at[1:]
    return (np.vstack(pts + [axy]).astype(np.float32),
            np.concatenate(ts + [at]).astype(np.float32), (cx, cy, sx))


@pytest.mark.parametrize("et", [2.0, 1.0, 0.0])
@pytest.mark.parametrize("s", [0, TNT - 1, 4], ids=["first", "last", "interior"])
def test_reach_in_time(gpu, s, et):
    xy, t, (cx, cy, sx) = _time_cloud(s)
    exp, g, cls = _run(xy, t, et)
    assert (g.nx, g.ny, g.nt) == (TNX, TNY, TNT) and g.rt == int(et)
    # the ends of the bit string: the first cell of the first slab, the last of the last
    if s == 0:
        assert g.cells[0, 0, 0]
    if s == TNT - 1:
        assert g.cells[-1, -1, -1]
    side = np.flatnonzero((g.cx == cx + 2 * sx) & (g.cy == cy))
    assert len(side) >= 3 and not g.core[side].any()
    dt = np.abs(g.cs[side] - s)
    # within eps_t of the clump: labelled; further: noise, and beyond every core cell's reach
    # not queued (the probes in the clump's cell are core where they reach the clump, so their
    # slabs hold core cells too)
    if et > 0:
        assert (exp[side[dt <= et]] >= 0).all() and (dt <= et).any()
    assert (exp[side[dt > et]] < 0).all() and (dt > et).any()
    if et < 2:
        assert cls["far"][side].any()
    else:  # the core probes of slabs s +- 2 reach slabs s +- 3: queued there, and found noise
        assert cls["near"][side[dt == 3]].all() and cls["far"].any()
    own =np.flatnonzero((g.cx == cx) & (g.cy == cy) & (g.cs != s))
    assert (g.core[own] == (np.abs(g.cs[own] - s) <= et)).all()


# ---------------------------------------------------------------- 3. wrap
def test_wrap_over_row_and_slab_ends(gpu):
    """A core cell in the last column of row 3 and a lone point in the first column of row 4;
    a core cell in the last cell of slab 0 and a lone point in the first cell of slab 1: next
    to each other in the bit string, far apart in the grid."""
    nx, ny = 13, 8
    rng = np.random.default_rng(3)
    pts = [_clump(nx - 1, 3, rng), np.array([_cell_pt(0, 4)]), _clump(nx - 1, ny - 1, rng),
           np.array([[0.0, 0.0]]), np.array([_cell_pt(0, 0)])]
    ts = [np.zeros(20), np.zeros(1), np.zeros(20), np.zeros(1), np.ones(1)]
    xy, t = np.vstack(pts).astype(np.float32), np.concatenate(ts).astype(np.float32)
    exp, g, cls = _run(xy, t, 0.0)
    assert (g.nx, g.ny, g.nt, g.rt) == (nx, ny, 2, 0)
    lone_row, lone_slab = 20, len(xy) - 1
    assert g.key[lone_row] == g.key[0] + 1 and g.key[lone_slab] == g.key[21] + 1
    assert cls["wrapped"][lone_row] and cls["wrapped"][lone_slab]
    assert exp[lone_row] == -1 and exp[lone_slab] == -1


# ---------------------------------------------------------------- 4. queue sizes
B, NB = 8, 34  # cells per block side, blocks per grid side


def _queue_cloud(clumps, near, far=12000, seed=11):
    """Blocks of 8 x 8 cells, three frames.  A clump block holds a clump in cell (4, 4) of frame
    1 and, with `near`, 20 lone points in the cells two away from it; a far block holds at most
    4 points per frame in its cells (3..5, 3..5), five cells or more from every other block's."""
    rng = np.random.default_rng(seed)
    blocks = rng.permutation(NB * NB)
    pts, ts = [], []
    a, b = IN / SIDE, 1.0 - IN / SIDE
    ring = [(sx, sy) for sx in (-2, 0, 2) for sy in (-2, 0, 2) if (sx, sy) != (0, 0)]
    for blk in blocks[:clumps]:
        bx, by = (blk % NB) * B + 4, (blk // NB) * B + 4
        pts.append(_clump(bx, by, rng))
        ts.append(np.ones(20))
        if near:
            for k in range(20):
                sx, sy = ring[k % 8]
                fn = ({-2: b, 0: 0.5, 2: a}[sx], {-2: b, 0: 0.5, 2: a}[sy])
                f = fn if k < 8 else tuple(rng.random(2) * 0.2 + np.where(np.array([sx, sy]) > 0,
                                                                           0.75, 0.05))
                if k >= 8 and sx == 0:
                    f = (0.5, f[1])
                if k >= 8 and sy == 0:
                    f = (f[0], 0.5)
                pts.append(np.array([_cell_pt(bx + sx, by + sy, *f)]))
                ts.append(np.array([float(k % 3)]))
    fb = blocks[clumps:]
    per = -(-far // (3 * len(fb)))
    assert per <= 4
    left = far
    for f in range(3):
        for blk in fb:
            k = min(per, left)
            if k == 0:
                break
            left -= k
            org = np.array([(blk % NB) * B + 3, (blk // NB) * B + 3]) * SIDE
            pts.append(org + rng.random((k, 2)) * 3 * SIDE)
            ts.append(np.full(k, float(f)))
    axy, at = _anchors(NB * B, NB * B, 0.0, 2.0)
    return (np.vstack(pts + [axy]).astype(np.float32),
            np.concatenate(ts + [at]).astype(np.float32))


@pytest.fixture(scope="module")
def mixed_queue():
    return _queue_cloud(clumps=100, near=True)


def test_queue_of_near_points_among_far_noise(gpu, mixed_queue):
    xy, t = mixed_queue
    exp, g, cls = _run(xy, t, 2.0)
    assert g.core.sum() == 2000
    queued = cls["border"] | cls["near"]
    assert 1900 <= queued.sum() <= 2100 and cls["border"].sum() >= 500 and cls["near"].sum() >= 500
    assert 11900 <= cls["far"].sum() <= 12100
    # the queued points spread over several 2,048-point tiles of the sorted points
    order = np.argsort(g.key, kind="stable")
    tiles = np.unique(np.flatnonzero(queued[order]) // 2048)
    assert len(tiles) >= 4 and len(xy) > 3 * 2048


def test_empty_queue(gpu):
    xy, t = _queue_cloud(clumps=100, near=False)
    exp, g, cls = _run(xy, t, 2.0)
    assert g.core.sum() == 2000 and (~g.core).sum() >= 12000
    assert not (cls["border"] | cls["near"] | cls["wrapped"]).any()  # nothing queued
    assert (exp[~g.core] == -1).all()


def test_no_core_point_at_all(gpu):
    xy, t = _queue_cloud(clumps=0, near=False)
    exp, g, cls = _run(xy, t, 2.0)
    assert not g.core.any() and not g.cells.any() and (exp == -1).all()


# ---------------------------------------------------------------- 5. other layouts
def test_fractional_eps_t_keeps_float4_points(gpu):
    xy, t, _ = _time_cloud(4)
    exp, g, cls = _run(xy, t, 1.5)
    assert g.rt == 1 and cls["border"].any() and cls["far"].any()


def test_nonintegral_times_build_no_near_bits(gpu, mixed_queue):
    xy, t = mixed_queue
    t = t.copy()
    t[len(t) // 2] += 0.5
    assert (t != np.floor(t)).sum() == 1
    exp, _, _ = _run(xy, t, 2.0, integral=False)
    assert (exp >= 0).any() and (exp == -1).any()


# ---------------------------------------------------------------- 6. the path is reached
CHILD = r'''
import sys
import numpy as np
from rpt import _abi
from rpt.processors import st_dbscan
assert _abi.load()._name.endswith("librpt_ab.so")
z = np.load(sys.argv[1])
np.save(sys.argv[2], st_dbscan(z["xy"], z["t"], float(z["p"][0]), float(z["p"][1]), int(z["p"][2])))
'''


def test_far_points_are_not_queued(gpu, mixed_queue):
    """The A/B build's `label:` line on the mixed cloud: fewer points queued than there are
    non-core points, and no fewer than those whose true window holds a core cell."""
    from rpt import _build

    assert _build.LIB_AB.exists(), "librpt_ab.so missing: run __graft_entry__.build()"
    xy, t = mixed_queue
    g = Grid(xy, t, 2.0)
    n_nc, n_win = int((~g.core).sum()), int((~g.core & g.window()).sum())
    assert 0 < n_win < n_nc
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.npz"), os.path.join(d, "out.npy")
        np.savez(src, xy=xy, t=t, p=np.array([EPS, 2.0, MS]))
        code = f"import sys\nsys.path[:0] = {sys.path!r}\n" + CHILD
        env = dict(os.environ, RPT_LIB=str(_build.LIB_AB), RPT_STATS="1")
        r = subprocess.run([sys.executable, "-c", code, src, dst], env=env, timeout=240,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        np.testing.assert_array_equal(np.load(dst), oracle.stdbscan(xy, t, EPS, 2.0, MS))
    assert "all_mutual=1 cell_comp=1" in r.stderr, r.stderr[-2000:]
    m = re.findall(r"label: queued=(\d+)", r.stderr)
    assert len(m) == 1, r.stderr[-2000:]
    assert n_win <= int(m[0]) < n_nc, (n_win, m[0], n_nc)
