"""K9 and land kernel forms at the smallest shapes where they can go wrong.

The frame-offset / u8 forms of K9 (`FramesOff`, `unsigned char`) exist only in the stack driver's
narrow path, so the scenes below are hand-built u8 stacks (1024 bins, 32 rows, 3 gains, stride 1)
driven through FrameStackPipeline as tests/test_stack_narrow_gpu.py does.  The echo decides the
labels: a cluster is a radial band of bins over all rows (rows 0.04 degrees apart lie within eps
of each other, bands 8 bins = 1.8 m apart do not), or one row's 16 bins where rows are 0.7 degrees
apart.  A band is filled cell by cell in (gain, row, bin) order, which fixes the run length of
its label in the frame; in the frame's point order a label's run comes in pieces, one per row and
gain, with the other bands' pieces between them.

Every stack case asserts its structure on the CPU first (frame sizes, run lengths, label counts,
from the oracle's labels), then checks the run against the oracle's run_path (labels, per-frame
cluster rows in reference order, tracks) and, segment by segment and bit for bit, against the
per-point-frame / float32 form of K9 (rpt_cluster_summaries) over the same kept points and
labels.  Point-by-point interleaving across a chunk boundary cannot come out of ST-DBSCAN on a
plane, so that case uses the public call with made-up labels."""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile
from collections import Counter

import numpy as np
import pytest
import torch

from _stack_check import check_stack_vs_oracle
from oracle import path as op
from test_path_gpu import _radix_summaries_in_child, _summaries_device
from test_stack_narrow_gpu import BINS, GAINS, SCALE, _frames, _geo

pytestmark = pytest.mark.gpu

R = 32
FS_MAX_KEYS = 512        # csrc/summaries_fsort.inc kFsMaxKeys
PARAMS = dict(stride=1, eps_space=1.0, eps_time=2.0, min_samples=15)


def _fill_band(echo, f, b0, w, total, rng):
    """The first `total` cells of the band of bins [b0, b0 + w) of frame f, in (gain, row, bin)
    order, get integer samples 60..99."""
    left = total
    for g in range(echo.shape[1]):
        k = min(left, R * w)
        blk = np.zeros(R * w, np.uint8)
        blk[:k] = rng.integers(60, 100, k)
        echo[f, g, :, b0:b0 + w] = blk.reshape(R, w)
        left -= k
    assert left == 0, "the band does not hold that many samples"


def _oracle(echo, geo, track=True):
    """run_path's outputs; track=False leaves the tracker out (the oracle's takes seconds over
    hundreds of objects, and no case here is about it)."""
    import oracle

    frames = _frames(echo, geo, SCALE, 10.0, PARAMS["stride"])
    assert len(frames) <= 10  # below the land gate: K9 reads K1's points
    if track:
        return frames, op.run_path(frames, land=False, eps_space=PARAMS["eps_space"],
                                   eps_time=PARAMS["eps_time"],
                                   min_samples=PARAMS["min_samples"])
    xy, t = op.stack_coords(frames)
    labels = oracle.stdbscan(xy, t, PARAMS["eps_space"], PARAMS["eps_time"],
                             PARAMS["min_samples"])
    return frames, (frames, labels, op.frame_clusters(frames, labels), None)


def _run_stack(gpu, echo, geo):
    from rpt.pipeline import FrameStackPipeline, PathParams

    F, G, rows, bins = echo.shape
    pipe = FrameStackPipeline(GAINS, rows, bins, PathParams(**PARAMS), gpu)
    pipe.set_geometry(np.full(rows, SCALE, np.float32), geo.cos_t, geo.sin_t, F * G)
    dev_echo = torch.from_numpy(echo).to(gpu)
    assert dev_echo.data_ptr() % 16 == 0  # the grouped K1 path, hence the narrow layout
    res = pipe.run(dev_echo, keep_points=True)
    torch.cuda.synchronize()
    return res


def _sorted_seg(seg):
    key = np.lexsort((seg["label"], seg["frame"]))  # K9's radix form is label-major
    return {k: np.asarray(v)[key] for k, v in seg.items()}


def _check_stack(gpu, echo, geo, frames, oracle_out):
    """One stack run against run_path and against the public K9 form on the same kept points."""
    F = echo.shape[0]
    res = _run_stack(gpu, echo, geo)
    o_frames, o_labels, o_clusters, o_trk = oracle_out
    if o_trk is not None:
        check_stack_vs_oracle(res, F, frames, *oracle_out)
    else:  # its label and row checks, without the tracks
        np.testing.assert_array_equal(res.labels.cpu().numpy(), o_labels)
        fo, order, seg = res.frame_order_offsets, res.frame_order, res.seg
        got = [(f, int(seg["label"][s]), int(seg["count"][s]), seg["cx"][s], seg["cy"][s],
                float(seg["mi"][s])) for f in range(F) for s in order[fo[f]:fo[f + 1]]]
        exp = [(fid, c[0], c[1], c[2][0], c[2][1], c[3]) for fid, _, _ in o_frames
               for c in o_clusters.get(fid, [])]
        assert got == exp
    pts = {k: v.cpu().numpy() for k, v in res.points.items()}
    lab = res.labels.cpu().numpy()
    p = np.column_stack([pts["x"], pts["y"], pts["v"]]).astype(np.float32)
    kept = [(f, p[pts["frame"] == f], None) for f in range(F)]
    pub, _, _ = _summaries_device(gpu, kept, lab, int(lab.max()) + 1)
    a, b = _sorted_seg(res.seg), _sorted_seg(pub)
    assert len(a["label"]) == res.n_segments > 0
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    return res


# ------------------------------------------------- 1. frame sizes and run lengths (frame sort)
SIZES = [0, 1, 63, 64, 65, 1025]  # points of frames 0..5; 1025: one point past a 16-wave step
# around kLaneChainMax (128), kSeqChunk (1024) and numpy's 8192-element buffer
RUNS = [128, 129, 1023, 1024, 1025, 2049, 8191, 8192, 8193]


def _runs_scene():
    rng = np.random.default_rng(41)
    F = len(SIZES) + 2
    echo = np.zeros((F, len(GAINS), R, BINS), np.uint8)
    echo[1, 0, 0, 20] = 50                      # one point: noise
    for f, m in ((2, 63), (3, 64), (4, 65)):
        _fill_band(echo, f, 100, 32, m, rng)    # one label, in three consecutive frames
    _fill_band(echo, 5, 150, 96, 1025, rng)
    # the nine run lengths, twice: six bands of 32 bins, three of 96; frame 7 rotates each group
    for f, runs in ((6, RUNS), (7, RUNS[1:6] + RUNS[:1] + RUNS[7:] + RUNS[6:7])):
        b0 = 400
        for k, m in enumerate(runs):
            w = 32 if k < 6 else 96
            _fill_band(echo, f, b0, w, m, rng)
            b0 += w + 8
        assert b0 <= BINS
    return echo, _geo(R, step=1.0)


@pytest.fixture(scope="module")
def runs_scene():
    echo, geo = _runs_scene()
    frames, o = _oracle(echo, geo)
    return echo, geo, frames, o


def _assert_runs_structure(frames, o):
    o_frames, o_labels, o_clusters, _ = o
    sizes = dict.fromkeys(range(len(SIZES) + 2), 0)
    sizes.update({fid: len(p) for fid, p, _ in frames})
    assert [sizes[f] for f in range(len(SIZES))] == SIZES
    assert sizes[6] == sizes[7] == sum(RUNS) and max(sizes.values()) <= 65536  # one block a frame
    assert sorted(c[1] for c in o_clusters[6]) == sorted(RUNS) == \
        sorted(c[1] for c in o_clusters[7])
    assert [c[1] for f in (2, 3, 4, 5) for c in o_clusters[f]] == [63, 64, 65, 1025]
    assert (o_labels == -1).sum() == 1 and 1 not in o_clusters


def test_frame_sizes_and_run_lengths_narrow_frame_sort(gpu, runs_scene):
    """k_frame_sort / k_runs_lane / k_summarize <FramesOff, unsigned char>."""
    echo, geo, frames, o = runs_scene
    _assert_runs_structure(frames, o)
    res = _check_stack(gpu, echo, geo, frames, o)
    assert np.all(np.diff(res.seg["frame"]) >= 0)  # frame-major: the frame sort's order
    assert res.first_noise[1] == 0 and (np.delete(res.first_noise, 1) == -1).all()


CHILD = r'''
import sys
sys.path[:0] = {path!r}
import numpy as np, torch
from rpt import _abi
assert _abi.load()._name.endswith('librpt_ab.so')
from test_k9_dispatch_gpu import _geo, _run_stack
g = np.load({inp!r})
res = _run_stack(torch.device('cuda', 0), g['echo'], _geo(g['echo'].shape[2], step=float(g['step'])))
np.savez({out!r}, labels=res.labels.cpu().numpy(), first_noise=res.first_noise,
         **{{'s_' + k: np.asarray(v) for k, v in res.seg.items()}})
'''


def test_frame_sizes_and_run_lengths_narrow_radix_path(gpu, runs_scene):
    """k_heads<FramesOff>, k_gather_runs<unsigned char> and the <false, FramesOff, unsigned char>
    forms of k_runs_lane / k_summarize: the same stack on librpt_ab.so with RPT_K9_RADIX=1, in a
    fresh child process, against this process's run on the shipped library."""
    from rpt import _build

    echo, geo, frames, o = runs_scene
    assert _build.LIB_AB.exists(), "librpt_ab.so missing: run __graft_entry__.build()"
    ref = _run_stack(gpu, echo, geo)
    with tempfile.TemporaryDirectory() as d:
        inp, out = os.path.join(d, "in.npz"), os.path.join(d, "out.npz")
        np.savez(inp, echo=echo, step=1.0)
        env = dict(os.environ, RPT_K9_RADIX="1", RPT_LIB=str(_build.LIB_AB))
        subprocess.run([sys.executable, "-c", CHILD.format(path=sys.path, inp=inp, out=out)],
                       check=True, env=env, timeout=240,
                       cwd=os.path.dirname(os.path.abspath(__file__)))
        got = np.load(out)
        seg = {k[2:]: got[k] for k in got.files if k.startswith("s_")}
        assert not np.all(np.diff(seg["frame"]) >= 0)  # label-major: the radix path's order
        np.testing.assert_array_equal(got["labels"], ref.labels.cpu().numpy())
        np.testing.assert_array_equal(got["first_noise"], ref.first_noise)
        a, b = _sorted_seg(seg), _sorted_seg(ref.seg)
        for k in b:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ------------------------------------------------- 2. kFsMaxKeys labels in a frame, and one more
def _labels_scene(n_mid):
    """Three frames of 512 one-row targets (16 bins each, the same places in every frame, so a
    target keeps its label); frame 1 holds n_mid of them."""
    echo = np.zeros((3, len(GAINS), R, BINS), np.uint8)
    spots = [(r, b) for r in range(R) for b in range(512, BINS - 16, 24)]
    assert len(spots) >= FS_MAX_KEYS + 1
    for f, m in ((0, FS_MAX_KEYS), (1, n_mid), (2, FS_MAX_KEYS)):
        for r, b in spots[:m]:
            echo[f, :, r, b:b + 16] = 80
    return echo, _geo(R, step=16.0)


@pytest.mark.parametrize("n_mid", [FS_MAX_KEYS, FS_MAX_KEYS + 1])
def test_frame_with_the_most_labels_the_frame_sort_takes_and_one_more(gpu, n_mid):
    """512 labels in a frame stay on the frame sort; 513 overflow its hash, the count comes back
    as -1 and the stack driver redoes K9 on the radix path (k_heads<FramesOff> and the
    <false, FramesOff, unsigned char> forms, in this process)."""
    echo, geo = _labels_scene(n_mid)
    frames, o = _oracle(echo, geo, track=False)
    assert [len(o[2][f]) for f in range(3)] == [FS_MAX_KEYS, n_mid, FS_MAX_KEYS]
    assert Counter(c[1] for f in range(3) for c in o[2][f]) == {48: 2 * FS_MAX_KEYS + n_mid}
    res = _check_stack(gpu, echo, geo, frames, o)
    assert res.n_segments == 2 * FS_MAX_KEYS + n_mid
    frame_major = bool(np.all(np.diff(res.seg["frame"]) >= 0))
    assert frame_major == (n_mid <= FS_MAX_KEYS)


# ------------------------------------------------- 3. two blocks per frame (chunked frame sort)
CHUNK_SIZES = (70000, 61100)


def test_chunked_frame_sort_narrow(gpu):
    """k_fsc_count / k_fsc_merge <FramesOff> and k_fsc_scatter<FramesOff, unsigned char> with two
    chunks a frame: 16 bands, every band's run in pieces on both sides of the chunk boundary."""
    rng = np.random.default_rng(43)
    echo = np.zeros((2, len(GAINS), R, BINS), np.uint8)
    band = np.zeros(BINS, bool)
    for b0 in range(0, BINS, 64):
        band[b0:b0 + 56] = True
    cols = np.flatnonzero(band)
    for f, m in enumerate(CHUNK_SIZES):
        cells = np.zeros(len(GAINS) * R * len(cols), np.uint8)
        cells[:m] = rng.integers(60, 100, m)
        echo[f][:, :, cols] = cells.reshape(len(GAINS), R, len(cols))
    geo = _geo(R, step=1.0)
    frames, o = _oracle(echo, geo)
    assert tuple(len(p) for _, p, _ in frames) == CHUNK_SIZES
    n = sum(CHUNK_SIZES)
    assert n // 2 == 65550 and (n // 2 + 65535) // 65536 == 2  # summaries_impl's C
    off = 0
    for m in CHUNK_SIZES:  # labels on either side of each frame's chunk boundary
        lab = o[1][off:off + m]
        assert len(o[2][0]) == 16 and len(set(lab)) == 16 and (lab >= 0).all()
        for l in set(lab):
            assert (lab[:m // 2] == l).any() and (lab[m // 2:] == l).any()
        assert len(set(lab[m // 2 - 60:m // 2 + 60])) >= 2
        off += m
    res = _check_stack(gpu, echo, geo, frames, o)
    assert np.all(np.diff(res.seg["frame"]) >= 0)


def test_chunked_frame_sort_run_interleaved_across_the_chunk_boundary(gpu):
    """The public form at the same sizes (C = 2): label 3 on every other point for 4,000 points
    around each frame's chunk boundary, non-integer intensities in frame 1 (numpy's pairwise
    sum); against numpy and against the radix path in a child process."""
    rng = np.random.default_rng(44)
    frames, labs = [], []
    for k, m in enumerate(CHUNK_SIZES):
        p = np.column_stack([rng.normal(0, 50, m), rng.normal(0, 50, m),
                             rng.integers(0, 255, m)]).astype(np.float32)
        if k == 1:
            p[:, 2] = rng.random(m).astype(np.float32) * 255
        lab = rng.integers(-1, 9, m).astype(np.int32)
        lab[m // 2 - 2000:m // 2 + 2000:2] = 3
        lab[m // 2 - 1999:m // 2 + 2000:2] = 5 + k
        frames.append((k, p, None))
        labs.append(lab)
    lab = np.concatenate(labs)
    ncl = int(lab.max()) + 1
    a = _summaries_device(gpu, frames, lab, ncl)
    b = _radix_summaries_in_child(frames, lab, ncl)
    assert np.all(np.diff(a[0]["frame"]) >= 0) and not np.all(np.diff(b[0]["frame"]) >= 0)
    sa, sb = _sorted_seg(a[0]), _sorted_seg(b[0])
    for key in sa:
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=key)
    pf = np.repeat(np.arange(2, dtype=np.int32), CHUNK_SIZES)
    pts = np.vstack([p for _, p, _ in frames])
    assert len(sa["label"]) == len({(f, l) for f, l in zip(pf, lab) if l >= 0})
    for s in range(len(sa["label"])):
        m = (pf == sa["frame"][s]) & (lab == sa["label"][s])
        assert sa["count"][s] == m.sum() and sa["first"][s] == np.flatnonzero(m)[0]
        c = np.mean(pts[m][:, :2], axis=0)
        assert sa["cx"][s] == c[0] and sa["cy"][s] == c[1]
        assert float(sa["mi"][s]) == float(np.mean(pts[m][:, 2]))


# ------------------------------------------------- 4. the land grid without LDS counts
@pytest.mark.parametrize("res", [5.0, 0.25])
def test_land_grid_global_memory_forms(gpu, res):
    """rpt_land_grid on more than 10,240 cells (k_land_grid<int, float>: global atomics), with
    the edges staged in LDS (5 m cells: 242 edges) and searched in global memory (0.25 m: 4,802
    edges, more than the 4,096 the stage holds), against numpy's digitize / add.at."""
    from rpt import _abi
    from rpt._device import stream_handle

    lib, st = _abi.load(), stream_handle(gpu)
    rng = np.random.default_rng(45)
    n = 20011
    p = np.column_stack([rng.uniform(-300, 300, n), rng.uniform(-300, 300, n),
                         rng.integers(11, 256, n)]).astype(np.float32)
    p[0, :2], p[1, :2] = (-300, -300), (300, 300)
    xe = np.arange(p[:, 0].min(), p[:, 0].max() + res, res)
    ye = np.arange(p[:, 1].min(), p[:, 1].max() + res, res)
    cells = (len(xe) - 1) * (len(ye) - 1)
    assert cells > 10240 and (len(xe) + len(ye) > 4096) == (res < 1)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    x, y, v, xed, yed = T(p[:, 0]), T(p[:, 1]), T(p[:, 2]), T(xe), T(ye)
    cnt = torch.empty(cells, dtype=torch.int32, device=gpu)
    tot = torch.empty(cells, dtype=torch.float64, device=gpu)
    _abi.check(lib.rpt_land_grid(x.data_ptr(), y.data_ptr(), v.data_ptr(), n, xed.data_ptr(),
                                 len(xe), yed.data_ptr(), len(ye), cnt.data_ptr(), tot.data_ptr(),
                                 st))
    ix = np.clip(np.digitize(p[:, 0], xe) - 1, 0, len(xe) - 2)
    iy = np.clip(np.digitize(p[:, 1], ye) - 1, 0, len(ye) - 2)
    e_cnt = np.zeros((len(xe) - 1, len(ye) - 1), np.int32)
    e_tot = np.zeros(e_cnt.shape, np.float64)
    np.add.at(e_cnt, (ix, iy), 1)
    np.add.at(e_tot, (ix, iy), p[:, 2])
    np.testing.assert_array_equal(cnt.cpu().numpy().reshape(e_cnt.shape), e_cnt)
    np.testing.assert_array_equal(tot.cpu().numpy().reshape(e_cnt.shape), e_tot)
