"""The staged K1 pair in its file-contiguous layout (csrc/polar_count.inc: k_group_count_u8_files
stores a file's emitted entries as one dense array in output order; csrc/polar_expand.inc:
k_file_staged + k_expand_stream write them as a stream) against the two-full-read pair
rpt_polar_count + rpt_polar_write: all six outputs by bit pattern, with NaN / -1 sentinels in the
output arrays.

File f owns C = ceil(rows / 4) * 512 words of the staging buffer; a group that emits the file's
outputs [first, first + m) is staged iff m != 0 and first + m <= C (k1_emit.h emit_staged_file),
and every later emitting group of the file is then written from the echo.  The layout is taken
from 1500 files on, so every case is a hand-made small stack repeated to 1500, 1946 and 3892
files (W = 4, 2, 1 waves per file in the count pass), as tests/test_k1_file_order_gpu.py does.
"""
from __future__ import annotations

import itertools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from test_k1_file_order_gpu import (EMITTED, GUARD, NF_W2, NF_W4, PATTERN, STAGE_SLOTS, _geometry,
                                    _random_stack, _repeat)

pytestmark = pytest.mark.gpu


def _run(dev, ed, thr, stride, staged, shift=0):
    """One count + write of the u8 stack ed [nf, rows, 1024].  shift: elements by which the x, y
    and intensity pointers are moved off their 16-byte alignment.  Returns the six outputs and,
    staged, the entries with their guard words."""
    from rpt import _abi
    from rpt._device import stream_handle

    lib = _abi.load()
    nf, rows, bins = ed.shape
    assert bins == 1024 and ed.dtype == torch.uint8 and ed.is_contiguous()
    sc, c, s, gain = _geometry(dev, nf, rows)
    rp = torch.empty(nf * rows + 1, dtype=torch.int64, device=dev)
    fo = torch.empty(nf + 1, dtype=torch.int64, device=dev)
    tot = _abi.C.c_int64(0)
    st = stream_handle(dev)
    mk = None
    if staged:
        words = int(lib.rpt_polar_stage_words(nf, rows))
        assert words == nf * ((rows + 3) // 4) * STAGE_SLOTS
        mk = torch.full((words + GUARD,), PATTERN, dtype=torch.int32, device=dev)
        _abi.check(lib.rpt_polar_count_staged(ed.data_ptr(), _abi.ECHO_U8, nf, rows, bins, thr,
                                              stride, rp.data_ptr(), fo.data_ptr(),
                                              _abi.C.byref(tot), mk.data_ptr(), st))
    else:
        _abi.check(lib.rpt_polar_count(ed.data_ptr(), _abi.ECHO_U8, nf, rows, bins, thr, stride,
                                       rp.data_ptr(), fo.data_ptr(), _abi.C.byref(tot), st))
    n = tot.value
    size = max(n, 1) + shift + 8  # sentinels behind the outputs too
    x = torch.full((size,), float("nan"), dtype=torch.float32, device=dev)
    y, v = x.clone(), x.clone()
    g = torch.full((size,), -1, dtype=torch.int32, device=dev)
    pf = g.clone()
    args = (ed.data_ptr(), _abi.ECHO_U8, nf, rows, bins, sc.data_ptr(), c.data_ptr(),
            s.data_ptr(), gain.data_ptr(), thr, stride, rp.data_ptr(), fo.data_ptr(), 3,
            x.data_ptr() + 4 * shift, y.data_ptr() + 4 * shift, v.data_ptr() + 4 * shift,
            g.data_ptr(), pf.data_ptr())
    if staged:
        _abi.check(lib.rpt_polar_write_staged(*args, mk.data_ptr(), st))
    else:
        _abi.check(lib.rpt_polar_write(*args, st))
    torch.cuda.synchronize(dev)
    # nothing before the first or behind the last output
    for a in (x, y, v):
        assert bool(a[:shift].isnan().all()) and bool(a[shift + n:].isnan().all())
    assert bool((g[n:] == -1).all()) and bool((pf[n:] == -1).all())
    return (x[shift:shift + n], y[shift:shift + n], v[shift:shift + n], g[:n], pf[:n], fo), mk


_REF = {}  # the unstaged pair's outputs, computed once per stack


def _check(dev, echo, thr, stride, key=None, shift=0):
    """Staged against unstaged, all six outputs by bit pattern; the guard words behind the
    entries untouched.  Returns (file_offsets as numpy, entries)."""
    ed = echo if isinstance(echo, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(echo)).to(dev)
    k = (key, thr, stride, tuple(ed.shape))
    if key is None or k not in _REF:
        a, _ = _run(dev, ed, thr, stride, staged=False)
        if key is not None:
            _REF.clear()  # (one stack at a time: the outputs are device tensors)
            _REF[k] = a
    else:
        a = _REF[k]
    b, mk = _run(dev, ed, thr, stride, staged=True, shift=shift)
    names = ("x", "y", "intensity", "gain", "point_frame", "file_offsets")
    for name, p, q in zip(names, a, b):
        assert p.shape == q.shape, (name, thr, stride, tuple(ed.shape))
        # (bit patterns: NaN never appears in an output, and an unwritten slot must show)
        same = torch.equal(p.view(torch.int32) if p.dtype == torch.float32 else p,
                           q.view(torch.int32) if q.dtype == torch.float32 else q)
        assert same, (name, thr, stride, tuple(ed.shape), shift)
    assert bool((mk[-GUARD:] == PATTERN).all()), ("guard words", thr, stride, tuple(ed.shape))
    return a[5].cpu().numpy(), mk


def _fill_group(echo, f, g, kept):
    """Group g of file f keeps `kept` samples (its 4 rows filled from the left, values > 10)."""
    flat = echo[f, 4 * g:4 * g + 4].reshape(-1)
    flat[:kept] = (np.arange(kept) % 200 + 20).astype(np.uint8)


def _counts_stack(rows, counts):
    """File 0: group g keeps counts[g] samples; a second, sparse file follows so that a wrong
    count or boundary shifts it."""
    echo = np.zeros((2, rows, 1024), np.uint8)
    for g, n in enumerate(counts):
        _fill_group(echo, 0, g, n)
    echo[1, :, ::37] = 55
    return echo


# ---------------------------------------------------------------- the capacity edge
C12 = 3 * STAGE_SLOTS  # 12 rows: 3 groups, 1536 words per file


@pytest.mark.parametrize("nf", EMITTED)
@pytest.mark.parametrize("counts", [(1000, 536, 0), (1000, 536, 5), (1000, 600, 5), (1537, 0, 0),
                                    (1536, 0, 1)])
def test_capacity_edge_at_stride_1(gpu, counts, nf):
    """Fits exactly; the third group starts at C (unstaged); the second straddles C (it and the
    third unstaged); one group one output too long; one group filling C and one output after."""
    fo, mk = _check(gpu, _repeat(gpu, _counts_stack(12, counts), nf), 10.0, 1)
    assert fo[1] == sum(counts)
    so = {(1000, 536, 0): 1536, (1000, 536, 5): 1536, (1000, 600, 5): 1000, (1537, 0, 0): 0,
          (1536, 0, 1): 1536}[counts]
    region = mk[:C12]  # file 0: exactly its first staged_out words are written
    assert bool((region[:so] != PATTERN).all()) and bool((region[so:] == PATTERN).all())


@pytest.mark.parametrize("nf", EMITTED)
@pytest.mark.parametrize("tail", [0, 5])
@pytest.mark.parametrize("before", [0, 1, 2, 3])
def test_capacity_edge_at_stride_4_depends_on_the_rank(gpu, before, tail, nf):
    """16 rows, C = 2048.  Groups 1 and 2 keep 4 * C - 1 samples between them: after a rank of 0
    or 1 the file's outputs through group 2 number C (staged, the region full), after 2 or 3
    they number C + 1 and group 2 is unstaged; a last group of `tail` samples follows."""
    C = 4 * STAGE_SLOTS
    echo = _counts_stack(16, (before, 4096, 4 * C - 1 - 4096, tail))
    fo, mk = _check(gpu, _repeat(gpu, echo, nf), 10.0, 4)
    assert fo[1] == -(-(before + 4 * C - 1 + tail) // 4)
    so = -(-(before + 4096) // 4) if before >= 2 else C
    region = mk[:C]
    assert bool((region[:so] != PATTERN).all()) and bool((region[so:] == PATTERN).all())


# ---------------------------------------------------------------- file boundaries
def _boundary_stack():
    """5-row files (a full group and a 1-row group) emitting 0, 1, 2, 3, 5 outputs at stride 1 in
    every order, runs of 2 .. 9 empty files between the orders, an empty first and last file."""
    files = [0]
    for i, perm in enumerate(itertools.permutations((0, 1, 2, 3, 5))):
        files += list(perm) + [0] * (i % 9 + 1 if i % 4 == 0 else 0)
    files += [0]
    echo = np.zeros((len(files), 5, 1024), np.uint8)
    for f, n in enumerate(files):
        for j in range(n):  # the last sample of a file in its 1-row group
            echo[f, 4 if j == n - 1 else j % 4, (f * 7 + j * 131) % 1024] = 30 + 40 * j + f % 9
    return echo, files


@pytest.mark.parametrize("nf", EMITTED)
@pytest.mark.parametrize("shift", [0, 1])
def test_file_boundaries_inside_a_threads_outputs(gpu, nf, shift):
    """shift = 1 moves x / y / intensity off their 16-byte alignment: the scalar store path."""
    small, files = _boundary_stack()
    echo = _repeat(gpu, small, nf)
    echo[-1] = 0
    per_file = np.array([files[f % len(files)] for f in range(nf)])
    per_file[-1] = 0
    fo, _ = _check(gpu, echo, 10.0, 1, key="boundary", shift=shift)
    np.testing.assert_array_equal(fo, np.concatenate([[0], np.cumsum(per_file)]))
    assert (fo % 4 != 0).sum() > nf // 4
    assert fo[1] == 0 and fo[-1] == fo[-2]


def test_file_boundaries_at_stride_3(gpu):
    small, _ = _boundary_stack()
    _check(gpu, _repeat(gpu, small, NF_W4), 10.0, 3)


# ---------------------------------------------------------------- determinism and the region
def _staged_out(echo, thr, stride):
    """Per file: the outputs and the staged outputs (emit_staged_out), from the groups' kept
    counts; rows must be a multiple of 4."""
    nf, rows, _ = echo.shape
    gpf = rows // 4
    C = gpf * STAGE_SLOTS
    kept = (echo > thr).view(nf, gpf, -1).sum(dim=2).cpu().numpy().astype(np.int64)
    end = np.cumsum(kept, axis=1)
    first = -(-(end - kept) // stride)
    last = -(-end // stride)
    un = (last > first) & (last > C)
    count = last[:, -1]
    so = np.where(un.any(axis=1), np.where(un, first, np.iinfo(np.int64).max).min(axis=1), count)
    return count, so, C


@pytest.mark.parametrize("stride", [1, 4])
def test_entries_identical_and_inside_their_regions(gpu, stride):
    """Two runs leave identical entries; the written words are exactly the first staged_out[f]
    words of every file's region (dense files overflow C = 1536 at stride 1, 12 rows)."""
    echo = _random_stack(gpu, NF_W2, 12, seed=21)
    _, mk1 = _check(gpu, echo, 10.0, stride)
    _, mk2 = _check(gpu, echo, 10.0, stride)
    assert torch.equal(mk1, mk2)
    count, so, C = _staged_out(echo, 10, stride)
    assert (so <= np.minimum(count, C)).all()
    if stride == 1:
        assert (count > C).any() and (so < count).any()
    written = (mk1[:-GUARD] != PATTERN).view(NF_W2, C)
    expect = torch.arange(C, device=gpu)[None, :] < torch.from_numpy(so).to(gpu)[:, None]
    assert torch.equal(written, expect)
    assert int(written.sum()) == int(so.sum())


# ---------------------------------------------------------------- through the stack driver
STACK_RUN = r'''
import numpy as np, torch
from rpt.pipeline import FrameStackPipeline, PathParams
from rpt.synth import DeviceSynth, SynthConfig

def stack_cfg(density):
    return SynthConfig(n_frames=500, rows=16, n_targets=6, clutter_density=density)

def make_pipe(cfg, ds, dev):
    pipe = FrameStackPipeline(cfg.gains, cfg.rows, cfg.bins, PathParams(), dev)
    pipe.set_geometry(np.full(cfg.rows, cfg.scale, np.float32), ds.geo.cos_t, ds.geo.sin_t,
                      cfg.n_frames * 3)
    return pipe

def run_stack():
    dev = torch.device("cuda", 0)
    cfg = stack_cfg(0.002)
    ds = DeviceSynth(cfg, dev)
    res = make_pipe(cfg, ds, dev).run(ds.echo(), keep_points=True).finish()
    out = {"labels": res.labels.cpu().numpy()}
    for k in ("x", "y", "v", "gain", "frame"):
        out["p_" + k] = res.points[k].cpu().numpy()
    return out
'''


def _ns():
    ns = {}
    exec(STACK_RUN, ns)  # noqa: S102 (the same code the children run)
    return ns


def test_stack_run_matches_oracle_then_regrows(gpu):
    """500 frames x 3 files of 16 rows, land filter on, against the oracle (the land grid's
    edges come from the bounds k_expand_stream leaves); then a stack with more points on the same
    handle: the speculative write is cut off at the first run's capacity (n + n / 8 + 64 = 58606,
    not a multiple of 4, inside a file), the buffers grow and the write repeats."""
    from _stack_check import check_stack_vs_oracle, oracle_stack
    from oracle import path as op
    from rpt.synth import DeviceSynth

    ns = _ns()
    cfg = ns["stack_cfg"](0.0005)
    ds = DeviceSynth(cfg, gpu)
    pipe = ns["make_pipe"](cfg, ds, gpu)
    echo = ds.echo()
    res = pipe.run(echo, keep_points=True)
    torch.cuda.synchronize(gpu)
    frames = oracle_stack(echo.cpu().numpy(), cfg, ds.geo)
    o_frames, o_labels, o_clusters, o_trk = op.run_path(frames)
    check_stack_vs_oracle(res, cfg.n_frames, frames, o_frames, o_labels, o_clusters, o_trk)
    n0 = res.n_points
    assert (n0 + n0 // 8 + 64) % 4 != 0
    cfg2 = ns["stack_cfg"](0.002)
    ds2 = DeviceSynth(cfg2, gpu)
    echo2 = ds2.echo()
    a = pipe.run(echo2, keep_points=True)
    b = ns["make_pipe"](cfg2, ds2, gpu).run(echo2, keep_points=True)
    assert a.n_points > n0 + n0 // 8 + 64
    assert a.n_points == b.n_points
    for k in a.points:
        assert torch.equal(a.points[k], b.points[k]), k
    assert torch.equal(a.labels, b.labels)
    for k in a.seg:
        np.testing.assert_array_equal(a.seg[k], b.seg[k])


@pytest.mark.parametrize("switch", ["RPT_K1_EXPAND", "RPT_K1_STAGE"])
def test_ab_switches_on_an_emitted_size_stack(gpu, switch):
    """RPT_K1_EXPAND=0 (the wave-per-group write reads the file-contiguous entries) and
    RPT_K1_STAGE=0 (two full reads) in a fresh child process on the A/B build: the shipped
    library's points and labels."""
    from rpt import _abi, _build

    assert _build.LIB_AB.exists(), "librpt_ab.so missing: run __graft_entry__.build()"
    assert _abi.load()._name.endswith("librpt.so")
    ref = _ns()["run_stack"]()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "out.npz")
        code = (f"import sys\nsys.path[:0] = {sys.path!r}\n" + STACK_RUN +
                "from rpt import _abi\nassert _abi.load()._name.endswith('librpt_ab.so')\n"
                f"np.savez({out!r}, **run_stack())\n")
        env = dict(os.environ, RPT_LIB=str(_build.LIB_AB), **{switch: "0"})
        subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=240)
        got = np.load(out)
        assert sorted(got.files) == sorted(ref)
        for k in ref:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{k} with {switch}=0")
    torch.cuda.synchronize()
