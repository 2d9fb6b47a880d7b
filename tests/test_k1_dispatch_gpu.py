"""The K1 kernel forms that the host driver (csrc/polar.hip count_impl / write_impl) can launch and
no other test selects (profiles/r18/polar_split/dispatch_coverage.md has the whole table):

    k_row_count<T, false> + k_row_write<T, false>   bins no multiple of the vector chunk, or an
                                                    echo that is not 16-B aligned
    k_group_count_u8_files<true, 4> and <true, 1>   a threshold above 127 at the smallest stacks
                                                    that take W = 4 and W = 1
    k_expand_write<false, float>                    by-rank staged write, outputs not 16-B aligned
    k_group_write_u8<HI, true, false, float>        staged entries at a stride of 2^23, beyond
                                                    what the by-rank expand write takes

The generic rows are compared with the CPU restatement that golden g1 pins
(oracle.path.polar_scatter), the staged forms with the two-full-read pair, everything exactly.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from test_k1_file_order_gpu import (GUARD, NF_W1, NF_W4, PATTERN, _check, _geometry, _mod7_stack,
                                    _repeat)
from test_k1_file_order_gpu import _run as _run_aligned

pytestmark = pytest.mark.gpu

PAD = 8  # guard elements before and after every output


def _k1(dev, echo_ptr, dt, nf, rows, bins, sc, c, s, gain, fpf, thr, stride, staged=False, shift=0):
    """One count + write.  Every output starts PAD + shift elements into its buffer (the buffers
    are 16-B aligned and PAD * 4 is a multiple of 16, so shift is the offset from a 16-B
    boundary); the elements before and after the outputs must come back untouched.  Returns x, y,
    intensity, gain, point frame, file offsets as numpy arrays."""
    from rpt import _abi
    from rpt._device import stream_handle

    lib = _abi.load()
    rp = torch.empty(nf * rows + 1, dtype=torch.int64, device=dev)
    fo = torch.empty(nf + 1, dtype=torch.int64, device=dev)
    tot = _abi.C.c_int64(0)
    st = stream_handle(dev)
    mk = None
    if staged:
        words = int(lib.rpt_polar_stage_words(nf, rows))
        mk = torch.full((words + GUARD,), PATTERN, dtype=torch.int32, device=dev)
        _abi.check(lib.rpt_polar_count_staged(echo_ptr, dt, nf, rows, bins, thr, stride,
                                              rp.data_ptr(), fo.data_ptr(), _abi.C.byref(tot),
                                              mk.data_ptr(), st))
    else:
        _abi.check(lib.rpt_polar_count(echo_ptr, dt, nf, rows, bins, thr, stride, rp.data_ptr(),
                                       fo.data_ptr(), _abi.C.byref(tot), st))
    n = tot.value
    lo = PAD + shift
    size = lo + n + PAD
    x = torch.full((size,), float("nan"), dtype=torch.float32, device=dev)
    y, v = x.clone(), x.clone()
    g = torch.full((size,), -1, dtype=torch.int32, device=dev)
    pf = g.clone()
    outs = (x, y, v, g, pf)
    for a in outs:
        assert a.data_ptr() % 16 == 0
    args = (echo_ptr, dt, nf, rows, bins, sc.data_ptr(), c.data_ptr(), s.data_ptr(),
            gain.data_ptr(), thr, stride, rp.data_ptr(), fo.data_ptr(), fpf,
            *(a.data_ptr() + 4 * lo for a in outs))
    if staged:
        _abi.check(lib.rpt_polar_write_staged(*args, mk.data_ptr(), st))
        torch.cuda.synchronize(dev)
        assert bool((mk[-GUARD:] == PATTERN).all())
    else:
        _abi.check(lib.rpt_polar_write(*args, st))
        torch.cuda.synchronize(dev)
    for a in (x, y, v):
        assert bool(a[:lo].isnan().all()) and bool(a[lo + n:].isnan().all())
    for a in (g, pf):
        assert bool((a[:lo] == -1).all()) and bool((a[lo + n:] == -1).all())
    return tuple(a[lo:lo + n].cpu().numpy() for a in outs) + (fo.cpu().numpy(),)


# ---------------------------------------------------------------- generic rows, no vector loads
NF, ROWS = 2, 5
GAINS = (40, 47)
_ROWS_REF = {}


def _rows_case(bins):
    """2 files x 5 rows: the samples (about a third above 10, the values 10 and 11 among them),
    the geometry, and per stride the oracle's outputs.  bins 1000: the samples themselves; 1024:
    the same samples with 24 zero bins behind every row.  Computed once."""
    if bins not in _ROWS_REF:
        import oracle.path as op

        rng = np.random.default_rng(18)
        e = rng.integers(0, 256, (NF, ROWS, 1000)).astype(np.uint8)
        e[rng.random(e.shape) < 0.65] = 0
        e[0, 0, :4] = (10, 11, 10, 11)
        e[1, 4, -2:] = (11, 10)
        echo = np.zeros((NF, ROWS, bins), np.uint8)
        echo[:, :, :1000] = e
        scale = (100.0 + 3.5 * np.arange(NF * ROWS)).astype(np.float32).reshape(NF, ROWS)
        trig = [op.trig_tables(rng.integers(0, 8192, ROWS)) for _ in range(NF)]
        exp = {}
        for stride in (1, 3):
            per = [op.polar_scatter(echo[f], scale[f], trig[f][0], trig[f][1], 10.0, stride)
                   for f in range(NF)]
            counts = [len(p[0]) for p in per]
            assert min(counts) > stride
            exp[stride] = (np.concatenate([p[0] for p in per]), np.concatenate([p[1] for p in per]),
                           np.concatenate([p[2] for p in per]),
                           np.repeat(np.array(GAINS, np.int32), counts),
                           np.repeat(np.arange(NF, dtype=np.int32), counts),
                           np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
        _ROWS_REF[bins] = (echo, scale, trig, exp)
    return _ROWS_REF[bins]


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("form", ["u8", "f32", "u8_1024_off1"])
def test_generic_rows_without_vector_loads(gpu, form, stride):
    """1000 bins is a multiple of neither 1024 (u8) nor 256 (f32); a 1024-bin u8 stack one byte
    off its alignment takes the generic pair too, through the alignment rule."""
    from rpt import _abi

    bins = 1024 if form == "u8_1024_off1" else 1000
    echo, scale, trig, exp = _rows_case(bins)
    if form == "f32":
        ed = torch.from_numpy(echo.astype(np.float32)).to(gpu)
        ptr, dt = ed.data_ptr(), _abi.ECHO_F32
    else:
        off = 1 if form == "u8_1024_off1" else 0
        ed = torch.zeros(echo.size + off, dtype=torch.uint8, device=gpu)
        ed[off:] = torch.from_numpy(echo.reshape(-1)).to(gpu)
        ptr, dt = ed.data_ptr() + off, _abi.ECHO_U8
        assert ptr % 16 == off
    sc = torch.from_numpy(scale.reshape(-1)).to(gpu)
    c = torch.from_numpy(np.concatenate([t[0] for t in trig])).to(gpu)
    s = torch.from_numpy(np.concatenate([t[1] for t in trig])).to(gpu)
    gain = torch.tensor(GAINS, dtype=torch.int32, device=gpu)
    got = _k1(gpu, ptr, dt, NF, ROWS, bins, sc, c, s, gain, 1, 10.0, stride)
    for name, a, b in zip(("x", "y", "intensity", "gain", "point_frame", "file_offsets"), got,
                          exp[stride]):
        assert a.dtype == b.dtype, name
        np.testing.assert_array_equal(a, b, err_msg=name)


# ---------------------------------------------------------------- HI at W = 4 and W = 1
@pytest.mark.parametrize("nf", [NF_W4, NF_W1])
def test_threshold_above_127_at_four_waves_and_one(gpu, nf):
    """_mod7_stack's samples are 20 + 30 j + f: above 128 for j = 4, 5, so a row k keeps
    max(k mod 7 - 4, 0) samples, 15 per file."""
    echo = _repeat(gpu, _mod7_stack(), nf)
    for stride in (1, 4):
        fo, _ = _check(gpu, echo, 128.0, stride)
        np.testing.assert_array_equal(fo, -(-15 // stride) * np.arange(nf + 1))


# ---------------------------------------------------------------- staged wave-per-group write
@pytest.mark.parametrize("thr", [10.0, 128.0])
def test_staged_write_at_a_stride_beyond_the_expand_bound(gpu, thr):
    """The by-rank expand write packs the stride into 23 bits of its group words; from 2^23 on the
    staged entries are read by the wave-per-group write instead (one output per file here)."""
    fo, _ = _check(gpu, _mod7_stack(), thr, 1 << 23)
    np.testing.assert_array_equal(fo, np.arange(4))


# ---------------------------------------------------------------- by-rank expand, unaligned outputs
@pytest.mark.parametrize("stride", [1, 4])
def test_by_rank_expand_write_to_unaligned_outputs(gpu, stride):
    """3 files x 37 rows take the by-rank layout; every output one element past a 16-B boundary
    selects the scalar-store form of k_expand_write."""
    ed = torch.from_numpy(_mod7_stack()).to(gpu)
    nf, rows, bins = ed.shape
    ref, _ = _run_aligned(gpu, ed, 10.0, stride, staged=False)
    from rpt import _abi

    sc, c, s, gain = _geometry(gpu, nf, rows)
    got = _k1(gpu, ed.data_ptr(), _abi.ECHO_U8, nf, rows, bins, sc, c, s, gain, 3, 10.0, stride,
              staged=True, shift=1)
    assert len(got[0]) == nf * -(-106 // stride)
    for name, a, b in zip(("x", "y", "intensity", "gain", "point_frame", "file_offsets"), got, ref):
        b = b.cpu().numpy()
        assert a.dtype == b.dtype, name
        # (bit patterns: an unwritten slot is NaN / -1 and must show)
        assert np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                              b.view(np.int32) if b.dtype == np.float32 else b), (name, stride)
