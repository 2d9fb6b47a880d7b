"""The staged K1 pair (rpt_polar_count_staged + rpt_polar_write_staged) in its emitted layout -- a
file's groups are counted in file order by one workgroup of W waves, and only the samples the
write pass emits are staged -- against the two-full-read pair rpt_polar_count + rpt_polar_write,
which golden vector g1 pins to the reference.  All six outputs must be equal exactly.

The layout and W follow from n_files alone (k1_emit.h staged_emitted, polar_count.inc
count_waves_per_file):

    emitted layout   n_files >= 1500 and 20 * n_files >= 19 * 256 * ceil(n_files / 256)
                     (the busiest of the 256 CUs has at most 1/19 more files than the average)
    W                ceil(n_files / 256) <= 7: 4;  <= 15: 2;  else 1

    n_files   1499   1500   1536   1537   1702   1703   1792   1793   1945   1946   3840   3841   3891   3892
    layout    rank   emit   emit   rank   rank   emit   emit   rank   rank   emit   emit   rank   rank   emit
    W           -      4      4      -      -      4      4      -      -      2      2      -      -      1

so a stack of a few files never reaches the file-ordered pass.  Every case below is therefore a
small stack written out as specified (3 files x 37 rows, 2 files x 12 rows, ...) and REPEATED to
1500 files (W = 4, the smallest stack that takes the emitted layout), to 1946 files (W = 2) and to
3892 files (W = 1): the smallest n_files of each W; the small stack itself runs too (the by-rank
layout).  The largest stack is 3892 files x 37 rows (147 MB of echo, built on the device).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 1024
PATTERN = 0x5A5A5A5A
STAGE_SLOTS = 512  # csrc/k1_emit.h kStageSlots


def _geometry(dev, nf, rows):
    g = torch.Generator(device="cpu").manual_seed(nf * 1009 + rows)
    n = nf * rows
    sc = (100.0 + 0.25 * torch.arange(n, dtype=torch.float32) % 97.0).to(dev)
    c = (torch.rand(n, generator=g) * 2 - 1).to(dev)
    s = (torch.rand(n, generator=g) * 2 - 1).to(dev)
    gain = (40 + 7 * (torch.arange(nf, dtype=torch.int32) % 3)).to(dev)
    return sc, c, s, gain


def _run(dev, ed, thr, stride, staged):
    """One count + write of the u8 stack ed [nf, rows, 1024] on the device.  Returns the six
    outputs (device tensors) and, staged, the entries tensor with its guard words."""
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
    x = torch.full((max(n, 1),), float("nan"), dtype=torch.float32, device=dev)
    y, v = x.clone(), x.clone()
    g = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
    pf = g.clone()
    args = (ed.data_ptr(), _abi.ECHO_U8, nf, rows, bins, sc.data_ptr(), c.data_ptr(),
            s.data_ptr(), gain.data_ptr(), thr, stride, rp.data_ptr(), fo.data_ptr(), 3,
            x.data_ptr(), y.data_ptr(), v.data_ptr(), g.data_ptr(), pf.data_ptr())
    if staged:
        _abi.check(lib.rpt_polar_write_staged(*args, mk.data_ptr(), st))
    else:
        _abi.check(lib.rpt_polar_write(*args, st))
    torch.cuda.synchronize(dev)
    return (x[:n], y[:n], v[:n], g[:n], pf[:n], fo), mk


def _check(dev, echo, thr, stride):
    """Staged against unstaged, all six outputs exactly; the guard words behind the entries
    untouched.  Returns (file_offsets as numpy, entries)."""
    ed = echo if isinstance(echo, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(echo)).to(dev)
    a, _ = _run(dev, ed, thr, stride, staged=False)
    b, mk = _run(dev, ed, thr, stride, staged=True)
    names = ("x", "y", "intensity", "gain", "point_frame", "file_offsets")
    for name, p, q in zip(names, a, b):
        assert p.shape == q.shape, (name, thr, stride, tuple(ed.shape))
        # (bit patterns: NaN never appears in an output, and an unwritten slot must show)
        assert torch.equal(p.view(torch.int32) if p.dtype == torch.float32 else p,
                           q.view(torch.int32) if q.dtype == torch.float32 else q), \
            (name, thr, stride, tuple(ed.shape))
    assert bool((mk[-GUARD:] == PATTERN).all()), ("guard words", thr, stride, tuple(ed.shape))
    return a[5].cpu().numpy(), mk


def _random_stack(dev, nf, rows, seed, densities=(0.0, 0.01, 0.1, 0.7)):
    """File f keeps about densities[f % len] of its samples above 10: empty, sparse (staged),
    mixed, and dense files (about 2870 kept per group: unstaged at strides below 6)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    val = torch.randint(11, 256, (nf, rows, 1024), generator=g, device=dev, dtype=torch.int32)
    u = torch.rand((nf, rows, 1024), generator=g, device=dev)
    p = torch.tensor([densities[f % len(densities)] for f in range(nf)], device=dev)
    return torch.where(u < p[:, None, None], val, torch.zeros_like(val)).to(torch.uint8)


NF_W4 = 1500  # the smallest stack in the emitted layout: W = 4
NF_W2 = 1946  # the smallest stack with W = 2
NF_W1 = 3892  # the smallest stack with W = 1
EMITTED = (NF_W4, NF_W2, NF_W1)


def _repeat(dev, echo, nf):
    """The files of the small stack, over and over, up to nf files (file f = small file f mod k)."""
    ed = echo if isinstance(echo, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(echo)).to(dev)
    k = ed.shape[0]
    return ed.repeat((nf + k - 1) // k, 1, 1)[:nf].contiguous()


# ---------------------------------------------------------------- rank carry
def _mod7_stack():
    """3 files x 37 rows (9 full groups and a 1-row group); row k keeps exactly k mod 7 samples,
    placed by hand at distinct bins that differ from file to file."""
    echo = np.zeros((3, 37, 1024), np.uint8)
    for f in range(3):
        for k in range(37):
            for j in range(k % 7):
                echo[f, k, (k * 131 + j * 97 + f * 13) % 1024] = 20 + 30 * j + f
    assert all((echo[f, k] > 10).sum() == k % 7 for f in range(3) for k in range(37))
    return echo


@pytest.mark.parametrize("nf", [3, *EMITTED])
@pytest.mark.parametrize("stride", [1, 2, 3, 4, 5, 7, 8, 64, 5000])
def test_rank_carried_across_groups(gpu, stride, nf):
    fo, _ = _check(gpu, _repeat(gpu, _mod7_stack(), nf), 10.0, stride)
    kept = sum(k % 7 for k in range(37))  # 106 per file
    per_file = -(-kept // stride)  # (stride 5000: one output per file)
    np.testing.assert_array_equal(fo, per_file * np.arange(nf + 1))


# ---------------------------------------------------------------- every W of the launch rule
@pytest.mark.parametrize("w,nf", [(4, NF_W4), (2, NF_W2), (1, NF_W1)])
def test_every_wave_count_and_row_count(gpu, w, nf):
    """Waves without a group (rows < 4W), short last rounds, 1-row last groups, two rounds and
    more, at the smallest n_files that selects each W."""
    for rows in sorted({3, 4, 5, 4 * w - 1, 4 * w, 4 * w + 1, 8 * w + 5}):
        echo = _random_stack(gpu, nf, rows, seed=100 * w + rows)
        for stride in (4, 3):
            _check(gpu, echo, 10.0, stride)


@pytest.mark.parametrize("nf", [1499, 1500, 1536, 1537, 1702, 1703, 1792, 1793, 1945, 1946, 3840,
                                3841, 3891, 3892])
def test_both_sides_of_each_threshold(gpu, nf):
    """Every n_files of the table above, 6 or 7 rows."""
    rows = 7 if nf % 2 else 6  # a 3-row / 2-row last group
    _check(gpu, _random_stack(gpu, nf, rows, seed=nf), 10.0, 4)


# ---------------------------------------------------------------- the staged / unstaged edge
def _edge_stack(before, kept):
    """A file of 12 rows: group 0 keeps `before` samples, group 1 keeps `kept` (rows filled
    from the left), group 2 keeps 5; a second file follows so that a wrong count shifts it."""
    echo = np.zeros((2, 12, 1024), np.uint8)
    echo[0, 1, 7:7 + before] = 99
    flat = echo[0, 4:8].reshape(-1)
    flat[:kept] = (np.arange(kept) % 200 + 20).astype(np.uint8)
    echo[0, 9, 100:105] = 77
    echo[1, :, ::37] = 55
    return echo


@pytest.mark.parametrize("nf", [2, *EMITTED])
@pytest.mark.parametrize("kept", [STAGE_SLOTS, STAGE_SLOTS + 1])
def test_edge_at_stride_1(gpu, kept, nf):
    """A group emitting exactly kStageSlots (staged) and kStageSlots + 1 (unstaged) outputs."""
    for before in (0, 3):
        _check(gpu, _repeat(gpu, _edge_stack(before, kept), nf), 10.0, 1)


@pytest.mark.parametrize("nf", [2, *EMITTED])
@pytest.mark.parametrize("before", [0, 1, 2, 3])
def test_edge_at_stride_4_depends_on_the_rank(gpu, before, nf):
    """The same kept count, 4 * kStageSlots + 1: kStageSlots + 1 outputs (unstaged) after a rank
    that is a multiple of 4, kStageSlots (a full slot) after 1, 2 or 3 kept samples."""
    kept = 4 * STAGE_SLOTS + 1
    fo, _ = _check(gpu, _repeat(gpu, _edge_stack(before, kept), nf), 10.0, 4)
    assert fo[1] == -(-(before + kept + 5) // 4)


@pytest.mark.parametrize("nf", [3, NF_W2])
@pytest.mark.parametrize("stride", [8, 7])
def test_every_sample_kept(gpu, stride, nf):
    """Threshold -3 keeps all 4096 samples of a group: stride 8 fills every slot (512 outputs per
    group), stride 7 leaves every full group unstaged (585 or 586)."""
    echo = _repeat(gpu, _random_stack(gpu, 3, 13, seed=5, densities=(0.5,)), nf)
    fo, _ = _check(gpu, echo, -3.0, stride)
    np.testing.assert_array_equal(fo, -(-13 * 1024 // stride) * np.arange(nf + 1))


# ---------------------------------------------------------------- thresholds
@pytest.mark.parametrize("nf", [3, NF_W2])
@pytest.mark.parametrize("thr", [127.5, 128.0, 255.0])
def test_thresholds(gpu, thr, nf):
    """127.5 and 128 take the HI form of the keep test; 255 keeps nothing (N = 0)."""
    g = torch.Generator(device=gpu).manual_seed(9)
    echo = torch.randint(0, 256, (3, 37, 1024), generator=g, device=gpu,
                         dtype=torch.int32).to(torch.uint8)
    echo[:, :, 300:] = torch.where(echo[:, :, 300:] > 250, echo[:, :, 300:], 0)  # sparse part
    echo = _repeat(gpu, echo, nf)
    for stride in (1, 4):
        fo, _ = _check(gpu, echo, thr, stride)
        if thr == 255.0:
            assert fo[-1] == 0


# ---------------------------------------------------------------- empty files
@pytest.mark.parametrize("nf", [5, NF_W2])
@pytest.mark.parametrize("empty", [(0,), (2,), (0, 1, 2, 3, 4)])
def test_empty_files(gpu, empty, nf):
    """An empty first file, an empty file between others, an all-empty stack."""
    echo = _random_stack(gpu, 5, 21, seed=3, densities=(0.02, 0.3))
    for f in empty:
        echo[f] = 0
    for stride in (1, 4):
        fo, _ = _check(gpu, _repeat(gpu, echo, nf), 10.0, stride)
        assert all(fo[f + 1] == fo[f] for f in empty)


# ---------------------------------------------------------------- the staging is deterministic
def test_entries_identical_between_runs(gpu):
    echo = _random_stack(gpu, NF_W2, 40, seed=11)
    _, mk1 = _check(gpu, echo, 10.0, 4)
    _, mk2 = _check(gpu, echo, 10.0, 4)
    assert torch.equal(mk1, mk2)
    # a staged group's slot holds its emitted entries only: at most the file's outputs
    written = int((mk1[:-GUARD] != PATTERN).sum())
    kept = int((echo > 10).sum())
    assert 0 < written <= kept // 4 + NF_W2
