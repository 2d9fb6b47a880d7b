"""The device shortest-repr row formatter (layout RPT_TEXT_XYZ_REPR of csrc/text.hip, through
rpt.core.text.format_xyz_rows) against numpy's ``np.float32(v).astype(str)`` on the stratified
pool: block edges and a multi-block scan, guard bytes around the output, offsets that are not the
input's, and the host fallback for NaN and inf."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from _repr_pool import numpy_repr, pool

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 255, 256, 257, 70001)
N_MAX = max(SIZES)


@pytest.fixture(scope="module")
def columns():
    """x, y, z: three rotations of the pool (N_MAX values: the named ones first, 131 random
    mantissas per exponent and sign, topped up with random finite bit patterns) and their rows as
    numpy prints them; a test of n rows takes the first n."""
    p = pool(131)
    rng = np.random.default_rng(1311)
    extra = rng.integers(0, 2**32, 4 * (N_MAX - len(p)), dtype=np.uint64).astype(np.uint32)
    extra = extra.view(np.float32)
    extra = extra[np.isfinite(extra)][:N_MAX - len(p)]
    p = np.concatenate([p, extra])
    assert len(p) == N_MAX
    x, y, z = p, np.roll(p, 23331)[::-1].copy(), np.roll(p, 46667).copy()
    rx, ry, rz = numpy_repr(x), numpy_repr(y), numpy_repr(z)
    rows = [f"{a},{b},{c}\n" for a, b, c in zip(rx.tolist(), ry.tolist(), rz.tolist())]
    assert max(len(r) for r in rows[:300]) <= 60
    return dict(x=x, y=y, z=z, rows=rows)


def _args(columns, n, gpu):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(columns[k][:n])).to(gpu) for k in "xyz"]


def _expected(columns, n) -> bytes:
    return "".join(columns["rows"][:n]).encode()


@pytest.mark.parametrize("n", SIZES)
def test_rows_match_numpy(columns, gpu, n):
    import torch

    from rpt.core import text

    out = text.format_xyz_rows(*_args(columns, n, gpu))
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8
    got = out.cpu().numpy().tobytes()
    exp = _expected(columns, n)
    if got != exp:  # name the first row that differs instead of dumping megabytes
        rows = got.split(b"\n")
        for i, want in enumerate(exp.split(b"\n")):
            assert i < len(rows) and rows[i] == want, (i, rows[i:i + 1], want)
    assert got == exp


def test_numpy_in_gives_bytes(columns, gpu):
    from rpt.core import text

    n = 300
    got = text.format_xyz_rows(columns["x"][:n], columns["y"][:n], columns["z"][:n])
    assert isinstance(got, bytes) and got == _expected(columns, n)


def _abi_rows(gpu, x, y, z, guard=0, shift=0, short=0, offsets=None):
    """rpt_text_rows_size + rpt_text_rows_write (tail NULL) straight through the ABI into a buffer
    with `guard` bytes of 0xA5 on both sides (the output starts `shift` bytes further in);
    out_bytes is the total minus `short`; `offsets` replaces the row offsets given to the write."""
    import torch

    from rpt import _abi
    from rpt._device import stream_handle

    lib = _abi.load()
    n = x.numel()
    off = torch.empty(n + 1, dtype=torch.int64, device=gpu)
    total, bad = C.c_int64(-1), C.c_int64(-1)
    st = stream_handle(gpu)
    _abi.check(lib.rpt_text_rows_size(_abi.TEXT_XYZ_REPR, x.data_ptr(), y.data_ptr(),
                                      z.data_ptr(), None, n, off.data_ptr(), C.byref(total),
                                      C.byref(bad), st))
    buf = torch.full((guard + shift + total.value + guard,), 0xA5, dtype=torch.uint8, device=gpu)
    used = off if offsets is None else offsets(off)
    _abi.check(lib.rpt_text_rows_write(_abi.TEXT_XYZ_REPR, x.data_ptr(), y.data_ptr(),
                                       z.data_ptr(), None, n, used.data_ptr(),
                                       buf.data_ptr() + guard + shift, total.value - short, st))
    torch.cuda.synchronize()
    return total.value, bad.value, off.cpu().numpy(), buf.cpu().numpy()


@pytest.mark.parametrize("shift", [0, 5])
def test_guard_bytes_untouched(columns, gpu, shift):
    n, guard = 1000, 64
    total, bad, off, buf = _abi_rows(gpu, *_args(columns, n, gpu), guard=guard, shift=shift)
    exp = _expected(columns, n)
    assert bad == 0 and total == len(exp) and off[0] == 0 and off[-1] == total
    np.testing.assert_array_equal(np.diff(off), [len(r) for r in columns["rows"][:n]])
    lo = guard + shift
    assert buf[lo:lo + total].tobytes() == exp
    assert (buf[:lo] == 0xA5).all() and (buf[lo + total:] == 0xA5).all()


def test_short_output_is_never_overrun(columns, gpu):
    """out_bytes one byte short of the total: the last block of rows does not fit and is left
    out as a whole; the rows before it are written and nothing lands behind out_bytes."""
    n, guard = 600, 64
    total, bad, off, buf = _abi_rows(gpu, *_args(columns, n, gpu), guard=guard, short=1)
    exp = _expected(columns, n)
    fits = int(off[512])  # blocks of 256 rows: rows 512.. belong to the block that does not fit
    assert buf[guard:guard + fits].tobytes() == exp[:fits]
    assert (buf[guard + fits:] == 0xA5).all() and (buf[:guard] == 0xA5).all()


@pytest.mark.parametrize("kind", ["doubled", "negative", "one_row_short", "beyond"])
def test_wrong_offsets_write_nothing_outside(columns, gpu, kind):
    """Offsets that are not this input's: whatever is skipped or written, every byte outside
    [out, out + out_bytes) keeps its guard value, and a row is written only where its own length
    fits its slot."""
    n, guard = 600, 256

    def wrong(off):
        o = off.clone()
        if kind == "doubled":
            o *= 2               # no row fits its slot; later blocks end behind out_bytes
        elif kind == "negative":
            o -= int(off[-1]) + 1
        elif kind == "one_row_short":
            o[300:] -= 1         # row 299 loses a byte: it is skipped, the block still fits
        else:
            o += int(off[-1])    # a consistent copy of the offsets, all of it behind out_bytes
        return o

    total, bad, off, buf = _abi_rows(gpu, *_args(columns, n, gpu), guard=guard, offsets=wrong)
    assert bad == 0
    assert (buf[:guard] == 0xA5).all() and (buf[guard + total:] == 0xA5).all()
    body = buf[guard:guard + total].tobytes()
    exp = _expected(columns, n)
    if kind in ("negative", "beyond"):
        assert body == b"\xa5" * total
    elif kind == "one_row_short":
        cut = int(off[299])
        assert body[:cut] == exp[:cut]                       # rows 0..298 where they belong
        assert body[int(off[300]) - 1:int(off[512]) - 1] == exp[int(off[300]):int(off[512])]


def test_nan_and_inf_take_the_host_formatter(columns, gpu):
    import pandas as pd
    import torch

    from rpt.core import text

    n = 700
    x, y, z = (columns[k][:n].copy() for k in "xyz")
    x[3], y[300], z[511], x[699], y[699] = np.nan, np.inf, -np.inf, np.nan, np.nan
    z[699] = 37.0
    dev = [torch.from_numpy(a).to(gpu) for a in (x, y, z)]
    total, bad, off, _ = _abi_rows(gpu, *dev)
    assert bad == 4
    assert [int(v) for v in np.flatnonzero(np.diff(off) == 0)] == [3, 300, 511, 699]
    exp = pd.DataFrame({"x": x, "y": y, "z": z}).to_csv(index=False)[len("x,y,z\n"):]
    assert "\n,,37.0\n" in exp and ",inf," in exp and ",-inf\n" in exp
    out = text.format_xyz_rows(*dev)
    assert isinstance(out, torch.Tensor) and out.cpu().numpy().tobytes() == exp.encode()
