"""The device "%.6f" row formatter (csrc/text.hip through rpt.core.text) against CPython's own
formatting of the same float32 values: both layouts, block edges and a multi-block scan, exact
ties, signed zeros, subnormals, the edge of the domain, the host fallback for values outside it,
and guard bytes around the output."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 255, 256, 257, 70001)
N_MAX = max(SIZES)
LABELS = np.array([-1, 0, 9, 10, 99999, 2**31 - 1, -2**31], dtype=np.int32)
RGB = np.array([0, 9, 10, 99, 100, 255], dtype=np.uint8)


def _pool() -> np.ndarray:
    """N_MAX float32 values: the special cases first, then (shuffled) every odd multiple of 2^-7
    below 313 -- exact ties at the sixth decimal --, random bit patterns inside the domain and
    uniform values in +-600."""
    rng = np.random.default_rng(20240612)
    special = np.array([0.0, -0.0, 2.5e-7, 5e-7, -4e-7, 2.0**40 - 2.0**17, -(2.0**40 - 2.0**17),
                        1e-45, -1e-45, 1.1754942e-38, -5e-39, 0.9999995, 0.99999994, 9.9999995,
                        999999.9375, 1e6, 1e12, 1.5e-6, 2.5e-6, 4.9999999e-7, 5.0000001e-7,
                        600.0, -600.0, 0.0078125, -0.0078125], dtype=np.float32)
    ties = (np.arange(1, 313 * 128, 2, dtype=np.float64) / 128.0).astype(np.float32)
    ties[1::2] *= -1.0
    bits = rng.integers(0, 2**32, 40000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    with np.errstate(invalid="ignore"):
        bits = bits[np.isfinite(bits) & (np.abs(bits) < np.float32(2.0**40))][:20000]
    rest = N_MAX - len(special) - len(ties) - len(bits)
    assert rest > 10000
    uni = rng.uniform(-600.0, 600.0, rest).astype(np.float32)
    body = np.concatenate([ties, bits, uni])
    rng.shuffle(body)
    return np.concatenate([special, body])


@pytest.fixture(scope="module")
def columns():
    """x, y, z (float32), rgb (uint8 [n][3]) and labels (int32) of N_MAX rows with their rows as
    CPython formats them; a test of n rows takes the first n."""
    p = _pool()
    x, y, z = p, np.roll(p, 23331)[::-1].copy(), -np.roll(p, 46667)
    k = np.arange(N_MAX)
    rgb = np.stack([RGB[k % 6], RGB[(k // 6) % 6], RGB[(k // 36) % 6]], axis=1)
    labels = LABELS[k % len(LABELS)]
    xs, ys, zs = x.tolist(), y.tolist(), z.tolist()  # float(np.float32(v)), exact
    ply = ["%.6f %.6f %.6f %d %d %d\n" % (a, b, c, int(r), int(g), int(bl))
           for a, b, c, (r, g, bl) in zip(xs, ys, zs, rgb.tolist())]
    lab = ["%.6f,%.6f,%.6f,%d\n" % (a, b, c, l) for a, b, c, l in zip(xs, ys, zs, labels.tolist())]
    return dict(x=x, y=y, z=z, rgb=rgb, labels=labels, ply=ply, lab=lab)


def _args(columns, layout, n, gpu):
    import torch

    tail = columns["rgb"] if layout == "ply" else columns["labels"]
    arrs = [columns["x"][:n], columns["y"][:n], columns["z"][:n], tail[:n]]
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrs]


def _expected(columns, layout, n) -> bytes:
    return "".join(columns["ply" if layout == "ply" else "lab"][:n]).encode()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", ["ply", "labels"])
def test_rows_match_python(columns, gpu, layout, n):
    import torch

    from rpt.core import text

    fmt = text.format_ply_rows if layout == "ply" else text.format_label_rows
    out = fmt(*_args(columns, layout, n, gpu))
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8
    got = out.cpu().numpy().tobytes()
    exp = _expected(columns, layout, n)
    if got != exp:  # name the first row that differs instead of dumping megabytes
        rows = got.split(b"\n")
        for i, want in enumerate(exp.split(b"\n")):
            assert i < len(rows) and rows[i] == want, (i, rows[i:i + 1], want)
    assert got == exp


def test_numpy_in_gives_bytes(columns, gpu):
    from rpt.core import text

    n = 300
    got = text.format_ply_rows(columns["x"][:n], columns["y"][:n], columns["z"][:n],
                               columns["rgb"][:n])
    assert isinstance(got, bytes) and got == _expected(columns, "ply", n)
    got = text.format_label_rows(columns["x"][:n], columns["y"][:n], columns["z"][:n],
                                 columns["labels"][:n].astype(np.int64))
    assert isinstance(got, bytes) and got == _expected(columns, "labels", n)


def _abi_rows(gpu, layout_code, x, y, z, tail, guard=0, shift=0, short=0):
    """rpt_text_rows_size + rpt_text_rows_write straight through the ABI into a buffer with
    `guard` bytes of 0xA5 on both sides (the output starts `shift` bytes further in, so that it
    is not 16-byte aligned); out_bytes is the total minus `short`."""
    import torch

    from rpt import _abi
    from rpt._device import stream_handle

    lib = _abi.load()
    n = x.numel()
    off = torch.empty(n + 1, dtype=torch.int64, device=gpu)
    total, bad = C.c_int64(-1), C.c_int64(-1)
    st = stream_handle(gpu)
    _abi.check(lib.rpt_text_rows_size(layout_code, x.data_ptr(), y.data_ptr(), z.data_ptr(),
                                      tail.data_ptr(), n, off.data_ptr(), C.byref(total),
                                      C.byref(bad), st))
    buf = torch.full((guard + shift + total.value + guard,), 0xA5, dtype=torch.uint8, device=gpu)
    _abi.check(lib.rpt_text_rows_write(layout_code, x.data_ptr(), y.data_ptr(), z.data_ptr(),
                                       tail.data_ptr(), n, off.data_ptr(),
                                       buf.data_ptr() + guard + shift, total.value - short, st))
    torch.cuda.synchronize()
    return total.value, bad.value, off.cpu().numpy(), buf.cpu().numpy()


@pytest.mark.parametrize("layout", ["ply", "labels"])
@pytest.mark.parametrize("shift", [0, 5])
def test_guard_bytes_untouched(columns, gpu, layout, shift):
    from rpt import _abi

    n, guard = 1000, 64
    code = _abi.TEXT_PLY if layout == "ply" else _abi.TEXT_LABELS
    total, bad, off, buf = _abi_rows(gpu, code, *_args(columns, layout, n, gpu), guard=guard,
                                     shift=shift)
    exp = _expected(columns, layout, n)
    assert bad == 0 and total == len(exp) and off[0] == 0 and off[-1] == total
    lens = [len(r) for r in columns["ply" if layout == "ply" else "lab"][:n]]
    np.testing.assert_array_equal(np.diff(off), lens)
    lo = guard + shift
    assert buf[lo:lo + total].tobytes() == exp
    assert (buf[:lo] == 0xA5).all() and (buf[lo + total:] == 0xA5).all()


def test_short_output_is_never_overrun(columns, gpu):
    """out_bytes one byte short of the total: the last block of rows does not fit and is left
    out as a whole; the rows before it are written and nothing lands behind out_bytes."""
    from rpt import _abi

    n, guard = 600, 64
    total, bad, off, buf = _abi_rows(gpu, _abi.TEXT_LABELS, *_args(columns, "labels", n, gpu),
                                     guard=guard, short=1)
    exp = _expected(columns, "labels", n)
    fits = int(off[512])  # blocks of 256 rows: rows 512.. belong to the block that does not fit
    assert buf[guard:guard + fits].tobytes() == exp[:fits]
    assert (buf[guard + fits:] == 0xA5).all() and (buf[:guard] == 0xA5).all()


@pytest.mark.parametrize("layout", ["ply", "labels"])
def test_out_of_domain_values_take_the_host_formatter(columns, gpu, layout):
    import torch

    from rpt import _abi
    from rpt.core import text

    n = 700
    x, y, z = (columns[k][:n].copy() for k in "xyz")
    x[3], y[300], z[511], x[699], y[0] = np.nan, np.inf, -np.inf, 1e20, 2.0**40
    tail = (columns["rgb"] if layout == "ply" else columns["labels"])[:n]
    dev = [torch.from_numpy(a).to(gpu) for a in (x, y, z, np.ascontiguousarray(tail))]
    code = _abi.TEXT_PLY if layout == "ply" else _abi.TEXT_LABELS
    total, bad, off, _ = _abi_rows(gpu, code, *dev)
    assert bad == 5
    assert [int(v) for v in np.flatnonzero(np.diff(off) == 0)] == [0, 3, 300, 511, 699]
    if layout == "ply":
        exp = "".join("%.6f %.6f %.6f %d %d %d\n" % (a, b, c, r, g, bl) for a, b, c, (r, g, bl)
                      in zip(x.tolist(), y.tolist(), z.tolist(), tail.tolist()))
        out = text.format_ply_rows(*dev)
    else:
        exp = "".join("%.6f,%.6f,%.6f,%d\n" % t
                      for t in zip(x.tolist(), y.tolist(), z.tolist(), tail.tolist()))
        out = text.format_label_rows(*dev)
    assert "nan" in exp and "-inf" in exp and "100000002004087734272.000000" in exp
    assert isinstance(out, torch.Tensor) and out.cpu().numpy().tobytes() == exp.encode()
