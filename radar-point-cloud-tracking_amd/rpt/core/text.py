"""``"%.6f"`` text rows: the vertex lines of ``write_ply`` (radar_pipeline/core/writers.py:45-46,
one f-string per point) and the rows of ``write_labels_csv`` (:79-81, ``np.savetxt``), formed on
the device by librpt (csrc/text.hip: rpt_text_rows_size / rpt_text_rows_write).

Both writers reduce to CPython's ``"%.6f" % float(np.float32(v))``; the kernel reproduces it in
integers for finite ``|v| < 2**40``.  Inputs outside that domain (NaN, inf, larger magnitudes),
inputs of other dtypes and hosts without a GPU take the host formatter below, which evaluates the
reference expression itself -- same bytes, at CPython's speed.

A third layout are the ``x,y,z`` rows ``DataFrame.to_csv`` writes for float32 columns
(radar_pipeline/processors/cartesian.py:46-53): every value as ``np.float32(v).astype(str)``, the
shortest decimal that reads back as the value (csrc/repr32.h).  The kernel covers every finite
value; NaN (an empty field) and inf go to the host formatter, which is the pandas expression.

A fourth are the ``"%.4f %.4f %.4f %d %d %d"`` rows ``np.savetxt`` writes in ``write_ply_fast``
(PointCloudWork/5_gain_fusion_ply_builder.py:370-403): the ``"%.6f"`` method at four decimals
(csrc/heat.h ``fixed4``), same domain, same host fallback.  ``ply4_rows_device`` also hands back
the row offsets, so that one launch over a group of frames can be cut into one slice per file.

Torch device tensors in -> a device ``uint8`` tensor out; numpy in -> ``bytes`` out.

The other way, ``parse_rows`` reads rows of plain decimal tokens (the vertex lines ``load_ply``
meets, radar_pipeline/core/loaders.py:149-220) into float32 columns on the device
(csrc/ply_parse.hip, csrc/parse32.h): ``np.float32(float(token))`` bit for bit inside a narrow
domain, ``None`` outside it -- the caller's host reader then produces the reference's value or
exception.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from .. import _abi
from .._device import is_torch, stream_handle

_HOST_CHUNK = 1 << 18      # rows per host-formatted piece
_COPY_CHUNK = 1 << 25      # bytes per pinned staging buffer
PLY4_ROW_MAX = 72          # 3 * (sign + 13 digits + '.' + 4 digits) + 3 * 3 colour digits + 6


def gpu_visible() -> bool:
    """A ROCm device and librpt.so are both there (the device formatter can run)."""
    return _abi.load(require=False) is not None and torch.cuda.is_available()


# ---- host formatter (the reference expressions) ---------------------------------------------

def _np(a) -> np.ndarray:
    return a.detach().cpu().numpy() if is_torch(a) else np.asarray(a)


def format_ply_rows_host(x, y, z, rgb) -> bytes:
    """``f"{xp:.6f} {yp:.6f} {zp:.6f} {r} {g} {b}\\n"`` per point (writers.py:45-46)."""
    x, y, z, rgb = _np(x), _np(y), _np(z), _np(rgb)
    if rgb.dtype.kind not in "iub":  # str() of a float colour is not "%d": the f-string itself
        return "".join(f"{xp:.6f} {yp:.6f} {zp:.6f} {r} {g} {b}\n"
                       for xp, yp, zp, (r, g, b) in zip(x, y, z, rgb)).encode()
    n = min(len(x), len(y), len(z), len(rgb))  # zip(strict=False)
    parts = []
    for lo in range(0, n, _HOST_CHUNK):
        s = slice(lo, min(lo + _HOST_CHUNK, n))
        c = rgb[s]
        parts.append("".join(
            ["%.6f %.6f %.6f %d %d %d\n" % t
             for t in zip(x[s].tolist(), y[s].tolist(), z[s].tolist(), c[:, 0].tolist(),
                          c[:, 1].tolist(), c[:, 2].tolist())]))
    return "".join(parts).encode()


def format_label_rows_host(x, y, z, labels) -> bytes:
    """The data rows of ``np.savetxt(column_stack((coords, labels)), fmt="%.6f,%.6f,%.6f,%d")``
    (writers.py:79-81): every column promoted to float64, ``%d`` of the label."""
    cols = [_np(a).astype(np.float64) for a in (x, y, z, labels)]
    n = len(cols[0])
    parts = []
    for lo in range(0, n, _HOST_CHUNK):
        s = slice(lo, min(lo + _HOST_CHUNK, n))
        parts.append("".join(["%.6f,%.6f,%.6f,%d\n" % t
                              for t in zip(*(c[s].tolist() for c in cols))]))
    return "".join(parts).encode()


def format_ply4_rows_host(x, y, z, rgb) -> bytes:
    """The rows of ``np.savetxt(fh, column_stack([x, y, z as float32, r, g, b as int]),
    fmt="%.4f %.4f %.4f %d %d %d")`` (5_gain_fusion_ply_builder.py:391-401): every column promoted
    to float64, ``%d`` of the colour."""
    cols = [_np(a).astype(np.float32).astype(np.float64) for a in (x, y, z)]
    c = _np(rgb)
    cols += [c[:, k].astype(int) for k in range(3)]
    n = len(cols[0])
    parts = []
    for lo in range(0, n, _HOST_CHUNK):
        s = slice(lo, min(lo + _HOST_CHUNK, n))
        parts.append("".join(["%.4f %.4f %.4f %d %d %d\n" % t
                              for t in zip(*(c[s].tolist() for c in cols))]))
    return "".join(parts).encode()


def format_xyz_rows_host(x, y, z) -> bytes:
    """The body of ``pd.DataFrame({"x": x, "y": y, "z": z}).to_csv(index=False)``
    (cartesian.py:46-53): the text without its ``x,y,z`` header line."""
    import pandas as pd

    csv = pd.DataFrame({"x": _np(x), "y": _np(y), "z": _np(z)}).to_csv(index=False)
    return csv[csv.index("\n") + 1:].encode()


# ---- device formatter -------------------------------------------------------------------------

def _device_rows(layout: int, x, y, z, tail, with_offsets: bool = False):
    """Rows of contiguous device tensors (x, y, z float32 [n]; tail uint8 [n][3], int32 [n] or
    None for the layout without one) as a device uint8 tensor, or None when a row is outside the
    kernel's domain.  with_offsets: (text, row offsets int64 [n + 1] on the device) instead."""
    dev = x.device
    n = x.numel()
    lib = _abi.load()
    tail_ptr = tail.data_ptr() if tail is not None else None
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    total = C.c_int64(0)
    bad = C.c_int64(0)
    with torch.cuda.device(dev):
        st = stream_handle(dev)
        _abi.check(lib.rpt_text_rows_size(layout, x.data_ptr(), y.data_ptr(), z.data_ptr(),
                                          tail_ptr, n, offsets.data_ptr(),
                                          C.byref(total), C.byref(bad), st),
                   "rpt_text_rows_size")
        if bad.value:
            return None
        out = torch.empty(int(total.value), dtype=torch.uint8, device=dev)
        _abi.check(lib.rpt_text_rows_write(layout, x.data_ptr(), y.data_ptr(), z.data_ptr(),
                                           tail_ptr, n, offsets.data_ptr(),
                                           out.data_ptr(), out.numel(), st),
                   "rpt_text_rows_write")
    return (out, offsets) if with_offsets else out


_RGB_LAYOUTS = (_abi.TEXT_PLY, _abi.TEXT_PLY4)


def _tail_dtype(layout: int):
    return (np.uint8, torch.uint8) if layout in _RGB_LAYOUTS else (np.int32, torch.int32)


def _device_ok(layout: int, x, y, z, tail) -> bool:
    """The arrays are what the kernel reads: float32 coordinates of one length and a uint8 [n][3]
    / int32 [n] tail (numpy labels of another integer type qualify when they fit int32)."""
    if x.ndim != 1:
        return False
    n = int(x.shape[0])
    for a in (x, y, z):
        if a.ndim != 1 or int(a.shape[0]) != n:
            return False
        if a.dtype != (torch.float32 if is_torch(a) else np.float32):
            return False
    if layout == _abi.TEXT_XYZ_REPR:
        return True
    np_t, torch_t = _tail_dtype(layout)
    want = (n, 3) if layout in _RGB_LAYOUTS else (n,)
    if tuple(tail.shape) != want:
        return False
    if is_torch(tail):
        return tail.dtype == torch_t
    if tail.dtype == np_t:
        return True
    if layout == _abi.TEXT_LABELS and tail.dtype.kind in "iu":
        return n == 0 or (int(tail.min()) >= -2**31 and int(tail.max()) < 2**31)
    return False


def _to_dev(a, dtype, dev) -> torch.Tensor:
    if not is_torch(a):
        a = torch.from_numpy(np.ascontiguousarray(a))
    return a.to(device=dev, dtype=dtype).contiguous()


def _format(layout: int, x, y, z, tail, as_tensor: Optional[bool] = None):
    arrays = (x, y, z) if layout == _abi.TEXT_XYZ_REPR else (x, y, z, tail)
    on_device = any(is_torch(a) and a.is_cuda for a in arrays)
    want_torch = all(is_torch(a) for a in arrays) if as_tensor is None else as_tensor
    text = None
    if (on_device or gpu_visible()) and _device_ok(layout, x, y, z, tail):
        dev = next((a.device for a in arrays if is_torch(a) and a.is_cuda),
                   None) or torch.device("cuda", torch.cuda.current_device())
        text = _device_rows(layout, _to_dev(x, torch.float32, dev),
                            _to_dev(y, torch.float32, dev), _to_dev(z, torch.float32, dev),
                            None if layout == _abi.TEXT_XYZ_REPR else
                            _to_dev(tail, _tail_dtype(layout)[1], dev))
    if text is None:  # no GPU, other dtypes, or values outside the kernel's domain
        raw = _HOST[layout](*arrays)
        if not want_torch:
            return raw
        t = torch.frombuffer(bytearray(raw), dtype=torch.uint8) if raw else \
            torch.empty(0, dtype=torch.uint8)
        return t.to(x.device) if is_torch(x) else t
    return text if want_torch else text.cpu().numpy().tobytes()


def format_ply_rows(x, y, z, rgb, as_tensor: Optional[bool] = None):
    """``"%.6f %.6f %.6f %d %d %d\\n"`` per point.  as_tensor: True keeps the text a tensor (on the
    device when it was formed there) whatever the inputs are, False returns bytes."""
    return _format(_abi.TEXT_PLY, x, y, z, rgb, as_tensor)


def format_label_rows(x, y, z, labels, as_tensor: Optional[bool] = None):
    """``"%.6f,%.6f,%.6f,%d\\n"`` per point; as_tensor as for format_ply_rows."""
    return _format(_abi.TEXT_LABELS, x, y, z, labels, as_tensor)


def format_xyz_rows(x, y, z, as_tensor: Optional[bool] = None):
    """``"repr(x),repr(y),repr(z)\\n"`` per point, the float32 rows of ``to_csv``; as_tensor as for
    format_ply_rows."""
    return _format(_abi.TEXT_XYZ_REPR, x, y, z, None, as_tensor)


def format_ply4_rows(x, y, z, rgb, as_tensor: Optional[bool] = None):
    """``"%.4f %.4f %.4f %d %d %d\\n"`` per point; as_tensor as for format_ply_rows."""
    return _format(_abi.TEXT_PLY4, x, y, z, rgb, as_tensor)


def ply4_rows_device(x, y, z, rgb):
    """The ``"%.4f"`` rows of contiguous device tensors (x, y, z float32 [n], rgb uint8 [n][3]) as
    (text uint8 [total], row offsets int64 [n + 1]), both on the device, or None when a coordinate
    is outside the kernel's domain (the caller then formats on the host)."""
    return _device_rows(_abi.TEXT_PLY4, x, y, z, rgb, with_offsets=True)


_HOST = {_abi.TEXT_PLY: format_ply_rows_host, _abi.TEXT_LABELS: format_label_rows_host,
         _abi.TEXT_XYZ_REPR: format_xyz_rows_host, _abi.TEXT_PLY4: format_ply4_rows_host}


# ---- device text -> file ------------------------------------------------------------------------

_pinned: list = []


def _staging(nbytes: int, count: int):
    size = min(max(nbytes, 1), _COPY_CHUNK)
    while len(_pinned) < count:
        _pinned.append(torch.empty(0, dtype=torch.uint8))
    for k in range(count):
        if _pinned[k].numel() < size:
            _pinned[k] = torch.empty(size, dtype=torch.uint8, pin_memory=True)
    return size, _pinned[:count]


def write_text(fh, text) -> None:
    """Append formatted rows to the binary file ``fh``: bytes as they are, a device tensor in
    pieces through two pinned buffers (the copy of piece k+1 runs while piece k is written)."""
    if not is_torch(text):
        fh.write(text)
        return
    n = text.numel()
    if n == 0:
        return
    if not text.is_cuda:
        fh.write(text.numpy().tobytes())
        return
    pieces = -(-n // _COPY_CHUNK)
    size, bufs = _staging(n, min(pieces, 2))
    events = [torch.cuda.Event() for _ in bufs]
    with torch.cuda.device(text.device):
        def start(k):
            lo = k * size
            cnt = min(size, n - lo)
            bufs[k % 2][:cnt].copy_(text[lo:lo + cnt], non_blocking=True)
            events[k % 2].record()
            return cnt

        cnt = start(0)
        for k in range(pieces):
            nxt = start(k + 1) if k + 1 < pieces else 0
            events[k % 2].synchronize()
            fh.write(memoryview(bufs[k % 2].numpy())[:cnt])
            cnt = nxt


# ---- text -> device columns (the reverse way) -----------------------------------------------------

PARSE_MAX_COLS = 16
_FIRST_LINE_PREFIX = 8192  # bytes of a device text looked at for the first row's token count


def text_to_device(text, dev: torch.device) -> torch.Tensor:
    """Host bytes as a device uint8 tensor, in pieces through the two pinned staging buffers (the
    host copy of piece k+1 into its buffer runs while piece k travels): write_text the other way."""
    src = np.frombuffer(text, dtype=np.uint8)
    n = src.size
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    if n == 0:
        return out
    pieces = -(-n // _COPY_CHUNK)
    size, bufs = _staging(n, min(pieces, 2))
    events = [torch.cuda.Event() for _ in bufs]
    with torch.cuda.device(dev):
        for k in range(pieces):
            lo = k * size
            cnt = min(size, n - lo)
            if k >= 2:
                events[k % 2].synchronize()  # the buffer's previous piece has left it
            bufs[k % 2].numpy()[:cnt] = src[lo:lo + cnt]
            out[lo:lo + cnt].copy_(bufs[k % 2][:cnt], non_blocking=True)
            events[k % 2].record()
        for ev in events:
            ev.synchronize()  # the staging buffers are free for the module's next user
    return out


def parse_rows_device(text: torch.Tensor, n_rows: int, n_cols: int):
    """The first n_rows lines of a contiguous device uint8 text as (float32 [n_cols, n_rows] on
    the device, None), or (None, reason) when the text is outside the kernels' domain: "size"
    (2**32 bytes or more, no row, n_cols outside 1..16), "bytes" (a byte that is none of
    ``0-9 + - . space tab \\r \\n``, a lone ``\\r``), "lines" (fewer than n_rows lines), "rows" (a
    row with another token count or a token outside csrc/parse32.h's domain)."""
    nbytes = text.numel()
    if n_rows < 1 or not 1 <= n_cols <= PARSE_MAX_COLS or nbytes >= 1 << 32:
        return None, "size"
    if n_rows > nbytes:  # a line takes a byte at least
        return None, "lines"
    dev = text.device
    if text.data_ptr() % 16:  # a slice: the kernels' 16-byte loads want an aligned base
        text = text.clone()
    lib = _abi.load()
    found = C.c_int64(0)
    bad = C.c_int64(0)
    with torch.cuda.device(dev):
        st = stream_handle(dev)
        row_start = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)  # uint32 offsets
        _abi.check(lib.rpt_text_rows_index(text.data_ptr(), nbytes, n_rows, row_start.data_ptr(),
                                           C.byref(found), C.byref(bad), st),
                   "rpt_text_rows_index")
        if bad.value:
            return None, "bytes"
        if found.value < n_rows:
            return None, "lines"
        out = torch.empty((n_cols, n_rows), dtype=torch.float32, device=dev)
        _abi.check(lib.rpt_text_rows_parse(text.data_ptr(), nbytes, row_start.data_ptr(), n_rows,
                                           n_cols, out.data_ptr(), C.byref(bad), st),
                   "rpt_text_rows_parse")
    if bad.value:
        return None, "rows"
    return out, None


def _text_len(text) -> int:
    return text.numel() if is_torch(text) else len(text)


def _first_line_tokens(text) -> int:
    """Token count of the first line (split on the host, from a prefix of the text)."""
    head = text[:_FIRST_LINE_PREFIX]
    head = head.cpu().numpy().tobytes() if is_torch(head) else bytes(head)
    end = head.find(b"\n")
    if end < 0 and _text_len(text) > _FIRST_LINE_PREFIX:
        return 0  # a first row longer than the kernels stage: outside the domain anyway
    return len((head if end < 0 else head[:end]).split())


def parse_rows_reason(text, n_rows: int, n_cols: Optional[int] = None):
    """parse_rows' work: (device float32 [n_cols, n_rows], None) or (None, reason)."""
    if is_torch(text):
        if text.dtype != torch.uint8 or text.ndim != 1:
            raise ValueError("parse_rows: text must be a one-dimensional uint8 tensor")
        on_device = text.is_cuda
    else:
        text = memoryview(text).cast("B")
        on_device = False
    if not on_device and not gpu_visible():
        raise RuntimeError("parse_rows: no ROCm device (the host reader is load_ply's)")
    n_rows = int(n_rows)
    if n_cols is None:
        n_cols = _first_line_tokens(text)
    if on_device:
        dev_text = text.contiguous()
    else:
        if n_rows < 1 or not 1 <= n_cols <= PARSE_MAX_COLS or _text_len(text) >= 1 << 32:
            return None, "size"  # before the copy
        dev = torch.device("cuda", torch.cuda.current_device())
        dev_text = text_to_device(text.contiguous().numpy() if is_torch(text) else text, dev)
    return parse_rows_device(dev_text, n_rows, int(n_cols))


def parse_rows(text, n_rows: int, n_cols: Optional[int] = None,
               as_tensor: Optional[bool] = None):
    """The first ``n_rows`` lines of ``text`` -- blank-separated decimal tokens, ``n_cols`` a line
    (None: as many as the first line holds) -- as float32 ``[n_cols, n_rows]``, every value
    ``np.float32(float(token))`` bit for bit, parsed on the device (csrc/ply_parse.hip).  text:
    bytes, a memoryview or a uint8 tensor on the host or the device.  Returns None when the text is
    outside the kernels' domain (parse_rows_device): the caller then reads it on the host.
    as_tensor: True returns a tensor (on the device for a device text), False a numpy array; by
    default a tensor in gives a tensor out."""
    want_torch = is_torch(text) if as_tensor is None else as_tensor
    to_host = not (is_torch(text) and text.is_cuda)
    out, _ = parse_rows_reason(text, n_rows, n_cols)
    if out is None:
        return None
    if not want_torch:
        return out.cpu().numpy()
    return out.cpu() if to_host and as_tensor is None else out


def text_to_host(text: torch.Tensor) -> memoryview:
    """A device text in host memory by ONE copy: through the first pinned staging buffer when it
    fits there (the view is valid until the next call of this module that stages), else by a
    pageable copy."""
    n = text.numel()
    if n == 0:
        return memoryview(b"")
    if not text.is_cuda:
        return memoryview(text.numpy())
    if n > _COPY_CHUNK:
        return memoryview(text.cpu().numpy())
    _, bufs = _staging(n, 1)
    with torch.cuda.device(text.device):
        bufs[0][:n].copy_(text, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    return memoryview(bufs[0].numpy())[:n]
