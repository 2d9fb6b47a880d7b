"""load_ply with its vertex rows parsed on the device (csrc/ply_parse.hip through
rpt.core.text.parse_rows) against the host reader ``load_ply(device=False)``, which is the
reference's code: x, y, z bit for bit as uint32, colours as uint8, exceptions by type and message,
and the parser that ran (``info["parser"]``)."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HEAD6 = ["property float x", "property float y", "property float z",
         "property uchar red", "property uchar green", "property uchar blue"]


def _header(n, props=HEAD6, eol="\n"):
    return eol.join(["ply", "format ascii 1.0", f"element vertex {n}", *props, "end_header"]) + eol


def _tile():
    from rpt import _abi

    return int(_abi.load().rpt_text_tile_bytes())


def _outcome(fn):
    try:
        return fn(), None
    except Exception as e:  # noqa: BLE001 -- the exception itself is what is compared
        return None, (type(e), str(e))


def _compare(path, parser, reason=None):
    """load_ply(path) against load_ply(path, device=False): identical result or exception, and
    the expected parser.  Returns the device-side cloud (None when both raised)."""
    from rpt.core.loaders import load_ply

    info = {}
    got, got_err = _outcome(lambda: load_ply(path, info=info))
    ref, ref_err = _outcome(lambda: load_ply(path, device=False))
    assert info.get("parser") == parser, info
    if reason is not None:
        assert info.get("reason") == reason, info
    assert got_err == ref_err
    if ref is None:
        return None
    for a, b in ((got.x, ref.x), (got.y, ref.y), (got.z, ref.z)):
        assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape
        assert a.ndim == 1
        np.testing.assert_array_equal(a.view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    if ref.colors is None:
        assert got.colors is None
    else:
        assert got.colors.dtype == np.uint8 and got.colors.shape == ref.colors.shape
        np.testing.assert_array_equal(got.colors, ref.colors)
    return got


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-5000.0, 5000.0, (3, n)).astype(np.float32)
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    return xyz, rgb


def _writer_rows(xyz, rgb) -> bytes:
    from rpt.core.text import format_ply_rows

    return format_ply_rows(xyz[0], xyz[1], xyz[2], rgb, as_tensor=False)


def _rows_over_tiles():
    """A row count whose body spans at least 3 tiles plus a remainder (rows of 36..54 bytes)."""
    return (3 * _tile()) // 36 + 101


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, "tiles"])
def test_round_trip_of_the_device_writer(gpu, tmp_path, n):
    if n == "tiles":
        n = _rows_over_tiles()
    xyz, rgb = _cloud(n, 100 + n)
    body = _writer_rows(xyz, rgb)
    if n >= 4097:
        assert len(body) > 3 * _tile() and len(body) % _tile() != 0
    p = tmp_path / "w.ply"
    p.write_bytes(_header(n).encode() + body)
    got = _compare(p, "device")
    # the writer rounds at the sixth decimal (<= 5e-7) and the reader to float32: half an ulp,
    # below 5e-7 for |v| < 16 and nothing above (the ulp there exceeds 1e-6: the value comes back)
    for k, col in enumerate((got.x, got.y, got.z)):
        np.testing.assert_allclose(col, xyz[k], rtol=0.0, atol=1e-6)
        big = np.abs(xyz[k]) >= 16.0
        np.testing.assert_array_equal(col[big].view(np.uint32), xyz[k][big].view(np.uint32))
    np.testing.assert_array_equal(got.colors, rgb)


def test_three_columns_no_colours(gpu, tmp_path):
    xyz, _ = _cloud(777, 3)
    rows = "".join("%.6f %.6f %.6f\n" % tuple(map(float, p)) for p in xyz.T)
    p = tmp_path / "k3.ply"
    p.write_text(_header(777, HEAD6[:3]) + rows)
    got = _compare(p, "device")
    assert got.colors is None and got.x.shape == (777,)


def test_seven_columns_with_alpha(gpu, tmp_path):
    xyz, rgb = _cloud(500, 7)
    rows = "".join("%.6f %.6f %.6f %d %d %d %d\n" % (*map(float, p), *c, 255 - int(c[0]))
                   for p, c in zip(xyz.T, rgb))
    p = tmp_path / "k7.ply"
    p.write_text(_header(500, HEAD6 + ["property uchar alpha"]) + rows)
    got = _compare(p, "device")
    np.testing.assert_array_equal(got.colors, rgb)


def test_mixed_separators_and_line_endings(gpu, tmp_path):
    xyz, rgb = _cloud(300, 11)
    rng = np.random.default_rng(12)
    seps = [" ", "  ", "\t", " \t ", "\t\t"]
    rows = []
    for i, (pt, c) in enumerate(zip(xyz.T, rgb)):
        toks = ["%.6f" % float(v) for v in pt] + [str(int(v)) for v in c]
        if i % 7 == 0:
            toks[0] = "+" + toks[0].lstrip("-")
        if i % 11 == 0:
            toks[1] = toks[1].rstrip("0")  # "12." style and fewer decimals
        row = "".join(t + seps[int(rng.integers(len(seps)))] for t in toks[:-1]) + toks[-1]
        rows.append(seps[int(rng.integers(len(seps)))] * (i % 3) + row + " \t" * (i % 2))
    faces = ["3 0 1 2", "3 1 2 3", "4 0 1 2 3"]
    props = HEAD6 + ["element face 3", "property list uchar int vertex_indices"]
    body = "\r\n".join(rows) + "\r\n" + "\r\n".join(faces) + "\r\n"
    p = tmp_path / "crlf.ply"
    p.write_bytes((_header(300, props, eol="\r\n") + body).encode())
    _compare(p, "device")
    # no newline behind the last row, \n line ends
    q = tmp_path / "open.ply"
    q.write_bytes((_header(300) + "\n".join(rows)).encode())
    _compare(q, "device")
    # ... and with \r\n everywhere else
    r = tmp_path / "open_crlf.ply"
    r.write_bytes((_header(300, eol="\r\n") + "\r\n".join(rows)).encode())
    _compare(r, "device")


def _token(rng, nd):
    """A token of nd bytes inside parse32's domain: digits, a point and a sign where they fit,
    leading zeros beyond 15 bytes (at most 19 digits count, and their integer stays below 2^53)."""
    s = "0" * max(nd - 15, 0) + "".join(str(int(d)) for d in rng.integers(0, 10, min(nd, 15)))
    if nd >= 3 and rng.random() < 0.8:
        k = int(rng.integers(max(nd - 15, 1), nd))
        s = s[:k] + "." + s[k + 1:]
    if nd >= 4 and rng.random() < 0.5:
        s = "-" + s[1:]
    return s


def _row(rng, length, eol, first_min=1):
    """A row of exactly `length` bytes: three tokens, single blanks, its line end."""
    digits = length - len(eol) - 2
    assert digits >= first_min + 2
    a = int(rng.integers(first_min, digits - 1))
    b = int(rng.integers(1, digits - a))
    row = " ".join(_token(rng, nd) for nd in (a, b, digits - a - b)) + eol
    assert len(row) == length
    return row


def _rows_until(rng, rows, pos, end):
    """Rows of 6..60 bytes appended until the text ends exactly at byte `end`; the last of them
    ends in \\r\\n."""
    while pos < end:
        left = end - pos
        if left <= 60:
            length, eol = left, "\r\n"
        elif left < 120:
            length, eol = left // 2, "\n"  # leaves 31..60 for the last row
        else:
            length = int(rng.integers(6, 61))
            eol = "\r\n" if length >= 7 and rng.random() < 0.5 else "\n"
        assert 6 + (eol == "\r\n") <= length <= 60
        rows.append(_row(rng, length, eol))
        pos += length
    assert pos == end
    return pos


def test_rows_across_tile_edges(gpu, tmp_path):
    """Row lengths from 6 to 60 bytes: a row start on every residue mod 16, a \\r\\n pair and a
    token straddling a multiple of the tile size."""
    T = _tile()
    rng = np.random.default_rng(16)
    rows = []
    pos = _rows_until(rng, rows, 0, T + 1)           # ... \r at T - 1, \n at T
    pos = _rows_until(rng, rows, pos, 2 * T - 2)     # the next row starts 2 bytes before 2T
    rows.append(_row(rng, 40, "\n", first_min=4))    # its first token lies across 2T
    pos = _rows_until(rng, rows, pos + 40, 2 * T + 1500)
    raw = "".join(rows).encode()
    n = len(rows)
    lengths = np.array([len(r) for r in rows])
    assert lengths.min() == 6 and lengths.max() == 60
    starts = np.concatenate(([0], np.cumsum(lengths)[:-1]))
    assert set((starts % 16).tolist()) == set(range(16))
    edges = [k * T for k in range(1, len(raw) // T + 1)]
    assert len(edges) == 2
    assert any(raw[e - 1:e + 1] == b"\r\n" for e in edges)
    blanks = b" \t\r\n"
    assert any(raw[e - 1] not in blanks and raw[e] not in blanks for e in edges)
    p = tmp_path / "edges.ply"
    p.write_bytes(_header(n, HEAD6[:3]).encode() + raw)
    _compare(p, "device")


def _defect_file(tmp_path, name, rows, n=None, eol="\n", tail=b""):
    p = tmp_path / f"{name}.ply"
    n = len(rows) if n is None else n
    p.write_bytes(_header(n).encode() + (eol.join(rows) + eol).encode("utf-8") + tail)
    return p


def _rows200(seed=5):
    xyz, rgb = _cloud(200, seed)
    return ["%.6f %.6f %.6f %d %d %d" % (*map(float, p), *c) for p, c in zip(xyz.T, rgb)]


DEFECTS = {
    "exponent": ("bytes", lambda r: r.replace(r.split()[1], "1.5e3", 1)),
    "nan": ("bytes", lambda r: r.replace(r.split()[2], "nan", 1)),
    "one_more": ("rows", lambda r: r + " 7"),
    "one_less": ("rows", lambda r: r.rsplit(" ", 1)[0]),
    "blank_row": ("rows", lambda r: "  "),
    "lone_cr": ("bytes", lambda r: r.replace(" ", "\r", 1)),
    "form_feed": ("bytes", lambda r: r.replace(" ", "\x0c", 1)),
    "utf8": ("bytes", lambda r: r.replace(" ", "é ", 1)),
    "twenty_digits": ("rows", lambda r: r.replace(r.split()[0], "18446744073709551621", 1)),
}


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_fallback_on_a_defect_in_row_150(gpu, tmp_path, name):
    reason, edit = DEFECTS[name]
    rows = _rows200()
    rows[150] = edit(rows[150])
    _compare(_defect_file(tmp_path, name, rows), "host", reason)


def test_rows_wider_than_the_staging_share(gpu, tmp_path):
    """64 rows of more than 96 bytes do not fit a wave's LDS span: the wave reads global memory
    per lane, still on the device.  One row beyond the staging capacity is outside the domain."""
    rows = [r.replace(" ", " " * 30) + " " * (k % 50) for k, r in enumerate(_rows200(seed=8))]
    assert min(len(r) for r in rows) > 150
    _compare(_defect_file(tmp_path, "wide", rows), "device")
    rows[150] = rows[150].replace(" " * 30, " " * 1400)
    assert len(rows[150]) > 6200
    _compare(_defect_file(tmp_path, "too_wide", rows), "host", "rows")


def test_fallback_on_too_few_lines(gpu, tmp_path):
    rows = _rows200()
    _compare(_defect_file(tmp_path, "short", rows, n=201), "host", "lines")


def test_fallback_on_zero_vertices(gpu, tmp_path):
    rows = _rows200()
    _compare(_defect_file(tmp_path, "zero", rows, n=0), "host", "size")


def test_parse_rows_on_device_tensors(gpu, tmp_path):
    import torch

    from rpt.core.loaders import load_ply
    from rpt.core.text import format_ply_rows, parse_rows

    n = 1000
    xyz, rgb = _cloud(n, 21)
    x, y, z = (torch.from_numpy(a).to(gpu) for a in xyz)
    text = format_ply_rows(x, y, z, torch.from_numpy(rgb).to(gpu))
    assert text.is_cuda and text.dtype == torch.uint8
    out = parse_rows(text, n, 6)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (6, n)
    p = tmp_path / "t.ply"
    p.write_bytes(_header(n).encode() + text.cpu().numpy().tobytes())
    ref = load_ply(p, device=False)
    host = out.cpu().numpy()
    for k, col in enumerate((ref.x, ref.y, ref.z)):
        np.testing.assert_array_equal(host[k].view(np.uint32),
                                      np.ascontiguousarray(col).view(np.uint32))
    np.testing.assert_array_equal(host[3:].T.astype(np.uint8), ref.colors)
    # n_cols from the first line; a misaligned slice of a device text; bytes in, numpy out
    np.testing.assert_array_equal(parse_rows(text, n).cpu().numpy(), host)
    first = int(text.cpu().numpy().tobytes().index(b"\n")) + 1
    np.testing.assert_array_equal(parse_rows(text[first:], n - 1, 6).cpu().numpy(), host[:, 1:])
    as_np = parse_rows(text.cpu().numpy().tobytes(), n)
    assert isinstance(as_np, np.ndarray) and as_np.dtype == np.float32
    np.testing.assert_array_equal(as_np, host)
    on_host = parse_rows(text.cpu(), n)  # a host tensor in: a host tensor out
    assert isinstance(on_host, torch.Tensor) and not on_host.is_cuda
    np.testing.assert_array_equal(on_host.numpy(), host)
    # outside the domain: None
    assert parse_rows(text, n + 1, 6) is None
    assert parse_rows(text, n, 5) is None
    assert parse_rows(b"1 2 3\n4 5 x\n", 2) is None


def test_cluster_labels_csv_is_the_same_with_either_parser(gpu, tmp_path, monkeypatch, capsys):
    from rpt.core import loaders
    from rpt.processors.clustering import process_ply_clustering

    rng = np.random.default_rng(31)
    pal = np.array([(0, 114, 255), (0, 200, 83), (255, 87, 34)], np.uint8)
    n = 5000
    centres = rng.random((25, 2)) * 400 - 200
    which = rng.integers(0, 25, n)
    gain = rng.integers(0, 3, n)
    xy = centres[which] + rng.normal(0, 2.0, (n, 2))
    z = np.array([500.0, 250.0, 0.0])[gain] + rng.random(n) * 40
    xyz = np.stack([xy[:, 0], xy[:, 1], z]).astype(np.float32)
    p = tmp_path / "stack.ply"
    p.write_bytes(_header(n).encode() + _writer_rows(xyz, pal[gain]))

    info = {}
    loaders.load_ply(p, info=info)
    assert info["parser"] == "device"
    out_dev = tmp_path / "dev"
    out_host = tmp_path / "host"
    out_dev.mkdir()
    out_host.mkdir()
    csv_dev, labels_dev = process_ply_clustering(p, out_dev)
    text_dev = capsys.readouterr().out
    monkeypatch.setattr(loaders.load_ply, "__defaults__", (False, None))
    loaders.load_ply(p, info=info)
    assert info == {"parser": "host", "reason": "forced"}
    csv_host, labels_host = process_ply_clustering(p, out_host)
    text_host = capsys.readouterr().out
    assert labels_dev.max() >= 1  # clusters were found: the CSVs are not trivially equal
    np.testing.assert_array_equal(labels_dev, labels_host)
    assert csv_dev.read_bytes() == csv_host.read_bytes()
    assert text_dev == text_host
