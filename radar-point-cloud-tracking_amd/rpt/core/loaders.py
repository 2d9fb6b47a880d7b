"""Drop-in for ``radar_pipeline.core.loaders`` containers and loaders
(radar-pipeline/src/radar_pipeline/core/loaders.py:15-101, :149-220).

The containers are the boundary types of the path.  load_radar_csv parses with librpt's native
CSV reader (csrc/csv.cpp; pandas read_csv semantics, checked against pandas
in tests/test_csv_ingest.py); the PLY reader keeps the reference's ASCII semantics.
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import numpy as np

from ..config import RadarConfig


@dataclass
class RadarSweep:
    """loaders.py:15-24"""

    angles_rad: np.ndarray
    ranges: np.ndarray
    intensities: np.ndarray
    scale: np.ndarray
    gain: Optional[int] = None
    source_path: Optional[Path] = None


@dataclass
class PointCloud:
    """loaders.py:27-43"""

    x: np.ndarray
    y: np.ndarray
    z: np.ndarray
    colors: Optional[np.ndarray] = None

    @property
    def size(self) -> int:
        numel = getattr(self.x, "numel", None)  # torch members (the build path keeps them there)
        return numel() if numel is not None else self.x.size

    def to_coords(self) -> np.ndarray:
        return np.column_stack((self.x, self.y, self.z))


def load_radar_csv(path: Path, config: Optional[RadarConfig] = None) -> RadarSweep:
    """loaders.py:46-101: pd.read_csv(names=Status..Echo_n, skiprows=1) semantics through the
    native parser; an empty CSV raises ValueError, a malformed one raises like read_csv."""
    from .ingest import (GAIN_DISAGREE, GAIN_FIRST_NAN, STATUS_EMPTY, STATUS_NON_NUMERIC,
                         STATUS_OK, read_sweeps)

    if config is None:
        config = RadarConfig()
    path = Path(path)
    if not path.exists():
        raise FileNotFoundError(f"[Errno 2] No such file or directory: '{path}'")
    b = read_sweeps([path], bins=config.num_echo_columns)
    st = int(b.status[0])
    if st == STATUS_EMPTY:
        raise ValueError(f"CSV is empty: {path}")
    if st == STATUS_NON_NUMERIC:
        raise ValueError(f"could not convert string to float in {path}")
    if st != STATUS_OK:  # read_csv's own exception text (ParserError is a ValueError)
        raise ValueError(b.errors[0] or f"Error tokenizing data in {path}")
    n = int(b.rows[0])
    angles_rad = np.deg2rad(b.angle[0, :n] * config.angle_scale)
    echo = b.echo[0, :n].astype(np.float32)
    scale = b.scale[0, :n].copy()
    ranges = (scale[:, None] / echo.shape[1]) * np.arange(echo.shape[1], dtype=np.float32)
    # gains = df["Gain"].unique(); one value -> int(it) (int(nan) raises), several -> None (:88-92)
    flags = int(b.gain_flags[0])
    gain = None
    if not flags & GAIN_DISAGREE:
        if flags & GAIN_FIRST_NAN:
            raise ValueError("cannot convert float NaN to integer")
        gain = int(float(b.gain[0]))
    return RadarSweep(angles_rad=angles_rad, ranges=ranges, intensities=echo, scale=scale,
                      gain=gain, source_path=path)


def _simple_sweep_echo(path: Path) -> np.ndarray:
    """Columns 5 onward of ``pd.read_csv(path, header=None, skiprows=1)`` through the native
    parser: the column count is that of the first data line, as read_csv infers it.  Empty echo
    fields read 0 where pandas reads NaN (neither passes a threshold >= 0)."""
    from .ingest import STATUS_EMPTY, STATUS_NON_NUMERIC, STATUS_OK, read_sweeps

    path = Path(path)
    first = None
    with path.open("r", encoding="utf-8") as fh:  # raises FileNotFoundError as read_csv does
        fh.readline()
        for line in fh:
            if line.strip():
                first = line
                break
    if first is None:
        raise ValueError("No columns to parse from file")  # pandas.errors.EmptyDataError
    bins = len(first.rstrip("\r\n").split(",")) - 5
    if bins < 1:  # no echo column at all: df.iloc[:, 5:] is empty
        rows = sum(1 for ln in path.read_text(encoding="utf-8").splitlines()[1:] if ln.strip())
        return np.zeros((rows, 0), np.float32)
    b = read_sweeps([path], bins=bins)
    st = int(b.status[0])
    if st == STATUS_EMPTY:
        raise ValueError("No columns to parse from file")
    if st == STATUS_NON_NUMERIC:
        raise ValueError(b.errors[0] or f"could not convert string to float in {path}")
    if st != STATUS_OK:
        raise ValueError(b.errors[0] or f"Error tokenizing data in {path}")
    echo = b.echo[0, :int(b.rows[0])]
    return echo if echo.dtype == np.float32 else echo.astype(np.float32)


def load_radar_sweep_simple(path: Path) -> tuple[np.ndarray, np.ndarray]:
    """loaders.py:104-122: (angles_rad, intensities) with the rows spread evenly over the circle
    (np.linspace(0, 2 pi, rows, endpoint=False, dtype=float32))."""
    intensities = _simple_sweep_echo(path)
    angles_rad = np.linspace(0.0, 2 * np.pi, len(intensities), endpoint=False, dtype=np.float32)
    return angles_rad, intensities


def load_cartesian_csv(path: Path) -> PointCloud:
    """loaders.py:125-146: a CSV with x, y, z columns (any case; else the first three), pandas as
    the reference."""
    import pandas as pd

    df = pd.read_csv(path)
    by_lower = {c.lower(): c for c in df.columns}
    cols = [by_lower.get(name, df.columns[k]) for k, name in enumerate("xyz")]
    x, y, z = (df[c].to_numpy(np.float32) for c in cols)
    return PointCloud(x=x, y=y, z=z)


def detect_csv_format(path: Path) -> str:
    """loaders.py:223-243: "cartesian" for an x/y/z header or three named columns, else "radar"."""
    import pandas as pd

    preview = pd.read_csv(path, nrows=2)
    names = [c.lower() for c in preview.columns]
    if {"x", "y", "z"}.issubset(names) or (preview.shape[1] == 3 and preview.columns[0] != 0):
        return "cartesian"
    return "radar"


_PLY_HEADER_PREFIX = 1 << 16  # bytes of the file the device path looks for the header in


def _ply_header(raw: bytes):
    """The header loop of the host reader over the prefix ``raw``, line by line in bytes:
    (element vertex count, property names, byte offset of the body), or None when the prefix does
    not hold a header the device path takes (no ``end_header``, a non-ASCII byte, a ``\\r`` that
    is not part of ``\\r\\n``, a count that is no integer): the host reader then decides."""
    n = None
    props = []
    pos = 0
    first = True
    while True:
        nl = raw.find(b"\n", pos)
        if nl < 0:
            return None
        line = raw[pos:nl]
        pos = nl + 1
        if b"\r" in line[:-1]:
            return None  # universal newlines would end a line here
        try:
            s = line.decode("ascii").strip()
        except UnicodeDecodeError:
            return None
        if first and not s.startswith("ply"):
            return None
        first = False
        if s.startswith("element vertex"):
            try:
                n = int(s.split()[-1])
            except ValueError:
                return None
        elif s.startswith("property"):
            props.append(s.split()[-1])
        elif s == "end_header":
            return (n, props, pos) if n is not None else None


def _load_ply_device(path: Path, text):
    """load_ply with the vertex rows parsed on the device: (PointCloud, None), or (None, reason)
    when the file is outside that path's domain."""
    raw = path.read_bytes()
    hdr = _ply_header(raw[:_PLY_HEADER_PREFIX])
    if hdr is None:
        return None, "header"
    n, props, body = hdr
    ix = {p: k for k, p in enumerate(props)}
    rgb = [ix[c] for c in ("red", "green", "blue")] if {"red", "green", "blue"} <= ix.keys() \
        else []
    if not {"x", "y", "z"} <= ix.keys():
        return None, "header"
    cols, reason = text.parse_rows_reason(memoryview(raw)[body:], n)
    if cols is None:
        return None, reason
    if max([ix["x"], ix["y"], ix["z"], *rgb]) >= cols.shape[0]:
        return None, "header"  # a property without a column: the host reader's IndexError
    data = cols.cpu().numpy()
    colors = np.stack([data[k] for k in rgb], axis=1).astype(np.uint8) if rgb else None
    return PointCloud(x=data[ix["x"]], y=data[ix["y"]], z=data[ix["z"]], colors=colors), None


def load_ply(path: Path, device: Optional[bool] = None,
             info: Optional[dict] = None) -> PointCloud:
    """ASCII PLY reader with x/y/z and optional uchar RGB (loaders.py:149-220 /
    3_stdbscan_point_clouds.py:38-79).

    With a GPU the vertex rows are parsed on the device (rpt.core.text.parse_rows): plain decimal
    tokens, every value ``np.float32(float(token))`` bit for bit.  A file outside that domain (an
    exponent, nan, a ragged row, too few lines, non-ASCII bytes, ...), ``device=False`` and a host
    without a GPU take the host reader below, which IS the reference's code: same values, same
    exceptions.  ``info`` (a dict) receives ``parser`` ("device" / "host") and, for "host", the
    ``reason``: no_gpu, forced, header, bytes, lines, rows or size."""
    path = Path(path)
    reason = "forced"
    if device is not False:
        from . import text

        reason = "no_gpu"
        if text.gpu_visible():
            cloud, reason = _load_ply_device(path, text)
            if cloud is not None:
                if info is not None:
                    info["parser"] = "device"
                    info.pop("reason", None)
                return cloud
    if info is not None:
        info["parser"] = "host"
        info["reason"] = reason
    with path.open("r", encoding="utf-8") as fh:
        lines = fh.readlines()
    if not lines or not lines[0].strip().startswith("ply"):
        raise ValueError(f"{path} is not a PLY file")
    n = None
    end = None
    props = []
    for i, line in enumerate(lines):
        s = line.strip()
        if s.startswith("element vertex"):
            n = int(s.split()[-1])
        elif s.startswith("property"):
            props.append(s.split()[-1])
        elif s == "end_header":
            end = i + 1
            break
    if n is None or end is None:
        raise ValueError(f"Could not parse header for {path}")
    rows = lines[end:end + n]
    data = np.fromiter((float(v) for ln in rows for v in ln.split()), dtype=np.float32,
                       count=len(rows[0].split()) * n if n else 0).reshape(n, -1)
    ix = {p: k for k, p in enumerate(props)}
    colors = None
    if {"red", "green", "blue"} <= ix.keys():
        colors = data[:, [ix["red"], ix["green"], ix["blue"]]].astype(np.uint8)
    return PointCloud(x=data[:, ix["x"]], y=data[:, ix["y"]], z=data[:, ix["z"]], colors=colors)
