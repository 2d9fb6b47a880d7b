"""Gain fusion of PointCloudWork/5_gain_fusion_ply_builder.py:
fuse_gains_absolute (:193-219, concatenation in ascending gain order) and fuse_gains_max
(:222-273, per-cell maximum intensity on a grid_resolution grid) over one frame's CSV files, with
that script's loader constants (INTENSITY_THRESHOLD 5.0, POINT_STRIDE 8, :57-58).  CSV parse in
librpt's native reader, polar scatter and max-pool on the device (K1 + rpt_fuse_gains_max)."""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Tuple

import numpy as np
import torch

from .. import _abi
from .._device import require_gpu, stream_handle

INTENSITY_THRESHOLD = 5.0   # 5_gain_fusion_ply_builder.py:57
POINT_STRIDE = 8            # :58


def fuse_gains_absolute(frame_files: Dict[int, Path], device=None
                        ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(x, y, intensity float32, gain int32), gains concatenated in ascending order."""
    from ..frames import frame_points

    dev = require_gpu(device)
    x, y, v, g = frame_points(frame_files, INTENSITY_THRESHOLD, POINT_STRIDE, dev)
    if x.numel() == 0:
        return np.array([]), np.array([]), np.array([]), np.array([])
    return x.cpu().numpy(), y.cpu().numpy(), v.cpu().numpy(), g.cpu().numpy()


def fuse_gains_max_points(x: torch.Tensor, y: torch.Tensor, v: torch.Tensor,
                          grid_resolution: float = 1.0):
    """Device form: max-pool float32 points (x, y, intensity > 0) -> (x f64, y f64, max f32)."""
    dev = x.device
    n = x.numel()
    ox = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
    oy = torch.empty_like(ox)
    oi = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    cnt = _abi.C.c_int64(0)
    with torch.cuda.device(dev):
        _abi.check(_abi.load().rpt_fuse_gains_max(
            x.data_ptr(), y.data_ptr(), v.data_ptr(), n, float(grid_resolution), ox.data_ptr(),
            oy.data_ptr(), oi.data_ptr(), _abi.C.byref(cnt), stream_handle(dev)),
            "rpt_fuse_gains_max")
    k = cnt.value
    return ox[:k], oy[:k], oi[:k]


def fuse_gains_max(frame_files: Dict[int, Path], grid_resolution: float = 1.0, device=None
                   ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """:222-273 — (out_x float64, out_y float64, max intensity float32); empty arrays when no
    gain keeps a point."""
    from ..frames import frame_points

    dev = require_gpu(device)
    x, y, v, _ = frame_points(frame_files, INTENSITY_THRESHOLD, POINT_STRIDE, dev)
    if x.numel() == 0:
        return np.array([]), np.array([]), np.array([])
    ox, oy, oi = fuse_gains_max_points(x, y, v, grid_resolution)
    return ox.cpu().numpy(), oy.cpu().numpy(), oi.cpu().numpy()


# ---- the rest of the script: normalisation, colours, PLY files, the three build modes ---------
#
# normalize_intensity (:276-289), intensity_to_rgb (:292-327), gain_to_rgb (:330-338), write_ply /
# write_ply_fast (:345-403), build_individual_frames (:473-532), build_stacked_sequence (:535-610)
# and build_gain_comparison (:613-677).  Frames are handled in GROUPS: their points are
# concatenated on the device until GROUP_POINT_BUDGET is reached, then one
# rpt_segment_percentile99, one rpt_heat_colors and one "%.4f" text pass (RPT_TEXT_PLY4) run over
# the group with the frames as segments, the text comes to the host in one copy and every file
# gets its slice.  The PNG previews (plot_point_cloud / plot_3d_point_cloud) are not rendered.

NORMALIZE_INTENSITY = True    # :62
INTENSITY_PERCENTILE = 99     # :63 (the device kernel implements this value only)
GAIN_COLORS = {               # :45-50
    40: (0, 114, 255),
    50: (0, 200, 83),
    70: (255, 165, 0),
    75: (255, 87, 34),
}


def _group_point_budget() -> int:
    """Points per group: as many "%.4f" rows as always fit ONE pinned staging buffer of
    rpt.core.text (32 MiB / 72 bytes, the longest row: 466 033 points), so that a group's text
    reaches the host in a single copy.  A frame larger than that is a group of its own."""
    from ..core import text

    return text._COPY_CHUNK // text.PLY4_ROW_MAX


GROUP_POINT_BUDGET = None     # None: _group_point_budget(); tests set a small number


def _budget() -> int:
    return int(GROUP_POINT_BUDGET) if GROUP_POINT_BUDGET else _group_point_budget()


def _require_p99() -> None:
    if INTENSITY_PERCENTILE != 99:
        raise NotImplementedError(
            f"INTENSITY_PERCENTILE={INTENSITY_PERCENTILE}: librpt implements the script's value, "
            "the 99th percentile")


def _offsets(sizes) -> np.ndarray:
    off = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(np.asarray(sizes, np.int64), out=off[1:])
    return off


def segment_heat(v: torch.Tensor, seg_off: torch.Tensor):
    """Device form of normalize_intensity + intensity_to_rgb over the segments of one float32
    array: (z float32 [n], rgb uint8 [n][3], min float32 [S], p99 float32 [S])."""
    _require_p99()
    dev = v.device
    n, S = v.numel(), seg_off.numel() - 1
    mn = torch.empty(max(S, 1), dtype=torch.float32, device=dev)
    p99 = torch.empty_like(mn)
    z = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    rgb = torch.empty((max(n, 1), 3), dtype=torch.uint8, device=dev)
    lib = _abi.load()
    with torch.cuda.device(dev):
        st = stream_handle(dev)
        _abi.check(lib.rpt_segment_percentile99(v.data_ptr(), n, seg_off.data_ptr(), S,
                                                mn.data_ptr(), p99.data_ptr(), st),
                   "rpt_segment_percentile99")
        _abi.check(lib.rpt_heat_colors(v.data_ptr(), n, seg_off.data_ptr(), S, mn.data_ptr(),
                                       p99.data_ptr(), 0, z.data_ptr(), rgb.data_ptr(), st),
                   "rpt_heat_colors")
    return z[:n], rgb[:n], mn[:S], p99[:S]


def heat_colors(z: torch.Tensor) -> torch.Tensor:
    """Device form of intensity_to_rgb: rgb uint8 [n][3] of an already normalised float32 z."""
    dev = z.device
    n = z.numel()
    rgb = torch.empty((max(n, 1), 3), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _abi.check(_abi.load().rpt_heat_colors(z.data_ptr(), n, None, 0, None, None, 1, None,
                                               rgb.data_ptr(), stream_handle(dev)),
                   "rpt_heat_colors")
    return rgb[:n]


def _heat_host(v: np.ndarray, colors_only: bool):
    """rpt_heat_host over one segment: (z, rgb)."""
    v = np.ascontiguousarray(v, np.float32)
    n = len(v)
    off = np.array([0, n], np.int64)
    z = np.empty(n, np.float32)
    rgb = np.empty((n, 3), np.uint8)
    _abi.check(_abi.load().rpt_heat_host(v.ctypes.data, n, off.ctypes.data, 1,
                                         int(colors_only), None, None, z.ctypes.data,
                                         rgb.ctypes.data), "rpt_heat_host")
    return z, rgb


def _on_device() -> bool:
    from ..core.text import gpu_visible

    return gpu_visible()


def _heat_numpy(v: np.ndarray, colors_only: bool):
    """(z, rgb) of one float32 numpy array: on the device when one is visible, else through
    rpt_heat_host -- the same per-value code (csrc/heat.h)."""
    if not _on_device():
        return _heat_host(v, colors_only)
    dev = torch.device("cuda", torch.cuda.current_device())
    t = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev)
    if colors_only:
        return v, heat_colors(t).cpu().numpy()
    off = torch.tensor([0, t.numel()], dtype=torch.int64, device=dev)
    z, rgb, _, _ = segment_heat(t, off)
    return z.cpu().numpy(), rgb.cpu().numpy()


def normalize_intensity(intensity: np.ndarray) -> np.ndarray:
    """:276-289 -- intensity scaled so that its minimum is 0 and its 99th percentile 255, clipped
    to 0..255.  float32 arrays (what the loader gives) go through librpt; any other dtype is
    evaluated by numpy in that dtype, as the script does."""
    intensity = np.asarray(intensity)
    if len(intensity) == 0:
        return intensity
    if intensity.dtype == np.float32 and intensity.ndim == 1:
        _require_p99()
        return _heat_numpy(intensity, colors_only=False)[0]
    top, low = np.percentile(intensity, INTENSITY_PERCENTILE), np.min(intensity)
    if top <= low:
        return np.zeros_like(intensity)
    return np.clip((intensity - low) / (top - low) * 255.0, 0, 255)


def intensity_to_rgb(intensity: np.ndarray) -> np.ndarray:
    """:292-327 -- uint8 [n][3] heat colours (blue, cyan, green, yellow, red) of values in 0..255.
    float32 arrays go through librpt; any other dtype is evaluated by numpy in that dtype."""
    intensity = np.asarray(intensity)
    if len(intensity) == 0:
        return np.zeros((0, 3), np.uint8)
    if intensity.dtype == np.float32 and intensity.ndim == 1:
        return _heat_numpy(intensity, colors_only=True)[1]
    u = intensity / 255.0
    piece = np.select([u < 0.25, u < 0.5, u < 0.75, u >= 0.75], [0, 1, 2, 3], default=-1)
    t = (u - 0.25 * np.maximum(piece, 0)) * 4
    up, down = (t * 255).astype(np.uint8), ((1 - t) * 255).astype(np.uint8)
    full, none = np.full(len(u), 255, np.uint8), np.zeros(len(u), np.uint8)
    rgb = np.zeros((len(u), 3), np.uint8)
    for k, (r, g, b) in enumerate(((none, up, full), (none, full, down), (up, full, none),
                                   (full, down, none))):
        m = piece == k
        rgb[m, 0], rgb[m, 1], rgb[m, 2] = r[m], g[m], b[m]
    return rgb


def gain_to_rgb(gains: np.ndarray) -> np.ndarray:
    """:330-338 -- GAIN_COLORS per gain label, black for any other."""
    gains = np.asarray(gains)
    rgb = np.zeros((len(gains), 3), dtype=np.uint8)
    for gain, color in GAIN_COLORS.items():
        rgb[gains == gain] = color
    return rgb


def _ply_header(num_points: int) -> bytes:
    return ("ply\nformat ascii 1.0\n"
            f"element vertex {num_points}\n"
            "property float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            "end_header\n").encode()


def _write_ply_bytes(path: Path, num_points: int, rows) -> None:
    """Header, the vertex rows (bytes-like pieces), and the script's line."""
    with Path(path).open("wb") as fh:
        fh.write(_ply_header(num_points))
        for piece in rows:
            fh.write(piece)
    print(f"  Wrote {num_points:,} points to {Path(path).name}")


def _f32(a):
    if isinstance(a, torch.Tensor):
        return a.to(torch.float32)
    return np.asarray(a).astype(np.float32)


def write_ply_fast(path: Path, x, y, z, colors) -> None:
    """:370-403 -- ASCII PLY with float32 coordinates at four decimals and integer colours (the
    bytes np.savetxt writes); rows formed on the device when one is visible."""
    from ..core.text import format_ply4_rows

    x, y, z = _f32(x), _f32(y), _f32(z)
    _write_ply_bytes(path, len(x), [format_ply4_rows(x, y, z, colors, as_tensor=False)])


# :345-367 writes the same bytes one f-string per point: "{xp:.4f}" of a float32 is "%.4f" of its
# float64 value and "{r}" of a uint8 its "%d"
write_ply = write_ply_fast


class _Group:
    """Frames (or gains of a frame) collected for one set of launches."""

    def __init__(self, dev):
        self.dev = dev
        self.items = []   # (tag, x, y, v) device float32 tensors, non-empty
        self.points = 0

    def add(self, tag, x, y, v) -> None:
        self.items.append((tag, x, y, v))
        self.points += x.numel()

    def heat(self):
        """(x, y, v, z, rgb, offsets numpy int64 [S + 1]) of the concatenated items; z and rgb by
        NORMALIZE_INTENSITY as the script chooses them."""
        off = _offsets([it[1].numel() for it in self.items])
        x = torch.cat([it[1] for it in self.items])
        y = torch.cat([it[2] for it in self.items])
        v = torch.cat([it[3] for it in self.items])
        if NORMALIZE_INTENSITY:
            z, rgb, _, _ = segment_heat(v, torch.from_numpy(off).to(self.dev))
        else:
            z, rgb = v, heat_colors(v)
        return x, y, v, z, rgb, off


def _rows_by_segment(x, y, z, rgb, off):
    """The "%.4f" rows of device arrays cut at the point offsets ``off``: a list of bytes-like
    slices, one per segment.  One text pass and one copy to the host; a coordinate outside the
    kernel's domain sends every segment through the host formatter."""
    from ..core.text import format_ply4_rows_host, ply4_rows_device, text_to_host

    x, y, z, rgb = x.contiguous(), y.contiguous(), z.contiguous(), rgb.contiguous()
    got = ply4_rows_device(x, y, z, rgb)
    if got is None:
        return [format_ply4_rows_host(x[a:b], y[a:b], z[a:b], rgb[a:b])
                for a, b in zip(off[:-1], off[1:])]
    text, row_off = got
    cut = row_off[torch.from_numpy(np.asarray(off, np.int64)).to(row_off.device)].cpu().tolist()
    host = text_to_host(text)
    return [host[a:b] for a, b in zip(cut[:-1], cut[1:])]


def _load_frame(ff: Dict[int, Path], mode: str, dev):
    """One frame's (x, y, intensity) float32 device tensors by fusion mode (max: the float64 cell
    centres cast to float32 on the device, as write_ply_fast's astype does)."""
    from ..frames import frame_points

    x, y, v, _ = frame_points(ff, INTENSITY_THRESHOLD, POINT_STRIDE, dev)
    if mode == "max" and x.numel():
        ox, oy, v = fuse_gains_max_points(x, y, v)
        x, y = ox.to(torch.float32), oy.to(torch.float32)
    return x, y, v


def _discover(data_dir: Path):
    from ..core.discovery import discover_files

    print("Discovering files...")
    files_by_gain = discover_files(Path(data_dir))
    if not files_by_gain:
        print("No data files found!")
    return files_by_gain


def build_individual_frames(data_dir: Path, output_dir: Path, max_frames: int = 0,
                            mode: str = "absolute", device=None) -> None:
    """:473-532 -- one PLY per frame, z the normalised intensity, heat colours."""
    import contextlib
    import io

    from ..core.discovery import group_files_by_frame

    data_dir, output_dir = Path(data_dir), Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    files_by_gain = _discover(data_dir)
    if not files_by_gain:
        return
    for gain, files in files_by_gain.items():
        print(f"  Gain {gain}: {len(files)} files")
    print("\nGrouping into frames...")
    frame_files = group_files_by_frame(files_by_gain)
    print(f"  Found {len(frame_files)} frames")
    if max_frames > 0:
        frame_files = frame_files[:max_frames]
        print(f"  Processing first {len(frame_files)} frames")
    print(f"\nBuilding point clouds (mode={mode})...")
    dev = require_gpu(device)
    total = len(frame_files)

    def flush(group: _Group, notes) -> None:
        # notes: (frame index, the loader's lines for it), empty frames included, in frame order
        pieces = {}
        if group.items:
            x, y, _, z, rgb, off = group.heat()
            rows = _rows_by_segment(x, y, z, rgb, off)
            pieces = {it[0]: (int(off[k + 1] - off[k]), rows[k])
                      for k, it in enumerate(group.items)}
        for i, said in notes:
            print(said, end="")
            if i not in pieces:
                continue
            gain_str = "_".join(str(g) for g in sorted(frame_files[i]))
            n, rows = pieces[i]
            _write_ply_bytes(output_dir / f"frame_{i:04d}_gains_{gain_str}.ply", n, [rows])
            if (i + 1) % 50 == 0:
                print(f"  Processed {i + 1}/{total} frames")

    budget = _budget()
    group, notes = _Group(dev), []
    for i, ff in enumerate(frame_files):
        said = io.StringIO()   # the loader's "Error loading" lines belong in front of this frame
        with contextlib.redirect_stdout(said):
            x, y, v = _load_frame(ff, mode, dev)
        notes.append((i, said.getvalue()))
        if x.numel():
            group.add(i, x, y, v)
        if group.points >= budget:
            flush(group, notes)
            group, notes = _Group(dev), []
    flush(group, notes)
    print(f"\nDone! PLY files saved to {output_dir}")


def build_stacked_sequence(data_dir: Path, output_dir: Path, max_frames: int = 100,
                           time_spacing: float = 10.0, mode: str = "absolute",
                           device=None) -> None:
    """:535-610 -- one PLY of all frames, z = frame index * time_spacing, heat colours of each
    frame's own normalised intensity."""
    from ..core.discovery import group_files_by_frame

    data_dir, output_dir = Path(data_dir), Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    files_by_gain = _discover(data_dir)
    if not files_by_gain:
        return
    print("\nGrouping into frames...")
    frame_files = group_files_by_frame(files_by_gain)
    if max_frames > 0:
        frame_files = frame_files[:max_frames]
    print(f"  Processing {len(frame_files)} frames")
    dev = require_gpu(device)
    body, n_points = [], 0

    def flush(group: _Group) -> None:
        nonlocal n_points
        if not group.items:
            return
        x, y, _, _, rgb, off = group.heat()
        # np.full_like(x, i * time_spacing): the float32 of the float64 product
        layer = torch.cat([torch.full((it[1].numel(),), float(np.float32(it[0] * time_spacing)),
                                      dtype=torch.float32, device=dev) for it in group.items])
        rows = _rows_by_segment(x, y, layer, rgb, np.array([0, int(off[-1])], np.int64))
        body.append(bytes(rows[0]))   # out of the staging buffer: the next group reuses it
        n_points += int(off[-1])

    budget = _budget()
    group = _Group(dev)
    for i, ff in enumerate(frame_files):
        x, y, v = _load_frame(ff, mode, dev)
        if x.numel() == 0:
            continue
        group.add(i, x, y, v)
        if (i + 1) % 50 == 0:
            print(f"  Processed {i + 1}/{len(frame_files)} frames")
        if group.points >= budget:
            flush(group)
            group = _Group(dev)
    flush(group)
    if not body:
        print("No points generated!")
        return
    print(f"\nTotal points: {n_points:,}")
    ply_path = output_dir / f"temporal_stack_{len(frame_files)}frames.ply"
    _write_ply_bytes(ply_path, n_points, body)
    print(f"Done! Stacked PLY saved to {ply_path}")


def build_gain_comparison(data_dir: Path, output_dir: Path, frame_idx: int = 0,
                          device=None) -> None:
    """:613-677 -- one frame: a PLY per gain in that gain's colour, the fused cloud coloured by
    gain and again by intensity.  The gains and the fused cloud are the segments of one group."""
    import contextlib
    import io

    from ..core.discovery import group_files_by_frame
    from ..frames import frame_points

    data_dir, output_dir = Path(data_dir), Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    files_by_gain = _discover(data_dir)
    if not files_by_gain:
        return
    print("\nGrouping into frames...")
    frame_files = group_files_by_frame(files_by_gain)
    if frame_idx >= len(frame_files):
        print(f"Frame {frame_idx} not found. Only {len(frame_files)} frames available.")
        return
    ff = frame_files[frame_idx]
    print(f"\nProcessing frame {frame_idx}...")
    dev = require_gpu(device)

    loaded = []   # (gain, x, y, v, the loader's lines), ascending gain
    for gain, path in sorted(ff.items()):
        said = io.StringIO()
        with contextlib.redirect_stdout(said):
            x, y, v, _ = frame_points({gain: path}, INTENSITY_THRESHOLD, POINT_STRIDE, dev)
        loaded.append((gain, x, y, v, said.getvalue()))
    kept = [(g, x, y, v) for g, x, y, v, _ in loaded if x.numel()]
    group = _Group(dev)
    for g, x, y, v in kept:
        group.add(g, x, y, v)
    rows, sizes = [], []
    if kept:
        # the fused cloud (fuse_gains_absolute: the gains in ascending order) as one more segment
        group.add("fused", torch.cat([k[1] for k in kept]), torch.cat([k[2] for k in kept]),
                  torch.cat([k[3] for k in kept]))
        x, y, _, z, heat_rgb, off = group.heat()
        n_f = int(off[-1] - off[-2])
        solid = [torch.tensor(GAIN_COLORS[g], dtype=torch.uint8, device=dev).expand(xg.numel(), 3)
                 for g, xg, _, _ in kept]
        by_gain = torch.from_numpy(gain_to_rgb(np.concatenate(
            [np.full(xg.numel(), g, np.int32) for g, xg, _, _ in kept]))).to(dev)
        f0 = int(off[-2])
        # rows of: every gain in its colour, the fused cloud by gain, the fused cloud by intensity
        rows_off = np.concatenate([off, [off[-1] + n_f]])
        rows = _rows_by_segment(torch.cat([x, x[f0:]]), torch.cat([y, y[f0:]]),
                                torch.cat([z, z[f0:]]),
                                torch.cat(solid + [by_gain, heat_rgb[f0:]]), rows_off)
        sizes = np.diff(rows_off).tolist()
    slot = {g: k for k, (g, *_rest) in enumerate(kept)}
    for gain, x, _, _, said in loaded:
        print(said, end="")
        if x.numel() == 0:
            print(f"  Gain {gain}: No points")
            continue
        k = slot[gain]
        _write_ply_bytes(output_dir / f"frame_{frame_idx:04d}_gain_{gain}.ply", sizes[k], [rows[k]])
        print(f"  Gain {gain}: {x.numel():,} points")
    for *_head, said in loaded:   # fuse_gains_absolute loads the files once more
        print(said, end="")
    if kept:
        _write_ply_bytes(output_dir / f"frame_{frame_idx:04d}_fused_by_gain.ply", sizes[-2],
                         [rows[-2]])
        _write_ply_bytes(output_dir / f"frame_{frame_idx:04d}_fused_by_intensity.ply", sizes[-1],
                         [rows[-1]])
    print(f"\nDone! Files saved to {output_dir}")
