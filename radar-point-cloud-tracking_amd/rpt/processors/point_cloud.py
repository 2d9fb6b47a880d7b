"""Drop-in for ``radar_pipeline.processors.point_cloud`` (radar-pipeline/src/radar_pipeline/
processors/point_cloud.py): gain-specific sweep CSVs -> the stacked, gain-coloured PLYs that
``cluster`` takes.

The points of every gain are made on the device (rpt_sweep_to_points) and stay there: the
per-gain stride, the z offset, the concatenation and the stack stride are torch slicing, the
vertex lines are formed by the device formatter (rpt/core/text.py) and only the finished text
crosses to the host, through a pinned buffer into the file.  The reference's behaviour is kept as
it is, including that the stride is applied twice (inside the loader, then again as gain_stride).
"""
from __future__ import annotations

import re
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .._device import is_torch, require_gpu, to_device
from ..config import GainConfig, ProcessingConfig, RadarConfig
from ..core.loaders import (PointCloud, detect_csv_format, load_cartesian_csv,
                            load_radar_sweep_simple)
from ..core.transforms import apply_stride, gain_to_colors, sweep_to_points_simple
from ..core.writers import write_ply


def find_gain_sweeps(directory: Path) -> Dict[int, Path]:
    """point_cloud.py:21-45: ``*.csv`` in sorted order whose stem holds ``gain[_-]?<digits>`` (any
    case).  A later file of the same gain replaces the path and keeps the first one's position;
    FileNotFoundError when nothing matches."""
    sweeps: Dict[int, Path] = {}
    for path in sorted(Path(directory).glob("*.csv")):
        m = re.search(r"gain[_-]?(\d+)", path.stem, flags=re.IGNORECASE)
        if m:
            sweeps[int(m.group(1))] = path
    if not sweeps:
        raise FileNotFoundError(f"No gain CSVs found in {directory}")
    return sweeps


def gain_stride_for(base_points: int, config: ProcessingConfig) -> int:
    """point_cloud.py:230: the second stride of a gain's points."""
    return max(config.point_stride, int(np.ceil(base_points / config.max_points_per_gain)))


def stack_stride_for(total_points: int, config: ProcessingConfig) -> int:
    """point_cloud.py:247 / :259"""
    return max(1, int(np.ceil(total_points / config.max_points_stack)))


def _load_points(path: Path, config: ProcessingConfig, radar_config: RadarConfig,
                 device: Optional[torch.device]):
    """(x, y, z) of one CSV; device tensors when ``device`` is given, numpy otherwise."""
    if detect_csv_format(path) == "cartesian":
        cloud = load_cartesian_csv(path)
        pts = (cloud.x, cloud.y, cloud.z)
        if device is None:
            return pts
        return tuple(to_device(a, torch.float32, device) for a in pts)
    angles_rad, intensities = load_radar_sweep_simple(path)
    if device is not None:
        intensities = to_device(intensities, torch.float32, device)
    return sweep_to_points_simple(angles_rad, intensities,
                                  range_bin_width=radar_config.range_bin_width_m,
                                  range_start=radar_config.range_start_m,
                                  min_intensity=config.intensity_threshold,
                                  stride=config.point_stride)


def load_points_from_csv(path: Path, config: Optional[ProcessingConfig] = None,
                         radar_config: Optional[RadarConfig] = None
                         ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """point_cloud.py:48-95: a Cartesian CSV as it is, a radar CSV through the uniform-angle
    sweep conversion with ``config.point_stride``."""
    return _load_points(Path(path), config or ProcessingConfig(), radar_config or RadarConfig(),
                        None)


def apply_gain_colors(z, gain: int, gain_config: Optional[GainConfig] = None):
    """point_cloud.py:98-122"""
    if gain_config is None:
        gain_config = GainConfig()
    return gain_to_colors(z, gain, gain_config.colors)


def combine_clouds(clouds: List[Tuple[int, PointCloud]], apply_offsets: bool = False,
                   gain_config: Optional[GainConfig] = None) -> PointCloud:
    """point_cloud.py:125-175: concatenation in list order; with apply_offsets each gain's z
    offset (0.0 for a gain without one) is added in the dtype of z.  Clouds of numpy arrays give
    numpy, clouds of torch tensors stay on their device."""
    if gain_config is None:
        gain_config = GainConfig()
    xs, ys, zs, cs = [], [], [], []
    for gain, cloud in clouds:
        xs.append(cloud.x)
        ys.append(cloud.y)
        zs.append(cloud.z + gain_config.z_offsets.get(gain, 0.0) if apply_offsets else cloud.z)
        cs.append(cloud.colors if cloud.colors is not None
                  else apply_gain_colors(cloud.z, gain, gain_config))
    cat = torch.cat if xs and is_torch(xs[0]) else np.concatenate
    return PointCloud(x=cat(xs), y=cat(ys), z=cat(zs), colors=cat(cs))


def build_stacked_clouds(sweep_dir: Path, output_dir: Path,
                         config: Optional[ProcessingConfig] = None,
                         gain_config: Optional[GainConfig] = None,
                         radar_config: Optional[RadarConfig] = None, generate_flat: bool = True,
                         generate_offset: bool = True, name_prefix: str = "frame_stack"
                         ) -> Dict[str, Path]:
    """point_cloud.py:178-268: ``{prefix}_v3.ply`` (z offsets per gain) and
    ``{prefix}_flat_v3.ply`` from the gain CSVs of ``sweep_dir``; prints the reference's lines."""
    if config is None:
        config = ProcessingConfig()
    if gain_config is None:
        gain_config = GainConfig()
    if radar_config is None:
        radar_config = RadarConfig()
    sweep_dir, output_dir = Path(sweep_dir), Path(output_dir)
    sweep_files = find_gain_sweeps(sweep_dir)
    dev = require_gpu()
    clouds: List[Tuple[int, PointCloud]] = []
    for gain, sweep_path in sweep_files.items():
        x, y, z = _load_points(sweep_path, config, radar_config, dev)
        gain_stride = gain_stride_for(x.numel(), config)
        if gain_stride > 1:
            x, y, z = x[::gain_stride], y[::gain_stride], z[::gain_stride]
        colors = apply_gain_colors(z, gain, gain_config)
        clouds.append((gain, PointCloud(x=x, y=y, z=z, colors=colors)))
        print(f"gain {gain}: {x.numel():,} points (stride={gain_stride})")

    output_dir.mkdir(parents=True, exist_ok=True)
    outputs: Dict[str, Path] = {}
    variants = []
    if generate_offset:
        variants.append(("offset", True, f"{name_prefix}_v3.ply", "Offset stack"))
    if generate_flat:
        variants.append(("flat", False, f"{name_prefix}_flat_v3.ply", "Flat stack"))
    for key, offsets, name, title in variants:
        cloud = combine_clouds(clouds, apply_offsets=offsets, gain_config=gain_config)
        cloud = apply_stride(cloud, stack_stride_for(cloud.size, config))
        path = output_dir / name
        write_ply(path, cloud)
        outputs[key] = path
        print(f"{title}: {cloud.size:,} points -> {path.name}")
    return outputs
