"""Drop-in for ``radar_pipeline.core.transforms`` (radar-pipeline/src/radar_pipeline/core/
transforms.py) — the polar -> Cartesian members run on the device (K1 kernels of librpt).

``trig_tables`` is the host half of the boundary: the reference evaluates numpy float32
cos/sin per azimuth row (4_temporal_object_tracker.py:203, :217-218); numpy's SIMD float32
cos/sin are not correctly rounded, so the tables are computed here exactly that way (4096 values
per sweep geometry) and handed to the kernels as inputs.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .. import _abi
from .._device import is_torch, require_gpu, stream_handle, to_device
from ..config import ProcessingConfig, RadarConfig
from .loaders import PointCloud, RadarSweep

ANGLE_SCALE = 360.0 / 8196.0


def trig_tables(angle_col, angle_scale: float = ANGLE_SCALE) -> Tuple[np.ndarray, np.ndarray]:
    """float32 cos/sin of deg2rad(float32(Angle) * angle_scale) as the reference evaluates them
    (np.cos(angles_rad[:, None]) over the column)."""
    a = np.deg2rad(np.asarray(angle_col).astype(np.float32) * angle_scale)
    return np.cos(a[:, None])[:, 0].copy(), np.sin(a[:, None])[:, 0].copy()


def polar_to_cartesian(angles_rad, ranges):
    """transforms.py:13-34: x = ranges * cos(angles)[:, None], y = ranges * sin(...)."""
    want_torch = is_torch(ranges)
    a = angles_rad.detach().cpu().numpy() if is_torch(angles_rad) else np.asarray(angles_rad)
    c = np.cos(a[:, None])
    s = np.sin(a[:, None])
    if (not want_torch and (np.asarray(ranges).dtype != np.float32 or c.dtype != np.float32)):
        raise NotImplementedError("rpt polar_to_cartesian: float32 angles and ranges required")
    c = c[:, 0].astype(np.float32)
    s = s[:, 0].astype(np.float32)
    dev = require_gpu(ranges.device if want_torch else None)
    rd = to_device(ranges, torch.float32, dev)
    rows, bins = rd.shape
    x = torch.empty_like(rd)
    y = torch.empty_like(rd)
    cd = to_device(c, torch.float32, dev)
    sd = to_device(s, torch.float32, dev)
    st = _abi.load().rpt_polar_to_cartesian(cd.data_ptr(), sd.data_ptr(), rd.data_ptr(), rows,
                                            bins, x.data_ptr(), y.data_ptr(), stream_handle(dev))
    _abi.check(st, "rpt_polar_to_cartesian")
    if want_torch:
        return x, y
    return x.cpu().numpy(), y.cpu().numpy()


def sweep_points_device(sweep: RadarSweep, threshold: float, stride: int = 1):
    """The thresholded points of a loaded sweep as device tensors (x, y, z): strict ``>`` against
    the threshold cast to float32, row-major order, every stride-th kept cell
    (rpt_sweep_to_points)."""
    a = np.asarray(sweep.angles_rad)
    c = np.cos(a[:, None])[:, 0]
    s = np.sin(a[:, None])[:, 0]
    inten = np.asarray(sweep.intensities)
    ranges = np.asarray(sweep.ranges)
    if inten.dtype != np.float32 or ranges.dtype != np.float32 or c.dtype != np.float32:
        raise NotImplementedError("rpt sweep_to_point_cloud: float32 sweep arrays required")
    rows, bins = inten.shape
    dev = require_gpu()
    idev = to_device(inten, torch.float32, dev)
    rdev = to_device(np.broadcast_to(ranges, inten.shape), torch.float32, dev)
    cd = to_device(c.astype(np.float32), torch.float32, dev)
    sd = to_device(s.astype(np.float32), torch.float32, dev)
    stride = max(int(stride), 1)
    cap = rows * bins // stride + 1
    x = torch.empty(cap, dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    z = torch.empty_like(x)
    nout = _abi.C.c_int64(0)
    with torch.cuda.device(dev):
        st = _abi.load().rpt_sweep_to_points(idev.data_ptr(), rdev.data_ptr(), cd.data_ptr(),
                                             sd.data_ptr(), rows, bins,
                                             float(np.float32(threshold)), stride,
                                             x.data_ptr(), y.data_ptr(), z.data_ptr(), cap,
                                             _abi.C.byref(nout), stream_handle(dev))
    _abi.check(st, "rpt_sweep_to_points")
    k = int(nout.value)
    return x[:k], y[:k], z[:k]


def sweep_to_point_cloud(sweep: RadarSweep, config: Optional[ProcessingConfig] = None,
                         radar_config: Optional[RadarConfig] = None) -> PointCloud:
    """transforms.py:37-79: threshold (strict >) + row-major flatten + stride, on the device."""
    if config is None:
        config = ProcessingConfig()
    if radar_config is None:
        radar_config = RadarConfig()
    x, y, z = sweep_points_device(sweep, config.intensity_threshold, config.point_stride)
    return PointCloud(x=x.cpu().numpy(), y=y.cpu().numpy(), z=z.cpu().numpy())


def simple_trig_tables(angles_rad) -> Tuple[np.ndarray, np.ndarray]:
    """float32 cos/sin per row as sweep_to_points_simple evaluates them (transforms.py:117-118):
    np.cos / np.sin over the 1-D array itself (numpy's contiguous float32 loop -- not the strided
    column form of ``trig_tables``), then astype(float32).  Host values handed to the kernel."""
    a = angles_rad.detach().cpu().numpy() if is_torch(angles_rad) else np.asarray(angles_rad)
    return np.cos(a).astype(np.float32), np.sin(a).astype(np.float32)


def sweep_to_points_simple(angles_rad, intensities, range_bin_width: float = 0.5,
                           range_start: float = 0.0, min_intensity: float = 0.0,
                           stride: int = 1):
    """transforms.py:82-132: uniform range bins, x = range * cos, y = range * sin, z = intensity
    for intensity > min_intensity (strict, compared in float32), every stride-th kept cell in
    row-major order -- on the device (rpt_sweep_to_points).  numpy intensities give numpy
    (x, y, z); a torch tensor gives tensors that stay on the device."""
    want_torch = is_torch(intensities)
    inten = intensities if want_torch else np.asarray(intensities)
    if inten.dtype != (torch.float32 if want_torch else np.float32) or inten.ndim != 2:
        raise NotImplementedError("rpt sweep_to_points_simple: a 2-D float32 sweep required")
    rows, bins = (int(v) for v in inten.shape)
    ranges = range_start + np.arange(bins, dtype=np.float32) * range_bin_width
    if ranges.dtype != np.float32:
        raise NotImplementedError("rpt sweep_to_points_simple: float32 range bins required")
    c, s = simple_trig_tables(angles_rad)
    if c.shape != (rows,):
        raise ValueError(f"{c.shape[0] if c.ndim == 1 else c.shape} angles for {rows} sweep rows")
    dev = require_gpu(inten.device if want_torch and inten.is_cuda else None)
    stride = max(int(stride), 1)
    cap = rows * bins // stride + 1
    x = torch.empty(cap, dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    z = torch.empty_like(x)
    k = 0
    if rows and bins:
        idev = to_device(inten, torch.float32, dev)
        rdev = to_device(np.broadcast_to(ranges, (rows, bins)), torch.float32, dev)
        cd = to_device(c, torch.float32, dev)
        sd = to_device(s, torch.float32, dev)
        nout = _abi.C.c_int64(0)
        with torch.cuda.device(dev):
            st = _abi.load().rpt_sweep_to_points(idev.data_ptr(), rdev.data_ptr(), cd.data_ptr(),
                                                 sd.data_ptr(), rows, bins,
                                                 float(np.float32(min_intensity)), stride,
                                                 x.data_ptr(), y.data_ptr(), z.data_ptr(), cap,
                                                 _abi.C.byref(nout), stream_handle(dev))
        _abi.check(st, "rpt_sweep_to_points")
        k = int(nout.value)
    if want_torch:
        return x[:k], y[:k], z[:k]
    return x[:k].cpu().numpy(), y[:k].cpu().numpy(), z[:k].cpu().numpy()


def subsample_cloud(cloud: PointCloud, max_points: int) -> Tuple[PointCloud, int]:
    """transforms.py:135-167 (host; unseeded random choice only above max_points)."""
    n = cloud.size
    if n <= max_points:
        return cloud, 1
    idx = np.random.choice(n, max_points, replace=False)
    stride = int(np.ceil(n / max_points))
    new_colors = cloud.colors[idx] if cloud.colors is not None else None
    return PointCloud(x=cloud.x[idx], y=cloud.y[idx], z=cloud.z[idx], colors=new_colors), stride


def apply_stride(cloud: PointCloud, stride: int) -> PointCloud:
    """transforms.py:170-198"""
    if stride <= 1:
        return cloud
    new_colors = cloud.colors[::stride] if cloud.colors is not None else None
    return PointCloud(x=cloud.x[::stride], y=cloud.y[::stride], z=cloud.z[::stride],
                      colors=new_colors)


def apply_z_offset(cloud: PointCloud, offset: float) -> PointCloud:
    """transforms.py:201-222: z + offset in the dtype of z (float32 + Python float = float32)."""
    return PointCloud(x=cloud.x, y=cloud.y, z=cloud.z + offset, colors=cloud.colors)


def intensity_to_colors(values: np.ndarray) -> np.ndarray:
    """transforms.py:225-240: grey RGB from intensities clipped to 0..255 (host)."""
    v = values.detach().cpu().numpy() if is_torch(values) else np.asarray(values)
    clipped = np.clip(v, 0, 255).astype(np.uint8)
    return np.stack([clipped, clipped, clipped], axis=1)


def gain_to_colors(values, gain: int, gain_colors: dict):
    """transforms.py:243-262: one constant RGB row per value, (180, 180, 180) for a gain without
    a colour.  A torch ``values`` gives a uint8 tensor on its device."""
    rgb = np.array(gain_colors.get(gain, (180, 180, 180)), dtype=np.uint8)
    if is_torch(values):
        return torch.from_numpy(rgb).to(values.device).repeat(values.numel(), 1)
    return np.repeat(rgb[None, :], np.asarray(values).size, axis=0)
