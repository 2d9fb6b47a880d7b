"""Drop-in for ``radar_pipeline.processors.clustering`` (radar-pipeline/src/radar_pipeline/
processors/clustering.py) and the ``st_dbscan`` of ``PointCloudWork/3_stdbscan_point_clouds.py``.

Same names, argument meaning and error behaviour; the work runs in librpt's HIP kernels:
numpy inputs are copied to the current ROCm device and numpy labels come back, torch inputs
stay on their device and a torch int32 tensor comes back.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from .. import _abi
from .._device import is_torch, ptr, require_gpu, stream_handle, to_device
from ..config import ClusteringConfig, GainConfig


def _times_to_f32(times, eps_time: float):
    """Reduce the reference's time comparison to the float32 form the kernel implements.

    float32 times: exact (NEP 50 makes the reference compare in float32).  Integer times, or
    float64 times that are all integers below 2^24: |dt| is an exact integer in every precision,
    so ``|dt| <= eps`` equals ``|dt| <= floor(eps)``, which float32 represents exactly.
    Returns None where the times have no such form (TypeError for a dtype that is no number).
    """
    if is_torch(times):
        dt = times.dtype
        if dt == torch.float32:
            return times, eps_time
        tt = times.to(torch.float64)
        fin = torch.isfinite(tt)
        integral = bool(torch.all(~fin | ((tt == torch.floor(tt)) & (tt.abs() < 2**24))))
        if not integral:
            return None
        return tt.to(torch.float32), float(np.floor(eps_time)) if np.isfinite(eps_time) else eps_time
    a = np.asarray(times)
    if a.dtype == np.float32:
        return a, eps_time
    if a.dtype.kind in "iub" or a.dtype.kind == "f":
        af = a.astype(np.float64)
        fin = np.isfinite(af)
        if not np.all(~fin | ((af == np.floor(af)) & (np.abs(af) < 2**24))):
            return None
        e = float(np.floor(eps_time)) if np.isfinite(eps_time) else eps_time
        return af.astype(np.float32), e
    raise TypeError(f"unsupported times dtype {a.dtype}")


def _coords_to_f32(coords):
    """The coordinates as float32 where every value round-trips through float32, else None."""
    if is_torch(coords):
        if coords.dtype == torch.float32:
            return coords
        c32 = coords.to(torch.float32)
        if not torch.equal(c32.to(coords.dtype), coords):
            return None
        return c32
    a = np.asarray(coords)
    if a.dtype == np.float32:
        return a
    with np.errstate(invalid="ignore", over="ignore"):  # (beyond float32's range: inf, not equal)
        a32 = a.astype(np.float32)
        same =np.array_equal(a32.astype(a.dtype), a, equal_nan=True)
    if not same:
        return None
    return a32


_TORCH_INT = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8, torch.bool)


def _times_to_f64(times):
    """The float64 kernel's times: (values, time dtype), or NotImplementedError.

    float32 stays float32 (the reference compares in float32 under NEP 50) and float64 stays
    float64.  Integers within +-2^53 become doubles: their differences are exact there, and numpy
    compares an integer difference with a Python float in float64.  Unsigned times stay exact
    integers (the reference's wrap-around is not reproduced).  float16, longdouble and integers
    beyond 2^53 are refused.
    """
    if is_torch(times):
        dt = times.dtype
        if dt == torch.float32:
            return times, "float32"
        if dt == torch.float64:
            return times, "float64"
        if dt in _TORCH_INT:
            lim = 2**53
            if dt == torch.int64 and bool(torch.any((times < -lim) | (times > lim))):
                raise NotImplementedError("rpt st_dbscan: integer times beyond 2^53")
            return times.to(torch.float64), "float64"
        raise NotImplementedError(f"rpt st_dbscan: times of dtype {dt} are not supported")
    a = np.asarray(times)
    if a.dtype == np.float32:
        return a, "float32"
    if a.dtype == np.float64:
        return a, "float64"
    if a.dtype.kind in "iub":
        lim = 2**53
        if a.dtype.kind == "i" and a.dtype.itemsize == 8 and np.any((a < -lim) | (a > lim)):
            raise NotImplementedError("rpt st_dbscan: integer times beyond 2^53")
        if a.dtype.kind == "u" and a.dtype.itemsize == 8 and np.any(a > np.uint64(lim)):
            raise NotImplementedError("rpt st_dbscan: integer times beyond 2^53")
        return a.astype(np.float64), "float64"
    if a.dtype.kind == "f":
        raise NotImplementedError(
            f"rpt st_dbscan: non-float32 times ({a.dtype}) must be float64, or integral below 2^24 "
            "with float32-representable coordinates")
    raise TypeError(f"unsupported times dtype {a.dtype}")


class _Plan(NamedTuple):
    precision: str    # "float32": rpt_stdbscan, "float64": rpt_stdbscan_f64
    coords: object    # array / tensor of that precision
    times: object     # float32, or float64 where time_dtype says so
    time_dtype: str   # "float32" | "float64": the dtype the time test runs in
    eps_time: float


def _plan_inputs(coords, times, eps_time: float) -> _Plan:
    """Which kernel an input takes, and in which form (host logic only: no kernel is called).

    The float32 route is unchanged: coordinates whose values all round-trip through float32, with
    float32 times or integral times below 2^24.  Everything else the reference computes goes to
    the float64 kernel: the coordinates as ``astype(float64)`` (sklearn's check_array makes the
    same cast; widening float32 is exact) and the times by ``_times_to_f64``.
    """
    c32 = _coords_to_f32(coords)
    if c32 is not None:
        t32 = _times_to_f32(times, eps_time)
        if t32 is not None:
            return _Plan("float32", c32, t32[0], "float32", t32[1])
    t, time_dtype = _times_to_f64(times)
    c = coords.to(torch.float64) if is_torch(coords) else np.asarray(coords).astype(np.float64)
    return _Plan("float64", c, t, time_dtype, eps_time)


def st_dbscan(coords, times, eps_space: float, eps_time: float, min_samples: int,
              stats: Optional[dict] = None):
    """Spatio-temporal DBSCAN (clustering.py:49-115; 3_stdbscan_point_clouds.py:101-136).

    coords: (N, 2|3) array/tensor; times: (N,).  float32-representable coordinates with float32
    or small integral times run in the float32 kernels (rpt_stdbscan); other real inputs --
    float64 decimals, large offsets, integer coordinates above 2^24, float64 or epoch times -- in
    the float64 kernel (rpt_stdbscan_f64), see ``_plan_inputs``.  ``stats`` reports which as
    ``precision`` and ``time_dtype``.
    Returns int32 labels, -1 for noise, ids ascending with each cluster's first core point —
    bit-identical to the reference BFS.  Empty input raises ValueError like sklearn's BallTree.
    """
    want_torch = is_torch(coords)
    plan = _plan_inputs(coords, times, float(eps_time))
    c = plan.coords
    f64 = plan.precision == "float64"
    shape = tuple(c.shape)
    if len(shape) != 2:
        raise ValueError(f"Expected 2D array, got {len(shape)}D array instead")
    n, dim = shape
    if n == 0:
        raise ValueError(
            f"Found array with 0 sample(s) (shape=(0, {dim})) while a minimum of 1 is required.")
    if dim not in (2, 3):
        raise NotImplementedError(f"rpt st_dbscan supports 2 or 3 coordinates, got {dim}")
    t, eps_t = plan.times, plan.eps_time
    if (t.shape[0] if is_torch(t) else len(t)) != n:
        raise ValueError("coords and times must have the same length")
    dev = require_gpu(c.device if is_torch(c) else None)
    cd = to_device(c, torch.float64 if f64 else torch.float32, dev)
    td = to_device(t, torch.float64 if plan.time_dtype == "float64" else torch.float32, dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    lib = _abi.load()
    st = _abi.StdbscanStats()
    st.timing = 1 if stats is not None else 0
    base = cd.data_ptr()
    with torch.cuda.device(dev):
        if f64:
            status = lib.rpt_stdbscan_f64(
                base, base + 8, (base + 16) if dim == 3 else None, dim, td.data_ptr(),
                _abi.TIME_F64 if plan.time_dtype == "float64" else _abi.TIME_F32, n,
                float(eps_space), float(eps_t), int(min_samples), labels.data_ptr(), st,
                stream_handle(dev))
        else:
            status = lib.rpt_stdbscan(base, base + 4, (base + 8) if dim == 3 else None, dim,
                                      td.data_ptr(), n, float(eps_space), float(eps_t),
                                      int(min_samples), labels.data_ptr(), st,
                                      stream_handle(dev))
    _abi.check(status, "rpt_stdbscan_f64" if f64 else "rpt_stdbscan")
    if stats is not None:
        stats.update(n_clusters=st.n_clusters, grid_dims=tuple(st.grid_dims),
                     grid_cells=st.grid_cells, ms_bounds=st.ms_bounds, ms_grid=st.ms_grid,
                     ms_core=st.ms_core, ms_union=st.ms_union, ms_label=st.ms_label,
                     precision=plan.precision, time_dtype=plan.time_dtype)
    if want_torch:
        return labels
    return labels.cpu().numpy()


def st_dbscan_soa(x: torch.Tensor, y: torch.Tensor, times: torch.Tensor, eps_space: float,
                  eps_time: float, min_samples: int, z: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, stats: Optional[dict] = None
                  ) -> torch.Tensor:
    """Device-resident form for structure-of-arrays float32 tensors (the tracker's frame stack)."""
    n = x.numel()
    if n == 0:
        raise ValueError("Found array with 0 sample(s) (shape=(0, 2)) while a minimum of 1 is "
                         "required.")
    dev = x.device
    labels = out if out is not None else torch.empty(n, dtype=torch.int32, device=dev)
    st = _abi.StdbscanStats()
    st.timing = 1 if stats is not None else 0
    with torch.cuda.device(dev):  # librpt allocates on the calling thread's current device
        status = _abi.load().rpt_stdbscan(ptr(x), ptr(y), ptr(z), 1, ptr(times), n,
                                          float(eps_space), float(eps_time), int(min_samples),
                                          labels.data_ptr(), st, stream_handle(dev))
    _abi.check(status, "rpt_stdbscan")
    if stats is not None:
        stats.update(n_clusters=st.n_clusters, grid_dims=tuple(st.grid_dims),
                     grid_cells=st.grid_cells, ms_bounds=st.ms_bounds, ms_grid=st.ms_grid,
                     ms_core=st.ms_core, ms_union=st.ms_union, ms_label=st.ms_label)
    return labels


def _f32_device_inputs(coords, times, eps_time: float, what: str):
    """(coords [n, dim] and times [n] as float32 device tensors, eps_time, n, dim, device) of an
    input that ``_plan_inputs`` routes to the float32 kernels; the float64 route is not built for
    ``what`` (NotImplementedError).  Shape errors as ``st_dbscan``."""
    plan = _plan_inputs(coords, times, float(eps_time))
    if plan.precision != "float32":
        raise NotImplementedError(
            f"rpt {what}: inputs that st_dbscan runs in its float64 kernel (coordinates or times "
            "that float32 cannot hold) are not supported; use st_dbscan per min_samples")
    c = plan.coords
    shape = tuple(c.shape)
    if len(shape) != 2:
        raise ValueError(f"Expected 2D array, got {len(shape)}D array instead")
    n, dim = shape
    if n == 0:
        raise ValueError(
            f"Found array with 0 sample(s) (shape=(0, {dim})) while a minimum of 1 is required.")
    if dim not in (2, 3):
        raise NotImplementedError(f"rpt {what} supports 2 or 3 coordinates, got {dim}")
    t = plan.times
    if (t.shape[0] if is_torch(t) else len(t)) != n:
        raise ValueError("coords and times must have the same length")
    dev = require_gpu(c.device if is_torch(c) else None)
    return (to_device(c, torch.float32, dev), to_device(t, torch.float32, dev), plan.eps_time, n,
            dim, dev)


def _counts_call(xyz, t_ptr, n, eps_space, eps_t, dev):
    """rpt_neighbour_counts on device pointers; xyz = (x, y, z or None, stride)."""
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        status = _abi.load().rpt_neighbour_counts(*xyz, t_ptr, n, float(eps_space), float(eps_t),
                                                  counts.data_ptr(), stream_handle(dev))
    _abi.check(status, "rpt_neighbour_counts")
    return counts


def neighbour_counts(coords, times, eps_space: float, eps_time: float):
    """Exact neighbour counts of ``st_dbscan``'s neighbour test, the point itself included: point
    i is core for ``min_samples = m`` exactly when ``counts[i] >= m``.  A point with a non-finite
    time counts 0, and so does every point when an eps is negative or NaN.  int32 ``[n]``; numpy
    in gives numpy out, tensor in a tensor on the same device."""
    want_torch = is_torch(coords)
    cd, td, eps_t, n, dim, dev = _f32_device_inputs(coords, times, eps_time, "neighbour_counts")
    base = cd.data_ptr()
    counts = _counts_call((base, base + 4, (base + 8) if dim == 3 else None, dim), td.data_ptr(),
                          n, eps_space, eps_t, dev)
    return counts if want_torch else counts.cpu().numpy()


def neighbour_counts_soa(x: torch.Tensor, y: torch.Tensor, times: torch.Tensor, eps_space: float,
                         eps_time: float, z: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``neighbour_counts`` for structure-of-arrays float32 device tensors (as st_dbscan_soa)."""
    n = x.numel()
    if n == 0:
        raise ValueError("Found array with 0 sample(s) (shape=(0, 2)) while a minimum of 1 is "
                         "required.")
    return _counts_call((ptr(x), ptr(y), ptr(z), 1), ptr(times), n, eps_space, eps_time, x.device)


_SWEEP_MAX_SETS = 64  # rpt_stdbscan_sweep's n_sets limit


def _sweep_call(xyz, t_ptr, n, eps_space, eps_t, ms, dev, stats):
    """Labels [len(ms), n] on dev: the entries >= 1 from rpt_stdbscan_sweep (64 per call), the
    others from rpt_stdbscan; xyz = (x, y, z or None, stride) device pointers."""
    if not ms:
        raise ValueError("st_dbscan_sweep: min_samples must hold at least one value")
    labels = torch.empty((len(ms), n), dtype=torch.int32, device=dev)
    lib = _abi.load()
    per_set = [None] * len(ms)
    first = None  # the first swept set's stats: the shared stages' times
    swept = [k for k, m in enumerate(ms) if m >= 1]
    with torch.cuda.device(dev):
        for c0 in range(0, len(swept), _SWEEP_MAX_SETS):
            ks = swept[c0:c0 + _SWEEP_MAX_SETS]
            # (rows of their own unless the swept sets are the consecutive rows ks[0] ..)
            direct = ks == list(range(ks[0], ks[0] + len(ks)))
            rows = labels[ks[0]:ks[0] + len(ks)] if direct else \
                torch.empty((len(ks), n), dtype=torch.int32, device=dev)
            st = (_abi.StdbscanStats * len(ks))()
            st[0].timing = 1 if stats is not None else 0
            msk = (_abi.C.c_int32 * len(ks))(*[ms[k] for k in ks])
            status = lib.rpt_stdbscan_sweep(
                *xyz, t_ptr, n, float(eps_space), float(eps_t), msk, len(ks), None,
                rows.data_ptr(), st if stats is not None else None, stream_handle(dev))
            _abi.check(status, "rpt_stdbscan_sweep")
            if not direct:
                labels[torch.as_tensor(ks, device=dev)] = rows
            for j, k in enumerate(ks):
                per_set[k] = st[j]
            first = first if first is not None else st[0]
        for k, m in enumerate(ms):
            if m >= 1:
                continue
            st = _abi.StdbscanStats()
            st.timing = 1 if stats is not None else 0
            status = lib.rpt_stdbscan(*xyz, t_ptr, n, float(eps_space), float(eps_t), m,
                                      labels[k].data_ptr(), st if stats is not None else None,
                                      stream_handle(dev))
            _abi.check(status, "rpt_stdbscan")
            st.n_core = n  # (min_samples <= 0: every point is core, each count >= 0)
            per_set[k] = st
    if stats is not None:
        head = first if first is not None else per_set[0]
        stats.update(min_samples=list(ms), n_core=[int(s.n_core) for s in per_set],
                     n_clusters=[int(s.n_clusters) for s in per_set],
                     n_noise=[int(v) for v in (labels < 0).sum(dim=1).tolist()],
                     grid_dims=tuple(head.grid_dims), grid_cells=head.grid_cells,
                     ms_bounds=head.ms_bounds, ms_grid=head.ms_grid, ms_core=head.ms_core,
                     ms_union=[s.ms_union for s in per_set],
                     ms_label=[s.ms_label for s in per_set])
    return labels


def st_dbscan_sweep(coords, times, eps_space: float, eps_time: float, min_samples,
                    stats: Optional[dict] = None):
    """``st_dbscan`` for every entry of ``min_samples`` (the parameter sweep of
    PointCloudWorkF/run_experiments.py along its min-samples axis): int32 labels
    ``[len(min_samples), n]``, row k bit-identical to ``st_dbscan(..., min_samples[k])``.

    The entries >= 1 share ONE bounds pass, grid build and exact neighbour-count pass
    (rpt_stdbscan_sweep); entries <= 0 (every point core) take the ordinary rpt_stdbscan call.
    ``stats`` receives ``min_samples``, ``n_core``, ``n_clusters``, ``n_noise`` as lists in the
    order given, ``grid_dims`` and the stage times: ``ms_bounds``, ``ms_grid`` and ``ms_core`` (the
    count pass) once, ``ms_union`` / ``ms_label`` as lists.
    """
    want_torch = is_torch(coords)
    ms = [int(m) for m in min_samples]
    cd, td, eps_t, n, dim, dev = _f32_device_inputs(coords, times, eps_time, "st_dbscan_sweep")
    base = cd.data_ptr()
    labels = _sweep_call((base, base + 4, (base + 8) if dim == 3 else None, dim), td.data_ptr(),
                         n, eps_space, eps_t, ms, dev, stats)
    return labels if want_torch else labels.cpu().numpy()


def st_dbscan_sweep_soa(x: torch.Tensor, y: torch.Tensor, times: torch.Tensor, eps_space: float,
                        eps_time: float, min_samples, z: Optional[torch.Tensor] = None,
                        stats: Optional[dict] = None) -> torch.Tensor:
    """``st_dbscan_sweep`` for structure-of-arrays float32 device tensors (as st_dbscan_soa)."""
    n = x.numel()
    if n == 0:
        raise ValueError("Found array with 0 sample(s) (shape=(0, 2)) while a minimum of 1 is "
                         "required.")
    return _sweep_call((ptr(x), ptr(y), ptr(z), 1), ptr(times), n, eps_space, eps_time,
                       [int(m) for m in min_samples], x.device, stats)


def infer_time_from_colors(colors, gain_colors: Optional[Dict[int, Tuple[int, int, int]]] = None):
    """clustering.py:17-46: nearest gain tint (first minimum) -> 0, 1, 2, ... as float32."""
    if gain_colors is None:
        gain_colors = GainConfig().colors
    gains_sorted = sorted(gain_colors.keys())
    palette = np.array([gain_colors[g] for g in gains_sorted], dtype=np.float32).reshape(-1, 3)
    want_torch = is_torch(colors)
    n = int(colors.shape[0])
    if n == 0:
        return colors.new_empty((0,), dtype=torch.float32) if want_torch else \
            np.zeros(0, dtype=np.float32)
    if palette.shape[0] == 0:
        raise ValueError("attempt to get argmin of an empty sequence")
    dev = require_gpu(colors.device if want_torch else None)
    cd = to_device(colors, torch.uint8, dev)
    pd = to_device(palette, torch.float32, dev)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        status = _abi.load().rpt_infer_time_from_colors(cd.data_ptr(), n, pd.data_ptr(),
                                                        palette.shape[0], out.data_ptr(),
                                                        stream_handle(dev))
    _abi.check(status, "rpt_infer_time_from_colors")
    return out if want_torch else out.cpu().numpy()


def cluster_point_cloud(cloud, config: Optional[ClusteringConfig] = None,
                        gain_config: Optional[GainConfig] = None):
    """clustering.py:118-154"""
    if config is None:
        config = ClusteringConfig()
    if gain_config is None:
        gain_config = GainConfig()
    coords = cloud.to_coords()
    times = infer_time_from_colors(cloud.colors, gain_config.colors)
    return st_dbscan(coords, times, eps_space=config.eps_space, eps_time=config.eps_time,
                     min_samples=config.min_samples)


def process_ply_clustering(ply_path: Path, output_dir: Optional[Path] = None,
                           config: Optional[ClusteringConfig] = None,
                           gain_config: Optional[GainConfig] = None):
    """clustering.py:157-208 (PLY load -> subsample -> cluster -> labels CSV)."""
    from ..core.loaders import load_ply
    from ..core.transforms import subsample_cloud
    from ..core.writers import write_labels_csv

    if config is None:
        config = ClusteringConfig()
    if gain_config is None:
        gain_config = GainConfig()
    ply_path = Path(ply_path)
    if output_dir is None:
        output_dir = ply_path.parent
    cloud = load_ply(ply_path)
    cloud, stride = subsample_cloud(cloud, config.max_points)
    print(f"{ply_path.name}: using {cloud.size:,} points (approx stride={stride})")
    labels = cluster_point_cloud(cloud, config, gain_config)
    unique, counts = np.unique(labels, return_counts=True)
    summary = dict(zip(unique.tolist(), counts.tolist()))
    print(f"{ply_path.name}: labels summary {summary}")
    out_stem = f"{ply_path.stem}_dbscan"
    csv_path = Path(output_dir) / f"{out_stem}_labels.csv"
    write_labels_csv(csv_path, cloud.to_coords(), labels)
    print(f"Labels CSV -> {csv_path.name}")
    return csv_path, labels
