#!/usr/bin/env python3
"""Gain-fusion builder timing: one ``stacked`` run on a synthetic capture, by stage.

    python tools/gain_fusion_bench.py [--frames 20] [--rows 512] [--runs 3] [--out result.json]

Writes a capture of ``--frames`` frames x gains 40 / 50 / 75, each sweep ``--rows`` x 1024 echo
columns (30 % of the cells non-zero, 1..255), then runs
rpt.processors.fusion.build_stacked_sequence on it ``--runs`` times after one warm-up and reports
  wall_s        the whole call (discovery, CSV ingest, K1, fusion colours, text, file)
  load_s        _load_frame: CSV parse + polar scatter, summed over the frames
  heat_s        segment_heat: rpt_segment_percentile99 + rpt_heat_colors, host-timed with a sync
  rows_s        _rows_by_segment: the "%.4f" text pass and its copy to the host
and, on the run's own concatenated arrays, each device entry point alone with device events
(median of 5) on the last group's arrays, next to numpy doing the same post-load work on the
host for those arrays: np.percentile + the normalisation per frame, and np.savetxt of the rows.
Needs a GPU.
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes as C
import io
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "radar-point-cloud-tracking_amd"))


def write_capture(root: Path, frames: int, rows: int) -> None:
    """One seeded sweep per gain; frame f holds it with its rows rotated by f (other angles per
    echo row, the same number of points), which keeps the generation cheap."""
    rng = np.random.default_rng(12)
    head = "Status,Scale,Range,Gain,Angle," + ",".join(f"Echo_{i}" for i in range(1024))
    for slot, gain in enumerate((40, 50, 75)):
        echo = np.where(rng.random((rows, 1024)) < 0.3, rng.integers(1, 256, (rows, 1024)), 0)
        body = [",".join(map(str, r)) for r in echo.tolist()]
        d = root / f"gain_{gain}"
        d.mkdir(parents=True)
        for f in range(frames):
            sec = 3 * f
            name = f"20250813_14{26 + sec // 60:02d}{sec % 60:02d}_{100 + 250 * slot:03d}.csv"
            lines = [f"1,4096,3,{gain},{(r * 8196) // rows}," + body[(r + f) % rows]
                     for r in range(rows)]
            (d / name).write_text(head + "\n" + "\n".join(lines) + "\n")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()

    import torch

    from rpt import _abi
    from rpt.core import text
    from rpt.processors import fusion

    if not text.gpu_visible():
        print("gain_fusion_bench: no GPU visible", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    tmp = tempfile.TemporaryDirectory()
    root = Path(tmp.name)
    t0 = time.perf_counter()
    write_capture(root / "data", args.frames, args.rows)
    gen_s = time.perf_counter() - t0

    spent = {}
    kept = {}

    def wrap(name, keep=False):
        real = getattr(fusion, name)

        def timed(*a, **k):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = real(*a, **k)
            torch.cuda.synchronize()
            spent[name] = spent.get(name, 0.0) + time.perf_counter() - t
            if keep:
                kept[name] = (a, r)
            return r
        setattr(fusion, name, timed)

    wrap("_load_frame")
    wrap("segment_heat", keep=True)
    wrap("_rows_by_segment", keep=True)
    runs = []
    for k in range(args.runs + 1):
        spent.clear()
        torch.cuda.synchronize()
        t = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()) as said:
            fusion.build_stacked_sequence(root / "data", root / f"out{k}", max_frames=0)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t
        if k:  # run 0 warms code objects, pinned buffers and the page cache
            runs.append({"wall_s": wall, "load_s": spent["_load_frame"],
                         "heat_s": spent["segment_heat"], "rows_s": spent["_rows_by_segment"]})
    ply = next((root / "out1").glob("*.ply"))
    n_points = int(said.getvalue().split("Total points: ")[1].split("\n")[0].replace(",", ""))

    # each device entry point alone, on the last group's arrays
    (v, seg_off), _ = kept["segment_heat"]
    (x, y, z, rgb, _), _ = kept["_rows_by_segment"]
    n, S = v.numel(), seg_off.numel() - 1
    lib = _abi.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    mn = torch.empty(S, dtype=torch.float32, device=dev)
    p99 = torch.empty_like(mn)
    zz = torch.empty(n, dtype=torch.float32, device=dev)
    cc = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    total, bad = C.c_int64(0), C.c_int64(0)
    ms = {"percentile99": [], "heat_colors": [], "text_size": [], "text_write": []}
    out = None
    for _ in range(6):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        e[0].record()
        _abi.check(lib.rpt_segment_percentile99(v.data_ptr(), n, seg_off.data_ptr(), S,
                                                mn.data_ptr(), p99.data_ptr(), st))
        e[1].record()
        _abi.check(lib.rpt_heat_colors(v.data_ptr(), n, seg_off.data_ptr(), S, mn.data_ptr(),
                                       p99.data_ptr(), 0, zz.data_ptr(), cc.data_ptr(), st))
        e[2].record()
        _abi.check(lib.rpt_text_rows_size(_abi.TEXT_PLY4, x.data_ptr(), y.data_ptr(),
                                          z.data_ptr(), rgb.data_ptr(), n, off.data_ptr(),
                                          C.byref(total), C.byref(bad), st))
        e[3].record()
        if out is None:
            out = torch.empty(total.value, dtype=torch.uint8, device=dev)
        _abi.check(lib.rpt_text_rows_write(_abi.TEXT_PLY4, x.data_ptr(), y.data_ptr(),
                                           z.data_ptr(), rgb.data_ptr(), n, off.data_ptr(),
                                           out.data_ptr(), out.numel(), st))
        e[4].record()
        torch.cuda.synchronize()
        for k, name in enumerate(ms):
            ms[name].append(e[k].elapsed_time(e[k + 1]))
    kernels = {k: statistics.median(t[1:]) for k, t in ms.items()}

    # numpy on the host, same arrays: the per-frame percentile + normalisation + colours, np.savetxt
    hv, ho = v.cpu().numpy(), seg_off.cpu().numpy()
    hx, hy, hz, hc = x.cpu().numpy(), y.cpu().numpy(), z.cpu().numpy(), rgb.cpu().numpy()
    t = time.perf_counter()
    for a, b in zip(ho[:-1], ho[1:]):
        seg = hv[a:b]
        top, low = np.percentile(seg, 99), seg.min()
        np.clip((seg - low) / (top - low) * 255.0, 0, 255)
    pct_s = time.perf_counter() - t
    t = time.perf_counter()
    with open(root / "host.txt", "w", encoding="utf-8") as fh:
        np.savetxt(fh, np.column_stack([hx, hy, hz, hc[:, 0].astype(int), hc[:, 1].astype(int),
                                        hc[:, 2].astype(int)]), fmt="%.4f %.4f %.4f %d %d %d")
    savetxt_s = time.perf_counter() - t
    same = (root / "host.txt").read_bytes() == ply.read_bytes().split(b"end_header\n")[1] \
        if n == n_points else None

    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    result = {"frames": args.frames, "rows": args.rows, "points": n_points,
              "ply_bytes": ply.stat().st_size, "device": torch.cuda.get_device_name(0),
              "generate_capture_s": gen_s, "runs": runs, "median": med,
              "last_group": {"points": n, "segments": S, "kernel_ms": kernels},
              "host_numpy": {"percentile_normalize_s": pct_s, "savetxt_s": savetxt_s,
                             "savetxt_equals_ply_body": same}}
    line = json.dumps(result)
    print(line)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + "\n")
    tmp.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
