#!/usr/bin/env python3
"""st_dbscan benchmark: the float64 kernels (rpt_stdbscan_f64) against the float32 general path
on the same clouds.

    python tools/stdbscan_f64_bench.py [--clouds E2,B3,F3] [--runs 4] [--out DIR]
    python tools/stdbscan_f64_bench.py --one B3      # one float64 run (for a kernel trace)

The clouds are the at-size cases of tests/test_stdbscan_f64_gpu.py (float32 values on a 2^-13
grid): each is run, device-resident, as X + 2^30 in float64 (the float64 kernels; the shift is
exact, so the labels are the same) and as X itself (the float32 kernels), in ABBA order (f64, f32,
f32, f64, ...) after one warm-up of each.  Per run: wall time around the call with a device
synchronisation, and the hipEvent stage times of ``stats`` (bounds, grid, core, union, label).
Medians, the per-stage ratio float64 / float32 and whether the two label arrays are equal go to
stdout as one JSON line; ``--out DIR`` also writes <cloud>.json and table.md there.  Needs a GPU.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "radar-point-cloud-tracking_amd"))
sys.path.insert(0, str(ROOT / "tests"))

STAGES = ("ms_bounds", "ms_grid", "ms_core", "ms_union", "ms_label")

# the generator arguments and (eps, eps_t, min_samples) of tests/test_stdbscan_f64_gpu.py SIZED
CLOUDS = {
    "E2": (dict(seed=21, n=30000, dim=2, extent=(120, 120), n_blobs=40, blob_w=30000,
                t_steps=20 * 1024), (5.0, 2.5, 30)),
    "B3": (dict(seed=22, n=90000, dim=3, extent=(100, 100, 100), n_blobs=40, blob_w=40000,
                t_steps=12, t_quant=1), (5.0, 1.0, 10)),
    "F3": (dict(seed=24, n=1100000, dim=3, extent=(200, 200, 200), n_blobs=600, blob_w=50000,
                t_steps=5, t_quant=1), (2.5, 1.0, 10)),
}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clouds", default="E2,B3,F3")
    ap.add_argument("--runs", type=int, default=4, help="runs per precision (even: ABBA)")
    ap.add_argument("--one", default=None, help="run this cloud once in float64 and exit")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()

    import torch

    from _f64_cases import quantised_cloud
    from rpt.processors import st_dbscan

    if not torch.cuda.is_available():
        print("stdbscan_f64_bench: no GPU visible", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)

    def inputs(name):
        kw, params = CLOUDS[name]
        c, t = quantised_cloud(**kw)
        c32 = torch.from_numpy(c).to(dev)
        c64 = torch.from_numpy(c.astype(np.float64) + 2.0 ** 30).to(dev)
        return c32, c64, torch.from_numpy(t).to(dev), params

    def run(c, t, params):
        stats = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        labels = st_dbscan(c, t, *params, stats=stats)
        torch.cuda.synchronize()
        stats["ms_wall"] = (time.perf_counter() - t0) * 1e3
        return labels, stats

    if args.one:
        _, c64, t, params = inputs(args.one)
        run(c64, t, params)
        _, stats = run(c64, t, params)
        print(json.dumps({"cloud": args.one, **{k: stats[k] for k in STAGES + ("ms_wall",)}}))
        return 0

    results, table = [], [
        "| cloud | points | precision | wall ms | bounds | grid | core | union | label |",
        "|---|---:|---|---:|---:|---:|---:|---:|---:|"]
    for name in [v for v in args.clouds.split(",") if v]:
        c32, c64, t, params = inputs(name)
        lab = {"float64": run(c64, t, params)[0], "float32": run(c32, t, params)[0]}  # warm-up
        runs = {"float64": [], "float32": []}
        for k in range(args.runs):
            for prec in (("float64", "float32") if k % 2 == 0 else ("float32", "float64")):
                _, stats = run(c64 if prec == "float64" else c32, t, params)
                assert stats["precision"] == prec
                runs[prec].append(stats)
        med = {p: {k: statistics.median(s[k] for s in runs[p]) for k in STAGES + ("ms_wall",)}
               for p in runs}
        row = {"cloud": name, "points": int(c32.shape[0]), "dim": int(c32.shape[1]),
               "params": params, "runs": args.runs, "median": med,
               "ratio_f64_over_f32": {k: med["float64"][k] / med["float32"][k]
                                      for k in STAGES + ("ms_wall",) if med["float32"][k] > 0},
               "all": runs, "labels_equal": bool(torch.equal(lab["float64"], lab["float32"])),
               "grid_dims": {p: runs[p][0]["grid_dims"] for p in runs}}
        results.append(row)
        for p in ("float64", "float32"):
            m = med[p]
            table.append(f"| {name} | {row['points']} | {p} | {m['ms_wall']:.3f} | "
                         + " | ".join(f"{m[k]:.3f}" for k in STAGES) + " |")
        if args.out:
            args.out.mkdir(parents=True, exist_ok=True)
            (args.out / f"{name}.json").write_text(json.dumps(row, indent=1) + "\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "clouds": results}))
    if args.out:
        (args.out / "table.md").write_text("\n".join(table) + "\n")
    return 0 if all(r["labels_equal"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
