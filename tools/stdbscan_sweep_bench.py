#!/usr/bin/env python3
"""min_samples sweep benchmark: one rpt_stdbscan_sweep against the rpt_stdbscan calls it replaces.

    python tools/stdbscan_sweep_bench.py [--clouds D,F,stack1000] [--runs 6] [--out DIR]
    python tools/stdbscan_sweep_bench.py --one D     # one sweep (for a kernel trace)

Device-resident structure-of-arrays clouds of a size a user would run: the at-size generators of
tests/test_stdbscan_general_gpu.py cases D (2-D, 182 k points, eps_t = 5) and F (3-D, 1.39 M
points), restated here, and the clustered points of one 1000-frame stack from rpt.synth (the
stack driver's K1 output, times = frame slot, the path's eps 8 / eps_t 2).  A = one
st_dbscan_sweep_soa over min_samples (5, 10, 15, 25); B = the four st_dbscan_soa calls.  Order
ABBA after one warm-up of each, wall time around each window with a device synchronisation inside
it; a second pass of one A and one B with ``stats`` gives the hipEvent stage times (with stats
both sides read a cluster count back per set, so those runs are not in the wall medians).  The
medians, min / max of the repeated identical runs (their spread), the ratio B / A and whether all
label rows are equal go to stdout as one JSON line; ``--out DIR`` also writes <cloud>.json and
table.md.  Needs a GPU.
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

SWEEP = (5, 10, 15, 25)
STAGES = ("ms_bounds", "ms_grid", "ms_core", "ms_union", "ms_label")


def vol(seed, n_blobs, per, noise, box, F, dim, spread=2.0, vel=1.0):
    """Moving Gaussian blobs plus uniform clutter, F frames, time = frame (the generator of
    tests/test_stdbscan_general_gpu.py, without its time jitter)."""
    rng = np.random.default_rng(seed)
    centres = rng.random((n_blobs, dim)) * box - box / 2
    vels = rng.normal(0, vel, (n_blobs, dim))
    pts, ts = [], []
    for f in range(F):
        for c, v in zip(centres, vels):
            m = int(rng.integers(per // 2, per * 2))
            pts.append(c + v * f + rng.normal(0, spread, (m, dim)))
            ts.append(np.full(m, f, np.float64))
        pts.append(rng.random((noise, dim)) * box * 1.2 - box * 0.6)
        ts.append(np.full(noise, f, np.float64))
    return np.vstack(pts).astype(np.float32), np.concatenate(ts).astype(np.float32)


def stack_cloud(dev, n_frames):
    """The clustered points of one synthetic stack: x, y, frame slot as float32, on the device."""
    import torch

    from rpt.pipeline import FrameStackPipeline, PathParams
    from rpt.synth import DeviceSynth, SynthConfig

    cfg = SynthConfig(n_frames=n_frames)
    ds = DeviceSynth(cfg, dev)
    pp = PathParams()
    pipe = FrameStackPipeline(cfg.gains, cfg.rows, cfg.bins, pp, dev)
    pipe.set_geometry(np.full(cfg.rows, cfg.scale, np.float32), ds.geo.cos_t, ds.geo.sin_t,
                      cfg.n_frames * len(cfg.gains))
    res = pipe.run(ds.echo(), keep_points=True)
    torch.cuda.synchronize()
    p = res.points
    return (p["x"].clone(), p["y"].clone(), None, p["frame"].to(torch.float32),
            (float(pp.eps_space), float(pp.eps_time)))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clouds", default="D,F,stack1000")
    ap.add_argument("--runs", type=int, default=6, help="timed windows per side (even: ABBA)")
    ap.add_argument("--one", default=None, help="run one sweep of this cloud and exit")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()

    import torch

    from rpt.processors.clustering import st_dbscan_soa, st_dbscan_sweep_soa

    if not torch.cuda.is_available():
        print("stdbscan_sweep_bench: no GPU visible", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)

    def inputs(name):
        if name.startswith("stack"):
            return stack_cloud(dev, int(name[5:] or 1000))
        c, t, eps = {
            "D": lambda: (*vol(14, 30, 100, 800, 300.0, 40, dim=2), (6.0, 5.0)),
            "F": lambda: (*vol(16, 400, 700, 2000, 200.0, 4, dim=3, spread=1.5, vel=0.5),
                          (5.0, 1.0)),
        }[name]()
        cd = torch.from_numpy(c).to(dev)
        cols = [cd[:, k].contiguous() for k in range(c.shape[1])]
        return cols[0], cols[1], cols[2] if len(cols) == 3 else None, \
            torch.from_numpy(t).to(dev), eps

    def side_a(x, y, z, t, eps, stats=None):  # the sweep
        return st_dbscan_sweep_soa(x, y, t, eps[0], eps[1], SWEEP, z=z, stats=stats)

    def side_b(x, y, z, t, eps, stats=None):  # the calls it replaces
        out = torch.empty((len(SWEEP), x.numel()), dtype=torch.int32, device=dev)
        per = []
        for k, m in enumerate(SWEEP):
            s = {} if stats is not None else None
            st_dbscan_soa(x, y, t, eps[0], eps[1], m, z=z, out=out[k], stats=s)
            per.append(s)
        if stats is not None:
            stats.update({k: [s[k] for s in per] for k in STAGES})
        return out

    def timed(fn, *a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*a)
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    if args.one:
        a = inputs(args.one)
        timed(side_a, *a)
        _, ms = timed(side_a, *a)
        print(json.dumps({"cloud": args.one, "ms_wall_sweep": ms}))
        return 0

    results, table = [], [
        "| cloud | points | sweep ms (min - max) | 4 calls ms (min - max) | calls / sweep | "
        "rows equal |", "|---|---:|---:|---:|---:|---|"]
    for name in [v for v in args.clouds.split(",") if v]:
        a = inputs(name)
        la, lb = timed(side_a, *a)[0], timed(side_b, *a)[0]  # warm-up
        equal = bool(torch.equal(la, lb))
        wall = {"sweep": [], "calls": []}
        for k in range(args.runs):
            for side in (("sweep", "calls") if k % 2 == 0 else ("calls", "sweep")):
                wall[side].append(timed(side_a if side == "sweep" else side_b, *a)[1])
        sa, sb = {}, {}
        side_a(*a, stats=sa)
        side_b(*a, stats=sb)
        torch.cuda.synchronize()
        med = {s: statistics.median(v) for s, v in wall.items()}
        row = {"cloud": name, "points": int(a[0].numel()), "dim": 3 if a[2] is not None else 2,
               "eps": a[4], "min_samples": SWEEP, "runs": args.runs, "wall_ms": wall,
               "median_ms": med, "calls_over_sweep": med["calls"] / med["sweep"],
               "rows_equal": equal,
               "stages_sweep": {k: sa[k] for k in STAGES}, "stages_calls": sb,
               "n_core": sa["n_core"], "n_clusters": sa["n_clusters"],
               "grid_dims": list(sa["grid_dims"])}
        results.append(row)
        table.append(
            f"| {name} | {row['points']} | {med['sweep']:.3f} ({min(wall['sweep']):.3f} - "
            f"{max(wall['sweep']):.3f}) | {med['calls']:.3f} ({min(wall['calls']):.3f} - "
            f"{max(wall['calls']):.3f}) | {row['calls_over_sweep']:.2f} | {equal} |")
        if args.out:
            args.out.mkdir(parents=True, exist_ok=True)
            (args.out / f"{name}.json").write_text(json.dumps(row, indent=1) + "\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "clouds": results}))
    if args.out:
        (args.out / "table.md").write_text("\n".join(table) + "\n")
    return 0 if all(r["rows_equal"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
