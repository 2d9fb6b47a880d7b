#!/usr/bin/env python3
"""Denoise pipeline step [5/5] benchmark: both binary PLYs (denoised_point_cloud.ply by
``labels >= 0``, raw_point_cloud.ply by intensity) from device tensors, the device writer against
the host writer.

    python tools/denoise_ply_bench.py [--points 2000000,20000000] [--runs 3] [--dir DIR]
                                      [--out DIR]

For every size a seeded labelled cloud lives on the device (x, y uniform in +-5000, intensity
uniform in [0, 255), 40 % of the points in 500 clusters, the rest noise) and step 5 is run
  host:   the labels and the three columns copied to the host, the boolean mask and the four
          fancy indexings, write_ply_host twice (matplotlib's colormap over every point, the
          structured array, tofile) -- what run_pipeline did before the device writer;
  device: write_ply twice (signal_only=True / no labels): size pass, record kernel, header and
          body through the pinned staging buffers;
alternately, `--runs` times each after one warm-up of both (code objects, pinned buffers,
matplotlib's tables); the medians are reported and the files compared byte for byte.  Files go to
`--dir` (default: a temporary directory under /dev/shm when there is one, so that no disk is in the
figures).  The device path's stages are also timed alone: the size pass and the record kernel of
both files by device events, the copy of the two bodies to the host and into the files by a host
clock.  `--out DIR` writes table.md and result.json.  Needs a GPU: there is nothing to measure
without one.
"""
from __future__ import annotations

import argparse
import contextlib
import filecmp
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

NAMES = ("denoised_point_cloud.ply", "raw_point_cloud.ply")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", default="2000000,20000000")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", type=Path, default=None, help="where the PLY files are written")
    ap.add_argument("--out", type=Path, default=None, help="directory for table.md, result.json")
    args = ap.parse_args()

    import torch

    from rpt.core import text
    from rpt.denoise import ply_records_device, write_ply, write_ply_host

    if not text.gpu_visible():
        print("denoise_ply_bench: no GPU visible", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    shm = Path("/dev/shm")
    tmp = tempfile.TemporaryDirectory(dir=shm if shm.is_dir() else None) \
        if args.dir is None else None
    work = Path(tmp.name) if tmp else args.dir
    (work / "host").mkdir(parents=True, exist_ok=True)
    (work / "device").mkdir(parents=True, exist_ok=True)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def events(fn):
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    results = []
    for n in [int(v) for v in args.points.split(",") if v]:
        rng = np.random.default_rng(n)
        x, y = (torch.from_numpy(rng.uniform(-5000.0, 5000.0, n).astype(np.float32)).to(dev)
                for _ in range(2))
        z = torch.from_numpy(rng.uniform(0.0, 255.0, n).astype(np.float32)).to(dev)
        lab = rng.integers(0, 500, n).astype(np.int32)
        lab[rng.random(n) >= 0.4] = -1
        lab = torch.from_numpy(lab).to(dev)

        def host_step():
            labels = lab.cpu().numpy()
            m = ~(labels == -1)
            ax, ay, az = x.cpu().numpy(), y.cpu().numpy(), z.cpu().numpy()
            write_ply_host(work / "host" / NAMES[0], ax[m], ay[m], az[m], labels[m])
            write_ply_host(work / "host" / NAMES[1], ax, ay, az)

        writers = []

        def device_step():
            for name, l in zip(NAMES, (lab, None)):
                info = {}
                write_ply(work / "device" / name, x, y, z, l, signal_only=l is not None,
                          info=info)
                writers.append(info["writer"])

        clock(host_step)     # warm-up
        clock(device_step)
        if set(writers) != {"device"}:
            print(f"denoise_ply_bench: the device writer did not run: {writers}", file=sys.stderr)
            return 1
        identical = all(filecmp.cmp(work / "host" / k, work / "device" / k, shallow=False)
                        for k in NAMES)
        nbytes = sum((work / "device" / k).stat().st_size for k in NAMES)
        dev_ms, host_ms = [], []
        for _ in range(args.runs):
            dev_ms.append(clock(device_step)[0])
            host_ms.append(clock(host_step)[0])

        kern_ms, out_ms = [], []
        for _ in range(args.runs):
            t, bodies = events(lambda: [ply_records_device(x, y, z, lab, True),
                                        ply_records_device(x, y, z, None)])
            kern_ms.append(t)

            def to_files():
                for name, body in zip(NAMES, bodies):
                    with open(work / "device" / name, "wb") as fh:
                        text.write_text(fh, body)

            out_ms.append(clock(to_files)[0])
            del bodies
        med = statistics.median
        row = {"points": n, "signal_points": int((lab >= 0).sum()), "bytes": nbytes,
               "host_ms": med(host_ms), "device_ms": med(dev_ms), "kernels_ms": med(kern_ms),
               "d2h_and_file_ms": med(out_ms), "host_all_ms": host_ms, "device_all_ms": dev_ms,
               "identical": identical}
        results.append(row)
        print(f"[denoise_ply_bench] {n} points, {nbytes} bytes in both files: host "
              f"{row['host_ms']:.1f} ms, device {row['device_ms']:.1f} ms (size pass + record "
              f"kernel of both files {row['kernels_ms']:.2f}, D2H + file "
              f"{row['d2h_and_file_ms']:.1f}), identical={identical}", file=sys.stderr, flush=True)
        for sub in ("host", "device"):
            for k in NAMES:
                (work / sub / k).unlink()
        del x, y, z, lab

    result = {"device": torch.cuda.get_device_name(0), "runs": args.runs,
              "files_under": str(work.parent if tmp else work), "sizes": results}
    table = ["| points | bytes (both files) | host ms | device ms | size + record kernels ms | "
             "D2H + file ms |", "|---:|---:|---:|---:|---:|---:|"]
    for r in results:
        table.append(f"| {r['points']} | {r['bytes']} | {r['host_ms']:.1f} | {r['device_ms']:.1f} "
                     f"| {r['kernels_ms']:.2f} | {r['d2h_and_file_ms']:.1f} |")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(result))
    if args.out:
        args.out.mkdir(parents=True, exist_ok=True)
        (args.out / "table.md").write_text("\n".join(table) + "\n")
        (args.out / "result.json").write_text(json.dumps(result, indent=1) + "\n")
    if tmp:
        tmp.cleanup()
    return 0 if all(r["identical"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
