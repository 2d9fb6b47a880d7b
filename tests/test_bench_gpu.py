"""bench.py as a command: a plain run times the steps and nothing else (the legs that take runs
of their own are null without --full), --steps sets the number of timed steps, and --dump-outputs
writes the last timed step's results as float32 / float64 .npy files that agree with the result
line.  One short run on a 12-frame stack (land filter active)."""
from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def test_plain_run_is_lean_and_dumps_outputs(tmp_path):
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--total-frames", "12", "--lanes", "2",
                        "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["steps"] == 3 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value = points of the timed steps / their time
    pts = d["config"]["points_per_step"]
    assert d["value"] == pytest.approx(pts / d["ms_per_step"] / 1e3, rel=1e-2)
    for leg in ("one_stack_in_flight", "h2d_inclusive", "cpu_baseline", "roofline_c4_share",
                "roofline_configs4_share"):
        assert d[leg] is None, leg
    assert d["stage_ms_from"] == "timed steps"

    files = sorted(dump.glob("*.npy"))
    arrays = {f.stem: np.load(f, allow_pickle=False) for f in files}
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), name
        assert np.isfinite(a).all(), name
    cfg = d["config"]
    n_points, n_clustered, _, n_clusters, n_segments, n_objects = arrays["counts"]
    assert n_points in cfg["points_per_stack"]
    assert (n_clustered, n_clusters, n_segments, n_objects) == (
        cfg["points_clustered_rank0"], cfg["clusters"], cfg["segments"], cfg["objects"])
    assert n_segments > 0 and n_objects > 0
    for k in ("frame", "label", "count", "first", "cx", "cy", "mi"):
        assert arrays[f"seg_{k}"].shape == (int(n_segments),), k
    assert arrays["seg_count"].sum() <= n_clustered
    assert arrays["frame_order"].shape == (int(n_segments),)
    assert arrays["frame_order_offsets"][-1] == n_segments
    assert arrays["objects"].shape == (int(n_objects), 9)
    assert arrays["object_positions"].shape == (int(arrays["objects"][:, 3].sum()), 4)
