#!/usr/bin/env python3
"""Generate g12_build.npz by RUNNING THE REFERENCE's ``radar-pipeline build`` in the build
container (radar_pipeline/processors/point_cloud.py:178-268 build_stacked_clouds and the click
command cli/main.py:117-161 with --no-plot).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_build_golden.py

Refuses to run unless /root/reference exists; importing this module does not need it: the tests
import the seeded input generators below (``CASES``, ``write_inputs``, ``inputs_digest``) and
regenerate the very same CSV files.

Stored per case c in A..D: ``{c}_offset_ply`` / ``{c}_flat_ply`` (the PLY texts, where the case
builds them), ``{c}_stdout``, ``{c}_digest`` (sha256 of the input files); per sweep row count R
``cos_R`` / ``sin_R`` (the float32 tables of sweep_to_points_simple on the generating host:
numpy's float32 cos/sin are not correctly rounded and may differ between hosts); ``info`` (numpy,
pandas, CPU of the generating run, JSON).

  A  gains 40 / 50 / 75, point_stride 3, caps not reached, both variants; every row of the gain-75
     sweep has an echo in the range-0 bin, so "-0.000000" is printed
  B  max_points_per_gain 100 with point_stride 2 (gain_stride 3 > point_stride), max_points_stack
     60 (stack_stride > 1), a gain-70 file (grey, no offset), stems "Gain-50_a" and "gain75", two
     files of gain 40 (the later path wins, the first position is kept)
  C  a Cartesian CSV with an x,y,z header as gain 50, an all-zero sweep as gain 75 ("gain 75: 0
     points")
  D  the click command with a YAML config (own colours, offsets, range bins, threshold 20) and
     --no-flat
"""
from __future__ import annotations

import hashlib
import io
import json
import platform
import sys
import tempfile
from contextlib import redirect_stdout
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.dont_write_bytecode = True

BINS = 64

YAML_D = """\
gains:
  values: [40, 50, 75]
  colors: {40: [10, 20, 30], 50: [0, 200, 83], 75: [255, 9, 100]}
  z_offsets: {75: 0.0, 50: 12.5, 40: 1000.25}
radar:
  range_bin_width_m: 0.75
  range_start_m: 1.5
processing:
  point_stride: 4
  intensity_threshold: 20.0
"""

# files: (name, kind, rows, gain column); kind "radar" (30 % of the cells non-zero), "radar0"
# (the same with an echo in every range-0 cell), "zero" (all-zero sweep), "xyz" (Cartesian CSV)
CASES = {
    "A": dict(seed=1201, processing=dict(point_stride=3),
              files=[("sweep_gain_40.csv", "radar", 17, 40), ("sweep_gain_50.csv", "radar", 23, 50),
                     ("sweep_gain_75.csv", "radar0", 32, 75)]),
    "B": dict(seed=1202,
              processing=dict(point_stride=2, max_points_per_gain=100, max_points_stack=60),
              files=[("Gain-50_a.csv", "radar", 29, 50), ("a_gain40.csv", "radar", 17, 40),
                     ("gain75.csv", "radar", 32, 75), ("scan_GAIN_70.csv", "radar", 31, 70),
                     ("z_gain_40.csv", "radar", 30, 40), ("notes.csv", "radar", 17, 40)]),
    "C": dict(seed=1203, processing=dict(point_stride=3),
              files=[("sweep_gain_40.csv", "radar", 19, 40), ("sweep_gain_50.csv", "xyz", 150, 50),
                     ("sweep_gain_75.csv", "zero", 21, 75)]),
    "D": dict(seed=1204, yaml=YAML_D,
              files=[("sweep_gain_40.csv", "radar", 20, 40), ("sweep_gain_50.csv", "radar0", 27, 50),
                     ("sweep_gain_75.csv", "radar", 18, 75)]),
}


def _radar_csv(path: Path, rng, rows: int, gain: int, kind: str) -> None:
    echo = np.zeros((rows, BINS), dtype=np.int64)
    if kind != "zero":
        m = rng.random((rows, BINS)) < 0.3
        echo[m] = rng.integers(1, 256, int(m.sum()))
    if kind == "radar0":
        echo[:, 0] = rng.integers(1, 256, rows)
    lines = ["Status,Scale,Range,Gain,Angle," + ",".join(f"Echo_{i}" for i in range(BINS))]
    for r in range(rows):
        lines.append(f"1,{BINS // 2},3,{gain},{r * 8}," + ",".join(str(int(v)) for v in echo[r]))
    path.write_text("\n".join(lines) + "\n")


def _xyz_csv(path: Path, rng, rows: int) -> None:
    pts = rng.uniform(-600.0, 600.0, (rows, 3))
    pts[:4] = [[0.0, -0.0, 1.0], [0.0000004, -0.0000004, 0.0000005], [123.4375, -0.0078125, 255.0],
               [-599.9999995, 0.1, 2.5]]
    lines = ["x,y,z"] + [",".join(repr(float(v)) for v in p) for p in pts]
    path.write_text("\n".join(lines) + "\n")


def write_inputs(case: str, directory: Path) -> dict:
    """The case's input CSVs (and config YAML, case D) written into ``directory`` from its seed;
    returns the case (``processing`` holds the ProcessingConfig overrides)."""
    c = CASES[case]
    directory = Path(directory)
    directory.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(c["seed"])
    for name, kind, rows, gain in c["files"]:
        if kind == "xyz":
            _xyz_csv(directory / name, rng, rows)
        else:
            _radar_csv(directory / name, rng, rows, gain, kind)
    return c


def inputs_digest(directory: Path) -> str:
    h = hashlib.sha256()
    for p in sorted(Path(directory).glob("*.csv")):
        h.update(p.name.encode())
        h.update(p.read_bytes())
    return h.hexdigest()


def sweep_row_counts():
    return sorted({rows for c in CASES.values() for _, kind, rows, _ in c["files"]
                   if kind != "xyz"})


def main() -> None:
    if not REF.exists():
        raise SystemExit("make_build_golden.py must run where /root/reference exists "
                         "(build container)")
    sys.path.insert(0, str(REF / "radar-pipeline" / "src"))
    from click.testing import CliRunner
    from radar_pipeline.cli.main import cli
    from radar_pipeline.config import ProcessingConfig
    from radar_pipeline.processors.point_cloud import build_stacked_clouds

    import pandas

    out = {}
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)
        for case in ("A", "B", "C"):
            c = write_inputs(case, td / case / "in")
            buf = io.StringIO()
            with redirect_stdout(buf):
                paths = build_stacked_clouds(td / case / "in", td / case / "out",
                                             ProcessingConfig(**c["processing"]))
            out[f"{case}_stdout"] = buf.getvalue()
            for key, p in paths.items():
                out[f"{case}_{key}_ply"] = p.read_text()
            out[f"{case}_digest"] = inputs_digest(td / case / "in")
        c = write_inputs("D", td / "D" / "in")
        cfg = td / "D" / "config.yaml"
        cfg.write_text(c["yaml"])
        r = CliRunner().invoke(cli, ["-c", str(cfg), "build", str(td / "D" / "in"),
                                     str(td / "D" / "out"), "--no-flat", "--no-plot"])
        assert r.exit_code == 0, r.output
        out["D_stdout"] = r.output
        out["D_offset_ply"] = (td / "D" / "out" / "frame_stack_v3.ply").read_text()
        assert not (td / "D" / "out" / "frame_stack_flat_v3.ply").exists()
        out["D_digest"] = inputs_digest(td / "D" / "in")

    assert "-0.000000" in out["A_offset_ply"]
    assert "(stride=3)" in out["B_stdout"] and "gain 70:" in out["B_stdout"]
    assert "gain 75: 0 points" in out["C_stdout"]
    for rows in sweep_row_counts():  # transforms.py:117-118 on loaders.py:121's angles
        a = np.linspace(0.0, 2 * np.pi, rows, endpoint=False, dtype=np.float32)
        out[f"cos_{rows}"] = np.cos(a)[:, None].astype(np.float32)[:, 0]
        out[f"sin_{rows}"] = np.sin(a)[:, None].astype(np.float32)[:, 0]
    cpu = ""
    try:
        for line in Path("/proc/cpuinfo").read_text().splitlines():
            if line.startswith("model name"):
                cpu = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    out["info"] = json.dumps({"numpy": np.__version__, "pandas": pandas.__version__,
                              "python": platform.python_version(),
                              "machine": platform.machine(), "cpu": cpu,
                              "generated_by": "tests/golden/make_build_golden.py"})
    np.savez_compressed(OUT / "g12_build.npz", **{k: np.asarray(v) for k, v in out.items()})
    size = (OUT / "g12_build.npz").stat().st_size
    print(f"g12_build.npz: {len(out)} entries, {size} bytes")
    for case in "ABCD":
        print(f"--- {case}\n{out[case + '_stdout']}", end="")
    assert size < 200_000


if __name__ == "__main__":
    main()
