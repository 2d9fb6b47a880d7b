#!/usr/bin/env python3
"""Generate g13_convert.npz by RUNNING THE REFERENCE's ``radar-pipeline convert`` and its helpers
``sort-by-gain`` / ``filter-range`` in the build container (radar_pipeline/processors/
cartesian.py, sorting.py, filtering.py and the click commands cli/main.py:38-114).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_convert_golden.py

Refuses to run unless /root/reference exists; importing this module does not need it: the tests
import the seeded input generators below (``CASES``, ``write_inputs``, ``inputs_digest``,
``angle_columns``) and regenerate the very same CSV files.

Everything runs with the case's directory as the working directory and relative paths, so that the
paths on stdout are the same wherever the case is replayed.

The sweeps have 64 echo columns while ``convert`` always reads with the default RadarConfig (1024
echo columns): read_csv fills the 960 missing columns of every row with NaN, fillna(0) zeroes
them, and the range of bin k is Scale / 1024 * k.  Only the first 64 bins can hold a point, which
keeps the golden small; nothing else depends on it.

Stored per case: ``{case}_digest`` (sha256 of the input files), ``{case}_steps`` (JSON: one
``{"stdout": ..., "files": {relative path: text}}`` per step, ``files`` holding every file below
the case's output directories after the step); per sweep ``cos_{case}_{file}`` / ``sin_...`` (the
float32 tables of polar_to_cartesian on the generating host: numpy's float32 cos/sin are not
correctly rounded and may differ between hosts); ``info`` (numpy, pandas, CPU, JSON).

  S1  one sweep, threshold 0: Angle 0, 2049, 4098 and 6147 first (90 and 180 degrees: cos prints
      as -4.371139e-08, the range-0 bin as -0.0), an echo in every range-0 bin, decimal echoes
  S2  Scale 2**65: every range beyond bin 0 is at least 2**55 > 1e16 (scientific notation)
  S3  threshold 128.5 above part of the samples
  S4  an all-zero sweep: the header alone
  S5  rows with an empty Scale field: NaN x and y (",,37.0" rows; the host formatter in rpt)
  B   convert_batch_aligned over gain_40 / gain_50 / gain_75 with 3 / 2 / 4 files, threshold 20,
      then again with limit=1; then a gain list with an empty folder (FileNotFoundError text)
  C   the click commands on a raw capture directory, with a YAML whose radar section the convert
      command ignores: sort-by-gain --dry-run, sort-by-gain, filter-range --dry-run, filter-range,
      filter-range -r 7 (nothing found), convert --batch --limit 1 -t 10, convert (single) -t 50
"""
from __future__ import annotations

import hashlib
import io
import json
import os
import platform
import sys
import tempfile
from contextlib import contextmanager, redirect_stdout
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.dont_write_bytecode = True

BINS = 64
SCALE_HUGE = 2**65

YAML_C = """\
gains:
  values: [40, 50, 75]
radar:
  num_echo_columns: 64
  angle_scale: 0.5
"""

# files: (relative path, kind, rows, Gain column, Range column)
#   "plain"  15 % of the cells non-zero integers, Angle r * 173 mod 8196
#   "axis"   30 % non-zero, an echo in every range-0 bin, a few decimal echoes, the first four
#            rows on the axes
#   "huge"   plain with Scale 2**65         "zero"  no echo at all
#   "nosc"   plain with every third row's Scale field empty and an echo of 37 in those rows
#   "short"  a first data row of two fields (no Gain column)
#   "text"   a first data row whose Gain and Range fields are not numbers
CASES = {
    "S1": dict(seed=1301, threshold=0.0, files=[("s1.csv", "axis", 23, 40, 3)]),
    "S2": dict(seed=1302, threshold=0.0, files=[("s2.csv", "huge", 17, 50, 3)]),
    "S3": dict(seed=1303, threshold=128.5, files=[("s3.csv", "axis", 32, 75, 3)]),
    "S4": dict(seed=1304, threshold=0.0, files=[("s4.csv", "zero", 19, 40, 3)]),
    "S5": dict(seed=1305, threshold=0.0, files=[("s5.csv", "nosc", 21, 40, 3)]),
    "B": dict(seed=1306, threshold=20.0,
              files=[("in/gain_40/a.csv", "plain", 17, 40, 3), ("in/gain_40/b.csv", "plain", 18, 40, 3),
                     ("in/gain_40/c.csv", "plain", 19, 40, 3), ("in/gain_50/k.csv", "plain", 20, 50, 3),
                     ("in/gain_50/j.csv", "axis", 17, 50, 3), ("in/gain_75/p1.csv", "plain", 17, 75, 3),
                     ("in/gain_75/p2.csv", "plain", 22, 75, 3), ("in/gain_75/p3.csv", "plain", 17, 75, 3),
                     ("in/gain_75/p0.csv", "plain", 18, 75, 3), ("in/gain_60/.keep", "dir", 0, 0, 0)]),
    "C": dict(seed=1307, yaml=YAML_C,
              files=[("raw/cap_001.csv", "plain", 17, 40, 3), ("raw/cap_002.csv", "plain", 18, 50, 3),
                     ("raw/cap_003.csv", "plain", 19, 75, 3), ("raw/cap_004.csv", "plain", 17, 40, 1),
                     ("raw/cap_005.csv", "plain", 17, 50, 2), ("raw/cap_006.csv", "plain", 20, 75, 3),
                     ("raw/cap_007.csv", "plain", 17, 60, 3), ("raw/cap_008.csv", "short", 17, 40, 3),
                     ("raw/cap_009.csv", "text", 17, 40, 3), ("raw/cap_010.csv", "axis", 21, 40, 3)]),
}


def _angles(rows: int, kind: str) -> np.ndarray:
    a = (np.arange(rows) * 173) % 8196
    if kind == "axis":
        a[:4] = [0, 2049, 4098, 6147]
    return a


def _sweep_csv(path: Path, rng, kind: str, rows: int, gain: int, rng_col: int) -> None:
    dens = 0.3 if kind == "axis" else 0.15
    echo = np.zeros((rows, BINS), dtype=np.int64)
    if kind != "zero":
        m = rng.random((rows, BINS)) < dens
        echo[m] = rng.integers(1, 256, int(m.sum()))
    cells = [[str(int(v)) for v in row] for row in echo]
    if kind == "axis":
        for r in range(rows):
            cells[r][0] = str(int(rng.integers(1, 256)))
        for r, k, text in ((1, 5, "0.1"), (2, 6, "65504.5"), (4, 7, "12.25"), (5, 1, "200.125")):
            cells[r][k] = text
    angles = _angles(rows, kind)
    lines = ["Status,Scale,Range,Gain,Angle," + ",".join(f"Echo_{i}" for i in range(BINS))]
    for r in range(rows):
        scale = str(SCALE_HUGE) if kind == "huge" else str(BINS // 2)
        if kind == "nosc" and r % 3 == 1:
            scale = ""
            cells[r][r % BINS] = "37"
        lines.append(f"1,{scale},{rng_col},{gain},{int(angles[r])}," + ",".join(cells[r]))
    if kind == "short":
        lines.insert(1, "1,2")
    if kind == "text":
        lines[1] = "1,32,two,forty," + lines[1].split(",", 4)[4]
    path.write_text("\n".join(lines) + "\n")


def write_inputs(case: str, directory: Path) -> dict:
    """The case's input CSVs (and config YAML, case C) written below ``directory`` from its
    seed; returns the case."""
    c = CASES[case]
    directory = Path(directory)
    rng = np.random.default_rng(c["seed"])
    for rel, kind, rows, gain, rng_col in c["files"]:
        path = directory / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        if kind != "dir":
            _sweep_csv(path, rng, kind, rows, gain, rng_col)
    if "yaml" in c:
        (directory / "config.yaml").write_text(c["yaml"])
    return c


def inputs_digest(case: str, directory: Path) -> str:
    h = hashlib.sha256()
    for rel, kind, *_ in CASES[case]["files"]:
        if kind != "dir":
            h.update(rel.encode())
            h.update((Path(directory) / rel).read_bytes())
    return h.hexdigest()


def angle_columns():
    """{"{case}_{file stem}": the Angle column} of every sweep a convert step reads."""
    return {f"{case}_{Path(rel).stem}": _angles(rows, kind).astype(np.float32)
            for case, c in CASES.items() for rel, kind, rows, *_ in c["files"]
            if kind not in ("dir", "short", "text")}


def tree(*roots) -> dict:
    """{relative path: text} of every file below the given directories / of the given files."""
    files = {}
    for root in roots:
        root = Path(root)
        for p in ([root] if root.is_file() else sorted(root.rglob("*")) if root.exists() else []):
            if p.is_file():
                files[p.as_posix()] = p.read_bytes().decode()
    return files


@contextmanager
def inside(directory: Path):
    old = os.getcwd()
    os.chdir(directory)
    try:
        yield
    finally:
        os.chdir(old)


def c_steps():
    """The argument lists of case C's commands, in order, and what to snapshot after each."""
    cfg = ["-c", "config.yaml"]
    return [
        (cfg + ["sort-by-gain", "raw", "--dry-run"], ["raw"]),
        (cfg + ["sort-by-gain", "raw"], ["raw"]),
        (cfg + ["filter-range", "raw", "--dry-run"], []),
        (cfg + ["filter-range", "raw"], []),
        (cfg + ["filter-range", "raw", "-r", "7"], []),
        (cfg + ["convert", "raw", "out", "--batch", "--limit", "1", "-t", "10"], ["out"]),
        (cfg + ["convert", "raw/gain_40/cap_010.csv", "one/single.csv", "-t", "50"], ["one"]),
    ]


def main() -> None:
    if not REF.exists():
        raise SystemExit("make_convert_golden.py must run where /root/reference exists "
                         "(build container)")
    sys.path.insert(0, str(REF / "radar-pipeline" / "src"))
    from click.testing import CliRunner
    from radar_pipeline.cli.main import cli
    from radar_pipeline.processors.cartesian import convert_batch_aligned, convert_single_csv

    import pandas

    out = {}
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)
        for case in ("S1", "S2", "S3", "S4", "S5"):
            c = write_inputs(case, td / case)
            with inside(td / case):
                src = Path(c["files"][0][0])
                n = convert_single_csv(src, Path("out") / "nested" / f"{src.stem}_xyz.csv",
                                       c["threshold"])
                steps = [dict(stdout="", files=tree("out"), n_points=int(n))]
            out[f"{case}_steps"] = json.dumps(steps)
            out[f"{case}_digest"] = inputs_digest(case, td / case)

        c = write_inputs("B", td / "B")
        steps = []
        with inside(td / "B"):
            for limit, dest in ((None, "out"), (1, "out1")):
                buf = io.StringIO()
                with redirect_stdout(buf):
                    convert_batch_aligned(Path("in"), Path(dest), (40, 50, 75), c["threshold"], limit)
                steps.append(dict(stdout=buf.getvalue(), files=tree(dest)))
            try:
                convert_batch_aligned(Path("in"), Path("out2"), (40, 60), c["threshold"])
                raise AssertionError("an empty gain folder must raise")
            except FileNotFoundError as e:
                steps.append(dict(stdout=str(e), files=tree("out2")))
        out["B_steps"] = json.dumps(steps)
        out["B_digest"] = inputs_digest("B", td / "B")

        write_inputs("C", td / "C")
        out["C_digest"] = inputs_digest("C", td / "C")
        steps = []
        with inside(td / "C"):
            for args, roots in c_steps():
                r = CliRunner().invoke(cli, args)
                assert r.exit_code == 0, (args, r.output, r.exception)
                files = tree(*roots)
                if roots == ["raw"]:  # where the inputs went, not their text again
                    files = {k: "" for k in files}
                steps.append(dict(stdout=r.output, files=files))
        out["C_steps"] = json.dumps(steps)

    s1 = json.loads(out["S1_steps"])[0]["files"]["out/nested/s1_xyz.csv"]
    assert "-0.0," in s1 and "e-08" in s1 and ",65504.5\n" in s1 and ",0.1\n" in s1
    assert "e+16" in json.loads(out["S2_steps"])[0]["files"]["out/nested/s2_xyz.csv"]
    assert json.loads(out["S4_steps"])[0]["files"]["out/nested/s4_xyz.csv"] == "x,y,z\n"
    assert "\n,,37.0\n" in json.loads(out["S5_steps"])[0]["files"]["out/nested/s5_xyz.csv"]
    b = json.loads(out["B_steps"])
    assert len(b[0]["files"]) == 6 and len(b[1]["files"]) == 3 and "No CSVs found" in b[2]["stdout"]
    cs = json.loads(out["C_steps"])
    assert "Would move 7 files total." in cs[0]["stdout"] and "Moved 7 files total." in cs[1]["stdout"]
    assert "Would remove 2 files." in cs[2]["stdout"] and "Removed 2 files." in cs[3]["stdout"]
    assert "Removed 0 files." in cs[4]["stdout"] and len(cs[5]["files"]) == 3

    cfg_scale = 360.0 / 8196.0
    for key, col in angle_columns().items():  # loaders.py:77, transforms.py:32-33
        a = np.deg2rad(col * cfg_scale)
        out[f"cos_{key}"] = np.cos(a[:, None])[:, 0].copy()
        out[f"sin_{key}"] = np.sin(a[:, None])[:, 0].copy()
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
                              "generated_by": "tests/golden/make_convert_golden.py"})
    np.savez_compressed(OUT / "g13_convert.npz", **{k: np.asarray(v) for k, v in out.items()})
    size = (OUT / "g13_convert.npz").stat().st_size
    print(f"g13_convert.npz: {len(out)} entries, {size} bytes")
    for case in ("B", "C"):
        for step in json.loads(out[f"{case}_steps"]):
            print(f"--- {case}\n{step['stdout']}", end="")
    assert size < 200_000


if __name__ == "__main__":
    main()
