#!/usr/bin/env python3
"""Generate g14_gain_fusion.npz by RUNNING THE REFERENCE's gain-fusion PLY builder
(PointCloudWork/5_gain_fusion_ply_builder.py: build_individual_frames, build_stacked_sequence,
build_gain_comparison and the helpers normalize_intensity / intensity_to_rgb) in the build
container, with its two plot functions replaced by no-ops (no PNG is part of the golden).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fusion_golden.py

Refuses to run unless /root/reference exists; importing this module does not need it: the tests
import the seeded input generators below (``CAPTURES``, ``STEPS``, ``write_inputs``,
``inputs_digest``, ``helper_inputs``, ``tree``) and regenerate the very same CSV files.

Every step runs with the capture's directory as the working directory and relative paths, so that
the paths on stdout are the same wherever the step is replayed.

The sweeps have 64 echo columns while the loader names 1024: read_csv fills the 960 missing
columns with NaN, fillna(0) zeroes them, and the range of bin k is Scale / 1024 * k.  Only the
first 64 bins can hold a point, which keeps the golden small; nothing else depends on it.

Stored: ``{capture}_digest`` (sha256 of the input files); ``{capture}_steps`` (JSON: one
``{"name", "stdout", "files"}`` per step, ``files`` mapping every file below the step's output
directory to its text, or to ``{"sha256", "length"}`` when it is longer than ``WHOLE_LIMIT``);
``h{k}_in`` / ``h{k}_z`` / ``h{k}_rgb`` (normalize_intensity and intensity_to_rgb of the vectors of
``helper_inputs``) and ``c{k}_in`` / ``c{k}_rgb`` (intensity_to_rgb alone, at the piece boundaries);
``cos_{file}`` / ``sin_{file}`` (the loader's float32 tables on the generating host: numpy's
float32 cos/sin may differ between hosts); ``info`` (numpy, pandas, CPU, JSON).

Capture "cap" (frames 3 s apart, the gains of a frame 250 ms apart):
  f0  gains 40 / 50 / 70 / 75                 f1  40 / 50 / 75, decimal echoes in gain 50
  f2  40 / 70 / 75 (gain 50 missing)          f3  every sample at or below the threshold (skipped)
  f4  exactly one kept point (gain 40)        f5  one intensity everywhere (p99 <= min: all zero)
  f6  gain 50 unreadable (a row of 1035 fields: read_csv's tokenizing error)
  f7  more rows, Scale 16384
Capture "long": 51 frames of one small gain-40 sweep each (the progress line every 50 frames).
Capture "none": a directory without gain folders.
"""
from __future__ import annotations

import hashlib
import importlib.util
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
SCRIPT = REF / "PointCloudWork" / "5_gain_fusion_ply_builder.py"
OUT = Path(__file__).resolve().parent
sys.dont_write_bytecode = True

BINS = 64
WHOLE_LIMIT = 24 * 1024   # a PLY up to this many bytes is stored whole, else as a digest
ANGLE_SCALE = 360.0 / 8196.0

# frames of "cap": {gain: (kind, rows, Scale)}
#   "plain"  half of the cells non-zero integers 1..255      "low"   non-zero cells 1..5
#   "dec"    plain with a few decimal echoes                 "flat"  non-zero cells all 100
#   "three"  low with three samples above the threshold      "long"  plain plus a 1035-field row
_CAP = [
    {40: ("plain", 24, 4096), 50: ("plain", 24, 4096), 70: ("plain", 20, 4096),
     75: ("plain", 24, 4096)},
    {40: ("plain", 22, 4096), 50: ("dec", 24, 4096), 75: ("plain", 23, 4096)},
    {40: ("plain", 24, 4096), 70: ("plain", 21, 4096), 75: ("plain", 24, 4096)},
    {40: ("low", 20, 4096), 50: ("low", 20, 4096), 75: ("low", 20, 4096)},
    {40: ("three", 20, 4096), 50: ("low", 20, 4096), 75: ("low", 20, 4096)},
    {40: ("flat", 20, 4096), 50: ("flat", 21, 4096), 75: ("flat", 20, 4096)},
    {40: ("plain", 24, 4096), 50: ("long", 24, 4096), 75: ("plain", 24, 4096)},
    {40: ("plain", 40, 16384), 50: ("plain", 37, 16384), 75: ("plain", 40, 16384)},
]
CAPTURES = {
    "cap": dict(seed=1401, frames=_CAP),
    "long": dict(seed=1402, frames=[{40: ("plain", 3, 4096)} for _ in range(51)]),
    "none": dict(seed=1403, frames=[]),
}

# (capture, step name, function, keyword arguments, the CLI's argument list); every path relative
STEPS = [
    ("cap", "ind_abs", "build_individual_frames", dict(data_dir="data", output_dir="o/ind_abs"),
     ["individual", "--data-dir", "data", "--output-dir", "o/ind_abs"]),
    ("cap", "ind_max", "build_individual_frames",
     dict(data_dir="data", output_dir="o/ind_max", mode="max"),
     ["individual", "--data-dir", "data", "--output-dir", "o/ind_max", "--mode", "max"]),
    ("cap", "ind_3", "build_individual_frames",
     dict(data_dir="data", output_dir="o/ind_3", max_frames=3),
     ["individual", "--data-dir", "data", "--output-dir", "o/ind_3", "--max-frames", "3"]),
    ("cap", "st_4", "build_stacked_sequence",
     dict(data_dir="data", output_dir="o/st_4", max_frames=4, time_spacing=2.5),
     ["stacked", "--data-dir", "data", "--output-dir", "o/st_4", "--max-frames", "4",
      "--time-spacing", "2.5"]),
    ("cap", "st_max", "build_stacked_sequence",
     dict(data_dir="data", output_dir="o/st_max", mode="max"),
     ["stacked", "--data-dir", "data", "--output-dir", "o/st_max", "--mode", "max"]),
    ("cap", "cmp_0", "build_gain_comparison", dict(data_dir="data", output_dir="o/cmp_0"),
     ["comparison", "--data-dir", "data", "--output-dir", "o/cmp_0"]),
    ("cap", "cmp_4", "build_gain_comparison",
     dict(data_dir="data", output_dir="o/cmp_4", frame_idx=4),
     ["comparison", "--data-dir", "data", "--output-dir", "o/cmp_4", "--frame", "4"]),
    ("cap", "cmp_6", "build_gain_comparison",
     dict(data_dir="data", output_dir="o/cmp_6", frame_idx=6),
     ["comparison", "--data-dir", "data", "--output-dir", "o/cmp_6", "--frame", "6"]),
    ("cap", "cmp_99", "build_gain_comparison",
     dict(data_dir="data", output_dir="o/cmp_99", frame_idx=99),
     ["comparison", "--data-dir", "data", "--output-dir", "o/cmp_99", "--frame", "99"]),
    ("long", "ind", "build_individual_frames", dict(data_dir="data", output_dir="o/ind"),
     ["individual", "--data-dir", "data", "--output-dir", "o/ind"]),
    ("long", "st", "build_stacked_sequence",
     dict(data_dir="data", output_dir="o/st", max_frames=0),
     ["stacked", "--data-dir", "data", "--output-dir", "o/st", "--max-frames", "0"]),
    ("none", "ind", "build_individual_frames", dict(data_dir="data", output_dir="o/ind"),
     ["individual", "--data-dir", "data", "--output-dir", "o/ind"]),
    ("none", "st", "build_stacked_sequence", dict(data_dir="data", output_dir="o/st"),
     ["stacked", "--data-dir", "data", "--output-dir", "o/st"]),
    ("none", "cmp", "build_gain_comparison", dict(data_dir="data", output_dir="o/cmp"),
     ["comparison", "--data-dir", "data", "--output-dir", "o/cmp"]),
]


def _angles(rows: int) -> np.ndarray:
    return (np.arange(rows) * 173) % 8196


def _stamp(frame: int, slot: int) -> str:
    sec = 2 + 3 * frame   # 14:26:02 onwards, 3 s a frame; the gains 250 ms apart
    return f"20250813_14{26 + sec // 60:02d}{sec % 60:02d}_{181 + 250 * slot:03d}.csv"


def capture_files(capture: str):
    """[(relative path, frame, gain, kind, rows, Scale)] in the order they are written."""
    out = []
    for f, frame in enumerate(CAPTURES[capture]["frames"]):
        for slot, (gain, (kind, rows, scale)) in enumerate(sorted(frame.items())):
            out.append((f"data/gain_{gain}/{_stamp(f, slot)}", f, gain, kind, rows, scale))
    return out


def _sweep_csv(path: Path, rng, kind: str, rows: int, gain: int, scale: int) -> None:
    echo = np.zeros((rows, BINS), dtype=np.int64)
    m = rng.random((rows, BINS)) < 0.5
    if kind in ("low", "three"):
        echo[m] = rng.integers(1, 6, int(m.sum()))
    elif kind == "flat":
        echo[m] = 100
    else:
        echo[m] = rng.integers(1, 256, int(m.sum()))
    cells = [[str(int(v)) for v in row] for row in echo]
    if kind == "three":
        for r, k, text in ((2, 9, "77"), (11, 30, "6"), (17, 3, "255")):
            cells[r][k] = text
    if kind == "dec":
        for r in range(1, rows, 2):   # every echo of the odd rows: the stride keeps some
            for k in range(BINS):
                if echo[r, k]:
                    cells[r][k] = f"{echo[r, k]}.{('25', '5', '75', '125')[k % 4]}"
        for r, k, text in ((1, 5, "0.1"), (2, 6, "200.125"), (4, 7, "12.25"), (5, 1, "6.5"),
                           (9, 40, "5.5"), (13, 63, "254.75")):
            cells[r][k] = text
    angles = _angles(rows)
    lines = ["Status,Scale,Range,Gain,Angle," + ",".join(f"Echo_{i}" for i in range(BINS))]
    for r in range(rows):
        lines.append(f"1,{scale},3,{gain},{int(angles[r])}," + ",".join(cells[r]))
    if kind == "long":
        lines.append(lines[-1] + ",7" * 966)
    path.write_text("\n".join(lines) + "\n")


def write_inputs(capture: str, directory: Path) -> None:
    """The capture's CSV files written below ``directory`` / data from its seed."""
    directory = Path(directory)
    (directory / "data").mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(CAPTURES[capture]["seed"])
    for rel, _, gain, kind, rows, scale in capture_files(capture):
        path = directory / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        _sweep_csv(path, rng, kind, rows, gain, scale)


def inputs_digest(capture: str, directory: Path) -> str:
    h = hashlib.sha256()
    for rel, *_ in capture_files(capture):
        h.update(rel.encode())
        h.update((Path(directory) / rel).read_bytes())
    return h.hexdigest()


def angle_columns():
    """{file key: the Angle column} of every readable sweep of "cap" and "long"."""
    return {f"{cap}_{Path(rel).parent.name}_{Path(rel).stem}": _angles(rows).astype(np.float32)
            for cap in ("cap", "long") for rel, _, _, kind, rows, _ in capture_files(cap)
            if kind != "long"}


def helper_inputs():
    """(vectors for normalize_intensity -> intensity_to_rgb, vectors for intensity_to_rgb alone):
    float32 arrays from a fixed seed."""
    rng = np.random.default_rng(1404)
    f32 = np.float32
    both = [
        rng.integers(6, 256, 1000).astype(f32),               # ties at the rank
        np.array([37.0], f32),                                # n = 1
        np.array([9.0, 200.0], f32),                          # n = 2
        np.full(57, 100.0, f32),                              # p99 <= min
        (rng.random(777) * 250 + 5.5).astype(f32),            # decimals
        rng.integers(6, 256, 101).astype(f32),                # the rank on an integer index
        np.concatenate([rng.integers(6, 40, 400), [255, 255, 255, 254]]).astype(f32),  # clipped
    ]
    edges = np.array([0.0, 63.75, 127.5, 191.25, 255.0], f32)
    near = np.concatenate([edges, np.nextafter(edges, f32(-1)), np.nextafter(edges, f32(300))])
    near = near[(near >= 0) & (near <= 255)]
    alone = [near.astype(f32), (rng.random(3000) * 255).astype(f32),
             np.arange(0, 256, dtype=f32)]
    return both, alone


def tree(root) -> dict:
    """{relative path: text, or {"sha256", "length"} of a longer file} below ``root``."""
    files = {}
    root = Path(root)
    for p in (sorted(root.rglob("*")) if root.exists() else []):
        if p.is_file():
            raw = p.read_bytes()
            files[p.as_posix()] = raw.decode() if len(raw) <= WHOLE_LIMIT else \
                {"sha256": hashlib.sha256(raw).hexdigest(), "length": len(raw)}
    return files


@contextmanager
def inside(directory: Path):
    old = os.getcwd()
    os.chdir(directory)
    try:
        yield
    finally:
        os.chdir(old)


def load_reference():
    spec = importlib.util.spec_from_file_location("gain_fusion_reference", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.plot_point_cloud = lambda *a, **k: None      # no PNG
    mod.plot_3d_point_cloud = lambda *a, **k: None
    return mod


def main() -> None:
    if not REF.exists():
        raise SystemExit("make_fusion_golden.py must run where /root/reference exists "
                         "(build container)")
    import pandas

    ref = load_reference()
    out = {}
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)
        steps = {c: [] for c in CAPTURES}
        for cap in CAPTURES:
            write_inputs(cap, td / cap)
            out[f"{cap}_digest"] = inputs_digest(cap, td / cap)
        for cap, name, fn, kw, _ in STEPS:
            with inside(td / cap):
                buf = io.StringIO()
                args = {k: Path(v) if k.endswith("_dir") else v for k, v in kw.items()}
                with redirect_stdout(buf):
                    getattr(ref, fn)(**args)
                steps[cap].append(dict(name=name, stdout=buf.getvalue(),
                                       files=tree(kw["output_dir"])))
        for cap in CAPTURES:
            out[f"{cap}_steps"] = json.dumps(steps[cap])

        # what the cases are there for
        by = {(c, s["name"]): s for c in CAPTURES for s in steps[c]}
        ind = by["cap", "ind_abs"]
        names = sorted(Path(p).name for p in ind["files"])
        assert "  Found 8 frames" in ind["stdout"], ind["stdout"]
        assert "frame_0000_gains_40_50_70_75.ply" in names       # gain 70 in some frames only
        assert "frame_0002_gains_40_70_75.ply" in names          # a frame missing a gain
        assert "frame_0001_gains_40_50_75.ply" in names
        assert not any(n.startswith("frame_0003") for n in names)  # skipped, index kept
        assert any(n.startswith("frame_0004") for n in names)
        one = ind["files"]["o/ind_abs/frame_0004_gains_40_50_75.ply"]
        assert "element vertex 1\n" in one and one.count("\n") == 11, one
        flat = ind["files"]["o/ind_abs/frame_0005_gains_40_50_75.ply"]
        rows = flat.split("end_header\n")[1].splitlines()
        assert len(rows) > 50 and all(r.endswith(" 0.0000 0 0 255") for r in rows)
        assert ind["stdout"].count("Error loading data/gain_50/") == 1
        assert by["cap", "cmp_6"]["stdout"].count("Error loading data/gain_50/") == 2
        assert "  Gain 50: No points" in by["cap", "cmp_4"]["stdout"]
        assert "Frame 99 not found. Only 8 frames available." in by["cap", "cmp_99"]["stdout"]
        assert "  Processing first 3 frames" in by["cap", "ind_3"]["stdout"]
        assert "temporal_stack_4frames.ply" in "".join(by["cap", "st_4"]["files"])
        assert "  Processed 50/51 frames" in by["long", "ind"]["stdout"]
        assert "  Processed 50/51 frames" in by["long", "st"]["stdout"]
        assert all("No data files found!" in s["stdout"] and not s["files"] for s in steps["none"])
        assert not any(p.endswith(".png") for c in CAPTURES for s in steps[c] for p in s["files"])
        dec = next(rel for rel, f, g, kind, *_ in capture_files("cap") if kind == "dec")
        v = ref.load_radar_csv(td / "cap" / dec)[2]
        assert v.dtype == np.float32 and np.any(v != np.floor(v))

    both, alone = helper_inputs()
    for k, a in enumerate(both):
        z = ref.normalize_intensity(a)
        assert z.dtype == np.float32
        out[f"h{k}_in"], out[f"h{k}_z"], out[f"h{k}_rgb"] = a, z, ref.intensity_to_rgb(z)
    assert not out["h3_z"].any() and (out["h3_rgb"] == (0, 0, 255)).all()
    for k, a in enumerate(alone):
        out[f"c{k}_in"], out[f"c{k}_rgb"] = a, ref.intensity_to_rgb(a)

    for key, col in angle_columns().items():  # load_radar_csv :98, :106-107
        a = np.deg2rad(col * ANGLE_SCALE)
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
                              "generated_by": "tests/golden/make_fusion_golden.py"})
    np.savez_compressed(OUT / "g14_gain_fusion.npz", **{k: np.asarray(v) for k, v in out.items()})
    size = (OUT / "g14_gain_fusion.npz").stat().st_size
    print(f"g14_gain_fusion.npz: {len(out)} entries, {size} bytes")
    for cap in CAPTURES:
        for step in steps[cap]:
            print(f"--- {cap} {step['name']}: {len(step['files'])} files\n{step['stdout']}", end="")
    assert size < 300_000


if __name__ == "__main__":
    main()
