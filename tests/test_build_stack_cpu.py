"""Host half of ``radar-pipeline build``: file discovery, CSV format detection, the stride
arithmetic, the host text formatter against the reference's PLY texts (g12_build.npz) and
np.savetxt, the CLI surface, and the seeded inputs of the golden file.  No GPU."""
from __future__ import annotations

import io
import sys
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))


def test_find_gain_sweeps_order_duplicates_and_error(tmp_path):
    from rpt.processors.point_cloud import find_gain_sweeps

    names = ["Gain-50_a.csv", "a_gain40.csv", "gain75.csv", "scan_GAIN_70.csv", "z_gain_40.csv",
             "notes.csv", "gain_12.txt", "regain9x.csv"]
    for n in names:
        (tmp_path / n).write_text("x\n")
    got = find_gain_sweeps(tmp_path)
    # sorted by file name (upper case first); the second gain-40 file replaces the path and keeps
    # the first one's place; the pattern is searched anywhere in the stem, any case
    assert list(got) == [50, 40, 75, 9, 70]
    assert got[40].name == "z_gain_40.csv" and got[9].name == "regain9x.csv"
    assert got[50].name == "Gain-50_a.csv" and got[70].name == "scan_GAIN_70.csv"
    empty = tmp_path / "none"
    empty.mkdir()
    (empty / "sweep.csv").write_text("x\n")
    with pytest.raises(FileNotFoundError, match="No gain CSVs found in"):
        find_gain_sweeps(empty)


def test_detect_csv_format_and_cartesian_loader(tmp_path):
    from make_build_golden import write_inputs

    from rpt.core.loaders import detect_csv_format, load_cartesian_csv

    write_inputs("C", tmp_path)
    assert detect_csv_format(tmp_path / "sweep_gain_40.csv") == "radar"
    assert detect_csv_format(tmp_path / "sweep_gain_50.csv") == "cartesian"
    cloud = load_cartesian_csv(tmp_path / "sweep_gain_50.csv")
    assert cloud.size == 150 and cloud.colors is None
    assert cloud.x.dtype == cloud.y.dtype == cloud.z.dtype == np.float32
    np.testing.assert_array_equal(cloud.x[:4], np.float32([0.0, 0.0000004, 123.4375,
                                                           -599.9999995]))
    assert np.signbit(cloud.y[0]) and cloud.z[3] == np.float32(2.5)
    # upper-case header in another order; three unnamed-but-headed columns
    (tmp_path / "up.csv").write_text("Z,Y,X\n1,2,3\n4,5,6\n")
    assert detect_csv_format(tmp_path / "up.csv") == "cartesian"
    c = load_cartesian_csv(tmp_path / "up.csv")
    assert c.x.tolist() == [3.0, 6.0] and c.z.tolist() == [1.0, 4.0]
    (tmp_path / "abc.csv").write_text("a,b,c\n1,2,3\n")
    assert detect_csv_format(tmp_path / "abc.csv") == "cartesian"
    c = load_cartesian_csv(tmp_path / "abc.csv")
    assert (c.x.tolist(), c.y.tolist(), c.z.tolist()) == ([1.0], [2.0], [3.0])


def test_simple_sweep_loader_reads_the_first_lines_width(tmp_path):
    from make_build_golden import BINS, write_inputs

    from rpt.core.loaders import load_radar_sweep_simple

    write_inputs("A", tmp_path)
    angles, echo = load_radar_sweep_simple(tmp_path / "sweep_gain_75.csv")
    assert echo.shape == (32, BINS) and echo.dtype == np.float32 and angles.dtype == np.float32
    np.testing.assert_array_equal(
        angles, np.linspace(0.0, 2 * np.pi, 32, endpoint=False, dtype=np.float32))
    import pandas as pd

    ref = pd.read_csv(tmp_path / "sweep_gain_75.csv", header=None, skiprows=1)
    np.testing.assert_array_equal(echo, ref.iloc[:, 5:].to_numpy(dtype=np.float32))
    assert (echo[:, 0] > 0).all()


def test_stride_arithmetic():
    from rpt.config import ProcessingConfig
    from rpt.processors.point_cloud import gain_stride_for, stack_stride_for

    d = ProcessingConfig()
    assert gain_stride_for(0, d) == 16 and gain_stride_for(10_000_000 * 16, d) == 16
    assert gain_stride_for(10_000_000 * 16 + 1, d) == 17
    assert stack_stride_for(0, d) == 1 and stack_stride_for(20_000_000, d) == 1
    assert stack_stride_for(20_000_001, d) == 2
    b = ProcessingConfig(point_stride=2, max_points_per_gain=100, max_points_stack=60)
    assert [gain_stride_for(n, b) for n in (0, 200, 201, 300, 301)] == [2, 2, 3, 3, 4]
    assert [stack_stride_for(n, b) for n in (1, 60, 61, 357)] == [1, 1, 2, 6]


def _parse_ply(text: str):
    lines = text.splitlines()
    end = lines.index("end_header")
    rows = [ln.split() for ln in lines[end + 1:]]
    xyz = np.array([[float(v) for v in r[:3]] for r in rows], dtype=np.float64).reshape(-1, 3)
    rgb = np.array([[int(v) for v in r[3:]] for r in rows], dtype=np.uint8).reshape(-1, 3)
    return "\n".join(lines[:end + 1]) + "\n", xyz, rgb


@pytest.mark.parametrize("key", ["A_offset_ply", "A_flat_ply", "B_offset_ply", "C_flat_ply",
                                 "D_offset_ply"])
def test_host_formatter_reproduces_reference_ply_text(golden, tmp_path, key):
    """Six-decimal texts read back as float64 print as themselves, so the host formatter (and
    write_ply around it: header, grey default) has to give the reference's file back."""
    from rpt.core import text
    from rpt.core.loaders import PointCloud
    from rpt.core.writers import write_ply

    ref = str(golden("g12_build.npz")[key])
    header, xyz, rgb = _parse_ply(ref)
    assert "-0.000000" in ref or not key.startswith("A")
    rows = text.format_ply_rows_host(xyz[:, 0], xyz[:, 1], xyz[:, 2], rgb)
    assert (header.encode() + rows) == ref.encode()
    write_ply(tmp_path / "sub" / "out.ply",
              PointCloud(x=xyz[:, 0], y=xyz[:, 1], z=xyz[:, 2], colors=rgb))
    assert (tmp_path / "sub" / "out.ply").read_bytes() == ref.encode()


def test_write_ply_defaults_to_grey_and_takes_float32(tmp_path):
    from rpt.core.loaders import PointCloud
    from rpt.core.writers import write_ply

    x = np.float32([0.0, -0.0, 1.5, -2.5e-7, 0.0078125])
    y = np.float32([1.0, 2.0, 3.0, 4.0, -0.0234375])
    z = np.float32([255.0, 0.1, 1e-7, 500.25, 600.0])
    write_ply(tmp_path / "grey.ply", PointCloud(x=x, y=y, z=z))
    body = "".join(f"{a:.6f} {b:.6f} {c:.6f} 180 180 180\n" for a, b, c in zip(x, y, z))
    text = (tmp_path / "grey.ply").read_text()
    assert text.startswith("ply\nformat ascii 1.0\nelement vertex 5\nproperty float x\n")
    assert text.endswith("property uchar blue\nend_header\n" + body)
    assert "-0.000000 2.000000 0.100000 180" in body and "0.007812 -0.023438 600.0" in body


def test_host_label_formatter_equals_savetxt():
    from rpt.core import text

    rng = np.random.default_rng(5)
    coords = rng.uniform(-600.0, 600.0, (400, 3)).astype(np.float32)
    coords[:4] = [[0.0, -0.0, np.nan], [np.inf, -np.inf, 1e20], [0.0078125, -0.0078125, 5e-7],
                  [2.5e-7, -4e-7, 1e-45]]
    labels = rng.integers(-1, 100000, 400).astype(np.int32)
    labels[:3] = [-1, 2**31 - 1, -2**31]
    buf = io.BytesIO()
    np.savetxt(buf, np.column_stack((coords, labels)), fmt="%.6f,%.6f,%.6f,%d")
    got = text.format_label_rows_host(coords[:, 0], coords[:, 1], coords[:, 2], labels)
    assert got == buf.getvalue()


def test_cli_help_lists_build():
    from click.testing import CliRunner

    from rpt.cli.main import cli

    r = CliRunner().invoke(cli, ["--help"])
    assert r.exit_code == 0 and "build" in r.output and "cluster" in r.output
    r = CliRunner().invoke(cli, ["build", "--help"])
    assert r.exit_code == 0
    for opt in ("--flat / --no-flat", "--offset / --no-offset", "--plot / --no-plot",
                "INPUT_DIR OUTPUT_DIR"):
        assert opt in r.output, r.output


@pytest.mark.parametrize("case", ["A", "B", "C", "D"])
def test_seeded_inputs_hash_to_the_golden_digests(tmp_path, golden, case):
    from make_build_golden import inputs_digest, write_inputs

    write_inputs(case, tmp_path)
    assert inputs_digest(tmp_path) == str(golden("g12_build.npz")[f"{case}_digest"])
