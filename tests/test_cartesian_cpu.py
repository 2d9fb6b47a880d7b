"""The host halves of ``convert`` and its helpers: aligned_inputs, sort-by-gain and filter-range
on temporary directories (return values, files and stdout), the host formatter of the x,y,z
rows against ``DataFrame.to_csv``, and the single-file cases of tests/golden/g13_convert.npz
recomputed with the native CSV reader and numpy."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

HDR = "Status,Scale,Range,Gain,Angle,Echo_0,Echo_1\n"


def _csv(path: Path, first_row: str = "1,32,3,40,0,5,0", more: int = 2) -> Path:
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(HDR + (first_row + "\n" if first_row is not None else "") +
                    "1,32,9,99,8,0,7\n" * (more if first_row is not None else 0))
    return path


@pytest.fixture
def raw(tmp_path):
    """A capture directory: gains 40, 50, 75 (float text), an unknown gain, a short first row, a
    non-numeric gain, a header-only file, an empty file and a file that is not a CSV."""
    d = tmp_path / "raw"
    _csv(d / "c01.csv", "1,32,3,40,0,5,0")
    _csv(d / "c02.csv", "1,32,1,50.0,0,5,0")
    _csv(d / "c03.csv", "1,32,2,75.9,0,5,0")
    _csv(d / "c04.csv", "1,32,3,40,0,5,0")
    _csv(d / "c05.csv", "1,32,3,60,0,5,0")
    _csv(d / "c06.csv", "1,32,3")
    _csv(d / "c07.csv", "1,32,3,forty,0,5,0")
    _csv(d / "c08.csv", None)
    (d / "c09.csv").write_text("")
    (d / "notes.txt").write_text(HDR + "1,32,3,40,0,5,0\n")
    return d


def test_sniff_gain_and_range(raw):
    from rpt.processors.filtering import get_csv_range
    from rpt.processors.sorting import sniff_gain

    assert [sniff_gain(raw / f"c0{k}.csv") for k in range(1, 10)] == \
        [40, 50, 75, 40, 60, None, None, None, None]
    assert [get_csv_range(raw / f"c0{k}.csv") for k in range(1, 10)] == \
        [3, 1, 2, 3, 3, 3, 3, None, None]
    two = _csv(raw / "two.csv", "1,32")
    assert get_csv_range(two) is None
    assert get_csv_range(_csv(raw / "txt.csv", "1,32,far,40")) is None


def test_sort_files_by_gain_moves_nothing(raw):
    from rpt.processors.sorting import sort_files_by_gain

    got = sort_files_by_gain(raw)
    assert got == {40: [raw / "c01.csv", raw / "c04.csv"], 50: [raw / "c02.csv"],
                   75: [raw / "c03.csv"]}
    assert sort_files_by_gain(raw, (60, 7)) == {60: [raw / "c05.csv"], 7: []}
    assert len(list(raw.glob("*.csv"))) == 9 and not (raw / "gain_40").exists()


def test_move_files_dry_run_then_real(raw, capsys):
    from rpt.processors.sorting import move_files_to_gain_folders

    moved = move_files_to_gain_folders(raw, dry_run=True)
    assert moved == {40: [raw / "c01.csv", raw / "c04.csv"], 50: [raw / "c02.csv"],
                     75: [raw / "c03.csv"]}
    assert capsys.readouterr().out == (
        "Would move gain 40: c01.csv -> gain_40/\nWould move gain 50: c02.csv -> gain_50/\n"
        "Would move gain 75: c03.csv -> gain_75/\nWould move gain 40: c04.csv -> gain_40/\n")
    assert not (raw / "gain_40").exists() and (raw / "c01.csv").exists()

    moved = move_files_to_gain_folders(raw, (40, 50, 75, 80))
    assert moved == {40: [raw / "gain_40" / "c01.csv", raw / "gain_40" / "c04.csv"],
                     50: [raw / "gain_50" / "c02.csv"], 75: [raw / "gain_75" / "c03.csv"], 80: []}
    assert capsys.readouterr().out == (
        "Moved gain 40: c01.csv -> gain_40/\nMoved gain 50: c02.csv -> gain_50/\n"
        "Moved gain 75: c03.csv -> gain_75/\nMoved gain 40: c04.csv -> gain_40/\n")
    assert all(p.exists() for v in moved.values() for p in v)
    assert (raw / "gain_80").is_dir()  # made although nothing went there
    assert sorted(p.name for p in raw.glob("*.csv")) == ["c05.csv", "c06.csv", "c07.csv",
                                                         "c08.csv", "c09.csv"]


def test_filter_range(raw, capsys):
    from rpt.processors.filtering import (find_files_by_range, find_targets,
                                          remove_files_by_range)
    from rpt.processors.sorting import move_files_to_gain_folders

    move_files_to_gain_folders(raw)
    capsys.readouterr()
    g40, g50, g75 = (raw / f"gain_{g}" for g in (40, 50, 75))
    assert sorted(find_targets(raw)) == [g40 / "c01.csv", g40 / "c04.csv", g50 / "c02.csv",
                                         g75 / "c03.csv"]
    assert list(find_targets(raw, (60, 50))) == [g50 / "c02.csv"]  # no gain_60 folder: skipped
    assert sorted(find_files_by_range(raw, {1, 2})) == [g50 / "c02.csv", g75 / "c03.csv"]

    assert remove_files_by_range(raw, {7}) == []
    assert capsys.readouterr().out == "No files with Range in {7} found.\n"

    got = remove_files_by_range(raw, {1, 2}, dry_run=True)
    lines = capsys.readouterr().out.splitlines()
    assert sorted(got) == [g50 / "c02.csv", g75 / "c03.csv"]
    assert lines[0] == "Would delete 2 files:"
    assert sorted(lines[1:]) == [f"  - {g50 / 'c02.csv'}", f"  - {g75 / 'c03.csv'}"]
    assert (g50 / "c02.csv").exists()

    got = remove_files_by_range(raw, {2}, (75,))
    assert got == [g75 / "c03.csv"] and not (g75 / "c03.csv").exists()
    assert capsys.readouterr().out == f"Deleting 1 files:\n  - {g75 / 'c03.csv'}\n"


def test_aligned_inputs(tmp_path):
    from rpt.processors.cartesian import aligned_inputs

    base = tmp_path / "in"
    for g, names in ((40, "cab"), (50, "yx"), (75, "prqs")):
        for nm in names:
            _csv(base / f"gain_{g}" / f"{nm}.csv")
    (base / "gain_40" / "d.txt").write_text("x")
    got = list(aligned_inputs(base, (40, 50, 75)))
    assert got == [
        (1, {40: base / "gain_40/a.csv", 50: base / "gain_50/x.csv", 75: base / "gain_75/p.csv"}),
        (2, {40: base / "gain_40/b.csv", 50: base / "gain_50/y.csv", 75: base / "gain_75/q.csv"})]
    assert [list(g) for _, g in aligned_inputs(base, (75, 40))] == [[75, 40]] * 3
    (base / "gain_60").mkdir()
    for gains in ((40, 60), (40, 99)):  # an empty folder and a missing one
        with pytest.raises(FileNotFoundError) as e:
            next(aligned_inputs(base, gains))
        assert str(e.value) == f"No CSVs found in {base / f'gain_{gains[1]}'}"


def test_batch_limit_and_names_without_a_gpu(tmp_path, monkeypatch, capsys):
    """--limit, the output names and the stdout line, with the conversion itself stubbed out."""
    from rpt.processors import cartesian

    base = tmp_path / "in"
    for g, count in ((40, 3), (50, 4)):
        for k in range(count):
            _csv(base / f"gain_{g}" / f"f{k}.csv")
    calls = []

    def fake(src, dst, threshold=0.0, config=None):
        calls.append((src, dst, threshold, config))
        return 1234567

    monkeypatch.setattr(cartesian, "convert_single_csv", fake)
    out = tmp_path / "out"
    cartesian.convert_batch_aligned(base, out, (50, 40), 12.5, limit=2)
    assert [c[:3] for c in calls] == [
        (base / "gain_50/f0.csv", out / "gain_50/0001_gain_50_cartesian.csv", 12.5),
        (base / "gain_40/f0.csv", out / "gain_40/0001_gain_40_cartesian.csv", 12.5),
        (base / "gain_50/f1.csv", out / "gain_50/0002_gain_50_cartesian.csv", 12.5),
        (base / "gain_40/f1.csv", out / "gain_40/0002_gain_40_cartesian.csv", 12.5)]
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == (f"[0001] gain 50: f0.csv -> {out / 'gain_50/0001_gain_50_cartesian.csv'} "
                        "(1,234,567 points)")
    assert len(lines) == 4
    calls.clear()
    cartesian.convert_batch_aligned(base, out, (50, 40))
    assert len(calls) == 6
    calls.clear()
    with pytest.raises(FileNotFoundError):  # the default gains include 75
        cartesian.convert_batch_aligned(base, out)
    assert calls == []


def test_cli_commands_without_a_gpu(raw):
    from click.testing import CliRunner

    from rpt.cli.main import cli

    r = CliRunner().invoke(cli, ["sort-by-gain", str(raw), "--dry-run"])
    assert r.exit_code == 0 and r.output.endswith("Would move 4 files total.\n")
    r = CliRunner().invoke(cli, ["sort-by-gain", str(raw)])
    assert r.exit_code == 0 and r.output.endswith("Moved 4 files total.\n")
    r = CliRunner().invoke(cli, ["filter-range", str(raw), "--dry-run"])
    assert r.exit_code == 0 and r.output.endswith("Would remove 2 files.\n")
    r = CliRunner().invoke(cli, ["filter-range", str(raw), "-r", "3", "-r", "2"])
    assert r.exit_code == 0 and r.output.startswith("Deleting 3 files:\n")
    assert r.output.endswith("Removed 3 files.\n")
    assert sorted(p.name for p in raw.rglob("gain_*/*.csv")) == ["c02.csv"]
    r = CliRunner().invoke(cli, ["convert", "--help"])
    assert r.exit_code == 0
    for opt in ("--threshold", "-t", "--batch", "--single", "--limit"):
        assert opt in r.output


def test_host_formatter_is_to_csv():
    import pandas as pd

    from _repr_pool import pool
    from rpt.core.text import format_xyz_rows_host

    p = pool(3)[:3000]
    x, y, z = p.copy(), np.roll(p, 7).copy(), -np.roll(p, 1001)
    x[5], y[9], z[11], x[12] = np.nan, np.inf, -np.inf, np.nan
    y[12] = np.nan
    z[12] = 37.0
    exp = pd.DataFrame({"x": x, "y": y, "z": z}).to_csv(index=False)
    assert exp.startswith("x,y,z\n")
    got = format_xyz_rows_host(x, y, z)
    assert b"x,y,z\n" + got == exp.encode()
    rows = got.split(b"\n")
    assert rows[12] == b",,37.0" and rows[5].startswith(b",")
    assert rows[9].split(b",")[1] == b"inf" and rows[11].split(b",")[2] == b"-inf"
    assert format_xyz_rows_host(x[:0], y[:0], z[:0]) == b""


def test_format_xyz_rows_without_device_inputs_matches_host():
    """float64 inputs are not the kernel's: whatever the machine, the host expression answers."""
    from rpt.core.text import format_xyz_rows, format_xyz_rows_host

    x = np.array([0.1, 2.5, 1e20])
    got = format_xyz_rows(x, x, x)
    assert isinstance(got, bytes) and got == format_xyz_rows_host(x, x, x)
    assert got.split(b"\n")[0] == b"0.1,0.1,0.1"


@pytest.mark.parametrize("case", ["S1", "S2", "S3", "S4", "S5"])
def test_golden_inputs_and_host_arithmetic(tmp_path, golden, case):
    """Without a GPU: the regenerated inputs are the recorded ones, and the native CSV reader,
    numpy's polar arithmetic and the host formatter give the reference's file (what the device
    path is compared with in tests/test_convert_gpu.py)."""
    import json
    import sys

    sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
    from make_convert_golden import inputs_digest, write_inputs

    from rpt.core.loaders import load_radar_csv
    from rpt.core.text import format_xyz_rows_host

    g = golden("g13_convert.npz")
    c = write_inputs(case, tmp_path)
    assert inputs_digest(case, tmp_path) == str(g[f"{case}_digest"])
    step = json.loads(str(g[f"{case}_steps"]))[0]
    sweep = load_radar_csv(tmp_path / c["files"][0][0])
    assert sweep.intensities.shape[1] == 1024 and sweep.intensities.dtype == np.float32
    x = sweep.ranges * np.cos(sweep.angles_rad[:, None])
    y = sweep.ranges * np.sin(sweep.angles_rad[:, None])
    mask = sweep.intensities > np.float32(c["threshold"])
    assert int(mask.sum()) == step["n_points"]
    text = b"x,y,z\n" + format_xyz_rows_host(x[mask], y[mask], sweep.intensities[mask])
    assert text.decode() == next(iter(step["files"].values()))
