"""``radar-pipeline convert`` (and ``sort-by-gain`` / ``filter-range`` in front of it) on the GPU
against the reference's own run (tests/golden/g13_convert.npz; the inputs are regenerated from the
seeds of tests/golden/make_convert_golden.py): output files and stdout byte for byte.  Every case
is replayed with its directory as the working directory and relative paths, as it was recorded."""
from __future__ import annotations

import contextlib
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))


def test_host_trig_tables_match_generating_host(golden):
    """Runs first: the cos/sin tables are host numpy values handed to the kernel.  If they differ
    here, the CSV comparisons below fail for that reason and not because of a kernel."""
    from make_convert_golden import angle_columns

    from rpt.core.transforms import trig_tables

    g = golden("g13_convert.npz")
    info = json.loads(str(g["info"]))
    for key, col in angle_columns().items():
        c, s = trig_tables(col)
        same = np.array_equal(c, g[f"cos_{key}"]) and np.array_equal(s, g[f"sin_{key}"])
        assert same, (
            f"this host's numpy {np.__version__} float32 cos/sin differ from the host that "
            f"generated g13_convert.npz ({info}) for sweep {key}: a host numpy difference, not a "
            "kernel fault -- the CSV comparisons of this file will differ in the same places")


def _case(golden, case, directory):
    from make_convert_golden import inputs_digest, write_inputs

    g = golden("g13_convert.npz")
    c = write_inputs(case, directory)
    assert inputs_digest(case, directory) == str(g[f"{case}_digest"])
    return c, json.loads(str(g[f"{case}_steps"]))


def _same_files(got: dict, want: dict, what):
    assert sorted(got) == sorted(want), what
    for name in want:
        if got[name] != want[name]:  # name the first line that differs
            a, b = got[name].split("\n"), want[name].split("\n")
            for i, line in enumerate(b):
                assert i < len(a) and a[i] == line, (what, name, i, a[i:i + 1], line)
        assert got[name] == want[name], (what, name)


@pytest.mark.parametrize("case", ["S1", "S2", "S3", "S4", "S5"])
def test_convert_single_csv_matches_reference(tmp_path, monkeypatch, golden, gpu, case):
    from make_convert_golden import tree

    from rpt.processors.cartesian import convert_single_csv

    c, steps = _case(golden, case, tmp_path)
    monkeypatch.chdir(tmp_path)
    src = Path(c["files"][0][0])
    n = convert_single_csv(src, Path("out") / "nested" / f"{src.stem}_xyz.csv", c["threshold"])
    assert n == steps[0]["n_points"]
    _same_files(tree("out"), steps[0]["files"], case)
    text = next(iter(steps[0]["files"].values()))
    assert text.count("\n") == n + 1 and text.startswith("x,y,z\n")


def test_special_rows_are_in_the_golden(golden):
    """What the cases are there for, read from the recorded files."""
    g = golden("g13_convert.npz")

    def text(case):
        return next(iter(json.loads(str(g[f"{case}_steps"]))[0]["files"].values()))

    s1 = text("S1")
    assert "\n-0.0,0.0," in s1 and "e-08," in s1 and ",65504.5\n" in s1 and ",0.1\n" in s1
    assert "e+16," in text("S2") or "e+17," in text("S2")
    assert text("S4") == "x,y,z\n"
    assert "\n,,37.0\n" in text("S5")


def test_convert_batch_aligned_matches_reference(tmp_path, monkeypatch, golden, gpu):
    from make_convert_golden import tree

    from rpt.processors.cartesian import convert_batch_aligned

    c, steps = _case(golden, "B", tmp_path)
    monkeypatch.chdir(tmp_path)
    for step, (limit, dest) in zip(steps, ((None, "out"), (1, "out1"))):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            convert_batch_aligned(Path("in"), Path(dest), (40, 50, 75), c["threshold"], limit)
        assert buf.getvalue() == step["stdout"]
        _same_files(tree(dest), step["files"], dest)
    with pytest.raises(FileNotFoundError) as e:
        convert_batch_aligned(Path("in"), Path("out2"), (40, 60), c["threshold"])
    assert str(e.value) == steps[2]["stdout"] and not Path("out2").exists()


def test_cli_commands_match_reference(tmp_path, monkeypatch, golden, gpu):
    from click.testing import CliRunner
    from make_convert_golden import c_steps, tree

    from rpt.cli.main import cli

    _, steps = _case(golden, "C", tmp_path)
    monkeypatch.chdir(tmp_path)
    assert len(steps) == len(c_steps())
    for (args, roots), step in zip(c_steps(), steps):
        r = CliRunner().invoke(cli, args)
        assert r.exit_code == 0, (args, r.output, r.exception)
        if args[2] == "filter-range":  # the folders are globbed unsorted: compare the lines sorted
            assert sorted(r.output.splitlines()) == sorted(step["stdout"].splitlines()), args
            assert r.output.splitlines()[-1] == step["stdout"].splitlines()[-1]
        else:
            assert r.output == step["stdout"], args
        files = tree(*roots)
        if roots == ["raw"]:
            files = {k: "" for k in files}
        _same_files(files, step["files"], args)
    assert steps[-1]["stdout"].startswith("Saved ") and "one/single.csv" in steps[-1]["stdout"]
