"""``radar-pipeline build`` on the GPU against the reference's own run (tests/golden/g12_build.npz;
the inputs are regenerated from the seeds of tests/golden/make_build_golden.py): PLY files and
stdout byte for byte, the click command, and the built PLY through ``cluster``."""
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
    here, the PLY comparisons below fail for that reason and not because of a kernel."""
    from make_build_golden import sweep_row_counts

    from rpt.core.transforms import simple_trig_tables

    g = golden("g12_build.npz")
    info = json.loads(str(g["info"]))
    for rows in sweep_row_counts():
        a = np.linspace(0.0, 2 * np.pi, rows, endpoint=False, dtype=np.float32)
        c, s = simple_trig_tables(a)
        same = np.array_equal(c, g[f"cos_{rows}"]) and np.array_equal(s, g[f"sin_{rows}"])
        assert same, (
            f"this host's numpy {np.__version__} float32 cos/sin differ from the host that "
            f"generated g12_build.npz ({info}) for {rows} rows: a host numpy difference, not a "
            "kernel fault -- the PLY comparisons of this file will differ in the same places")


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_build_stacked_clouds_matches_reference(tmp_path, golden, gpu, case):
    from make_build_golden import inputs_digest, write_inputs

    from rpt.config import ProcessingConfig
    from rpt.processors.point_cloud import build_stacked_clouds

    g = golden("g12_build.npz")
    c = write_inputs(case, tmp_path / "in")
    assert inputs_digest(tmp_path / "in") == str(g[f"{case}_digest"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        outs = build_stacked_clouds(tmp_path / "in", tmp_path / "out",
                                    ProcessingConfig(**c["processing"]))
    assert buf.getvalue() == str(g[f"{case}_stdout"])
    assert list(outs) == ["offset", "flat"]
    assert outs["offset"].name == "frame_stack_v3.ply"
    assert outs["flat"].name == "frame_stack_flat_v3.ply"
    for key, path in outs.items():
        assert path.read_bytes() == str(g[f"{case}_{key}_ply"]).encode(), (case, key)


def test_build_cli_matches_reference(tmp_path, golden, gpu):
    from click.testing import CliRunner
    from make_build_golden import write_inputs

    from rpt.cli.main import cli

    g = golden("g12_build.npz")
    c = write_inputs("D", tmp_path / "in")
    cfg = tmp_path / "config.yaml"
    cfg.write_text(c["yaml"])
    r = CliRunner().invoke(cli, ["-c", str(cfg), "build", str(tmp_path / "in"),
                                 str(tmp_path / "out"), "--no-flat", "--no-plot"])
    assert r.exit_code == 0, r.output
    assert r.output == str(g["D_stdout"])
    assert r.output.endswith("Build complete.\n")
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["frame_stack_v3.ply"]
    assert (tmp_path / "out" / "frame_stack_v3.ply").read_bytes() == \
        str(g["D_offset_ply"]).encode()


def test_built_ply_goes_through_cluster(tmp_path, gpu):
    from make_build_golden import write_inputs

    from rpt.config import ClusteringConfig, ProcessingConfig
    from rpt.core.loaders import load_ply
    from rpt.processors.clustering import cluster_point_cloud
    from rpt.processors.point_cloud import build_stacked_clouds

    c = write_inputs("A", tmp_path / "in")
    with contextlib.redirect_stdout(io.StringIO()):
        outs = build_stacked_clouds(tmp_path / "in", tmp_path / "out",
                                    ProcessingConfig(**c["processing"]), generate_offset=False)
    assert list(outs) == ["flat"]
    cloud = load_ply(outs["flat"])
    assert cloud.size == 156 and cloud.colors.shape == (156, 3)
    labels = cluster_point_cloud(cloud, ClusteringConfig(eps_space=6.0, eps_time=1.0,
                                                         min_samples=3))
    assert labels.shape == (156,) and labels.dtype == np.int32 and labels.min() >= -1


def test_write_labels_csv_device_path_equals_savetxt(tmp_path, gpu):
    from rpt.core import text
    from rpt.core.writers import write_labels_csv

    assert text.gpu_visible()
    rng = np.random.default_rng(77)
    n = 5000
    coords = rng.uniform(-600.0, 600.0, (n, 3)).astype(np.float32)
    coords[:5] = [[0.0, -0.0, 2.5e-7], [0.0078125, -0.0078125, 5e-7], [-4e-7, 1.0, 255.0],
                  [599.9999, -599.9999, 0.5], [1e-45, -1e-45, 123456.7]]
    labels = rng.integers(-1, 40, n).astype(np.int32)
    write_labels_csv(tmp_path / "dev" / "labels.csv", coords, labels)
    np.savetxt(tmp_path / "ref.csv", np.column_stack((coords, labels)),
               fmt="%.6f,%.6f,%.6f,%d", header="x,y,z,label", comments="")
    assert (tmp_path / "dev" / "labels.csv").read_bytes() == (tmp_path / "ref.csv").read_bytes()
    # non-finite coordinates: the host formatter, same bytes as savetxt
    coords[7, 1] = np.nan
    coords[9, 2] = -np.inf
    write_labels_csv(tmp_path / "nan.csv", coords, labels)
    np.savetxt(tmp_path / "nan_ref.csv", np.column_stack((coords, labels)),
               fmt="%.6f,%.6f,%.6f,%d", header="x,y,z,label", comments="")
    assert (tmp_path / "nan.csv").read_bytes() == (tmp_path / "nan_ref.csv").read_bytes()
