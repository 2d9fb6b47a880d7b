"""The host side of the gain-fusion PLY builder (PointCloudWork/5_gain_fusion_ply_builder.py in
rpt.processors.fusion / rpt.cli.gain_fusion): rpt_heat_host and rpt_fixed4_repr -- the per-value
code the kernels run (csrc/heat.h) -- and the host "%.4f" row formatter against the reference's
own outputs (tests/golden/g14_gain_fusion.npz), against numpy's percentile and against CPython's
"%.4f"; the CLI surface; the golden's seeded inputs.  No GPU.  Every comparison is exact."""
from __future__ import annotations

import contextlib
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))

G14 = "g14_gain_fusion.npz"

# the edge values of the "%.4f" layout: exact ties (-> even), a negative that rounds to zero, a
# carry into the integer part, the signed zero, the top of the domain, subnormals
EDGE_VALUES = np.array(
    [0.03125, 0.09375, -0.00001, 9999.99995, -0.0, 0.0, 2.0**39, -(2.0**39), 1e-45, -1e-40,
     0.00005, 0.00015, 0.00025, 123456.789, 1.5, 2.5e-5, 0.99995, 0.99994, 1099511500000.0,
     255.0, 63.75, 1e-4, 4.9999e-5, 5.0001e-5], np.float32)


@pytest.fixture(scope="module")
def lib():
    from rpt import _abi

    return _abi.load()


def heat_host(lib, v, off=None, colors_only=False):
    """rpt_heat_host -> (min, p99, z, rgb)."""
    from rpt import _abi

    v = np.ascontiguousarray(v, np.float32)
    off = np.array([0, len(v)] if off is None else off, np.int64)
    S = len(off) - 1
    mn, p = np.empty(S, np.float32), np.empty(S, np.float32)
    z, rgb = np.empty(len(v), np.float32), np.empty((len(v), 3), np.uint8)
    _abi.check(lib.rpt_heat_host(v.ctypes.data, len(v), off.ctypes.data, S, int(colors_only),
                                 mn.ctypes.data, p.ctypes.data, z.ctypes.data, rgb.ctypes.data),
               "rpt_heat_host")
    return mn, p, z, rgb


def fixed4(lib, v):
    from rpt import _abi

    v = np.ascontiguousarray(v, np.float32)
    out = np.zeros((len(v), _abi.FIXED4_SLOT), np.uint8)
    lens = np.zeros(len(v), np.int32)
    _abi.check(lib.rpt_fixed4_repr(v.ctypes.data, len(v), out.ctypes.data, lens.ctypes.data),
               "rpt_fixed4_repr")
    return [out[i, :max(lens[i], 0)].tobytes().decode() for i in range(len(v))], lens


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_heat_host_matches_reference_helpers(lib, golden):
    from make_fusion_golden import helper_inputs

    g = golden(G14)
    both, alone = helper_inputs()
    for k, a in enumerate(both):
        assert np.array_equal(bits(a), bits(g[f"h{k}_in"])), k
        mn, p, z, rgb = heat_host(lib, a)
        assert np.array_equal(bits(z), bits(g[f"h{k}_z"])), k
        assert np.array_equal(rgb, g[f"h{k}_rgb"]), k
        assert mn[0] == a.min()
    for k, a in enumerate(alone):
        assert np.array_equal(bits(a), bits(g[f"c{k}_in"])), k
        assert np.array_equal(heat_host(lib, a, colors_only=True)[3], g[f"c{k}_rgb"]), k


def test_heat_host_segments_equal_single_calls(lib):
    rng = np.random.default_rng(5)
    sizes = [1, 0, 2, 255, 0, 1000, 31, 0]
    v = rng.integers(6, 256, sum(sizes)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(sizes)])
    mn, p, z, rgb = heat_host(lib, v, off)
    for s, (a, b) in enumerate(zip(off[:-1], off[1:])):
        if a == b:
            continue
        m1, p1, z1, c1 = heat_host(lib, v[a:b])
        assert bits(mn[s:s + 1]) == bits(m1) and bits(p[s:s + 1]) == bits(p1)
        assert np.array_equal(bits(z[a:b]), bits(z1)) and np.array_equal(rgb[a:b], c1)


def test_heat_host_rejects_foreign_offsets(lib):
    from rpt import _abi

    v = np.ones(4, np.float32)
    for off in ([0, 3], [1, 4], [0, 3, 2, 4]):
        o = np.array(off, np.int64)
        assert lib.rpt_heat_host(v.ctypes.data, 4, o.ctypes.data, len(o) - 1, 0, None, None,
                                 None, None) == _abi.RPT_EINVAL
    assert lib.rpt_heat_host(None, 0, None, 0, 1, None, None, None, None) == _abi.RPT_OK


@pytest.mark.parametrize("n", [1, 2, 11, 26, 31, 52, 101, 1000, 3001, 4096])
def test_host_percentile_is_numpys(lib, golden, n):
    """The float32 rule of heat::rank99 / lerp99 against np.percentile(a, 99) itself.  n = 101:
    the virtual index is the integer 99 (t = 0); 11, 26, 31, 52: both branches of the lerp."""
    info = json.loads(str(golden(G14)["info"]))
    if np.__version__ != info["numpy"]:
        pytest.skip(f"np.percentile's float32 rule was recorded for numpy {info['numpy']}")
    rng = np.random.default_rng(1000 + n)
    for kind in range(4):
        for _ in range(25):
            if kind == 0:
                a = rng.integers(6, 256, n).astype(np.float32)            # the loader's echoes
            elif kind == 1:
                a = (rng.random(n) * 300 - 100).astype(np.float32)        # mixed sign
            elif kind == 2:
                a = rng.integers(6, 9, n).astype(np.float32)              # heavy ties
            else:
                a = np.sort(rng.standard_normal(n).astype(np.float32) * 1e3)[::-1].copy()
            mn, p, _, _ = heat_host(lib, a)
            want = np.percentile(a, 99)
            assert want.dtype == np.float32
            assert bits(p)[0] == bits([want])[0], (n, kind, p[0], want)
            assert mn[0] == a.min()


def test_fixed4_is_cpythons_percent_4f(lib):
    rng = np.random.default_rng(7)
    v = np.concatenate([
        EDGE_VALUES,
        (rng.standard_normal(20000) * 10.0 ** rng.integers(-7, 12, 20000)).astype(np.float32),
        rng.integers(0, 2**32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32),
        (np.arange(-2000, 2000) * 0.00005).astype(np.float32)])      # around the ties
    text, lens = fixed4(lib, v)
    n_out = 0
    for t, ln, x in zip(text, lens, v):
        if not np.isfinite(x) or abs(float(x)) >= 2.0**40:
            assert ln == 0
            n_out += 1
        else:
            assert t == "%.4f" % float(x), (x, t)
            assert 6 <= ln <= 19
    assert n_out > 100
    assert fixed4(lib, EDGE_VALUES[:5])[0] == ["0.0312", "0.0938", "-0.0000", "10000.0000",
                                               "-0.0000"]
    assert max(lens) == 19 and "%.4f" % -(2.0**39) == "-549755813888.0000"


def test_format_ply4_rows_host_is_percent_4f():
    from rpt.core.text import format_ply4_rows_host

    v = EDGE_VALUES
    n = len(v)
    rgb = np.array([0, 9, 10, 99, 100, 255], np.uint8)[np.arange(3 * n) % 6].reshape(n, 3)
    got = format_ply4_rows_host(v, v[::-1], -v, rgb)
    want = "".join("%s %s %s %d %d %d\n" % ("%.4f" % float(a), "%.4f" % float(b),
                                            "%.4f" % float(np.float32(-a)), *c)
                   for a, b, c in zip(v, v[::-1], rgb)).encode()
    assert got == want
    assert format_ply4_rows_host(v[:0], v[:0], v[:0], rgb[:0]) == b""


def _golden_plys(golden):
    """Every PLY the golden stores whole: (name, text)."""
    g = golden(G14)
    out = []
    for cap in ("cap", "long"):
        for step in json.loads(str(g[f"{cap}_steps"])):
            for name, text in step["files"].items():
                if isinstance(text, str):
                    out.append((f"{cap}/{name}", text))
    return out


def test_host_rows_and_fixed4_reproduce_golden_plys(lib, golden):
    """Parse every stored PLY's rows back (a float32 whose "%.4f" is the field) and format them
    again: the host formatter and the kernels' per-value code give the golden's bytes."""
    from rpt.core.text import format_ply4_rows_host
    from rpt.processors.fusion import _ply_header

    plys = _golden_plys(golden)
    assert len(plys) > 60
    n_rows = 0
    for name, text in plys:
        head, body = text.split("end_header\n")
        rows = [r.split(" ") for r in body.splitlines()]
        assert (head + "end_header\n").encode() == _ply_header(len(rows)), name
        if not rows:
            continue
        xyz = np.array([[np.float32(f) for f in r[:3]] for r in rows], np.float32)
        rgb = np.array([[int(c) for c in r[3:]] for r in rows], np.uint8)
        assert format_ply4_rows_host(xyz[:, 0], xyz[:, 1], xyz[:, 2], rgb).decode() == body, name
        flat = fixed4(lib, xyz.reshape(-1))[0]
        assert flat == [f for r in rows for f in r[:3]], name
        n_rows += len(rows)
    assert n_rows > 3000


def test_golden_plys_colours_follow_from_their_z(lib, golden):
    """individual mode writes z = the normalised intensity at four decimals and its colour; the
    map is continuous, so the colour of the ROUNDED z is within one count of the stored one -- a
    coarse check that the golden and heat::rgb speak of the same map."""
    g = golden(G14)
    step = next(s for s in json.loads(str(g["cap_steps"])) if s["name"] == "ind_abs")
    text = step["files"]["o/ind_abs/frame_0002_gains_40_70_75.ply"]
    rows = [r.split(" ") for r in text.split("end_header\n")[1].splitlines()]
    z = np.array([np.float32(r[2]) for r in rows], np.float32)
    rgb = np.array([[int(c) for c in r[3:]] for r in rows], np.int32)
    got = heat_host(lib, z, colors_only=True)[3].astype(np.int32)
    assert np.abs(got - rgb).max() <= 1
    assert z.max() == 255.0 and z.min() == 0.0


def test_numpy_helpers_without_gpu_use_the_host_code(lib, golden, monkeypatch):
    from make_fusion_golden import helper_inputs

    from rpt.processors import fusion

    monkeypatch.setattr(fusion, "_on_device", lambda: False)
    g = golden(G14)
    both, alone = helper_inputs()
    for k, a in enumerate(both):
        z = fusion.normalize_intensity(a)
        assert z.dtype == np.float32 and np.array_equal(bits(z), bits(g[f"h{k}_z"]))
        assert np.array_equal(fusion.intensity_to_rgb(z), g[f"h{k}_rgb"])
    for k, a in enumerate(alone):
        assert np.array_equal(fusion.intensity_to_rgb(a), g[f"c{k}_rgb"])
        # another dtype is numpy's business, in that dtype; on exactly representable inputs the
        # float64 map agrees wherever the float32 division was exact
    a = np.arange(0, 256, dtype=np.float64)
    assert fusion.intensity_to_rgb(a).shape == (256, 3)
    assert fusion.normalize_intensity(np.array([], np.float32)).size == 0
    assert fusion.intensity_to_rgb(np.array([], np.float32)).shape == (0, 3)
    gains = np.array([40, 50, 60, 70, 75], np.int32)
    assert fusion.gain_to_rgb(gains).tolist() == [[0, 114, 255], [0, 200, 83], [0, 0, 0],
                                                  [255, 165, 0], [255, 87, 34]]
    assert (fusion.NORMALIZE_INTENSITY, fusion.INTENSITY_PERCENTILE) == (True, 99)
    assert fusion.GAIN_COLORS[75] == (255, 87, 34)
    monkeypatch.setattr(fusion, "INTENSITY_PERCENTILE", 95)
    with pytest.raises(NotImplementedError):
        fusion.normalize_intensity(both[0])


def test_write_ply_host_path(tmp_path, monkeypatch, capsys):
    """write_ply and write_ply_fast are one path; without a GPU the rows come from the host
    formatter."""
    from rpt.core import text
    from rpt.processors import fusion

    monkeypatch.setattr(text, "gpu_visible", lambda: False)
    assert fusion.write_ply is fusion.write_ply_fast
    x = np.array([1.5, -0.00001, 0.03125], np.float64)
    rgb = np.array([[0, 9, 10], [99, 100, 255], [1, 2, 3]], np.uint8)
    fusion.write_ply_fast(tmp_path / "a.ply", x, x, x.astype(np.float32), rgb)
    assert capsys.readouterr().out == "  Wrote 3 points to a.ply\n"
    assert (tmp_path / "a.ply").read_text() == (
        "ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\n"
        "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
        "end_header\n1.5000 1.5000 1.5000 0 9 10\n-0.0000 -0.0000 -0.0000 99 100 255\n"
        "0.0312 0.0312 0.0312 1 2 3\n")


def test_group_budget_is_one_staging_buffer():
    from rpt.core import text
    from rpt.processors import fusion

    assert text.PLY4_ROW_MAX == 3 * 19 + 3 * 3 + 6
    assert fusion._group_point_budget() == text._COPY_CHUNK // 72 == 466033
    assert fusion._budget() == 466033


@pytest.mark.parametrize("cmd", ["individual", "stacked", "comparison"])
def test_cli_help(cmd):
    from rpt.cli import gain_fusion

    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit) as e:
        gain_fusion.main([cmd, "--help"])
    assert e.value.code == 0
    for opt in ("--data-dir", "--output-dir", "--device"):
        assert opt in buf.getvalue()


def test_cli_defaults_and_epilog(capsys):
    from rpt.cli import gain_fusion

    ap = gain_fusion.build_parser()
    a = ap.parse_args(["individual"])
    assert (a.max_frames, a.mode, a.device) == (0, "absolute", None)
    assert a.output_dir == Path.cwd() / "gain_fused_ply" / "individual"
    a = ap.parse_args(["stacked"])
    assert (a.max_frames, a.time_spacing, a.mode) == (100, 10.0, "absolute")
    assert a.output_dir == Path.cwd() / "gain_fused_ply" / "stacked"
    a = ap.parse_args(["comparison"])
    assert a.frame == 0 and a.output_dir == Path.cwd() / "gain_fused_ply" / "comparison"
    a = ap.parse_args(["stacked", "--max-frames", "4", "--time-spacing", "2.5", "--mode", "max",
                       "--device", "cuda:0"])
    assert (a.max_frames, a.time_spacing, a.mode, a.device) == (4, 2.5, "max", "cuda:0")
    with pytest.raises(SystemExit):
        ap.parse_args(["individual", "--mode", "mean"])
    gain_fusion.main([])   # no sub-command: the help text, like the script
    out = capsys.readouterr().out
    assert "Build gain-fused PLY point clouds" in out
    assert "comparison  - Create separate PLYs for each gain at one frame" in out


def test_generator_inputs_by_digest(tmp_path, golden):
    from make_fusion_golden import CAPTURES, STEPS, inputs_digest, write_inputs

    g = golden(G14)
    for cap in CAPTURES:
        write_inputs(cap, tmp_path / cap)
        assert inputs_digest(cap, tmp_path / cap) == str(g[f"{cap}_digest"]), cap
        assert [s["name"] for s in json.loads(str(g[f"{cap}_steps"]))] == \
            [name for c, name, *_ in STEPS if c == cap]
    assert (GOLDEN / G14).stat().st_size < 300_000
    assert set(json.loads(str(g["info"]))) >= {"numpy", "pandas", "cpu"}
