"""The gain-fusion PLY builder on the GPU (PointCloudWork/5_gain_fusion_ply_builder.py in
rpt.processors.fusion / rpt.cli.gain_fusion): the segmented percentile kernel and the colour
kernel bit for bit against the host code (rpt_heat_host, itself pinned to the reference and to
numpy by tests/test_gain_fusion_cpu.py), the "%.4f" text layout byte for byte against CPython,
and every case of tests/golden/g14_gain_fusion.npz (the reference's own run; the inputs are
regenerated from the seeds of tests/golden/make_fusion_golden.py) end to end: stdout and files.
Every comparison is exact."""
from __future__ import annotations

import contextlib
import ctypes as C
import hashlib
import io
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))

G14 = "g14_gain_fusion.npz"
# one call holds all of these: one point, two, around the 256-bin histogram and the 1024-thread
# block, an empty segment in the middle, a rank on an integer index (101), a long one, an empty end
SEG_SIZES = [1, 2, 255, 256, 257, 0, 101, 2049, 70001, 0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def heat_host(v, off, colors_only=False):
    from rpt import _abi

    v = np.ascontiguousarray(v, np.float32)
    off = np.asarray(off, np.int64)
    S = len(off) - 1
    mn, p = np.empty(S, np.float32), np.empty(S, np.float32)
    z, rgb = np.empty(len(v), np.float32), np.empty((len(v), 3), np.uint8)
    _abi.check(_abi.load().rpt_heat_host(v.ctypes.data, len(v), off.ctypes.data, S,
                                         int(colors_only), mn.ctypes.data, p.ctypes.data,
                                         z.ctypes.data, rgb.ctypes.data), "rpt_heat_host")
    return mn, p, z, rgb


def rank99(m):
    """lo, hi of np.percentile(a, 99) for m values (the float32 rule)."""
    vi = np.float32(m - 1) * (np.float32(99) / np.float32(100))
    lo = int(np.floor(vi))
    return lo, min(lo + 1, m - 1)


def _value_sets():
    rng = np.random.default_rng(1410)
    n = sum(SEG_SIZES)
    off = offsets(SEG_SIZES)
    sets = {
        "echo_ties": rng.integers(6, 256, n).astype(np.float32),
        "all_equal": np.full(n, 100.0, np.float32),
        "random": (rng.standard_normal(n) * 1e3).astype(np.float32),
        "mixed_sign": ((rng.random(n) - 0.5) * 1000).astype(np.float32),
        "negative": (-rng.random(n) * 50 - 1).astype(np.float32),
        "few_values": rng.integers(6, 9, n).astype(np.float32),
    }
    # sorted[lo] = 255.0 and sorted[hi] = 65536.5: the keys differ in their top byte, and the
    # upper neighbour is found by the fifth pass
    top = np.empty(n, np.float32)
    for a, b in zip(off[:-1], off[1:]):
        m = int(b - a)
        if m == 0:
            continue
        lo, _ = rank99(m)
        seg = np.concatenate([rng.integers(6, 256, lo).astype(np.float32), [255.0],
                              np.full(m - lo - 1, 65536.5, np.float32)])
        top[a:b] = rng.permutation(seg)
    sets["top_byte"] = top
    return off, sets


@pytest.fixture(scope="module")
def value_sets():
    return _value_sets()


@pytest.mark.parametrize("name", ["echo_ties", "all_equal", "top_byte", "random", "mixed_sign",
                                  "negative", "few_values"])
def test_segment_percentile_kernel_is_the_host_code(gpu, value_sets, name):
    from rpt.processors.fusion import segment_heat

    off, sets = value_sets
    v = sets[name]
    mn_h, p_h, z_h, rgb_h = heat_host(v, off)
    z, rgb, mn, p = segment_heat(torch.from_numpy(v).to(gpu), torch.from_numpy(off).to(gpu))
    live = np.diff(off) > 0
    assert live.sum() == len(SEG_SIZES) - 2
    assert np.array_equal(bits(mn.cpu().numpy())[live], bits(mn_h)[live])
    assert np.array_equal(bits(p.cpu().numpy())[live], bits(p_h)[live]), (
        name, p.cpu().numpy()[live], p_h[live])
    assert np.array_equal(bits(z.cpu().numpy()), bits(z_h))
    assert np.array_equal(rgb.cpu().numpy(), rgb_h)
    # the host code is numpy's rule: spot-check it here on the two longest segments
    for s in (7, 8):
        seg = v[off[s]:off[s + 1]]
        assert bits([np.percentile(seg, 99)])[0] == bits(p_h[s:s + 1])[0]
        assert seg.min() == mn_h[s]
    if name == "top_byte":
        for s in np.nonzero(live)[0]:
            srt = np.sort(v[off[s]:off[s + 1]])
            lo, hi = rank99(len(srt))
            assert srt[lo] == 255.0 and (hi == lo or srt[hi] == 65536.5)
    if name == "all_equal":
        assert not z_h.any() and (rgb_h == (0, 0, 255)).all()


def _colour_case():
    """One array, three segments: min 0 and p99 255 exactly (so that chosen values land on
    normalized 0, 0.25, 0.5, 0.75, 1 and on their float32 neighbours, others above p99 are
    clipped); random echoes; a constant segment."""
    rng = np.random.default_rng(1411)
    f32 = np.float32
    edges = np.array([0.0, 63.75, 127.5, 191.25, 255.0], f32)
    near = np.concatenate([edges, np.nextafter(edges, f32(-1)), np.nextafter(edges, f32(999))])
    near = near[near >= 0]
    a = np.concatenate([near, (rng.random(4000) * 255).astype(f32), np.full(300, 255.0, f32),
                        np.array([255.5, 300.0, 1e6], f32)])
    b = rng.integers(6, 256, 3001).astype(f32)
    c = np.full(77, 42.0, f32)
    return np.concatenate([a, b, c]), offsets([len(a), len(b), len(c)]), near


def test_colour_kernel_is_the_host_code(gpu):
    from rpt.processors.fusion import heat_colors, segment_heat

    v, off, near = _colour_case()
    mn_h, p_h, z_h, rgb_h = heat_host(v, off)
    assert mn_h[0] == 0.0 and p_h[0] == 255.0 and p_h[2] <= mn_h[2]
    z, rgb, _, _ = segment_heat(torch.from_numpy(v).to(gpu), torch.from_numpy(off).to(gpu))
    z, rgb = z.cpu().numpy(), rgb.cpu().numpy()
    assert np.array_equal(bits(z), bits(z_h)) and np.array_equal(rgb, rgb_h)
    # the pieces' end points, by the script's own arithmetic
    for val, colour in ((0.0, (0, 0, 255)), (63.75, (0, 255, 255)), (127.5, (0, 255, 0)),
                        (191.25, (255, 255, 0)), (255.0, (255, 0, 0))):
        i = list(near).index(np.float32(val))
        assert z[i] == np.float32(val) and tuple(rgb[i]) == colour
    assert (z[off[1] - 3:off[1]] == 255.0).all()          # above p99: clipped
    assert not z[off[2]:].any() and (rgb[off[2]:] == (0, 0, 255)).all()
    # colours only, from an already normalised z
    only = heat_colors(torch.from_numpy(z_h).to(gpu)).cpu().numpy()
    assert np.array_equal(only, heat_host(z_h, [0, len(z_h)], colors_only=True)[3])
    assert np.array_equal(only, rgb_h)


def test_numpy_helpers_run_on_the_device(gpu, golden, monkeypatch):
    from make_fusion_golden import helper_inputs

    from rpt.processors import fusion

    calls = []
    real = fusion._heat_host
    monkeypatch.setattr(fusion, "_heat_host", lambda *a: calls.append(a) or real(*a))
    g = golden(G14)
    both, alone = helper_inputs()
    for k, a in enumerate(both):
        z = fusion.normalize_intensity(a)
        assert np.array_equal(bits(z), bits(g[f"h{k}_z"])), k
        assert np.array_equal(fusion.intensity_to_rgb(z), g[f"h{k}_rgb"]), k
    for k, a in enumerate(alone):
        assert np.array_equal(fusion.intensity_to_rgb(a), g[f"c{k}_rgb"]), k
    assert not calls


EDGE_VALUES = np.array(
    [0.03125, 0.09375, -0.00001, 9999.99995, -0.0, 0.0, 2.0**39, -(2.0**39), 1e-45, -1e-40,
     1.1754942e-38, 0.00005, 0.00015, 0.00025, 123456.789, 1.5, 0.99995, 255.0, 63.75,
     1099511500000.0], np.float32)
EDGE_COLOURS = np.array([0, 9, 10, 99, 100, 255], np.uint8)


def _ply4_inputs(n):
    rng = np.random.default_rng(1412 + n)
    pool = np.concatenate([
        EDGE_VALUES,
        (rng.standard_normal(max(n, 1)) * 10.0 ** rng.integers(-6, 11, max(n, 1))).astype(
            np.float32)])
    x, y, z = (pool[rng.permutation(len(pool))[np.arange(n) % len(pool)]] for _ in range(3))
    if n >= len(EDGE_VALUES):
        x[:len(EDGE_VALUES)] = EDGE_VALUES
    rgb = EDGE_COLOURS[rng.integers(0, 6, (n, 3))]
    if n:
        rgb[0] = (0, 9, 10)
        rgb[-1] = (99, 100, 255)
    return x, y, z, rgb


def _percent_4f(x, y, z, rgb):
    return "".join("%s %s %s %d %d %d\n" % ("%.4f" % float(np.float32(a)),
                                            "%.4f" % float(np.float32(b)),
                                            "%.4f" % float(np.float32(c)), *col)
                   for a, b, c, col in zip(x, y, z, rgb)).encode()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 5003])
def test_ply4_rows_are_cpythons(gpu, n, monkeypatch):
    from rpt.core import text

    monkeypatch.setitem(text._HOST, 3, lambda *a: pytest.fail("host formatter used"))
    x, y, z, rgb = _ply4_inputs(n)
    want = _percent_4f(x, y, z, rgb)
    assert text.format_ply4_rows(x, y, z, rgb) == want            # numpy in -> bytes
    dev = [torch.from_numpy(a).to(gpu) for a in (x, y, z, rgb)]
    got = text.format_ply4_rows(*dev)                             # device in -> device tensor
    assert got.is_cuda and got.cpu().numpy().tobytes() == want
    t, row_off = text.ply4_rows_device(*dev)
    row_off = row_off.cpu().numpy()
    assert row_off[0] == 0 and row_off[-1] == len(want) == t.numel()
    lens = np.diff(row_off)
    assert n == 0 or (lens.min() >= 24 and lens.max() <= text.PLY4_ROW_MAX)
    assert bytes(text.text_to_host(t)) == want
    if n >= len(EDGE_VALUES):
        rows = want.decode().split("\n")
        assert [r.split(" ")[0] for r in rows[:8]] == [
            "0.0312", "0.0938", "-0.0000", "10000.0000", "-0.0000", "0.0000",
            "549755813888.0000", "-549755813888.0000"]


def test_ply4_unsupported_rows_fall_back_to_the_host(gpu):
    from rpt import _abi
    from rpt._device import stream_handle
    from rpt.core import text

    x, y, z, rgb = _ply4_inputs(600)
    y[17] = np.nan
    z[300] = 2.0**40
    dev = [torch.from_numpy(a).to(gpu) for a in (x, y, z, rgb)]
    off = torch.empty(601, dtype=torch.int64, device=gpu)
    total, bad = C.c_int64(0), C.c_int64(0)
    _abi.check(_abi.load().rpt_text_rows_size(_abi.TEXT_PLY4, dev[0].data_ptr(),
                                              dev[1].data_ptr(), dev[2].data_ptr(),
                                              dev[3].data_ptr(), 600, off.data_ptr(),
                                              C.byref(total), C.byref(bad), stream_handle(gpu)))
    assert bad.value == 2
    o = off.cpu().numpy()
    assert o[18] == o[17] and o[301] == o[300] and o[-1] == total.value
    assert text.ply4_rows_device(*dev) is None
    want = _percent_4f(x, y, z, rgb)
    assert b" nan " in want and b" 1099511627776.0000 " in want
    assert text.format_ply4_rows(x, y, z, rgb) == want
    assert text.format_ply4_rows(*dev).cpu().numpy().tobytes() == want


def test_existing_layouts_still_equal_their_host_formatters(gpu):
    from rpt.core import text

    x, y, z, rgb = _ply4_inputs(700)
    labels = (np.arange(700, dtype=np.int32) * 7919) % 2001 - 1000
    finite = np.random.default_rng(3).standard_normal(700).astype(np.float32)
    assert text.format_ply_rows(x, y, z, rgb) == text.format_ply_rows_host(x, y, z, rgb)
    assert text.format_label_rows(x, y, z, labels) == text.format_label_rows_host(x, y, z, labels)
    assert text.format_xyz_rows(x, finite, z) == text.format_xyz_rows_host(x, finite, z)
    assert text.format_ply_rows(x, y, z, rgb) == "".join(
        "%.6f %.6f %.6f %d %d %d\n" % (float(a), float(b), float(c), *col)
        for a, b, c, col in zip(x, y, z, rgb)).encode()


# ---- end to end against the reference's run -------------------------------------------------

def test_host_trig_tables_match_generating_host(golden):
    """Runs before the cases: the cos/sin tables are host numpy values handed to K1.  If they
    differ here, the PLY comparisons below fail for that reason and not because of a kernel."""
    from make_fusion_golden import angle_columns

    from rpt.core.transforms import trig_tables

    g = golden(G14)
    info = json.loads(str(g["info"]))
    for key, col in angle_columns().items():
        c, s = trig_tables(col)
        same = np.array_equal(c, g[f"cos_{key}"]) and np.array_equal(s, g[f"sin_{key}"])
        assert same, (
            f"this host's numpy {np.__version__} float32 cos/sin differ from the host that "
            f"generated {G14} ({info}) for sweep {key}: a host numpy difference, not a kernel "
            "fault -- the PLY comparisons of this file will differ in the same places")


_GAIN_LINE = re.compile(r"  Gain \d+: \d+ files")


def _canon(stdout: str) -> str:
    """The "  Gain G: N files" block sorted: its order is the directory iteration's."""
    lines = stdout.split("\n")
    k = [i for i, line in enumerate(lines) if _GAIN_LINE.fullmatch(line)]
    if k:
        assert k == list(range(k[0], k[-1] + 1))
        lines[k[0]:k[-1] + 1] = sorted(lines[k[0]:k[-1] + 1])
    return "\n".join(lines)


def _snapshot(root) -> dict:
    """{path: bytes} of every file below root."""
    return {p.as_posix(): p.read_bytes() for p in sorted(Path(root).rglob("*")) if p.is_file()}


def _same_files(got: dict, want: dict, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    assert not any(p.endswith(".png") for p in got)
    for name, w in want.items():
        raw = got[name]
        if isinstance(w, dict):
            assert len(raw) == w["length"], (what, name)
            assert hashlib.sha256(raw).hexdigest() == w["sha256"], (what, name)
            continue
        if raw.decode() != w:  # name the first line that differs
            a, b = raw.decode().split("\n"), w.split("\n")
            for i, line in enumerate(b):
                assert i < len(a) and a[i] == line, (what, name, i, a[i:i + 1], line)
        assert raw.decode() == w, (what, name)


def _steps():
    from make_fusion_golden import STEPS

    return [(cap, name) for cap, name, *_ in STEPS]


def _run_step(golden, tmp_path, monkeypatch, cap, name, via):
    from make_fusion_golden import STEPS, inputs_digest, write_inputs

    from rpt.cli import gain_fusion
    from rpt.processors import fusion

    g = golden(G14)
    write_inputs(cap, tmp_path)
    assert inputs_digest(cap, tmp_path) == str(g[f"{cap}_digest"])
    want = next(s for s in json.loads(str(g[f"{cap}_steps"])) if s["name"] == name)
    _, _, fn, kw, argv = next(s for s in STEPS if s[0] == cap and s[1] == name)
    monkeypatch.chdir(tmp_path)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        if via == "cli":
            gain_fusion.main(argv)
        else:
            getattr(fusion, fn)(**{k: Path(v) if k.endswith("_dir") else v
                                   for k, v in kw.items()})
    assert _canon(buf.getvalue()) == _canon(want["stdout"]), (cap, name, via)
    _same_files(_snapshot(kw["output_dir"]), want["files"], (cap, name, via))
    return want


@pytest.mark.parametrize("via", ["api", "cli"])
@pytest.mark.parametrize("cap,name", _steps())
def test_golden_case(gpu, golden, tmp_path, monkeypatch, cap, name, via):
    _run_step(golden, tmp_path, monkeypatch, cap, name, via)


@pytest.mark.parametrize("name", ["ind_abs", "ind_max", "st_max", "cmp_0"])
def test_small_group_budget_changes_nothing(gpu, golden, tmp_path, monkeypatch, name):
    """A budget of 300 points cuts the capture's frames (about 290 points each) into at least
    three groups; stdout and files are those of the one-group run."""
    from rpt.processors import fusion

    launches = []
    real = fusion.segment_heat
    monkeypatch.setattr(fusion, "segment_heat",
                        lambda v, off: launches.append(off.numel() - 1) or real(v, off))
    monkeypatch.setattr(fusion, "GROUP_POINT_BUDGET", 300)
    _run_step(golden, tmp_path, monkeypatch, "cap", name, "api")
    if name == "cmp_0":   # one frame: the gains and the fused cloud are one group's segments
        assert launches == [5]
    else:
        assert len(launches) >= 3 and sum(launches) == 7 and max(launches) >= 2


def test_default_budget_is_one_group(gpu, golden, tmp_path, monkeypatch):
    from rpt.processors import fusion

    launches = []
    real = fusion.segment_heat
    monkeypatch.setattr(fusion, "segment_heat",
                        lambda v, off: launches.append(off.numel() - 1) or real(v, off))
    _run_step(golden, tmp_path, monkeypatch, "long", "ind", "api")
    assert launches == [51]
