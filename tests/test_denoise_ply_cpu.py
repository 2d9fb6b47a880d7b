"""The denoise pipeline's PLY records on the host (write_ply,
PointCloudWorkF/stdbscan_denoising_pipeline.py:767-855): rpt_ply_records_host -- the per-value code
the kernels of csrc/plyrec.hip run (csrc/plyrec.h) -- against the reference's own files (g16), the
``[labels >= 0]`` indexing, the viridis row rule against matplotlib, the counts and the limits."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
REC = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("c", "u1", (3,))])


def _body(ply: np.ndarray) -> bytes:
    return ply.tobytes().split(b"end_header\n", 1)[1]


@pytest.fixture(scope="module")
def g16(golden):
    return golden("g16_denoise_ply.npz")


def test_generator_inputs_are_the_golden_inputs(g16):
    sys.path.insert(0, str(GOLDEN))
    from make_denoise_ply_golden import cloud

    for name, a in zip(("x", "y", "z", "labels"), cloud()):
        assert a.dtype == g16[name].dtype
        assert a.tobytes() == g16[name].tobytes(), name   # bit patterns: NaN payloads included


def test_luts_are_the_writers_expressions(g16):
    from rpt.denoise import ply_luts

    lut20, lutv = ply_luts()
    assert lut20.shape == (20, 3) and lutv.shape == (257, 3)
    np.testing.assert_array_equal(lut20, g16["lut_tab20"])
    np.testing.assert_array_equal(lutv, g16["lut_viridis"])


@pytest.mark.parametrize("mode", ["labels", "plain"])
def test_host_records_match_reference_files(g16, mode):
    from rpt.denoise import ply_records_host

    lab = g16["labels"] if mode == "labels" else None
    lut = g16["lut_tab20"] if mode == "labels" else g16["lut_viridis"]
    got, kept, max_label = ply_records_host(g16["x"], g16["y"], g16["z"], lab, lut=lut)
    assert got == _body(g16[f"bin_{mode}"])
    assert kept == len(g16["x"])
    assert max_label == (2**31 - 1 if mode == "labels" else -1)


def test_signal_only_is_the_mask_indexing(g16):
    from rpt.denoise import ply_records_host

    lab = g16["labels"]
    keep = lab >= 0
    assert 0 < keep.sum() < len(lab) and (lab[~keep] == -7).any() and (lab[~keep] == -1).any()
    ref = np.frombuffer(_body(g16["bin_labels"]), REC)[keep].tobytes()
    got, kept, max_label = ply_records_host(g16["x"], g16["y"], g16["z"], lab, signal_only=True,
                                            lut=g16["lut_tab20"])
    assert got == ref
    assert kept == int(keep.sum()) and max_label == int(lab.max())


def test_viridis_row_rule_matches_matplotlib():
    """A LUT whose row r holds (r & 255, r >> 8, 0) makes a record's colour name the row taken;
    matplotlib's row is read off the same way from a colormap built on that table."""
    import matplotlib
    from matplotlib.colors import ListedColormap

    sys.path.insert(0, str(GOLDEN))
    from make_denoise_ply_golden import viridis_edges

    from rpt.denoise import ply_records_host

    rng = np.random.default_rng(1602)
    z = np.concatenate([viridis_edges(), rng.uniform(-5, 300, 20000).astype(np.float32)])
    rows = np.arange(257)
    lut = np.stack([rows & 255, rows >> 8, np.zeros_like(rows)], 1).astype(np.uint8)
    got, kept, _ = ply_records_host(z, z, z, None, lut=lut)
    c = np.frombuffer(got, REC)["c"].astype(int)
    got_rows = c[:, 0] + 256 * c[:, 1]
    # the same table as a 256-entry colormap; under / over / bad as viridis has them (rows 0,
    # 255 and the extra row 256)
    cmap = ListedColormap(lut[:256] / 255.0, N=256)
    cmap.set_bad((0.0, 1.0 / 255.0, 0.0))
    ref = (cmap(np.clip(z / 255.0, 0, 1))[:, :3] * 255 + 0.5).astype(int)
    ref_rows = ref[:, 0] + 256 * ref[:, 1]
    assert kept == len(z)
    np.testing.assert_array_equal(got_rows, ref_rows)
    assert got_rows[np.isnan(z)].tolist() == [256]
    assert got_rows[np.isposinf(z)].tolist() == [255] and got_rows[np.isneginf(z)].tolist() == [0]
    # and viridis itself: the colours the writer would take
    vir = matplotlib.colormaps["viridis"]
    want = (vir(np.clip(z / 255.0, 0, 1))[:, :3] * 255).astype(np.uint8)
    got_v, _, _ = ply_records_host(z, z, z, None)
    np.testing.assert_array_equal(np.frombuffer(got_v, REC)["c"], want)


def test_empty_input_and_limits():
    from rpt import _abi
    from rpt.denoise import ply_records_host

    e = np.zeros(0, np.float32)
    assert ply_records_host(e, e, e) == (b"", 0, -1)
    assert ply_records_host(e, e, e, np.zeros(0, np.int32), signal_only=True) == (b"", 0, -1)
    one = np.ones(1, np.float32)
    # every label negative: nothing kept, no label
    assert ply_records_host(one, one, one, np.array([-3], np.int32), True) == (b"", 0, -1)
    with pytest.raises(ValueError):
        ply_records_host(one, one, one, None, signal_only=True)
    lib = _abi.load()
    assert lib.rpt_ply_records_host(None, None, None, None, 0, None, 2**31, None, 0, None) == \
        -_abi.RPT_ENOTSUP
    assert [lib.rpt_ply_record_tiles(n) for n in (0, 1, 1024, 1025, 2**31 - 1)] == \
        [0, 1, 1, 2, 2**21]
