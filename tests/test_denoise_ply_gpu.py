"""The denoise pipeline's PLY writer on the GPU (csrc/plyrec.hip; write_ply,
PointCloudWorkF/stdbscan_denoising_pipeline.py:767-855): the device records against the host twin
and the reference's own files (g16); the in-kernel ``[labels >= 0]`` compaction at the tile sizes
and keep patterns where ranks, byte residues and shared words can go wrong, between guard bytes;
offsets that are not the input's; write_ply and run_pipeline through the device writer, byte for
byte against g16 / g10; the colours alone."""
from __future__ import annotations

import contextlib
import io
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
REC = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("c", "u1", (3,))])
T = 1024          # points of one tile (plyrec::kTile)
GUARD = 64


def _body(ply: np.ndarray) -> bytes:
    return ply.tobytes().split(b"end_header\n", 1)[1]


@pytest.fixture(scope="module")
def g16(golden):
    return golden("g16_denoise_ply.npz")


def test_tile_size_is_the_librarys(gpu):
    from rpt import _abi

    lib = _abi.load()
    assert lib.rpt_ply_record_tiles(T) == 1 and lib.rpt_ply_record_tiles(T + 1) == 2


@pytest.mark.parametrize("mode", ["labels", "plain"])
def test_device_records_match_host_and_reference(gpu, g16, mode):
    from rpt.denoise import ply_records_device, ply_records_host

    lab = g16["labels"] if mode == "labels" else None
    D = lambda a: None if a is None else torch.from_numpy(a).to(gpu)  # noqa: E731
    got = ply_records_device(D(g16["x"]), D(g16["y"]), D(g16["z"]), D(lab)).cpu().numpy().tobytes()
    host, _, _ = ply_records_host(g16["x"], g16["y"], g16["z"], lab)
    assert got == host
    assert got == _body(g16[f"bin_{mode}"])


def _expected(x, y, z, lab, keep) -> bytes:
    """numpy's structured-array bytes of the kept points, coloured by the writer's expressions."""
    import matplotlib

    from rpt.denoise import ply_luts

    rec = np.empty(len(x), REC)
    rec["x"], rec["y"], rec["z"] = x, y, z
    if lab is not None:
        c = np.full((len(x), 3), 128, np.uint8)
        m = lab >= 0
        c[m] = ply_luts()[0][lab[m] % 20]
    else:
        c = (matplotlib.colormaps["viridis"](np.clip(z / 255.0, 0, 1))[:, :3] * 255).astype(
            np.uint8)
    rec["c"] = c
    return rec[keep].tobytes()


def _write_guarded(dev, x, y, z, lab, signal_only, shift=0, offsets=None, out_bytes=None):
    """rpt_ply_records_size / _write into a buffer with GUARD bytes of 0xA5 in front and behind
    (and `shift` more in front: the 16-byte phase of out); returns (the whole buffer on the host,
    kept, the true tile offsets).  offsets / out_bytes replace what the write pass is given."""
    from rpt import _abi
    from rpt._device import stream_handle
    from rpt.denoise import _lut_device, ply_records_size

    def D(a, t):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, t)).to(dev)

    xd, yd, zd, ld = D(x, np.float32), D(y, np.float32), D(z, np.float32), D(lab, np.int32)
    n = len(x)
    offs, kept, _ = ply_records_size(ld, n, signal_only, dev)
    buf = torch.full((GUARD + shift + 15 * kept + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    out = buf[GUARD + shift:]
    lut = _lut_device(lab is not None, dev)
    use = offs if offsets is None else offsets(offs)
    _abi.check(_abi.load().rpt_ply_records_write(
        xd.data_ptr() if n else None, yd.data_ptr() if n else None, zd.data_ptr() if n else None,
        None if ld is None else ld.data_ptr(), int(signal_only), lut.data_ptr(), n,
        use.data_ptr(), out.data_ptr(), 15 * kept if out_bytes is None else out_bytes,
        stream_handle(dev)), "rpt_ply_records_write")
    torch.cuda.synchronize(dev)
    return buf.cpu().numpy(), kept, offs.cpu().numpy()


def _patterns(n: int):
    """{name: keep mask [n]} -- the keep patterns of the issue at size n."""
    idx = np.arange(n)
    edge = min(n, T)
    pats = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": idx % 2 == 0}
    for r in (1, 2, 3, 4):   # a kept run of r points ending at the tile edge, then every point:
        m = idx >= T         # the next tile starts at byte residue 15 * r mod 4
        m[max(edge - r, 0):edge] = True
        pats[f"run{r}_to_edge"] = m
    pats["noise_tile_between"] = (idx < T) | (idx >= 2 * T)
    last = np.zeros(n, bool)
    last[n - 1] = True
    pats["one_in_last_tile"] = last
    return pats


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, T - 1, T, T + 1, 2 * T + 7])
def test_compaction_sizes_and_patterns(gpu, n):
    rng = np.random.default_rng(1610 + n)
    x = rng.standard_normal(n).astype(np.float32)
    y = rng.standard_normal(n).astype(np.float32)
    z = rng.uniform(-5, 300, n).astype(np.float32)
    ids = rng.integers(0, 45, n).astype(np.int32)
    for k, (name, keep) in enumerate(_patterns(n).items()):
        lab = np.where(keep, ids, -1).astype(np.int32)
        shift = (5 * k) % 16
        buf, kept, offs = _write_guarded(gpu, x, y, z, lab, True, shift)
        assert kept == int(keep.sum()), name
        assert offs[-1] == kept and len(offs) == -(-n // T) + 1, name
        assert (buf[:GUARD + shift] == 0xA5).all() and (buf[-GUARD:] == 0xA5).all(), name
        assert buf[GUARD + shift:len(buf) - GUARD].tobytes() == _expected(x, y, z, lab, keep), name
    # every point, labelled (noise grey) and coloured by intensity
    for lab in (np.where(_patterns(n)["alternating"], ids, -1).astype(np.int32), None):
        buf, kept, _ = _write_guarded(gpu, x, y, z, lab, False, 3)
        assert kept == n
        assert (buf[:GUARD + 3] == 0xA5).all() and (buf[-GUARD:] == 0xA5).all()
        assert buf[GUARD + 3:len(buf) - GUARD].tobytes() == \
            _expected(x, y, z, lab, np.ones(n, bool))


def test_inconsistent_offsets_are_skipped(gpu):
    n = 3 * T + 5
    rng = np.random.default_rng(1620)
    x, y, z = (rng.uniform(-5, 300, n).astype(np.float32) for _ in range(3))
    lab = rng.integers(0, 45, n).astype(np.int32)
    full = np.frombuffer(_expected(x, y, z, lab, np.ones(n, bool)), np.uint8)

    def check(buf, written_tiles):
        assert (buf[:GUARD] == 0xA5).all() and (buf[-GUARD:] == 0xA5).all()
        body = buf[GUARD:len(buf) - GUARD]
        for t in range(4):
            s = slice(15 * T * t, min(15 * T * (t + 1), 15 * n))
            want = full[s] if t in written_tiles else np.full(s.stop - s.start, 0xA5, np.uint8)
            np.testing.assert_array_equal(body[s], want, err_msg=f"tile {t}")

    def pushed(offs):      # tile 1's range pushed past out_bytes (its count still matches)
        o = offs.clone()
        o[1:3] += 10**6
        return o

    buf, kept, _ = _write_guarded(gpu, x, y, z, lab, True, offsets=pushed)
    assert kept == n
    check(buf, {3})        # tiles 0 and 2 no longer match their counts either

    def overflowing(offs):  # 15 * offset beyond int64
        o = offs.clone()
        o[2] = 2**62
        return o

    buf, _, _ = _write_guarded(gpu, x, y, z, lab, True, offsets=overflowing)
    check(buf, {0, 3})

    def miscounted(offs):  # tile 0 one short, tile 1 one over the tile size
        o = offs.clone()
        o[1] -= 1
        return o

    buf, _, _ = _write_guarded(gpu, x, y, z, lab, True, offsets=miscounted)
    check(buf, {2, 3})
    # an out that ends inside tile 2: the tiles that fit are written, nothing behind out_bytes
    buf, _, _ = _write_guarded(gpu, x, y, z, lab, True, out_bytes=15 * (2 * T + 100))
    check(buf, {0, 1})


def test_offsets_that_miscount_a_partly_kept_tile(gpu):
    """Tile 1 keeps every other point; its offsets claim one record too many (still no more than
    a tile holds) and tile 2's therefore one too few: both are skipped by the block's own count,
    tiles 0 and 3 are written where the true offsets put them."""
    n = 3 * T + 5
    rng = np.random.default_rng(1621)
    x, y, z = (rng.uniform(-5, 300, n).astype(np.float32) for _ in range(3))
    idx = np.arange(n)
    keep = (idx < T) | (idx >= 2 * T) | (idx % 2 == 0)
    lab = np.where(keep, rng.integers(0, 45, n), -1).astype(np.int32)
    full = np.frombuffer(_expected(x, y, z, lab, keep), np.uint8)

    def one_more(offs):
        o = offs.clone()
        o[2] += 1
        return o

    buf, kept, offs = _write_guarded(gpu, x, y, z, lab, True, 7, offsets=one_more)
    assert offs.tolist() == [0, T, T + T // 2, 2 * T + T // 2, kept] and kept == int(keep.sum())
    assert (buf[:GUARD + 7] == 0xA5).all() and (buf[-GUARD:] == 0xA5).all()
    body = buf[GUARD + 7:len(buf) - GUARD]
    for t in range(4):
        s = slice(15 * int(offs[t]), 15 * int(offs[t + 1]))
        want = full[s] if t in (0, 3) else np.full(s.stop - s.start, 0xA5, np.uint8)
        np.testing.assert_array_equal(body[s], want, err_msg=f"tile {t}")


def test_limits_and_errors(gpu):
    from rpt import _abi
    from rpt.denoise import ply_records_device, ply_records_size, write_ply

    lib = _abi.load()
    e = torch.zeros(0, dtype=torch.float32, device=gpu)
    assert ply_records_device(e, e, e).numel() == 0
    offs, kept, mx = ply_records_size(None, 0, False, gpu)
    assert (kept, mx) == (0, -1) and offs.cpu().tolist() == [0]
    with pytest.raises(ValueError):
        ply_records_size(None, 5, True, gpu)
    k = _abi.C.c_int64(0)
    assert lib.rpt_ply_records_size(offs.data_ptr(), 2**31, 0, offs.data_ptr(), _abi.C.byref(k),
                                    None, None) == _abi.RPT_ENOTSUP
    with pytest.raises(ValueError):
        write_ply("unused.ply", np.zeros(3, np.float32), np.zeros(3, np.float32),
                  np.zeros(3, np.float32), None, signal_only=True)


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("source", ["numpy", "device"])
def test_write_ply_through_the_device(gpu, g16, tmp_path, binary, source):
    from rpt.denoise import write_ply, write_ply_host

    conv = (lambda a: a) if source == "numpy" else (lambda a: torch.from_numpy(a).to(gpu))
    x, y, z, lab = (conv(g16[k]) for k in ("x", "y", "z", "labels"))
    form = "bin" if binary else "ascii"
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        for mode, l in (("labels", lab), ("plain", None)):
            info = {}
            write_ply(tmp_path / f"{form}_{mode}.ply", x, y, z, l, use_binary=binary, info=info)
            assert info == {"writer": "device"}
            assert (tmp_path / f"{form}_{mode}.ply").read_bytes() == \
                g16[f"{form}_{mode}"].tobytes(), mode
    assert buf.getvalue() == "".join(l + "\n" for l in str(g16["stdout"]).splitlines()
                                     if f" {form}_" in l)
    # signal_only against the host writer on the indexed arrays; no kept point: no file
    keep = g16["labels"] >= 0
    with contextlib.redirect_stdout(io.StringIO()):
        write_ply_host(tmp_path / "ref.ply", g16["x"][keep], g16["y"][keep], g16["z"][keep],
                       g16["labels"][keep], binary)
    info = {}
    with contextlib.redirect_stdout(io.StringIO()):
        write_ply(tmp_path / "sig.ply", x, y, z, lab, use_binary=binary, signal_only=True,
                  info=info)
    assert info["writer"] == "device"
    assert (tmp_path / "sig.ply").read_bytes() == (tmp_path / "ref.ply").read_bytes()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        write_ply(tmp_path / "none.ply", x, y, z, conv(np.full(len(keep), -1, np.int32)),
                  use_binary=binary, signal_only=True)
    assert buf.getvalue() == "Skipping empty point cloud: none.ply\n"
    assert not (tmp_path / "none.ply").exists()


def test_write_ply_other_dtypes(gpu, g16, tmp_path):
    """float64 coordinates and int64 labels qualify (astype(np.float32) on the device); float64
    intensities that colour the points do not (z / 255.0 is a float64 division): host writer."""
    from rpt.denoise import write_ply, write_ply_host

    fin = np.isfinite(g16["x"]) & np.isfinite(g16["y"])
    x, y = g16["x"][fin].astype(np.float64) + 1e-9, g16["y"][fin].astype(np.float64)
    z, lab = g16["z"][fin], g16["labels"][fin].astype(np.int64)
    with contextlib.redirect_stdout(io.StringIO()):
        info = {}
        write_ply(tmp_path / "a.ply", x, y, z, lab, info=info)
        write_ply_host(tmp_path / "a_ref.ply", x, y, z, lab)
        assert info == {"writer": "device"}
        write_ply(tmp_path / "b.ply", x, y, z.astype(np.float64), None, info=info)
        write_ply_host(tmp_path / "b_ref.ply", x, y, z.astype(np.float64), None)
        assert info == {"writer": "host", "reason": "dtypes"}
        write_ply(tmp_path / "c.ply", x, y, z, lab + 2**40, info=info)
        assert info == {"writer": "host", "reason": "labels outside int32"}
    for k in "ab":
        assert (tmp_path / f"{k}.ply").read_bytes() == (tmp_path / f"{k}_ref.ply").read_bytes()


def test_colors_alone(gpu):
    import matplotlib

    from rpt.denoise import ply_colors_device, ply_luts

    rng = np.random.default_rng(1630)
    lab = rng.integers(-3, 100, 5000).astype(np.int32)
    z = rng.uniform(-5, 300, 5000).astype(np.float32)
    want = np.full((5000, 3), 128, np.uint8)
    want[lab >= 0] = ply_luts()[0][lab[lab >= 0] % 20]
    got = ply_colors_device(None, torch.from_numpy(lab).to(gpu))
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    want = (matplotlib.colormaps["viridis"](np.clip(z / 255.0, 0, 1))[:, :3] * 255).astype(np.uint8)
    got = ply_colors_device(torch.from_numpy(z).to(gpu))
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_pipeline_writes_both_plys_on_the_device(tmp_path, golden):
    sys.path.insert(0, str(GOLDEN))
    from make_golden import synth_csv_stack

    from rpt.denoise import run_pipeline

    g = golden("g10_denoise_pipeline.npz")
    data = synth_csv_stack(tmp_path / "stack")
    out = tmp_path / "out"
    buf = io.StringIO()
    info = {}
    with contextlib.redirect_stdout(buf):
        run_pipeline(data, out, eps_space=8.0, eps_time=2.0, min_samples=15, min_frames=2,
                     max_frames=0, no_viz=True, parallel=False, info=info)
    assert info["ply_writers"] == {"denoised_point_cloud.ply": "device",
                                   "raw_point_cloud.ply": "device"}
    ref_out = str(g["stdout"])
    ref_dir = [l for l in ref_out.splitlines() if l.startswith("Results saved to: ")][0]
    ref_dir = ref_dir[len("Results saved to: "):]
    assert buf.getvalue().replace(str(out), "<OUT>") == ref_out.replace(ref_dir, "<OUT>")
    for name in ("denoised_point_cloud.ply", "raw_point_cloud.ply"):
        assert (out / name).read_bytes() == bytes(g[name.replace(".", "_")]), name
    for name in ("denoising_stats.csv", "clusters.csv"):
        assert (out / name).read_text() == str(g[name.replace(".", "_")]), name
