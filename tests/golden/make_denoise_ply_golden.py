#!/usr/bin/env python3
"""Generate g16_denoise_ply.npz by RUNNING THE REFERENCE's write_ply
(PointCloudWorkF/stdbscan_denoising_pipeline.py:767-855) in the build container over one cloud of
about 3 000 points that holds the edge values of its colour rules.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_denoise_ply_golden.py

Refuses to run unless /root/reference exists; importing this module does not need it: the tests
import ``cloud`` and ``viridis_edges`` and regenerate the very same inputs.

Stored: ``x``, ``y``, ``z`` (float32) and ``labels`` (int32), the inputs; the four files' bytes
``bin_labels`` / ``bin_plain`` (binary, with and without labels) and ``ascii_labels`` /
``ascii_plain``; ``stdout`` (the four "Wrote ..." lines); ``lut_tab20`` ([20][3]) and
``lut_viridis`` ([257][3], row 256 the colour of a NaN), by the writer's own expressions on the
generating host's matplotlib; ``info`` (numpy, matplotlib, JSON).

z: 0, -0.0, 255, 254.99998, 255.00002, negatives, values above 255, every k * 255 / 256 for
k = 0..256 with both float32 neighbours, +-inf, NaN, then random eighths in [-5, 300).
labels: -1, 0, 19, 20, 39, 2**31 - 1 and -7 in turn, then random ones in [-1, 60).
x, y: random quarter units in [-1000, 1000), with -0.0, a subnormal, an inf and a NaN that
carries a payload.
"""
from __future__ import annotations

import contextlib
import importlib.util
import io
import json
import platform
import sys
import tempfile
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
SCRIPT = REF / "PointCloudWorkF" / "stdbscan_denoising_pipeline.py"
OUT = Path(__file__).resolve().parent
sys.dont_write_bytecode = True

N = 3001   # no multiple of the kernel's tile, three tiles
F32 = np.float32


def viridis_edges() -> np.ndarray:
    """The intensities at which the colour row can change, float32."""
    k = (np.arange(257, dtype=np.float64) * 255.0 / 256.0).astype(F32)
    named = np.array([0.0, -0.0, 255.0, 254.99998, 255.00002, -1.0, -0.5, -1e-30, -300.0, 256.0,
                      300.0, 1e10, np.inf, -np.inf, np.nan], F32)
    return np.concatenate([named, k, np.nextafter(k, F32(-1e9)), np.nextafter(k, F32(1e9))])


def cloud():
    """(x, y, z float32 [N], labels int32 [N]) from a fixed seed."""
    rng = np.random.default_rng(1601)
    edges = viridis_edges()
    # (coordinates on a quarter-unit grid and intensities in eighths: the fixture compresses)
    z = np.concatenate([edges, rng.integers(-40, 2400, N - len(edges)) / 8.0]).astype(F32)
    x = (rng.integers(-4000, 4000, N) / 4.0).astype(F32)
    y = (rng.integers(-4000, 4000, N) / 4.0).astype(F32)
    x[:4] = np.array([-0.0, 1e-40, np.inf, 0.0], F32)
    x[4:5].view(np.uint32)[:] = 0x7FC12345       # a NaN with a payload
    y[5:6].view(np.uint32)[:] = 0xFFC00001
    named = np.array([-1, 0, 19, 20, 39, 2**31 - 1, -7], np.int64)
    labels = rng.integers(-1, 60, N)
    labels[:70] = np.tile(named, 10)
    labels[1024 - 7:1024] = named                # across the first tile edge
    return x, y, z, labels.astype(np.int32)


def luts():
    """The writer's own LUT expressions (:786-795) on the installed matplotlib."""
    import matplotlib

    tab = matplotlib.colormaps["tab20"]
    vir = matplotlib.colormaps["viridis"]
    lut20 = (np.array([tab(i)[:3] for i in range(20)]) * 255).astype(np.uint8)
    lutv = (vir(np.arange(256))[:, :3] * 255).astype(np.uint8)
    bad = (vir(np.array([np.nan], F32))[:, :3] * 255).astype(np.uint8)
    return lut20, np.concatenate([lutv, bad])


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_denoise_ply", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_denoise_ply"] = mod
    spec.loader.exec_module(mod)
    return mod


def main() -> None:
    if not REF.exists():
        raise SystemExit("make_denoise_ply_golden.py must run where /root/reference exists "
                         "(build container)")
    import matplotlib

    ref = load_reference()
    x, y, z, labels = cloud()
    out = dict(x=x, y=y, z=z, labels=labels)
    buf = io.StringIO()
    with tempfile.TemporaryDirectory() as td, contextlib.redirect_stdout(buf):
        for key, lab, binary in (("bin_labels", labels, True), ("bin_plain", None, True),
                                 ("ascii_labels", labels, False), ("ascii_plain", None, False)):
            p = Path(td) / f"{key}.ply"
            ref.write_ply(p, x, y, z, lab, use_binary=binary)
            out[key] = np.frombuffer(p.read_bytes(), np.uint8)
    out["stdout"] = buf.getvalue()
    out["lut_tab20"], out["lut_viridis"] = luts()
    out["info"] = json.dumps({"numpy": np.__version__, "matplotlib": matplotlib.__version__,
                              "python": platform.python_version(),
                              "generated_by": "tests/golden/make_denoise_ply_golden.py"})

    # what the cases are there for
    body = out["bin_plain"].tobytes().split(b"end_header\n", 1)[1]
    assert len(body) == 15 * N
    rec = np.frombuffer(body, np.dtype([("x", "<u4"), ("y", "<u4"), ("z", "<f4"),
                                        ("c", "u1", (3,))]))
    assert rec["x"][4] == 0x7FC12345 and rec["y"][5] == 0xFFC00001   # payloads kept
    nan = np.isnan(rec["z"])
    assert nan.sum() == 1 and (rec["c"][nan] == out["lut_viridis"][256]).all()
    assert (rec["c"][z == np.inf] == out["lut_viridis"][255]).all()
    assert (rec["c"][z == -np.inf] == out["lut_viridis"][0]).all()
    lab_rec = np.frombuffer(out["bin_labels"].tobytes().split(b"end_header\n", 1)[1], rec.dtype)
    assert (lab_rec["c"][labels < 0] == 128).all()
    assert (lab_rec["c"][labels == 2**31 - 1] == out["lut_tab20"][(2**31 - 1) % 20]).all()

    np.savez_compressed(OUT / "g16_denoise_ply.npz", **{k: np.asarray(v) for k, v in out.items()})
    size = (OUT / "g16_denoise_ply.npz").stat().st_size
    print(f"g16_denoise_ply.npz: {len(out)} entries, {size} bytes")
    print(out["stdout"], end="")
    assert size < 200_000


if __name__ == "__main__":
    main()
