"""rpt_decimal_parse_host -- the per-token routine of the PLY row kernels (csrc/parse32.h) run on
the host -- against ``np.float32(float(token))``, compared as uint32 bit patterns, and the host
path of ``load_ply``."""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest


def _parse(tokens):
    """(values float32 [n], ok bool [n]) of byte-string tokens through exactly sized buffers."""
    from rpt import _abi

    lib = _abi.load()
    toks = [t if isinstance(t, bytes) else t.encode("utf-8") for t in tokens]
    lens = np.array([len(t) for t in toks], np.int32)
    offs = np.concatenate(([0], np.cumsum(lens[:-1], dtype=np.int64))).astype(np.int64)
    text = np.frombuffer(b"".join(toks) or b"\0", np.uint8).copy()
    n = len(toks)
    out = np.full(n, np.float32(-77.0), np.float32)
    ok = np.full(n, 9, np.uint8)
    _abi.check(lib.rpt_decimal_parse_host(text.ctypes.data, offs.ctypes.data, lens.ctypes.data, n,
                                          out.ctypes.data, ok.ctypes.data),
               "rpt_decimal_parse_host")
    assert set(np.unique(ok).tolist()) <= {0, 1}
    return out, ok.astype(bool)


def _reference(tokens) -> np.ndarray:
    return np.array([np.float32(float(t)) for t in tokens], np.float32)


def _assert_bits(tokens):
    got, ok = _parse(tokens)
    assert ok.all(), [tokens[i] for i in np.flatnonzero(~ok)[:10]]
    exp = _reference(tokens)
    bad = np.flatnonzero(got.view(np.uint32) != exp.view(np.uint32))
    assert bad.size == 0, [(tokens[i], float(got[i]), float(exp[i])) for i in bad[:10]]


def test_percent_6f_texts_of_random_float32():
    rng = np.random.default_rng(20261)
    mag = 10.0 ** rng.uniform(-7.0, np.log10(9e9), 20000)
    v = (mag * rng.choice([-1.0, 1.0], mag.size)).astype(np.float32)
    assert np.abs(v).min() < 1e-6 and 1e9 < np.abs(v).max() < 1e10 and (v < 0).any()
    tokens = ["%.6f" % float(x) for x in v]
    _assert_bits(tokens)


def test_named_tokens_inside_the_domain():
    tokens = ["0", "-0.000000", "0.000000", "007", ".5", "5.", "+1.5", "-.25", "255",
              "9007199254740992", "-9007199254740992", "0.1", "16777217", "0.000001",
              "0.0000000000000000000001", "00000000000000000000000012.5", "-0", "+0.", "+.0"]
    _assert_bits(tokens)
    got, _ = _parse(["-0.000000", "0.000000", "-0", "9007199254740992"])
    assert got.view(np.uint32).tolist() == [0x80000000, 0, 0x80000000, 0x5A000000]


def test_two_to_the_53_plus_one_is_outside():
    got, ok = _parse(["9007199254740992", "9007199254740993"])
    assert ok.tolist() == [True, False] and got[1] == 0.0


def _double_rounding_tokens(want: int, max_draws: int = 20000):
    """Tokens whose two-step value (string -> double -> float32) differs from the direct rounding
    to float32: the 15-significant-digit fixed-notation text of the exact midpoint between a
    float32 and its successor, kept when it reads back as that midpoint (a double) while the
    decimal itself is not the midpoint.  The double then ties to even; the decimal lies strictly
    on one side, and on the odd neighbour's side for about half of them."""
    rng = np.random.default_rng(53)
    found = []
    draws = 0
    while len(found) < want and draws < max_draws:
        draws += 1
        a = np.float32(10.0 ** rng.uniform(-3.0, 4.0))
        b = np.nextafter(a, np.float32(np.inf))
        mid = (float(a) + float(b)) / 2.0  # exact: 25 significant bits
        e = int(np.floor(np.log10(mid)))
        tok = "%.*f" % (max(14 - e, 0), mid)
        if float(tok) != mid or Fraction(tok) == Fraction(mid):
            continue
        # the direct rounding: the neighbour on the decimal's side of the midpoint
        direct = b if Fraction(tok) > Fraction(mid) else a
        two_step = np.float32(float(tok))
        if direct.view(np.uint32) != two_step.view(np.uint32):
            found.append((tok, two_step, direct))
    return found, draws


def test_double_rounding_tokens_give_the_two_step_value():
    found, draws = _double_rounding_tokens(16)
    assert len(found) >= 16, (len(found), draws)
    tokens = [t for t, _, _ in found] + ["5.73106837272644"]
    got, ok = _parse(tokens)
    assert ok.all()
    exp = np.array([s for _, s, _ in found] + [np.float32(5.7310686111450195)], np.float32)
    direct = np.array([d for _, _, d in found] + [np.float32(5.731068134307861)], np.float32)
    assert (exp.view(np.uint32) != direct.view(np.uint32)).all()
    assert got.view(np.uint32).tolist() == exp.view(np.uint32).tolist(), tokens


def test_domain_edges():
    inside = ["1234567890123456", "0.1234567890123456", "0.000" + "1234567890123456",
              "0." + "0" * 21 + "1", "1." + "0" * 15, "0" * 30 + "1", "0" * 20 + "." + "0" * 22,
              "9007199254.740992"]
    _assert_bits(inside)
    outside = ["1234567890123456789",      # 19 digits: above 2^53
               "18446744073709551621",     # 20 digits: 2^64 + 5, must not wrap round to 5
               "12345678901234567890", "0.12345678901234567890",
               "1." + "0" * 18,            # 19 digits with the trailing zeros: 10^18 > 2^53
               "1." + "0" * 19,            # 20 digits
               "0." + "0" * 22 + "1",      # f = 23
               "0." + "0" * 23,            # f = 23, m = 0
               "9007199254740993", "9007199254.740993",
               "1e5", "1E-3", "nan", "inf", "-inf", "1_0", "1..2", "--1", "+", ".", "", "-",
               "+.", "1-", "1+1", "1 ", " 1", "1\t", "0x10", "1,5", "１", "1é", "1\0"]
    got, ok = _parse(outside)
    assert not ok.any(), [outside[i] for i in np.flatnonzero(ok)]
    assert (got == 0.0).all()


def test_empty_and_bad_arguments():
    from rpt import _abi

    lib = _abi.load()
    assert lib.rpt_decimal_parse_host(None, None, None, 0, None, None) == _abi.RPT_OK
    assert lib.rpt_decimal_parse_host(None, None, None, 2, None, None) == _abi.RPT_EINVAL
    assert lib.rpt_decimal_parse_host(None, None, None, -1, None, None) == _abi.RPT_EINVAL
    assert lib.rpt_text_tile_bytes() > 0 and lib.rpt_text_tile_bytes() % 16 == 0


# ---- load_ply on the host ------------------------------------------------------------------------

def _write_ply(path, rows, n=None):
    head = ["ply", "format ascii 1.0", f"element vertex {len(rows) if n is None else n}",
            "property float x", "property float y", "property float z",
            "property uchar red", "property uchar green", "property uchar blue", "end_header"]
    path.write_text("\n".join(head + rows) + "\n")


def _rows(n, seed=0):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-5000, 5000, (n, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (n, 3))
    return xyz, rgb, ["%.6f %.6f %.6f %d %d %d" % (*map(float, p), *c) for p, c in zip(xyz, rgb)]


def test_load_ply_forced_host_path(tmp_path):
    from rpt.core.loaders import load_ply

    xyz, rgb, rows = _rows(300)
    p = tmp_path / "a.ply"
    _write_ply(p, rows)
    info = {}
    cloud = load_ply(p, device=False, info=info)
    assert info == {"parser": "host", "reason": "forced"}
    exp = np.array([[np.float32(float(t)) for t in r.split()[:3]] for r in rows], np.float32)
    for k, got in enumerate((cloud.x, cloud.y, cloud.z)):
        assert got.dtype == np.float32 and got.shape == (300,)
        np.testing.assert_array_equal(got.view(np.uint32), exp[:, k].view(np.uint32))
    assert cloud.colors.dtype == np.uint8
    np.testing.assert_array_equal(cloud.colors, rgb.astype(np.uint8))
    # positional use is the old signature
    np.testing.assert_array_equal(load_ply(p, False).x, cloud.x)


def test_load_ply_without_a_gpu_reads_on_the_host(tmp_path):
    import torch

    from rpt.core.loaders import load_ply

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: load_ply parses on the device")
    _, _, rows = _rows(50, seed=1)
    p = tmp_path / "b.ply"
    _write_ply(p, rows)
    info = {}
    cloud = load_ply(p, info=info)
    assert info == {"parser": "host", "reason": "no_gpu"}
    ref = load_ply(p, device=False)
    np.testing.assert_array_equal(cloud.x.view(np.uint32), ref.x.view(np.uint32))
    np.testing.assert_array_equal(cloud.colors, ref.colors)


def test_load_ply_host_exceptions_are_the_reference_ones(tmp_path):
    from rpt.core.loaders import load_ply

    _, _, rows = _rows(20, seed=2)
    p = tmp_path / "c.ply"
    _write_ply(p, rows, n=21)
    with pytest.raises(ValueError, match="iterator too short"):
        load_ply(p, device=False)
    rows[7] = rows[7].replace(" ", " x", 1)
    _write_ply(p, rows)
    with pytest.raises(ValueError, match="could not convert string to float"):
        load_ply(p, device=False)
    p.write_text("not a ply\n")
    with pytest.raises(ValueError, match="is not a PLY file"):
        load_ply(p, info={})


def test_ply_header_prefix_parser():
    from rpt.core.loaders import _ply_header

    head = b"ply\r\nformat ascii 1.0\r\nelement vertex 3\r\nproperty float x\r\n" \
           b"property float y\r\nproperty float z\r\nend_header\r\n"
    assert _ply_header(head + b"1 2 3\r\n") == (3, ["x", "y", "z"], len(head))
    assert _ply_header(head[:-2]) is None                       # no end of the header line
    assert _ply_header(head.replace(b"float x\r\n", b"float x\r")) is None    # a lone \r
    assert _ply_header(head.replace(b"float x", b"float \xc3\xa9")) is None   # not ASCII
    assert _ply_header(head.replace(b"vertex 3", b"vertex 3.0")) is None
    assert _ply_header(b"plx\n" + head) is None
    assert _ply_header(head.replace(b"element vertex 3\r\n", b"")) is None
