"""rpt_float32_repr -- the per-value routine of the RPT_TEXT_XYZ_REPR kernels (csrc/repr32.h) run
on the host -- against numpy's ``np.float32(v).astype(str)`` over about a million stratified bit
patterns: every string identical."""
from __future__ import annotations

import numpy as np
import pytest

from _repr_pool import BOUNDARY_EVEN, KNOWN, numpy_repr, pool


def _repr(values: np.ndarray):
    from rpt import _abi

    lib = _abi.load()
    v = np.ascontiguousarray(values, dtype=np.float32)
    n = len(v)
    out = np.full((max(n, 1), _abi.FLOAT32_REPR_SLOT), 0x55, np.uint8)
    lens = np.full(max(n, 1), -7, np.int32)
    _abi.check(lib.rpt_float32_repr(v.ctypes.data, n, out.ctypes.data, lens.ctypes.data),
               "rpt_float32_repr")
    return out[:n], lens[:n]


@pytest.fixture(scope="module")
def big():
    values = pool(1955)  # 255 exponents x 2 signs x (6 + 1955) mantissas: 1,000,110 + the named
    assert 1_000_000 <= len(values) <= 1_001_000
    out, lens = _repr(values)
    return values, out, lens


def test_yardstick_prints_the_known_values():
    bits = np.array(list(KNOWN), dtype=np.uint32)
    assert numpy_repr(bits.view(np.float32)).tolist() == list(KNOWN.values())


def test_every_string_equals_numpy(big):
    values, out, lens = big
    exp = numpy_repr(values)
    got = np.ascontiguousarray(out).view(f"S{out.shape[1]}")[:, 0].astype(str)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, [(hex(int(values[i:i + 1].view(np.uint32)[0])), got[i], exp[i])
                           for i in bad[:10]]
    np.testing.assert_array_equal(lens, np.char.str_len(exp))
    assert lens.max() == 19 and lens.min() == 3  # "-9999999000000000.0" ... "0.0"


def test_slots_are_nul_padded_and_nul_free_inside(big):
    _, out, lens = big
    col = np.arange(out.shape[1])[None, :]
    inside = col < lens[:, None]
    assert (out[inside] != 0).all() and (out[~inside] == 0).all()


def test_boundary_cases_are_end_points():
    """The pool's even-mantissa cases really are ones where only the closed interval gives the
    short string: the printed decimal is exactly half-way to a neighbour."""
    from fractions import Fraction

    for b in BOUNDARY_EVEN:
        v = np.array([b], np.uint32).view(np.float32)[0]
        mids = [(Fraction(float(v)) + Fraction(float(np.nextafter(v, np.float32(t))))) / 2
                for t in (0.0, np.inf)]
        assert b % 2 == 0 and Fraction(str(v)) in mids, hex(b)
    out, lens = _repr(np.array(BOUNDARY_EVEN, np.uint32).view(np.float32))
    assert bytes(out[0][:lens[0]]) == b"42298370.0"


def test_nan_and_inf_are_outside_the_domain():
    out, lens = _repr(np.array([np.nan, np.inf, -np.inf, 1.5, -np.nan], np.float32))
    assert lens.tolist() == [0, 0, 0, 3, 0]
    assert (out[[0, 1, 2, 4]] == 0).all() and bytes(out[3][:3]) == b"1.5"


def test_empty_and_bad_arguments():
    from rpt import _abi

    lib = _abi.load()
    assert lib.rpt_float32_repr(None, 0, None, None) == _abi.RPT_OK
    assert lib.rpt_float32_repr(None, 3, None, None) == _abi.RPT_EINVAL
    assert lib.rpt_float32_repr(None, -1, None, None) == _abi.RPT_EINVAL
