"""rpt_neighbour_counts / rpt_stdbscan_sweep without a GPU: the exports, the argument checks (all
made before the first device call, so no pointer given here is ever followed) and the Python
entry's refusal of inputs that st_dbscan routes to its float64 kernel."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from rpt import _abi

    return _abi.load()


@pytest.fixture(scope="module")
def buf():
    """A host array whose address stands in for every device pointer."""
    return np.zeros(64, np.float32)


def test_library_exports_both_symbols(lib):
    from rpt import _abi

    assert lib.rpt_missing_symbols == []
    for name in ("rpt_neighbour_counts", "rpt_stdbscan_sweep"):
        assert getattr(lib, name, None) is not None
        assert name in _abi.EXPORTED


def _counts(lib, p, n, counts):
    return lib.rpt_neighbour_counts(p, p, None, 1, p, n, 5.0, 1.0, counts, None)


def _sweep(lib, p, n, ms, n_sets, labels):
    arr = (C.c_int32 * max(len(ms), 1))(*ms)
    return lib.rpt_stdbscan_sweep(p, p, None, 1, p, n, 5.0, 1.0, arr, n_sets, None, labels, None,
                                  None)


def test_counts_argument_checks(lib, buf):
    from rpt import _abi

    p = buf.ctypes.data
    assert _counts(lib, p, -1, p) == _abi.RPT_EINVAL
    assert b"n < 0" in lib.rpt_last_error()
    assert _counts(lib, p, 16, None) == _abi.RPT_EINVAL
    assert b"counts" in lib.rpt_last_error()
    assert _counts(lib, None, 16, p) == _abi.RPT_EINVAL
    assert _counts(lib, p, 0, p) == _abi.RPT_EEMPTY  # (as rpt_stdbscan)


@pytest.mark.parametrize("n_sets", [0, 65, -1])
def test_sweep_set_count_limits(lib, buf, n_sets):
    from rpt import _abi

    p = buf.ctypes.data
    assert _sweep(lib, p, 16, [5] * 65, n_sets, p) == _abi.RPT_EINVAL
    assert b"n_sets" in lib.rpt_last_error()


def test_sweep_argument_checks(lib, buf):
    from rpt import _abi

    p = buf.ctypes.data
    assert _sweep(lib, p, -1, [5], 1, p) == _abi.RPT_EINVAL
    assert _sweep(lib, p, 16, [5], 1, None) == _abi.RPT_EINVAL
    assert b"labels" in lib.rpt_last_error()
    assert _sweep(lib, p, 16, [5, 0, 7], 3, p) == _abi.RPT_EINVAL
    assert b"min_samples[1]" in lib.rpt_last_error()
    assert _sweep(lib, p, 16, [5, -2], 2, p) == _abi.RPT_EINVAL
    assert lib.rpt_stdbscan_sweep(p, p, None, 1, p, 16, 5.0, 1.0, None, 1, None, p, None,
                                  None) == _abi.RPT_EINVAL
    assert _sweep(lib, p, 0, [5], 1, p) == _abi.RPT_EEMPTY  # (as rpt_stdbscan)


def test_float64_only_inputs_are_refused():
    """Coordinates offset by 2^30 + 0.1 do not round-trip through float32: st_dbscan takes its
    float64 kernel for them, the sweep and the counts say they do not."""
    from rpt.processors import neighbour_counts, st_dbscan_sweep

    rng = np.random.default_rng(3)
    c = rng.random((50, 2)) * 100.0 + (2.0 ** 30 + 0.1)
    t = np.arange(50, dtype=np.float32)
    with pytest.raises(NotImplementedError, match="st_dbscan"):
        st_dbscan_sweep(c, t, 5.0, 1.0, (3, 10))
    with pytest.raises(NotImplementedError, match="st_dbscan"):
        neighbour_counts(c, t, 5.0, 1.0)

