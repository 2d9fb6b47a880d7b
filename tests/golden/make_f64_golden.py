#!/usr/bin/env python3
"""Generate g15_stdbscan_f64.npz by RUNNING THE REFERENCE's st_dbscan on float64 inputs.

Refuses to run unless /root/reference exists (loaded as make_golden.py loads it).  The inputs are
the named cases of tests/_f64_cases.py; the fixture stores, per case, the reference's labels
(``<name>``) and in ``meta`` (JSON) the sha256 of the input bytes, the parameters and what the
generator found.  For EVERY case the generator asserts, and fails loudly otherwise, that

* the reference's labels equal the brute-force restatement tests/_f64_ref.py, and
* for a case marked discriminating, the restatement on float32-rounded coordinates differs in at
  least 100 labels.

No case is dropped silently: a case whose reference labels differ from the restatement (the
BallTree node residual of DESIGN.md §3) must be given another seed in tests/_f64_cases.py, and
``meta[name]["reseeded"]`` is there to say so.

    python tests/golden/make_f64_golden.py
"""
from __future__ import annotations

import importlib.util
import json
import platform
import sys
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.dont_write_bytecode = True
sys.path.insert(0, str(OUT.parent))

from _f64_cases import CASES, digest, round_coords_f32  # noqa: E402
from _f64_ref import st_dbscan_ref  # noqa: E402

# cases that needed another seed because the reference hit the BallTree residual (none so far)
RESEEDED: dict = {}


def _load(name: str, path: Path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    if not REF.exists():
        raise SystemExit("make_f64_golden.py must run where /root/reference exists")
    ref3 = _load("ref_stdbscan3", REF / "PointCloudWork" / "3_stdbscan_point_clouds.py")
    import sklearn

    arrays, meta = {}, {}
    for name, make in CASES.items():
        case = make()
        assert len(case.coords) <= 6000, name
        got = np.asarray(ref3.st_dbscan(case.coords, case.times, case.eps_space, case.eps_time,
                                        case.min_samples), np.int32)
        want = st_dbscan_ref(case.coords, case.times, case.eps_space, case.eps_time,
                             case.min_samples)
        diff = int((got != want).sum())
        assert diff == 0, (f"{name}: the reference differs from tests/_f64_ref.py in {diff} "
                           "labels; give the case another seed and record it in RESEEDED")
        n_diff32 = None
        if case.discriminating:
            c32 = round_coords_f32(case)
            l32 = st_dbscan_ref(c32.coords, c32.times, c32.eps_space, c32.eps_time,
                                c32.min_samples)
            n_diff32 = int((l32 != want).sum())
            assert n_diff32 >= 100, f"{name}: float32 rounding changes only {n_diff32} labels"
        arrays[name] = got
        meta[name] = dict(sha256=digest(case), n=int(len(got)), dim=int(case.coords.shape[1]),
                          coords_dtype=str(case.coords.dtype), times_dtype=str(case.times.dtype),
                          eps_space=repr(case.eps_space), eps_time=repr(case.eps_time),
                          min_samples=int(case.min_samples),
                          n_clusters=int(got.max() + 1), n_noise=int((got < 0).sum()),
                          discriminating=bool(case.discriminating), labels_changed_by_f32=n_diff32,
                          reseeded=RESEEDED.get(name))
        print(f"{name:28s} n={len(got):5d} clusters={got.max() + 1:5d} noise={(got < 0).sum():5d} "
              f"f32-diff={n_diff32}")
    info = dict(numpy=np.__version__, sklearn=sklearn.__version__, python=platform.python_version(),
                cases=meta)
    arrays["meta"] = np.frombuffer(json.dumps(info, sort_keys=True).encode(), np.uint8)
    path = OUT / "g15_stdbscan_f64.npz"
    np.savez_compressed(path, **arrays)
    print(f"{path.name}: {path.stat().st_size} bytes, {len(CASES)} cases")


if __name__ == "__main__":
    main()
